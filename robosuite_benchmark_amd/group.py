"""SACTrainerGroup / TD3TrainerGroup: several SAC or TD3 runs of one configuration trained together (sac_group_*,
td3_group_create of include/sac_hip.h); MixedSACTrainerGroup / MixedTD3TrainerGroup: runs of different tasks
(sac_group_create_mixed, td3_group_create_mixed); MlpSACTrainerGroup / MlpTD3TrainerGroup: runs of the general step --
hidden sizes other than two layers of at most 256 units (sac_group_create_mlp, td3_group_create_mlp);
ArchSACTrainerGroup / ArchTD3TrainerGroup: runs of any hidden sizes, a network-size sweep (sac_group_create_arch,
td3_group_create_arch, and mixed groups for the fused shapes).

The reference's real workload is many independent runs -- seeds x configurations, one job each
(/root/reference/launch_jobs.sh).  One run at batch 256 cannot fill an MI355X; a group steps R runs of the same shape
with grouped launches (each launch R times wider) while every member stays an ordinary SACTrainer (TD3Trainer): its own
weights, optimizer state, hyperparameters, noise seed and replay buffer, and a result bit for bit that of training alone."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

from . import _lib
from .sac import SACTrainer, _check_stats, _eval_columns, _merge_all, _stats_moments, moments_statistics
from .td3 import TD3Trainer

MAX_MEMBERS = 16


def _general_shape(hs):
    return len(hs) != 2 or max(hs) > 256


def runs_general_step(t):
    """Does trainer t run the general step (hidden sizes other than two layers of at most 256 units)?  Such runs group in
    MlpSACTrainerGroup / MlpTD3TrainerGroup, the others in the remaining kinds."""
    return _general_shape(t._hidden("policy")) or _general_shape(t._hidden("qf1"))


GENERAL = ("host", "device")
GENERAL_SESSIONS = True         # GroupActor(general="device")'s default for general_sessions: switched on by the
                                # measurement of DESIGN.md, section 6d (the actions are the same bits either way)


def _check_general(general):
    if general not in GENERAL:
        raise RuntimeError(f"general must be one of {GENERAL}, got {general!r}")
    return general


def _act_general_many(lib, trainers, ids, n_rows, obs, det, eps, out):
    """ONE sac_policy_act_general_many call per 16 of the general-step members `ids`: obs / eps / out hold a float32 array
    (or None) per trainer, n_rows and det one value per trainer."""
    for c in range(0, len(ids), MAX_MEMBERS):
        part = ids[c:c + MAX_MEMBERS]
        n = len(part)
        vp = lambda arrs: (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in arrs])  # noqa: E731
        _lib.check(lib.sac_policy_act_general_many((C.c_void_p * n)(*[trainers[i]._h.value for i in part]), n,
                                                   (C.c_int32 * n)(*[n_rows[i] for i in part]), vp([obs[i] for i in part]),
                                                   (C.c_int32 * n)(*[int(bool(det[i])) for i in part]),
                                                   vp([eps[i] for i in part]), vp([out[i] for i in part])),
                   "sac_policy_act_general_many")


def act_many(trainers, obs_list, deterministic_list, eps_list, general="host"):
    """policy.get_actions for many runs at once: actions[i] = trainers[i]'s policy on obs_list[i] ((n_i, O_i); None or no
    rows: the member sits out and gets an empty array), deterministic_list[i] as MakeDeterministic, eps_list[i] the
    (n_i, A_i) N(0,1) draws of a stochastic SAC member (None otherwise).  The members with the fused kernels' shapes act
    in ONE launch per 16 of them (sac_policy_act_many: SAC and TD3, dims and row counts mixed; up to 1024 rows each);
    members of the general step act on the host through their own policy_act.  A member's actions never depend on its
    neighbours: they are bit for bit those of its own policy_act_device (policy_act for the general step).
    general="device": the members of the general step act on the device as well, in ONE sac_policy_act_general_many call
    per 16 of them; their actions are bit for bit those of their own policy_act_general."""
    _check_general(general)
    trainers = list(trainers)
    R = len(trainers)
    if not (len(obs_list) == len(deterministic_list) == len(eps_list) == R):
        raise RuntimeError("act_many takes one observation array, deterministic flag and eps per trainer")
    if len({id(t) for t in trainers}) != R:
        raise RuntimeError("a trainer appears twice in act_many")
    obs = [None if o is None else _lib.f32(np.atleast_2d(o)) for o in obs_list]
    eps = [None if e is None else _lib.f32(np.atleast_2d(e)) for e in eps_list]
    out = [np.empty((0 if o is None else o.shape[0], t.act_dim), np.float32) for t, o in zip(trainers, obs)]
    dev, gen = [], []
    for i, t in enumerate(trainers):
        if out[i].shape[0] == 0:
            continue
        if obs[i].shape[1] != t.obs_dim or (eps[i] is not None and eps[i].shape != out[i].shape):
            raise RuntimeError(f"act_many member {i}: observations {obs[i].shape} / eps "
                               f"{None if eps[i] is None else eps[i].shape} do not fit dims ({t.obs_dim}, {t.act_dim})")
        if out[i].shape[0] > _lib.ACT_MAX_ROWS:
            raise RuntimeError(f"act_many member {i}: {out[i].shape[0]} rows (at most {_lib.ACT_MAX_ROWS} per call)")
        if not runs_general_step(t):
            dev.append(i)
        elif general == "device":
            gen.append(i)
        else:
            out[i] = t.policy_act(obs[i], deterministic_list[i], eps[i])
    lib = _lib.load()
    _act_general_many(lib, trainers, gen, [o.shape[0] for o in out], obs, deterministic_list, eps, out)
    for c in range(0, len(dev), MAX_MEMBERS):
        ids = dev[c:c + MAX_MEMBERS]
        n = len(ids)
        vp = lambda arrs: (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in arrs])  # noqa: E731
        _lib.check(lib.sac_policy_act_many((C.c_void_p * n)(*[trainers[i]._h.value for i in ids]), n,
                                           (C.c_int32 * n)(*[out[i].shape[0] for i in ids]), vp([obs[i] for i in ids]),
                                           (C.c_int32 * n)(*[int(bool(deterministic_list[i])) for i in ids]),
                                           vp([eps[i] for i in ids]), vp([out[i] for i in ids])), "sac_policy_act_many")
    return out


def q_values_many(trainers, obs_list, act_list, nets_list, general="host"):
    """SACTrainer.q_values for many runs at once: q[i] = trainers[i]'s critics nets_list[i] (names, as q_values takes
    them) on obs_list[i] / act_list[i] ((n_i, O_i) / (n_i, A_i); None or no rows: the member sits out and gets an empty
    (len(nets), 0) array).  The members with the fused kernels' shapes are served by ONE launch per 16 of them and 1024
    rows (sac_q_values_many: SAC and TD3, dims, row counts and nets mixed); members of the general step take q_values'
    host path inside the same call.  A member's values never depend on its neighbours: they are bit for bit those of its
    own q_values.
    general="device": the members of the general step are evaluated on the device as well, by ONE
    sac_q_values_general_many call per 16 of them and 1024 rows; their values are bit for bit those of their own
    q_values(general="device")."""
    _check_general(general)
    trainers = list(trainers)
    R = len(trainers)
    if not (len(obs_list) == len(act_list) == len(nets_list) == R):
        raise RuntimeError("q_values_many takes one observation array, action array and net selection per trainer")
    if len({id(t) for t in trainers}) != R:
        raise RuntimeError("a trainer appears twice in q_values_many")
    obs, act, rows, names, masks, out = [None] * R, [None] * R, [None] * R, [None] * R, [0] * R, [None] * R
    dev, gen = [], []
    for i, t in enumerate(trainers):
        names[i] = [nets_list[i]] if isinstance(nets_list[i], str) else list(nets_list[i])
        masks[i], rows[i] = _lib.q_net_mask(names[i])
        if obs_list[i] is None or np.atleast_2d(obs_list[i]).shape[0] == 0:
            out[i] = np.empty((len(names[i]), 0), np.float32)
            continue
        obs[i], act[i], _, _ = t._q_inputs(obs_list[i], act_list[i], names[i])
        general_step = t._h is not None and runs_general_step(t)
        if t._h is None or (general_step and general != "device"):
            out[i] = t._q_values_host(obs[i], act[i], names[i])
        else:
            out[i] = np.empty((len(names[i]), obs[i].shape[0]), np.float32)
            (gen if general_step else dev).append(i)
    lib = _lib.load() if dev or gen else None
    for members, entry in ((dev, "sac_q_values_many"), (gen, "sac_q_values_general_many")):
        for r0 in range(0, max([obs[i].shape[0] for i in members], default=0), _lib.ACT_MAX_ROWS):
            live = [i for i in members if obs[i].shape[0] > r0]
            for c in range(0, len(live), MAX_MEMBERS):
                ids = live[c:c + MAX_MEMBERS]
                n = len(ids)
                n_rows = [min(obs[i].shape[0] - r0, _lib.ACT_MAX_ROWS) for i in ids]
                o = [obs[i][r0:r0 + k] for i, k in zip(ids, n_rows)]
                a = [act[i][r0:r0 + k] for i, k in zip(ids, n_rows)]
                q = [np.empty((len(names[i]), k), np.float32) for i, k in zip(ids, n_rows)]
                vp = lambda arrs: (C.c_void_p * n)(*[x.ctypes.data for x in arrs])  # noqa: E731
                _lib.check(getattr(lib, entry)((C.c_void_p * n)(*[trainers[i]._h.value for i in ids]), n,
                                               (C.c_int32 * n)(*n_rows), vp(o), vp(a),
                                               (C.c_uint32 * n)(*[masks[i] for i in ids]), vp(q)), entry)
                for i, k, part in zip(ids, n_rows, q):
                    out[i][:, r0:r0 + k] = part[rows[i]]
    return out


def evaluate_many(trainers, batches, eps=None, rngs=None, rows=False, general="host", stats="host"):
    """SACTrainer.evaluate for many runs at once: result[i] = trainers[i].evaluate(batches[i], eps[i], rngs[i]) (eps / rngs:
    one entry per trainer or None; batches[i] None or without rows: the member sits out and gets None).  The SAC members
    with the fused kernels' shapes are served by ONE launch per 16 of them and 1024 rows (sac_evaluate_many: dims, hidden
    sizes and row counts mixed); the others -- the general step, trainers without a handle -- go through their own
    evaluate inside the same call (a TD3 member raises there).  A member's columns never depend on its neighbours: they
    are bit for bit those of its own evaluate.  Results come back in member order; rows=True as for evaluate.
    general="device": the SAC members of the general step are evaluated on the device as well, by ONE
    sac_evaluate_general_many call per 16 of them and 1024 rows; their results are bit for bit those of their own
    evaluate(general="device").
    stats="device" (evaluate's `stats`): the members served by those two entries get their statistics reduced on the device
    in the same call (sac_evaluate_stats_many / sac_evaluate_general_stats_many: one k_eval_moments launch in front of the
    call's wait) -- no eval_statistics and no sac_get_scalars for them, and with rows=False no column is copied back.  A
    member's records are byte for byte those of its own evaluate(stats="device").  The members on the host path get
    eval_statistics under either value."""
    _check_stats(stats)
    _check_general(general)
    on_device = stats == "device"
    trainers = list(trainers)
    R = len(trainers)
    eps = [None] * R if eps is None else list(eps)
    rngs = [None] * R if rngs is None else list(rngs)
    if not (len(batches) == len(eps) == len(rngs) == R):
        raise RuntimeError("evaluate_many takes one batch (and eps pair, and rng) per trainer")
    if len({id(t) for t in trainers}) != R:
        raise RuntimeError("a trainer appears twice in evaluate_many")
    out, arrs, chunks, alphas, dev, gen = [None] * R, [None] * R, [None] * R, [1.0] * R, [], []
    moments, log_alphas = [None] * R, [0.0] * R
    for i, t in enumerate(trainers):
        b = batches[i]
        if b is None or np.atleast_2d(b["observations"]).shape[0] == 0:
            continue
        general_step = runs_general_step(t)
        if isinstance(t, TD3Trainer) or t._h is None or (general_step and general != "device") or t._evaluate_on_host:
            out[i] = t.evaluate(b, eps=eps[i], rng=rngs[i], rows=rows)
            continue
        arrs[i], chunks[i] = t._eval_inputs(b, eps[i], rngs[i]), []
        (gen if general_step else dev).append(i)
    lib = _lib.load() if dev or gen else None
    for members, entry in ((dev, "sac_evaluate_stats_many" if on_device else "sac_evaluate_many"),
                           (gen, "sac_evaluate_general_stats_many" if on_device else "sac_evaluate_general_many")):
        for r0 in range(0, max([arrs[i][0].shape[0] for i in members], default=0), _lib.ACT_MAX_ROWS):
            live = [i for i in members if arrs[i][0].shape[0] > r0]
            for c in range(0, len(live), MAX_MEMBERS):
                ids = live[c:c + MAX_MEMBERS]
                n = len(ids)
                n_rows = [min(arrs[i][0].shape[0] - r0, _lib.ACT_MAX_ROWS) for i in ids]
                made = [trainers[i]._eval_io(arrs[i], r0, r0 + k, outputs=rows or not on_device) for i, k in zip(ids, n_rows)]
                ios = (_lib.SacEvalIO * n)(*[m[0] for m in made])
                sts = (_lib.SacEvalStats * n)() if on_device else None
                _lib.check(getattr(lib, entry)((C.c_void_p * n)(*[trainers[i]._h.value for i in ids]), n,
                                               (C.c_int32 * n)(*n_rows), ios, *([sts] if on_device else [])), entry)
                for k, i in enumerate(ids):
                    chunks[i].append(made[k][1])
                    alphas[i] = float(ios[k].alpha)
                    if on_device:
                        moments[i], log_alphas[i] = _merge_all(moments[i], _stats_moments(sts[k])), sts[k].log_alpha
    for i in dev + gen:
        t = trainers[i]
        cols = _eval_columns(chunks[i], alphas[i]) if rows or not on_device else None
        if on_device:
            result = moments_statistics(moments[i], alphas[i], log_alphas[i], t.target_entropy, t.use_automatic_entropy_tuning)
        else:
            result = t._eval_stats(cols)
        out[i] = (result, cols) if rows else result
    return out


class _ActorSession:
    """One acting session (at most 16 members): its handle, the members' handles it was opened on, and the per-call
    argument arrays, made once.  entry: "sac_actor" (the fused kernels' shapes) or "sac_gactor" (the general step) --
    the two families of include/sac_hip.h have the same four signatures."""

    def __init__(self, lib, ids, trainers, max_rows, entry="sac_actor"):
        n = len(ids)
        self.lib, self.ids, self.a, self.entry = lib, ids, C.c_void_p(), entry
        self.handles = [trainers[i]._h.value for i in ids]
        self.gens = [trainers[i]._handle_gen for i in ids]      # (an address can come back; the count cannot)
        self.n_rows, self.det = (C.c_int32 * n)(), (C.c_int32 * n)()
        self._act = getattr(lib, entry + "_act")
        _lib.check(getattr(lib, entry + "_create")(C.byref(self.a), (C.c_void_p * n)(*self.handles), n,
                                                   (C.c_int32 * n)(*[max_rows[i] for i in ids])), entry + "_create")

    def arrays(self, k, rows, O, A):
        o, e, a = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(getattr(self.lib, self.entry + "_arrays")(self.a, k, C.byref(o), C.byref(e), C.byref(a)),
                   self.entry + "_arrays")
        view = lambda p, ct, cols: np.ctypeslib.as_array((ct * (rows * cols)).from_address(p.value)).reshape(rows, cols)  # noqa: E731
        return view(o, C.c_double, O), view(e, C.c_float, A), view(a, C.c_float, A)

    def act(self):
        """One tick on n_rows / det as they stand."""
        _lib.check(self._act(self.a, self.n_rows, self.det), self.entry + "_act")

    def destroy(self):
        a, self.a = self.a, None
        if a:
            getattr(self.lib, self.entry + "_destroy")(a)


class _ActRows(list):
    """GroupActor.act: the members' action views, act[i] -- and the tick itself, act(n_rows, deterministic)."""

    def __init__(self, tick, rows):
        super().__init__(rows)
        self._tick = tick

    def __call__(self, n_rows, deterministic):
        return self._tick(n_rows, deterministic)

    def __reduce__(self):
        raise TypeError("the action views of a GroupActor are never pickled")


class GroupActor:
    """policy.get_actions for a FIXED list of runs, tick after tick, without marshalling: act_many as a session.

    obs[i] (max_rows_i, O_i) float64, eps[i] (max_rows_i, A_i) float32 and act[i] (max_rows_i, A_i) float32 are NumPy
    views of the staging the kernel reads and writes (sac_actor_arrays: a mapped pinned slab; nothing is copied).  A tick
    is: write rows [0, n_i) of obs[i] (and of eps[i], for a stochastic SAC member), call act(n_rows, deterministic), read
    rows [0, n_i) of act[i] -- and copy them before the next tick overwrites them.  n_i == 0: member i sits out and its
    arrays are left alone.  Observations are rounded to float32 as astype(np.float32) rounds them; each member's actions
    are bit for bit those of its own policy_act_device on obs.astype(np.float32) with the same eps.

    Like act_many it opens one session per 16 members with the fused kernels' shapes; members of the general step act on
    the host through their own policy_act inside the same act() call, with ordinary arrays behind the same attributes.
    A session is bound to its members' handles: when a trainer has replaced its handle (a first step at another batch
    size; seen by the trainer's count of handles made, since an address can come back), act() reopens the sessions,
    carries the staged rows over and REPLACES the views, so read obs[i] / eps[i] / act[i] from the attributes on each
    tick.  close() (and the finaliser) destroys the sessions.  The object holds device state only and is never pickled.

    general="device": the members of the general step act on the device too -- all of them that have rows in ONE
    sac_policy_act_general_many call per 16, on obs.astype(np.float32), the value the sessions' conversion produces --
    and their actions are bit for bit those of their own policy_act_general on those rows.

    general="device", general_sessions=True: the members of the general step get acting sessions of their own
    (sac_gactor_*, csrc/sac_actor_general.h), one per 16 of them: obs[i] (float64), eps[i] and act[i] are views into that
    session's slab like the other members', their tick is one C call, and reopening, close() and the pickling refusal
    cover them too.  This is the default (None: GENERAL_SESSIONS).  The actions are the same bits as with
    general_sessions=False, which keeps the sac_policy_act_general_many path described above, to measure against.  With
    general="host" the keyword changes nothing."""

    def __init__(self, trainers, max_rows=1, general="host", general_sessions=None):
        self.general = _check_general(general)
        self.general_sessions = general == "device" and bool(GENERAL_SESSIONS if general_sessions is None else general_sessions)
        self.trainers = list(trainers)
        R = len(self.trainers)
        if R == 0 or len({id(t) for t in self.trainers}) != R:
            raise RuntimeError("GroupActor takes one or more trainers, each once")
        self.max_rows = [int(max_rows)] * R if np.isscalar(max_rows) else [int(m) for m in max_rows]
        if len(self.max_rows) != R or not all(1 <= m <= _lib.ACT_MAX_ROWS for m in self.max_rows):
            raise RuntimeError(f"GroupActor: max_rows is 1..{_lib.ACT_MAX_ROWS}, one value or one per trainer")
        for i, t in enumerate(self.trainers):
            if getattr(t, "_h", None) is None:
                raise RuntimeError(f"GroupActor member {i} has no device handle yet (create it with batch_size=, or train once)")
        self._lib = _lib.load()
        self._td3 = [isinstance(t, TD3Trainer) for t in self.trainers]
        self._host = [i for i, t in enumerate(self.trainers) if runs_general_step(t)]
        self._dev = [i for i in range(R) if i not in set(self._host)]
        self._gen = self._host if self.general_sessions else []      # the general-step members with sessions
        self.obs, self.eps, self.act = [None] * R, [None] * R, _ActRows(self._act, [None] * R)
        for i in self._host if not self.general_sessions else ():
            t, m = self.trainers[i], self.max_rows[i]
            self.obs[i], self.eps[i] = np.zeros((m, t.obs_dim), np.float64), np.zeros((m, t.act_dim), np.float32)
            self.act[i] = np.zeros((m, t.act_dim), np.float32)
        self._sessions, self._closed = [], False
        self._open()

    def _open(self):
        for ids, entry in ((self._dev, "sac_actor"), (self._gen, "sac_gactor")):
            for c in range(0, len(ids), MAX_MEMBERS):
                s = _ActorSession(self._lib, ids[c:c + MAX_MEMBERS], self.trainers, self.max_rows, entry)
                self._sessions.append(s)
                for k, i in enumerate(s.ids):
                    t = self.trainers[i]
                    self.obs[i], self.eps[i], self.act[i] = s.arrays(k, self.max_rows[i], t.obs_dim, t.act_dim)

    def _reopen(self):
        """A member's handle was replaced: new sessions on the handles of now, the staged rows carried over."""
        members = self._dev + self._gen
        for i in members:
            if self.trainers[i]._h is None:
                raise RuntimeError(f"GroupActor member {i} has lost its device handle")
        kept = {i: (self.obs[i].copy(), self.eps[i].copy(), self.act[i].copy()) for i in members}
        self._destroy()
        self._open()
        for i, (o, e, a) in kept.items():
            self.obs[i][...], self.eps[i][...], self.act[i][...] = o, e, a

    def _act(self, n_rows, deterministic):
        """act(n_rows, deterministic), one tick: actions of rows [0, n_rows[i]) of every member into act[i].
        deterministic: one flag or one per member (MakeDeterministic; TD3 members are deterministic whatever it says)."""
        if self._closed:
            raise RuntimeError("this GroupActor is closed")
        R = len(self.trainers)
        det = [bool(deterministic)] * R if np.isscalar(deterministic) else [bool(d) for d in deterministic]
        n_rows = [int(n) for n in n_rows]
        if len(n_rows) != R or len(det) != R:
            raise RuntimeError("GroupActor.act takes one row count (and one deterministic flag, or one for all) per trainer")
        for i, n in enumerate(n_rows):                        # every refusal first: nothing has acted when one raises
            if not 0 <= n <= self.max_rows[i]:
                raise RuntimeError(f"GroupActor member {i}: {n} rows (0..{self.max_rows[i]} in this session, 0 = sits out)")
        if not any(n_rows):
            raise RuntimeError("no trainer has rows to act on")
        if any(self.trainers[i]._h is None or self.trainers[i]._handle_gen != g
               for s in self._sessions for i, g in zip(s.ids, s.gens)):
            self._reopen()
        for s in self._sessions:
            rows = [n_rows[i] for i in s.ids]
            if not any(rows):
                continue
            s.n_rows[:], s.det[:] = rows, [det[i] for i in s.ids]
            s.act()
        if self.general_sessions:
            return
        if self.general == "device":
            ids = [i for i in self._host if n_rows[i]]
            obs, eps, out = [None] * R, [None] * R, [None] * R
            for i in ids:
                obs[i] = np.ascontiguousarray(self.obs[i][:n_rows[i]].astype(np.float32))
                eps[i] = None if det[i] or self._td3[i] else self.eps[i][:n_rows[i]]
                out[i] = self.act[i][:n_rows[i]]
            _act_general_many(self._lib, self.trainers, ids, n_rows, obs, det, eps, out)
            return
        for i in self._host:
            n = n_rows[i]
            if n:
                stochastic = not det[i] and not self._td3[i]
                self.act[i][:n] = self.trainers[i].policy_act(self.obs[i][:n], det[i], self.eps[i][:n] if stochastic else None)

    def _destroy(self):
        sessions, self._sessions = getattr(self, "_sessions", []), []
        for s in sessions:
            s.destroy()

    def close(self):
        """Destroy the sessions: the views must not be used afterwards, and act() raises."""
        self._closed = True
        self.obs, self.eps = [], []
        del self.act[:]
        self._destroy()

    def __del__(self):
        self._destroy()

    def __reduce__(self):
        raise TypeError("a GroupActor holds device staging and is never pickled: build a new one on the restored trainers")


class _Members:
    """The member checks that hold for every kind of trainer group (host metadata: nothing is created for a group that
    cannot exist).  The algorithm comes from _SACMembers / _TD3Members."""
    _ONLY = None                # why a member of another kind is refused

    @staticmethod
    def _member_ok(t):
        raise NotImplementedError

    def _check_member(self, i, t, t0):
        """Refuse member i (i >= 1) against member 0 from host metadata."""
        raise NotImplementedError

    def _check_step(self, i, t):
        """Refuse member i for the step its hidden sizes select (the fused kernels' groups check it at train_loop)."""

    def _checked_members(self, trainers):
        trainers = list(trainers)
        if not 1 <= len(trainers) <= MAX_MEMBERS:
            raise RuntimeError(f"a trainer group holds 1..{MAX_MEMBERS} trainers (got {len(trainers)})")
        for i, t in enumerate(trainers):
            if not self._member_ok(t):
                raise RuntimeError(f"trainer group member {i} is a {type(t).__name__}: {self._ONLY}")
            self._check_step(i, t)
        if len({id(t) for t in trainers}) != len(trainers):
            raise RuntimeError("a trainer appears twice in the group")
        for i, t in enumerate(trainers[1:], 1):
            self._check_member(i, t, trainers[0])
        return trainers

    @staticmethod
    def _check_device(i, t, t0):
        if t.device != t0.device:
            raise RuntimeError(f"trainer group member {i} lives on device {t.device}, member 0 on {t0.device}")

    def q_many(self, obs_list, act_list, nets_list=None, general="host"):
        """q_values_many over the group's members (nets_list None: qf1 and qf2 of every member; general as there)."""
        _check_general(general)
        if nets_list is None:
            nets_list = [("qf1", "qf2")] * len(self.trainers)
        return q_values_many(self.trainers, obs_list, act_list, nets_list, general=general)

    def evaluate_many(self, batches, eps=None, rngs=None, rows=False, general="host", stats="host"):
        """evaluate_many over the group's members (general and stats as there)."""
        return evaluate_many(self.trainers, batches, eps=eps, rngs=rngs, rows=rows, general=general, stats=stats)


class _SACMembers:
    _ONLY = "groups hold SAC trainers only"

    @staticmethod
    def _member_ok(t):
        return isinstance(t, SACTrainer) and not isinstance(t, TD3Trainer)


class _TD3Members:
    _ONLY = "TD3 groups hold TD3 trainers only"

    @staticmethod
    def _member_ok(t):
        return isinstance(t, TD3Trainer)


class _GroupBase(_Members):
    """What every kind of trainer group with a C group shares: the C group over the members' handles and the call of
    sac_group_train_loop."""
    _CREATE = None              # the C entry point that makes the group (sac_group_create / td3_group_create / ..._mixed)

    def __init__(self, trainers):
        self.trainers = self._checked_members(trainers)
        self._lib = _lib.load()
        self._g, self._handles = None, None

    @staticmethod
    def _check_hidden(i, t, t0):
        for net in ("policy", "qf1"):
            if t._hidden(net) != t0._hidden(net):
                raise RuntimeError(f"trainer group member {i} has {net} hidden sizes {t._hidden(net)}, member 0 "
                                   f"{t0._hidden(net)}")

    def __len__(self):
        return len(self.trainers)

    def _group(self):
        """The C group over the members' current handles (a member re-creates its handle for another batch size or after
        unpickling: the group follows)."""
        hs = tuple(t._h.value for t in self.trainers)
        if self._g is None or hs != self._handles:
            self._destroy()
            arr = (C.c_void_p * len(hs))(*hs)
            g = C.c_void_p()
            _lib.check(getattr(self._lib, self._CREATE)(C.byref(g), arr, len(hs)), self._CREATE)
            self._g, self._handles = g, hs
        return self._g

    def stage_count(self):
        """sac_group_stage_count: the grouped stages of one full step (the members need their handles: after a
        train_loop, or trainers created with a batch size)."""
        if any(t._h is None for t in self.trainers):
            raise RuntimeError("stage_count needs every member's handle: run train_loop first")
        return _lib.check(self._lib.sac_group_stage_count(self._group()), "sac_group_stage_count")

    def _destroy(self):
        g, self._g = getattr(self, "_g", None), None
        if g:
            self._lib.sac_group_destroy(g)

    def __del__(self):
        self._destroy()

    def _check_general(self):
        for i, t in enumerate(self.trainers):
            if runs_general_step(t):
                net = "policy" if _general_shape(t._hidden("policy")) else "qf1"
                raise RuntimeError(f"trainer group member {i} runs the general step ({net} hidden sizes "
                                   f"{t._hidden(net)}): groups take two hidden layers of at most 256 units")

    @staticmethod
    def _check_buffer(r, b, buffers, dims, whose):
        if b is None or b._h is None:
            raise RuntimeError(f"trainer group buffer {r} has no device storage")
        if any(b is c for c in buffers[:r]):
            raise RuntimeError(f"trainer group buffer {r} is the same buffer as an earlier one")
        if (b._observation_dim, b._action_dim) != dims:
            raise RuntimeError(f"trainer group buffer {r} has dims ({b._observation_dim},{b._action_dim}), {whose} "
                               f"({dims[0]},{dims[1]})")
        if b.num_steps_can_sample() <= 0:
            raise RuntimeError(f"trainer group buffer {r} is empty: random_batch on an empty replay buffer")

    def _run(self, buffers, batches, n_steps):
        """Every member on its batch size, then one sac_group_train_loop call."""
        R = len(self.trainers)
        for t, B in zip(self.trainers, batches):
            if t._h is None or t._batch != B:
                t._create(B)
        g = self._group()
        bufs = (C.c_void_p * R)(*[b._h.value for b in buffers])
        first = np.empty((R, _lib.SAC_DIAG_N), np.float32)
        last = np.empty((R, _lib.SAC_DIAG_N), np.float32)
        _lib.check(self._lib.sac_group_train_loop(g, bufs, int(n_steps), _lib.ptr(first), _lib.ptr(last)),
                   "sac_group_train_loop")
        for r, t in enumerate(self.trainers):
            t._num_train_steps += int(n_steps)
            t._host_policy_stale = True
            t._record(first[r])
        return first, last


class _TrainerGroup(_GroupBase):
    """Members of one shape: the same dims and batch."""

    def _check_member(self, i, t, t0):
        if (t.obs_dim, t.act_dim) != (t0.obs_dim, t0.act_dim):
            raise RuntimeError(f"trainer group member {i} has dims ({t.obs_dim},{t.act_dim}), member 0 "
                               f"({t0.obs_dim},{t0.act_dim})")
        self._check_hidden(i, t, t0)
        self._check_device(i, t, t0)
        if t._batch is not None and t0._batch is not None and t._batch != t0._batch:
            raise RuntimeError(f"trainer group member {i} has batch {t._batch}, member 0 {t0._batch}")

    def train_loop(self, replay_buffers, n_steps, batch_size=None):
        """n_steps x {batch_r = replay_buffers[r].random_batch(B); trainers[r].train(batch_r)} for every member r.
        Returns the first and last step's diagnostics, arrays of shape (R, SAC_DIAG_N)."""
        buffers = list(replay_buffers)
        R = len(self.trainers)
        if len(buffers) != R:
            raise RuntimeError(f"{R} trainers but {len(buffers)} replay buffers")
        B = int(batch_size or self.trainers[0]._batch or 0)
        if B <= 0:
            raise RuntimeError("the batch size is unknown: pass batch_size or create the trainers with one")
        # what can be refused from host metadata is refused before any member's handle is (re)created
        if B > 256:
            raise RuntimeError(f"batch {B}: trainer groups take batches of at most 256 rows")
        self._check_general()
        dims = (self.trainers[0].obs_dim, self.trainers[0].act_dim)
        for r, b in enumerate(buffers):
            self._check_buffer(r, b, buffers, dims, "the trainers")
        return self._run(buffers, [B] * R, n_steps)


class _MixedTrainerGroup(_GroupBase):
    """Members of different tasks: obs_dim, act_dim and batch may differ per member (hidden sizes, algorithm and device
    may not).  Each member trains on its own buffer with its own batch size, bit for bit as its solo train_loop."""
    _MAX_BATCH = 256            # (the fused kernels' grouped instances; the general step has no such bound)

    def _check_member(self, i, t, t0):
        self._check_hidden(i, t, t0)
        self._check_device(i, t, t0)

    def train_loop(self, replay_buffers, n_steps, batch_sizes=None):
        """n_steps x {batch_r = replay_buffers[r].random_batch(B_r); trainers[r].train(batch_r)} for every member r,
        with B_r = batch_sizes[r] (default: the trainer's own batch size).  Returns the first and last step's
        diagnostics, arrays of shape (R, SAC_DIAG_N)."""
        buffers = list(replay_buffers)
        return self._run(buffers, self._prepare(buffers, batch_sizes), n_steps)

    def _prepare(self, buffers, batch_sizes):
        """Every refusal train_loop can make from host metadata; returns the members' batch sizes."""
        R = len(self.trainers)
        if len(buffers) != R:
            raise RuntimeError(f"{R} trainers but {len(buffers)} replay buffers")
        if batch_sizes is None:
            batch_sizes = [None] * R
        batch_sizes = list(batch_sizes)
        if len(batch_sizes) != R:
            raise RuntimeError(f"{R} trainers but {len(batch_sizes)} batch sizes")
        batches = []
        for r, (t, B) in enumerate(zip(self.trainers, batch_sizes)):
            B = int(B or t._batch or 0)
            if B <= 0:
                raise RuntimeError(f"trainer group member {r} has no batch size: pass batch_sizes or create the trainers "
                                   "with one")
            if self._MAX_BATCH and B > self._MAX_BATCH:
                raise RuntimeError(f"trainer group member {r} has batch {B}: trainer groups take batches of at most 256 rows")
            batches.append(B)
        self._check_general()
        for r, b in enumerate(buffers):
            t = self.trainers[r]
            self._check_buffer(r, b, buffers, (t.obs_dim, t.act_dim), "its member")
        return batches


class SACTrainerGroup(_SACMembers, _TrainerGroup):
    _CREATE = "sac_group_create"


class TD3TrainerGroup(_TD3Members, _TrainerGroup):
    """R TD3 runs of one shape; each member keeps its own delayed-update phase (policy_and_target_update_period and the
    step count may differ), and train_loop advances each as TD3Trainer.train_loop does."""
    _CREATE = "td3_group_create"


class MixedSACTrainerGroup(_SACMembers, _MixedTrainerGroup):
    """R SAC runs of different tasks (observation size, action size and batch per member) on one device: the members of
    one kernel variant share each grouped launch, the variants follow one another."""
    _CREATE = "sac_group_create_mixed"


class MixedTD3TrainerGroup(_TD3Members, _MixedTrainerGroup):
    """R TD3 runs of different tasks; each keeps its own delayed-update phase as in TD3TrainerGroup."""
    _CREATE = "td3_group_create_mixed"


class _MlpTrainerGroup(_MixedTrainerGroup):
    """Members of the general step with one set of hidden sizes (the seeds and tasks of one architecture; a sweep over
    architectures is an ArchSACTrainerGroup / ArchTD3TrainerGroup): the hidden sizes, algorithm and device are shared;
    obs_dim, act_dim and batch may differ per member, as in mixed groups.  Members with the shapes of the fused kernels
    are refused: their solo step is not the general step."""
    _MAX_BATCH = None

    def _check_step(self, i, t):
        if not runs_general_step(t):
            raise RuntimeError(f"trainer group member {i} has the shapes of the fused kernels (policy hidden sizes "
                               f"{t._hidden('policy')}, qf hidden sizes {t._hidden('qf1')}): MLP groups take general-step "
                               "members only")

    def _check_general(self):
        pass                    # (checked at construction, by _check_step)


class MlpSACTrainerGroup(_SACMembers, _MlpTrainerGroup):
    """R SAC runs of the general step with one set of hidden sizes (e.g. the seeds of a [512, 512] variant, or several
    tasks at [256, 256, 256]); each stage of the step is one grouped launch over all members."""
    _CREATE = "sac_group_create_mlp"


class MlpTD3TrainerGroup(_TD3Members, _MlpTrainerGroup):
    """R TD3 runs of the general step; each keeps its own delayed-update phase as in TD3TrainerGroup."""
    _CREATE = "td3_group_create_mlp"


class _ArchGeneral(_MlpTrainerGroup):
    """The general-step members of an arch group: one C arch group, hidden sizes free per member."""

    def _check_member(self, i, t, t0):
        self._check_device(i, t, t0)


class _ArchGeneralSAC(_SACMembers, _ArchGeneral):
    _CREATE = "sac_group_create_arch"


class _ArchGeneralTD3(_TD3Members, _ArchGeneral):
    _CREATE = "td3_group_create_arch"


_MEMBER_REF = re.compile(r"\b(member|buffer) (\d+)\b")


class _ArchTrainerGroup(_Members):
    """Members of ANY hidden sizes (a network-size sweep; the paper default [256, 256] included), one algorithm, one
    device.  The general-step members form one C arch group (sac_group_create_arch / td3_group_create_arch: the merged
    schedule of their launch lists, one grouped launch per merged stage); the members with the shapes of the fused
    kernels form one mixed group per distinct (policy, Q) hidden-size pair, which keeps that kind's own rules (batches of
    at most 256 rows ...).  train_loop runs the subgroups one after another, in `run_order`: the fused subgroups in order
    of first appearance, then the general one, each in member order.  Every member's result is bit for bit that of its
    solo train_loop; buffers that sample one host generator (EnvReplayBuffer's default: np.random) continue it as solo
    train_loop calls in `run_order` would."""
    _MIXED = None               # the fused subgroups' kind
    _GENERAL = None             # the general subgroup's kind
    _check_member = staticmethod(_Members._check_device)     # (hidden sizes are free)

    def __init__(self, trainers):
        trainers = self._checked_members(trainers)
        fused, general = {}, []
        for i, t in enumerate(trainers):
            if runs_general_step(t):
                general.append(i)
            else:
                fused.setdefault((tuple(t._hidden("policy")), tuple(t._hidden("qf1"))), []).append(i)
        # (member indices per subgroup, the subgroup): the fused ones in order of first appearance, the general one last
        self._subs = [(idx, self._MIXED([trainers[i] for i in idx])) for idx in fused.values()]
        if general:
            self._subs.append((general, self._GENERAL([trainers[i] for i in general])))
        self.trainers = trainers
        self.run_order = [i for idx, _ in self._subs for i in idx]

    def __len__(self):
        return len(self.trainers)

    @property
    def subgroups(self):
        """The subgroups in run order, each with the indices of its members in the whole group."""
        return [(list(idx), sub) for idx, sub in self._subs]

    @staticmethod
    def _renumber(e, idx):
        """A subgroup's refusal, its member and buffer numbers mapped to the whole group's."""
        def sub(m):
            k = int(m.group(2))
            return f"{m.group(1)} {idx[k]}" if k < len(idx) else m.group(0)
        return RuntimeError(_MEMBER_REF.sub(sub, str(e)))

    def train_loop(self, replay_buffers, n_steps, batch_sizes=None):
        """n_steps x {batch_r = replay_buffers[r].random_batch(B_r); trainers[r].train(batch_r)} for every member r, with
        B_r = batch_sizes[r] (default: the trainer's own batch size), one subgroup after another in `run_order`.
        Every refusal from host metadata comes before any subgroup runs.  Returns the first and last step's
        diagnostics, arrays of shape (R, SAC_DIAG_N) in member order."""
        buffers = list(replay_buffers)
        R = len(self.trainers)
        if len(buffers) != R:
            raise RuntimeError(f"{R} trainers but {len(buffers)} replay buffers")
        batch_sizes = [None] * R if batch_sizes is None else list(batch_sizes)
        if len(batch_sizes) != R:
            raise RuntimeError(f"{R} trainers but {len(batch_sizes)} batch sizes")
        for r, b in enumerate(buffers):
            if b is not None and any(b is c for c in buffers[:r]):
                raise RuntimeError(f"trainer group buffer {r} is the same buffer as an earlier one")
        plans = []
        for idx, sub in self._subs:
            bufs = [buffers[i] for i in idx]
            try:
                plans.append((idx, sub, bufs, sub._prepare(bufs, [batch_sizes[i] for i in idx])))
            except RuntimeError as e:
                raise self._renumber(e, idx) from None
        first = np.empty((R, _lib.SAC_DIAG_N), np.float32)
        last = np.empty((R, _lib.SAC_DIAG_N), np.float32)
        for idx, sub, bufs, batches in plans:
            try:
                f, l = sub._run(bufs, batches, n_steps)
            except RuntimeError as e:
                raise self._renumber(e, idx) from None
            first[idx], last[idx] = f, l
        return first, last


class ArchSACTrainerGroup(_SACMembers, _ArchTrainerGroup):
    """R SAC runs of any hidden sizes (e.g. [256, 256], [512, 512], [256, 256, 256] and [1024] of one or several tasks)
    on one device; see _ArchTrainerGroup."""
    _MIXED = MixedSACTrainerGroup
    _GENERAL = _ArchGeneralSAC


class ArchTD3TrainerGroup(_TD3Members, _ArchTrainerGroup):
    """R TD3 runs of any hidden sizes; each keeps its own delayed-update phase as in TD3TrainerGroup."""
    _MIXED = MixedTD3TrainerGroup
    _GENERAL = _ArchGeneralTD3
