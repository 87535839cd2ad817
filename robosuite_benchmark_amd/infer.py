"""Inference above the C ABI: acting, Q values, loss evaluation, per-unit statistics and per-tensor parameter statistics
for one trainer or many, on live weights.

Every Python inference call -- SACTrainer.policy_act_device / policy_act_general / q_values / evaluate / unit_moments,
act_many, q_values_many, evaluate_many, unit_moments_many, GroupActor and the drivers above them -- goes through three
things defined here once
(DESIGN.md, section 6g):
  the predicate   runs_general_step: does this trainer run the general step?
  the route       route: does one member's request run on the host, through the fused entry or the general entry?
  the windows     windows: a request cut into calls of at most 1024 rows and 16 members, marshalled by handles / ints /
                  pointers.
A solo request is a group of one: the library's solo entries do nothing else.  Also here, because the routes end in
them: the statistics of an evaluation (eval_statistics on the host, the moment records of the device)."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict, namedtuple

import numpy as np

from . import _lib

MAX_MEMBERS = 16                # members of one *_many call, of one acting session, of one trainer group
GENERAL = ("host", "device")
GENERAL_SESSIONS = True         # GroupActor(general="device")'s default for general_sessions: switched on by the
                                # measurement of DESIGN.md, section 6d (the actions are the same bits either way)
STATS = ("host", "device")      # where evaluate's statistics are reduced: eval_statistics, or k_eval_moments on the device


def check_general(general):
    if general not in GENERAL:
        raise RuntimeError(f"general must be one of {GENERAL}, got {general!r}")
    return general


def check_stats(stats):
    if stats not in STATS:
        raise RuntimeError(f"stats must be one of {STATS}, got {stats!r}")
    return stats


# ---- the predicate ------------------------------------------------------------------------------------------------------
def general_shape(hs):
    return len(hs) != 2 or max(hs) > 256


def general_step(t):
    """The predicate behind SACTrainer.runs_general_step: a trainer with a handle runs what the library built
    (sac_trainer_step_kind; SAC_GENERAL=1 builds the general step for the fused kernels' shapes too), a trainer without
    one is judged by its hidden sizes -- a policy or a Q family that is not two layers of at most 256 units."""
    if t._h is not None:
        return int(t._lib.sac_trainer_step_kind(t._h)) == 3
    return _general_sizes(t)


def _general_sizes(t):
    return general_shape(t._hidden("policy")) or general_shape(t._hidden("qf1"))


def runs_general_step(t):
    """Does trainer t run the general step (hidden sizes other than two layers of at most 256 units)?  Such runs group in
    MlpSACTrainerGroup / MlpTD3TrainerGroup, the others in the remaining kinds.  A SACTrainer answers itself
    (runs_general_step); an object without that method -- a stand-in with a handle's face and _hidden, no library behind
    it -- is judged by its hidden sizes."""
    own = getattr(t, "runs_general_step", None)
    return own() if own is not None else _general_sizes(t)


def _is_td3(t):
    return "target_policy" in getattr(t, "NETS", ())


# ---- the route ----------------------------------------------------------------------------------------------------------
HOST, FUSED, GENERAL_STEP = "host", "fused", "general"
ACT_ENTRIES = {FUSED: "sac_policy_act_many", GENERAL_STEP: "sac_policy_act_general_many"}
SESSION_ENTRIES = {FUSED: "sac_actor", GENERAL_STEP: "sac_gactor"}
Q_ENTRIES = {FUSED: "sac_q_values_many", GENERAL_STEP: "sac_q_values_general_many"}
EVAL_ENTRIES = {FUSED: ("sac_evaluate_many", "sac_evaluate_stats_many"),             # (stats "host", "device")
                GENERAL_STEP: ("sac_evaluate_general_many", "sac_evaluate_general_stats_many")}
EVAL_REPLAY_ENTRIES = {FUSED: "sac_evaluate_replay_many",                            # (stats: an argument, NULL for "host")
                       GENERAL_STEP: "sac_evaluate_replay_general_many"}
TD3_EVAL_ENTRIES = {FUSED: "td3_evaluate_many", GENERAL_STEP: "td3_evaluate_general_many"}
TD3_EVAL_STATS_ENTRIES = {FUSED: "td3_evaluate_stats_many",                          # (stats "device")
                          GENERAL_STEP: "td3_evaluate_general_stats_many"}
TD3_EVAL_REPLAY_ENTRIES = {FUSED: "td3_evaluate_replay_many",                        # (stats: an argument, NULL for "host")
                           GENERAL_STEP: "td3_evaluate_replay_general_many"}


def route(t, general, on_host=False):
    """Where one member's request runs: HOST (its own host forward), FUSED or GENERAL_STEP (the key of the request's
    *_ENTRIES).  No handle: the host.  The fused kernels' shapes: the fused entry under either `general`.  The general
    step: the host, or the general entry under general="device".  on_host (evaluation: _evaluate_on_host) sends a member
    with a handle to the host too; a TD3 member's evaluate never gets here (its own evaluate refuses), its evaluate_td3
    does, with TD3_EVAL_ENTRIES: td3_evaluate_many is the fused entry and td3_evaluate_general_many the general one."""
    if t._h is None or on_host:
        return HOST
    if not runs_general_step(t):
        return FUSED
    return GENERAL_STEP if general == "device" else HOST


UNIT_ENTRIES = {FUSED: "sac_unit_moments_many", GENERAL_STEP: "sac_unit_moments_general_many"}


# ---- the windows --------------------------------------------------------------------------------------------------------
def windows(members, n_rows):
    """(r0, ids, counts) per library call: rows r0 = 0, 1024, ... of the members (indices into n_rows) that still have
    rows there, 16 members per call; counts[k] = the rows of ids[k] in this window."""
    for r0 in range(0, max([n_rows[i] for i in members], default=0), _lib.ACT_MAX_ROWS):
        live = [i for i in members if n_rows[i] > r0]
        for c in range(0, len(live), MAX_MEMBERS):
            ids = live[c:c + MAX_MEMBERS]
            yield r0, ids, [min(n_rows[i] - r0, _lib.ACT_MAX_ROWS) for i in ids]


def _handles(trainers, ids):
    return (C.c_void_p * len(ids))(*[trainers[i]._h.value for i in ids])


def _ints(values, ctype=C.c_int32):
    return (ctype * len(values))(*values)


def _pointers(arrays):
    return (C.c_void_p * len(arrays))(*[None if a is None else a.ctypes.data for a in arrays])


def _row_pointers(arrays, r0, ids, counts):
    """The pointer array of one window: rows r0.. of arrays[i] (a C-contiguous array per trainer, or None)."""
    return _pointers([None if arrays[i] is None else arrays[i][r0:r0 + k] for i, k in zip(ids, counts)])


# ---- acting -------------------------------------------------------------------------------------------------------------
def act_calls(lib, entry, trainers, members, n_rows, obs, det, eps, out):
    """The `entry` calls (one of ACT_ENTRIES) for `members`: obs / eps / out hold a float32 array (eps: or None) per
    trainer, n_rows and det one value per trainer; out[i] is written in place."""
    fn = getattr(lib, entry)
    for r0, ids, counts in windows(members, n_rows):
        _lib.check(fn(_handles(trainers, ids), len(ids), _ints(counts), _row_pointers(obs, r0, ids, counts),
                      _ints([int(bool(det[i])) for i in ids]), _row_pointers(eps, r0, ids, counts),
                      _row_pointers(out, r0, ids, counts)), entry)


def act_many(trainers, obs_list, deterministic_list, eps_list, general="host"):
    """policy.get_actions for many runs at once: actions[i] = trainers[i]'s policy on obs_list[i] ((n_i, O_i); None or no
    rows: the member sits out and gets an empty array), deterministic_list[i] as MakeDeterministic, eps_list[i] the
    (n_i, A_i) N(0,1) draws of a stochastic SAC member (None otherwise).  The members with the fused kernels' shapes act
    in ONE launch per 16 of them (sac_policy_act_many: SAC and TD3, dims and row counts mixed; up to 1024 rows each);
    members of the general step act on the host through their own policy_act.  A member's actions never depend on its
    neighbours: they are bit for bit those of its own policy_act_device (policy_act for the general step).
    general="device": the members of the general step act on the device as well, in ONE sac_policy_act_general_many call
    per 16 of them; their actions are bit for bit those of their own policy_act_general."""
    check_general(general)
    trainers = list(trainers)
    R = len(trainers)
    if not (len(obs_list) == len(deterministic_list) == len(eps_list) == R):
        raise RuntimeError("act_many takes one observation array, deterministic flag and eps per trainer")
    if len({id(t) for t in trainers}) != R:
        raise RuntimeError("a trainer appears twice in act_many")
    obs = [None if o is None else _lib.f32(np.atleast_2d(o)) for o in obs_list]
    eps = [None if e is None else _lib.f32(np.atleast_2d(e)) for e in eps_list]
    out = [np.empty((0 if o is None else o.shape[0], t.act_dim), np.float32) for t, o in zip(trainers, obs)]
    served = {FUSED: [], GENERAL_STEP: []}
    for i, t in enumerate(trainers):
        if out[i].shape[0] == 0:
            continue
        if obs[i].shape[1] != t.obs_dim or (eps[i] is not None and eps[i].shape != out[i].shape):
            raise RuntimeError(f"act_many member {i}: observations {obs[i].shape} / eps "
                               f"{None if eps[i] is None else eps[i].shape} do not fit dims ({t.obs_dim}, {t.act_dim})")
        if out[i].shape[0] > _lib.ACT_MAX_ROWS:
            raise RuntimeError(f"act_many member {i}: {out[i].shape[0]} rows (at most {_lib.ACT_MAX_ROWS} per call)")
        where = route(t, general)
        if where == HOST:
            out[i] = t.policy_act(obs[i], deterministic_list[i], eps[i])
        else:
            served[where].append(i)
    lib, n_rows = _lib.load(), [o.shape[0] for o in out]
    for family in (GENERAL_STEP, FUSED):
        act_calls(lib, ACT_ENTRIES[family], trainers, served[family], n_rows, obs, deterministic_list, eps, out)
    return out


# ---- Q values -----------------------------------------------------------------------------------------------------------
def q_values_of(trainers, obs, act, names, masks, rows, general):
    """q_values / q_values_many behind their argument checks, one entry per trainer: obs / act as SACTrainer._q_inputs
    checked them (None: the member sits out), names the nets asked for, masks / rows their _lib.q_net_mask.  The host
    members first, in member order; then the fused family, then the general one, each in windows."""
    R = len(trainers)
    out, n_rows, served = [None] * R, [0] * R, {FUSED: [], GENERAL_STEP: []}
    for i, t in enumerate(trainers):
        if obs[i] is None:
            out[i] = np.empty((len(names[i]), 0), np.float32)
            continue
        where = route(t, general)
        if where == HOST:
            out[i] = t._q_values_host(obs[i], act[i], names[i])
        else:
            out[i], n_rows[i] = np.empty((len(names[i]), obs[i].shape[0]), np.float32), obs[i].shape[0]
            served[where].append(i)
    lib = _lib.load() if served[FUSED] or served[GENERAL_STEP] else None
    for family in (FUSED, GENERAL_STEP):
        entry = Q_ENTRIES[family]
        for r0, ids, counts in windows(served[family], n_rows):
            q = [np.empty((len(names[i]), k), np.float32) for i, k in zip(ids, counts)]
            _lib.check(getattr(lib, entry)(_handles(trainers, ids), len(ids), _ints(counts), _row_pointers(obs, r0, ids, counts),
                                           _row_pointers(act, r0, ids, counts), _ints([masks[i] for i in ids], C.c_uint32),
                                           _pointers(q)), entry)
            for i, k, part in zip(ids, counts, q):
                out[i][:, r0:r0 + k] = part[rows[i]]
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
    check_general(general)
    trainers = list(trainers)
    R = len(trainers)
    if not (len(obs_list) == len(act_list) == len(nets_list) == R):
        raise RuntimeError("q_values_many takes one observation array, action array and net selection per trainer")
    if len({id(t) for t in trainers}) != R:
        raise RuntimeError("a trainer appears twice in q_values_many")
    obs, act, rows, names, masks = [None] * R, [None] * R, [None] * R, [None] * R, [0] * R
    for i, t in enumerate(trainers):
        names[i] = [nets_list[i]] if isinstance(nets_list[i], str) else list(nets_list[i])
        masks[i], rows[i] = _lib.q_net_mask(names[i])
        if obs_list[i] is not None and np.atleast_2d(obs_list[i]).shape[0] != 0:
            obs[i], act[i], _, _ = t._q_inputs(obs_list[i], act_list[i], names[i])
    return q_values_of(trainers, obs, act, names, masks, rows, general)


# ---- per-unit statistics of the hidden layers ---------------------------------------------------------------------------
UNIT_NET_TITLES = OrderedDict([("policy", "Policy"), ("qf1", "QF1"), ("qf2", "QF2"), ("target_qf1", "Target QF1"),
                               ("target_qf2", "Target QF2"), ("target_policy", "Target Policy")])
UNIT_FIGURES = ("Dormant Fraction", "Dead Fraction", "Active Fraction", "Feature Norm")


def _np_max(m, x):
    """em_max (csrc/sac_eval_moments.h) on arrays: x where x > m or x is NaN, else m -- a NaN on either side stays."""
    return np.where((x > m) | (x != x), x, m)


def unit_moments_reference(h):
    """k_unit_moments (csrc/sac_units.h) restated in NumPy float64, operation for operation -- the reference of its tests
    and the body of the host path: the record {count, sum, sumsq, active, max} of one hidden layer's post-ReLU activations
    h (n, N) float32, four float64 arrays of N.  Partial w of 0..3 starts at 0 (max: -inf) and takes rows w, w + 4, ...
    ascending: sum += x, sumsq += x x, active += (h > 0), max = x if x > max or x is NaN; the four partials meet as
    (p0 + p1) + (p2 + p3), max likewise.  A NaN element makes its unit's sum, sumsq and max NaN and is not active."""
    h = np.asarray(h, np.float32)
    if h.ndim != 2 or h.shape[0] < 1:
        raise ValueError(f"unit_moments_reference takes (n, N) activations with at least one row, got {h.shape}")
    n, N = h.shape
    x = h.astype(np.float64)
    part = []
    with np.errstate(all="ignore"):
        for w in range(4):
            s, q, a, m = np.zeros(N), np.zeros(N), np.zeros(N), np.full(N, -np.inf)
            for r in range(w, n, 4):
                s = s + x[r]
                q = q + x[r] * x[r]
                a = a + (h[r] > 0)
                m = _np_max(m, x[r])
            part.append((s, q, a, m))
        p = list(zip(*part))
        total = [(f[0] + f[1]) + (f[2] + f[3]) for f in p[:3]]
        mx = _np_max(_np_max(p[3][0], p[3][1]), _np_max(p[3][2], p[3][3]))
    return dict(count=float(n), sum=total[0], sumsq=total[1], active=total[2], max=mx)


def merge_unit_moments(a, b):
    """The record of two disjoint sets of rows of one layer from their records a and b (a call above 1024 rows runs as
    several windows): count, sum, sumsq and active add, max combines and keeps a NaN.  With activations ("h") the rows
    are joined too."""
    with np.errstate(all="ignore"):
        out = dict(count=a["count"] + b["count"], sum=a["sum"] + b["sum"], sumsq=a["sumsq"] + b["sumsq"],
                   active=a["active"] + b["active"], max=_np_max(a["max"], b["max"]))
    if "h" in a and "h" in b:
        out["h"] = np.concatenate([a["h"], b["h"]], axis=0)
    return out


def unit_statistics(moments, tau=0.025):
    """The figures of a unit_moments result (OrderedDict net -> [record per hidden layer]): an OrderedDict with, per net in
    the order given, under its title of UNIT_NET_TITLES,
      "<Net> Dormant Fraction"   the share of the net's hidden units that are tau-dormant (Sokar et al. 2023): unit u of a
                                 layer is dormant iff sum[u] <= tau * mean_k(sum[k]) of its layer -- the mean activation
                                 against the layer's, without a division: an all-zero layer is all dormant
      "<Net> Dead Fraction"      the share of hidden units with active == 0: active on no row
      "<Net> Active Fraction"    the mean over hidden units of active / count
      "<Net> Feature Norm"       sqrt(sum_u sumsq[u] / count) of the LAST hidden layer: the RMS norm of the features
    NaN follows NumPy: a comparison with a NaN is False (a NaN unit is not dormant, and makes no unit of its layer
    dormant through the layer mean), a NaN is not active, and a NaN sumsq makes the Feature Norm NaN."""
    d = OrderedDict()
    with np.errstate(all="ignore"):
        for net, records in moments.items():
            title = UNIT_NET_TITLES.get(net, net)
            units = sum(r["sum"].size for r in records)
            dormant = sum(int(np.count_nonzero(r["sum"] <= tau * np.mean(r["sum"]))) for r in records)
            dead = sum(int(np.count_nonzero(r["active"] == 0)) for r in records)
            active = sum(float(np.sum(r["active"] / r["count"])) for r in records)
            last = records[-1]
            d[title + " Dormant Fraction"] = dormant / units
            d[title + " Dead Fraction"] = dead / units
            d[title + " Active Fraction"] = active / units
            d[title + " Feature Norm"] = float(np.sqrt(np.sum(last["sumsq"]) / last["count"]))
    return d


def _unit_records(widths, moments, taps, k):
    """One net's records out of a window's outputs: `moments` the net's float64 block (per layer len(UNIT_FIELDS) arrays
    of N), `taps` its float32 activations block ((k, N) per layer) or None."""
    out, m0, h0 = [], 0, 0
    for N in widths:
        rec = dict(count=float(k))
        for f in _lib.UNIT_FIELDS:
            rec[f] = moments[m0:m0 + N].copy()
            m0 += N
        if taps is not None:
            rec["h"] = taps[h0:h0 + k * N].reshape(k, N).copy()
            h0 += k * N
        out.append(rec)
    return out


def unit_moments_of(trainers, obs, act, names, activations, general):
    """unit_moments / unit_moments_many behind their argument checks, one entry per trainer: obs / act as
    SACTrainer._unit_inputs checked them (obs None: the member sits out and gets None), names the nets asked for.  The
    host members first, in member order; then the device families of UNIT_ENTRIES, each in windows, a member's windows
    joined by merge_unit_moments."""
    R = len(trainers)
    out, n_rows, served = [None] * R, [0] * R, {FUSED: [], GENERAL_STEP: []}
    for i, t in enumerate(trainers):
        if obs[i] is None:
            continue
        where = route(t, general)
        if where == HOST:
            out[i] = t._unit_moments_host(obs[i], act[i], names[i], activations)
        else:
            n_rows[i] = obs[i].shape[0]
            served[where].append(i)
    lib = _lib.load() if served[FUSED] or served[GENERAL_STEP] else None
    for family in (FUSED, GENERAL_STEP):
        if not served[family]:
            continue
        entry = UNIT_ENTRIES[family]
        order = {i: sorted(names[i], key=_lib.UNIT_NET_BITS.get) for i in served[family]}
        widths = {i: [trainers[i]._hidden(name) for name in order[i]] for i in served[family]}
        for r0, ids, counts in windows(served[family], n_rows):
            units = [sum(sum(w) for w in widths[i]) for i in ids]
            mom = [np.empty(len(_lib.UNIT_FIELDS) * u, np.float64) for u in units]
            taps = [np.empty(k * u, np.float32) if activations else None for k, u in zip(counts, units)]
            o = [np.ascontiguousarray(obs[i][r0:r0 + k]) for i, k in zip(ids, counts)]
            a = [None if act[i] is None else np.ascontiguousarray(act[i][r0:r0 + k]) for i, k in zip(ids, counts)]
            ios = (_lib.SacUnitsIO * len(ids))(*[
                _lib.SacUnitsIO(o[j].ctypes.data, None if a[j] is None else a[j].ctypes.data,
                                sum(_lib.UNIT_NET_BITS[name] for name in names[i]), 0, mom[j].ctypes.data,
                                None if taps[j] is None else taps[j].ctypes.data) for j, i in enumerate(ids)])
            _lib.check(getattr(lib, entry)(_handles(trainers, ids), len(ids), _ints(counts), ios), entry)
            for j, (i, k) in enumerate(zip(ids, counts)):
                part, m0, h0 = {}, 0, 0
                for name, ws in zip(order[i], widths[i]):
                    u = sum(ws)
                    part[name] = _unit_records(ws, mom[j][m0:m0 + len(_lib.UNIT_FIELDS) * u],
                                               None if taps[j] is None else taps[j][h0:h0 + k * u], k)
                    m0, h0 = m0 + len(_lib.UNIT_FIELDS) * u, h0 + k * u
                if out[i] is None:
                    out[i] = OrderedDict((name, part[name]) for name in names[i])
                else:
                    for name in names[i]:
                        out[i][name] = [merge_unit_moments(x, y) for x, y in zip(out[i][name], part[name])]
    return out


def unit_moments_many(trainers, obs_list, act_list, nets_list, activations=False, general="host"):
    """SACTrainer.unit_moments for many runs at once: result[i] = trainers[i]'s per-unit records of the nets nets_list[i]
    (names, as unit_moments takes them) on obs_list[i] / act_list[i] ((n_i, O_i) / (n_i, A_i), act None where no Q net is
    named; obs None or no rows: the member sits out and gets None).  Routing is unit_moments': the members with the fused
    kernels' shapes are served by ONE k_units launch per 16 of them and 1024 rows (sac_unit_moments_many: SAC and TD3,
    dims, hidden sizes, row counts and nets mixed), under general="device" the members of the general step by ONE
    sac_unit_moments_general_many call per 16 of them and 1024 rows; the others take their own host path inside the same
    call.  A member's records never depend on its neighbours: they are byte for byte those of its own unit_moments."""
    check_general(general)
    trainers = list(trainers)
    R = len(trainers)
    if not (len(obs_list) == len(act_list) == len(nets_list) == R):
        raise RuntimeError("unit_moments_many takes one observation array, action array and net selection per trainer")
    if len({id(t) for t in trainers}) != R:
        raise RuntimeError("a trainer appears twice in unit_moments_many")
    obs, act, names = [None] * R, [None] * R, [None] * R
    for i, t in enumerate(trainers):
        names[i] = [nets_list[i]] if isinstance(nets_list[i], str) else list(nets_list[i])
        if obs_list[i] is not None and np.atleast_2d(obs_list[i]).shape[0] != 0:
            obs[i], act[i] = t._unit_inputs(obs_list[i], act_list[i], names[i])
        else:
            t._unit_names(names[i])
    return unit_moments_of(trainers, obs, act, names, bool(activations), general)


# ---- per-tensor statistics of parameters, Adam moments and target gaps ---------------------------------------------------
PARAM_CH, PARAM_LANES = 16384, 256          # k_param_moments: elements of a chunk, lanes of its workgroup
PARAM_ROUTES = ("device", "host")
PARAM_TRAINED = ("policy", "qf1", "qf2")    # the nets with Adam moments
PARAM_FIGURES = ("Weight Norm", "Weight Abs Max", "Adam M Norm", "Adam V Mean", "Adam V Max")
_FLT_MAX = float(np.finfo(np.float32).max)


def check_route(route_):
    if route_ not in PARAM_ROUTES:
        raise RuntimeError(f"route must be one of {PARAM_ROUTES}, got {route_!r}")
    return route_


def param_target(t, net):
    """The target net whose distance param_moments' gap measures for `net` of trainer t, or None: qf1 / qf2 against
    their targets, on a TD3 trainer the policy against the target policy."""
    if net in ("qf1", "qf2"):
        return "target_" + net
    return "target_policy" if net == "policy" and _is_td3(t) else None


def _param_reduce(x, is_max=False, start=0.0):
    """One field of k_param_moments over the float64 elements x (E,): per chunk of PARAM_CH elements lane l takes
    e = l, l + 256, ... ascending from `start`, the 256 lanes meet by halving (128, 64, ..., 1), the chunks are joined in
    ascending order, left to right; sums add, max fields use em_max.  Positions past E hold `start`, which changes
    nothing (p + 0.0 == p for a p that started at +0.0; em_max(p, start) == p)."""
    op = _np_max if is_max else np.add
    E = x.size
    nch = -(-E // PARAM_CH)
    buf = np.full(nch * PARAM_CH, start, np.float64)
    buf[:E] = x
    buf = buf.reshape(nch, PARAM_CH // PARAM_LANES, PARAM_LANES)
    p = np.full((nch, PARAM_LANES), start, np.float64)
    for r in range(PARAM_CH // PARAM_LANES):
        p = op(p, buf[:, r])
    s = PARAM_LANES // 2
    while s > 0:
        p = op(p[:, :s], p[:, s:2 * s])
        s //= 2
    acc = p[0, 0]
    for c in range(1, nch):
        acc = op(acc, p[c, 0])
    return float(acc)


def param_moments_reference(x, m=None, v=None, target=None):
    """k_param_moments / k_param_finish (csrc/sac_params.h) restated in NumPy float64, operation for operation -- the
    reference of its tests and the body of the host route: the record of one tensor, len(_lib.PARAM_FIELDS) float64
    values, from its float32 elements x in flat order, Adam's moments m and v (None: their fields are 0.0) and the
    target's elements (None: the gap is 0.0).  sum x, sum x x, max |x| (a NaN stays), the count of non-finite elements,
    sum m m, max |m|, sum v, max v (from -inf), sum (x - target)^2 with the difference in float64; the order of every sum
    is _param_reduce's, a function of x.size alone."""
    x = np.asarray(x, np.float32).ravel()
    if x.size < 1:
        raise ValueError("param_moments_reference takes a tensor of at least one element")
    rec = np.zeros(len(_lib.PARAM_FIELDS), np.float64)
    with np.errstate(all="ignore"):
        xd = x.astype(np.float64)
        ax = np.abs(xd)
        rec[0] = _param_reduce(xd)
        rec[1] = _param_reduce(xd * xd)
        rec[2] = _param_reduce(ax, True)
        rec[3] = _param_reduce(np.where(ax <= _FLT_MAX, 0.0, 1.0))
        if m is not None:
            md = np.asarray(m, np.float32).ravel().astype(np.float64)
            vd = np.asarray(v, np.float32).ravel().astype(np.float64)
            if md.size != x.size or vd.size != x.size:
                raise ValueError("param_moments_reference: the moments do not have the tensor's size")
            rec[4] = _param_reduce(md * md)
            rec[5] = _param_reduce(np.abs(md), True)
            rec[6] = _param_reduce(vd)
            rec[7] = _param_reduce(vd, True, -np.inf)
        if target is not None:
            td = np.asarray(target, np.float32).ravel().astype(np.float64)
            if td.size != x.size:
                raise ValueError("param_moments_reference: the target does not have the tensor's size")
            d = xd - td
            rec[8] = _param_reduce(d * d)
    return rec


def param_statistics(moments, sizes, targets=("qf1", "qf2")):
    """The logged figures of a param_moments result (OrderedDict net -> (n_tensors, 9) float64; sizes: net -> the element
    counts of its tensors, as SACTrainer.param_tensors gives the shapes; targets: the nets whose gap was taken -- a TD3
    trainer's include the policy).  An OrderedDict with, per TRAINED net (policy, qf1, qf2) in the order given, under its
    title of UNIT_NET_TITLES,
      "<Net> Weight Norm"      sqrt of the net's sumsq total
      "<Net> Weight Abs Max"   the largest |x| of the net (a NaN stays)
      "<Net> Adam M Norm"      sqrt of the m_sumsq total
      "<Net> Adam V Mean"      the v_sum total over the net's element count
      "<Net> Adam V Max"       the largest second moment
      "<Net> Target Gap"       sqrt(gap_sumsq total) / sqrt(sumsq total), for the nets of `targets`: the distance to the
                               target relative to the net's norm
    and last "Non Finite": the nonfinite total over everything in `moments`, target nets included."""
    F = {k: i for i, k in enumerate(_lib.PARAM_FIELDS)}
    d, bad = OrderedDict(), 0.0
    with np.errstate(all="ignore"):
        for net, rec in moments.items():
            rec = np.asarray(rec, np.float64).reshape(-1, len(_lib.PARAM_FIELDS))
            bad += float(np.sum(rec[:, F["nonfinite"]]))
            if net not in PARAM_TRAINED:
                continue
            title = UNIT_NET_TITLES.get(net, net)
            sumsq = float(np.sum(rec[:, F["sumsq"]]))
            d[title + " Weight Norm"] = float(np.sqrt(sumsq))
            d[title + " Weight Abs Max"] = float(np.max(rec[:, F["absmax"]]))
            d[title + " Adam M Norm"] = float(np.sqrt(np.sum(rec[:, F["m_sumsq"]])))
            d[title + " Adam V Mean"] = float(np.sum(rec[:, F["v_sum"]]) / float(sum(int(e) for e in sizes[net])))
            d[title + " Adam V Max"] = float(np.max(rec[:, F["v_max"]]))
            if net in targets:
                d[title + " Target Gap"] = float(np.sqrt(np.sum(rec[:, F["gap_sumsq"]])) / np.sqrt(sumsq))
    d["Non Finite"] = bad
    return d


def param_moments_of(trainers, names, opt, gap, route_):
    """param_moments / param_moments_many behind their argument checks: names[i] the nets asked of trainers[i] (None: the
    member sits out and gets None).  The members without a handle, and all of them under route "host", take their own
    host route; the others ONE sac_param_moments_many call per 16 of them, both families and both algorithms mixed."""
    R = len(trainers)
    out, served = [None] * R, []
    for i, t in enumerate(trainers):
        if names[i] is None:
            continue
        if t._h is None or route_ == "host":
            out[i] = t._param_moments_host(names[i], opt, gap)
        else:
            served.append(i)
    if not served:
        return out
    lib = _lib.load()
    nf = len(_lib.PARAM_FIELDS)
    flags = (_lib.PARAMS_OPT if opt else 0) | (_lib.PARAMS_GAP if gap else 0)
    order = {i: sorted(names[i], key=_lib.UNIT_NET_BITS.get) for i in served}
    counts = {i: [len(trainers[i].param_tensors(name)) for name in order[i]] for i in served}
    for c in range(0, len(served), MAX_MEMBERS):
        ids = served[c:c + MAX_MEMBERS]
        mom = [np.empty(nf * sum(counts[i]), np.float64) for i in ids]
        ios = (_lib.SacParamsIO * len(ids))(*[
            _lib.SacParamsIO(sum(_lib.UNIT_NET_BITS[name] for name in names[i]), flags, mom[j].ctypes.data)
            for j, i in enumerate(ids)])
        _lib.check(lib.sac_param_moments_many(_handles(trainers, ids), len(ids), ios), "sac_param_moments_many")
        for j, i in enumerate(ids):
            part, m0 = {}, 0
            for name, k in zip(order[i], counts[i]):
                part[name] = mom[j][m0:m0 + nf * k].reshape(k, nf).copy()
                m0 += nf * k
            out[i] = OrderedDict((name, part[name]) for name in names[i])
            trainers[i]._settled()
    return out


def param_moments_many(trainers, nets_list=None, opt=True, gap=True, route="device"):
    """SACTrainer.param_moments for many runs at once: result[i] = trainers[i]'s per-tensor records of the nets
    nets_list[i] (names; None for the list: every net of every trainer; None for a member: it sits out and gets None).
    The members with a handle are served by ONE k_param_moments launch per 16 of them (sac_param_moments_many: SAC and
    TD3, the fused kernels' shapes and the general step, dims and nets mixed), the others -- and all of them under
    route="host" -- by their own host route.  A member's records never depend on its neighbours: they are byte for byte
    those of its own param_moments."""
    check_route(route)
    trainers = list(trainers)
    R = len(trainers)
    if nets_list is None:
        nets_list = [tuple(t.NETS) for t in trainers]
    if len(nets_list) != R:
        raise RuntimeError("param_moments_many takes one net selection per trainer")
    if len({id(t) for t in trainers}) != R:
        raise RuntimeError("a trainer appears twice in param_moments_many")
    names = [None if n is None else t._param_names(n) for t, n in zip(trainers, nets_list)]
    return param_moments_of(trainers, names, bool(opt), bool(gap), route)


# ---- recycling dormant hidden units (ReDo, Sokar et al. 2023) ------------------------------------------------------------
RECYCLE_ROUTES = ("device", "host")
B_INIT_VALUE = 0.1                          # networks._Mlp.__init__'s constant hidden bias


def dormant_units(moments, tau=0.025):
    """The tau-dormant units of a unit_moments result (OrderedDict net -> [record per hidden layer]): an OrderedDict
    net -> [int32 array per hidden layer], ascending -- exactly unit_statistics' predicate, sum[u] <= tau * mean(sum) of
    the layer, with its NaN behaviour (a NaN unit is not listed and, through the mean, nothing of its layer is; an
    all-zero layer is listed whole).  The listed count over the unit count is unit_statistics' Dormant Fraction."""
    out = OrderedDict()
    with np.errstate(all="ignore"):
        for net, records in moments.items():
            out[net] = [np.flatnonzero(r["sum"] <= tau * np.mean(r["sum"])).astype(np.int32) for r in records]
    return out


def _recycle_layers(t, net):
    """[(N_l, K_l, first element of fc<l>.weight, of fc<l>.bias)] per hidden layer of `net` in the flat vector, then
    [(rows, first element)] of every weight that reads the LAST hidden layer (last_fc, and a SAC policy's
    last_fc_log_std), and the vector's size."""
    hidden, heads, off = [], [], 0
    nh = len(t._hidden(net))
    for j, (_, (w, b)) in enumerate(getattr(t, net).layers.items()):
        n, k = w.shape
        if j < nh:
            hidden.append((n, k, off, off + n * k))
        else:
            heads.append((n, off))
        off += n * k + b.size
    return hidden, heads, off


def check_recycle_units(t, units, caller="recycle_units"):
    """recycle_units' unit selection, checked before any library call: a mapping net -> [unit list per hidden layer] over
    trained nets of trainer t (policy, qf1, qf2), each once, one list per hidden layer, every list strictly ascending
    and inside the layer's true width.  Returns it as an OrderedDict net -> [int32 array per hidden layer]."""
    if not hasattr(units, "items"):
        raise ValueError(f"{caller}: units is a mapping net -> [unit list per hidden layer], got {type(units).__name__}")
    out = OrderedDict()
    for net, lists in units.items():
        if net not in _lib.RECYCLE_NETS or net not in t.NETS:
            raise ValueError(f"{caller}: {net!r} is not recycled: one of {_lib.RECYCLE_NETS} (target nets are left alone: "
                             "the Polyak average carries the change over)")
        widths = t._hidden(net)
        lists = list(lists)
        if len(lists) != len(widths):
            raise ValueError(f"{caller}: {net} has {len(widths)} hidden layers, got {len(lists)} unit lists")
        out[net] = []
        for l, (us, N) in enumerate(zip(lists, widths)):
            raw = np.asarray(us if us is not None else [])
            if raw.ndim != 1 or (raw.size and not np.issubdtype(raw.dtype, np.integer)):
                raise ValueError(f"{caller}: {net}, hidden layer {l}: a unit list is a 1-d array of integers")
            a = raw.astype(np.int64)
            if a.size and (a.min() < 0 or a.max() >= N):
                raise ValueError(f"{caller}: {net}, hidden layer {l}: units {a.min()}..{a.max()} outside the layer's "
                                 f"width 0..{N - 1}")
            if a.size > 1 and not (np.diff(a) > 0).all():
                raise ValueError(f"{caller}: {net}, hidden layer {l}: the unit list is not strictly ascending")
            out[net].append(np.ascontiguousarray(a, np.int32))
    if not out:
        raise ValueError(f"{caller} needs at least one network")
    return out


def fresh_unit_rows(trainer, units, rng, b_init_value=B_INIT_VALUE):
    """Fresh incoming rows for the listed units, as networks._Mlp.__init__ draws a hidden layer: per (net, layer) WITH
    units -- nets in the order given, layers ascending -- ONE rng.uniform(-1/sqrt(N_l), 1/sqrt(N_l), (n, K_l)) as
    float32, and the constant bias b_init_value.  An OrderedDict net -> [float32 array (n, K_l + 1) per hidden layer]:
    a unit's K_l weights in flat row order, then its bias (sac_recycle_io_t.fresh).  A layer without units draws nothing."""
    units = check_recycle_units(trainer, units, "fresh_unit_rows")
    out = OrderedDict()
    for net, lists in units.items():
        hidden, _, _ = _recycle_layers(trainer, net)
        out[net] = []
        for us, (N, K, _, _) in zip(lists, hidden):
            rows = np.empty((us.size, K + 1), np.float32)
            if us.size:
                bound = 1.0 / np.sqrt(N)
                rows[:, :K] = rng.uniform(-bound, bound, (us.size, K)).astype(np.float32)
                rows[:, K] = np.float32(b_init_value)
            out[net].append(rows)
    return out


def check_recycle_fresh(t, units, fresh, caller="recycle_units"):
    """The fresh rows that go with checked `units`: net -> [float32 (n, K_l + 1) per hidden layer], shapes checked."""
    out = OrderedDict()
    for net, lists in units.items():
        hidden, _, _ = _recycle_layers(t, net)
        if net not in fresh or len(fresh[net]) != len(lists):
            raise ValueError(f"{caller}: fresh holds no rows for {net}, or not one array per hidden layer")
        out[net] = []
        for l, (us, (N, K, _, _)) in enumerate(zip(lists, hidden)):
            rows = _lib.f32(np.empty((0, K + 1)) if fresh[net][l] is None else fresh[net][l])
            if rows.size != us.size * (K + 1):
                raise ValueError(f"{caller}: {net}, hidden layer {l}: fresh rows must be ({us.size}, {K + 1}): K_l weights, "
                                 "then the bias, per listed unit")
            out[net].append(rows.reshape(us.size, K + 1))
    return out


def recycle_reference(state, trainer, units, fresh, opt=True):
    """sac_recycle_units restated on the flat vectors of SACTrainer._export_state(): a new state (the given one is left
    alone) in which, for a listed unit u of hidden layer l of a trained net,
      incoming   fc<l>.weight[u, :] and fc<l>.bias[u] are the fresh row (K_l weights, then the bias),
      outgoing   column u of fc<l+1>.weight -- for the last hidden layer of last_fc.weight and, on a SAC policy, of
                 last_fc_log_std.weight -- is +0.0,
      moments    with opt, Adam's m and v of every element written are +0.0,
    all incoming rows first, then all outgoing columns: at a crossing zero wins.  Everything else -- target nets, scalars,
    counters -- is the same bytes."""
    units = check_recycle_units(trainer, units, "recycle_reference")
    fresh = check_recycle_fresh(trainer, units, fresh, "recycle_reference")
    new = dict(params={k: np.array(v, np.float32) for k, v in state["params"].items()},
               opt={k: (np.array(m, np.float32), np.array(v, np.float32)) for k, (m, v) in state["opt"].items()},
               scalars=np.array(state["scalars"], np.float64))
    for net, lists in units.items():
        hidden, heads, size = _recycle_layers(trainer, net)
        x = new["params"][net]
        if x.size != size:
            raise ValueError(f"recycle_reference: {net} holds {x.size} parameters, the trainer's has {size}")
        written = np.zeros(size, bool)
        for us, rows, (N, K, off_w, off_b) in zip(lists, fresh[net], hidden):
            for u, row in zip(us, rows):
                x[off_w + u * K:off_w + (u + 1) * K] = row[:K]
                x[off_b + u] = row[K]
                written[off_w + u * K:off_w + (u + 1) * K] = True
                written[off_b + u] = True
        for l, us in enumerate(lists):
            N = hidden[l][0]
            readers = [(hidden[l + 1][0], hidden[l + 1][2])] if l + 1 < len(hidden) else heads
            for rows_out, off in readers:
                for u in us:
                    idx = off + np.arange(rows_out) * N + u
                    x[idx] = np.float32(0.0)
                    written[idx] = True
        if opt:
            m, v = new["opt"][net]
            m[written] = np.float32(0.0)
            v[written] = np.float32(0.0)
    return new


def _recycle_counts(units):
    return OrderedDict((net, int(sum(us.size for us in lists))) for net, lists in units.items())


def recycle_units_of(trainers, units, fresh, opt, route_):
    """recycle_units / recycle_units_many behind their argument checks: units[i] / fresh[i] as check_recycle_units /
    check_recycle_fresh left them (units None: the member sits out and gets None).  The members without a handle, and all
    of them under route "host", take their own host route (export, recycle_reference, import); the others ONE
    sac_recycle_units_many call per 16 of them, both families and both algorithms mixed.  Returns the per-net counts."""
    R = len(trainers)
    out, served = [None] * R, []
    for i, t in enumerate(trainers):
        if units[i] is None:
            continue
        out[i] = _recycle_counts(units[i])
        if t._h is None or route_ == "host":
            t._recycle_host(units[i], fresh[i], opt)
        else:
            served.append(i)
    if not served:
        return out
    lib = _lib.load()
    for c in range(0, len(served), MAX_MEMBERS):
        ids = served[c:c + MAX_MEMBERS]
        keep, ios = [], []
        for i in ids:
            order = sorted(units[i], key=_lib.UNIT_NET_BITS.get)
            counts = np.array([us.size for net in order for us in units[i][net]], np.int32)
            us = np.concatenate([us for net in order for us in units[i][net]] + [np.empty(0, np.int32)]).astype(np.int32)
            rows = np.concatenate([r.ravel() for net in order for r in fresh[i][net]] + [np.empty(0, np.float32)])
            rows = _lib.f32(rows)
            keep.append((counts, us, rows))
            ios.append(_lib.SacRecycleIO(sum(_lib.UNIT_NET_BITS[net] for net in order), _lib.RECYCLE_OPT if opt else 0,
                                         counts.ctypes.data, us.ctypes.data if us.size else None,
                                         rows.ctypes.data if rows.size else None))
        arr = (_lib.SacRecycleIO * len(ids))(*ios)
        _lib.check(lib.sac_recycle_units_many(_handles(trainers, ids), len(ids), arr), "sac_recycle_units_many")
        for i in ids:
            trainers[i]._settled()
            if out[i].get("policy"):
                trainers[i]._host_policy_stale = True        # (as _set_params: the holder's arrays are refreshed at their next use)
    return out


def recycle_units_many(trainers, units_list, fresh_list=None, rngs=None, opt=True, route="device"):
    """SACTrainer.recycle_units for many runs at once: trainers[i]'s units units_list[i] (net -> [unit list per hidden
    layer]; None: the member sits out and gets None) take the rows fresh_list[i], or where those are None rows drawn by
    fresh_unit_rows from rngs[i].  The members with a handle are served by ONE sac_recycle_units_many call per 16 of them
    (two k_unit_recycle launches: SAC and TD3, the fused kernels' shapes and the general step mixed); the others -- and
    all of them under route="host" -- by their own host route.  A member's state never depends on its neighbours: it is
    byte for byte that of its own recycle_units.  Returns per member the per-net counts."""
    if route not in RECYCLE_ROUTES:
        raise RuntimeError(f"route must be one of {RECYCLE_ROUTES}, got {route!r}")
    trainers = list(trainers)
    R = len(trainers)
    fresh_list = [None] * R if fresh_list is None else list(fresh_list)
    rngs = [None] * R if rngs is None else list(rngs)
    if not (len(units_list) == len(fresh_list) == len(rngs) == R):
        raise RuntimeError("recycle_units_many takes one unit selection, one set of fresh rows and one generator per trainer")
    if len({id(t) for t in trainers}) != R:
        raise RuntimeError("a trainer appears twice in recycle_units_many")
    units, fresh = [None] * R, [None] * R
    for i, t in enumerate(trainers):
        if units_list[i] is None:
            continue
        units[i], fresh[i] = t._recycle_inputs(units_list[i], fresh_list[i], rngs[i])
    return recycle_units_of(trainers, units, fresh, bool(opt), route)


# ---- whole-network reset and shrink-and-perturb (Nikishin et al. 2022; Ash & Adams 2020) -----------------------------------
PERTURB_INIT_W = OrderedDict([("policy", 1e-3), ("qf1", 3e-3), ("qf2", 3e-3)])      # the Python constructors' init_w
_U64 = 0xFFFFFFFFFFFFFFFF


def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (csrc/sac_perturb_map.h's philox4x32_10) on uint32-valued uint64 arrays: the four output words."""
    mask, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    c0, c1, c2, c3, k0, k1 = (np.array(x, np.uint64) & mask for x in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & mask, (p0 >> s32) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return c0, c1, c2, c3


def _sign_uniform(net_id, j, E, seed, draw):
    """s = 2u - 1 of the E elements of tensor j of net net_id: u = (float32(word >> 8) + 0.5f) * 2^-24, word = output
    word e & 3 of Philox4x32-10 with counter (e >> 2, j | net_id << 8, draw lo, draw hi), key (seed lo, seed hi)."""
    q = np.arange((E + 3) // 4, dtype=np.uint64)
    words = _philox4x32_10(q, j | net_id << 8, draw & 0xFFFFFFFF, draw >> 32, seed & 0xFFFFFFFF, seed >> 32)
    word = np.stack(words, axis=1).reshape(-1)[:E]
    u = ((word >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    return (u + u) - np.float32(1.0)


def _per_net(value, names, default, what):
    """A per-net float argument: None (the defaults), one number for every net, or a mapping net -> number."""
    out = OrderedDict()
    for net in names:
        v = default[net] if value is None else value.get(net, default[net]) if hasattr(value, "get") else value
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{what} is a number or a mapping net -> number, got {v!r} for {net}")
        out[net] = float(np.float32(v))
    return out


PerturbArgs = namedtuple("PerturbArgs", "nets shrink perturb seed draw opt targets init_w b_init")


def check_shrink_perturb(t, nets=None, shrink=0.8, perturb=0.2, seed=None, draw=0, opt=True, targets=False, init_w=None,
                         b_init=None, caller="shrink_perturb"):
    """shrink_perturb's arguments, checked before any library call (sac_shrink_perturb's refusals): a PerturbArgs with the
    selected trained nets in id order, shrink and perturb as float32 values, seed (None: the trainer's noise seed) and
    draw as 64-bit words, init_w / b_init per selected net as float32 values."""
    if nets is None:
        nets = PARAM_TRAINED
    if isinstance(nets, str):
        nets = (nets,)
    nets = tuple(nets)
    for net in nets:
        if net not in PARAM_TRAINED or net not in t.NETS:
            raise ValueError(f"{caller}: {net!r} is not a trained net: one of {PARAM_TRAINED} (a target is written through "
                             "its trained net with targets=True)")
    if not nets or len(set(nets)) != len(nets):
        raise ValueError(f"{caller} needs at least one network, each once")
    names = tuple(n for n in PARAM_TRAINED if n in nets)
    with np.errstate(all="ignore"):
        sh, pe = np.float32(shrink), np.float32(perturb)
    if not (np.isfinite(sh) and np.isfinite(pe) and sh >= 0 and pe >= 0):
        raise ValueError(f"{caller}: shrink {shrink!r} and perturb {perturb!r} must be finite float32 values, not negative")
    if sh == 0 and pe == 0:
        raise ValueError(f"{caller}: shrink and perturb are both zero")
    for what, v in (("seed", t.noise_seed if seed is None else seed), ("draw", draw)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= _U64:
            raise ValueError(f"{caller}: {what} is a 64-bit unsigned integer, got {v!r}")
    with np.errstate(all="ignore"):
        iw = _per_net(init_w, names, PERTURB_INIT_W, f"{caller}: init_w")
        bi = _per_net(b_init, names, dict.fromkeys(PARAM_TRAINED, B_INIT_VALUE), f"{caller}: b_init")
    for net in names:
        if not (np.isfinite(iw[net]) and iw[net] >= 0):
            raise ValueError(f"{caller}: init_w of {net} must be finite and not negative, got {iw[net]!r}")
        if not np.isfinite(bi[net]):
            raise ValueError(f"{caller}: b_init of {net} must be finite, got {bi[net]!r}")
    return PerturbArgs(names, float(sh), float(pe), int(t.noise_seed if seed is None else seed), int(draw), bool(opt),
                       bool(targets), iw, bi)


def fresh_params(trainer, net, seed, draw, init_w=None, b_init=None):
    """The flat float32 vector of FRESH values of a trained net, as k_param_perturb draws them (csrc/sac_perturb_map.h):
    element e of tensor j of net k (its C id) is
      hidden weight fc<l>.weight   bound * s, bound = float32(1 / sqrt(N_l))    (networks._Mlp's out-size rule)
      hidden bias   fc<l>.bias     the constant b_init
      head weight and head bias    init_w * s
    with s = 2u - 1 from Philox4x32-10 at counter (e >> 2, j | k << 8, draw), key seed, output word e & 3.  init_w and
    b_init default to the Python constructors' (1e-3 for a policy, 3e-3 for a Q net; B_INIT_VALUE)."""
    a = check_shrink_perturb(trainer, (net,), 0.0, 1.0, seed, draw, init_w=init_w, b_init=b_init, caller="fresh_params")
    k, nh = _lib.NET_IDS[net], len(trainer._hidden(net))
    out = []
    for j, (_, shape) in enumerate(trainer.param_tensors(net)):
        E = int(np.prod(shape))
        if j < 2 * nh and j & 1:
            out.append(np.full(E, a.b_init[net], np.float32))
            continue
        scale = np.float32(1.0 / np.sqrt(np.float64(shape[0]))) if j < 2 * nh else np.float32(a.init_w[net])
        out.append(scale * _sign_uniform(k, j, E, a.seed, a.draw))
    return np.concatenate(out).astype(np.float32)


def _shrink_perturb_state(state, trainer, a):
    """shrink_perturb_reference behind the argument checks (a: PerturbArgs)."""
    new = dict(params={k: np.array(v, np.float32) for k, v in state["params"].items()},
               opt={k: (np.array(m, np.float32), np.array(v, np.float32)) for k, (m, v) in state["opt"].items()},
               scalars=np.array(state["scalars"], np.float64))
    sh, pe = np.float32(a.shrink), np.float32(a.perturb)
    for net in a.nets:
        x = new["params"][net]
        with np.errstate(all="ignore"):
            if pe != 0:
                y = pe * fresh_params(trainer, net, a.seed, a.draw, a.init_w[net], a.b_init[net])
                if y.size != x.size:
                    raise ValueError(f"shrink_perturb_reference: {net} holds {x.size} parameters, the trainer's has {y.size}")
                if sh != 0:
                    y = sh * x + y
            else:
                y = sh * x
        new["params"][net] = y.astype(np.float32)
        if a.opt:
            new["opt"][net] = (np.zeros(x.size, np.float32), np.zeros(x.size, np.float32))
        tname = param_target(trainer, net) if a.targets else None
        if tname is not None and tname in new["params"]:
            new["params"][tname] = new["params"][net].copy()
    return new


def shrink_perturb_reference(state, trainer, nets=None, shrink=0.8, perturb=0.2, seed=None, draw=0, opt=True, targets=False,
                             init_w=None, b_init=None):
    """sac_shrink_perturb restated on the flat vectors of SACTrainer._export_state(): a new state (the given one is left
    alone) in which every element x of a selected trained net is
      x' = float32(shrink) * x + float32(perturb) * f       each product and the sum rounded to float32 on its own;
    f = fresh_params' value of the element; a term whose factor is 0 is not formed (shrink == 0: the old value, a NaN too,
    does not reach the result; shrink != 0: a NaN stays).  With opt, Adam's m and v of the selected nets are +0.0; with
    targets, the paired target (param_target) is the same bits.  Everything else -- scalars, counters -- is the same bytes."""
    a = check_shrink_perturb(trainer, nets, shrink, perturb, seed, draw, opt, targets, init_w, b_init, "shrink_perturb_reference")
    return _shrink_perturb_state(state, trainer, a)


def shrink_perturb_of(trainers, args, route_):
    """shrink_perturb / shrink_perturb_many behind their argument checks: args[i] a PerturbArgs, or None: the member sits
    out and gets None.  The members without a handle, and all of them under route "host", take their own host route
    (export, shrink_perturb_reference, import); the others ONE sac_shrink_perturb_many call -- one k_param_perturb launch --
    per 16 of them, both families and both algorithms mixed.  Returns per member the names of the nets written."""
    out, served = [None] * len(trainers), []
    for i, (t, a) in enumerate(zip(trainers, args)):
        if a is None:
            continue
        out[i] = a.nets
        if t._h is None or route_ == "host":
            t._shrink_perturb_host(a)
        else:
            served.append(i)
    if not served:
        return out
    lib = _lib.load()
    for c in range(0, len(served), MAX_MEMBERS):
        ids = served[c:c + MAX_MEMBERS]
        ios = []
        for i in ids:
            a = args[i]
            iw = [a.init_w.get(n, 0.0) for n in PARAM_TRAINED]
            bi = [a.b_init.get(n, 0.0) for n in PARAM_TRAINED]
            flags = (_lib.PERTURB_OPT if a.opt else 0) | (_lib.PERTURB_TARGETS if a.targets else 0)
            ios.append(_lib.SacPerturbIO(sum(_lib.UNIT_NET_BITS[n] for n in a.nets), flags, a.shrink, a.perturb, a.seed, a.draw,
                                         (C.c_float * 3)(*iw), (C.c_float * 3)(*bi)))
        arr = (_lib.SacPerturbIO * len(ids))(*ios)
        _lib.check(lib.sac_shrink_perturb_many(_handles(trainers, ids), len(ids), arr), "sac_shrink_perturb_many")
        for i in ids:
            trainers[i]._settled()
            if "policy" in args[i].nets:
                trainers[i]._host_policy_stale = True        # (as _set_params: the holder's arrays are refreshed at their next use)
    return out


def _member_values(value, R, what):
    """A shared argument, or one per member (a list or tuple of R)."""
    if isinstance(value, (list, tuple)):
        if len(value) != R:
            raise RuntimeError(f"shrink_perturb_many takes one {what} per trainer, or one for all")
        return list(value)
    return [value] * R


def shrink_perturb_many(trainers, nets_list=None, shrink=0.8, perturb=0.2, seeds=None, draws=0, opt=True, targets=False,
                        init_w=None, b_init=None, route="device"):
    """SACTrainer.shrink_perturb for many runs at once.  nets_list: None for the list: every trained net of every trainer;
    else one selection per trainer, None for a member: it sits out and gets None.  shrink, perturb, seeds, draws, opt,
    targets, init_w and b_init are shared values or lists with one value per trainer (seeds None: each trainer's noise
    seed).  The members with a handle are served by ONE sac_shrink_perturb_many call per 16 of them (one k_param_perturb
    launch: SAC and TD3, the fused kernels' shapes and the general step mixed); the others -- and all of them under
    route="host" -- by their own host route.  A member's state never depends on its neighbours: it is byte for byte that
    of its own shrink_perturb.  Returns per member the names of the nets written."""
    if route not in RECYCLE_ROUTES:
        raise RuntimeError(f"route must be one of {RECYCLE_ROUTES}, got {route!r}")
    trainers = list(trainers)
    R = len(trainers)
    if nets_list is None:
        nets_list = [PARAM_TRAINED] * R
    if len(nets_list) != R:
        raise RuntimeError("shrink_perturb_many takes one net selection per trainer")
    if len({id(t) for t in trainers}) != R:
        raise RuntimeError("a trainer appears twice in shrink_perturb_many")
    per = [_member_values(v, R, w) for v, w in ((shrink, "shrink"), (perturb, "perturb"), (seeds, "seed"), (draws, "draw"),
                                                (opt, "opt"), (targets, "targets"), (init_w, "init_w"), (b_init, "b_init"))]
    args = [None if nets_list[i] is None else
            check_shrink_perturb(t, nets_list[i], *(v[i] for v in per), caller="shrink_perturb_many")
            for i, t in enumerate(trainers)]
    return shrink_perturb_of(trainers, args, route)


# ---- evaluation: its statistics -----------------------------------------------------------------------------------------
def eval_target(rew, term, tq1, tq2, log_pi_next, alpha, reward_scale, discount):
    """k_eval's y in float32 NumPy, operation for operation:
    y = rs * r + ((1 - d) * discount) * (min(tq1, tq2) - alpha * log_pi_next), each result rounded to float32."""
    f = np.float32
    rew, term, tq1, tq2, lp = (np.asarray(x, f) for x in (rew, term, tq1, tq2, log_pi_next))
    return f(reward_scale) * rew + ((f(1.0) - term) * f(discount)) * (np.fmin(tq1, tq2) - f(alpha) * lp)


def _eval_columns(chunks, row_names, array_names):
    """The per-row columns of an evaluation from its chunks' outputs: rows (len(row_names), k) and one (k, A) array per
    name of array_names -- _lib.EVAL_ROWS / EVAL_ARRAYS for evaluate, _lib.TD3_EVAL_ROWS / TD3_EVAL_ARRAYS for evaluate_td3."""
    cols = OrderedDict()
    rows = np.concatenate([c["rows"] for c in chunks], axis=1)
    for i, name in enumerate(row_names):
        cols[name] = np.ascontiguousarray(rows[i])
    for name in array_names:
        cols[name] = np.concatenate([c[name] for c in chunks], axis=0)
    return cols


def _sac_eval_columns(chunks, alpha):
    cols = _eval_columns(chunks, _lib.EVAL_ROWS, _lib.EVAL_ARRAYS)
    cols["alpha"] = float(alpha)
    return cols


def _eval_io(struct, row_names, array_names, arrs, i, j, act_dim, outputs=True):
    """(io, out, parts): `struct` (SacEvalIO, Td3EvalIO) over rows i..j of an evaluation's inputs arrs, the output arrays
    it points to -- out["rows"] and one (j - i, act_dim) array per name of array_names -- and the input slices, to be kept
    alive.  An input that is None (evaluate_replay: the arrays the device takes from the replay storage) stays NULL.
    outputs=False (the *_stats_many entries alone take it): no output array is made, out is None and its fields NULL."""
    parts = [None if a is None else np.ascontiguousarray(a[i:j]) for a in arrs]
    ins = [None if p is None else p.ctypes.data for p in parts]
    if not outputs:
        return struct(*ins), None, parts
    out = dict(rows=np.empty((len(row_names), j - i), np.float32))
    out.update((name, np.empty((j - i, act_dim), np.float32)) for name in array_names)
    return struct(*ins, out["rows"].ctypes.data, *[out[name].ctypes.data for name in array_names]), out, parts


def _four_figures(d, name, x):
    """d[name + " Mean" / " Std" (np.std) / " Max" / " Min"] of x in float64."""
    x = np.asarray(x, np.float64).ravel()
    d[name + " Mean"], d[name + " Std"] = float(np.mean(x)), float(np.std(x))
    d[name + " Max"], d[name + " Min"] = float(np.max(x)), float(np.min(x))


def _member_args(caller, takes, trainers, *per_member):
    """The per-member arguments of the *_many evaluation calls: the trainers as a list, each of them once, and every
    argument of per_member as a list of one entry per trainer (None: no entry for anyone)."""
    trainers = list(trainers)
    R = len(trainers)
    lists = [[None] * R if x is None else list(x) for x in per_member]
    if any(len(x) != R for x in lists):
        raise RuntimeError(f"{caller} takes one {takes} per trainer")
    if len({id(t) for t in trainers}) != R:
        raise RuntimeError(f"a trainer appears twice in {caller}")
    return [trainers] + lists


def eval_statistics(rows, mu, log_std, alpha, log_alpha, target_entropy, auto):
    """The statistics of SACTrainer.evaluate from its per-row columns, on the host in float64: `rows` is the
    (SAC_EVAL_ROWS_N, n) array q1, q2, q1_new, q2_new, tq1, tq2, log_pi, log_pi_next, y (_lib.EVAL_ROWS), mu / log_std the
    policy head's (n, A) mean and clamped log_std.  An OrderedDict with get_diagnostics()' keys in their order --
    QF Loss = mean((q - y)^2); Policy Loss = mean(log_pi - min(q1_new, q2_new)), the reference's logged form without
    alpha; Mean / Std (np.std) / Max / Min of q1, q2, y, log_pi, mu, log_std; Alpha; Alpha Loss =
    -mean(log_alpha * (log_pi + target_entropy)), 0 with tuning off -- followed by TD Error 1 / TD Error 2 Mean / Std /
    Max / Min (q - y, signed)."""
    r = [np.asarray(x, np.float64).ravel() for x in rows]
    q1, q2, q1n, q2n, _, _, lp, _, y = r
    stats = _four_figures
    d = OrderedDict()
    d["QF1 Loss"] = float(np.mean((q1 - y) ** 2))
    d["QF2 Loss"] = float(np.mean((q2 - y) ** 2))
    d["Policy Loss"] = float(np.mean(lp - np.minimum(q1n, q2n)))
    stats(d, "Q1 Predictions", q1)
    stats(d, "Q2 Predictions", q2)
    stats(d, "Q Targets", y)
    stats(d, "Log Pis", lp)
    stats(d, "Policy mu", mu)
    stats(d, "Policy log std", log_std)
    d["Alpha"] = float(alpha)
    d["Alpha Loss"] = float(-np.mean(float(log_alpha) * (lp + float(target_entropy)))) if auto else 0.0
    stats(d, "TD Error 1", q1 - y)
    stats(d, "TD Error 2", q2 - y)
    return d


def _moment_records(names, xs):
    """One record {count, sum, m2, sumsq, max, min} per name over its elements x, in float64: m2 = sum((x - sum / count)^2),
    a second pass as np.std's; max and min keep a NaN."""
    out = OrderedDict()
    with np.errstate(all="ignore"):
        for name, x in zip(names, xs):
            s = float(np.sum(x))
            out[name] = dict(count=float(x.size), sum=s, m2=float(np.sum((x - s / x.size) ** 2)), sumsq=float(np.sum(x * x)),
                             max=float(np.max(x)), min=float(np.min(x)))
    return out


def eval_moments(rows, mu, log_std):
    """k_eval_moments (csrc/sac_eval_moments.h) restated in NumPy float64 -- the reference of its tests and nothing else:
    an OrderedDict with one record {count, sum, m2, sumsq, max, min} per name of _lib.EVAL_MOMENTS, over q1, q2, y, log_pi
    (n elements), mu, log_std (n A), td1 = q1 - y, td2 = q2 - y and policy = log_pi - min(q1_new, q2_new) (n), every
    element formed in float64 from the columns given.  m2 = sum((x - sum / count)^2), a second pass as np.std's; max and
    min keep a NaN."""
    r = [np.asarray(x, np.float64).ravel() for x in rows]
    q1, q2, q1n, q2n, _, _, lp, _, y = r
    flat = lambda x: np.asarray(x, np.float64).ravel()               # noqa: E731
    return _moment_records(_lib.EVAL_MOMENTS, [q1, q2, y, lp, flat(mu), flat(log_std), q1 - y, q2 - y, lp - np.minimum(q1n, q2n)])


def merge_moments(a, b):
    """The record of two disjoint sets of elements of one quantity from their records a and b (a call above 1024 rows
    runs as several launches): count, sum and sumsq add, max and min combine (a NaN stays), and
    m2 = m2_a + m2_b + delta^2 n_a n_b / (n_a + n_b) with delta the difference of the two means."""
    na, nb = a["count"], b["count"]
    n = na + nb
    delta = b["sum"] / nb - a["sum"] / na
    return dict(count=n, sum=a["sum"] + b["sum"], m2=a["m2"] + b["m2"] + delta * delta * (na * nb / n),
                sumsq=a["sumsq"] + b["sumsq"], max=float(np.maximum(a["max"], b["max"])),
                min=float(np.minimum(a["min"], b["min"])))


def _merge_all(a, b):
    """merge_moments per quantity; a None: b."""
    return b if a is None else OrderedDict((k, merge_moments(a[k], b[k])) for k in a)


def _stats_moments(st, names=_lib.EVAL_MOMENTS):
    """The records of one sac_eval_stats_t as eval_moments returns them (names=_lib.TD3_EVAL_MOMENTS: of one
    td3_eval_stats_t, as td3_eval_moments does)."""
    vals = np.frombuffer(st, np.float64, len(names) * len(_lib.EVAL_MOMENT_FIELDS)).tolist()
    k = len(_lib.EVAL_MOMENT_FIELDS)
    return OrderedDict((name, dict(zip(_lib.EVAL_MOMENT_FIELDS, vals[i * k:(i + 1) * k])))
                       for i, name in enumerate(names))


def _moment_figures(d, name, m):
    """_four_figures from a moment record: Mean = sum / count, Std = sqrt(m2 / count), Max and Min as stored."""
    d[name + " Mean"], d[name + " Std"] = m["sum"] / m["count"], float(np.sqrt(m["m2"] / m["count"]))
    d[name + " Max"], d[name + " Min"] = m["max"], m["min"]


def moments_statistics(moments, alpha, log_alpha, target_entropy, auto):
    """eval_statistics' OrderedDict -- the same keys in the same order -- from the moment records of eval_moments or of
    the device (sac_evaluate_stats_many): Mean = sum / count, Std = sqrt(m2 / count), Max and Min as stored, QF Loss =
    td.sumsq / count, Policy Loss = policy.sum / count, Alpha Loss = -(log_alpha (log_pi.sum / count + target_entropy)),
    0 with tuning off."""
    M, stats = moments, _moment_figures
    d = OrderedDict()
    with np.errstate(all="ignore"):
        d["QF1 Loss"] = M["td1"]["sumsq"] / M["td1"]["count"]
        d["QF2 Loss"] = M["td2"]["sumsq"] / M["td2"]["count"]
        d["Policy Loss"] = M["policy"]["sum"] / M["policy"]["count"]
        for name, key in (("Q1 Predictions", "q1"), ("Q2 Predictions", "q2"), ("Q Targets", "y"), ("Log Pis", "log_pi"),
                          ("Policy mu", "mu"), ("Policy log std", "log_std")):
            stats(d, name, M[key])
        d["Alpha"] = float(alpha)
        d["Alpha Loss"] = -(float(log_alpha) * (M["log_pi"]["sum"] / M["log_pi"]["count"] + float(target_entropy))) if auto else 0.0
        stats(d, "TD Error 1", M["td1"])
        stats(d, "TD Error 2", M["td2"])
    return d


# ---- evaluation of the TD3 objectives: its statistics -------------------------------------------------------------------
def td3_eval_target(rew, term, tq1, tq2, reward_scale, discount):
    """k_eval_td3's y in float32 NumPy, operation for operation:
    y = rs * r + ((1 - d) * discount) * min(tq1, tq2), each result rounded to float32 (np.fmin, as fminf)."""
    f = np.float32
    rew, term, tq1, tq2 = (np.asarray(x, f) for x in (rew, term, tq1, tq2))
    return f(reward_scale) * rew + ((f(1.0) - term) * f(discount)) * np.fmin(tq1, tq2)


def td3_smooth(a_target, eps, sigma, clip):
    """The smoothed target action of the TD3 step in float32 NumPy: a_target + clip(eps * sigma, -clip, clip).  The sum is
    not clipped again; a NaN draw stays a NaN."""
    f = np.float32
    a_target, eps = np.asarray(a_target, f), np.asarray(eps, f)
    return a_target + np.clip(eps * f(sigma), -f(clip), f(clip))


def td3_eval_statistics(rows, a_pi):
    """The statistics of TD3Trainer.evaluate_td3 from its per-row columns, on the host in float64: `rows` is the
    (TD3_EVAL_ROWS_N, n) array q1, q2, q_pi, tq1, tq2, y (_lib.TD3_EVAL_ROWS), a_pi the policy's (n, A) actions.  An
    OrderedDict with TD3Trainer.get_diagnostics()' keys in their order -- QF Loss = mean((q - y)^2); Policy Loss =
    -mean(q_pi); Mean / Std (np.std) / Max / Min of q1, q2, y, the Bellman errors (q - y)^2 and a_pi -- followed by
    TD Error 1 / TD Error 2 Mean / Std / Max / Min (q - y, signed)."""
    q1, q2, q_pi, _, _, y = [np.asarray(x, np.float64).ravel() for x in rows]
    stats = _four_figures
    d = OrderedDict()
    with np.errstate(all="ignore"):
        b1, b2 = (q1 - y) ** 2, (q2 - y) ** 2
        d["QF1 Loss"] = float(np.mean(b1))
        d["QF2 Loss"] = float(np.mean(b2))
        d["Policy Loss"] = float(-np.mean(q_pi))
        stats(d, "Q1 Predictions", q1)
        stats(d, "Q2 Predictions", q2)
        stats(d, "Q Targets", y)
        stats(d, "Bellman Errors 1", b1)
        stats(d, "Bellman Errors 2", b2)
        stats(d, "Policy Action", a_pi)
        stats(d, "TD Error 1", q1 - y)
        stats(d, "TD Error 2", q2 - y)
    return d


def td3_eval_moments(rows, a_pi):
    """k_eval_moments_td3 (csrc/td3_eval_moments.h) restated in NumPy float64 -- the reference of its tests and nothing
    else: an OrderedDict with one record {count, sum, m2, sumsq, max, min} per name of _lib.TD3_EVAL_MOMENTS, over q1, q2,
    y, q_pi (n elements), a_pi (n A), td1 = q1 - y, td2 = q2 - y and bellman1 / bellman2 = (q - y)^2 (n), every element
    formed in float64 from the columns given.  m2 = sum((x - sum / count)^2), a second pass as np.std's; max and min keep
    a NaN."""
    q1, q2, q_pi, _, _, y = [np.asarray(x, np.float64).ravel() for x in rows]
    with np.errstate(all="ignore"):
        xs = [q1, q2, y, q_pi, np.asarray(a_pi, np.float64).ravel(), q1 - y, q2 - y, (q1 - y) ** 2, (q2 - y) ** 2]
    return _moment_records(_lib.TD3_EVAL_MOMENTS, xs)


def td3_moments_statistics(moments):
    """td3_eval_statistics' OrderedDict -- the same keys in the same order -- from the moment records of td3_eval_moments
    or of the device (td3_evaluate_stats_many): Mean = sum / count, Std = sqrt(m2 / count), Max and Min as stored,
    QF Loss = bellman.sum / count, Policy Loss = -(q_pi.sum / count)."""
    M = moments
    d = OrderedDict()
    with np.errstate(all="ignore"):
        d["QF1 Loss"] = M["bellman1"]["sum"] / M["bellman1"]["count"]
        d["QF2 Loss"] = M["bellman2"]["sum"] / M["bellman2"]["count"]
        d["Policy Loss"] = -(M["q_pi"]["sum"] / M["q_pi"]["count"])
        for name, key in (("Q1 Predictions", "q1"), ("Q2 Predictions", "q2"), ("Q Targets", "y"),
                          ("Bellman Errors 1", "bellman1"), ("Bellman Errors 2", "bellman2"), ("Policy Action", "a_pi"),
                          ("TD Error 1", "td1"), ("TD Error 2", "td2")):
            _moment_figures(d, name, M[key])
    return d


# ---- evaluation: one call path for both objectives ----------------------------------------------------------------------
def replay_route(t, buffer, general):
    """route for a member of evaluate_replay: a buffer without device storage (no handle) sends it to the host too."""
    return route(t, general, t._evaluate_on_host or getattr(buffer, "_h", None) is None)


def _refuse_sac_members(caller, trainers, instead):
    for i, t in enumerate(trainers):
        if not _is_td3(t):
            raise RuntimeError(f"{caller} member {i} is a SAC trainer: this call evaluates the TD3 objective (a "
                               f"deterministic policy with target smoothing); {instead} evaluates the SAC objective")


# What the call path below needs to know about an objective:
#   td3                               the TD3 objective: it refuses SAC members in front of everything (_refuse_sac_members);
#                                     the SAC objective refuses a TD3 member through TD3Trainer.evaluate[_replay] raising
#   io, stats                         the ctypes structs of the entries
#   rows, arrays, moments             the names of the per-row columns, of the (n, A) arrays and of the moment records
#   entries, stats_entries, replay_entries   family -> entry: plain, with statistics, on replay rows
#   draws                             the N(0,1) arrays of a request: the inputs behind the five arrays of a transition
#   inputs, host, request             the trainer's methods: a batch's checked arrays, the host forward (arrays ->
#                                     columns), a replay request's checked (indices, draws)
#   host_stats(t, cols)               the statistics of the columns on the host
#   device_stats(t, moments, alpha, log_alpha)   the same keys from the device's moment records
#   columns(chunks, alpha)            what becomes of a member's chunks (SAC adds `alpha`)
Objective = namedtuple("Objective", "td3 io stats rows arrays moments entries stats_entries replay_entries draws inputs host "
                                    "request host_stats device_stats columns")
SAC_OBJECTIVE = Objective(
    False, _lib.SacEvalIO, _lib.SacEvalStats, _lib.EVAL_ROWS, _lib.EVAL_ARRAYS, _lib.EVAL_MOMENTS,
    {f: e[0] for f, e in EVAL_ENTRIES.items()}, {f: e[1] for f, e in EVAL_ENTRIES.items()}, EVAL_REPLAY_ENTRIES, 2,
    "_eval_inputs", "_evaluate_host", "_replay_request", lambda t, cols: t._eval_stats(cols),
    lambda t, m, alpha, log_alpha: moments_statistics(m, alpha, log_alpha, t.target_entropy, t.use_automatic_entropy_tuning),
    _sac_eval_columns)
TD3_OBJECTIVE = Objective(
    True, _lib.Td3EvalIO, _lib.Td3EvalStats, _lib.TD3_EVAL_ROWS, _lib.TD3_EVAL_ARRAYS, _lib.TD3_EVAL_MOMENTS,
    TD3_EVAL_ENTRIES, TD3_EVAL_STATS_ENTRIES, TD3_EVAL_REPLAY_ENTRIES, 1,
    "_td3_eval_inputs", "_evaluate_td3_host", "_td3_replay_request",
    lambda t, cols: td3_eval_statistics(np.stack([cols[k] for k in _lib.TD3_EVAL_ROWS]), cols["a_pi"]),
    lambda t, m, alpha, log_alpha: td3_moments_statistics(m),
    lambda chunks, alpha: _eval_columns(chunks, _lib.TD3_EVAL_ROWS, _lib.TD3_EVAL_ARRAYS))


def _evaluate_of(ob, trainers, inputs, rows, general, stats, replay=None):
    """evaluate_of / td3_evaluate_of for objective ob.  The host members first, in member order; then the fused family, then
    the general one, each in windows of its entry: 16 members and 1024 rows per call.  Every member served on the device
    is settled behind its calls (the library ran sac_sync on it)."""
    on_device = stats == "device"
    R = len(trainers)
    out, n_rows, served = [None] * R, [0] * R, {FUSED: [], GENERAL_STEP: []}
    for i, (t, arrs) in enumerate(zip(trainers, inputs)):
        if arrs is None:
            continue
        where = route(t, general, t._evaluate_on_host) if replay is None else replay_route(t, replay[i][0], general)
        if where == HOST:
            if replay is not None:
                arrs = getattr(t, ob.inputs)(replay[i][0].gather(replay[i][1]), arrs[5:] if ob.draws > 1 else arrs[5], None)
            cols = getattr(t, ob.host)(arrs)
            result = ob.host_stats(t, cols)
            out[i] = (result, cols) if rows else result
        else:
            n_rows[i] = arrs[5].shape[0]
            served[where].append(i)
    members = served[FUSED] + served[GENERAL_STEP]
    if not members:
        return out
    lib = _lib.load()
    chunks, alphas, moments, log_alphas = {i: [] for i in members}, [1.0] * R, [None] * R, [0.0] * R
    for family in (FUSED, GENERAL_STEP):
        if replay is not None:
            entry = ob.replay_entries[family]
        else:
            entry = (ob.stats_entries if on_device else ob.entries)[family]
        for r0, ids, counts in windows(served[family], n_rows):
            made = [_eval_io(ob.io, ob.rows, ob.arrays, inputs[i], r0, r0 + k, trainers[i].act_dim,
                             outputs=rows or not on_device) for i, k in zip(ids, counts)]
            ios = (ob.io * len(ids))(*[m[0] for m in made])
            sts = (ob.stats * len(ids))() if on_device else None
            if replay is None:
                args = [ios] + ([sts] if on_device else [])
            else:
                idx = [np.ascontiguousarray(replay[i][1][r0:r0 + k]) for i, k in zip(ids, counts)]
                srcs = (_lib.SacEvalSrc * len(ids))(*[_lib.SacEvalSrc(replay[i][0]._h.value, x.ctypes.data)
                                                      for i, x in zip(ids, idx)])
                args = [srcs, ios, sts]
            _lib.check(getattr(lib, entry)(_handles(trainers, ids), len(ids), _ints(counts), *args), entry)
            for k, i in enumerate(ids):
                chunks[i].append(made[k][1])
                if not ob.td3:                                        # (the entropy coefficient of the call, and its log)
                    alphas[i] = float(ios[k].alpha)
                if on_device:
                    moments[i] = _merge_all(moments[i], _stats_moments(sts[k], ob.moments))
                    if not ob.td3:
                        log_alphas[i] = sts[k].log_alpha
    for i in members:
        t = trainers[i]
        t._settled()
        cols = ob.columns(chunks[i], alphas[i]) if rows or not on_device else None
        result = ob.device_stats(t, moments[i], alphas[i], log_alphas[i]) if on_device else ob.host_stats(t, cols)
        out[i] = (result, cols) if rows else result
    return out


def _evaluate_replay_of(ob, trainers, buffers, requests, rows, general, stats):
    """evaluate_replay_of / td3_evaluate_replay_of for objective ob: requests[i] = (indices, the draws)."""
    inputs = [None if q is None else (None,) * 5 + tuple(q[1:]) for q in requests]
    replay = [None if q is None else (b, q[0]) for b, q in zip(buffers, requests)]
    out = _evaluate_of(ob, trainers, inputs, rows, general, stats, replay=replay)
    if rows:
        for q, res in zip(requests, out):
            if q is not None:
                res[1]["indices"] = q[0]
    return out


def _evaluate_many(ob, caller, takes, trainers, batches, eps, rngs, rows, general, stats):
    """evaluate_many / td3_evaluate_many (`caller`) for objective ob."""
    check_stats(stats)
    check_general(general)
    trainers, batches, eps, rngs = _member_args(caller, takes, trainers, batches, eps, rngs)
    if ob.td3:
        _refuse_sac_members(caller, trainers, "evaluate_many")
    inputs = [None] * len(trainers)
    for i, (t, b) in enumerate(zip(trainers, batches)):
        if b is None or np.atleast_2d(b["observations"]).shape[0] == 0:
            continue
        if not ob.td3 and _is_td3(t):
            t.evaluate(b, eps=eps[i], rng=rngs[i], rows=rows)        # (TD3Trainer.evaluate refuses: the SAC objective)
        inputs[i] = getattr(t, ob.inputs)(b, eps[i], rngs[i])
    return _evaluate_of(ob, trainers, inputs, rows, general, stats)


def _evaluate_replay_many(ob, caller, takes, trainers, buffers, n, indices, eps, rngs, rows, general, stats):
    """evaluate_replay_many / td3_evaluate_replay_many (`caller`) for objective ob."""
    check_stats(stats)
    check_general(general)
    trainers = list(trainers)
    R = len(trainers)
    if (n is None) == (indices is None):
        raise ValueError(f"{caller} takes exactly one of n and indices")
    trainers, buffers, counts, indices, eps, rngs = _member_args(
        caller, takes, trainers, buffers, [n] * R if np.isscalar(n) else n, indices, eps, rngs)
    if ob.td3:
        _refuse_sac_members(caller, trainers, "evaluate_replay_many")
    requests = [None] * R
    for i, (t, b) in enumerate(zip(trainers, buffers)):
        if n is not None and not counts[i]:
            continue
        if n is None and (indices[i] is None or np.asarray(indices[i]).size == 0):
            continue
        if not ob.td3 and _is_td3(t):
            t.evaluate_replay(b, n=counts[i], indices=indices[i])     # (TD3Trainer.evaluate_replay refuses: the SAC objective)
        requests[i] = getattr(t, ob.request)(b, counts[i], indices[i], eps[i], rngs[i])
    return _evaluate_replay_of(ob, trainers, buffers, requests, rows, general, stats)


def evaluate_of(trainers, inputs, rows, general, stats, replay=None):
    """evaluate / evaluate_many behind their argument checks: inputs[i] = the member's arrays as SACTrainer._eval_inputs
    checked them, or None for a member that sits out (its result: None).  The host members first, in member order; then
    the fused family, then the general one, each in windows.
    replay (evaluate_replay_of): replay[i] = (buffer, indices) of a member with rows, whose inputs[i] then holds None for
    the five arrays the device takes from the replay storage (EVAL_REPLAY_ENTRIES); a host member evaluates the gathered
    batch."""
    return _evaluate_of(SAC_OBJECTIVE, trainers, inputs, rows, general, stats, replay)


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
    return _evaluate_many(SAC_OBJECTIVE, "evaluate_many", "batch (and eps pair, and rng)", trainers, batches, eps, rngs, rows,
                          general, stats)


def evaluate_replay_of(trainers, buffers, requests, rows, general, stats):
    """evaluate_replay / evaluate_replay_many behind their argument checks: requests[i] = (indices, eps, eps_next) as
    SACTrainer._replay_request checked them, or None for a member that sits out.  With rows the column dict of a member
    additionally holds "indices"."""
    return _evaluate_replay_of(SAC_OBJECTIVE, trainers, buffers, requests, rows, general, stats)


def evaluate_replay_many(trainers, buffers, n=None, indices=None, eps=None, rngs=None, rows=False, general="host",
                         stats="host"):
    """SACTrainer.evaluate_replay for many runs at once: result[i] = trainers[i].evaluate_replay(buffers[i], n or
    indices[i], eps[i], rngs[i]).  Exactly one of n and indices: n one row count for every member or one per member,
    indices one array of storage rows per member; an entry of None / 0 / no rows: the member sits out and gets None.
    eps / rngs: one entry per trainer or None.  Two members may share a buffer (rows are only read).  The members on
    the device are served by ONE call per 16 of them and 1024 rows per family (sac_evaluate_replay_many /
    sac_evaluate_replay_general_many; general and stats as for evaluate_many); the others run evaluate on their gathered
    batch inside the same call.  A member's result is bit for bit that of its own evaluate_replay; a TD3 member raises."""
    return _evaluate_replay_many(SAC_OBJECTIVE, "evaluate_replay_many", "buffer (and row count or indices, eps pair, rng)",
                                 trainers, buffers, n, indices, eps, rngs, rows, general, stats)


def td3_evaluate_of(trainers, inputs, rows, general="host", stats="host", replay=None):
    """evaluate_td3 / td3_evaluate_many behind their argument checks: inputs[i] = the member's arrays as
    TD3Trainer._td3_eval_inputs checked them, or None for a member that sits out (its result: None).  The host members
    first, in member order; then the fused family, then the general one (general="device"), each in windows of its
    entry of TD3_EVAL_ENTRIES (stats="device": of TD3_EVAL_STATS_ENTRIES): 16 members and 1024 rows per call.
    stats="device": a member on the device gets its statistics from the moment records of the same call
    (td3_moments_statistics; the windows of a member joined by merge_moments) -- no td3_eval_statistics, and with
    rows=False no column is copied back.  The host members get td3_eval_statistics under either value.
    replay (td3_evaluate_replay_of): replay[i] = (buffer, indices) of a member with rows, whose inputs[i] then holds None
    for the five arrays the device takes from the replay storage (TD3_EVAL_REPLAY_ENTRIES); a host member evaluates the
    gathered batch."""
    return _evaluate_of(TD3_OBJECTIVE, trainers, inputs, rows, general, stats, replay)


def td3_evaluate_replay_of(trainers, buffers, requests, rows, general, stats):
    """evaluate_td3_replay / td3_evaluate_replay_many behind their argument checks: requests[i] = (indices, eps) as
    TD3Trainer._td3_replay_request checked them, or None for a member that sits out.  With rows the column dict of a
    member additionally holds "indices"."""
    return _evaluate_replay_of(TD3_OBJECTIVE, trainers, buffers, requests, rows, general, stats)


def td3_evaluate_replay_many(trainers, buffers, n=None, indices=None, eps=None, rngs=None, rows=False, general="host",
                             stats="host"):
    """TD3Trainer.evaluate_td3_replay for many runs at once: result[i] = trainers[i].evaluate_td3_replay(buffers[i], n or
    indices[i], eps[i], rngs[i]).  Exactly one of n and indices: n one row count for every member or one per member,
    indices one array of storage rows per member; an entry of None / 0 / no rows: the member sits out and gets None.
    eps / rngs: one entry per trainer or None.  Two members may share a buffer (rows are only read).  The members on
    the device are served by ONE call per 16 of them and 1024 rows per family (td3_evaluate_replay_many /
    td3_evaluate_replay_general_many; general and stats as for td3_evaluate_many); the others run evaluate_td3 on their
    gathered batch inside the same call.  A member's result is bit for bit that of its own evaluate_td3_replay; a SAC
    member raises (evaluate_replay_many is the call for the SAC objective)."""
    return _evaluate_replay_many(TD3_OBJECTIVE, "td3_evaluate_replay_many", "buffer (and row count or indices, eps, rng)",
                                 trainers, buffers, n, indices, eps, rngs, rows, general, stats)


def td3_evaluate_many(trainers, batches, eps=None, rngs=None, rows=False, general="host", stats="host"):
    """TD3Trainer.evaluate_td3 for many runs at once: result[i] = trainers[i].evaluate_td3(batches[i], eps[i], rngs[i])
    (eps / rngs: one entry per trainer or None; batches[i] None or without rows: the member sits out and gets None).  The
    TD3 members with the fused kernels' shapes are served by ONE launch per 16 of them and 1024 rows (td3_evaluate_many:
    dims, hidden sizes and row counts mixed); the others -- the general step, trainers without a handle -- take their
    host path inside the same call.  A member's columns never depend on its neighbours: they are bit for bit those of
    its own evaluate_td3.  Results come back in member order; rows=True as for evaluate_td3.  A SAC member raises
    (evaluate_many is the call for the SAC objective).
    general="device": the TD3 members of the general step are evaluated on the device as well, by ONE
    td3_evaluate_general_many call per 16 of them and 1024 rows; their results are bit for bit those of their own
    evaluate_td3(general="device").
    stats="device" (evaluate_td3's `stats`): the members served by those two entries get their statistics reduced on the
    device in the same call (td3_evaluate_stats_many / td3_evaluate_general_stats_many: one k_eval_moments_td3 launch in
    front of the call's wait) -- no td3_eval_statistics for them, and with rows=False no column is copied back.  A
    member's records are byte for byte those of its own evaluate_td3(stats="device").  The members on the host path get
    td3_eval_statistics under either value."""
    return _evaluate_many(TD3_OBJECTIVE, "td3_evaluate_many", "batch (and eps, and rng)", trainers, batches, eps, rngs, rows,
                          general, stats)


# ---- acting sessions ----------------------------------------------------------------------------------------------------
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
        _lib.check(getattr(lib, entry + "_create")(C.byref(self.a), _handles(trainers, ids), n,
                                                   _ints([max_rows[i] for i in ids])), entry + "_create")

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
        self.general = check_general(general)
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
        self._td3 = [_is_td3(t) for t in self.trainers]
        # each member's route, fixed here: a session per 16 of a family (the general one under general_sessions), ONE
        # general call per tick and 16 members (_calls: general="device" without sessions), or its own policy_act (_host)
        routes = [route(t, general) for t in self.trainers]
        general_step = [i for i in range(R) if routes[i] == GENERAL_STEP]
        self._session_ids = {FUSED: [i for i in range(R) if routes[i] == FUSED],
                             GENERAL_STEP: general_step if self.general_sessions else []}
        self._calls = [] if self.general_sessions else general_step
        self._host = [i for i in range(R) if routes[i] == HOST]
        self.obs, self.eps, self.act = [None] * R, [None] * R, _ActRows(self._act, [None] * R)
        for i in self._calls + self._host:
            t, m = self.trainers[i], self.max_rows[i]
            self.obs[i], self.eps[i] = np.zeros((m, t.obs_dim), np.float64), np.zeros((m, t.act_dim), np.float32)
            self.act[i] = np.zeros((m, t.act_dim), np.float32)
        self._sessions, self._closed = [], False
        self._open()

    def _open(self):
        for family in (FUSED, GENERAL_STEP):
            ids = self._session_ids[family]
            for c in range(0, len(ids), MAX_MEMBERS):
                s = _ActorSession(self._lib, ids[c:c + MAX_MEMBERS], self.trainers, self.max_rows, SESSION_ENTRIES[family])
                self._sessions.append(s)
                for k, i in enumerate(s.ids):
                    t = self.trainers[i]
                    self.obs[i], self.eps[i], self.act[i] = s.arrays(k, self.max_rows[i], t.obs_dim, t.act_dim)

    def _reopen(self):
        """A member's handle was replaced: new sessions on the handles of now, the staged rows carried over."""
        members = self._session_ids[FUSED] + self._session_ids[GENERAL_STEP]
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
        if not (self._calls or self._host):                   # (every member has a session)
            return
        eps = {i: None if det[i] or self._td3[i] else self.eps[i][:n_rows[i]] for i in self._calls + self._host}
        obs = {i: np.ascontiguousarray(self.obs[i][:n_rows[i]].astype(np.float32)) for i in self._calls}
        act_calls(self._lib, ACT_ENTRIES[GENERAL_STEP], self.trainers, self._calls, n_rows, obs, det, eps, self.act)
        for i in self._host:
            if n_rows[i]:
                self.act[i][:n_rows[i]] = self.trainers[i].policy_act(self.obs[i][:n_rows[i]], det[i], eps[i])

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
