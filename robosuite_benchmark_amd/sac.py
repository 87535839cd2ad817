"""SACTrainer over libsac_hip.so (mirror of rlkit.torch.sac.sac.SACTrainer).

Reference call sites: /root/reference/util/rlkit_utils.py:98-106 (constructor kwargs =
variant['trainer_kwargs'], scripts/train.py:29-37), /root/reference/util/rlkit_custom.py:238
(``train(np_batch)``), :258 (``get_diagnostics``), :63,:70 (``get_snapshot``), :306-312
(``networks``), :291 (``reward_scale``).  Step semantics: SURVEY.md Appendix A."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np

from . import _lib, infer
from ._lib import DIAG_NAMES, NET_IDS, SacConfig
from .infer import (STATS, eval_moments, eval_statistics, eval_target, merge_moments,  # noqa: F401  (their home is infer)
                    moments_statistics)
from .networks import process_seed


def _hidden_layers(h, layers):
    """The hidden layers of the host forwards, float32: relu(h W^T + b) per (W, b)."""
    for w, b in layers:
        h = h @ w.T + b
        h = np.where(h < 0, np.float32(0), h)
    return h


def _q_forward(layers, x):
    """Q(x) of one net's [(W, b)] on the rows x = [obs, act], float32 (n,)."""
    h = _hidden_layers(x, layers[:-1])
    return (h @ layers[-1][0].T + layers[-1][1])[:, 0]


class SACTrainer:
    def __init__(self, env=None, policy=None, qf1=None, qf2=None, target_qf1=None, target_qf2=None,
                 discount=0.99, reward_scale=1.0, policy_lr=1e-3, qf_lr=1e-3, optimizer_class=None,
                 soft_target_tau=1e-2, target_update_period=1, plotter=None, render_eval_paths=False,
                 use_automatic_entropy_tuning=True, target_entropy=None, batch_size=None, noise_seed=None,
                 device=0):
        assert optimizer_class is None, "only Adam (rlkit's default) is implemented"
        self.env = env
        self.policy, self.qf1, self.qf2 = policy, qf1, qf2
        self.target_qf1, self.target_qf2 = target_qf1, target_qf2
        self.discount, self.reward_scale = float(discount), float(reward_scale)
        self.policy_lr, self.qf_lr = float(policy_lr), float(qf_lr)
        self.soft_target_tau, self.target_update_period = float(soft_target_tau), int(target_update_period)
        self.use_automatic_entropy_tuning = bool(use_automatic_entropy_tuning)
        self.obs_dim, self.act_dim = policy.obs_dim, policy.action_dim
        self.target_entropy = float(-self.act_dim if target_entropy is None else target_entropy)
        # rsample noise of the step: rlkit draws it from the generator torch.manual_seed(args.seed) seeded
        # (/root/reference/scripts/train.py:113); here a device counter-based stream keyed by that same process seed
        # unless the caller names one -- two runs with different seeds see different noise, as in the reference
        self.noise_seed = (process_seed() if noise_seed is None else int(noise_seed)) & 0xFFFFFFFFFFFFFFFF
        self.device = int(device)
        self.eval_statistics = OrderedDict()
        self._need_to_update_eval_statistics = True
        self._num_train_steps = 0
        self._lib = _lib.load()
        self._h, self._batch = None, None
        self._handle_gen = 0                     # handles made so far (an acting session is bound to ONE of them)
        self._host_policy_stale = False
        self._saved_state = None
        for name in self.NETS:                   # (a holder finds its trainer: acting path, pickling)
            getattr(self, name)._trainer = self
        if batch_size is not None:
            self._create(int(batch_size))

    # ---- handle management -----------------------------------------------------------------
    NETS = NET_IDS                           # name -> C net id (TD3Trainer adds target_policy)

    # The replay buffers of device batches this trainer has stepped on WITHOUT waiting (train() returned None): the
    # library keeps those steps on record by buffer and slot until it has seen them applied, and re-runs them from their
    # slots should a fused step have given up -- at the next call that settles the trainer, which may be a state read long
    # after the caller dropped its buffer (a DeviceBatch is gone as soon as train() returns).  The references keep such a
    # buffer alive until then; every call that settles drops them (_settled).
    _stepped_buffers = ()

    def _settled(self):
        """The library has just settled this trainer (a step that returned diagnostics, train_loop, a state read or write,
        sac_sync): no step is on record for any buffer."""
        self._stepped_buffers = ()

    def _new_handle(self, batch):
        hp, hq = self._hidden("policy"), self._hidden("qf1")
        cfg = SacConfig(self.obs_dim, self.act_dim, 256, batch, self.discount, self.reward_scale, self.policy_lr,
                        self.qf_lr, self.soft_target_tau, self.target_update_period,
                        int(self.use_automatic_entropy_tuning), self.target_entropy, self.noise_seed, self.device, 0,
                        (C.c_int32 * 2)(0, 0), (C.c_int32 * 2)(0, 0))
        h = C.c_void_p()
        _lib.check(self._lib.sac_trainer_create_mlp(C.byref(h), C.byref(cfg), (C.c_int32 * len(hp))(*hp), len(hp),
                                                    (C.c_int32 * len(hq))(*hq), len(hq)), "sac_trainer_create_mlp")
        return h

    MAX_HIDDEN_LAYERS, MAX_HIDDEN_UNITS = 7, 4096

    def _hidden(self, net):
        """variant['policy_kwargs'|'qf_kwargs']['hidden_sizes'] of a network family (arguments.py:98,104).  Two layers of at
        most 256 units (every shipped variant.json: [256, 256]) run on the fused kernels -- narrower layers exactly, as
        zero rows / columns of the 256-wide ones; any other depth / width runs the library's general step."""
        hs = [int(h) for h in getattr(self, net).hidden_sizes]
        if not 1 <= len(hs) <= self.MAX_HIDDEN_LAYERS or not all(1 <= h <= self.MAX_HIDDEN_UNITS for h in hs):
            raise RuntimeError(f"hidden_sizes {hs} unsupported: 1..{self.MAX_HIDDEN_LAYERS} hidden layers of "
                               f"1..{self.MAX_HIDDEN_UNITS} units")
        return hs

    def _create(self, batch):
        if not all(self._hidden(n) == self._hidden("qf1") for n in ("qf2", "target_qf1", "target_qf2")):
            raise RuntimeError("the four Q networks must share their hidden_sizes (rlkit_utils.py:64-83 builds them so)")
        h = self._new_handle(batch)
        state = self._export_state() if self._h else self._saved_state
        self._saved_state = None
        self._destroy()
        self._h, self._batch = h, batch
        self._handle_gen = getattr(self, "_handle_gen", 0) + 1
        if state is None:
            for name in self.NETS:
                self._set_params(name, getattr(self, name).flat())
        else:
            self._import_state(state)

    def _destroy(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.sac_trainer_destroy(h)
        self._settled()                          # (the record went with the handle)

    def __del__(self):
        self._destroy()

    # A trainer can be pickled too (rlkit's snapshot never holds one, but callers copy / checkpoint whole algorithms):
    # the device state -- parameters, Adam moments, entropy coefficient, counters -- travels as host arrays and goes
    # back into a fresh handle on the first step after loading.
    def __getstate__(self):
        st = dict(self.__dict__)
        if self._h is not None:
            self.sync_networks_to_host()
            st["_saved_state"] = self._export_state()
        st["_h"], st["_lib"], st["_stepped_buffers"] = None, None, ()
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)
        self._lib = _lib.load()
        for name in self.NETS:
            getattr(self, name)._trainer = self

    def _set_params(self, name, flat):
        flat = _lib.f32(flat)
        _lib.check(self._lib.sac_set_params(self._h, self.NETS[name], _lib.ptr(flat), flat.size), "sac_set_params")
        self._settled()
        if name == "policy":
            self._host_policy_stale = True           # (the holder's arrays are refreshed at their next use)

    def _get_params(self, name):
        n = int(self._lib.sac_param_count(self._h, self.NETS[name]))
        out = np.empty(n, np.float32)
        _lib.check(self._lib.sac_get_params(self._h, self.NETS[name], _lib.ptr(out), n), "sac_get_params")
        self._settled()
        return out

    def _export_state(self):
        st = dict(params={k: self._get_params(k) for k in self.NETS}, opt={})
        for k in ("policy", "qf1", "qf2"):
            n = st["params"][k].size
            m, v = np.empty(n, np.float32), np.empty(n, np.float32)
            _lib.check(self._lib.sac_get_opt_state(self._h, NET_IDS[k], _lib.ptr(m), _lib.ptr(v), n),
                       "sac_get_opt_state")
            st["opt"][k] = (m, v)
        sc = np.zeros(6, np.float64)
        _lib.check(self._lib.sac_get_scalars(self._h, _lib.ptr(sc)), "sac_get_scalars")
        st["scalars"] = sc
        return st

    def _import_state(self, st):
        for k, v in st["params"].items():
            self._set_params(k, v)
        for k, (m, v) in st["opt"].items():
            _lib.check(self._lib.sac_set_opt_state(self._h, NET_IDS[k], _lib.ptr(_lib.f32(m)), _lib.ptr(_lib.f32(v)),
                                                   m.size), "sac_set_opt_state")
        sc = np.ascontiguousarray(st["scalars"], np.float64)
        _lib.check(self._lib.sac_set_scalars(self._h, _lib.ptr(sc)), "sac_set_scalars")
        self._settled()
        self._host_policy_stale = True           # the acting copy on the host is refreshed at its next use

    state_dict, load_state_dict = _export_state, _import_state

    # ---- rlkit Trainer interface -------------------------------------------------------------
    @property
    def networks(self):
        return [self.policy, self.qf1, self.qf2, self.target_qf1, self.target_qf2]

    def train(self, np_batch, eps=None):
        """TorchTrainer.train: np_to_pytorch_batch + train_from_torch (one gradient step).

        A batch that random_batch() left on the device (DeviceBatch, not read by anyone) is trained on where it
        is: no host copy and no synchronisation; like rlkit the call then returns None, and the step's
        diagnostics are fetched only when the epoch's statistics are due.  Host batches return the diagnostics."""
        self._num_train_steps += 1
        if eps is None and getattr(np_batch, "on_device", False) and np_batch._buffer._h is not None:
            B = np_batch._batch_size
            if self._h is None or B != self._batch:
                self._create(B)
            diag = np.empty(_lib.SAC_DIAG_N, np.float32) if self._need_to_update_eval_statistics else None
            _lib.check(self._lib.sac_step_device(self._h, np_batch._buffer._h, np_batch._token, _lib.ptr(diag)),
                       "sac_step_device")
            self._host_policy_stale = True
            if diag is not None:
                self._record(diag)
                self._settled()
            elif not any(b is np_batch._buffer for b in self._stepped_buffers):
                self._stepped_buffers += (np_batch._buffer,)
            return diag
        obs = _lib.f32(np_batch["observations"])
        B = obs.shape[0]
        if self._h is None or B != self._batch:
            self._create(B)
        act, nobs = _lib.f32(np_batch["actions"]), _lib.f32(np_batch["next_observations"])
        rew = _lib.f32(np.asarray(np_batch["rewards"]).reshape(B))
        term = _lib.f32(np.asarray(np_batch["terminals"]).reshape(B))
        e1 = e2 = None
        if eps is not None:
            e1, e2 = (None if e is None else _lib.f32(e) for e in eps)
        diag = np.empty(_lib.SAC_DIAG_N, np.float32)
        _lib.check(self._lib.sac_step(self._h, _lib.ptr(obs), _lib.ptr(act), _lib.ptr(rew), _lib.ptr(term),
                                      _lib.ptr(nobs), _lib.ptr(e1), _lib.ptr(e2), _lib.ptr(diag)), "sac_step")
        self._settled()
        self._host_policy_stale = True
        self._record(diag)
        return diag

    def train_loop(self, replay_buffer, n_steps, batch_size=None):
        """The fused hot loop of rlkit_custom.py:234-238 (n_steps x {random_batch; train})."""
        B = int(batch_size or self._batch)
        if self._h is None or B != self._batch:
            self._create(B)
        first, last = np.empty(_lib.SAC_DIAG_N, np.float32), np.empty(_lib.SAC_DIAG_N, np.float32)
        _lib.check(self._lib.sac_train_loop(self._h, replay_buffer._h, int(n_steps), _lib.ptr(first), _lib.ptr(last)),
                   "sac_train_loop")
        self._settled()
        self._num_train_steps += int(n_steps)
        self._host_policy_stale = True
        self._record(first)
        return first, last

    def profile_loop(self, replay_buffer, n_steps, batch_size=None):
        """Instrumented pass: per-kernel mean launch duration (ms) from HIP events."""
        B = int(batch_size or self._batch)
        if self._h is None or B != self._batch:
            self._create(B)
        ms = np.zeros(9, np.float32)
        _lib.check(self._lib.sac_profile_loop(self._h, replay_buffer._h, int(n_steps), _lib.ptr(ms)),
                   "sac_profile_loop")
        self._num_train_steps += int(n_steps)
        self._host_policy_stale = True
        names = ["k_mt_randint", "k_gather", "k_fwd_a", "k_fwd_b", "k_bwd", "reserved", "k_dw_adam",
                 "event_pair", "steps_wall"]
        mode = self.fused_mode()
        if mode == 1:                # the fused step: k_abc = launches A + B + C in one (the next two slots read 0)
            names[2], names[3], names[4] = "k_fwd_abc", "fused_b", "fused_c"
        elif mode == 2:              # column split 1: k_chain = launches A + B in one (the next slot reads 0)
            names[2], names[3] = "k_chain", "chain_b"
        elif mode == 4:              # ... with the backward blocks inside too (the next two slots read 0)
            names[2], names[3], names[4] = "k_chain_bwd", "chain_b", "chain_c"
        return OrderedDict(zip(names, [float(x) for x in ms]))

    def fused_mode(self):
        """0: four launches per step; 1: the fused step, k_abc + k_dw_adam; 2: k_chain + k_bwd + k_dw_adam (batch >= 1024);
        3: the general step (hidden_sizes beyond two layers of at most 256 units); 4: k_chain8 with the backward blocks inside
        + k_dw_adam (batch 1024, SAC_CHAIN_BWD=1)."""
        return int(self._lib.sac_trainer_step_kind(self._h)) if self._h is not None else 0

    def is_fused(self):
        return self.fused_mode() == 1

    def runs_general_step(self):
        """Does this trainer run the general step?  With a handle: what the library built; without one: hidden sizes other
        than two layers of at most 256 units (infer.general_step)."""
        return infer.general_step(self)

    def loop_timing_ms(self):
        v = [C.c_float() for _ in range(4)]
        _lib.check(self._lib.sac_last_loop_ms(self._h, *[C.byref(x) for x in v]), "sac_last_loop_ms")
        return dict(total=v[0].value, sample=v[1].value, gather=v[2].value, steps=v[3].value)

    def _record(self, diag):
        if self._need_to_update_eval_statistics:
            self._need_to_update_eval_statistics = False
            for i, name in enumerate(DIAG_NAMES):
                if name != "Actor Loss":          # not an rlkit column
                    self.eval_statistics[name] = float(diag[i])

    def get_diagnostics(self):
        return self.eval_statistics

    def end_epoch(self, epoch):
        self._need_to_update_eval_statistics = True

    def policy_act(self, obs, deterministic, eps):
        """policy.get_actions through the C ABI: sac_policy_act per observation row (rlkit_custom.py:437 acts on one
        observation at a time).  The library mirrors the policy D2H on the first call after a training block."""
        obs = _lib.f32(obs)
        n, A = obs.shape[0], self.act_dim
        out = np.empty((n, A), np.float32)
        e = None if eps is None else _lib.f32(eps)
        for i in range(n):
            _lib.check(self._lib.sac_policy_act(self._h, obs[i].ctypes.data_as(C.c_void_p), int(bool(deterministic)),
                                                None if e is None else e[i].ctypes.data_as(C.c_void_p),
                                                out[i].ctypes.data_as(C.c_void_p)), "sac_policy_act")
        if n:                                    # (the mirror behind a training block is a state read: it settles)
            self._settled()
        return out

    def policy_act_device(self, obs, deterministic, eps):
        """policy.get_actions on the DEVICE from the live weights (sac_policy_act_device): all rows of `obs` in one launch
        per 1024 rows, no mirror of the policy on the host.  Trainers of the general step are refused by the library: they
        act through policy_act."""
        return self._act_on_device(infer.FUSED, obs, deterministic, eps)

    def policy_act_general(self, obs, deterministic, eps):
        """policy.get_actions on the DEVICE for a trainer of the general step (sac_policy_act_general: k_act_layer, one
        launch per layer on the live weights): all rows of `obs` in one call per 1024 rows, no mirror of the policy on the
        host.  Trainers with the fused kernels' shapes are refused by the library: policy_act_device is their entry."""
        return self._act_on_device(infer.GENERAL_STEP, obs, deterministic, eps)

    def _act_on_device(self, family, obs, deterministic, eps):
        """policy_act_device / policy_act_general: this trainer alone through its family's entry of infer.ACT_ENTRIES."""
        obs = _lib.f32(obs)
        out = np.empty((obs.shape[0], self.act_dim), np.float32)
        infer.act_calls(self._lib, infer.ACT_ENTRIES[family], [self], [0], [obs.shape[0]], [obs], [deterministic],
                        [None if eps is None else _lib.f32(eps)], [out])
        return out

    def _q_inputs(self, obs, act, nets):
        """q_values' arguments, checked before any library call: (obs, act, mask, rows)."""
        mask, rows = _lib.q_net_mask(nets)
        obs, act = _lib.f32(np.atleast_2d(obs)), _lib.f32(np.atleast_2d(act))
        if obs.ndim != 2 or act.ndim != 2 or obs.shape[1] != self.obs_dim or act.shape[1] != self.act_dim:
            raise ValueError(f"q_values: observations {obs.shape} / actions {act.shape} do not fit dims "
                             f"({self.obs_dim}, {self.act_dim})")
        if obs.shape[0] != act.shape[0] or obs.shape[0] < 1:
            raise ValueError(f"q_values: {obs.shape[0]} observation rows and {act.shape[0]} action rows (one action per "
                             "observation, at least one row)")
        return obs, act, mask, rows

    def _q_values_host(self, obs, act, nets):
        """The host path of q_values: the nets' current weights (sac_sync, sac_get_params; the holders' own arrays while
        the trainer has no handle yet) and a float32 NumPy forward."""
        if self._h is not None:
            _lib.check(self._lib.sac_sync(self._h), "sac_sync")
            self._settled()
        x = np.concatenate([obs, act], axis=1)
        out = np.empty((len(nets), x.shape[0]), np.float32)
        for r, name in enumerate(nets):
            out[r] = _q_forward(self._host_net(name), x)
        return out

    def q_values(self, obs, act, nets=("qf1", "qf2"), general="host"):
        """Q_net(obs, act) of this run's critics from the LIVE weights: float32 (len(nets), n), one row per name in `nets`
        (of "qf1", "qf2", "target_qf1", "target_qf2") in the order given.  On the device (sac_q_values: k_qval, one launch
        per 1024 rows for all the nets asked for, no parameter copy); a trainer of the general step, which the library's
        entry refuses, takes the host path -- sac_sync, sac_get_params, a float32 NumPy forward.  Nothing the step reads
        is written either way.
        general (one of group.GENERAL) decides for a trainer of the general step only: "host", the default, keeps the host
        path; "device" evaluates on the device as well (sac_q_values_general: k_qval_layer, one launch per layer on the
        live weights, in calls of at most 1024 rows, no parameter copy).  A trainer with the fused kernels' shapes takes
        sac_q_values and a trainer without a handle the host path under either value."""
        infer.check_general(general)
        obs, act, mask, rows = self._q_inputs(obs, act, nets)
        names = [nets] if isinstance(nets, str) else list(nets)
        return infer.q_values_of([self], [obs], [act], [names], [mask], [rows], general)[0]

    # ---- per-unit statistics of the hidden layers ----------------------------------------------
    def _unit_names(self, nets):
        """unit_moments' net selection, checked: names of this trainer's nets, each once, at least one."""
        names = [nets] if isinstance(nets, str) else list(nets)
        if not names:
            raise ValueError("unit_moments needs at least one network")
        for name in names:
            if name not in self.NETS:
                raise ValueError(f"unknown network {name!r}: one of {tuple(self.NETS)}")
        if len(set(names)) != len(names):
            raise ValueError(f"a network is named twice in {tuple(names)}")
        return names

    def _unit_inputs(self, obs, act, nets):
        """unit_moments' arguments, checked before any library call: (obs, act); act None where no Q net is named."""
        names = self._unit_names(nets)
        obs = _lib.f32(np.atleast_2d(obs))
        if obs.ndim != 2 or obs.shape[1] != self.obs_dim or obs.shape[0] < 1:
            raise ValueError(f"unit_moments: observations {obs.shape} do not fit obs_dim {self.obs_dim} (at least one row)")
        if not any(name in _lib.UNIT_Q_NETS for name in names):
            return obs, None
        if act is None:
            raise ValueError(f"unit_moments: {tuple(names)} names a Q network and the actions are None")
        act = _lib.f32(np.atleast_2d(act))
        if act.shape != (obs.shape[0], self.act_dim):
            raise ValueError(f"unit_moments: actions {act.shape} for {obs.shape[0]} observation rows and act_dim {self.act_dim}")
        return obs, act

    def _host_hidden(self, name):
        """[(W, b)] of one net's HIDDEN layers from the current weights (sac_get_params, or the holder's arrays without a
        handle): the front of the flat vector, whatever output layer or head follows."""
        flat = self._get_params(name) if self._h is not None else _lib.f32(getattr(self, name).flat())
        k = self.obs_dim + (self.act_dim if name in _lib.UNIT_Q_NETS else 0)
        layers, off = [], 0
        for n_out in self._hidden(name):
            layers.append((flat[off:off + n_out * k].reshape(n_out, k), flat[off + n_out * k:off + n_out * k + n_out]))
            off, k = off + n_out * k + n_out, n_out
        return layers

    def _unit_moments_host(self, obs, act, nets, activations=False):
        """The host path of unit_moments: the nets' current weights (sac_sync, sac_get_params; the holders' own arrays
        while the trainer has no handle yet), the float32 NumPy forward layer by layer, infer.unit_moments_reference."""
        if self._h is not None:
            _lib.check(self._lib.sac_sync(self._h), "sac_sync")
            self._settled()
        out = OrderedDict()
        with np.errstate(all="ignore"):
            for name in nets:
                h = np.concatenate([obs, act], axis=1) if name in _lib.UNIT_Q_NETS else obs
                out[name] = []
                for layer in self._host_hidden(name):
                    h = _lib.f32(_hidden_layers(h, [layer]))
                    rec = infer.unit_moments_reference(h)
                    if activations:
                        rec["h"] = h
                    out[name].append(rec)
        return out

    def unit_moments(self, obs, act=None, nets=("policy", "qf1", "qf2"), activations=False, general="host"):
        """How much of each network is alive: per-unit records of the hidden layers' post-ReLU activations on the rows
        obs (n, O) / act (n, A; needed where a Q net is named) from the LIVE weights.  An OrderedDict net -> [record per
        hidden layer] for the names in `nets` (of "policy", "qf1", "qf2", "target_qf1", "target_qf2"; a TD3Trainer also
        "target_policy") in the order given; a record is a dict of count (n) and four float64 arrays of the layer's true
        width -- sum, sumsq, active (rows with h > 0), max -- as infer.unit_moments_reference defines them, plus h (n, N)
        float32 with activations=True.  infer.unit_statistics turns the result into dormant / dead / active fractions and
        the feature norm.  Nothing the step reads is written, and no generator is touched.
        Routing is q_values': a trainer with the fused kernels' shapes goes to the device under either `general`
        (sac_unit_moments: k_units keeps the two hidden layers of k_act / k_qval, k_unit_moments reduces them; calls of at
        most 1024 rows joined by infer.merge_unit_moments, no parameter copy).  A trainer of the general step takes the
        host path by default -- sac_sync, sac_get_params, a float32 NumPy forward, unit_moments_reference -- and under
        general="device" the device (sac_unit_moments_general: k_qval_layer per layer depth and k_unit_moments on its
        outputs).  A trainer without a handle takes the host path."""
        infer.check_general(general)
        names = self._unit_names(nets)
        obs, act = self._unit_inputs(obs, act, names)
        return infer.unit_moments_of([self], [obs], [act], [names], bool(activations), general)[0]

    # ---- per-tensor statistics of parameters, Adam moments and target gaps ----------------------
    def _param_names(self, nets):
        """param_moments' net selection, checked: None is every net of the trainer; else names, each once, at least one."""
        if nets is None:
            return list(self.NETS)
        names = [nets] if isinstance(nets, str) else list(nets)
        if not names:
            raise ValueError("param_moments needs at least one network")
        for name in names:
            if name not in self.NETS:
                raise ValueError(f"unknown network {name!r}: one of {tuple(self.NETS)}")
        if len(set(names)) != len(names):
            raise ValueError(f"a network is named twice in {tuple(names)}")
        return names

    def param_tensors(self, net):
        """[(name, shape)] of the tensors of `net` in the flat nn.Linear order of sac_get_params: fc0.weight, fc0.bias,
        ..., last_fc.weight, last_fc.bias (a SAC policy: last_fc_log_std.weight, last_fc_log_std.bias too) -- the rows of
        param_moments' arrays."""
        if net not in self.NETS:
            raise ValueError(f"unknown network {net!r}: one of {tuple(self.NETS)}")
        out = []
        for name, (w, b) in getattr(self, net).layers.items():
            out += [(name + ".weight", tuple(w.shape)), (name + ".bias", tuple(b.shape))]
        return out

    def _param_moments_host(self, names, opt=True, gap=True):
        """The host route of param_moments: the flat vectors (sac_get_params / sac_get_opt_state; without a handle the
        holders' arrays and the saved or fresh -- zero -- Adam moments), cut into tensors, infer.param_moments_reference."""
        def flat(name):
            return self._get_params(name) if self._h is not None else _lib.f32(getattr(self, name).flat())
        out = OrderedDict()
        for name in names:
            x, m, v, tg = flat(name), None, None, None
            if opt and name in infer.PARAM_TRAINED:
                if self._h is not None:
                    m, v = np.empty(x.size, np.float32), np.empty(x.size, np.float32)
                    _lib.check(self._lib.sac_get_opt_state(self._h, self.NETS[name], _lib.ptr(m), _lib.ptr(v), x.size),
                               "sac_get_opt_state")
                    self._settled()
                elif self._saved_state is not None:
                    m, v = (_lib.f32(a) for a in self._saved_state["opt"][name])
                else:
                    m, v = np.zeros(x.size, np.float32), np.zeros(x.size, np.float32)
            tname = infer.param_target(self, name) if gap else None
            if tname is not None:
                tg = flat(tname)
            rec, off = [], 0
            for _, shape in self.param_tensors(name):
                e = int(np.prod(shape))
                cut = slice(off, off + e)
                rec.append(infer.param_moments_reference(x[cut], None if m is None else m[cut], None if v is None else v[cut],
                                                         None if tg is None else tg[cut]))
                off += e
            out[name] = np.stack(rec)
        return out

    def param_moments(self, nets=None, opt=True, gap=True, route="device"):
        """The state the step kernels write, reduced per tensor where it lives: an OrderedDict net -> float64 array
        (n_tensors, 9) for the names in `nets` (None: every net of the trainer; a TD3Trainer has "target_policy" too), rows
        in param_tensors' order, columns _lib.PARAM_FIELDS: sum, sumsq, absmax, nonfinite over the parameters; m_sumsq,
        m_absmax, v_sum, v_max over Adam's moments (opt; 0.0 on target nets); gap_sumsq, sum (x - x_target)^2 (gap; qf1 /
        qf2 against their targets, a TD3 policy against the target policy, 0.0 elsewhere).  infer.param_statistics turns
        the result into weight norms, Adam figures, target gaps and a non-finite count.
        route="device": sac_param_moments -- ONE k_param_moments launch over every selected tensor, read in place, no
        parameter copy; both step families.  route="host", and a trainer without a handle: sac_get_params /
        sac_get_opt_state and infer.param_moments_reference -- the same bytes.  Nothing the step reads is written."""
        infer.check_route(route)
        names = self._param_names(nets)
        return infer.param_moments_of([self], [names], bool(opt), bool(gap), route)[0]

    # ---- recycling dormant hidden units ---------------------------------------------------------
    def _recycle_inputs(self, units, fresh, rng):
        """recycle_units' arguments, checked before any library call: (units, fresh) as infer.check_recycle_units and
        infer.check_recycle_fresh leave them; fresh None: rows drawn by infer.fresh_unit_rows from rng, which must then be
        given (np.random is never touched)."""
        units = infer.check_recycle_units(self, units)
        if fresh is None:
            if rng is None:
                raise ValueError("recycle_units needs fresh rows or a generator to draw them from")
            fresh = infer.fresh_unit_rows(self, units, rng)
        return units, infer.check_recycle_fresh(self, units, fresh)

    def _recycle_host(self, units, fresh, opt=True):
        """The host route of recycle_units: export, infer.recycle_reference, import -- ten full-state transfers.  Without
        a handle the state is the saved one, if any, and the holders' own arrays."""
        if self._h is not None:
            self._import_state(infer.recycle_reference(self._export_state(), self, units, fresh, opt))
            return
        st = self._saved_state
        if st is None:
            zeros = {k: np.zeros(getattr(self, k).flat().size, np.float32) for k in infer.PARAM_TRAINED}
            st = dict(params={k: _lib.f32(getattr(self, k).flat()) for k in self.NETS},
                      opt={k: (z, z.copy()) for k, z in zeros.items()}, scalars=np.zeros(6, np.float64))
        new = infer.recycle_reference(st, self, units, fresh, opt)
        if self._saved_state is not None:
            self._saved_state = new
        for k in units:
            getattr(self, k).load_flat(new["params"][k])

    def recycle_units(self, units, fresh=None, rng=None, opt=True, route="device"):
        """ReDo (Sokar et al. 2023) on the live state: every listed unit of a hidden layer of a trained net gets a fresh
        incoming row and bias, +0.0 on its outgoing column(s) and, with opt, +0.0 in Adam's m and v of every element
        written; where a fresh row crosses a zeroed column, zero wins.  units: a mapping net -> [unit list per hidden
        layer] over "policy", "qf1", "qf2" (strictly ascending lists, e.g. infer.dormant_units of a unit_moments result);
        fresh: net -> [(n, K_l + 1) float32 per hidden layer], or None: drawn by infer.fresh_unit_rows from rng.  Target
        nets are left alone -- the Polyak average carries the change over, and params/* Target Gap jumps for a while --
        as are scalars, counters, generators and buffers.
        route="device": sac_recycle_units -- two k_unit_recycle launches write the selected rows and columns in place, both
        weight copies and the moments where they live, no parameter copy; both step families.  route="host", and a trainer
        without a handle: export, infer.recycle_reference, import -- the same bytes.  Returns the per-net counts."""
        if route not in infer.RECYCLE_ROUTES:
            raise RuntimeError(f"route must be one of {infer.RECYCLE_ROUTES}, got {route!r}")
        units, fresh = self._recycle_inputs(units, fresh, rng)
        return infer.recycle_units_of([self], [units], [fresh], bool(opt), route)[0]

    def recycle_dormant(self, obs, act=None, nets=("policy", "qf1", "qf2"), tau=0.025, rng=None, general="host", opt=True):
        """unit_moments on the rows obs / act -> infer.dormant_units(tau) -> recycle_units with rows drawn from rng: the
        tau-dormant units of `nets` on those rows are recycled.  Returns the per-net counts."""
        if rng is None:
            raise ValueError("recycle_dormant needs a generator to draw the fresh rows from")
        units = infer.dormant_units(self.unit_moments(obs, act, nets=nets, general=general), tau)
        return self.recycle_units(units, rng=rng, opt=opt)

    # ---- whole-network reset and shrink-and-perturb --------------------------------------------
    def _shrink_perturb_host(self, a):
        """The host route of shrink_perturb (a: infer.PerturbArgs): export, the reference, import -- full-state transfers.
        Without a handle the state is the saved one, if any, and the holders' own arrays."""
        if self._h is not None:
            self._import_state(infer._shrink_perturb_state(self._export_state(), self, a))
            return
        st = self._saved_state
        if st is None:
            zeros = {k: np.zeros(getattr(self, k).flat().size, np.float32) for k in infer.PARAM_TRAINED}
            st = dict(params={k: _lib.f32(getattr(self, k).flat()) for k in self.NETS},
                      opt={k: (z, z.copy()) for k, z in zeros.items()}, scalars=np.zeros(6, np.float64))
        new = infer._shrink_perturb_state(st, self, a)
        if self._saved_state is not None:
            self._saved_state = new
        for k in self.NETS:
            getattr(self, k).load_flat(new["params"][k])

    def shrink_perturb(self, nets=None, shrink=0.8, perturb=0.2, seed=None, draw=0, opt=True, targets=False, init_w=None,
                       b_init=None, route="device"):
        """Shrink and perturb (Ash & Adams 2020) on the live state: every element x of the trained nets `nets` (None: all of
        policy, qf1, qf2) becomes shrink * x + perturb * f, each operation rounded to float32 once, f the element's fresh
        value -- what the constructors would have drawn (hidden weights uniform in +-1/sqrt(N_l), hidden biases b_init,
        heads uniform in +-init_w), from a Philox stream keyed by (seed, draw): seed None takes the trainer's noise seed,
        and a caller that wants new values passes a new draw.  A term whose factor is 0 is not formed: shrink=0 clears a
        NaN or Inf weight, shrink != 0 keeps it.  opt: Adam's m and v of every element written become +0.0; the step
        counts and bias corrections are NOT reset.  targets: the paired target (target_qf1 / target_qf2, a TD3 trainer's
        target_policy) receives the same bits; without it targets are left alone and params/* Target Gap jumps.  Scalars,
        counters, generators and buffers are untouched.
        route="device": sac_shrink_perturb -- ONE k_param_perturb launch draws and writes in place, both weight copies and
        the moments where they live, no parameter crosses the link; both step families.  route="host", and a trainer
        without a handle: export, infer.shrink_perturb_reference, import -- the same bytes.  Returns the nets written."""
        if route not in infer.RECYCLE_ROUTES:
            raise RuntimeError(f"route must be one of {infer.RECYCLE_ROUTES}, got {route!r}")
        a = infer.check_shrink_perturb(self, nets, shrink, perturb, seed, draw, opt, targets, init_w, b_init)
        return infer.shrink_perturb_of([self], [a], route)[0]

    def reset_networks(self, nets=None, seed=None, draw=0, alpha=False, route="device"):
        """Periodic reset (Nikishin et al. 2022): shrink_perturb(shrink=0, perturb=1, opt=True, targets=True) -- the trained
        nets `nets` and their targets take fresh values, Adam's moments +0.0; the replay buffer, the step counts and every
        counter stay.  alpha=True also puts log_alpha and its two Adam moments back to their initial values (0; alpha 1);
        a TD3 trainer has no entropy coefficient, and nothing is done for it there."""
        done = self.shrink_perturb(nets, 0.0, 1.0, seed, draw, True, True, route=route)
        if alpha and not infer._is_td3(self):
            if self._h is not None:
                sc = np.zeros(6, np.float64)
                _lib.check(self._lib.sac_get_scalars(self._h, _lib.ptr(sc)), "sac_get_scalars")
                sc[[0, 1, 2]], sc[5] = 0.0, 1.0
                _lib.check(self._lib.sac_set_scalars(self._h, _lib.ptr(sc)), "sac_set_scalars")
                self._settled()
            elif self._saved_state is not None:
                self._saved_state["scalars"][[0, 1, 2]] = 0.0
                self._saved_state["scalars"][5] = 1.0
        return done

    # ---- evaluation on held-out transitions --------------------------------------------------
    _evaluate_on_host = False      # private switch: the host path for a fused-shape trainer too (scripts/bench_evaluate.py
                                     # measures the two paths of ONE trainer against each other)
    _eval_rng = None                 # evaluate's private noise stream, made on first use

    def _eval_stream(self, rng):
        """rng, or for None the stream private to the trainer (seeded from noise_seed): np.random is never touched."""
        if rng is None:
            if self._eval_rng is None:
                self._eval_rng = np.random.RandomState(
                    [int(self.noise_seed & 0xFFFFFFFF), int(self.noise_seed >> 32), 0x4556414C])
            rng = self._eval_rng
        return rng

    def _eval_batch(self, caller, batch):
        """The batch of `caller` (evaluate, evaluate_td3), checked before any library call: float32 obs, act, rew, term,
        next_obs."""
        obs = _lib.f32(np.atleast_2d(batch["observations"]))
        n = obs.shape[0]
        act, nobs = _lib.f32(np.atleast_2d(batch["actions"])), _lib.f32(np.atleast_2d(batch["next_observations"]))
        if n < 1 or obs.shape != (n, self.obs_dim) or nobs.shape != obs.shape or act.shape != (n, self.act_dim):
            raise ValueError(f"{caller}: observations {obs.shape} / actions {act.shape} / next_observations {nobs.shape} "
                             f"do not fit dims ({self.obs_dim}, {self.act_dim}) (at least one row)")
        rew, term = (_lib.f32(np.asarray(batch[k]).reshape(-1)) for k in ("rewards", "terminals"))
        if rew.shape != (n,) or term.shape != (n,):
            raise ValueError(f"{caller}: {rew.size} rewards and {term.size} terminals for {n} rows")
        return obs, act, rew, term, nobs

    def _eval_inputs(self, batch, eps, rng):
        """evaluate's arguments, checked before any library call: float32 obs, act, rew, term, next_obs, eps, eps_next."""
        obs, act, rew, term, nobs = self._eval_batch("evaluate", batch)
        n = obs.shape[0]
        if eps is None:
            rng = self._eval_stream(rng)
            eps = (rng.standard_normal((n, self.act_dim)), rng.standard_normal((n, self.act_dim)))
        e1, e2 = (_lib.f32(np.atleast_2d(e)) for e in eps)
        if e1.shape != act.shape or e2.shape != act.shape:
            raise ValueError(f"evaluate: eps {e1.shape} / eps_next {e2.shape} for actions {act.shape}")
        return obs, act, rew, term, nobs, e1, e2

    _POLICY_HEADS = 2                # heads of act_dim units behind the policy's hidden layers: mean and log_std

    def _host_net(self, name):
        """[(W, b)] of one net from the current weights: sac_get_params, or the holder's arrays without a handle.  A
        policy's heads all read the last hidden layer; a Q net ends in one unit over cat(obs, act)."""
        flat = self._get_params(name) if self._h is not None else _lib.f32(getattr(self, name).flat())
        is_policy, hidden = name.endswith("policy"), self._hidden(name)
        heads = [self.act_dim] * self._POLICY_HEADS if is_policy else [1]
        k = self.obs_dim if is_policy else self.obs_dim + self.act_dim
        layers, off = [], 0
        for l, n_out in enumerate(hidden + heads):
            layers.append((flat[off:off + n_out * k].reshape(n_out, k), flat[off + n_out * k:off + n_out * k + n_out]))
            off += n_out * k + n_out
            if l < len(hidden):
                k = n_out
        assert off == flat.size
        return layers

    def _evaluate_host(self, arrs):
        """The host path of evaluate: the nets' current weights (sac_sync, sac_get_params; the holders' own arrays while
        the trainer has no handle yet), a float32 NumPy forward and the device path's y expression."""
        obs, act, rew, term, nobs, e1, e2 = arrs
        alpha = 1.0
        if self._h is not None:
            _lib.check(self._lib.sac_sync(self._h), "sac_sync")
            self._settled()
            if self.use_automatic_entropy_tuning:        # (as sac_evaluate: no alpha before the first step, exp(log_alpha))
                sc = self._scalars()
                alpha = float(sc[5]) if sc[5] > 0 else float(np.exp(np.float32(sc[0])))
        elif self.use_automatic_entropy_tuning and self._saved_state is not None:
            alpha = float(np.exp(np.float32(self._saved_state["scalars"][0])))
        nets = {name: self._host_net(name) for name in NET_IDS}
        f = np.float32

        def q(name, s, a):
            return _q_forward(nets[name], np.concatenate([s, a], axis=1))

        def pi(s, e):
            layers = nets["policy"]
            h = _hidden_layers(s, layers[:-2])
            mean = h @ layers[-2][0].T + layers[-2][1]
            ls = np.clip(h @ layers[-1][0].T + layers[-1][1], f(-20.0), f(2.0))
            std = np.exp(ls)
            z = mean + std * e
            a = np.tanh(z)
            dd = z - mean
            nlp = -(dd * dd) / (f(2.0) * (std * std)) - np.log(std) - f(0.91893853320467274178)
            lp = nlp - np.log(f(1.0) - a * a + f(1e-6))
            return a, mean, ls, lp.sum(axis=1, dtype=f)

        with np.errstate(all="ignore"):
            a_new, mu, log_std, log_pi = pi(obs, e1)
            a_next, _, _, log_pi_next = pi(nobs, e2)
            tq1, tq2 = q("target_qf1", nobs, a_next), q("target_qf2", nobs, a_next)
            cols = dict(q1=q("qf1", obs, act), q2=q("qf2", obs, act), q1_new=q("qf1", obs, a_new),
                        q2_new=q("qf2", obs, a_new), tq1=tq1, tq2=tq2, log_pi=log_pi, log_pi_next=log_pi_next,
                        y=eval_target(rew, term, tq1, tq2, log_pi_next, alpha, self.reward_scale, self.discount))
        out = dict(rows=np.stack([_lib.f32(cols[k]) for k in _lib.EVAL_ROWS]), mu=_lib.f32(mu), log_std=_lib.f32(log_std),
                   a_new=_lib.f32(a_new), a_next=_lib.f32(a_next))
        return infer._sac_eval_columns([out], alpha)

    def _scalars(self):
        sc = np.zeros(6, np.float64)
        _lib.check(self._lib.sac_get_scalars(self._h, _lib.ptr(sc)), "sac_get_scalars")
        self._settled()
        return sc

    def _eval_log_alpha(self):
        if self._h is not None:
            return float(self._scalars()[0])
        return float(self._saved_state["scalars"][0]) if self._saved_state is not None else 0.0

    def _eval_stats(self, cols):
        return eval_statistics(np.stack([cols[k] for k in _lib.EVAL_ROWS]), cols["mu"], cols["log_std"], cols["alpha"],
                               self._eval_log_alpha(), self.target_entropy, self.use_automatic_entropy_tuning)

    def evaluate(self, batch, eps=None, rng=None, rows=False, general="host", stats="host"):
        """The SAC objectives of this run on `batch` WITHOUT a gradient step: `batch` is the dict train() takes
        (observations, actions, rewards, terminals, next_observations; any n >= 1), typically transitions the run has not
        trained on -- an epoch's evaluation paths.  From the LIVE weights and the CURRENT entropy coefficient: on the
        device (sac_evaluate: k_eval, one launch per 1024 rows, no parameter copy); a trainer of the general step, which
        the library's entry refuses, and a trainer without a handle take the host path -- sac_sync, sac_get_params, a
        float32 NumPy forward.  Nothing the step reads is written either way, and the trainer's own statistics
        (get_diagnostics, the step counters) are left alone.
        eps: (eps, eps_next), the (n, A) N(0,1) draws of a_new and a_next; None: drawn as standard_normal((n, A)) twice
        from `rng`, or from a RandomState private to the trainer (seeded from noise_seed) when that is None too --
        np.random is never touched.
        Returns an OrderedDict with get_diagnostics()' keys plus TD Error 1 / TD Error 2 Mean / Std / Max / Min (q - y,
        signed): eval_statistics of the per-row columns.  The training step logs its values behind its own alpha update;
        these are one alpha step earlier.  rows=True: (stats, columns), columns a dict of the float32 per-row arrays q1,
        q2, q1_new, q2_new, tq1, tq2, log_pi, log_pi_next, y (n,), mu, log_std, a_new, a_next (n, A), and alpha.
        general (one of group.GENERAL) decides for a trainer of the general step only: "host", the default, keeps the host
        path; "device" evaluates on the device as well (sac_evaluate_general: k_eval_layer, one launch per layer on the
        live weights, in calls of at most 1024 rows, no parameter copy).  A trainer with the fused kernels' shapes takes
        sac_evaluate and a trainer without a handle the host path under either value.
        stats (one of sac.STATS) decides where the statistics of a trainer that is evaluated on the device are reduced:
        "host", the default, copies the columns out and runs eval_statistics; "device" reduces them on the device as well
        (sac_evaluate_stats_many / sac_evaluate_general_stats_many: k_eval_moments behind the evaluation's kernels, in
        front of the same wait) and builds the same keys from the moment records (moments_statistics) -- no
        eval_statistics, no sac_get_scalars, and with rows=False no column leaves the staging.  The values agree with
        "host" up to the rounding of a float64 sum in another order; Max, Min and Alpha are equal.  A trainer on the host
        path gets eval_statistics under either value."""
        infer.check_stats(stats)
        infer.check_general(general)
        return infer.evaluate_of([self], [self._eval_inputs(batch, eps, rng)], rows, general, stats)[0]

    def _replay_request(self, buffer, n, indices, eps, rng, caller="evaluate_replay", draws=2):
        """`caller`'s arguments, checked before any library call: (indices int64 (k,), then the `draws` float32 (k, A)
        arrays: eps and eps_next for evaluate_replay, the single eps of evaluate_td3_replay).  Exactly one of n and
        indices; with n the indices are rng.randint(0, size, n), drawn IN FRONT of the standard_normal((k, A)) draws from
        the same stream (rng None: evaluate's private one)."""
        if (n is None) == (indices is None):
            raise ValueError(f"{caller} takes exactly one of n and indices")
        size = int(buffer.num_steps_can_sample())
        if size < 1:
            raise RuntimeError(f"{caller}: the replay buffer is empty")
        if indices is None:
            if int(n) < 1:
                raise ValueError(f"{caller}: n = {n} (at least one row)")
            rng = self._eval_stream(rng)
            idx = np.ascontiguousarray(rng.randint(0, size, int(n)), dtype=np.int64)
        else:
            idx = np.ascontiguousarray(np.asarray(indices).reshape(-1), dtype=np.int64)
            if idx.size < 1:
                raise ValueError(f"{caller}: no indices (at least one row)")
            if int(idx.min()) < 0 or int(idx.max()) >= size:
                bad = idx[(idx < 0) | (idx >= size)][0]
                raise RuntimeError(f"{caller}: index {int(bad)} out of range [0, {size})")
        k, A = idx.size, self.act_dim
        if eps is None:
            rng = self._eval_stream(rng)
            eps = [rng.standard_normal((k, A)) for _ in range(draws)]
        elif draws == 1:
            eps = [eps]
        es = [_lib.f32(np.atleast_2d(e)) for e in eps]
        if len(es) != draws or any(e.shape != (k, A) for e in es):
            shapes = " / ".join(f"{name} {e.shape}" for name, e in zip(("eps", "eps_next"), es))
            raise ValueError(f"{caller}: {shapes} for {k} rows of {A} actions")
        return (idx, *es)

    def evaluate_replay(self, buffer, n=None, indices=None, eps=None, rng=None, rows=False, general="host", stats="host"):
        """evaluate on rows of `buffer` (an EnvReplayBuffer of this run's dims) IN PLACE: the SAC objectives at the
        current parameters on the data the run trains on -- the figure validation/QF1 Loss stands next to.  Exactly one
        of n and indices: `indices` are STORAGE rows (0 <= index < buffer size, any count, repeats allowed), `n` draws
        them as rng.randint(0, size, n) in front of the eps pair from the same `rng` (None: evaluate's private stream;
        np.random is never touched).  eps, rng, rows, general and stats are evaluate's; the result is what
        evaluate(buffer.gather(indices), eps=the same pair, ...) returns, bit for bit, and with rows=True the column dict
        additionally holds "indices".
        On the device sac_evaluate_replay_many / sac_evaluate_replay_general_many copy the rows with a kernel from the
        replay storage into the evaluation's staging (k_eval_rows, one launch per 1024 rows in front of the evaluation's
        kernels), ordered behind pending add_* copies by an event.  That staging is mapped pinned HOST memory, as for
        evaluate: the rows still cross the link, once out by the kernel's stores and once back by the evaluation's loads.
        What is saved is the host's part -- no synchronised D2H copy, no NumPy dict, no conversion and no memcpy into
        the staging.  The buffer is only read: its generator, np.random, its read-ahead and loop speculation stay as they
        are, and training continues bit for bit as if the call had not happened.  A trainer that evaluate sends to the
        host path (no handle; the general step under general="host"), and a buffer without device storage, run
        evaluate(buffer.gather(indices) as a batch, ...)."""
        infer.check_stats(stats)
        infer.check_general(general)
        request = self._replay_request(buffer, n, indices, eps, rng)
        return infer.evaluate_replay_of([self], [buffer], [request], rows, general, stats)[0]

    def refresh_host_policy(self):
        """Mirror the trained policy D2H once per training block (acting stays on the host)."""
        if self._h is not None and self._host_policy_stale:
            self.policy.load_flat(self._get_params("policy"))
            self._host_policy_stale = False

    def sync_holder_to_host(self, holder):
        """The trained weights of ONE network holder (whichever of this trainer's nets it is) into its host arrays."""
        for name in self.NETS:
            if getattr(self, name) is holder:
                holder.load_flat(self._get_params(name))
                if name == "policy":
                    self._host_policy_stale = False

    def sync_networks_to_host(self):
        for name in self.NETS:
            getattr(self, name).load_flat(self._get_params(name))
        self._host_policy_stale = False

    def get_snapshot(self):
        if self._h is not None:
            self.sync_networks_to_host()
        return dict(policy=self.policy, qf1=self.qf1, qf2=self.qf2, target_qf1=self.target_qf1,
                    target_qf2=self.target_qf2)

    def debug_fetch(self, name, n):
        out = np.empty(int(n), np.float32)
        got = self._lib.sac_debug_fetch(self._h, name.encode(), _lib.ptr(out), out.size)
        _lib.check(int(got), "sac_debug_fetch")
        return out[:got]

    def set_launch_number(self, seq):
        """Test hook (sac_debug_set_launch_number): this trainer as `seq` (modulo 2^32) completed fused launches leave it
        -- launch number, hand-off counters, tagged words.  Trained state is untouched; a trainer that does not run a
        fused step is refused."""
        if self._h is None:
            raise RuntimeError("set_launch_number: no device trainer")
        _lib.check(self._lib.sac_debug_set_launch_number(self._h, int(seq) & 0xFFFFFFFF), "sac_debug_set_launch_number")
