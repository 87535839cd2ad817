"""TD3Trainer with rlkit's constructor signature over the C ABI (td3_trainer_create + the shared sac_* entry points).

Reference assembly: /root/reference/util/rlkit_utils.py:107-135 (TanhMlpPolicy x2, GaussianStrategy,
PolicyWrappedWithExplorationStrategy, TD3Trainer(policy=, qf1=, qf2=, target_qf1=, target_qf2=, target_policy=,
**trainer_kwargs)); kwargs: /root/reference/scripts/train.py:38-47."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np

from . import _lib, infer
from ._lib import TD3_DIAG_NAMES, TD3_NET_IDS, Td3Config
from .sac import SACTrainer, _hidden_layers, _q_forward


class TD3Trainer(SACTrainer):
    NETS = TD3_NET_IDS
    TRAINED = ("policy", "qf1", "qf2")

    def __init__(self, policy=None, qf1=None, qf2=None, target_qf1=None, target_qf2=None, target_policy=None,
                 target_policy_noise=0.2, target_policy_noise_clip=0.5, discount=0.99, reward_scale=1.0,
                 policy_learning_rate=1e-3, qf_learning_rate=1e-3, policy_and_target_update_period=2, tau=0.005,
                 qf_criterion=None, optimizer_class=None, batch_size=None, noise_seed=None, device=0):
        assert optimizer_class is None and qf_criterion is None, "only Adam / MSELoss (rlkit's defaults) are implemented"
        self.target_policy = target_policy
        self.target_policy_noise, self.target_policy_noise_clip = float(target_policy_noise), float(target_policy_noise_clip)
        self.policy_and_target_update_period, self.tau = int(policy_and_target_update_period), float(tau)
        self.policy_learning_rate, self.qf_learning_rate = float(policy_learning_rate), float(qf_learning_rate)
        super().__init__(env=None, policy=policy, qf1=qf1, qf2=qf2, target_qf1=target_qf1, target_qf2=target_qf2,
                         discount=discount, reward_scale=reward_scale, policy_lr=policy_learning_rate,
                         qf_lr=qf_learning_rate, soft_target_tau=tau, target_update_period=1,
                         use_automatic_entropy_tuning=False, target_entropy=0.0, batch_size=batch_size,
                         noise_seed=noise_seed, device=device)

    def _new_handle(self, batch):
        hp, hq = self._hidden("policy"), self._hidden("qf1")
        cfg = Td3Config(self.obs_dim, self.act_dim, 256, batch, self.discount, self.reward_scale,
                        self.policy_learning_rate, self.qf_learning_rate, self.tau, self.target_policy_noise,
                        self.target_policy_noise_clip, self.policy_and_target_update_period, self.noise_seed,
                        self.device, 0, (C.c_int32 * 2)(0, 0), (C.c_int32 * 2)(0, 0))
        h = C.c_void_p()
        _lib.check(self._lib.td3_trainer_create_mlp(C.byref(h), C.byref(cfg), (C.c_int32 * len(hp))(*hp), len(hp),
                                                    (C.c_int32 * len(hq))(*hq), len(hq)), "td3_trainer_create_mlp")
        return h

    def _create(self, batch):
        if self._hidden("target_policy") != self._hidden("policy"):
            raise RuntimeError("policy and target_policy must share their hidden_sizes (rlkit_utils.py:108-117 builds them so)")
        super()._create(batch)

    @property
    def networks(self):
        return [self.policy, self.qf1, self.qf2, self.target_qf1, self.target_qf2, self.target_policy]

    def train(self, np_batch, eps=None):
        """eps: the (B, A) N(0,1) draw of the target-policy smoothing noise (None: device stream)."""
        return super().train(np_batch, eps=None if eps is None else (None, eps))

    def _record(self, diag):
        if self._need_to_update_eval_statistics:
            self._need_to_update_eval_statistics = False
            for i, name in enumerate(TD3_DIAG_NAMES):
                if name != "Actor Loss":
                    self.eval_statistics[name] = float(diag[i])

    def evaluate(self, batch, eps=None, rng=None, rows=False, general="host", stats="host"):
        raise NotImplementedError("TD3Trainer.evaluate: evaluate computes the SAC objective (entropy-regularised targets of "
                                  "a tanh-Gaussian policy); TD3's objective -- a deterministic policy with target "
                                  "smoothing -- is not implemented")

    def evaluate_replay(self, buffer, n=None, indices=None, eps=None, rng=None, rows=False, general="host", stats="host"):
        raise NotImplementedError("TD3Trainer.evaluate_replay: evaluate computes the SAC objective (entropy-regularised "
                                  "targets of a tanh-Gaussian policy); TD3's objective -- a deterministic policy with "
                                  "target smoothing -- is not implemented")

    # ---- the TD3 objectives on held-out transitions ------------------------------------------
    def _td3_eval_inputs(self, batch, eps, rng):
        """evaluate_td3's arguments, checked before any library call: float32 obs, act, rew, term, next_obs, eps."""
        obs, act, rew, term, nobs = self._eval_batch("evaluate_td3", batch)
        if eps is None:
            eps = self._eval_stream(rng).standard_normal(act.shape)
        eps = _lib.f32(np.atleast_2d(eps))
        if eps.shape != act.shape:
            raise ValueError(f"evaluate_td3: eps {eps.shape} for actions {act.shape}")
        return obs, act, rew, term, nobs, eps

    _POLICY_HEADS = 1                # (_host_net) the two policies are TanhMlpPolicy: one head of act_dim units

    def _evaluate_td3_host(self, arrs):
        """The host path of evaluate_td3: the nets' current weights (sac_sync, sac_get_params; the holders' own arrays
        while the trainer has no handle yet), a float32 NumPy forward and the device path's smoothing and y expressions."""
        obs, act, rew, term, nobs, eps = arrs
        if self._h is not None:
            _lib.check(self._lib.sac_sync(self._h), "sac_sync")
            self._settled()
        nets = {name: self._host_net(name) for name in self.NETS}

        def q(name, s, a):
            return _q_forward(nets[name], np.concatenate([s, a], axis=1))

        def pi(name, s):
            layers = nets[name]
            return np.tanh(_hidden_layers(s, layers[:-1]) @ layers[-1][0].T + layers[-1][1])

        with np.errstate(all="ignore"):
            a_pi, a_target = pi("policy", obs), pi("target_policy", nobs)
            a_smooth = infer.td3_smooth(a_target, eps, self.target_policy_noise, self.target_policy_noise_clip)
            tq1, tq2 = q("target_qf1", nobs, a_smooth), q("target_qf2", nobs, a_smooth)
            cols = dict(q1=q("qf1", obs, act), q2=q("qf2", obs, act), q_pi=q("qf1", obs, a_pi), tq1=tq1, tq2=tq2,
                        y=infer.td3_eval_target(rew, term, tq1, tq2, self.reward_scale, self.discount))
        out = dict(rows=np.stack([_lib.f32(cols[k]) for k in _lib.TD3_EVAL_ROWS]), a_pi=_lib.f32(a_pi),
                   a_target=_lib.f32(a_target), a_smooth=_lib.f32(a_smooth))
        return infer._eval_columns([out], _lib.TD3_EVAL_ROWS, _lib.TD3_EVAL_ARRAYS)

    def evaluate_td3(self, batch, eps=None, rng=None, rows=False, general="host", stats="host"):
        """The TD3 objectives of this run on `batch` WITHOUT a gradient step: `batch` is the dict train() takes
        (observations, actions, rewards, terminals, next_observations; any n >= 1), typically transitions the run has not
        trained on -- an epoch's evaluation paths.  From the LIVE weights: on the device (td3_evaluate: k_eval_td3, one
        launch per 1024 rows, no parameter copy); a trainer of the general step, which that entry refuses, and a
        trainer without a handle take the host path -- sac_sync, sac_get_params, a float32 NumPy forward.  Nothing the
        step reads is written either way, and the trainer's own statistics (get_diagnostics, the step counters) are left
        alone.
        general="device": a trainer of the general step is evaluated on the device as well (td3_evaluate_general:
        k_eval_layer_td3 and k_eval_layer, one launch per layer depth and 1024 rows, on the general step's own weights);
        its Q columns are bit for bit q_values(general="device")'s and a_pi policy_act_general's.  For the fused kernels'
        shapes and for a trainer without a handle the keyword changes nothing.
        eps: the (n, A) N(0,1) draw of the target smoothing; None: drawn as standard_normal((n, A)) from `rng`, or from a
        RandomState private to the trainer (seeded from noise_seed) when that is None too -- np.random is never touched.
        Returns an OrderedDict with get_diagnostics()' keys plus TD Error 1 / TD Error 2 Mean / Std / Max / Min (q - y,
        signed): infer.td3_eval_statistics of the per-row columns.  rows=True: (stats, columns), columns a dict of the
        float32 per-row arrays q1, q2, q_pi, tq1, tq2, y (n,) and a_pi, a_target, a_smooth (n, A):
        q_pi = Q1(s, a_pi), a_pi the policy's action on s; a_target the TARGET policy's action on s',
        a_smooth = a_target + clip(eps * target_policy_noise, +-target_policy_noise_clip), the targets tq1 / tq2 on
        (s', a_smooth), y = reward_scale r + (1 - d) discount min(tq1, tq2).
        stats (one of infer.STATS) decides where the statistics of a trainer that is evaluated on the device are reduced:
        "host", the default, copies the columns out and runs td3_eval_statistics; "device" reduces them on the device as
        well (td3_evaluate_stats_many / td3_evaluate_general_stats_many: k_eval_moments_td3 behind the evaluation's
        kernels, in front of the same wait) and builds the same keys from the moment records (td3_moments_statistics) --
        no td3_eval_statistics, and with rows=False no column leaves the staging.  The values agree with "host" up to the
        rounding of a float64 sum in another order; Max and Min are equal.  A trainer on the host path gets
        td3_eval_statistics under either value."""
        infer.check_stats(stats)
        infer.check_general(general)
        return infer.td3_evaluate_of([self], [self._td3_eval_inputs(batch, eps, rng)], rows, general, stats)[0]

    def _td3_replay_request(self, buffer, n, indices, eps, rng):
        """evaluate_td3_replay's arguments, checked before any library call: (indices int64 (k,), eps float32 (k, A)).
        Exactly one of n and indices; with n the indices are rng.randint(0, size, n), drawn IN FRONT of the single
        standard_normal((k, A)) from the same stream (rng None: evaluate_td3's private one)."""
        return self._replay_request(buffer, n, indices, eps, rng, caller="evaluate_td3_replay", draws=1)

    def evaluate_td3_replay(self, buffer, n=None, indices=None, eps=None, rng=None, rows=False, general="host",
                            stats="host"):
        """evaluate_td3 on rows of `buffer` (an EnvReplayBuffer of this run's dims) IN PLACE: the TD3 objectives at the
        current parameters on the data the run trains on -- the figure validation/QF1 Loss stands next to.  Exactly one
        of n and indices: `indices` are STORAGE rows (0 <= index < buffer size, any count, repeats allowed), `n` draws
        them as rng.randint(0, size, n) in front of the single standard_normal((k, A)) from the same `rng` (None:
        evaluate_td3's private stream; np.random is never touched).  eps, rng, rows, general and stats are evaluate_td3's;
        the result is what evaluate_td3(buffer.gather(indices), eps=the same draw, ...) returns, bit for bit, and with
        rows=True the column dict additionally holds "indices".
        On the device td3_evaluate_replay_many / td3_evaluate_replay_general_many copy the rows with a kernel from the
        replay storage into the evaluation's staging (k_eval_rows, one launch per 1024 rows in front of the evaluation's
        kernels), ordered behind pending add_* copies by an event: no synchronised D2H copy, no NumPy dict, no conversion
        and no memcpy into the staging.  The buffer is only read: its generator, np.random, its read-ahead and loop
        speculation stay as they are, and training continues bit for bit as if the call had not happened.  A trainer
        that evaluate_td3 sends to the host path (no handle; the general step under general="host"), and a buffer
        without device storage, run evaluate_td3(buffer.gather(indices) as a batch, ...)."""
        infer.check_stats(stats)
        infer.check_general(general)
        request = self._td3_replay_request(buffer, n, indices, eps, rng)
        return infer.td3_evaluate_replay_of([self], [buffer], [request], rows, general, stats)[0]

    def get_snapshot(self):
        snap = super().get_snapshot()
        snap["target_policy"] = self.target_policy
        snap["trained_policy"] = self.policy            # rlkit TD3Trainer.get_snapshot key
        return snap
