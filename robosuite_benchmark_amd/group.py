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
# (the inference names live in infer.py; they stay importable from here)
from .infer import (GENERAL, GENERAL_SESSIONS, MAX_MEMBERS, GroupActor, act_many, check_general,  # noqa: F401
                    evaluate_many, evaluate_replay_many, general_shape, merge_unit_moments, param_moments_many,
                    param_moments_reference, param_statistics, q_values_many, recycle_units_many, runs_general_step, shrink_perturb_many,
                    td3_eval_moments, td3_evaluate_many,
                    td3_evaluate_replay_many, td3_moments_statistics, unit_moments_many, unit_moments_reference, unit_statistics)
from .sac import SACTrainer
from .td3 import TD3Trainer


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
        check_general(general)
        if nets_list is None:
            nets_list = [("qf1", "qf2")] * len(self.trainers)
        return q_values_many(self.trainers, obs_list, act_list, nets_list, general=general)

    def unit_moments_many(self, obs_list, act_list, nets_list=None, activations=False, general="host"):
        """unit_moments_many over the group's members (nets_list None: policy, qf1 and qf2 of every member; activations
        and general as there)."""
        check_general(general)
        if nets_list is None:
            nets_list = [("policy", "qf1", "qf2")] * len(self.trainers)
        return unit_moments_many(self.trainers, obs_list, act_list, nets_list, activations=activations, general=general)

    def param_moments_many(self, nets_list=None, opt=True, gap=True, route="device"):
        """param_moments_many over the group's members (nets_list None: every net of every member; opt, gap and route as
        there): one sac_param_moments_many call per 16 members."""
        return param_moments_many(self.trainers, nets_list, opt=opt, gap=gap, route=route)

    def recycle_units_many(self, units_list, fresh_list=None, rngs=None, opt=True, route="device"):
        """recycle_units_many over the group's members (units_list[i] None: member i sits out; fresh_list, rngs, opt and
        route as there): one sac_recycle_units_many call per 16 members."""
        return recycle_units_many(self.trainers, units_list, fresh_list=fresh_list, rngs=rngs, opt=opt, route=route)

    def shrink_perturb_many(self, nets_list=None, shrink=0.8, perturb=0.2, seeds=None, draws=0, opt=True, targets=False,
                            init_w=None, b_init=None, route="device"):
        """shrink_perturb_many over the group's members (nets_list[i] None: member i sits out; the other arguments shared
        or one per member, as there): one sac_shrink_perturb_many call per 16 members."""
        return shrink_perturb_many(self.trainers, nets_list, shrink=shrink, perturb=perturb, seeds=seeds, draws=draws,
                                   opt=opt, targets=targets, init_w=init_w, b_init=b_init, route=route)

    def evaluate_many(self, batches, eps=None, rngs=None, rows=False, general="host", stats="host"):
        """evaluate_many over the group's members (general and stats as there)."""
        return evaluate_many(self.trainers, batches, eps=eps, rngs=rngs, rows=rows, general=general, stats=stats)

    def evaluate_replay_many(self, replay_buffers, n=None, indices=None, eps=None, rngs=None, rows=False, general="host",
                             stats="host"):
        """evaluate_replay_many over the group's members on their replay buffers -- the ones train_loop takes, one per
        member (n, indices, general and stats as there)."""
        return evaluate_replay_many(self.trainers, replay_buffers, n=n, indices=indices, eps=eps, rngs=rngs, rows=rows,
                                    general=general, stats=stats)

    def td3_evaluate_many(self, batches, eps=None, rngs=None, rows=False, general="host", stats="host"):
        """td3_evaluate_many over the group's members: the TD3 objectives (a SAC group raises through the member check
        there; general and stats as there)."""
        return td3_evaluate_many(self.trainers, batches, eps=eps, rngs=rngs, rows=rows, general=general, stats=stats)

    def td3_evaluate_replay_many(self, replay_buffers, n=None, indices=None, eps=None, rngs=None, rows=False, general="host",
                                 stats="host"):
        """td3_evaluate_replay_many over the group's members on their replay buffers -- the ones train_loop takes, one per
        member (n, indices, general and stats as there; a SAC group raises through the member check there)."""
        return td3_evaluate_replay_many(self.trainers, replay_buffers, n=n, indices=indices, eps=eps, rngs=rngs, rows=rows,
                                        general=general, stats=stats)


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
                net = "policy" if general_shape(t._hidden("policy")) else "qf1"
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
