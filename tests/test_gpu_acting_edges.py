"""GPU: acting at its edges and behind every path that moves the policy -- both implementations, k_act (csrc/sac_act.h,
through sac_policy_act_device / sac_policy_act_many) and the host forward sac_policy_act (csrc/sac_trainer.hip), which
reads a mirror of the policy guarded by mirror_valid.

Reference: oracle.sac_step_torch.PolicyNet.  Bound (helpers.check_act, the constants of
test_gpu_device_acting.check_against_oracle): max|K - f64| <= max(2e-5, 8 x max|fp32 oracle - f64|), and atol 2e-5 against
the fp32 oracle, which holds wherever 8 x max|fp32 oracle - f64| <= 2e-5: in every case of the matrix
(tests/test_acting_edges_host.py asserts it; check_act asserts it again for the call at hand).  Exact facts are exact: saturated actions, clamped == on-the-bound, zero rows, grouped == solo, untouched rows.
The edge states and what they claim: tests/edge_states.py (build_acting), checked on the CPU by
tests/test_acting_edges_host.py."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

from robosuite_benchmark_amd import (ArchSACTrainerGroup, MakeDeterministic, MixedSACTrainerGroup,
                                     MlpSACTrainerGroup, SACTrainerGroup, TD3TrainerGroup, _lib)
from robosuite_benchmark_amd.group import runs_general_step
from tests import edge_states as ES
from tests.helpers import (ACT_ERRORS, act_c, act_reference, check_act, draws, filled_buffer, flat_of, full_state, is_td3,
                           layers_from_flat, make_pair, make_td3_pair, pair_of_hip, plain_buffer, synth_transitions)

pytestmark = pytest.mark.gpu
case_id = ES.acting_case_id


def trainer(algo, O, A, hidden, seed=5):
    """A fresh trainer of one shape (the edge matrix puts each edge's policy in through sac_set_params)."""
    return (make_pair if algo == "sac" else make_td3_pair)(O, A, 32, seed=seed, hidden=tuple(hidden))[1]


def policy_layers(t):
    """The policy the device holds NOW, as the oracle's layer list (any depth)."""
    dims = [t.obs_dim] + t._hidden("policy")
    shapes = [(dims[i + 1], dims[i]) for i in range(len(dims) - 1)] + [(t.act_dim, dims[-1])] * (1 if is_td3(t) else 2)
    return layers_from_flat(t.state_dict()["params"]["policy"], shapes)


def impls(t):
    """{name: act(obs, deterministic, eps)}: the host forward row by row, and k_act unless t runs the general step."""
    out = {"host": lambda o, d, e: t.policy_act(o, d, None if (d or is_td3(t)) else e)}
    if not runs_general_step(t):
        out["device"] = lambda o, d, e: act_c(t, o, d, None if (d or is_td3(t)) else e)
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- a. the edge matrix -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ES.acting_cases(), ids=case_id)
def test_edge_matrix(case):
    edge, algo, O, A, hidden = case
    t = trainer(algo, O, A, hidden)
    general = runs_general_step(t)
    assert general == (tuple(hidden) in ES.ACT_GENERAL_HIDDEN)
    for n in ES.ACT_ROWS:
        layers, obs, eps, meta = ES.build_acting(edge, algo, O, A, hidden, n, seed=11)
        twin_out = {}
        if edge == "clamp":                          # the twin whose clamped columns sit exactly on the bound
            t._set_params("policy", flat_of(ES.clamp_twin(layers, meta)))
            twin_out = {(k, det): f(obs, det, eps) for k, f in impls(t).items() for det in (True, False)}
        t._set_params("policy", flat_of(layers))
        for name, act in impls(t).items():
            for det in (True, False):
                got = act(obs, det, eps)
                where = (case_id(case), n, name, "deterministic" if det else "stochastic")
                check_act(t, got, layers, obs, det, eps, where, tag=(edge, name))
                if edge == "clamp":
                    assert same_bits(got, twin_out[(name, det)]), where
                elif edge == "tanh":
                    for c, sign in meta["saturated_cols"].items():
                        assert np.all(got[:, c] == sign), (where, c)
                    if meta["stoch_col"] is not None and not det:
                        assert np.all(got[meta["stoch_rows"], meta["stoch_col"]] == meta["stoch_signs"]), where
                elif edge == "relu":
                    zr = meta["zero_rows"]
                    assert same_bits(got[zr], np.repeat(got[:1], zr.size, 0)), where
    if general:                                      # the device entry refuses it, in C and in Python
        out = np.full((n, A), 3.0, np.float32)
        rc = _lib.load().sac_policy_act_device(t._h, n, _lib.ptr(obs), 1, None, _lib.ptr(out))
        assert rc < 0 and "general step" in _lib.last_error() and np.all(out == 3.0)
        with pytest.raises(RuntimeError, match="sac_policy_act is the acting path"):
            t.policy_act_device(obs, True, None)


# ---- b. extents -------------------------------------------------------------------------------------------------------
def many(ts, n_rows, obs, det, eps, outs):
    R = len(ts)
    vp = lambda arrs: (C.c_void_p * R)(*[None if a is None else a.ctypes.data for a in arrs])  # noqa: E731
    rc = _lib.load().sac_policy_act_many((C.c_void_p * R)(*[t._h.value for t in ts]), R, (C.c_int32 * R)(*n_rows), vp(obs),
                                         (C.c_int32 * R)(*[int(d) for d in det]), vp(eps), vp(outs))
    _lib.check(rc, "sac_policy_act_many")


def test_sixteen_members_of_1024_rows_and_staging_growth_in_both_orders():
    dims = [(496, 16), (42, 7), (89, 14), (379, 6), (64, 4), (1, 1), (17, 9), (42, 16)]
    hiddens = [(256, 256), (256, 256), (128, 64), (100, 50)]
    ts = []
    for i in range(16):
        O, A = dims[i % len(dims)]
        if i % 3 == 2:
            ts.append(trainer("td3", O, A, (256, 256), seed=40 + i))
        else:
            ts.append(trainer("sac", O, A, hiddens[i % 4], seed=40 + i))
    assert any(is_td3(t) for t in ts) and (ts[0].obs_dim, ts[0].act_dim) == (496, 16)
    rs = np.random.RandomState(16)
    o1, e1 = draws(rs, 1, 496, 16)
    first = act_c(ts[0], o1, False, e1)              # a 1-row call: the staging buffer at its smallest
    obs, eps, det, outs = [], [], [], []
    for i, t in enumerate(ts):
        o, e = draws(rs, 1024, t.obs_dim, t.act_dim)
        obs.append(o); det.append(i % 2 == 0)
        eps.append(None if (det[-1] or is_td3(t)) else e)
        outs.append(np.full((1024, t.act_dim), -5.0, np.float32))
    many(ts, [1024] * 16, obs, det, eps, outs)       # ... grown to 16 x 1024 rows in one call
    again = act_c(ts[0], o1, False, e1)              # ... and a 1-row call in the large buffer
    assert same_bits(first, again)
    check_act(ts[0], again, policy_layers(ts[0]), o1, False, e1, "1 row after 16 x 1024", tag=("extents", "device"))
    for i, t in enumerate(ts):
        assert same_bits(outs[i], act_c(t, obs[i], det[i], eps[i])), i
        check_act(t, outs[i], policy_layers(t), obs[i], det[i], eps[i], ("16 x 1024", i), tag=("extents", "device"))


@pytest.mark.parametrize("rows", [(0, 9, 33), (0, 0, 1024)], ids=["first sits out", "only the last acts"])
def test_trainer_0_sits_out_with_steps_in_flight(rows):
    """trainers[0] owns the staging buffer and the stream of the call; here it has no rows, and device-batch steps nobody
    has synchronised.  The others act as in their solo calls, and trainers[0] ends as a twin that was never in an
    acting call."""
    O, A, B = 42, 7, 64
    (_, t0), (_, twin) = make_pair(O, A, B, seed=12, noise_seed=5), make_pair(O, A, B, seed=12, noise_seed=5)
    b0, bt = filled_buffer(2000, O, A, 8), filled_buffer(2000, O, A, 8)
    a, b = trainer("sac", 46, 7, (256, 256)), trainer("td3", 89, 14, (256, 256))
    rs = np.random.RandomState(3)
    obs = [None] + [draws(rs, n, t.obs_dim, t.act_dim)[0] if n else None for n, t in zip(rows[1:], (a, b))]
    eps = [None, draws(rs, rows[1], 46, 7)[1] if rows[1] else None, None]
    outs = [np.full((3, A), -5.0, np.float32)] + [np.full((max(n, 3), t.act_dim), -5.0, np.float32) for n, t in zip(rows[1:], (a, b))]
    for block in range(3):
        for x, buf in ((t0, b0), (twin, bt)):
            for _ in range(7):                       # (the first step of all publishes diagnostics; none after it waits)
                x.train(buf.random_batch(B))
        many([t0, a, b], rows, obs, [0, 0, 0], eps, outs)
        assert np.all(outs[0] == -5.0)
        for i, t in ((1, a), (2, b)):
            if rows[i]:
                assert same_bits(outs[i][:rows[i]], act_c(t, obs[i], False, eps[i])), (block, i)
                check_act(t, outs[i][:rows[i]], policy_layers(t), obs[i], False, eps[i], ("trainer 0 sits out", i),
                          tag=("extents", "device"))
            else:
                assert np.all(outs[i] == -5.0)
    for x, y in zip(full_state(t0, b0), full_state(twin, bt)):
        assert np.array_equal(x, y)


# ---- c. non-finite rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,O,A,hidden", [("sac", 42, 7, (256, 256)), ("sac", 17, 7, (100, 50)), ("td3", 42, 7, (256, 256))])
def test_a_non_finite_row_stays_in_its_row(algo, O, A, hidden):
    """NaN / +Inf / -Inf in one observation element: ordinary IEEE arithmetic.  Every other row of the call is bit for
    bit the clean call's; the poisoned row is what torch's fp32 forward makes of it -- NaN where that is NaN, and
    within the bound where it is not (+-1 included)."""
    t = trainer(algo, O, A, hidden)
    layers = ES.build_acting("relu", algo, O, A, hidden, 1, seed=11)[0]        # its own policy: zero and dead units too
    t._set_params("policy", flat_of(layers))
    n = 33
    obs, eps = draws(np.random.RandomState(7), n, O, A)
    for name, act in impls(t).items():
        for det in (True, False):
            clean = act(obs, det, eps)
            for row, k in ((0, 0), (16, O // 2), (32, O - 1), (5, O - 1)):
                for bad in (np.nan, np.inf, -np.inf):
                    o = obs.copy()
                    o[row, k] = bad
                    got = act(o, det, eps)
                    where = (name, det, row, k, bad)
                    others = np.arange(n) != row
                    assert same_bits(got[others], clean[others]), where
                    want = act_reference(layers, is_td3(t), o[row:row + 1], det, eps[row:row + 1], torch.float32)[0]
                    assert np.any(np.isnan(want)) or np.all(np.abs(want) == 1.0), where          # (the case is one)
                    assert np.array_equal(np.isnan(got[row]), np.isnan(want)), (where, got[row], want)
                    ok = ~np.isnan(want)
                    assert np.allclose(got[row][ok], want[ok], atol=2e-5), (where, got[row], want)


# ---- d. acting follows the weights behind every path ------------------------------------------------------------------
class Watch:
    """One trainer, fixed observations and eps; acts through every entry that has a copy of the policy to go stale."""

    def __init__(self, t, seed=6):
        self.t = t
        self.obs, self.eps = draws(np.random.RandomState(seed), 40, t.obs_dim, t.act_dim)

    def act(self):
        return {(k, det): f(self.obs, det, self.eps) for k, f in impls(self.t).items() for det in (True, False)}

    def moved(self, before, where):
        t, obs, eps = self.t, self.obs, self.eps
        assert t._host_policy_stale, (where, "_host_policy_stale")     # (Python's flag; reading it syncs nothing)
        # act FIRST: after device-batch steps nobody has waited for, each entry has to drain and settle them itself
        # (the device entry through sac_sync, the host entry through its mirror); the reference weights are read after
        now, bounds = self.act(), {}
        layers = policy_layers(t)                    # state_dict()["params"]["policy"] as it is now
        for (name, det), got in now.items():
            bounds[(name, det)] = check_act(t, got, layers, obs, det, eps, (where, name, det), tag=("paths", name))
            assert not np.array_equal(got, before[(name, det)]), (where, name, det)
        for det in (True, False):
            if ("device", det) in now:
                gap = float(np.max(np.abs(now[("host", det)] - now[("device", det)])))
                assert gap <= bounds[("host", det)] + bounds[("device", det)], (where, det, gap)
        # the Python holders: through the trainer while it is bound, from their own arrays once unpickled
        td3 = is_td3(t)
        t.policy._noise = np.random.RandomState(9)
        a, info = t.policy.get_action(obs[0])
        e9 = None if td3 else np.random.RandomState(9).standard_normal((1, t.act_dim)).astype(np.float32)
        assert info == {}
        check_act(t, a[None], layers, obs[:1], td3, e9, (where, "policy.get_action"), tag=("paths", "holder"))
        if not td3:
            a, _ = MakeDeterministic(t.policy).get_action(obs[0])
            check_act(t, a[None], layers, obs[:1], True, None, (where, "MakeDeterministic"), tag=("paths", "holder"))
        snap = pickle.loads(pickle.dumps(t.policy if td3 else MakeDeterministic(t.policy)))      # evaluation/policy
        assert (snap if td3 else snap.stochastic_policy)._trainer is None
        a = np.stack([snap.get_action(o)[0] for o in obs[:8]])
        check_act(t, a, layers, obs[:8], True, None, (where, "unpickled snapshot"), tag=("paths", "holder"))
        t._host_policy_stale = True                  # (pickling brought the holder up; ask for it once more)
        t.refresh_host_policy()
        assert not t._host_policy_stale and np.array_equal(t.policy.flat(), t.state_dict()["params"]["policy"]), where


def host_batch(O, A, B, seed):
    obs, act, rew, term, nobs = synth_transitions(B, O, A, seed=seed)
    return dict(observations=obs, actions=act, rewards=rew, terminals=term.astype(np.float32), next_observations=nobs)


def solo(seed=9, B=64, hidden=(256, 256), td3=False, O=42, A=7):
    t = (make_td3_pair if td3 else make_pair)(O, A, B, seed=seed, hidden=hidden)[1]
    t.train(host_batch(O, A, B, seed))               # (the epoch's diagnostics are in: later steps fetch none)
    return t, filled_buffer(2000, O, A, seed)


def identities(ts):
    from robosuite_benchmark_amd import group_checkpoint as gc
    v = dict(policy_kwargs=dict(hidden_sizes=[256, 256]), qf_kwargs=dict(hidden_sizes=[256, 256]))
    return [gc.member_identity(f"m{i}", i, v, t) for i, t in enumerate(ts)]


# each path: (the trainers to watch, run) -- run() changes their weights; it may return the trainers that replace them
def path_train_host(tmp):
    t, _ = solo()
    return [t], lambda: [t.train(host_batch(42, 7, 64, 100 + i)) for i in range(3)] and None


def path_train_device(tmp):
    t, buf = solo()

    def run():
        for _ in range(20):
            assert t.train(buf.random_batch(64)) is None            # on the device, nothing synchronised
    return [t], run


def path_train_loop(tmp):
    t, buf = solo()
    return [t], lambda: t.train_loop(buf, 30, batch_size=64) and None


def path_profile_loop(tmp):
    t, buf = solo()
    return [t], lambda: t.profile_loop(buf, 20, batch_size=64) and None


def path_set_params(tmp):
    from oracle.sac_step_torch import init_sac_params
    t, _ = solo()
    return [t], lambda: t._set_params("policy", flat_of(init_sac_params(42, 7, seed=77)["policy"]))


def path_load_state_dict(tmp):
    (t, _), (u, ubuf) = solo(), solo(seed=10)
    u.train_loop(ubuf, 10, batch_size=64)
    return [t], lambda: t.load_state_dict(u.state_dict())


def path_pickle(tmp):
    t, buf = solo()

    def run():
        t.train_loop(buf, 10, batch_size=64)
        t2 = pickle.loads(pickle.dumps(t))
        assert t2._h is None
        t2.train(host_batch(42, 7, 64, 5))           # the state goes back into a fresh handle on the first step
        return [t2]
    return [t], run


def path_checkpoint(tmp):
    from robosuite_benchmark_amd.checkpoint import load_checkpoint, save_checkpoint
    t, buf = solo()
    save_checkpoint(str(tmp / "ck"), t, buf)
    t.train_loop(buf, 20, batch_size=64)             # (the weights the mirrors are warm with are not the saved ones)
    return [t], lambda: load_checkpoint(str(tmp / "ck"), t, buf) and None


def path_group_checkpoint(tmp):
    from robosuite_benchmark_amd import group_checkpoint as gc
    (t, tb), (u, ub) = solo(), solo(seed=10)
    ck = gc.GroupCheckpoint(str(tmp / "gck"), 512)
    ck.save([t, u], [tb, ub], identities([t, u]), [dict(epoch=0), dict(epoch=0)])
    SACTrainerGroup([t, u]).train_loop([tb, ub], 20, batch_size=64)
    return [t, u], lambda: ck.load([t, u], [tb, ub], identities([t, u])) and None


def group_path(kind, members):
    def make(tmp):
        pairs = [solo(**kw) for kw in members]
        ts, bufs = [p[0] for p in pairs], [p[1] for p in pairs]
        return ts, lambda: kind(ts).train_loop(bufs, 25) and None
    return make


def path_stall(tmp):
    """A train_loop in which fused launch 3 gives up (the test hook of test_gpu_fused_step.py, used as there, once): the
    call re-runs the lost steps on the four-launch step."""
    fused, _ = pair_of_hip(42, 7, 256, seed=4, noise_seed=9, SAC_FUSED_TEST_STALL=3)
    buf = plain_buffer(4000, 42, 7, 8)
    buf.seed(31)

    def run():
        assert fused.is_fused()
        fused.train_loop(buf, 10, batch_size=256)
        assert not fused.is_fused() and fused.state_dict()["scalars"][4] == 10
    return [fused], run


PATHS = {
    "train on a host batch": path_train_host, "train on device batches": path_train_device, "train_loop": path_train_loop,
    "profile_loop": path_profile_loop, "_set_params": path_set_params, "load_state_dict": path_load_state_dict,
    "pickle round trip": path_pickle, "checkpoint restore": path_checkpoint, "group checkpoint restore": path_group_checkpoint,
    "SACTrainerGroup": group_path(SACTrainerGroup, [dict(seed=30), dict(seed=31), dict(seed=32)]),
    "TD3TrainerGroup": group_path(TD3TrainerGroup, [dict(seed=33, td3=True), dict(seed=34, td3=True)]),
    "MixedSACTrainerGroup": group_path(MixedSACTrainerGroup, [dict(seed=35, B=48), dict(seed=36, B=100, O=46)]),
    "MlpSACTrainerGroup": group_path(MlpSACTrainerGroup, [dict(seed=37, hidden=(512, 512)), dict(seed=38, hidden=(512, 512), O=46)]),
    "ArchSACTrainerGroup": group_path(ArchSACTrainerGroup, [dict(seed=39), dict(seed=40, hidden=(128, 64)),
                                                            dict(seed=41, hidden=(512, 512)), dict(seed=42, hidden=(64, 96, 48))]),
    "train_loop with a fused step that gives up": path_stall,
}


@pytest.mark.parametrize("path", list(PATHS))
def test_acting_follows_the_weights_behind(path, tmp_path):
    ts, run = PATHS[path](tmp_path)
    ws = [Watch(t) for t in ts]
    before = [w.act() for w in ws]                   # both mirrors warm, the holder's copy in step
    for w in ws:
        w.t.sync_networks_to_host()
    out = run()
    for w, t in zip(ws, out or ts):
        w.t = t
    for i, (w, b) in enumerate(zip(ws, before)):
        w.moved(b, (path, i))


def test_zz_report_the_largest_errors():
    """(prints, per edge and implementation, the largest |K - f64| seen by this file's checks and the fp32 oracle's own
    |fp32 - f64| of that call: run with -s)"""
    for tag in sorted(ACT_ERRORS):
        e, e32, where = ACT_ERRORS[tag]
        print(f"acting errors {tag}: largest |K - f64| {e:.3g} (|fp32 oracle - f64| {e32:.3g}) at {where}")
