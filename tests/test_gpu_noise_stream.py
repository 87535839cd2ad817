"""GPU: the device N(0,1) stream (philox_normal, the noise of every step not given eps by its caller) against its NumPy
restatement oracle/noise_stream.py.

(a) With the policy's heads at zero (and policy_lr = 0, so they stay there) mean = 0 and std = 1: z IS the draw on s
    (stream 0) and a_next = tanh(the draw on s', stream 1); TD3 with the target policy's head at zero has
    a_next = clamp(0.2 draw, +-0.5) (stream 1).  Every row and action, every path, steps 0..2 and 2^32 + 3, two seeds
    that differ only in their high word.
(b) The same after the production drivers: train_loop, stepwise device batches, trainer groups, checkpoint resume.
(c) The whole step on device noise against the float64 oracle (tests/helpers.py check_step_f64) fed the reference draw.

Tolerance of a draw: |z - ref| <= 1e-6 max(1, |ref|) -- the kernel's logf / sqrtf / cosf and float32 product against
float64 are a few float32 ulp; a counter or word mix-up is O(1)."""
import numpy as np
import pytest

from oracle import noise_stream as ns
from robosuite_benchmark_amd import _lib
from tests.helpers import check_step_f64, make_pair, make_td3_pair, synth_transitions
from tests.test_gpu_step_edges import ENV, PATHS

pytestmark = pytest.mark.gpu

DRAW_TOL, ACT_TOL = 1e-6, 2e-6
SIGMA, CLIP = 0.2, 0.5
SEED_LO, SEED_HI = 5, (1 << 32) | 5
BIG_STEP = 2 ** 32 + 3
ULP = {}                     # label -> largest float32 ulp distance of a device draw from the rounded reference


def _env(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _batch(B, O, A, seed=21):
    obs, act, rew, term, nobs = synth_transitions(B, O, A, seed=seed, term_frac=0.1)
    return dict(observations=obs, actions=act, rewards=rew, terminals=term.astype(np.float32), next_observations=nobs)


def _zero_head_sac(O, A, B, hidden, noise_seed, **kw):
    """A SAC trainer whose policy heads (last_fc, last_fc_log_std) are 0 and stay 0: z = eps, a = tanh(eps)."""
    from oracle.sac_step_torch import init_sac_params
    nets = init_sac_params(O, A, hidden=hidden, seed=3)
    for i in (-2, -1):
        w, b = nets["policy"][i]
        nets["policy"][i] = (np.zeros_like(w), np.zeros_like(b))
    return make_pair(O, A, B, nets=nets, hidden=hidden, policy_lr=0.0, noise_seed=noise_seed, **kw)[1]


def _zero_head_td3(O, A, B, hidden, noise_seed):
    """A TD3 trainer whose target policy's last_fc is 0 and stays 0 (so is the online policy's, which the Polyak average
    of every second step mixes in, and its learning rate): a_next = tanh(0) + clamp(sigma eps, +-clip)."""
    from oracle.td3_step_torch import init_td3_params
    nets = init_td3_params(O, A, hidden=hidden, seed=3)
    for name in ("policy", "target_policy"):
        w, b = nets[name][-1]
        nets[name][-1] = (np.zeros_like(w), np.zeros_like(b))
    return make_td3_pair(O, A, B, nets=nets, hidden=hidden, noise_seed=noise_seed, target_policy_noise=SIGMA,
                         target_policy_noise_clip=CLIP, policy_learning_rate=0.0)[1]


def _set_step(t, step):
    sc = np.zeros(6, np.float64)
    _lib.check(t._lib.sac_get_scalars(t._h, _lib.ptr(sc)), "sac_get_scalars")
    sc[4] = float(step)
    assert int(sc[4]) == step
    _lib.check(t._lib.sac_set_scalars(t._h, _lib.ptr(sc)), "sac_set_scalars")


def _step_count(t):
    sc = np.zeros(6, np.float64)
    _lib.check(t._lib.sac_get_scalars(t._h, _lib.ptr(sc)), "sac_get_scalars")
    return int(sc[4])


def _ulp(got, ref, label):
    want = np.asarray(ref, np.float64).astype(np.float32)
    d = np.abs(np.asarray(got, np.float32).view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    same = np.sign(got) == np.sign(want)
    u = int(np.max(np.where(same, d, 0))) if d.size else 0
    if u > ULP.get(label, -1):
        ULP[label] = u
    return u


def check_draw(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    i = np.unravel_index(int(np.argmax(err)), err.shape)
    assert err[i] <= DRAW_TOL, f"{what}: draw {i} is {got[i]!r}, the reference {ref[i]!r} (error {err[i]:.3g})"


def check_tanh(got, ref, what):
    got, want = np.asarray(got, np.float64), np.tanh(np.asarray(ref, np.float64))
    err = np.abs(got - want)
    i = np.unravel_index(int(np.argmax(err)), err.shape)
    assert err[i] <= ACT_TOL, f"{what}: tanh of draw {i} is {got[i]!r}, the reference {want[i]!r}"


def check_sac_step(t, seed, step, B, A, general, what):
    """The draws of the step that just ran at `step` (stream 0 through z -- a_new on the general step, which keeps no z --
    and stream 1 through a_next); returns the device's (B, A) views of the two streams."""
    r0, r1 = ns.draws(seed, step, B, A, 0), ns.draws(seed, step, B, A, 1)
    a2 = t.debug_fetch("a_next", B * A).reshape(B, A)
    check_tanh(a2, r1, f"{what} a_next (stream 1)")
    if general:
        s0 = t.debug_fetch("a_new", B * A).reshape(B, A)
        check_tanh(s0, r0, f"{what} a_new (stream 0)")
    else:
        s0 = t.debug_fetch("z", B * A).reshape(B, A)
        check_draw(s0, r0, f"{what} z (stream 0)")
        _ulp(s0, r0, what.split(" step")[0])
    return s0, a2


def check_td3_step(t, seed, step, B, A, what):
    ref = ns.draws(seed, step, B, A, 1)
    a2 = t.debug_fetch("a_next", B * A).reshape(B, A).astype(np.float64)
    want = np.clip(ref * SIGMA, -CLIP, CLIP)
    tol = SIGMA * DRAW_TOL * np.maximum(1.0, np.abs(ref)) + 2.0 ** -24
    i = np.unravel_index(int(np.argmax(np.abs(a2 - want) - tol)), a2.shape)
    assert np.all(np.abs(a2 - want) <= tol), f"{what}: a_next {i} is {a2[i]!r}, the reference {want[i]!r}"
    clipped = np.abs(ref * SIGMA) >= CLIP + 1e-5
    assert np.all(a2[clipped] == np.sign(ref[clipped]) * CLIP), what
    return clipped, a2


def _distinct_rows(vecs, what):
    """No two (row, action vector)s of the device's draws are equal across the steps and streams collected."""
    rows = np.concatenate([np.ascontiguousarray(v, np.float32) for v in vecs])
    keys = {r.tobytes() for r in rows}
    assert len(keys) == rows.shape[0], f"{what}: {rows.shape[0] - len(keys)} repeated rows of draws"


# SAC paths as test_gpu_step_edges.PATHS sets them, and more action counts: A = 16 is where one row's counters end at
# the next row's, A = 1 the narrowest head
SAC_DRAW = [p for p in PATHS if p[1] == "sac"]
SAC_DRAW += [("sac kind 1 A=1", "sac", {}, (42, 1, 255), (256, 256), 1),
             ("sac kind 1 A=16", "sac", {}, (42, 16, 255), (256, 256), 1),
             ("sac kind 0 A=16", "sac", dict(SAC_FUSED=0), (42, 16, 201), (256, 256), 0),
             ("sac kind 2 A=16", "sac", dict(SAC_CHAIN=1, SAC_CHAIN_BWD=0), (42, 16, 1009), (256, 256), 2),
             ("sac kind 4 A=16", "sac", dict(SAC_CHAIN_BWD=1), (46, 16, 1009), (256, 256), 4),
             ("sac kind 3 A=1", "sac", dict(SAC_GENERAL=1), (42, 1, 255), (256, 256), 3),
             ("sac kind 3 deep A=16", "sac", {}, (42, 16, 129), (64, 96, 48), 3)]
TD3_DRAW = [p for p in PATHS if p[1] == "td3"]
TD3_DRAW += [("td3 fused critic A=16", "td3", {}, (42, 16, 255), (256, 256), True),
             ("td3 general A=1", "td3", {}, (42, 1, 129), (64, 96, 48), None)]


def _assert_kind(t, algo, kind):
    if algo == "sac" or kind is None:
        assert t.fused_mode() == (kind if algo == "sac" else 3)
    else:
        assert t.is_fused() == kind


@pytest.mark.parametrize("path", SAC_DRAW, ids=[p[0] for p in SAC_DRAW])
def test_sac_draws_equal_the_reference(path, monkeypatch):
    label, _, env, (O, A, B), hidden, kind = path
    _env(monkeypatch, env)
    general = kind == 3
    t = _zero_head_sac(O, A, B, hidden, SEED_LO)
    batch = _batch(B, O, A)
    seen = []
    for step in (0, 1, 2):
        t.train(batch)
        if step == 0:
            _assert_kind(t, "sac", kind)
        assert _step_count(t) == step + 1
        seen += list(check_sac_step(t, SEED_LO, step, B, A, general, f"{label} step {step}"))
    # the high word of the step counter: step 2^32 + 3 is its own draw, not step 3's
    _set_step(t, BIG_STEP)
    t.train(batch)
    z_big, a_big = check_sac_step(t, SEED_LO, BIG_STEP, B, A, general, f"{label} step 2^32+3")
    low = ns.draws(SEED_LO, 3, B, A, 0)
    assert np.max(np.abs(z_big - (np.tanh(low) if general else low))) > 0.1
    seen += [z_big, a_big]
    if A >= 2:          # (one float per row: equal values by chance are too likely to mean anything)
        _distinct_rows(seen, label)
    # the high word of the seed: its own stream
    t2 = _zero_head_sac(O, A, B, hidden, SEED_HI)
    t2.train(batch)
    z_hi, _ = check_sac_step(t2, SEED_HI, 0, B, A, general, f"{label} seed 2^32|5 step 0")
    assert np.max(np.abs(z_hi - seen[0])) > 0.1
    print(f"[noise] {label}: largest ulp distance of z from float32(reference) {ULP.get(label, 'n/a')}")


@pytest.mark.parametrize("path", TD3_DRAW, ids=[p[0] for p in TD3_DRAW])
def test_td3_smoothing_draws_equal_the_reference(path, monkeypatch):
    label, _, env, (O, A, B), hidden, kind = path
    _env(monkeypatch, env)
    t = _zero_head_td3(O, A, B, hidden, SEED_LO)
    batch = _batch(B, O, A)
    nclip, seen = 0, []
    for step in (0, 1, 2):
        t.train(batch)
        if step == 0:
            _assert_kind(t, "td3", kind)
        clipped, a2 = check_td3_step(t, SEED_LO, step, B, A, f"{label} step {step}")
        nclip += int(clipped.sum())
        seen.append(a2)
    assert nclip > 0
    _set_step(t, BIG_STEP)
    t.train(batch)
    _, a_big = check_td3_step(t, SEED_LO, BIG_STEP, B, A, f"{label} step 2^32+3")
    assert np.max(np.abs(a_big - np.clip(ns.draws(SEED_LO, 3, B, A, 1) * SIGMA, -CLIP, CLIP))) > 0.1
    if A >= 2:
        _distinct_rows(seen + [a_big], label)
    t2 = _zero_head_td3(O, A, B, hidden, SEED_HI)
    t2.train(batch)
    _, a_hi = check_td3_step(t2, SEED_HI, 0, B, A, f"{label} seed 2^32|5 step 0")
    assert np.max(np.abs(a_hi - seen[0])) > 0.1


# ---- (b) the production drivers --------------------------------------------------------------------------------------
O_, A_, B_ = 42, 7, 256


def _buffer(n, seed, rng_seed):
    from robosuite_benchmark_amd import EnvReplayBuffer
    obs, act, rew, term, nobs = synth_transitions(n, O_, A_, seed=seed, term_frac=0.1)
    buf = EnvReplayBuffer(n, obs_dim=O_, action_dim=A_)
    buf.add_block(obs, act, rew, nobs, term)
    buf.seed(rng_seed)
    return buf


@pytest.mark.parametrize("n", [1, 17, 70])
def test_train_loop_draws_equal_the_reference(n, monkeypatch):
    _env(monkeypatch, {})
    seed = 0xABCDEF0123 + n
    t = _zero_head_sac(O_, A_, B_, (256, 256), seed)
    t.train_loop(_buffer(5000, 8, 17), n, batch_size=B_)
    assert _step_count(t) == n
    check_sac_step(t, seed, n - 1, B_, A_, False, f"train_loop({n}) last step")


def test_stepwise_device_batches_draw_equal_the_reference(monkeypatch):
    _env(monkeypatch, {})
    seed, n = 991, 6
    t = _zero_head_sac(O_, A_, B_, (256, 256), seed)
    buf = _buffer(5000, 8, 17)
    for step in range(n):
        batch = buf.random_batch(B_)
        assert getattr(batch, "on_device", False)
        t.train(batch)
        check_sac_step(t, seed, step, B_, A_, False, f"device batch step {step}")


def test_trainer_group_members_draw_their_own_stream(monkeypatch):
    from robosuite_benchmark_amd import SACTrainerGroup
    _env(monkeypatch, {})
    seeds = [7, (3 << 32) | 7, 0xFEEDFACECAFEBEEF]
    ts = [_zero_head_sac(O_, A_, B_, (256, 256), s) for s in seeds]
    bufs = [_buffer(4000 + 100 * i, 8 + i, 17 + i) for i in range(3)]
    group = SACTrainerGroup(ts)
    n = 9
    group.train_loop(bufs, n, batch_size=B_)
    zs = []
    for s, t in zip(seeds, ts):
        assert _step_count(t) == n
        zs.append(check_sac_step(t, s, n - 1, B_, A_, False, f"group member seed {s:#x}")[0])
    assert np.max(np.abs(zs[0] - zs[1])) > 0.5 and np.max(np.abs(zs[1] - zs[2])) > 0.5


def test_resume_draws_equal_the_reference(tmp_path, monkeypatch):
    from robosuite_benchmark_amd import EnvReplayBuffer, checkpoint as ck
    _env(monkeypatch, {})
    seed, k = 4242, 13
    t = _zero_head_sac(O_, A_, B_, (256, 256), seed)
    buf = _buffer(5000, 8, 17)
    t.train_loop(buf, k, batch_size=B_)
    ck.save_checkpoint(str(tmp_path / "ck"), t, buf)
    del t, buf
    t2 = _zero_head_sac(O_, A_, B_, (256, 256), seed)
    buf2 = EnvReplayBuffer(5000, obs_dim=O_, action_dim=A_)
    ck.load_checkpoint(str(tmp_path / "ck"), t2, buf2)
    t2.train_loop(buf2, 1, batch_size=B_)
    assert _step_count(t2) == k + 1
    check_sac_step(t2, seed, k, B_, A_, False, f"resumed at step {k}")


# ---- (c) the whole step on device noise against the float64 oracle ---------------------------------------------------
HIGH = [p for p in PATHS if p[0] in ("sac kind 1", "sac kind 3 deep", "td3 fused critic", "td3 general")]
CASES = [(p, 0) for p in PATHS] + [(p, 2 ** 32 + 4) for p in HIGH]


@pytest.mark.parametrize("path,step", CASES, ids=[f"{p[0]}-step{s}" for p, s in CASES])
def test_step_on_device_noise_against_float64(path, step, monkeypatch):
    """From the usual init state: the kernel draws its own noise, the oracles step on float32(reference draw).
    2^32 + 4 is a multiple of 5 and of 2: the Polyak average (SAC, period 5) and the TD3 policy step run there."""
    label, algo, env, (O, A, B), hidden, kind = path
    _env(monkeypatch, env)
    seed = 0x5EED0000_00000011
    batch = _batch(B, O, A, seed=31)
    mk = make_pair if algo == "sac" else make_td3_pair
    o32, hip, o64 = mk(O, A, B, hidden=hidden, with_f64=True, noise_seed=seed)
    if step:
        _set_step(hip, step)
        o32.n_train_steps_total = o64.n_train_steps_total = step
    diag = hip.train(batch)
    _assert_kind(hip, algo, kind)
    e1 = ns.draws(seed, step, B, A, 0).astype(np.float32)
    e2 = ns.draws(seed, step, B, A, 1).astype(np.float32)
    args = (batch["observations"], batch["actions"], batch["rewards"], batch["terminals"], batch["next_observations"])
    if algo == "sac":
        want, want64 = o32.step(*args, e1, e2), o64.step(*args, e1, e2)
    else:
        want, want64 = o32.step(*args, e2), o64.step(*args, e2)
        if step:
            assert o32.last["policy_step"]
    check_step_f64(hip, o32, o64, diag, want, want64, path=f"device noise {label} step {step}")
