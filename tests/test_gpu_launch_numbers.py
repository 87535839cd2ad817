"""GPU: the fused step at LARGE launch numbers.  Every in-launch hand-off of k_abc (csrc/sac_fused.h) and k_chain8<.., BWD>
(csrc/sac_chain.h) waits for a counter to reach units x launch number modulo 2^32, and the row-block sums of log pi travel
tagged with the launch number itself.  A trainer starts at launch number 0 and 2^28 launches are hours away, so the test
hook sac_debug_set_launch_number puts a fused trainer a few launches in front of each power of two that one of the
multiples crosses, and the launches then straddle it.

The reference is the four-launch step of the same library (k_chain8 + k_bwd8 for the chained launch): it carries no
launch number, the fused step has to equal it bit for bit (test_gpu_fused_step.py, test_gpu_td3.py, test_gpu_large_batch.py)
and the suite ties it to the float64 oracle.  So every comparison here is np.array_equal -- there is no tolerance -- and two
cases run their first step at launch number 2^28 + 1 straight against the float32 and float64 oracles as well.

The give-up cases use the orderly 50 ms time-out of the existing SAC_FUSED_TEST_STALL hook (one producer leaves without
publishing); the variable counts from the launch number the hook set."""
import numpy as np
import pytest

from tests.helpers import (_td3_pair_of_hip, check_step_f64, make_pair, make_td3_pair, pair_of_hip, plain_buffer)

pytestmark = pytest.mark.gpu

# what crosses: 8 seq passes 2^31 | 4 seq passes 2^31, 8 seq wraps | 4 seq wraps | seq changes sign | seq wraps to 0 (tag 0)
BOUNDARIES = [2**28, 2**29, 2**30, 2**31, 2**32]
SAC_SHAPES = [(42, 7, 256), (10, 3, 16), (60, 7, 250),      # narrow first layers: sixteen row-blocks, one, a padded one
              (379, 6, 64)]                                 # wide first layers: the cnt_zx exchange
TD3_SHAPES = [(42, 7, 128), (1, 1, 17)]
CHAIN_SHAPE = (10, 3, 544)                                  # 34 row-blocks: the smallest batch the chained launch takes
CHAIN_NB = 34


def _same_state(sa, sb):
    for k in sa["params"]:
        assert np.array_equal(sa["params"][k], sb["params"][k]), k
    for k in sa["opt"]:
        assert np.array_equal(sa["opt"][k][0], sb["opt"][k][0]) and np.array_equal(sa["opt"][k][1], sb["opt"][k][1]), k
    assert np.array_equal(sa["scalars"], sb["scalars"])


def _same_generators(ba, bb):
    (ka, pa), (kb, pb) = ba.rng_state(), bb.rng_state()
    assert pa == pb and np.array_equal(ka, kb)


def _buffers(O, A, seed=8, n=5000, k=2):
    bufs = [plain_buffer(n, O, A, seed) for _ in range(k)]
    for b in bufs:
        b.seed(31)
    return bufs


def _loop_both(a, b, bufs, steps, B):
    """train_loop on both trainers: first and last diagnostics and the whole per-step trace, bit for bit"""
    fa, la = a.train_loop(bufs[0], steps, batch_size=B)
    fb, lb = b.train_loop(bufs[1], steps, batch_size=B)
    assert np.array_equal(fa, fb) and np.array_equal(la, lb)
    ta = a.debug_fetch("diag_trace", steps * 32).reshape(steps, 32)
    tb = b.debug_fetch("diag_trace", steps * 32).reshape(steps, 32)
    assert np.array_equal(ta, tb)


def _same_rows(a, b, B, A):
    for name, n in (("q1", B), ("q2", B), ("q_target", B), ("a_next", B * A)):
        assert np.array_equal(a.debug_fetch(name, n), b.debug_fetch(name, n)), name


def _host_batch(B, O, A, seed):
    from tests.helpers import synth_transitions
    obs, act, rew, term, nobs = synth_transitions(B, O, A, seed=seed, term_frac=0.1)
    return dict(observations=obs, actions=act, rewards=rew, terminals=term.astype(np.float32), next_observations=nobs)


# ---- k_abc, SAC -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", BOUNDARIES)
@pytest.mark.parametrize("O,A,B", SAC_SHAPES)
def test_sac_fused_step_across_a_launch_number_boundary(O, A, B, S):
    fused, plain = pair_of_hip(O, A, B, seed=4, noise_seed=9)
    assert fused.is_fused() and not plain.is_fused()
    fused.set_launch_number(S - 4)
    bufs = _buffers(O, A)
    _loop_both(fused, plain, bufs, 9, B)                       # launches S - 3 .. S + 5
    _same_state(fused.state_dict(), plain.state_dict())
    _same_rows(fused, plain, B, A)
    assert fused.is_fused()                                    # no wait timed out into a give-up
    _same_generators(*bufs)


# ---- k_abc, the TD3 critic pass ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", BOUNDARIES)
@pytest.mark.parametrize("O,A,B", TD3_SHAPES)
def test_td3_fused_critic_pass_across_a_launch_number_boundary(O, A, B, S):
    """Stepwise host batches with given noise, the loop, stepwise again: policy steps and critic-only steps alternate across
    the boundary (launches S - 3 .. S + 5)."""
    fused, plain = _td3_pair_of_hip(O, A, B, seed=4, noise_seed=9)
    assert fused.is_fused() and not plain.is_fused()
    fused.set_launch_number(S - 4)
    bufs = _buffers(O, A)
    rs = np.random.RandomState(5)

    def stepwise(n, seed):
        for i in range(n):
            nb, eps = _host_batch(B, O, A, seed + i), rs.standard_normal((B, A)).astype(np.float32)
            da, db = fused.train(nb, eps=eps), plain.train(nb, eps=eps)
            fused.end_epoch(i); plain.end_epoch(i)
            assert np.array_equal(da, db), (seed, i)
    stepwise(2, 50)                                            # launches S - 3, S - 2
    _loop_both(fused, plain, bufs, 4, B)                       # S - 1 .. S + 2
    stepwise(3, 60)                                            # S + 3 .. S + 5
    _same_state(fused.state_dict(), plain.state_dict())
    _same_rows(fused, plain, B, A)
    assert fused.is_fused()
    _same_generators(*bufs)


# ---- k_chain8<.., BWD>: targets seq and NB x seq -----------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2**31 // CHAIN_NB + 1, 2**32 // CHAIN_NB + 1, 2**31, 2**32])
def test_chained_launch_with_backward_across_a_launch_number_boundary(S, monkeypatch):
    from tests.test_gpu_large_batch import _chain_pair
    O, A, B = CHAIN_SHAPE
    one, two = _chain_pair(O, A, B, monkeypatch)
    assert one.fused_mode() == 4 and two.fused_mode() == 2
    one.set_launch_number(S - 4)
    bufs = _buffers(O, A, seed=2)
    _loop_both(one, two, bufs, 8, B)                           # launches S - 3 .. S + 4
    _same_state(one.state_dict(), two.state_dict())
    _same_rows(one, two, B, A)
    assert one.fused_mode() == 4
    _same_generators(*bufs)


# ---- the launch number does not enter the arithmetic ----------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_a_fused_trainer_at_a_large_launch_number_equals_one_at_zero(algo):
    O, A, B, S = 42, 7, 128, 2**28
    pair = pair_of_hip if algo == "sac" else _td3_pair_of_hip
    high, _ = pair(O, A, B, seed=4, noise_seed=9)
    zero, _ = pair(O, A, B, seed=4, noise_seed=9)
    assert high.is_fused() and zero.is_fused()
    before = high.state_dict()
    high.set_launch_number(S - 4)
    _same_state(before, high.state_dict())                     # the hook leaves the trained state alone
    bufs = _buffers(O, A)
    _loop_both(high, zero, bufs, 9, B)
    _same_state(high.state_dict(), zero.state_dict())
    _same_rows(high, zero, B, A)
    assert high.is_fused() and zero.is_fused()
    _same_generators(*bufs)


def test_a_trainer_that_is_not_fused_is_refused():
    _, plain = pair_of_hip(42, 7, 64, seed=1, noise_seed=1)
    with pytest.raises(RuntimeError, match="does not run the fused step"):
        plain.set_launch_number(7)
    _, td3_plain = _td3_pair_of_hip(42, 7, 64, seed=1, noise_seed=1)
    with pytest.raises(RuntimeError, match="does not run the fused step"):
        td3_plain.set_launch_number(7)


# ---- launch number 2^28 + 1 against the float32 and float64 oracles ---------------------------------------------------------
def test_sac_single_step_at_a_large_launch_number_against_the_oracles():
    from tests.test_gpu_sac_step import batch_and_noise, check_diag
    O, A, B = 42, 7, 256
    oracle, hip, o64 = make_pair(O, A, B, seed=11, with_f64=True)
    assert hip.is_fused()
    hip.set_launch_number(2**28)
    np_batch, eps = batch_and_noise(B, O, A, seed=21, term_frac=0.05)
    args = (np_batch["observations"], np_batch["actions"], np_batch["rewards"], np_batch["terminals"],
            np_batch["next_observations"], *eps)
    want, want64 = oracle.step(*args), o64.step(*args)
    diag = hip.train(np_batch, eps=eps)
    check_diag(diag, want)
    check_step_f64(hip, oracle, o64, diag, want, want64)
    assert hip.is_fused()


def test_td3_single_step_at_a_large_launch_number_against_the_oracles():
    from tests.test_gpu_td3 import batch_and_noise, check_diag
    O, A, B = 42, 7, 256
    oracle, hip, o64 = make_td3_pair(O, A, B, seed=11, with_f64=True)
    assert hip.is_fused()
    hip.set_launch_number(2**28)
    nb, eps = batch_and_noise(B, O, A, seed=21)
    args = (nb["observations"], nb["actions"], nb["rewards"], nb["terminals"], nb["next_observations"], eps)
    want, want64 = oracle.step(*args), o64.step(*args)
    diag = hip.train(nb, eps=eps)                              # step 0 is a policy step
    check_diag(diag, want)
    check_step_f64(hip, oracle, o64, diag, want, want64)
    assert hip.is_fused()


# ---- a give-up across a boundary --------------------------------------------------------------------------------------------
# SAC_FUSED_TEST_STALL=3 with the trainer at S - 2: the first lost launch is number S + 1.  Launch D leaves that number in the
# diagnostics' slot 30 as a float's bits: a large positive float (2^28 + 1), the first pattern past -0.0 (2^31 + 1: a negative
# denormal), 1 after the wrap (2^32 + 1) -- and a quiet NaN's pattern, 0x7fc00000, which has to come back bit for bit.
GIVE_UP_AT = [2**28 + 1, 2**31 + 1, 2**32 + 1, 0x7FC00000]


@pytest.mark.parametrize("first_lost", GIVE_UP_AT)
def test_td3_give_up_across_a_boundary_inside_the_loop_call(first_lost):
    O, A, B, steps = 42, 7, 256, 10
    fused, plain = _td3_pair_of_hip(O, A, B, seed=4, noise_seed=9, SAC_FUSED_TEST_STALL=3)
    fused.set_launch_number(first_lost - 3)
    bufs = _buffers(O, A, n=4000)
    assert fused.is_fused()
    fa, la = fused.train_loop(bufs[0], steps, batch_size=B)
    assert not fused.is_fused()
    fb, lb = plain.train_loop(bufs[1], steps, batch_size=B)
    assert np.array_equal(fa, fb) and np.array_equal(la, lb)
    _same_state(fused.state_dict(), plain.state_dict())
    sc = fused.state_dict()["scalars"]
    assert (sc[0], sc[3], sc[4]) == ((steps + 1) // 2, steps, steps)
    _same_generators(*bufs)


@pytest.mark.parametrize("first_lost", GIVE_UP_AT)
def test_sac_give_up_across_a_boundary_inside_the_loop_call(first_lost):
    O, A, B, steps = 42, 7, 256, 10
    fused, plain = pair_of_hip(O, A, B, seed=4, noise_seed=9, SAC_FUSED_TEST_STALL=3)
    fused.set_launch_number(first_lost - 3)
    bufs = _buffers(O, A, n=4000)
    assert fused.is_fused()
    fa, la = fused.train_loop(bufs[0], steps, batch_size=B)
    assert not fused.is_fused()
    fb, lb = plain.train_loop(bufs[1], steps, batch_size=B)
    assert np.array_equal(fa, fb) and np.array_equal(la, lb)
    _same_state(fused.state_dict(), plain.state_dict())
    sc = fused.state_dict()["scalars"]
    assert sc[3] == steps and sc[4] == steps
    _same_generators(*bufs)


@pytest.mark.parametrize("first_lost", GIVE_UP_AT)
def test_sac_give_up_across_a_boundary_on_the_stepwise_device_batch_interface(first_lost):
    """random_batch(); train() on device batches, nobody waiting for a step: the steps queued behind the lost launch apply
    nothing, and the host computes how many were lost from the recorded launch number -- across the boundary -- when it
    settles the trainer, then re-runs them from their slots."""
    from robosuite_benchmark_amd import _lib
    O, A, B, steps = 42, 7, 128, 12
    fused, plain = pair_of_hip(O, A, B, seed=5, noise_seed=3, SAC_FUSED_TEST_STALL=3)
    fused.set_launch_number(first_lost - 3)
    bufs = _buffers(O, A, seed=2, n=3000)
    for tr, b in ((fused, bufs[0]), (plain, bufs[1])):
        for _ in range(steps):
            tr.train(b.random_batch(B))
        _lib.check(tr._lib.sac_sync(tr._h), "sac_sync")
    _same_state(fused.state_dict(), plain.state_dict())        # (state_dict settles the trainer)
    assert not fused.is_fused()
    sc = fused.state_dict()["scalars"]
    assert sc[3] == steps and sc[4] == steps
    _same_generators(*bufs)


def test_chained_launch_give_up_across_the_wrap(monkeypatch):
    from tests.test_gpu_large_batch import _chain_pair
    O, A, B = CHAIN_SHAPE
    one, two = _chain_pair(O, A, B, monkeypatch, SAC_FUSED_TEST_STALL=3)
    one.set_launch_number(2**32 - 2)
    bufs = _buffers(O, A, seed=2)
    fa, la = one.train_loop(bufs[0], 8, batch_size=B)
    fb, lb = two.train_loop(bufs[1], 8, batch_size=B)
    assert one.fused_mode() == 2
    assert np.array_equal(fa, fb) and np.array_equal(la, lb)
    _same_state(one.state_dict(), two.state_dict())
    _same_generators(*bufs)
