"""GPU parity of the TD3 step against oracle/td3_step_torch.py (rlkit-equivalent restatement;
parity unpinned: the reference ships no TD3 number).  Tolerances as for SAC: logged scalars 1e-5 * max(1, |b|)."""
import numpy as np
import pytest

from robosuite_benchmark_amd import EnvReplayBuffer
from robosuite_benchmark_amd._lib import TD3_DIAG_NAMES
from tests.helpers import _td3_pair_of_hip, check_step_f64, flat_of, make_td3_pair, rel_err, synth_transitions

pytestmark = pytest.mark.gpu


def batch_and_noise(B, O, A, seed, term_frac=0.1):
    obs, act, rew, term, nobs = synth_transitions(B, O, A, seed=seed, term_frac=term_frac)
    eps = np.random.RandomState(seed + 1).standard_normal((B, A)).astype(np.float32)
    return dict(observations=obs, actions=act, rewards=rew, terminals=term.astype(np.float32), next_observations=nobs), eps


def check_diag(diag, want, policy=True):
    for i, name in enumerate(TD3_DIAG_NAMES):
        if name in want and (policy or not name.startswith("Policy")):
            assert abs(float(diag[i]) - want[name]) <= 1e-5 * max(1.0, abs(want[name])), (name, float(diag[i]), want[name])


def scale_err(got, want):
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want)) / max(1e-30, np.max(np.abs(want))))


# (992, 334, 1328: SP * NB % 4 == 2 -- the TD3 critic launches' groups of four blocks per twin end in a partial group there;
#  round 2 mis-mapped it, found by scratch/fuzz_fused.py in round 3)
@pytest.mark.parametrize("O,A,B", [(42, 7, 256), (46, 7, 1024), (89, 14, 256), (379, 6, 64), (11, 3, 512), (5, 2, 16),
                                   (49, 5, 992), (97, 14, 334), (40, 11, 1328), (300, 13, 1095)])
def test_policy_step_from_identical_state(O, A, B):
    oracle, hip, o64 = make_td3_pair(O, A, B, seed=11, with_f64=True)
    nb, eps = batch_and_noise(B, O, A, seed=21)
    want = oracle.step(nb["observations"], nb["actions"], nb["rewards"], nb["terminals"], nb["next_observations"], eps)
    want64 = o64.step(nb["observations"], nb["actions"], nb["rewards"], nb["terminals"], nb["next_observations"], eps)
    diag = hip.train(nb, eps=eps)                          # step 0 is a policy step
    check_diag(diag, want)
    check_step_f64(hip, oracle, o64, diag, want, want64)
    L = oracle.last
    for name, ref in (("a_next", L["noisy"]), ("a_new", L["pa"])):
        assert scale_err(hip.debug_fetch(name, B * A), ref.detach().numpy().ravel()) < 2e-5, name
    for name, ref in (("q1", L["q1"]), ("q2", L["q2"]), ("q_target", L["y"]), ("tq1", L["tq1"]), ("tq2", L["tq2"]),
                      ("q1_new", L["q_pi"])):
        assert rel_err(hip.debug_fetch(name, B), ref.detach().numpy().ravel()) < 2e-5, name
    for g in ("g_qf1", "g_qf2", "g_policy"):
        assert scale_err(hip.debug_fetch(g, L[g].size), L[g]) < 5e-5, g
    # parameters after the step: Adam's first step is +-lr per element, compare to a fraction of lr; targets exactly Polyak
    nets = oracle.export_nets()
    got = hip.state_dict()["params"]
    for name, lr in (("qf1", 5e-4), ("qf2", 5e-4), ("policy", 1e-3)):
        d = np.abs(got[name] - flat_of(nets[name]))
        assert np.mean(d > 0.1 * lr) < 2e-3, name          # sign flips only where the gradient is ~0
    for name in ("target_qf1", "target_qf2", "target_policy"):
        assert np.max(np.abs(got[name] - flat_of(nets[name]))) < 2e-5, name


def test_five_steps_track_the_oracle_with_delayed_updates():
    O, A, B = 42, 7, 128
    oracle, hip = make_td3_pair(O, A, B, seed=5, policy_and_target_update_period=2)
    pol0 = hip.state_dict()["params"]["policy"].copy()
    for step in range(5):
        nb, eps = batch_and_noise(B, O, A, seed=100 + step)
        want = oracle.step(nb["observations"], nb["actions"], nb["rewards"], nb["terminals"], nb["next_observations"], eps)
        before = hip.state_dict()["params"]
        diag = hip.train(nb, eps=eps)
        after = hip.state_dict()["params"]
        pstep = step % 2 == 0
        for i, name in enumerate(TD3_DIAG_NAMES):            # trajectories drift apart slowly (Adam sign flips): 1e-3
            if name in want:
                assert abs(float(diag[i]) - want[name]) <= 1e-3 * max(1.0, abs(want[name])), (step, name)
        for name in ("policy", "target_policy", "target_qf1", "target_qf2"):
            assert np.array_equal(before[name], after[name]) == (not pstep), (step, name)
        assert not np.array_equal(before["qf1"], after["qf1"])
    assert not np.array_equal(pol0, hip.state_dict()["params"]["policy"])
    sc = hip.state_dict()["scalars"]
    assert (sc[0], sc[3], sc[4]) == (3.0, 5.0, 5.0)          # policy Adam steps, critic Adam steps, train steps


def test_fused_loop_equals_stepwise_and_device_batches():
    O, A, B, steps, n = 42, 7, 256, 21, 6000
    _, fused = make_td3_pair(O, A, B, seed=4, noise_seed=7)
    _, stepw = make_td3_pair(O, A, B, seed=4, noise_seed=7)
    obs, act, rew, term, nobs = synth_transitions(n, O, A, seed=8)
    bufs = []
    for _ in range(2):
        b = EnvReplayBuffer(n, obs_dim=O, action_dim=A)
        b.add_block(obs, act, rew, nobs, term)
        b.seed(17)
        bufs.append(b)
    first, last = fused.train_loop(bufs[0], steps, batch_size=B)
    outs = [stepw.train(bufs[1].random_batch(B)) for _ in range(steps)]
    assert outs[0] is not None and np.array_equal(outs[0], first)
    sa, sb = fused.state_dict(), stepw.state_dict()
    for k in sa["params"]:
        assert np.array_equal(sa["params"][k], sb["params"][k]), k
    for k in sa["opt"]:
        assert np.array_equal(sa["opt"][k][0], sb["opt"][k][0]) and np.array_equal(sa["opt"][k][1], sb["opt"][k][1]), k
    assert np.array_equal(sa["scalars"], sb["scalars"])
    assert np.all(np.isfinite(last[:28]))


def test_learning_and_snapshot_keys():
    O, A, B = 11, 3, 64
    _, hip = make_td3_pair(O, A, B, seed=9, noise_seed=1)
    obs, act, rew, term, nobs = synth_transitions(3000, O, A, seed=3)
    buf = EnvReplayBuffer(3000, obs_dim=O, action_dim=A)
    buf.add_block(obs, act, rew, nobs, term)
    buf.seed(1)
    first, last = hip.train_loop(buf, 400, batch_size=B)
    i = TD3_DIAG_NAMES.index
    assert last[i("QF1 Loss")] < first[i("QF1 Loss")]
    assert last[i("Policy Loss")] < first[i("Policy Loss")]      # the actor climbs Q1
    snap = hip.get_snapshot()
    assert {"policy", "qf1", "qf2", "target_qf1", "target_qf2", "target_policy", "trained_policy"} <= set(snap)
    a, _ = snap["trained_policy"].get_action(obs[0])
    assert a.shape == (A,) and np.all(np.abs(a) <= 1)
    assert set(hip.get_diagnostics()) >= {"QF1 Loss", "Policy Loss", "Bellman Errors 1 Mean", "Policy Action Max"}


def test_td3_variant_through_the_driver_with_checkpoint_resume(tmp_path):
    """agent == "TD3" (rlkit_utils.py:107-135) through the epoch driver; checkpoint + resume continue bit for bit."""
    from robosuite_benchmark_amd.driver import experiment
    from robosuite_benchmark_amd.variant import default_variant
    v = default_variant(env="Lift", seed=3, batch_size=128, agent="TD3")
    assert v["algorithm"] == "TD3" and v["trainer_kwargs"]["policy_and_target_update_period"] == 2
    v["algorithm_kwargs"].update(num_epochs=3, num_trains_per_train_loop=41, num_expl_steps_per_train_loop=100,
                                 num_eval_steps_per_epoch=100, min_num_steps_before_training=200,
                                 expl_max_path_length=50, eval_max_path_length=50)
    v["replay_buffer_size"] = 5000
    straight = experiment(v, seed=3, quiet=True)
    assert len(straight) == 3
    row = straight[-1]
    for k in ("trainer/QF1 Loss", "trainer/Policy Loss", "trainer/Bellman Errors 2 Mean", "trainer/Policy Action Std",
              "exploration/Returns Mean", "evaluation/Returns Mean", "replay_buffer/size"):
        assert k in row and np.isfinite(row[k]), k
    assert "trainer/Alpha" not in row and row["replay_buffer/size"] == 200 + 3 * 100
    ckd = str(tmp_path / "ck")
    experiment(v, seed=3, quiet=True, num_epochs=2, checkpoint_dir=ckd)
    resumed = experiment(v, seed=3, quiet=True, checkpoint_dir=ckd, resume=True)
    assert [r["Epoch"] for r in resumed] == [2]
    for k in straight[2]:
        if not k.startswith("time/"):
            assert straight[2][k] == resumed[0][k], k


# ---- round 3: the TD3 critic pass as ONE launch (k_abc<.., M_TD3_CRITIC>, csrc/sac_fused.h) ----------------------------
def _filled(n, O, A, seed):
    obs, act, rew, term, nobs = synth_transitions(n, O, A, seed=seed, term_frac=0.05)
    b = EnvReplayBuffer(n, obs_dim=O, action_dim=A)
    b.add_block(obs, act, rew, nobs, term)
    return b


def _same_state(sa, sb):
    for k in sa["params"]:
        assert np.array_equal(sa["params"][k], sb["params"][k]), k
    for k in sa["opt"]:
        assert np.array_equal(sa["opt"][k][0], sb["opt"][k][0]) and np.array_equal(sa["opt"][k][1], sb["opt"][k][1]), k
    assert np.array_equal(sa["scalars"], sb["scalars"])


# narrow and wide first layers, odd batches (padded row-blocks), one row-block, the largest action chunk
@pytest.mark.parametrize("O,A,B,steps", [(42, 7, 256, 21), (42, 7, 128, 15), (89, 14, 256, 9), (379, 6, 256, 7), (10, 3, 16, 13),
                                         (60, 7, 250, 9), (130, 16, 64, 7), (1, 1, 17, 6)])
def test_fused_critic_pass_equals_four_launch_critic_pass_bitwise(O, A, B, steps):
    fused, plain = _td3_pair_of_hip(O, A, B, seed=4, noise_seed=9)
    assert fused.is_fused() and not plain.is_fused()
    bufs = [_filled(5000, O, A, 8), _filled(5000, O, A, 8)]
    for b in bufs:
        b.seed(31)
    fa, la = fused.train_loop(bufs[0], steps, batch_size=B)
    fb, lb = plain.train_loop(bufs[1], steps, batch_size=B)
    assert np.array_equal(fa, fb) and np.array_equal(la, lb)
    ta = fused.debug_fetch("diag_trace", steps * 32).reshape(steps, 32)
    tb = plain.debug_fetch("diag_trace", steps * 32).reshape(steps, 32)
    assert np.array_equal(ta, tb)
    _same_state(fused.state_dict(), plain.state_dict())
    for name, n in (("q1", B), ("q2", B), ("q_target", B), ("a_next", B * A)):
        assert np.array_equal(fused.debug_fetch(name, n), plain.debug_fetch(name, n)), name


def test_td3_single_steps_with_given_noise_fused_vs_four_launch():
    O, A, B = 46, 7, 256
    fused, plain = _td3_pair_of_hip(O, A, B, seed=2, noise_seed=1)
    for step in range(5):                                    # policy steps and critic-only steps alternate
        nb, eps = batch_and_noise(B, O, A, seed=50 + step)
        da, db = fused.train(nb, eps=eps), plain.train(nb, eps=eps)
        fused.end_epoch(step); plain.end_epoch(step)
        assert np.array_equal(da, db), step
    _same_state(fused.state_dict(), plain.state_dict())


@pytest.mark.parametrize("stall_at,steps", [(3, 10), (6, 11)])
def test_td3_fused_pass_giving_up_falls_back_transparently(stall_at, steps):
    """Launch `stall_at` loses a producer (test hook): that critic pass, its actor pass if it had one, and everything queued
    behind apply nothing; the call re-runs the lost steps on the four-launch kernels.  The policy's own optimizer-step
    count (every second step) comes back right too."""
    O, A, B = 42, 7, 256
    fused, plain = _td3_pair_of_hip(O, A, B, seed=4, noise_seed=9, SAC_FUSED_TEST_STALL=stall_at)
    bufs = [_filled(4000, O, A, 8), _filled(4000, O, A, 8)]
    for b in bufs:
        b.seed(31)
    fa, la = fused.train_loop(bufs[0], steps, batch_size=B)
    assert not fused.is_fused()
    fb, lb = plain.train_loop(bufs[1], steps, batch_size=B)
    assert np.array_equal(fa, fb) and np.array_equal(la, lb)
    _same_state(fused.state_dict(), plain.state_dict())
    sc = fused.state_dict()["scalars"]
    assert (sc[0], sc[3], sc[4]) == ((steps + 1) // 2, steps, steps)
    (ka, pa), (kb, pb) = bufs[0].rng_state(), bufs[1].rng_state()
    assert pa == pb and np.array_equal(ka, kb)
