"""GPU: one step on EVERY step path from the trained regime (tests/trained_states.py: the networks of a shipped run, weights
up to 39, Q about -114, a tenth of a_new exactly +-1.0f, log_std on its clamp) with target networks that differ from the
online ones -- against the float64 oracle per tensor (helpers.check_step_f64), against the fp32 oracle on the logged
scalars (1e-5 max(1, |b|)) and on the target values per row, and what the step wrote back per element
(helpers.check_optimizer_step), from zero moments and from injected moments at t = 1000.  Then the paths that are one
arithmetic stay bit for bit from that state, trainer groups against their solo twins included.

tests/test_trained_states_host.py shows on the CPU that every (state, batch) here is inside the regime, that swapping the
targets for the online nets moves the target values far beyond the bound, and that every row of the table selects the
path it names."""
import numpy as np
import pytest

from tests import trained_states as ts
from tests.helpers import (F64_ERRORS, OPT_ULPS, check_optimizer_step, check_step_f64, make_pair, make_td3_pair, optimizer_cfg,
                           rel_err)
from tests.test_gpu_optimizer_step import _inject
from tests.test_trained_states_host import ROW_TOL, STAT_TOL, ill_conditioned, ill_conditioned_rows, oracle_of, step

pytestmark = pytest.mark.gpu

# label -> what is held to the float64 rule alone on that path: logged statistics, and per-row target values by their
# debug_fetch name.  Only a quantity on which the fp32 oracle ITSELF is more than bound / 8 from the float64 one
# (test_trained_states_host.ill_conditioned / ill_conditioned_rows, decided by the two references) may stand here, and
# test_one_step_on_every_path asserts that it is.  Everything else is held to the fp32 oracle: statistics to
# 1e-5 max(1, |b|), target values per row to 2e-5.  The figures measured on the MI355X are in that test's docstring.
FLOAT64_ONLY = {"td3 fused critic": ("q_target", "tq1"),
                "td3 four-launch SP 4": ("q_target", "tq1"),
                "td3 four-launch SP 2": ("Bellman Errors 1 Min", "q_target", "tq1"),
                "td3 four-launch SP 1": ("tq2",),
                "td3 general": ("Bellman Errors 1 Min", "Bellman Errors 2 Min"),
                "td3 inflated 126/14": ("Bellman Errors 1 Min",)}


def _setenv(monkeypatch, env):
    for k in ts.ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _kind_ok(hip, algo, kind):
    if algo == "sac":
        return hip.fused_mode() in (kind if isinstance(kind, tuple) else (kind,))
    return hip.fused_mode() == 3 if kind is None else hip.is_fused() == kind


@pytest.mark.parametrize("path", ts.PATHS, ids=[p[0] for p in ts.PATHS])
def test_one_step_on_every_path(path, monkeypatch):
    """Every SAC path holds every logged scalar to 1e-5 max(1, |b|) and q_target per row to 2e-5 of the fp32 oracle.

    TD3 quantities held to the float64 rule alone (FLOAT64_ONLY), measured on the MI355X as distance kernel - fp32 oracle /
    kernel - float64 / fp32 oracle - float64 (relative, max(1, |b|) denominators).  In each the two fp32 computations are
    about equally far from float64 and their mutual distance is the sum: TD3's target action tanh(.) + noise carries the
    ~1e-5 rounding of a saturating policy into critics whose action gradient is O(100), and a Bellman error minimum is the
    square of a difference of two Q values of about -114.
      td3 fused critic, td3 four-launch SP 4 (B 255): q_target 2.26e-5 / 1.04e-5 / 1.23e-5; tq1 2.29e-5 / 1.08e-5 / 1.24e-5
      td3 four-launch SP 2 (B 288): q_target 3.46e-5 / 6.81e-5 / 3.35e-5; tq1 3.71e-5 / 7.29e-5 / 3.58e-5;
        Bellman Errors 1 Min 0.16316615 against 0.16314766: 1.85e-5, the fp32 oracle 7.07e-6 from float64
      td3 four-launch SP 1 (B 544): tq2 3.21e-5 / 2.96e-5 / 3.55e-5
      td3 general (B 255): Bellman Errors 1 Min 0.12302822 against 0.12300681: 2.14e-5, the fp32 oracle 2.40e-5 from float64;
        Bellman Errors 2 Min 0.07122495 against 0.07121070: 1.42e-5, the fp32 oracle 1.13e-5
      td3 inflated 126/14 (B 255): Bellman Errors 1 Min 0.34594739 against 0.34601918: 7.18e-5, the fp32 oracle 4.69e-5"""
    label, algo, env, (ko, ka, B), kind = path
    _setenv(monkeypatch, env)
    td3 = algo == "td3"
    O, A = ts.O0 * ko, ts.A0 * ka
    nets, batch, eps = ts.state(algo, ko, ka, B)
    o32, hip, o64 = (make_td3_pair if td3 else make_pair)(O, A, B, nets=nets, with_f64=True)
    before = hip.state_dict()
    for name in nets:                                     # the trainer holds the lagged targets, not the online nets
        if name.startswith("target_"):
            assert not np.array_equal(before["params"][name], before["params"][name[len("target_"):]]), name
    diag = hip.train(batch, eps=eps[0] if td3 else eps)
    after = hip.state_dict()
    assert _kind_ok(hip, algo, kind), (label, hip.fused_mode())
    want, want64 = step(o32, algo, batch, eps), step(o64, algo, batch, eps)

    # against float64: gradients per named tensor, per-row outputs, diagnostics
    tag = "trained " + label
    check_step_f64(hip, o32, o64, diag, want, want64, path=tag)
    print(f"{tag}: largest kernel error / scale, its tensor, the fp32 oracle's: {F64_ERRORS.get(tag)}")

    # against the fp32 oracle: logged scalars
    from robosuite_benchmark_amd._lib import DIAG_NAMES, TD3_DIAG_NAMES
    ill = ill_conditioned(want, want64)
    misses = []
    for i, name in enumerate(TD3_DIAG_NAMES if td3 else DIAG_NAMES):
        if name not in want:
            continue
        d = abs(float(diag[i]) - want[name]) / max(1.0, abs(want[name]))
        if name in FLOAT64_ONLY.get(label, ()):
            assert name in ill, (label, name, "the two references do not show this statistic ill-conditioned")
            print(f"{tag}: {name} held to float64 alone: {d:.3g} of the fp32 oracle, which is {ill[name]:.3g} from float64")
        elif not d <= STAT_TOL:
            misses.append((name, float(diag[i]), want[name], d, ill.get(name)))
            print(f"{tag}: MISS {name}: kernel {float(diag[i]):.9g}, fp32 oracle {want[name]:.9g} ({d:.3g}); "
                  f"fp32 oracle from float64: {ill.get(name)}")

    # the target values per row: the target nets, not the online ones
    swapped = oracle_of(algo, ts.with_online_targets(nets))
    step(swapped, algo, batch, eps)
    ill_rows = ill_conditioned_rows(o32, o64)
    for name, key in (("q_target", "y"),) + ((("tq1", "tq1"), ("tq2", "tq2")) if td3 else ()):
        ref, ref64 = o32.last[key].detach().numpy().ravel(), o64.last[key].detach().numpy().ravel()
        got = hip.debug_fetch(name, B)
        e, e64, p64 = rel_err(got, ref), rel_err(got, ref64), rel_err(ref, ref64)
        moved = rel_err(swapped.last[key].detach().numpy().ravel(), ref)
        print(f"{tag}: {name} per row {e:.3g} of the fp32 oracle (bound {ROW_TOL}), {e64:.3g} of float64, the fp32 oracle "
              f"{p64:.3g} of float64; online nets in their place: {moved:.3g}")
        assert moved > ROW_TOL, (label, name, "this case cannot tell the target nets from the online ones", moved)
        if name in FLOAT64_ONLY.get(label, ()):          # (check_step_f64 above held these rows to float64)
            assert key in ill_rows, (label, name, "the two references do not show these rows ill-conditioned")
        elif not e < ROW_TOL:
            misses.append((name, e, e64, p64))
            print(f"{tag}: MISS {name}")
    assert not misses, (label, misses)

    # what the step wrote back, per element; then from injected moments at t = 1000 (on the period: Polyak, TD3's policy step)
    cfg = optimizer_cfg(hip)
    check_optimizer_step(hip, before, after, cfg, tag)
    _inject(hip, np.random.RandomState(11), 999, 1000, 499 if td3 else None)
    before = hip.state_dict()
    hip.train(batch, eps=eps[0] if td3 else eps)
    check_optimizer_step(hip, before, hip.state_dict(), cfg, tag)
    print(f"{tag}: written state, largest distances in ulp and of the bound: {OPT_ULPS.get(tag)}")


# ---- paths that are one arithmetic stay bit for bit from trained state ----------------------------------------------------
STEPS = 6                     # Polyak fires at steps 0 and 5 (period 5); TD3's policy steps at 0, 2, 4


def _trainer(algo, ko, ka, B, env, monkeypatch, noise_seed, lag_seed=0):
    _setenv(monkeypatch, env)
    nets = ts.inflate(ts.trained_nets(algo, seed=lag_seed), ko, ka, seed=1)
    return (make_td3_pair if algo == "td3" else make_pair)(ts.O0 * ko, ts.A0 * ka, B, nets=nets, noise_seed=noise_seed)[1]


def _buffer(ko, ka, seed, n=3000):
    """helpers.filled_buffer's rows (terminal fraction 0.1, generator seeded), tiled for an inflated shape."""
    from robosuite_benchmark_amd import EnvReplayBuffer
    obs, act, rew, term, nobs = ts.trained_rows(n, ko, ka, seed, term_frac=0.1)
    buf = EnvReplayBuffer(n, obs_dim=ts.O0 * ko, action_dim=ts.A0 * ka)
    buf.add_block(obs, act, rew, nobs, term)
    buf.seed(seed)
    return buf


def _run(t, buf, B, steps=STEPS):
    """(first and last diagnostics, params, both Adam moments, scalars, generator state) after `steps` loop steps."""
    first, last = t.train_loop(buf, steps, batch_size=B)
    st = t.state_dict()
    k, p = buf.rng_state()
    out = {"first": np.array(first), "last": np.array(last), "scalars": np.array(st["scalars"]), "generator": np.asarray(k),
           "generator position": np.asarray([p])}
    for name, v in st["params"].items():
        out["params " + name] = v
    for name, (m, v) in st["opt"].items():
        out["exp_avg " + name], out["exp_avg_sq " + name] = m, v
    assert np.all(np.isfinite(out["last"][:28])) and out["scalars"][4] == steps
    return out


def _same(a, b, where):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (where, k)


def _pair_bitwise(algo, ko, ka, B, env_a, env_b, check_a, check_b, monkeypatch, where):
    a = _trainer(algo, ko, ka, B, env_a, monkeypatch, noise_seed=9)
    b = _trainer(algo, ko, ka, B, env_b, monkeypatch, noise_seed=9)
    ra, rb = _run(a, _buffer(ko, ka, 8), B), _run(b, _buffer(ko, ka, 8), B)
    assert check_a(a) and check_b(b), (where, a.fused_mode(), b.fused_mode())
    _same(ra, rb, where)
    moved = ts.inflate(ts.trained_nets(algo), ko, ka, seed=1)["target_qf1"][0][0]
    w0 = ra["params target_qf1"][:moved.size].reshape(moved.shape)
    assert not np.array_equal(w0, moved)                 # Polyak moved the targets


@pytest.mark.parametrize("ko,ka", [(1, 1), (3, 2)])
def test_fused_step_equals_four_launch_step_bitwise(ko, ka, monkeypatch):
    _pair_bitwise("sac", ko, ka, 255, {}, dict(SAC_FUSED=0), lambda t: t.fused_mode() == 1, lambda t: t.fused_mode() == 0,
                  monkeypatch, ("fused / four-launch", ko, ka))


def test_td3_fused_critic_equals_four_launch_critic_bitwise(monkeypatch):
    _pair_bitwise("td3", 1, 1, 255, {}, dict(SAC_FUSED=0), lambda t: t.is_fused(), lambda t: not t.is_fused(), monkeypatch,
                  "td3 fused / four-launch")


SP1 = [(1, 1, 530), (2, 1, 544)]


@pytest.mark.parametrize("ko,ka,B", SP1)
def test_eight_wave_chain_equals_four_wave_chain_bitwise(ko, ka, B, monkeypatch):
    _pair_bitwise("sac", ko, ka, B, dict(ts.CHAIN, SAC_CHAIN8=1), dict(ts.CHAIN, SAC_CHAIN8=0), lambda t: t.fused_mode() == 2,
                  lambda t: t.fused_mode() == 2, monkeypatch, ("k_chain8 / k_chain", ko, ka, B))


@pytest.mark.parametrize("ko,ka,B", SP1)
def test_eight_wave_backward_equals_four_wave_backward_bitwise(ko, ka, B, monkeypatch):
    _pair_bitwise("sac", ko, ka, B, dict(SAC_CHAIN=0, SAC_BWD8=1), dict(SAC_CHAIN=0, SAC_BWD8=0), lambda t: t.fused_mode() == 0,
                  lambda t: t.fused_mode() == 0, monkeypatch, ("k_bwd8 / k_bwd", ko, ka, B))


@pytest.mark.parametrize("ko,ka,B", SP1)
def test_backward_inside_the_chained_launch_equals_two_launches_bitwise(ko, ka, B, monkeypatch):
    _pair_bitwise("sac", ko, ka, B, dict(SAC_CHAIN_BWD=1), ts.CHAIN, lambda t: t.fused_mode() == 4, lambda t: t.fused_mode() == 2,
                  monkeypatch, ("kind 4 / kind 2", ko, ka, B))


def _group_against_solo_twins(algo, shapes, group_cls, monkeypatch, mixed=False):
    """Members from trained_nets with different lag seeds and noise seeds at B 128: each solo twin runs first and is
    released, then the group of the same members runs -- bit for bit the same."""
    B = 128
    solo = []
    for r, (ko, ka) in enumerate(shapes):
        t = _trainer(algo, ko, ka, B, {}, monkeypatch, noise_seed=50 + r, lag_seed=r)
        solo.append(_run(t, _buffer(ko, ka, 60 + r), B))
        t._destroy()
    members = [_trainer(algo, ko, ka, B, {}, monkeypatch, noise_seed=50 + r, lag_seed=r) for r, (ko, ka) in enumerate(shapes)]
    bufs = [_buffer(ko, ka, 60 + r) for r, (ko, ka) in enumerate(shapes)]
    group = group_cls(members)
    first, last = group.train_loop(bufs, STEPS, **(dict(batch_sizes=[B] * len(shapes)) if mixed else dict(batch_size=B)))
    assert not np.array_equal(solo[0]["last"], solo[1]["last"])
    for r, (t, buf) in enumerate(zip(members, bufs)):
        st = t.state_dict()
        k, p = buf.rng_state()
        got = {"first": first[r], "last": last[r], "scalars": np.array(st["scalars"]), "generator": np.asarray(k),
               "generator position": np.asarray([p])}
        for name, v in st["params"].items():
            got["params " + name] = v
        for name, (m, v) in st["opt"].items():
            got["exp_avg " + name], got["exp_avg_sq " + name] = m, v
        _same(got, solo[r], (algo, "member", r))


def test_sac_group_equals_its_solo_twins_bitwise(monkeypatch):
    from robosuite_benchmark_amd import SACTrainerGroup
    _group_against_solo_twins("sac", [(1, 1), (1, 1)], SACTrainerGroup, monkeypatch)


def test_td3_group_equals_its_solo_twins_bitwise(monkeypatch):
    from robosuite_benchmark_amd import TD3TrainerGroup
    _group_against_solo_twins("td3", [(1, 1), (1, 1)], TD3TrainerGroup, monkeypatch)


def test_mixed_sac_group_equals_its_solo_twins_bitwise(monkeypatch):
    from robosuite_benchmark_amd import MixedSACTrainerGroup
    _group_against_solo_twins("sac", [(1, 1), (3, 2)], MixedSACTrainerGroup, monkeypatch, mixed=True)
