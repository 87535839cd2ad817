"""CPU: the trained-regime states of tests/trained_states.py -- distinct targets, inflation that keeps what the networks
compute, and, from the fp32 and float64 oracles on every (state, batch) the GPU tests use, that each of them is inside the
regime (large Q, a_new saturated to exactly +-1, log_std on its clamp) and can see a mix-up of target and online nets.
Exports ill_conditioned(): the logged statistics on which the fp32 oracle itself is farther from float64 than the 1e-5
rule allows a kernel to be from it; tests/test_gpu_trained_paths.py may hold only those to the float64 rule alone."""
import functools

import numpy as np
import pytest
import torch

from oracle.sac_step_torch import RlkitEquivalentSAC
from oracle.td3_step_torch import RlkitEquivalentTD3
from tests import trained_states as ts
from tests.helpers import F64_FACTOR, rel_err

KW = {"sac": dict(policy_lr=1e-3, qf_lr=5e-4, soft_target_tau=0.005, target_update_period=5),
      "td3": dict(policy_learning_rate=1e-3, qf_learning_rate=5e-4)}
ROW_TOL = 2e-5                   # the per-row bound of tests/test_gpu_td3.py on q_target, tq1, tq2: rel_err < 2e-5
STAT_TOL = 1e-5                  # logged scalars: |a - b| <= 1e-5 max(1, |b|)


def oracle_of(algo, nets, dtype=torch.float32):
    return (RlkitEquivalentSAC if algo == "sac" else RlkitEquivalentTD3)(nets, len(nets["policy"][-1][1]), dtype=dtype, **KW[algo])


def step(o, algo, batch, eps):
    return o.step(*ts.batch_args(batch), *(eps if algo == "sac" else eps[:1]))


def ill_conditioned(want32, want64):
    """{statistic: d} where d = |P - R| / max(1, |R|), the fp32 oracle's relative distance to float64, times the project's
    factor 8 exceeds 1e-5: decided by the two references alone."""
    out = {}
    for name, r in want64.items():
        d = abs(want32[name] - r) / max(1.0, abs(r))
        if F64_FACTOR * d > STAT_TOL:
            out[name] = d
    return out


def ill_conditioned_rows(o32, o64, keys=("y", "tq1", "tq2")):
    """The same for the per-row target values (oracle.last keys): {key: d} where d = rel_err(P, R) over the rows, times 8,
    exceeds the per-row bound 2e-5."""
    out = {}
    for key in keys:
        if key in o64.last:
            d = rel_err(o32.last[key].detach().numpy(), o64.last[key].detach().numpy())
            if F64_FACTOR * d > ROW_TOL:
                out[key] = d
    return out


@functools.lru_cache(maxsize=None)
def references(algo, ko, ka, B):
    nets, batch, eps = ts.state(algo, ko, ka, B)
    o32, o64 = oracle_of(algo, nets), oracle_of(algo, nets, torch.float64)
    want32, want64 = step(o32, algo, batch, eps), step(o64, algo, batch, eps)
    swapped = oracle_of(algo, ts.with_online_targets(nets))
    step(swapped, algo, batch, eps)
    return o32, o64, want32, want64, swapped


STATES = ts.gpu_states()
IDS = ["%s-%dx%d-B%d" % s for s in STATES]


# ---- the states themselves -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_no_target_tensor_equals_its_online_tensor(algo):
    for seed in (0, 1):
        nets = ts.trained_nets(algo, seed=seed)
        assert list(nets) == ["qf1", "qf2", "target_qf1", "target_qf2", "policy"] + (["target_policy"] if algo == "td3" else [])
        for name in nets:
            if not name.startswith("target_"):
                continue
            for (wt, bt), (w, b) in zip(nets[name], nets[name[len("target_"):]]):
                assert wt.dtype == bt.dtype == np.float32 and wt.shape == w.shape
                assert not np.array_equal(wt, w) and not np.array_equal(bt, b), name
                assert np.all(np.abs(wt - w) <= 1.01 * ts.LAG * np.abs(w)) and np.mean(wt != w) > 0.9
    a, b = ts.trained_nets(algo, seed=0), ts.trained_nets(algo, seed=1)
    assert not np.array_equal(a["target_qf1"][0][0], b["target_qf1"][0][0])          # the lag is seeded
    assert np.array_equal(a["target_qf1"][0][0], ts.trained_nets(algo, seed=0)["target_qf1"][0][0])
    on = ts.trained_nets(algo, targets="online")
    assert np.array_equal(on["target_qf2"][1][0], on["qf2"][1][0])
    if algo == "td3":                                       # the fixture's policy without its log_std head
        sac = ts.trained_nets("sac")
        assert len(a["policy"]) == 3 and np.array_equal(a["policy"][2][0], sac["policy"][2][0])


@pytest.mark.parametrize("algo", ["sac", "td3"])
@pytest.mark.parametrize("ko,ka", [(3, 2), (2, 1)])
def test_inflated_networks_compute_what_the_fixture_computes(algo, ko, ka):
    nets = ts.trained_nets(algo)
    big = ts.inflate(nets, ko, ka, seed=1)
    O, A = ts.O0 * ko, ts.A0 * ka
    for name, layers in big.items():
        w0 = layers[0][0]
        src = nets[name][0][0]
        if "policy" in name:
            assert w0.shape == (256, O)
            for h in layers[len(ts.HIDDEN):]:
                assert h[0].shape == (A, 256) and h[1].shape == (A,)
                assert np.array_equal(h[0][:ts.A0], h[0][-ts.A0:])
            folded = w0.astype(np.float64).reshape(256, ko, ts.O0).sum(axis=1)
        else:
            assert w0.shape == (256, O + A) and layers[-1][0].shape == (1, 256)
            folded = np.concatenate([w0[:, :O].astype(np.float64).reshape(256, ko, ts.O0).sum(axis=1),
                                     w0[:, O:].astype(np.float64).reshape(256, ka, ts.A0).sum(axis=1)], axis=1)
        # the shares of a column sum to 1: folding the split columns gives the column back, to fp32 rounding of each share
        assert np.all(np.abs(folded - src) <= ko * 2.0 ** -23 * np.abs(src)), name
        if ko > 1:
            assert not np.array_equal(w0[:, :ts.O0], w0[:, ts.O0:2 * ts.O0])         # shares, not copies
    # on tiled rows the Q nets give the fixture's Q
    B = 64
    small, _ = ts.trained_batch(ts.O0, ts.A0, B)
    tiled, eps = ts.trained_batch(ts.O0, ts.A0, B, ko, ka)
    assert tiled["observations"].shape == (B, O) and tiled["actions"].shape == (B, A) and eps[0].shape == (B, A)
    assert np.array_equal(tiled["observations"][:, -ts.O0:], small["observations"])
    from oracle.sac_step_torch import QNet
    t = torch.from_numpy
    with torch.no_grad():
        q = QNet(nets["qf1"], torch.float64)(t(small["observations"]).double(), t(small["actions"]).double()).numpy()
        qb = QNet(big["qf1"], torch.float64)(t(tiled["observations"]).double(), t(tiled["actions"]).double()).numpy()
    assert rel_err(qb, q) < 1e-4 and abs(q.mean()) > 50


# ---- every (state, batch) of the GPU tests: inside the regime, and it sees swapped targets ---------------------------------
@pytest.mark.parametrize("state", STATES, ids=IDS)
def test_gpu_case_is_inside_the_trained_regime(state):
    algo, ko, ka, B = state
    o32, o64, want32, want64, _ = references(*state)
    assert abs(want32["Q1 Predictions Mean"]) > 1.0 and abs(want64["Q1 Predictions Mean"]) > 1.0
    a_new = o32.last["a_new" if algo == "sac" else "pa"].detach().numpy()
    sat = float(np.mean(np.abs(a_new) == 1.0))
    print(f"{state}: Q1 mean {want32['Q1 Predictions Mean']:.4g}, a_new exactly +-1: {sat:.3f}", end="")
    assert a_new.shape == (B, ts.A0 * ka) and sat >= 0.05, sat
    if algo == "sac":
        clamp = float(np.mean(o32.last["log_std"].detach().numpy() == 2.0))
        print(f", log_std on the clamp: {clamp:.3f}, |a| > 0.999: {float(np.mean(np.abs(a_new) > 0.999)):.3f}", end="")
        assert clamp >= 0.01, clamp
    print("; fp32 oracle farther than 1e-5 / 8 from float64 on:", ill_conditioned(want32, want64),
          "and than 2e-5 / 8 on the rows of:", ill_conditioned_rows(o32, o64))


@pytest.mark.parametrize("state", STATES, ids=IDS)
def test_swapping_targets_for_online_nets_moves_the_target_values(state):
    algo = state[0]
    o32, _, _, _, swapped = references(*state)
    for key in ("y",) + (("tq1", "tq2") if algo == "td3" else ()):
        moved = rel_err(swapped.last[key].detach().numpy(), o32.last[key].detach().numpy())
        print(f"{state}: {key} moves by {moved:.3g} (rel_err) when the targets are the online nets; the bound is {ROW_TOL}")
        assert moved > ROW_TOL, (key, moved)


def test_ill_conditioned_set_follows_the_two_references():
    r = {"a": 100.0, "b": 0.5, "c": -3.0}
    p = {"a": 100.0 + 100.0 * 1.3e-6, "b": 0.5 + 1.2e-6, "c": -3.0 - 3.0 * 1.26e-6}
    assert set(ill_conditioned(p, r)) == {"a", "c"}                 # 8 d > 1e-5 where d > 1.25e-6
    assert ill_conditioned(r, r) == {}


# ---- every row of the path table selects the path it names (the library's own step plan, on the host) ---------------------
from tests.test_step_plan_host import lib, plan  # noqa: E402,F401  (the plan wrapper's fixture)


@pytest.mark.parametrize("path", ts.PATHS, ids=[p[0] for p in ts.PATHS])
def test_path_table_rows_select_their_paths(lib, path):  # noqa: F811
    label, algo, env, (ko, ka, B), kind = path
    if env.get("SAC_GENERAL"):
        return                                               # the general step is chosen outside the plan
    env = {k: v for k, v in env.items() if k != "SAC_ROW_IMAGES"}
    p = plan(lib, ts.O0 * ko, ts.A0 * ka, B, algo=int(algo == "td3"), **env)
    assert p["ok"] == 1
    if algo == "sac":
        assert p["kind"] in (kind if isinstance(kind, tuple) else (kind,)), p["kind"]
    else:
        assert bool(p["fused"]) == kind, p
    want = {"four-launch SP 4": dict(SP=4), "four-launch SP 2": dict(SP=2, compact=1),
            "four-launch SP 2 compact 0": dict(SP=2, compact=0), "four-launch SP 1 k_bwd8": dict(SP=1, bwd8=1),
            "four-launch SP 1 k_bwd": dict(SP=1, bwd8=0), "chained": dict(chain8=1), "chained four-wave": dict(chain8=0),
            "fused padded": dict(dw_one=1), "fused loop-form dW": dict(dw_one=0), "inflated 126/14 fused": dict(wide=1, nth=2),
            "inflated 84/7 fused": dict(wide=0), "td3 four-launch SP 4": dict(SP=4), "td3 four-launch SP 2": dict(SP=2),
            "td3 four-launch SP 1": dict(SP=1)}.get(label, {})
    for k, v in want.items():
        assert p[k] == v, (label, k, p[k])


@pytest.mark.parametrize("ko,ka,B", [(1, 1, 530), (2, 1, 544)])
def test_bitwise_pairs_select_both_kernels_of_each_pair(lib, ko, ka, B):  # noqa: F811
    """The pairs tests/test_gpu_trained_paths.py holds bit for bit at column split 1 really are two kernels."""
    O, A = ts.O0 * ko, ts.A0 * ka
    for c8 in (0, 1):
        p = plan(lib, O, A, B, SAC_CHAIN8=c8, **ts.CHAIN)
        assert (p["kind"], p["chain8"], p["SP"]) == (2, c8, 1), p
    for b8 in (0, 1):
        p = plan(lib, O, A, B, SAC_CHAIN=0, SAC_BWD8=b8)
        assert (p["kind"], p["bwd8"], p["SP"]) == (0, b8, 1), p
    assert plan(lib, O, A, B, SAC_CHAIN_BWD=1)["kind"] == 4
