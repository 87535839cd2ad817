"""The float64 twin of the oracle and the per-tensor checker built on it (tests/helpers.py check_f64), on the CPU.

The GPU parity tests compare every weight / bias gradient, per-row output and logged statistic of a step with the float64
oracle at the tensor's own scale, allowing 8x the fp32 oracle's own distance to float64 (floor 1e-5).  These tests pin
that the yardstick is the same step (bitwise the default in fp32, within 1e-5 per tensor in float64 at init) and that
the checker rejects a gradient the whole-vector bound accepted."""
import numpy as np
import pytest
import torch

from oracle.sac_step_torch import QNet, RlkitEquivalentSAC, init_sac_params
from oracle.td3_step_torch import RlkitEquivalentTD3, init_td3_params
from tests.helpers import (TASK_DIMS, _net_info, check_f64, named_tensors, oracle_flat_grad, synth_transitions)


def _batch(B, O, A, seed, term_frac=0.1):
    obs, act, rew, term, nobs = synth_transitions(B, O, A, seed=seed, term_frac=term_frac)
    rs = np.random.RandomState(seed + 1)
    e1, e2 = rs.standard_normal((B, A)).astype(np.float32), rs.standard_normal((B, A)).astype(np.float32)
    return (obs, act, rew, term.astype(np.float32), nobs), (e1, e2)


def _sac(O, A, dtype=None, seed=11, **kw):
    nets = init_sac_params(O, A, seed=seed, hidden=kw.pop("hidden", (256, 256)), hidden_q=kw.pop("hidden_q", None))
    return RlkitEquivalentSAC(nets, A, policy_lr=1e-3, qf_lr=5e-4, **({} if dtype is None else {"dtype": dtype}), **kw)


def test_explicit_float32_is_the_default_bit_for_bit():
    O, A, B = 42, 7, 64
    a, b = _sac(O, A), _sac(O, A, torch.float32)
    for s in range(3):
        data, eps = _batch(B, O, A, 40 + s)
        da, db = a.step(*data, *eps), b.step(*data, *eps)
        assert da == db
        for k in ("a_new", "log_pi", "q1", "y", "log_pi2"):
            assert torch.equal(a.last[k], b.last[k]) and a.last[k].dtype == torch.float32, k
        for k in ("g_policy", "g_qf1", "g_qf2"):
            assert all(np.array_equal(x, y) for x, y in zip(a.last[k], b.last[k])), k
    nets = init_td3_params(O, A, seed=2)
    t1, t2 = RlkitEquivalentTD3(nets, A), RlkitEquivalentTD3(nets, A, dtype=torch.float32)
    for s in range(2):
        data, eps = _batch(B, O, A, 60 + s)
        assert t1.step(*data, eps[0]) == t2.step(*data, eps[0])
        assert np.array_equal(t1.last["g_qf1"], t2.last["g_qf1"])


def _sac_pair_errors(O, A, B, **kw):
    o32, o64 = _sac(O, A, **kw), _sac(O, A, torch.float64, **kw)
    data, eps = _batch(B, O, A, 21)
    w32, w64 = o32.step(*data, *eps), o64.step(*data, *eps)
    assert o64.last["q1"].dtype == torch.float64 and o64.log_alpha.dtype == torch.float64
    errs = {}
    for net in ("policy", "qf1", "qf2"):
        shapes, names = _net_info(o32, net)
        P = named_tensors(oracle_flat_grad(o32.last["g_" + net]), shapes, names, net)
        R = named_tensors(oracle_flat_grad(o64.last["g_" + net]), shapes, names, net)
        for k in R:
            errs[k] = np.max(np.abs(P[k] - R[k])) / np.max(np.abs(R[k]))
    for k in ("q1", "q2", "q1_new", "q2_new", "y", "log_pi", "log_pi2", "a_new", "mu", "log_std", "a2"):
        R = o64.last[k].detach().numpy()
        errs[k] = np.max(np.abs(o32.last[k].detach().numpy() - R)) / np.max(np.abs(R))
    return errs, w32, w64


@pytest.mark.parametrize("task,B,kw", [("Lift", 256, {}), ("Door", 1024, {}), ("Wipe", 128, {}),
                                       ("Lift", 40, dict(hidden=(32,) * 7, hidden_q=(48,) * 7)),
                                       ("TwoArmLift", 64, dict(hidden=(64, 64, 64, 64), hidden_q=(400, 300)))])
def test_float32_and_float64_oracles_agree_at_init(task, B, kw):
    O, A = TASK_DIMS[task]
    errs, w32, w64 = _sac_pair_errors(O, A, B, **kw)
    worst = max(errs, key=errs.get)
    assert errs[worst] <= 1e-5, (worst, errs[worst])
    for k in w64:
        assert abs(w32[k] - w64[k]) <= 1e-5 * max(1e-3, abs(w64[k])), k


def test_td3_float32_and_float64_oracles_agree_at_init():
    O, A, B = 46, 7, 256
    nets = init_td3_params(O, A, seed=3)
    o32, o64 = RlkitEquivalentTD3(nets, A), RlkitEquivalentTD3(nets, A, dtype=torch.float64)
    data, eps = _batch(B, O, A, 5)
    o32.step(*data, eps[0]); o64.step(*data, eps[0])
    for net in ("policy", "qf1", "qf2"):
        shapes, names = _net_info(o32, net)
        P = named_tensors(o32.last["g_" + net], shapes, names, net)
        R = named_tensors(o64.last["g_" + net], shapes, names, net)
        for k in R:
            assert np.max(np.abs(P[k] - R[k])) <= 1e-5 * np.max(np.abs(R[k])), k


def _qf1_fc0_grad_without_last_rows(O, A, B, drop):
    """The fp32 oracle's qf1 fc0 weight gradient dZ^T X with the last `drop` batch rows left out -- what a weight-gradient
    reduction that loses the last row-block computes -- next to the oracle's own gradients (fp32 and float64)."""
    nets = init_sac_params(O, A, seed=11)
    o32 = RlkitEquivalentSAC(nets, A, policy_lr=1e-3, qf_lr=5e-4)
    o64 = RlkitEquivalentSAC(nets, A, policy_lr=1e-3, qf_lr=5e-4, dtype=torch.float64)
    data, eps = _batch(B, O, A, 21)
    o32.step(*data, *eps); o64.step(*data, *eps)
    q = QNet(nets["qf1"])                                    # the pre-step qf1, pre-activation of fc0 kept
    x = torch.cat([torch.from_numpy(data[0]), torch.from_numpy(data[1])], dim=1)
    z0 = torch.nn.functional.linear(x, q.ws[0], q.bs[0])
    z0.retain_grad()
    h = torch.relu(torch.nn.functional.linear(torch.relu(z0), q.ws[1], q.bs[1]))
    q1 = torch.nn.functional.linear(h, q.ws[2], q.bs[2])
    torch.mean((q1 - o32.last["y"]) ** 2).backward()
    dz = z0.grad
    full = (dz.T @ x).numpy()
    assert np.max(np.abs(full - o32.last["g_qf1"][0])) <= 1e-6 * np.max(np.abs(full))     # really the oracle's dZ^T X
    bad = [g.copy() for g in o32.last["g_qf1"]]
    bad[0] = (dz[:B - drop].T @ x[:B - drop]).numpy()
    return o32, o64, bad


@pytest.mark.parametrize("task,B,drop", [("Lift", 250, 10), ("Door", 1024, 16)])
def test_checker_rejects_a_gradient_missing_its_last_row_block(task, B, drop):
    O, A = TASK_DIMS[task]
    o32, o64, bad = _qf1_fc0_grad_without_last_rows(O, A, B, drop)
    ref32, flat_bad = oracle_flat_grad(o32.last["g_qf1"]), oracle_flat_grad(bad)
    # the whole-vector bound the parity tests keep passes this gradient ...
    assert np.max(np.abs(flat_bad - ref32)) <= 5e-5 * np.max(np.abs(ref32))
    # ... the per-tensor one names the tensor
    shapes, names = _net_info(o32, "qf1")
    K = named_tensors(flat_bad, shapes, names, "qf1")
    P = named_tensors(ref32, shapes, names, "qf1")
    R = named_tensors(oracle_flat_grad(o64.last["g_qf1"]), shapes, names, "qf1")
    with pytest.raises(AssertionError, match="qf1 fc0.weight"):
        for k in R:
            check_f64("gradient of " + k, K[k], P[k], R[k])
    for k in R:                                              # and passes every other tensor, and the oracle's own
        check_f64(k, P[k], P[k], R[k])
        if k != "qf1 fc0.weight":
            check_f64(k, K[k], P[k], R[k])


def test_checker_rules():
    R = np.array([1.0, -2.0, 0.5])
    P = R + np.array([1e-7, 0, 0])
    check_f64("t", R + 1e-5, P, R)                           # within the floor (1e-5 of max|R| = 2e-5 absolute)
    with pytest.raises(AssertionError, match="t:"):
        check_f64("t", R + 1e-4, P, R)
    check_f64("t", R + 5e-6 * 2 * 8, R + 1e-5 * 2, R)        # 8x the fp32 oracle's error
    check_f64("z", np.zeros(3), np.zeros(3), np.zeros(3))
    check_f64("z", -np.zeros(3), np.zeros(3), np.zeros(3))
    with pytest.raises(AssertionError, match="exactly 0"):
        check_f64("z", np.array([0, 1e-30, 0]), np.zeros(3), np.zeros(3))
    with pytest.raises(AssertionError):
        check_f64("n", R * np.nan, P, R)


# ---- the edge states of tests/edge_states.py produce what they claim, in both oracles --------------------------------
from tests.edge_states import EDGES, TD3_EDGES, build, pad_detectable, structural_zeros  # noqa: E402

EDGE_SHAPES = [((256, 256), 255), ((64, 96, 48), 129)]


def _oracles(st):
    A = st.act.shape[1]
    cls = RlkitEquivalentSAC if st.algo == "sac" else RlkitEquivalentTD3
    o32, o64 = cls(st.nets, A, **st.kw), cls(st.nets, A, dtype=torch.float64, **st.kw)
    o32.step(*st.args()); o64.step(*st.args())
    return o32, o64


def _named_grads(o, net):
    shapes, names = _net_info(o, net)
    return named_tensors(oracle_flat_grad(o.last["g_" + net]), shapes, names, net)


@pytest.mark.parametrize("hidden,B", EDGE_SHAPES)
@pytest.mark.parametrize("algo,edge", [("sac", e) for e in EDGES] + [("td3", e) for e in TD3_EDGES])
def test_edge_builders_produce_what_they_claim(algo, edge, hidden, B):
    st = build(edge, algo, 42, 7, B, hidden=hidden)
    o32, o64 = _oracles(st)
    n_zero = 0
    for net in ("policy", "qf1", "qf2"):               # the structural zeros are exactly 0 (float64 too, but at saturation)
        for k, z in structural_zeros(st, *_net_info(o32, net), net).items():
            n_zero += int(z.sum())
            assert np.all(_named_grads(o32, net)[k][z] == 0), k
            if edge != "tanh":
                assert np.all(_named_grads(o64, net)[k][z] == 0), k
    assert (n_zero > 0) == (edge in ("clamp", "tanh", "relu")), n_zero
    for o in (o32, o64):
        L = o.last
        if edge == "clamp":
            ls = L["log_std"].detach().numpy()
            assert np.all(ls[:, 0] == 2.0) and np.all(ls[:, 2] == 2.0) and np.all(ls[:, 1] == -20.0) and np.all(ls[:, 3] == -20.0)
            assert np.any(ls[:, 4] == 2.0) and np.any(ls[:, 4] < 2.0)         # the straddling row
            g = _named_grads(o, "policy")
            gw, gb = g["policy last_fc_log_std.weight"], g["policy last_fc_log_std.bias"]
            assert np.all(gw[[2, 3]] == 0) and np.all(gb[[2, 3]] == 0)         # clamped on every row
            assert np.all(gb[[0, 1, 4]] != 0)                                    # the boundary passes the gradient
            assert np.max(np.abs(L["z"].detach().numpy()[:, [0, 2, 4]])) < 7.0
            assert np.all(L["mu"].detach().numpy()[:, 1] == 0)
        elif edge == "tanh":
            z = (L["z"] if algo == "sac" else None)
            a = (L["a_new"] if algo == "sac" else L["pa"]).detach().numpy()
            sat, mod = st.meta["saturated_cols"], st.meta["moderate_cols"]
            if algo == "sac":
                z = z.detach().numpy()
                assert np.min(np.abs(z[:, sat])) >= 9.1 and np.max(np.abs(z[:, mod])) <= 7.0
            if o is o32:
                assert np.all(np.abs(a[:, sat]) == 1.0)
                g = _named_grads(o, "policy")
                assert np.all(g["policy last_fc.weight"][sat] == 0) and np.all(g["policy last_fc.bias"][sat] == 0)
                assert np.all(g["policy last_fc.bias"][mod] != 0)
        elif edge == "relu":
            zr = st.meta["zero_rows"]
            assert np.all(st.obs[zr] == 0) and np.all(st.act[zr] == 0)
            for net in ("policy", "qf1", "qf2"):
                g = _named_grads(o, net)
                assert np.all(g[f"{net} fc0.weight"][8:12] == 0) and np.all(g[f"{net} fc0.bias"][8:12] == 0)   # dead
                assert np.all(g[f"{net} fc1.weight"][:, 8:12] == 0)
                assert np.all(g[f"{net} fc0.bias"][:8] != 0)                                # zero bias: alive elsewhere
                assert np.all(g[f"{net} fc1.weight"][:6] == 0) and np.all(g[f"{net} fc1.bias"][:6] == 0)   # exactly-0 units
            # the pre-activations really are exactly 0: fc0 of the zero-bias units on the zero rows, fc1's on every row
            for net in ("policy", "qf1", "qf2"):
                (w0, b0), (w1, b1) = st.nets[net][:2]
                x = st.obs if net == "policy" else np.concatenate([st.obs, st.act], axis=1)
                z0 = x.astype(np.float64) @ w0.T + b0
                z1 = np.maximum(z0, 0) @ w1.T + b1
                assert np.all(z0[zr, :8] == 0) and np.all(z0[:, 8:12] < -50) and np.all(z1[:, :6] == 0)
        elif edge == "pad":
            want = {"Q1 Predictions", "Q2 Predictions"} | ({"Policy mu", "Policy log std"} if algo == "sac" else {"Policy Action"})
            if o is o64:
                assert want <= set(pad_detectable(o64, st)), pad_detectable(o64, st)
        elif edge == "terminal":
            y = L["y"].detach().numpy().ravel()
            if o is o32:
                assert np.array_equal(y, np.float32(3.0) * st.rew.ravel())
