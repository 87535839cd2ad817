"""CPU: the acting edge states of tests/edge_states.py (build_acting) do what they claim, in oracle.sac_step_torch.PolicyNet
at fp32 and float64 -- for every case and row count tests/test_gpu_acting_edges.py runs on the GPU.

Also the one property of the reference those GPU tests lean on: e32 = max|fp32 PolicyNet - float64 PolicyNet| per case.
In every case, `big` included, 8 x e32 <= 2e-5 (asserted), so both bounds of helpers.check_act apply everywhere: atol
2e-5 against the fp32 oracle and max(2e-5, 8 x e32) against float64.  And no pre-tanh value of any case lies between
Z_MODERATE and Z_SATURATED, where a == +-1.0f would hang on the last bit of a float32 tanh."""
import numpy as np
import pytest
import torch

from tests import edge_states as ES
from tests.helpers import ACT_ATOL, ACT_F64_FACTOR, act_reference

CASES = ES.acting_cases()
E32 = {}


case_id = ES.acting_case_id


def forward(layers, heads, obs, dtype):
    """Pre-activations of every hidden layer, and the heads' raw outputs, in `dtype`."""
    h = torch.from_numpy(obs).to(dtype)
    pre = []
    for w, b in layers[:len(layers) - heads]:
        pre.append(torch.nn.functional.linear(h, torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype)))
        h = torch.relu(pre[-1])
    out = [torch.nn.functional.linear(h, torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype)).numpy()
           for w, b in layers[len(layers) - heads:]]
    return [p.numpy() for p in pre], out


def test_the_matrix_is_the_one_the_issue_names():
    shapes = {(a, O, A, h) for _, a, O, A, h in CASES}
    for O, A in ES.ACT_SAC_DIMS:
        assert ("sac", O, A, (256, 256)) in shapes
    for h in ES.ACT_SAC_HIDDEN + ES.ACT_GENERAL_HIDDEN:
        assert ("sac", 42, 7, h) in shapes
    for A in (1, 7, 16):
        assert ("td3", 42, A, (256, 256)) in shapes
    for e in ES.ACTING_EDGES:
        assert (e, "sac", 42, 7, (256, 256)) in CASES
    for O, A in ES.ACT_SAC_DIMS:
        for e in ("clamp", "relu"):
            assert (e, "sac", O, A, (256, 256)) in CASES
    assert len(CASES) == len(set(CASES)) and len(CASES) >= 55
    assert ES.ACT_ROWS == (1, 16, 17, 1024)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_constructions_do_what_they_claim(case):
    edge, algo, O, A, hidden = case
    sac = algo == "sac"
    heads = 2 if sac else 1
    for n in ES.ACT_ROWS:
        layers, obs, eps, meta = ES.build_acting(edge, algo, O, A, hidden, n, seed=11)
        assert obs.shape == (n, O) and eps.shape == (n, A) and obs.dtype == eps.dtype == np.float32
        assert len(layers) == len(hidden) + heads and float(np.max(np.abs(eps))) <= 4.0
        for dtype in (torch.float32, torch.float64):
            pre, out = forward(layers, heads, obs, dtype)
            mean = out[0]
            zs = [mean]
            if sac:
                raw = out[1]
                zs.append(mean + np.exp(np.clip(raw, -20.0, 2.0)) * eps)
            for z in zs:                                 # nothing in the band where a == +-1.0f is undecided
                assert not np.any((np.abs(z) > ES.Z_MODERATE) & (np.abs(z) < ES.Z_SATURATED)), (n, dtype)
            if edge == "clamp":
                for c, b in meta["fixed_cols"].items():
                    assert np.all(raw[:, c] == b), (c, b)
                for c, bound in meta["clamped_cols"].items():        # beyond the bound on every row
                    assert np.all(raw[:, c] > bound) if bound > 0 else np.all(raw[:, c] < bound), c
                for c, bound in meta["boundary_cols"].items():       # exactly on it
                    assert np.all(raw[:, c] == bound), c
                for c, bound in meta["straddle_cols"].items():       # both sides, well apart
                    assert raw[:, c].min() < bound - 0.5 and raw[:, c].max() > bound + 0.5, (c, raw[:, c].min(), raw[:, c].max())
                if n >= 16:
                    assert sorted(meta["straddle_cols"]) == [c for c in (4, 5) if c < A]
                assert np.all(mean[:, meta["zero_mean_cols"]] == 0.0)
                assert sorted(meta["zero_mean_cols"]) == sorted(c for c in (1, 3, 5) if c < A and (c != 5 or 5 in meta["straddle_cols"]))
                b_mean, b_ls = layers[-2][1], layers[-1][1]          # distinct biases: a column mix-up shows
                rest = [c for c in range(A) if c not in meta["zero_mean_cols"]]
                assert len(set(b_mean[rest].tolist())) == len(rest) and len(set(b_ls.tolist())) == A
                assert np.all(b_mean != b_ls)
            elif edge == "tanh":
                assert sorted(meta["saturated_cols"]) == [c for c in (0, 1) if c < A]
                for z in zs:
                    for c, sign in meta["saturated_cols"].items():
                        assert np.all(z[:, c] * sign >= ES.Z_SATURATED), c
                if meta["stoch_col"] is not None:
                    c, rows = meta["stoch_col"], meta["stoch_rows"]
                    assert np.all(raw[:, c] == 2.0) and rows.size >= 1
                    assert np.all(zs[1][rows, c] * meta["stoch_signs"] >= ES.Z_SATURATED)
                    others = np.setdiff1d(np.arange(n), rows)
                    assert np.all(np.abs(zs[1][others, c]) < ES.Z_MODERATE)
                else:
                    assert not (sac and A >= 5)
            elif edge == "relu":
                zr = meta["zero_rows"]
                assert zr[0] == 0 and np.all(obs[zr] == 0.0) and np.all(eps[zr] == eps[0])
                n0 = pre[0].shape[1]
                zb = [u for u in meta["zero_bias_units"] if u < n0]
                dead = [u for u in meta["dead_units"] if u < n0]
                assert np.all(pre[0][np.ix_(zr, zb)] == 0.0)         # pre-activation exactly 0
                assert np.all(pre[0][:, dead] < 0.0)                 # dead on every row
                for p in pre[1:]:
                    assert np.all(p[:, [u for u in meta["zero_units_deep"] if u < p.shape[1]]] == 0.0)
                for z in zs:
                    assert np.all(z[zr] == z[0])
            elif edge == "big":
                assert np.std(obs) > 20 and np.all(np.abs(obs[:, meta["big_cols"]]).max(0) > 100)
        # what the GPU bounds rest on: the fp32 oracle's own distance from float64
        td3 = not sac
        e32 = 0.0
        for det in (True, False):
            w32, w64 = (act_reference(layers, td3, obs, det, eps, d) for d in (torch.float32, torch.float64))
            e32 = max(e32, float(np.max(np.abs(w32.astype(np.float64) - w64))))
            if edge == "tanh":                                       # the oracle itself gives the exact values claimed
                for c, sign in meta["saturated_cols"].items():
                    assert np.all(w32[:, c] == sign)
                if not det and meta["stoch_col"] is not None:
                    assert np.all(w32[meta["stoch_rows"], meta["stoch_col"]] == meta["stoch_signs"])
        E32[(case_id(case), n)] = e32
        print(f"{case_id(case)} n={n}: e32 = {e32:.3g}")
        assert ACT_F64_FACTOR * e32 <= ACT_ATOL, (n, e32)


def test_clamp_twin_differs_only_in_the_clamped_biases():
    """The bitwise twin the GPU tests act with: the clamped columns' log-std bias on the bound instead of beyond it."""
    layers, obs, eps, meta = ES.build_acting("clamp", "sac", 42, 7, (256, 256), 17, seed=11)
    twin = ES.clamp_twin(layers, meta)
    for (w, b), (w2, b2) in zip(layers[:-1], twin[:-1]):
        assert np.array_equal(w, w2) and np.array_equal(b, b2)
    assert np.array_equal(layers[-1][0], twin[-1][0])
    diff = np.nonzero(layers[-1][1] != twin[-1][1])[0].tolist()
    assert diff == sorted(meta["clamped_cols"]) and all(twin[-1][1][c] == meta["clamped_cols"][c] for c in diff)
    for det in (True, False):
        a, b = (act_reference(l, False, obs, det, eps, torch.float32) for l in (layers, twin))
        assert np.array_equal(a, b)
