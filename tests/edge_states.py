"""Edge states of one SAC / TD3 step (test infrastructure, used by tests/test_gpu_step_edges.py and checked on the CPU by
tests/test_oracle_float64.py): parameters and batches built so that the masked and saturating branches of the step run --
the log-std clamp, full tanh saturation, ReLU at an exactly-zero pre-activation, pad rows of a partial row-block next to
the statistics, an all-terminal batch.  At init none of them is reached.

Every builder returns an EdgeState: `nets` in the oracle's layout (init_sac_params / init_td3_params), the batch, the
noise, and `meta`, what the construction claims (checked against both oracles by the CPU tests)."""
from __future__ import annotations

import copy
from dataclasses import dataclass, field

import numpy as np

from oracle.sac_step_torch import init_sac_params
from oracle.td3_step_torch import init_td3_params

EDGES = ("clamp", "tanh", "relu", "pad", "terminal")
TD3_EDGES = ("tanh", "relu", "pad", "terminal")          # (TD3's policy has no log-std head)


@dataclass
class EdgeState:
    edge: str
    algo: str
    nets: dict
    obs: np.ndarray
    act: np.ndarray
    rew: np.ndarray
    term: np.ndarray
    nobs: np.ndarray
    eps: tuple                       # SAC: (eps1, eps2); TD3: (eps,)
    kw: dict = field(default_factory=dict)      # trainer kwargs the state needs
    meta: dict = field(default_factory=dict)

    def batch(self):
        return dict(observations=self.obs, actions=self.act, rewards=self.rew, terminals=self.term,
                    next_observations=self.nobs)

    def args(self):
        return (self.obs, self.act, self.rew, self.term, self.nobs, *self.eps)


def _base(algo, O, A, B, hidden, seed):
    nets = (init_sac_params(O, A, hidden=hidden, seed=seed) if algo == "sac" else init_td3_params(O, A, hidden=hidden, seed=seed))
    nets = copy.deepcopy(nets)
    rs = np.random.RandomState(seed + 100)
    obs = rs.normal(0, 0.5, (B, O)).astype(np.float32)
    nobs = rs.normal(0, 0.5, (B, O)).astype(np.float32)
    act = rs.uniform(-1, 1, (B, A)).astype(np.float32)
    rew = rs.uniform(0, 1, (B, 1)).astype(np.float32)
    term = (rs.uniform(0, 1, (B, 1)) < 0.1).astype(np.float32)
    eps = tuple(np.clip(rs.standard_normal((B, A)), -4, 4).astype(np.float32) for _ in range(2 if algo == "sac" else 1))
    return nets, obs, act, rew, term, nobs, list(eps)


def _fixed_rows(w, b, rows):
    """Head rows {row: bias} with zero weights: the output is the bias on every input."""
    for c, v in rows.items():
        w[c] = 0.0
        b[c] = v


def _relu_units(layers, heads):
    """The relu edge of one net: first-layer units 0..7 with bias 0, 8..11 dead (bias -100); in the deeper hidden layers
    units 0..5 with zero row and bias (as many of each as the layer has)."""
    for l in range(len(layers) - heads):
        w, b = layers[l]
        n = w.shape[0]
        if l == 0:
            b[[u for u in range(8) if u < n]] = 0.0
            b[[u for u in range(8, 12) if u < n]] = -100.0
        else:
            zu = [u for u in range(6) if u < n]
            w[zu] = 0.0
            b[zu] = 0.0


def build(edge, algo, O, A, B, hidden=(256, 256), seed=7):
    nets, obs, act, rew, term, nobs, eps = _base(algo, O, A, B, hidden, seed)
    kw, meta = {}, {}
    rs = np.random.RandomState(seed + 200)
    if edge == "clamp":
        # log-std head rows: W = 0 and bias exactly 2 / -20 (on the clamp's boundary: the gradient passes), 2.5 / -25
        # (clamped on every row: W and b get exactly 0), one row whose weights make raw straddle 2 across the batch.
        assert algo == "sac" and A >= 5
        wm, bm = nets["policy"][-2]
        wl, bl = nets["policy"][-1]
        _fixed_rows(wl, bl, {0: 2.0, 1: -20.0, 2: 2.5, 3: -25.0})
        _fixed_rows(wm, bm, {1: 0.0})    # the column at -20: a zero mean, so z = std * eps does not cancel against it
        wl[4] = rs.uniform(-1, 1, wl.shape[1]).astype(np.float32) * np.float32(4.0 / np.sqrt(wl.shape[1]))
        bl[4] = 2.0
        for e in eps:                # std = e^2 on columns 0, 2, 4: keep |z| below the ill-conditioned tanh band
            e[:, [0, 2, 4]] *= np.float32(0.15)
        meta.update(boundary_cols=[0, 1], clamped_cols=[2, 3], straddle_col=4)
    elif edge == "tanh":
        # mean-head biases +-15 (|z| >= 9.1 on every row: a = +-1.0f and the mean head's gradient is exactly 0), +-3
        last = -2 if algo == "sac" else -1
        wm, bm = nets["policy"][last]
        sat, mod = [0, 1], [2, 3]
        _fixed_rows(wm, bm, dict(zip(sat + mod, (15.0, -15.0, 3.0, -3.0))))
        if algo == "td3":
            wt, bt = nets["target_policy"][-1]
            wt[sat] = 0.0
            bt[sat] = bm[sat]
        else:
            for e in eps:
                e[:, mod] = np.clip(e[:, mod], -3.5, 3.5)      # |z| <= 6.5 on the moderate columns
        meta.update(saturated_cols=sat, moderate_cols=mod)
    elif edge == "relu":
        # rows with zero observations and actions; units with zero bias (pre-activation exactly 0 on those rows), units
        # dead on every row (bias -100); in the deeper layers units whose row and bias are zero (exactly 0 on every row)
        zero_rows = np.arange(0, B, 5)
        obs[zero_rows] = 0.0
        act[zero_rows] = 0.0
        nobs[zero_rows] = 0.0
        meta.update(zero_rows=zero_rows, zero_bias_units=list(range(0, 8)), dead_units=list(range(8, 12)),
                    zero_units_deep=list(range(0, 6)))
        for name, layers in nets.items():
            _relu_units(layers, (2 if algo == "sac" else 1) if "policy" in name else 1)
    elif edge == "pad":
        # odd B, non-negative weights, observations >= 0.5, actions >= 0: the nets are monotone, so a row computed on
        # zero inputs (a pad row of the last row-block) would fall outside the real rows' range of each statistic
        assert B % 2 == 1
        for name, layers in nets.items():
            nets[name] = [(np.abs(w), np.abs(b)) for w, b in layers]
        obs[:] = rs.uniform(0.5, 1.5, obs.shape).astype(np.float32)
        nobs[:] = rs.uniform(0.5, 1.5, nobs.shape).astype(np.float32)
        act[:] = rs.uniform(0.0, 1.0, act.shape).astype(np.float32)
    elif edge == "terminal":
        term[:] = 1.0
        kw["reward_scale"] = 3.0
    else:
        raise ValueError(edge)
    return EdgeState(edge, algo, nets, obs, act, rew, term, nobs, tuple(eps), kw, meta)


def pad_row_values(o64, st):
    """{statistic prefix: (value of a row computed on zero inputs -- observations, actions, noise, reward, terminal all 0 --
    by the float64 nets of `st`, the real rows' values from the float64 oracle `o64` after its step on `st`)}."""
    import torch
    from oracle.sac_step_torch import PolicyNet, QNet
    from oracle.td3_step_torch import TanhMlp
    f64 = torch.float64
    O, A = st.obs.shape[1], st.act.shape[1]
    zo, za = torch.zeros(1, O, dtype=f64), torch.zeros(1, A, dtype=f64)
    q = {k: QNet(st.nets[k], f64) for k in ("qf1", "qf2", "target_qf1", "target_qf2")}
    L, g = o64.last, o64.discount
    with torch.no_grad():
        out = {"Q1 Predictions": (q["qf1"](zo, za), L["q1"]), "Q2 Predictions": (q["qf2"](zo, za), L["q2"])}
        if st.algo == "sac":
            pol = PolicyNet(st.nets["policy"], f64)
            a, mu, log_std, log_pi, _ = pol(zo, za)
            alpha = o64.log_alpha.exp() if o64.auto_alpha else 1.0
            y = g * (torch.min(q["target_qf1"](zo, a), q["target_qf2"](zo, a)) - alpha * log_pi)
            out.update({"Q Targets": (y, L["y"]), "Log Pis": (log_pi, L["log_pi"]), "Policy mu": (mu, L["mu"]),
                        "Policy log std": (log_std, L["log_std"])})
        else:
            a2 = TanhMlp(st.nets["target_policy"], f64)(zo)
            y = g * torch.min(q["target_qf1"](zo, a2), q["target_qf2"](zo, a2))
            out.update({"Q Targets": (y, L["y"]), "Policy Action": (TanhMlp(st.nets["policy"], f64)(zo), L["pa"])})
    return {k: (v.detach().numpy().ravel(), r.detach().numpy().ravel()) for k, (v, r) in out.items()}


def pad_detectable(o64, st, margin=1e-3):
    """The statistics whose Max or Min a leaked zero-input row would change by more than `margin` of max|rows|:
    {prefix: "Max" / "Min"}."""
    got = {}
    for k, (pad, rows) in pad_row_values(o64, st).items():
        s = np.max(np.abs(rows))
        if np.all(pad > rows.max() + margin * s):
            got[k] = "Max"
        elif np.all(pad < rows.min() - margin * s):
            got[k] = "Min"
    return got


def structural_zeros(st, shapes, names, net):
    """{tensor name: boolean mask} of the gradient entries of `net` the construction makes exactly 0 in the fp32 oracle
    (a mask or a saturation removes them).  shapes / names: the net's layers as tests.helpers._net_info gives them."""
    out = {}

    def mark(layer, part, rows=None, cols=None):
        n, k = shapes[layer]
        key = f"{net} {names[layer]}.{part}"
        m = out.setdefault(key, np.zeros((n, k) if part == "weight" else (n,), bool))
        if part == "bias":
            m[rows] = True
        elif rows is not None:
            m[rows, :] = True
        else:
            m[:, cols] = True

    heads = (2 if st.algo == "sac" else 1) if net == "policy" else 1
    if st.edge == "clamp" and net == "policy":
        c = st.meta["clamped_cols"]
        mark(len(shapes) - 1, "weight", rows=c); mark(len(shapes) - 1, "bias", rows=c)
    elif st.edge == "tanh" and net == "policy":
        c, l = st.meta["saturated_cols"], len(shapes) - heads
        mark(l, "weight", rows=c); mark(l, "bias", rows=c)
    elif st.edge == "relu":
        for l in range(len(shapes) - heads):
            dead = [u for u in (range(8, 12) if l == 0 else range(6)) if u < shapes[l][0]]
            mark(l, "weight", rows=dead); mark(l, "bias", rows=dead)
            for nxt in ([l + 1] if l + 1 < len(shapes) - heads else range(len(shapes) - heads, len(shapes))):
                mark(nxt, "weight", cols=dead)
    return out


# ---- edge states of ACTING: the policy's forward alone (k_act, sac_policy_act) -----------------------------------------
# Used by tests/test_gpu_acting_edges.py; every claim in `meta` is checked against the fp32 and float64 PolicyNet by
# tests/test_acting_edges_host.py.
ACTING_EDGES = ("clamp", "tanh", "relu", "big")
TD3_ACTING_EDGES = ("tanh", "relu", "big")               # (TD3's policy has no log-std head)
# float32 tanh: 1 - tanh(z) = 2 exp(-2z) falls below half an ulp of 1 (2^-25) at |z| = 9.01, so beyond Z_SATURATED the
# correctly rounded action is exactly +-1.0f; between Z_MODERATE and Z_SATURATED whether a == +-1.0f depends on the last
# bit of the tanh at hand.  No construction puts a pre-tanh value into that band: exact claims never rest on it.
Z_SATURATED, Z_MODERATE = 9.1, 7.0
ACT_ROWS = (1, 16, 17, 1024)
ACT_SAC_DIMS = ((42, 1), (42, 8), (42, 9), (42, 16), (1, 7), (15, 7), (16, 7), (17, 7), (64, 4), (65, 4), (496, 16))
ACT_SAC_HIDDEN = ((100, 50), (7, 255), (255, 17), (1, 1))
ACT_GENERAL_HIDDEN = ((64, 96, 48), (512, 512))          # the general step: these act through sac_policy_act only


def acting_cases():
    """The edge matrix [(edge, algo, O, A, hidden)]: every edge at (42, 7, (256, 256)); clamp and relu at every head
    width, observation width and hidden size (tanh too where the head width or the hidden size changes); TD3 at
    A = 1, 7, 16 -- its policy has no log-std head, so where SAC's shapes take clamp and relu, TD3's take tanh and relu
    (every TD3 edge, big included, runs at A = 7); every edge on the general-step policies."""
    std = (256, 256)
    cases = [(e, "sac", 42, 7, std) for e in ACTING_EDGES] + [(e, "td3", 42, 7, std) for e in TD3_ACTING_EDGES]
    for O, A in ACT_SAC_DIMS:
        cases += [(e, "sac", O, A, std) for e in ("clamp", "relu") + (("tanh",) if O == 42 else ())]
    for hidden in ACT_SAC_HIDDEN:
        cases += [(e, "sac", 42, 7, hidden) for e in ("clamp", "relu", "tanh")]
    cases += [(e, "td3", 42, A, std) for A in (1, 16) for e in ("tanh", "relu")]
    cases += [(e, "sac", 42, 7, hidden) for hidden in ACT_GENERAL_HIDDEN for e in ACTING_EDGES]
    return cases


def acting_case_id(case):
    edge, algo, O, A, hidden = case
    return f"{edge}-{algo}-O{O}-A{A}-h{'x'.join(str(h) for h in hidden)}"


def _hidden64(layers, heads, obs):
    """The last hidden layer's activations in float64 (NumPy): what the head rows of a construction are fitted to."""
    h = np.asarray(obs, np.float64)
    for w, b in layers[:len(layers) - heads]:
        h = np.maximum(h @ np.asarray(w, np.float64).T + np.asarray(b, np.float64), 0.0)
    return h


def _straddle_row(h2, bound):
    """A head row whose output straddles `bound` across the rows of h2: weights along the direction in which the rows
    differ most (so the output is as well conditioned as the rows allow), scaled and shifted so that the outputs span
    [bound - 1, bound + 1].  None where the rows cannot be told apart (one row; a dead net)."""
    d = h2 - h2.mean(0)
    if h2.shape[0] < 2 or not np.max(np.abs(d)) > 0:
        return None
    w = np.linalg.svd(d, full_matrices=False)[2][0]
    raw = h2 @ w
    lo, hi = float(raw.min()), float(raw.max())
    if not hi - lo > 1e-6 * max(1.0, abs(lo), abs(hi)):
        return None
    s = 2.0 / (hi - lo)
    return (w * s).astype(np.float32), np.float32(bound - s * (lo + hi) / 2)


def build_acting(edge, algo, O, A, hidden=(256, 256), n=16, seed=7):
    """(layers, obs, eps, meta): a policy in the oracle's layout -- the hidden layers, last_fc, and for SAC
    last_fc_log_std -- with n observation rows (n, O) and N(0,1) draws (n, A) (|eps| <= 4) that make acting run the
    branches it never reaches at init, for A in 1..16 and any hidden sizes; `meta` holds what the construction claims.

    clamp  log-std rows with W = 0 and bias 2.5, -25 (clamped on every row), 2, -20 (on the bound), one row that
           straddles 2 and one that straddles -20 across the rows -- in that order over the columns that exist; a zero
           mean where the std is tiny (so z = std * eps is not absorbed); every other mean and log-std bias distinct
    tanh   mean rows with W = 0 and bias +15, -15 (a = +-1.0f exactly), +3, -3; SAC: a fifth column with mean 0.25 and
           log-std exactly 2 whose eps alternates between 2 <= |eps| <= 4 (saturated by exp(2) * eps) and |eps| <= 0.5
    relu   zero observation rows (all with one eps row); the unit pattern of build("relu")
    big    observations at scale 30, a few columns at 1e3; weights at init"""
    from oracle.sac_step_torch import init_mlp_params
    sac = algo == "sac"
    assert algo in ("sac", "td3") and 1 <= A <= 16 and O >= 1 and n >= 1, (algo, O, A, n)
    assert edge in (ACTING_EDGES if sac else TD3_ACTING_EDGES), (edge, algo)
    heads = 2 if sac else 1
    layers = [(w.copy(), b.copy()) for w, b in init_mlp_params(np.random.RandomState(seed), O, hidden, [A] * heads, 1e-3)]
    rs = np.random.RandomState(seed + 100)
    obs = rs.normal(0, 0.5, (n, O)).astype(np.float32)
    eps = np.clip(rs.standard_normal((n, A)), -4, 4).astype(np.float32)
    rs = np.random.RandomState(seed + 200)
    wm, bm = layers[len(layers) - heads]
    meta = {}
    if edge == "clamp":
        wl, bl = layers[-1]
        for c in range(A):                                   # distinct everywhere: a column mix-up changes the answer
            bm[c] = np.float32(0.05 * (c + 1) * (-1) ** c)
            bl[c] = np.float32(-0.25 * (c - 5) - 0.125)
        fixed = {c: b for c, b in enumerate((2.5, -25.0, 2.0, -20.0)) if c < A}
        _fixed_rows(wl, bl, fixed)
        bounds = {c: (2.0 if b > 0 else -20.0) for c, b in fixed.items()}
        straddle, h2 = {}, _hidden64(layers, heads, obs)
        for c, bound in ((4, 2.0), (5, -20.0)):
            row = _straddle_row(h2, bound) if c < A else None
            if row is not None:
                wl[c], bl[c] = row
                straddle[c] = bound
                bounds[c] = bound
        low = [c for c, b in bounds.items() if b < 0]
        _fixed_rows(wm, bm, {c: 0.0 for c in low})
        eps[:, [c for c, b in bounds.items() if b > 0]] *= np.float32(0.15)       # std = e^2: |z| <= 4.5 + |mean|
        meta.update(fixed_cols=fixed, clamped_cols={c: bounds[c] for c, b in fixed.items() if b in (2.5, -25.0)},
                    boundary_cols={c: bounds[c] for c, b in fixed.items() if b in (2.0, -20.0)}, straddle_cols=straddle,
                    zero_mean_cols=low)
    elif edge == "tanh":
        want = {c: b for c, b in enumerate((15.0, -15.0, 3.0, -3.0)) if c < A}
        _fixed_rows(wm, bm, want)
        sat = {c: np.float32(np.sign(b)) for c, b in want.items() if abs(b) == 15.0}
        mod = [c for c, b in want.items() if abs(b) == 3.0]
        eps[:, mod] = np.clip(eps[:, mod], -3.5, 3.5)        # |z| <= 6.5 + |std - 1| * 3.5 on the moderate columns
        meta.update(saturated_cols=sat, moderate_cols=mod, stoch_col=None)
        if sac and A >= 5:
            _fixed_rows(wm, bm, {4: 0.25})
            _fixed_rows(layers[-1][0], layers[-1][1], {4: 2.0})
            rows = np.arange(0, n, 2)
            eps[:, 4] = rs.uniform(-0.5, 0.5, n).astype(np.float32)
            eps[rows, 4] = (rs.uniform(2, 4, rows.size) * rs.choice([-1.0, 1.0], rows.size)).astype(np.float32)
            meta.update(stoch_col=4, stoch_rows=rows, stoch_signs=np.sign(eps[rows, 4]).astype(np.float32))
    elif edge == "relu":
        zero_rows = np.arange(0, n, 5)
        obs[zero_rows] = 0.0
        eps[zero_rows] = eps[0]
        _relu_units(layers, heads)
        meta.update(zero_rows=zero_rows, zero_bias_units=list(range(0, 8)), dead_units=list(range(8, 12)),
                    zero_units_deep=list(range(0, 6)))
    elif edge == "big":
        cols = sorted({0, O // 2, O - 1})
        obs[:] = rs.normal(0, 30.0, obs.shape).astype(np.float32)
        obs[:, cols] = rs.normal(0, 1e3, (n, len(cols))).astype(np.float32)
        meta.update(big_cols=cols)
    return layers, obs, eps, meta


def clamp_twin(layers, meta):
    """The clamp policy with the log-std bias of its clamped columns set exactly ON the bound (2.5 -> 2, -25 -> -20):
    with the clamp in place both policies act the same, bit for bit."""
    twin = [(w.copy(), b.copy()) for w, b in layers]
    for c, bound in meta["clamped_cols"].items():
        twin[-1][1][c] = bound
    return twin
