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
        for c, b in ((0, 2.0), (1, -20.0), (2, 2.5), (3, -25.0)):
            wl[c] = 0.0
            bl[c] = b
        wm[1] = 0.0                  # the column at -20: a zero mean, so z = std * eps does not cancel against it
        bm[1] = 0.0
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
        for c, b in zip(sat + mod, (15.0, -15.0, 3.0, -3.0)):
            wm[c] = 0.0
            bm[c] = b
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
            heads = (2 if algo == "sac" else 1) if "policy" in name else 1
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
