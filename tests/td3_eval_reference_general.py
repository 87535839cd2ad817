"""Reference of TD3Trainer.evaluate_td3 for nets of ANY depth (test infrastructure; imports oracle/): the layers of every
net from flat parameter vectors in library layout (state_dict()["params"]) -- the policy and the target policy
hidden..., (A, last), a Q net hidden..., (1, last) -- handed to tests.td3_eval_reference.evaluate_reference in float32 and
float64.  Bound of every column: helpers.check_f64 as it stands, max|K - R| / max|R| <= max(8 max|P - R| / max|R|, 1e-5),
K == 0 where R == 0, on inputs at which max|R| is a meaningful unit (conditioned_inputs: the rules of
tests/td3_eval_reference.py, chosen from the float64 reference alone)."""
from collections import OrderedDict

import numpy as np
import torch

from tests.helpers import check_f64, layers_from_flat
from tests.td3_eval_reference import COLUMNS, CONDITIONED, Q_NETS, evaluate_reference, inputs

# policy hidden sizes, critic hidden sizes (None: the policy's), O, A
SHAPES = [((512, 512), None, 42, 7),               # baseline general shape
          ((256, 256, 256), None, 42, 7),          # three hidden layers
          ((1,), None, 17, 5),                     # width 1
          ((257,), None, 48, 16),                  # a full 16-column head; first Q K of 64
          ((300, 7, 129), None, 379, 6),           # first Q K of 385
          ((64, 96, 48), None, 122, 6),            # first Q K of 128: exactly one chunk
          ((64, 96, 48), None, 123, 6),            # first Q K of 129
          ((16,), None, 1, 1),                     # head of 1 column
          ((64,) * 7, None, 42, 7),                # depth 7
          ((4096,), None, 42, 7),                  # widest layer
          ((64, 64, 64), (512, 512), 42, 7),       # policy deeper than the critics
          ((512, 512), (256, 256), 42, 7)]         # fused-shape critics in a general trainer
BIG_ROWS = {(512, 512), (300, 7, 129)}             # these run 15, 16, 1000 and 1024 rows too


def shape_id(shape):
    hp, hq, O, A = shape
    return f"p{'x'.join(map(str, hp))}" + ("" if hq is None else f"-q{'x'.join(map(str, hq))}") + f"-O{O}-A{A}"


def rows_of(shape):
    hp, hq, _, _ = shape
    return (1, 17, 33) + ((15, 16, 1000, 1024) if tuple(hp) in BIG_ROWS and hq is None else ())


def net_layers(params, O, A, hidden, hidden_q=None):
    """{net: [(W, b), ...]} of the six nets, of any depth, from flat parameter vectors in library layout."""
    hp, hq = list(hidden), list(hidden_q or hidden)
    dp, dq = [O] + hp, [O + A] + hq
    pol = [(dp[i + 1], dp[i]) for i in range(len(hp))] + [(A, hp[-1])]
    q = [(dq[i + 1], dq[i]) for i in range(len(hq))] + [(1, hq[-1])]
    nets = OrderedDict((name, layers_from_flat(params[name], q)) for name in Q_NETS)
    for name in ("policy", "target_policy"):
        nets[name] = layers_from_flat(params[name], pol)
    return nets


def trainer_layers(t, params=None):
    """net_layers of a trainer: from `params`, its state_dict()'s, or (without a handle) its holders' arrays."""
    if params is None:
        params = t.state_dict()["params"] if t._h is not None else {k: getattr(t, k).flat() for k in t.NETS}
    return net_layers(params, t.obs_dim, t.act_dim, t._hidden("policy"), t._hidden("qf1"))


def trainer_reference(t, batch, eps, dtype, params=None):
    """evaluate_reference on the weights trainer `t` holds now (params: its state_dict()["params"], read once)."""
    return evaluate_reference(trainer_layers(t, params), t.target_policy_noise, t.target_policy_noise_clip, t.reward_scale,
                              t.discount, batch, eps, dtype)


def column_scales(t, seed, params=None):
    """Per column the median |R| of the float64 reference on inputs(1024, ..., seed): what a value of that column
    typically measures on t's weights."""
    batch, eps = inputs(1024, t.obs_dim, t.act_dim, seed)
    r64 = trainer_reference(t, batch, eps, torch.float64, params)
    return {k: float(np.median(np.abs(r64[k]))) for k in COLUMNS}


def conditioned_inputs(t, n, seed, scales, tries=64, params=None):
    """inputs(n, O, A, s) at the first s of seed, seed + 10007, ... at which every column's max|R| of the float64
    REFERENCE is at least CONDITIONED times the median |R| of that column over 1024 rows of the same weights (`scales`):
    tests.td3_eval_reference.conditioned_inputs' rule and its reasons, on nets of any depth.  At most `tries` (64) seeds;
    an assertion if none qualifies."""
    assert tries <= 64
    for k in range(tries):
        batch, eps = inputs(n, t.obs_dim, t.act_dim, seed + 10007 * k)
        r64 = trainer_reference(t, batch, eps, torch.float64, params)
        if all(float(np.max(np.abs(r64[c]))) >= CONDITIONED * scales[c] for c in COLUMNS):
            return batch, eps
    raise AssertionError(f"no well-conditioned draw of {n} rows in {tries} seeds from {seed}")


def check_columns(cols, t, batch, eps, case, errors=None, params=None):
    """Every column of an evaluate_td3(rows=True) result under helpers.check_f64 against the reference on t's live state;
    `errors`: column -> largest error seen, updated.  Returns the float64 reference."""
    params = t.state_dict()["params"] if params is None and t._h is not None else params
    p32 = trainer_reference(t, batch, eps, torch.float32, params)
    r64 = trainer_reference(t, batch, eps, torch.float64, params)
    n = batch[0].shape[0]
    for k in COLUMNS:
        got = np.asarray(cols[k])
        assert got.dtype == np.float32 and got.shape == r64[k].shape, (case, k, got.shape, r64[k].shape)
        e = check_f64(f"{case} {k} n={n}", got, p32[k], r64[k])
        if errors is not None:
            errors[k] = max(errors.get(k, 0.0), e)
    return r64
