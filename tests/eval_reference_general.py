"""Reference of SACTrainer.evaluate for nets of ANY depth (test infrastructure; imports oracle/): the layers of every net
from flat parameter vectors in library layout (state_dict()["params"]) -- the policy hidden..., (A, last), (A, last), a Q
net hidden..., (1, last) -- handed to tests.eval_reference.evaluate_reference in float32 and float64.  Bound of every
per-row column: helpers.check_f64 as it stands, max|K - R| / max|R| <= max(8 max|P - R| / max|R|, 1e-5)."""
from collections import OrderedDict

import numpy as np
import torch

from tests.eval_reference import COLUMNS, evaluate_reference
from tests.helpers import check_f64, layers_from_flat


def net_layers(params, O, A, hidden, hidden_q):
    """{net: [(W, b), ...]} of any depth from flat parameter vectors in library layout."""
    hp, hq = list(hidden), list(hidden_q)
    dp, dq = [O] + hp, [O + A] + hq
    pol = [(dp[i + 1], dp[i]) for i in range(len(hp))] + [(A, hp[-1]), (A, hp[-1])]
    q = [(dq[i + 1], dq[i]) for i in range(len(hq))] + [(1, hq[-1])]
    nets = OrderedDict((name, layers_from_flat(params[name], q)) for name in ("qf1", "qf2", "target_qf1", "target_qf2"))
    nets["policy"] = layers_from_flat(params["policy"], pol)
    return nets


def trainer_reference(t, batch, eps, dtype, state=None):
    """evaluate_reference on the weights and the log_alpha trainer `t` holds now (state: its state_dict(), read once)."""
    state = t.state_dict() if state is None else state
    log_alpha = state["scalars"][0] if t.use_automatic_entropy_tuning else None
    nets = net_layers(state["params"], t.obs_dim, t.act_dim, t._hidden("policy"), t._hidden("qf1"))
    return evaluate_reference(nets, log_alpha, t.reward_scale, t.discount, batch, eps, dtype)


def check_columns(cols, t, batch, eps, case, errors=None, state=None):
    """Every column of an evaluate(rows=True) result under helpers.check_f64 against the reference on t's live state;
    `errors`: column -> largest error seen, updated.  Returns the float64 reference."""
    state = t.state_dict() if state is None else state
    p32 = trainer_reference(t, batch, eps, torch.float32, state)
    r64 = trainer_reference(t, batch, eps, torch.float64, state)
    n = batch[0].shape[0]
    for k in COLUMNS:
        got = np.asarray(cols[k])
        assert got.dtype == np.float32 and got.shape == r64[k].shape, (case, k, got.shape, r64[k].shape)
        e = check_f64(f"{case} {k} n={n}", got, p32[k], r64[k])
        if errors is not None:
            errors[k] = max(errors.get(k, 0.0), e)
    return r64
