"""Reference of SACTrainer.evaluate (test infrastructure; imports oracle/): the forward half of the SAC step WITHOUT any
update, restated on oracle.sac_step_torch.PolicyNet / QNet in float32 or float64, log_alpha taken as given.

The thirteen arrays: q1, q2, q1_new, q2_new, tq1, tq2, log_pi, log_pi_next, y (n,), mu, log_std, a_new, a_next (n, A).
With alpha = exp(log_alpha) (1 with automatic tuning off):
    y = reward_scale r + (1 - d) discount (min(tq1, tq2)(s', a_next) - alpha log_pi(a_next | s'))

On the CPU at 1024 rows of helpers.synth_transitions(term_frac=0.1), for (O, A, hidden) = (42, 7, (256, 256)),
(1, 1, (16, 16)), (379, 6, (256, 256)), (46, 16, (240, 256)), (496, 7, (128, 64)), the float32 reference is within
6.1e-7 of max|R| of the float64 one on every Q column and within 1.7e-6 to 1.3e-5 on log_pi, log_pi_next and y (largest
|a| 0.9997): helpers.check_f64 as it stands -- max(8 x the fp32 oracle's error, 1e-5) of max|R| -- is the bound of every
per-row column."""
from collections import OrderedDict

import numpy as np
import torch

from oracle.sac_step_torch import PolicyNet, QNet
from tests.helpers import layers_from_flat

ROW_COLUMNS = ("q1", "q2", "q1_new", "q2_new", "tq1", "tq2", "log_pi", "log_pi_next", "y")
ARRAY_COLUMNS = ("mu", "log_std", "a_new", "a_next")
COLUMNS = ROW_COLUMNS + ARRAY_COLUMNS
SHAPES = [(42, 7, (256, 256)), (1, 1, (16, 16)), (379, 6, (256, 256)), (46, 16, (240, 256)), (496, 7, (128, 64))]


def net_layers(params, O, A, hidden, hidden_q=None):
    """{net: [(W, b), ...]} from flat parameter vectors in library layout (state_dict()["params"], holder.flat())."""
    hp, hq = list(hidden), list(hidden_q or hidden)
    pol = [(hp[0], O), (hp[1], hp[0]), (A, hp[1]), (A, hp[1])]
    q = [(hq[0], O + A), (hq[1], hq[0]), (1, hq[1])]
    nets = OrderedDict((name, layers_from_flat(params[name], q)) for name in ("qf1", "qf2", "target_qf1", "target_qf2"))
    nets["policy"] = layers_from_flat(params["policy"], pol)
    return nets


def trainer_layers(t, params=None):
    """net_layers of a trainer: from `params`, its state_dict()'s, or (without a handle) its holders' arrays."""
    if params is None:
        params = t.state_dict()["params"] if t._h is not None else {k: getattr(t, k).flat() for k in t.NETS}
    return net_layers(params, t.obs_dim, t.act_dim, t._hidden("policy"), t._hidden("qf1"))


def evaluate_reference(nets, log_alpha, reward_scale, discount, batch, eps, dtype):
    """The thirteen arrays on `nets` (net_layers) in `dtype`; log_alpha None: automatic tuning off, alpha = 1.
    batch: (obs, act, rew, term, nobs) float32 as helpers.synth_transitions gives them; eps: (eps, eps_next)."""
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype)      # noqa: E731
    obs, act, rew, term, nobs = (t(x) for x in batch)
    rew, term = rew.reshape(-1, 1), term.reshape(-1, 1)
    e1, e2 = (t(x) for x in eps)
    policy = PolicyNet(nets["policy"], dtype)
    qf1, qf2, tqf1, tqf2 = (QNet(nets[k], dtype) for k in ("qf1", "qf2", "target_qf1", "target_qf2"))
    with torch.no_grad():
        alpha = torch.ones(1, dtype=dtype) if log_alpha is None else torch.tensor([np.float32(log_alpha)]).to(dtype).exp()
        a_new, mu, log_std, log_pi, _ = policy(obs, e1)
        a_next, _, _, log_pi_next, _ = policy(nobs, e2)
        tq1, tq2 = tqf1(nobs, a_next), tqf2(nobs, a_next)
        y = reward_scale * rew + (1.0 - term) * discount * (torch.min(tq1, tq2) - alpha * log_pi_next)
        out = dict(q1=qf1(obs, act), q2=qf2(obs, act), q1_new=qf1(obs, a_new), q2_new=qf2(obs, a_new), tq1=tq1, tq2=tq2,
                   log_pi=log_pi, log_pi_next=log_pi_next, y=y, mu=mu, log_std=log_std, a_new=a_new, a_next=a_next)
    return OrderedDict((k, out[k].numpy()[:, 0] if k in ROW_COLUMNS else out[k].numpy()) for k in COLUMNS)


def trainer_reference(t, batch, eps, dtype, params=None, log_alpha="live"):
    """evaluate_reference on the weights and the log_alpha trainer `t` holds now."""
    if log_alpha == "live":
        log_alpha = None
        if t.use_automatic_entropy_tuning:
            log_alpha = t.state_dict()["scalars"][0] if t._h is not None else 0.0
    return evaluate_reference(trainer_layers(t, params), log_alpha, t.reward_scale, t.discount, batch, eps, dtype)


def batch_dict(batch):
    obs, act, rew, term, nobs = batch
    return dict(observations=obs, actions=act, rewards=rew, terminals=term, next_observations=nobs)


def check_columns(cols, t, batch, eps, case, errors=None, params=None):
    """Every column of an evaluate(rows=True) result under helpers.check_f64 against the reference on t's live state;
    `errors`: column -> largest error seen, updated."""
    from tests.helpers import check_f64
    p32 = trainer_reference(t, batch, eps, torch.float32, params)
    r64 = trainer_reference(t, batch, eps, torch.float64, params)
    n = batch[0].shape[0]
    for k in COLUMNS:
        got = np.asarray(cols[k])
        assert got.dtype == np.float32 and got.shape == r64[k].shape, (case, k, got.shape, r64[k].shape)
        e = check_f64(f"{case} {k} n={n}", got, p32[k], r64[k])
        if errors is not None:
            errors[k] = max(errors.get(k, 0.0), e)
