"""Trained-regime states (test infrastructure, pure NumPy; checked on the CPU by tests/test_trained_states_host.py, used
by tests/test_gpu_trained_paths.py and tests/test_gpu_trained_inference.py): the networks of a shipped run
(tests/golden/trained_weights_lift_seed129.npz -- weights up to 39, hidden activations O(100), Q about -114) in the
oracle's layout, with target networks that DIFFER from the online ones, and the same networks inflated to wider
observation and action dimensions.  In this regime a step runs its masked, saturating and cancelling branches at once:
about a tenth of a_new is exactly +-1.0f, a few percent of log_std sit on the upper clamp, and a Q value is a
cancellation of O(100) terms.

helpers.make_pair_from_flat builds from the same fixture with targets that alias the critics; here every target tensor
differs from its online tensor, so a kernel that read the wrong one of the two would be seen."""
from __future__ import annotations

import os
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "trained_weights_lift_seed129.npz")
O0, A0, HIDDEN = 42, 7, (256, 256)                   # the fixture's task (Lift) and hidden sizes
LAG = 0.01                                           # a lagged target: online * (1 + LAG * U(-1, 1)) per element


def _layers(flat, shapes):
    out, off = [], 0
    for n, k in shapes:
        w = np.asarray(flat[off:off + n * k], np.float32).reshape(n, k).copy(); off += n * k
        b = np.asarray(flat[off:off + n], np.float32).copy(); off += n
        out.append((w, b))
    assert off == len(flat)
    return out


def _copy(layers):
    return [(w.copy(), b.copy()) for w, b in layers]


def lagged(layers, rs):
    """Every element times 1 + LAG * U(-1, 1): no tensor of the copy equals its source."""
    f = np.float32
    return [((w * (1 + LAG * rs.uniform(-1, 1, w.shape))).astype(f), (b * (1 + LAG * rs.uniform(-1, 1, b.shape))).astype(f))
            for w, b in layers]


def trained_nets(algo, targets="lagged", seed=0):
    """The fixture's networks in the oracle's layout (init_sac_params / init_td3_params), for make_pair(nets=...) and
    make_td3_pair(nets=...).  SAC: policy, qf1, qf2 of the run.  TD3: the policy without its log_std head, and a
    target_policy.  targets: "lagged" (seeded by `seed`; every target tensor differs from its online tensor) or "online"
    (copies of the online nets -- what a kernel reading the wrong nets would compute with)."""
    assert algo in ("sac", "td3") and targets in ("lagged", "online")
    z = np.load(FIXTURE)
    q_shapes = [(256, O0 + A0), (256, 256), (1, 256)]
    p_shapes = [(256, O0), (256, 256), (A0, 256), (A0, 256)]
    online = OrderedDict(qf1=_layers(z["qf1"], q_shapes), qf2=_layers(z["qf2"], q_shapes))
    policy = _layers(z["policy"], p_shapes)
    online["policy"] = policy if algo == "sac" else policy[:3]
    rs = np.random.RandomState(seed)
    tgt = (lambda l: lagged(l, rs)) if targets == "lagged" else _copy
    nets = OrderedDict()
    for name in ("qf1", "qf2"):
        nets[name] = online[name]
    for name in ("qf1", "qf2"):
        nets["target_" + name] = tgt(online[name])
    nets["policy"] = online["policy"]
    if algo == "td3":
        nets["target_policy"] = tgt(online["policy"])
    return nets


def with_online_targets(nets):
    """`nets` with every target net replaced by a copy of its online net."""
    return OrderedDict((k, _copy(nets[k[len("target_"):]]) if k.startswith("target_") else v) for k, v in nets.items())


def _split_columns(w, lo, hi, k, rs):
    """Columns lo..hi of `w`, each split into k columns (tiled order: copy c of column j at c * (hi - lo) + j) whose
    weights are the original times a Dirichlet share; the shares of a column sum to 1."""
    n = hi - lo
    share = rs.dirichlet(np.ones(k), size=n).T if k > 1 else np.ones((1, n))          # (k, n), columns sum to 1
    return np.concatenate([w[:, lo:hi] * share[c][None, :] for c in range(k)], axis=1).astype(np.float32)


def inflate(nets, ko, ka, seed=0):
    """The same networks at O * ko observation and A * ka action dimensions, for a batch whose observations and actions are
    tiled ko and ka times (trained_batch): every first-layer observation column is split into ko columns, the Q nets'
    action columns into ka, and the policy heads' rows are repeated ka times.  On tiled inputs the first layers compute
    what they did (to rounding: the shares sum to 1), so the hidden activations and Q keep their trained magnitudes."""
    if (ko, ka) == (1, 1):
        return nets
    rs = np.random.RandomState(seed)
    out = OrderedDict()
    for name, layers in nets.items():
        layers = _copy(layers)
        w0, b0 = layers[0]
        if "policy" in name:
            O = w0.shape[1]
            layers[0] = (_split_columns(w0, 0, O, ko, rs), b0)
            heads = 2 if len(layers) == len(HIDDEN) + 2 else 1
            for h in range(len(layers) - heads, len(layers)):
                w, b = layers[h]
                layers[h] = (np.tile(w, (ka, 1)), np.tile(b, ka))
        else:
            O = O0
            A = w0.shape[1] - O
            layers[0] = (np.concatenate([_split_columns(w0, 0, O, ko, rs), _split_columns(w0, O, O + A, ka, rs)], axis=1), b0)
        out[name] = layers
    return out


def trained_rows(n, ko, ka, seed, term_frac=0.05):
    """n synthetic Lift transitions (helpers.synth_transitions' distributions) with observations and actions tiled."""
    rs = np.random.RandomState(seed)
    obs = rs.normal(0, 0.5, (n, O0)).astype(np.float32)
    nobs = rs.normal(0, 0.5, (n, O0)).astype(np.float32)
    act = rs.uniform(-1, 1, (n, A0)).astype(np.float32)
    rew = rs.uniform(0, 1, (n, 1)).astype(np.float32)
    term = (rs.uniform(0, 1, (n, 1)) < term_frac).astype(np.float32)
    return np.tile(obs, (1, ko)), np.tile(act, (1, ka)), rew, term, np.tile(nobs, (1, ko))


def trained_batch(O, A, B, ko=1, ka=1, seed=77):
    """(batch, eps) at O * ko / A * ka: B rows of trained_rows(seed) and two (B, A * ka) N(0, 1) draws of RandomState(5)."""
    assert (O, A) == (O0, A0)
    obs, act, rew, term, nobs = trained_rows(B, ko, ka, seed)
    rs = np.random.RandomState(5)
    eps = (rs.normal(size=(B, A * ka)).astype(np.float32), rs.normal(size=(B, A * ka)).astype(np.float32))
    return dict(observations=obs, actions=act, rewards=rew, terminals=term, next_observations=nobs), eps


def batch_args(batch):
    return (batch["observations"], batch["actions"], batch["rewards"], batch["terminals"], batch["next_observations"])


def state(algo, ko, ka, B, lag_seed=0):
    """(nets, batch, eps) of one GPU case."""
    nets = inflate(trained_nets(algo, seed=lag_seed), ko, ka, seed=1)
    batch, eps = trained_batch(O0, A0, B, ko, ka)
    return nets, batch, eps


# ---- one step on every path: label, algo, environment, (ko, ka, B), kind (TD3: whether the critic pass is the fused
# launch; None: the general step).  The smallest batches that still select the path.
CHAIN = dict(SAC_CHAIN=1, SAC_CHAIN_BWD=0)
PATHS = [
    ("fused padded", "sac", {}, (1, 1, 255), 1),
    ("fused own row conversion", "sac", dict(SAC_ROW_IMAGES=0), (1, 1, 255), 1),
    ("fused loop-form dW", "sac", dict(SAC_DW_FORM="loop"), (1, 1, 255), 1),
    ("four-launch SP 4", "sac", dict(SAC_FUSED=0), (1, 1, 255), 0),
    ("four-launch SP 2", "sac", {}, (1, 1, 288), 0),
    ("four-launch SP 2 compact 0", "sac", {}, (1, 1, 1040), 0),
    ("four-launch SP 1 k_bwd8", "sac", dict(SAC_CHAIN=0), (1, 1, 544), 0),
    ("four-launch SP 1 k_bwd", "sac", dict(SAC_CHAIN=0, SAC_BWD8=0), (1, 1, 544), 0),
    ("chained", "sac", CHAIN, (1, 1, 530), 2),
    ("chained four-wave", "sac", dict(CHAIN, SAC_CHAIN8=0), (1, 1, 530), 2),
    ("chained backward inside", "sac", dict(SAC_CHAIN_BWD=1), (1, 1, 530), 4),
    ("general", "sac", dict(SAC_GENERAL=1), (1, 1, 255), 3),
    ("inflated 126/14 fused", "sac", {}, (3, 2, 255), 1),
    ("inflated 126/14 four-launch", "sac", dict(SAC_FUSED=0), (3, 2, 255), 0),
    ("inflated 126/14 chained", "sac", dict(SAC_CHAIN=1), (3, 2, 544), (2, 4)),
    ("inflated 84/7 fused", "sac", {}, (2, 1, 255), 1),
    ("inflated 84/7 chained", "sac", dict(SAC_CHAIN=1), (2, 1, 544), (2, 4)),
    ("td3 fused critic", "td3", {}, (1, 1, 255), True),
    ("td3 four-launch SP 4", "td3", dict(SAC_FUSED=0), (1, 1, 255), False),
    ("td3 four-launch SP 2", "td3", {}, (1, 1, 288), False),
    ("td3 four-launch SP 1", "td3", {}, (1, 1, 544), False),
    ("td3 general", "td3", dict(SAC_GENERAL=1), (1, 1, 255), None),
    ("td3 inflated 126/14", "td3", {}, (3, 2, 255), True),
]
ENV = ("SAC_FUSED", "SAC_CHAIN", "SAC_CHAIN_BWD", "SAC_GENERAL", "SAC_CHAIN8", "SAC_BWD8", "SAC_ROW_IMAGES", "SAC_DW_FORM",
       "SAC_FUSED_TEST_STALL")
# the trainer groups (B 128) and the row counts of tests/test_gpu_trained_inference.py start from these states too
EXTRA_STATES = [("sac", 1, 1, 128), ("td3", 1, 1, 128), ("sac", 3, 2, 128), ("sac", 2, 1, 544), ("sac", 1, 1, 256),
                ("sac", 3, 2, 256), ("td3", 1, 1, 256), ("sac", 1, 1, 17), ("td3", 1, 1, 17)]


def gpu_states():
    """Every (algo, ko, ka, B) a GPU test steps or evaluates from, once each."""
    seen = []
    for s in [(p[1],) + p[3] for p in PATHS] + EXTRA_STATES:
        if s not in seen:
            seen.append(s)
    return seen
