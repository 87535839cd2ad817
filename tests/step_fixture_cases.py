"""The cases of tests/golden/step_fixtures.npz: the complete input of one SAC / TD3 step each -- shapes, trainer keywords,
every net as a flat float32 vector in library layout (W0 b0 W1 b1 ...), the Adam moments of the trained nets, the scalars
vector as state_dict()["scalars"] has it, the batch and the noise.

The inputs are not stored: build(name) rebuilds them from np.random.RandomState draws (the legacy stream, frozen by NumPy)
and float32 casts alone, and the fixture holds the SHA-256 of every input array's bytes.  This module imports neither the
oracles nor the package: an edit to either cannot move an input.  tests/golden/make_step_fixture.py writes the fixture,
tests/test_step_fixture_host.py holds the oracles to it, tests/test_gpu_step_fixture.py every step path."""
from __future__ import annotations

import hashlib
from collections import OrderedDict
from dataclasses import dataclass, field

import numpy as np

SAC_NETS = ("policy", "qf1", "qf2", "target_qf1", "target_qf2")
TD3_NETS = SAC_NETS + ("target_policy",)
TRAINED = ("policy", "qf1", "qf2")
GRAD_STRIDE = 97                  # full-size cases: every 97th element of a gradient tensor (prime: every lane and tile position)

# Narrow widths: one that is no multiple of 4 (22), one below 16 (7, 12); the fused family takes any width up to 256.
NARROW = dict(hidden=(22, 12), hidden_q=(7, 36))
# More than two hidden layers: the general step natively.  (Narrow relatives of (64, 96, 48) / (48, 64), whose per-element
# state alone would fill the file: widths above and below one 16-row tile, none a multiple of 16.)
DEEP = dict(hidden=(20, 28, 12), hidden_q=(12, 20))
# The gradients' magnitude per net at inputs of this recipe (a few times the median |g| of a step's elements; the largest are some
# ten times that): the scale of the injected Adam moments.  Constants of the recipe, not derived at run time -- nothing here
# may follow the oracles.
G_SCALE = {"sac": dict(policy=0.03, qf1=0.3, qf2=0.3), "td3": dict(policy=0.004, qf1=0.05, qf2=0.05)}

_SAC_DEFAULT = dict(policy_lr=1e-3, qf_lr=5e-4, soft_target_tau=0.005, target_update_period=5)
_TD3_DEFAULT = dict(policy_learning_rate=1e-3, qf_learning_rate=5e-4, tau=0.005, policy_and_target_update_period=2,
                    target_policy_noise=0.3, target_policy_noise_clip=0.4)

# name -> specification.  state: "trained" (weights at working scale, injected moments, log_alpha != 0) or "fresh" (the
# constructors' init, zero moments, counters 0).  adam_t / n: scalars[3] / scalars[4]; adam_t_pi: TD3's scalars[0].
# The generator refuses a case in which the fp32 oracle alone is more than 2.5e-4 / 8 of a tensor's scale off float64 (a
# one-element tensor whose gradient happens to cancel its exp_avg does that): the remedy is the case's inputs -- the
# recipe below or the seed -- never the cap.
SPECS = OrderedDict([
    ("sac on-period", dict(algo="sac", dims=(42, 7, 40), seed=101, state="trained", adam_t=999, n=1000, **NARROW)),
    ("sac off-period", dict(algo="sac", dims=(42, 7, 40), seed=102, state="trained", adam_t=1000, n=1001, **NARROW)),
    ("sac early", dict(algo="sac", dims=(42, 7, 40), seed=103, state="trained", adam_t=6, n=7, **NARROW)),
    ("sac fixed alpha", dict(algo="sac", dims=(42, 7, 40), seed=104, state="trained", adam_t=1000, n=1001, **NARROW,
                             kw=dict(use_automatic_entropy_tuning=False, reward_scale=2.5, discount=0.97, soft_target_tau=0.05,
                                     target_update_period=1, policy_lr=3e-4, qf_lr=3e-4))),
    ("td3 policy step", dict(algo="td3", dims=(42, 7, 40), seed=105, state="trained", adam_t=999, n=1000, adam_t_pi=499,
                             **NARROW)),
    ("td3 critic step", dict(algo="td3", dims=(42, 7, 40), seed=106, state="trained", adam_t=1000, n=1001, adam_t_pi=500,
                             **NARROW)),
    ("sac deep", dict(algo="sac", dims=(42, 7, 33), seed=107, state="trained", adam_t=999, n=1000, **DEEP)),
    ("td3 deep", dict(algo="td3", dims=(42, 7, 33), seed=108, state="trained", adam_t=999, n=1000, adam_t_pi=499, **DEEP)),
    # 34 row-blocks: the smallest batch the chained launch takes
    ("sac chained", dict(algo="sac", dims=(10, 3, 544), seed=109, state="trained", adam_t=999, n=1000, hidden=(64, 32),
                         hidden_q=(64, 32))),
    ("lift full", dict(algo="sac", dims=(42, 7, 256), seed=110, state="fresh", hidden=(256, 256), hidden_q=(256, 256))),
    ("door full", dict(algo="sac", dims=(46, 7, 1024), seed=111, state="fresh", hidden=(256, 256), hidden_q=(256, 256))),
    ("twoarmlift full", dict(algo="sac", dims=(89, 14, 256), seed=112, state="fresh", hidden=(256, 256),
                             hidden_q=(256, 256))),
    ("td3 lift full", dict(algo="td3", dims=(42, 7, 256), seed=113, state="fresh", hidden=(256, 256), hidden_q=(256, 256))),
])
NAMES = tuple(SPECS)
NARROW_CASES = tuple(k for k, v in SPECS.items() if v["state"] == "trained")
FULL_CASES = tuple(k for k, v in SPECS.items() if v["state"] == "fresh")


@dataclass
class Case:
    name: str
    algo: str
    O: int
    A: int
    B: int
    hidden: tuple
    hidden_q: tuple
    kw: dict                          # the trainer's (and the oracle's) keywords, complete
    full: bool                        # a full-size case: pinned by samples, no state out
    params: dict = field(default_factory=OrderedDict)      # net -> flat float32
    opt: dict = field(default_factory=OrderedDict)         # trained net -> (exp_avg, exp_avg_sq), flat float32
    scalars: np.ndarray = None        # float64 (6,): log_alpha | TD3 policy Adam count, a_m, a_v, adam_t, n_train_steps_total, 0
    batch: dict = field(default_factory=OrderedDict)       # observations, actions, rewards, terminals, next_observations
    eps: tuple = ()                   # SAC: (eps, eps_next); TD3: (eps,)

    @property
    def td3(self):
        return self.algo == "td3"

    @property
    def nets(self):
        return TD3_NETS if self.td3 else SAC_NETS

    def shapes(self, net):
        """[(out, in)] of the layers of `net` in library order: the hidden layers, then the head(s)."""
        policy = net.endswith("policy")
        hs = list(self.hidden if policy else self.hidden_q)
        dims = [self.O if policy else self.O + self.A] + hs
        heads = ([self.A] if self.td3 else [self.A, self.A]) if policy else [1]
        return [(dims[i + 1], dims[i]) for i in range(len(hs))] + [(n, hs[-1]) for n in heads]

    def count(self, net):
        return sum(n * k + n for n, k in self.shapes(net))

    def period(self):
        return self.kw["policy_and_target_update_period" if self.td3 else "target_update_period"]

    def on_period(self):
        """rlkit: targets move (TD3: and the policy steps) where n_train_steps_total % period == 0."""
        return int(self.scalars[4]) % self.period() == 0

    def unchanged_params(self):
        """The nets a step from this case must leave bit for bit as they are."""
        if self.on_period():
            return ()
        return tuple(n for n in self.nets if n.startswith("target_")) + (("policy",) if self.td3 else ())

    def stepped(self):
        """The trained nets whose optimizer steps."""
        return tuple(n for n in TRAINED if not (self.td3 and n == "policy" and not self.on_period()))

    def auto_alpha(self):
        return not self.td3 and self.kw["use_automatic_entropy_tuning"]

    def train_batch(self):
        return dict(self.batch)

    def step_args(self):
        b = self.batch
        return (b["observations"], b["actions"], b["rewards"], b["terminals"], b["next_observations"], *self.eps)

    def inputs(self):
        """Every input array by name, in a fixed order: what the fixture's checksums cover."""
        out = OrderedDict()
        for net in self.nets:
            out["params " + net] = self.params[net]
        for net in TRAINED:
            out["exp_avg " + net], out["exp_avg_sq " + net] = self.opt[net]
        out["scalars"] = self.scalars
        for k, v in self.batch.items():
            out[k] = v
        for i, e in enumerate(self.eps):
            out[f"eps {i}"] = e
        return out

    def checksums(self):
        return OrderedDict((k, sha256(v)) for k, v in self.inputs().items())


def sha256(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def _net(rs, k, hidden, heads, fresh):
    """One net, flat.  fresh: rlkit's constructors -- hidden weights uniform in +-1/sqrt(out), hidden biases 0.1, head
    (width, init_w, -, -): uniform in +-init_w.  Otherwise weights at working scale: uniform in +-min(sqrt(3 / in), 0.45)
    (unit gain), hidden biases in [-0.1, 0.24), head (width, gain, bias low, bias high): weights gain * that bound, biases
    in [low, high).  Every trained value stays below 0.5: an Adam update of lr = 3e-4 must stand well above the float32
    rounding of the parameter it is added to (2^-25 |p|), or the file could not pin a learning rate to 0.1 %."""
    parts, d = [], k
    for h in hidden:
        b = 1.0 / np.sqrt(h) if fresh else min(np.sqrt(3.0 / d), 0.45)
        parts.append(_f32(rs.uniform(-b, b, (h, d))).ravel())
        parts.append(np.full(h, 0.1, np.float32) if fresh else _f32(rs.uniform(-0.1, 0.24, h)))
        d = h
    for n, gain, lo, hi in heads:
        b = gain if fresh else gain * min(np.sqrt(3.0 / d), 0.45)
        parts.append(_f32(rs.uniform(-b, b, (n, d))).ravel())
        parts.append(_f32(rs.uniform(-b, b, n)) if fresh else _f32(rs.uniform(lo, hi, n)))
    return np.concatenate(parts)


def _moments(rs, n, scale, floor, t):
    """Nonzero Adam moments with exp_avg_sq on the scale of g^2: a stand-in |g| = scale * |N(0, 1)| floored at `floor` of
    its maximum, exp_avg = +-|g| U(0.5, 2), exp_avg_sq = g^2 U(0.2, 5) (the construction of _inject in
    tests/test_gpu_optimizer_step.py, with the gradient's scale a constant and no exp_avg near 0: a net's one-element
    tensor must move too), each times the weight t steps of Adam from zero moments have put on it (1 - beta^t: what the
    bias corrections of step t + 1 nearly undo)."""
    g = np.abs(rs.standard_normal(n)) * scale
    s = np.maximum(g, floor * np.max(g))
    m = s * rs.uniform(0.5, 2, n) * np.where(rs.uniform(0, 1, n) < 0.5, -1.0, 1.0)
    return _f32((1 - 0.9 ** t) * m), _f32((1 - 0.999 ** t) * s * s * rs.uniform(0.2, 5, n))


def build(name):
    """The case `name`, rebuilt from its seed: the same bytes on every machine."""
    sp = SPECS[name]
    algo, (O, A, B), fresh = sp["algo"], sp["dims"], sp["state"] == "fresh"
    td3 = algo == "td3"
    kw = dict(_TD3_DEFAULT if td3 else _SAC_DEFAULT)
    if not td3:
        kw.update(discount=0.99, reward_scale=1.0, use_automatic_entropy_tuning=True, target_entropy=float(-A))
    else:
        kw.update(discount=0.99, reward_scale=1.0)
    kw.update(sp.get("kw", {}))
    c = Case(name, algo, O, A, B, tuple(sp["hidden"]), tuple(sp["hidden_q"]), kw, fresh)
    rs = np.random.RandomState(sp["seed"])
    if td3:
        pi_head = [(A, 1e-3, 0, 0)] if fresh else [(A, 0.5, -0.1, 0.1)]
    else:
        pi_head = [(A, 1e-3, 0, 0)] * 2 if fresh else [(A, 0.5, -0.1, 0.1), (A, 0.3, -0.25, -0.05)]
    # Every net its own draw, the targets too: a Polyak update tau (p - t) must stand well above the float32 rounding of
    # the target it is added to (2^-25 |t|), or the file could not pin tau to 0.1 % -- so |p - t| is as large as |t|, and
    # the one-element bias of a critic's head and its target's lie on opposite sides of 0.
    for net in c.nets:
        policy = net.endswith("policy")
        q_head = [(1, 3e-3, 0, 0)] if fresh else [(1, 1.0, -0.06, -0.02) if net.startswith("target_") else (1, 1.0, 0.02, 0.06)]
        c.params[net] = _net(rs, O if policy else O + A, c.hidden if policy else c.hidden_q, pi_head if policy else q_head,
                             fresh)
    floor = 1e-3                       # (_inject's; a case that fails the generator's cap over a small exp_avg_sq raises it)
    for net in TRAINED:
        n = c.count(net)
        assert c.params[net].size == n, (name, net)
        if fresh:
            c.opt[net] = (np.zeros(n, np.float32), np.zeros(n, np.float32))
        else:
            c.opt[net] = _moments(rs, n, G_SCALE[algo][net], floor, sp["adam_t_pi"] if td3 and net == "policy" else sp["adam_t"])
    sc = np.zeros(6, np.float64)
    if not fresh:
        sc[3], sc[4] = sp["adam_t"], sp["n"]
        if td3:
            sc[0] = sp["adam_t_pi"]
        else:                          # log_alpha != 0 and its two moments, float32-representable
            sc[0], sc[1], sc[2] = (float(np.float32(x)) for x in (rs.uniform(-1.2, -0.3), (1 - 0.9 ** sp["adam_t"]) * rs.uniform(-8, 8),
                                                           (1 - 0.999 ** sp["adam_t"]) * rs.uniform(30, 150)))
    c.scalars = sc
    c.batch = OrderedDict([("observations", _f32(rs.normal(0, 0.5, (B, O)))), ("actions", _f32(rs.uniform(-1, 1, (B, A)))),
                           ("rewards", _f32(rs.uniform(0, 1, (B, 1)))),
                           ("terminals", (rs.uniform(0, 1, (B, 1)) < 0.1).astype(np.float32)),
                           ("next_observations", _f32(rs.normal(0, 0.5, (B, O))))])
    c.eps = tuple(_f32(np.clip(rs.standard_normal((B, A)), -4, 4)) for _ in range(1 if td3 else 2))
    assert c.batch["terminals"].sum() >= 1, (name, "no terminal row")
    return c


def terminal_rows(c):
    return np.flatnonzero(c.batch["terminals"].ravel() != 0)


# ---- what a step leaves, by name -----------------------------------------------------------------------------------------
# debug_fetch name of every per-row output (tests/helpers.py SAC_ROWS / TD3_ROWS hold the oracles' keys for them)
ROW_NAMES = {"sac": ("q1", "q2", "q1_new", "q2_new", "q_target", "log_pi", "log_pi_next", "a_new", "mu", "log_std", "a_next"),
             "td3": ("q1", "q2", "q_target", "tq1", "tq2", "q1_new", "a_new", "a_next")}


def layer_names(c, net):
    heads = ("last_fc",) if not net.endswith("policy") or c.td3 else ("last_fc", "last_fc_log_std")
    return [f"fc{i}" for i in range(len(c.shapes(net)) - len(heads))] + list(heads)


def split(c, net, flat, what):
    """A flat vector of `net` in library layout -> {"<what> <net> fc0.weight": ..., "<what> <net> fc0.bias": ..., ...}."""
    flat = np.asarray(flat, np.float64).ravel()
    assert flat.size == c.count(net), (c.name, net, flat.size, c.count(net))
    out, off = OrderedDict(), 0
    for (n, k), nm in zip(c.shapes(net), layer_names(c, net)):
        out[f"{what} {net} {nm}.weight"] = flat[off:off + n * k]; off += n * k
        out[f"{what} {net} {nm}.bias"] = flat[off:off + n]; off += n
    return out


def step_tensors(c, rows, grads, params_out=None, opt_out=None, scalars_out=None):
    """Every tensor of one step from `c` that the fixture pins under the per-tensor rule, by name, float64, in the file's
    order: rows {debug_fetch name: values}; grads {net: flat gradient} of the nets that stepped; and, for the narrow cases,
    the state out -- params_out {net: flat}: stored as the UPDATE out - in (the input taken exactly in float64), of every
    net the case does not leave unchanged; opt_out {net: (exp_avg, exp_avg_sq)} of the nets that stepped; scalars_out:
    log_alpha and its two moments where alpha is tuned."""
    out = OrderedDict()
    for name in ROW_NAMES[c.algo]:
        out["row " + name] = np.asarray(rows[name], np.float64).ravel()
    for net in c.stepped():
        out.update(split(c, net, grads[net], "gradient of"))
    if c.full:
        return out
    for net in c.nets:
        if net not in c.unchanged_params():
            out.update(split(c, net, np.asarray(params_out[net], np.float64) - c.params[net].astype(np.float64), "update of"))
    for i, what in enumerate(("exp_avg of", "exp_avg_sq of")):
        for net in c.stepped():
            out.update(split(c, net, opt_out[net][i], what))
    if c.auto_alpha():
        for i, what in enumerate(("log_alpha", "log_alpha exp_avg", "log_alpha exp_avg_sq")):
            out[what] = np.asarray([scalars_out[i]], np.float64)
    return out


def stored_view(c, name, x):
    """What the file keeps of tensor `name`: a full-size case's gradients every GRAD_STRIDE-th element, all else whole."""
    return x[::GRAD_STRIDE] if c.full and name.startswith("gradient of") else x


def counters_out(c):
    """scalars[3], scalars[4] (and TD3's scalars[0]) behind one step: compared exactly."""
    sc = c.scalars
    out = {"adam_t": sc[3] + 1, "n_train_steps_total": sc[4] + 1}
    if c.td3:
        out["adam_t_pi"] = sc[0] + (1 if c.on_period() else 0)
    return out


class Fixture:
    """tests/golden/step_fixtures.npz, read once: per case `values` (the stored view of every step_tensors entry, float32,
    back to back), `stats` (per entry s = max|R64| and e32 = max|P32 - R64| / s over the WHOLE tensor), `diag` (per
    diagnostic: float64 value, scale, e32), `scalars` (state_dict()["scalars"][:5] behind the step, float64); and `meta`
    (JSON: names, checksums, versions)."""

    def __init__(self, path):
        import json
        with np.load(path) as z:
            self.arrays = {k: z[k] for k in z.files}
        self.meta = json.loads(bytes(self.arrays["meta"]).decode())

    def case(self, c):
        m = self.meta["cases"][c.name]
        values, stats = self.arrays[c.name + "|values"], self.arrays[c.name + "|stats"]
        assert values.dtype == np.float32 and stats.shape == (len(m["tensors"]), 2), (c.name, values.dtype, stats.shape)
        out, off = OrderedDict(), 0
        for (name, n), (s, e32) in zip(m["tensors"], stats):
            out[name] = (values[off:off + n].astype(np.float64), float(s), float(e32)); off += n
        assert off == values.size, (c.name, off, values.size)
        diag = OrderedDict((name, tuple(float(x) for x in row)) for name, row in zip(m["diag"], self.arrays[c.name + "|diag"]))
        return out, diag, self.arrays[c.name + "|scalars"]
