"""Non-finite states of one SAC / TD3 step (test infrastructure, used by tests/test_gpu_step_nonfinite.py and checked on the
CPU by tests/test_nonfinite_states_host.py): the states of tests/edge_states._base with ONE element poisoned by a literal
NaN or +inf -- an observation, a next observation (also on a terminal row: 0 * NaN), a reward, an action, a weight, a
noise draw.  No poison is a finite value that overflows, so no class depends on the order of a sum.

Every builder returns an EdgeState whose `meta` holds what the ORACLES say of one step from that state (nothing the
kernels give enters it):
  classes / classes64   {name: int8 array} from the fp32 / float64 oracle: FINITE, POS_INF, NEG_INF or NAN for every
                        element of "diag <statistic>", "row <per-row output>", "grad <net>" (flat, library layout) and
                        the state after the step in the layout of trainer.state_dict(): "param <net>", "exp_avg <net>",
                        "exp_avg_sq <net>", and for SAC "log_alpha" (log alpha, its two Adam moments, alpha)
  values32 / values64   the same arrays' values (float64 arrays of the fp32 / float64 oracle's numbers)
  bit_equal             the state tensors whose fp32-oracle bits equal the clean run's (the same state, poison removed)
  same_diags            the statistics whose fp32-oracle bits equal the clean run's
  ambiguous             {name: bool mask}, the elements left out of the class comparison (below)
  clean, rows           the clean twin (an EdgeState without meta); the poisoned rows
  clean_values32 / 64   the oracles' numbers on the clean twin

Ambiguous elements.  Where the poison reaches a net's gradient through dL/dq alone (a reward, a next observation), unit u
of a hidden layer passes it at the poisoned row r exactly when relu'(h[r, u]) = 1: row u of that layer's weight gradient
and element u of its bias gradient are NaN when h[r, u] > 0 and finite otherwise, and so are the parameter, both Adam
moments and the Polyak target behind them.  A kernel that sums in another order may land a pre-activation of about 0 on
the other side.  A unit whose float64 pre-activation at a poisoned row lies within F64_FLOOR (1e-5, the floor of
helpers.check_f64) of the layer's largest finite |pre-activation| is ambiguous, and the elements it gates are left out.
At most AMBIGUOUS_CAP (1 %) of any tensor may be left out: the seeds below keep the reference inside that (asserted by
the host test)."""
from __future__ import annotations

import copy
from functools import lru_cache

import numpy as np
import torch

from oracle.sac_step_torch import RlkitEquivalentSAC
from oracle.td3_step_torch import RlkitEquivalentTD3
from tests.edge_states import EdgeState, _base
from tests.helpers import F64_FLOOR, SAC_ROWS, TD3_ROWS, layer_names, NET_HEADS, named_tensors, oracle_flat_grad

FINITE, POS_INF, NEG_INF, NAN = 0, 1, 2, 3
CLASS_NAMES = ("finite", "+inf", "-inf", "NaN")
AMBIGUOUS_CAP = 0.01
ROW = 3                                                   # the poisoned row

# poison -> what it sets (one element, or one element of each poisoned row)
SAC_POISONS = ("obs nan", "obs nan last", "obs inf", "next_obs nan", "next_obs nan terminal", "reward inf", "reward nan",
               "action nan", "qf1 weight nan", "target_qf2 weight nan", "policy weight inf", "eps1 nan")
TD3_POISONS = ("obs nan", "obs nan last", "next_obs nan", "reward inf", "action nan", "qf1 weight nan", "noise nan")
POISONS = {"sac": SAC_POISONS, "td3": TD3_POISONS}
SAC_NETS = ("policy", "qf1", "qf2", "target_qf1", "target_qf2")
TD3_NETS = SAC_NETS + ("target_policy",)
TRAINED = ("policy", "qf1", "qf2")

# What stays bit-equal to the clean run per poison (the issue's table; the host test asserts the oracle gives exactly
# this).  Names are those of state_names().
_ALL_POLICY = ("param policy", "exp_avg policy", "exp_avg_sq policy")
_QF2_SIDE = ("param qf2", "exp_avg qf2", "exp_avg_sq qf2", "param target_qf2")
EXPECTED_BIT_EQUAL = {
    "sac": {"obs nan": (), "obs nan last": (), "obs inf": (), "policy weight inf": (), "eps1 nan": (),
            "next_obs nan": _ALL_POLICY + ("log_alpha",), "next_obs nan terminal": _ALL_POLICY + ("log_alpha",),
            "reward inf": _ALL_POLICY + ("log_alpha",), "reward nan": _ALL_POLICY + ("log_alpha",),
            "action nan": _ALL_POLICY + ("log_alpha",), "target_qf2 weight nan": _ALL_POLICY + ("log_alpha",),
            "qf1 weight nan": _QF2_SIDE + ("log_alpha",)},
    # TD3's policy step runs through the UPDATED qf1: whatever poisons qf1's gradient poisons the policy one step on
    "td3": {"obs nan": (), "obs nan last": (), "next_obs nan": (), "reward inf": (), "noise nan": (),
            "action nan": (), "qf1 weight nan": _QF2_SIDE},
}


def class_of(x):
    x = np.asarray(x, np.float64)
    c = np.full(x.shape, FINITE, np.int8)
    c[np.isposinf(x)] = POS_INF
    c[np.isneginf(x)] = NEG_INF
    c[np.isnan(x)] = NAN
    return c


def _poison(st, poison):
    """Set the poison of `poison` in the EdgeState `st` (in place); returns the poisoned rows."""
    B, nan, inf = st.obs.shape[0], np.float32(np.nan), np.float32(np.inf)
    rows = [ROW]
    if poison == "obs nan":
        st.obs[ROW, 5] = nan
    elif poison == "obs nan last":           # also the last live row: inside a partial row-block, next to the pads
        rows = [ROW, B - 1]
        st.obs[rows, 5] = nan
    elif poison == "obs inf":
        st.obs[ROW, 5] = inf
    elif poison == "next_obs nan":
        st.term[ROW] = 0.0
        st.nobs[ROW, 5] = nan
    elif poison == "next_obs nan terminal":
        st.term[ROW] = 1.0
        st.nobs[ROW, 5] = nan
    elif poison == "reward inf":
        st.rew[ROW] = inf
    elif poison == "reward nan":
        st.rew[ROW] = nan
    elif poison == "action nan":
        st.act[ROW, 2] = nan
    elif poison == "qf1 weight nan":         # a hidden weight: the last hidden layer, unit 1, input 2
        rows = list(range(B))
        st.nets["qf1"][len(st.nets["qf1"]) - 2][0][1, 2] = nan
    elif poison == "target_qf2 weight nan":
        rows = list(range(B))
        st.nets["target_qf2"][len(st.nets["target_qf2"]) - 2][0][1, 2] = nan
    elif poison == "policy weight inf":
        rows = list(range(B))
        st.nets["policy"][0][0][1, 2] = inf
    elif poison in ("eps1 nan", "noise nan"):
        st.eps[0][ROW, 2] = nan
    else:
        raise ValueError(poison)
    return rows


def _oracle(st, dtype):
    if st.algo == "sac":
        return RlkitEquivalentSAC(st.nets, st.act.shape[1], dtype=dtype, policy_lr=1e-3, qf_lr=5e-4, soft_target_tau=0.005, **st.kw)
    return RlkitEquivalentTD3(st.nets, st.act.shape[1], dtype=dtype, policy_learning_rate=1e-3, qf_learning_rate=5e-4, **st.kw)


def _flat_lib(ws, bs):
    """Per-layer tensors in library layout: W0 b0 W1 b1 ..."""
    return np.concatenate([np.concatenate([np.ravel(w), np.ravel(b)]) for w, b in zip(ws, bs)])


def oracle_state(o):
    """The oracle's state after its step(s) in the layout of trainer.state_dict(): params / opt per net (flat, library
    layout) and the scalars (SAC: log_alpha, its exp_avg, exp_avg_sq, optimizer steps, train steps, alpha)."""
    td3 = hasattr(o, "target_policy")
    num = lambda t: t.detach().numpy().astype(np.float64)        # noqa: E731
    st = dict(params={}, opt={})
    for net in (TD3_NETS if td3 else SAC_NETS):
        m = getattr(o, net)
        st["params"][net] = _flat_lib([num(w) for w in m.ws], [num(b) for b in m.bs])
    for net in TRAINED:
        m, opt = getattr(o, net), getattr(o, net + "_opt")
        mom = []
        for key in ("exp_avg", "exp_avg_sq"):
            get = lambda p: num(opt.state[p][key]) if p in opt.state else np.zeros(tuple(p.shape))    # noqa: E731
            mom.append(_flat_lib([get(w) for w in m.ws], [get(b) for b in m.bs]))
        st["opt"][net] = tuple(mom)
    if not td3:
        s = o.alpha_opt.state.get(o.log_alpha, {})
        la = float(o.log_alpha.detach())
        st["scalars"] = np.array([la, float(s["exp_avg"]) if s else 0.0, float(s["exp_avg_sq"]) if s else 0.0,
                                  o.n_train_steps_total, o.n_train_steps_total, np.exp(la) if o.auto_alpha else 1.0])
    return st


def state_tensors(sd, td3):
    """{name: flat array} of a state_dict()-shaped record (the oracle's or the trainer's): "param <net>", "exp_avg <net>",
    "exp_avg_sq <net>", and for SAC "log_alpha" (log_alpha, its two Adam moments, alpha)."""
    out = {}
    for net in (TD3_NETS if td3 else SAC_NETS):
        out["param " + net] = np.asarray(sd["params"][net])
    for net in TRAINED:
        out["exp_avg " + net], out["exp_avg_sq " + net] = (np.asarray(x) for x in sd["opt"][net])
    if not td3:
        sc = np.asarray(sd["scalars"], np.float64)
        out["log_alpha"] = sc[[0, 1, 2, 5]]
    return out


def net_layout(st, net):
    """(shapes, layer names) of one net of the EdgeState `st`."""
    layers = st.nets[net]
    heads = NET_HEADS["q"] if "qf" in net else NET_HEADS["sac_policy" if st.algo == "sac" else "td3_policy"]
    return [tuple(w.shape) for w, _ in layers], layer_names(len(layers), heads)


def _record(o, diag, td3):
    """Everything one oracle step gives, by name, as float64 arrays."""
    out = {}
    for k, v in diag.items():
        out["diag " + k] = np.asarray([v], np.float64)
    for name, key in (TD3_ROWS if td3 else SAC_ROWS).items():
        out["row " + name] = o.last[key].detach().numpy().astype(np.float64).ravel()
    for net in TRAINED:
        g = o.last["g_" + net]
        if g is not None:
            out["grad " + net] = np.asarray(oracle_flat_grad(g), np.float64).ravel()
    out.update({k: np.asarray(v, np.float64).ravel() for k, v in state_tensors(oracle_state(o), td3).items()})
    return out


def _pre_activations(layers, x, n_hidden):
    """float64 pre-activations of the hidden layers on the rows x."""
    pre, h = [], np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        for w, b in layers[:n_hidden]:
            z = h @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)
            pre.append(z)
            h = np.where(z < 0, 0.0, z)                  # (a NaN stays a NaN, as in torch's relu)
    return pre


def _ambiguous(st, rows):
    """{name: bool mask over the flat tensor}: what the ambiguous units of the trained nets gate."""
    td3 = st.algo == "td3"
    out = {}
    for net in TRAINED:
        shapes, names = net_layout(st, net)
        n_hidden = len(shapes) - (1 if "qf" in net or td3 else 2)
        x = np.concatenate([st.obs, st.act], axis=1) if "qf" in net else st.obs
        pre = _pre_activations(st.nets[net], x, n_hidden)
        flat, off = np.zeros(sum(n * k + n for n, k in shapes), bool), 0
        for l, (n, k) in enumerate(shapes):
            if l < n_hidden:
                z = pre[l]
                top = np.max(np.abs(z[np.isfinite(z)]), initial=0.0)
                with np.errstate(invalid="ignore"):
                    near = np.any(np.abs(z[rows]) <= F64_FLOOR * top, axis=0)
                    live = np.any((z[rows] > F64_FLOOR * top) | np.isnan(z[rows]), axis=0)
                amb = near & ~live                       # (a unit clearly live on another poisoned row is NaN either way)
                flat[off:off + n * k].reshape(n, k)[amb] = True
                flat[off + n * k:off + n * k + n][amb] = True
            off += n * k + n
        for name in ("grad " + net, "param " + net, "exp_avg " + net, "exp_avg_sq " + net, "param target_" + net):
            if name != "param target_policy" or td3:
                out[name] = flat
    return out


def ambiguous_share(st, name):
    """The largest share of one named tensor (a layer's weight or bias) of `name` that is left out."""
    amb = st.meta["ambiguous"].get(name)
    if amb is None:
        return 0.0
    net = name.split(" ", 1)[1].replace("target_", "")
    shapes, names = net_layout(st, net)
    return max(float(np.mean(m)) for m in named_tensors(amb, shapes, names, net).values())


def _bits_equal(a, b):
    a, b = np.asarray(a).astype(np.float32).ravel(), np.asarray(b).astype(np.float32).ravel()
    return a.shape == b.shape and bool(np.all(a.view(np.uint32) == b.view(np.uint32)))


def step_kwargs(algo):
    """Trainer kwargs under which the step under test writes the targets (and TD3's policy)."""
    return dict(target_update_period=1) if algo == "sac" else dict(policy_and_target_update_period=1)


@lru_cache(maxsize=None)
def build(poison, algo, O, A, B, hidden=(256, 256), seed=7):
    """The EdgeState of `poison` (one of POISONS[algo]) with the oracles' verdict in meta.  Cached: treat it as read-only."""
    nets, obs, act, rew, term, nobs, eps = _base(algo, O, A, B, tuple(hidden), seed)
    kw = step_kwargs(algo)
    clean = EdgeState("clean", algo, nets, obs, act, rew, term, nobs, tuple(eps), dict(kw), {})
    if poison in ("next_obs nan", "next_obs nan terminal"):          # the twin differs in the poison alone
        clean.term[ROW] = 1.0 if poison.endswith("terminal") else 0.0
    st = copy.deepcopy(clean)
    st.edge = poison
    rows = _poison(st, poison)
    td3 = algo == "td3"
    rec = {}
    for tag, s, dtype in (("p32", st, torch.float32), ("p64", st, torch.float64), ("c32", clean, torch.float32),
                          ("c64", clean, torch.float64)):
        o = _oracle(s, dtype)
        with np.errstate(all="ignore"):
            rec[tag] = _record(o, o.step(*s.args()), td3)
    p32, c32 = rec["p32"], rec["c32"]
    state_names = [k for k in p32 if not k.startswith(("diag ", "row ", "grad "))]
    st.meta.update(
        classes={k: class_of(v) for k, v in p32.items()}, classes64={k: class_of(v) for k, v in rec["p64"].items()},
        values32=p32, values64=rec["p64"], clean_values32=c32, clean_values64=rec["c64"],
        bit_equal={k for k in state_names if _bits_equal(p32[k], c32[k])},
        same_diags={k[5:] for k in p32 if k.startswith("diag ") and _bits_equal(p32[k], c32[k])},
        ambiguous=_ambiguous(st, rows), clean=clean, rows=rows, state_names=state_names)
    return st


def cases(algo):
    return POISONS[algo]


# ---- pad rows against a poisoned buffer row 0 (tests/test_gpu_step_nonfinite.py) ------------------------------------------
# The buffer seeds draw no index 0 in PAD_STEPS batches of any size below: tests/test_nonfinite_states_host.py asserts it
# on np.random.RandomState itself.
PAD_BUFFER_ROWS, PAD_STEPS, PAD_SEED, PAD_SEED_MEMBER_1, PAD_EVAL_SEED = 3000, 4, 3, 5, 12
PAD_CASES = [("fused B1", 1), ("fused B17", 17), ("fused B255", 255), ("fused B201", 201), ("chain B1009", 1009),
             ("general B129", 129)]                      # label, batch size
PAD_GROUP_BATCHES = (17, 255)


def pad_eval_indices():
    """evaluate_replay's 17 storage rows: none is row 0."""
    return np.random.RandomState(PAD_EVAL_SEED).randint(1, PAD_BUFFER_ROWS, 17)
