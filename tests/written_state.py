"""Helpers of the tests that start from the state the step kernels wrote (tests/test_written_state_host.py,
tests/test_gpu_written_state.py): the oracles rebuilt from a state_dict(), and the checkers of the two invariants of the
fused kernels' padded arrays -- the transposed weight copy equals the forward copy bit for bit, every pad is zero."""
import numpy as np
import torch

from oracle.sac_step_torch import RlkitEquivalentSAC
from oracle.td3_step_torch import RlkitEquivalentTD3
from tests.helpers import layers_from_flat, optimizer_cfg

TRAINED = ("policy", "qf1", "qf2")


# ---- oracles from a state_dict() -----------------------------------------------------------------------------------------
def _adam_entry(step, m, v, dtype):
    """One torch.optim.Adam state entry from float32 values (exact in float64)."""
    as_t = lambda x: torch.from_numpy(np.array(x, np.float32)).to(dtype)        # noqa: E731
    return dict(step=torch.tensor(float(int(step))), exp_avg=as_t(m), exp_avg_sq=as_t(v))


def _set_net_adam(opt, net, shapes, m_flat, v_flat, step, dtype):
    """The Adam state of every parameter of an oracle net from flat moment vectors in library layout (W0 b0 W1 b1 ...)."""
    for l, ((mw, mb), (vw, vb)) in enumerate(zip(layers_from_flat(m_flat, shapes), layers_from_flat(v_flat, shapes))):
        opt.state[net.ws[l]] = _adam_entry(step, mw, vw, dtype)
        opt.state[net.bs[l]] = _adam_entry(step, mb, vb, dtype)


def oracles_from_state(hip, state, with_optimizer_state=True):
    """(float32 oracle, float64 oracle) holding what `state` (a state_dict() of `hip`) holds, as far as it enters the
    gradients, per-row outputs and diagnostics of the NEXT step (what tests/helpers.py check_step_f64 compares):
      SAC: the five nets, log_alpha, log_alpha's Adam state (exp_avg, exp_avg_sq, step = scalars[3]: the oracle steps alpha
           in front of the actor loss, so the alpha of the step depends on it) and n_train_steps_total = scalars[4];
      TD3: the six nets, n_train_steps_total (which steps are policy steps) and qf1's Adam state (step = scalars[3]: the
           actor pass goes through the already updated qf1).
    The other moments only enter what the step writes back (tests/test_gpu_optimizer_step.py).  with_optimizer_state=False
    leaves those Adam states out -- the host test's proof that they matter."""
    cfg = optimizer_cfg(hip)
    td3 = cfg["td3"]
    sc = [float(x) for x in state["scalars"]]
    shapes = {n: cfg["nets"][n][0] for n in TRAINED}
    shapes.update({tgt: shapes[src] for tgt, src in cfg["targets"].items()})
    nets = {n: layers_from_flat(np.asarray(state["params"][n], np.float32), s) for n, s in shapes.items()}
    out = []
    for dtype in (torch.float32, torch.float64):
        if td3:
            o = RlkitEquivalentTD3(nets, hip.act_dim, target_policy_noise=hip.target_policy_noise,
                                   target_policy_noise_clip=hip.target_policy_noise_clip, discount=hip.discount,
                                   reward_scale=hip.reward_scale, policy_learning_rate=hip.policy_learning_rate,
                                   qf_learning_rate=hip.qf_learning_rate,
                                   policy_and_target_update_period=hip.policy_and_target_update_period, tau=hip.tau, dtype=dtype)
            if with_optimizer_state:
                m, v = state["opt"]["qf1"]
                _set_net_adam(o.qf1_opt, o.qf1, shapes["qf1"], m, v, sc[3], dtype)
        else:
            o = RlkitEquivalentSAC(nets, hip.act_dim, discount=hip.discount, reward_scale=hip.reward_scale,
                                   policy_lr=hip.policy_lr, qf_lr=hip.qf_lr, soft_target_tau=hip.soft_target_tau,
                                   target_update_period=hip.target_update_period,
                                   use_automatic_entropy_tuning=hip.use_automatic_entropy_tuning,
                                   target_entropy=hip.target_entropy, dtype=dtype)
            if hip.use_automatic_entropy_tuning:
                with torch.no_grad():
                    o.log_alpha.fill_(float(np.float32(sc[0])))
                if with_optimizer_state:
                    o.alpha_opt.state[o.log_alpha] = _adam_entry(sc[3], [sc[1]], [sc[2]], dtype)
        o.n_train_steps_total = int(sc[4])
        out.append(o)
    return tuple(out)


# ---- the two invariants of the padded arrays -----------------------------------------------------------------------------
def copy_differences(a, b):
    """Indices where two float32 vectors differ as BIT patterns (-0 != +0; a NaN equals the same NaN)."""
    a, b = np.ascontiguousarray(a, np.float32).ravel(), np.ascontiguousarray(b, np.float32).ravel()
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))


def pad_labels(td3, general):
    """The order of debug_fetch("pad_nonzero"): for each trained net (policy, qf1, qf2) the count of elements that are not
    zero, at the positions of its padded arrays that no flat index reaches, in P, PT, MT, VT (fused kernels: forward copy,
    transposed copy, the two transposed Adam moments) or P, M, V (general step); then the count in P of each target net."""
    arrays = ("P", "M", "V") if general else ("P", "PT", "MT", "VT")
    targets = ("target_qf1", "target_qf2") + (("target_policy",) if td3 else ())
    return [f"{net} {a}" for net in TRAINED for a in arrays] + [f"{t} P" for t in targets]


def pad_report(counts, td3, general):
    """{label: count} of the nonzero entries of a pad_nonzero vector (empty: every pad is zero)."""
    labels = pad_labels(td3, general)
    counts = np.asarray(counts).ravel()
    assert counts.size == len(labels), (counts.size, len(labels))
    return {k: float(c) for k, c in zip(labels, counts) if not c == 0}


def check_copies_and_pads(hip, where):
    """Leg A on a trainer: the transposed copy as the backward passes read it ("pt_<net>": weights from PT, biases from P)
    equals the forward copy that every reader sees (state_dict) bit for bit, and no pad element is nonzero.  A trainer of
    the general step keeps one copy: "pt_<net>" is refused there, and its pads are the alignment gaps."""
    td3, general = hasattr(hip, "target_policy"), hip.fused_mode() == 3
    params = hip.state_dict()["params"]
    for net in TRAINED:
        if general:
            try:
                hip.debug_fetch("pt_" + net, params[net].size)
            except RuntimeError as e:
                assert "unknown debug tensor" in str(e), (where, net, str(e))
            else:
                raise AssertionError(f"{where}: a general-step trainer answered pt_{net}")
            continue
        pt = hip.debug_fetch("pt_" + net, params[net].size)
        diff = copy_differences(pt, params[net])
        assert diff.size == 0, (f"{where}: the transposed copy of {net} differs from the forward copy in {diff.size} of "
                                f"{pt.size} elements, first at flat index {int(diff[0])}: PT {pt[diff[0]]!r}, "
                                f"P {params[net][diff[0]]!r}")
    bad = pad_report(hip.debug_fetch("pad_nonzero", 16), td3, general)
    assert not bad, f"{where}: nonzero pad elements {bad}"
