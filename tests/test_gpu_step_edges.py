"""GPU: one step from the edge states of tests/edge_states.py -- log-std clamp, full tanh saturation, ReLU at an
exactly-zero pre-activation, pad rows next to the statistics, an all-terminal batch -- on every path that takes the
shape, against the float64 oracle per tensor (tests/helpers.py check_step_f64), and exactly 0 wherever a mask or a
saturation makes the fp32 oracle's gradient exactly 0."""
import numpy as np
import pytest

from tests.edge_states import EDGES, TD3_EDGES, build, pad_detectable, structural_zeros
from tests.helpers import (_net_info, check_f64, check_step_f64, make_pair, make_td3_pair, named_tensors,
                           oracle_flat_grad)

pytestmark = pytest.mark.gpu

# label, algo, environment, (O, A, B), hidden, kind (TD3: whether the critic pass is the fused launch)
PATHS = [("sac kind 1", "sac", {}, (42, 7, 255), (256, 256), 1),
         ("sac kind 1 odd", "sac", {}, (46, 7, 201), (256, 256), 1),
         ("sac kind 0", "sac", dict(SAC_FUSED=0), (42, 7, 255), (256, 256), 0),
         ("sac kind 2", "sac", dict(SAC_CHAIN=1, SAC_CHAIN_BWD=0), (42, 7, 1009), (256, 256), 2),
         ("sac kind 4", "sac", dict(SAC_CHAIN_BWD=1), (46, 7, 1009), (256, 256), 4),
         ("sac kind 3", "sac", dict(SAC_GENERAL=1), (42, 7, 255), (256, 256), 3),
         ("sac kind 3 deep", "sac", {}, (42, 7, 129), (64, 96, 48), 3),
         ("td3 fused critic", "td3", {}, (42, 7, 255), (256, 256), True),
         ("td3 four-launch critic", "td3", dict(SAC_FUSED=0), (42, 7, 255), (256, 256), False),
         ("td3 general", "td3", {}, (42, 7, 129), (64, 96, 48), None)]
ENV = ("SAC_FUSED", "SAC_CHAIN", "SAC_CHAIN_BWD", "SAC_GENERAL", "SAC_CHAIN8", "SAC_BWD8", "SAC_FUSED_TEST_STALL")
CASES = [(p, e) for p in PATHS for e in (EDGES if p[1] == "sac" else TD3_EDGES)]


def _run(path, edge, monkeypatch):
    label, algo, env, (O, A, B), hidden, kind = path
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    st = build(edge, algo, O, A, B, hidden=hidden)
    if algo == "sac":
        o32, hip, o64 = make_pair(O, A, B, nets=st.nets, hidden=hidden, with_f64=True, **st.kw)
        diag = hip.train(st.batch(), eps=st.eps)
    else:
        o32, hip, o64 = make_td3_pair(O, A, B, nets=st.nets, hidden=hidden, with_f64=True, **st.kw)
        diag = hip.train(st.batch(), eps=st.eps[0])
    if algo == "sac":
        assert hip.fused_mode() == kind
    elif kind is None:
        assert hip.fused_mode() == 3
    else:
        assert hip.is_fused() == kind
    want, want64 = o32.step(*st.args()), o64.step(*st.args())
    return st, o32, hip, o64, diag, want, want64


def _grads(hip, o32, o64, net):
    shapes, names = _net_info(o32, net)
    n = sum(a * b + a for a, b in shapes)
    return [named_tensors(x, shapes, names, net) for x in
            (hip.debug_fetch("g_" + net, n), oracle_flat_grad(o32.last["g_" + net]), oracle_flat_grad(o64.last["g_" + net]))]


@pytest.mark.parametrize("path,edge", CASES, ids=[f"{p[0]}-{e}" for p, e in CASES])
def test_edge_state_step(path, edge, monkeypatch):
    st, o32, hip, o64, diag, want, want64 = _run(path, edge, monkeypatch)
    label = path[0]
    # exactly 0 where the construction's masks, saturation or dead units make the fp32 oracle's gradient exactly 0
    zeros = 0
    for net in ("policy", "qf1", "qf2"):
        K, P, _ = _grads(hip, o32, o64, net)
        for k, z in structural_zeros(st, *_net_info(o32, net), net).items():
            zeros += int(z.sum())
            assert np.all(P[k][z] == 0), k
            assert np.all(K[k][z] == 0), (k, "gradient not exactly 0", float(np.max(np.abs(K[k][z]))))
    assert zeros > 0 or edge in ("pad", "terminal")
    check_step_f64(hip, o32, o64, diag, want, want64, path=f"edges {label}")
    B, A = st.act.shape
    if edge == "clamp":
        ls = hip.debug_fetch("log_std", B * A).reshape(B, A)
        assert np.all(ls[:, [0, 2]] == 2.0) and np.all(ls[:, [1, 3]] == -20.0)
        K, P, R = _grads(hip, o32, o64, "policy")
        gb = K["policy last_fc_log_std.bias"]
        assert np.all(gb[st.meta["boundary_cols"]] != 0)             # the boundary passes the gradient
        assert np.all(gb[st.meta["clamped_cols"]] == 0)
    elif edge == "tanh":
        a = hip.debug_fetch("a_new", B * A).reshape(B, A)
        sat = st.meta["saturated_cols"]
        assert np.all(a[:, sat] == np.sign(a[:, sat])) and np.all(np.abs(a[:, sat]) == 1.0)
        last = "last_fc"
        K, P, R = _grads(hip, o32, o64, "policy")
        live = [c for c in range(A) if c not in sat]
        for part in ("weight", "bias"):            # the live rows of the mean head at their own scale
            k = f"policy {last}.{part}"
            check_f64(k + " (unsaturated rows)", K[k][live], P[k][live], R[k][live], f"edges {label}")
            assert np.all(K[k][sat] == 0)
    elif edge == "terminal":
        y = hip.debug_fetch("q_target", B)
        assert np.array_equal(y, (np.float32(3.0) * st.rew.ravel()).astype(np.float32))
    elif edge == "pad":
        assert {"Q1 Predictions", "Q2 Predictions"} <= set(pad_detectable(o64, st))


BAND_PATHS = [p for p in PATHS if p[1] == "sac" and p[5] != 3]


@pytest.mark.parametrize("path", BAND_PATHS, ids=[p[0] for p in BAND_PATHS])
def test_tanh_in_the_ill_conditioned_band(path, monkeypatch):
    """|z| about 7-9: no value is asserted there (1 - a^2 + 1e-6 is ill-conditioned); a = tanh(z) of the kernel's own z to
    2 ulp of float32."""
    label, algo, env, (O, A, B), hidden, kind = path
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    st = build("tanh", algo, O, A, B, hidden=hidden)
    wm, bm = st.nets["policy"][-2]
    wm[:] = 0.0
    bm[:] = np.float32(8.0) * np.sign(np.arange(A) % 2 - 0.5).astype(np.float32)     # +-8: z in about [5, 11]
    _, hip = make_pair(O, A, B, nets=st.nets, hidden=hidden)
    assert hip.fused_mode() == kind
    hip.train(st.batch(), eps=st.eps)
    z = hip.debug_fetch("z", B * A).astype(np.float64)
    a = hip.debug_fetch("a_new", B * A)
    assert np.any((np.abs(z) > 7) & (np.abs(z) < 9))
    want = np.tanh(z).astype(np.float32)
    ulp = np.abs(a.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert ulp.max() <= 2, (int(ulp.max()), label)
