"""GPU: trained state through the parameter map (csrc/sac_param_map.h), no step launched.

Every net's parameters and the trained nets' Adam moments are set to distinct values (arange-based: a permutation cannot
hide) and read back through every reader that goes through the map -- sac_get_params, sac_get_opt_state, "pt_<net>",
"pad_nonzero", sac_param_tensors / sac_param_count -- on the fused kernels' shapes and the general step, SAC and TD3; and
one row tensor and one vector through sac_debug_fetch's table (tests/test_param_map_host.py checks the map itself)."""
import numpy as np
import pytest

from robosuite_benchmark_amd import _lib
from tests.helpers import make_pair, make_td3_pair
from tests.written_state import TRAINED, copy_differences, pad_report

pytestmark = pytest.mark.gpu

B = 16
CASES = [
    ("fused sac 5x3", "sac", 5, 3, dict()),
    ("fused sac 17x16", "sac", 17, 16, dict()),
    ("fused sac, hidden below 256", "sac", 5, 3, dict(hidden=(48, 32), hidden_q=(40, 24))),
    ("fused td3 5x3", "td3", 5, 3, dict()),
    ("general sac [21]", "sac", 5, 3, dict(hidden=(21,))),
    ("general sac [23, 41, 13]", "sac", 5, 3, dict(hidden=(23, 41, 13))),
    ("general td3 [21]", "td3", 5, 3, dict(hidden=(21,))),
]


def _refused(t, name, cap, text):
    with pytest.raises(RuntimeError) as e:
        t.debug_fetch(name, cap)
    assert text in str(e.value), str(e.value)


@pytest.mark.parametrize("label, algo, O, A, kw", CASES, ids=[c[0] for c in CASES])
def test_state_goes_in_and_comes_back(label, algo, O, A, kw):
    td3 = algo == "td3"
    t = (make_td3_pair if td3 else make_pair)(O, A, B, seed=5, **kw)[1]
    general = t.runs_general_step()
    assert general == label.startswith("general")
    lib = _lib.load()
    # distinct values everywhere: net i's parameters i * 1e5 + 1, 2, ..., its moments the same with a fraction
    state = dict(params={}, opt={}, scalars=t.state_dict()["scalars"])
    for name, net in t.NETS.items():
        n = int(lib.sac_param_count(t._h, net))
        ramp = np.arange(1, n + 1, dtype=np.float32) + np.float32(1e5 * net)
        state["params"][name] = ramp
        if name in TRAINED:
            state["opt"][name] = (-(ramp + np.float32(0.5)), ramp + np.float32(0.25))
        sizes = np.zeros(32, np.int64)
        nt = lib.sac_param_tensors(t._h, net, _lib.ptr(sizes))
        assert nt == len(t.param_tensors(name)) and int(sizes[:nt].sum()) == n and not sizes[nt:].any()
        assert [int(s) for s in sizes[:nt]] == [int(np.prod(shape)) for _, shape in t.param_tensors(name)]
    t.load_state_dict(state)
    back = t.state_dict()
    for name in t.NETS:
        assert copy_differences(back["params"][name], state["params"][name]).size == 0, (label, name)
    for name in TRAINED:
        for got, want in zip(back["opt"][name], state["opt"][name]):
            assert copy_differences(got, want).size == 0, (label, name)
        if general:
            _refused(t, "pt_" + name, state["params"][name].size, f"unknown debug tensor 'pt_{name}'")
        else:
            pt = t.debug_fetch("pt_" + name, state["params"][name].size)
            assert copy_differences(pt, state["params"][name]).size == 0, (label, name)
            _refused(t, "pt_" + name, state["params"][name].size - 1, "buffer too small")
    pads = t.debug_fetch("pad_nonzero", 16)
    assert pads.size == (11 if general else 14) + (1 if td3 else 0)
    assert not pad_report(pads, td3, general)
    _refused(t, "pad_nonzero", pads.size - 1, "buffer too small")
    # the fetch table: a row tensor and a vector, rows of the true batch
    assert t.debug_fetch("a_next", B * A + 3).size == B * A and t.debug_fetch("q1", B + 3).size == B
    _refused(t, "a_next", B * A - 1, "buffer too small")
    _refused(t, "q1", B - 1, "buffer too small")
    _refused(t, "no_such_tensor", 4, "unknown debug tensor 'no_such_tensor'")
