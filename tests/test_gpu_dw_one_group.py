"""GPU: the one-group form of the weight-gradient launch (dw_adam_body<true>: batches up to 256 rows, straight-line code,
the MFMAs of a batch chunk wait for that chunk's loads only) against the loop form (SAC_DW_FORM=loop) -- the same bits.

Per case two trainers are created in this process from the same seed, one under SAC_DW_FORM=loop and one with the
default, and run six stepwise steps on device batches with the same rows (two buffers of the same rows and generator
seed); six steps include one Polyak step at period 5 (TD3: three policy steps at period 2).  Compared as raw 32-bit
patterns: every network's parameters (targets included), both Adam moments of the trained networks, the scalars, and the
diagnostics of the first and of the last step."""
import contextlib
import os

import numpy as np
import pytest

from robosuite_benchmark_amd import SACTrainerGroup
from tests.helpers import filled_buffer, make_pair, make_td3_pair

pytestmark = pytest.mark.gpu
STEPS, ROWS = 6, 700


@contextlib.contextmanager
def dw_form(value):
    old = os.environ.get("SAC_DW_FORM")
    try:
        if value is None:
            os.environ.pop("SAC_DW_FORM", None)
        else:
            os.environ["SAC_DW_FORM"] = value
        yield
    finally:
        if old is None:
            os.environ.pop("SAC_DW_FORM", None)
        else:
            os.environ["SAC_DW_FORM"] = old


def both_forms(make):
    """make() under SAC_DW_FORM=loop, then with the default (the form is chosen when the trainer is created)."""
    with dw_form("loop"):
        loop = make()
    with dw_form(None):
        one = make()
    return loop, one


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def assert_same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    ba, bb = bits(a), bits(b)
    assert np.array_equal(ba, bb), (what, int(np.count_nonzero(ba != bb)), "words differ")


def assert_same_state(loop, one, where):
    sa, sb = loop.state_dict(), one.state_dict()
    assert set(sa["params"]) == set(sb["params"]) == set(loop.NETS)
    for name in sa["params"]:
        assert_same_bits(sa["params"][name], sb["params"][name], (where, "params", name))
    for name in ("policy", "qf1", "qf2"):
        for which, x, y in zip(("m", "v"), sa["opt"][name], sb["opt"][name]):
            assert_same_bits(x, y, (where, "adam " + which, name))
    assert_same_bits(sa["scalars"], sb["scalars"], (where, "scalars"))


def stepwise(t, buf, B):
    """six steps of the stepwise interface on device batches; the diagnostics of the first and of the last step"""
    out = []
    for i in range(STEPS):
        if i == STEPS - 1:
            t.end_epoch(0)                      # the last step publishes its diagnostics too
        batch = buf.random_batch(B)
        assert batch.on_device
        out.append(t.train(batch))
    assert out[0] is not None and out[-1] is not None and all(o is None for o in out[1:-1])
    return out[0], out[-1]


def check_solo(make, O, A, B, where):
    loop, one = both_forms(make)
    fresh = one.state_dict()["params"]
    d_loop = stepwise(loop, filled_buffer(ROWS, O, A, 21), B)
    d_one = stepwise(one, filled_buffer(ROWS, O, A, 21), B)
    for which, x, y in zip(("first", "last"), d_loop, d_one):
        assert np.all(np.isfinite(x)), (where, which)
        assert_same_bits(x, y, (where, "diagnostics", which))
    assert_same_state(loop, one, where)
    # the steps did something: parameters moved, and the Polyak step moved the targets
    now = one.state_dict()["params"]
    for name in ("policy", "qf1", "target_qf1"):
        assert not np.array_equal(fresh[name], now[name]), (where, name, "unchanged after six steps")


# obs/act: 5/2 one 16-column first-layer chunk (nv = 1); 42/7 a 48-wide policy first layer (wave 3's tile outside) and a
# 64-wide Q one; 89/14 a first layer as strip plus tail entry.  batch: 1 (waves 1-3 hold no chunk), 16, 17, 64 (one chunk
# per wave), 80 (rem = 1), 250, 256, and 300 (the loop form on both sides).
@pytest.mark.parametrize("B", [1, 16, 17, 64, 80, 250, 256, 300])
@pytest.mark.parametrize("O,A", [(5, 2), (42, 7), (89, 14)])
def test_one_group_form_equals_loop_form(O, A, B):
    check_solo(lambda: make_pair(O, A, B, seed=6, noise_seed=31)[1], O, A, B, (O, A, B))


def test_td3_one_group_form_equals_loop_form():
    O, A, B = 42, 7, 256
    check_solo(lambda: make_td3_pair(O, A, B, seed=6, noise_seed=31)[1], O, A, B, ("td3", O, A, B))


def test_group_one_group_form_equals_loop_form():
    O, A, B = 42, 7, 64
    make = lambda: [make_pair(O, A, B, seed=8 + i, noise_seed=40 + i)[1] for i in range(2)]
    loop, one = both_forms(make)
    outs = []
    for members in (loop, one):
        bufs = [filled_buffer(ROWS + 100 * i, O, A, 50 + i) for i in range(2)]
        outs.append(SACTrainerGroup(members).train_loop(bufs, STEPS, batch_size=B))
    for which, x, y in zip(("first", "last"), outs[0], outs[1]):
        assert np.all(np.isfinite(x)), which
        assert_same_bits(np.asarray(x), np.asarray(y), ("group diagnostics", which))
    for r in range(2):
        assert_same_state(loop[r], one[r], ("group member", r))
