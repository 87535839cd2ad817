"""Reset and shrink-and-perturb on the host: the fresh-value header (csrc/sac_perturb_map.h, compiled with the host C++
compiler alone, which also proves it free of HIP) against infer.fresh_params, fresh_params against the oracle's Philox and
uniform, infer.shrink_perturb_reference (the NumPy statement of sac_shrink_perturb) on small SAC and TD3 states, the
argument refusals of the Python entry points, and the drivers' reset_period over the stand-ins of
test_driver_epochs_host -- none of which needs a device."""
import ctypes
import inspect
import os
import subprocess
from collections import OrderedDict

import numpy as np
import pytest

from oracle import noise_stream
from robosuite_benchmark_amd import _lib, driver, group, infer
from robosuite_benchmark_amd.group import shrink_perturb_many
from tests import test_driver_epochs_host as epochs
from tests.test_recycle_host import sac_trainer, state_of, td3_trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robosuite_benchmark_amd", "csrc")
FUSED, GENERAL, SAC, TD3 = 0, 1, 0, 1
NET_ID = dict(policy=0, qf1=1, qf2=2)

WRAPPER = r"""
#include "sac_perturb_map.h"
using namespace sac;
static ParamShape S;
static ParamTensor T[PARAM_MAX_TENSORS];
extern "C" void shape(int family, int algo, int O, int A, const int *hp, int nhp, const int *hq, int nhq) {
    S = param_shape(family, algo, O, A, hp, nhp, hq, nhq);
}
extern "C" long long count(int net) { return param_count(T, param_tensor_list(S, net, T)); }
extern "C" void fresh(int net, unsigned long long seed, unsigned long long draw, float init_w, float b_init, float *out) {
    perturb_fresh_flat(S, net, seed, draw, init_w, b_init, out);
}
"""


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("perturb_map")
    src, so = d / "perturb_wrapper.cpp", d / "libperturb_map.so"
    src.write_text(WRAPPER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.count.restype = ctypes.c_longlong
    lib.fresh.argtypes = [ctypes.c_int, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_float, ctypes.c_float,
                          ctypes.POINTER(ctypes.c_float)]
    return lib


# (family, O, A, hidden): (1,) with O = A = 1; (300,7,129) with O = 123; tensors of 16384 and of 16383 elements, one chunk
# exactly and one short of it; a fused 379/6 shape
MAP_SHAPES = [(GENERAL, 1, 1, (1,)), (GENERAL, 123, 7, (300, 7, 129)), (GENERAL, 11, 3, (128, 128)), (GENERAL, 11, 3, (127, 129)),
              (FUSED, 379, 6, (256, 256))]
SEED, DRAW = 0xF1E2D3C4B5A69788, 0x0123456789ABCDEF


@pytest.mark.parametrize("algo", [SAC, TD3])
@pytest.mark.parametrize("family, O, A, hidden", MAP_SHAPES)
def test_the_header_draws_fresh_params(lib, family, O, A, hidden, algo):
    t = (sac_trainer if algo == SAC else td3_trainer)(O, A, hidden, hidden)
    hs = (ctypes.c_int * len(hidden))(*hidden)
    lib.shape(family, algo, O, A, hs, len(hidden), hs, len(hidden))
    sizes = set()
    for net, k in NET_ID.items():
        for seed, draw, iw, bi in ((SEED, DRAW, None, None), (7, 0, 0.25, -0.5)):
            want = infer.fresh_params(t, net, seed, draw, iw, bi)
            assert lib.count(k) == want.size == getattr(t, net).flat().size
            got = np.full(want.size, np.nan, np.float32)
            lib.fresh(k, seed, draw, infer.PERTURB_INIT_W[net] if iw is None else iw, infer.B_INIT_VALUE if bi is None else bi,
                      got.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
            assert np.array_equal(bits(got), bits(want)), (net, seed)
        sizes |= {int(np.prod(s)) for _, s in t.param_tensors(net)}
    if hidden == (128, 128):
        assert 16384 in sizes
    if hidden == (127, 129):
        assert 16383 in sizes


def oracle_sign_uniform(k, j, E, seed, draw):
    """s = 2u - 1 of tensor j of net k from the oracle's Philox and uniform, element by element."""
    e = np.arange(E, dtype=np.uint64)
    words = noise_stream.philox4x32(e >> np.uint64(2), j | k << 8, draw & 0xFFFFFFFF, draw >> 32, seed & 0xFFFFFFFF, seed >> 32)
    word = np.choose((e & np.uint64(3)).astype(np.int64), words)
    u = noise_stream.uniform_f32(word)
    assert u.dtype == np.float32
    s = np.float32(2.0) * u - np.float32(1.0)
    assert np.array_equal(s.astype(np.float64), 2.0 * u.astype(np.float64) - 1.0)          # exact in float32
    return s


@pytest.mark.parametrize("make", [sac_trainer, td3_trainer])
def test_fresh_params_against_the_oracle(make):
    t = make(5, 3, (6, 4), (5, 7, 3))
    for net, k in NET_ID.items():
        nh = len(t._hidden(net))
        got = infer.fresh_params(t, net, SEED, DRAW)
        off = 0
        for j, (name, shape) in enumerate(t.param_tensors(net)):
            E = int(np.prod(shape))
            x = got[off:off + E]
            off += E
            if j < 2 * nh and j & 1:
                assert name.endswith(".bias") and np.array_equal(bits(x), bits(np.full(E, infer.B_INIT_VALUE, np.float32)))
                continue
            bound = np.float32(1.0 / np.sqrt(np.float64(shape[0]))) if j < 2 * nh else np.float32(infer.PERTURB_INIT_W[net])
            want = bound * oracle_sign_uniform(k, j, E, SEED, DRAW)
            assert want.dtype == np.float32 and np.array_equal(bits(x), bits(want)), (net, name)
            assert (np.abs(x) <= bound).all(), (net, name)
        assert off == got.size
    # the seed None is the trainer's noise seed; two nets, two tensors and two draws give different words
    assert np.array_equal(bits(infer.fresh_params(t, "qf1", None, 3)), bits(infer.fresh_params(t, "qf1", t.noise_seed, 3)))
    a, b = infer.fresh_params(t, "qf1", SEED, DRAW), infer.fresh_params(t, "qf2", SEED, DRAW)
    assert a.size == b.size and not np.array_equal(bits(a), bits(b))
    assert not np.array_equal(bits(a), bits(infer.fresh_params(t, "qf1", SEED, DRAW + 1)))
    assert not np.array_equal(bits(a), bits(infer.fresh_params(t, "qf1", SEED + 1, DRAW)))
    s0, s2 = oracle_sign_uniform(1, 0, 64, SEED, DRAW), oracle_sign_uniform(1, 2, 64, SEED, DRAW)
    assert not np.array_equal(bits(s0), bits(s2))
    # custom init_w and b_init, per net
    c = infer.fresh_params(t, "policy", 1, 2, init_w=0.5, b_init=-2.0)
    tensors = t.param_tensors("policy")
    n0 = int(np.prod(tensors[0][1]))
    assert np.array_equal(bits(c[n0:n0 + tensors[1][1][0]]), bits(np.full(tensors[1][1][0], -2.0, np.float32)))
    head = int(np.prod(tensors[-2][1])) + tensors[-1][1][0]
    assert np.abs(c[-head:]).max() <= 0.5 and np.abs(c[-head:]).max() > 0.25


def test_the_sign_uniform_is_centred():
    """Over the 4096 x 49 tensor the mean of s is within five standard errors of a uniform on [-1, 1] of 0."""
    t = sac_trainer(49, 3, (4096,), (8,))
    name, shape = t.param_tensors("policy")[0]
    assert shape == (4096, 49)
    n = 4096 * 49
    s = oracle_sign_uniform(0, 0, n, SEED, DRAW).astype(np.float64)
    bound = np.float32(1.0 / np.sqrt(np.float64(4096)))
    assert np.array_equal(bits(infer.fresh_params(t, "policy", SEED, DRAW)[:n]), bits(bound * s.astype(np.float32)))
    assert abs(s.mean()) <= 5.0 / np.sqrt(3.0 * n), s.mean()
    assert s.min() > -1.0 and s.max() <= 1.0


# ---- shrink_perturb_reference ------------------------------------------------------------------------------------------------
def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def copy_state(st):
    return dict(params={k: v.copy() for k, v in st["params"].items()},
                opt={k: (m.copy(), v.copy()) for k, (m, v) in st["opt"].items()}, scalars=st["scalars"].copy())


def plant(st):
    """NaN and Inf in a weight, in a bias and in a target."""
    st["params"]["qf1"][0] = np.nan
    st["params"]["qf1"][-1] = np.inf                                 # (the head's bias)
    st["params"]["policy"][3] = -np.inf
    st["params"]["target_qf2"][5] = np.nan


@pytest.mark.parametrize("make", [sac_trainer, td3_trainer])
def test_shrink_perturb_reference(make):
    t = make()
    st = state_of(t)
    kept = copy_state(st)
    td3 = "target_policy" in t.NETS
    pairs = [("qf1", "target_qf1"), ("qf2", "target_qf2")] + ([("policy", "target_policy")] if td3 else [])

    def untouched_input():
        for k in kept["params"]:
            assert same_bytes(st["params"][k], kept["params"][k])
        for k in kept["opt"]:
            assert all(same_bytes(x, y) for x, y in zip(st["opt"][k], kept["opt"][k]))
        assert same_bytes(st["scalars"], kept["scalars"])

    # a reset: the fresh values themselves, whatever stood there -- NaN and Inf included
    new = infer.shrink_perturb_reference(st, t, None, 0.0, 1.0, SEED, DRAW, opt=True, targets=True)
    untouched_input()
    dirty = copy_state(st)
    plant(dirty)
    for k in dirty["params"]:
        dirty["params"][k][1::2] *= np.float32(-3.0)
    again = infer.shrink_perturb_reference(dirty, t, None, 0.0, 1.0, SEED, DRAW, opt=True, targets=True)
    for net in ("policy", "qf1", "qf2"):
        f = infer.fresh_params(t, net, SEED, DRAW)
        assert same_bytes(new["params"][net], f) and same_bytes(again["params"][net], f)
        assert all(same_bytes(x, np.zeros(f.size, np.float32)) for x in new["opt"][net])
    for net, tg in pairs:
        assert same_bytes(new["params"][tg], new["params"][net]) and same_bytes(again["params"][tg], new["params"][net])
    if not td3:
        assert set(new["params"]) == set(st["params"]) and "target_policy" not in new["params"]
    assert all(np.isfinite(v).all() for v in again["params"].values())
    assert same_bytes(new["scalars"], st["scalars"]) and same_bytes(again["scalars"], dirty["scalars"])
    # shrink != 0: x' = fl(fl(s x) + fl(p f)), and a NaN stays
    sh, pe = np.float32(0.8), np.float32(0.2)
    mixed = infer.shrink_perturb_reference(dirty, t, ("qf2", "qf1"), 0.8, 0.2, SEED, DRAW, opt=False, targets=False)
    for net in ("qf1", "qf2"):
        with np.errstate(all="ignore"):
            want = (sh * dirty["params"][net]).astype(np.float32) + (pe * infer.fresh_params(t, net, SEED, DRAW)).astype(np.float32)
        assert same_bytes(mixed["params"][net], want.astype(np.float32))
        assert all(same_bytes(x, y) for x, y in zip(mixed["opt"][net], dirty["opt"][net]))         # without opt: left alone
        assert same_bytes(mixed["params"]["target_" + net], dirty["params"]["target_" + net])     # without targets: left alone
    assert np.isnan(mixed["params"]["qf1"][0]) and np.isinf(mixed["params"]["qf1"][-1])
    assert same_bytes(mixed["params"]["policy"], dirty["params"]["policy"])                      # not selected
    assert all(same_bytes(x, y) for x, y in zip(mixed["opt"]["policy"], dirty["opt"]["policy"]))
    assert same_bytes(mixed["scalars"], dirty["scalars"])
    # each flag on its own
    only_opt = infer.shrink_perturb_reference(st, t, ("qf1",), 0.8, 0.2, SEED, DRAW, opt=True, targets=False)
    assert all(not x.any() for x in only_opt["opt"]["qf1"]) and same_bytes(only_opt["params"]["target_qf1"], st["params"]["target_qf1"])
    assert all(same_bytes(x, y) for x, y in zip(only_opt["opt"]["qf2"], st["opt"]["qf2"]))
    only_tg = infer.shrink_perturb_reference(st, t, ("qf1",), 0.8, 0.2, SEED, DRAW, opt=False, targets=True)
    assert same_bytes(only_tg["params"]["target_qf1"], only_tg["params"]["qf1"])
    assert same_bytes(only_tg["params"]["target_qf2"], st["params"]["target_qf2"])
    assert all(same_bytes(x, y) for x, y in zip(only_tg["opt"]["qf1"], st["opt"]["qf1"]))
    # perturb = 0: float32(shrink) * x exactly, and no draw behind it (seed and draw do not matter)
    for shrink in (0.5, 0.8, 1.0):
        a = infer.shrink_perturb_reference(st, t, None, shrink, 0.0, 1, 2, opt=False)
        b = infer.shrink_perturb_reference(st, t, None, shrink, 0.0, 3, 4, opt=False)
        for net in ("policy", "qf1", "qf2"):
            assert same_bytes(a["params"][net], np.float32(shrink) * st["params"][net]) and same_bytes(b["params"][net], a["params"][net])
    untouched_input()


# ---- the Python entry points ---------------------------------------------------------------------------------------------------
def test_the_signatures_and_the_abi():
    for cls in (sac_trainer().__class__, td3_trainer().__class__):
        p = inspect.signature(cls.shrink_perturb).parameters
        assert [(k, v.default) for k, v in p.items()][1:] == [
            ("nets", None), ("shrink", 0.8), ("perturb", 0.2), ("seed", None), ("draw", 0), ("opt", True), ("targets", False),
            ("init_w", None), ("b_init", None), ("route", "device")]
        p = inspect.signature(cls.reset_networks).parameters
        assert [(k, v.default) for k, v in p.items()][1:] == [("nets", None), ("seed", None), ("draw", 0), ("alpha", False),
                                                              ("route", "device")]
    assert group.shrink_perturb_many is infer.shrink_perturb_many
    for name in ("SACTrainerGroup", "TD3TrainerGroup", "MixedSACTrainerGroup", "MixedTD3TrainerGroup", "MlpSACTrainerGroup",
                 "MlpTD3TrainerGroup", "ArchSACTrainerGroup", "ArchTD3TrainerGroup"):
        assert inspect.signature(getattr(group, name).shrink_perturb_many).parameters["route"].default == "device", name
    assert [(n, c) for n, c in _lib.SacPerturbIO._fields_] == [
        ("nets", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("shrink", ctypes.c_float), ("perturb", ctypes.c_float),
        ("seed", ctypes.c_uint64), ("draw", ctypes.c_uint64), ("init_w", ctypes.c_float * 3), ("b_init", ctypes.c_float * 3)]
    assert ctypes.sizeof(_lib.SacPerturbIO) == 56 and (_lib.PERTURB_OPT, _lib.PERTURB_TARGETS) == (1, 2)
    assert _lib.SYMBOLS["sac_shrink_perturb"][1] == [ctypes.c_void_p] * 2
    assert _lib.SYMBOLS["sac_shrink_perturb_many"][1] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    header = open(os.path.join(ROOT, "include", "sac_hip.h")).read()
    assert "int sac_shrink_perturb(sac_trainer_t *t, const sac_perturb_io_t *io);" in header
    assert "enum { SAC_PERTURB_OPT = 1, SAC_PERTURB_TARGETS = 2 };" in header


BAD = [
    (dict(nets=()), "at least one network"),
    (dict(nets=("qf1", "qf1")), "each once"),
    (dict(nets=("target_qf1",)), "not a trained net"),
    (dict(nets=("critic",)), "not a trained net"),
    (dict(shrink=-0.5), "not negative"),
    (dict(perturb=-1.0), "not negative"),
    (dict(shrink=float("nan")), "finite"),
    (dict(perturb=float("inf")), "finite"),
    (dict(shrink=1e39), "finite"),
    (dict(shrink=0.0, perturb=0.0), "both zero"),
    (dict(seed=-1), "64-bit"),
    (dict(draw=1 << 64), "64-bit"),
    (dict(seed=1.5), "64-bit"),
    (dict(init_w=-1e-3), "init_w of policy"),
    (dict(init_w=dict(qf2=float("nan"))), "init_w of qf2"),
    (dict(b_init=float("inf")), "b_init of policy"),
    (dict(init_w="big"), "number"),
]


@pytest.mark.parametrize("make", [sac_trainer, td3_trainer])
@pytest.mark.parametrize("kw, what", BAD)
def test_argument_checks(make, kw, what):
    t = make()
    before = {k: getattr(t, k).flat().copy() for k in t.NETS}
    for call in (lambda: t.shrink_perturb(**kw), lambda: infer.shrink_perturb_reference(state_of(t), t, **kw),
                 lambda: shrink_perturb_many([make(seed=1), t], **{{"nets": "nets_list", "seed": "seeds", "draw": "draws"}.get(k, k):
                                                                   ([v, v] if k == "nets" else v) for k, v in kw.items()})):
        with pytest.raises(ValueError, match=what):
            call()
    assert all(same_bytes(getattr(t, k).flat(), before[k]) for k in t.NETS)


def test_more_refusals_and_the_route_without_a_handle():
    t, twin = sac_trainer(), sac_trainer()
    with pytest.raises(RuntimeError, match="route must be one of"):
        t.shrink_perturb(route="gpu")
    with pytest.raises(RuntimeError, match="route must be one of"):
        t.reset_networks(route="gpu")
    with pytest.raises(RuntimeError, match="appears twice"):
        shrink_perturb_many([t, t])
    with pytest.raises(RuntimeError, match="one net selection per trainer"):
        shrink_perturb_many([t], [None, None])
    with pytest.raises(RuntimeError, match="one shrink per trainer"):
        shrink_perturb_many([t, twin], shrink=[0.5])
    with pytest.raises(ValueError, match="not a trained net"):
        sac_trainer().shrink_perturb(("target_policy",))
    # route="device" asked, no handle: the host route, on the holders' arrays
    st = dict(params={k: getattr(twin, k).flat().copy() for k in twin.NETS},
              opt={k: (np.zeros(getattr(twin, k).flat().size, np.float32),) * 2 for k in ("policy", "qf1", "qf2")},
              scalars=np.zeros(6))
    assert t.shrink_perturb(("qf2", "policy"), 0.5, 0.25, seed=9, draw=1, targets=True) == ("policy", "qf2")
    want = infer.shrink_perturb_reference(st, twin, ("policy", "qf2"), 0.5, 0.25, seed=9, draw=1, targets=True)
    for k in t.NETS:
        assert same_bytes(np.ascontiguousarray(getattr(t, k).flat(), np.float32), want["params"][k]), k
    assert not same_bytes(want["params"]["qf2"], st["params"]["qf2"]) and same_bytes(want["params"]["qf1"], st["params"]["qf1"])
    # many: a member that sits out; per-member values; reset_networks is shrink 0, perturb 1, opt, targets
    a, b, c = sac_trainer(seed=1), td3_trainer(seed=2), sac_trainer(seed=3)
    got = shrink_perturb_many([a, b, c], [("qf1",), None, None], shrink=[0.0, 0.5, 0.5], perturb=1.0, seeds=[4, 5, 6], draws=7,
                              targets=True)
    assert got == [("qf1",), None, None]
    assert same_bytes(np.ascontiguousarray(a.qf1.flat(), np.float32), infer.fresh_params(a, "qf1", 4, 7))
    assert same_bytes(np.ascontiguousarray(a.target_qf1.flat(), np.float32), infer.fresh_params(a, "qf1", 4, 7))
    assert b.reset_networks(seed=11, draw=12, alpha=True) == ("policy", "qf1", "qf2")
    for net, tg in (("policy", "target_policy"), ("qf1", "target_qf1"), ("qf2", "target_qf2")):
        f = infer.fresh_params(b, net, 11, 12)
        assert same_bytes(np.ascontiguousarray(getattr(b, net).flat(), np.float32), f)
        assert same_bytes(np.ascontiguousarray(getattr(b, tg).flat(), np.float32), f)


# ---- the drivers: reset_period over the stand-ins of test_driver_epochs_host ----------------------------------------------------
class ResetTrainer(epochs.FakeTrainer):
    def shrink_perturb(self, nets=None, shrink=0.8, perturb=0.2, seed=None, draw=0, opt=True, targets=False, **kw):
        epochs.LOG.append(("shrink_perturb", self.seed, dict(nets=tuple(nets), shrink=shrink, perturb=perturb, seed=seed, draw=draw,
                                                             opt=opt, targets=targets, **kw)))
        p = self.policy.flat()
        rs = np.random.RandomState([seed & 0xFFFFFFFF, seed >> 32, draw & 0xFFFFFFFF, draw >> 32])
        self.policy.load_flat(np.float32(shrink) * p + np.float32(perturb) * rs.uniform(-1, 1, p.size).astype(np.float32))
        return tuple(nets)


def fake_shrink_perturb_many(trainers, nets_list=None, seeds=None, draws=0, **kw):
    epochs.LOG.append(("shrink_perturb_many", None, dict(kw, n=len(trainers))))
    return [t.shrink_perturb(n, seed=s, draw=d, **kw) for t, n, s, d in zip(trainers, nets_list, seeds, draws)]


@pytest.fixture
def stand_ins(monkeypatch):
    for name, fake in dict(SACTrainer=ResetTrainer, EnvReplayBuffer=epochs.FakeBuffer, SACTrainerGroup=epochs.FakeGroup,
                           MixedSACTrainerGroup=epochs.FakeGroup, SyntheticEnv=epochs.LoggingEnv, GroupCheckpoint=epochs.FakeStore,
                           save_checkpoint=epochs.fake_save_checkpoint, load_checkpoint=epochs.fake_load_checkpoint,
                           checkpoint_exists=lambda d: d in epochs.FakeStore.saved,
                           _checkpoint_exists=lambda d: d in epochs.FakeStore.saved,
                           shrink_perturb_many=fake_shrink_perturb_many).items():
        assert hasattr(driver, name), name
        monkeypatch.setattr(driver, name, fake)
    epochs.FakeStore.saved.clear()
    del epochs.LOG[:], epochs.FakeTrainer.made[:]


E3 = 4                                                            # epochs of the driver runs below


def test_the_reset_keywords():
    for fn in (driver.experiment, driver.experiment_group, driver.experiment_sweep):
        p = inspect.signature(fn).parameters
        assert (p["reset_period"].default, p["reset_shrink"].default, p["reset_perturb"].default) == (0, 0.0, 1.0), fn.__name__
    assert driver.RESET_BLOCKS == driver.ROW_BLOCKS + ("reset",) and driver.ROW_BLOCKS == driver.ALL_BLOCKS + ("recycle",)
    sac = epochs.variant()
    for kw, what in ((dict(reset_period=-1), "reset_period"), (dict(reset_period=True), "reset_period"),
                     (dict(reset_period=1.5), "reset_period"), (dict(reset_period=1, reset_shrink=-0.1), "reset_shrink"),
                     (dict(reset_period=1, reset_shrink=0.0, reset_perturb=0.0), "not both 0"),
                     (dict(reset_period=1, reset_perturb=float("nan")), "reset_perturb")):
        with pytest.raises(RuntimeError, match=what):
            driver.experiment(sac, seed=1, num_epochs=1, quiet=True, **kw)
    w = driver._reset_words(3, 2)
    r = [int(x) for x in np.random.RandomState([3, 2, 0x525354]).randint(0, 2**32, 4)]
    assert w == (r[0] | r[1] << 32, r[2] | r[3] << 32) and w != driver._reset_words(3, 1) and w != driver._reset_words(4, 2)
    # scripts/train.py: --reset [E] --reset_shrink S --reset_perturb P
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_script", os.path.join(ROOT, "scripts", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    ap = train.build_parser()
    base = [x for a in ap._actions if a.required for x in (a.option_strings[0], "v.json")]
    a = ap.parse_args(base)
    assert (a.reset, a.reset_shrink, a.reset_perturb) == (0, 0.0, 1.0)
    assert ap.parse_args(base + ["--reset"]).reset == 1
    a = ap.parse_args(base + ["--reset", "5", "--reset_shrink", "0.8", "--reset_perturb", "0.2"])
    assert (a.reset, a.reset_shrink, a.reset_perturb) == (5, 0.8, 0.2)


def test_reset_period_zero_is_the_parents_call(stand_ins):
    plain = {s: epochs.solo(s, num_epochs=E3) for s in epochs.SEEDS}
    for s in epochs.SEEDS:
        epochs.assert_rows_equal(epochs.solo(s, num_epochs=E3, reset_period=0, reset_shrink=0.8, reset_perturb=0.2), plain[s], s)
    for entry in (epochs.group, epochs.sweep):
        got, log = epochs.logged(entry, num_epochs=E3, reset_period=0)
        assert not any(n.startswith("shrink_perturb") for n, _, _ in log)
        for s in epochs.SEEDS:
            epochs.assert_rows_equal(got[s], plain[s], (entry.__name__, s))
            assert not any(k.startswith("reset/") for k in got[s][0])


@pytest.mark.parametrize("period, shrink, perturb", [(1, 0.0, 1.0), (2, 0.8, 0.2), (3, 0.0, 1.0)])
def test_the_drivers_reset(stand_ins, period, shrink, perturb):
    on = dict(num_epochs=E3, reset_period=period, reset_shrink=shrink, reset_perturb=perturb)
    plain = epochs.solo(3, num_epochs=E3)
    want = {}
    for s in epochs.SEEDS:
        want[s], log = epochs.logged(epochs.solo, s, **on)
        due = [e for e in range(E3) if e > 0 and e % period == 0]
        calls = [kw for n, _, kw in log if n == "shrink_perturb"]
        assert [(kw["seed"], kw["draw"]) for kw in calls] == [driver._reset_words(s, e) for e in due]
        assert all(kw["nets"] == ("policy", "qf1", "qf2") and kw["opt"] is True and kw["targets"] is True
                   and (kw["shrink"], kw["perturb"]) == (shrink, perturb) for kw in calls)
        names = [n for n, _, _ in log if n in ("shrink_perturb", "train", "add_paths")]
        for i, n in enumerate(names):                             # directly in front of the training block
            if n == "shrink_perturb":
                assert names[i - 1] == "add_paths" and names[i + 1] == "train"
        for e, row in enumerate(want[s]):
            cols = list(row)
            assert cols[cols.index("reset/Networks") + 1] == "time/data storing (s)"             # the row's last block
            assert row["reset/Networks"] == (3 if e in due else 0), (s, e)
            assert [k for k in cols if k != "reset/Networks"] == list(plain[e])
        epochs.assert_times(want[s], s)
    assert any(a["trainer/QF1 Loss"] != b["trainer/QF1 Loss"] for a, b in zip(want[3], plain))   # (it does change the run)
    for entry, kw in ((epochs.group, dict(acting="host")), (epochs.sweep, dict(acting="host")),
                      (epochs.group, dict(acting="device", sessions=True))):
        got, log = epochs.logged(entry, **kw, **on)
        many = [k for n, _, k in log if n == "shrink_perturb_many"]
        assert len(many) == len(due) and all(k["n"] == len(epochs.SEEDS) for k in many)          # ONE call per reset epoch
        names = [n for n, _, _ in log if n in ("shrink_perturb_many", "train_group")]
        assert names.count("train_group") == E3
        assert all(names[i + 1] == "train_group" for i, n in enumerate(names) if n == "shrink_perturb_many")
        for s in epochs.SEEDS:
            epochs.assert_rows_equal(got[s], want[s], (entry.__name__, s))
            epochs.assert_times(got[s], (entry.__name__, s))


def test_the_reset_block_stands_behind_recycle_and_across_a_resume(stand_ins, tmp_path, monkeypatch):
    on = dict(reset_period=1)
    straight = epochs.group(num_epochs=3, **on)
    ck = str(tmp_path / "ck")
    first = epochs.group(num_epochs=1, checkpoint_dir=ck, **on)
    resumed = epochs.group(num_epochs=3, checkpoint_dir=ck, resume=True, **on)
    for s in epochs.SEEDS:
        epochs.assert_rows_equal(first[s] + resumed[s], straight[s], s)
        assert [r["reset/Networks"] for r in straight[s]] == [0, 3, 3]
    # with recycle_period on as well the reset block is the last one, behind recycle/
    monkeypatch.setattr(driver, "unit_moments_many", lambda trainers, *a, **k: [None] * len(trainers))
    monkeypatch.setattr(driver, "recycle_units_many", lambda trainers, units, **k: [None] * len(trainers))
    rows = epochs.group(num_epochs=2, recycle_period=1, **on)
    cols = list(rows[3][1])
    i = cols.index("recycle/Policy Units")
    assert cols[i:i + 5] == ["recycle/Policy Units", "recycle/QF1 Units", "recycle/QF2 Units", "reset/Networks",
                             "time/data storing (s)"]
