"""The parameter map (csrc/sac_param_map.h) on the host: where element e of a net's flat nn.Linear vector lives on the
device, for the fused kernels' shapes and the general step, SAC and TD3.  The header is compiled with the host C++
compiler alone (which also proves it free of HIP) behind a few-line extern "C" wrapper and checked against a NumPy
restatement that places fc*.weight, fc*.bias, last_fc.* and last_fc_log_std.* from per-layer matrices."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robosuite_benchmark_amd", "csrc")
FUSED, GENERAL, SAC, TD3 = 0, 1, 0, 1
H = 256

WRAPPER = r"""
#include "sac_param_map.h"
using namespace sac;
static ParamShape S;
static ParamTensor T[PARAM_MAX_TENSORS];
// sizes: floats of a policy's forward / transposed array, then of a Q net's
extern "C" void shape(int family, int algo, int O, int A, const int *hp, int nhp, const int *hq, int nhq, long long *sizes) {
    S = param_shape(family, algo, O, A, hp, nhp, hq, nhq);
    for (int q = 0; q < 2; ++q) { sizes[2 * q] = S.n[q]; sizes[2 * q + 1] = S.nT[q]; }
}
extern "C" int tensors(int net, long long *sizes) {
    const int nt = param_tensor_list(S, net, T);
    for (int j = 0; j < nt; ++j) sizes[j] = T[j].E;
    return nt;
}
extern "C" long long count(int net) { return param_count(T, param_tensor_list(S, net, T)); }
extern "C" void scatter(int net, const float *flat, float *image, int tr) { param_scatter(T, param_tensor_list(S, net, T), flat, image, tr); }
extern "C" void gather(int net, const float *image, float *flat, int tr) { param_gather(T, param_tensor_list(S, net, T), image, flat, tr); }
extern "C" void reach(int net, char *mask, int tr) { param_reach(T, param_tensor_list(S, net, T), mask, tr); }
// addr[flat index]: its address (untouched where the image holds no copy of it)
extern "C" void addresses(int net, long long *addr, int tr) {
    param_walk(T, param_tensor_list(S, net, T), tr, [&](long long fi, long long a) { addr[fi] = a; });
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("param_map")
    src, so = d / "map_wrapper.cpp", d / "libparam_map.so"
    src.write_text(WRAPPER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.count.restype = ctypes.c_longlong
    return lib


# ---- the NumPy restatement ------------------------------------------------------------------------------------------------
def pad16(x):
    return (x + 15) // 16 * 16


def frag_off(row, k, ld):
    return ((row >> 4) * (ld >> 4) + (k >> 4)) * 256 + ((row & 15) + 16 * ((k & 15) >> 2)) * 4 + (k & 3)


def split_flat(flat, sizes):
    """The named tensors of a flat vector: [(W [out][in], b [out])] per logical layer -- fc<i>, last_fc and, with two
    heads, last_fc_log_std."""
    out, off = [], 0
    for n, k in sizes:
        out.append((flat[off:off + n * k].reshape(n, k), flat[off + n * k:off + n * k + n]))
        off += n * k + n
    assert off == flat.size
    return out


def logical_layers(algo, O, A, hidden, net):
    """(out, in) of every logical layer of a net in flat order, and how many of the last ones are heads of one device layer."""
    policy = net in (0, 5)
    heads = 2 if (policy and algo == SAC) else 1
    dims, d = [], (O if policy else O + A)
    for h in hidden:
        dims.append((h, d))
        d = h
    dims += [(A if policy else 1, d)] * heads
    return dims, heads


def device_layers(layers, heads):
    """One (W, b) per DEVICE layer: the heads stacked, mean rows first."""
    body, last = layers[:len(layers) - heads], layers[len(layers) - heads:]
    return body + [(np.vstack([w for w, _ in last]), np.concatenate([b for _, b in last]))]


def images(family, algo, O, A, hidden, net, flat):
    """(forward image, transposed image) of a flat vector, pads +0.0."""
    dims, heads = logical_layers(algo, O, A, hidden, net)
    dev = device_layers(split_flat(flat, dims), heads)
    if family == GENERAL:
        off, parts = 0, []
        for w, b in dev:
            al = (off + 3) // 4 * 4
            parts += [np.zeros(al - off, np.float32), w.ravel(), b]
            off = al + w.size + b.size
        parts.append(np.zeros((off + 3) // 4 * 4 - off, np.float32))
        return np.concatenate(parts), np.zeros(0, np.float32)
    KP, q_in = pad16(O), net not in (0, 5)
    fwd, tr = [], []
    for l, (w, b) in enumerate(dev):
        if l == 0 and q_in:                                  # [obs | pad to KP | act | pad]
            wide = np.zeros((w.shape[0], KP + 16), np.float32)
            wide[:, :O], wide[:, KP:KP + A] = w[:, :O], w[:, O:]
            w = wide
        Np, Kp = (H if l < 2 else pad16(w.shape[0])), pad16(w.shape[1] if l == 0 else H)
        D = np.zeros((Np, Kp), np.float32)
        D[:w.shape[0], :w.shape[1]] = w
        rows, ks = np.meshgrid(np.arange(Np), np.arange(Kp), indexing="ij")
        W = np.zeros(Np * Kp, np.float32)
        W[frag_off(rows, ks, Kp)] = D
        WT = np.zeros((Kp + 16) * Np, np.float32)
        WT[frag_off(ks, rows, Np)] = D
        bias = np.zeros(Np, np.float32)
        bias[:b.size] = b
        fwd += [W, bias]
        tr.append(WT)
    return np.concatenate(fwd), np.concatenate(tr)


# ---- the cases -------------------------------------------------------------------------------------------------------------
CASES = [(FUSED, SAC, O, A, [256, 256], [256, 256]) for O, A in ((5, 3), (17, 16), (42, 7), (379, 6))] + [
    (FUSED, SAC, 5, 3, [48, 32], [40, 24]),
    (FUSED, TD3, 5, 3, [256, 256], [256, 256]),
    (FUSED, TD3, 17, 16, [256, 256], [256, 256]),
    (GENERAL, SAC, 5, 3, [21], [21]),
    (GENERAL, SAC, 5, 3, [23, 41, 13], [23, 41, 13]),
    (GENERAL, TD3, 5, 3, [21], [21]),
]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def ptr(a, ty):
    return a.ctypes.data_as(ctypes.POINTER(ty))


@pytest.mark.parametrize("family, algo, O, A, hp, hq", CASES)
def test_the_map_against_numpy(lib, family, algo, O, A, hp, hq):
    sizes = (ctypes.c_longlong * 4)()
    lib.shape(family, algo, O, A, (ctypes.c_int * len(hp))(*hp), len(hp), (ctypes.c_int * len(hq))(*hq), len(hq), sizes)
    for net in range(6 if algo == TD3 else 5):
        policy = net in (0, 5)
        hidden = hp if policy else hq
        dims, _ = logical_layers(algo, O, A, hidden, net)
        n = sum(N * K + N for N, K in dims)
        n_weights = sum(N * K for N, K in dims)
        assert lib.count(net) == n
        per_tensor = (ctypes.c_longlong * 32)()
        assert lib.tensors(net, per_tensor) == 2 * len(dims)
        assert list(per_tensor)[:2 * len(dims)] == [e for N, K in dims for e in (N * K, N)]
        flat = np.arange(1, n + 1, dtype=np.float32)
        want = images(family, algo, O, A, hidden, net, flat)
        size = [sizes[0 if policy else 2], sizes[1 if policy else 3]]
        assert family == FUSED or size[1] == 0
        for tr in (0, 1):
            assert size[tr] == want[tr].size
            covered = n if tr == 0 else (n_weights if family == FUSED else 0)
            # every address inside the array, no two flat indices on one address
            addr = np.full(n, -1, np.int64)
            lib.addresses(net, ptr(addr, ctypes.c_longlong), tr)
            hit = addr[addr >= 0]
            assert hit.size == covered and (hit < size[tr]).all() and np.unique(hit).size == hit.size
            # the reach mask: exactly the addresses
            mask = np.zeros(size[tr] + 1, np.int8)
            lib.reach(net, ptr(mask, ctypes.c_char), tr)
            assert mask.sum() == covered and mask[hit].all() and mask[-1] == 0
            # the scatter equals the NumPy image bit for bit; everything the mask does not cover is +0.0
            img = np.zeros(size[tr] + 1, np.float32)
            lib.scatter(net, ptr(flat, ctypes.c_float), ptr(img, ctypes.c_float), tr)
            assert np.array_equal(bits(img[:-1]), bits(want[tr]))
            assert not bits(img)[mask == 0].any()
            # the gather returns the flat vector (from the transposed image: its weights, the biases left alone)
            back = np.full(n, -1.0, np.float32)
            lib.gather(net, ptr(want[tr], ctypes.c_float) if want[tr].size else None, ptr(back, ctypes.c_float), tr)
            assert np.array_equal(bits(back[addr >= 0]), bits(flat[addr >= 0])) and (back[addr < 0] == -1.0).all()
