// The parameter map: where element e of a network's flat nn.Linear vector (sac_get_params: fc<i>.weight, fc<i>.bias, ...,
// last_fc.weight, last_fc.bias and, on a SAC policy, last_fc_log_std.weight, last_fc_log_std.bias) lives on the device.
// THE one statement of it: parameter and optimizer-state transfer, the written-state readers ("pt_<net>", "g_<net>",
// "pad_nonzero"), sac_param_tensors and k_param_moments all go through param_tensor_list and param_addr.  Free of HIP
// (tests/test_param_map_host.py compiles it with the host compiler alone).
//
// Two families of device layout, one shape record (ParamShape) for both:
//
//   PF_FUSED    the fused kernels' shapes: three device layers of H = 256 units per net, zero-padded, W [Np][Kp] and
//               W^T [Kp + 16][Np] fragment-major (frag_off), b [Np] behind W.  A Q net's first layer reads
//               [obs | pad to KP | act | pad]: its action columns start at KP, not at O (the action-column gap).
//   PF_GENERAL  the general step: any depth and width, W [N][K] row-major on a 16-byte boundary, b [N] behind it, no
//               transposed copy.
//
// In both a SAC policy's two heads are ONE device layer of 2A rows -- [W_mean ; W_log_std], [b_mean ; b_log_std] -- and
// two layers of the flat vector; a TD3 policy (nets 0 and 5, the target policy) has one head of A rows.
#pragma once
#include <stddef.h>

#include "sac_step_plan.h"      // H, round_up

#ifdef __HIPCC__
#define SAC_HD __host__ __device__
#else
#define SAC_HD
#endif

namespace sac {

// Weight matrices AND the feature-major activations ([feature][batch]: rows = features, k = batch row) live in HBM in
// FRAGMENT-MAJOR order: the 16x16 block (row tile, k-chunk) of a [rows][ld] matrix is
// 1 KB contiguous, in MFMA operand order -- lane l = (row & 15) + 16 * ((k & 15) >> 2) holds the four floats k & 3.
// One wave-instruction of the weight stream (a 16x16 fragment, 16 B per lane) then reads 8 whole 128-B lines instead
// of 16 half lines: a kernel's first pass over freshly written weights (cold L2, every step) is bound by the number
// of cache lines per instruction -- scratch/vmem_wall.hip: 66 GB/s per CU for 1 KB-contiguous instructions against
// 33 GB/s for 16 rows x 64 B.
static inline SAC_HD size_t frag_off(int row, int k, int ld) {
    return ((size_t)(row >> 4) * (ld >> 4) + (k >> 4)) * 256 + (size_t)(((row & 15) + 16 * ((k & 15) >> 2)) * 4 + (k & 3));
}

enum { PA_FLAT = 0, PA_FRAG = 1 };

//   PA_FLAT   off + e: every bias, and every weight of the general step
//   PA_FRAG   a weight of the fused kernels' shapes, element (n, k) = (e / K, e % K): k' = k below O, KP + (k - O) from
//             O on, row n + nshift (nshift = A for the log-std head); the forward copy at off + frag_off(n + nshift, k', ld),
//             the transposed copy -- where the weights' Adam moments live (MT / VT) -- at offT + frag_off(k', n + nshift, ldT)
struct ParamAddr {
    long long off, offT;           // PA_FLAT: first element.  PA_FRAG: the layer's offW / offWt
    int kind, K, O, KP, nshift, ld, ldT, pad_;
};

// where flat element e of a tensor lives (transposed: in the transposed copy, PA_FRAG only)
static inline SAC_HD long long param_addr(const ParamAddr &a, long long e, bool transposed) {
    if (a.kind == PA_FLAT) return a.off + e;
    const int n = (int)(e / a.K), k = (int)(e - (long long)n * a.K);
    const int kk = k >= a.O ? a.KP + (k - a.O) : k;
    return transposed ? a.offT + (long long)frag_off(kk, n + a.nshift, a.ldT)
                      : a.off + (long long)frag_off(n + a.nshift, kk, a.ld);
}

struct ParamTensor { ParamAddr a; long long E; };      // one tensor of the flat vector: its E elements in flat order

struct Layer {                     // one device layer (N, K: its device shape; general: Np = N, Kp = K)
    int N, K, Np, Kp;
    long long offW, offB;          // in P / M / V / G : W (fused: [Np][Kp] fragment-major), b
    long long offWt;               // fused, in PT / MT / VT : W^T [Kp + 16][Np] fragment-major
};

enum { PF_FUSED = 0, PF_GENERAL = 1 };
constexpr int PARAM_LAYERS_MAX = 8;                                 // device layers of one net (gen::GMAXL)
constexpr int PARAM_MAX_TENSORS = 2 * PARAM_LAYERS_MAX + 2;         // W and b per layer; a SAC policy's second head

// the nets of a trainer come in two kinds: [0] a policy (nets 0 and 5), [1] a Q net (nets 1..4)
static inline int param_kind(int net) { return (net == 0 || net == 5) ? 0 : 1; }

struct ParamShape {
    int family, algo, O, A, KP;            // algo: 0 SAC, 1 TD3; KP = round_up(O, 16)
    int nh[2], hidden[2][PARAM_LAYERS_MAX];   // per kind: the hidden layers and their logical sizes
    Layer L[2][PARAM_LAYERS_MAX];          // per kind: the nh + 1 device layers
    long long n[2], nT[2];                 // per kind: floats of a forward array (P, M, V, G) / a transposed one (PT, MT, VT)
};

static inline ParamShape param_shape(int family, int algo, int O, int A, const int *hp, int nhp, const int *hq, int nhq) {
    ParamShape S{};
    const bool fused = family == PF_FUSED;
    S.family = family; S.algo = algo; S.O = O; S.A = A; S.KP = round_up(O, 16);
    const int *hid[2] = {hp, hq}, nh[2] = {nhp, nhq};
    for (int q = 0; q < 2; ++q) {
        S.nh[q] = nh[q];
        long long off = 0, offt = 0;
        int d = q ? (fused ? S.KP + 16 : O + A) : O;        // (fused: the padded [obs | act] layout is the device K)
        for (int l = 0; l <= nh[q]; ++l) {
            Layer &L = S.L[q][l];
            if (l < nh[q]) S.hidden[q][l] = hid[q][l];
            L.N = l < nh[q] ? (fused ? H : hid[q][l]) : (q ? 1 : (algo == 0 ? 2 : 1) * A);
            L.K = d;
            L.Np = fused ? round_up(L.N, 16) : L.N; L.Kp = fused ? round_up(L.K, 16) : L.K;
            off = (off + 3) & ~3LL;                          // (16-byte loads of the weights)
            L.offW = off; off += (long long)L.Np * L.Kp;
            L.offB = off; off += L.Np;
            L.offWt = offt; offt += fused ? (long long)(L.Kp + 16) * L.Np : 0;
            d = L.N;
        }
        S.n[q] = (off + 3) & ~3LL; S.nT[q] = offt;
    }
    return S;
}

// the tensors of net `net` in flat order: where each lives.  Returns their number (<= PARAM_MAX_TENSORS).
static inline int param_tensor_list(const ParamShape &S, int net, ParamTensor *out) {
    const int q = param_kind(net), nh = S.nh[q];
    const int heads = (S.algo == 0 && net == 0) ? 2 : 1;
    int n = 0, K = q ? S.O + S.A : S.O;
    for (int l = 0; l <= nh; ++l) {
        const Layer &L = S.L[q][l];
        const int N = l < nh ? S.hidden[q][l] : (q ? 1 : S.A);
        for (int h = 0; h < (l == nh ? heads : 1); ++h) {
            const int nshift = h * S.A;
            ParamTensor &W = out[n++], &B = out[n++];
            W = B = ParamTensor{};
            if (S.family == PF_FUSED) {
                W.a.kind = PA_FRAG; W.a.off = L.offW; W.a.offT = L.offWt;
                W.a.K = K; W.a.O = (q && l == 0) ? S.O : K; W.a.KP = S.KP;
                W.a.nshift = nshift; W.a.ld = L.Kp; W.a.ldT = L.Np;
            } else {
                W.a.kind = PA_FLAT; W.a.off = L.offW + (long long)nshift * K; W.a.K = 1;
            }
            W.E = (long long)N * K;
            B.a.kind = PA_FLAT; B.a.off = L.offB + nshift; B.a.K = 1; B.E = N;
        }
        K = N;
    }
    return n;
}

static inline long long param_count(const ParamTensor *T, int nt) {
    long long n = 0;
    for (int j = 0; j < nt; ++j) n += T[j].E;
    return n;
}

// f(flat index, address) for every element of the list that lives in the forward image (every tensor) or in the
// transposed one (the PA_FRAG weights alone: biases have no transposed copy)
template <typename F>
static inline void param_walk(const ParamTensor *T, int nt, bool transposed, F &&f) {
    long long fi = 0;
    for (int j = 0; j < nt; fi += T[j++].E)
        if (!transposed || T[j].a.kind == PA_FRAG)
            for (long long e = 0; e < T[j].E; ++e) f(fi + e, param_addr(T[j].a, e, transposed));
}

static inline void param_scatter(const ParamTensor *T, int nt, const float *flat, float *image, bool transposed) {
    param_walk(T, nt, transposed, [&](long long fi, long long a) { image[a] = flat[fi]; });
}
static inline void param_gather(const ParamTensor *T, int nt, const float *image, float *flat, bool transposed) {
    param_walk(T, nt, transposed, [&](long long fi, long long a) { flat[fi] = image[a]; });
}
// marks every position of an image that some flat index maps to
static inline void param_reach(const ParamTensor *T, int nt, char *mask, bool transposed) {
    param_walk(T, nt, transposed, [&](long long, long long a) { mask[a] = 1; });
}

}  // namespace sac
