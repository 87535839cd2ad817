// The forward pass of the device inference kernels, once (included by sac_trainer.hip in front of sac_act.h).
//
// Nine kernels run a network forward on live weights without training: k_act, k_act_session, k_qval, k_eval, k_eval_td3
// (the fused kernels' shapes: one workgroup carries a 16-row block through a whole net in LDS) and k_act_layer,
// k_act_layer_session<F64>, k_qval_layer, k_eval_layer<SPLIT> (general shapes: one launch per layer, one workgroup per
// 16 x 64 output tile).
// Each of the fused-shape kernels is a prologue that finds its member, calls into the pieces below, and an epilogue of
// its own.  Each general-shape kernel is a prologue that finds its job (LayerJob) and ONE call:
//
//   kernel                      job found by                   infer_layer_frame<T, SPLIT, Head>
//   k_act_layer                 infer_layer_find               <float, false, LayerHead<false>>
//   k_qval_layer                infer_layer_find               <float, true,  LayerStore>
//   k_eval_layer<false>         infer_layer_find               <float, false, LayerHead<true>>
//   k_eval_layer<true>          infer_layer_find               <float, true,  LayerStore>
//   k_act_layer_session<F64>    the control block, by member   <double | float, false, LayerHead<false>>
//
// Every bit-for-bit promise between them -- a session's actions are the device call's, k_eval's Q values are k_qval's
// and its actions k_act's, the general evaluation's Q columns are sac_q_values_general's and the unit statistics'
// activations k_qval_layer's -- holds because they run THESE functions, not copies of them, on job tables that ONE
// builder writes (LayerSchedule: the layer chain, the ping-pong of the activation scratch, wg0).  A new inference kernel
// composes the same pieces; it does not paste a body, and a new per-layer entry appends chains; it does not spell the
// schedule.
//
//   fused shapes     infer_member, infer_fill, infer_hidden, infer_head, infer_q_out, infer_action
//   general shapes   LayerJob, infer_layer_find, infer_layer_frame = infer_layer_tile + a Head (LayerStore, LayerHead<EVAL>:
//                    infer_layer_store, infer_layer_head / infer_layer_head_eval, infer_action again)
//   host             infer_admit / infer_admit_session / infer_admit_solo (the refusals), InferStage (a grouped call's staging:
//                    carve, reserve, in, dev, back) over infer_carve and act_stage_reserve, infer_slab (a session's slab),
//                    infer_raise_lds, LayerSchedule over infer_widest / infer_layer_job (per-layer job tables, their launches),
//                    infer_scratch_reserve over act_general_reserve (the activation scratch)
#pragma once

#include <atomic>
#include <initializer_list>
#include <type_traits>

namespace sac {

constexpr int ACT_MAX_ROWS = 1024;        // rows per member and call
constexpr int ACT_HEAD_LD = 32;           // head pre-activations [16][32]: mean | log_std (A <= 16)

// ---- fused shapes: two hidden layers of at most 256 units, padded to 256, weights in Net::P (fragment-major) ----

// The hidden layers' bias + ReLU, as the step kernels' hidden_epilogue spells it (relu_nan): x < 0 ? 0 : x, not
// fmaxf(x, 0), which gives 0 for NaN and would turn a non-finite observation row into a finite action, where torch's relu
// and the host forward keep the NaN.  Every finite value comes out as from fmaxf, up to the sign of
// a zero, which no sum downstream can see.  With hidden sizes below 256 an Inf observation becomes NaN already in the
// zero-weight pad units (0 * inf) and from there in every unit of the next layer; torch has no pad units but reaches NaN
// in its second layer too, through inf - inf over units of both signs, so the actions agree (NaN) all the same.
template <int NT>
__device__ __forceinline__ void act_hidden_epilogue(const f32x4 (&acc)[NT], int n_base, int n_stride, const float (&bv)[NT],
                                                    float *Xn, int KL) {
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n = n_base + t * n_stride + c;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float v = acc[t][i] + bv[t];
            Xn[lds_off(4 * g + i, n, KL)] = v < 0.f ? 0.f : v;
        }
    }
}

// this workgroup's member of a per-member table: the last one whose first workgroup (the field wg0) is not behind this
// workgroup (wave-uniform, scalar loads); the field may be a base's (B) of the table's struct
template <class M, class B>
__device__ __forceinline__ int infer_member(const M *tab, int n_members, int B::*wg0) {
    int mi = 0;
    for (int i = 1; i < n_members; ++i)
        if ((int)blockIdx.x >= sload(&(tab[i].*wg0))) mi = i;
    return mi;
}

// the row-block's input X0 [16][KL0]: observations (float, or double rounded by a plain cast) in columns 0..O-1, with
// A > 0 the actions in columns KP..KP+A-1; the other columns and the rows beyond n are zero
template <class T>
__device__ __forceinline__ void infer_fill(float *X0, int KL0, int row0, int n, const T *obs, int O,
                                           const float *act = nullptr, int KP = 0, int A = 0) {
    for (int i = threadIdx.x; i < RB * KL0; i += 256) {
        const int r = i / KL0, k = i - r * KL0;
        float v = 0.f;
        if (row0 + r < n) {
            if (k < O) v = (float)obs[(size_t)(row0 + r) * O + k];
            else if (k >= KP && k < KP + A) v = act[(size_t)(row0 + r) * A + (k - KP)];
        }
        X0[lds_off(r, k, KL0)] = v;
    }
}

// two hidden layers of one net on the row-block in X0: X2 = relu(W1 relu(W0 X0 + b0) + b1).  Wave w owns hidden units
// 64 w .. 64 w + 63 of both layers.  The first layer's weight requests and both layers' biases go out in front of
// fill(), which writes X0 (or nothing, where X0 is in place already); the first barrier stands behind it: X0 is
// complete and a previous net's readers of X1 / X2 are through.  Ends behind a barrier.
template <class Fill>
__device__ __forceinline__ void infer_hidden(const float *P, const long long *offW, const long long *offB, const float *X0,
                                             int KL0, int K0, float *X1, float *X2, Fill fill) {
    const int wave = threadIdx.x >> 6, c = threadIdx.x & 15;
    WRing<4> r0;
    r0.init(P + sload(&offW[0]), K0, 64 * wave, 16);
    r0.fill(K0 >> 4);
    float bv0[4], bv1[4];
    const float *b0 = P + sload(&offB[0]), *b1 = P + sload(&offB[1]);
#pragma unroll
    for (int t = 0; t < 4; ++t) { bv0[t] = b0[64 * wave + 16 * t + c]; bv1[t] = b1[64 * wave + 16 * t + c]; }
    fill();
    lds_barrier();
    {
        f32x4 acc[4] = {};
        gemm_ring(r0, X0, KL0, K0 >> 4, acc);
        act_hidden_epilogue<4>(acc, 64 * wave, 16, bv0, X1, H);
    }
    WRing<4> r1;
    r1.init(P + sload(&offW[1]), H, 64 * wave, 16);
    r1.fill(H >> 4);
    lds_barrier();
    {
        f32x4 acc[4] = {};
        gemm_ring(r1, X1, H, H >> 4, acc);
        act_hidden_epilogue<4>(acc, 64 * wave, 16, bv1, X2, H);
    }
    lds_barrier();
}

// the policy head's pre-activations into HL [16][ACT_HEAD_LD]: wave w owns head rows 16 w .. 16 w + 15 of the NH padded
// ones (wave-uniform).  Ends behind a barrier.
__device__ __forceinline__ void infer_head(const float *P, const long long *offW, const long long *offB, int NH,
                                           const float *X2, float *HL) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    if (16 * wave < NH) {
        WRing<1> rh;
        rh.init(P + sload(&offW[2]), H, 16 * wave, 16);
        rh.fill(H >> 4);
        const float bh = (P + sload(&offB[2]))[16 * wave + c];
        f32x4 acc[1] = {};
        gemm_ring(rh, X2, H, H >> 4, acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) HL[(4 * g + i) * ACT_HEAD_LD + 16 * wave + c] = acc[0][i] + bh;
    }
    lds_barrier();
}

// the Q output unit (row 0 of the padded last layer: wave 0, one tile, column c == 0) into QL [16].  Ends behind a barrier.
__device__ __forceinline__ void infer_q_out(const float *P, const long long *offW, const long long *offB, const float *X2,
                                            float *QL) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    if (wave == 0) {
        WRing<1> rq;
        rq.init(P + sload(&offW[2]), H, 0, 16);
        rq.fill(H >> 4);
        const float bq = (P + sload(&offB[2]))[c];
        f32x4 acc[1] = {};
        gemm_ring(rq, X2, H, H >> 4, acc);
        if (c == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) QL[4 * g + i] = acc[0][i] + bq;
        }
    }
    lds_barrier();
}

__device__ __forceinline__ float infer_log_std(float raw) { return fminf(fmaxf(raw, LOG_SIG_MIN), LOG_SIG_MAX); }

// action a of row r from the head tile HL: tanh(mean), or with `stochastic` tanh(mean + exp(clamp(log_std)) * eps());
// eps is called only then.  *pre gets the value under the tanh.
template <class Eps>
__device__ __forceinline__ float infer_action(const float *HL, int r, int a, int A, bool stochastic, Eps eps,
                                              float *pre = nullptr) {
    float v = HL[r * ACT_HEAD_LD + a];
    if (stochastic) v += expf(infer_log_std(HL[r * ACT_HEAD_LD + A + a])) * eps();
    if (pre) *pre = v;
    return tanhf(v);
}

// ---- general shapes: nn.Linear layout W [N][K] then b, one launch per layer ----

constexpr int AG_KC = 128;                // reduction chunk
constexpr int AG_LD = AG_KC + 4;          // LDS row stride of the staged input rows
constexpr int AG_NQ = AG_KC / 16;         // groups of four MFMAs per chunk
constexpr int AG_XE = RB * AG_KC / 256;   // input values of a chunk per thread
constexpr int AG_CT = 64;                 // columns of an output tile

// One layer of one net for one member's rows: a job of a per-layer launch (device-visible memory, read with scalar
// loads; LayerSchedule, below, is the tables' one writer)
enum { LAYER_STORE = 0,           // a hidden layer or a critic's output unit: infer_layer_store
       LAYER_SAC_MEAN = 1,        // a SAC policy's head, tanh(mean)
       LAYER_SAC_SAMPLE = 2,      // the same head with the draws: tanh(mean + exp(clamp(log_std)) * eps)
       LAYER_TD3 = 3,             // a TD3 policy's head, tanh(last_fc)
       LAYER_EVAL = 4 };          // the stochastic SAC head with what the objectives need: infer_layer_head_eval

struct LayerJob {
    const float *W, *b;            // [N][K], [N]
    const float *X, *X2;           // input rows: columns 0 .. K1-1 from X [n][K1], columns K1 .. K-1 from X2 [n][K - K1].
                                   // The frame reads them as its T: a session's layer 0 keeps FLOAT64 rows behind X
    float *Y;                      // LAYER_STORE: [n][N] (N == 1: the net's row of values, [n]); a head: the actions [n][A]
    const float *eps;              // head: the N(0,1) draws [n][A]
    float *lp, *mu, *ls;           // LAYER_EVAL: log_pi [n]; mean and clamped log_std [n][A], or null
    int N, K, K1, n;
    int wg0, tiles_n, relu, vec;   // wg0: first workgroup of this job in the launch; vec: 16-byte pieces of W's rows
    int kind, A, pad[2];
};

__device__ __forceinline__ double ld1gd(const double *p) { return *(const __attribute__((address_space(1))) double *)(uintptr_t)p; }

struct LayerTile { f32x4 acc; float bias; };       // this lane's four rows (4 g + i) of column ncol, and that column's bias

// One 16-row x 64-column tile of X W^T: rows row0 .. row0 + 15 of the n input rows, wave w's lane column
// ncol = n0 + 16 w + c.  fp32 MFMA 16x16x4 over K in ascending chunks of AG_KC: the chunk's 16 input rows go through LDS
// (Xs [16][AG_LD]), the weights come straight from global memory, 16 bytes per lane along K where `vec` allows it (one
// lane's four consecutive k feed four successive MFMAs, as in k_g_gemm); the next chunk's loads are in flight under
// this chunk's MFMAs.  Loads are unconditional from clamped indices -- rows beyond n repeat row n - 1, columns beyond N
// column N - 1 -- and what lies beyond K is zeroed in the edge chunk only (k_g_gemm's comments say why).
//   T       the input rows' element type: float, or double, which stays double until it goes into LDS (the loads stay
//           in flight) and is rounded there by a plain cast
//   SPLIT   two sources: element k of row r is X[r K1 + k] for k < K1 and X2[r (K - K1) + k - K1] otherwise, both loaded
//           from clamped indices, then a select.  Without it K1 and X2 are unused and the loads are X's alone.
template <class T, bool SPLIT>
__device__ __forceinline__ LayerTile infer_layer_tile(float *Xs, const float *W, const float *bp, const T *X, const T *X2,
                                                      int N, int K, int K1, int n, bool vec, int row0, int ncol) {
    typedef const __attribute__((address_space(1))) f32x4 *gvec;
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
    // this lane's weight row and this thread's input elements (chunk coordinates: row xr + 2 j, k = xk), both clamped
    const unsigned wrow = (unsigned)min(ncol, N - 1) * (unsigned)K;
    const int xk = tid & (AG_KC - 1), xr = tid >> 7;
    const int K2 = K - K1, k2max = max(K2 - 1, 0);
    unsigned xrow[AG_XE], xrow2[AG_XE];
#pragma unroll
    for (int j = 0; j < AG_XE; ++j) {
        const unsigned r = (unsigned)min(row0 + xr + 2 * j, n - 1);
        xrow[j] = r * (unsigned)(SPLIT ? K1 : K);
        if constexpr (SPLIT) xrow2[j] = r * (unsigned)K2;
    }
    LayerTile t;
    t.bias = ld1g(bp + min(ncol, N - 1));
    auto ldx = [](const T *p) -> T {
        if constexpr (std::is_same<T, double>::value) return ld1gd(p); else return ld1g(p);
    };

    f32x4 wn[AG_NQ], wc[AG_NQ];
    T xn[AG_XE];
    // the chunk's input elements (k beyond K is zeroed by fix)
    auto fetch_x = [&](int kc, bool full) {
        const int k = kc + xk;
        if constexpr (SPLIT) {
            const unsigned k1 = (unsigned)min(k, K1 - 1), k2 = (unsigned)min(max(k - K1, 0), k2max);
#pragma unroll
            for (int j = 0; j < AG_XE; ++j) {
                const T a = ldx(X + (xrow[j] + k1)), b = ldx(X2 + (xrow2[j] + k2));
                xn[j] = k < K1 ? a : b;
            }
        } else {
#pragma unroll
            for (int j = 0; j < AG_XE; ++j) xn[j] = ldx(X + (xrow[j] + (unsigned)(full ? k : min(k, K - 1))));
        }
    };
    auto fetch = [&](int kc) {
        if (kc + AG_KC <= K) {
            if (vec) {
#pragma unroll
                for (int q = 0; q < AG_NQ; ++q) wn[q] = *(gvec)(uintptr_t)(W + (wrow + (unsigned)(kc + 16 * q + 4 * g)));
            } else {
#pragma unroll
                for (int q = 0; q < AG_NQ; ++q)
#pragma unroll
                    for (int i = 0; i < 4; ++i) wn[q][i] = ld1g(W + (wrow + (unsigned)(kc + 16 * q + 4 * g + i)));
            }
            fetch_x(kc, true);
            return;
        }
        // the edge chunk: reduction indices clamped (zeroed by fix); whole vectors stay inside K (K % 4 == 0)
        if (vec) {
#pragma unroll
            for (int q = 0; q < AG_NQ; ++q) wn[q] = *(gvec)(uintptr_t)(W + (wrow + (unsigned)min(kc + 16 * q + 4 * g, K - 4)));
        } else {
#pragma unroll
            for (int q = 0; q < AG_NQ; ++q)
#pragma unroll
                for (int i = 0; i < 4; ++i) wn[q][i] = ld1g(W + (wrow + (unsigned)min(kc + 16 * q + 4 * g + i, K - 1)));
        }
        fetch_x(kc, false);
    };
    // behind the loads' arrival: the reduction's zero padding, on both operands
    auto fix = [&](int kc) {
        if (kc + AG_KC <= K) return;
#pragma unroll
        for (int q = 0; q < AG_NQ; ++q)
#pragma unroll
            for (int i = 0; i < 4; ++i) if (kc + 16 * q + 4 * g + i >= K) wc[q][i] = 0.f;
        if (kc + xk >= K) {
#pragma unroll
            for (int j = 0; j < AG_XE; ++j) xn[j] = 0;
        }
    };

    t.acc = f32x4{};
    const int nS = (K + AG_KC - 1) / AG_KC;
    fetch(0);
    for (int s = 0; s < nS; ++s) {
        const int kc = AG_KC * s;
        if (s > 0) __syncthreads();
#pragma unroll
        for (int q = 0; q < AG_NQ; ++q) wc[q] = wn[q];
        fix(kc);
#pragma unroll
        for (int j = 0; j < AG_XE; ++j) Xs[(xr + 2 * j) * AG_LD + xk] = (float)xn[j];
        __syncthreads();
        if (s + 1 < nS) fetch(kc + AG_KC);
        SB();
#pragma unroll
        for (int q = 0; q < AG_NQ; ++q) {
            const f32x4 a = ld4(Xs + c * AG_LD + 16 * q + 4 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) t.acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], wc[q][i], t.acc, 0, 0, 0);
        }
        SB();
    }
    return t;
}

// the tile's values into Y [n][N]: bias, with `relu` x < 0 ? 0 : x (act_hidden_epilogue's ReLU: a NaN stays a NaN).  A
// hidden layer's store; with N == 1 and no relu the Q column: column 0 alone passes ncol < N and lands in Y[row].
__device__ __forceinline__ void infer_layer_store(const LayerTile &t, float *Y, int N, int n, int row0, int ncol, bool relu) {
    typedef __attribute__((address_space(1))) float *gout;
    const int g = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = row0 + 4 * g + i;
        float v = t.acc[i] + t.bias;
        if (relu) v = v < 0.f ? 0.f : v;
        if (row < n && ncol < N) *(gout)(uintptr_t)(Y + ((unsigned)row * (unsigned)N + (unsigned)ncol)) = v;
    }
}

// the policy head of job J (one column tile, kind is uniform over the workgroup): pre-activations through HL, then one
// thread per action; J->A, J->eps and J->Y are read with scalar loads where they are needed
// the head tile's pre-activations (bias added) into HL [16][ACT_HEAD_LD].  Ends behind a barrier.
__device__ __forceinline__ void infer_layer_head_lds(const LayerTile &t, float *HL) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    if (16 * wave < ACT_HEAD_LD) {
#pragma unroll
        for (int i = 0; i < 4; ++i) HL[(4 * g + i) * ACT_HEAD_LD + 16 * wave + c] = t.acc[i] + t.bias;
    }
    __syncthreads();
}

__device__ __forceinline__ void infer_layer_head(const LayerTile &t, float *HL, const LayerJob *J, int kind, int n, int row0) {
    typedef __attribute__((address_space(1))) float *gout;
    infer_layer_head_lds(t, HL);
    const int tid = threadIdx.x;
    const int A = sload(&J->A);
    const int r = tid >> 4, a = tid & 15;
    if (a < A && row0 + r < n) {
        const unsigned o = (unsigned)(row0 + r) * (unsigned)A + (unsigned)a;
        *(gout)(uintptr_t)(sload(&J->Y) + o) =
            infer_action(HL, r, a, A, kind == LAYER_SAC_SAMPLE, [&] { return ld1g(sload(&J->eps) + o); });
    }
}

// infer_layer_head's sibling for loss evaluation: the stochastic SAC head of job J with everything the objectives need
// from it.  The action is infer_action's (bit for bit k_act_layer's LAYER_SAC_SAMPLE action) and goes to J->Y always; log_pi is
// k_eval's expression on the same head values -- Normal.log_prob of the value under the tanh, minus
// log(1 - a^2 + TANH_EPS), summed over the actions by group16_sum -- and goes to J->lp [n]; J->mu / J->ls [n][A], where
// not null, get the mean and the clamped log_std (a NaN stays a NaN: fmaxf would drop it).
__device__ __forceinline__ void infer_layer_head_eval(const LayerTile &t, float *HL, const LayerJob *J, int n, int row0) {
    typedef __attribute__((address_space(1))) float *gout;
    infer_layer_head_lds(t, HL);
    const int tid = threadIdx.x;
    const int A = sload(&J->A);
    const int r = tid >> 4, a = tid & 15;
    const bool live = row0 + r < n;
    float lp = 0.f;
    if (a < A) {
        const unsigned o = (unsigned)(row0 + r) * (unsigned)A + (unsigned)a;
        const float mean = HL[r * ACT_HEAD_LD + a], raw = HL[r * ACT_HEAD_LD + A + a], ls = infer_log_std(raw);
        float v;
        const float actv = infer_action(HL, r, a, A, true, [&] { return live ? ld1g(sload(&J->eps) + o) : 0.f; }, &v);
        const float stdv = expf(ls);
        const float dd = __fsub_rn(v, mean);                             // Normal.log_prob(z)
        const float var = __fmul_rn(stdv, stdv);
        const float nlp = -(dd * dd) / (2.0f * var) - logf(stdv) - 0.91893853320467274178f;
        lp = nlp - logf(1.0f - actv * actv + TANH_EPS);
        if (live) {
            *(gout)(uintptr_t)(sload(&J->Y) + o) = actv;
            float *pm = sload(&J->mu), *pl = sload(&J->ls);
            if (pm) *(gout)(uintptr_t)(pm + o) = mean;
            if (pl) *(gout)(uintptr_t)(pl + o) = raw != raw ? raw : ls;
        }
    }
    const float lsum = group16_sum(lp);
    if (a == 0 && live) *(gout)(uintptr_t)(sload(&J->lp) + (unsigned)(row0 + r)) = lsum;
}

// What follows the tile (the frame's Head).  A kernel gets the epilogues of its Head and no other: LayerStore has no HL
// and no head branch; the two with a head store a hidden layer with its ReLU and send every other kind through HL.
struct LayerStore {                // the critics' launches: every job is a store, ReLU as the job says (off: the output unit)
    static __device__ __forceinline__ void finish(const LayerTile &t, const LayerJob *J, int, int N, int n, int row0, int ncol) {
        infer_layer_store(t, sload(&J->Y), N, n, row0, ncol, sload(&J->relu) != 0);
    }
};
template <bool EVAL>               // a policy's launches: hidden layers, and the acting heads or (EVAL) the evaluation head
struct LayerHead {
    static __device__ __forceinline__ void finish(const LayerTile &t, const LayerJob *J, int kind, int N, int n, int row0, int ncol) {
        __shared__ float HL[RB * ACT_HEAD_LD];
        if (kind == LAYER_STORE) infer_layer_store(t, sload(&J->Y), N, n, row0, ncol, true);
        else if constexpr (EVAL) infer_layer_head_eval(t, HL, J, n, row0);
        else infer_layer_head(t, HL, J, kind, n, row0);
    }
};

// this workgroup's job of a launch's table: the last one whose first workgroup is not behind this one (wave-uniform,
// scalar loads).  A bisection over wg0, which LayerSchedule writes in ascending order: at most 7 dependent loads where a
// scan over the 96 jobs of an evaluation launch would chain 96.
__device__ __forceinline__ const LayerJob *infer_layer_find(const LayerJob *tab, int n_jobs) {
    int lo = 0, hi = n_jobs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int)blockIdx.x >= sload(&tab[mid].wg0)) lo = mid; else hi = mid;
    }
    return tab + lo;
}

// The layer frame: the body of every per-layer kernel behind its prologue, which resolves the job J and, with it, the
// job's first workgroup, its rows and its kind (a session reads those three from its control block).  T and SPLIT are
// infer_layer_tile's: without SPLIT neither X2 nor K1 is loaded.
template <class T, bool SPLIT, class Head>
__device__ __forceinline__ void infer_layer_frame(const LayerJob *J, int wg0, int n, int kind) {
    __shared__ __attribute__((aligned(16))) float Xs[RB * AG_LD];
    const float *W = sload(&J->W), *bp = sload(&J->b);
    const T *X = reinterpret_cast<const T *>(sload(&J->X));
    const int N = sload(&J->N), K = sload(&J->K);
    const int tiles_n = sload(&J->tiles_n);
    const bool vec = sload(&J->vec) != 0;
    const int tile = (int)blockIdx.x - wg0;
    const int row0 = RB * (tile / tiles_n), n0 = AG_CT * (tile % tiles_n);
    const int ncol = n0 + 16 * (threadIdx.x >> 6) + (threadIdx.x & 15);
    const T *X2 = SPLIT ? reinterpret_cast<const T *>(sload(&J->X2)) : X;
    const LayerTile t = infer_layer_tile<T, SPLIT>(Xs, W, bp, X, X2, N, K, SPLIT ? sload(&J->K1) : K, n, vec, row0, ncol);
    Head::finish(t, J, kind, N, n, row0, ncol);
}

}  // namespace sac

// ---- the host halves ----

namespace {

// What an entry's refusals say about itself.  The messages are part of the interface (the tests match them).
struct InferEntry {
    const char *fn;          // the entry's name
    bool general;            // serves general-step trainers and refuses the fused kernels' shapes; false: the reverse
    bool sac_only;           // refuses TD3 trainers
    const char *what;        // "device acting", "device Q evaluation", "device evaluation"
    const char *instead;     // the shape refusal's advice
    const char *rows_to;     // no trainer has rows to ...
    bool both = false;       // serves both families (no forward pass: sac_params.h); `general` and `instead` are unused
    bool td3_only = false;   // refuses SAC trainers (td3_eval.h)
};

// trainer i of a list: not null, not listed twice, on trainer 0's device, of the algorithm and shapes the entry serves
int infer_admit_trainer(const InferEntry &E, sac_trainer_t *const *trainers, int i) {
    const sac_trainer *t = trainers[i];
    SAC_REQUIRE(t, "trainer %d is null", i);
    for (int j = 0; j < i; ++j) SAC_REQUIRE(trainers[j] != t, "trainer %d is trainer %d again", i, j);
    SAC_REQUIRE(t->device == trainers[0]->device, "trainer %d lives on device %d, trainer 0 on device %d", i, t->device,
                trainers[0]->device);
    SAC_REQUIRE(!E.sac_only || t->algo == 0, "trainer %d is a TD3 trainer: this entry evaluates the SAC objective "
                "(entropy-regularised targets of a tanh-Gaussian policy)", i);
    SAC_REQUIRE(!E.td3_only || t->algo == 1, "trainer %d is a SAC trainer: this entry evaluates the TD3 objective (a "
                "deterministic policy with target smoothing); sac_evaluate is the entry for the SAC objective", i);
    if (E.both) return 0;
    if (E.general)
        SAC_REQUIRE(t->gen, "trainer %d has the fused kernels' shapes (two hidden layers of at most 256 units): %s", i, E.instead);
    else
        SAC_REQUIRE(!t->gen, "trainer %d runs the general step (hidden sizes beyond two layers of at most 256 units): %s serves "
                    "the fused kernels' shapes, %s for this trainer", i, E.what, E.instead);
    return 0;
}

// The refusals of a *_many entry, all of them in front of anything that changes: per trainer the list checks above, no
// XCD confinement, the row count, and for a trainer with rows the entry's own checks, member(i).  Then the drain: the
// weights as of the last completed step of any step path (sac_sync re-runs what a fused step that gave up left undone),
// for every member with rows.
template <class Member>
int infer_admit(const InferEntry &E, sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, Member member) {
    SAC_REQUIRE(n_trainers >= 1 && n_trainers <= SAC_GROUP_MAX, "%s takes 1..%d trainers (got %d)", E.fn, SAC_GROUP_MAX,
                n_trainers);
    int active = 0;
    for (int i = 0; i < n_trainers; ++i) {
        if (int rc = infer_admit_trainer(E, trainers, i)) return rc;
        SAC_REQUIRE(trainers[i]->xcd_mask == 0xffu, "trainer %d is confined by sac_trainer_set_xcd[_mask]: %s launches on the "
                    "whole chip", i, E.what);
        SAC_REQUIRE(n_rows[i] >= 0 && n_rows[i] <= ACT_MAX_ROWS, "trainer %d: %d rows (0..%d per call, 0 = sits out)", i,
                    (int)n_rows[i], ACT_MAX_ROWS);
        if (n_rows[i] == 0) continue;
        active += 1;
        if (int rc = member(i)) return rc;
    }
    SAC_REQUIRE(active > 0, "no trainer has rows to %s", E.rows_to);
    SAC_HIP(hipSetDevice(trainers[0]->device));
    for (int i = 0; i < n_trainers; ++i)
        if (n_rows[i] > 0 && sac_sync(trainers[i])) return -1;
    return 0;
}

// the refusals of a *_create entry
int infer_admit_session(const InferEntry &E, sac_trainer_t *const *trainers, int n_trainers, const int32_t *max_rows) {
    SAC_REQUIRE(n_trainers >= 1 && n_trainers <= SAC_GROUP_MAX, "%s takes 1..%d trainers (got %d)", E.fn, SAC_GROUP_MAX,
                n_trainers);
    for (int i = 0; i < n_trainers; ++i) {
        if (int rc = infer_admit_trainer(E, trainers, i)) return rc;
        SAC_REQUIRE(max_rows[i] >= 1 && max_rows[i] <= ACT_MAX_ROWS, "trainer %d: max_rows %d (1..%d)", i, (int)max_rows[i],
                    ACT_MAX_ROWS);
    }
    return 0;
}

// the row count of a one-trainer entry
int infer_admit_solo(const char *fn, int64_t n) {
    SAC_REQUIRE(n >= 1 && n <= ACT_MAX_ROWS, "%s: %lld rows (1..%d per call)", fn, (long long)n, ACT_MAX_ROWS);
    return 0;
}

inline size_t infer_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// carves `count` arrays of part[k] elements out of a buffer that is `bytes` long so far: each on a 256-byte boundary
inline void infer_carve(size_t &bytes, size_t *off, const size_t *part, int count, size_t elem = sizeof(float)) {
    for (int k = 0; k < count; ++k) { off[k] = bytes; bytes += infer_align(elem * part[k]); }
}

// the staging of inference calls (sac_trainer::act_stage, mapped pinned), owned by the trainer that launches: the first
int act_stage_reserve(sac_trainer *t, size_t bytes) {
    sac_trainer::ActStage &S = t->act_stage;
    if (S.bytes >= bytes) return 0;
    if (S.h) SAC_HIP(hipHostFree(S.h));
    S = sac_trainer::ActStage{};
    bytes = (bytes + 65535) & ~(size_t)65535;
    SAC_HIP(hipHostMalloc(reinterpret_cast<void **>(&S.h), bytes, hipHostMallocMapped));
    SAC_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&S.d), S.h, 0));
    S.bytes = bytes;
    return 0;
}

// A grouped call's place in the first member's staging: the kernels' tables in front (head_bytes), then per member its
// parts -- arrays of float, or of elem[k] bytes per element, each on a 256-byte boundary -- in the order of the caller's
// size table.
struct InferStage {
    size_t off[SAC_GROUP_MAX][12], size[SAC_GROUP_MAX][12], bytes;       // size: bytes of a part
    const sac_trainer::ActStage *S = nullptr;                            // behind reserve()
    explicit InferStage(size_t head_bytes) : bytes(infer_align(head_bytes)) {}
    void carve(int i, const size_t *part, int count, const size_t *elem = nullptr) {
        for (int k = 0; k < count; ++k) {
            size[i][k] = (elem ? elem[k] : sizeof(float)) * part[k];
            infer_carve(bytes, off[i] + k, size[i] + k, 1, 1);
        }
    }
    int reserve(sac_trainer *t0) { S = &t0->act_stage; return act_stage_reserve(t0, bytes); }
    // part k of member i on the device (`asked` false: null); as an input, filled from `from` first (null: a kernel in
    // front fills the part)
    template <class T = float>
    T *dev(int i, int k, bool asked = true) const { return asked ? reinterpret_cast<T *>(S->d + off[i][k]) : nullptr; }
    const float *in(int i, int k, const float *from) const {
        if (from) memcpy(S->h + off[i][k], from, size[i][k]);
        return dev(i, k);
    }
    // behind the wait: the parts the caller asked for (dst not null) into its arrays
    struct Back { void *dst; int part; };
    void back(int i, std::initializer_list<Back> table) const {
        for (const Back &b : table)
            if (b.dst) memcpy(b.dst, S->h + off[i][b.part], size[i][b.part]);
    }
};

// the slab of an acting session: the control block, then per member obs (max_rows, O) FLOAT64, eps (max_rows, A) fp32,
// act (max_rows, A) fp32, each 256-byte aligned.  Returns the slab's size.
inline size_t infer_slab(size_t ctl_bytes, sac_trainer_t *const *trainers, int n_trainers, const int32_t *max_rows,
                         size_t (*off)[3]) {
    size_t bytes = infer_align(ctl_bytes);
    for (int i = 0; i < n_trainers; ++i) {
        const size_t rows = (size_t)max_rows[i];
        const size_t part[3] = {sizeof(double) * rows * trainers[i]->O, sizeof(float) * rows * trainers[i]->A,
                                sizeof(float) * rows * trainers[i]->A};
        infer_carve(bytes, off[i], part, 3, 1);
    }
    return bytes;
}

inline void infer_slab_arrays(char *slab_h, const size_t *off, double **obs, float **eps, float **act) {
    if (obs) *obs = reinterpret_cast<double *>(slab_h + off[0]);
    if (eps) *eps = reinterpret_cast<float *>(slab_h + off[1]);
    if (act) *act = reinterpret_cast<float *>(slab_h + off[2]);
}

// A kernel that needs `lds` bytes of dynamic LDS may use them: beyond 48 KB its limit is raised to `most`, once per
// kernel and device (`raised`: the kernel's flags, one per device).
int infer_raise_lds(const void *kernel, std::atomic<bool> (&raised)[64], int device, size_t lds, size_t most) {
    if (lds <= 48 * 1024 || raised[device & 63]) return 0;
    SAC_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
    raised[device & 63] = true;
    return 0;
}

// the widest hidden layer of a general-step net: the columns of its activation scratch
int infer_widest(const GenNet &N) {
    int widest = 1;
    for (int l = 0; l + 1 < N.nl; ++l) widest = std::max(widest, N.L[l].N);
    return widest;
}

// the two activation buffers of a general-step trainer's inference calls (sac_trainer::act_gen), `floats` each.  The
// per-layer entries share them: each call ends with a wait on the stream, so they never overlap
int act_general_reserve(sac_trainer *t, size_t floats) {
    if (t->act_gen_floats >= floats) return 0;
    for (float *&p : t->act_gen) { if (p) SAC_HIP(hipFree(p)); p = nullptr; }
    t->act_gen_floats = 0;
    floats = (floats + 16383) & ~(size_t)16383;
    for (float *&p : t->act_gen) SAC_HIP(hipMalloc(reinterpret_cast<void **>(&p), sizeof(float) * floats));
    t->act_gen_floats = floats;
    return 0;
}

// a member's scratch for `slices` chains side by side: a slice is n rows x the widest hidden layer; *slice (or null)
// gets its floats
int infer_scratch_reserve(sac_trainer *t, int n, int widest, int slices, size_t *slice = nullptr) {
    const size_t floats = (size_t)n * widest;
    if (slice) *slice = floats;
    return act_general_reserve(t, floats * slices);
}

// what every per-layer job says about layer L of net N (vec: W's rows may be fetched in 16-byte pieces)
void infer_layer_job(sac::LayerJob &J, const GenNet &N, const Layer &L) {
    J.W = N.P + L.offW; J.b = N.P + L.offB;
    J.N = L.N; J.K = L.K;
    J.tiles_n = (L.N + AG_CT - 1) / AG_CT;
    J.vec = (L.K % 4 == 0 && L.offW % 4 == 0) ? 1 : 0;
}

// The job tables of a call's per-layer launches and the one place that writes them: table [launch][stride] of LayerJob
// in the staging, per launch the jobs so far and their workgroups.  A chain is one net on one member's rows; a launch
// holds layer l of every chain that has one, in the order of the chain() calls, wg0 ascending (infer_layer_find).
struct LayerSchedule {
    static constexpr int MAX_LAUNCHES = 2 * gen::GMAXL;               // evaluation: the policy's launches, then the critics'
    sac::LayerJob *h = nullptr; const sac::LayerJob *d = nullptr;     // the table: host view, device view
    int stride;                                                       // jobs of one launch, at most
    int launches = 0, njobs[MAX_LAUNCHES] = {}, blocks[MAX_LAUNCHES] = {};
    explicit LayerSchedule(int jobs_per_launch) : stride(jobs_per_launch) {}
    size_t bytes(int max_launches = gen::GMAXL) const { return infer_align(sizeof(sac::LayerJob) * stride * max_launches); }
    void bind(void *host, const void *device) {
        h = static_cast<sac::LayerJob *>(host);
        d = static_cast<const sac::LayerJob *>(device);
    }
    // One chain: net G on n rows, layer l into launch `at` + l.  The first layer reads x | x2 split at K1 (one source:
    // x2 = x, K1 = its K); every later layer reads the layer in front of it, which went to pp[l & 1] + slice -- the
    // ping-pong pair and this chain's slice of it; the last layer (left out without `with_last`: unit statistics stop
    // in front of it) writes `out` with no ReLU.
    struct Chain {
        const GenNet &G;
        const float *x, *x2;
        int K1, n;
        float *const *pp;
        size_t slice;
        float *out;
        bool with_last = true;
        int at = 0;
    };
    // own(J, l) sets what is the caller's: a head's kind, eps, lp, mu and ls, another Y (the chain follows it), the job's
    // companion in a table of the caller's
    template <class Own>
    void chain(const Chain &c, Own own) {
        const GenNet &G = c.G;
        const float *x = c.x, *x2 = c.x2;
        const int n = c.n;
        for (int l = 0; l < (c.with_last ? G.nl : G.nl - 1); ++l) {
            const Layer &L = G.L[l];
            const bool last = l + 1 == G.nl;
            const int launch = c.at + l;
            sac::LayerJob &J = h[(size_t)launch * stride + njobs[launch]++];
            J = sac::LayerJob{};
            infer_layer_job(J, G, L);
            J.X = x; J.X2 = x2; J.K1 = l == 0 ? c.K1 : L.K;
            J.Y = last ? c.out : c.pp[l & 1] + c.slice;
            J.n = n; J.relu = last ? 0 : 1; J.kind = sac::LAYER_STORE;
            J.wg0 = blocks[launch];
            blocks[launch] += ((n + RB - 1) / RB) * J.tiles_n;
            launches = std::max(launches, launch + 1);
            own(J, l);
            x = x2 = J.Y;
        }
    }
    void chain(const Chain &c) { chain(c, [](sac::LayerJob &, int) {}); }
    // launch l of the table on t0's stream
    int launch(void (*kernel)(const sac::LayerJob *, int), sac_trainer *t0, int l) const {
        hipLaunchKernelGGL(kernel, dim3(blocks[l]), dim3(256), 0, t0->stream, d + (size_t)l * stride, njobs[l]);
        SAC_HIP(hipGetLastError());
        return 0;
    }
    int launch_all(void (*kernel)(const sac::LayerJob *, int), sac_trainer *t0) const {
        for (int l = 0; l < launches; ++l)
            if (launch(kernel, t0, l)) return -1;
        return 0;
    }
};

}  // namespace
