// Acting on the device for general-step trainers: policies of any depth and width (included by sac_trainer.hip).
//
// k_act_layer computes ONE layer of the policy's forward pass -- Y = act(X W^T + b) -- for up to SAC_GROUP_MAX members in
// one launch; a call is one launch per layer depth, max(layers) launches on the first member's stream and one wait at the
// end.  It reads the general step's live policy weights where they are (sac_general::net[SAC_NET_POLICY].P: nn.Linear
// layout W [N][K] then b, every matrix on a 16-byte boundary, SAC's two heads merged into one layer of 2A rows): nothing
// is repacked, mirrored or copied.
//
//   table   a launch carries up to SAC_GROUP_MAX jobs (ActLayerJob, device-visible memory, read with scalar loads): a job
//           is one member's layer l.  Launch l holds layer l of every member that has one; a member's head is its last
//           layer, whatever the launch index.
//   grid    one workgroup (4 waves) per 16-row x 64-column output tile of one job; wave w owns columns 16 w .. 16 w + 15
//   GEMM    fp32 MFMA 16x16x4 over K in ascending chunks of AG_KC: the chunk's 16 input rows go through LDS, the weights
//           come straight from global memory, 16 bytes per lane along K (one lane's four consecutive k feed four
//           successive MFMAs, as in k_g_gemm); the next chunk's loads are in flight under this chunk's MFMAs.  Loads are
//           unconditional from clamped indices, and what lies beyond K is zeroed in the edge chunk only (k_g_gemm's
//           comments say why).  The reduction is never split across workgroups.
//   hidden  bias, then x < 0 ? 0 : x (act_hidden_epilogue's ReLU: a NaN stays a NaN)
//   head    at most 32 outputs: one column tile; bias, then through LDS --
//           SAC: tanh(mean) | tanh(mean + exp(clamp(log_std, -20, 2)) * eps);  TD3: tanh(last_fc)
//
// Row independence.  An output element is one MFMA chain over k in an order fixed by K alone (chunk, then the MFMA's index
// inside the chunk): neither the row's place in its block, nor the number of rows, nor the other jobs of the launch
// enter it.  Rows beyond a job's n repeat row n - 1 on the way in and are never written.  n rows are therefore bit for bit
// n one-row calls, and grouped acting is bit for bit solo acting (tests/test_gpu_general_acting.py).
//
// The kernel writes the member's activation scratch (two ping-pong buffers owned by the trainer, used by nothing else)
// and the caller's actions: nothing the step kernels read.  There is no hand-off between workgroups and no wait inside a
// launch: the layers are separate launches.  Observations, eps, actions and the job tables live in the mapped pinned
// staging of sac_act.h (act_stage_reserve).
#pragma once

namespace sac {

constexpr int AG_KC = 128;                // reduction chunk
constexpr int AG_LD = AG_KC + 4;          // LDS row stride of the staged input rows
constexpr int AG_NQ = AG_KC / 16;         // groups of four MFMAs per chunk
constexpr int AG_XE = RB * AG_KC / 256;   // input values of a chunk per thread
constexpr int AG_CT = 64;                 // columns of an output tile
enum { AG_HIDDEN = 0, AG_SAC_MEAN = 1, AG_SAC_SAMPLE = 2, AG_TD3 = 3 };

struct ActLayerJob {
    const float *W, *b;            // [N][K], [N]
    const float *X, *eps;          // input rows [n][K]; head of a stochastic SAC member: the N(0,1) draws [n][A]
    float *Y;                      // hidden layer: [n][N]; head: the actions [n][A]
    int N, K, n, wg0;              // wg0: first workgroup of this job in the launch
    int kind, tiles_n, A, vec;     // vec: W's rows may be fetched in 16-byte pieces (K % 4 == 0)
};

__global__ __launch_bounds__(256) void k_act_layer(const ActLayerJob *__restrict__ tab, int n_jobs) {
    __shared__ __attribute__((aligned(16))) float Xs[RB * AG_LD];
    __shared__ float HL[RB * ACT_HEAD_LD];
    typedef const __attribute__((address_space(1))) f32x4 *gvec;
    typedef __attribute__((address_space(1))) float *gout;
    // this workgroup's job: the last one whose first workgroup is not behind this one (wave-uniform, scalar loads)
    int ji = 0;
    for (int i = 1; i < n_jobs; ++i)
        if ((int)blockIdx.x >= sload(&tab[i].wg0)) ji = i;
    const ActLayerJob *J = tab + ji;
    const float *W = sload(&J->W), *X = sload(&J->X), *bp = sload(&J->b);
    const int N = sload(&J->N), K = sload(&J->K), n = sload(&J->n), kind = sload(&J->kind);
    const int tiles_n = sload(&J->tiles_n);
    const bool vec = sload(&J->vec) != 0;
    const int tile = (int)blockIdx.x - sload(&J->wg0);
    const int row0 = RB * (tile / tiles_n), n0 = AG_CT * (tile % tiles_n);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int ncol = n0 + 16 * wave + c;
    // this lane's weight row and this thread's input elements (chunk coordinates: row xr + 2 j, k = xk), both clamped
    const unsigned wrow = (unsigned)min(ncol, N - 1) * (unsigned)K;
    const int xk = tid & (AG_KC - 1), xr = tid >> 7;
    unsigned xrow[AG_XE];
#pragma unroll
    for (int j = 0; j < AG_XE; ++j) xrow[j] = (unsigned)min(row0 + xr + 2 * j, n - 1) * (unsigned)K;
    const float bias = ld1g(bp + min(ncol, N - 1));

    f32x4 wn[AG_NQ], wc[AG_NQ];
    float xn[AG_XE];
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
#pragma unroll
            for (int j = 0; j < AG_XE; ++j) xn[j] = ld1g(X + (xrow[j] + (unsigned)(kc + xk)));
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
#pragma unroll
        for (int j = 0; j < AG_XE; ++j) xn[j] = ld1g(X + (xrow[j] + (unsigned)min(kc + xk, K - 1)));
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
            for (int j = 0; j < AG_XE; ++j) xn[j] = 0.f;
        }
    };

    f32x4 acc = {};
    const int nS = (K + AG_KC - 1) / AG_KC;
    fetch(0);
    for (int s = 0; s < nS; ++s) {
        const int kc = AG_KC * s;
        if (s > 0) __syncthreads();
#pragma unroll
        for (int q = 0; q < AG_NQ; ++q) wc[q] = wn[q];
        fix(kc);
#pragma unroll
        for (int j = 0; j < AG_XE; ++j) Xs[(xr + 2 * j) * AG_LD + xk] = xn[j];
        __syncthreads();
        if (s + 1 < nS) fetch(kc + AG_KC);
        SB();
#pragma unroll
        for (int q = 0; q < AG_NQ; ++q) {
            const f32x4 a = ld4(Xs + c * AG_LD + 16 * q + 4 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], wc[q][i], acc, 0, 0, 0);
        }
        SB();
    }

    if (kind == AG_HIDDEN) {
        float *Y = sload(&J->Y);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = row0 + 4 * g + i;
            const float v = acc[i] + bias;
            if (row < n && ncol < N) *(gout)(uintptr_t)(Y + ((unsigned)row * (unsigned)N + (unsigned)ncol)) = v < 0.f ? 0.f : v;
        }
        return;
    }
    // the head (one column tile, kind is uniform over the workgroup): pre-activations through LDS, one thread per action
    if (16 * wave < ACT_HEAD_LD) {
#pragma unroll
        for (int i = 0; i < 4; ++i) HL[(4 * g + i) * ACT_HEAD_LD + 16 * wave + c] = acc[i] + bias;
    }
    __syncthreads();
    const int A = sload(&J->A);
    const int r = tid >> 4, a = tid & 15;
    if (a < A && row0 + r < n) {
        const unsigned o = (unsigned)(row0 + r) * (unsigned)A + (unsigned)a;
        float v = HL[r * ACT_HEAD_LD + a];
        if (kind == AG_SAC_SAMPLE) {
            const float ls = fminf(fmaxf(HL[r * ACT_HEAD_LD + A + a], LOG_SIG_MIN), LOG_SIG_MAX);
            v += expf(ls) * ld1g(sload(&J->eps) + o);
        }
        *(gout)(uintptr_t)(sload(&J->Y) + o) = tanhf(v);
    }
}

}  // namespace sac

namespace {

// the two activation buffers of a general-step trainer's acting calls: rows x its widest hidden layer each
int act_general_reserve(sac_trainer *t, size_t floats) {
    if (t->act_gen_floats >= floats) return 0;
    for (float *&p : t->act_gen) { if (p) SAC_HIP(hipFree(p)); p = nullptr; }
    t->act_gen_floats = 0;
    floats = (floats + 16383) & ~(size_t)16383;
    for (float *&p : t->act_gen) SAC_HIP(hipMalloc(reinterpret_cast<void **>(&p), sizeof(float) * floats));
    t->act_gen_floats = floats;
    return 0;
}

}  // namespace

// (declared extern "C" in include/sac_hip.h)
int sac_policy_act_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, const float *const *obs,
                                const int32_t *deterministic, const float *const *eps, float *const *act) {
    SAC_REQUIRE(trainers && n_rows && obs && deterministic && act, "bad arguments to sac_policy_act_general_many");
    SAC_REQUIRE(n_trainers >= 1 && n_trainers <= SAC_GROUP_MAX, "sac_policy_act_general_many takes 1..%d trainers (got %d)",
                SAC_GROUP_MAX, n_trainers);
    // every refusal comes first: nothing has changed when one of them returns
    bool stoch[SAC_GROUP_MAX];
    int active = 0;
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        SAC_REQUIRE(t, "trainer %d is null", i);
        for (int j = 0; j < i; ++j) SAC_REQUIRE(trainers[j] != t, "trainer %d is trainer %d again", i, j);
        SAC_REQUIRE(t->device == trainers[0]->device, "trainer %d lives on device %d, trainer 0 on device %d", i, t->device,
                    trainers[0]->device);
        SAC_REQUIRE(t->gen, "trainer %d has the fused kernels' shapes (two hidden layers of at most 256 units): "
                    "sac_policy_act_device is its device acting entry, sac_policy_act_general serves the general step", i);
        SAC_REQUIRE(t->xcd_mask == 0xffu, "trainer %d is confined by sac_trainer_set_xcd[_mask]: device acting launches on the "
                    "whole chip", i);
        SAC_REQUIRE(n_rows[i] >= 0 && n_rows[i] <= ACT_MAX_ROWS, "trainer %d: %d rows (0..%d per call, 0 = sits out)", i,
                    (int)n_rows[i], ACT_MAX_ROWS);
        stoch[i] = t->algo == 0 && !deterministic[i];
        if (n_rows[i] == 0) continue;
        active += 1;
        SAC_REQUIRE(obs[i] && act[i], "trainer %d: null observations or actions", i);
        SAC_REQUIRE(!stoch[i] || (eps && eps[i]), "trainer %d: stochastic acting needs the N(0,1) draws (eps)", i);
    }
    SAC_REQUIRE(active > 0, "no trainer has rows to act on");
    sac_trainer *t0 = trainers[0];
    SAC_HIP(hipSetDevice(t0->device));
    // the weights as of the last completed step of any step path: drain every member with rows
    for (int i = 0; i < n_trainers; ++i)
        if (n_rows[i] > 0 && sac_sync(trainers[i])) return -1;

    const size_t tab_bytes = (sizeof(ActLayerJob) * SAC_GROUP_MAX * gen::GMAXL + 255) & ~(size_t)255;
    size_t off[SAC_GROUP_MAX][3], bytes = tab_bytes;
    int launches = 0;
    for (int i = 0; i < n_trainers; ++i) {
        sac_trainer *t = trainers[i];
        const size_t n = (size_t)n_rows[i];
        const size_t part[3] = {n * t->O, stoch[i] ? n * t->A : 0, n * t->A};
        for (int k = 0; k < 3; ++k) { off[i][k] = bytes; bytes += (sizeof(float) * part[k] + 255) & ~(size_t)255; }
        if (n == 0) continue;
        const GenNet &P = t->gen->net[SAC_NET_POLICY];
        int widest = 1;
        for (int l = 0; l + 1 < P.nl; ++l) widest = std::max(widest, P.L[l].N);
        if (act_general_reserve(t, n * (size_t)widest)) return -1;
        launches = std::max(launches, P.nl);
    }
    if (act_stage_reserve(t0, bytes)) return -1;
    const sac_trainer::ActStage &S = t0->act_stage;
    ActLayerJob *tab = reinterpret_cast<ActLayerJob *>(S.h);
    int njobs[gen::GMAXL] = {}, blocks[gen::GMAXL] = {};
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        const GenNet &P = t->gen->net[SAC_NET_POLICY];
        const float *x = reinterpret_cast<const float *>(S.d + off[i][0]);
        for (int l = 0; l < P.nl; ++l) {
            const GenLayer &L = P.L[l];
            const bool head = l + 1 == P.nl;
            ActLayerJob &J = tab[(size_t)l * SAC_GROUP_MAX + njobs[l]++];
            J.W = P.P + L.offW; J.b = P.P + L.offB;
            J.X = x;
            J.eps = reinterpret_cast<const float *>(S.d + off[i][1]);
            J.Y = head ? reinterpret_cast<float *>(S.d + off[i][2]) : t->act_gen[l & 1];
            J.N = L.N; J.K = L.K; J.n = n_rows[i]; J.wg0 = blocks[l];
            J.kind = !head ? AG_HIDDEN : (t->algo == 1 ? AG_TD3 : (stoch[i] ? AG_SAC_SAMPLE : AG_SAC_MEAN));
            J.tiles_n = (L.N + AG_CT - 1) / AG_CT;
            J.A = t->A;
            J.vec = (L.K % 4 == 0 && L.offW % 4 == 0) ? 1 : 0;
            blocks[l] += ((n_rows[i] + RB - 1) / RB) * J.tiles_n;
            x = J.Y;
        }
        memcpy(S.h + off[i][0], obs[i], sizeof(float) * (size_t)n_rows[i] * t->O);
        if (stoch[i]) memcpy(S.h + off[i][1], eps[i], sizeof(float) * (size_t)n_rows[i] * t->A);
    }
    for (int l = 0; l < launches; ++l) {
        hipLaunchKernelGGL(k_act_layer, dim3(blocks[l]), dim3(256), 0, t0->stream,
                           reinterpret_cast<const ActLayerJob *>(S.d) + (size_t)l * SAC_GROUP_MAX, njobs[l]);
        SAC_HIP(hipGetLastError());
    }
    if (wait_trainer_stream(t0)) return -1;
    for (int i = 0; i < n_trainers; ++i)
        if (n_rows[i] > 0) memcpy(act[i], S.h + off[i][2], sizeof(float) * (size_t)n_rows[i] * trainers[i]->A);
    return 0;
}

int sac_policy_act_general(sac_trainer_t *t, int64_t n, const float *obs, int deterministic, const float *eps, float *act) {
    SAC_REQUIRE(t && obs && act, "bad arguments to sac_policy_act_general");
    SAC_REQUIRE(n >= 1 && n <= ACT_MAX_ROWS, "sac_policy_act_general: %lld rows (1..%d per call)", (long long)n, ACT_MAX_ROWS);
    const int32_t rows = (int32_t)n, det = deterministic;
    return sac_policy_act_general_many(&t, 1, &rows, &obs, &det, &eps, &act);
}
