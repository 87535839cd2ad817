// Evaluating the critics on the device for general-step trainers: Q networks of any depth and width (included by
// sac_trainer.hip).
//
// k_qval_layer computes ONE layer of the Q networks' forward pass -- Y = f(X W^T + b) -- for up to SAC_GROUP_MAX members
// times up to 4 selected nets in one launch; a call is one launch per layer depth, max(layers) launches on the first
// member's stream and one wait at the end: k_act_layer's scheme (sac_act_general.h).  It reads the general step's live
// critic weights where they are (sac_general::net[SAC_NET_QF1 .. SAC_NET_TARGET_QF2].P: nn.Linear layout W [N][K] then
// b, at GenLayer::offW / offB): nothing is repacked, mirrored or copied.
//
//   table   a launch carries up to QG_JOBS = 4 SAC_GROUP_MAX jobs (QvalLayerJob, device-visible memory, read with scalar
//           loads): a job is (member, selected net, layer l).  Launch l holds layer l of every (member, net) that has
//           one; a net's output layer is its last layer, whatever the launch index.  A workgroup finds its job by a
//           bisection over wg0 (ascending): at most 6 dependent scalar loads where a scan would chain 64.
//   grid    one workgroup (4 waves) per 16-row x 64-column output tile of one job; wave w owns columns 16 w .. 16 w + 15
//   GEMM    fp32 MFMA 16x16x4 over K in ascending chunks of AG_KC: the chunk's 16 input rows go through LDS, the weights
//           come straight from global memory, 16 bytes per lane along K where K % 4 == 0 and offW % 4 == 0; the next
//           chunk's loads are in flight under this chunk's MFMAs.  Loads are unconditional from clamped indices, and what
//           lies beyond K is zeroed in the edge chunk only.  The reduction is never split across workgroups.
//   input   two sources and a split point K1: element k of row r is X[r K1 + k] for k < K1 and X2[r (K - K1) + k - K1]
//           otherwise -- both loads from clamped indices, then a select.  The first layer reads cat(obs, act) this way
//           (X = obs, X2 = act, K1 = O: the host stages the two blocks and never builds the concatenated rows; all
//           selected nets of a member read the same two blocks); hidden layers set K1 = K and X2 = X.
//   hidden  bias, then x < 0 ? 0 : x (act_hidden_epilogue's ReLU: a NaN stays a NaN)
//   output  N = 1: the same tile with the columns clamped to the one weight row -- every column of the tile computes the
//           net's value by the same MFMA chain, column 0 of wave 0 stores it: bias, no activation, row r of selected net s
//           to q[s n + r].  The order of summation is that of any other column: it depends on K alone.
//
// Row independence.  An output element is one MFMA chain over k in an order fixed by K alone (chunk, then the MFMA's index
// inside the chunk): neither the row's place in its block, nor the number of rows, nor the other nets selected, nor the
// other jobs of the launch enter it.  Rows beyond a job's n repeat row n - 1 on the way in and are never written.  n rows
// are therefore bit for bit n one-row calls, and grouped evaluation is bit for bit solo evaluation
// (tests/test_gpu_q_values_general.py).
//
// The kernel writes the member's activation scratch and the caller's Q values: nothing the step kernels read.  The
// scratch is the trainer's act_gen pair (act_general_reserve), shared with sac_policy_act_general: each buffer holds
// n_sel slices of n x the widest hidden layer.  Acting and Q calls each end with a wait on the trainer's stream, so they
// never overlap; acting sessions own their scratch.  Worst case 4 nets x 1024 rows x 4096 units x 4 bytes x 2 buffers =
// 128 MB per trainer.  Vector stores only.
#pragma once

namespace sac {

constexpr int QG_JOBS = 4 * SAC_GROUP_MAX;      // jobs of one launch

struct QvalLayerJob {
    const float *W, *b;            // [N][K], [N]
    const float *X, *X2;           // input rows: columns 0 .. K1-1 from X [n][K1], columns K1 .. K-1 from X2 [n][K - K1]
    float *Y;                      // hidden layer: [n][N]; output layer (N == 1): the net's row of q, [n]
    int N, K, K1, n;
    int wg0, tiles_n, relu, vec;   // wg0: first workgroup of this job in the launch; vec: 16-byte pieces of W's rows
};

__global__ __launch_bounds__(256) void k_qval_layer(const QvalLayerJob *__restrict__ tab, int n_jobs) {
    __shared__ __attribute__((aligned(16))) float Xs[RB * AG_LD];
    typedef const __attribute__((address_space(1))) f32x4 *gvec;
    typedef __attribute__((address_space(1))) float *gout;
    // this workgroup's job: the last one whose first workgroup is not behind this one (wave-uniform, scalar loads)
    int lo = 0, hi = n_jobs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int)blockIdx.x >= sload(&tab[mid].wg0)) lo = mid; else hi = mid;
    }
    const QvalLayerJob *J = tab + lo;
    const float *W = sload(&J->W), *X = sload(&J->X), *X2 = sload(&J->X2), *bp = sload(&J->b);
    const int N = sload(&J->N), K = sload(&J->K), K1 = sload(&J->K1), n = sload(&J->n);
    const int tiles_n = sload(&J->tiles_n);
    const bool vec = sload(&J->vec) != 0, relu = sload(&J->relu) != 0;
    const int tile = (int)blockIdx.x - sload(&J->wg0);
    const int row0 = RB * (tile / tiles_n), n0 = AG_CT * (tile % tiles_n);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int ncol = n0 + 16 * wave + c;
    // this lane's weight row and this thread's input elements (chunk coordinates: row xr + 2 j, k = xk), both clamped
    const unsigned wrow = (unsigned)min(ncol, N - 1) * (unsigned)K;
    const int xk = tid & (AG_KC - 1), xr = tid >> 7;
    const int K2 = K - K1, k2max = max(K2 - 1, 0);
    unsigned xrow[AG_XE], xrow2[AG_XE];
#pragma unroll
    for (int j = 0; j < AG_XE; ++j) {
        const unsigned r = (unsigned)min(row0 + xr + 2 * j, n - 1);
        xrow[j] = r * (unsigned)K1; xrow2[j] = r * (unsigned)K2;
    }
    const float bias = ld1g(bp + min(ncol, N - 1));

    f32x4 wn[AG_NQ], wc[AG_NQ];
    float xn[AG_XE];
    // the chunk's input elements: both sources from clamped indices, then the select (k beyond K is zeroed by fix)
    auto fetch_x = [&](int kc) {
        const int k = kc + xk;
        const unsigned k1 = (unsigned)min(k, K1 - 1), k2 = (unsigned)min(max(k - K1, 0), k2max);
#pragma unroll
        for (int j = 0; j < AG_XE; ++j) {
            const float a = ld1g(X + (xrow[j] + k1)), b = ld1g(X2 + (xrow2[j] + k2));
            xn[j] = k < K1 ? a : b;
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
            fetch_x(kc);
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
        fetch_x(kc);
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

    // hidden layer: ReLU; output layer (N == 1, relu == 0): column 0 alone passes ncol < N and lands in q[s n + row]
    float *Y = sload(&J->Y);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = row0 + 4 * g + i;
        float v = acc[i] + bias;
        if (relu) v = v < 0.f ? 0.f : v;
        if (row < n && ncol < N) *(gout)(uintptr_t)(Y + ((unsigned)row * (unsigned)N + (unsigned)ncol)) = v;
    }
}

}  // namespace sac

// (declared extern "C" in include/sac_hip.h)
int sac_q_values_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, const float *const *obs,
                              const float *const *act, const uint32_t *nets, float *const *q) {
    SAC_REQUIRE(trainers && n_rows && obs && act && nets && q, "bad arguments to sac_q_values_general_many");
    SAC_REQUIRE(n_trainers >= 1 && n_trainers <= SAC_GROUP_MAX, "sac_q_values_general_many takes 1..%d trainers (got %d)",
                SAC_GROUP_MAX, n_trainers);
    // every refusal comes first: nothing has changed when one of them returns
    int active = 0;
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        SAC_REQUIRE(t, "trainer %d is null", i);
        for (int j = 0; j < i; ++j) SAC_REQUIRE(trainers[j] != t, "trainer %d is trainer %d again", i, j);
        SAC_REQUIRE(t->device == trainers[0]->device, "trainer %d lives on device %d, trainer 0 on device %d", i, t->device,
                    trainers[0]->device);
        SAC_REQUIRE(t->gen, "trainer %d has the fused kernels' shapes (two hidden layers of at most 256 units): sac_q_values "
                    "is its device Q evaluation entry, sac_q_values_general serves the general step", i);
        SAC_REQUIRE(t->xcd_mask == 0xffu, "trainer %d is confined by sac_trainer_set_xcd[_mask]: device Q evaluation launches "
                    "on the whole chip", i);
        SAC_REQUIRE(n_rows[i] >= 0 && n_rows[i] <= ACT_MAX_ROWS, "trainer %d: %d rows (0..%d per call, 0 = sits out)", i,
                    (int)n_rows[i], ACT_MAX_ROWS);
        if (n_rows[i] == 0) continue;
        active += 1;
        SAC_REQUIRE(nets[i] != 0 && nets[i] <= 15u, "trainer %d: nets 0x%x selects no Q network or an unknown one (bits "
                    "SAC_Q_QF1 | SAC_Q_QF2 | SAC_Q_TARGET_QF1 | SAC_Q_TARGET_QF2)", i, (unsigned)nets[i]);
        SAC_REQUIRE(obs[i] && act[i] && q[i], "trainer %d: null observations, actions or Q values", i);
    }
    SAC_REQUIRE(active > 0, "no trainer has rows to evaluate");
    sac_trainer *t0 = trainers[0];
    SAC_HIP(hipSetDevice(t0->device));
    // the weights as of the last completed step of any step path: drain every member with rows
    for (int i = 0; i < n_trainers; ++i)
        if (n_rows[i] > 0 && sac_sync(trainers[i])) return -1;

    const size_t tab_bytes = (sizeof(QvalLayerJob) * QG_JOBS * gen::GMAXL + 255) & ~(size_t)255;
    size_t off[SAC_GROUP_MAX][3], slice[SAC_GROUP_MAX] = {}, bytes = tab_bytes;
    int launches = 0;
    for (int i = 0; i < n_trainers; ++i) {
        sac_trainer *t = trainers[i];
        const size_t n = (size_t)n_rows[i];
        const size_t part[3] = {n * t->O, n * t->A, n ? n * __builtin_popcount(nets[i]) : 0};
        for (int k = 0; k < 3; ++k) { off[i][k] = bytes; bytes += (sizeof(float) * part[k] + 255) & ~(size_t)255; }
        if (n == 0) continue;
        const GenNet &Q = t->gen->net[SAC_NET_QF1];                    // (the four Q nets share their layout)
        int widest = 1;
        for (int l = 0; l + 1 < Q.nl; ++l) widest = std::max(widest, Q.L[l].N);
        slice[i] = n * (size_t)widest;
        if (act_general_reserve(t, slice[i] * __builtin_popcount(nets[i]))) return -1;
        launches = std::max(launches, Q.nl);
    }
    if (act_stage_reserve(t0, bytes)) return -1;
    const sac_trainer::ActStage &S = t0->act_stage;
    QvalLayerJob *tab = reinterpret_cast<QvalLayerJob *>(S.h);
    int njobs[gen::GMAXL] = {}, blocks[gen::GMAXL] = {};
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        const float *o = reinterpret_cast<const float *>(S.d + off[i][0]);
        const float *a = reinterpret_cast<const float *>(S.d + off[i][1]);
        int s = 0;
        for (int k = 0; k < 4; ++k) {
            if (!(nets[i] >> k & 1u)) continue;
            const GenNet &Q = t->gen->net[SAC_NET_QF1 + k];
            const float *x = o, *x2 = a;
            for (int l = 0; l < Q.nl; ++l) {
                const GenLayer &L = Q.L[l];
                const bool last = l + 1 == Q.nl;
                QvalLayerJob &J = tab[(size_t)l * QG_JOBS + njobs[l]++];
                J.W = Q.P + L.offW; J.b = Q.P + L.offB;
                J.X = x; J.X2 = x2;
                J.Y = last ? reinterpret_cast<float *>(S.d + off[i][2]) + (size_t)s * n_rows[i]
                           : t->act_gen[l & 1] + (size_t)s * slice[i];
                J.N = L.N; J.K = L.K; J.K1 = l == 0 ? t->O : L.K; J.n = n_rows[i];
                J.wg0 = blocks[l];
                J.tiles_n = (L.N + AG_CT - 1) / AG_CT;
                J.relu = last ? 0 : 1;
                J.vec = (L.K % 4 == 0 && L.offW % 4 == 0) ? 1 : 0;
                blocks[l] += ((n_rows[i] + RB - 1) / RB) * J.tiles_n;
                x = x2 = J.Y;
            }
            s += 1;
        }
        memcpy(S.h + off[i][0], obs[i], sizeof(float) * (size_t)n_rows[i] * t->O);
        memcpy(S.h + off[i][1], act[i], sizeof(float) * (size_t)n_rows[i] * t->A);
    }
    for (int l = 0; l < launches; ++l) {
        hipLaunchKernelGGL(k_qval_layer, dim3(blocks[l]), dim3(256), 0, t0->stream,
                           reinterpret_cast<const QvalLayerJob *>(S.d) + (size_t)l * QG_JOBS, njobs[l]);
        SAC_HIP(hipGetLastError());
    }
    if (wait_trainer_stream(t0)) return -1;
    for (int i = 0; i < n_trainers; ++i)
        if (n_rows[i] > 0)
            memcpy(q[i], S.h + off[i][2], sizeof(float) * (size_t)n_rows[i] * __builtin_popcount(nets[i]));
    return 0;
}

int sac_q_values_general(sac_trainer_t *t, int64_t n, const float *obs, const float *act, uint32_t nets, float *q) {
    SAC_REQUIRE(t && obs && act && q, "bad arguments to sac_q_values_general");
    SAC_REQUIRE(n >= 1 && n <= ACT_MAX_ROWS, "sac_q_values_general: %lld rows (1..%d per call)", (long long)n, ACT_MAX_ROWS);
    const int32_t rows = (int32_t)n;
    return sac_q_values_general_many(&t, 1, &rows, &obs, &act, &nets, &q);
}
