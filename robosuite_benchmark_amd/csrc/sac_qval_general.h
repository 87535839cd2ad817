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
//   GEMM    infer_layer_tile<float, true> (sac_infer.h): k_act_layer's tile with two input sources.  The reduction is
//           never split across workgroups.
//   input   the split point K1: the first layer reads cat(obs, act) through it (X = obs, X2 = act, K1 = O: the host
//           stages the two blocks and never builds the concatenated rows; all selected nets of a member read the same
//           two blocks); hidden layers set K1 = K and X2 = X.
//   hidden  infer_layer_store: bias, then x < 0 ? 0 : x (a NaN stays a NaN)
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
    const int ncol = n0 + 16 * (threadIdx.x >> 6) + (threadIdx.x & 15);
    const LayerTile t = infer_layer_tile<float, true>(Xs, W, bp, X, X2, N, K, K1, n, vec, row0, ncol);
    // hidden layer: ReLU; output layer (N == 1, relu == 0): column 0 alone passes ncol < N and lands in q[s n + row]
    infer_layer_store(t, sload(&J->Y), N, n, row0, ncol, relu);
}

}  // namespace sac

// (declared extern "C" in include/sac_hip.h)
int sac_q_values_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, const float *const *obs,
                              const float *const *act, const uint32_t *nets, float *const *q) {
    SAC_REQUIRE(trainers && n_rows && obs && act && nets && q, "bad arguments to sac_q_values_general_many");
    const InferEntry E = {"sac_q_values_general_many", true, false, "device Q evaluation",
                          "sac_q_values is its device Q evaluation entry, sac_q_values_general serves the general step", "evaluate"};
    if (int rc = qval_admit(E, trainers, n_trainers, n_rows, obs, act, nets, q)) return rc;
    sac_trainer *t0 = trainers[0];
    size_t off[SAC_GROUP_MAX][3], slice[SAC_GROUP_MAX] = {}, bytes = infer_align(sizeof(QvalLayerJob) * QG_JOBS * gen::GMAXL);
    qval_carve(bytes, off, trainers, n_trainers, n_rows, nets);
    int launches = 0;
    for (int i = 0; i < n_trainers; ++i) {
        if (n_rows[i] == 0) continue;
        const GenNet &Q = trainers[i]->gen->net[SAC_NET_QF1];          // (the four Q nets share their layout)
        slice[i] = (size_t)n_rows[i] * infer_widest(Q);
        if (act_general_reserve(trainers[i], slice[i] * __builtin_popcount(nets[i]))) return -1;
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
                infer_layer_job(J, Q, L);
                J.X = x; J.X2 = x2;
                J.Y = last ? reinterpret_cast<float *>(S.d + off[i][2]) + (size_t)s * n_rows[i]
                           : t->act_gen[l & 1] + (size_t)s * slice[i];
                J.K1 = l == 0 ? t->O : L.K; J.n = n_rows[i];
                J.wg0 = blocks[l];
                J.relu = last ? 0 : 1;
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
