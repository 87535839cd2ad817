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
//   GEMM    infer_layer_tile<float, false> (sac_infer.h): fp32 MFMA 16x16x4 over K in ascending chunks of AG_KC.  The
//           reduction is never split across workgroups.
//   hidden  infer_layer_store: bias, then x < 0 ? 0 : x (a NaN stays a NaN)
//   head    at most 32 outputs: one column tile; infer_layer_head: bias, then through LDS --
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
    const int ncol = n0 + 16 * (threadIdx.x >> 6) + (threadIdx.x & 15);
    const LayerTile t = infer_layer_tile<float, false>(Xs, W, bp, X, X, N, K, K, n, vec, row0, ncol);
    if (kind == AG_HIDDEN) infer_layer_store(t, sload(&J->Y), N, n, row0, ncol, true);
    else infer_layer_head(t, HL, J, kind, n, row0);
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
    const InferEntry E = {"sac_policy_act_general_many", true, false, "device acting",
                          "sac_policy_act_device is its device acting entry, sac_policy_act_general serves the general step", "act on"};
    bool stoch[SAC_GROUP_MAX] = {};
    if (int rc = act_admit(E, trainers, n_trainers, n_rows, obs, deterministic, eps, act, stoch)) return rc;
    sac_trainer *t0 = trainers[0];
    size_t off[SAC_GROUP_MAX][3], bytes = infer_align(sizeof(ActLayerJob) * SAC_GROUP_MAX * gen::GMAXL);
    act_carve(bytes, off, trainers, n_trainers, n_rows, stoch);
    int launches = 0;
    for (int i = 0; i < n_trainers; ++i) {
        if (n_rows[i] == 0) continue;
        const GenNet &P = trainers[i]->gen->net[SAC_NET_POLICY];
        if (act_general_reserve(trainers[i], (size_t)n_rows[i] * infer_widest(P))) return -1;
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
            infer_layer_job(J, P, L);
            J.X = x;
            J.eps = reinterpret_cast<const float *>(S.d + off[i][1]);
            J.Y = head ? reinterpret_cast<float *>(S.d + off[i][2]) : t->act_gen[l & 1];
            J.n = n_rows[i]; J.wg0 = blocks[l];
            J.kind = !head ? AG_HIDDEN : (t->algo == 1 ? AG_TD3 : (stoch[i] ? AG_SAC_SAMPLE : AG_SAC_MEAN));
            J.A = t->A;
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
