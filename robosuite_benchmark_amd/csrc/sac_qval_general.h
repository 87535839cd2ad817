// Evaluating the critics on the device for general-step trainers: Q networks of any depth and width (included by
// sac_trainer.hip).
//
// k_qval_layer computes ONE layer of the Q networks' forward pass -- Y = f(X W^T + b) -- for up to SAC_GROUP_MAX members
// times up to 4 selected nets in one launch; a call is one launch per layer depth, max(layers) launches on the first
// member's stream and one wait at the end: k_act_layer's scheme (sac_act_general.h).  It reads the general step's live
// critic weights where they are (sac_general::net[SAC_NET_QF1 .. SAC_NET_TARGET_QF2].P: nn.Linear layout W [N][K] then
// b, at Layer::offW / offB): nothing is repacked, mirrored or copied.
//
//   table   a launch carries up to QG_JOBS = 4 SAC_GROUP_MAX jobs (LayerJob, device-visible memory, read with scalar
//           loads): a job is (member, selected net, layer l).  Launch l holds layer l of every (member, net) that has
//           one; a net's output layer is its last layer, whatever the launch index.  LayerSchedule (sac_infer.h) writes
//           the tables: one chain per (member, selected net), each on its own slice of the member's scratch.
//   kernel  infer_layer_find (a bisection over wg0), then infer_layer_frame<float, true, LayerStore> (sac_infer.h): no
//           head, no HL
//   grid    one workgroup (4 waves) per 16-row x 64-column output tile of one job; wave w owns columns 16 w .. 16 w + 15
//   GEMM    infer_layer_tile<float, true>: k_act_layer's tile with two input sources.  The reduction is never split
//           across workgroups.
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
// scratch is the trainer's act_gen pair (infer_scratch_reserve), shared with sac_policy_act_general: each buffer holds
// n_sel slices of n x the widest hidden layer.  Acting and Q calls each end with a wait on the trainer's stream, so they
// never overlap; acting sessions own their scratch.  Worst case 4 nets x 1024 rows x 4096 units x 4 bytes x 2 buffers =
// 128 MB per trainer.  Vector stores only.
#pragma once

namespace sac {

constexpr int QG_JOBS = 4 * SAC_GROUP_MAX;      // jobs of one launch

__global__ __launch_bounds__(256) void k_qval_layer(const LayerJob *__restrict__ tab, int n_jobs) {
    const LayerJob *J = infer_layer_find(tab, n_jobs);
    infer_layer_frame<float, true, LayerStore>(J, sload(&J->wg0), sload(&J->n), LAYER_STORE);
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
    // the staging: the job tables, then per member obs (n, O), act (n, A), q (selected nets, n)
    enum { P_OBS, P_ACT, P_Q, NPART };
    LayerSchedule LS(QG_JOBS);
    InferStage ST(LS.bytes());
    size_t slice[SAC_GROUP_MAX] = {};
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        const size_t n = (size_t)n_rows[i];
        const size_t part[NPART] = {n * t->O, n * t->A, n ? n * __builtin_popcount(nets[i]) : 0};
        ST.carve(i, part, NPART);
        // (the four Q nets share their layout)
        if (n && infer_scratch_reserve(trainers[i], n_rows[i], infer_widest(t->gen->net[SAC_NET_QF1]), __builtin_popcount(nets[i]),
                                       &slice[i])) return -1;
    }
    if (ST.reserve(t0)) return -1;
    LS.bind(ST.S->h, ST.S->d);
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        const float *o = ST.in(i, P_OBS, obs[i]), *a = ST.in(i, P_ACT, act[i]);
        int s = 0;
        for (int k = 0; k < 4; ++k) {
            if (!(nets[i] >> k & 1u)) continue;
            // selected net s: its output unit writes row s of q
            LS.chain({t->gen->net[SAC_NET_QF1 + k], o, a, t->O, n_rows[i], t->act_gen, s * slice[i],
                      ST.dev(i, P_Q) + (size_t)s * n_rows[i]});
            s += 1;
        }
    }
    if (LS.launch_all(k_qval_layer, t0) || wait_trainer_stream(t0)) return -1;
    for (int i = 0; i < n_trainers; ++i)
        if (n_rows[i] > 0) ST.back(i, {{q[i], P_Q}});
    return 0;
}

int sac_q_values_general(sac_trainer_t *t, int64_t n, const float *obs, const float *act, uint32_t nets, float *q) {
    SAC_REQUIRE(t && obs && act && q, "bad arguments to sac_q_values_general");
    if (int rc = infer_admit_solo("sac_q_values_general", n)) return rc;
    const int32_t rows = (int32_t)n;
    return sac_q_values_general_many(&t, 1, &rows, &obs, &act, &nets, &q);
}
