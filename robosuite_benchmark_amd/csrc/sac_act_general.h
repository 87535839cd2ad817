// Acting on the device for general-step trainers: policies of any depth and width (included by sac_trainer.hip).
//
// k_act_layer computes ONE layer of the policy's forward pass -- Y = act(X W^T + b) -- for up to SAC_GROUP_MAX members in
// one launch; a call is one launch per layer depth, max(layers) launches on the first member's stream and one wait at the
// end.  It reads the general step's live policy weights where they are (sac_general::net[SAC_NET_POLICY].P: nn.Linear
// layout W [N][K] then b, every matrix on a 16-byte boundary, SAC's two heads merged into one layer of 2A rows): nothing
// is repacked, mirrored or copied.
//
//   table   a launch carries up to SAC_GROUP_MAX jobs (LayerJob, device-visible memory, read with scalar loads): a job
//           is one member's layer l.  Launch l holds layer l of every member that has one; a member's head is its last
//           layer, whatever the launch index.  LayerSchedule (sac_infer.h) writes the tables: one chain per member.
//   kernel  infer_layer_find, then infer_layer_frame<float, false, LayerHead<false>> (sac_infer.h):
//   grid    one workgroup (4 waves) per 16-row x 64-column output tile of one job; wave w owns columns 16 w .. 16 w + 15
//   GEMM    infer_layer_tile<float, false>: fp32 MFMA 16x16x4 over K in ascending chunks of AG_KC.  The reduction is
//           never split across workgroups.
//   hidden  LAYER_STORE, infer_layer_store: bias, then x < 0 ? 0 : x (a NaN stays a NaN)
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
// launch: the layers are separate launches.  Observations, eps, actions and the job tables live in the first member's
// mapped pinned staging (InferStage, sac_infer.h).
#pragma once

namespace sac {

// the job: infer_layer_find.  The table once was searched with a scan; the bisection finds the same job by construction,
// because wg0 ascends along a launch's table (LayerSchedule)
__global__ __launch_bounds__(256) void k_act_layer(const LayerJob *__restrict__ tab, int n_jobs) {
    const LayerJob *J = infer_layer_find(tab, n_jobs);
    infer_layer_frame<float, false, LayerHead<false>>(J, sload(&J->wg0), sload(&J->n), sload(&J->kind));
}

}  // namespace sac

// (declared extern "C" in include/sac_hip.h)
int sac_policy_act_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, const float *const *obs,
                                const int32_t *deterministic, const float *const *eps, float *const *act) {
    SAC_REQUIRE(trainers && n_rows && obs && deterministic && act, "bad arguments to sac_policy_act_general_many");
    const InferEntry E = {"sac_policy_act_general_many", true, false, "device acting",
                          "sac_policy_act_device is its device acting entry, sac_policy_act_general serves the general step", "act on"};
    bool stoch[SAC_GROUP_MAX] = {};
    if (int rc = act_admit(E, trainers, n_trainers, n_rows, obs, deterministic, eps, act, stoch)) return rc;
    sac_trainer *t0 = trainers[0];
    // the staging: the job tables, then per member obs (n, O), eps (n, A) where stochastic, act (n, A)
    enum { P_OBS, P_EPS, P_ACT, NPART };
    LayerSchedule LS(SAC_GROUP_MAX);
    InferStage ST(LS.bytes());
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        const size_t n = (size_t)n_rows[i];
        const size_t part[NPART] = {n * t->O, stoch[i] ? n * t->A : 0, n * t->A};
        ST.carve(i, part, NPART);
        if (n && infer_scratch_reserve(trainers[i], n_rows[i], infer_widest(t->gen->net[SAC_NET_POLICY]), 1)) return -1;
    }
    if (ST.reserve(t0)) return -1;
    LS.bind(ST.S->h, ST.S->d);
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        const GenNet &P = t->gen->net[SAC_NET_POLICY];
        const float *x = ST.in(i, P_OBS, obs[i]), *e = ST.in(i, P_EPS, stoch[i] ? eps[i] : nullptr);
        LS.chain({P, x, x, P.L[0].K, n_rows[i], t->act_gen, 0, ST.dev(i, P_ACT)}, [&](sac::LayerJob &J, int l) {
            if (l + 1 < P.nl) return;
            J.kind = t->algo == 1 ? LAYER_TD3 : (stoch[i] ? LAYER_SAC_SAMPLE : LAYER_SAC_MEAN);
            J.eps = e; J.A = t->A;
        });
    }
    if (LS.launch_all(k_act_layer, t0) || wait_trainer_stream(t0)) return -1;
    for (int i = 0; i < n_trainers; ++i)
        if (n_rows[i] > 0) ST.back(i, {{act[i], P_ACT}});
    return 0;
}

int sac_policy_act_general(sac_trainer_t *t, int64_t n, const float *obs, int deterministic, const float *eps, float *act) {
    SAC_REQUIRE(t && obs && act, "bad arguments to sac_policy_act_general");
    if (int rc = infer_admit_solo("sac_policy_act_general", n)) return rc;
    const int32_t rows = (int32_t)n, det = deterministic;
    return sac_policy_act_general_many(&t, 1, &rows, &obs, &det, &eps, &act);
}
