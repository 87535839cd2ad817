// Evaluating the TD3 objectives on the device for general-step trainers: the TD3 half of the general-step body (included
// by sac_trainer.hip behind sac_eval_general.h and td3_eval.h).
//
// eval_general_many (sac_eval_general.h: the schedule, the tables, the scratch, the single wait) runs here with
// Td3Eval::General.  What differs from the SAC objective:
//
//   policy launches   k_eval_layer_td3 = infer_layer_frame<float, false, LayerHeadTd3>: the policy on the rows s and the
//                     TARGET policy (a net of its own, SAC_NET_TARGET_POLICY) on the rows s'
//   heads             N = A <= 16, one column tile, through HL: the deterministic action is infer_action's with
//                     stochastic = false (k_act_layer's LAYER_TD3 action, bit for bit).  LAYER_TD3: a_pi into J->Y.
//                     LAYER_TD3_EVAL, the target chain: a_target into J->mu where the caller asked for it, and a_smooth =
//                     td3_eval_smooth(a_target, eps, sigma, clip) (td3_eval.h, as it stands) into J->Y; sigma and clip ride
//                     in the job's two pad words.  a_pi and a_smooth ALWAYS go to the staging, where the critic launches
//                     read them.  eps is loaded for live rows only.
//   critic launches   k_eval_layer<true> unchanged, FIVE jobs per member in the order of TD3_EVAL_Q1 .. TQ2: [s | a] through
//                     qf1 and qf2, [s | a_pi] through qf1, [s' | a_smooth] through target_qf1 and target_qf2 -- bit for bit
//                     sac_q_values_general's columns on the same rows
//   y                 k_eval_y_td3: eval_y (sac_eval.h) with alpha = 0 and log_pi = 0, as k_eval_td3 calls it
//
// As there: no atomics, vector stores only.  SAC trainers are refused (sac_evaluate_general is their entry) and so are TD3 trainers
// with the fused kernels' shapes (td3_evaluate is theirs).
#pragma once

namespace sac {

constexpr int LAYER_TD3_EVAL = 5;          // the TARGET policy's head of an evaluation: a_target, then the smoothed action
static_assert(LAYER_TD3_EVAL > LAYER_EVAL, "a job kind of its own");

struct EvalYTd3Member {
    const float *rew, *term;       // [n]
    float *rows;                   // (TD3_EVAL_ROWS_N, n)
    int n, wg0;
    float rs, discount;
};

// the TD3 heads of an evaluation (one column tile, kind is uniform over the workgroup): pre-activations through HL, then
// one thread per action
__device__ __forceinline__ void infer_layer_head_td3(const LayerTile &t, float *HL, const LayerJob *J, int kind, int n, int row0) {
    typedef __attribute__((address_space(1))) float *gout;
    infer_layer_head_lds(t, HL);
    const int tid = threadIdx.x;
    const int A = sload(&J->A);
    const int r = tid >> 4, a = tid & 15;
    if (a < A && row0 + r < n) {
        const unsigned o = (unsigned)(row0 + r) * (unsigned)A + (unsigned)a;
        const float det = infer_action(HL, r, a, A, false, [] { return 0.f; });
        float out = det;
        if (kind == LAYER_TD3_EVAL) {
            float *pt = sload(&J->mu);
            if (pt) *(gout)(uintptr_t)(pt + o) = det;
            out = td3_eval_smooth(det, ld1g(sload(&J->eps) + o), __int_as_float(sload(&J->pad[0])),
                                  __int_as_float(sload(&J->pad[1])));
        }
        *(gout)(uintptr_t)(sload(&J->Y) + o) = out;
    }
}

struct LayerHeadTd3 {              // a TD3 evaluation's policy launches: hidden layers and the two heads
    static __device__ __forceinline__ void finish(const LayerTile &t, const LayerJob *J, int kind, int N, int n, int row0, int ncol) {
        __shared__ float HL[RB * ACT_HEAD_LD];
        if (kind == LAYER_STORE) infer_layer_store(t, sload(&J->Y), N, n, row0, ncol, true);
        else infer_layer_head_td3(t, HL, J, kind, n, row0);
    }
};

__global__ __launch_bounds__(256) void k_eval_layer_td3(const LayerJob *__restrict__ tab, int n_jobs) {
    const LayerJob *J = infer_layer_find(tab, n_jobs);
    infer_layer_frame<float, false, LayerHeadTd3>(J, sload(&J->wg0), sload(&J->n), sload(&J->kind));
}

__global__ __launch_bounds__(EG_YROWS) void k_eval_y_td3(const EvalYTd3Member *__restrict__ tab, int n_members) {
    typedef __attribute__((address_space(1))) float *gout;
    const EvalYTd3Member *M = tab + infer_member(tab, n_members, &EvalYTd3Member::wg0);
    const int n = sload(&M->n);
    const int row = ((int)blockIdx.x - sload(&M->wg0)) * EG_YROWS + (int)threadIdx.x;
    if (row >= n) return;
    float *rows = sload(&M->rows);
    const float tq1 = ld1g(rows + ((unsigned)T3E_TQ1 * (unsigned)n + (unsigned)row));
    const float tq2 = ld1g(rows + ((unsigned)T3E_TQ2 * (unsigned)n + (unsigned)row));
    const float rew = ld1g(sload(&M->rew) + row), d = ld1g(sload(&M->term) + row);
    *(gout)(uintptr_t)(rows + ((unsigned)T3E_Y * (unsigned)n + (unsigned)row)) =
        eval_y(sload(&M->rs), rew, d, sload(&M->discount), tq1, tq2, 0.f, 0.f);
}

}  // namespace sac

static_assert(T3E_Q_PI == 2 && T3E_TQ1 == 3 && T3E_TQ2 == 4, "the five critic chains write rows TD3_EVAL_Q1 .. TQ2 in order");

namespace {

// the general step's half of the TD3 description (sac_eval_general.h says what one names)
struct Td3Eval::General {
    typedef sac::EvalYTd3Member YMember;
    static constexpr auto y_kernel = sac::k_eval_y_td3;
    static constexpr auto policy_kernel = sac::k_eval_layer_td3;
    static constexpr int policy_net[2] = {SAC_NET_POLICY, SAC_NET_TARGET_POLICY}, action[2] = {P_A_PI, P_A_SMOOTH};
    static constexpr int CRITICS = 5;
    static constexpr EvalCritic critics[CRITICS] = {
        {SAC_NET_QF1, EVAL_P_OBS, EVAL_P_ACT}, {SAC_NET_QF2, EVAL_P_OBS, EVAL_P_ACT}, {SAC_NET_QF1, EVAL_P_OBS, P_A_PI},
        {SAC_NET_TARGET_QF1, EVAL_P_NOBS, P_A_SMOOTH}, {SAC_NET_TARGET_QF2, EVAL_P_NOBS, P_A_SMOOTH}};
    // the policy's head writes a_pi; the target policy's a_target where the caller asked for it, and a_smooth
    template <class Dev> static void head(sac::LayerJob &J, const sac_trainer *t, int s, int, Dev dev) {
        J.kind = s ? LAYER_TD3_EVAL : LAYER_TD3; J.A = t->A;
        if (!s) return;
        J.eps = dev(P_EPS);
        J.mu = dev(P_A_TARGET);
        static_assert(sizeof(J.pad[0]) == sizeof(float), "sigma and clip ride in the pad words");
        memcpy(&J.pad[0], &t->gen->dev.td3_sigma, sizeof(float));       // (the general step's own record:
        memcpy(&J.pad[1], &t->gen->dev.td3_clip, sizeof(float));        // gen_build_td3 fills it, not t->dev)
    }
};

}  // namespace

// (declared extern "C" in include/sac_hip.h)
int td3_evaluate_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, td3_eval_io_t *io) {
    SAC_REQUIRE(trainers && n_rows && io, "bad arguments to td3_evaluate_general_many");
    const InferEntry IE = eval_entry<Td3Eval>(
        "td3_evaluate_general_many", true,
        "td3_evaluate is its device evaluation entry, td3_evaluate_general serves the general step");
    return eval_general_many<Td3Eval>(IE, trainers, n_trainers, n_rows, io, nullptr);
}

int td3_evaluate_general_stats_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, td3_eval_io_t *io,
                                    td3_eval_stats_t *stats) {
    SAC_REQUIRE(trainers && n_rows && io && stats, "bad arguments to td3_evaluate_general_stats_many");
    const InferEntry IE = eval_entry<Td3Eval>(
        "td3_evaluate_general_stats_many", true,
        "td3_evaluate_stats_many is its entry, td3_evaluate_general_stats_many serves the general step");
    return eval_general_many<Td3Eval>(IE, trainers, n_trainers, n_rows, io, stats);
}

int td3_evaluate_replay_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
                                     const sac_eval_src_t *src, td3_eval_io_t *io, td3_eval_stats_t *stats) {
    SAC_REQUIRE(trainers && n_rows && src && io, "bad arguments to td3_evaluate_replay_general_many");
    const InferEntry IE = eval_entry<Td3Eval>(
        "td3_evaluate_replay_general_many", true,
        "td3_evaluate_replay_many is its entry, td3_evaluate_replay_general_many serves the general step");
    return eval_general_many<Td3Eval>(IE, trainers, n_trainers, n_rows, io, stats, src);
}

int td3_evaluate_general(sac_trainer_t *t, int64_t n, td3_eval_io_t *io) {
    SAC_REQUIRE(t && io, "bad arguments to td3_evaluate_general");
    if (int rc = infer_admit_solo("td3_evaluate_general", n)) return rc;
    const int32_t rows = (int32_t)n;
    return td3_evaluate_general_many(&t, 1, &rows, io);
}
