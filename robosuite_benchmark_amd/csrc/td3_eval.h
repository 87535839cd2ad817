// Evaluating the TD3 objectives on the device: the forward half of the TD3 step on rows the run has not trained on
// (included by sac_trainer.hip behind sac_eval.h, whose row-block frame, host body and y expression it uses).
//
// k_eval_td3 = eval_frame<Td3Objective> (sac_eval.h: the grid, the LDS layout, chain Q and the critics behind the heads)
// computes, for 1..1024 transitions (s, a, r, d, s') with their N(0,1) smoothing draw eps, of each of 1..SAC_GROUP_MAX
// TD3 trainers in ONE launch and from the live weights,
//
//   chain Q   [s | a] -> qf1 -> qf2                                               q1, q2
//   chain P   s -> policy: a_pi = tanh(last_fc) (k_act's TD3 action); [s | a_pi] -> qf1          q_pi (a_pi)
//   chain N   s' -> TARGET policy (a net of its own: P[5], tW / tB): a_target = tanh(last_fc);
//             a_smooth = a_target + clamp_nan(eps sigma, -clip, clip), the step's expression: the sum is NOT clipped to
//             the action range; [s' | a_smooth] -> target_qf1 -> target_qf2       tq1, tq2, y (a_target, a_smooth)
//   y = rs r + ((1 - d) discount) fminf(tq1, tq2), every operation rounded to float32 on its own and none fused:
//       eval_y (sac_eval.h) with alpha = 0 and log_pi = 0, which subtracts a zero and leaves every bit where it was
//
// sigma and clip are the trainer's target_policy_noise / target_policy_noise_clip, handed in through the member table.
// There is no entropy term and no stochastic head: a TD3 policy is TanhMlpPolicy (infer_action with stochastic = false).
//
// So q1, q2, q_pi, tq1, tq2 are bit for bit k_qval's values on the same rows and a_pi bit for bit k_act's; a NaN row stays
// in its row.
//
// SAC trainers are refused (sac_evaluate is their entry) and so are general-step TD3 trainers (td3_eval_general.h serves
// them, or TD3Trainer.evaluate_td3's host path).
//
// The entries are eval_fused_many (sac_eval.h) with Td3Eval, the objective's host description below.
#pragma once

namespace sac {

struct Td3EvalMember : EvalCommon {
    const float *eps;
    float *a_pi, *a_target, *a_smooth;       // (n, A) each, or null
    long long tW[3], tB[3];                  // the layers inside the target policy's P
    float sigma, clip;
};

// the smoothed target action, each operation rounded to float32 on its own (as eval_y: NumPy float32 restates it bit
// for bit); a NaN draw passes both comparisons of clamp_nan and stays a NaN
__device__ __forceinline__ float td3_eval_smooth(float a_target, float eps, float sigma, float clip) {
#pragma clang fp contract(off)
    const float noise = clamp_nan(eps * sigma, -clip, clip);
    return a_target + noise;
}

enum { T3E_Q1, T3E_Q2, T3E_Q_PI, T3E_TQ1, T3E_TQ2, T3E_Y, T3E_ROWS_N };

struct Td3Objective {
    typedef Td3EvalMember Member;
    // chain N reads the target policy; chain P runs qf1 alone (the policy loss is -mean Q1(s, pi(s)))
    static __device__ __forceinline__ EvalPolicy policy(const Member *M, bool next) {
        return {sload(&M->P[next ? 5 : 0]), next ? M->tW : M->pW, next ? M->tB : M->pB};
    }
    static __device__ __forceinline__ int critics(bool next) { return next ? 2 : 1; }
    // TanhMlpPolicy: the action as k_act's (infer_action, no noise under the tanh); the target's is smoothed behind it
    static __device__ __forceinline__ float head(const Member *M, const float *HL, int r, int a, int A, int grow, int n,
                                                 bool next, float &) {
        float actv = 0.f;
        if (a < A) {
            const size_t o = (size_t)grow * A + a;
            const float det = infer_action(HL, r, a, A, false, [] { return 0.f; });
            actv = det;
            if (next) {
                const float e = grow < n ? sload(&M->eps)[o] : 0.f;
                actv = td3_eval_smooth(det, e, sload(&M->sigma), sload(&M->clip));
            }
            if (grow < n) {
                float *pd = next ? sload(&M->a_target) : sload(&M->a_pi);
                if (pd) pd[o] = det;
                if (next) {
                    float *ps = sload(&M->a_smooth);
                    if (ps) ps[o] = actv;
                }
            }
        }
        return actv;
    }
    static __device__ __forceinline__ void rows(const Member *M, float *rows, int n, int grow, bool next, const float *QL,
                                                int r, float) {
        const float qa = QL[r];
        if (!next) {
            rows[(size_t)T3E_Q_PI * n + grow] = qa;
        } else {
            const float qb = QL[RB + r];
            const float rew = sload(&M->rew)[grow], d = sload(&M->term)[grow];
            rows[(size_t)T3E_TQ1 * n + grow] = qa;
            rows[(size_t)T3E_TQ2 * n + grow] = qb;
            rows[(size_t)T3E_Y * n + grow] = eval_y(sload(&M->rs), rew, d, sload(&M->discount), qa, qb, 0.f, 0.f);
        }
    }
};

__global__ __launch_bounds__(256) void k_eval_td3(const Td3EvalMember *__restrict__ tab, int n_members) {
    eval_frame<Td3Objective>(tab, n_members);
}

}  // namespace sac

static_assert((int)T3E_ROWS_N == (int)TD3_EVAL_ROWS_N && (int)T3E_Y == (int)TD3_EVAL_Y && (int)T3E_Q_PI == (int)TD3_EVAL_Q_PI &&
              T3E_Q1 == 0 && T3E_Q2 == 1, "k_eval_td3's rows are sac_hip.h's, chain Q's the first two");

namespace {

// the TD3 objective's host description (sac_eval.h says what one names)
struct Td3Eval {
    typedef td3_eval_io_t IO;
    typedef td3_eval_stats_t Stats;
    typedef sac::Td3EvalMember Member;
    typedef sac::Td3MomentsMember Moments;
    static constexpr auto kernel = sac::k_eval_td3;
    static constexpr auto moments_kernel = sac::k_eval_moments_td3;
    static constexpr bool TD3 = true;
    static constexpr int NETS = 6, DRAWS = 1, ARRAYS = 3, ROWS_N = TD3_EVAL_ROWS_N, MOMENTS_N = TD3_EVAL_MOMENTS_N;
    enum { P_EPS = EVAL_P_DRAW, P_ROWS, P_A_PI, P_A_TARGET, P_A_SMOOTH, NPART };
    static constexpr const float *IO::*draws[DRAWS] = {&IO::eps};
    static constexpr EvalArray<IO> arrays[ARRAYS] = {{&IO::a_pi, true, true}, {&IO::a_target, false, false},
                                                     {&IO::a_smooth, true, false}};
    struct Call {                            // (nothing is read per call, nothing handed back)
        int prepare(sac_trainer_t *const *, int, const int32_t *, bool) { return 0; }
        void finish(int, IO &, Stats *) const {}
    };
    template <class Dev> static void member(Member &M, const sac_trainer *t, const Call &, int, Dev dev) {
        M.eps = dev(P_EPS);
        M.a_pi = dev(P_A_PI); M.a_target = dev(P_A_TARGET); M.a_smooth = dev(P_A_SMOOTH);
        eval_layers(M.tW, M.tB, t->net[SAC_NET_TARGET_POLICY]);
        M.sigma = t->dev.td3_sigma; M.clip = t->dev.td3_clip;
    }
    template <class Dev> static void moments(Moments &M, Dev dev) { M.rows = dev(P_ROWS); M.a_pi = dev(P_A_PI); }
    struct General;
};

}  // namespace

// (declared extern "C" in include/sac_hip.h)
int td3_evaluate_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, td3_eval_io_t *io) {
    SAC_REQUIRE(trainers && n_rows && io, "bad arguments to td3_evaluate_many");
    const InferEntry IE = eval_entry<Td3Eval>("td3_evaluate_many", false,
                                             "sac_get_params and a forward on the host is the path");
    return eval_fused_many<Td3Eval>(IE, trainers, n_trainers, n_rows, io, nullptr);
}

int td3_evaluate_stats_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, td3_eval_io_t *io,
                            td3_eval_stats_t *stats) {
    SAC_REQUIRE(trainers && n_rows && io && stats, "bad arguments to td3_evaluate_stats_many");
    const InferEntry IE = eval_entry<Td3Eval>("td3_evaluate_stats_many", false,
                                             "td3_evaluate_general_stats_many is the entry");
    return eval_fused_many<Td3Eval>(IE, trainers, n_trainers, n_rows, io, stats);
}

int td3_evaluate_replay_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, const sac_eval_src_t *src,
                             td3_eval_io_t *io, td3_eval_stats_t *stats) {
    SAC_REQUIRE(trainers && n_rows && src && io, "bad arguments to td3_evaluate_replay_many");
    const InferEntry IE = eval_entry<Td3Eval>("td3_evaluate_replay_many", false,
                                             "td3_evaluate_replay_general_many is the entry");
    return eval_fused_many<Td3Eval>(IE, trainers, n_trainers, n_rows, io, stats, src);
}

int td3_evaluate(sac_trainer_t *t, int64_t n, td3_eval_io_t *io) {
    SAC_REQUIRE(t && io, "bad arguments to td3_evaluate");
    if (int rc = infer_admit_solo("td3_evaluate", n)) return rc;
    const int32_t rows = (int32_t)n;
    return td3_evaluate_many(&t, 1, &rows, io);
}
