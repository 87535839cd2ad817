// Evaluating the SAC objectives on the device for general-step trainers: nets of any depth and width (included by
// sac_trainer.hip behind sac_eval.h, sac_act_general.h and sac_qval_general.h).
//
// What k_eval (sac_eval.h) computes in one launch for the fused kernels' shapes -- the thirteen arrays of sac_eval_io_t
// for 1..1024 transitions (s, a, r, d, s') with their draws eps / eps_next, of each of 1..SAC_GROUP_MAX SAC trainers, from
// the live weights -- is computed here layer by layer: k_act_layer's and k_qval_layer's scheme, one table-driven launch
// per layer depth on the first member's stream and ONE wait at the end.  The nets are read where the general step keeps
// them (sac_general::net[...].P: nn.Linear layout W [N][K] then b): nothing is repacked, mirrored or copied.
//
//   schedule  with LP = the deepest policy of the call (hidden layers + head) and LQ = the deepest critic:
//               launches 0 .. LP-1        k_eval_layer<false>: policy layer l of every member that has one, TWO jobs per
//                                         member -- the rows s with eps and the rows s' with eps_next (rows are
//                                         independent: two jobs are the stacked 2n rows).  A member's head is its last
//                                         layer, whatever the launch index.
//               launches LP .. LP+LQ-1    k_eval_layer<true>: critic layer l of every member that has one, SIX jobs per
//                                         member -- [s | a] and [s | a_new] through qf1 and qf2, [s' | a_next] through
//                                         target_qf1 and target_qf2.  Chain Q needs no policy, but it waits for the
//                                         critic phase: one rule for all six jobs, and no launch more.
//               launch LP+LQ              k_eval_y: y, elementwise, from the columns the launches in front of it wrote
//   table     a launch carries up to EG_JOBS = 6 SAC_GROUP_MAX jobs (LayerJob, device-visible memory, read with scalar
//             loads).  LayerSchedule (sac_infer.h) writes the tables: per member two policy chains from launch 0 and six
//             critic chains from launch LP, k_act_layer's and k_qval_layer's chains.
//   kernel    infer_layer_find, then infer_layer_frame<float, SPLIT, Head>: LayerHead<true> for the policy launches,
//             LayerStore (no head, no HL) for the critics'
//   grid      one workgroup (4 waves) per 16-row x 64-column output tile of one job
//   policy    infer_layer_tile<float, false> and infer_layer_store: k_act_layer's hidden layers
//   head      N = 2A <= 32, one column tile, through HL: infer_layer_head_eval (sac_infer.h) -- the action is
//             infer_action's with the draws (k_act_layer's stochastic action, bit for bit), log_pi is k_eval's expression
//             summed by group16_sum, and for the rows s the mean and the clamped log_std (a NaN stays a NaN).  a_new and
//             a_next ALWAYS go to the staging, where the critic launches read them, whether or not the caller asked for
//             them.
//   critics   infer_layer_tile<float, true> and infer_layer_store: k_qval_layer's layers.  The first layer reads its two
//             blocks through the split point K1 = O; the output unit (N = 1) is summed like any other column and lands in
//             its row of `rows`: the six Q columns are bit for bit sac_q_values_general's on the same rows.
//   y         eval_y (sac_eval.h) unchanged: every operation rounded to float32 on its own, none fused
//
// Workgroups never talk to each other: no hand-offs, no spinning, no atomics; the order between layers is the order of
// the launches on one stream.  Row independence as in k_act_layer / k_qval_layer: an output element is one MFMA chain
// over k in an order fixed by K alone, rows beyond a job's n repeat row n - 1 on the way in and are never written.
//
// The kernels write the caller's outputs in the staging (InferStage) and the members' activation scratch: nothing
// the step reads.  The scratch is the trainer's act_gen pair (act_general_reserve), shared with sac_policy_act_general
// and sac_q_values_general -- each of those calls, and this one, ends with a wait on the stream, so they never overlap.
// Each buffer holds max(2 n x the widest policy layer, 6 n x the widest critic layer) floats; the worst case is
// 6 jobs x 1024 rows x 4096 units x 4 bytes x 2 buffers = 192 MB per trainer.  Vector stores only.
#pragma once

namespace sac {

constexpr int EG_JOBS = 6 * SAC_GROUP_MAX;      // jobs of one launch
constexpr int EG_LAUNCHES = 2 * gen::GMAXL;     // layer launches of one call, at most
constexpr int EG_YROWS = 256;                   // rows of one k_eval_y workgroup
struct EvalYMember {
    const float *rew, *term;       // [n]
    float *rows;                   // (SAC_EVAL_ROWS_N, n)
    int n, wg0;
    float alpha, rs, discount;
    int pad;
};

// SPLIT false: a policy launch (hidden layers and heads); true: a critic launch
template <bool SPLIT>
__global__ __launch_bounds__(256) void k_eval_layer(const LayerJob *__restrict__ tab, int n_jobs) {
    const LayerJob *J = infer_layer_find(tab, n_jobs);
    typedef typename std::conditional<SPLIT, LayerStore, LayerHead<true>>::type Head;
    infer_layer_frame<float, SPLIT, Head>(J, sload(&J->wg0), sload(&J->n), SPLIT ? (int)LAYER_STORE : sload(&J->kind));
}

__global__ __launch_bounds__(EG_YROWS) void k_eval_y(const EvalYMember *__restrict__ tab, int n_members) {
    typedef __attribute__((address_space(1))) float *gout;
    const EvalYMember *M = tab + infer_member(tab, n_members, &EvalYMember::wg0);
    const int n = sload(&M->n);
    const int row = ((int)blockIdx.x - sload(&M->wg0)) * EG_YROWS + (int)threadIdx.x;
    if (row >= n) return;
    float *rows = sload(&M->rows);
    const float tq1 = ld1g(rows + ((unsigned)EVAL_TQ1 * (unsigned)n + (unsigned)row));
    const float tq2 = ld1g(rows + ((unsigned)EVAL_TQ2 * (unsigned)n + (unsigned)row));
    const float lpn = ld1g(rows + ((unsigned)EVAL_LOG_PI_NEXT * (unsigned)n + (unsigned)row));
    const float rew = ld1g(sload(&M->rew) + row), d = ld1g(sload(&M->term) + row);
    *(gout)(uintptr_t)(rows + ((unsigned)EVAL_Y * (unsigned)n + (unsigned)row)) =
        eval_y(sload(&M->rs), rew, d, sload(&M->discount), tq1, tq2, sload(&M->alpha), lpn);
}

}  // namespace sac

// sac_evaluate_general_many (stats null) and sac_evaluate_general_stats_many: with stats, mu and log_std always have
// their place in the staging, k_eval_moments (sac_eval_moments.h) runs behind k_eval_y in front of the wait, and a null
// io[i].rows is taken -- as evaluate_many (sac_eval.h) does for the fused shapes.  sac_evaluate_replay_general_many (src
// not null): k_eval_rows (sac_eval_rows.h) fills the five input parts from src[i]'s replay storage in front of the first
// layer launch, as there
static int evaluate_general_many(const InferEntry &IE, sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
                                 sac_eval_io_t *io, sac_eval_stats_t *stats, const sac_eval_src_t *src = nullptr) {
    if (int rc = infer_admit(IE, trainers, n_trainers, n_rows, [&](int i) {
            return src ? eval_rows_admit(io[i], src[i], trainers[i], i, n_rows[i], !stats) : eval_admit_io(io[i], i, !stats);
        })) return rc;
    sac_trainer *t0 = trainers[0];
    float alpha[SAC_GROUP_MAX], log_alpha[SAC_GROUP_MAX];
    if (eval_read_alpha(trainers, n_trainers, n_rows, alpha, stats ? log_alpha : nullptr)) return -1;

    // the staging: the layer tables, k_eval_y's table, then per member
    //   obs act rew term nobs eps eps_next | rows a_new a_next (always: the critic launches read them) mu log_std
    enum { P_OBS, P_ACT, P_REW, P_TERM, P_NOBS, P_EPS, P_EPS_NEXT, P_ROWS, P_A_NEW, P_A_NEXT, P_MU, P_LOG_STD, NPART };
    LayerSchedule LS(EG_JOBS);
    static_assert(EG_LAUNCHES <= LayerSchedule::MAX_LAUNCHES, "the schedule counts every launch of an evaluation");
    const size_t tab_bytes = LS.bytes(EG_LAUNCHES);
    InferStage ST(tab_bytes + infer_align(sizeof(EvalYMember) * SAC_GROUP_MAX));
    int LP = 0, LQ = 0;
    size_t slice_p[SAC_GROUP_MAX] = {}, slice_q[SAC_GROUP_MAX] = {};
    for (int i = 0; i < n_trainers; ++i) {
        sac_trainer *t = trainers[i];
        const size_t n = (size_t)n_rows[i], nO = n * t->O, nA = n * t->A;
        const sac_eval_io_t &E = io[i];
        const size_t part[NPART] = {nO, nA, n, n, nO, nA, nA, n * SAC_EVAL_ROWS_N, nA, nA,
                                    n && (E.mu || stats) ? nA : 0, n && (E.log_std || stats) ? nA : 0};
        ST.carve(i, part, NPART);
        if (n == 0) continue;
        const GenNet &P = t->gen->net[SAC_NET_POLICY], &Q = t->gen->net[SAC_NET_QF1];      // (the four Q nets share their layout)
        // (one reservation for the larger of the two phases, not infer_scratch_reserve twice: that would free and
        // allocate again where the second phase is the larger)
        slice_p[i] = n * infer_widest(P); slice_q[i] = n * infer_widest(Q);
        if (act_general_reserve(t, std::max(2 * slice_p[i], 6 * slice_q[i]))) return -1;
        LP = std::max(LP, P.nl); LQ = std::max(LQ, Q.nl);
    }
    MomentsStage MS;
    if (stats) moments_carve(ST.bytes, MS, n_trainers);
    EvalRowsStage RS;
    if (src) eval_rows_carve(ST.bytes, RS, n_trainers, n_rows);
    if (ST.reserve(t0)) return -1;
    const sac_trainer::ActStage &S = t0->act_stage;
    LS.bind(S.h, S.d);
    EvalYMember *ytab = reinterpret_cast<EvalYMember *>(S.h + tab_bytes);
    int yblocks = 0, m = 0, row_wgs = 0;
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        const sac_eval_io_t &E = io[i];
        const int n = n_rows[i];
        auto dev = [&](int k) { return ST.dev(i, k); };
        auto in = [&](int k, const float *from) { ST.in(i, k, from); };
        if (src) {
            row_wgs += eval_rows_member(S, RS, m, i, row_wgs, src[i], n, dev(P_OBS), dev(P_ACT), dev(P_REW), dev(P_TERM), dev(P_NOBS));
        } else {
            in(P_OBS, E.obs); in(P_ACT, E.act); in(P_REW, E.rew); in(P_TERM, E.term); in(P_NOBS, E.next_obs);
        }
        in(P_EPS, E.eps); in(P_EPS_NEXT, E.eps_next);
        float *rows = dev(P_ROWS);
        // the policy on s (with eps) and on s' (with eps_next), launches 0 .. : its head writes the action and log_pi
        const GenNet &P = t->gen->net[SAC_NET_POLICY];
        for (int s = 0; s < 2; ++s) {
            const float *x = dev(s ? P_NOBS : P_OBS);
            LS.chain({P, x, x, P.L[0].K, n, t->act_gen, s * slice_p[i], dev(s ? P_A_NEXT : P_A_NEW)},
                     [&](sac::LayerJob &J, int l) {
                if (l + 1 < P.nl) return;
                J.kind = LAYER_EVAL; J.A = t->A;
                J.eps = dev(s ? P_EPS_NEXT : P_EPS);
                J.lp = rows + (size_t)(s ? EVAL_LOG_PI_NEXT : EVAL_LOG_PI) * n;
                J.mu = !s && (E.mu || stats) ? dev(P_MU) : nullptr;
                J.ls = !s && (E.log_std || stats) ? dev(P_LOG_STD) : nullptr;
            });
        }
        // the critics, launches LP .. : chain s writes row s of `rows` (EVAL_Q1 .. EVAL_TQ2)
        const int net_of[6] = {SAC_NET_QF1, SAC_NET_QF2, SAC_NET_QF1, SAC_NET_QF2, SAC_NET_TARGET_QF1, SAC_NET_TARGET_QF2};
        const int obs_of[6] = {P_OBS, P_OBS, P_OBS, P_OBS, P_NOBS, P_NOBS};
        const int act_of[6] = {P_ACT, P_ACT, P_A_NEW, P_A_NEW, P_A_NEXT, P_A_NEXT};
        for (int s = 0; s < 6; ++s)
            LS.chain({t->gen->net[net_of[s]], dev(obs_of[s]), dev(act_of[s]), t->O, n, t->act_gen, s * slice_q[i],
                      rows + (size_t)s * n, true, LP});
        if (stats) moments_member(S, MS, m, i, rows, dev(P_MU), dev(P_LOG_STD), n, t->A);
        EvalYMember &M = ytab[m++];
        M.rew = dev(P_REW); M.term = dev(P_TERM); M.rows = rows;
        M.n = n; M.wg0 = yblocks;
        M.alpha = alpha[i]; M.rs = t->cfg.reward_scale; M.discount = t->cfg.discount; M.pad = 0;
        yblocks += (n + EG_YROWS - 1) / EG_YROWS;
    }
    if (src && eval_rows_launch(t0, RS, m, row_wgs, src, n_trainers, n_rows)) return -1;
    for (int l = 0; l < LP + LQ; ++l)
        if (LS.launch(l < LP ? k_eval_layer<false> : k_eval_layer<true>, t0, l)) return -1;
    hipLaunchKernelGGL(k_eval_y, dim3(yblocks), dim3(EG_YROWS), 0, t0->stream,
                       reinterpret_cast<const EvalYMember *>(S.d + tab_bytes), m);
    SAC_HIP(hipGetLastError());
    if (stats && moments_launch(t0, MS, m)) return -1;
    if (wait_trainer_stream(t0)) return -1;
    for (int i = 0; i < n_trainers; ++i) {
        if (n_rows[i] == 0) continue;
        sac_eval_io_t &E = io[i];
        ST.back(i, {{E.rows, P_ROWS}, {E.a_new, P_A_NEW}, {E.a_next, P_A_NEXT}, {E.mu, P_MU}, {E.log_std, P_LOG_STD}});
        E.alpha = alpha[i];
        if (stats) moments_read(S, MS, i, alpha[i], log_alpha[i], &stats[i]);
    }
    return 0;
}

// (declared extern "C" in include/sac_hip.h)
int sac_evaluate_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, sac_eval_io_t *io) {
    SAC_REQUIRE(trainers && n_rows && io, "bad arguments to sac_evaluate_general_many");
    const InferEntry IE = {"sac_evaluate_general_many", true, true, "device evaluation",
                           "sac_evaluate is its device evaluation entry, sac_evaluate_general serves the general step", "evaluate"};
    return evaluate_general_many(IE, trainers, n_trainers, n_rows, io, nullptr);
}

int sac_evaluate_general_stats_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, sac_eval_io_t *io,
                                    sac_eval_stats_t *stats) {
    SAC_REQUIRE(trainers && n_rows && io && stats, "bad arguments to sac_evaluate_general_stats_many");
    const InferEntry IE = {"sac_evaluate_general_stats_many", true, true, "device evaluation",
                           "sac_evaluate_stats_many is its entry, sac_evaluate_general_stats_many serves the general step", "evaluate"};
    return evaluate_general_many(IE, trainers, n_trainers, n_rows, io, stats);
}

int sac_evaluate_replay_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
                                     const sac_eval_src_t *src, sac_eval_io_t *io, sac_eval_stats_t *stats) {
    SAC_REQUIRE(trainers && n_rows && src && io, "bad arguments to sac_evaluate_replay_general_many");
    const InferEntry IE = {"sac_evaluate_replay_general_many", true, true, "device evaluation",
                           "sac_evaluate_replay_many is its entry, sac_evaluate_replay_general_many serves the general step", "evaluate"};
    return evaluate_general_many(IE, trainers, n_trainers, n_rows, io, stats, src);
}

int sac_evaluate_general(sac_trainer_t *t, int64_t n, sac_eval_io_t *io) {
    SAC_REQUIRE(t && io, "bad arguments to sac_evaluate_general");
    if (int rc = infer_admit_solo("sac_evaluate_general", n)) return rc;
    const int32_t rows = (int32_t)n;
    return sac_evaluate_general_many(&t, 1, &rows, io);
}
