// Evaluating the SAC objectives on the device for general-step trainers: nets of any depth and width (included by
// sac_trainer.hip behind sac_eval.h, sac_act_general.h and sac_qval_general.h).
// Here: the general-step body of both objectives (eval_general_many), described with the SAC objective's kernels, which
// live here; td3_eval_general.h says what differs for TD3.
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

namespace {

// a critic chain of the general body: net `net` on [part obs | part act] of the member's staging; chain s writes row s of `rows`
struct EvalCritic { int net, obs, act; };

// The general step's half of the SAC description.  An objective's General names
//   YMember, y_kernel            the y kernel and its member table
//   policy_kernel                the kernel of the policy launches
//   policy_net, action           the two policy chains (0: on s, 1: on s'): their nets, and the parts their heads write
//   head(J, t, s, n, dev)        the head job of policy chain s
//   critics[CRITICS]             the critic chains, in the order of their rows
struct SacEval::General {
    typedef sac::EvalYMember YMember;
    static constexpr auto y_kernel = sac::k_eval_y;
    static constexpr auto policy_kernel = sac::k_eval_layer<false>;
    static constexpr int policy_net[2] = {SAC_NET_POLICY, SAC_NET_POLICY}, action[2] = {P_A_NEW, P_A_NEXT};
    static constexpr int CRITICS = 6;
    static constexpr EvalCritic critics[CRITICS] = {
        {SAC_NET_QF1, EVAL_P_OBS, EVAL_P_ACT}, {SAC_NET_QF2, EVAL_P_OBS, EVAL_P_ACT},
        {SAC_NET_QF1, EVAL_P_OBS, P_A_NEW}, {SAC_NET_QF2, EVAL_P_OBS, P_A_NEW},
        {SAC_NET_TARGET_QF1, EVAL_P_NOBS, P_A_NEXT}, {SAC_NET_TARGET_QF2, EVAL_P_NOBS, P_A_NEXT}};
    // the head writes the action and log_pi, and for the rows s the mean and the clamped log_std where they have a place
    template <class Dev> static void head(sac::LayerJob &J, const sac_trainer *t, int s, int n, Dev dev) {
        J.kind = LAYER_EVAL; J.A = t->A;
        J.eps = dev(s ? P_EPS_NEXT : P_EPS);
        J.lp = dev(P_ROWS) + (size_t)(s ? EVAL_LOG_PI_NEXT : EVAL_LOG_PI) * n;
        J.mu = s ? nullptr : dev(P_MU);
        J.ls = s ? nullptr : dev(P_LOG_STD);
    }
};

}  // namespace

// The general-step body of an objective: *_evaluate_general_many (stats and src null), *_evaluate_general_stats_many and
// *_evaluate_replay_general_many, as eval_fused_many (sac_eval.h) serves the fixed-shape entries of the same names: with
// stats, the moments kernel runs behind the y kernel in front of the wait and a null io[i].rows is taken; with src,
// k_eval_rows (sac_eval_rows.h) fills the five input parts from src[i]'s replay storage in front of the first layer launch.
// The staging: the layer tables, the y kernel's table, then per member the parts as there -- the actions that the critic
// launches read always have their place.
template <class Obj>
static int eval_general_many(const InferEntry &IE, sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
                             typename Obj::IO *io, typename Obj::Stats *stats, const sac_eval_src_t *src = nullptr) {
    typedef typename Obj::General G;
    static_assert(G::CRITICS * SAC_GROUP_MAX <= EG_JOBS, "a critic launch fits the evaluation's job table");
    if (int rc = infer_admit(IE, trainers, n_trainers, n_rows, [&](int i) {
            return eval_admit_io<Obj>(io[i], src, trainers[i], i, n_rows[i], !stats);
        })) return rc;
    sac_trainer *t0 = trainers[0];
    typename Obj::Call C;
    if (C.prepare(trainers, n_trainers, n_rows, stats != nullptr)) return -1;

    LayerSchedule LS(EG_JOBS);
    static_assert(EG_LAUNCHES <= LayerSchedule::MAX_LAUNCHES, "the schedule counts every launch of an evaluation");
    const size_t tab_bytes = LS.bytes(EG_LAUNCHES);
    InferStage ST(tab_bytes + infer_align(sizeof(typename G::YMember) * SAC_GROUP_MAX));
    int LP = 0, LQ = 0;
    size_t slice_p[SAC_GROUP_MAX] = {}, slice_q[SAC_GROUP_MAX] = {};
    for (int i = 0; i < n_trainers; ++i) {
        sac_trainer *t = trainers[i];
        const size_t n = (size_t)n_rows[i];
        eval_carve<Obj>(ST, i, t, n_rows[i], io[i], stats != nullptr, true);
        if (n == 0) continue;
        // (a policy and its target share their layout, and so do the four Q nets)
        const GenNet &P = t->gen->net[SAC_NET_POLICY], &Q = t->gen->net[SAC_NET_QF1];
        // (one reservation for the larger of the two phases, not infer_scratch_reserve twice: that would free and
        // allocate again where the second phase is the larger)
        slice_p[i] = n * infer_widest(P); slice_q[i] = n * infer_widest(Q);
        if (act_general_reserve(t, std::max(2 * slice_p[i], G::CRITICS * slice_q[i]))) return -1;
        LP = std::max(LP, P.nl); LQ = std::max(LQ, Q.nl);
    }
    MomentsStage MS;
    if (stats) moments_carve(ST.bytes, MS, n_trainers);
    EvalRowsStage RS;
    if (src) eval_rows_carve(ST.bytes, RS, n_trainers, n_rows);
    if (ST.reserve(t0)) return -1;
    const sac_trainer::ActStage &S = t0->act_stage;
    LS.bind(S.h, S.d);
    typename G::YMember *ytab = reinterpret_cast<typename G::YMember *>(S.h + tab_bytes);
    int yblocks = 0, m = 0, row_wgs = 0;
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        const int n = n_rows[i];
        auto dev = [&](int k) { return ST.dev(i, k, ST.size[i][k] != 0); };        // (null: a part nobody asked for)
        row_wgs += eval_inputs<Obj>(ST, RS, m, i, n, io[i], src, row_wgs);
        float *rows = dev(Obj::P_ROWS);
        // the policy chains, launches 0 .. : on s and on s'
        for (int s = 0; s < 2; ++s) {
            const GenNet &P = t->gen->net[G::policy_net[s]];
            const float *x = dev(s ? EVAL_P_NOBS : EVAL_P_OBS);
            LS.chain({P, x, x, P.L[0].K, n, t->act_gen, s * slice_p[i], dev(G::action[s])}, [&](sac::LayerJob &J, int l) {
                if (l + 1 == P.nl) G::head(J, t, s, n, dev);
            });
        }
        // the critics, launches LP .. : chain s writes row s of `rows`
        for (int s = 0; s < G::CRITICS; ++s) {
            const EvalCritic &c = G::critics[s];
            LS.chain({t->gen->net[c.net], dev(c.obs), dev(c.act), t->O, n, t->act_gen, s * slice_q[i], rows + (size_t)s * n,
                      true, LP});
        }
        if (stats) moments_member<Obj>(S, MS, m, i, dev, n, t->A);
        typename G::YMember &M = ytab[m++];
        M.rew = dev(EVAL_P_REW); M.term = dev(EVAL_P_TERM); M.rows = rows;
        M.n = n; M.wg0 = yblocks;
        M.rs = t->cfg.reward_scale; M.discount = t->cfg.discount;
        if constexpr (!Obj::TD3) { M.alpha = C.alpha[i]; M.pad = 0; }       // (y's entropy term)
        yblocks += (n + EG_YROWS - 1) / EG_YROWS;
    }
    if (src && eval_rows_launch(t0, RS, m, row_wgs, src, n_trainers, n_rows)) return -1;
    for (int l = 0; l < LP + LQ; ++l)
        if (LS.launch(l < LP ? G::policy_kernel : k_eval_layer<true>, t0, l)) return -1;
    hipLaunchKernelGGL(G::y_kernel, dim3(yblocks), dim3(EG_YROWS), 0, t0->stream,
                       reinterpret_cast<const typename G::YMember *>(S.d + tab_bytes), m);
    SAC_HIP(hipGetLastError());
    if (stats && moments_launch<Obj>(t0, MS, m)) return -1;
    if (wait_trainer_stream(t0)) return -1;
    for (int i = 0; i < n_trainers; ++i)
        if (n_rows[i]) eval_finish<Obj>(ST, MS, C, i, io[i], stats ? &stats[i] : nullptr);
    return 0;
}

// (declared extern "C" in include/sac_hip.h)
int sac_evaluate_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, sac_eval_io_t *io) {
    SAC_REQUIRE(trainers && n_rows && io, "bad arguments to sac_evaluate_general_many");
    const InferEntry IE = eval_entry<SacEval>(
        "sac_evaluate_general_many", true,
        "sac_evaluate is its device evaluation entry, sac_evaluate_general serves the general step");
    return eval_general_many<SacEval>(IE, trainers, n_trainers, n_rows, io, nullptr);
}

int sac_evaluate_general_stats_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, sac_eval_io_t *io,
                                    sac_eval_stats_t *stats) {
    SAC_REQUIRE(trainers && n_rows && io && stats, "bad arguments to sac_evaluate_general_stats_many");
    const InferEntry IE = eval_entry<SacEval>(
        "sac_evaluate_general_stats_many", true,
        "sac_evaluate_stats_many is its entry, sac_evaluate_general_stats_many serves the general step");
    return eval_general_many<SacEval>(IE, trainers, n_trainers, n_rows, io, stats);
}

int sac_evaluate_replay_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
                                     const sac_eval_src_t *src, sac_eval_io_t *io, sac_eval_stats_t *stats) {
    SAC_REQUIRE(trainers && n_rows && src && io, "bad arguments to sac_evaluate_replay_general_many");
    const InferEntry IE = eval_entry<SacEval>(
        "sac_evaluate_replay_general_many", true,
        "sac_evaluate_replay_many is its entry, sac_evaluate_replay_general_many serves the general step");
    return eval_general_many<SacEval>(IE, trainers, n_trainers, n_rows, io, stats, src);
}

int sac_evaluate_general(sac_trainer_t *t, int64_t n, sac_eval_io_t *io) {
    SAC_REQUIRE(t && io, "bad arguments to sac_evaluate_general");
    if (int rc = infer_admit_solo("sac_evaluate_general", n)) return rc;
    const int32_t rows = (int32_t)n;
    return sac_evaluate_general_many(&t, 1, &rows, io);
}
