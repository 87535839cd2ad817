// Evaluating the TD3 objectives on the device for general-step trainers: nets of any depth and width (included by
// sac_trainer.hip behind sac_eval_general.h and td3_eval.h).
//
// What k_eval_td3 (td3_eval.h) computes in one launch for the fused kernels' shapes -- the nine arrays of td3_eval_io_t
// for 1..1024 transitions (s, a, r, d, s') with their smoothing draw eps, of each of 1..SAC_GROUP_MAX TD3 trainers, from
// the live weights -- is computed here layer by layer: evaluate_general_many's scheme (sac_eval_general.h), one
// table-driven launch per layer depth on the first member's stream and ONE wait at the end.  The six nets are read where
// the general step keeps them (sac_general::net[...].P: nn.Linear layout W [N][K] then b): nothing is repacked.
//
//   schedule  with LP = the deepest policy of the call (hidden layers + head) and LQ = the deepest critic:
//               launches 0 .. LP-1        k_eval_layer_td3: policy layer l of every member that has one, TWO jobs per
//                                         member -- the policy on the rows s and the TARGET policy (a net of its own,
//                                         SAC_NET_TARGET_POLICY) on the rows s'.  A member's head is its last layer,
//                                         whatever the launch index.
//               launches LP .. LP+LQ-1    k_eval_layer<true> (sac_eval_general.h) unchanged: critic layer l of every
//                                         member that has one, FIVE jobs per member in the order of TD3_EVAL_Q1 .. TQ2 --
//                                         [s | a] through qf1 and qf2, [s | a_pi] through qf1, [s' | a_smooth] through
//                                         target_qf1 and target_qf2.  Chain s writes row s of `rows`.
//               launch LP+LQ              k_eval_y_td3: y, elementwise, from the columns the launches in front of it wrote
//   table     a launch carries up to 5 SAC_GROUP_MAX = 80 jobs of the EG_JOBS a table holds (LayerJob, LayerSchedule)
//   kernel    infer_layer_find, then infer_layer_frame<float, false, LayerHeadTd3>
//   hidden    infer_layer_tile<float, false> and infer_layer_store with ReLU: k_act_layer's hidden layers
//   head      N = A <= 16, one column tile, through HL: the deterministic action is infer_action's with stochastic = false
//             (k_act_layer's LAYER_TD3 action, bit for bit).  LAYER_TD3: a_pi into J->Y.  LAYER_TD3_EVAL, the target chain:
//             a_target into J->mu where the caller asked for it, and a_smooth = td3_eval_smooth(a_target, eps, sigma, clip)
//             (td3_eval.h, as it stands) into J->Y; sigma and clip ride in the job's two pad words.  a_pi and a_smooth
//             ALWAYS go to the staging, where the critic launches read them.  eps is loaded for live rows only.
//   critics   the five Q columns are bit for bit sac_q_values_general's on the same rows
//   y         eval_y (sac_eval.h) with alpha = 0 and log_pi = 0, as k_eval_td3 calls it
//
// Workgroups never talk to each other: no hand-offs, no spinning, no atomics; the order between layers is the order of
// the launches on one stream.  Rows beyond a job's n repeat row n - 1 on the way in and are never written.  Vector stores
// only.
//
// The scratch is the trainer's act_gen pair (act_general_reserve), shared with sac_policy_act_general and
// sac_q_values_general -- each of those calls, and this one, ends with a wait on the stream, so they never overlap.  Each
// buffer holds max(2 n x the widest policy layer, 5 n x the widest critic layer) floats.
//
// SAC trainers are refused (sac_evaluate_general is their entry) and so are TD3 trainers with the fused kernels' shapes
// (td3_evaluate is theirs).
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
static_assert(5 * SAC_GROUP_MAX <= EG_JOBS, "a critic launch of a TD3 evaluation fits the evaluation's job table");

// td3_evaluate_general_many (stats and src null), td3_evaluate_general_stats_many and td3_evaluate_replay_general_many,
// as evaluate_general_many (sac_eval_general.h) serves the SAC entries of the same names: with stats,
// k_eval_moments_td3 (td3_eval_moments.h) runs behind k_eval_y_td3 in front of the wait and a null io[i].rows is taken
// (a_pi has its place in the staging either way); with src, k_eval_rows (sac_eval_rows.h) fills the five input parts
// from src[i]'s replay storage in front of the first layer launch
static int td3_evaluate_general_body(const InferEntry &IE, sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
                                     td3_eval_io_t *io, td3_eval_stats_t *stats, const sac_eval_src_t *src = nullptr) {
    if (int rc = infer_admit(IE, trainers, n_trainers, n_rows, [&](int i) {
            return src ? eval_rows_admit(io[i], src[i], trainers[i], i, n_rows[i], !stats) : td3_eval_admit_io(io[i], i, !stats);
        })) return rc;
    sac_trainer *t0 = trainers[0];

    // the staging: the layer tables, k_eval_y_td3's table, then per member
    //   obs act rew term nobs eps | rows a_pi a_smooth (always: the critic launches read them) a_target
    enum { P_OBS, P_ACT, P_REW, P_TERM, P_NOBS, P_EPS, P_ROWS, P_A_PI, P_A_SMOOTH, P_A_TARGET, NPART };
    LayerSchedule LS(EG_JOBS);
    const size_t tab_bytes = LS.bytes(EG_LAUNCHES);
    InferStage ST(tab_bytes + infer_align(sizeof(EvalYTd3Member) * SAC_GROUP_MAX));
    int LP = 0, LQ = 0;
    size_t slice_p[SAC_GROUP_MAX] = {}, slice_q[SAC_GROUP_MAX] = {};
    for (int i = 0; i < n_trainers; ++i) {
        sac_trainer *t = trainers[i];
        const size_t n = (size_t)n_rows[i], nO = n * t->O, nA = n * t->A;
        const td3_eval_io_t &E = io[i];
        const size_t part[NPART] = {nO, nA, n, n, nO, nA, n * TD3_EVAL_ROWS_N, nA, nA, n && E.a_target ? nA : 0};
        ST.carve(i, part, NPART);
        if (n == 0) continue;
        // (the policy and its target share their layout, and so do the four Q nets)
        const GenNet &P = t->gen->net[SAC_NET_POLICY], &Q = t->gen->net[SAC_NET_QF1];
        slice_p[i] = n * infer_widest(P); slice_q[i] = n * infer_widest(Q);
        if (act_general_reserve(t, std::max(2 * slice_p[i], 5 * slice_q[i]))) return -1;
        LP = std::max(LP, P.nl); LQ = std::max(LQ, Q.nl);
    }
    MomentsStage MS;
    if (stats) moments_carve(ST.bytes, MS, n_trainers);
    EvalRowsStage RS;
    if (src) eval_rows_carve(ST.bytes, RS, n_trainers, n_rows);
    if (ST.reserve(t0)) return -1;
    const sac_trainer::ActStage &S = t0->act_stage;
    LS.bind(S.h, S.d);
    EvalYTd3Member *ytab = reinterpret_cast<EvalYTd3Member *>(S.h + tab_bytes);
    int yblocks = 0, m = 0, row_wgs = 0;
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        const td3_eval_io_t &E = io[i];
        const int n = n_rows[i];
        auto dev = [&](int k) { return ST.dev(i, k); };
        if (src) {
            row_wgs += eval_rows_member(S, RS, m, i, row_wgs, src[i], n, dev(P_OBS), dev(P_ACT), dev(P_REW), dev(P_TERM), dev(P_NOBS));
        } else {
            ST.in(i, P_OBS, E.obs); ST.in(i, P_ACT, E.act); ST.in(i, P_REW, E.rew); ST.in(i, P_TERM, E.term);
            ST.in(i, P_NOBS, E.next_obs);
        }
        ST.in(i, P_EPS, E.eps);
        float *rows = dev(P_ROWS);
        // the policy on s and the target policy on s', launches 0 .. : their heads write a_pi and a_smooth (a_target)
        for (int s = 0; s < 2; ++s) {
            const GenNet &P = t->gen->net[s ? SAC_NET_TARGET_POLICY : SAC_NET_POLICY];
            const float *x = dev(s ? P_NOBS : P_OBS);
            LS.chain({P, x, x, P.L[0].K, n, t->act_gen, s * slice_p[i], dev(s ? P_A_SMOOTH : P_A_PI)},
                     [&](sac::LayerJob &J, int l) {
                if (l + 1 < P.nl) return;
                J.kind = s ? LAYER_TD3_EVAL : LAYER_TD3; J.A = t->A;
                if (!s) return;
                J.eps = dev(P_EPS);
                J.mu = E.a_target ? dev(P_A_TARGET) : nullptr;
                static_assert(sizeof(J.pad[0]) == sizeof(float), "sigma and clip ride in the pad words");
                memcpy(&J.pad[0], &t->gen->dev.td3_sigma, sizeof(float));       // (the general step's own record:
                memcpy(&J.pad[1], &t->gen->dev.td3_clip, sizeof(float));        // gen_build_td3 fills it, not t->dev)
            });
        }
        // the critics, launches LP .. : chain s writes row s of `rows` (TD3_EVAL_Q1 .. TD3_EVAL_TQ2)
        const int net_of[5] = {SAC_NET_QF1, SAC_NET_QF2, SAC_NET_QF1, SAC_NET_TARGET_QF1, SAC_NET_TARGET_QF2};
        const int obs_of[5] = {P_OBS, P_OBS, P_OBS, P_NOBS, P_NOBS};
        const int act_of[5] = {P_ACT, P_ACT, P_A_PI, P_A_SMOOTH, P_A_SMOOTH};
        for (int s = 0; s < 5; ++s)
            LS.chain({t->gen->net[net_of[s]], dev(obs_of[s]), dev(act_of[s]), t->O, n, t->act_gen, s * slice_q[i],
                      rows + (size_t)s * n, true, LP});
        if (stats) td3_moments_member(S, MS, m, i, rows, dev(P_A_PI), n, t->A);
        EvalYTd3Member &M = ytab[m++];
        M.rew = dev(P_REW); M.term = dev(P_TERM); M.rows = rows;
        M.n = n; M.wg0 = yblocks;
        M.rs = t->cfg.reward_scale; M.discount = t->cfg.discount;
        yblocks += (n + EG_YROWS - 1) / EG_YROWS;
    }
    if (src && eval_rows_launch(t0, RS, m, row_wgs, src, n_trainers, n_rows)) return -1;
    for (int l = 0; l < LP + LQ; ++l)
        if (LS.launch(l < LP ? k_eval_layer_td3 : k_eval_layer<true>, t0, l)) return -1;
    hipLaunchKernelGGL(k_eval_y_td3, dim3(yblocks), dim3(EG_YROWS), 0, t0->stream,
                       reinterpret_cast<const EvalYTd3Member *>(S.d + tab_bytes), m);
    SAC_HIP(hipGetLastError());
    if (stats && td3_moments_launch(t0, MS, m)) return -1;
    if (wait_trainer_stream(t0)) return -1;
    for (int i = 0; i < n_trainers; ++i) {
        if (n_rows[i] == 0) continue;
        const td3_eval_io_t &E = io[i];
        ST.back(i, {{E.rows, P_ROWS}, {E.a_pi, P_A_PI}, {E.a_target, P_A_TARGET}, {E.a_smooth, P_A_SMOOTH}});
        if (stats) td3_moments_read(S, MS, i, &stats[i]);
    }
    return 0;
}

static InferEntry td3_eval_general_entry(const char *fn, const char *instead) {
    InferEntry IE = {fn, true, false, "device evaluation", instead, "evaluate"};
    IE.td3_only = true;
    return IE;
}

// (declared extern "C" in include/sac_hip.h)
int td3_evaluate_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, td3_eval_io_t *io) {
    SAC_REQUIRE(trainers && n_rows && io, "bad arguments to td3_evaluate_general_many");
    const InferEntry IE = td3_eval_general_entry(
        "td3_evaluate_general_many", "td3_evaluate is its device evaluation entry, td3_evaluate_general serves the general step");
    return td3_evaluate_general_body(IE, trainers, n_trainers, n_rows, io, nullptr);
}

int td3_evaluate_general_stats_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, td3_eval_io_t *io,
                                    td3_eval_stats_t *stats) {
    SAC_REQUIRE(trainers && n_rows && io && stats, "bad arguments to td3_evaluate_general_stats_many");
    const InferEntry IE = td3_eval_general_entry(
        "td3_evaluate_general_stats_many", "td3_evaluate_stats_many is its entry, td3_evaluate_general_stats_many serves the general step");
    return td3_evaluate_general_body(IE, trainers, n_trainers, n_rows, io, stats);
}

int td3_evaluate_replay_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
                                     const sac_eval_src_t *src, td3_eval_io_t *io, td3_eval_stats_t *stats) {
    SAC_REQUIRE(trainers && n_rows && src && io, "bad arguments to td3_evaluate_replay_general_many");
    const InferEntry IE = td3_eval_general_entry(
        "td3_evaluate_replay_general_many",
        "td3_evaluate_replay_many is its entry, td3_evaluate_replay_general_many serves the general step");
    return td3_evaluate_general_body(IE, trainers, n_trainers, n_rows, io, stats, src);
}

int td3_evaluate_general(sac_trainer_t *t, int64_t n, td3_eval_io_t *io) {
    SAC_REQUIRE(t && io, "bad arguments to td3_evaluate_general");
    if (int rc = infer_admit_solo("td3_evaluate_general", n)) return rc;
    const int32_t rows = (int32_t)n;
    return td3_evaluate_general_many(&t, 1, &rows, io);
}
