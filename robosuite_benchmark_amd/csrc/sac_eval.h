// Evaluating an objective on the device: the forward half of the step on rows the run has not trained on (included by
// sac_trainer.hip).  Here: the row-block frame of every such evaluation, once, and the SAC objective; td3_eval.h holds
// the TD3 objective.  The host staging is InferStage (sac_infer.h), which the general-shape entries share.
//
// eval_frame<Objective> computes, for 1..1024 transitions (s, a, r, d, s') of each of 1..SAC_GROUP_MAX trainers in ONE
// launch and from the live weights, three chains per 16-row block:
//   chain Q   [s | a] -> qf1 -> qf2                                               rows 0, 1 of `rows`: q1, q2
//   chain P   s  -> Objective::policy -> Objective::head -> action; [s  | action] -> qf1 (-> qf2: Objective::critics)
//   chain N   s' -> Objective::policy -> Objective::head -> action; [s' | action] -> target_qf1 -> target_qf2
//             behind either, Objective::rows: the chain's columns of `rows`
// An objective is a struct of static __device__ functions that supplies these four and nothing else; head is what stands
// between infer_head and the write of the action chunk: the action that goes into the Q nets' input, the objective's own
// (n, A) outputs, and one per-row value handed to rows.
//
//   grid    one workgroup (4 waves) per (member, chain, 16-row block): three workgroups per row-block, the workgroups of
//           all members side by side, found through the objective's per-member table (device-visible memory, read with
//           scalar loads; EvalCommon leads it).  Workgroups never talk to each other: no hand-offs, no spinning, no atomics.
//   LDS     the row-block's input [16][round_up(KQ, 64)] -- the policy reads its first KP columns, the Q nets all KQ --
//           both hidden layers [16][256], the head [16][32], the Q output columns [2][16]
//   math    the nets where the step keeps them (Net::P, fragment-major, padded to 256; first Q layer over
//           [obs | pad | act | pad]), through the pieces of sac_infer.h that k_act and k_qval run: infer_fill,
//           infer_hidden, infer_head, infer_action, infer_q_out
//
// So the Q columns are bit for bit k_qval's values on the same rows and the actions bit for bit k_act's.  Row
// independence as there: a row's columns are a function of that row's inputs and the member's weights only.  Rows beyond
// a member's n are zero padding and are never written.  A kernel writes the caller's outputs in the staging
// (act_stage_reserve, sac_infer.h) and nothing else: nothing the step kernels read, no noise counter, no parameter.
//
// k_eval = eval_frame<SacObjective>, with the N(0,1) draws eps / eps_next:
//   chain P   the policy with eps: a_new = tanh(mean + exp(clamp(log_std)) eps), log_pi, mu, clamped log_std; qf1, qf2
//                                                                                 q1_new, q2_new, log_pi (mu, log_std, a_new)
//   chain N   the same policy with eps_next: a_next, log_pi_next                  tq1, tq2, log_pi_next, y (a_next)
//   y = rs r + ((1 - d) discount) (fminf(tq1, tq2) - alpha log_pi_next), every operation rounded to float32 on its own
//       and none fused (eval_y), so that NumPy float32 restates it bit for bit
//   log_pi is the step's expression (k_fwd_b's tanh-Gaussian head) on the same head values, summed by group16_sum
//
// alpha is the trainer's CURRENT entropy coefficient (what sac_get_scalars reports as scalars[5]; 1 with automatic tuning
// off; exp(log_alpha) while a trainer has neither stepped nor been given scalars and its alpha still reads 0), read on
// the host behind the drain and handed in through the member table: this is the objective at the current parameters.
// The training step logs its Alpha, Q Targets and losses behind its own alpha update, so they differ from
// an evaluation of the same batch by that one alpha step.
//
// General-step trainers are refused (SACTrainer.evaluate's host path serves them, or sac_evaluate_general:
// sac_eval_general.h), TD3 trainers too: this is the SAC objective.
#pragma once

namespace sac {

// the fields every objective's member table starts with
struct EvalCommon {
    const float *P[6];                       // forward copies (Net::P): policy, qf1, qf2, target_qf1, target_qf2, TD3's target policy
    const float *obs, *act, *rew, *term, *nobs;
    float *rows;                             // (the objective's columns, n)
    long long pW[3], pB[3], qW[3], qB[3];    // the layers inside the policy's P / a Q net's P
    int O, A, KP, NH;
    int n, wg0;                              // rows; first workgroup of this member in the launch
    float rs, discount;
};

struct EvalPolicy { const float *P; const long long *W, *B; };     // a policy's forward copy and the layers inside it

// y, every operation rounded to float32 on its own so that NumPy float32 restates it bit for bit.  With this compiler
// __fmul_rn / __fadd_rn are plain `x * y` / `x + y`, which -ffp-contract=fast fuses into FMAs like any other product
// and sum; contraction is switched off for this body instead (the operations stay unfused after inlining: an FMA is only
// formed from operations that both allow it).
__device__ __forceinline__ float eval_y(float rs, float r, float d, float discount, float tq1, float tq2, float alpha,
                                        float lp_next) {
#pragma clang fp contract(off)
    const float soft = fminf(tq1, tq2) - alpha * lp_next;
    const float w = (1.0f - d) * discount;
    const float a = rs * r, b = w * soft;
    return a + b;
}

// the row-block frame of Objective (the file comment): the body of k_eval and k_eval_td3
template <class Objective>
__device__ __forceinline__ void eval_frame(const typename Objective::Member *__restrict__ tab, int n_members) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const typename Objective::Member *M = tab + infer_member(tab, n_members, &EvalCommon::wg0);
    const int O = sload(&M->O), A = sload(&M->A), KP = sload(&M->KP), NH = sload(&M->NH), n = sload(&M->n);
    const int KQ = KP + 16, nrb = (n + RB - 1) / RB;
    const int local = (int)blockIdx.x - sload(&M->wg0);
    const int chain = local / nrb, row0 = (local - chain * nrb) * RB;      // 0: Q, 1: P, 2: N
    const int KL0 = (KQ + 63) & ~63;
    float *X0 = lds;                     // [16][KL0]
    float *X1 = X0 + RB * KL0;           // [16][256]
    float *X2 = X1 + RB * H;             // [16][256]
    float *HL = X2 + RB * H;             // [16][32]
    float *QL = HL + RB * ACT_HEAD_LD;   // [2][16]
    const int r = threadIdx.x >> 4, a = threadIdx.x & 15, grow = row0 + r;
    float *rows = sload(&M->rows);
    // X0 is filled in front of the nets, so they get no fill of their own: a net's weight requests follow it
    const auto in_place = [] {};
    if (chain == 0) {
        infer_fill(X0, KL0, row0, n, sload(&M->obs), O, sload(&M->act), KP, A);
#pragma unroll 1
        for (int q = 0; q < 2; ++q) {    // qf1, qf2: their values into QL [2][16]
            const float *P = sload(&M->P[1 + q]);
            infer_hidden(P, M->qW, M->qB, X0, KL0, KQ, X1, X2, in_place);
            infer_q_out(P, M->qW, M->qB, X2, QL + RB * q);
        }
        if (a == 0 && grow < n) {        // q1, q2: rows 0 and 1 of every objective
            rows[grow] = QL[r];
            rows[(size_t)n + grow] = QL[RB + r];
        }
        return;
    }

    const bool next = chain == 2;        // (wave-uniform)
    // [s or s' | 0]: the action columns are written behind the head
    infer_fill(X0, KL0, row0, n, next ? sload(&M->nobs) : sload(&M->obs), O);
    const EvalPolicy pi = Objective::policy(M, next);
    infer_hidden(pi.P, pi.W, pi.B, X0, KL0, KP, X1, X2, in_place);
    infer_head(pi.P, pi.W, pi.B, NH, X2, HL);
    float carry;                         // the head's per-row value, for the epilogue
    X0[lds_off(r, KP + a, KL0)] = Objective::head(M, HL, r, a, A, grow, n, next, carry);   // the whole action chunk (0 beyond A)
    const int nq = Objective::critics(next);
#pragma unroll 1
    for (int q = 0; q < nq; ++q) {       // qf1 (, qf2) or the two target nets
        const float *P = sload(&M->P[(next ? 3 : 1) + q]);
        infer_hidden(P, M->qW, M->qB, X0, KL0, KQ, X1, X2, in_place);
        infer_q_out(P, M->qW, M->qB, X2, QL + RB * q);
    }
    if (a == 0 && grow < n) Objective::rows(M, rows, n, grow, next, QL, r, carry);
}

struct EvalMember : EvalCommon {
    const float *eps, *eps_next;
    float *mu, *log_std, *a_new, *a_next;    // (n, A) each, or null
    float alpha;
    int pad;
};

enum { EVAL_Q1, EVAL_Q2, EVAL_Q1_NEW, EVAL_Q2_NEW, EVAL_TQ1, EVAL_TQ2, EVAL_LOG_PI, EVAL_LOG_PI_NEXT, EVAL_Y, EVAL_ROWS_N };

struct SacObjective {
    typedef EvalMember Member;
    // both chains read the trainer's own policy, and both run two critics
    static __device__ __forceinline__ EvalPolicy policy(const Member *M, bool) { return {sload(&M->P[0]), M->pW, M->pB}; }
    static __device__ __forceinline__ int critics(bool) { return 2; }
    // tanh-Gaussian head: the action as k_act's (infer_action), log_pi as the step's; *lsum: log_pi of the row
    static __device__ __forceinline__ float head(const Member *M, const float *HL, int r, int a, int A, int grow, int n,
                                                 bool next, float &lsum) {
        float lp = 0.f, actv = 0.f;
        if (a < A) {
            const size_t o = (size_t)grow * A + a;
            const float mean = HL[r * ACT_HEAD_LD + a], raw = HL[r * ACT_HEAD_LD + A + a], ls = infer_log_std(raw);
            float v;
            actv = infer_action(HL, r, a, A, true, [&] { return grow < n ? (next ? sload(&M->eps_next) : sload(&M->eps))[o] : 0.f; }, &v);
            const float stdv = expf(ls);
            const float dd = __fsub_rn(v, mean);                             // Normal.log_prob(z)
            const float var = __fmul_rn(stdv, stdv);
            const float nlp = -(dd * dd) / (2.0f * var) - logf(stdv) - 0.91893853320467274178f;
            lp = nlp - logf(1.0f - actv * actv + TANH_EPS);
            if (grow < n) {
                float *pa = next ? sload(&M->a_next) : sload(&M->a_new);
                if (pa) pa[o] = actv;
                if (!next) {
                    float *pm = sload(&M->mu), *pl = sload(&M->log_std);
                    if (pm) pm[o] = mean;
                    if (pl) pl[o] = raw != raw ? raw : ls;       // (fmaxf drops a NaN; torch.clamp and the host path keep it)
                }
            }
        }
        lsum = group16_sum(lp);
        return actv;
    }
    static __device__ __forceinline__ void rows(const Member *M, float *rows, int n, int grow, bool next, const float *QL,
                                                int r, float lsum) {
        const float qa = QL[r], qb = QL[RB + r];
        if (!next) {
            rows[(size_t)EVAL_Q1_NEW * n + grow] = qa;
            rows[(size_t)EVAL_Q2_NEW * n + grow] = qb;
            rows[(size_t)EVAL_LOG_PI * n + grow] = lsum;
        } else {
            const float rew = sload(&M->rew)[grow], d = sload(&M->term)[grow];
            const float alpha = sload(&M->alpha), rs = sload(&M->rs), gamma = sload(&M->discount);
            rows[(size_t)EVAL_TQ1 * n + grow] = qa;
            rows[(size_t)EVAL_TQ2 * n + grow] = qb;
            rows[(size_t)EVAL_LOG_PI_NEXT * n + grow] = lsum;
            rows[(size_t)EVAL_Y * n + grow] = eval_y(rs, rew, d, gamma, qa, qb, alpha, lsum);
        }
    }
};

__global__ __launch_bounds__(256) void k_eval(const EvalMember *__restrict__ tab, int n_members) {
    eval_frame<SacObjective>(tab, n_members);
}

}  // namespace sac

namespace {

size_t eval_lds_bytes(int KQ) { return sizeof(float) * (size_t)RB * (((KQ + 63) & ~63) + 2 * H + ACT_HEAD_LD + 2); }

template <class Member> std::atomic<bool> g_eval_lds_raised[64];     // (infer_raise_lds: per kernel, that is per member table)

void eval_layers(long long *W, long long *B, const Net &N) {
    for (int l = 0; l < 3; ++l) { W[l] = N.L[l].offW; B[l] = N.L[l].offB; }
}

// EvalCommon of trainer t with n rows and its first n_nets nets, but for the parts; the member's three workgroups per
// row-block go behind wgs, its KQ into kq_max
void eval_member(sac::EvalCommon &M, const sac_trainer *t, int n_nets, int n, int &wgs, int &kq_max) {
    for (int k = 0; k < 6; ++k) M.P[k] = k < n_nets ? t->net[k].P : nullptr;
    eval_layers(M.pW, M.pB, t->net[SAC_NET_POLICY]);
    eval_layers(M.qW, M.qB, t->net[SAC_NET_QF1]);
    M.O = t->O; M.A = t->A; M.KP = t->KP; M.NH = t->NH;
    M.n = n; M.wg0 = wgs;
    M.rs = t->cfg.reward_scale; M.discount = t->cfg.discount;
    wgs += 3 * ((n + RB - 1) / RB);
    kq_max = std::max(kq_max, t->KQ);
}

// the frame's launch on t0's stream (wgs workgroups, the m members of the table at the staging's start), and the wait
// behind `behind`, which may launch a reader of the frame's outputs
template <class Member, class Behind>
int eval_launch(void (*kernel)(const Member *, int), sac_trainer *t0, int wgs, int m, int kq_max, Behind behind) {
    const size_t lds = eval_lds_bytes(kq_max);
    if (infer_raise_lds(reinterpret_cast<const void *>(kernel), g_eval_lds_raised<Member>, t0->device, lds, eval_lds_bytes(512)))
        return -1;
    hipLaunchKernelGGL(kernel, dim3(wgs), dim3(256), lds, t0->stream, reinterpret_cast<const Member *>(t0->act_stage.d), m);
    SAC_HIP(hipGetLastError());
    return behind() || wait_trainer_stream(t0) ? -1 : 0;
}

// the entropy coefficient of this moment for every member with rows (sac_get_scalars' scalars[5]; 1 with automatic
// tuning off), behind the drain: what sac_evaluate_many and sac_evaluate_general_many both evaluate y with.  log_alpha
// (the *_stats_many entries; null otherwise): sac_get_scalars' scalars[0] from the same copy of Ctl, which is then made
// with tuning off too.
int eval_read_alpha(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, float *alpha,
                    float *log_alpha = nullptr) {
    for (int i = 0; i < n_trainers; ++i) {
        sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        alpha[i] = 1.0f;
        if (t->cfg.use_automatic_entropy_tuning || log_alpha) {
            Ctl c;
            SAC_HIP(hipMemcpyAsync(&c, t->d_ctl, sizeof(c), hipMemcpyDeviceToHost, t->stream));
            SAC_HIP(hipStreamSynchronize(t->stream));
            // (a trainer that has neither stepped nor been given scalars holds log_alpha and no alpha yet: exp(log_alpha))
            if (t->cfg.use_automatic_entropy_tuning) alpha[i] = c.alpha > 0.f ? c.alpha : expf(c.log_alpha);
            if (log_alpha) log_alpha[i] = c.log_alpha;
        }
    }
    return 0;
}

// ---- the host half of every evaluation entry: one description per objective, one body per family ----
//
// An objective's host description (SacEval below, Td3Eval in td3_eval.h) is a struct of static members that names
//   IO, Stats                    the caller's structs
//   Member, kernel               the fixed-shape member table and its kernel; NETS of the trainer's nets go into it
//   Moments, moments_kernel      the statistics' member table and kernel; moments(M, dev) names its columns
//   draws[DRAWS]                 the N(0,1) inputs, as pointers to IO's fields
//   arrays[ARRAYS]               the (n, A) outputs, as pointers to IO's fields, with what makes one staged unasked
//   Call                         what is read once per call in front of the staging (prepare) and handed back per member
//                                behind the wait (finish): SAC's alpha and log_alpha, nothing for TD3
//   member(M, t, C, i, dev)      the member's fields beyond EvalCommon
//   General                      the general step's half (sac_eval_general.h, td3_eval_general.h)
// A member's staging, for both families: obs act rew term nobs | the draws | rows | the arrays, in the order of `arrays`.

// an (n, A) output of an objective: staged where the caller asked for it, and besides
template <class IO> struct EvalArray {
    float *IO::*field;
    bool critics;        // the general step's critic launches read it there: always staged by the general body
    bool moments;        // the moments kernel reads it there: staged under stats
};

enum { EVAL_P_OBS, EVAL_P_ACT, EVAL_P_REW, EVAL_P_TERM, EVAL_P_NOBS, EVAL_P_DRAW };      // the parts every objective starts with

struct SacEval {
    typedef sac_eval_io_t IO;
    typedef sac_eval_stats_t Stats;
    typedef sac::EvalMember Member;
    typedef sac::MomentsMember Moments;
    static constexpr auto kernel = sac::k_eval;
    static constexpr auto moments_kernel = sac::k_eval_moments;
    static constexpr bool TD3 = false;
    static constexpr int NETS = 5, DRAWS = 2, ARRAYS = 4, ROWS_N = SAC_EVAL_ROWS_N, MOMENTS_N = SAC_EVAL_MOMENTS_N;
    enum { P_EPS = EVAL_P_DRAW, P_EPS_NEXT, P_ROWS, P_MU, P_LOG_STD, P_A_NEW, P_A_NEXT, NPART };
    static constexpr const float *IO::*draws[DRAWS] = {&IO::eps, &IO::eps_next};
    static constexpr EvalArray<IO> arrays[ARRAYS] = {{&IO::mu, false, true}, {&IO::log_std, false, true},
                                                     {&IO::a_new, true, false}, {&IO::a_next, true, false}};
    struct Call {
        float alpha[SAC_GROUP_MAX], log_alpha[SAC_GROUP_MAX];
        int prepare(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, bool stats) {
            return eval_read_alpha(trainers, n_trainers, n_rows, alpha, stats ? log_alpha : nullptr);
        }
        // the alpha the entry evaluated y with, and under stats the log_alpha of the same Ctl copy
        void finish(int i, IO &E, Stats *st) const {
            E.alpha = alpha[i];
            if (st) { st->alpha = (double)alpha[i]; st->log_alpha = (double)log_alpha[i]; }
        }
    };
    template <class Dev> static void member(Member &M, const sac_trainer *, const Call &C, int i, Dev dev) {
        M.eps = dev(P_EPS); M.eps_next = dev(P_EPS_NEXT);
        M.mu = dev(P_MU); M.log_std = dev(P_LOG_STD); M.a_new = dev(P_A_NEW); M.a_next = dev(P_A_NEXT);
        M.alpha = C.alpha[i]; M.pad = 0;
    }
    template <class Dev> static void moments(Moments &M, Dev dev) {
        M.rows = dev(P_ROWS); M.mu = dev(P_MU); M.log_std = dev(P_LOG_STD);
    }
    struct General;
};

template <class Obj> InferEntry eval_entry(const char *fn, bool general, const char *instead) {
    InferEntry IE = {fn, general, !Obj::TD3, "device evaluation", instead, "evaluate"};
    IE.td3_only = Obj::TD3;
    return IE;
}

// an entry's own refusal for a member with rows: every input array is there, and `rows` unless the entry returns
// statistics (there a null `rows` means that no column is copied back); with src (the replay entries) the draws, `rows`
// and the source (eval_rows_admit, sac_eval_rows.h)
template <class Obj>
int eval_admit_io(const typename Obj::IO &E, const sac_eval_src_t *src, const sac_trainer *t, int i, int n, bool need_rows) {
    if (src) return eval_rows_admit(E, src[i], t, i, n, need_rows);
    bool inputs = E.obs && E.act && E.rew && E.term && E.next_obs;
    for (auto draw : Obj::draws) inputs = inputs && E.*draw;
    if (need_rows) SAC_REQUIRE(inputs && E.rows, "trainer %d: a null input array or null rows", i);
    SAC_REQUIRE(inputs, "trainer %d: a null input array", i);
    return 0;
}

// member i's parts into the call's staging: an array has its place where the caller asked for it, where the moments
// kernel reads it (stats) and where the general step's critic launches do (general)
template <class Obj>
void eval_carve(InferStage &ST, int i, const sac_trainer *t, int n_rows, const typename Obj::IO &E, bool stats, bool general) {
    const size_t n = (size_t)n_rows, nO = n * t->O, nA = n * t->A;
    size_t part[Obj::NPART] = {nO, nA, n, n, nO};
    for (int d = 0; d < Obj::DRAWS; ++d) part[EVAL_P_DRAW + d] = nA;
    part[Obj::P_ROWS] = n * Obj::ROWS_N;
    for (int k = 0; k < Obj::ARRAYS; ++k) {
        const EvalArray<typename Obj::IO> &a = Obj::arrays[k];
        part[Obj::P_ROWS + 1 + k] = n && (E.*a.field || (stats && a.moments) || (general && a.critics)) ? nA : 0;
    }
    ST.carve(i, part, Obj::NPART);
}

// the inputs of member i with n rows (entry m of the launch) into its staging: the five arrays of a transition from the
// caller's, or with src by k_eval_rows from src[i]'s replay storage (its table entry is written here), and the draws.
// Returns the member's k_eval_rows workgroups.
template <class Obj>
int eval_inputs(const InferStage &ST, const EvalRowsStage &RS, int m, int i, int n, const typename Obj::IO &E,
                const sac_eval_src_t *src, int row_wg0) {
    int row_wgs = 0;
    if (src) {
        row_wgs = eval_rows_member(*ST.S, RS, m, i, row_wg0, src[i], n, ST.dev(i, EVAL_P_OBS), ST.dev(i, EVAL_P_ACT),
                                   ST.dev(i, EVAL_P_REW), ST.dev(i, EVAL_P_TERM), ST.dev(i, EVAL_P_NOBS));
    } else {
        ST.in(i, EVAL_P_OBS, E.obs); ST.in(i, EVAL_P_ACT, E.act); ST.in(i, EVAL_P_REW, E.rew); ST.in(i, EVAL_P_TERM, E.term);
        ST.in(i, EVAL_P_NOBS, E.next_obs);
    }
    for (int d = 0; d < Obj::DRAWS; ++d) ST.in(i, EVAL_P_DRAW + d, E.*Obj::draws[d]);
    return row_wgs;
}

// behind the wait: what member i's caller asked for into its arrays, the call's own values, the moment records
template <class Obj>
void eval_finish(const InferStage &ST, const MomentsStage &MS, const typename Obj::Call &C, int i, typename Obj::IO &E,
                 typename Obj::Stats *st) {
    ST.back(i, {{E.rows, Obj::P_ROWS}});
    for (int k = 0; k < Obj::ARRAYS; ++k) ST.back(i, {{E.*Obj::arrays[k].field, Obj::P_ROWS + 1 + k}});
    if (st) moments_read(*ST.S, MS, i, st);
    C.finish(i, E, st);
}

}  // namespace

static_assert((int)EVAL_ROWS_N == (int)SAC_EVAL_ROWS_N && (int)EVAL_Y == (int)SAC_EVAL_Y && EVAL_Q1 == 0 && EVAL_Q2 == 1,
              "k_eval's rows are sac_hip.h's, chain Q's the first two");

// The fixed-shape body of an objective: *_evaluate_many (stats and src null), *_evaluate_stats_many and
// *_evaluate_replay_many.  With stats, the arrays the moments kernel reads always have their place in the staging (only
// the copy to the caller depends on what was asked for), the moments kernel runs behind the frame's kernel in front of the
// wait, and a null io[i].rows is taken.  With src the five input parts of the staging are filled on the device, by
// k_eval_rows (sac_eval_rows.h) in front of the frame's kernel, from src[i]'s replay storage instead of io[i]'s arrays.
template <class Obj>
static int eval_fused_many(const InferEntry &IE, sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
                           typename Obj::IO *io, typename Obj::Stats *stats, const sac_eval_src_t *src = nullptr) {
    if (int rc = infer_admit(IE, trainers, n_trainers, n_rows, [&](int i) {
            return eval_admit_io<Obj>(io[i], src, trainers[i], i, n_rows[i], !stats);
        })) return rc;
    sac_trainer *t0 = trainers[0];
    typename Obj::Call C;
    if (C.prepare(trainers, n_trainers, n_rows, stats != nullptr)) return -1;

    InferStage ST(sizeof(typename Obj::Member) * SAC_GROUP_MAX);
    for (int i = 0; i < n_trainers; ++i) eval_carve<Obj>(ST, i, trainers[i], n_rows[i], io[i], stats != nullptr, false);
    MomentsStage MS;
    if (stats) moments_carve(ST.bytes, MS, n_trainers);
    EvalRowsStage RS;
    if (src) eval_rows_carve(ST.bytes, RS, n_trainers, n_rows);
    if (ST.reserve(t0)) return -1;
    const sac_trainer::ActStage &S = t0->act_stage;
    typename Obj::Member *tab = reinterpret_cast<typename Obj::Member *>(S.h);
    int wgs = 0, m = 0, kq_max = 0, row_wgs = 0;
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        auto dev = [&](int k) { return ST.dev(i, k, ST.size[i][k] != 0); };        // (null: a part nobody asked for)
        typename Obj::Member &M = tab[m];
        eval_member(M, t, Obj::NETS, n_rows[i], wgs, kq_max);
        row_wgs += eval_inputs<Obj>(ST, RS, m, i, n_rows[i], io[i], src, row_wgs);
        M.obs = dev(EVAL_P_OBS); M.act = dev(EVAL_P_ACT); M.rew = dev(EVAL_P_REW); M.term = dev(EVAL_P_TERM);
        M.nobs = dev(EVAL_P_NOBS); M.rows = dev(Obj::P_ROWS);
        Obj::member(M, t, C, i, dev);
        if (stats) moments_member<Obj>(S, MS, m, i, dev, n_rows[i], t->A);
        ++m;
    }
    if (src && eval_rows_launch(t0, RS, m, row_wgs, src, n_trainers, n_rows)) return -1;
    if (eval_launch(Obj::kernel, t0, wgs, m, kq_max, [&] { return stats ? moments_launch<Obj>(t0, MS, m) : 0; })) return -1;
    for (int i = 0; i < n_trainers; ++i)
        if (n_rows[i]) eval_finish<Obj>(ST, MS, C, i, io[i], stats ? &stats[i] : nullptr);
    return 0;
}

// (declared extern "C" in include/sac_hip.h)
int sac_evaluate_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, sac_eval_io_t *io) {
    SAC_REQUIRE(trainers && n_rows && io, "bad arguments to sac_evaluate_many");
    const InferEntry IE = eval_entry<SacEval>("sac_evaluate_many", false,
                                             "sac_get_params and a forward on the host is the path");
    return eval_fused_many<SacEval>(IE, trainers, n_trainers, n_rows, io, nullptr);
}

int sac_evaluate_stats_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, sac_eval_io_t *io,
                            sac_eval_stats_t *stats) {
    SAC_REQUIRE(trainers && n_rows && io && stats, "bad arguments to sac_evaluate_stats_many");
    const InferEntry IE = eval_entry<SacEval>("sac_evaluate_stats_many", false,
                                             "sac_evaluate_general_stats_many is the entry");
    return eval_fused_many<SacEval>(IE, trainers, n_trainers, n_rows, io, stats);
}

int sac_evaluate_replay_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, const sac_eval_src_t *src,
                             sac_eval_io_t *io, sac_eval_stats_t *stats) {
    SAC_REQUIRE(trainers && n_rows && src && io, "bad arguments to sac_evaluate_replay_many");
    const InferEntry IE = eval_entry<SacEval>("sac_evaluate_replay_many", false,
                                             "sac_evaluate_replay_general_many is the entry");
    return eval_fused_many<SacEval>(IE, trainers, n_trainers, n_rows, io, stats, src);
}

int sac_evaluate(sac_trainer_t *t, int64_t n, sac_eval_io_t *io) {
    SAC_REQUIRE(t && io, "bad arguments to sac_evaluate");
    if (int rc = infer_admit_solo("sac_evaluate", n)) return rc;
    const int32_t rows = (int32_t)n;
    return sac_evaluate_many(&t, 1, &rows, io);
}
