// Evaluating the TD3 objectives on the device: the forward half of the TD3 step on rows the run has not trained on
// (included by sac_trainer.hip behind sac_eval.h, whose LDS layout and y expression it shares).
//
// k_eval_td3 computes, for 1..1024 transitions (s, a, r, d, s') with their N(0,1) smoothing draw eps, of each of
// 1..SAC_GROUP_MAX TD3 trainers in ONE launch and from the live weights,
//
//   chain Q   [s | a] -> qf1 -> qf2                                               q1, q2
//   chain P   s -> policy: a_pi = tanh(last_fc) (k_act's TD3 action); [s | a_pi] -> qf1          q_pi (a_pi)
//   chain N   s' -> TARGET policy: a_target = tanh(last_fc);
//             a_smooth = a_target + clamp_nan(eps sigma, -clip, clip), the step's expression: the sum is NOT clipped to
//             the action range; [s' | a_smooth] -> target_qf1 -> target_qf2       tq1, tq2, y (a_target, a_smooth)
//   y = rs r + ((1 - d) discount) fminf(tq1, tq2), every operation rounded to float32 on its own and none fused:
//       eval_y (sac_eval.h) with alpha = 0 and log_pi = 0, which subtracts a zero and leaves every bit where it was
//
// sigma and clip are the trainer's target_policy_noise / target_policy_noise_clip, handed in through the member table.
// There is no entropy term and no stochastic head: a TD3 policy is TanhMlpPolicy.
//
//   grid    one workgroup (4 waves) per (member, chain, 16-row block), as k_eval: three workgroups per row-block, found
//           through the per-member table Td3EvalMember (device-visible memory, read with scalar loads).  Workgroups never
//           talk to each other: no hand-offs, no spinning, no atomics.
//   LDS     k_eval's layout (eval_lds_bytes): input [16][round_up(KQ, 64)], both hidden layers [16][256], the head
//           [16][32], the Q output columns [2][16]
//   math    the pieces of sac_infer.h, unchanged: infer_fill, infer_hidden, infer_head, infer_action (stochastic = false),
//           infer_q_out
//
// So q1, q2, q_pi, tq1, tq2 are bit for bit k_qval's values on the same rows and a_pi bit for bit k_act's.  Row
// independence as there: a row's columns are a function of that row's inputs and the member's weights only; rows beyond a
// member's n are zero padding and are never written; a NaN row stays in its row.  The kernel writes the caller's outputs
// in the staging (act_stage_reserve, sac_act.h) and nothing else: nothing the step kernels read, no noise counter, no
// parameter.
//
// SAC trainers are refused (sac_evaluate is their entry) and so are general-step TD3 trainers (TD3Trainer.evaluate_td3's
// host path serves them).
#pragma once

namespace sac {

struct Td3EvalMember {
    const float *P[6];                       // forward copies (Net::P): policy, qf1, qf2, target_qf1, target_qf2, target policy
    const float *obs, *act, *rew, *term, *nobs, *eps;
    float *rows;                             // (TD3_EVAL_ROWS_N, n)
    float *a_pi, *a_target, *a_smooth;       // (n, A) each, or null
    long long pW[3], pB[3], tW[3], tB[3], qW[3], qB[3];   // the layers inside the policy's / the target policy's / a Q net's P
    int O, A, KP, NH;
    int n, wg0;                              // rows; first workgroup of this member in the launch
    float sigma, clip, rs, discount;
};

// the smoothed target action, each operation rounded to float32 on its own (as eval_y: NumPy float32 restates it bit
// for bit); a NaN draw passes both comparisons of clamp_nan and stays a NaN
__device__ __forceinline__ float td3_eval_smooth(float a_target, float eps, float sigma, float clip) {
#pragma clang fp contract(off)
    const float noise = clamp_nan(eps * sigma, -clip, clip);
    return a_target + noise;
}

enum { T3E_Q1, T3E_Q2, T3E_Q_PI, T3E_TQ1, T3E_TQ2, T3E_Y, T3E_ROWS_N };

__global__ __launch_bounds__(256) void k_eval_td3(const Td3EvalMember *__restrict__ tab, int n_members) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Td3EvalMember *M = tab + infer_member(tab, n_members, &Td3EvalMember::wg0);
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
        if (a == 0 && grow < n) {
            rows[(size_t)T3E_Q1 * n + grow] = QL[r];
            rows[(size_t)T3E_Q2 * n + grow] = QL[RB + r];
        }
        return;
    }

    const bool next = chain == 2;        // (wave-uniform)
    // [s or s' | 0]: the action columns are written by the head below
    infer_fill(X0, KL0, row0, n, next ? sload(&M->nobs) : sload(&M->obs), O);
    const float *PP = sload(&M->P[next ? 5 : 0]);
    const long long *hW = next ? M->tW : M->pW, *hB = next ? M->tB : M->pB;
    infer_hidden(PP, hW, hB, X0, KL0, KP, X1, X2, in_place);
    infer_head(PP, hW, hB, NH, X2, HL);
    // TanhMlpPolicy: the action as k_act's (infer_action, no noise under the tanh); the target's is smoothed behind it
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
    X0[lds_off(r, KP + a, KL0)] = actv;  // the whole action chunk (0 beyond A)
    const int nq = next ? 2 : 1;         // chain P: qf1 alone (the policy loss is -mean Q1(s, pi(s)))
#pragma unroll 1
    for (int q = 0; q < nq; ++q) {       // qf1, or the two target nets
        const float *P = sload(&M->P[(next ? 3 : 1) + q]);
        infer_hidden(P, M->qW, M->qB, X0, KL0, KQ, X1, X2, in_place);
        infer_q_out(P, M->qW, M->qB, X2, QL + RB * q);
    }
    if (a == 0 && grow < n) {
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
}

}  // namespace sac

namespace {

std::atomic<bool> g_td3_eval_lds_raised[64];

}  // namespace

static_assert((int)T3E_ROWS_N == (int)TD3_EVAL_ROWS_N && (int)T3E_Y == (int)TD3_EVAL_Y && (int)T3E_Q_PI == (int)TD3_EVAL_Q_PI,
              "k_eval_td3's rows are sac_hip.h's");

// (declared extern "C" in include/sac_hip.h)
int td3_evaluate_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, td3_eval_io_t *io) {
    SAC_REQUIRE(trainers && n_rows && io, "bad arguments to td3_evaluate_many");
    InferEntry IE = {"td3_evaluate_many", false, false, "device evaluation",
                     "sac_get_params and a forward on the host is the path", "evaluate"};
    IE.td3_only = true;
    if (int rc = infer_admit(IE, trainers, n_trainers, n_rows, [&](int i) {
            const td3_eval_io_t &E = io[i];
            SAC_REQUIRE(E.obs && E.act && E.rew && E.term && E.next_obs && E.eps && E.rows,
                        "trainer %d: a null input array or null rows", i);
            return 0;
        })) return rc;
    sac_trainer *t0 = trainers[0];

    // per member: obs act rew term nobs eps | rows a_pi a_target a_smooth
    enum { NPART = 10 };
    size_t off[SAC_GROUP_MAX][NPART], bytes = infer_align(sizeof(Td3EvalMember) * SAC_GROUP_MAX);
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        const size_t n = (size_t)n_rows[i], nO = n * t->O, nA = n * t->A;
        const td3_eval_io_t &E = io[i];
        const size_t part[NPART] = {nO, nA, n, n, nO, nA, n * TD3_EVAL_ROWS_N,
                                    n && E.a_pi ? nA : 0, n && E.a_target ? nA : 0, n && E.a_smooth ? nA : 0};
        infer_carve(bytes, off[i], part, NPART);
    }
    if (act_stage_reserve(t0, bytes)) return -1;
    const sac_trainer::ActStage &S = t0->act_stage;
    Td3EvalMember *tab = reinterpret_cast<Td3EvalMember *>(S.h);
    int wgs = 0, m = 0, kq_max = 0;
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        const td3_eval_io_t &E = io[i];
        const size_t n = (size_t)n_rows[i], nO = n * t->O, nA = n * t->A;
        Td3EvalMember &M = tab[m++];
        for (int k = 0; k < 6; ++k) M.P[k] = t->net[k].P;
        auto in = [&](int k, const float *from, size_t count) {
            memcpy(S.h + off[i][k], from, sizeof(float) * count);
            return reinterpret_cast<const float *>(S.d + off[i][k]);
        };
        auto out = [&](int k, bool asked) { return asked ? reinterpret_cast<float *>(S.d + off[i][k]) : nullptr; };
        M.obs = in(0, E.obs, nO); M.act = in(1, E.act, nA); M.rew = in(2, E.rew, n); M.term = in(3, E.term, n);
        M.nobs = in(4, E.next_obs, nO); M.eps = in(5, E.eps, nA);
        M.rows = out(6, true); M.a_pi = out(7, E.a_pi); M.a_target = out(8, E.a_target); M.a_smooth = out(9, E.a_smooth);
        const Net &NP = t->net[SAC_NET_POLICY], &NT = t->net[SAC_NET_TARGET_POLICY], &NQ = t->net[SAC_NET_QF1];
        for (int l = 0; l < 3; ++l) {
            M.pW[l] = NP.L[l].offW; M.pB[l] = NP.L[l].offB;
            M.tW[l] = NT.L[l].offW; M.tB[l] = NT.L[l].offB;
            M.qW[l] = NQ.L[l].offW; M.qB[l] = NQ.L[l].offB;
        }
        M.O = t->O; M.A = t->A; M.KP = t->KP; M.NH = t->NH;
        M.n = n_rows[i]; M.wg0 = wgs;
        M.sigma = t->dev.td3_sigma; M.clip = t->dev.td3_clip;
        M.rs = t->cfg.reward_scale; M.discount = t->cfg.discount;
        wgs += 3 * ((n_rows[i] + RB - 1) / RB);
        kq_max = std::max(kq_max, t->KQ);
    }
    const size_t lds = eval_lds_bytes(kq_max);
    if (infer_raise_lds(reinterpret_cast<const void *>(k_eval_td3), g_td3_eval_lds_raised, t0->device, lds,
                        eval_lds_bytes(512))) return -1;
    hipLaunchKernelGGL(k_eval_td3, dim3(wgs), dim3(256), lds, t0->stream, reinterpret_cast<const Td3EvalMember *>(S.d), m);
    SAC_HIP(hipGetLastError());
    if (wait_trainer_stream(t0)) return -1;
    for (int i = 0; i < n_trainers; ++i) {
        if (n_rows[i] == 0) continue;
        td3_eval_io_t &E = io[i];
        const size_t n = (size_t)n_rows[i], nA = n * trainers[i]->A;
        memcpy(E.rows, S.h + off[i][6], sizeof(float) * n * TD3_EVAL_ROWS_N);
        float *const dst[3] = {E.a_pi, E.a_target, E.a_smooth};
        for (int k = 0; k < 3; ++k)
            if (dst[k]) memcpy(dst[k], S.h + off[i][7 + k], sizeof(float) * nA);
    }
    return 0;
}

int td3_evaluate(sac_trainer_t *t, int64_t n, td3_eval_io_t *io) {
    SAC_REQUIRE(t && io, "bad arguments to td3_evaluate");
    SAC_REQUIRE(n >= 1 && n <= ACT_MAX_ROWS, "td3_evaluate: %lld rows (1..%d per call)", (long long)n, ACT_MAX_ROWS);
    const int32_t rows = (int32_t)n;
    return td3_evaluate_many(&t, 1, &rows, io);
}
