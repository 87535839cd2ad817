// Evaluating the SAC objectives on the device: the forward half of the step on rows the run has not trained on (included
// by sac_trainer.hip).
//
// k_eval computes, for 1..1024 transitions (s, a, r, d, s') with their N(0,1) draws eps / eps_next, of each of
// 1..SAC_GROUP_MAX SAC trainers in ONE launch and from the live weights,
//
//   chain Q   [s | a] -> qf1 -> qf2                                               q1, q2
//   chain P   s -> policy with eps: a_new = tanh(mean + exp(clamp(log_std)) eps), log_pi, mu, clamped log_std;
//             [s | a_new] -> qf1 -> qf2                                           q1_new, q2_new, log_pi (mu, log_std, a_new)
//   chain N   s' -> policy with eps_next: a_next, log_pi_next; [s' | a_next] -> target_qf1 -> target_qf2
//                                                                                 tq1, tq2, log_pi_next, y (a_next)
//   y = rs r + ((1 - d) discount) (fminf(tq1, tq2) - alpha log_pi_next), every operation rounded to float32 on its own
//       and none fused (eval_y), so that NumPy float32 restates it bit for bit
//
// alpha is the trainer's CURRENT entropy coefficient (what sac_get_scalars reports as scalars[5]; 1 with automatic tuning
// off; exp(log_alpha) while a trainer has neither stepped nor been given scalars and its alpha still reads 0), read on
// the host behind the drain and handed in through the member table: this is the objective at the current parameters.
// The training step logs its Alpha, Q Targets and losses behind its own alpha update, so they differ from
// an evaluation of the same batch by that one alpha step.
//
//   grid    one workgroup (4 waves) per (member, chain, 16-row block): three workgroups per row-block, the workgroups of
//           all members side by side, found through the per-member table EvalMember (device-visible memory, read with
//           scalar loads).  Workgroups never talk to each other: no hand-offs, no spinning, no atomics.
//   LDS     the row-block's input [16][round_up(KQ, 64)] -- the policy reads its first KP columns, the Q nets all KQ --
//           both hidden layers [16][256], the head [16][32], the Q output columns [2][16]
//   math    the nets where the step keeps them (Net::P, fragment-major, padded to 256; first Q layer over
//           [obs | pad | act | pad]); GEMMs through WRing / gemm_ring in ascending k; hidden layers through
//           act_hidden_epilogue (NaN stays NaN); head and action as k_act's, Q output unit as k_qval's; log_pi is the
//           step's expression (k_fwd_b's tanh-Gaussian head), summed over the actions by group16_sum
//
// So q1, q2, q1_new, q2_new, tq1, tq2 are bit for bit k_qval's values on the same rows and a_new / a_next bit for bit
// k_act's.  Row independence as there: a row's columns are a function of that row's inputs and the member's weights
// only.  Rows beyond a member's n are zero padding and are never written.  The kernel writes the caller's outputs in the
// staging (act_stage_reserve, sac_act.h) and nothing else: nothing the step kernels read, no noise counter, no
// parameter.
//
// General-step trainers are refused (SACTrainer.evaluate's host path serves them), TD3 trainers too: this is the SAC
// objective.
#pragma once

namespace sac {

struct EvalMember {
    const float *P[5];                       // forward copies (Net::P): policy, qf1, qf2, target_qf1, target_qf2
    const float *obs, *act, *rew, *term, *nobs, *eps, *eps_next;
    float *rows;                             // (SAC_EVAL_ROWS_N, n)
    float *mu, *log_std, *a_new, *a_next;    // (n, A) each, or null
    long long pW[3], pB[3], qW[3], qB[3];    // the layers inside the policy's P / a Q net's P
    int O, A, KP, NH;
    int n, wg0;                              // rows; first workgroup of this member in the launch
    float alpha, rs, discount;
    int pad;
};

// two hidden layers of one net on the row-block in X0: X2 = relu(W1 relu(W0 X0 + b0) + b1); ends behind a barrier
__device__ __forceinline__ void eval_hidden(const float *P, const long long *offW, const long long *offB, const float *X0,
                                            int KL0, int K0, float *X1, float *X2) {
    const int wave = threadIdx.x >> 6, c = threadIdx.x & 15;
    WRing<4> r0;
    r0.init(P + sload(&offW[0]), K0, 64 * wave, 16);
    r0.fill(K0 >> 4);
    float bv0[4], bv1[4];
    const float *b0 = P + sload(&offB[0]), *b1 = P + sload(&offB[1]);
#pragma unroll
    for (int t = 0; t < 4; ++t) { bv0[t] = b0[64 * wave + 16 * t + c]; bv1[t] = b1[64 * wave + 16 * t + c]; }
    lds_barrier();                       // X0 is complete; the previous net's readers of X1 / X2 are through
    {
        f32x4 acc[4] = {};
        gemm_ring(r0, X0, KL0, K0 >> 4, acc);
        act_hidden_epilogue<4>(acc, 64 * wave, 16, bv0, X1, H);
    }
    WRing<4> r1;
    r1.init(P + sload(&offW[1]), H, 64 * wave, 16);
    r1.fill(H >> 4);
    lds_barrier();
    {
        f32x4 acc[4] = {};
        gemm_ring(r1, X1, H, H >> 4, acc);
        act_hidden_epilogue<4>(acc, 64 * wave, 16, bv1, X2, H);
    }
    lds_barrier();
}

// the Q output unit (row 0 of the padded last layer: wave 0, one tile, column c == 0) into QL[16]; ends behind a barrier
__device__ __forceinline__ void eval_q_out(const float *P, const long long *offW, const long long *offB, const float *X2,
                                           float *QL) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    if (wave == 0) {
        WRing<1> rq;
        rq.init(P + sload(&offW[2]), H, 0, 16);
        rq.fill(H >> 4);
        const float bq = (P + sload(&offB[2]))[c];
        f32x4 acc[1] = {};
        gemm_ring(rq, X2, H, H >> 4, acc);
        if (c == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) QL[4 * g + i] = acc[0][i] + bq;
        }
    }
    lds_barrier();
}

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

enum { EVAL_Q1, EVAL_Q2, EVAL_Q1_NEW, EVAL_Q2_NEW, EVAL_TQ1, EVAL_TQ2, EVAL_LOG_PI, EVAL_LOG_PI_NEXT, EVAL_Y, EVAL_ROWS_N };

__global__ __launch_bounds__(256) void k_eval(const EvalMember *__restrict__ tab, int n_members) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // this workgroup's member: the last one whose first workgroup is not behind this one (wave-uniform, scalar loads)
    int mi = 0;
    for (int i = 1; i < n_members; ++i)
        if ((int)blockIdx.x >= sload(&tab[i].wg0)) mi = i;
    const EvalMember *M = tab + mi;
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
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int r = threadIdx.x >> 4, a = threadIdx.x & 15, grow = row0 + r;
    float *rows = sload(&M->rows);

    if (chain == 0) {
        {   // [obs | 0 | act | 0] of the row-block; rows beyond n are zero
            const float *obs = sload(&M->obs), *act = sload(&M->act);
            for (int i = threadIdx.x; i < RB * KL0; i += 256) {
                const int rr = i / KL0, k = i - rr * KL0;
                float v = 0.f;
                if (row0 + rr < n) {
                    if (k < O) v = obs[(size_t)(row0 + rr) * O + k];
                    else if (k >= KP && k < KP + A) v = act[(size_t)(row0 + rr) * A + (k - KP)];
                }
                X0[lds_off(rr, k, KL0)] = v;
            }
        }
#pragma unroll 1
        for (int q = 0; q < 2; ++q) {
            const float *P = sload(&M->P[1 + q]);
            eval_hidden(P, M->qW, M->qB, X0, KL0, KQ, X1, X2);
            eval_q_out(P, M->qW, M->qB, X2, QL + RB * q);
        }
        if (a == 0 && grow < n) {
            rows[(size_t)EVAL_Q1 * n + grow] = QL[r];
            rows[(size_t)EVAL_Q2 * n + grow] = QL[RB + r];
        }
        return;
    }

    const bool next = chain == 2;        // (wave-uniform)
    {   // [s or s' | 0] of the row-block: the action columns are written by the head below
        const float *obs = next ? sload(&M->nobs) : sload(&M->obs);
        for (int i = threadIdx.x; i < RB * KL0; i += 256) {
            const int rr = i / KL0, k = i - rr * KL0;
            X0[lds_off(rr, k, KL0)] = (row0 + rr < n && k < O) ? obs[(size_t)(row0 + rr) * O + k] : 0.f;
        }
    }
    const float *PP = sload(&M->P[0]);
    eval_hidden(PP, M->pW, M->pB, X0, KL0, KP, X1, X2);
    if (16 * wave < NH) {                // head rows 16 wave .. 16 wave + 15 (wave-uniform)
        WRing<1> rh;
        rh.init(PP + sload(&M->pW[2]), H, 16 * wave, 16);
        rh.fill(H >> 4);
        const float bh = (PP + sload(&M->pB[2]))[16 * wave + c];
        f32x4 acc[1] = {};
        gemm_ring(rh, X2, H, H >> 4, acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) HL[(4 * g + i) * ACT_HEAD_LD + 16 * wave + c] = acc[0][i] + bh;
    }
    lds_barrier();
    // tanh-Gaussian head: the action as k_act's, log_pi as the step's
    float lp = 0.f, actv = 0.f;
    if (a < A) {
        const size_t o = (size_t)grow * A + a;
        const float mean = HL[r * ACT_HEAD_LD + a];
        float v = mean;
        const float raw = HL[r * ACT_HEAD_LD + A + a];
        const float ls = fminf(fmaxf(raw, LOG_SIG_MIN), LOG_SIG_MAX);
        const float e = grow < n ? (next ? sload(&M->eps_next) : sload(&M->eps))[o] : 0.f;
        v += expf(ls) * e;
        actv = tanhf(v);
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
    X0[lds_off(r, KP + a, KL0)] = actv;  // the whole action chunk (0 beyond A)
    const float lsum = group16_sum(lp);
#pragma unroll 1
    for (int q = 0; q < 2; ++q) {
        const float *P = sload(&M->P[(next ? 3 : 1) + q]);
        eval_hidden(P, M->qW, M->qB, X0, KL0, KQ, X1, X2);
        eval_q_out(P, M->qW, M->qB, X2, QL + RB * q);
    }
    if (a == 0 && grow < n) {
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
}

}  // namespace sac

namespace {

size_t eval_lds_bytes(int KQ) {
    return sizeof(float) * (size_t)RB * (((KQ + 63) & ~63) + 2 * H + ACT_HEAD_LD + 2);
}

}  // namespace

static_assert((int)EVAL_ROWS_N == (int)SAC_EVAL_ROWS_N && (int)EVAL_Y == (int)SAC_EVAL_Y, "k_eval's rows are sac_hip.h's");

// (declared extern "C" in include/sac_hip.h)
int sac_evaluate_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, sac_eval_io_t *io) {
    SAC_REQUIRE(trainers && n_rows && io, "bad arguments to sac_evaluate_many");
    SAC_REQUIRE(n_trainers >= 1 && n_trainers <= SAC_GROUP_MAX, "sac_evaluate_many takes 1..%d trainers (got %d)",
                SAC_GROUP_MAX, n_trainers);
    // every refusal comes first: nothing has changed when one of them returns
    int active = 0;
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        SAC_REQUIRE(t, "trainer %d is null", i);
        for (int j = 0; j < i; ++j) SAC_REQUIRE(trainers[j] != t, "trainer %d is trainer %d again", i, j);
        SAC_REQUIRE(t->device == trainers[0]->device, "trainer %d lives on device %d, trainer 0 on device %d", i, t->device,
                    trainers[0]->device);
        SAC_REQUIRE(t->algo == 0, "trainer %d is a TD3 trainer: this entry evaluates the SAC objective (entropy-regularised "
                    "targets of a tanh-Gaussian policy)", i);
        SAC_REQUIRE(!t->gen, "trainer %d runs the general step (hidden sizes beyond two layers of at most 256 units): device "
                    "evaluation serves the fused kernels' shapes, sac_get_params and a forward on the host is the path for "
                    "this trainer", i);
        SAC_REQUIRE(t->xcd_mask == 0xffu, "trainer %d is confined by sac_trainer_set_xcd[_mask]: device evaluation launches "
                    "on the whole chip", i);
        SAC_REQUIRE(n_rows[i] >= 0 && n_rows[i] <= ACT_MAX_ROWS, "trainer %d: %d rows (0..%d per call, 0 = sits out)", i,
                    (int)n_rows[i], ACT_MAX_ROWS);
        if (n_rows[i] == 0) continue;
        active += 1;
        const sac_eval_io_t &E = io[i];
        SAC_REQUIRE(E.obs && E.act && E.rew && E.term && E.next_obs && E.eps && E.eps_next && E.rows,
                    "trainer %d: a null input array or null rows", i);
    }
    SAC_REQUIRE(active > 0, "no trainer has rows to evaluate");
    sac_trainer *t0 = trainers[0];
    SAC_HIP(hipSetDevice(t0->device));
    // the weights as of the last completed step: drain every member, re-run what a fused step that gave up left undone
    for (int i = 0; i < n_trainers; ++i)
        if (n_rows[i] > 0 && sac_sync(trainers[i])) return -1;
    // the entropy coefficient of this moment (sac_get_scalars' scalars[5]; 1 with automatic tuning off)
    float alpha[SAC_GROUP_MAX];
    for (int i = 0; i < n_trainers; ++i) {
        sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        alpha[i] = 1.0f;
        if (t->cfg.use_automatic_entropy_tuning) {
            Ctl c;
            SAC_HIP(hipMemcpyAsync(&c, t->d_ctl, sizeof(c), hipMemcpyDeviceToHost, t->stream));
            SAC_HIP(hipStreamSynchronize(t->stream));
            // (a trainer that has neither stepped nor been given scalars holds log_alpha and no alpha yet: exp(log_alpha))
            alpha[i] = c.alpha > 0.f ? c.alpha : expf(c.log_alpha);
        }
    }

    // per member: obs act rew term nobs eps eps_next | rows mu log_std a_new a_next
    enum { NPART = 12 };
    size_t off[SAC_GROUP_MAX][NPART], bytes = (sizeof(EvalMember) * SAC_GROUP_MAX + 255) & ~(size_t)255;
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        const size_t n = (size_t)n_rows[i], nO = n * t->O, nA = n * t->A;
        const sac_eval_io_t &E = io[i];
        const size_t part[NPART] = {nO, nA, n, n, nO, nA, nA, n * SAC_EVAL_ROWS_N,
                                    n && E.mu ? nA : 0, n && E.log_std ? nA : 0, n && E.a_new ? nA : 0, n && E.a_next ? nA : 0};
        for (int k = 0; k < NPART; ++k) { off[i][k] = bytes; bytes += (sizeof(float) * part[k] + 255) & ~(size_t)255; }
    }
    if (act_stage_reserve(t0, bytes)) return -1;
    const sac_trainer::ActStage &S = t0->act_stage;
    EvalMember *tab = reinterpret_cast<EvalMember *>(S.h);
    int wgs = 0, m = 0, kq_max = 0;
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        const sac_eval_io_t &E = io[i];
        const size_t n = (size_t)n_rows[i], nO = n * t->O, nA = n * t->A;
        EvalMember &M = tab[m++];
        for (int k = 0; k < 5; ++k) M.P[k] = t->net[SAC_NET_POLICY + k].P;
        auto in = [&](int k, const float *src, size_t count) {
            memcpy(S.h + off[i][k], src, sizeof(float) * count);
            return reinterpret_cast<const float *>(S.d + off[i][k]);
        };
        M.obs = in(0, E.obs, nO); M.act = in(1, E.act, nA); M.rew = in(2, E.rew, n); M.term = in(3, E.term, n);
        M.nobs = in(4, E.next_obs, nO); M.eps = in(5, E.eps, nA); M.eps_next = in(6, E.eps_next, nA);
        auto out = [&](int k, const float *asked) { return asked ? reinterpret_cast<float *>(S.d + off[i][k]) : nullptr; };
        M.rows = out(7, E.rows); M.mu = out(8, E.mu); M.log_std = out(9, E.log_std);
        M.a_new = out(10, E.a_new); M.a_next = out(11, E.a_next);
        const Net &NP = t->net[SAC_NET_POLICY], &NQ = t->net[SAC_NET_QF1];
        for (int l = 0; l < 3; ++l) {
            M.pW[l] = NP.L[l].offW; M.pB[l] = NP.L[l].offB;
            M.qW[l] = NQ.L[l].offW; M.qB[l] = NQ.L[l].offB;
        }
        M.O = t->O; M.A = t->A; M.KP = t->KP; M.NH = t->NH;
        M.n = n_rows[i]; M.wg0 = wgs;
        M.alpha = alpha[i]; M.rs = t->cfg.reward_scale; M.discount = t->cfg.discount; M.pad = 0;
        wgs += 3 * ((n_rows[i] + RB - 1) / RB);
        kq_max = std::max(kq_max, t->KQ);
    }
    const size_t lds = eval_lds_bytes(kq_max);
    if (lds > 48 * 1024 && !t0->eval_lds_raised) {
        SAC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_eval), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)eval_lds_bytes(512)));
        t0->eval_lds_raised = true;
    }
    hipLaunchKernelGGL(k_eval, dim3(wgs), dim3(256), lds, t0->stream, reinterpret_cast<const EvalMember *>(S.d), m);
    SAC_HIP(hipGetLastError());
    if (wait_trainer_stream(t0)) return -1;
    for (int i = 0; i < n_trainers; ++i) {
        if (n_rows[i] == 0) continue;
        sac_eval_io_t &E = io[i];
        const size_t n = (size_t)n_rows[i], nA = n * trainers[i]->A;
        memcpy(E.rows, S.h + off[i][7], sizeof(float) * n * SAC_EVAL_ROWS_N);
        float *const dst[4] = {E.mu, E.log_std, E.a_new, E.a_next};
        for (int k = 0; k < 4; ++k)
            if (dst[k]) memcpy(dst[k], S.h + off[i][8 + k], sizeof(float) * nA);
        E.alpha = alpha[i];
    }
    return 0;
}

int sac_evaluate(sac_trainer_t *t, int64_t n, sac_eval_io_t *io) {
    SAC_REQUIRE(t && io, "bad arguments to sac_evaluate");
    SAC_REQUIRE(n >= 1 && n <= ACT_MAX_ROWS, "sac_evaluate: %lld rows (1..%d per call)", (long long)n, ACT_MAX_ROWS);
    const int32_t rows = (int32_t)n;
    return sac_evaluate_many(&t, 1, &rows, io);
}
