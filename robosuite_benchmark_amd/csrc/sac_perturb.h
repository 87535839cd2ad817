// Whole-network reset and shrink-and-perturb on the device (Nikishin et al. 2022; Ash & Adams 2020): k_param_perturb and
// sac_shrink_perturb[_many] (included by sac_trainer.hip behind sac_recycle.h) -- the whole-tensor WRITER next to
// k_unit_recycle, the per-unit one.  Every element of a selected trained net becomes
//
//     x' = shrink * x + perturb * f        (each product and the sum rounded once, no FMA; a term whose factor is 0 is
//                                           not formed, so with shrink == 0 the old value -- a NaN too -- is not read)
//
// with f the element's fresh value (sac_perturb_map.h: drawn on the device, a function of (seed, draw, net, tensor,
// element) alone).  With SAC_PERTURB_OPT Adam's m and v of every element become +0.0; with SAC_PERTURB_TARGETS the paired
// target (param_target_of) receives the same bits.  Where each element lives -- both weight copies of the fused kernels'
// shapes, the moments in MT / VT or M / V -- is param_addr's business: nothing about a layout is restated here.
//
//   table   PerturbJob in device-visible staging, read with scalar loads: one job per TENSOR of a selected net of a member;
//           a workgroup finds its job by bisection over wg0
//   grid    one workgroup (256 lanes) per CHUNK of PM_CH = 16384 consecutive flat elements of one job; lane l takes the
//           quads e = 4 (c 4096 + l + 256 i) .. + 3, i < 16, up to E: one Philox evaluation per quad
//   stores  plain vector stores: the forward copy, the transposed copy of a PA_FRAG weight by the same lane, the two
//           moment words, the target's copies.  No atomics, nothing shared between workgroups, no two lanes write one
//           address (param_addr is one-to-one on a tensor, and tensors do not overlap)
// An element's new value does not depend on the grid, the job's place in the table or its neighbours: grouped == solo.
// The kernel boundary makes every copy visible to whatever the stream (or, behind the entry's wait, any stream) launches
// next.  infer.shrink_perturb_reference restates the rule in NumPy.
#pragma once
#include "sac_perturb_map.h"

namespace sac {

struct PerturbJob {
    float *X, *XT;                 // the net's parameters: forward image, transposed image (fused) or null
    float *M, *V;                  // Adam moments or null: a fused weight's in the transposed copies (mt), else as X
    float *T, *TT;                 // the paired target's images or null (TT: null where the target keeps no second copy)
    ParamAddr a;
    long long E;
    unsigned long long seed, draw;
    float shrink, perturb;
    PerturbRule rule;
    int net, tensor;               // the counter's k and j
    int wg0, mt;                   // wg0: first workgroup (= first chunk) of this job in the launch
};

__global__ __launch_bounds__(PM_LANES) void k_param_perturb(const PerturbJob *__restrict__ tab, int n_jobs) {
#pragma clang fp contract(off)
    int lo = 0, hi = n_jobs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int)blockIdx.x >= sload(&tab[mid].wg0)) lo = mid; else hi = mid;
    }
    const PerturbJob *J = tab + lo;
    float *X = sload(&J->X), *XT = sload(&J->XT), *M = sload(&J->M), *V = sload(&J->V), *T = sload(&J->T), *TT = sload(&J->TT);
    ParamAddr a;
    a.off = sload(&J->a.off); a.offT = sload(&J->a.offT);
    a.kind = sload(&J->a.kind); a.K = sload(&J->a.K); a.O = sload(&J->a.O); a.KP = sload(&J->a.KP);
    a.nshift = sload(&J->a.nshift); a.ld = sload(&J->a.ld); a.ldT = sload(&J->a.ldT); a.pad_ = 0;
    const long long E = sload(&J->E);
    const unsigned long long seed = sload(&J->seed), draw = sload(&J->draw);
    const float shrink = sload(&J->shrink), perturb = sload(&J->perturb);
    PerturbRule rule;
    rule.scale = sload(&J->rule.scale); rule.draws = sload(&J->rule.draws);
    const int net = sload(&J->net), tensor = sload(&J->tensor);
    const bool mt = sload(&J->mt) != 0, frag = a.kind == PA_FRAG;
    const int c = (int)blockIdx.x - sload(&J->wg0);
    const long long q0 = (long long)c * (PM_CH / 4), q1 = (E + 3) >> 2;
    for (int i = 0; i < PM_CH / 4 / PM_LANES; ++i) {
        const long long q = q0 + threadIdx.x + (long long)i * PM_LANES;
        if (q >= q1) break;
        PhiloxWords w = PhiloxWords{{0u, 0u, 0u, 0u}};
        if (rule.draws && perturb != 0.f) w = perturb_words(seed, draw, net, tensor, q);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long e = 4 * q + r;
            if (e >= E) break;
            const long long fwd = param_addr(a, e, false), tr = frag ? param_addr(a, e, true) : fwd;
            // (plain operators under this kernel's `fp contract(off)`: __fmul_rn / __fadd_rn are inline x * y / x + y that
            // carry their header's contraction flags into the caller, and the pair would meet in one v_fma_f32)
            float y;
            if (perturb != 0.f) {
                y = perturb * perturb_fresh(rule, w.w[r]);
                if (shrink != 0.f) { const float sx = shrink * ld1g(X + fwd); y = sx + y; }
            } else {
                y = shrink * ld1g(X + fwd);
            }
            X[fwd] = y;
            if (frag) XT[tr] = y;
            if (M) {
                const long long mom = mt ? tr : fwd;
                M[mom] = 0.f;
                V[mom] = 0.f;
            }
            if (T) {
                T[fwd] = y;
                if (frag && TT) TT[tr] = y;
            }
        }
    }
}

}  // namespace sac

// (declared extern "C" in include/sac_hip.h)
int sac_shrink_perturb_many(sac_trainer_t *const *trainers, int n_trainers, const sac_perturb_io_t *io) {
    SAC_REQUIRE(trainers && io, "bad arguments to sac_shrink_perturb_many");
    const InferEntry E = {"sac_shrink_perturb_many", false, false, "device shrink-and-perturb", "", "perturb", true};
    int32_t ones[SAC_GROUP_MAX];
    for (int i = 0; i < SAC_GROUP_MAX; ++i) ones[i] = 1;
    const int rc = infer_admit(E, trainers, n_trainers, ones, [&](int i) {
        const sac_perturb_io_t &p = io[i];
        SAC_REQUIRE(!(p.nets & ~0x3fu), "trainer %d: nets 0x%x has an unknown bit (bit k selects SAC_NET_* == k)", i, (unsigned)p.nets);
        SAC_REQUIRE(!(p.nets & 0x38u), "trainer %d: nets 0x%x selects a target net: a target is written through its trained "
                    "net with SAC_PERTURB_TARGETS; bits 0..2 select policy, qf1, qf2", i, (unsigned)p.nets);
        SAC_REQUIRE(p.nets != 0, "trainer %d: nets 0x0 selects no network (bit k selects SAC_NET_* == k, k in 0..2)", i);
        SAC_REQUIRE(!(p.flags & ~(uint32_t)(SAC_PERTURB_OPT | SAC_PERTURB_TARGETS)), "trainer %d: unknown flags 0x%x", i,
                    (unsigned)p.flags);
        SAC_REQUIRE(std::isfinite(p.shrink) && std::isfinite(p.perturb) && p.shrink >= 0.f && p.perturb >= 0.f,
                    "trainer %d: shrink %g and perturb %g must be finite and not negative", i, (double)p.shrink, (double)p.perturb);
        SAC_REQUIRE(p.shrink != 0.f || p.perturb != 0.f, "trainer %d: shrink and perturb are both zero", i);
        for (int k = 0; k < 3; ++k) {
            if (!(p.nets >> k & 1u)) continue;
            SAC_REQUIRE(std::isfinite(p.init_w[k]) && p.init_w[k] >= 0.f, "trainer %d: net %d: init_w %g must be finite and "
                        "not negative", i, k, (double)p.init_w[k]);
            SAC_REQUIRE(std::isfinite(p.b_init[k]), "trainer %d: net %d: b_init %g must be finite", i, k, (double)p.b_init[k]);
        }
        return 0;
    });
    if (rc) return rc;
    for (int i = 0; i < n_trainers; ++i)
        if (settle_trainer(trainers[i])) return -1;          // (as the setters: unverified fused steps first)
    sac_trainer *t0 = trainers[0];
    ParamTensor T[PARAM_MAX_TENSORS];
    size_t jobs = 0, chunks = 0;
    for (int i = 0; i < n_trainers; ++i)
        for (int k = 0; k < 3; ++k) {
            if (!(io[i].nets >> k & 1u)) continue;
            const int n = param_tensor_list(trainers[i]->shape, k, T);
            for (int j = 0; j < n; ++j) chunks += (size_t)((T[j].E + PM_CH - 1) / PM_CH);
            jobs += (size_t)n;
        }
    SAC_REQUIRE(chunks < ((size_t)1 << 30), "internal: %zu chunks in one call", chunks);
    if (act_stage_reserve(t0, infer_align(sizeof(PerturbJob) * jobs))) return -1;      // the staging holds the job table alone
    const sac_trainer::ActStage &S = t0->act_stage;
    PerturbJob *tab = reinterpret_cast<PerturbJob *>(S.h);
    int nj = 0, wgs = 0;
    for (int i = 0; i < n_trainers; ++i) {
        sac_trainer *t = trainers[i];
        t->mirror_valid = false;
        const sac_perturb_io_t &p = io[i];
        for (int k = 0; k < 3; ++k) {
            if (!(p.nets >> k & 1u)) continue;
            const int n = param_tensor_list(t->shape, k, T);
            const int tk = (p.flags & SAC_PERTURB_TARGETS) ? param_target_of(t, k) : -1;
            const NetArrays N = net_arrays(t, k);
            for (int j = 0; j < n; ++j) {
                PerturbJob &J = tab[nj];
                J = PerturbJob{};
                J.a = T[j].a; J.E = T[j].E;
                J.X = N.P; J.XT = N.PT;
                J.mt = T[j].a.kind == PA_FRAG ? 1 : 0;
                if (p.flags & SAC_PERTURB_OPT) { J.M = J.mt ? N.MT : N.M; J.V = J.mt ? N.VT : N.V; }
                if (tk >= 0) { const NetArrays G = net_arrays(t, tk); J.T = G.P; J.TT = G.PT; }
                J.seed = p.seed; J.draw = p.draw;
                J.shrink = p.shrink; J.perturb = p.perturb;
                J.rule = perturb_rule(t->shape, k, j, p.init_w[k], p.b_init[k]);
                J.net = k; J.tensor = j;
                J.wg0 = wgs;
                wgs += (int)((J.E + PM_CH - 1) / PM_CH);
                nj += 1;
            }
        }
    }
    hipLaunchKernelGGL(sac::k_param_perturb, dim3(wgs), dim3(PM_LANES), 0, t0->stream, reinterpret_cast<const PerturbJob *>(S.d), nj);
    SAC_HIP(hipGetLastError());
    return wait_trainer_stream(t0);
}

int sac_shrink_perturb(sac_trainer_t *t, const sac_perturb_io_t *io) {
    SAC_REQUIRE(t && io, "bad arguments to sac_shrink_perturb");
    return sac_shrink_perturb_many(&t, 1, io);
}
