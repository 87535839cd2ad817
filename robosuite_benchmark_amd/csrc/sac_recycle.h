// Recycling hidden units on the device (ReDo, Sokar et al. 2023): k_unit_recycle and sac_recycle_units[_many] (included by
// sac_trainer.hip behind sac_params.h) -- the WRITER that goes with k_param_moments, the reader.  A listed unit of a
// hidden layer of a trained net gets the caller's fresh incoming row and bias, +0.0 on its outgoing column(s) and, with
// SAC_RECYCLE_OPT, +0.0 in Adam's m and v of every element written.  Which elements those are and where each lives --
// both weight copies of the fused kernels' shapes, the moments in MT / VT or M / V, the action-column gap, the merged SAC
// head -- is sac_recycle_map.h's business, which rests on param_addr: nothing about a layout is restated here.
//
//   table   RecycleJob in device-visible staging, read with scalar loads: one job per (member, net, hidden layer) with
//           units listed, all of ONE phase; a workgroup finds its job by bisection over wg0
//   grid    one workgroup (256 lanes) per listed unit; the lanes stride over a span's elements -- the K_l of the unit's
//           incoming row (and its bias), or the N_{l+1} of an outgoing column
//   stores  plain vector stores: the forward copy, the transposed copy of a PA_FRAG weight by the same lane, the two
//           moment words.  No atomics, nothing shared between workgroups: within a phase no two jobs write one address
//   phases  two launches on one stream, RC_INCOMING first: where a fresh row crosses a zeroed column the zero is the
//           later store.  The kernel boundary also makes both copies visible to whatever the stream (or, behind the
//           entry's wait, any stream) launches next.
// Unit lists and fresh rows sit behind the table in the same staging.  infer.recycle_reference restates the rule in NumPy.
#pragma once
#include "sac_recycle_map.h"

namespace sac {

constexpr int RC_LANES = 256;

struct RecycleJob {
    float *X, *XT;                 // the net's parameters: forward image, transposed image (fused) or null
    float *M, *V, *MT, *VT;        // Adam moments, all null without SAC_RECYCLE_OPT (MT / VT null for a general net)
    const int *units;              // the listed units, ascending
    const float *fresh;            // per listed unit fanin + 1 floats (RC_INCOMING; unused by RC_OUTGOING)
    RecycleSpan s[RC_MAX_SPANS];
    int n_spans, n_units, wg0, fstride;      // wg0: first workgroup (= first unit) of this job in the launch
};

__global__ __launch_bounds__(RC_LANES) void k_unit_recycle(const RecycleJob *__restrict__ tab, int n_jobs) {
    int lo = 0, hi = n_jobs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int)blockIdx.x >= sload(&tab[mid].wg0)) lo = mid; else hi = mid;
    }
    const RecycleJob *J = tab + lo;
    const int j = (int)blockIdx.x - sload(&J->wg0);
    if (j >= sload(&J->n_units)) return;
    float *X = sload(&J->X), *XT = sload(&J->XT), *M = sload(&J->M), *V = sload(&J->V), *MT = sload(&J->MT), *VT = sload(&J->VT);
    const int u = sload(sload(&J->units) + j);
    const float *fresh = sload(&J->fresh) + (size_t)j * sload(&J->fstride);
    const int ns = sload(&J->n_spans);
    for (int k = 0; k < ns; ++k) {
        RecycleSpan s;
        s.a.off = sload(&J->s[k].a.off); s.a.offT = sload(&J->s[k].a.offT);
        s.a.kind = sload(&J->s[k].a.kind); s.a.K = sload(&J->s[k].a.K); s.a.O = sload(&J->s[k].a.O);
        s.a.KP = sload(&J->s[k].a.KP); s.a.nshift = sload(&J->s[k].a.nshift); s.a.ld = sload(&J->s[k].a.ld);
        s.a.ldT = sload(&J->s[k].a.ldT); s.a.pad_ = 0;
        s.flat0 = 0; s.mul = sload(&J->s[k].mul); s.stride = sload(&J->s[k].stride);
        s.count = sload(&J->s[k].count); s.src0 = sload(&J->s[k].src0);
        for (int i = threadIdx.x; i < s.count; i += RC_LANES) {
            const RecycleElem x = recycle_elem(s, u, i);
            const float val = s.src0 >= 0 ? ld1g(fresh + s.src0 + i) : 0.f;
            X[x.fwd] = val;
            if (x.mt) XT[x.tr] = val;
            if (M) {
                float *m = x.mt ? MT : M, *v = x.mt ? VT : V;
                m[x.mom] = 0.f;
                v[x.mom] = 0.f;
            }
        }
    }
}

}  // namespace sac

namespace {

// a trainer's hidden-layer count of net k
int recycle_nh(const sac_trainer *t, int k) { return recycle_layers(t->shape, k); }

}  // namespace

// (declared extern "C" in include/sac_hip.h)
int sac_recycle_units_many(sac_trainer_t *const *trainers, int n_trainers, const sac_recycle_io_t *io) {
    SAC_REQUIRE(trainers && io, "bad arguments to sac_recycle_units_many");
    const InferEntry E = {"sac_recycle_units_many", false, false, "device unit recycling", "", "recycle", true};
    int32_t ones[SAC_GROUP_MAX];
    for (int i = 0; i < SAC_GROUP_MAX; ++i) ones[i] = 1;
    size_t total_units = 0, total_fresh = 0, n_jobs = 0;
    const int rc = infer_admit(E, trainers, n_trainers, ones, [&](int i) {
        const sac_trainer *t = trainers[i];
        const uint32_t nets = io[i].nets;
        SAC_REQUIRE(!(nets & ~0x3fu), "trainer %d: nets 0x%x has an unknown bit (bit k selects SAC_NET_* == k)", i, (unsigned)nets);
        SAC_REQUIRE(!(nets & 0x38u), "trainer %d: nets 0x%x selects a target net: target nets are not recycled (the Polyak "
                    "average carries the change over); bits 0..2 select policy, qf1, qf2", i, (unsigned)nets);
        SAC_REQUIRE(nets != 0, "trainer %d: nets 0x0 selects no network (bit k selects SAC_NET_* == k, k in 0..2)", i);
        SAC_REQUIRE(!(io[i].flags & ~(uint32_t)SAC_RECYCLE_OPT), "trainer %d: unknown flags 0x%x", i, (unsigned)io[i].flags);
        SAC_REQUIRE(io[i].counts, "trainer %d: null counts", i);
        size_t c = 0, units = 0, fresh = 0;
        for (int k = 0; k < 3; ++k) {
            if (!(nets >> k & 1u)) continue;
            for (int l = 0; l < recycle_nh(t, k); ++l, ++c) {
                const int n = io[i].counts[c], N = recycle_width(t->shape, k, l);
                SAC_REQUIRE(n >= 0 && n <= N, "trainer %d: net %d, hidden layer %d: %d units listed (0..%d)", i, k, l, n, N);
                SAC_REQUIRE(n == 0 || (io[i].units && io[i].fresh), "trainer %d: null units or fresh with units listed", i);
                for (int j = 0; j < n; ++j) {
                    const int u = io[i].units[units + j];
                    SAC_REQUIRE(u >= 0 && u < N, "trainer %d: net %d, hidden layer %d: unit %d is outside the layer's true "
                                "width %d (pads are not units)", i, k, l, u, N);
                    SAC_REQUIRE(j == 0 || u > io[i].units[units + j - 1], "trainer %d: net %d, hidden layer %d: the unit "
                                "list is not strictly ascending at position %d", i, k, l, j);
                }
                units += (size_t)n;
                fresh += (size_t)n * (size_t)(recycle_fanin(t->shape, k, l) + 1);
                n_jobs += n ? 1 : 0;
            }
        }
        total_units += units; total_fresh += fresh;
        return 0;
    });
    if (rc) return rc;
    if (total_units == 0) return 0;
    SAC_REQUIRE(total_units < ((size_t)1 << 30), "internal: %zu units in one call", total_units);
    for (int i = 0; i < n_trainers; ++i)
        if (settle_trainer(trainers[i])) return -1;          // (as the setters: unverified fused steps first)
    sac_trainer *t0 = trainers[0];
    // staging: the job tables of the two phases, the unit lists, the fresh rows
    const size_t off_units = infer_align(sizeof(RecycleJob) * n_jobs * RC_PHASES);
    const size_t off_fresh = off_units + infer_align(sizeof(int32_t) * total_units);
    const size_t bytes = off_fresh + infer_align(sizeof(float) * total_fresh);
    if (act_stage_reserve(t0, bytes)) return -1;
    const sac_trainer::ActStage &S = t0->act_stage;
    RecycleJob *tab = reinterpret_cast<RecycleJob *>(S.h);
    int32_t *h_units = reinterpret_cast<int32_t *>(S.h + off_units);
    float *h_fresh = reinterpret_cast<float *>(S.h + off_fresh);
    const int32_t *d_units = reinterpret_cast<const int32_t *>(S.d + off_units);
    const float *d_fresh = reinterpret_cast<const float *>(S.d + off_fresh);
    size_t nj = 0, at_u = 0, at_f = 0;
    int wgs = 0;
    for (int i = 0; i < n_trainers; ++i) {
        sac_trainer *t = trainers[i];
        t->mirror_valid = false;
        const bool opt = io[i].flags & SAC_RECYCLE_OPT;
        size_t c = 0, units = 0, fresh = 0;
        for (int k = 0; k < 3; ++k) {
            if (!(io[i].nets >> k & 1u)) continue;
            const NetArrays N = net_arrays(t, k);
            for (int l = 0; l < recycle_nh(t, k); ++l, ++c) {
                const int n = io[i].counts[c];
                if (n == 0) continue;
                const int row = recycle_fanin(t->shape, k, l) + 1;
                memcpy(h_units + at_u, io[i].units + units, sizeof(int32_t) * (size_t)n);
                memcpy(h_fresh + at_f, io[i].fresh + fresh, sizeof(float) * (size_t)n * row);
                for (int ph = 0; ph < RC_PHASES; ++ph) {
                    RecycleSpans R;
                    SAC_REQUIRE(recycle_spans(t->shape, k, l, ph, &R) == 0, "internal: no hidden layer %d in net %d", l, k);
                    RecycleJob &J = tab[(size_t)ph * n_jobs + nj];
                    J = RecycleJob{};
                    J.X = N.P; J.XT = N.PT;
                    if (opt) { J.M = N.M; J.V = N.V; J.MT = N.MT; J.VT = N.VT; }
                    J.units = d_units + at_u; J.fresh = d_fresh + at_f;
                    for (int s = 0; s < R.n; ++s) J.s[s] = R.s[s];
                    J.n_spans = R.n; J.n_units = n; J.wg0 = wgs; J.fstride = row;
                }
                wgs += n; nj += 1;
                at_u += (size_t)n; at_f += (size_t)n * row;
                units += (size_t)n; fresh += (size_t)n * row;
            }
        }
    }
    const RecycleJob *d_tab = reinterpret_cast<const RecycleJob *>(S.d);
    for (int ph = 0; ph < RC_PHASES; ++ph) {
        hipLaunchKernelGGL(sac::k_unit_recycle, dim3(wgs), dim3(RC_LANES), 0, t0->stream, d_tab + (size_t)ph * n_jobs, (int)n_jobs);
        SAC_HIP(hipGetLastError());
    }
    return wait_trainer_stream(t0);
}

int sac_recycle_units(sac_trainer_t *t, const sac_recycle_io_t *io) {
    SAC_REQUIRE(t && io, "bad arguments to sac_recycle_units");
    return sac_recycle_units_many(&t, 1, io);
}
