// Per-tensor statistics of the state the step kernels write -- parameters, Adam moments, Polyak targets -- reduced on
// the device where that state lives: k_param_moments, k_param_finish and sac_param_moments[_many] (included by
// sac_trainer.hip behind sac_units_general.h).  No forward pass is involved, so ONE entry serves the fused kernels'
// shapes and the general step, SAC and TD3, mixed in one launch.
//
// A job is one TENSOR of the flat nn.Linear layout of sac_get_params: fc<i>.weight, fc<i>.bias, ..., last_fc.weight,
// last_fc.bias and, on a SAC policy, last_fc_log_std.weight, last_fc_log_std.bias (two tensors of their own, although the
// device keeps both heads in one layer).  Its E elements are taken in flat order e = 0 .. E - 1; where element e lives
// is param_addr's business (sac_param_map.h: the tensor list and the address rule the getters use, PA_FLAT or PA_FRAG).
//
// Pads are never an element, so they cannot enter a sum.  The record is SAC_PARAM_FIELDS_N float64 per tensor, every
// value formed in float64 from the float32 words with add, multiply, compare and fabs only (the product of two float32
// values is exact in float64; the gap's square is rounded once: no contraction into an FMA, `fp contract(off)`):
//
//   SAC_PARAM_SUM, SUMSQ         sum x, sum x x over the parameters
//   SAC_PARAM_ABSMAX             the largest |x|; a NaN stays (em_max)
//   SAC_PARAM_NONFINITE          the number of elements that are not finite
//   SAC_PARAM_M_SUMSQ, M_ABSMAX  the same over Adam's first moment
//   SAC_PARAM_V_SUM, V_MAX       the sum and the largest value of Adam's second moment
//   SAC_PARAM_GAP_SUMSQ          sum (x - x_target)^2, the difference taken in float64
//
// A field that does not apply (no moments: a target net or SAC_PARAMS_OPT not set; no target: a SAC policy, a target net
// or SAC_PARAMS_GAP not set) is exactly 0.0.
//
//   table   ParamJob in device-visible staging, read with scalar loads; a workgroup finds its job by bisection over wg0
//   grid    one workgroup (256 lanes) per CHUNK of PM_CH = 16384 consecutive elements of one job
//   order   lane l adds e = c PM_CH + l, + 256, ... ascending from 0.0 (V_MAX from -inf); the 256 partials meet in LDS by
//           halving, p[l] (+)= p[l + 128], 64, ..., 1 (the max fields with em_max); the chunk's nine values go to the
//           scratch; k_param_finish, one lane per (tensor, field), joins the chunks in ascending c, left to right.  The
//           order of every sum is a function of E ALONE: not of the grid, the job's place in the table, its neighbours,
//           the mask, the flags or the family.  No atomics, vector stores only.
//   reads   general tensors are contiguous (consecutive lanes, consecutive floats); a fused tensor is read through
//           frag_off in flat order -- not line-friendly, but the largest is 256 x 512 -- the sum is not reordered to suit
//
// The kernels read the nets and write scratch and records in the staging: nothing the step reads.
// infer.param_moments_reference restates the order in NumPy float64.
#pragma once

namespace sac {

constexpr int PM_CH = 16384;              // elements of one chunk (one workgroup)
constexpr int PM_LANES = 256;

struct ParamJob {
    const float *X, *T;            // the net's parameters; its target's (same layout) or null
    const float *M, *V;            // Adam moments or null: a fused weight's in the transposed copies (mt), else as X
    ParamAddr a;
    long long E;
    double *part, *out;            // [nch][SAC_PARAM_FIELDS_N] chunk partials; the record
    int wg0, nch, mt, pad_;        // wg0: first workgroup (= first chunk) of this job in the launch
};

__device__ __forceinline__ constexpr bool pm_is_max(int f) {
    return f == SAC_PARAM_ABSMAX || f == SAC_PARAM_M_ABSMAX || f == SAC_PARAM_V_MAX;
}

__global__ __launch_bounds__(PM_LANES) void k_param_moments(const ParamJob *__restrict__ tab, int n_jobs) {
#pragma clang fp contract(off)
    __shared__ double L[SAC_PARAM_FIELDS_N][PM_LANES];
    int lo = 0, hi = n_jobs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int)blockIdx.x >= sload(&tab[mid].wg0)) lo = mid; else hi = mid;
    }
    const ParamJob *J = tab + lo;
    const float *X = sload(&J->X), *T = sload(&J->T), *M = sload(&J->M), *V = sload(&J->V);
    ParamAddr a;
    a.off = sload(&J->a.off); a.offT = sload(&J->a.offT);
    a.kind = sload(&J->a.kind); a.K = sload(&J->a.K); a.O = sload(&J->a.O); a.KP = sload(&J->a.KP);
    a.nshift = sload(&J->a.nshift); a.ld = sload(&J->a.ld); a.ldT = sload(&J->a.ldT); a.pad_ = 0;
    const bool mt = sload(&J->mt) != 0;
    const long long E = sload(&J->E);
    const int c = (int)blockIdx.x - sload(&J->wg0), t = threadIdx.x;
    const long long e0 = (long long)c * PM_CH, e1 = e0 + PM_CH < E ? e0 + PM_CH : E;
    double p[SAC_PARAM_FIELDS_N];
#pragma unroll
    for (int f = 0; f < SAC_PARAM_FIELDS_N; ++f) p[f] = 0.0;
    p[SAC_PARAM_V_MAX] = -__builtin_huge_val();
    for (long long e = e0 + t; e < e1; e += PM_LANES) {
        const long long i = param_addr(a, e, false);
        const double x = (double)ld1g(X + i), ax = fabs(x);
        p[SAC_PARAM_SUM] = p[SAC_PARAM_SUM] + x;
        p[SAC_PARAM_SUMSQ] = p[SAC_PARAM_SUMSQ] + x * x;
        p[SAC_PARAM_ABSMAX] = em_max(p[SAC_PARAM_ABSMAX], ax);
        p[SAC_PARAM_NONFINITE] = p[SAC_PARAM_NONFINITE] + (ax <= 3.4028234663852886e38 ? 0.0 : 1.0);
        if (M) {
            const long long j = mt ? param_addr(a, e, true) : i;
            const double m = (double)ld1g(M + j), v = (double)ld1g(V + j);
            p[SAC_PARAM_M_SUMSQ] = p[SAC_PARAM_M_SUMSQ] + m * m;
            p[SAC_PARAM_M_ABSMAX] = em_max(p[SAC_PARAM_M_ABSMAX], fabs(m));
            p[SAC_PARAM_V_SUM] = p[SAC_PARAM_V_SUM] + v;
            p[SAC_PARAM_V_MAX] = em_max(p[SAC_PARAM_V_MAX], v);
        }
        if (T) {
            const double d = x - (double)ld1g(T + i);
            const double dd = d * d;
            p[SAC_PARAM_GAP_SUMSQ] = p[SAC_PARAM_GAP_SUMSQ] + dd;
        }
    }
#pragma unroll
    for (int f = 0; f < SAC_PARAM_FIELDS_N; ++f) L[f][t] = p[f];
    __syncthreads();
#pragma unroll 1
    for (int s = PM_LANES / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int f = 0; f < SAC_PARAM_FIELDS_N; ++f)
                L[f][t] = pm_is_max(f) ? em_max(L[f][t], L[f][t + s]) : L[f][t] + L[f][t + s];
        }
        __syncthreads();
    }
    if (t < SAC_PARAM_FIELDS_N) sload(&J->part)[(size_t)c * SAC_PARAM_FIELDS_N + t] = L[t][0];
}

// one lane per (tensor, field): the chunks in ascending c, left to right; a field that does not apply is 0.0
__global__ __launch_bounds__(PM_LANES) void k_param_finish(const ParamJob *__restrict__ tab, int n_jobs) {
    const int id = (int)blockIdx.x * PM_LANES + (int)threadIdx.x;
    if (id >= n_jobs * SAC_PARAM_FIELDS_N) return;
    const int j = id / SAC_PARAM_FIELDS_N, f = id - j * SAC_PARAM_FIELDS_N;
    const ParamJob *J = tab + j;
    const double *part = J->part;
    const int nch = J->nch;
    double acc = part[f];
    for (int c = 1; c < nch; ++c) {
        const double x = part[(size_t)c * SAC_PARAM_FIELDS_N + f];
        acc = pm_is_max(f) ? em_max(acc, x) : acc + x;
    }
    const bool opt_field = f >= SAC_PARAM_M_SUMSQ && f <= SAC_PARAM_V_MAX;
    if ((opt_field && !J->M) || (f == SAC_PARAM_GAP_SUMSQ && !J->T)) acc = 0.0;
    J->out[f] = acc;
}

}  // namespace sac

namespace {

constexpr int PARAM_NETS = 6;

// the target a trained net is paired with, or -1
int param_target_of(const sac_trainer *t, int net) {
    if (net == SAC_NET_QF1 || net == SAC_NET_QF2) return net + 2;
    if (net == SAC_NET_POLICY && t->algo == 1) return SAC_NET_TARGET_POLICY;
    return -1;
}

}  // namespace

// (declared extern "C" in include/sac_hip.h)
int sac_param_tensors(const sac_trainer_t *t, int net, int64_t *sizes) {
    SAC_REQUIRE(t && net >= 0 && net <= (t->algo == 1 ? 5 : 4), "bad arguments to sac_param_tensors");
    ParamTensor T[PARAM_MAX_TENSORS];
    const int n = param_tensor_list(t->shape, net, T);
    if (sizes) for (int i = 0; i < n; ++i) sizes[i] = T[i].E;
    return n;
}

int sac_param_moments_many(sac_trainer_t *const *trainers, int n_trainers, sac_params_io_t *io) {
    SAC_REQUIRE(trainers && io, "bad arguments to sac_param_moments_many");
    const InferEntry E = {"sac_param_moments_many", false, false, "device parameter statistics", "", "reduce", true};
    int32_t ones[SAC_GROUP_MAX];
    for (int i = 0; i < SAC_GROUP_MAX; ++i) ones[i] = 1;
    const int rc = infer_admit(E, trainers, n_trainers, ones, [&](int i) {
        const uint32_t nets = io[i].nets;
        SAC_REQUIRE(nets != 0 && nets < (1u << PARAM_NETS), "trainer %d: nets 0x%x selects no network or an unknown one (bit k "
                    "selects SAC_NET_* == k)", i, (unsigned)nets);
        SAC_REQUIRE(!(nets >> SAC_NET_TARGET_POLICY & 1u) || trainers[i]->algo == 1, "trainer %d: nets 0x%x selects the target "
                    "policy, which only a TD3 trainer has", i, (unsigned)nets);
        SAC_REQUIRE(!(io[i].flags & ~(uint32_t)(SAC_PARAMS_OPT | SAC_PARAMS_GAP)), "trainer %d: unknown flags 0x%x", i,
                    (unsigned)io[i].flags);
        SAC_REQUIRE(io[i].moments, "trainer %d: null moments", i);
        return 0;
    });
    if (rc) return rc;
    for (int i = 0; i < n_trainers; ++i)
        if (settle_trainer(trainers[i])) return -1;          // (as the getters: unverified fused steps first)
    sac_trainer *t0 = trainers[0];
    ParamTensor T[PARAM_MAX_TENSORS];
    // staging: the job table, the chunk scratch, the records (per member, per selected net ascending, per tensor)
    size_t jobs = 0, chunks = 0, recs[SAC_GROUP_MAX] = {};
    for (int i = 0; i < n_trainers; ++i)
        for (int k = 0; k < PARAM_NETS; ++k) {
            if (!(io[i].nets >> k & 1u)) continue;
            const int n = param_tensor_list(trainers[i]->shape, k, T);
            for (int j = 0; j < n; ++j) chunks += (size_t)((T[j].E + PM_CH - 1) / PM_CH);
            recs[i] += (size_t)n;
            jobs += (size_t)n;
        }
    const size_t off_part = infer_align(sizeof(ParamJob) * jobs);
    const size_t off_rec = off_part + infer_align(sizeof(double) * SAC_PARAM_FIELDS_N * chunks);
    const size_t bytes = off_rec + infer_align(sizeof(double) * SAC_PARAM_FIELDS_N * jobs);
    SAC_REQUIRE(chunks < ((size_t)1 << 30), "internal: %zu chunks in one call", chunks);
    if (act_stage_reserve(t0, bytes)) return -1;
    const sac_trainer::ActStage &S = t0->act_stage;
    ParamJob *tab = reinterpret_cast<ParamJob *>(S.h);
    double *part = reinterpret_cast<double *>(S.d + off_part), *rec = reinterpret_cast<double *>(S.d + off_rec);
    int nj = 0, wgs = 0;
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        for (int k = 0; k < PARAM_NETS; ++k) {
            if (!(io[i].nets >> k & 1u)) continue;
            const int n = param_tensor_list(t->shape, k, T);
            const bool opt = (io[i].flags & SAC_PARAMS_OPT) && k <= 2;
            const int tk = (io[i].flags & SAC_PARAMS_GAP) ? param_target_of(t, k) : -1;
            const NetArrays N = net_arrays(t, k);
            for (int j = 0; j < n; ++j) {
                ParamJob &J = tab[nj];
                J = ParamJob{};
                J.a = T[j].a; J.E = T[j].E;
                J.X = N.P;
                J.mt = T[j].a.kind == PA_FRAG ? 1 : 0;
                if (opt) { J.M = J.mt ? N.MT : N.M; J.V = J.mt ? N.VT : N.V; }
                if (tk >= 0) J.T = net_arrays(t, tk).P;
                J.nch = (int)((J.E + PM_CH - 1) / PM_CH);
                J.wg0 = wgs;
                J.part = part + (size_t)wgs * SAC_PARAM_FIELDS_N;
                J.out = rec + (size_t)nj * SAC_PARAM_FIELDS_N;
                wgs += J.nch;
                nj += 1;
            }
        }
    }
    const ParamJob *d_tab = reinterpret_cast<const ParamJob *>(S.d);
    hipLaunchKernelGGL(sac::k_param_moments, dim3(wgs), dim3(PM_LANES), 0, t0->stream, d_tab, nj);
    SAC_HIP(hipGetLastError());
    hipLaunchKernelGGL(sac::k_param_finish, dim3((nj * SAC_PARAM_FIELDS_N + PM_LANES - 1) / PM_LANES), dim3(PM_LANES), 0,
                       t0->stream, d_tab, nj);
    SAC_HIP(hipGetLastError());
    if (wait_trainer_stream(t0)) return -1;
    const double *h_rec = reinterpret_cast<const double *>(S.h + off_rec);
    for (int i = 0; i < n_trainers; ++i) {
        memcpy(io[i].moments, h_rec, sizeof(double) * SAC_PARAM_FIELDS_N * recs[i]);
        h_rec += SAC_PARAM_FIELDS_N * recs[i];
    }
    return 0;
}

int sac_param_moments(sac_trainer_t *t, sac_params_io_t *io) {
    SAC_REQUIRE(t && io, "bad arguments to sac_param_moments");
    return sac_param_moments_many(&t, 1, io);
}
