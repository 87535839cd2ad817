// The statistics of an evaluation reduced on the device: k_eval_moments (included by sac_trainer.hip in front of
// sac_eval.h and sac_eval_general.h, whose *_stats_many entries launch it).
//
// One launch on the first member's stream behind k_eval (fused shapes) or k_eval_y (general step) and in front of the
// entry's single wait.  It reads the float32 columns where those kernels left them in the staging -- `rows`
// (SAC_EVAL_ROWS_N, n), mu and log_std (n, A) -- and writes, per member with rows, SAC_EVAL_MOMENTS_N records
// sac_eval_moment_t {count, sum, m2, sumsq, max, min} of float64 into the staging:
//
//   SAC_EVAL_M_Q1 / Q2 / Y / LOG_PI     the column, n elements
//   SAC_EVAL_M_MU / LOG_STD             the head's mean / clamped log_std, n A elements
//   SAC_EVAL_M_TD1 / TD2                (double)q - (double)y, n elements
//   SAC_EVAL_M_POLICY                   (double)log_pi - min((double)q1_new, (double)q2_new), n elements; the min keeps a
//                                       NaN as np.minimum does
//
// every element formed in float64 from the float32 columns: what sac.eval_statistics forms on the host.
//
//   grid    one workgroup (256 lanes) per (member, quantity): at most SAC_GROUP_MAX x SAC_EVAL_MOMENTS_N = 144
//   sums    lane t adds the elements t, t + 256, t + 512, ... in this order; the 256 partial sums meet in a fixed LDS
//           tree (128, 64, ... 1).  So the order of every sum is a function of the quantity's own element count and of
//           nothing else: not of the grid, the member's place in the table, its neighbours or the optional outputs the
//           caller asked for.  No atomics.
//   m2      sum (x - sum / count)^2 over the same elements in a SECOND pass, as np.std does -- never sumsq - sum^2 / count
//           -- so a constant column has m2 == 0 exactly
//   max/min keep a NaN as np.max / np.min do (fmax / fmin would drop it): one NaN element makes both NaN
//
// The kernel writes its records and nothing else.  Workgroups never talk to each other.
#pragma once

namespace sac {

constexpr int EM_LANES = 256;

struct MomentsMember {
    const float *rows, *mu, *log_std;   // (SAC_EVAL_ROWS_N, n), (n, A), (n, A): where the evaluation kernels wrote them
    sac_eval_moment_t *out;             // [SAC_EVAL_MOMENTS_N]
    int n, A;
};

// np.maximum / np.minimum on two values: a NaN on either side stays
__device__ __forceinline__ double em_max(double m, double x) { return (x > m || x != x) ? x : m; }
__device__ __forceinline__ double em_min(double m, double x) { return (x < m || x != x) ? x : m; }

enum { EM_COLUMN, EM_DIFF, EM_POLICY, EM_SQDIFF };

// element i of a quantity: a[i], a[i] - b[i], a[i] - min(b[i], c[i]), or (a[i] - b[i])^2 (td3_eval_moments.h: the
// product rounded on its own, never fused into the sum behind it, as (q - y) ** 2 is in float64 NumPy)
template <int KIND>
__device__ __forceinline__ double em_elem(const float *a, const float *b, const float *c, int i) {
    const double x = (double)a[i];
    if constexpr (KIND == EM_COLUMN) return x;
    else if constexpr (KIND == EM_DIFF) return x - (double)b[i];
    else if constexpr (KIND == EM_POLICY) return x - em_min((double)b[i], (double)c[i]);
    else {
#pragma clang fp contract(off)
        const double d = x - (double)b[i];
        return d * d;
    }
}

// L[k][t] <- the tree over lanes of L[k], for k < NK: sums for k < NSUM, then one max, then one min.  The result is in L[k][0].
template <int NSUM, int NK>
__device__ __forceinline__ void em_tree(double (*L)[EM_LANES]) {
    const int t = threadIdx.x;
    __syncthreads();
#pragma unroll 1
    for (int s = EM_LANES / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < NSUM; ++k) L[k][t] = L[k][t] + L[k][t + s];
            if constexpr (NK > NSUM) {
                L[NSUM][t] = em_max(L[NSUM][t], L[NSUM][t + s]);
                L[NSUM + 1][t] = em_min(L[NSUM + 1][t], L[NSUM + 1][t + s]);
            }
        }
        __syncthreads();
    }
}

template <int KIND>
__device__ __forceinline__ void em_reduce(const float *a, const float *b, const float *c, int count, sac_eval_moment_t *out,
                                          double (*L)[EM_LANES]) {
    const int t = threadIdx.x;
    double sum = 0.0, sumsq = 0.0, mx = -__builtin_huge_val(), mn = __builtin_huge_val();
    for (int i = t; i < count; i += EM_LANES) {
        const double x = em_elem<KIND>(a, b, c, i);
        sum = sum + x;
        sumsq = sumsq + x * x;
        mx = em_max(mx, x);
        mn = em_min(mn, x);
    }
    L[0][t] = sum; L[1][t] = sumsq; L[2][t] = mx; L[3][t] = mn;
    em_tree<2, 4>(L);
    const double tsum = L[0][0], tsumsq = L[1][0], tmax = L[2][0], tmin = L[3][0];
    const double mean = tsum / (double)count;
    double m2 = 0.0;
    for (int i = t; i < count; i += EM_LANES) {
        const double d = em_elem<KIND>(a, b, c, i) - mean;
        m2 = m2 + d * d;
    }
    __syncthreads();                     // (every lane has read the first tree's results)
    L[0][t] = m2;
    em_tree<1, 1>(L);
    if (t == 0) {
        out->count = (double)count; out->sum = tsum; out->m2 = L[0][0];
        out->sumsq = tsumsq; out->max = tmax; out->min = tmin;
    }
}

__global__ __launch_bounds__(EM_LANES) void k_eval_moments(const MomentsMember *__restrict__ tab) {
    __shared__ double L[4][EM_LANES];
    const MomentsMember *M = tab + (int)blockIdx.x / SAC_EVAL_MOMENTS_N;
    const int q = (int)blockIdx.x % SAC_EVAL_MOMENTS_N;
    const int n = M->n, nA = n * M->A;      // (n <= 1024, A <= 16)
    const float *rows = M->rows;
    sac_eval_moment_t *out = M->out + q;
    const float *y = rows + SAC_EVAL_Y * n;
    switch (q) {
    case SAC_EVAL_M_Q1: em_reduce<EM_COLUMN>(rows + SAC_EVAL_Q1 * n, nullptr, nullptr, n, out, L); break;
    case SAC_EVAL_M_Q2: em_reduce<EM_COLUMN>(rows + SAC_EVAL_Q2 * n, nullptr, nullptr, n, out, L); break;
    case SAC_EVAL_M_Y: em_reduce<EM_COLUMN>(y, nullptr, nullptr, n, out, L); break;
    case SAC_EVAL_M_LOG_PI: em_reduce<EM_COLUMN>(rows + SAC_EVAL_LOG_PI * n, nullptr, nullptr, n, out, L); break;
    case SAC_EVAL_M_MU: em_reduce<EM_COLUMN>(M->mu, nullptr, nullptr, nA, out, L); break;
    case SAC_EVAL_M_LOG_STD: em_reduce<EM_COLUMN>(M->log_std, nullptr, nullptr, nA, out, L); break;
    case SAC_EVAL_M_TD1: em_reduce<EM_DIFF>(rows + SAC_EVAL_Q1 * n, y, nullptr, n, out, L); break;
    case SAC_EVAL_M_TD2: em_reduce<EM_DIFF>(rows + SAC_EVAL_Q2 * n, y, nullptr, n, out, L); break;
    default:
        em_reduce<EM_POLICY>(rows + SAC_EVAL_LOG_PI * n, rows + SAC_EVAL_Q1_NEW * n, rows + SAC_EVAL_Q2_NEW * n, n, out, L);
    }
}

}  // namespace sac

namespace {

// The staging of the moments behind an entry's own parts: the member table, then one block of records per member.
struct MomentsStage { size_t tab = 0, rec[SAC_GROUP_MAX] = {}; };

void moments_carve(size_t &bytes, MomentsStage &MS, int n_trainers) {
    MS.tab = bytes;
    bytes += infer_align(sizeof(MomentsMember) * SAC_GROUP_MAX);
    for (int i = 0; i < n_trainers; ++i) {
        MS.rec[i] = bytes;
        bytes += infer_align(sizeof(sac_eval_moment_t) * SAC_EVAL_MOMENTS_N);
    }
}

// member m of the launch (trainer i of the call): its columns in the staging (dev(k): part k of the member on the device),
// named by the objective (Obj::moments)
template <class Obj, class Dev>
void moments_member(const sac_trainer::ActStage &S, const MomentsStage &MS, int m, int i, Dev dev, int n, int A) {
    typename Obj::Moments &M = reinterpret_cast<typename Obj::Moments *>(S.h + MS.tab)[m];
    Obj::moments(M, dev);
    M.out = reinterpret_cast<sac_eval_moment_t *>(S.d + MS.rec[i]);
    M.n = n; M.A = A;
}

template <class Obj>
int moments_launch(sac_trainer *t0, const MomentsStage &MS, int m) {
    const sac_trainer::ActStage &S = t0->act_stage;
    hipLaunchKernelGGL(Obj::moments_kernel, dim3(m * Obj::MOMENTS_N), dim3(sac::EM_LANES), 0, t0->stream,
                       reinterpret_cast<const typename Obj::Moments *>(S.d + MS.tab));
    SAC_HIP(hipGetLastError());
    return 0;
}

// behind the wait: trainer i's records
template <class Stats>
void moments_read(const sac_trainer::ActStage &S, const MomentsStage &MS, int i, Stats *st) {
    memcpy(st->m, S.h + MS.rec[i], sizeof(st->m));
}

}  // namespace
