// The statistics of a TD3 evaluation reduced on the device: k_eval_moments_td3 (included by sac_trainer.hip behind
// sac_eval_moments.h, whose reduction it runs and whose host helpers launch it, and in front of td3_eval.h).
//
// One launch on the first member's stream behind k_eval_td3 (fused shapes) or k_eval_y_td3 (general step) and in front of
// the entry's single wait.  It reads the float32 columns where those kernels left them in the staging -- `rows`
// (TD3_EVAL_ROWS_N, n) and a_pi (n, A) -- and writes, per member with rows, TD3_EVAL_MOMENTS_N records sac_eval_moment_t
// {count, sum, m2, sumsq, max, min} of float64 into the staging:
//
//   TD3_EVAL_M_Q1 / Q2 / Y / Q_PI       the column, n elements
//   TD3_EVAL_M_A_PI                     the policy's action, n A elements
//   TD3_EVAL_M_TD1 / TD2                (double)q - (double)y, n elements
//   TD3_EVAL_M_BELLMAN1 / BELLMAN2      d * d with d as above, n elements: the product is rounded on its own (EM_SQDIFF),
//                                       what (q - y) ** 2 is in float64 NumPy
//
// every element formed in float64 from the float32 columns: what infer.td3_eval_statistics forms on the host.
//
// The grid (one 256-lane workgroup per (member, quantity): at most SAC_GROUP_MAX x TD3_EVAL_MOMENTS_N = 144), the order of
// the sums (lane t adds elements t, t + 256, ...; the fixed LDS tree), m2's second pass and the NaN-keeping max / min are
// em_reduce's (sac_eval_moments.h), as they stand: the order of every sum is a function of the record's own element
// count and of nothing else, so a member's records are byte for byte those of its solo call.  No atomics; the kernel
// writes its records and nothing else; workgroups never talk to each other.  Vector stores only.
#pragma once

namespace sac {

struct Td3MomentsMember {
    const float *rows, *a_pi;           // (TD3_EVAL_ROWS_N, n), (n, A): where the evaluation kernels wrote them
    sac_eval_moment_t *out;             // [TD3_EVAL_MOMENTS_N]
    int n, A;
};

__global__ __launch_bounds__(EM_LANES) void k_eval_moments_td3(const Td3MomentsMember *__restrict__ tab) {
    __shared__ double L[4][EM_LANES];
    const Td3MomentsMember *M = tab + (int)blockIdx.x / TD3_EVAL_MOMENTS_N;
    const int q = (int)blockIdx.x % TD3_EVAL_MOMENTS_N;
    const int n = M->n, nA = n * M->A;      // (n <= 1024, A <= 16)
    const float *rows = M->rows;
    sac_eval_moment_t *out = M->out + q;
    const float *q1 = rows + TD3_EVAL_Q1 * n, *q2 = rows + TD3_EVAL_Q2 * n, *y = rows + TD3_EVAL_Y * n;
    switch (q) {
    case TD3_EVAL_M_Q1: em_reduce<EM_COLUMN>(q1, nullptr, nullptr, n, out, L); break;
    case TD3_EVAL_M_Q2: em_reduce<EM_COLUMN>(q2, nullptr, nullptr, n, out, L); break;
    case TD3_EVAL_M_Y: em_reduce<EM_COLUMN>(y, nullptr, nullptr, n, out, L); break;
    case TD3_EVAL_M_Q_PI: em_reduce<EM_COLUMN>(rows + TD3_EVAL_Q_PI * n, nullptr, nullptr, n, out, L); break;
    case TD3_EVAL_M_A_PI: em_reduce<EM_COLUMN>(M->a_pi, nullptr, nullptr, nA, out, L); break;
    case TD3_EVAL_M_TD1: em_reduce<EM_DIFF>(q1, y, nullptr, n, out, L); break;
    case TD3_EVAL_M_TD2: em_reduce<EM_DIFF>(q2, y, nullptr, n, out, L); break;
    case TD3_EVAL_M_BELLMAN1: em_reduce<EM_SQDIFF>(q1, y, nullptr, n, out, L); break;
    default: em_reduce<EM_SQDIFF>(q2, y, nullptr, n, out, L);
    }
}

}  // namespace sac

namespace {

// the staging is MomentsStage as moments_carve lays it out (sac_eval_moments.h): a table at least as large, as many records
static_assert(sizeof(sac::Td3MomentsMember) <= sizeof(sac::MomentsMember) && (int)TD3_EVAL_MOMENTS_N == (int)SAC_EVAL_MOMENTS_N,
              "k_eval_moments_td3's table and records fit the places moments_carve makes");

}  // namespace
