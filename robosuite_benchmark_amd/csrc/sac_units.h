// Per-unit statistics of the hidden layers, reduced on the device: k_unit_moments, the reducer of both families, and
// k_units with sac_unit_moments[_many], the fused kernels' shapes (included by sac_trainer.hip behind sac_qval_general.h,
// in front of sac_units_general.h, whose entries serve the general step).
//
// One hidden layer of one net is an activation matrix X (n rows, N true units, row stride ld) of float32 post-ReLU
// values, where a forward kernel left them.  Its record is SAC_UNIT_FIELDS_N arrays of N float64, out[f N + u]:
//
//   SAC_UNIT_SUM      sum over rows of (double)x
//   SAC_UNIT_SUMSQ    sum over rows of (double)x (double)x (the product of two float32 values is exact in float64: a
//                     contraction into an FMA cannot change it)
//   SAC_UNIT_ACTIVE   the number of rows with x > 0 (a NaN is not active)
//   SAC_UNIT_MAX      the largest x; a NaN stays (em_max, sac_eval_moments.h)
//
//   table   a launch carries jobs (UnitJob, device-visible memory, read with scalar loads): one job per matrix.  A
//           workgroup finds its job by a bisection over wg0 (ascending), as k_qval_layer does.
//   grid    one workgroup (256 lanes) per 64 consecutive units of one job
//   order   lane (wave w, column c) adds rows w, w + 4, w + 8, ... ascending for unit 64 tile + c; the four partials meet
//           through LDS as (p0 + p1) + (p2 + p3), max and active likewise.  The order of every sum is a function of n
//           alone: not of the grid, the job's place in the table, its neighbours or the stride.  No atomics.
//
// The kernel reads X and writes its records: nothing else.  Workgroups never talk to each other, so a member's records
// are byte for byte those of its solo call.  infer.unit_moments_reference restates it in NumPy float64.  Vector stores
// only.
#pragma once

namespace sac {

constexpr int UM_COLS = 64;               // units of one workgroup

struct UnitJob {
    const float *X;                // [n][ld], the units in columns 0 .. N - 1
    double *out;                   // [SAC_UNIT_FIELDS_N][N]
    int ld, N, n, wg0;             // wg0: first workgroup of this job in the launch
};

__global__ __launch_bounds__(256) void k_unit_moments(const UnitJob *__restrict__ tab, int n_jobs) {
    __shared__ double L[SAC_UNIT_FIELDS_N][4][UM_COLS];
    int lo = 0, hi = n_jobs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int)blockIdx.x >= sload(&tab[mid].wg0)) lo = mid; else hi = mid;
    }
    const UnitJob *J = tab + lo;
    const float *X = sload(&J->X);
    const int ld = sload(&J->ld), N = sload(&J->N), n = sload(&J->n);
    const int u0 = UM_COLS * ((int)blockIdx.x - sload(&J->wg0));
    const int w = threadIdx.x >> 6, c = threadIdx.x & 63;
    double sum = 0.0, sumsq = 0.0, active = 0.0, mx = -__builtin_huge_val();
    if (u0 + c < N) {
        const float *col = X + (u0 + c);
        for (int r = w; r < n; r += 4) {
            const float h = col[(size_t)r * ld];
            const double x = (double)h;
            sum = sum + x;
            sumsq = sumsq + x * x;
            active = active + (h > 0.f ? 1.0 : 0.0);
            mx = em_max(mx, x);
        }
    }
    L[SAC_UNIT_SUM][w][c] = sum; L[SAC_UNIT_SUMSQ][w][c] = sumsq;
    L[SAC_UNIT_ACTIVE][w][c] = active; L[SAC_UNIT_MAX][w][c] = mx;
    __syncthreads();
    // wave f finishes field f
    const int f = w;
    if (u0 + c < N) {
        const double p0 = L[f][0][c], p1 = L[f][1][c], p2 = L[f][2][c], p3 = L[f][3][c];
        const double v = f == SAC_UNIT_MAX ? em_max(em_max(p0, p1), em_max(p2, p3)) : (p0 + p1) + (p2 + p3);
        sload(&J->out)[(size_t)f * N + (u0 + c)] = v;
    }
}

}  // namespace sac

namespace {

// the nets a mask may select: bit k is SAC_NET_* == k; bit SAC_NET_TARGET_POLICY on TD3 handles only
constexpr int UNIT_NETS = 6;
constexpr uint32_t UNIT_Q_NETS = 0x1eu;
constexpr int UNIT_JOBS = UNIT_NETS * SAC_GROUP_MAX;      // matrices of one launch

// What the unit entries refuse alike in front of their tables (infer_admit: the refusals and the drain)
int units_admit(const InferEntry &E, sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
                const sac_units_io_t *io) {
    return infer_admit(E, trainers, n_trainers, n_rows, [&](int i) {
        const uint32_t nets = io[i].nets;
        SAC_REQUIRE(nets != 0 && nets < (1u << UNIT_NETS), "trainer %d: nets 0x%x selects no network or an unknown one (bit k "
                    "selects SAC_NET_* == k)", i, (unsigned)nets);
        SAC_REQUIRE(!(nets >> SAC_NET_TARGET_POLICY & 1u) || trainers[i]->algo == 1, "trainer %d: nets 0x%x selects the target "
                    "policy, which only a TD3 trainer has", i, (unsigned)nets);
        SAC_REQUIRE(io[i].obs && io[i].moments, "trainer %d: null observations or moments", i);
        SAC_REQUIRE(!(nets & UNIT_Q_NETS) || io[i].act, "trainer %d: nets 0x%x selects a Q network and the actions are null", i,
                    (unsigned)nets);
        return 0;
    });
}

int units_launch(sac_trainer *t0, const sac::UnitJob *d_tab, int n_jobs, int blocks) {
    hipLaunchKernelGGL(sac::k_unit_moments, dim3(blocks), dim3(256), 0, t0->stream, d_tab, n_jobs);
    SAC_HIP(hipGetLastError());
    return 0;
}

}  // namespace

// ---- the fused kernels' shapes: k_units keeps the two hidden layers k_act / k_qval throw away ----
//
//   grid    one workgroup (4 waves) per (member, selected net, 16-row block); the workgroups of all members side by side
//           -- a member's nets one behind the other, each with its row-blocks -- found through the per-member table
//           UnitsMember: up to SAC_GROUP_MAX members, 6 nets and 1024 rows in ONE launch
//   math    a policy block runs infer_hidden behind infer_fill(obs) exactly as k_act does (KL0 from KP), a Q block
//           infer_hidden behind infer_fill(obs, act) exactly as k_qval does (KQ = KP + 16): the activations are those
//           kernels' bit for bit.  No head and no output layer.
//   store   rows < n and columns < the TRUE width of X1 and X2 (pad units are not units) to the net's two tap matrices
//           (n, h1), (n, h2), which k_unit_moments reduces behind it in the same stream
//   LDS     k_qval's (qval_lds_bytes)
namespace sac {

struct UnitsMember {
    const float *P[UNIT_NETS];             // forward copies (Net::P) of the SELECTED nets, in ascending SAC_NET_* order
    float *tap[UNIT_NETS][2];              // their tap matrices (n, h1), (n, h2)
    long long offW[UNIT_NETS][2], offB[UNIT_NETS][2];   // the two hidden layers inside P
    int h[UNIT_NETS][2];                   // true widths
    int q[UNIT_NETS];                      // 1: a Q net (reads cat(obs, act))
    const float *obs, *act;                // (n, O) / (n, A) row-major
    int O, A, KP, n;
    int n_sel, wg0;                        // selected nets; first workgroup of this member in the launch
};

__global__ __launch_bounds__(256) void k_units(const UnitsMember *__restrict__ tab, int n_members) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const UnitsMember *M = tab + infer_member(tab, n_members, &UnitsMember::wg0);
    const int O = sload(&M->O), A = sload(&M->A), KP = sload(&M->KP), n = sload(&M->n);
    const int nrb = (n + RB - 1) / RB;
    const int local = (int)blockIdx.x - sload(&M->wg0);
    const int sel = local / nrb, row0 = (local - sel * nrb) * RB;      // which selected net, which row-block
    const float *P = sload(&M->P[sel]);
    const bool q = sload(&M->q[sel]) != 0;
    const int K0 = q ? KP + 16 : KP, KL0 = (K0 + 63) & ~63;
    float *X0 = lds;                     // [16][KL0]
    float *X1 = X0 + RB * KL0;           // [16][256]
    float *X2 = X1 + RB * H;             // [16][256]
    infer_hidden(P, M->offW[sel], M->offB[sel], X0, KL0, K0, X1, X2, [&] {
        if (q) infer_fill(X0, KL0, row0, n, sload(&M->obs), O, sload(&M->act), KP, A);
        else infer_fill(X0, KL0, row0, n, sload(&M->obs), O);
    });
    const int rows = min(RB, n - row0);
#pragma unroll
    for (int l = 0; l < 2; ++l) {
        const float *X = l ? X2 : X1;
        const int h = sload(&M->h[sel][l]);
        float *out = sload(&M->tap[sel][l]) + (size_t)row0 * h;
        for (int i = threadIdx.x; i < rows * h; i += 256) {
            const int r = i / h, c = i - r * h;
            out[i] = X[lds_off(r, c, H)];
        }
    }
}

}  // namespace sac

namespace {

std::atomic<bool> g_units_lds_raised[64];

}  // namespace

// (declared extern "C" in include/sac_hip.h)
int sac_unit_moments_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, sac_units_io_t *io) {
    SAC_REQUIRE(trainers && n_rows && io, "bad arguments to sac_unit_moments_many");
    const InferEntry E = {"sac_unit_moments_many", false, false, "device unit statistics",
                          "sac_unit_moments_general is the entry", "reduce"};
    if (int rc = units_admit(E, trainers, n_trainers, n_rows, io)) return rc;
    sac_trainer *t0 = trainers[0];
    // staging: the two tables, then per member obs (n, O), act (n, A), the records, the taps
    const size_t tab_m = 0, tab_u = infer_align(sizeof(UnitsMember) * SAC_GROUP_MAX);
    size_t bytes = tab_u + infer_align(sizeof(UnitJob) * 2 * UNIT_JOBS);
    size_t off[SAC_GROUP_MAX][4] = {}, units[SAC_GROUP_MAX] = {};
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        for (int k = 0; k < UNIT_NETS; ++k)
            if (io[i].nets >> k & 1u) units[i] += (UNIT_Q_NETS >> k & 1u) ? t->HQ[0] + t->HQ[1] : t->HP[0] + t->HP[1];
        const size_t n = (size_t)n_rows[i];
        const size_t part[4] = {sizeof(float) * n * t->O, sizeof(float) * n * t->A,
                                sizeof(double) * SAC_UNIT_FIELDS_N * units[i], sizeof(float) * n * units[i]};
        infer_carve(bytes, off[i], part, 4, 1);
    }
    if (act_stage_reserve(t0, bytes)) return -1;
    const sac_trainer::ActStage &S = t0->act_stage;
    UnitsMember *mtab = reinterpret_cast<UnitsMember *>(S.h + tab_m);
    UnitJob *utab = reinterpret_cast<UnitJob *>(S.h + tab_u);
    int wgs = 0, m = 0, kq_max = 0, jobs = 0, ublocks = 0;
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        const size_t n = (size_t)n_rows[i];
        UnitsMember &M = mtab[m++];
        M = UnitsMember{};
        double *rec = reinterpret_cast<double *>(S.d + off[i][2]);
        float *taps = reinterpret_cast<float *>(S.d + off[i][3]);
        for (int k = 0; k < UNIT_NETS; ++k) {
            if (!(io[i].nets >> k & 1u)) continue;
            const Net &N = t->net[k];
            const bool q = (UNIT_Q_NETS >> k & 1u) != 0;
            const int s = M.n_sel++;
            M.P[s] = N.P; M.q[s] = q ? 1 : 0;
            for (int l = 0; l < 2; ++l) {
                const int h = q ? t->HQ[l] : t->HP[l];
                M.offW[s][l] = N.L[l].offW; M.offB[s][l] = N.L[l].offB;
                M.h[s][l] = h; M.tap[s][l] = taps;
                UnitJob &U = utab[jobs++];
                U.X = taps; U.out = rec; U.ld = h; U.N = h; U.n = n_rows[i];
                U.wg0 = ublocks;
                ublocks += (h + UM_COLS - 1) / UM_COLS;
                taps += n * h;
                rec += (size_t)SAC_UNIT_FIELDS_N * h;
            }
        }
        M.obs = reinterpret_cast<const float *>(S.d + off[i][0]);
        M.act = reinterpret_cast<const float *>(S.d + off[i][1]);
        M.O = t->O; M.A = t->A; M.KP = t->KP; M.n = n_rows[i];
        M.wg0 = wgs;
        wgs += M.n_sel * ((n_rows[i] + RB - 1) / RB);
        kq_max = std::max(kq_max, t->KQ);
        memcpy(S.h + off[i][0], io[i].obs, sizeof(float) * n * t->O);
        if (io[i].nets & UNIT_Q_NETS) memcpy(S.h + off[i][1], io[i].act, sizeof(float) * n * t->A);
    }
    const size_t lds = qval_lds_bytes(kq_max);
    if (infer_raise_lds(reinterpret_cast<const void *>(k_units), g_units_lds_raised, t0->device, lds, qval_lds_bytes(512))) return -1;
    hipLaunchKernelGGL(k_units, dim3(wgs), dim3(256), lds, t0->stream, reinterpret_cast<const UnitsMember *>(S.d + tab_m), m);
    SAC_HIP(hipGetLastError());
    if (units_launch(t0, reinterpret_cast<const UnitJob *>(S.d + tab_u), jobs, ublocks)) return -1;
    if (wait_trainer_stream(t0)) return -1;
    for (int i = 0; i < n_trainers; ++i) {
        if (n_rows[i] == 0) continue;
        memcpy(io[i].moments, S.h + off[i][2], sizeof(double) * SAC_UNIT_FIELDS_N * units[i]);
        if (io[i].activations) memcpy(io[i].activations, S.h + off[i][3], sizeof(float) * (size_t)n_rows[i] * units[i]);
    }
    return 0;
}

int sac_unit_moments(sac_trainer_t *t, int64_t n, sac_units_io_t *io) {
    SAC_REQUIRE(t && io, "bad arguments to sac_unit_moments");
    SAC_REQUIRE(n >= 1 && n <= ACT_MAX_ROWS, "sac_unit_moments: %lld rows (1..%d per call)", (long long)n, ACT_MAX_ROWS);
    const int32_t rows = (int32_t)n;
    return sac_unit_moments_many(&t, 1, &rows, io);
}
