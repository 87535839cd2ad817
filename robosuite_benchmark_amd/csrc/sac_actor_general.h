// Acting sessions for general-step trainers: sac_policy_act_general_many without the per-call marshalling (included by
// sac_trainer.hip behind sac_act_general.h).
//
// A session (sac_gactor) is made once for a fixed list of general-step trainers.  What never changes between two ticks
// is written once, at creation:
//
//   device memory   the job table GActJob[GMAXL][SAC_GROUP_MAX]: slot [l][i] is member i's layer l -- W and b inside
//                   GenNet::P, the input and output pointers, eps, N, K, tiles_n, A, vec and the static part of the kind
//                   (hidden, SAC head, TD3 head).  A member shallower than l has no job there (live == 0).
//   scratch         two ping-pong activation buffers per member, max_rows x its widest hidden layer each, owned by the
//                   SESSION: the trainer's act_gen buffers (sac_act_general.h) may be freed and reallocated by
//                   act_general_reserve, and two sessions over the same trainers must not meet in one buffer.
//   the slab        ONE mapped pinned allocation: the control block GActCtl, then per member obs (max_rows, O) FLOAT64,
//                   eps (max_rows, A) fp32, act (max_rows, A) fp32, each 256-byte aligned and fixed for the session's
//                   life.  The caller writes observations and eps THERE and reads actions THERE: a call copies nothing.
//
// A call (sac_gactor_act) drains the members with rows (sac_sync), rewrites the control block -- per member {rows,
// stochastic}, per layer depth l and member the first workgroup in launch l -- launches k_act_layer_session once per
// layer depth on member 0's stream and waits for one event of its own.  As with sac_actor_act the launches go on member
// 0's stream even when member 0 sits out.
//
// k_act_layer_session is k_act_layer (sac_act_general.h) line for line behind the prologue: the same tile mapping, AG_KC
// chunking, clamped loads and fix, MFMA order, hidden epilogue and head, so every action element is the same chain of
// operations and a session's actions are bit for bit sac_policy_act_general's.  The prologue reads the launch's wg0 row,
// n and stochastic with three 16-dword scalar loads issued together, picks the member with scalar compares and reads
// that member's static job from device memory.  In launch 0 (template parameter F64) the input rows are float64 in the
// slab and are rounded to fp32 on the way into LDS: a plain cast, round to nearest even, the value of numpy's
// astype(float32).  The fp32 instance has exactly k_act_layer's loads.
//
// GenNet::P and the layer offsets.  A general-step trainer's networks live in sac_general::arena, which
// gen_build_sac / gen_build_td3 (sac_general_host.h) allocate once and carve with a bump allocator; gen_shape_net, the
// only writer of offW / offB, runs there and nowhere else.  No general step path, no group loop (MLP and arch groups
// launch on the members' own tables), no sac_set_params / sac_set_opt_state / sac_set_scalars and no checkpoint load
// allocates, frees or re-lays the arena: all of them write INTO GenNet::P.  The table is therefore valid for the trainer
// handle's life and sac_gactor_act only asserts that (one pointer compare per member).  What does end a table entry is
// the end of the handle itself: the members must outlive the session (the Python GroupActor reopens its sessions when a
// trainer replaces its handle).
#pragma once

#include <type_traits>

namespace sac {

struct GActJob {                   // static, device memory: member i's layer l
    const float *W, *b;            // [N][K], [N] inside GenNet::P
    const void *X;                 // input rows [max_rows][K]: l == 0 the slab's float64 obs, else session scratch (fp32)
    const float *eps;              // the slab's eps [max_rows][A]
    float *Y;                      // session scratch [max_rows][N]; the member's last layer: the slab's act [max_rows][A]
    int N, K, tiles_n, A;
    int vec, kind;                 // kind: AG_HIDDEN, AG_SAC_MEAN (a SAC head: the call's flag makes it AG_SAC_SAMPLE), AG_TD3
    int live, pad;                 // 0: the member has no layer l
};

struct GActCtl {                   // per call, at the head of the slab
    int n[SAC_GROUP_MAX];          // rows of member i (0: sits out)
    int stochastic[SAC_GROUP_MAX]; // 1: SAC with exploration noise
    int wg0[gen::GMAXL][SAC_GROUP_MAX];   // first workgroup of member i in launch l (members without rows or without a
                                          // layer l share theirs with the next member; behind the last: the grid size)
};

__device__ __forceinline__ double ld1gd(const double *p) { return *(const __attribute__((address_space(1))) double *)(uintptr_t)p; }

template <bool F64>
__global__ __launch_bounds__(256) void k_act_layer_session(const GActJob *__restrict__ tab, const GActCtl *__restrict__ ctl, int l) {
    __shared__ __attribute__((aligned(16))) float Xs[RB * AG_LD];
    __shared__ float HL[RB * ACT_HEAD_LD];
    typedef const __attribute__((address_space(1))) f32x4 *gvec;
    typedef __attribute__((address_space(1))) float *gout;
    typedef typename std::conditional<F64, double, float>::type xin_t;
    // this workgroup's member: the last one whose first workgroup is not behind this one (wave-uniform; the three arrays
    // come over the link in one go: three 16-dword scalar loads); a member without a job here is passed over
    const i32x16 w0s = sload(reinterpret_cast<const i32x16 *>(ctl->wg0[l]));
    const i32x16 ns = sload(reinterpret_cast<const i32x16 *>(ctl->n));
    const i32x16 sts = sload(reinterpret_cast<const i32x16 *>(ctl->stochastic));
    int mi = 0, wg0 = w0s[0], n = ns[0], stochastic = sts[0];
#pragma unroll
    for (int i = 1; i < SAC_GROUP_MAX; ++i)
        if ((int)blockIdx.x >= w0s[i]) { mi = i; wg0 = w0s[i]; n = ns[i]; stochastic = sts[i]; }
    const GActJob *J = tab + mi;
    const float *W = sload(&J->W), *bp = sload(&J->b);
    const xin_t *X = reinterpret_cast<const xin_t *>(sload(&J->X));
    const int N = sload(&J->N), K = sload(&J->K), kind_s = sload(&J->kind);
    const int kind = (kind_s == AG_SAC_MEAN && stochastic) ? AG_SAC_SAMPLE : kind_s;
    const int tiles_n = sload(&J->tiles_n);
    const bool vec = sload(&J->vec) != 0;
    const int tile = (int)blockIdx.x - wg0;
    const int row0 = RB * (tile / tiles_n), n0 = AG_CT * (tile % tiles_n);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int ncol = n0 + 16 * wave + c;
    // this lane's weight row and this thread's input elements (chunk coordinates: row xr + 2 j, k = xk), both clamped
    const unsigned wrow = (unsigned)min(ncol, N - 1) * (unsigned)K;
    const int xk = tid & (AG_KC - 1), xr = tid >> 7;
    unsigned xrow[AG_XE];
#pragma unroll
    for (int j = 0; j < AG_XE; ++j) xrow[j] = (unsigned)min(row0 + xr + 2 * j, n - 1) * (unsigned)K;
    const float bias = ld1g(bp + min(ncol, N - 1));
    auto ldx = [&](unsigned i) -> xin_t {
        if constexpr (F64) return ld1gd(X + i); else return ld1g(X + i);
    };

    f32x4 wn[AG_NQ], wc[AG_NQ];
    xin_t xn[AG_XE];                   // (float64 rows stay float64 until they go into LDS: the loads stay in flight)
    auto fetch = [&](int kc) {
        if (kc + AG_KC <= K) {
            if (vec) {
#pragma unroll
                for (int q = 0; q < AG_NQ; ++q) wn[q] = *(gvec)(uintptr_t)(W + (wrow + (unsigned)(kc + 16 * q + 4 * g)));
            } else {
#pragma unroll
                for (int q = 0; q < AG_NQ; ++q)
#pragma unroll
                    for (int i = 0; i < 4; ++i) wn[q][i] = ld1g(W + (wrow + (unsigned)(kc + 16 * q + 4 * g + i)));
            }
#pragma unroll
            for (int j = 0; j < AG_XE; ++j) xn[j] = ldx(xrow[j] + (unsigned)(kc + xk));
            return;
        }
        // the edge chunk: reduction indices clamped (zeroed by fix); whole vectors stay inside K (K % 4 == 0)
        if (vec) {
#pragma unroll
            for (int q = 0; q < AG_NQ; ++q) wn[q] = *(gvec)(uintptr_t)(W + (wrow + (unsigned)min(kc + 16 * q + 4 * g, K - 4)));
        } else {
#pragma unroll
            for (int q = 0; q < AG_NQ; ++q)
#pragma unroll
                for (int i = 0; i < 4; ++i) wn[q][i] = ld1g(W + (wrow + (unsigned)min(kc + 16 * q + 4 * g + i, K - 1)));
        }
#pragma unroll
        for (int j = 0; j < AG_XE; ++j) xn[j] = ldx(xrow[j] + (unsigned)min(kc + xk, K - 1));
    };
    // behind the loads' arrival: the reduction's zero padding, on both operands
    auto fix = [&](int kc) {
        if (kc + AG_KC <= K) return;
#pragma unroll
        for (int q = 0; q < AG_NQ; ++q)
#pragma unroll
            for (int i = 0; i < 4; ++i) if (kc + 16 * q + 4 * g + i >= K) wc[q][i] = 0.f;
        if (kc + xk >= K) {
#pragma unroll
            for (int j = 0; j < AG_XE; ++j) xn[j] = 0;
        }
    };

    f32x4 acc = {};
    const int nS = (K + AG_KC - 1) / AG_KC;
    fetch(0);
    for (int s = 0; s < nS; ++s) {
        const int kc = AG_KC * s;
        if (s > 0) __syncthreads();
#pragma unroll
        for (int q = 0; q < AG_NQ; ++q) wc[q] = wn[q];
        fix(kc);
#pragma unroll
        for (int j = 0; j < AG_XE; ++j) Xs[(xr + 2 * j) * AG_LD + xk] = (float)xn[j];
        __syncthreads();
        if (s + 1 < nS) fetch(kc + AG_KC);
        SB();
#pragma unroll
        for (int q = 0; q < AG_NQ; ++q) {
            const f32x4 a = ld4(Xs + c * AG_LD + 16 * q + 4 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], wc[q][i], acc, 0, 0, 0);
        }
        SB();
    }

    if (kind == AG_HIDDEN) {
        float *Y = sload(&J->Y);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = row0 + 4 * g + i;
            const float v = acc[i] + bias;
            if (row < n && ncol < N) *(gout)(uintptr_t)(Y + ((unsigned)row * (unsigned)N + (unsigned)ncol)) = v < 0.f ? 0.f : v;
        }
        return;
    }
    // the head (one column tile, kind is uniform over the workgroup): pre-activations through LDS, one thread per action
    if (16 * wave < ACT_HEAD_LD) {
#pragma unroll
        for (int i = 0; i < 4; ++i) HL[(4 * g + i) * ACT_HEAD_LD + 16 * wave + c] = acc[i] + bias;
    }
    __syncthreads();
    const int A = sload(&J->A);
    const int r = tid >> 4, a = tid & 15;
    if (a < A && row0 + r < n) {
        const unsigned o = (unsigned)(row0 + r) * (unsigned)A + (unsigned)a;
        float v = HL[r * ACT_HEAD_LD + a];
        if (kind == AG_SAC_SAMPLE) {
            const float ls = fminf(fmaxf(HL[r * ACT_HEAD_LD + A + a], LOG_SIG_MIN), LOG_SIG_MAX);
            v += expf(ls) * ld1g(sload(&J->eps) + o);
        }
        *(gout)(uintptr_t)(sload(&J->Y) + o) = tanhf(v);
    }
}

}  // namespace sac

struct sac_gactor {
    int device = 0, n = 0, launches = 0;               // launches: the deepest member's layers
    sac_trainer *member[SAC_GROUP_MAX] = {};
    int max_rows[SAC_GROUP_MAX] = {};
    const float *P[SAC_GROUP_MAX] = {};                // GenNet::P of the policy, as the table holds it
    char *slab_h = nullptr, *slab_d = nullptr;         // the mapped pinned slab: host view, device view
    size_t off[SAC_GROUP_MAX][3] = {};                 // obs / eps / act of member i inside the slab
    float *scratch = nullptr;                          // every member's two activation buffers, one allocation
    GActJob tab[gen::GMAXL][SAC_GROUP_MAX] = {};       // host copy of the device table
    GActJob *d_tab = nullptr;
    hipEvent_t ev = nullptr;                           // the one event a call waits for
};

namespace {

int gactor_widest(const GenNet &P) {
    int widest = 1;
    for (int l = 0; l + 1 < P.nl; ++l) widest = std::max(widest, P.L[l].N);
    return widest;
}

// the session's allocations: the slab, the scratch, the device table (written here, once), the event
int gactor_build(sac_gactor *a, size_t slab_bytes) {
    SAC_HIP(hipSetDevice(a->device));
    SAC_HIP(hipHostMalloc(reinterpret_cast<void **>(&a->slab_h), slab_bytes, hipHostMallocMapped));
    SAC_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&a->slab_d), a->slab_h, 0));
    memset(a->slab_h, 0, slab_bytes);
    size_t buf[SAC_GROUP_MAX], floats = 0;             // floats of ONE of member i's two buffers (a multiple of 64)
    for (int i = 0; i < a->n; ++i) {
        buf[i] = ((size_t)a->max_rows[i] * gactor_widest(a->member[i]->gen->net[SAC_NET_POLICY]) + 63) & ~(size_t)63;
        floats += 2 * buf[i];
    }
    SAC_HIP(hipMalloc(reinterpret_cast<void **>(&a->scratch), sizeof(float) * floats));
    float *next = a->scratch;
    for (int i = 0; i < a->n; ++i) {
        const sac_trainer *t = a->member[i];
        const GenNet &P = t->gen->net[SAC_NET_POLICY];
        float *pp[2] = {next, next + buf[i]};
        next += 2 * buf[i];
        a->P[i] = P.P;
        a->launches = std::max(a->launches, P.nl);
        const void *x = a->slab_d + a->off[i][0];
        for (int l = 0; l < P.nl; ++l) {
            const GenLayer &L = P.L[l];
            const bool head = l + 1 == P.nl;
            GActJob &J = a->tab[l][i];
            J.W = P.P + L.offW; J.b = P.P + L.offB;
            J.X = x;
            J.eps = reinterpret_cast<const float *>(a->slab_d + a->off[i][1]);
            J.Y = head ? reinterpret_cast<float *>(a->slab_d + a->off[i][2]) : pp[l & 1];
            J.N = L.N; J.K = L.K;
            J.tiles_n = (L.N + AG_CT - 1) / AG_CT;
            J.A = t->A;
            J.vec = (L.K % 4 == 0 && L.offW % 4 == 0) ? 1 : 0;
            J.kind = !head ? AG_HIDDEN : (t->algo == 1 ? AG_TD3 : AG_SAC_MEAN);
            J.live = 1;
            x = J.Y;
        }
    }
    SAC_HIP(hipMalloc(reinterpret_cast<void **>(&a->d_tab), sizeof(a->tab)));
    SAC_HIP(hipMemcpy(a->d_tab, a->tab, sizeof(a->tab), hipMemcpyHostToDevice));
    SAC_HIP(hipEventCreateWithFlags(&a->ev, hipEventDisableTiming));
    return 0;
}

int gactor_free(sac_gactor *a) {
    (void)hipSetDevice(a->device);
    if (a->ev) (void)hipEventDestroy(a->ev);
    if (a->d_tab) (void)hipFree(a->d_tab);
    if (a->scratch) (void)hipFree(a->scratch);
    if (a->slab_h) (void)hipHostFree(a->slab_h);
    delete a;
    return 0;
}

}  // namespace

// (declared extern "C" in include/sac_hip.h)
int sac_gactor_create(sac_gactor_t **out, sac_trainer_t *const *trainers, int n_trainers, const int32_t *max_rows) {
    SAC_REQUIRE(out, "null out pointer to sac_gactor_create");
    *out = nullptr;
    SAC_REQUIRE(trainers && max_rows, "bad arguments to sac_gactor_create");
    SAC_REQUIRE(n_trainers >= 1 && n_trainers <= SAC_GROUP_MAX, "sac_gactor_create takes 1..%d trainers (got %d)", SAC_GROUP_MAX,
                n_trainers);
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        SAC_REQUIRE(t, "trainer %d is null", i);
        for (int j = 0; j < i; ++j) SAC_REQUIRE(trainers[j] != t, "trainer %d is trainer %d again", i, j);
        SAC_REQUIRE(t->device == trainers[0]->device, "trainer %d lives on device %d, trainer 0 on device %d", i, t->device,
                    trainers[0]->device);
        SAC_REQUIRE(t->gen, "trainer %d has the fused kernels' shapes (two hidden layers of at most 256 units): sac_actor_create "
                    "makes its acting sessions, sac_gactor_create serves the general step", i);
        SAC_REQUIRE(max_rows[i] >= 1 && max_rows[i] <= ACT_MAX_ROWS, "trainer %d: max_rows %d (1..%d)", i, (int)max_rows[i],
                    ACT_MAX_ROWS);
    }
    sac_gactor *a = new sac_gactor;
    a->device = trainers[0]->device;
    a->n = n_trainers;
    size_t bytes = (sizeof(GActCtl) + 255) & ~(size_t)255;
    for (int i = 0; i < n_trainers; ++i) {
        sac_trainer *t = trainers[i];
        a->member[i] = t;
        a->max_rows[i] = max_rows[i];
        const size_t rows = (size_t)max_rows[i];
        const size_t part[3] = {sizeof(double) * rows * t->O, sizeof(float) * rows * t->A, sizeof(float) * rows * t->A};
        for (int k = 0; k < 3; ++k) { a->off[i][k] = bytes; bytes += (part[k] + 255) & ~(size_t)255; }
    }
    if (gactor_build(a, bytes)) { gactor_free(a); return -1; }
    *out = a;
    return 0;
}

int sac_gactor_destroy(sac_gactor_t *a) {
    if (!a) return 0;
    return gactor_free(a);
}

int sac_gactor_arrays(sac_gactor_t *a, int member, double **obs, float **eps, float **act) {
    SAC_REQUIRE(a, "null acting session");
    SAC_REQUIRE(member >= 0 && member < a->n, "sac_gactor_arrays: member %d of %d", member, a->n);
    if (obs) *obs = reinterpret_cast<double *>(a->slab_h + a->off[member][0]);
    if (eps) *eps = reinterpret_cast<float *>(a->slab_h + a->off[member][1]);
    if (act) *act = reinterpret_cast<float *>(a->slab_h + a->off[member][2]);
    return 0;
}

int sac_gactor_act(sac_gactor_t *a, const int32_t *n_rows, const int32_t *deterministic) {
    SAC_REQUIRE(a && n_rows && deterministic, "bad arguments to sac_gactor_act");
    // every refusal comes first: nothing has changed when one of them returns
    int active = 0;
    for (int i = 0; i < a->n; ++i) {
        const sac_trainer *t = a->member[i];
        SAC_REQUIRE(t->xcd_mask == 0xffu, "trainer %d is confined by sac_trainer_set_xcd[_mask]: device acting launches on the "
                    "whole chip", i);
        SAC_REQUIRE(n_rows[i] >= 0 && n_rows[i] <= a->max_rows[i], "trainer %d: %d rows (0..%d in this session, 0 = sits out)", i,
                    (int)n_rows[i], a->max_rows[i]);
        SAC_REQUIRE(t->gen && t->gen->net[SAC_NET_POLICY].P == a->P[i], "internal: the policy of trainer %d has moved under its "
                    "acting session", i);
        active += n_rows[i] > 0;
    }
    SAC_REQUIRE(active > 0, "no trainer has rows to act on");
    sac_trainer *t0 = a->member[0];
    SAC_HIP(hipSetDevice(a->device));
    // the weights as of the last completed step of any step path: drain every member with rows
    for (int i = 0; i < a->n; ++i)
        if (n_rows[i] > 0 && sac_sync(a->member[i])) return -1;
    GActCtl *ctl = reinterpret_cast<GActCtl *>(a->slab_h);
    int blocks[gen::GMAXL] = {};
    for (int i = 0; i < SAC_GROUP_MAX; ++i) {
        const bool rows = i < a->n && n_rows[i] > 0;
        ctl->n[i] = rows ? n_rows[i] : 0;
        ctl->stochastic[i] = (rows && a->member[i]->algo == 0 && !deterministic[i]) ? 1 : 0;
        for (int l = 0; l < gen::GMAXL; ++l) {
            ctl->wg0[l][i] = blocks[l];
            if (rows && a->tab[l][i].live) blocks[l] += ((n_rows[i] + RB - 1) / RB) * a->tab[l][i].tiles_n;
        }
    }
    const GActCtl *d_ctl = reinterpret_cast<const GActCtl *>(a->slab_d);
    for (int l = 0; l < a->launches && blocks[l] > 0; ++l) {
        if (l == 0) hipLaunchKernelGGL(k_act_layer_session<true>, dim3(blocks[l]), dim3(256), 0, t0->stream, a->d_tab, d_ctl, l);
        else hipLaunchKernelGGL(k_act_layer_session<false>, dim3(blocks[l]), dim3(256), 0, t0->stream,
                                a->d_tab + (size_t)l * SAC_GROUP_MAX, d_ctl, l);
        SAC_HIP(hipGetLastError());
    }
    SAC_HIP(hipEventRecord(a->ev, t0->stream));
    return wait_event(a->ev);
}
