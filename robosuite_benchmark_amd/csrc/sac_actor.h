// Acting sessions: sac_policy_act_many without the per-call marshalling (included by sac_trainer.hip behind sac_act.h).
//
// A session (sac_actor) is made once for a fixed list of trainers.  What never changes between two ticks is written
// once, at creation:
//
//   device memory   the member table ActEntry[n]: Net::P, the three layers' offW / offB, O, A, KP, NH, the algorithm and
//                   the device addresses of the member's obs / eps / act arrays -- read by the kernel with scalar loads
//                   from device memory, not over the link
//   the slab        ONE mapped pinned allocation: the control block ActCtl (256 B), then per member obs (max_rows, O)
//                   FLOAT64, eps (max_rows, A) fp32, act (max_rows, A) fp32, each 256-byte aligned and fixed for the
//                   session's life.  The caller writes observations and eps THERE and reads actions THERE: a call copies
//                   nothing.
//
// A call (sac_actor_act) drains the members with rows (sac_sync: a fused step that gave up is recovered), rewrites the
// control block -- per member {first workgroup, rows, stochastic} -- launches k_act_session once on member 0's stream
// and waits for one event of its own.  The control block is the only thing the kernel reads over the link in front of
// the observations: three 64-byte scalar loads, issued together.  Like k_act the launch goes on member 0's stream even
// when member 0 sits out and so was not drained: the tick then queues behind member 0's steps in flight (the result is
// the same; a caller that wants the short latency keeps a member with rows in front).
//
// Behind its prologue k_act_session calls what k_act (sac_act.h) calls, the pieces of sac_infer.h, on the same workgroup
// mapping and LDS layout: a session's actions are bit for bit sac_policy_act_device's.  The observations are float64 in
// the slab (what the environments produce) and rounded to fp32 as infer_fill loads them: a plain cast, round to nearest
// even, the value of numpy's astype(float32) and of sac_buffer_add_f64.
//
// Net::P and the layer offsets.  A fused-shape trainer's networks live in its arena, allocated and laid out once in
// trainer_build; no step path (the four-launch step, the fused step and its fall-back, the chained steps, the group
// loops), no sac_set_params / sac_set_opt_state and no checkpoint load allocates, frees or re-lays them: all of them
// write INTO Net::P.  The table is therefore valid for the trainer handle's life, and sac_actor_act only asserts that
// (one pointer compare per member).  What does end a table entry is the end of the handle itself: the members must
// outlive the session (the Python GroupActor reopens its sessions when a trainer replaces its handle).
#pragma once

namespace sac {

struct ActEntry {                  // static, device memory
    const float *P;                // the policy's forward copy (Net::P)
    const double *obs;             // (max_rows, O) row-major, float64: device address inside the slab
    const float *eps;              // (max_rows, A)
    float *act;                    // (max_rows, A)
    long long offW[3], offB[3];    // the three layers inside P
    int O, A, KP, NH;              // NH: padded head rows (SAC: mean + log_std; TD3: last_fc)
    int algo, pad;                 // 0 SAC, 1 TD3
};

struct ActCtl {                    // per call, at the head of the slab (256 B)
    int rb0[SAC_GROUP_MAX];        // first workgroup of member i in this launch (members beyond the session's, and those
                                   // behind the last one with rows: the launch's workgroup count)
    int n[SAC_GROUP_MAX];          // rows of member i (0: sits out)
    int stochastic[SAC_GROUP_MAX]; // 1: SAC with exploration noise
    int pad[SAC_GROUP_MAX];
};

typedef int i32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void k_act_session(const ActEntry *__restrict__ tab, const ActCtl *__restrict__ ctl) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // this workgroup's member: the last one whose first workgroup is not behind this one.  Both arrays come over the
    // link in one go (wave-uniform: three 16-dword scalar loads); a member that sits out shares its first workgroup with
    // the next one and is passed over.
    const i32x16 rb0s = sload(reinterpret_cast<const i32x16 *>(ctl->rb0));
    const i32x16 ns = sload(reinterpret_cast<const i32x16 *>(ctl->n));
    const i32x16 sts = sload(reinterpret_cast<const i32x16 *>(ctl->stochastic));
    int mi = 0, rb0 = rb0s[0], n = ns[0], stochastic = sts[0];
#pragma unroll
    for (int i = 1; i < SAC_GROUP_MAX; ++i)
        if ((int)blockIdx.x >= rb0s[i]) { mi = i; rb0 = rb0s[i]; n = ns[i]; stochastic = sts[i]; }
    const ActEntry *M = tab + mi;
    const float *P = sload(&M->P);
    const int O = sload(&M->O), A = sload(&M->A), KP = sload(&M->KP), NH = sload(&M->NH);
    const int row0 = ((int)blockIdx.x - rb0) * RB;
    const int KL0 = (KP + 63) & ~63;
    float *X0 = lds;                     // [16][KL0]
    float *X1 = X0 + RB * KL0;           // [16][256]
    float *X2 = X1 + RB * H;             // [16][256]
    float *HL = X2 + RB * H;             // [16][32]
    // (the observations are float64 in the slab: infer_fill rounds them)
    infer_hidden(P, M->offW, M->offB, X0, KL0, KP, X1, X2, [&] { infer_fill(X0, KL0, row0, n, sload(&M->obs), O); });
    infer_head(P, M->offW, M->offB, NH, X2, HL);
    const int r = threadIdx.x >> 4, a = threadIdx.x & 15;
    if (a < A && row0 + r < n) {
        const size_t o = (size_t)(row0 + r) * A + a;
        sload(&M->act)[o] = infer_action(HL, r, a, A, stochastic != 0, [&] { return sload(&M->eps)[o]; });
    }
}

}  // namespace sac

struct sac_actor {
    int device = 0, n = 0;
    sac_trainer *member[SAC_GROUP_MAX] = {};
    int max_rows[SAC_GROUP_MAX] = {};
    char *slab_h = nullptr, *slab_d = nullptr;         // the mapped pinned slab: host view, device view
    size_t off[SAC_GROUP_MAX][3] = {};                 // obs / eps / act of member i inside the slab
    ActEntry tab[SAC_GROUP_MAX] = {};                  // host copy of the device table
    ActEntry *d_tab = nullptr;
    hipEvent_t ev = nullptr;                           // the one event a call waits for
};

namespace {

// k_act_session may use more than 48 KB of LDS on this device (set once, by the first session with wide observations)
std::atomic<bool> g_session_lds_raised[64];

void actor_entry(const sac_actor *a, int i, ActEntry &E) {
    const sac_trainer *t = a->member[i];
    const Net &N = t->net[SAC_NET_POLICY];
    E = ActEntry{};
    E.P = N.P;
    E.obs = reinterpret_cast<const double *>(a->slab_d + a->off[i][0]);
    E.eps = reinterpret_cast<const float *>(a->slab_d + a->off[i][1]);
    E.act = reinterpret_cast<float *>(a->slab_d + a->off[i][2]);
    for (int l = 0; l < 3; ++l) { E.offW[l] = N.L[l].offW; E.offB[l] = N.L[l].offB; }
    E.O = t->O; E.A = t->A; E.KP = t->KP; E.NH = t->NH;
    E.algo = t->algo;
}

// the session's allocations: the slab, the device table (written here, once), the event, the kernel's LDS attribute
int actor_build(sac_actor *a, size_t bytes, int kp_max) {
    SAC_HIP(hipSetDevice(a->device));
    SAC_HIP(hipHostMalloc(reinterpret_cast<void **>(&a->slab_h), bytes, hipHostMallocMapped));
    SAC_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&a->slab_d), a->slab_h, 0));
    memset(a->slab_h, 0, bytes);
    SAC_HIP(hipMalloc(reinterpret_cast<void **>(&a->d_tab), sizeof(a->tab)));
    for (int i = 0; i < a->n; ++i) actor_entry(a, i, a->tab[i]);
    SAC_HIP(hipMemcpy(a->d_tab, a->tab, sizeof(a->tab), hipMemcpyHostToDevice));
    SAC_HIP(hipEventCreateWithFlags(&a->ev, hipEventDisableTiming));
    if (infer_raise_lds(reinterpret_cast<const void *>(k_act_session), g_session_lds_raised, a->device, act_lds_bytes(kp_max),
                        act_lds_bytes(512))) return -1;
    return 0;
}

int actor_free(sac_actor *a) {
    (void)hipSetDevice(a->device);
    if (a->ev) (void)hipEventDestroy(a->ev);
    if (a->d_tab) (void)hipFree(a->d_tab);
    if (a->slab_h) (void)hipHostFree(a->slab_h);
    delete a;
    return 0;
}

}  // namespace

// (declared extern "C" in include/sac_hip.h)
int sac_actor_create(sac_actor_t **out, sac_trainer_t *const *trainers, int n_trainers, const int32_t *max_rows) {
    SAC_REQUIRE(out, "null out pointer to sac_actor_create");
    *out = nullptr;
    SAC_REQUIRE(trainers && max_rows, "bad arguments to sac_actor_create");
    const InferEntry E = {"sac_actor_create", false, false, "device acting", "sac_policy_act is the acting path", "act on"};
    if (int rc = infer_admit_session(E, trainers, n_trainers, max_rows)) return rc;
    sac_actor *a = new sac_actor;
    a->device = trainers[0]->device;
    a->n = n_trainers;
    const size_t bytes = infer_slab(sizeof(ActCtl), trainers, n_trainers, max_rows, a->off);
    int kp_max = 0;
    for (int i = 0; i < n_trainers; ++i) {
        a->member[i] = trainers[i];
        a->max_rows[i] = max_rows[i];
        kp_max = std::max(kp_max, trainers[i]->KP);
    }
    if (actor_build(a, bytes, kp_max)) { actor_free(a); return -1; }
    *out = a;
    return 0;
}

int sac_actor_destroy(sac_actor_t *a) {
    if (!a) return 0;
    return actor_free(a);
}

int sac_actor_arrays(sac_actor_t *a, int member, double **obs, float **eps, float **act) {
    SAC_REQUIRE(a, "null acting session");
    SAC_REQUIRE(member >= 0 && member < a->n, "sac_actor_arrays: member %d of %d", member, a->n);
    infer_slab_arrays(a->slab_h, a->off[member], obs, eps, act);
    return 0;
}

int sac_actor_act(sac_actor_t *a, const int32_t *n_rows, const int32_t *deterministic) {
    SAC_REQUIRE(a && n_rows && deterministic, "bad arguments to sac_actor_act");
    // every refusal comes first: nothing has changed when one of them returns
    int active = 0;
    for (int i = 0; i < a->n; ++i) {
        SAC_REQUIRE(a->member[i]->xcd_mask == 0xffu, "trainer %d is confined by sac_trainer_set_xcd[_mask]: device acting launches "
                    "on the whole chip", i);
        SAC_REQUIRE(n_rows[i] >= 0 && n_rows[i] <= a->max_rows[i], "trainer %d: %d rows (0..%d in this session, 0 = sits out)", i,
                    (int)n_rows[i], a->max_rows[i]);
        SAC_REQUIRE(a->member[i]->net[SAC_NET_POLICY].P == a->tab[i].P, "internal: the policy of trainer %d has moved under its "
                    "acting session", i);
        active += n_rows[i] > 0;
    }
    SAC_REQUIRE(active > 0, "no trainer has rows to act on");
    sac_trainer *t0 = a->member[0];
    SAC_HIP(hipSetDevice(a->device));
    // the weights as of the last completed step: drain every member, re-run what a fused step that gave up left undone
    for (int i = 0; i < a->n; ++i)
        if (n_rows[i] > 0 && sac_sync(a->member[i])) return -1;
    ActCtl *ctl = reinterpret_cast<ActCtl *>(a->slab_h);
    int blocks = 0, kp_max = 0;
    for (int i = 0; i < a->n; ++i) {
        const sac_trainer *t = a->member[i];
        ctl->rb0[i] = blocks;
        ctl->n[i] = n_rows[i];
        ctl->stochastic[i] = (t->algo == 0 && !deterministic[i]) ? 1 : 0;
        if (n_rows[i] == 0) continue;
        blocks += (n_rows[i] + RB - 1) / RB;
        kp_max = std::max(kp_max, t->KP);
    }
    for (int i = a->n; i < SAC_GROUP_MAX; ++i) { ctl->rb0[i] = blocks; ctl->n[i] = 0; ctl->stochastic[i] = 0; }
    hipLaunchKernelGGL(k_act_session, dim3(blocks), dim3(256), act_lds_bytes(kp_max), t0->stream, a->d_tab,
                       reinterpret_cast<const ActCtl *>(a->slab_d));
    SAC_HIP(hipGetLastError());
    SAC_HIP(hipEventRecord(a->ev, t0->stream));
    return wait_event(a->ev);
}
