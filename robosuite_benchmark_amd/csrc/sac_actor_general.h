// Acting sessions for general-step trainers: sac_policy_act_general_many without the per-call marshalling (included by
// sac_trainer.hip behind sac_act_general.h).
//
// A session (sac_gactor) is made once for a fixed list of general-step trainers.  What never changes between two ticks
// is written once, at creation:
//
//   device memory   the job table GActJob[GMAXL][SAC_GROUP_MAX]: slot [l][i] is member i's layer l -- the LayerJob that
//                   LayerSchedule::chain (sac_infer.h) writes for sac_policy_act_general_many, on the slab and the
//                   session's scratch; a SAC head's kind is its static part.  GActJob stays a struct of its own around
//                   it: the table is indexed by member and never rewritten, the per-call part (rows, stochastic, wg0)
//                   is GActCtl.  A member shallower than l has no job there (live == 0).
//   scratch         two ping-pong activation buffers per member, max_rows x its widest hidden layer each, owned by the
//                   SESSION: the trainer's act_gen buffers (sac_infer.h) may be freed and reallocated by
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
// Behind its prologue k_act_layer_session runs k_act_layer's frame (infer_layer_frame<T, false, LayerHead<false>> of
// sac_infer.h) on a job the same builder wrote: a session's actions are bit for bit sac_policy_act_general's.  The
// prologue reads the launch's wg0 row, n and stochastic with three 16-dword scalar loads issued together, picks the
// member with scalar compares and reads that member's static job from device memory.  In launch 0 (template parameter
// F64) the input rows are float64 in the slab (infer_layer_tile<double, false>) and are rounded to fp32 on the way into
// LDS: a plain cast, round to nearest even, the value of numpy's astype(float32).  The fp32 instance is k_act_layer's.
//
// GenNet::P and the layer offsets.  A general-step trainer's networks live in sac_general::arena, which
// gen_build / gen_build_td3 (sac_general_host.h) allocate once and carve with the trainer's Arena; param_shape
// (sac_param_map.h), the only writer of offW / offB, runs in their opening (gen_open) and nowhere else.  No general step path, no group loop (MLP and arch groups
// launch on the members' own tables), no sac_set_params / sac_set_opt_state / sac_set_scalars and no checkpoint load
// allocates, frees or re-lays the arena: all of them write INTO GenNet::P.  The table is therefore valid for the trainer
// handle's life and sac_gactor_act only asserts that (one pointer compare per member).  What does end a table entry is
// the end of the handle itself: the members must outlive the session (the Python GroupActor reopens its sessions when a
// trainer replaces its handle).
#pragma once

namespace sac {

struct GActJob {                   // static, device memory: member i's layer l
    LayerJob J;                    // X: the slab's FLOAT64 obs for l == 0; a SAC head says LAYER_SAC_MEAN (the call's flag makes
                                   // it LAYER_SAC_SAMPLE); n and wg0 are unused (the control block has the call's)
    int live, pad;                 // 0: the member has no layer l
};

struct GActCtl {                   // per call, at the head of the slab
    int n[SAC_GROUP_MAX];          // rows of member i (0: sits out)
    int stochastic[SAC_GROUP_MAX]; // 1: SAC with exploration noise
    int wg0[gen::GMAXL][SAC_GROUP_MAX];   // first workgroup of member i in launch l (members without rows or without a
                                          // layer l share theirs with the next member; behind the last: the grid size)
};

template <bool F64>
__global__ __launch_bounds__(256) void k_act_layer_session(const GActJob *__restrict__ tab, const GActCtl *__restrict__ ctl, int l) {
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
    const LayerJob *J = &tab[mi].J;
    const int kind_s = sload(&J->kind);
    infer_layer_frame<xin_t, false, LayerHead<false>>(J, wg0, n, (kind_s == LAYER_SAC_MEAN && stochastic) ? LAYER_SAC_SAMPLE : kind_s);
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

// the session's allocations: the slab, the scratch, the device table (written here, once), the event
int gactor_build(sac_gactor *a, size_t slab_bytes) {
    SAC_HIP(hipSetDevice(a->device));
    SAC_HIP(hipHostMalloc(reinterpret_cast<void **>(&a->slab_h), slab_bytes, hipHostMallocMapped));
    SAC_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&a->slab_d), a->slab_h, 0));
    memset(a->slab_h, 0, slab_bytes);
    size_t buf[SAC_GROUP_MAX], floats = 0;             // floats of ONE of member i's two buffers (a multiple of 64)
    for (int i = 0; i < a->n; ++i) {
        buf[i] = ((size_t)a->max_rows[i] * infer_widest(a->member[i]->gen->net[SAC_NET_POLICY]) + 63) & ~(size_t)63;
        floats += 2 * buf[i];
    }
    SAC_HIP(hipMalloc(reinterpret_cast<void **>(&a->scratch), sizeof(float) * floats));
    // the static table through the schedule builder: its own table is thrown away, each job goes to its member's slot
    std::vector<LayerJob> jobs((size_t)SAC_GROUP_MAX * gen::GMAXL);
    LayerSchedule LS(SAC_GROUP_MAX);
    LS.bind(jobs.data(), nullptr);
    float *next = a->scratch;
    for (int i = 0; i < a->n; ++i) {
        const sac_trainer *t = a->member[i];
        const GenNet &P = t->gen->net[SAC_NET_POLICY];
        float *pp[2] = {next, next + buf[i]};
        next += 2 * buf[i];
        a->P[i] = P.P;
        const float *x = reinterpret_cast<const float *>(a->slab_d + a->off[i][0]);        // (float64 rows: GActJob)
        LS.chain({P, x, x, P.L[0].K, a->max_rows[i], pp, 0, reinterpret_cast<float *>(a->slab_d + a->off[i][2])},
                 [&](LayerJob &J, int l) {
            if (l + 1 == P.nl) {
                J.kind = t->algo == 1 ? LAYER_TD3 : LAYER_SAC_MEAN;
                J.eps = reinterpret_cast<const float *>(a->slab_d + a->off[i][1]); J.A = t->A;
            }
            a->tab[l][i].J = J;
            a->tab[l][i].live = 1;
        });
    }
    a->launches = LS.launches;
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
    const InferEntry E = {"sac_gactor_create", true, false, "device acting",
                          "sac_actor_create makes its acting sessions, sac_gactor_create serves the general step", "act on"};
    if (int rc = infer_admit_session(E, trainers, n_trainers, max_rows)) return rc;
    sac_gactor *a = new sac_gactor;
    a->device = trainers[0]->device;
    a->n = n_trainers;
    const size_t bytes = infer_slab(sizeof(GActCtl), trainers, n_trainers, max_rows, a->off);
    for (int i = 0; i < n_trainers; ++i) {
        a->member[i] = trainers[i];
        a->max_rows[i] = max_rows[i];
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
    infer_slab_arrays(a->slab_h, a->off[member], obs, eps, act);
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
            if (rows && a->tab[l][i].live) blocks[l] += ((n_rows[i] + RB - 1) / RB) * a->tab[l][i].J.tiles_n;
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
