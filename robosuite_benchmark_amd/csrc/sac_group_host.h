// ==========================================================================================
// Trainer groups, host side: R SAC (or TD3) trainers stepped together in grouped launches.  Included by sac_trainer.hip
// inside its extern "C" block, behind everything it uses -- the grouped kernels are templates instantiated in that
// translation unit (GroupMember, Td3GroupStep, k_*_group there; gen::GenMember, gen::GenGroupStep, k_g_*_group in
// sac_general.h).
//
// Every kind of group is a STAGE LIST built at creation (GroupStage) and one loop that walks it:
//   * same-shape and mixed groups of the fused kernels' shapes (sac_group_create[_mixed], td3_group_create[_mixed]): the
//     members' four-launch step, read from the list the solo step walks (step_schedule, sac_step_plan.h) -- SAC: A, B, C,
//     dW; TD3: A, B, C, dW of the critic pass, then B, C, dW of the actor pass.  A, B, C go once per variant class (GroupClass: members of different dims and batches run different kernel
//     instances), the weight-gradient launch once for all members;
//   * MLP and arch groups (sac_group_create_mlp / _arch, td3_...): the merged schedule of the members' general-step
//     launch lists, one grouped launch per GEMM stage and one per class (or one for all) per elementwise stage.
// A stage carries its kernel, x-extent, LDS and block size, whether it goes per class, and when it runs (always / some
// member runs TD3's actor pass / some member is on a policy step).  The kernels take (member table, step table row,
// slot, one int) -- the GEMM stages their headers and block map in addition -- and are launched type-erased.
//
// The loop is sac_train_loop's for every member at once -- same index stream per buffer, same steps, same results bit
// for bit (every step's arguments come from step_arg / td3_plan, like the solo steps') -- without its latency devices
// (no speculative next chunk, no stepwise read-ahead): chunks of LOOP_CH steps alternate between the two halves of each
// buffer's loop slots; the draws (each member's batch) and gathers (one launch per NIT class) of a chunk run on the
// group's second stream under the steps of the previous one (unless the device's fused-launch gate is live -- another
// fused trainer or group on the device, fused members included: then every grouped launch, draws and gathers too, is
// serialised behind the gate's last launch, at a cost of ~0.3 ms per 256-step chunk).
// ==========================================================================================
#pragma once

// One variant class of a group: the members whose step runs the same instances of the grouped kernels, a contiguous
// range of the device tables.  A group of one shape is one class; a mixed group has up to four (by the (nth, wide) of
// its members' step plans), an MLP or arch group up to two (by the elementwise kernels' action bound).
struct GroupClass {
    int lo = 0, n = 0;                                // device table entries lo .. lo + n - 1
    int ma = 0;                                       // MLP groups: the action bound of the class's elementwise kernels (8 / 16)
};

// One grouped stage of a step.  per_class: one launch per variant class c -- kernel fn[c] on gx[c] x (class size)
// workgroups with lds[c] bytes, over the class's range of the member and step tables; else one launch fn[0], gx[0] x R,
// over all members.  A GEMM stage (hdr >= 0) is one flat launch of gx[0] blocks: `map` is its block -> member prefix
// table, its members' stage headers are d_hdr[hdr R .. hdr R + R - 1].
struct GroupStage {
    const void *fn[4] = {};
    int gx[4] = {};                                   // the largest extent among the members served
    size_t lds[4] = {};                               // the largest dynamic LDS among them
    int block = 256;
    bool per_class = false;
    int need = 0;                                     // runs on a step where: 0 always, 1 some member runs the actor pass, 2 some member is on a policy step (TD3)
    bool idle_one = false;                            // TD3 actor weight gradients: 1 block per member (statistics only) unless some member is on a policy step
    bool ends_only = false;                           // SAC general-step diagnostics: on the call's first and last step only
    int arg = 0;                                      // the kernel's last argument: k_bwd_group's `compact` / an elementwise stage's gen::GSEL_*
    int hdr = -1;
    gen::GemmGroupMap map{};
};

// the host fills one step row for every kind; a TD3 group's rows are Td3GroupStep, a fused SAC group's the leading StepArg
static_assert(sizeof(Td3GroupStep) == sizeof(gen::GenGroupStep) && offsetof(Td3GroupStep, sq) == offsetof(gen::GenGroupStep, sa) &&
              offsetof(Td3GroupStep, sp) == offsetof(gen::GenGroupStep, sp) && offsetof(Td3GroupStep, actor) == offsetof(gen::GenGroupStep, actor) &&
              offsetof(Td3GroupStep, pstep) == offsetof(gen::GenGroupStep, pstep) && offsetof(gen::GenGroupStep, sa) == 0,
              "Td3GroupStep and gen::GenGroupStep share one host image");

struct sac_group {
    int R = 0, device = 0, algo = 0;                  // algo: 0 SAC, 1 TD3 (every member's)
    bool mixed = false;                               // sac_group_create_mixed / td3_group_create_mixed
    bool mlp = false;                                 // sac_group_create_mlp / _arch, td3_...: general-step members
    sac_trainer *m[SAC_GROUP_MAX] = {};
    int ord[SAC_GROUP_MAX] = {};                      // device table entry k (member and step tables) is member ord[k]
    int ncls = 0;
    GroupClass cls[4];
    std::vector<GroupStage> stages;                   // one full step, in launch order
    hipStream_t s = nullptr, s2 = nullptr;           // steps / draws + gathers
    hipEvent_t ev_ready[2] = {}, ev_done[2] = {}, ev_copied[2] = {}, ev_end = nullptr;
    hipEvent_t ev_in[2 * SAC_GROUP_MAX] = {};         // the members' and the buffers' streams in front of a call
    // device tables and their pinned host images: members [R] of mem_bytes each (device order; GroupMember, or
    // gen::GenMember in MLP groups) at the front | draws | gathers | steps
    char *d_tab = nullptr, *h_tab = nullptr;
    size_t mem_bytes = 0;
    SampleMember *d_smp = nullptr, *h_smp = nullptr;  // [2 halves][R] (member order)
    GatherMember *d_gat = nullptr, *h_gat = nullptr;  // [2 halves][R] (sorted by gather class, per call)
    // steps [2 halves][LOOP_CH steps][R] (device order) of step_bytes each: StepArg (fused SAC), Td3GroupStep (fused TD3),
    // gen::GenGroupStep (MLP groups)
    char *d_step = nullptr, *h_step = nullptr;
    size_t step_bytes = 0;
    gen::GemmStage *d_hdr = nullptr;                  // MLP groups: the members' GEMM stage headers [GEMM stage][R], written at creation
};

static void group_free(sac_group *g) {
    if (g->s) (void)hipStreamSynchronize(g->s);
    if (g->s2) (void)hipStreamSynchronize(g->s2);
    for (auto &e : g->ev_ready) if (e) (void)hipEventDestroy(e);
    for (auto &e : g->ev_done) if (e) (void)hipEventDestroy(e);
    for (auto &e : g->ev_copied) if (e) (void)hipEventDestroy(e);
    for (auto &e : g->ev_in) if (e) (void)hipEventDestroy(e);
    if (g->ev_end) (void)hipEventDestroy(g->ev_end);
    if (g->d_tab) (void)hipFree(g->d_tab);
    if (g->d_hdr) (void)hipFree(g->d_hdr);
    if (g->h_tab) (void)hipHostFree(g->h_tab);
    if (g->s) (void)hipStreamDestroy(g->s);
    if (g->s2) (void)hipStreamDestroy(g->s2);
    delete g;
}

// what a member must be (checked at creation and again in front of every call: a member may have been confined since)
static int group_member_ok(const sac_trainer *t, int i, int algo, bool mlp = false) {
    if (algo == 0) SAC_REQUIRE(t->algo == 0, "trainer group member %d is a TD3 trainer: groups hold SAC trainers only", i);
    else SAC_REQUIRE(t->algo == 1, "trainer group member %d is a SAC trainer: TD3 groups hold TD3 trainers only", i);
    if (mlp) {
        SAC_REQUIRE(t->gen, "trainer group member %d has the shapes of the fused kernels (two hidden layers of at most 256 "
                    "units): MLP groups take general-step members only", i);
        SAC_REQUIRE(t->xcd_mask == 0xffu, "trainer group member %d is confined to XCDs (sac_trainer_set_xcd[_mask]): a group "
                    "spans the whole chip", i);
        return 0;
    }
    SAC_REQUIRE(!t->gen, "trainer group member %d runs the general step (hidden sizes beyond two layers of at most 256 units): "
                "groups take the shapes of the fused kernels only", i);
    SAC_REQUIRE(t->Bt <= 256, "trainer group member %d has batch %d: groups take batches of at most 256 rows", i, t->Bt);
    SAC_REQUIRE(t->xcd_mask == 0xffu, "trainer group member %d is confined to XCDs (sac_trainer_set_xcd[_mask]): a group spans "
                "the whole chip", i);
    SAC_REQUIRE(t->plan.SP == 4 && !t->plan.chain && !t->plan.bwd8, "trainer group member %d runs column split %d: groups take the "
                "default split 4 only", i, t->plan.SP);
    return 0;
}

// members of one variant class run the same instances of the step kernels (the column split is 4: group_member_ok)
static bool same_variant(const sac_trainer *a, const sac_trainer *b) {
    return a->plan.nth == b->plan.nth && a->plan.wide == b->plan.wide;
}

// a group's tables (device, with their pinned host images: members | draws | gathers | steps), its two streams, its
// events, and its tenancy of the device's fused-launch gate
static int group_tables(sac_group *g, size_t mem_bytes, size_t step_bytes) {
    const int R = g->R;
    g->mem_bytes = mem_bytes; g->step_bytes = step_bytes;
    const size_t b_mem = mem_bytes * R, b_sa = step_bytes * 2 * LOOP_CH * R;
    const size_t b_smp = sizeof(SampleMember) * 2 * R, b_gat = sizeof(GatherMember) * 2 * R;
    const size_t o_smp = (b_mem + 255) & ~(size_t)255, o_gat = o_smp + ((b_smp + 255) & ~(size_t)255);
    const size_t o_sa = o_gat + ((b_gat + 255) & ~(size_t)255), total = o_sa + b_sa;
    if (hipMalloc(reinterpret_cast<void **>(&g->d_tab), total) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&g->h_tab), total, hipHostMallocDefault) != hipSuccess ||
        hipStreamCreateWithFlags(&g->s, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&g->s2, hipStreamNonBlocking) != hipSuccess) {
        sac::set_error("out of device or pinned host memory for a trainer group");
        return -1;
    }
    for (int k = 0; k < 2; ++k)
        if (hipEventCreateWithFlags(&g->ev_ready[k], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&g->ev_done[k], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&g->ev_copied[k], hipEventDisableTiming) != hipSuccess) {
            sac::set_error("hipEventCreate failed");
            return -1;
        }
    for (auto &e : g->ev_in)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { sac::set_error("hipEventCreate failed"); return -1; }
    if (hipEventCreateWithFlags(&g->ev_end, hipEventDisableTiming) != hipSuccess) { sac::set_error("hipEventCreate failed"); return -1; }
    g->d_smp = reinterpret_cast<SampleMember *>(g->d_tab + o_smp); g->h_smp = reinterpret_cast<SampleMember *>(g->h_tab + o_smp);
    g->d_gat = reinterpret_cast<GatherMember *>(g->d_tab + o_gat); g->h_gat = reinterpret_cast<GatherMember *>(g->h_tab + o_gat);
    g->d_step = g->d_tab + o_sa; g->h_step = g->h_tab + o_sa;
    // a tenant of the device's fused-launch gate: no fused trainer's launch may overlap the group's grids
    if (gate_join(g->device)) { sac::set_error("hipEventCreate failed"); return -1; }
    return 0;
}

// A member of a same-shape or mixed group against member 0.  Two parts, because the refusal a caller gets for a group
// with several faults follows the order of the checks: these come in front of the device check ...
static int fused_member_shape(const sac_trainer *t, const sac_trainer *t0, int i, bool mixed) {
    if (!mixed) {
        SAC_REQUIRE(t->O == t0->O && t->A == t0->A, "trainer group member %d has dims (%d,%d), member 0 (%d,%d)", i, t->O,
                    t->A, t0->O, t0->A);
        SAC_REQUIRE(t->Bt == t0->Bt, "trainer group member %d has batch %d, member 0 %d", i, t->Bt, t0->Bt);
    }
    SAC_REQUIRE(t->HP[0] == t0->HP[0] && t->HP[1] == t0->HP[1] && t->HQ[0] == t0->HQ[0] && t->HQ[1] == t0->HQ[1],
                "trainer group member %d has hidden sizes policy [%d,%d] qf [%d,%d], member 0 policy [%d,%d] qf [%d,%d]", i,
                t->HP[0], t->HP[1], t->HQ[0], t->HQ[1], t0->HP[0], t0->HP[1], t0->HQ[0], t0->HQ[1]);
    return 0;
}

// ... and these behind it
static int fused_member_kernels(const sac_trainer *t, const sac_trainer *t0, int i, bool mixed) {
    if (!mixed)
        SAC_REQUIRE(same_variant(t, t0) && t->dw.njobs == t0->dw.njobs, "trainer group member %d runs another kernel "
                    "variant than member 0", i);
    SAC_REQUIRE(t->A <= 16 && 3 * 4 * t->NB <= 192, "trainer group member %d: act_dim %d / batch %d outside the grouped "
                "kernels", i, t->A, t->Bt);
    return 0;
}

// the grouped instance of an elementwise stage of the general step (ma: the class's action bound; 0: a kernel without one)
typedef void (*GenSmallFn)(const gen::GenMember *, const gen::GenGroupStep *, int, int);
static GenSmallFn gen_small_fn(int kind, int ma) {
#define GEN_SMALL(K) (ma == 16 ? &gen::k_g_small_group<gen::K, 16> : &gen::k_g_small_group<gen::K, 8>)
    switch (kind) {
    case GS_HEAD: return GEN_SMALL(GK_HEAD);
    case GS_POLGRAD: return GEN_SMALL(GK_POLGRAD);
    case GS_TD3_HEAD: return GEN_SMALL(GK_TD3_HEAD);
    case GS_TD3_AHEAD: return GEN_SMALL(GK_TD3_AHEAD);
    case GS_TD3_POLGRAD: return GEN_SMALL(GK_TD3_POLGRAD);
    case GS_LOSS: return &gen::k_g_small_group<gen::GK_LOSS, 0>;
    case GS_DIAG: return &gen::k_g_small_group<gen::GK_DIAG, 0>;
    case GS_TD3_LOSS: return &gen::k_g_small_group<gen::GK_TD3_LOSS, 0>;
    case GS_TD3_QA: return &gen::k_g_small_group<gen::GK_TD3_QA, 0>;
    }
#undef GEN_SMALL
    return nullptr;
}

// an elementwise stage's x-extent for a member of batch n (gen_run_list's grid)
static int gen_small_extent(int kind, int n) {
    switch (kind) {
    case GS_HEAD: return (2 * n + gen::GRW - 1) / gen::GRW;
    case GS_LOSS: case GS_TD3_LOSS: case GS_TD3_QA: return n;
    case GS_DIAG: return 1;
    default: return (n + gen::GRW - 1) / gen::GRW;
    }
}

// A member's launch list as a skeleton: its plain (elementwise) stages in order, and in front of each of them -- and
// behind the last -- its GEMM stages as three equal-mode sub-runs in the fixed order forward (0), backward (1), weight
// gradients (2), each in list order; a sub-run may be empty (e.g. no backward launch of the policy at Lp = 1).  false:
// the list does not have that form (a GEMM stage of a lower mode behind a higher one in the same gap).
struct GenSkeleton {
    std::vector<int> plain;                                    // list indices of the plain stages
    std::vector<std::array<std::vector<int>, 3>> runs;        // runs[p][mode]: list indices in front of plain stage p
};
static bool gen_skeleton(const std::vector<GenStage> &L, GenSkeleton &S) {
    S.plain.clear();
    S.runs.assign(1, {});
    int last = 0;
    for (size_t k = 0; k < L.size(); ++k) {
        if (L[k].kind != GS_GEMM) {
            S.plain.push_back((int)k);
            S.runs.emplace_back();
            last = 0;
            continue;
        }
        if (L[k].mode < last || L[k].mode > 2) return false;
        last = L[k].mode;
        S.runs.back()[L[k].mode].push_back((int)k);
    }
    return true;
}

// what a member of an MLP group must share with member 0 (an arch group's members: nothing but the device)
static int mlp_member_shape(const sac_trainer *t, const sac_trainer *t0, int i, bool arch) {
    if (arch) return 0;
    const sac_general *a = t->gen, *b = t0->gen;
    bool same = a->Lp == b->Lp && a->Lq == b->Lq;
    for (int l = 0; same && l < a->Lp; ++l) same = a->hp[l] == b->hp[l];
    for (int l = 0; same && l < a->Lq; ++l) same = a->hq[l] == b->hq[l];
    SAC_REQUIRE(same, "trainer group member %d has other hidden sizes than member 0 (an MLP group shares them)", i);
    return 0;
}

// MLP groups (members of the general step with one set of hidden sizes) and arch groups (any hidden sizes of the
// general step).  Both walk the merged schedule of the members' launch lists: the plain stages in order, every member in
// each; at each GEMM sub-run the largest count over the members of grouped launches, member m in the first count_m of
// them and with zero blocks in the rest.  Each member thus runs its own stages in its own order, each with its own
// header (jobs, tiles, split factor, scratch, counters): what its solo launch list runs.  Members of one set of hidden
// sizes have one list shape, and the merged schedule is their list.
static int group_build_mlp(sac_group *g) {
    const int R = g->R, algo = g->algo;
    sac_trainer *const *members = g->m;
    const sac_trainer *t0 = members[0];
    // the members' launch lists (SAC: the step; TD3: the critic pass, then the actor pass, whose statistics-only form is
    // its head up to the Q1 last layer), each as its skeleton: one sequence of plain stages for all of them (same
    // algorithm), checked, not assumed
    auto lists_of = [algo](const sac_trainer *t) {
        std::vector<const std::vector<GenStage> *> L;
        if (algo == 0) L.push_back(&t->gen->stages);
        else { L.push_back(&t->gen->td3_critic); L.push_back(&t->gen->td3_actor); }
        return L;
    };
    const size_t nlists = lists_of(t0).size();
    std::vector<std::vector<GenSkeleton>> sk(nlists, std::vector<GenSkeleton>((size_t)R));   // [list][member]
    for (int i = 0; i < R; ++i) {
        const auto L = lists_of(members[i]);
        for (size_t q = 0; q < nlists; ++q) {
            SAC_REQUIRE(gen_skeleton(*L[q], sk[q][(size_t)i]), "internal: trainer group member %d has a launch list whose "
                        "GEMM stages are out of mode order", i);
            const GenSkeleton &a = sk[q][(size_t)i], &b = sk[q][0];
            bool same = a.plain.size() == b.plain.size();
            for (size_t k = 0; same && k < a.plain.size(); ++k) {
                const GenStage &x = (*L[q])[(size_t)a.plain[k]], &y = (*lists_of(t0)[q])[(size_t)b.plain[k]];
                same = x.kind == y.kind && x.mode == y.mode;
            }
            SAC_REQUIRE(same, "internal: trainer group member %d has another sequence of elementwise stages than member 0", i);
        }
    }
    // variant classes: the elementwise kernels' action bound (up to 8 actions, up to 16), each class in member order
    int pos = 0;
    for (int ma : {8, 16}) {
        GroupClass &K = g->cls[g->ncls];
        K.lo = pos; K.ma = ma;
        for (int i = 0; i < R; ++i)
            if ((members[i]->A <= 8) == (ma == 8)) g->ord[pos++] = i;
        K.n = pos - K.lo;
        if (K.n > 0) g->ncls += 1;
    }
    // the merged schedule and the GEMM stages' headers, [grouped GEMM stage][device member]; a member without a stage in
    // a grouped GEMM launch gets an inert header (no tiles, never read: it owns no block of that launch)
    const void *const gemm_fn[3] = {reinterpret_cast<const void *>(&gen::k_g_gemm_group<true, true>),      // by mode: forward,
                                    reinterpret_cast<const void *>(&gen::k_g_gemm_group<true, false>),     // backward,
                                    reinterpret_cast<const void *>(&gen::k_g_gemm_group<false, false>)};   // weight gradients
    std::vector<gen::GemmStage> hdr;
    gen::GemmStage inert;
    memset(&inert, 0, sizeof(inert));
    inert.splitk = 1;
    for (size_t li = 0; li < nlists; ++li) {
        const std::vector<GenStage> &L0 = *lists_of(t0)[li];
        const GenSkeleton &S0 = sk[li][0];
        bool past_qa = false;
        // TD3's actor pass: every member with `actor` up to Q1's last layer (whose backward half follows pstep), the
        // policy's backward pass and update for members on a policy step, the statistics behind them for all of `actor`
        auto sel_of = [&](int kind) {
            return li == 0 ? gen::GSEL_ALL : ((past_qa && kind != GS_DIAG) ? gen::GSEL_PSTEP : gen::GSEL_ACTOR);
        };
        auto need_of = [&](int sel) { return sel == gen::GSEL_PSTEP ? 2 : (li == 1 ? 1 : 0); };
        for (size_t p = 0; p < S0.runs.size(); ++p) {
            for (int mode = 0; mode < 3; ++mode) {
                size_t cnt = 0;
                for (int d = 0; d < R; ++d) cnt = std::max(cnt, sk[li][(size_t)g->ord[d]].runs[p][(size_t)mode].size());
                for (size_t c = 0; c < cnt; ++c) {
                    GroupStage st;
                    const int sel = sel_of(GS_GEMM);
                    st.fn[0] = gemm_fn[mode]; st.block = 64 * gen::GW; st.need = need_of(sel);
                    st.hdr = (int)(hdr.size() / R);
                    int at = 0;
                    for (int q = 0; q <= SAC_GROUP_MAX; ++q) st.map.start[q] = 1 << 30;
                    for (int d = 0; d < R; ++d) {
                        const sac_trainer *t = members[g->ord[d]];
                        const std::vector<int> &run = sk[li][(size_t)g->ord[d]].runs[p][(size_t)mode];
                        gen::GemmStage gs = inert;
                        if (c < run.size()) {
                            gs = (*lists_of(t)[li])[(size_t)run[c]].gs;
                            gs.tau = t->gen->dev.tau;      // (gen_run_list sets it per launch; the rest per step, in the kernel)
                        }
                        hdr.push_back(gs);
                        st.map.start[d] = at;
                        at += gs.ntiles * gs.splitk;
                    }
                    st.map.sel = sel;
                    st.gx[0] = at;
                    g->stages.push_back(st);
                }
            }
            if (p == S0.plain.size()) break;
            const GenStage &s0 = L0[(size_t)S0.plain[p]];
            GroupStage st;
            st.arg = sel_of(s0.kind); st.need = need_of(st.arg);
            st.ends_only = s0.kind == GS_DIAG && algo == 0;
            if (s0.kind == GS_TD3_QA) past_qa = true;
            st.per_class = s0.kind == GS_HEAD || s0.kind == GS_POLGRAD || s0.kind == GS_TD3_HEAD || s0.kind == GS_TD3_AHEAD ||
                           s0.kind == GS_TD3_POLGRAD;
            for (int c = 0; c < (st.per_class ? g->ncls : 1); ++c) {
                const int lo = st.per_class ? g->cls[c].lo : 0, hi = st.per_class ? lo + g->cls[c].n : R;
                st.fn[c] = reinterpret_cast<const void *>(gen_small_fn(s0.kind, st.per_class ? g->cls[c].ma : 0));
                for (int d = lo; d < hi; ++d) st.gx[c] = std::max(st.gx[c], gen_small_extent(s0.kind, members[g->ord[d]]->Bt));
            }
            g->stages.push_back(st);
        }
    }
    if (hipMalloc(reinterpret_cast<void **>(&g->d_hdr), sizeof(gen::GemmStage) * hdr.size()) != hipSuccess ||
        hipMemcpy(g->d_hdr, hdr.data(), sizeof(gen::GemmStage) * hdr.size(), hipMemcpyHostToDevice) != hipSuccess) {
        sac::set_error("out of device memory for a trainer group");
        return -1;
    }
    return 0;
}

// Same-shape and mixed groups: the variant classes and the stage list of the members' four-launch step.
static int group_build_fused(sac_group *g) {
    const int R = g->R, algo = g->algo;
    // the variant classes (the (nth, wide) of a member's step plan), in order of first appearance; the device tables
    // hold them one after another, each in member order
    const sac_trainer *key[4] = {};
    for (int i = 0; i < R; ++i) {
        const sac_trainer *k = g->m[i];
        int c = 0;
        while (c < g->ncls && !same_variant(key[c], k)) ++c;
        if (c == g->ncls) {
            if (g->ncls == 4) { sac::set_error("internal: more than four kernel variants in a trainer group"); return -1; }
            key[g->ncls++] = k;
        }
    }
    // the classes' ranges of the device tables and their grouped kernel instances (step_kernels: a, b, c, b2, c2)
    StepKernels sk[4];
    int pos = 0;
    for (int c = 0; c < g->ncls; ++c) {
        GroupClass &K = g->cls[c];
        K.lo = pos;
        for (int i = 0; i < R; ++i)
            if (same_variant(g->m[i], key[c])) g->ord[pos++] = i;
        K.n = pos - K.lo;
        const StepPlan &P0 = key[c]->plan;
        sk[c] = step_kernels(P0.nth, P0.wide, 4, algo, P0.chain8, P0.wide4);
        if (!sk[c].group[0]) {
            sac::set_error("internal: no grouped instance of the members' step kernels");
            return -1;
        }
    }
    // the one-group form of the weight-gradient body where every member runs it solo (batch <= 256, not SAC_DW_FORM=loop)
    bool one = true;
    for (int i = 0; i < R; ++i) one = one && g->m[i]->plan.dw_one;
    auto dw_group = [one](int kernel) {
        auto fn = [](auto f) { return reinterpret_cast<const void *>(f); };
        if (kernel == SK_DW) return one ? fn(&k_dw_adam_group<M_SAC, true>) : fn(&k_dw_adam_group<M_SAC, false>);
        if (kernel == SK_DW_Q) return one ? fn(&k_dw_adam_group<M_TD3_CRITIC, true>) : fn(&k_dw_adam_group<M_TD3_CRITIC, false>);
        return one ? fn(&k_dw_adam_group<M_TD3_ACTOR, true>) : fn(&k_dw_adam_group<M_TD3_ACTOR, false>);
    };
    // The stage list is the members' four-launch schedule (sac_trainer::sched[0]: step_schedule(plan, false) as the solo
    // step walks it), the same for every member: A, B, C, B2, C2 once per class over the largest member extent and LDS,
    // a weight-gradient stage once for all members over the largest njobs + 1 of the tables it chooses between.
    const sac_trainer *t0 = g->m[0];
    for (int k = 0; k < t0->n_sched[0]; ++k) {
        const StepStage &s0 = t0->sched[0][k].st;
        GroupStage st;
        st.need = s0.need; st.block = s0.launch.threads;
        st.arg = std::max(s0.tail, 0);                // (launch C's `compact`; TD3's launch A reads "an actor pass follows" from its step row)
        st.per_class = s0.kernel <= SK_C2;
        st.idle_one = s0.kernel == SK_DW_PI;          // (off a policy step every member's table is dw_none: one block each)
        if (!st.per_class) st.fn[0] = dw_group(s0.kernel);
        for (int d = 0; d < R; ++d) {
            const sac_trainer *t = g->m[g->ord[d]];
            SAC_REQUIRE(t->n_sched[0] == t0->n_sched[0], "internal: trainer group member %d has another step schedule than member 0", g->ord[d]);
            const sac_trainer::Stage &ms = t->sched[0][k];
            SAC_REQUIRE(ms.st.kernel == s0.kernel && ms.st.need == s0.need && ms.st.arg == s0.arg && ms.st.tail == s0.tail,
                        "internal: trainer group member %d has another step schedule than member 0", g->ord[d]);
            int c = 0;
            while (st.per_class && !(d >= g->cls[c].lo && d < g->cls[c].lo + g->cls[c].n)) ++c;
            if (st.per_class) {
                st.fn[c] = sk[c].group[s0.kernel];
                st.gx[c] = std::max(st.gx[c], ms.st.launch.grid);
                st.lds[c] = std::max(st.lds[c], ms.st.launch.lds);
            } else st.gx[0] = std::max(st.gx[0], std::max(ms.tab[0]->njobs, ms.tab[1]->njobs) + 1);
        }
        g->stages.push_back(st);
    }
    for (const GroupStage &st : g->stages)
        for (int c = 0; c < 4; ++c)
            if (st.fn[c] && st.lds[c] > 64 * 1024 &&
                hipFuncSetAttribute(st.fn[c], hipFuncAttributeMaxDynamicSharedMemorySize, (int)st.lds[c]) != hipSuccess) {
                sac::set_error("hipFuncSetAttribute failed for the grouped step kernels");
                return -1;
            }
    return 0;
}

// Creation, every kind: the refusals (each member in turn: the checks of all kinds, its kind's shape checks, the device,
// its kind's kernel checks), the group, its kind's classes and stage list, its tables.
enum { GROUP_SAME = 0, GROUP_MIXED = 1, GROUP_MLP = 2, GROUP_ARCH = 3 };
static int group_create(sac_group_t **out, sac_trainer_t *const *members, int n_members, int algo, int kind) {
    static const char *const fname[2][4] = {
        {"sac_group_create", "sac_group_create_mixed", "sac_group_create_mlp", "sac_group_create_arch"},
        {"td3_group_create", "td3_group_create_mixed", "td3_group_create_mlp", "td3_group_create_arch"}};
    const bool mlp = kind == GROUP_MLP || kind == GROUP_ARCH, mixed = kind == GROUP_MIXED;
    SAC_REQUIRE(out && members, "null argument to %s", fname[algo][kind]);
    *out = nullptr;
    SAC_REQUIRE(n_members >= 1 && n_members <= SAC_GROUP_MAX, "a trainer group holds 1..%d members (got %d)", SAC_GROUP_MAX,
                n_members);
    const sac_trainer *t0 = members[0];
    for (int i = 0; i < n_members; ++i) {
        const sac_trainer *t = members[i];
        SAC_REQUIRE(t != nullptr, "trainer group member %d is null", i);
        for (int j = 0; j < i; ++j)
            SAC_REQUIRE(members[j] != t, "trainer group members %d and %d are the same trainer", j, i);
        if (group_member_ok(t, i, algo, mlp)) return -1;
        if (int rc = mlp ? mlp_member_shape(t, t0, i, kind == GROUP_ARCH) : fused_member_shape(t, t0, i, mixed)) return rc;
        SAC_REQUIRE(t->device == t0->device, "trainer group member %d lives on device %d, member 0 on %d", i, t->device, t0->device);
        if (int rc = mlp ? 0 : fused_member_kernels(t, t0, i, mixed)) return rc;
    }
    SAC_HIP(hipSetDevice(t0->device));
    sac_group *g = new sac_group();
    g->R = n_members;
    g->device = t0->device;
    g->algo = algo;
    g->mixed = mixed;
    g->mlp = mlp;
    for (int i = 0; i < n_members; ++i) g->m[i] = members[i];
    int rc = mlp ? group_build_mlp(g) : group_build_fused(g);
    if (rc == 0)
        rc = group_tables(g, mlp ? sizeof(gen::GenMember) : sizeof(GroupMember),
                          mlp ? sizeof(gen::GenGroupStep) : algo ? sizeof(Td3GroupStep) : sizeof(StepArg));
    if (rc) { group_free(g); return rc; }
    *out = g;
    return 0;
}

int sac_group_create(sac_group_t **out, sac_trainer_t *const *members, int n_members) {
    return group_create(out, members, n_members, 0, GROUP_SAME);
}

int td3_group_create(sac_group_t **out, sac_trainer_t *const *members, int n_members) {
    return group_create(out, members, n_members, 1, GROUP_SAME);
}

int sac_group_create_mixed(sac_group_t **out, sac_trainer_t *const *members, int n_members) {
    return group_create(out, members, n_members, 0, GROUP_MIXED);
}

int td3_group_create_mixed(sac_group_t **out, sac_trainer_t *const *members, int n_members) {
    return group_create(out, members, n_members, 1, GROUP_MIXED);
}

int sac_group_create_mlp(sac_group_t **out, sac_trainer_t *const *members, int n_members) {
    return group_create(out, members, n_members, 0, GROUP_MLP);
}

int td3_group_create_mlp(sac_group_t **out, sac_trainer_t *const *members, int n_members) {
    return group_create(out, members, n_members, 1, GROUP_MLP);
}

int sac_group_create_arch(sac_group_t **out, sac_trainer_t *const *members, int n_members) {
    return group_create(out, members, n_members, 0, GROUP_ARCH);
}

int td3_group_create_arch(sac_group_t **out, sac_trainer_t *const *members, int n_members) {
    return group_create(out, members, n_members, 1, GROUP_ARCH);
}

int sac_group_stage_count(const sac_group_t *g) {
    SAC_REQUIRE(g, "null argument to sac_group_stage_count");
    return (int)g->stages.size();
}

int sac_group_destroy(sac_group_t *g) {
    if (!g) return 0;
    (void)hipSetDevice(g->device);
    if (g->s) (void)hipStreamSynchronize(g->s);
    gate_leave(g->device, true, g->s, g->s2);
    group_free(g);
    return 0;
}

int sac_group_train_loop(sac_group_t *g, sac_buffer_t *const *bufs, int64_t n_steps, float *diag_first, float *diag_last) {
    SAC_REQUIRE(g && bufs && n_steps > 0 && n_steps < (1 << 30), "bad arguments to sac_group_train_loop");
    const int R = g->R;
    const sac_trainer *t0 = g->m[0];
    // every refusal comes before anything changes
    for (int r = 0; r < R; ++r) {
        if (group_member_ok(g->m[r], r, g->algo, g->mlp)) return -1;
        const sac_buffer *b = bufs[r];
        SAC_REQUIRE(b != nullptr, "trainer group buffer %d is null", r);
        for (int q = 0; q < r; ++q) SAC_REQUIRE(bufs[q] != b, "trainer group buffers %d and %d are the same buffer", q, r);
        SAC_REQUIRE(b->device == g->device, "trainer group buffer %d lives on device %d, the group on %d", r, b->device, g->device);
        if (g->mixed || g->mlp) {
            const sac_trainer *t = g->m[r];
            SAC_REQUIRE(b->O == t->O && b->A == t->A, "trainer group buffer %d has dims (%d,%d), its member (%d,%d)", r, b->O,
                        b->A, t->O, t->A);
        } else {
            SAC_REQUIRE(b->O == t0->O && b->A == t0->A, "trainer group buffer %d has dims (%d,%d), the trainers (%d,%d)", r, b->O,
                        b->A, t0->O, t0->A);
        }
        SAC_REQUIRE(b->size > 0, "trainer group buffer %d is empty: random_batch on an empty replay buffer", r);
        SAC_REQUIRE(b->size - 1 <= 0xffffffffLL, "replay buffers above 2^32 slots are not supported");
    }
    SAC_HIP(hipSetDevice(g->device));
    // what sac_train_loop does first, for every member and every buffer (each with its member's own batch)
    for (int r = 0; r < R; ++r) {
        sac_trainer *t = g->m[r];
        if (settle_trainer(t)) return -1;         // (device-batch steps nobody has verified yet come first)
        sac_buffer *b = bufs[r];
        if (host_rng_sync_in(b)) return -1;
        if (b->ra_ahead > 0) { if (readahead_rollback(b)) return -1; }
        else b->ra_streak = 0;
        if (loop_spec_drop(b)) return -1;
        b->loop_streak = 0;
        if (ensure_slots(b, t->Bt, LOOP_RING)) return -1;
        if (ensure_idx(b, LOOP_RING * t->B)) return -1;
    }
    // Buffers bound to the SAME host generator (sac_rng_bind_host: by default every EnvReplayBuffer samples np.random)
    // continue it one after another, as R sac_train_loop calls in member order would: buffer r starts where the previous
    // buffer of that generator ends (its n_steps batches of ITS member's batch size, drawn from its own size), and the
    // host words end at the last one's end state (host_rng_advance below runs in member order).
    for (int r = 1; r < R; ++r) {
        sac_buffer *b = bufs[r];
        if (!b->host_key) continue;
        int q = r - 1;
        while (q >= 0 && bufs[q]->host_key != b->host_key) --q;
        if (q < 0) continue;
        MtState st = bufs[q]->host_seen;
        host_rng_skip(bufs[q], st, g->m[q]->Bt, n_steps);
        if (host_rng_adopt(b, st)) return -1;
    }
    hipStream_t s = g->s, s2 = g->s2;
    // both group streams behind everything already queued on the members' and the buffers' streams
    for (int r = 0; r < R; ++r) {
        SAC_HIP(hipEventRecord(g->ev_in[2 * r], g->m[r]->stream));
        SAC_HIP(hipEventRecord(g->ev_in[2 * r + 1], bufs[r]->stream));
        for (int k = 0; k < 2; ++k) {
            SAC_HIP(hipStreamWaitEvent(s, g->ev_in[2 * r + k], 0));
            SAC_HIP(hipStreamWaitEvent(s2, g->ev_in[2 * r + k], 0));
        }
    }
    // the member table of this call, in device order (the step table follows chunk by chunk)
    gen::GenMember *const h_gm = reinterpret_cast<gen::GenMember *>(g->h_tab);     // (MLP groups)
    GroupMember *const h_mem = reinterpret_cast<GroupMember *>(g->h_tab);          // (the others)
    for (int k = 0; k < R && g->mlp; ++k) {
        const int r = g->ord[k];
        const sac_trainer *t = g->m[r];
        sac_buffer *b = bufs[r];
        SAC_REQUIRE(b->slot.off_obs == t->ext_layout.off_obs && b->slot.off_nobs == t->ext_layout.off_nobs && b->slot.Bt == t->gen->n,
                    "internal: minibatch slot layout differs from the one the general step was built for");
        gen::GenMember &M = h_gm[k];
        M.d = t->gen->dev;
        M.d.eps1 = M.d.eps2 = nullptr;                // (loop steps draw their noise on the device)
        M.SL = b->slot;
        M.slots = b->d_slots;
    }
    for (int k = 0; k < R && !g->mlp; ++k) {
        const int r = g->ord[k];
        const sac_trainer *t = g->m[r];
        sac_buffer *b = bufs[r];
        GroupMember &M = h_mem[k];
        M.d = t->dev;
        M.d.eps1 = M.d.eps2 = nullptr;                // (loop steps draw their noise on the device)
        M.T = t->dw;
        M.T.abort = nullptr;                          // (the four-launch step: no fused launch can give up in front of it)
        M.SL = b->slot;
        M.slots = b->d_slots;
        if (g->algo == 1) {
            M.T = t->dw_q; M.T.abort = nullptr;
            M.T_tp = t->dw_q_tp; M.T_pi = t->dw_pi; M.T_none = t->dw_none;
            M.T_tp.abort = M.T_pi.abort = M.T_none.abort = nullptr;
        }
        M.xa = t->plan.a.grid; M.xb = t->plan.b.grid; M.xc = t->plan.c.grid; M.xpi = t->plan.b2.grid;
    }
    // the draw table in member order (one launch); the gather table sorted by gather class (one launch per class: the
    // obs chunks per thread, NIT = 1 / 2 / 4 / 8), each class in member order
    int gord[SAC_GROUP_MAX], gnit[4] = {}, glo[5] = {}, ngc = 0;
    size_t glds[4] = {};
    for (int nit : {1, 2, 4, 8}) {
        const int lo = glo[ngc];
        int n = lo;
        size_t lds = 0;
        for (int r = 0; r < R; ++r) {
            const int v = gather_nit(bufs[r]), cl = v <= 1 ? 1 : v <= 2 ? 2 : v <= 4 ? 4 : 8;
            SAC_REQUIRE(v <= 8, "observation rows too wide for the gather kernel (obs_dim %d)", bufs[r]->O);
            if (cl != nit) continue;
            gord[n++] = r;
            lds = std::max(lds, sizeof(float) * (size_t)(2 * RB * bufs[r]->Ost + RB * bufs[r]->Ast));
        }
        if (n == lo) continue;
        gnit[ngc] = nit; glds[ngc] = lds;
        glo[++ngc] = n;
    }
    for (int r = 0; r < R; ++r) {
        const sac_trainer *t = g->m[r];
        sac_buffer *b = bufs[r];
        uint32_t rng = (uint32_t)(b->size - 1), mask = rng;
        mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
        for (int h = 0; h < 2; ++h)
            g->h_smp[h * R + r] = SampleMember{b->d_rng, b->d_idx + (int64_t)h * LOOP_CH * t->B, rng, mask, t->Bt, t->B};
    }
    for (int p = 0; p < R; ++p) {
        const int r = gord[p];
        const sac_trainer *t = g->m[r];
        sac_buffer *b = bufs[r];
        for (int h = 0; h < 2; ++h)
            g->h_gat[h * R + p] = GatherMember{b->view(), b->d_idx + (int64_t)h * LOOP_CH * t->B,
                                               b->d_slots + (size_t)h * LOOP_CH * b->slot.slot_floats, b->slot, t->B};
    }
    SAC_HIP(hipMemcpyAsync(g->d_tab, g->h_tab, g->mem_bytes * R, hipMemcpyHostToDevice, s2));
    SAC_HIP(hipMemcpyAsync(g->d_smp, g->h_smp, sizeof(SampleMember) * 2 * R, hipMemcpyHostToDevice, s2));
    SAC_HIP(hipMemcpyAsync(g->d_gat, g->h_gat, sizeof(GatherMember) * 2 * R, hipMemcpyHostToDevice, s2));
    long long pi_steps[SAC_GROUP_MAX] = {};           // TD3: policy steps of each member so far in this call
    unsigned char plan[LOOP_CH];                      // TD3: per step of a chunk, bit 0: some member runs the actor pass, bit 1: some policy step
    FusedGate &G = g_gate[g->device & 63];
    int64_t done = 0;
    for (int c = 0; done < n_steps; ++c) {
        const int64_t m = (n_steps - done < LOOP_CH) ? n_steps - done : LOOP_CH;
        const int h = c & 1;
        // the chunk's draws and gathers into half h of every buffer's loop slots, once the steps of chunk c - 2 are done there
        if (c >= 2) SAC_HIP(hipStreamWaitEvent(s2, g->ev_done[h], 0));
        {   // (tenants of the gate too: at R = 16 the grouped gather is 16 x 1024 workgroups that must not overlap a k_abc)
            std::lock_guard<std::mutex> lk(G.mu);
            const bool gate = G.live > 1;
            if (gate && G.last && G.last != s2) SAC_HIP(hipStreamWaitEvent(s2, G.ev, 0));
            if (launch_sample_group(g->d_smp + h * R, R, m, s2)) return -1;
            for (int q = 0; q < ngc; ++q) {
                int grid = 0;
                for (int p = glo[q]; p < glo[q + 1]; ++p) {
                    const int64_t nb = (int64_t)(g->m[gord[p]]->B / RB) * m;
                    grid = std::max(grid, (int)(nb < 1024 ? nb : 1024));     // (the x-extent of a solo launch_gather)
                }
                if (launch_gather_group(g->d_gat + h * R + glo[q], glo[q + 1] - glo[q], gnit[q], m, grid, glds[q], 1, s2)) return -1;
            }
            if (gate) { SAC_HIP(hipEventRecord(G.ev, s2)); G.last = s2; }
        }
        SAC_HIP(hipEventRecord(g->ev_ready[h], s2));
        // the chunk's step rows, one per step and member: the arguments its solo step would get (step_arg; TD3: td3_plan,
        // the actor pass also on the call's first step), the diagnostics published on the call's last step.  One host
        // image serves every kind: a fused SAC group's row is its leading StepArg.  (The host half is free once its last
        // copy has run.)
        if (c >= 2 && wait_event(g->ev_copied[h])) return -1;
        const size_t step_off = (size_t)h * LOOP_CH * R * g->step_bytes;
        for (int64_t j = 0; j < m; ++j) {
            plan[j] = 0;
            for (int k = 0; k < R; ++k) {
                const int r = g->ord[k];
                const sac_trainer *t = g->m[r];
                const long long i = (long long)(done + j);
                const bool last = i == n_steps - 1;
                gen::GenGroupStep gs;
                memset(&gs, 0, sizeof(gs));
                if (g->algo == 0) {
                    gs.sa = step_arg(t->n_train_steps_total + i, t->adam_t + i + 1, (int)i, g->algo, last);
                    if (g->mlp) gs.polyak = (gs.sa.step_now % t->gen->dev.period) == 0 ? 1 : 0;
                } else {
                    const Td3Plan P = td3_plan(t, i, pi_steps[r], i == 0);
                    gs.sa = step_arg(P.step, P.t_q, (int)i, g->algo, last);
                    gs.sp = step_arg(P.step, P.t_pi, (int)i, 2, last);
                    gs.actor = P.actor ? 1 : 0;
                    gs.pstep = P.pstep ? 1 : 0;
                    if (g->mlp) gs.polyak = gs.pstep;     // (the critics' targets follow on policy steps)
                    plan[j] |= (P.actor ? 1 : 0) | (P.pstep ? 2 : 0);
                    pi_steps[r] += P.pstep ? 1 : 0;
                }
                memcpy(g->h_step + step_off + (size_t)(j * R + k) * g->step_bytes, &gs, g->step_bytes);
            }
        }
        SAC_HIP(hipMemcpyAsync(g->d_step + step_off, g->h_step + step_off, g->step_bytes * m * R, hipMemcpyHostToDevice, s));
        SAC_HIP(hipEventRecord(g->ev_copied[h], s));
        SAC_HIP(hipStreamWaitEvent(s, g->ev_ready[h], 0));
        {
            std::lock_guard<std::mutex> lk(G.mu);
            const bool gate = G.live > 1;
            if (gate && G.last && G.last != s) SAC_HIP(hipStreamWaitEvent(s, G.ev, 0));
            // per step, the stage list: a stage per variant class goes over the class's range of the tables (gridDim.y =
            // its size), the others over all members
            for (int64_t j = 0; j < m; ++j) {
                int slot = (int)(h * LOOP_CH + j);
                const long long i = (long long)(done + j);
                const char *row = g->d_step + step_off + (size_t)j * R * g->step_bytes;
                for (const GroupStage &st : g->stages) {
                    if ((plan[j] & st.need) != st.need) continue;
                    if (st.ends_only && i != 0 && i != n_steps - 1) continue;
                    for (int q = 0; q < (st.per_class ? g->ncls : 1); ++q) {
                        const int lo = st.per_class ? g->cls[q].lo : 0, n = st.per_class ? g->cls[q].n : R;
                        const void *mem = g->d_tab + (size_t)lo * g->mem_bytes, *step = row + (size_t)lo * g->step_bytes;
                        int arg = st.arg;
                        if (st.hdr >= 0) {
                            const gen::GemmStage *H = g->d_hdr + (size_t)st.hdr * R;
                            void *args[] = {&H, &mem, &step, &slot, const_cast<gen::GemmGroupMap *>(&st.map)};
                            (void)hipLaunchKernel(st.fn[0], dim3(st.gx[0]), dim3(st.block), args, 0, s);
                        } else {
                            const int gx = (st.idle_one && !(plan[j] & 2)) ? 1 : st.gx[q];
                            void *args[] = {&mem, &step, &slot, &arg};
                            (void)hipLaunchKernel(st.fn[q], dim3(gx, n), dim3(st.block), args, st.lds[q], s);
                        }
                    }
                }
            }
            SAC_HIP(hipGetLastError());
            if (gate) { SAC_HIP(hipEventRecord(G.ev, s)); G.last = s; }
        }
        SAC_HIP(hipEventRecord(g->ev_done[h], s));
        done += m;
    }
    // the host mirrors of the generators follow behind the launches (each buffer by its member's batch)
    for (int r = 0; r < R; ++r) host_rng_advance(bufs[r], g->m[r]->Bt, n_steps);
    SAC_HIP(hipEventRecord(g->ev_end, s));
    if (wait_event(g->ev_end)) return -1;
    SAC_HIP(hipStreamSynchronize(s2));
    for (int r = 0; r < R; ++r) {
        sac_trainer *t = g->m[r];
        t->n_train_steps_total += n_steps;
        t->adam_t += n_steps;
        t->adam_t_pi += pi_steps[r];                  // (TD3; zero for SAC)
        t->mirror_valid = false;
        if (diag_first) memcpy(diag_first + (size_t)r * SAC_DIAG_N, t->h_diag, sizeof(float) * SAC_DIAG_N);
        if (diag_last) memcpy(diag_last + (size_t)r * SAC_DIAG_N, t->h_diag + SAC_DIAG_N, sizeof(float) * SAC_DIAG_N);
    }
    return 0;
}

