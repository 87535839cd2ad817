// The step plan: which kernels, grids, block sizes and LDS a trainer of the fused kernels' shapes runs, decided once at
// creation as a pure function of (obs_dim, act_dim, batch, algo, CU count, environment).  Plain C++17: no HIP header,
// no HIP call, no kernel named -- sac_trainer.hip binds the plan to template instances (step_kernels); the order of a
// step's launches is step_schedule below, which the solo step and the trainer groups both walk;
// tests/test_step_plan_host.py checks plan and schedule with the host compiler alone.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>

namespace sac {

constexpr int RB = 16;            // rows of one row-block (one MFMA 16x16x4 M tile)
constexpr int H = 256;            // hidden width (every shipped variant.json)
constexpr int WLD = 64 + 4;       // 64 staged weight rows; +4: scatter writes and 16-B reads are bank-conflict free
constexpr int RD0 = 8;            // narrow first layers: up to 8 k-chunks (K <= 128) held at once
constexpr int FUSED_RED = 2048;   // floats of split-K scratch (k_abc)
constexpr size_t LDS_CAP = 160 * 1024 - 512;      // dynamic LDS a workgroup may ask for
constexpr size_t LDS_DEFAULT = 64 * 1024;         // ... without hipFuncAttributeMaxDynamicSharedMemorySize raised

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// an integer variable of the environment: unset, or atoi of its value
struct EnvInt {
    bool set = false;
    int v = 0;
    bool is(int x) const { return set && v == x; }
};

struct StepEnv {
    EnvInt force_sp;              // SAC_FORCE_SP: the column split (tuning experiments only)
    EnvInt wide_min_kq;           // SAC_WIDE_MIN_KQ: the narrowest "wide" first layer (tuning experiments only)
    bool dw_form_loop = false;    // SAC_DW_FORM=loop: the weight-gradient launch keeps its loop form (ablations, tests)
    EnvInt fused;                 // SAC_FUSED=0: the four-launch step (co-tenant processes on one GPU; ablations)
    EnvInt fused_test_stall;      // SAC_FUSED_TEST_STALL=<n>: the n-th fused launch loses a producer (tests; counted from the
                                  // launch number sac_debug_set_launch_number last set, 0 without it: test_stall_hits)
    EnvInt chain;                 // SAC_CHAIN=0 / 1: never / wherever it can run (A/B comparisons)
    EnvInt chain8;                // SAC_CHAIN8=0: the four-wave k_chain (A/B comparisons)
    EnvInt bwd8;                  // SAC_BWD8=0: the four-wave backward launch at column split 1 (A/B comparisons)
    EnvInt chain_bwd;             // SAC_CHAIN_BWD=1 / 0: forces the backward blocks into the chained launch / out of it
    EnvInt row_images;            // SAC_ROW_IMAGES=0: k_abc converts its input rows itself (RowRegs; A/B comparisons)
};

// the only getenv() calls for these names
static inline StepEnv step_env_from_environment() {
    auto num = [](const char *name) {
        const char *e = getenv(name);
        return e ? EnvInt{true, atoi(e)} : EnvInt{};
    };
    const char *form = getenv("SAC_DW_FORM");
    return StepEnv{num("SAC_FORCE_SP"), num("SAC_WIDE_MIN_KQ"), form && strcmp(form, "loop") == 0, num("SAC_FUSED"),
                   num("SAC_FUSED_TEST_STALL"), num("SAC_CHAIN"), num("SAC_CHAIN8"), num("SAC_BWD8"), num("SAC_CHAIN_BWD"),
                   num("SAC_ROW_IMAGES")};
}

struct StepLaunch {
    int grid = 0, threads = 256;
    size_t lds = 0;
};

struct StepPlan {
    int algo = 0;                                     // 0 SAC, 1 TD3
    int B = 0, NB = 0, KP = 0, KQ = 0, NH = 0;        // B: batch padded to row-blocks; NB: its row-blocks
    int nth = 1, SP = 4;                              // head tiles; column split
    bool wide = false;                                // k_fwd_* / k_abc: first layers of more than RD0 k-chunks
    bool wide4 = false;                               // k_chain*: first layers of more than four k-chunks
    bool fused = false;                               // the step starts as one fused launch (k_abc, or k_chain8<.., BWD>) + dW
    bool chain = false, chain8 = false;               // A + B as one launch (k_chain); its eight-wave variant
    bool bwd8 = false;                                // launch C at column split 1 on eight waves (k_bwd8)
    bool chain_bwd = false;                           // the fused launch is k_chain8 with the backward blocks inside
    bool dw_one = false;                              // the weight-gradient launch in its one-group form
    bool row_images = false;                          // k_abc copies its input rows from the slot's ready LDS images (SlotLayout::off_img_sa)
    unsigned test_stall_at = 0;
    // The launches.  a / b / c are the four-launch step's (what a fused trainer falls back to -- with `chained` in place
    // of a + b where `chain` is set); compact: k_bwd's last argument (SAC).  b2 / c2: TD3's actor pass.
    StepLaunch a, b, c, fused_launch, chained, b2, c2;
    int compact = 0;
    bool ok = true;
    int refusal = 0;                                  // !ok: 1 launch A, 2 launch B asks for more LDS than a workgroup gets
};

static inline StepPlan step_plan(int obs_dim, int act_dim, int batch, int algo, int cus, const StepEnv &E) {
    StepPlan P;
    const bool td3 = algo == 1;
    P.algo = algo;
    P.B = round_up(batch, RB); P.NB = P.B / RB;
    P.KP = round_up(obs_dim, 16); P.KQ = P.KP + 16; P.NH = round_up((td3 ? 1 : 2) * act_dim, 16);
    P.nth = P.NH / 16;
    const int NB = P.NB, KQ = P.KQ, nth = P.nth;
    // column split: small batches spread every 256-wide layer over 4 workgroups per row-block; once the
    // row-blocks alone fill the 256 CUs (B >= 512) fewer, fatter workgroups win.  SP*NB stays even (XCD map).
    P.SP = (NB <= 16) ? 4 : (NB <= 32 ? 2 : ((NB & 1) ? 2 : 1));
    if (E.force_sp.set) {
        const int v = E.force_sp.v;
        if ((v == 1 || v == 2 || v == 4) && ((v * NB) % 2 == 0)) P.SP = v;
    }
    const int SP = P.SP;
    const int KL0q = round_up(KQ, 64);
    const int sw = 64 * (4 / SP);
    const size_t lds_fa = sizeof(float) * (size_t)(RB * KL0q + RB * H + RB * sw + 4 * nth * 256);
    const size_t lds_fb = sizeof(float) * (size_t)(RB * KL0q + RB * H + RB * sw + 1024 + (SP == 4 ? H * WLD : 0));
    const size_t lds_bw = sizeof(float) * (size_t)(RB * 64 + RB * H);
    if (lds_fa > LDS_CAP) { P.ok = false; P.refusal = 1; }
    else if (lds_fb > LDS_CAP) { P.ok = false; P.refusal = 2; }
    P.wide = KQ >= (E.wide_min_kq.set ? E.wide_min_kq.v : 16 * RD0 + 1);
    P.wide4 = KQ > 64;
    // the weight-gradient launch: one group of four batch chunks per wave covers 256 rows => its straight-line form
    // (dw_adam_body<true>)
    P.dw_one = NB <= 16 && !E.dw_form_loop;
    P.test_stall_at = E.fused_test_stall.set ? (unsigned)E.fused_test_stall.v : 0u;
    // The fused step (sac_fused.h) needs: column split 4 (at most 16 row-blocks), and every one of its 16*NB
    // workgroups resident at once (one per CU: 100-160 KB of LDS each, which also bounds obs_dim to ~1000).
    const size_t lds_abc = sizeof(float) * (size_t)(RB * KL0q + RB * H + RB * 64 + FUSED_RED + H * WLD);
    P.fused = SP == 4 && NB <= 16 && 16 * NB <= cus && lds_abc <= LDS_CAP && !E.fused.is(0);
    P.fused_launch = StepLaunch{16 * NB, 256, lds_abc};
    // k_abc takes its input rows as the slot's row images.  Every writer of a slot produces them (the gather kernels, the
    // staging of an external batch: SlotLayout::has_images), so the choice is by kernel alone -- the other step kernels
    // convert the row-major rows themselves.
    P.row_images = P.fused && !E.row_images.is(0);
    // Column split 1: the forward launches as one (sac_chain.h).
    // Where it pays (measured, scripts/large_batch_matrix.sh; round 3's second half with the eight-wave kernel): first layers
    // of at most eight k-chunks -- Door 46/7 batch 1024 58.1 -> 51.8 us per step, TwoArmHandoff 86/14 64.9 -> 60.9, and
    // now batches of more than one round of workgroups too (Door batch 1536 87.7 -> 83.9, batch 2048 95.3 -> 91.7: the
    // four-wave kernel's 350 registers lost there); Wipe's 25-chunk first layers (recomputed by both P items) still lose
    // (83.4 against 86.6).
    const size_t lds_chain = sizeof(float) * (size_t)(RB * KL0q + 2 * RB * H + 4 * nth * 256 + RB * 32);
    P.chain8 = !E.chain8.is(0);
    const bool pays = ((P.chain8 || 4 * NB <= cus) && KQ <= 128) || E.chain.is(1);
    P.chain = !td3 && !P.fused && SP == 1 && (NB % 2) == 0 && lds_chain <= LDS_CAP && pays && !E.chain.is(0);
    P.chained = StepLaunch{4 * NB, P.chain8 ? 512 : 256, lds_chain};
    // column split 1, SAC: the backward launch on eight waves too
    P.bwd8 = !td3 && SP == 1 && !E.bwd8.is(0);
    // One round of workgroups (batch 1024): the backward blocks inside the forward launch behind in-launch hand-offs
    // (k_chain8<.., BWD>, sac_chain.h) -- a fused step like k_abc's: same give-up protocol, same fall-back (to k_chain8 + k_bwd8).
    // Where it pays (A/B on one box, 2 x 2000 steps): exactly one workgroup per CU and narrow first layers -- Door 46/7
    // batch 1024 19 290 -> 19 860 steps/s (the launch 33.6 us for 22.3 + 10.6 + a boundary); TwoArmHandoff 86/14 batch 1024
    // -3.5 %, batch 992 -3 %, batch 800 -8 % (fewer workgroups than CUs: the separate backward launch was spreading its
    // 192 blocks over idle CUs).  SAC_CHAIN_BWD=1 / 0 forces it (any batch whose workgroups are all resident) / off.
    const bool pays_b = 4 * NB == cus && KQ <= 64;
    P.chain_bwd = P.chain && P.chain8 && P.bwd8 && 4 * NB <= cus && (E.chain_bwd.set ? E.chain_bwd.v == 1 : pays_b);
    if (P.chain_bwd) {
        P.fused = true;
        P.row_images = false;
        P.fused_launch = StepLaunch{4 * NB, 512, lds_chain > lds_bw ? lds_chain : lds_bw};
    }
    // the four launches (launch C of SAC: see k_bwd for `compact`; TD3's critic map: two twins x groups of four blocks)
    P.a = StepLaunch{4 * SP * NB, 256, lds_fa};
    if (!td3) {
        P.compact = (3 * SP * NB <= 192) ? 1 : 0;
        P.b = StepLaunch{4 * SP * NB, 256, lds_fb};
        P.c = StepLaunch{P.compact ? 4 * SP * NB : 3 * SP * NB, P.bwd8 ? 512 : 256, lds_bw};
    } else {
        const int g2 = 8 * ((SP * NB + 3) / 4);
        P.b = StepLaunch{g2, 256, lds_fb};
        P.c = StepLaunch{g2, 256, lds_bw};
        P.b2 = StepLaunch{SP * NB, 256, lds_fb};
        P.c2 = StepLaunch{SP * NB, 256, lds_bw};
    }
    return P;
}

// ---- The step schedule: the plan's launches of ONE step, in launch order -------------------------------------------------
// The solo step (launch_step walks it, sac_profile_loop with events between its stages) and the trainer groups of these
// shapes (group_build_fused) read this one list.  fused_now: the trainer still runs the plan's fused launch (a give-up or
// a confinement drops it for good: the four-launch list, with `chained` in place of A + B where the plan chains).
enum StepKernelId { SK_A, SK_B, SK_C, SK_B2, SK_C2, SK_FUSED, SK_CHAINED, SK_DW, SK_DW_Q, SK_DW_PI };
constexpr int STEP_NEED_ACTOR = 1, STEP_NEED_PSTEP = 2;       // (the bits of GroupStage::need)
constexpr int TAIL_ACTOR_FOLLOWS = -1;
struct StepStage {
    int kernel = 0;               // StepKernelId
    StepLaunch launch;            // the plan's; a weight-gradient stage: threads 256, lds 0, the grid left to whoever binds its tables
    int need = 0;                 // runs on: 0 every step, STEP_NEED_ACTOR steps with an actor pass, STEP_NEED_PSTEP policy steps (TD3)
    int arg = 0;                  // its StepArg: 0 the step's first (SAC, TD3's critic pass), 1 the actor pass's
    int tail = 0;                 // the launch's trailing int where it has one: >= 0 as it stands (launch C: `compact`);
                                  // TAIL_ACTOR_FOLLOWS: 1 on the steps an actor pass follows (TD3's launch A and fused launch)
    int last_event = 0;           // sac_profile_loop: the events up to this one (of 1..6) are recorded behind the stage; 0: none
};
constexpr int STEP_STAGES_MAX = 8;
static inline int step_schedule(const StepPlan &P, bool fused_now, StepStage out[STEP_STAGES_MAX]) {
    const bool td3 = P.algo == 1;
    const int follows = td3 ? TAIL_ACTOR_FOLLOWS : 0, ev = td3 ? 0 : 1;       // (the profiling pass is the SAC step's)
    const StepLaunch dw{0, 256, 0};
    int n = 0;
    if (P.fused && fused_now) out[n++] = StepStage{SK_FUSED, P.fused_launch, 0, 0, follows, 4 * ev};
    else {
        if (P.chain) out[n++] = StepStage{SK_CHAINED, P.chained, 0, 0, 0, 2 * ev};
        else {
            out[n++] = StepStage{SK_A, P.a, 0, 0, follows, 1 * ev};
            out[n++] = StepStage{SK_B, P.b, 0, 0, 0, 2 * ev};
        }
        out[n++] = StepStage{SK_C, P.c, 0, 0, P.compact, 4 * ev};
    }
    out[n++] = StepStage{td3 ? SK_DW_Q : SK_DW, dw, 0, 0, 0, 6 * ev};
    if (td3) {                    // the actor pass: Q1(s, pi(s)) on every step that wants it, the policy's backward and update on policy steps
        out[n++] = StepStage{SK_B2, P.b2, STEP_NEED_ACTOR, 1, 0, 0};
        out[n++] = StepStage{SK_C2, P.c2, STEP_NEED_PSTEP, 1, 0, 0};
        out[n++] = StepStage{SK_DW_PI, dw, STEP_NEED_ACTOR, 1, 0, 0};
    }
    return n;
}

// ---- The hand-off words of the fused launches (k_abc: sac_fused.h; k_chain8<.., BWD>: sac_chain.h) ----------------------
// One allocation per trainer (sac_trainer::d_sync), cut into 128-byte lines of SYNC_STRIDE words; a counter is the first
// word of its line.  INVARIANT: after launch number n of a trainer every counter holds units * n modulo 2^32, where
// `units` is how often one launch adds to it, and a consumer of launch n waits for (int)(counter - units * n) >= 0.  Every
// value of a counter, of a launch number and of a tag is an ordinary value: none is reserved to mean "nothing".  The
// kernels take their targets from the constants below and the host's test hook (sac_debug_set_launch_number) fills the
// words from the same table, so the two cannot drift apart; tests/test_sync_words_host.py checks table and fill.
constexpr int SYNC_STRIDE = 32;                   // unsigned words per line
enum SyncRegion {
    SYNC_HEAD = 0,      // [2][NB]  k_abc: a policy chain's head partials of (side, row-block)
    SYNC_QA,            // [NB]     critic-chain phase A (k_abc) / item C's Q2 pass (k_chain8)
    SYNC_TQ,            // [NB]     the target partials
    SYNC_AC,            // [NB]     the actor tails (k_abc, SAC) / item P1 (k_chain8)
    SYNC_LP,            // [1]      k_chain8: the log-pi sums of every P0 item
    SYNC_ABORT,         // [1]      the sticky give-up word
    SYNC_ZX,            // [6][NB]  k_abc, wide first layers: the exchange of the split first layers
    SYNC_LP_TAG,        // [1]      k_abc: NB (<= 16) 8-byte words {value, launch number} -- the row-block sums of log pi
    SYNC_REGIONS
};
enum FusedKernel { FUSED_ABC_SAC = 0, FUSED_ABC_TD3 = 1, FUSED_CHAIN8 = 2 };

// per-launch units, named once
constexpr unsigned ABC_UNITS_HEAD = 4;            // the four column parts of a policy chain
constexpr unsigned ABC_UNITS_QA = 8;              // two twins x four parts
constexpr unsigned ABC_UNITS_TQ = 8;              // two policy chains x four parts
constexpr unsigned ABC_UNITS_AC = 8;              // two twins x four parts (SAC; the TD3 critic pass has no actor tail: 0)
constexpr unsigned ABC_UNITS_ZX = 4;              // the four parts of a chain (wide first layers only)
constexpr unsigned CHAIN_UNITS_RB = 1;            // k_chain8: one item per row-block counter
constexpr unsigned chain_units_lp(int NB) { return (unsigned)NB; }          // k_chain8: every P0 item (constexpr: host and kernels)

static inline int sync_region_lines(int region, int NB) {
    switch (region) {
    case SYNC_HEAD: return 2 * NB;
    case SYNC_QA: case SYNC_TQ: case SYNC_AC: return NB;
    case SYNC_ZX: return 6 * NB;
    case SYNC_LP: case SYNC_ABORT: case SYNC_LP_TAG: return 1;
    default: return 0;
    }
}
// first line of a region: the regions lie back to back in the order of the enum
static inline int sync_region_line(int region, int NB) {
    int at = 0;
    for (int r = 0; r < region; ++r) at += sync_region_lines(r, NB);
    return at;
}
static inline size_t sync_words(int NB) { return (size_t)SYNC_STRIDE * (size_t)sync_region_line(SYNC_REGIONS, NB); }

// what ONE launch of `kernel` adds to each counter of `region` (wide: k_abc's split first layers run).
// The TD3 critic pass adds to the head counters of side 0 only on launches an actor pass follows; nothing waits for
// them in that mode (the actor pass is a launch of its own), so the table carries the side-1 figure for both.
static inline unsigned sync_units(int kernel, int region, int NB, bool wide) {
    if (kernel == FUSED_CHAIN8) {
        if (region == SYNC_QA || region == SYNC_TQ || region == SYNC_AC) return CHAIN_UNITS_RB;
        return region == SYNC_LP ? chain_units_lp(NB) : 0u;
    }
    switch (region) {
    case SYNC_HEAD: return ABC_UNITS_HEAD;
    case SYNC_QA: return ABC_UNITS_QA;
    case SYNC_TQ: return ABC_UNITS_TQ;
    case SYNC_AC: return kernel == FUSED_ABC_SAC ? ABC_UNITS_AC : 0u;
    case SYNC_ZX: return wide ? ABC_UNITS_ZX : 0u;
    default: return 0u;
    }
}

// The sync_words(NB) words as `seq` completed launches of `kernel` leave them: every counter at units * seq modulo 2^32,
// every tagged word {0.0f, seq} (k_abc, SAC), the give-up word clear, everything else 0.
static inline void sync_fill(unsigned *w, int NB, int kernel, bool wide, unsigned seq) {
    memset(w, 0, sizeof(unsigned) * sync_words(NB));
    for (int r = 0; r < SYNC_REGIONS; ++r) {
        if (r == SYNC_ABORT || r == SYNC_LP_TAG) continue;
        const unsigned v = sync_units(kernel, r, NB, wide) * seq;
        unsigned *p = w + (size_t)SYNC_STRIDE * sync_region_line(r, NB);
        for (int i = 0; i < sync_region_lines(r, NB); ++i) p[(size_t)SYNC_STRIDE * i] = v;
    }
    if (kernel == FUSED_ABC_SAC) {
        unsigned *p = w + (size_t)SYNC_STRIDE * sync_region_line(SYNC_LP_TAG, NB);
        for (int i = 0; i < NB && i < SYNC_STRIDE / 2; ++i) p[2 * i + 1] = seq;       // (little-endian: the tag is the high word)
    }
}

// SAC_FUSED_TEST_STALL=<n> counts from the launch number the test hook last set (0 without it): is launch `seq` the one?
static inline bool test_stall_hits(unsigned stall_at, unsigned base, unsigned seq) { return stall_at != 0u && seq - base == stall_at; }

}  // namespace sac
