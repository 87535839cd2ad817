// Acting on the device: policy.get_actions(obs) from the trainer's own weights (included by sac_trainer.hip).
//
// k_act is the forward pass of the policy alone -- TanhGaussianPolicy (SAC) or TanhMlpPolicy (TD3) with the fused
// kernels' shapes: two hidden layers of at most 256 units, zero-padded to 256 as in the step -- for 1..1024 observation
// rows of each of 1..SAC_GROUP_MAX trainers in ONE launch.  It reads the policy's forward copy Net::P where the step
// kernels keep it (padded, fragment-major: frag_off); nothing is repacked, mirrored or copied.
//
//   grid    one workgroup (4 waves) per 16-row block of one member; the blocks of all members side by side, found
//           through the per-member table ActMember (device-visible memory, read with scalar loads)
//   LDS     the row-block's observations [16][round_up(KP, 64)], both hidden layers [16][256], the head [16][32]
//   GEMMs   fp32 MFMA 16x16x4 through the step kernels' weight ring (WRing / gemm_ring): wave w owns hidden
//           units 64 w .. 64 w + 63 of both hidden layers; waves 0 (and 1) own the head's 16 (32) rows
//   head    SAC: tanh(mean) | tanh(mean + exp(clamp(log_std, -20, 2)) * eps);  TD3: tanh(last_fc)
//
// Row independence.  A row's action is a function of that row's observation, that row's eps and the member's weights
// only: every output element is one MFMA dot product over k in ascending chunks, and neither the row's place in its
// block, nor the number of rows, nor the other members of the launch enter it.  Rows beyond a member's n are zero
// padding and are never written.  Grouped acting is therefore bit for bit solo acting
// (tests/test_gpu_device_acting.py).
//
// The kernel writes the caller's actions and nothing else: nothing the step kernels read.  Observations, eps, actions
// and the member table live in ONE mapped pinned staging buffer (allocated on first use, grown as needed) which the
// kernel reads and writes over the link: a call is one launch and one wait, without a copy call of its own.
//
// General-step trainers (hidden sizes beyond the fused kernels') are out of scope here: these entries refuse them, and
// they act on the host (sac_policy_act) or through the entries of their own, sac_policy_act_general[_many]
// (k_act_layer, sac_act_general.h).
#pragma once

namespace sac {

constexpr int ACT_MAX_ROWS = 1024;        // rows per member and call
constexpr int ACT_HEAD_LD = 32;           // head pre-activations [16][32]: mean | log_std (A <= 16)

struct ActMember {
    const float *P;                // the policy's forward copy (Net::P)
    const float *obs, *eps;        // (n, O) / (n, A) row-major (eps unused unless SAC and stochastic)
    float *act;                    // (n, A)
    long long offW[3], offB[3];    // the three layers inside P
    int O, A, KP, NH;              // NH: padded head rows (SAC: mean + log_std; TD3: last_fc)
    int n, rb0;                    // rows; first workgroup of this member in the launch
    int stochastic, pad;           // 1: SAC with exploration noise
};

// The hidden layers' bias + ReLU of k_act.  It stands in for the step kernels' hidden_epilogue, whose ReLU is
// fmaxf(x, 0): that gives 0 for NaN and would turn a non-finite observation row into a finite action, where torch's relu
// and the host forward keep the NaN.  Here x < 0 ? 0 : x; every finite value comes out as from fmaxf, up to the sign of
// a zero, which no sum downstream can see.  With hidden sizes below 256 an Inf observation becomes NaN already in the
// zero-weight pad units (0 * inf) and from there in every unit of the next layer; torch has no pad units but reaches NaN
// in its second layer too, through inf - inf over units of both signs, so the actions agree (NaN) all the same.
template <int NT>
__device__ __forceinline__ void act_hidden_epilogue(const f32x4 (&acc)[NT], int n_base, int n_stride, const float (&bv)[NT],
                                                    float *Xn, int KL) {
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n = n_base + t * n_stride + c;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float v = acc[t][i] + bv[t];
            Xn[lds_off(4 * g + i, n, KL)] = v < 0.f ? 0.f : v;
        }
    }
}

__global__ __launch_bounds__(256) void k_act(const ActMember *__restrict__ tab, int n_members) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // this workgroup's member: the last one whose first workgroup is not behind this one (wave-uniform, scalar loads)
    int mi = 0;
    for (int i = 1; i < n_members; ++i)
        if ((int)blockIdx.x >= sload(&tab[i].rb0)) mi = i;
    const ActMember *M = tab + mi;
    const float *P = sload(&M->P);
    const int O = sload(&M->O), A = sload(&M->A), KP = sload(&M->KP), NH = sload(&M->NH), n = sload(&M->n);
    const int row0 = ((int)blockIdx.x - sload(&M->rb0)) * RB;
    const int KL0 = (KP + 63) & ~63;
    float *X0 = lds;                     // [16][KL0]
    float *X1 = X0 + RB * KL0;           // [16][256]
    float *X2 = X1 + RB * H;             // [16][256]
    float *HL = X2 + RB * H;             // [16][32]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;

    // weight requests of the first layer go out in front of the observation rows
    WRing<4> r0;
    r0.init(P + sload(&M->offW[0]), KP, 64 * wave, 16);
    r0.fill(KP >> 4);
    float bv0[4], bv1[4];
    const float *b0 = P + sload(&M->offB[0]), *b1 = P + sload(&M->offB[1]);
#pragma unroll
    for (int t = 0; t < 4; ++t) { bv0[t] = b0[64 * wave + 16 * t + c]; bv1[t] = b1[64 * wave + 16 * t + c]; }
    {   // observations of the row-block; rows beyond n and columns beyond O are zero
        const float *obs = sload(&M->obs);
        for (int i = threadIdx.x; i < RB * KL0; i += 256) {
            const int r = i / KL0, k = i - r * KL0;
            X0[lds_off(r, k, KL0)] = (row0 + r < n && k < O) ? obs[(size_t)(row0 + r) * O + k] : 0.f;
        }
    }
    lds_barrier();
    {
        f32x4 acc[4] = {};
        gemm_ring(r0, X0, KL0, KP >> 4, acc);
        act_hidden_epilogue<4>(acc, 64 * wave, 16, bv0, X1, H);
    }
    WRing<4> r1;
    r1.init(P + sload(&M->offW[1]), H, 64 * wave, 16);
    r1.fill(H >> 4);
    lds_barrier();
    {
        f32x4 acc[4] = {};
        gemm_ring(r1, X1, H, H >> 4, acc);
        act_hidden_epilogue<4>(acc, 64 * wave, 16, bv1, X2, H);
    }
    lds_barrier();
    if (16 * wave < NH) {                // head rows 16 wave .. 16 wave + 15 (wave-uniform)
        WRing<1> rh;
        rh.init(P + sload(&M->offW[2]), H, 16 * wave, 16);
        rh.fill(H >> 4);
        const float bh = (P + sload(&M->offB[2]))[16 * wave + c];
        f32x4 acc[1] = {};
        gemm_ring(rh, X2, H, H >> 4, acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) HL[(4 * g + i) * ACT_HEAD_LD + 16 * wave + c] = acc[0][i] + bh;
    }
    lds_barrier();
    const int r = threadIdx.x >> 4, a = threadIdx.x & 15;
    if (a < A && row0 + r < n) {
        const size_t o = (size_t)(row0 + r) * A + a;
        float v = HL[r * ACT_HEAD_LD + a];
        if (sload(&M->stochastic)) {
            const float ls = fminf(fmaxf(HL[r * ACT_HEAD_LD + A + a], LOG_SIG_MIN), LOG_SIG_MAX);
            v += expf(ls) * sload(&M->eps)[o];
        }
        sload(&M->act)[o] = tanhf(v);
    }
}

}  // namespace sac

namespace {

// the staging of acting calls (sac_trainer::act_stage), owned by the trainer that launches: the first of a call
int act_stage_reserve(sac_trainer *t, size_t bytes) {
    sac_trainer::ActStage &S = t->act_stage;
    if (S.bytes >= bytes) return 0;
    if (S.h) SAC_HIP(hipHostFree(S.h));
    S = sac_trainer::ActStage{};
    bytes = (bytes + 65535) & ~(size_t)65535;
    SAC_HIP(hipHostMalloc(reinterpret_cast<void **>(&S.h), bytes, hipHostMallocMapped));
    SAC_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&S.d), S.h, 0));
    S.bytes = bytes;
    return 0;
}

size_t act_lds_bytes(int KP) { return sizeof(float) * (size_t)RB * (((KP + 63) & ~63) + 2 * H + ACT_HEAD_LD); }

}  // namespace

// (declared extern "C" in include/sac_hip.h)
int sac_policy_act_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, const float *const *obs,
                        const int32_t *deterministic, const float *const *eps, float *const *act) {
    SAC_REQUIRE(trainers && n_rows && obs && deterministic && act, "bad arguments to sac_policy_act_many");
    SAC_REQUIRE(n_trainers >= 1 && n_trainers <= SAC_GROUP_MAX, "sac_policy_act_many takes 1..%d trainers (got %d)",
                SAC_GROUP_MAX, n_trainers);
    // every refusal comes first: nothing has changed when one of them returns
    bool stoch[SAC_GROUP_MAX];
    int active = 0;
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        SAC_REQUIRE(t, "trainer %d is null", i);
        for (int j = 0; j < i; ++j) SAC_REQUIRE(trainers[j] != t, "trainer %d is trainer %d again", i, j);
        SAC_REQUIRE(t->device == trainers[0]->device, "trainer %d lives on device %d, trainer 0 on device %d", i, t->device,
                    trainers[0]->device);
        SAC_REQUIRE(!t->gen, "trainer %d runs the general step (hidden sizes beyond two layers of at most 256 units): device "
                    "acting serves the fused kernels' shapes, sac_policy_act is the acting path for this trainer", i);
        SAC_REQUIRE(t->xcd_mask == 0xffu, "trainer %d is confined by sac_trainer_set_xcd[_mask]: device acting launches on the "
                    "whole chip", i);
        SAC_REQUIRE(n_rows[i] >= 0 && n_rows[i] <= ACT_MAX_ROWS, "trainer %d: %d rows (0..%d per call, 0 = sits out)", i,
                    (int)n_rows[i], ACT_MAX_ROWS);
        stoch[i] = t->algo == 0 && !deterministic[i];
        if (n_rows[i] == 0) continue;
        active += 1;
        SAC_REQUIRE(obs[i] && act[i], "trainer %d: null observations or actions", i);
        SAC_REQUIRE(!stoch[i] || (eps && eps[i]), "trainer %d: stochastic acting needs the N(0,1) draws (eps)", i);
    }
    SAC_REQUIRE(active > 0, "no trainer has rows to act on");
    sac_trainer *t0 = trainers[0];
    SAC_HIP(hipSetDevice(t0->device));
    // the weights as of the last completed step: drain every member, re-run what a fused step that gave up left undone
    for (int i = 0; i < n_trainers; ++i)
        if (n_rows[i] > 0 && sac_sync(trainers[i])) return -1;

    size_t off[SAC_GROUP_MAX][3], bytes = (sizeof(ActMember) * SAC_GROUP_MAX + 255) & ~(size_t)255;
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        const size_t n = (size_t)n_rows[i];
        const size_t part[3] = {n * t->O, stoch[i] ? n * t->A : 0, n * t->A};
        for (int k = 0; k < 3; ++k) { off[i][k] = bytes; bytes += (sizeof(float) * part[k] + 255) & ~(size_t)255; }
    }
    if (act_stage_reserve(t0, bytes)) return -1;
    const sac_trainer::ActStage &S = t0->act_stage;
    ActMember *tab = reinterpret_cast<ActMember *>(S.h);
    int blocks = 0, m = 0, kp_max = 0;
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        const Net &N = t->net[SAC_NET_POLICY];
        ActMember &M = tab[m++];
        M.P = N.P;
        M.obs = reinterpret_cast<const float *>(S.d + off[i][0]);
        M.eps = reinterpret_cast<const float *>(S.d + off[i][1]);
        M.act = reinterpret_cast<float *>(S.d + off[i][2]);
        for (int l = 0; l < 3; ++l) { M.offW[l] = N.L[l].offW; M.offB[l] = N.L[l].offB; }
        M.O = t->O; M.A = t->A; M.KP = t->KP; M.NH = t->NH;
        M.n = n_rows[i]; M.rb0 = blocks;
        M.stochastic = stoch[i] ? 1 : 0; M.pad = 0;
        blocks += (n_rows[i] + RB - 1) / RB;
        kp_max = std::max(kp_max, t->KP);
        memcpy(S.h + off[i][0], obs[i], sizeof(float) * (size_t)n_rows[i] * t->O);
        if (stoch[i]) memcpy(S.h + off[i][1], eps[i], sizeof(float) * (size_t)n_rows[i] * t->A);
    }
    const size_t lds = act_lds_bytes(kp_max);
    if (lds > 48 * 1024 && !t0->act_lds_raised) {
        SAC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_act), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)act_lds_bytes(512)));
        t0->act_lds_raised = true;
    }
    hipLaunchKernelGGL(k_act, dim3(blocks), dim3(256), lds, t0->stream, reinterpret_cast<const ActMember *>(S.d), m);
    SAC_HIP(hipGetLastError());
    if (wait_trainer_stream(t0)) return -1;
    for (int i = 0; i < n_trainers; ++i)
        if (n_rows[i] > 0) memcpy(act[i], S.h + off[i][2], sizeof(float) * (size_t)n_rows[i] * trainers[i]->A);
    return 0;
}

int sac_policy_act_device(sac_trainer_t *t, int64_t n, const float *obs, int deterministic, const float *eps, float *act) {
    SAC_REQUIRE(t && obs && act, "bad arguments to sac_policy_act_device");
    SAC_REQUIRE(n >= 1 && n <= ACT_MAX_ROWS, "sac_policy_act_device: %lld rows (1..%d per call)", (long long)n, ACT_MAX_ROWS);
    const int32_t rows = (int32_t)n, det = deterministic;
    return sac_policy_act_many(&t, 1, &rows, &obs, &det, &eps, &act);
}
