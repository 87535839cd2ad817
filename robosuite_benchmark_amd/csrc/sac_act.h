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
//   math    the pieces of sac_infer.h: infer_fill, infer_hidden (fp32 MFMA 16x16x4 through the step kernels' weight
//           ring), infer_head, infer_action -- SAC: tanh(mean) | tanh(mean + exp(clamp(log_std, -20, 2)) * eps);
//           TD3: tanh(last_fc)
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

struct ActMember {
    const float *P;                // the policy's forward copy (Net::P)
    const float *obs, *eps;        // (n, O) / (n, A) row-major (eps unused unless SAC and stochastic)
    float *act;                    // (n, A)
    long long offW[3], offB[3];    // the three layers inside P
    int O, A, KP, NH;              // NH: padded head rows (SAC: mean + log_std; TD3: last_fc)
    int n, rb0;                    // rows; first workgroup of this member in the launch
    int stochastic, pad;           // 1: SAC with exploration noise
};

__global__ __launch_bounds__(256) void k_act(const ActMember *__restrict__ tab, int n_members) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const ActMember *M = tab + infer_member(tab, n_members, &ActMember::rb0);
    const float *P = sload(&M->P);
    const int O = sload(&M->O), A = sload(&M->A), KP = sload(&M->KP), NH = sload(&M->NH), n = sload(&M->n);
    const int row0 = ((int)blockIdx.x - sload(&M->rb0)) * RB;
    const int KL0 = (KP + 63) & ~63;
    float *X0 = lds;                     // [16][KL0]
    float *X1 = X0 + RB * KL0;           // [16][256]
    float *X2 = X1 + RB * H;             // [16][256]
    float *HL = X2 + RB * H;             // [16][32]
    infer_hidden(P, M->offW, M->offB, X0, KL0, KP, X1, X2, [&] { infer_fill(X0, KL0, row0, n, sload(&M->obs), O); });
    infer_head(P, M->offW, M->offB, NH, X2, HL);
    const int r = threadIdx.x >> 4, a = threadIdx.x & 15;
    if (a < A && row0 + r < n) {
        const size_t o = (size_t)(row0 + r) * A + a;
        sload(&M->act)[o] = infer_action(HL, r, a, A, sload(&M->stochastic) != 0, [&] { return sload(&M->eps)[o]; });
    }
}

}  // namespace sac

namespace {

size_t act_lds_bytes(int KP) { return sizeof(float) * (size_t)RB * (((KP + 63) & ~63) + 2 * H + ACT_HEAD_LD); }

std::atomic<bool> g_act_lds_raised[64];

// What sac_policy_act_many and sac_policy_act_general_many do alike in front of their tables.  The refusals and the
// drain (infer_admit); stoch[i]: member i has rows and is a SAC trainer acting with exploration noise.
int act_admit(const InferEntry &E, sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
              const float *const *obs, const int32_t *deterministic, const float *const *eps, float *const *act, bool *stoch) {
    return infer_admit(E, trainers, n_trainers, n_rows, [&](int i) {
        stoch[i] = trainers[i]->algo == 0 && !deterministic[i];
        SAC_REQUIRE(obs[i] && act[i], "trainer %d: null observations or actions", i);
        SAC_REQUIRE(!stoch[i] || (eps && eps[i]), "trainer %d: stochastic acting needs the N(0,1) draws (eps)", i);
        return 0;
    });
}

// The staging behind the call's table (`bytes` so far): per member obs (n, O), eps (n, A) where stochastic, act (n, A).
void act_carve(size_t &bytes, size_t (*off)[3], sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
               const bool *stoch) {
    for (int i = 0; i < n_trainers; ++i) {
        const size_t n = (size_t)n_rows[i];
        const size_t part[3] = {n * trainers[i]->O, stoch[i] ? n * trainers[i]->A : 0, n * trainers[i]->A};
        infer_carve(bytes, off[i], part, 3);
    }
}

}  // namespace

// (declared extern "C" in include/sac_hip.h)
int sac_policy_act_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, const float *const *obs,
                        const int32_t *deterministic, const float *const *eps, float *const *act) {
    SAC_REQUIRE(trainers && n_rows && obs && deterministic && act, "bad arguments to sac_policy_act_many");
    const InferEntry E = {"sac_policy_act_many", false, false, "device acting", "sac_policy_act is the acting path", "act on"};
    bool stoch[SAC_GROUP_MAX] = {};
    if (int rc = act_admit(E, trainers, n_trainers, n_rows, obs, deterministic, eps, act, stoch)) return rc;
    sac_trainer *t0 = trainers[0];
    size_t off[SAC_GROUP_MAX][3], bytes = infer_align(sizeof(ActMember) * SAC_GROUP_MAX);
    act_carve(bytes, off, trainers, n_trainers, n_rows, stoch);
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
    if (infer_raise_lds(reinterpret_cast<const void *>(k_act), g_act_lds_raised, t0->device, lds, act_lds_bytes(512))) return -1;
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
