// Evaluating the critics on the device: Q_net(obs, act) from the trainer's own weights (included by sac_trainer.hip).
//
// k_qval is the forward pass of the Q networks alone -- FlattenMlp over cat(obs, act) with the fused kernels' shapes: two
// hidden layers of at most 256 units, zero-padded to 256 as in the step -- for 1..1024 (obs, act) rows, any non-empty
// subset of {qf1, qf2, target_qf1, target_qf2}, of each of 1..SAC_GROUP_MAX trainers (SAC and TD3) in ONE launch.  It
// reads the nets' forward copies Net::P where the step kernels keep them (padded, fragment-major: frag_off; first layer
// over [obs | pad | act | pad], KQ = KP + 16 columns); nothing is repacked, mirrored or copied.
//
//   grid    one workgroup (4 waves) per (member, selected net, 16-row block); the workgroups of all members side by
//           side -- a member's nets one behind the other, each with its row-blocks -- found through the per-member
//           table QvalMember (device-visible memory, read with scalar loads)
//   LDS     the row-block's input [16][round_up(KQ, 64)]: observations in columns 0..O-1, actions in columns
//           KP..KP+A-1, zeros elsewhere and in the rows beyond n; both hidden layers [16][256]; the output column [16]
//   math    the pieces of sac_infer.h: infer_fill, infer_hidden (a NaN row stays NaN as in torch), infer_q_out (the
//           last layer is row 0 of its padded [16][256] matrix: wave 0, one tile)
//
// Row independence.  A row's Q value is a function of that row's observation and action and the net's weights only:
// every output element is one MFMA dot product over k in ascending chunks, and neither the row's place in its block,
// nor the number of rows, nor which other nets are selected, nor the other members of the launch enter it.  Rows
// beyond a member's n are zero padding and are never written.  Grouped evaluation is therefore bit for bit solo
// evaluation, and row r of any call the one-row call of that row (tests/test_gpu_q_values.py).
//
// The kernel writes the caller's Q values and nothing else: nothing the step kernels read.  Inputs, outputs and the
// member table live in the trainer's mapped pinned staging (act_stage_reserve, sac_infer.h): a call is one launch and one
// wait, without a copy call of its own.
//
// General-step trainers (hidden sizes beyond the fused kernels') are out of scope here: these entries refuse them.  Their
// Q values come from the host (sac_get_params and a forward there: SACTrainer.q_values' default) or from the device
// through sac_q_values_general[_many] (k_qval_layer, sac_qval_general.h: one launch per layer, as k_act_layer), which in
// turn refuses the shapes served here.
#pragma once

namespace sac {

struct QvalMember {
    const float *P[4];             // forward copies (Net::P) of the SELECTED nets, in ascending SAC_NET_* order
    const float *obs, *act;        // (n, O) / (n, A) row-major
    float *q;                      // (n_sel, n): one row of n values per selected net
    long long offW[3], offB[3];    // the three layers inside P (the four Q nets share their layout)
    int O, A, KP, n;
    int n_sel, wg0;                // selected nets; first workgroup of this member in the launch
};

__global__ __launch_bounds__(256) void k_qval(const QvalMember *__restrict__ tab, int n_members) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const QvalMember *M = tab + infer_member(tab, n_members, &QvalMember::wg0);
    const int O = sload(&M->O), A = sload(&M->A), KP = sload(&M->KP), n = sload(&M->n);
    const int KQ = KP + 16, nrb = (n + RB - 1) / RB;
    const int local = (int)blockIdx.x - sload(&M->wg0);
    const int sel = local / nrb, row0 = (local - sel * nrb) * RB;      // which selected net, which row-block
    const float *P = sload(&M->P[sel]);
    const int KL0 = (KQ + 63) & ~63;
    float *X0 = lds;                     // [16][KL0]
    float *X1 = X0 + RB * KL0;           // [16][256]
    float *X2 = X1 + RB * H;             // [16][256]
    float *QL = X2 + RB * H;             // [16]
    infer_hidden(P, M->offW, M->offB, X0, KL0, KQ, X1, X2,
                 [&] { infer_fill(X0, KL0, row0, n, sload(&M->obs), O, sload(&M->act), KP, A); });
    infer_q_out(P, M->offW, M->offB, X2, QL);
    if (threadIdx.x < RB && row0 + (int)threadIdx.x < n)
        sload(&M->q)[(size_t)sel * n + row0 + threadIdx.x] = QL[threadIdx.x];
}

}  // namespace sac

namespace {

size_t qval_lds_bytes(int KQ) { return sizeof(float) * (size_t)RB * (((KQ + 63) & ~63) + 2 * H + 1); }

std::atomic<bool> g_qval_lds_raised[64];

// What sac_q_values_many and sac_q_values_general_many do alike in front of their tables: the refusals and the drain
// (infer_admit)
int qval_admit(const InferEntry &E, sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
               const float *const *obs, const float *const *act, const uint32_t *nets, float *const *q) {
    return infer_admit(E, trainers, n_trainers, n_rows, [&](int i) {
        SAC_REQUIRE(nets[i] != 0 && nets[i] <= 15u, "trainer %d: nets 0x%x selects no Q network or an unknown one (bits "
                    "SAC_Q_QF1 | SAC_Q_QF2 | SAC_Q_TARGET_QF1 | SAC_Q_TARGET_QF2)", i, (unsigned)nets[i]);
        SAC_REQUIRE(obs[i] && act[i] && q[i], "trainer %d: null observations, actions or Q values", i);
        return 0;
    });
}

// The staging behind the call's table (`bytes` so far): per member obs (n, O), act (n, A), q (selected nets, n).
void qval_carve(size_t &bytes, size_t (*off)[3], sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows,
                const uint32_t *nets) {
    for (int i = 0; i < n_trainers; ++i) {
        const size_t n = (size_t)n_rows[i];
        const size_t part[3] = {n * trainers[i]->O, n * trainers[i]->A, n ? n * __builtin_popcount(nets[i]) : 0};
        infer_carve(bytes, off[i], part, 3);
    }
}

}  // namespace

// (declared extern "C" in include/sac_hip.h)
int sac_q_values_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, const float *const *obs,
                      const float *const *act, const uint32_t *nets, float *const *q) {
    SAC_REQUIRE(trainers && n_rows && obs && act && nets && q, "bad arguments to sac_q_values_many");
    const InferEntry E = {"sac_q_values_many", false, false, "device Q evaluation",
                          "sac_get_params and a forward on the host is the path", "evaluate"};
    if (int rc = qval_admit(E, trainers, n_trainers, n_rows, obs, act, nets, q)) return rc;
    sac_trainer *t0 = trainers[0];
    size_t off[SAC_GROUP_MAX][3], bytes = infer_align(sizeof(QvalMember) * SAC_GROUP_MAX);
    qval_carve(bytes, off, trainers, n_trainers, n_rows, nets);
    if (act_stage_reserve(t0, bytes)) return -1;
    const sac_trainer::ActStage &S = t0->act_stage;
    QvalMember *tab = reinterpret_cast<QvalMember *>(S.h);
    int wgs = 0, m = 0, kq_max = 0;
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        QvalMember &M = tab[m++];
        M.n_sel = 0;
        for (int k = 0; k < 4; ++k) {
            M.P[k] = nullptr;
            if (nets[i] >> k & 1u) M.P[M.n_sel++] = t->net[SAC_NET_QF1 + k].P;
        }
        M.obs = reinterpret_cast<const float *>(S.d + off[i][0]);
        M.act = reinterpret_cast<const float *>(S.d + off[i][1]);
        M.q = reinterpret_cast<float *>(S.d + off[i][2]);
        const Net &N = t->net[SAC_NET_QF1];
        for (int l = 0; l < 3; ++l) { M.offW[l] = N.L[l].offW; M.offB[l] = N.L[l].offB; }
        M.O = t->O; M.A = t->A; M.KP = t->KP; M.n = n_rows[i];
        M.wg0 = wgs;
        wgs += M.n_sel * ((n_rows[i] + RB - 1) / RB);
        kq_max = std::max(kq_max, t->KQ);
        memcpy(S.h + off[i][0], obs[i], sizeof(float) * (size_t)n_rows[i] * t->O);
        memcpy(S.h + off[i][1], act[i], sizeof(float) * (size_t)n_rows[i] * t->A);
    }
    const size_t lds = qval_lds_bytes(kq_max);
    if (infer_raise_lds(reinterpret_cast<const void *>(k_qval), g_qval_lds_raised, t0->device, lds, qval_lds_bytes(512))) return -1;
    hipLaunchKernelGGL(k_qval, dim3(wgs), dim3(256), lds, t0->stream, reinterpret_cast<const QvalMember *>(S.d), m);
    SAC_HIP(hipGetLastError());
    if (wait_trainer_stream(t0)) return -1;
    for (int i = 0; i < n_trainers; ++i)
        if (n_rows[i] > 0)
            memcpy(q[i], S.h + off[i][2], sizeof(float) * (size_t)n_rows[i] * __builtin_popcount(nets[i]));
    return 0;
}

int sac_q_values(sac_trainer_t *t, int64_t n, const float *obs, const float *act, uint32_t nets, float *q) {
    SAC_REQUIRE(t && obs && act && q, "bad arguments to sac_q_values");
    SAC_REQUIRE(n >= 1 && n <= ACT_MAX_ROWS, "sac_q_values: %lld rows (1..%d per call)", (long long)n, ACT_MAX_ROWS);
    const int32_t rows = (int32_t)n;
    return sac_q_values_many(&t, 1, &rows, &obs, &act, &nets, &q);
}
