// Evaluating the SAC objectives on REPLAY rows in place: the input rows of an evaluation taken from the replay storage on
// the device (included by sac_trainer.hip in front of sac_eval.h).
//
// k_eval_rows copies, for 1..1024 storage rows idx[j] of each of 1..SAC_GROUP_MAX members' replay buffers in ONE launch,
// the five arrays of a transition out of the strided storage (ReplayView: row strides Ost / Ast, multiples of 4 floats)
// into the DENSE input parts of the evaluation staging -- obs (n, O), act (n, A), rew (n), term (n), nobs (n, O) -- the
// parts eval_fused_many (sac_eval.h) and eval_general_many (sac_eval_general.h) otherwise fill with the caller's
// arrays.  The layout infer_fill and k_eval_layer read is unchanged, so k_eval, k_eval_layer, k_eval_y and
// k_eval_moments run behind it as they are, and the columns are bit for bit those of an evaluation of the gathered batch.
//
//   grid    one workgroup (4 waves) per (member, 16-row block), the workgroups of all members side by side, found
//           through the per-member table EvalRowsMember (in the staging, read with scalar loads: infer_member)
//   rows    a wave owns rows wave, wave + 4, wave + 8, wave + 12 of its block: the row's index is loaded ONCE (all lanes
//           one address: one request), then the lanes walk the row's elements side by side -- coalesced loads, coalesced
//           dense stores
//   bounds  none beyond j < n: the host has checked every index against [0, size) in front of the launch
//           (eval_rows_admit), so the kernel cannot read outside the storage
// No LDS, no atomics, no word shared between workgroups.  Vector stores only.
//
// Ordering against the asynchronous ingest (sac_buffer_add*: copies on the buffer's own stream): each distinct buffer
// of the call records an event on its stream, behind whatever is pending there, and the trainer's stream waits for it
// in front of the launch.  The buffer's rows are only read; its generator, its bound host words, its read-ahead and its
// loop speculation are not looked at.
#pragma once

namespace sac {

constexpr int ER_ROWS = 16;               // rows of one k_eval_rows workgroup: four per wave

struct EvalRowsMember {
    ReplayView rv;
    const int64_t *idx;                        // [n] storage rows (in the staging)
    float *obs, *act, *rew, *term, *nobs;      // the dense input parts of the evaluation staging
    int n, wg0;                                // rows; first workgroup of this member in the launch
};

__global__ __launch_bounds__(256) void k_eval_rows(const EvalRowsMember *__restrict__ tab, int n_members) {
    typedef __attribute__((address_space(1))) float *gout;
    typedef const __attribute__((address_space(1))) int64_t *gidx;
    const EvalRowsMember *M = tab + infer_member(tab, n_members, &EvalRowsMember::wg0);
    const int n = sload(&M->n), O = sload(&M->rv.O), A = sload(&M->rv.A);
    const size_t Ost = (size_t)sload(&M->rv.Ost), Ast = (size_t)sload(&M->rv.Ast);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row0 = ((int)blockIdx.x - sload(&M->wg0)) * ER_ROWS + wave;
    const int64_t *idx = sload(&M->idx);
    // the four rows' indices first (rows beyond n repeat row n - 1 and are not copied): four requests in flight
    size_t src[ER_ROWS / 4];
#pragma unroll
    for (int q = 0; q < ER_ROWS / 4; ++q) src[q] = (size_t)*(gidx)(uintptr_t)(idx + min(row0 + 4 * q, n - 1));
    const float *s_obs = sload(&M->rv.obs), *s_nobs = sload(&M->rv.nobs), *s_act = sload(&M->rv.act);
    const float *s_rew = sload(&M->rv.rew), *s_term = sload(&M->rv.term);
    float *d_obs = sload(&M->obs), *d_nobs = sload(&M->nobs), *d_act = sload(&M->act);
    float *d_rew = sload(&M->rew), *d_term = sload(&M->term);
#pragma unroll
    for (int q = 0; q < ER_ROWS / 4; ++q) {
        const int j = row0 + 4 * q;
        if (j >= n) break;                // (wave-uniform)
        const size_t s = src[q];
        const float *po = s_obs + s * Ost, *pn = s_nobs + s * Ost, *pa = s_act + s * Ast;
        for (int k = lane; k < O; k += 64) {
            const float vo = ld1g(po + k), vn = ld1g(pn + k);
            *(gout)(uintptr_t)(d_obs + ((size_t)j * O + k)) = vo;
            *(gout)(uintptr_t)(d_nobs + ((size_t)j * O + k)) = vn;
        }
        for (int k = lane; k < A; k += 64) *(gout)(uintptr_t)(d_act + ((size_t)j * A + k)) = ld1g(pa + k);
        if (lane == 0) {
            *(gout)(uintptr_t)(d_rew + j) = ld1g(s_rew + s);
            *(gout)(uintptr_t)(d_term + j) = ld1g(s_term + s);
        }
    }
}

}  // namespace sac

namespace {

// where a call's k_eval_rows table and its members' indices lie in the staging
struct EvalRowsStage { size_t tab = 0, idx[SAC_GROUP_MAX] = {}; };

// the replay entries' own refusals for member i with n rows: eps and eps_next (and `rows` unless the entry returns
// statistics) -- the five input arrays of io are not looked at -- then the source (eval_rows_admit_src): a buffer and
// indices, the buffer on the trainer's device, of its dims and not empty, every index inside [0, size)
int eval_rows_admit_src(const sac_eval_src_t &R, const sac_trainer *t, int i, int n) {
    SAC_REQUIRE(R.buf && R.idx, "trainer %d: a null replay buffer or null indices", i);
    const sac_buffer *b = R.buf;
    SAC_REQUIRE(b->device == t->device, "trainer %d lives on device %d, its replay buffer on device %d", i, t->device, b->device);
    SAC_REQUIRE(b->O == t->O && b->A == t->A, "trainer %d: its replay buffer has dims (%d, %d), the trainer (%d, %d)", i,
                b->O, b->A, t->O, t->A);
    SAC_REQUIRE(b->size > 0, "trainer %d: its replay buffer is empty", i);
    for (int j = 0; j < n; ++j)
        SAC_REQUIRE(R.idx[j] >= 0 && R.idx[j] < b->size, "trainer %d: index %lld (row %d) out of range [0, %lld)", i,
                    (long long)R.idx[j], j, (long long)b->size);
    return 0;
}

int eval_rows_admit(const sac_eval_io_t &E, const sac_eval_src_t &R, const sac_trainer *t, int i, int n, bool need_rows) {
    const bool inputs = E.eps && E.eps_next;
    if (need_rows) SAC_REQUIRE(inputs && E.rows, "trainer %d: null eps, eps_next or rows", i);
    SAC_REQUIRE(inputs, "trainer %d: null eps or eps_next", i);
    return eval_rows_admit_src(R, t, i, n);
}

// the same for the TD3 objective's single draw (td3_eval.h, td3_eval_general.h)
int eval_rows_admit(const td3_eval_io_t &E, const sac_eval_src_t &R, const sac_trainer *t, int i, int n, bool need_rows) {
    if (need_rows) SAC_REQUIRE(E.eps && E.rows, "trainer %d: null eps or rows", i);
    SAC_REQUIRE(E.eps, "trainer %d: null eps", i);
    return eval_rows_admit_src(R, t, i, n);
}

void eval_rows_carve(size_t &bytes, EvalRowsStage &RS, int n_trainers, const int32_t *n_rows) {
    RS.tab = bytes;
    bytes += infer_align(sizeof(EvalRowsMember) * SAC_GROUP_MAX);
    for (int i = 0; i < n_trainers; ++i) {
        const size_t part = (size_t)n_rows[i];
        infer_carve(bytes, &RS.idx[i], &part, 1, sizeof(int64_t));
    }
}

// entry m of the table: trainer i's n rows from R into the five dense parts (device addresses of the staging); the
// indices go into the staging here.  Returns the workgroups of this member.
int eval_rows_member(const sac_trainer::ActStage &S, const EvalRowsStage &RS, int m, int i, int wg0, const sac_eval_src_t &R,
                     int n, float *obs, float *act, float *rew, float *term, float *nobs) {
    EvalRowsMember &M = reinterpret_cast<EvalRowsMember *>(S.h + RS.tab)[m];
    memcpy(S.h + RS.idx[i], R.idx, sizeof(int64_t) * (size_t)n);
    M.rv = R.buf->view();
    M.idx = reinterpret_cast<const int64_t *>(S.d + RS.idx[i]);
    M.obs = obs; M.act = act; M.rew = rew; M.term = term; M.nobs = nobs;
    M.n = n; M.wg0 = wg0;
    return (n + ER_ROWS - 1) / ER_ROWS;
}

// the launch on t0's stream, behind what is pending on the stream of every distinct buffer of the call
int eval_rows_launch(sac_trainer *t0, const EvalRowsStage &RS, int m, int wgs, const sac_eval_src_t *src, int n_trainers,
                     const int32_t *n_rows) {
    for (int i = 0; i < n_trainers; ++i) {
        if (n_rows[i] == 0) continue;
        sac_buffer *b = src[i].buf;
        bool seen = false;
        for (int j = 0; j < i; ++j) seen = seen || (n_rows[j] > 0 && src[j].buf == b);
        if (seen) continue;
        if (!b->eval_ev) SAC_HIP(hipEventCreateWithFlags(&b->eval_ev, hipEventDisableTiming));
        SAC_HIP(hipEventRecord(b->eval_ev, b->stream));
        SAC_HIP(hipStreamWaitEvent(t0->stream, b->eval_ev, 0));
    }
    hipLaunchKernelGGL(k_eval_rows, dim3(wgs), dim3(256), 0, t0->stream,
                       reinterpret_cast<const EvalRowsMember *>(t0->act_stage.d + RS.tab), m);
    SAC_HIP(hipGetLastError());
    return 0;
}

}  // namespace
