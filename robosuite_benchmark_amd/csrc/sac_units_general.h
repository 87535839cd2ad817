// Per-unit statistics of the hidden layers for general-step trainers: sac_unit_moments_general[_many] (included by
// sac_trainer.hip behind sac_units.h).
//
// No forward kernel of its own: a hidden layer of any net -- the policy's too, with K1 = K -- is a QvalLayerJob, "one
// layer Y = relu(X W^T + b) with a split input".  Per depth l the entry builds the jobs of every (member, selected net)
// that has a HIDDEN layer l -- no output layer, no head --, launches k_qval_layer unchanged, then k_unit_moments on that
// depth's outputs, then depth l + 1: two launches per depth on the first member's stream and one wait at the end.
//
//   Y       without io->activations the trainer's act_gen ping-pong pair (act_general_reserve), one slice per selected
//           net of n x the widest hidden layer selected: stream order keeps reducer l in front of layer l + 2's writes.
//           With io->activations the staging's output block itself, (n, N_l) row-major per net and layer: no copy kernel.
//   records the mapped staging, per selected net in ascending id, per hidden layer: SAC_UNIT_FIELDS_N arrays of N_l
//
// The activations are k_qval_layer's (the policy's: the same tile, so k_act_layer's values): row independence, grouped ==
// solo and n rows == n one-row calls carry over, and the reducer's order depends on n alone.  The entry writes the
// members' activation scratch and the caller's outputs: nothing the step kernels read, and no generator.
#pragma once

// (declared extern "C" in include/sac_hip.h)
int sac_unit_moments_general_many(sac_trainer_t *const *trainers, int n_trainers, const int32_t *n_rows, sac_units_io_t *io) {
    SAC_REQUIRE(trainers && n_rows && io, "bad arguments to sac_unit_moments_general_many");
    const InferEntry E = {"sac_unit_moments_general_many", true, false, "device unit statistics",
                          "sac_unit_moments is its device unit statistics entry, sac_unit_moments_general serves the general step",
                          "reduce"};
    if (int rc = units_admit(E, trainers, n_trainers, n_rows, io)) return rc;
    sac_trainer *t0 = trainers[0];
    // staging: the two job tables, then per member obs (n, O), act (n, A), the records, the activations asked for
    const size_t tab_q = 0, tab_u = infer_align(sizeof(QvalLayerJob) * UNIT_JOBS * gen::GMAXL);
    size_t bytes = tab_u + infer_align(sizeof(UnitJob) * UNIT_JOBS * gen::GMAXL);
    size_t off[SAC_GROUP_MAX][4] = {}, slice[SAC_GROUP_MAX] = {}, units[SAC_GROUP_MAX] = {};
    int launches = 0;
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        const size_t n = (size_t)n_rows[i];
        int widest = 1;
        for (int k = 0; k < UNIT_NETS; ++k) {
            if (!(io[i].nets >> k & 1u)) continue;
            const GenNet &G = t->gen->net[k];
            for (int l = 0; l + 1 < G.nl; ++l) units[i] += (size_t)G.L[l].N;
            widest = std::max(widest, infer_widest(G));
            launches = std::max(launches, G.nl - 1);
        }
        slice[i] = n * widest;
        bytes = infer_align(bytes);
        off[i][0] = bytes; bytes += infer_align(sizeof(float) * n * t->O);
        off[i][1] = bytes; bytes += infer_align(sizeof(float) * n * t->A);
        off[i][2] = bytes; bytes += infer_align(sizeof(double) * SAC_UNIT_FIELDS_N * units[i]);
        off[i][3] = bytes; bytes += io[i].activations ? infer_align(sizeof(float) * n * units[i]) : 0;
        if (!io[i].activations && act_general_reserve(trainers[i], slice[i] * __builtin_popcount(io[i].nets))) return -1;
    }
    if (act_stage_reserve(t0, bytes)) return -1;
    const sac_trainer::ActStage &S = t0->act_stage;
    QvalLayerJob *qtab = reinterpret_cast<QvalLayerJob *>(S.h + tab_q);
    UnitJob *utab = reinterpret_cast<UnitJob *>(S.h + tab_u);
    int njobs[gen::GMAXL] = {}, qblocks[gen::GMAXL] = {}, ublocks[gen::GMAXL] = {};
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        const size_t n = (size_t)n_rows[i];
        const float *o = reinterpret_cast<const float *>(S.d + off[i][0]);
        const float *a = reinterpret_cast<const float *>(S.d + off[i][1]);
        double *rec = reinterpret_cast<double *>(S.d + off[i][2]);
        float *taps = io[i].activations ? reinterpret_cast<float *>(S.d + off[i][3]) : nullptr;
        int s = 0;
        for (int k = 0; k < UNIT_NETS; ++k) {
            if (!(io[i].nets >> k & 1u)) continue;
            const GenNet &G = t->gen->net[k];
            const bool q = (UNIT_Q_NETS >> k & 1u) != 0;
            const float *x = o, *x2 = q ? a : o;
            for (int l = 0; l + 1 < G.nl; ++l) {
                const GenLayer &L = G.L[l];
                const size_t slot = (size_t)l * UNIT_JOBS + njobs[l];
                QvalLayerJob &J = qtab[slot];
                infer_layer_job(J, G, L);
                J.X = x; J.X2 = x2;
                J.Y = taps ? taps : t->act_gen[l & 1] + (size_t)s * slice[i];
                J.K1 = (l == 0 && q) ? t->O : L.K; J.n = n_rows[i];
                J.wg0 = qblocks[l];
                J.relu = 1;
                qblocks[l] += ((n_rows[i] + RB - 1) / RB) * J.tiles_n;
                UnitJob &U = utab[slot];
                U.X = J.Y; U.out = rec; U.ld = L.N; U.N = L.N; U.n = n_rows[i];
                U.wg0 = ublocks[l];
                ublocks[l] += (L.N + UM_COLS - 1) / UM_COLS;
                njobs[l] += 1;
                x = x2 = J.Y;
                rec += (size_t)SAC_UNIT_FIELDS_N * L.N;
                if (taps) taps += n * L.N;
            }
            s += 1;
        }
        memcpy(S.h + off[i][0], io[i].obs, sizeof(float) * n * t->O);
        if (io[i].nets & UNIT_Q_NETS) memcpy(S.h + off[i][1], io[i].act, sizeof(float) * n * t->A);
    }
    for (int l = 0; l < launches; ++l) {
        hipLaunchKernelGGL(k_qval_layer, dim3(qblocks[l]), dim3(256), 0, t0->stream,
                           reinterpret_cast<const QvalLayerJob *>(S.d + tab_q) + (size_t)l * UNIT_JOBS, njobs[l]);
        SAC_HIP(hipGetLastError());
        if (units_launch(t0, reinterpret_cast<const UnitJob *>(S.d + tab_u) + (size_t)l * UNIT_JOBS, njobs[l], ublocks[l])) return -1;
    }
    if (wait_trainer_stream(t0)) return -1;
    for (int i = 0; i < n_trainers; ++i) {
        if (n_rows[i] == 0) continue;
        memcpy(io[i].moments, S.h + off[i][2], sizeof(double) * SAC_UNIT_FIELDS_N * units[i]);
        if (io[i].activations) memcpy(io[i].activations, S.h + off[i][3], sizeof(float) * (size_t)n_rows[i] * units[i]);
    }
    return 0;
}

int sac_unit_moments_general(sac_trainer_t *t, int64_t n, sac_units_io_t *io) {
    SAC_REQUIRE(t && io, "bad arguments to sac_unit_moments_general");
    SAC_REQUIRE(n >= 1 && n <= ACT_MAX_ROWS, "sac_unit_moments_general: %lld rows (1..%d per call)", (long long)n, ACT_MAX_ROWS);
    const int32_t rows = (int32_t)n;
    return sac_unit_moments_general_many(&t, 1, &rows, io);
}
