// Per-unit statistics of the hidden layers for general-step trainers: sac_unit_moments_general[_many] (included by
// sac_trainer.hip behind sac_units.h).
//
// No forward kernel of its own: a hidden layer of any net -- the policy's too, with K1 = K -- is a LAYER_STORE job, "one
// layer Y = relu(X W^T + b) with a split input".  Per (member, selected net) the entry appends one chain WITHOUT its last
// layer to a LayerSchedule (sac_infer.h) -- no output layer, no head -- and gives every job its UnitJob in the same slot
// of the reducer's table; per depth l it launches k_qval_layer unchanged, then k_unit_moments on that depth's outputs,
// then depth l + 1: two launches per depth on the first member's stream and one wait at the end.
//
//   Y       without io->activations the trainer's act_gen ping-pong pair (infer_scratch_reserve), one slice per selected
//           net of n x the widest hidden layer selected: stream order keeps reducer l in front of layer l + 2's writes.
//           With io->activations the staging's output block itself, (n, N_l) row-major per net and layer: no copy kernel.
//   records the mapped staging (InferStage, a part of doubles), per selected net in ascending id, per hidden layer:
//           SAC_UNIT_FIELDS_N arrays of N_l
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
    // the staging: the layer jobs' tables and the reducer's (slot for slot the same jobs), then per member obs (n, O),
    // act (n, A), the records (double), the activations asked for
    enum { P_OBS, P_ACT, P_REC, P_TAPS, NPART };
    LayerSchedule LS(UNIT_JOBS);
    const size_t tab_u = LS.bytes();
    InferStage ST(tab_u + infer_align(sizeof(UnitJob) * UNIT_JOBS * gen::GMAXL));
    size_t slice[SAC_GROUP_MAX] = {};
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        const size_t n = (size_t)n_rows[i];
        size_t units = 0;
        int widest = 1;
        for (int k = 0; n && k < UNIT_NETS; ++k) {
            if (!(io[i].nets >> k & 1u)) continue;
            const GenNet &G = t->gen->net[k];
            for (int l = 0; l + 1 < G.nl; ++l) units += (size_t)G.L[l].N;
            widest = std::max(widest, infer_widest(G));
        }
        const size_t part[NPART] = {n * t->O, n * t->A, SAC_UNIT_FIELDS_N * units, n && io[i].activations ? n * units : 0};
        const size_t elem[NPART] = {sizeof(float), sizeof(float), sizeof(double), sizeof(float)};
        ST.carve(i, part, NPART, elem);
        if (n && !io[i].activations &&
            infer_scratch_reserve(trainers[i], n_rows[i], widest, __builtin_popcount(io[i].nets), &slice[i])) return -1;
    }
    if (ST.reserve(t0)) return -1;
    LS.bind(ST.S->h, ST.S->d);
    UnitJob *utab = reinterpret_cast<UnitJob *>(ST.S->h + tab_u);
    int ublocks[gen::GMAXL] = {};
    for (int i = 0; i < n_trainers; ++i) {
        const sac_trainer *t = trainers[i];
        if (n_rows[i] == 0) continue;
        const size_t n = (size_t)n_rows[i];
        const float *o = ST.in(i, P_OBS, io[i].obs), *a = ST.in(i, P_ACT, (io[i].nets & UNIT_Q_NETS) ? io[i].act : nullptr);
        double *rec = ST.dev<double>(i, P_REC);
        float *taps = ST.dev(i, P_TAPS, io[i].activations != nullptr);
        int s = 0;
        for (int k = 0; k < UNIT_NETS; ++k) {
            if (!(io[i].nets >> k & 1u)) continue;
            const bool q = (UNIT_Q_NETS >> k & 1u) != 0;
            // the hidden layers only; with activations a layer writes its (n, N_l) block of the staging instead of the scratch
            LS.chain({t->gen->net[k], o, q ? a : o, t->O, n_rows[i], t->act_gen, taps ? 0 : s * slice[i], nullptr, false},
                     [&](sac::LayerJob &J, int l) {
                if (taps) { J.Y = taps; taps += n * J.N; }
                UnitJob &U = utab[(size_t)l * UNIT_JOBS + LS.njobs[l] - 1];       // the job's own slot
                U.X = J.Y; U.out = rec; U.ld = J.N; U.N = J.N; U.n = n_rows[i];
                U.wg0 = ublocks[l];
                ublocks[l] += (J.N + UM_COLS - 1) / UM_COLS;
                rec += (size_t)SAC_UNIT_FIELDS_N * J.N;
            });
            s += 1;
        }
    }
    const UnitJob *d_utab = reinterpret_cast<const UnitJob *>(ST.S->d + tab_u);
    for (int l = 0; l < LS.launches; ++l)
        if (LS.launch(k_qval_layer, t0, l) || units_launch(t0, d_utab + (size_t)l * UNIT_JOBS, LS.njobs[l], ublocks[l])) return -1;
    if (wait_trainer_stream(t0)) return -1;
    for (int i = 0; i < n_trainers; ++i)
        if (n_rows[i] > 0) ST.back(i, {{io[i].moments, P_REC}, {io[i].activations, P_TAPS}});
    return 0;
}

int sac_unit_moments_general(sac_trainer_t *t, int64_t n, sac_units_io_t *io) {
    SAC_REQUIRE(t && io, "bad arguments to sac_unit_moments_general");
    if (int rc = infer_admit_solo("sac_unit_moments_general", n)) return rc;
    const int32_t rows = (int32_t)n;
    return sac_unit_moments_general_many(&t, 1, &rows, io);
}
