// Stand-alone host check of the address rule of the per-tensor parameter statistics (csrc/sac_params.h): param_addr /
// param_tensor_list against for_each_param (the fused kernels' shapes) and gen_shape_net's perm (the general step) --
// the same address sequence as the getters', every flat index exactly once, every access inside buffers of exactly
// nP / nPT / GenNet::n floats.  No GPU is touched: the library's source is compiled into this program and only its
// host layout code runs.  Build with the sanitizers on the host side and run (from the repository root):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-unused-value -Wno-pass-failed -UNDEBUG \
//         -Xarch_host -fsanitize=address,undefined scripts/param_addr_check.hip \
//         robosuite_benchmark_amd/csrc/replay_buffer.hip robosuite_benchmark_amd/csrc/peaks.hip -o /tmp/param_addr_check
//   ASAN_OPTIONS=detect_leaks=0 /tmp/param_addr_check
#include "../robosuite_benchmark_amd/csrc/sac_trainer.hip"
#include <cassert>

static long long g_checked = 0;

static void check_fused(int algo, int O, int A, int hp0, int hp1, int hq0, int hq1) {
    sac_trainer *t = new sac_trainer();
    t->algo = algo; t->O = O; t->A = A; t->KP = round_up(O, 16); t->KQ = t->KP + 16;
    t->HP[0] = hp0; t->HP[1] = hp1; t->HQ[0] = hq0; t->HQ[1] = hq1;
    const bool td3 = algo == 1;
    const int shp[3][2] = {{H, t->O}, {H, H}, {(td3 ? 1 : 2) * t->A, H}};
    const int shq[3][2] = {{H, t->KQ}, {H, H}, {1, H}};
    const int nnets = td3 ? 6 : 5;
    for (int i = 0; i < nnets; ++i) {
        Net &n = t->net[i];
        build_layers(n, (i == 0 || i == 5) ? shp : shq, 3);
        float *P = new float[n.nP](), *PT = new float[n.nPT]();
        std::vector<long long> ref, refT;
        for_each_param(t, i, [&](int64_t fi, int l, int nn, int k, bool is_b) {
            const Layer &L = n.L[l];
            assert((size_t)fi == ref.size());
            ref.push_back(is_b ? L.offB + nn : L.offW + (long long)frag_off(nn, k, L.Kp));
            refT.push_back(is_b ? -1 : L.offWt + (long long)frag_off(k, nn, L.Np));
        });
        ParamTensor T[PARAM_MAX_TENSORS];
        const int nt = param_tensor_list(t, i, T);
        size_t fi = 0;
        for (int j = 0; j < nt; ++j)
            for (long long e = 0; e < T[j].E; ++e, ++fi) {
                const long long a = param_addr(T[j].a, e, false);
                assert(fi < ref.size() && a == ref[fi]);
                assert(P[a] == 0.f);           // (ASan: inside the buffer; the mark: visited once)
                P[a] = 1.f;
                if (T[j].a.kind == PA_FRAG) {
                    const long long b = param_addr(T[j].a, e, true);
                    assert(b == refT[fi] && PT[b] == 0.f);
                    PT[b] = 1.f;
                } else assert(refT[fi] == -1);
                g_checked += 1;
            }
        assert(fi == ref.size() && (int64_t)fi == flat_count(flat_map(t, i)));
        delete[] P; delete[] PT;
    }
    delete t;
}

static void check_general(int algo, int O, int A, std::vector<int> hp, std::vector<int> hq) {
    sac_trainer *t = new sac_trainer();
    t->algo = algo; t->O = O; t->A = A;
    t->gen = new sac_general();
    const bool td3 = algo == 1;
    if (td3) {
        gen_shape_net(t->gen->net[0], hp.data(), (int)hp.size(), O, A, false, A);
        gen_shape_net(t->gen->net[5], hp.data(), (int)hp.size(), O, A, false, A);
    } else gen_shape_net(t->gen->net[0], hp.data(), (int)hp.size(), O, 2 * A, true, A);
    for (int i = 1; i < 5; ++i) gen_shape_net(t->gen->net[i], hq.data(), (int)hq.size(), O + A, 1, false, A);
    for (int i = 0; i < (td3 ? 6 : 5); ++i) {
        const GenNet &N = t->gen->net[i];
        float *P = new float[N.n]();
        ParamTensor T[PARAM_MAX_TENSORS];
        const int nt = param_tensor_list(t, i, T);
        assert(nt <= PARAM_MAX_TENSORS);
        size_t fi = 0;
        for (int j = 0; j < nt; ++j)
            for (long long e = 0; e < T[j].E; ++e, ++fi) {
                const long long a = param_addr(T[j].a, e, false);
                assert(fi < N.perm.size() && a == N.perm[fi] && a == param_addr(T[j].a, e, true));
                assert(P[a] == 0.f);
                P[a] = 1.f;
                g_checked += 1;
            }
        assert((long long)fi == N.nflat);
        delete[] P;
    }
    delete t->gen;
    delete t;
}

int main() {
    check_fused(0, 1, 1, 16, 16, 16, 16);
    check_fused(0, 42, 7, 256, 256, 256, 256);
    check_fused(0, 379, 6, 256, 256, 256, 256);
    check_fused(0, 46, 16, 240, 256, 240, 256);
    check_fused(0, 42, 7, 64, 32, 256, 256);
    check_fused(1, 42, 7, 240, 256, 240, 256);
    check_fused(1, 496, 16, 1, 256, 256, 1);
    check_general(0, 1, 1, {1}, {1});
    check_general(0, 1, 1, {16}, {16});
    check_general(0, 42, 7, {300, 7, 129}, {300, 7, 129});
    check_general(0, 42, 7, {64, 64, 64, 64, 64, 64, 64}, {64, 64, 64, 64, 64, 64, 64});
    check_general(0, 42, 7, {4096}, {4096});
    check_general(0, 42, 7, {128, 128}, {128, 128});
    check_general(0, 42, 7, {129, 127}, {129, 127});
    check_general(0, 45, 7, {512, 512}, {512, 512});
    check_general(1, 17, 5, {300, 200, 100}, {300, 200, 100});
    printf("param_addr_check: %lld elements, every flat index once, inside the buffers\n", g_checked);
    return 0;
}
