// The perturb map: the FRESH value of every element of a trained net's flat nn.Linear vector, as networks._Mlp /
// TanhGaussianPolicy / FlattenMlp would have initialised it, drawn from a counter-based stream so that it is a function of
// (seed, draw, net, tensor, element) alone.  Built on param_tensor_list (sac_param_map.h) and, like that header, free of
// HIP: the host job builder of sac_shrink_perturb_many (sac_perturb.h), k_param_perturb itself and
// tests/test_shrink_perturb_host.py read the same few lines.
//
// Element e of tensor j (its place in the net's flat tensor list) of net k:
//
//   hidden weight fc<l>.weight   bound * s,   bound = float32(1 / sqrt((double)N_l))   (the out-size rule of networks._Mlp)
//   hidden bias   fc<l>.bias     the constant b_init: no draw
//   head weight and head bias    init_w * s   (last_fc and, on a SAC policy, last_fc_log_std)
//
// s = 2u - 1 (exact in float32), u = (float(word >> 8) + 0.5f) * 2^-24 in (0, 1] -- philox_normal's uniform -- and word is
// output word e & 3 of Philox4x32-10 with counter (e >> 2, j | k << 8, draw lo, draw hi) and key (seed lo, seed hi): ONE
// evaluation serves the four elements e & ~3 .. e | 3.  The product with the bound is rounded once.
// infer.fresh_params restates this in NumPy.
#pragma once
#include <math.h>

#include "sac_param_map.h"

namespace sac {

struct PhiloxWords { unsigned w[4]; };

// Philox4x32-10 (Salmon et al. 2011): the rounds of philox_normal, all four output words
static inline SAC_HD PhiloxWords philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
    for (int i = 0; i < 10; ++i) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return PhiloxWords{{c0, c1, c2, c3}};
}

// the four words that serve elements 4 q .. 4 q + 3 of tensor j of net k
static inline SAC_HD PhiloxWords perturb_words(unsigned long long seed, unsigned long long draw, int net, int j, long long q) {
    return philox4x32_10((unsigned)q, (unsigned)j | (unsigned)net << 8, (unsigned)draw, (unsigned)(draw >> 32),
                         (unsigned)seed, (unsigned)(seed >> 32));
}

// the sign-scaled uniform s = 2u - 1 in (-1, 1]: both steps are exact (u is a multiple of 2^-25 below 1/2 and of 2^-24 above)
static inline SAC_HD float perturb_sign_uniform(unsigned word) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float u = ((float)(word >> 8) + 0.5f) * (1.0f / 16777216.0f);
    return (u + u) - 1.0f;
}

// a tensor's fresh-value rule: f = draws ? scale * s : scale
struct PerturbRule { float scale; int draws; };

static inline SAC_HD float perturb_fresh(const PerturbRule &r, unsigned word) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return r.draws ? r.scale * perturb_sign_uniform(word) : r.scale;
}

// the rule of tensor j of net `net` (host: the job builder fills the table with it)
static inline PerturbRule perturb_rule(const ParamShape &S, int net, int j, float init_w, float b_init) {
    const int q = param_kind(net), nh = S.nh[q];
    if (j >= 2 * nh) return PerturbRule{init_w, 1};                            // a head's weight or bias
    if (j & 1) return PerturbRule{b_init, 0};                                  // a hidden bias
    return PerturbRule{(float)(1.0 / sqrt((double)S.hidden[q][j >> 1])), 1};  // a hidden weight
}

// the fresh flat vector of a net (host: the header's own walk, for the tests)
static inline void perturb_fresh_flat(const ParamShape &S, int net, unsigned long long seed, unsigned long long draw,
                                      float init_w, float b_init, float *flat) {
    ParamTensor T[PARAM_MAX_TENSORS];
    const int nt = param_tensor_list(S, net, T);
    for (int j = 0; j < nt; flat += T[j++].E) {
        const PerturbRule r = perturb_rule(S, net, j, init_w, b_init);
        for (long long e = 0; e < T[j].E; ++e)
            flat[e] = perturb_fresh(r, r.draws ? perturb_words(seed, draw, net, j, e >> 2).w[e & 3] : 0u);
    }
}

}  // namespace sac
