// The recycle map: which elements of a trained net's flat nn.Linear vector a recycled hidden unit owns, and where each
// lives on the device.  Built on param_tensor_list / param_addr (sac_param_map.h) and, like that header, free of HIP: the
// host job builder of sac_recycle_units_many (sac_recycle.h), k_unit_recycle itself and tests/test_recycle_map_host.py
// read the same few lines.
//
// Unit u of hidden layer l (0-based) owns, in two PHASES that run as two launches, incoming first:
//
//   RC_INCOMING   row u of fc<l>.weight (K_l elements, flat e = u K_l + i) and element u of fc<l>.bias: they take the
//                 caller's fresh row -- K_l weights, then the bias
//   RC_OUTGOING   column u of every tensor that reads layer l (flat e = i N_l + u over its rows i): fc<l+1>.weight, or for
//                 the last hidden layer last_fc.weight and, on a SAC policy, last_fc_log_std.weight too: they take +0.0
//
// Both are SPANS of one tensor: e(u, i) = u * mul + i * stride, i < count.  An element's forward address is
// param_addr(a, e, false); a PA_FRAG weight (the fused kernels' shapes) has a second copy at param_addr(a, e, true), and
// that is where its Adam moments live (MT / VT; every other tensor's in M / V at the forward address): ParamJob's mt rule.
// Within a phase no two (unit, span, i) share an address; the phases meet only where (v, u) of fc<l+1>.weight has v
// listed in layer l + 1 and u listed in layer l -- there the later launch, the zero, wins.
#pragma once
#include "sac_param_map.h"

namespace sac {

enum { RC_INCOMING = 0, RC_OUTGOING = 1, RC_PHASES = 2 };
constexpr int RC_MAX_SPANS = 2;

struct RecycleSpan {
    ParamAddr a;                   // the tensor
    long long flat0;               // its first element in the net's flat vector
    long long mul, stride;         // e(u, i) = u * mul + i * stride
    int count;                     // i < count
    int src0;                      // element i takes fresh[src0 + i] of the unit's fresh row; -1: +0.0
};

struct RecycleSpans {
    RecycleSpan s[RC_MAX_SPANS];
    int n;                         // spans in use
    int width, fanin;              // N_l (units of the layer: u < width) and K_l (a fresh row holds fanin + 1 floats)
};

// hidden layers of a net, the true width N_l of one of them and its fan-in K_l
static inline int recycle_layers(const ParamShape &S, int net) { return S.nh[param_kind(net)]; }
static inline int recycle_width(const ParamShape &S, int net, int l) { return S.hidden[param_kind(net)][l]; }
static inline int recycle_fanin(const ParamShape &S, int net, int l) {
    return l ? S.hidden[param_kind(net)][l - 1] : (param_kind(net) ? S.O + S.A : S.O);
}

// the spans of (net, hidden layer l, phase); returns 0, or -1 where the net has no such hidden layer
static inline int recycle_spans(const ParamShape &S, int net, int l, int phase, RecycleSpans *out) {
    ParamTensor T[PARAM_MAX_TENSORS];
    const int nt = param_tensor_list(S, net, T), nh = recycle_layers(S, net);
    if (l < 0 || l >= nh) return -1;
    long long flat0[PARAM_MAX_TENSORS], f = 0;
    for (int j = 0; j < nt; f += T[j++].E) flat0[j] = f;
    RecycleSpans R{};
    R.width = recycle_width(S, net, l);
    R.fanin = recycle_fanin(S, net, l);
    if (phase == RC_INCOMING) {
        const int w = 2 * l, b = 2 * l + 1;
        R.s[0] = RecycleSpan{T[w].a, flat0[w], R.fanin, 1, R.fanin, 0};
        R.s[1] = RecycleSpan{T[b].a, flat0[b], 1, 1, 1, R.fanin};
        R.n = 2;
    } else {
        for (int w = 2 * (l + 1); w < nt && R.n < RC_MAX_SPANS; w += 2) {      // (past the last hidden layer: every head)
            R.s[R.n++] = RecycleSpan{T[w].a, flat0[w], 1, R.width, (int)(T[w].E / R.width), -1};
            if (l + 1 < nh) break;
        }
    }
    *out = R;
    return 0;
}

// one written element: its place in the flat vector, in the forward image, in the transposed image (-1: it has no second
// copy) and in the moment images (mt: those are the transposed ones, MT / VT)
struct RecycleElem { long long flat, fwd, tr, mom; int mt, span, i; };

static inline SAC_HD RecycleElem recycle_elem(const RecycleSpan &s, int u, int i) {
    const long long e = (long long)u * s.mul + (long long)i * s.stride;
    RecycleElem x;
    x.flat = s.flat0 + e;
    x.fwd = param_addr(s.a, e, false);
    x.mt = s.a.kind == PA_FRAG ? 1 : 0;
    x.tr = x.mt ? param_addr(s.a, e, true) : -1;
    x.mom = x.mt ? x.tr : x.fwd;
    x.span = 0; x.i = i;
    return x;
}

// f(element) for everything unit u owns in these spans
template <typename F>
static inline void recycle_walk(const RecycleSpans &R, int u, F &&f) {
    for (int k = 0; k < R.n; ++k)
        for (int i = 0; i < R.s[k].count; ++i) {
            RecycleElem x = recycle_elem(R.s[k], u, i);
            x.span = k;
            f(x);
        }
}

}  // namespace sac
