"""The hidden layers of a SAC or TD3 net in NumPy, from sac_get_params blobs: the reference of the unit_moments tests.

hidden_forward(t, flat, net, obs, act, dtype) returns every hidden layer's post-ReLU activations, [(n, N_l)], computed
in `dtype` -- float64 is the reference R, float32 the plain forward P whose own error sets the bound (tests/helpers.py:
max|K - R| / max|R| <= max(8 max|P - R| / max|R|, 1e-5) per layer).  The flat vector is nn.Linear's: W (N, K) then b
(N) per layer, the hidden layers first; whatever output layer or head follows is not read."""
import numpy as np

Q_NETS = ("qf1", "qf2", "target_qf1", "target_qf2")
ALL_NETS = ("policy",) + Q_NETS


def hidden_layers(t, flat, net):
    """[(W, b)] of the hidden layers of `net` out of its flat parameter vector."""
    k = t.obs_dim + (t.act_dim if net in Q_NETS else 0)
    flat = np.asarray(flat, np.float32)
    out, off = [], 0
    for n in t._hidden(net):
        out.append((flat[off:off + n * k].reshape(n, k), flat[off + n * k:off + n * k + n]))
        off, k = off + n * k + n, n
    return out


def hidden_forward(t, flat, net, obs, act, dtype=np.float64):
    x = np.concatenate([obs, act], axis=1) if net in Q_NETS else obs
    h = np.asarray(x, dtype)
    out = []
    with np.errstate(all="ignore"):
        for w, b in hidden_layers(t, flat, net):
            h = h @ w.astype(dtype).T + b.astype(dtype)
            h = np.where(h < 0, dtype(0), h)
            out.append(h)
    return out


def loop_moments(h):
    """The record of one layer by a plain Python loop over rows and units, in the reducer's order: rows w, w + 4, ...
    per partial w, then (p0 + p1) + (p2 + p3)."""
    h = np.asarray(h, np.float32)
    n, N = h.shape
    rec = dict(count=float(n), sum=np.zeros(N), sumsq=np.zeros(N), active=np.zeros(N), max=np.zeros(N))
    for u in range(N):
        p = []
        for w in range(4):
            s, q, a, m = 0.0, 0.0, 0.0, float("-inf")
            for r in range(w, n, 4):
                x = float(h[r, u])
                s, q = s + x, q + x * x
                a += 1.0 if x > 0 else 0.0
                m = x if (x > m or x != x) else m
            p.append((s, q, a, m))
        mx = lambda a, b: b if (b > a or b != b) else a          # noqa: E731
        rec["sum"][u] = (p[0][0] + p[1][0]) + (p[2][0] + p[3][0])
        rec["sumsq"][u] = (p[0][1] + p[1][1]) + (p[2][1] + p[3][1])
        rec["active"][u] = (p[0][2] + p[1][2]) + (p[2][2] + p[3][2])
        rec["max"][u] = mx(mx(p[0][3], p[1][3]), mx(p[2][3], p[3][3]))
    return rec


def same_record(a, b, fields=("sum", "sumsq", "active", "max")):
    """Byte for byte: count equal, every field's float64 words equal (+0 is not -0).  A NaN equals any NaN: which
    payload an addition hands on is the processor's choice, not the reducer's."""
    def words(x, y):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        return bool(np.all((x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))))

    return a["count"] == b["count"] and all(
        a[f].shape == b[f].shape and a[f].dtype == np.float64 and b[f].dtype == np.float64 and words(a[f], b[f])
        for f in fields)
