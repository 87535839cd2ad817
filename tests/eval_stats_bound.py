"""The bound between the statistics of an evaluation reduced in two orders (shared by tests/test_evaluate_stats_host.py
and tests/test_gpu_evaluate_stats.py).

A float64 sum of N terms in any order is within (N - 1) 2^-53 sum|x| of the exact sum, NumPy's pairwise sum too; the
division, the square root and the m2 pass about a slightly different mean add terms of the same order.  So for a Mean, a
Std or a loss over N elements whose averaged terms are x:

    |a - b| <= 8 N 2^-53 max|x|

x: the element for Mean and Std (and for Policy Loss, the mean of log_pi - min(q1_new, q2_new)), (q - y)^2 for a QF
loss, |log_alpha (log_pi + target_entropy)| for Alpha Loss; N = n, or n A for mu and log_std.  The factor 8 covers the
handful of extra roundings in the divide, the sqrt and the chunk merge.  Max, Min and Alpha are exact."""
import numpy as np

EXACT = ("Max", "Min")
QUANTITIES = (("Q1 Predictions", "q1"), ("Q2 Predictions", "q2"), ("Q Targets", "y"), ("Log Pis", "log_pi"),
              ("Policy mu", "mu"), ("Policy log std", "log_std"), ("TD Error 1", "td1"), ("TD Error 2", "td2"))


def elements(rows, mu, log_std):
    """name -> the float64 elements behind each statistic (the names of _lib.EVAL_MOMENTS)."""
    q1, q2, q1n, q2n, _, _, lp, _, y = [np.asarray(x, np.float64).ravel() for x in rows]
    flat = lambda x: np.asarray(x, np.float64).ravel()               # noqa: E731
    return dict(q1=q1, q2=q2, y=y, log_pi=lp, mu=flat(mu), log_std=flat(log_std), td1=q1 - y, td2=q2 - y,
                policy=lp - np.minimum(q1n, q2n))


def bounds(rows, mu, log_std, log_alpha, target_entropy):
    """key of eval_statistics -> the largest |a - b| allowed (0.0: equal)."""
    el = elements(rows, mu, log_std)
    top = lambda x: float(np.max(np.abs(x)))                         # noqa: E731
    rule = lambda x, terms: 8.0 * x.size * 2.0 ** -53 * top(terms)   # noqa: E731
    with np.errstate(all="ignore"):
        out = {"QF1 Loss": rule(el["td1"], el["td1"] ** 2), "QF2 Loss": rule(el["td2"], el["td2"] ** 2),
               "Policy Loss": rule(el["policy"], el["policy"]), "Alpha": 0.0,
               "Alpha Loss": rule(el["log_pi"], float(log_alpha) * (el["log_pi"] + float(target_entropy)))}
        for name, key in QUANTITIES:
            out[name + " Mean"] = out[name + " Std"] = rule(el[key], el[key])
            out[name + " Max"] = out[name + " Min"] = 0.0
    return out


def check_statistics(got, want, rows, mu, log_std, log_alpha, target_entropy, where=""):
    """got (the moments' statistics) against want (eval_statistics of the same columns): the same keys in the same order,
    each value within bounds(); a NaN on one side is a NaN on the other.  Returns the largest |got - want| / bound."""
    assert list(got.keys()) == list(want.keys()), where
    B = bounds(rows, mu, log_std, log_alpha, target_entropy)
    worst = 0.0
    for k, w in want.items():
        g = got[k]
        assert isinstance(g, float), (where, k, type(g))
        if np.isnan(w) or np.isnan(g):
            assert np.isnan(w) and np.isnan(g), (where, k, g, w)
            continue
        if B[k] == 0.0 or np.isinf(w):
            assert g == w, (where, k, g, w)
            continue
        assert abs(g - w) <= B[k], (where, k, g, w, abs(g - w), B[k])
        worst = max(worst, abs(g - w) / B[k])
    return worst
