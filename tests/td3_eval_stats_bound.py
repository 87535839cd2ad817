"""The bound between the statistics of a TD3 evaluation reduced in two orders (shared by
tests/test_td3_evaluate_stats_host.py, tests/test_gpu_td3_evaluate_stats.py and tests/test_gpu_td3_evaluate_replay.py).

The rule is the project's (tests/eval_stats_bound.py, where it is derived): for a Mean, a Std or a loss over N elements
whose averaged terms are x,

    |a - b| <= 8 N 2^-53 max|x|

x: the element for Mean and Std (and for Policy Loss, the mean of -q_pi); for the Bellman records and the QF losses the
element is (q - y)^2.  N = n, or n A for a_pi.  Max and Min are exact."""
import numpy as np

QUANTITIES = (("Q1 Predictions", "q1"), ("Q2 Predictions", "q2"), ("Q Targets", "y"), ("Bellman Errors 1", "bellman1"),
              ("Bellman Errors 2", "bellman2"), ("Policy Action", "a_pi"), ("TD Error 1", "td1"), ("TD Error 2", "td2"))
RULE = 8.0 * 2.0 ** -53


def elements(rows, a_pi):
    """name -> the float64 elements behind each record (the names of _lib.TD3_EVAL_MOMENTS)."""
    q1, q2, q_pi, _, _, y = [np.asarray(x, np.float64).ravel() for x in rows]
    with np.errstate(all="ignore"):
        return dict(q1=q1, q2=q2, y=y, q_pi=q_pi, a_pi=np.asarray(a_pi, np.float64).ravel(), td1=q1 - y, td2=q2 - y,
                    bellman1=(q1 - y) ** 2, bellman2=(q2 - y) ** 2)


def bounds(rows, a_pi):
    """key of td3_eval_statistics -> the largest |a - b| allowed (0.0: equal)."""
    el = elements(rows, a_pi)
    rule = lambda x: RULE * x.size * float(np.max(np.abs(x)))        # noqa: E731
    with np.errstate(all="ignore"):
        out = {"QF1 Loss": rule(el["bellman1"]), "QF2 Loss": rule(el["bellman2"]), "Policy Loss": rule(el["q_pi"])}
        for name, key in QUANTITIES:
            out[name + " Mean"] = out[name + " Std"] = rule(el[key])
            out[name + " Max"] = out[name + " Min"] = 0.0
    return out


def check_statistics(got, want, rows, a_pi, where=""):
    """got (the moments' statistics) against want (td3_eval_statistics of the same columns): the same keys in the same
    order, each value within bounds(); a NaN on one side is a NaN on the other.  Returns the largest |got - want| / bound."""
    assert list(got.keys()) == list(want.keys()), where
    B = bounds(rows, a_pi)
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


def check_records(got, want, rows, a_pi, where=""):
    """Moment records (td3_eval_moments' layout) against the reference's records of the same columns: the same names in
    the same order, count, max and min equal (a NaN on both sides), and the statistics the two sets of records give
    (td3_moments_statistics: Mean = sum / count, Std = sqrt(m2 / count), the losses) within the rule.  Returns the
    largest ratio to a bound."""
    from robosuite_benchmark_amd.infer import td3_moments_statistics
    el = elements(rows, a_pi)
    assert list(got.keys()) == list(want.keys()), where
    for k, w in want.items():
        g = got[k]
        assert g["count"] == w["count"] == float(el[k].size), (where, k)
        for f in ("max", "min"):
            assert g[f] == w[f] or (np.isnan(g[f]) and np.isnan(w[f])), (where, k, f, g[f], w[f])
        assert np.isnan(g["sum"]) == np.isnan(w["sum"]) and np.isnan(g["m2"]) == np.isnan(w["m2"]), (where, k)
    return check_statistics(td3_moments_statistics(got), td3_moments_statistics(want), rows, a_pi, where)
