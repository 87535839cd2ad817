"""CPU: what tests/nonfinite_states.py claims of its states, on the oracles alone -- the fp32 and the float64 oracle put
every NaN and every infinity on the same elements, the state that stays bit-equal to the clean run is the state the
poison cannot reach, the ambiguous elements stay under their cap, and the clean twin is finite throughout.  Also, on
np.random.RandomState itself: the buffer seeds of the pad-row tests draw no index 0."""
import numpy as np
import pytest

from tests import nonfinite_states as NS

SHAPES = [((42, 7, 255), (256, 256)), ((42, 7, 129), (64, 96, 48))]
CASES = [(algo, shape, hidden, p) for algo in ("sac", "td3") for shape, hidden in SHAPES for p in NS.POISONS[algo]]


def _id(c):
    algo, (O, A, B), hidden, p = c
    return f"{algo}-B{B}-h{'x'.join(map(str, hidden))}-{p}"


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_the_oracles_agree_on_every_class(case):
    algo, shape, hidden, poison = case
    st = NS.build(poison, algo, *shape, hidden=hidden)
    m = st.meta
    assert set(m["classes"]) == set(m["classes64"])
    for name, c32 in m["classes"].items():
        c64 = m["classes64"][name]
        assert np.array_equal(c32, c64), (name, int(np.sum(c32 != c64)), "elements of", c32.size)
    assert any(np.any(c != NS.FINITE) for c in m["classes"].values()), "the poison reached nothing"
    # the poison is a literal NaN or infinity in ONE place per poisoned row; everything else of the state is finite
    assert m["bit_equal"] == set(NS.EXPECTED_BIT_EQUAL[algo][poison]), sorted(m["bit_equal"] ^ set(NS.EXPECTED_BIT_EQUAL[algo][poison]))
    for name in m["ambiguous"]:
        assert NS.ambiguous_share(st, name) <= NS.AMBIGUOUS_CAP, (name, NS.ambiguous_share(st, name))
    for name, v in m["clean_values32"].items():
        assert np.all(np.isfinite(v)), ("clean twin, fp32 oracle", name)
    for name, v in m["clean_values64"].items():
        assert np.all(np.isfinite(v)), ("clean twin, float64 oracle", name)


SAC_FINITE = {   # the issue's table: statistics that stay FINITE (and bit-equal to the clean run's)
    "next_obs nan": ("Policy Loss", "Actor Loss", "Q1 Predictions", "Q2 Predictions", "Log Pis", "Policy mu", "Policy log std",
                     "Alpha", "Alpha Loss"),
    "reward nan": ("Policy Loss", "Actor Loss", "Q1 Predictions", "Q2 Predictions", "Log Pis", "Policy mu", "Policy log std",
                   "Alpha", "Alpha Loss"),
    "action nan": ("Q Targets", "Policy Loss", "Log Pis", "Alpha"),
    "qf1 weight nan": ("QF2 Loss", "Q2 Predictions", "Q Targets"),
    "policy weight inf": ("Q1 Predictions", "Q2 Predictions"),
    "eps1 nan": ("Q1 Predictions", "Q2 Predictions", "Policy mu", "Policy log std"),
}


@pytest.mark.parametrize("shape,hidden", SHAPES, ids=["B255", "B129-deep"])
def test_the_statistics_the_poison_cannot_reach(shape, hidden):
    for poison, groups in SAC_FINITE.items():
        m = NS.build(poison, "sac", *shape, hidden=hidden).meta
        for g in groups:
            names = [g] if g in ("Policy Loss", "Actor Loss", "QF2 Loss", "Alpha", "Alpha Loss") else [f"{g} {s}" for s in ("Mean", "Std", "Max", "Min")]
            for n in names:
                assert n in m["same_diags"], (poison, n, m["values32"]["diag " + n], m["clean_values32"]["diag " + n])
    m = NS.build("reward inf", "sac", *shape, hidden=hidden).meta
    got = {s: float(m["values32"]["diag Q Targets " + s][0]) for s in ("Mean", "Std", "Max", "Min")}
    assert got["Mean"] == np.inf and got["Max"] == np.inf and np.isnan(got["Std"]) and np.isfinite(got["Min"]), got
    assert "Q Targets Min" in m["same_diags"]
    for poison in ("obs nan", "obs nan last", "obs inf"):
        m = NS.build(poison, "sac", *shape, hidden=hidden).meta
        assert not m["same_diags"], (poison, m["same_diags"])


def test_gradients_follow_relu_at_the_poisoned_row():
    """next_obs NaN: a critic's gradient is NaN except where it is exactly 0 -- the rows of the units that are off at the
    poisoned row -- and that is a real share of both kinds."""
    m = NS.build("next_obs nan", "sac", 42, 7, 255).meta
    for net in ("qf1", "qf2"):
        c, v = m["classes"]["grad " + net], m["values32"]["grad " + net]
        assert set(np.unique(c)) == {NS.FINITE, NS.NAN}
        assert 0.05 < np.mean(c == NS.FINITE) < 0.95
    assert np.all(m["classes"]["grad policy"] == NS.FINITE)


def test_pad_row_seeds_draw_no_index_zero():
    """tests/test_gpu_step_nonfinite.py poisons buffer row 0 and must never draw it."""
    for seed, sizes in ((NS.PAD_SEED, [B for _, B in NS.PAD_CASES]), (NS.PAD_SEED_MEMBER_1, NS.PAD_GROUP_BATCHES)):
        for B in sizes:
            rs = np.random.RandomState(seed)
            for _ in range(NS.PAD_STEPS):
                idx = rs.randint(0, NS.PAD_BUFFER_ROWS, B)
                assert idx.size == B and not np.any(idx == 0), (seed, B)
    idx = NS.pad_eval_indices()
    assert idx.size == 17 and not np.any(idx == 0), NS.PAD_EVAL_SEED
