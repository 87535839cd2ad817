"""Host side of the TD3 objectives' device statistics and replay evaluation (no GPU): infer.td3_eval_moments /
merge_moments / td3_moments_statistics against infer.td3_eval_statistics under the bound of tests/td3_eval_stats_bound.py,
the exact cases (a constant column, a NaN element), the declarations of the four new entries, the draw order of
TD3Trainer._td3_replay_request, the option checks of the drivers in front of any build, and the handle-less path of
evaluate_td3 / evaluate_td3_replay under both values of `stats`."""
import ctypes as C
import importlib.util
import inspect
import os

import numpy as np
import pytest

from robosuite_benchmark_amd import TD3Trainer, _lib, driver, group, infer
from robosuite_benchmark_amd.infer import merge_moments, td3_eval_moments, td3_eval_statistics, td3_moments_statistics
from tests.td3_eval_reference import COLUMNS, batch_dict, inputs, make_td3_trainer
from tests.td3_eval_stats_bound import check_records, check_statistics
from tests.test_evaluate_host import handle_less
from tests.test_evaluate_replay_host import HostBuffer, no_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 1024


def columns(n, A, seed, scale=1.0, offset=0.0):
    """Random float32 columns: rows (6, n) and a_pi (n, A) in [-1, 1]."""
    rs = np.random.RandomState(seed)
    rows = (offset + scale * rs.standard_normal((6, n))).astype(np.float32)
    return rows, np.tanh(rs.standard_normal((n, A))).astype(np.float32)


def merged(rows, a_pi, cuts=None):
    """td3_eval_moments of row windows (1024 rows each, or up to each of `cuts`), merged in order: what a call above 1024
    rows does."""
    n = rows.shape[1]
    edges = list(range(0, n, CHUNK)) + [n] if cuts is None else [0] + list(cuts)
    out = None
    for lo, hi in zip(edges[:-1], edges[1:]):
        part = td3_eval_moments(rows[:, lo:hi], a_pi[lo:hi])
        out = part if out is None else {k: merge_moments(out[k], part[k]) for k in out}
    return out


# ---- the statistics against the host form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,A", [(1, 1), (2, 3), (255, 7), (256, 1), (257, 16), (1024, 16)])
@pytest.mark.parametrize("scale,offset", [(1.0, 0.0), (1e-3, 5.0), (1e3, -1e4)])
def test_moments_statistics_agree_with_td3_eval_statistics(n, A, scale, offset):
    rows, a_pi = columns(n, A, n + A, scale, offset)
    want = td3_eval_statistics(rows, a_pi)
    M = td3_eval_moments(rows, a_pi)
    assert list(M.keys()) == _lib.TD3_EVAL_MOMENTS and all(list(m.keys()) == _lib.EVAL_MOMENT_FIELDS for m in M.values())
    assert M["q1"]["count"] == n and M["a_pi"]["count"] == n * A and M["bellman2"]["count"] == n
    got = td3_moments_statistics(M)
    check_statistics(got, want, rows, a_pi, (n, A, scale))
    for k in want:                                                   # Max and Min are exact
        assert not k.endswith((" Max", " Min")) or got[k] == want[k], k
    assert got["QF1 Loss"] == got["Bellman Errors 1 Mean"] and got["Policy Loss"] == -(M["q_pi"]["sum"] / n)
    if n == 1:
        assert all(got[k] == 0.0 for k in got if k.endswith(" Std") and (A == 1 or k != "Policy Action Std"))


def test_the_bellman_elements_are_the_squared_differences():
    rows, a_pi = columns(300, 2, 9, 3.0, 1.0)
    q1, q2, _, _, _, y = rows.astype(np.float64)
    M = td3_eval_moments(rows, a_pi)
    assert M["bellman1"]["max"] == float(np.max((q1 - y) ** 2)) and M["bellman2"]["min"] == float(np.min((q2 - y) ** 2))
    assert M["bellman1"]["sum"] == float(np.sum((q1 - y) ** 2)) and M["td2"]["sum"] == float(np.sum(q2 - y))
    assert M["td1"]["sumsq"] == float(np.sum((q1 - y) * (q1 - y)))


# ---- the edge cases of the records ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1000, 2500])
def test_a_constant_column_has_no_deviation(n):
    c = np.float32(0.1)
    rows, a_pi = columns(n, 3, 4)
    rows[0] = c
    a_pi[:] = np.float32(-0.75)
    for M in (td3_eval_moments(rows, a_pi), merged(rows, a_pi)):
        got = td3_moments_statistics(M)
        assert got["Q1 Predictions Std"] == 0.0 and got["Q1 Predictions Mean"] == float(c)
        assert got["Q1 Predictions Max"] == got["Q1 Predictions Min"] == float(c)
        assert got["Policy Action Std"] == 0.0 and got["Policy Action Mean"] == -0.75


def test_one_nan_element_reaches_its_own_records_and_no_other():
    rows, a_pi = columns(40, 3, 6)
    rows[2, 17] = np.nan                                             # q_pi: its own record and Policy Loss alone
    M = td3_eval_moments(rows, a_pi)
    for name, m in M.items():
        hit = name == "q_pi"
        assert all(np.isnan(m[f]) == hit for f in ("sum", "max", "min", "m2", "sumsq")), name
        assert m["count"] == (120.0 if name == "a_pi" else 40.0)
    rows, a_pi = columns(40, 3, 6)
    rows[0, 5] = np.nan                                              # q1: q1, td1 and bellman1
    a_pi[39, 2] = np.nan
    want = td3_eval_statistics(rows, a_pi)
    for M in (td3_eval_moments(rows, a_pi), merged(rows, a_pi)):
        assert [k for k, m in M.items() if np.isnan(m["sum"])] == ["q1", "a_pi", "td1", "bellman1"]
        assert all(np.isnan(M[k]["max"]) and np.isnan(M[k]["min"]) for k in ("q1", "a_pi", "td1", "bellman1"))
        got = td3_moments_statistics(M)
        assert np.isnan(got["QF1 Loss"]) and not np.isnan(got["QF2 Loss"]) and not np.isnan(got["Policy Loss"])
        check_statistics(got, want, rows, a_pi)
    rows, a_pi = columns(2500, 2, 6)
    rows[5, 2000] = np.nan                                           # a NaN in the second window survives the merge
    got = td3_moments_statistics(merged(rows, a_pi))
    assert all(np.isnan(got[f"Q Targets {s}"]) for s in ("Mean", "Std", "Max", "Min")) and np.isnan(got["QF2 Loss"])
    assert not np.isnan(got["Q1 Predictions Max"])


@pytest.mark.parametrize("scale,offset", [(1.0, 0.0), (1e-3, 1e4)])
def test_merged_windows_meet_the_unsplit_records(scale, offset):
    n = 2500
    rows, a_pi = columns(n, 5, n, scale, offset)
    whole = td3_eval_moments(rows, a_pi)
    for M in (merged(rows, a_pi), merged(rows, a_pi, cuts=(1024, 2048, 2500))):       # 1024 / 1024 / 452
        assert M["q1"]["count"] == n and M["a_pi"]["count"] == 5 * n
        check_records(M, whole, rows, a_pi, (scale, "records"))
        check_statistics(td3_moments_statistics(M), td3_eval_statistics(rows, a_pi), rows, a_pi, (scale, "host form"))


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_bindings_and_header_declare_the_feature():
    header = open(os.path.join(ROOT, "include", "sac_hip.h")).read()
    assert ("enum { TD3_EVAL_M_Q1, TD3_EVAL_M_Q2, TD3_EVAL_M_Y, TD3_EVAL_M_Q_PI, TD3_EVAL_M_A_PI,\n"
            "       TD3_EVAL_M_TD1, TD3_EVAL_M_TD2, TD3_EVAL_M_BELLMAN1, TD3_EVAL_M_BELLMAN2, TD3_EVAL_MOMENTS_N };") in header
    assert "typedef struct { sac_eval_moment_t m[TD3_EVAL_MOMENTS_N]; } td3_eval_stats_t;" in header
    for name in ("td3_evaluate_stats_many", "td3_evaluate_general_stats_many"):
        assert f"int {name}(" in header and _lib.SYMBOLS[name] == (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 3)
    for name in ("td3_evaluate_replay_many", "td3_evaluate_replay_general_many"):
        assert f"int {name}(" in header and _lib.SYMBOLS[name] == (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4)
    assert _lib.TD3_EVAL_MOMENTS == ["q1", "q2", "y", "q_pi", "a_pi", "td1", "td2", "bellman1", "bellman2"]
    assert C.sizeof(_lib.Td3EvalStats) == 9 * 6 * 8
    assert len(_lib.Td3EvalIO._fields_) == 10                        # (td3_eval_io_t is what it was)
    assert infer.TD3_EVAL_STATS_ENTRIES == {infer.FUSED: "td3_evaluate_stats_many",
                                            infer.GENERAL_STEP: "td3_evaluate_general_stats_many"}
    assert infer.TD3_EVAL_REPLAY_ENTRIES == {infer.FUSED: "td3_evaluate_replay_many",
                                             infer.GENERAL_STEP: "td3_evaluate_replay_general_many"}
    csrc = os.path.join(ROOT, "robosuite_benchmark_amd", "csrc")
    kernel = open(os.path.join(csrc, "td3_eval_moments.h")).read()
    assert "k_eval_moments_td3" in kernel and "atomic" not in kernel.replace("No atomics", "") and "asm" not in kernel
    # the reduction is sac_eval_moments.h's, used and not copied
    assert "em_reduce<EM_SQDIFF>" in kernel and "void em_reduce" not in kernel and "void em_tree" not in kernel
    assert '#include "td3_eval_moments.h"' in open(os.path.join(csrc, "sac_trainer.hip")).read()
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "k_eval_moments_td3" in text and "td3_replay_eval" in text, doc


def test_defaults():
    for fn in (TD3Trainer.evaluate_td3, TD3Trainer.evaluate_td3_replay, infer.td3_evaluate_many, infer.td3_evaluate_replay_many,
               infer.td3_evaluate_of, group.td3_evaluate_many, group.td3_evaluate_replay_many,
               group.ArchTD3TrainerGroup.td3_evaluate_many, group.ArchTD3TrainerGroup.td3_evaluate_replay_many):
        p = inspect.signature(fn).parameters
        assert p["general"].default == "host" and p["stats"].default == "host", fn.__qualname__
    for fn in (TD3Trainer.evaluate_td3_replay, infer.td3_evaluate_replay_many):
        p = inspect.signature(fn).parameters
        assert p["n"].default is None and p["indices"].default is None and p["rows"].default is False
    for fn in (driver.experiment, driver.experiment_group, driver.experiment_sweep):
        assert inspect.signature(fn).parameters["td3_replay_eval"].default == 0, fn.__name__
    assert driver.EvalOptions._field_defaults["td3_replay_eval"] == 0
    doc = " ".join(inspect.getdoc(driver.EvalOptions).split())
    assert "Without validation, replay_eval, td3_validation and td3_replay_eval it has no effect" in doc
    assert "Without validation and replay_eval it has no effect" not in doc


# ---- the request and the drivers' checks ----------------------------------------------------------------------------------
def test_the_request_draws_the_indices_and_then_one_eps(monkeypatch):
    O, A, size, n = 5, 2, 37, 11
    t = make_td3_trainer(O, A, (8, 8))
    buf = HostBuffer(size, O, A)
    np.random.seed(123)
    before = np.random.get_state()
    rs = np.random.RandomState(9)
    idx, eps = t._td3_replay_request(buf, n, None, None, rs)
    mine = np.random.RandomState(9)
    want_idx = mine.randint(0, size, n)
    want_eps = mine.standard_normal((n, A))
    assert idx.dtype == np.int64 and np.array_equal(idx, want_idx)
    assert eps.dtype == np.float32 and np.array_equal(eps, want_eps.astype(np.float32))
    assert rs.randint(0, 1 << 30) == mine.randint(0, 1 << 30)         # nothing else was drawn
    # given indices: the single draw alone; given eps: nothing is drawn
    rs = np.random.RandomState(4)
    idx, eps = t._td3_replay_request(buf, None, [3, 3, 36, 0], None, rs)
    assert idx.tolist() == [3, 3, 36, 0] and np.array_equal(eps, np.random.RandomState(4).standard_normal((4, A)).astype(np.float32))
    rs = np.random.RandomState(4)
    t._td3_replay_request(buf, None, [1], np.zeros((1, A)), rs)
    assert rs.randint(0, 1 << 30) == np.random.RandomState(4).randint(0, 1 << 30)
    # rng None: evaluate_td3's private stream, indices first
    idx, eps = t._td3_replay_request(buf, n, None, None, None)
    mine = np.random.RandomState([int(t.noise_seed & 0xFFFFFFFF), int(t.noise_seed >> 32), 0x4556414C])
    assert np.array_equal(idx, mine.randint(0, size, n)) and np.array_equal(eps, mine.standard_normal((n, A)).astype(np.float32))
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    # the argument checks, all in front of any gather
    for kw in (dict(n=None, indices=None), dict(n=3, indices=[0, 1, 2])):
        with pytest.raises(ValueError, match="exactly one of n and indices"):
            t._td3_replay_request(buf, kw["n"], kw["indices"], None, None)
        with pytest.raises(ValueError, match="exactly one of n and indices"):
            infer.td3_evaluate_replay_many([t], [buf], n=kw["n"], indices=None if kw["indices"] is None else [kw["indices"]])
    for bad in ([37], [-1], [0, 5, 37]):
        with pytest.raises(RuntimeError, match="out of range"):
            t.evaluate_td3_replay(buf, indices=bad)
    with pytest.raises(ValueError, match="eps"):
        t.evaluate_td3_replay(buf, indices=[1, 2, 3], eps=np.zeros((2, A)))
    with pytest.raises(ValueError, match="at least one row"):
        t.evaluate_td3_replay(buf, n=0)
    with pytest.raises(RuntimeError, match="empty"):
        t.evaluate_td3_replay(HostBuffer(0, O, A), n=4)
    with pytest.raises(RuntimeError, match="stats must be"):
        t.evaluate_td3_replay(buf, n=4, stats="gpu", general="gpu")
    with pytest.raises(RuntimeError, match="stats must be"):
        t.evaluate_td3(batch_dict(inputs(4, O, A, 1)[0]), stats="gpu", general="gpu")
    with pytest.raises(RuntimeError, match="general must be"):
        t.evaluate_td3_replay(buf, n=4, general="gpu")
    with pytest.raises(RuntimeError, match="twice"):
        infer.td3_evaluate_replay_many([t, t], [buf, buf], n=4)
    assert buf.gathered == []


def test_a_sac_member_is_refused_and_the_message_names_evaluate_replay_many():
    sac_t = handle_less(5, 2, (8, 8))
    buf = HostBuffer(10, 5, 2)
    with pytest.raises(RuntimeError, match=r"td3_evaluate_replay_many member 0 is a SAC trainer.*evaluate_replay_many evaluates"):
        infer.td3_evaluate_replay_many([sac_t], [buf], n=4)
    with pytest.raises(RuntimeError, match=r"td3_evaluate_many member 1 is a SAC trainer.*; evaluate_many evaluates"):
        infer.td3_evaluate_many([make_td3_trainer(5, 2, (8, 8)), sac_t], [None, None], stats="device")
    assert buf.gathered == []
    # TD3Trainer.evaluate and evaluate_replay keep raising exactly as they do
    t = make_td3_trainer(5, 2, (8, 8))
    with pytest.raises(NotImplementedError, match=r"TD3Trainer\.evaluate: evaluate computes the SAC objective .* is not implemented"):
        t.evaluate(batch_dict(inputs(4, 5, 2, 1)[0]), stats="device")
    with pytest.raises(NotImplementedError, match=r"TD3Trainer\.evaluate_replay: evaluate computes the SAC objective"):
        t.evaluate_replay(buf, n=4)


def test_the_option_checks_come_before_any_build():
    from robosuite_benchmark_amd.variant import default_variant
    td3 = default_variant(env="Lift", seed=1, batch_size=64, agent="TD3")
    sac_v = default_variant(env="Lift", seed=1, batch_size=64, agent="SAC")
    calls = ((driver.experiment, (sac_v,), dict(obs_dim=5, action_dim=2)),
             (driver.experiment_group, (sac_v, [1, 2]), dict(obs_dim=5, action_dim=2)),
             (driver.experiment_sweep, ([(td3, 1, 5, 2), (sac_v, 2, 5, 2)],), {}))
    for fn, args, kw in calls:                                       # a SAC variant: refused, naming replay_eval
        with pytest.raises(RuntimeError, match=r"td3_replay_eval=N.*TD3 objective.*replay_eval=N"):
            fn(*args, td3_replay_eval=64, **kw)
    for bad in (-1, 1.5, "many", True):
        for fn, args in ((driver.experiment, (None,)), (driver.experiment_group, (None, None)), (driver.experiment_sweep, (None,))):
            with pytest.raises(RuntimeError, match="td3_replay_eval is a row count"):
                fn(*args, td3_replay_eval=bad)
    # replay_eval keeps refusing TD3 with its present text
    for fn, args, kw in ((driver.experiment, (td3,), dict(obs_dim=5, action_dim=2)),
                         (driver.experiment_group, (td3, [1, 2]), dict(obs_dim=5, action_dim=2)),
                         (driver.experiment_sweep, ([(td3, 1, 5, 2)],), {})):
        with pytest.raises(RuntimeError, match=r"replay_eval=N\): the replay evaluation computes the SAC objective "
                                               r"\(SACTrainer\.evaluate_replay\); a TD3 variant has no such evaluation"):
            fn(*args, replay_eval=64, **kw)
    with pytest.raises(RuntimeError, match="replay_eval is a row count"):
        driver.experiment(None, replay_eval=True)
    opts = driver._options("experiment", [(td3,)], "host", False, "host", False, "host", "device", 0, td3_replay_eval=32,
                           td3_validation=True)
    assert opts.td3_replay_eval == 32 and opts.replay_eval == 0 and opts.eval_stats == "device" and opts.td3_validation is True


def test_the_driver_passes_stats_and_leaves_it_out_at_the_default(monkeypatch):
    import types
    O, A, n = 5, 2, 3
    seen = []

    class Buf:
        def num_steps_can_sample(self):
            return 20

    class T:
        obs_dim, act_dim = O, A

        def evaluate_td3(self, batch, eps=None, **kw):
            seen.append(("solo", kw))

        def evaluate_td3_replay(self, buffer, n=None, rng=None, **kw):
            seen.append(("solo replay", n, rng.randint(0, 1 << 30), kw))

    def many(trainers, batches, eps=None, **kw):
        seen.append(("many", kw))
        return [None] * len(trainers)

    def replay_many(trainers, bufs, n=None, rngs=None, **kw):
        seen.append(("many replay", n, [g.randint(0, 1 << 30) for g in rngs], kw))
        return [None] * len(trainers)

    path = dict(observations=np.zeros((n, O)), actions=np.zeros((n, A)), rewards=np.zeros((n, 1)), terminals=np.zeros((n, 1)),
                next_observations=np.zeros((n, O)))
    runs = [dict(trainer=T(), evalc=types.SimpleNamespace(epoch_paths=[path]), seed=7, buf=Buf())]
    monkeypatch.setattr(driver, "td3_evaluate_many", many)
    monkeypatch.setattr(driver, "td3_evaluate_replay_many", replay_many)
    opts = driver.EvalOptions(td3_validation=True, td3_replay_eval=32)
    draw = np.random.RandomState([7, 4, 0x52504C]).randint(0, 1 << 30)
    blocks, _ = driver._epoch_evaluations(runs, 4, opts)
    assert seen == [("many", {}), ("many replay", [20], [draw], {})]
    assert list(blocks[0]) == ["validation", "replay"] and blocks[0]["replay"]["replay/Num Transitions"] == 20
    keys = list(td3_eval_statistics(np.zeros((6, 1)), np.zeros((1, 1))))
    assert list(blocks[0]["replay"]) == ["replay/" + k for k in keys] + ["replay/Num Transitions"]
    del seen[:]
    dev = opts._replace(eval_stats="device", eval_general="device")
    driver._epoch_evaluations(runs, 4, dev)
    driver._epoch_evaluations(runs, 4, dev, many=False)
    driver._epoch_evaluations(runs, 4, opts, many=False)
    kw = dict(general="device", stats="device")
    assert seen == [("many", kw), ("many replay", [20], [draw], kw), ("solo", kw), ("solo replay", 20, draw, kw),
                    ("solo", {}), ("solo replay", 20, draw, {})]
    # an empty buffer: no call, the columns stay, empty
    del seen[:]
    runs[0]["buf"].num_steps_can_sample = lambda: 0
    blocks, _ = driver._epoch_evaluations(runs, 0, driver.EvalOptions(td3_replay_eval=32))
    assert seen == [] and blocks[0]["replay"]["replay/Num Transitions"] == 0
    assert all(np.isnan(v) for k, v in blocks[0]["replay"].items() if k != "replay/Num Transitions")
    # with the option off the blocks are what they were
    blocks, _ = driver._epoch_evaluations(runs, 0, driver.EvalOptions(td3_validation=True))
    assert list(blocks[0]) == ["validation"]


def test_the_train_script_takes_the_option():
    spec = importlib.util.spec_from_file_location("train_script", os.path.join(ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    assert ap.parse_args([]).td3_replay_eval == 0
    assert ap.parse_args(["--agent", "TD3", "--td3_replay_eval"]).td3_replay_eval == 1024
    assert ap.parse_args(["--td3_replay_eval", "300"]).td3_replay_eval == 300
    assert ap.parse_args(["--td3_replay_eval", "--td3_validation"]).td3_replay_eval == 1024


# ---- the host-path trainer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [(8, 8), (24, 12, 20)])
def test_without_a_handle_the_host_path_answers_under_both_values(monkeypatch, hidden):
    O, A, size = 9, 3, 50
    t = make_td3_trainer(O, A, hidden, reward_scale=1.5, discount=0.97)
    u = make_td3_trainer(O, A, hidden, seed=8)
    assert t._h is None
    no_library(monkeypatch, t, u)
    buf = HostBuffer(size, O, A)
    idx = np.array([0, size - 1, 7, 7, 31, 2], np.int64)
    eps = np.random.RandomState(5).standard_normal((idx.size, A)).astype(np.float32)
    want_stats, want = t.evaluate_td3(buf.gather(idx), eps=eps, rows=True)
    assert want_stats == td3_eval_statistics(np.stack([want[k] for k in _lib.TD3_EVAL_ROWS]), want["a_pi"])
    for general in infer.GENERAL:
        for stats in infer.STATS:
            kw = dict(general=general, stats=stats)
            s, c = t.evaluate_td3_replay(buf, indices=idx, eps=eps, rows=True, **kw)
            assert s == want_stats and all(np.array_equal(c[k].view(np.uint32), want[k].view(np.uint32)) for k in COLUMNS)
            assert np.array_equal(c["indices"], idx) and list(c.keys()) == list(want.keys()) + ["indices"]
            assert t.evaluate_td3_replay(buf, indices=idx, eps=eps, **kw) == want_stats
            s, c = t.evaluate_td3(buf.gather(idx), eps=eps, rows=True, **kw)
            assert s == want_stats and all(np.array_equal(c[k], want[k]) for k in COLUMNS)
            assert t.evaluate_td3(buf.gather(idx), eps=eps, **kw) == want_stats
    # many: member 1 sits out, two members share one buffer
    grp = group.ArchTD3TrainerGroup.__new__(group.ArchTD3TrainerGroup)
    grp.trainers = [t, u, make_td3_trainer(O, A, hidden, seed=8)]
    w2 = make_td3_trainer(O, A, hidden, seed=8).evaluate_td3(buf.gather(idx[:2]), eps=eps[:2], rows=True)
    for stats in infer.STATS:
        for got in (infer.td3_evaluate_replay_many(grp.trainers, [buf] * 3, indices=[idx, None, idx[:2]],
                                                   eps=[eps, None, eps[:2]], rows=True, stats=stats),
                    grp.td3_evaluate_replay_many([buf] * 3, indices=[idx, [], idx[:2]], eps=[eps, None, eps[:2]], rows=True,
                                                 stats=stats)):
            assert got[1] is None and got[0][0] == want_stats and all(np.array_equal(got[0][1][k], want[k]) for k in COLUMNS)
            assert got[2][0] == w2[0] and all(np.array_equal(got[2][1][k], w2[1][k]) for k in COLUMNS)
        assert grp.td3_evaluate_many([buf.gather(idx), None, None], eps=[eps, None, None], stats=stats)[0] == want_stats
    # n per member, 0 sits out
    got = infer.td3_evaluate_replay_many([t, u], [buf, buf], n=[4, 0], rngs=[np.random.RandomState(1), None], rows=True)
    assert got[1] is None and np.array_equal(got[0][1]["indices"], np.random.RandomState(1).randint(0, size, 4))
