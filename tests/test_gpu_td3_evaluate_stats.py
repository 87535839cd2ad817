"""GPU: the TD3 objectives' statistics reduced on the device -- td3_evaluate_stats_many / td3_evaluate_general_stats_many
(k_eval_moments_td3, csrc/td3_eval_moments.h), TD3Trainer.evaluate_td3(stats="device"),
group.td3_evaluate_many(stats="device") and the sweep driver's eval_stats="device" under td3_validation / td3_replay_eval.

Only the statistics comparison has a tolerance: the device's records and the statistics built from them against
infer.td3_eval_moments / infer.td3_eval_statistics of the float32 columns the SAME call returned (rows=True), under the
bound of tests/td3_eval_stats_bound.py: |device - host| <= 8 N 2^-53 max|x| for a Mean, a Std or a loss over N elements
whose averaged terms are x.  What is exact is asserted exactly: the columns (bit for bit those of stats="host"), count,
Max and Min, Std at one row and of a constant column, and a member's records against its solo call's (byte for byte)."""
import copy
import ctypes as C

import numpy as np
import pytest

from robosuite_benchmark_amd import ArchTD3TrainerGroup, _lib
from robosuite_benchmark_amd.group import runs_general_step, td3_evaluate_many
from robosuite_benchmark_amd.infer import _stats_moments, td3_eval_moments, td3_eval_statistics
from tests.helpers import filled_buffer, make_pair, make_td3_pair
from tests.td3_eval_reference import ARRAY_COLUMNS, COLUMNS, ROW_COLUMNS, batch_dict, inputs, make_td3_trainer
from tests.td3_eval_stats_bound import check_records, check_statistics

pytestmark = pytest.mark.gpu
# (O, A, policy hidden, critic hidden or None): O = A = 1; Lift; A = 16, so that n A reaches 16384
FUSED = [(1, 1, (16, 16), None), (42, 7, (256, 256), None), (11, 16, (32, 16), None)]
# one hidden unit; two wide layers; a policy deeper than its critics
GENERAL = [(5, 3, (1,), None), (42, 7, (512, 512), None), (9, 4, (24, 16, 8), (32,))]
ROWS = (1, 255, 256, 257, 1024, 2500)       # around the lane stride of 256; one full call; three calls merged
ENTRY = {False: "td3_evaluate_stats_many", True: "td3_evaluate_general_stats_many"}
WORST = {}                  # family -> largest |device - host| / bound seen (printed; README quotes it)


def make(O, A, hidden, hidden_q=None, seed=5, steps=0):
    if hidden_q is None:
        t = make_td3_pair(O, A, 32, seed=seed, hidden=hidden)[1]
    else:
        t = make_td3_trainer(O, A, hidden, hidden_q, seed=seed, batch_size=32, policy_learning_rate=1e-3, qf_learning_rate=5e-4)
    if steps:
        t.train_loop(filled_buffer(600, O, A, 3), steps, batch_size=32)
    return t


def bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same(a, b):
    return all(bits(a[k], b[k]) for k in COLUMNS)


def rows_of(cols):
    return np.stack([cols[k] for k in ROW_COLUMNS])


def check(t, stats, cols, where):
    """stats (the device's) against td3_eval_statistics of `cols`, the columns of the same call."""
    want = td3_eval_statistics(rows_of(cols), cols["a_pi"])
    w = check_statistics(stats, want, rows_of(cols), cols["a_pi"], where)
    for k in want:
        if k.endswith((" Max", " Min")):
            assert stats[k] == want[k] or (np.isnan(stats[k]) and np.isnan(want[k])), (where, k)
    key = "general" if runs_general_step(t) else "fused"
    WORST[key] = max(WORST.get(key, 0.0), w)
    return want


# ---- the C entries ----------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A
UNTOUCHED = bytes([SENTINEL]) * C.sizeof(_lib.Td3EvalStats)


def make_io(t, batch, eps, rows=True, arrays=ARRAY_COLUMNS, fill=7.0):
    """(td3_eval_io_t, outputs, inputs kept alive); rows=False: io.rows NULL; arrays: the optional arrays asked for."""
    obs, act, rew, term, nobs = batch
    n = obs.shape[0]
    keep = [_lib.f32(obs), _lib.f32(act), _lib.f32(np.asarray(rew).reshape(-1)), _lib.f32(np.asarray(term).reshape(-1)),
            _lib.f32(nobs), _lib.f32(eps)]
    out = dict(rows=np.full((len(ROW_COLUMNS), n), fill, np.float32)) if rows else {}
    out.update((k, np.full((n, t.act_dim), fill, np.float32)) for k in arrays)
    io = _lib.Td3EvalIO(*[x.ctypes.data for x in keep], out["rows"].ctypes.data if rows else None,
                        *[out[k].ctypes.data if k in out else None for k in ARRAY_COLUMNS])
    return io, out, keep


def stats_many(general, ts, n_rows, ios, stats=True):
    """The *_stats_many entry of one family: (rc, the members' td3_eval_stats_t as bytes; they start as 0x5A)."""
    R = len(ts)
    arr, sts = (_lib.Td3EvalIO * R)(*ios), (_lib.Td3EvalStats * R)()
    C.memset(sts, SENTINEL, C.sizeof(sts))
    rc = getattr(_lib.load(), ENTRY[general])((C.c_void_p * R)(*[t._h.value for t in ts]), R, (C.c_int32 * R)(*n_rows), arr,
                                              sts if stats else None)
    return rc, [bytes(sts[i]) for i in range(R)]


def records(raw):
    return _stats_moments(_lib.Td3EvalStats.from_buffer_copy(raw), _lib.TD3_EVAL_MOMENTS)


# ---- 1. against the host reduction of the same call's columns ------------------------------------------------------------
@pytest.mark.parametrize("steps", [0, 20], ids=["fresh", "20 steps"])
@pytest.mark.parametrize("O,A,hidden,hidden_q", FUSED + GENERAL)
def test_statistics_against_the_host_reduction(O, A, hidden, hidden_q, steps):
    t = make(O, A, hidden, hidden_q, steps=steps)
    general = (O, A, hidden, hidden_q) in GENERAL
    assert runs_general_step(t) == general
    for n in ROWS:
        batch, eps = inputs(n, O, A, 50 + n)
        bd = batch_dict(batch)
        stats, cols = t.evaluate_td3(bd, eps=eps, rows=True, general="device", stats="device")
        h_stats, h_cols = t.evaluate_td3(bd, eps=eps, rows=True, general="device")
        assert same(cols, h_cols), n                                  # the columns are stats="host"'s, bit for bit
        want = check(t, stats, cols, (O, A, hidden, steps, n))
        assert want == h_stats, n
        if n == 1:                                                    # one element: no deviation (a_pi holds A)
            assert all(stats[k] == 0.0 for k in stats if k.endswith(" Std") and (A == 1 or k != "Policy Action Std")), stats
        # without the columns: the same statistics, and nothing else comes back
        assert t.evaluate_td3(bd, eps=eps, general="device", stats="device") == stats, n
        if n <= 1024:                                                 # the records themselves, from the C entry
            io, out, _keep = make_io(t, batch, eps)
            rc, raw = stats_many(general, [t], [n], [io])
            _lib.check(rc, ENTRY[general])
            assert all(bits(out["rows"][i], cols[k]) for i, k in enumerate(ROW_COLUMNS)) and bits(out["a_pi"], cols["a_pi"])
            got = records(raw[0])
            w = check_records(got, td3_eval_moments(rows_of(cols), cols["a_pi"]), rows_of(cols), cols["a_pi"], (hidden, n))
            WORST["records"] = max(WORST.get("records", 0.0), w)
            assert got["a_pi"]["count"] == n * A and got["bellman2"]["count"] == n
    print(f"largest |device - host| / bound so far: {WORST}")


@pytest.mark.parametrize("O,hidden", [(5, (16, 16)), (5, (24,))], ids=["fused", "general"])
def test_a_constant_column_has_no_deviation(O, hidden):
    A = 2
    t = make(O, A, hidden)
    flat = np.array(t.state_dict()["params"]["policy"], np.float32)
    flat[-(A * hidden[-1] + A):-A] = 0.0                              # the head: no weights, one bias for every action
    flat[-A:] = np.float32(0.3)
    t._set_params("policy", flat)
    for n in (1, 300, 1025):
        batch, eps = inputs(n, O, A, n)
        stats, cols = t.evaluate_td3(batch_dict(batch), eps=eps, rows=True, general="device", stats="device")
        c = cols["a_pi"][0, 0]
        assert np.all(cols["a_pi"] == c) and abs(float(c) - np.tanh(0.3)) < 1e-5, n       # (the set-up took)
        assert stats["Policy Action Std"] == 0.0 and stats["Policy Action Mean"] == float(c), n
        assert stats["Policy Action Max"] == stats["Policy Action Min"] == float(c), n
        check(t, stats, cols, (hidden, n))


# ---- 2. grouped == solo, byte for byte -----------------------------------------------------------------------------------
@pytest.mark.parametrize("general", [False, True], ids=["fused", "general"])
def test_sixteen_mixed_members_equal_their_solo_calls(general):
    shapes = (GENERAL + [(6, 16, (16, 16, 16), None)]) if general else (FUSED + [(5, 3, (64, 32), None)])
    n_rows = [257, 1, 33, 1024, 0, 255, 256, 16, 300, 2, 1000, 17, 64, 5, 511, 100]          # member 4 sits out
    ts = [make(*shapes[i % 4], seed=20 + i, steps=5 * (i % 3)) for i in range(16)]
    assert all(runs_general_step(t) == general for t in ts)
    data = [inputs(max(n, 1), t.obs_dim, t.act_dim, 300 + i) for i, (t, n) in enumerate(zip(ts, n_rows))]
    made = [make_io(t, *d) for t, d in zip(ts, data)]
    rc, grouped = stats_many(general, ts, n_rows, [m[0] for m in made])
    _lib.check(rc, ENTRY[general])
    assert grouped[4] == UNTOUCHED and all(np.all(v == 7.0) for v in made[4][1].values())       # sits out
    assert stats_many(general, ts, n_rows, [m[0] for m in made])[1] == grouped                  # a second identical call
    plain = "td3_evaluate_general" if general else "td3_evaluate"
    for i, t in enumerate(ts):
        if n_rows[i] == 0:
            continue
        batch, eps = data[i]
        io, out, keep = make_io(t, batch, eps)
        rc, solo = stats_many(general, [t], [n_rows[i]], [io])
        _lib.check(rc, ENTRY[general])
        assert solo[0] == grouped[i], i                               # byte for byte the solo call's records
        assert all(bits(out[k], made[i][1][k]) for k in out), i
        got = records(solo[0])
        assert [got[k]["count"] for k in got] == [n_rows[i] * (t.act_dim if k == "a_pi" else 1) for k in got], i
        if i % 5:
            continue
        # the columns are those of the entry without statistics
        io0, out0, keep0 = make_io(t, batch, eps)
        _lib.check(getattr(_lib.load(), plain)(t._h, n_rows[i], C.byref(io0)), plain)
        assert all(bits(out[k], out0[k]) for k in out), i
        # no columns copied back (rows NULL, no optional array), and the optional arrays alone left out: the same records
        for kw in (dict(rows=False, arrays=()), dict(arrays=()), dict(arrays=("a_smooth",))):
            io2, out2, keep2 = make_io(t, batch, eps, **kw)
            rc, got2 = stats_many(general, [t], [n_rows[i]], [io2])
            _lib.check(rc, ENTRY[general])
            assert got2[0] == solo[0], (i, kw)
            assert all(bits(out2[k], out[k]) for k in out2), (i, kw)
    # another place in the table, other neighbours: the same records
    order = [15, 3, 0]
    again = [make_io(ts[i], *data[i]) for i in order]                 # (kept: the entry reads and writes the arrays they hold)
    rc, moved = stats_many(general, [ts[i] for i in order], [n_rows[i] for i in order], [m[0] for m in again])
    _lib.check(rc, ENTRY[general])
    assert moved == [grouped[i] for i in order]
    # the Python form: a mixed call, each member's own evaluate_td3(stats="device")
    sub = [0, 4, 3, 9]
    batches = [batch_dict(data[i][0]) if n_rows[i] else None for i in sub]
    epss = [data[i][1] for i in sub]
    for rows in (True, False):
        got = td3_evaluate_many([ts[i] for i in sub], batches, eps=epss, rows=rows, general="device", stats="device")
        assert got[1] is None
        for k, i in enumerate(sub):
            if not n_rows[i]:
                continue
            want = ts[i].evaluate_td3(batches[k], eps=epss[k], rows=rows, general="device", stats="device")
            if rows:
                assert got[k][0] == want[0] and same(got[k][1], want[1]), i
                check(ts[i], got[k][0], got[k][1], ("grouped", general, i))
            else:
                assert got[k] == want, i
    group = ArchTD3TrainerGroup.__new__(ArchTD3TrainerGroup)
    group.trainers = [ts[i] for i in sub]
    assert group.td3_evaluate_many(batches, eps=epss, general="device", stats="device") == got


@pytest.mark.parametrize("general", [False, True], ids=["fused", "general"])
def test_a_nan_observation_reaches_only_its_own_records(general):
    shapes = GENERAL if general else FUSED
    n_rows = [20, 40, 300]
    ts = [make(*shape, seed=30 + i) for i, shape in enumerate(shapes)]
    data = [inputs(n, t.obs_dim, t.act_dim, 400 + i) for i, (t, n) in enumerate(zip(ts, n_rows))]
    first = [make_io(t, *d) for t, d in zip(ts, data)]               # (kept: the entry writes the arrays the ios point to)
    rc, clean = stats_many(general, ts, n_rows, [m[0] for m in first])
    _lib.check(rc, ENTRY[general])
    batch = [x.copy() for x in data[1][0]]
    batch[0][7, ts[1].obs_dim - 1] = np.nan                          # one NaN observation element of member 1
    made = [make_io(t, *d) for t, d in zip(ts, data)]
    made[1] = make_io(ts[1], tuple(batch), data[1][1])
    rc, got = stats_many(general, ts, n_rows, [m[0] for m in made])
    _lib.check(rc, ENTRY[general])
    assert got[0] == clean[0] and got[2] == clean[2] and got[1] != clean[1]     # the neighbours: byte-identical records
    stats, cols = ts[1].evaluate_td3(batch_dict(tuple(batch)), eps=data[1][1], rows=True, general="device", stats="device")
    assert np.isnan(cols["q1"][7]) and np.isnan(cols["a_pi"][7]).all() and not np.isnan(cols["y"]).any()
    want = check(ts[1], stats, cols, ("nan", general))                # NaN where the host's are NaN, within the bound elsewhere
    for name in ("Q1 Predictions", "Policy Action", "Bellman Errors 1", "TD Error 2"):
        assert all(np.isnan(stats[f"{name} {s}"]) and np.isnan(want[f"{name} {s}"]) for s in ("Mean", "Std", "Max", "Min")), name
    assert np.isnan(stats["QF1 Loss"]) and np.isnan(stats["Policy Loss"]) and not np.isnan(stats["Q Targets Mean"])
    rec, before = records(got[1]), records(clean[1])
    for k in ("q1", "q2", "q_pi", "a_pi", "td1", "td2", "bellman1", "bellman2"):
        assert np.isnan(rec[k]["max"]) and np.isnan(rec[k]["min"]) and np.isnan(rec[k]["sum"]) and rec[k]["count"] == before[k]["count"]
    assert rec["y"] == before["y"]                                    # the row's own target is untouched: s' is clean


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    O, A = 6, 3
    fused, fused2 = make(O, A, (16, 16), seed=1), make(O, A, (32, 16), seed=2)
    gen, gen2 = make(O, A, (16, 16, 16), seed=3), make(O, A, (24,), seed=4)
    sac, sacg = make_pair(O, A, 32, seed=4, hidden=(16, 16))[1], make_pair(O, A, 32, seed=4, hidden=(16, 16, 16))[1]
    batch, eps = inputs(8, O, A, 1)
    io1, out1, keep1 = make_io(fused, batch, eps, fill=3.0)
    io2, out2, keep2 = make_io(fused, batch, eps, fill=3.0)

    def refused(general, ts, what, **kw):
        rc, sts = stats_many(general, ts, [8] * len(ts), [io1, io2][:len(ts)], **kw)
        assert rc < 0 and what in _lib.last_error(), (rc, what, _lib.last_error())
        assert all(s == UNTOUCHED for s in sts), what
        assert all(np.all(v == 3.0) for v in list(out1.values()) + list(out2.values())), what

    refused(False, [fused, gen], "general step")                      # each family refuses the other's trainers ...
    refused(False, [fused, gen], "td3_evaluate_general_stats_many")   # ... and names the right entry
    refused(True, [gen, fused], "td3_evaluate_stats_many is its")
    refused(False, [gen], "general step")
    refused(True, [fused], "fused kernels' shapes")
    refused(False, [fused, sac], "is a SAC trainer: this entry evaluates the TD3 objective")
    refused(True, [gen, sacg], "is a SAC trainer: this entry evaluates the TD3 objective")
    refused(False, [fused, fused2], "bad arguments to td3_evaluate_stats_many", stats=False)      # null stats
    refused(True, [gen, gen2], "bad arguments to td3_evaluate_general_stats_many", stats=False)
    refused(False, [fused, fused], "again")
    # a null input array is still refused; null rows alone is not
    broken = _lib.Td3EvalIO.from_buffer_copy(io2)
    broken.obs = None
    rc, sts = stats_many(False, [fused, fused2], [8, 8], [io1, broken])
    assert rc < 0 and "null" in _lib.last_error() and sts == [UNTOUCHED] * 2 and np.all(out1["rows"] == 3.0)
    # and the valid calls behind all this serve
    for general, ts in ((False, [fused, fused2]), (True, [gen, gen2])):
        rc, sts = stats_many(general, ts, [8, 8], [io1, io2])
        assert rc == 0 and UNTOUCHED not in sts and not np.any(out1["rows"] == 3.0)
        out1["rows"][:] = 3.0


# ---- 4. the sweep driver --------------------------------------------------------------------------------------------------
def test_hidden_sweep_logs_each_members_own_results_and_resumes(monkeypatch, tmp_path):
    from robosuite_benchmark_amd import driver
    from tests.test_gpu_td3_evaluate import small_td3_variant
    vs = []
    for hidden in ((128, 64), (64, 96, 48)):                          # the first has the fused kernels' shapes
        v = small_td3_variant()
        v["policy_kwargs"]["hidden_sizes"] = list(hidden)
        v["qf_kwargs"]["hidden_sizes"] = list(hidden)
        vs.append(v)
    runs = [(v, 17 + i) for i, v in enumerate(vs)]
    seen, own = [], dict(validation=[], replay=[])
    real, real_replay = driver.td3_evaluate_many, driver.td3_evaluate_replay_many
    opt = dict(general="device", stats="device")

    def recording(trainers, batches, eps=None, **kw):
        got = real(trainers, batches, eps=eps, **kw)
        seen.append(("validation", kw))
        assert [runs_general_step(t) for t in trainers] == [False, True]
        mine = [t.evaluate_td3(b, eps=e, **kw) for t, b, e in zip(trainers, batches, eps)]
        assert mine == got                                            # each member's own solo result at this moment
        own["validation"].append(mine)
        return got

    def recording_replay(trainers, bufs, n=None, rngs=None, **kw):
        states = [g.get_state() for g in rngs]
        got = real_replay(trainers, bufs, n=n, rngs=rngs, **kw)
        seen.append(("replay", kw))
        mine = []
        for t, b, k, st in zip(trainers, bufs, n, states):
            g = np.random.RandomState()
            g.set_state(st)
            mine.append(t.evaluate_td3_replay(b, n=k, rng=g, **kw))
            g.set_state(st)                                           # and what it stands for: the gathered batch
            idx = g.randint(0, b.num_steps_can_sample(), k)
            assert mine[-1] == t.evaluate_td3(b.gather(idx), eps=g.standard_normal((k, t.act_dim)), **kw)
        assert mine == got and list(n) == [min(32, b.num_steps_can_sample()) for b in bufs]
        own["replay"].append(mine)
        return got

    monkeypatch.setattr(driver, "td3_evaluate_many", recording)
    monkeypatch.setattr(driver, "td3_evaluate_replay_many", recording_replay)
    kw = dict(quiet=True, hidden_sweep=True, td3_validation=True, td3_replay_eval=32, eval_stats="device", eval_general="device")
    ck = str(tmp_path / "ck")
    rows = driver.experiment_sweep(copy.deepcopy(runs), num_epochs=2, checkpoint_dir=ck, **kw)
    # (runs that act on the host: the replay rows of all runs are read in front of the epoch's paths, as SAC's are)
    assert seen == [("replay", opt), ("validation", opt)] * 2
    keys = list(own["validation"][0][0].keys())
    for i, member in enumerate(rows):
        assert len(member) == 2
        for epoch, row in enumerate(member):
            header = list(row.keys())
            at = header.index("validation/Num Transitions")
            assert header[at + 1:at + 2 + len(keys)] == ["replay/" + k for k in keys] + ["replay/Num Transitions"]
            assert row["replay/Num Transitions"] == 32 and row["validation/Num Transitions"] > 0
            for k in keys:
                assert row["validation/" + k] == own["validation"][epoch][i][k], (i, epoch, k)
                assert row["replay/" + k] == own["replay"][epoch][i][k] and np.isfinite(row["replay/" + k]), (i, epoch, k)
        assert member[0]["replay/QF1 Loss"] != member[1]["replay/QF1 Loss"]
    # a resumed run logs the same rows: epoch 0 alone, then epoch 1 behind the checkpoint
    ck1 = str(tmp_path / "ck1")
    first = driver.experiment_sweep(copy.deepcopy(runs), num_epochs=1, checkpoint_dir=ck1, **kw)
    resumed = driver.experiment_sweep(copy.deepcopy(runs), num_epochs=2, checkpoint_dir=ck1, resume=True, **kw)
    for i in range(2):
        assert len(first[i]) == len(resumed[i]) == 1 and resumed[i][0]["Epoch"] == 1
        for a, b in ((first[i][0], rows[i][0]), (resumed[i][0], rows[i][1])):
            assert list(a.keys()) == list(b.keys())
            for k in b:
                assert k.startswith("time/") or a[k] == b[k], (i, k)
    # with the options off the row is what it was
    monkeypatch.setattr(driver, "td3_evaluate_many", real)
    plain = driver.experiment_sweep(copy.deepcopy(runs), num_epochs=1, quiet=True, hidden_sweep=True)
    assert not any(k.startswith(("replay/", "validation/")) for k in plain[0][0])
    assert [k for k in rows[0][0] if not k.startswith(("replay/", "validation/"))] == list(plain[0][0].keys())
    for i in range(2):
        for k in plain[i][0]:
            assert k.startswith("time/") or plain[i][0][k] == rows[i][0][k], (i, k)


def test_zz_report_the_largest_ratio():
    """(prints the largest |device - host| / bound seen above: run with -s)"""
    print(f"td3 device statistics, largest |device - host| / bound: {WORST}")
