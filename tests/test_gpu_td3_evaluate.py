"""GPU: the TD3 objectives on held-out transitions -- td3_evaluate / td3_evaluate_many (k_eval_td3, csrc/td3_eval.h), the
Python entry points over them (TD3Trainer.evaluate_td3, group.td3_evaluate_many) and the epoch drivers'
td3_validation=True.

Reference: tests/td3_eval_reference.py, the forward half of the TD3 step without any update on the oracle's nets from the
weights the device holds now, in float32 (P) and float64 (R).  Bound of every column: the project's per-tensor rule
helpers.check_f64, max|K - R| / max|R| <= max(8 max|P - R| / max|R|, 1e-5), K == 0 where R == 0, on inputs at which
max|R| is a meaningful unit (td3_eval_reference.conditioned_inputs: chosen from the reference alone).  Everything else --
against sac_q_values and sac_policy_act_device, a_smooth and y against their float32 NumPy restatements, row independence,
grouped == solo, "disturbs nothing" -- is bit for bit."""
import copy
import ctypes as C

import numpy as np
import pytest

from oracle.td3_step_torch import init_td3_params
from robosuite_benchmark_amd import TD3TrainerGroup, _lib
from robosuite_benchmark_amd.checkpoint import load_checkpoint, save_checkpoint
from robosuite_benchmark_amd.group import td3_evaluate_many
from robosuite_benchmark_amd.infer import td3_eval_statistics, td3_eval_target, td3_smooth
from tests.helpers import filled_buffer, full_state, make_pair, make_td3_pair, synth_transitions
from tests.td3_eval_reference import (ARRAY_COLUMNS, COLUMNS, ROW_COLUMNS, SHAPES, batch_dict, check_columns, column_scales,
                                      conditioned_inputs, inputs, make_td3_trainer)

pytestmark = pytest.mark.gpu
ROWS = (1, 15, 16, 17, 1024)
EVAL_ERRORS = {}            # column -> largest |K - f64| / max|R| seen in the parity tests (printed; README quotes them)
TARGETS = ("target_qf1", "target_qf2")
SIGMA, CLIP = 0.3, 0.25     # non-default smoothing: draws beyond clip / sigma = 0.83 clip, the others do not


def make_io(t, batch, eps, n=None, fill=7.0, arrays=ARRAY_COLUMNS):
    """(td3_eval_io_t, outputs, inputs kept alive) for the C ABI; the outputs start as `fill` (a sentinel)."""
    obs, act, rew, term, nobs = batch
    n = obs.shape[0] if n is None else n
    keep = [_lib.f32(obs), _lib.f32(act), _lib.f32(np.asarray(rew).reshape(-1)), _lib.f32(np.asarray(term).reshape(-1)),
            _lib.f32(nobs), _lib.f32(eps)]
    out = dict(rows=np.full((len(ROW_COLUMNS), n), fill, np.float32))
    out.update((k, np.full((n, t.act_dim), fill, np.float32)) for k in arrays)
    io = _lib.Td3EvalIO(*[x.ctypes.data for x in keep], out["rows"].ctypes.data,
                        *[out[k].ctypes.data if k in out else None for k in ARRAY_COLUMNS])
    return io, out, keep


def as_columns(out):
    cols = {k: out["rows"][i] for i, k in enumerate(ROW_COLUMNS)}
    cols.update((k, out[k]) for k in ARRAY_COLUMNS if k in out)
    return cols


def eval_c(t, batch, eps):
    """td3_evaluate through the C ABI: the nine arrays."""
    io, out, _keep = make_io(t, batch, eps)
    _lib.check(_lib.load().td3_evaluate(t._h, batch[0].shape[0], C.byref(io)), "td3_evaluate")
    return as_columns(out)


def many(ts, n_rows, ios):
    R = len(ts)
    arr = (_lib.Td3EvalIO * R)(*ios)
    return _lib.load().td3_evaluate_many((C.c_void_p * R)(*[None if t is None else t._h.value for t in ts]), R,
                                         (C.c_int32 * R)(*n_rows), arr)


def same(a, b, keys=COLUMNS):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def td3_state(t, buf):
    return full_state(t, buf) + [t.state_dict()["params"]["target_policy"]]


def sweep_rows(t, seed, case, rows=ROWS):
    scales = column_scales(t, seed)
    for n in rows:
        batch, eps = conditioned_inputs(t, n, seed + n, scales)
        check_columns(eval_c(t, batch, eps), t, batch, eps, case, EVAL_ERRORS)
    print(f"{case}: largest |K - f64| / max|R| so far: " + "  ".join(f"{k} {EVAL_ERRORS[k]:.3g}" for k in COLUMNS))


# ---- 1. parity with the reference --------------------------------------------------------------------------------------
PARITY = [(O, A, h, None) for O, A, h in SHAPES] + [(42, 7, (64, 32), (256, 256))]


def parity_trainer(O, A, hidden, hidden_q):
    if hidden_q is None:
        return make_td3_pair(O, A, 32, seed=5, hidden=hidden)[1]
    return make_td3_trainer(O, A, hidden, hidden_q, seed=5, batch_size=32, policy_learning_rate=1e-3, qf_learning_rate=5e-4)


@pytest.mark.parametrize("O,A,hidden,hidden_q", PARITY)
def test_parity_on_fresh_weights(O, A, hidden, hidden_q):
    sweep_rows(parity_trainer(O, A, hidden, hidden_q), O + A, ("fresh", O, A, hidden, hidden_q))


@pytest.mark.parametrize("O,A,hidden,hidden_q", PARITY)
def test_parity_behind_twenty_steps(O, A, hidden, hidden_q):
    hip = parity_trainer(O, A, hidden, hidden_q)
    before = hip.state_dict()["params"]
    hip.train_loop(filled_buffer(600, O, A, 3), 20, batch_size=32)
    p = hip.state_dict()["params"]
    assert not np.array_equal(p["target_policy"], p["policy"])       # chain N reads a net of its own ...
    assert not np.array_equal(p["target_policy"], before["target_policy"]) and not np.array_equal(p["policy"], before["policy"])
    sweep_rows(hip, O + A + 1, ("20 steps", O, A, hidden, hidden_q))


# ---- 2. bit for bit against what exists ---------------------------------------------------------------------------------
@pytest.mark.parametrize("O,A,hidden", [(42, 7, (256, 256)), (379, 6, (256, 256)), (46, 16, (240, 256)), (1, 1, (16, 16)),
                                        (42, 7, (128, 64))])
def test_bitwise_against_the_existing_entries(O, A, hidden):
    _, hip = make_td3_pair(O, A, 32, seed=6, hidden=hidden, reward_scale=2.5, discount=0.98, target_policy_noise=SIGMA,
                           target_policy_noise_clip=CLIP)
    hip.train_loop(filled_buffer(600, O, A, 4), 12, batch_size=32)
    clipped = np.zeros(0, bool)
    for n in ROWS:
        batch, eps = inputs(n, O, A, 100 + n)
        obs, act, rew, term, nobs = batch
        c = eval_c(hip, batch, eps)
        q = hip.q_values(obs, act)
        assert np.array_equal(c["q1"], q[0]) and np.array_equal(c["q2"], q[1]), n
        assert np.array_equal(c["a_pi"], hip.policy_act_device(obs, True, None)), n
        assert np.array_equal(c["q_pi"], hip.q_values(obs, c["a_pi"], ("qf1",))[0]), n
        assert np.array_equal(c["a_smooth"], td3_smooth(c["a_target"], eps, SIGMA, CLIP)), n
        tq = hip.q_values(nobs, c["a_smooth"], TARGETS)
        assert np.array_equal(c["tq1"], tq[0]) and np.array_equal(c["tq2"], tq[1]), n
        r, d = rew.reshape(-1), term.reshape(-1).astype(np.float32)
        y = td3_eval_target(r, d, c["tq1"], c["tq2"], 2.5, 0.98)
        assert y.dtype == np.float32 and np.array_equal(c["y"], y), n
        assert np.array_equal(c["y"][d == 1], (np.float32(2.5) * r)[d == 1]), n
        clipped = np.concatenate([clipped, (np.abs(eps * np.float32(SIGMA)) > np.float32(CLIP)).ravel()])
    assert np.any(d == 1) and np.any(d == 0)
    assert np.any(clipped) and np.any(~clipped)                      # some draws clip and some do not


def test_a_target_policy_holding_the_policys_parameters_acts_as_the_policy():
    O, A = 42, 7
    nets = init_td3_params(O, A, seed=9)
    nets["target_policy"] = nets["policy"]
    _, hip = make_td3_pair(O, A, 32, nets=nets)
    batch, eps = inputs(40, O, A, 3)
    c = eval_c(hip, batch, eps)
    assert np.array_equal(c["a_target"], hip.policy_act_device(batch[4], True, None))
    assert not np.array_equal(c["a_target"], c["a_pi"])              # (s' is not s)


# ---- 3. row independence; grouped == solo -------------------------------------------------------------------------------
def test_rows_are_independent_bitwise():
    _, hip = make_td3_pair(42, 7, 32, seed=6)
    batch, eps = inputs(1024, 42, 7, 2)
    full = eval_c(hip, batch, eps)
    for r in (0, 1, 15, 16, 17, 511, 1008, 1023):
        one = eval_c(hip, tuple(x[r:r + 1].copy() for x in batch), eps[r:r + 1].copy())
        for k in COLUMNS:
            assert np.array_equal(one[k][0], full[k][r]), (r, k)


def mixed_members():
    """Sixteen TD3 members of mixed dims, hidden sizes and row counts (0, 1, 15, 16, 17 and 1024 among them)."""
    dims = [(42, 7), (46, 7), (89, 14), (379, 6), (64, 4), (73, 12), (50, 4), (1, 1)]
    rows = [1, 17, 0, 64, 5, 16, 33, 300, 1, 15, 2, 1024, 7, 48, 1, 100]
    members = []
    for i in range(16):
        O, A = dims[i % len(dims)]
        hidden, hidden_q = [((256, 256), None), ((128, 64), None), ((64, 32), (256, 256))][i % 3]
        t = make_td3_trainer(O, A, hidden, hidden_q, seed=20 + i, batch_size=32, target_policy_noise=0.1 + 0.05 * (i % 4))
        members.append((t, rows[i]))
    return members


def test_grouped_equals_solo_bitwise():
    members = mixed_members()
    made = []
    for i, (t, n) in enumerate(members):
        batch, eps = inputs(max(n, 1), t.obs_dim, t.act_dim, 300 + i)
        made.append((batch, eps) + make_io(t, batch, eps, fill=-5.0))
    _lib.check(many([t for t, _ in members], [n for _, n in members], [m[2] for m in made]), "td3_evaluate_many")
    for i, ((t, n), (batch, eps, _, out, _)) in enumerate(zip(members, made)):
        if n == 0:
            assert all(np.all(v == -5.0) for v in out.values()), i    # sits out: untouched
            continue
        assert same(as_columns(out), eval_c(t, batch, eps)), i
    # the Python form: each member's own evaluate_td3, None for the member that sits out
    batches = [batch_dict(m[0]) if n else None for (_, n), m in zip(members, made)]
    got = td3_evaluate_many([t for t, _ in members], batches, eps=[m[1] for m in made], rows=True)
    for i, ((t, n), m) in enumerate(zip(members, made)):
        if n == 0:
            assert got[i] is None
            continue
        stats, cols = t.evaluate_td3(batches[i], eps=m[1], rows=True)
        assert got[i][0] == stats and same(got[i][1], cols) and same(cols, as_columns(m[3])), i


def test_python_windows_above_1024_rows_and_the_host_paths():
    O, A = 42, 7
    _, hip = make_td3_pair(O, A, 32, seed=3)
    hip.train_loop(filled_buffer(600, O, A, 5), 10, batch_size=32)
    batch, eps = inputs(2500, O, A, 9)
    stats, cols = hip.evaluate_td3(batch_dict(batch), eps=eps, rows=True)
    assert stats == td3_eval_statistics(np.stack([cols[k] for k in ROW_COLUMNS]), cols["a_pi"])
    assert list(stats.keys())[:-8] == list(hip.get_diagnostics().keys())
    assert stats["Policy Loss"] == -float(np.mean(cols["q_pi"].astype(np.float64)))
    for lo in (0, 1024, 2048):                                       # any n, in calls of at most 1024 rows
        part = eval_c(hip, tuple(x[lo:lo + 1024] for x in batch), eps[lo:lo + 1024])
        assert all(np.array_equal(cols[k][lo:lo + 1024], part[k]) for k in COLUMNS), lo
    # the private switch of scripts/bench_td3_evaluate.py: the host path of the same trainer, same rule
    small, seps = inputs(33, O, A, 10)
    hip._evaluate_on_host = True
    check_columns(hip.evaluate_td3(batch_dict(small), eps=seps, rows=True)[1], hip, small, seps, "host path of a fused-shape trainer")
    hip._evaluate_on_host = False
    # a trainer of the general step takes the host path, alone and inside a group call
    _, gen = make_td3_pair(O, A, 32, seed=4, hidden=(512, 512))
    assert gen.fused_mode() == 3
    gen.train_loop(filled_buffer(600, O, A, 6), 5, batch_size=32)
    gstats, gcols = gen.evaluate_td3(batch_dict(small), eps=seps, rows=True)
    check_columns(gcols, gen, small, seps, "general step, host path")
    got = td3_evaluate_many([hip, gen], [batch_dict(small)] * 2, eps=[seps] * 2)
    assert got[1] == gstats and got[0] == hip.evaluate_td3(batch_dict(small), eps=seps)
    _, sac = make_pair(O, A, 32, seed=4)
    with pytest.raises(RuntimeError, match="SAC trainer"):
        td3_evaluate_many([hip, sac], [batch_dict(small)] * 2, eps=[seps] * 2)
    with pytest.raises(NotImplementedError, match="SAC objective"):
        hip.evaluate(batch_dict(small))


# ---- 5. nothing disturbed -------------------------------------------------------------------------------------------------
def test_evaluate_disturbs_nothing():
    O, A, B = 42, 7, 64
    (_, a), (_, b) = make_td3_pair(O, A, B, seed=12, noise_seed=5), make_td3_pair(O, A, B, seed=12, noise_seed=5)
    ba, bb = filled_buffer(2000, O, A, 8), filled_buffer(2000, O, A, 8)
    a.train_loop(ba, 5, batch_size=B); b.train_loop(bb, 5, batch_size=B)
    before, diag = td3_state(a, ba), dict(a.get_diagnostics())
    counters = (a._num_train_steps, a._need_to_update_eval_statistics)
    batch, eps = inputs(100, O, A, 4)
    a.evaluate_td3(batch_dict(batch), eps=eps)
    a.evaluate_td3(batch_dict(batch))
    io, out, _keep = make_io(a, batch, eps, arrays=())               # null a_* outputs are accepted
    assert _lib.load().td3_evaluate(a._h, 100, C.byref(io)) == 0
    full = eval_c(a, batch, eps)
    assert np.array_equal(out["rows"], np.stack([full[k] for k in ROW_COLUMNS]))
    for x, y in zip(td3_state(a, ba), before):
        assert np.array_equal(x, y)
    assert dict(a.get_diagnostics()) == diag and (a._num_train_steps, a._need_to_update_eval_statistics) == counters
    for t in (a, b):
        t.end_epoch(0)
    # a loop behind an evaluation == the loop without it: the device noise stream (the smoothing draws) is unmoved
    fa, la = a.train_loop(ba, 10, batch_size=B)
    fb, lb = b.train_loop(bb, 10, batch_size=B)
    assert np.array_equal(fa, fb) and np.array_equal(la, lb) and a.get_diagnostics() == b.get_diagnostics()
    for x, y in zip(td3_state(a, ba), td3_state(b, bb)):
        assert np.array_equal(x, y)
    for _ in range(4):                                                # the stepwise path, on device batches
        a.train(ba.random_batch(B)); b.train(bb.random_batch(B))
        a.evaluate_td3(batch_dict(batch), eps=eps)
    for x, y in zip(td3_state(a, ba), td3_state(b, bb)):
        assert np.array_equal(x, y)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    lib = _lib.load()
    O, A = 42, 7
    (_, a), (_, b) = make_td3_pair(O, A, 32, seed=1), make_td3_pair(O, A, 32, seed=2)
    _, gen = make_td3_pair(O, A, 32, seed=4, hidden=(512, 512))
    _, sac = make_pair(O, A, 32, seed=4)
    _, conf = make_td3_pair(O, A, 32, seed=5)
    _lib.check(lib.sac_trainer_set_xcd(conf._h, 0), "sac_trainer_set_xcd")
    buf = filled_buffer(500, O, A, 2)
    a.train_loop(buf, 3, batch_size=32)
    batch, eps = inputs(8, O, A, 1)
    want, state = eval_c(a, batch, eps), td3_state(a, buf)
    io1, out1, keep1 = make_io(a, batch, eps, fill=3.0)
    io2, out2, keep2 = make_io(b, batch, eps, fill=3.0)

    def refused(rc, what):
        assert rc < 0 and what in _lib.last_error(), (rc, what, _lib.last_error())
        assert all(np.all(v == 3.0) for v in list(out1.values()) + list(out2.values())), what
        for x, y in zip(td3_state(a, buf), state):
            assert np.array_equal(x, y), what
        assert same(eval_c(a, batch, eps), want), what                # a valid call still gives the right values

    def without(io, field):
        c = _lib.Td3EvalIO.from_buffer_copy(io)
        setattr(c, field, None)
        return c

    refused(many([a, None], [8, 8], [io1, io2]), "null")
    refused(many([a, a], [8, 8], [io1, io2]), "again")
    refused(many([a, gen], [8, 8], [io1, io2]), "forward on the host")
    refused(many([a, sac], [8, 8], [io1, io2]), "sac_evaluate")
    refused(many([a, conf], [8, 8], [io1, io2]), "confined")
    refused(many([a, b], [8, 1025], [io1, io2]), "rows")
    refused(many([a, b], [8, -1], [io1, io2]), "rows")
    refused(many([a, b], [0, 0], [io1, io2]), "no trainer has rows")
    refused(many([a] * 17, [8] * 17, [io1] * 17), "1..16 trainers")
    for field in ("obs", "act", "rew", "term", "next_obs", "eps", "rows"):
        refused(many([a, b], [8, 8], [io1, without(io2, field)]), "null")
    refused(lib.td3_evaluate(a._h, 0, C.byref(io1)), "rows")
    refused(lib.td3_evaluate(a._h, 1025, C.byref(io1)), "rows")
    refused(lib.td3_evaluate(a._h, 8, None), "bad arguments")
    refused(lib.td3_evaluate(None, 8, C.byref(io1)), "bad arguments")
    refused(lib.td3_evaluate(gen._h, 8, C.byref(io1)), "general step")
    refused(lib.td3_evaluate(sac._h, 8, C.byref(io1)), "SAC trainer")
    # a member that sits out is not looked at
    assert many([a, b], [8, 0], [io1, _lib.Td3EvalIO()]) == 0 and same(as_columns(out1), want)


# ---- 7. behind every path that moves the nets ---------------------------------------------------------------------------
def test_evaluate_follows_the_live_weights(tmp_path):
    O, A, B = 42, 7, 64
    _, hip = make_td3_pair(O, A, B, seed=9)
    _, other = make_td3_pair(O, A, B, seed=10)
    buf, obuf = filled_buffer(2000, O, A, 3), filled_buffer(2000, O, A, 4)
    batch, eps = inputs(40, O, A, 6)
    other.train_loop(obuf, 7, batch_size=B)
    save_checkpoint(str(tmp_path), other, obuf, dict(epoch=0))
    o, ac, rew, term, nobs = synth_transitions(B, O, A, seed=50)
    donor = make_td3_pair(O, A, B, seed=11)[1].state_dict()
    steps = [("initial", lambda: None),
             ("train", lambda: [hip.train(dict(observations=o, actions=ac, rewards=rew, terminals=term, next_observations=nobs))
                                for _ in range(2)]),
             ("train_loop", lambda: hip.train_loop(buf, 8, batch_size=B)),
             ("group loop", lambda: TD3TrainerGroup([hip]).train_loop([buf], 6, batch_size=B)),
             ("load_state_dict", lambda: hip.load_state_dict(donor)),
             ("checkpoint load", lambda: load_checkpoint(str(tmp_path), hip, buf))]
    last = None
    for what, move in steps:
        move()
        _, now = hip.evaluate_td3(batch_dict(batch), eps=eps, rows=True)
        check_columns(now, hip, batch, eps, what)
        if last is not None:
            changed = [k for k in COLUMNS if not np.array_equal(now[k], last[k])]
            assert set(changed) == set(COLUMNS), (what, changed)
        last = now
    assert same(last, other.evaluate_td3(batch_dict(batch), eps=eps, rows=True)[1])      # the loaded state, exactly


# ---- 8. non-finite ----------------------------------------------------------------------------------------------------------
CHAIN_Q, CHAIN_P, CHAIN_N = ("q1", "q2"), ("q_pi", "a_pi"), ("tq1", "tq2", "y", "a_target", "a_smooth")


@pytest.mark.parametrize("hidden", [(256, 256), (128, 64)])
def test_a_nan_row_stays_nan_and_alone(hidden):
    _, hip = make_td3_pair(42, 7, 32, seed=8, hidden=hidden)
    batch, eps = inputs(20, 42, 7, 5)
    clean = eval_c(hip, batch, eps)
    assert all(np.all(np.isfinite(clean[k])) for k in COLUMNS)
    keep = np.arange(20) != 3
    for which, hit, spared in ((0, CHAIN_Q + CHAIN_P, CHAIN_N), (4, CHAIN_N, CHAIN_Q + CHAIN_P)):
        b = [x.copy() for x in batch]
        b[which][3, 2] = np.nan
        got = eval_c(hip, tuple(b), eps)
        for k in hit:
            assert np.all(np.isnan(got[k][3])), (which, k)
            assert np.array_equal(got[k][keep], clean[k][keep]), (which, k)
        for k in spared:
            assert np.array_equal(got[k], clean[k]), (which, k)
    # a NaN draw: a NaN a_smooth element there and nowhere else; that row's targets follow, a_target and the rest do not
    e = eps.copy()
    e[5, 2] = np.nan
    got = eval_c(hip, batch, e)
    at = np.zeros_like(e, bool)
    at[5, 2] = True
    assert np.all(np.isnan(got["a_smooth"][at])) and np.array_equal(got["a_smooth"][~at], clean["a_smooth"][~at])
    assert np.array_equal(got["a_target"], clean["a_target"]) and all(np.array_equal(got[k], clean[k]) for k in CHAIN_Q + CHAIN_P)
    rest = np.arange(20) != 5
    for k in ("tq1", "tq2", "y"):
        assert np.isnan(got[k][5]) and np.array_equal(got[k][rest], clean[k][rest]), k


# ---- 9. driver --------------------------------------------------------------------------------------------------------------
def small_td3_variant():
    from robosuite_benchmark_amd.variant import default_variant
    v = default_variant(env="Lift", seed=17, batch_size=64, agent="TD3")
    v["algorithm_kwargs"].update(min_num_steps_before_training=150, num_eval_steps_per_epoch=130,
                                 num_expl_steps_per_train_loop=170, num_trains_per_train_loop=40,
                                 eval_max_path_length=50, expl_max_path_length=60)
    v["replay_buffer_size"] = 3000
    return v


def test_experiment_group_td3_validation(monkeypatch):
    from robosuite_benchmark_amd import driver
    v, seeds = small_td3_variant(), [17, 18]
    plain = driver.experiment_group(copy.deepcopy(v), seeds=seeds, num_epochs=2, quiet=True)
    calls, many_fn = [], driver.td3_evaluate_many

    def recording(trainers, batches, eps=None, rngs=None, rows=False):
        got = many_fn(trainers, batches, eps=eps, rngs=rngs, rows=rows)
        solo = []
        for s, t, b in zip(seeds, trainers, batches):                # each member's own evaluate_td3 at this point
            n = b["observations"].shape[0]
            mine = np.random.RandomState([s, len(calls), 0x56414C]).standard_normal((n, t.act_dim))
            stats, cols = t.evaluate_td3(b, eps=mine, rows=True)
            check_columns(cols, t, tuple(b[k] for k in ("observations", "actions", "rewards", "terminals",
                                                         "next_observations")), mine, "experiment_group")
            solo.append((stats, n))
        assert got == [s for s, _ in solo] and rngs is None and rows is False
        calls.append(solo)
        return got

    monkeypatch.setattr(driver, "td3_evaluate_many", recording)
    rows = driver.experiment_group(copy.deepcopy(v), seeds=seeds, num_epochs=2, quiet=True, td3_validation=True)
    assert len(calls) == 2                                           # ONE td3_evaluate_many call per epoch
    for i, s in enumerate(seeds):
        assert len(rows[s]) == len(plain[s]) == 2
        header = list(plain[s][0].keys())
        at = header.index("time/data storing (s)")
        keys = list(calls[0][i][0].keys())
        assert keys[:-8] == [k[len("trainer/"):] for k in header if k.startswith("trainer/")]
        v_columns = ["validation/" + k for k in keys] + ["validation/Num Transitions"]
        for epoch, (row, want) in enumerate(zip(rows[s], plain[s])):
            assert list(row.keys()) == header[:at] + v_columns + header[at:]
            for k in want:                                           # every other column: the run with the option off
                if not k.startswith("time/"):
                    assert row[k] == want[k], (s, k)
            stats, n = calls[epoch][i]
            assert row["validation/Num Transitions"] == n == 100
            assert all(row["validation/" + k] == stats[k] for k in keys)
        assert rows[s][0]["validation/QF1 Loss"] != rows[s][1]["validation/QF1 Loss"]      # the critics moved
    # the solo driver logs the same rows
    solo = driver.experiment(copy.deepcopy(v), seed=17, num_epochs=2, quiet=True, td3_validation=True)
    for rg, rw in zip(rows[17], solo):
        assert list(rg.keys()) == list(rw.keys())
        assert all(rg[k] == rw[k] for k in rw if not k.startswith("time/"))
