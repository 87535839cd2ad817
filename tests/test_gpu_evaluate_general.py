"""GPU: the SAC objectives on held-out transitions for general-step trainers -- sac_evaluate_general /
sac_evaluate_general_many (k_eval_layer, csrc/sac_eval_general.h), the Python entries over them (SACTrainer.evaluate /
evaluate_many with general="device") and the drivers' eval_general="device".

Reference: tests/eval_reference_general.py -- eval_reference.evaluate_reference on nets of any depth built from the
weights and the log_alpha the device holds now, in float32 (P) and float64 (R).  Bound of every column: the project's
per-tensor rule helpers.check_f64 as it stands, max|K - R| / max|R| <= max(8 max|P - R| / max|R|, 1e-5).  Everything else
-- against sac_q_values_general and sac_policy_act_general, y against its float32 NumPy restatement, row independence,
grouped == solo, isolation of a NaN row, "disturbs nothing", the statistics -- is bit for bit.
In the sweep driver the device columns are also held against the HOST path as the fp32 reference P of the same rule.
On an MI355X the largest |K - f64| / max|R| seen per column is q1 3.7e-6, q2 4.7e-6, q1_new 4.5e-6, q2_new 4.8e-6, tq1
5.3e-6, tq2 1.8e-5, log_pi 1.6e-5, log_pi_next 1.7e-5, y 1.6e-5, mu 1.9e-6, log_std 1.7e-6, a_new 6.6e-7, a_next 1.1e-6;
test_zz_report_the_largest_errors prints the largest error per column and shape (run with -s)."""
import copy
import ctypes as C

import numpy as np
import pytest

from robosuite_benchmark_amd import ArchSACTrainerGroup, _lib
from robosuite_benchmark_amd.group import evaluate_many, runs_general_step
from robosuite_benchmark_amd.sac import eval_statistics, eval_target
from tests.eval_reference import ARRAY_COLUMNS, COLUMNS, ROW_COLUMNS, batch_dict
from tests.eval_reference_general import check_columns
from tests.helpers import check_f64, filled_buffer, full_state, make_pair, make_td3_pair, synth_transitions

pytestmark = pytest.mark.gpu
TARGETS = ("target_qf1", "target_qf2")
EVAL_ERRORS = {}            # shape id -> {column: largest |K - f64| / max|R| seen in the parity tests}

# policy hidden sizes, critic hidden sizes (None: the policy's), O, A
SHAPES = [((512, 512), None, 42, 7),               # baseline general shape
          ((256, 256, 256), None, 42, 7),          # three hidden layers
          ((1,), None, 17, 5),                     # width 1
          ((257,), None, 48, 16),                  # head of 32 columns; first Q K of 64
          ((300, 7, 129), None, 379, 6),           # first Q K of 385
          ((64, 96, 48), None, 122, 6),            # first Q K of 128: exactly one chunk
          ((64, 96, 48), None, 123, 6),            # first Q K of 129
          ((16,), None, 1, 1),                     # head of 2 columns
          ((64,) * 7, None, 42, 7),                # depth 7
          ((4096,), None, 42, 7),                  # widest layer
          ((64, 64, 64), (512, 512), 42, 7),       # policy deeper than the critics
          ((512, 512), (256, 256), 42, 7)]         # fused-shape critics in a general trainer
BIG_ROWS = {(512, 512), (300, 7, 129)}             # these run 15, 16, 1000 and 1024 rows too


def shape_id(shape):
    hp, hq, O, A = shape
    return f"p{'x'.join(map(str, hp))}" + ("" if hq is None else f"-q{'x'.join(map(str, hq))}") + f"-O{O}-A{A}"


def rows_of(shape):
    hp, hq, _, _ = shape
    return (1, 17, 33) + ((15, 16, 1000, 1024) if tuple(hp) in BIG_ROWS and hq is None else ())


def fresh(hp, hq=None, O=42, A=7, seed=5, B=32, **kw):
    t = make_pair(O, A, B, seed=seed, hidden=tuple(hp), hidden_q=tuple(hq or hp), **kw)[1]
    assert runs_general_step(t) and t.fused_mode() == 3
    return t


_TRAINERS = {}


def trainer(hp, hq=None, O=42, A=7, seed=5):
    """A general-step trainer of one shape, weights as created (shared by the tests that do not change them)."""
    key = (tuple(hp), None if hq is None else tuple(hq), O, A, seed)
    if key not in _TRAINERS:
        _TRAINERS[key] = fresh(hp, hq, O, A, seed)
    return _TRAINERS[key]


def inputs(n, O, A, seed):
    """(batch, eps): helpers.synth_transitions(term_frac=0.1) and the two (n, A) N(0,1) draws."""
    batch = synth_transitions(n, O, A, seed=seed, term_frac=0.1)
    rs = np.random.RandomState(seed + 7)
    return batch, (rs.standard_normal((n, A)).astype(np.float32), rs.standard_normal((n, A)).astype(np.float32))


def make_io(t, batch, eps, n=None, fill=7.0, arrays=ARRAY_COLUMNS):
    """(sac_eval_io_t, outputs, inputs kept alive) for the C ABI; the outputs start as `fill` (a sentinel)."""
    obs, act, rew, term, nobs = batch
    n = obs.shape[0] if n is None else n
    keep = [_lib.f32(obs), _lib.f32(act), _lib.f32(np.asarray(rew).reshape(-1)), _lib.f32(np.asarray(term).reshape(-1)),
            _lib.f32(nobs), _lib.f32(eps[0]), _lib.f32(eps[1])]
    out = dict(rows=np.full((len(ROW_COLUMNS), n), fill, np.float32))
    out.update((k, np.full((n, t.act_dim), fill, np.float32)) for k in arrays)
    io = _lib.SacEvalIO(*[x.ctypes.data for x in keep], out["rows"].ctypes.data,
                        *[out[k].ctypes.data if k in out else None for k in ARRAY_COLUMNS], -1.0)
    return io, out, keep


def as_columns(out, io):
    cols = {k: out["rows"][i] for i, k in enumerate(ROW_COLUMNS)}
    cols.update((k, out[k]) for k in ARRAY_COLUMNS if k in out)
    cols["alpha"] = float(io.alpha)
    return cols


def eval_g(t, batch, eps, arrays=ARRAY_COLUMNS):
    """sac_evaluate_general through the C ABI: the thirteen arrays (or fewer) and alpha."""
    io, out, _keep = make_io(t, batch, eps, arrays=arrays)
    _lib.check(_lib.load().sac_evaluate_general(t._h, batch[0].shape[0], C.byref(io)), "sac_evaluate_general")
    return as_columns(out, io)


def many_g(ts, n_rows, ios):
    R = len(ts)
    arr = (_lib.SacEvalIO * R)(*ios)
    rc = _lib.load().sac_evaluate_general_many((C.c_void_p * R)(*[None if t is None else t._h.value for t in ts]), R,
                                               (C.c_int32 * R)(*n_rows), arr)
    return rc, arr


def bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same(a, b, keys=COLUMNS):
    return all(bits(a[k], b[k]) for k in keys)


def sweep_rows(t, shape, seed, case):
    errors = EVAL_ERRORS.setdefault(shape_id(shape), {})
    state = t.state_dict()
    for n in rows_of(shape):
        batch, eps = inputs(n, t.obs_dim, t.act_dim, seed + n)
        check_columns(eval_g(t, batch, eps), t, batch, eps, (case, shape_id(shape)), errors, state)
    print(f"{case} {shape_id(shape)}: largest |K - f64| / max|R| so far: " + "  ".join(f"{k} {errors[k]:.3g}" for k in COLUMNS))


# ---- 1. parity with the float64 reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_parity_on_fresh_weights(shape):
    hp, hq, O, A = shape
    t = trainer(hp, hq, O, A)
    assert t._hidden("policy") == list(hp) and t._hidden("qf1") == list(hq or hp)
    sweep_rows(t, shape, O + A, "fresh")


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_parity_behind_twenty_steps(shape):
    hp, hq, O, A = shape
    t = fresh(hp, hq, O, A)
    t.train_loop(filled_buffer(600, O, A, 3), 20, batch_size=32)
    assert t.state_dict()["scalars"][0] != 0.0                        # log_alpha has moved: alpha != 1 in y
    sweep_rows(t, shape, O + A + 1, "20 steps")


# ---- 2. bit for bit against what exists ---------------------------------------------------------------------------------
@pytest.mark.parametrize("hp,hq,O,A,auto", [((512, 512), None, 42, 7, True), ((300, 7, 129), None, 379, 6, True),
                                            ((64, 64, 64), (512, 512), 42, 7, True), ((257,), None, 48, 16, False)])
def test_bitwise_against_the_existing_entries(hp, hq, O, A, auto):
    t = fresh(hp, hq, O, A, seed=6, use_automatic_entropy_tuning=auto, reward_scale=2.5, discount=0.98)
    t.train_loop(filled_buffer(600, O, A, 4), 12, batch_size=32)
    for n in (1, 17, 33, 1000):
        batch, eps = inputs(n, O, A, 100 + n)
        obs, act, rew, term, nobs = batch
        c = eval_g(t, batch, eps)
        q = t.q_values(obs, act, general="device")
        assert bits(c["q1"], q[0]) and bits(c["q2"], q[1]), n
        assert bits(c["a_new"], t.policy_act_general(obs, False, eps[0])), n
        assert bits(c["a_next"], t.policy_act_general(nobs, False, eps[1])), n
        qn = t.q_values(obs, c["a_new"], general="device")
        assert bits(c["q1_new"], qn[0]) and bits(c["q2_new"], qn[1]), n
        tq = t.q_values(nobs, c["a_next"], TARGETS, general="device")
        assert bits(c["tq1"], tq[0]) and bits(c["tq2"], tq[1]), n
        alpha = np.float32(t.state_dict()["scalars"][5]) if auto else np.float32(1.0)
        assert np.float32(c["alpha"]) == alpha and (auto or c["alpha"] == 1.0), (c["alpha"], alpha)
        assert not auto or alpha != 1.0
        r, d = rew.reshape(-1), term.reshape(-1).astype(np.float32)
        y = eval_target(r, d, c["tq1"], c["tq2"], c["log_pi_next"], c["alpha"], 2.5, 0.98)
        assert y.dtype == np.float32 and bits(c["y"], y), n
        assert bits(c["y"][d == 1], (np.float32(2.5) * r)[d == 1]), n
        # the optional arrays may be left out: a_new and a_next still reach the critics
        few = eval_g(t, batch, eps, arrays=("log_std",))
        assert bits(few["log_std"], c["log_std"]) and same(few, c, ROW_COLUMNS), n
    assert np.any(d == 1) and np.any(d == 0)


# ---- 3. independence and isolation --------------------------------------------------------------------------------------
def test_rows_are_independent_bitwise():
    t = trainer((512, 512))
    batch, eps = inputs(1024, 42, 7, 2)
    full = eval_g(t, batch, eps)
    for r in (0, 15, 16, 17, 1023):
        one = eval_g(t, tuple(x[r:r + 1].copy() for x in batch), tuple(e[r:r + 1].copy() for e in eps))
        for k in COLUMNS:
            assert bits(one[k][0], full[k][r]), (r, k)


def mixed_members():
    """Nine general-step SAC members: depths 1 to 7, a policy deeper than its critics, fused-shape critics, mixed dims and
    row counts (0, 1, 16, 17 and 1024 among them), automatic tuning off for one."""
    shapes = [((512, 512), None, 42, 7), ((300, 7, 129), None, 379, 6), ((64,) * 7, None, 42, 7), ((64, 64, 64), (512, 512), 42, 7),
              ((257,), None, 48, 16), ((1,), None, 17, 5), ((512, 512), (256, 256), 42, 7), ((16,), None, 1, 1),
              ((64, 96, 48), None, 123, 6)]
    rows = [17, 1, 0, 64, 16, 33, 5, 1024, 300]
    members = [(trainer(hp, hq, O, A), n) for (hp, hq, O, A), n in zip(shapes, rows)]
    members[4] = (fresh((257,), None, 48, 16, seed=8, use_automatic_entropy_tuning=False), rows[4])
    return members


def test_grouped_equals_solo_bitwise():
    members = mixed_members()
    made = []
    for i, (t, n) in enumerate(members):
        batch, eps = inputs(max(n, 1), t.obs_dim, t.act_dim, 300 + i)
        made.append((batch, eps) + make_io(t, batch, eps, fill=-5.0))
    ts, n_rows = [t for t, _ in members], [n for _, n in members]
    rc, arr = many_g(ts, n_rows, [m[2] for m in made])
    _lib.check(rc, "sac_evaluate_general_many")
    solo = [None if n == 0 else eval_g(t, m[0], m[1]) for (t, n), m in zip(members, made)]
    for i, ((t, n), (batch, eps, _, out, _)) in enumerate(zip(members, made)):
        if n == 0:
            assert all(np.all(v == -5.0) for v in out.values()) and arr[i].alpha == -1.0, i      # sits out: untouched
            continue
        assert same(as_columns(out, arr[i]), solo[i]) and arr[i].alpha == solo[i]["alpha"], i
        check_columns(solo[i], t, batch, eps, ("grouped", i))
    # a member that sits out in front: trainers[0] owns the call's stream and staging
    order = [2] + [i for i in range(len(members)) if i != 2]
    again = [make_io(members[i][0], made[i][0], made[i][1], fill=-5.0) for i in order]
    rc, arr2 = many_g([ts[i] for i in order], [n_rows[i] for i in order], [m[0] for m in again])
    _lib.check(rc, "sac_evaluate_general_many")
    for k, i in enumerate(order):
        assert n_rows[i] == 0 or same(as_columns(again[k][1], arr2[k]), solo[i]), i
    # the Python form: each member's own evaluate(general="device"), None for the member that sits out
    batches = [batch_dict(m[0]) if n else None for (_, n), m in zip(members, made)]
    got = evaluate_many(ts, batches, eps=[m[1] for m in made], rows=True, general="device")
    for i, ((t, n), m) in enumerate(zip(members, made)):
        if n == 0:
            assert got[i] is None
            continue
        stats, cols = t.evaluate(batches[i], eps=m[1], rows=True, general="device")
        assert got[i][0] == stats and same(got[i][1], cols) and same(cols, solo[i]), i


CHAIN_Q, CHAIN_P = ("q1", "q2"), ("q1_new", "q2_new", "log_pi", "mu", "log_std", "a_new")
CHAIN_N = ("tq1", "tq2", "log_pi_next", "y", "a_next")


@pytest.mark.parametrize("hp,O,A", [((512, 512), 42, 7), ((300, 7, 129), 379, 6)])
def test_a_nan_row_stays_nan_and_alone(hp, O, A):
    t = trainer(hp, None, O, A)
    batch, eps = inputs(33, O, A, 5)
    clean = eval_g(t, batch, eps)
    assert all(np.all(np.isfinite(clean[k])) for k in COLUMNS)
    for row in (3, 16, 32):
        keep = np.arange(33) != row
        for which, hit, spared in ((0, CHAIN_Q + CHAIN_P, CHAIN_N), (4, CHAIN_N, CHAIN_Q + CHAIN_P)):
            b = [x.copy() for x in batch]
            b[which][row, 2 % O] = np.nan
            got = eval_g(t, tuple(b), eps)
            for k in hit:
                assert np.all(np.isnan(got[k][row])), (row, which, k)
                assert bits(got[k][keep], clean[k][keep]), (row, which, k)
            for k in spared:
                assert bits(got[k], clean[k]), (row, which, k)


# ---- 4. disturbs nothing ------------------------------------------------------------------------------------------------
def test_evaluate_disturbs_nothing():
    O, A, B = 42, 7, 64
    a, b = fresh((512, 512), O=O, A=A, seed=12, B=B, noise_seed=5), fresh((512, 512), O=O, A=A, seed=12, B=B, noise_seed=5)
    ba, bb = filled_buffer(2000, O, A, 8), filled_buffer(2000, O, A, 8)
    a.train_loop(ba, 5, batch_size=B); b.train_loop(bb, 5, batch_size=B)
    before, diag = full_state(a, ba), dict(a.get_diagnostics())
    counters = (a._num_train_steps, a._need_to_update_eval_statistics)
    batch, eps = inputs(100, O, A, 4)
    a.evaluate(batch_dict(batch), eps=eps, general="device")
    a.evaluate(batch_dict(batch), general="device")
    for x, y in zip(full_state(a, ba), before):
        assert np.array_equal(x, y)
    assert dict(a.get_diagnostics()) == diag and (a._num_train_steps, a._need_to_update_eval_statistics) == counters
    for t in (a, b):
        t.end_epoch(0)
    fa, la = a.train_loop(ba, 10, batch_size=B)                       # a loop behind an evaluation == the loop without it
    fb, lb = b.train_loop(bb, 10, batch_size=B)
    assert np.array_equal(fa, fb) and np.array_equal(la, lb) and a.get_diagnostics() == b.get_diagnostics()
    for _ in range(3):                                                # the stepwise path, on device batches
        a.train(ba.random_batch(B)); b.train(bb.random_batch(B))
        a.evaluate(batch_dict(batch), eps=eps, general="device")
    for x, y in zip(full_state(a, ba), full_state(b, bb)):
        assert np.array_equal(x, y)


def test_the_shared_scratch_does_not_leak():
    O, A = 42, 7
    t = fresh((300, 7, 129), O=O, A=A, seed=7)
    batch, eps = inputs(200, O, A, 9)
    obs, act = batch[0], batch[1]
    first, q1 = t.policy_act_general(obs, False, eps[0]), t.q_values(obs, act, nets=TARGETS + ("qf1", "qf2"), general="device")
    big, beps = inputs(1000, O, A, 10)                                # (the evaluation grows the scratch and fills both buffers)
    cols = eval_g(t, big, beps)
    assert bits(t.policy_act_general(obs, False, eps[0]), first)
    assert bits(t.q_values(obs, act, nets=TARGETS + ("qf1", "qf2"), general="device"), q1)
    assert same(eval_g(t, big, beps), cols)
    check_columns(cols, t, big, beps, "behind acting and Q calls")


# ---- 5. refusals --------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    lib = _lib.load()
    O, A = 42, 7
    a, b = fresh((512, 512), O=O, A=A, seed=1), trainer((64,) * 7, None, O, A)
    fused = make_pair(O, A, 32, seed=4)[1]
    td3 = make_td3_pair(O, A, 32, seed=4, hidden=(512, 512))[1]
    conf = fresh((512, 512), O=O, A=A, seed=6)
    _lib.check(lib.sac_trainer_set_xcd(conf._h, 0), "sac_trainer_set_xcd")
    buf = filled_buffer(500, O, A, 2)
    a.train_loop(buf, 3, batch_size=32)
    batch, eps = inputs(8, O, A, 1)
    want, state = eval_g(a, batch, eps), full_state(a, buf)
    io1, out1, keep1 = make_io(a, batch, eps, fill=3.0)
    io2, out2, keep2 = make_io(b, batch, eps, fill=3.0)

    def refused(rc, what):
        rc = rc[0] if isinstance(rc, tuple) else rc
        assert rc < 0 and what in _lib.last_error(), (rc, what, _lib.last_error())
        assert all(np.all(v == 3.0) for v in list(out1.values()) + list(out2.values())), what
        assert io1.alpha == -1.0 and io2.alpha == -1.0, what
        for x, y in zip(full_state(a, buf), state):
            assert np.array_equal(x, y), what
        assert same(eval_g(a, batch, eps), want), what                # a valid call still gives the right values

    def without(io, field):
        c = _lib.SacEvalIO.from_buffer_copy(io)
        setattr(c, field, None)
        return c

    refused(many_g([a, None], [8, 8], [io1, io2]), "null")
    refused(many_g([a, a], [8, 8], [io1, io2]), "again")
    refused(many_g([a, fused], [8, 8], [io1, io2]), "sac_evaluate is its")
    refused(many_g([a, td3], [8, 8], [io1, io2]), "SAC objective")
    refused(many_g([a, conf], [8, 8], [io1, io2]), "confined")
    refused(many_g([a] * 17, [8] * 17, [io1] * 17), "1..16 trainers")
    refused(many_g([a, b], [8, 1025], [io1, io2]), "rows")
    refused(many_g([a, b], [8, -1], [io1, io2]), "rows")
    refused(many_g([a, b], [0, 0], [io1, io2]), "no trainer has rows")
    for field in ("obs", "act", "rew", "term", "next_obs", "eps", "eps_next", "rows"):
        refused(many_g([a, b], [8, 8], [io1, without(io2, field)]), "null")
    refused(lib.sac_evaluate_general(a._h, 0, C.byref(io1)), "rows")
    refused(lib.sac_evaluate_general(a._h, 1025, C.byref(io1)), "rows")
    refused(lib.sac_evaluate_general(a._h, 8, None), "bad arguments")
    refused(lib.sac_evaluate_general(None, 8, C.byref(io1)), "bad arguments")
    refused(lib.sac_evaluate_general(fused._h, 8, C.byref(io1)), "sac_evaluate is its")
    refused(lib.sac_evaluate_general(td3._h, 8, C.byref(io1)), "SAC objective")
    if _lib.device_count() > 1:                                       # (needs a second GPU to build the case)
        far = fresh((512, 512), O=O, A=A, seed=6, device=1)
        refused(many_g([a, far], [8, 8], [io1, io2]), "device")
    # the fused shapes' entries keep refusing the general-step trainer with their texts
    refused(lib.sac_evaluate(a._h, 8, C.byref(io1)), "general step")
    refused(lib.sac_evaluate(a._h, 8, C.byref(io1)), "forward on the host")
    refused(lib.sac_evaluate(td3._h, 8, C.byref(io1)), "SAC objective")
    # a member that sits out is not looked at
    rc, arr = many_g([a, b], [8, 0], [io1, _lib.SacEvalIO()])
    assert rc == 0 and same(as_columns(out1, arr[0]), want)
    # a confined member is served again once its mask is back to the whole chip
    _lib.check(lib.sac_trainer_set_xcd_mask(conf._h, 0xff), "sac_trainer_set_xcd_mask")
    check_columns(eval_g(conf, batch, eps), conf, batch, eps, "unconfined again")


# ---- 6. Python and drivers ------------------------------------------------------------------------------------------------
def test_statistics_chunks_and_routing():
    O, A = 42, 7
    gen = fresh((512, 512), O=O, A=A, seed=3)
    gen.train_loop(filled_buffer(600, O, A, 5), 10, batch_size=32)
    batch, eps = inputs(2500, O, A, 9)
    stats, cols = gen.evaluate(batch_dict(batch), eps=eps, rows=True, general="device")
    sc = gen.state_dict()["scalars"]
    assert stats == eval_statistics(np.stack([cols[k] for k in ROW_COLUMNS]), cols["mu"], cols["log_std"], cols["alpha"],
                                    sc[0], gen.target_entropy, True)
    assert list(stats.keys())[:-8] == list(gen.get_diagnostics().keys()) and stats["Alpha"] == float(np.float32(sc[5]))
    for lo in (0, 1024, 2048):                                       # any n, in calls of at most 1024 rows
        part = eval_g(gen, tuple(x[lo:lo + 1024] for x in batch), tuple(e[lo:lo + 1024] for e in eps))
        assert all(bits(cols[k][lo:lo + 1024], part[k]) for k in COLUMNS), lo
    # the default stays the host path, bit for bit, and differs from the device's somewhere
    small, seps = inputs(33, O, A, 10)
    host = gen.evaluate(batch_dict(small), eps=seps, rows=True)
    assert host[0] == gen.evaluate(batch_dict(small), eps=seps, general="host") and same(host[1], gen._evaluate_host(
        gen._eval_inputs(batch_dict(small), seps, None)))
    dev = gen.evaluate(batch_dict(small), eps=seps, rows=True, general="device")
    assert same(dev[1], eval_g(gen, small, seps)) and not same(dev[1], host[1])
    check_columns(host[1], gen, small, seps, "host path")
    # a fused-shape trainer takes sac_evaluate under either value; a group call serves both kinds
    fused = make_pair(O, A, 32, seed=4)[1]
    f = fused.evaluate(batch_dict(small), eps=seps, rows=True)
    assert same(fused.evaluate(batch_dict(small), eps=seps, rows=True, general="device")[1], f[1])
    group = ArchSACTrainerGroup([fused, gen])
    got = group.evaluate_many([batch_dict(small)] * 2, eps=[seps] * 2, rows=True, general="device")
    assert got[0][0] == f[0] and same(got[0][1], f[1]) and got[1][0] == dev[0] and same(got[1][1], dev[1])
    got = group.evaluate_many([batch_dict(small)] * 2, eps=[seps] * 2)
    assert got == [f[0], host[0]]
    with pytest.raises(RuntimeError, match="general"):
        gen.evaluate(batch_dict(small), eps=seps, general="gpu")


def test_hidden_sweep_validation_on_the_device(monkeypatch):
    from robosuite_benchmark_amd import driver
    from tests.test_gpu_device_acting import small_variant
    vs = [small_variant("Lift-Panda-OSC-POSE-SEED17", (256, 256), batch=100),
          small_variant("Lift-Panda-OSC-POSE-SEED17", (512, 512), batch=100),
          small_variant("Lift-Panda-OSC-POSE-SEED17", (64, 96, 48), batch=100)]
    runs = [(v, 17 + i) for i, v in enumerate(vs)]
    seen, pairs, real = [], [], driver.evaluate_many
    keys = ("observations", "actions", "rewards", "terminals", "next_observations")

    def recording(trainers, batches, eps=None, **kw):
        got = real(trainers, batches, eps=eps, **kw)
        seen.append(kw)
        for i, (t, b, e, s) in enumerate(zip(trainers, batches, eps, got)):
            if b is None or not runs_general_step(t) or kw.get("general", "host") != "device":
                continue
            # the columns behind the statistics.  Against float64 under the bound of 1.; and against the host run's: the
            # host path is the fp32 reference P of helpers.check_f64 there, max|K - R| <= max(8 max|P - R|, 1e-5) max|R|
            batch, state = tuple(b[k] for k in keys), t.state_dict()
            stats, cols = t.evaluate(b, eps=e, rows=True, general="device")
            h_stats, h_cols = t.evaluate(b, eps=e, rows=True)
            assert stats == s
            r64 = check_columns(cols, t, batch, e, ("sweep", i), state=state)
            for k in COLUMNS:
                check_f64(f"sweep, device against the host path: {k}", cols[k], h_cols[k], r64[k])
            pairs.append((i, stats, h_stats))
        return got

    monkeypatch.setattr(driver, "evaluate_many", recording)
    kw = dict(num_epochs=2, quiet=True, hidden_sweep=True, validation=True)
    dev = driver.experiment_sweep(copy.deepcopy(runs), eval_general="device", **kw)
    assert seen == [dict(general="device")] * 2 and [i for i, _, _ in pairs] == [1, 2, 1, 2]
    host = driver.experiment_sweep(copy.deepcopy(runs), **kw)
    assert seen[2:] == [{}] * 2                                       # (the default call is what it was)
    differs = False
    for i, (rows_d, rows_h) in enumerate(zip(dev, host)):
        assert len(rows_d) == len(rows_h) == 2
        for epoch, (rd, rh) in enumerate(zip(rows_d, rows_h)):
            assert list(rd.keys()) == list(rh.keys()) and "validation/TD Error 2 Min" in rd
            for k in rh:
                if k.startswith("time/"):
                    continue
                if not k.startswith("validation/") or k == "validation/Num Transitions" or i == 0:
                    assert rd[k] == rh[k], (i, k)                     # (run 0 has the fused kernels' shapes)
                else:                                                 # the statistics of the columns checked in `recording`
                    _, d_stats, h_stats = pairs[2 * epoch + i - 1]
                    assert rd[k] == d_stats[k[len("validation/"):]] and rh[k] == h_stats[k[len("validation/"):]], (i, k)
                    differs |= rd[k] != rh[k]
    assert differs                                                    # the general-step runs really were evaluated elsewhere


def test_zz_report_the_largest_errors():
    """(prints the largest |K - f64| / max|R| seen by the parity tests, per shape and column: run with -s)"""
    for case in sorted(EVAL_ERRORS):
        print(f"general evaluate {case}: " + "  ".join(f"{k} {v:.3g}" for k, v in EVAL_ERRORS[case].items()))
    worst = {k: max((e.get(k, 0.0) for e in EVAL_ERRORS.values()), default=0.0) for k in COLUMNS}
    print("general evaluate, largest per column: " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))
