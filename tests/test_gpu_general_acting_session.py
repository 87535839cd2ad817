"""GPU: acting sessions for general-step policies (sac_gactor_*, k_act_layer_session, csrc/sac_actor_general.h;
group.GroupActor(general="device", general_sessions=True)) against the solo entry.

There are no tolerances here.  The reference is sac_policy_act_general on obs.astype(np.float32) with the same eps, and
every comparison views the float32 actions as uint32.  Accuracy against the float64 oracle is bounded for that entry in
tests/test_gpu_general_acting.py; bit equality carries the bound over."""
import copy
import ctypes as C

import numpy as np
import pytest

from robosuite_benchmark_amd import ArchSACTrainerGroup, GroupActor, MlpSACTrainerGroup, _lib
from robosuite_benchmark_amd.group import runs_general_step
from tests.helpers import filled_buffer, is_td3, make_pair, make_td3_pair

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-7.5)

# policy hidden sizes, O, A: N and K on both sides of the 16- and 64-wide tile edges and of the 128-wide reduction chunk,
# K not a multiple of 4 with a K edge chunk, depth 1 and 7, head widths 2 and 32
SHAPES = [((1,), 17, 5), ((257,), 42, 16), ((300, 7, 129), 379, 6), ((64,) * 7, 42, 7), ((64, 96, 48), 42, 1),
          ((512, 512), 42, 7)]
CASES = [("sac", *s) for s in SHAPES] + [("td3", (300, 7, 129), 379, 6), ("td3", (1,), 17, 5)]


def case_id(case):
    algo, hidden, O, A = case
    return f"{algo}-h{'x'.join(map(str, hidden))}-O{O}-A{A}"


_TRAINERS = {}


def trainer(algo, hidden, O, A, seed=5, B=32):
    """A general-step trainer of one shape, weights as created (shared by the tests that do not change them)."""
    key = (algo, tuple(hidden), O, A, seed, B)
    if key not in _TRAINERS:
        _TRAINERS[key] = fresh(algo, hidden, O, A, seed, B)
    return _TRAINERS[key]


def fresh(algo, hidden, O=42, A=7, seed=5, B=32):
    t = (make_pair if algo == "sac" else make_td3_pair)(O, A, B, seed=seed, hidden=tuple(hidden))[1]
    assert runs_general_step(t)
    return t


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def draws64(rs, n, O, A):
    """(n, O) float64 observations that are NOT float32 values, and (n, A) float32 eps."""
    obs = rs.normal(0, 0.4, (n, O))
    assert np.all(obs.astype(np.float32).astype(np.float64) != obs)
    return obs, rs.normal(size=(n, A)).astype(np.float32)


def solo(t, obs64, det, eps):
    """The reference: sac_policy_act_general through the C ABI on the observations cast to float32."""
    with np.errstate(over="ignore"):
        obs = np.ascontiguousarray(obs64.astype(np.float32))
    n = obs.shape[0]
    out = np.full((n, t.act_dim), 7.0, np.float32)
    e = None if (det or is_td3(t)) else np.ascontiguousarray(eps, np.float32)
    _lib.check(_lib.load().sac_policy_act_general(t._h, n, _lib.ptr(obs), int(det), _lib.ptr(e), _lib.ptr(out)),
               "sac_policy_act_general")
    return out


def create(hs, max_rows):
    a, n = C.c_void_p(), len(hs)
    rc = _lib.load().sac_gactor_create(C.byref(a), (C.c_void_p * n)(*hs), n, (C.c_int32 * n)(*max_rows))
    return rc, a


class Session:
    """sac_gactor_* through the C ABI: the handle and the slab views of every member."""

    def __init__(self, ts, max_rows):
        self.lib, self.ts, self.max_rows = _lib.load(), ts, list(max_rows)
        rc, self.a = create([t._h.value for t in ts], max_rows)
        _lib.check(rc, "sac_gactor_create")
        self.obs, self.eps, self.act, self.addr = [], [], [], []
        for k, (t, m) in enumerate(zip(ts, max_rows)):
            p = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
            _lib.check(self.lib.sac_gactor_arrays(self.a, k, *[C.byref(x) for x in p]), "sac_gactor_arrays")
            self.addr.append([x.value for x in p])
            view = lambda x, ct, cols: np.ctypeslib.as_array((ct * (m * cols)).from_address(x.value)).reshape(m, cols)  # noqa: E731
            self.obs.append(view(p[0], C.c_double, t.obs_dim))
            self.eps.append(view(p[1], C.c_float, t.act_dim))
            self.act.append(view(p[2], C.c_float, t.act_dim))

    def call(self, n_rows, det):
        n = len(self.ts)
        return self.lib.sac_gactor_act(self.a, (C.c_int32 * n)(*n_rows), (C.c_int32 * n)(*[int(d) for d in det]))

    def tick(self, n_rows, det):
        _lib.check(self.call(n_rows, det), "sac_gactor_act")

    def close(self):
        a, self.a = self.a, None
        if a:
            assert self.lib.sac_gactor_destroy(a) == 0

    def __del__(self):
        self.close()


def fill(s, k, obs, eps):
    n = obs.shape[0]
    s.obs[k][:n], s.eps[k][:n] = obs, eps
    s.act[k][...] = SENTINEL


def check_member(s, k, n, det, obs, eps, where):
    """Rows [0, n) of member k equal the solo call; the rows behind them keep the sentinel."""
    if n:
        assert np.array_equal(bits(s.act[k][:n]), bits(solo(s.ts[k], obs[:n], det, eps[:n]))), where
    assert np.all(s.act[k][n:] == SENTINEL), where


# ---- one member against the solo entry ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_one_member_equals_the_solo_entry(case):
    algo, hidden, O, A = case
    t = trainer(algo, hidden, O, A)
    sizes = (1, 17, 33) + ((1024,) if tuple(hidden) == (512, 512) else ())
    obs, eps = draws64(np.random.RandomState(O * 31 + A + len(hidden)), max(sizes), O, A)
    for max_rows in sizes:
        s = Session([t], [max_rows])
        assert all(a % 256 == 0 for a in s.addr[0])
        for rows in sorted({r for r in (1, 16, 17, max_rows) if r <= max_rows}):
            got = {}
            for det in (True, False):
                fill(s, 0, obs[:max_rows], eps[:max_rows])
                s.tick([rows], [det])
                check_member(s, 0, rows, det, obs, eps, (case_id(case), max_rows, rows, det))
                got[det] = s.act[0][:rows].copy()
            assert np.array_equal(got[True], got[False]) == (algo == "td3")       # TD3 is deterministic whatever the flag
        assert np.array_equal(s.obs[0], obs[:max_rows])                           # the inputs are only read
        s.close()


def test_observations_are_rounded_as_astype_float32_rounds_them():
    u = 2.0 ** -24                                                       # half an ulp of float32 at 1
    fmax = float(np.finfo(np.float32).max)
    sub = 2.0 ** -149                                                    # the smallest float32 subnormal
    finite = np.array([1 + u, 1 + 3 * u, 1 + u - 2.0 ** -50, 1 + u + 2.0 ** -50, 1 + 3 * u - 2.0 ** -50, 1 + 3 * u + 2.0 ** -50,
                       1.0 / 3.0, 1e-40, 1.5 * sub, 2.5 * sub, 0.5 * sub, 0.5 * sub * (1 + 2.0 ** -40), 1e-46], np.float64)
    huge = np.array([1e39, fmax + 2.0 ** 103, fmax + 2.0 ** 103 - 2.0 ** 80, 1e300], np.float64)
    with np.errstate(over="ignore"):
        cf, ch = finite.astype(np.float32), huge.astype(np.float32)
    one = np.float32(1.0)
    assert np.all(cf.astype(np.float64) != finite)                       # none is a float32 value
    assert cf[0] == one and cf[1] == np.float32(1 + 4 * u)                # ties go to even: down, and up
    assert cf[2] == one and cf[3] == np.float32(1 + 2 * u) and cf[4] == np.float32(1 + 2 * u) and cf[5] == np.float32(1 + 4 * u)
    assert cf[7] == np.float32(1e-40) and 0 < cf[7] < np.finfo(np.float32).tiny          # a subnormal result
    assert cf[8] == np.float32(2 * sub) and cf[9] == np.float32(2 * sub)                 # subnormal ties, to even
    assert cf[10] == 0.0 and cf[11] == np.float32(sub) and cf[12] == 0.0
    assert np.isinf(ch[0]) and np.isinf(ch[1]) and ch[2] == np.float32(fmax) and np.isinf(ch[3])     # beyond the range
    vals = np.concatenate([finite, -finite])
    rs = np.random.RandomState(2)
    for algo, hidden, O, A in (("sac", (512, 512), 42, 7), ("td3", (300, 7, 129), 379, 6), ("sac", (1,), 17, 5)):
        n = 19
        obs = vals[rs.randint(0, vals.size, (n, O))]
        obs[0, :13], obs[1, :13] = finite[:min(13, O)], -finite[:min(13, O)]
        obs[2, :O] = np.resize(vals, O)
        obs[n - 2, :4], obs[n - 1, 4:8] = huge, -huge                    # two rows hold what overflows to +-inf
        with np.errstate(over="ignore"):
            o32 = obs.astype(np.float32)
        assert np.all(o32[:n - 2].astype(np.float64) != obs[:n - 2]) and np.isinf(o32[n - 2:]).sum() == 6
        assert np.signbit(o32[1, 12]) and o32[1, 12] == 0.0               # -1e-46 -> -0.0
        eps = rs.normal(size=(n, A)).astype(np.float32)
        t = trainer(algo, hidden, O, A)
        s = Session([t], [n])
        for det in (True, False):
            fill(s, 0, obs, eps)
            s.tick([n], [det])
            check_member(s, 0, n, det, obs, eps, (algo, hidden, det))
        assert np.all(np.isfinite(s.act[0][:n - 2]))
        s.close()


# ---- several members ------------------------------------------------------------------------------------------------------
def test_mixed_depths_in_one_session():
    ts = [trainer("sac", (512, 512), 42, 7), trainer("td3", (300, 7, 129), 379, 6), trainer("sac", (64,) * 7, 42, 7),
          trainer("sac", (1,), 17, 5), trainer("sac", (1024,), 42, 7)]
    max_rows = [5, 17, 4, 2, 16]
    s = Session(ts, max_rows)
    rs = np.random.RandomState(4)
    for step, (rows, det) in enumerate([([3, 17, 0, 1, 16], [False, False, False, True, False]),
                                        ([0, 17, 4, 2, 16], [False, True, False, False, True]),        # member 0 sits out
                                        ([5, 0, 0, 0, 0], [True] * 5), ([0, 0, 0, 2, 0], [False] * 5)]):
        data = [draws64(rs, m, t.obs_dim, t.act_dim) for t, m in zip(ts, max_rows)]
        for k, (o, e) in enumerate(data):
            fill(s, k, o, e)
        s.tick(rows, det)
        for k, (o, e) in enumerate(data):
            check_member(s, k, rows[k], det[k], o, e, (step, k))
            assert np.array_equal(s.obs[k], o) and np.array_equal(bits(s.eps[k]), bits(e)), (step, k)
    s.close()


def test_sixteen_members_with_one_row_each():
    small = [("sac", (1,), 17, 5), ("sac", (257,), 42, 16), ("sac", (64, 96, 48), 42, 1), ("td3", (1,), 17, 5)]
    ts = [trainer(*small[i % 4], seed=5 + i // 4) for i in range(16)]
    assert len({id(t) for t in ts}) == 16
    s = Session(ts, [1] * 16)
    rs = np.random.RandomState(16)
    for det in ([False] * 16, [i % 2 == 0 for i in range(16)]):
        data = [draws64(rs, 1, t.obs_dim, t.act_dim) for t in ts]
        for k, (o, e) in enumerate(data):
            fill(s, k, o, e)
        s.tick([1] * 16, det)
        for k, (o, e) in enumerate(data):
            check_member(s, k, 1, det[k], o, e, k)
    # the same architecture with another seed is another policy
    assert not np.array_equal(s.act[0], s.act[4])
    s.close()


def test_one_session_reused_across_row_counts_and_flags():
    ts = [trainer("sac", (512, 512), 42, 7), trainer("sac", (300, 7, 129), 379, 6)]
    s = Session(ts, [17, 17])
    rs = np.random.RandomState(8)
    for step, (rows, det) in enumerate([((17, 17), (False, True)), ((1, 16), (True, False)), ((16, 1), (False, False)),
                                        ((17, 0), (True, True)), ((1, 17), (False, False))]):
        data = [draws64(rs, 17, t.obs_dim, t.act_dim) for t in ts]
        for k, (o, e) in enumerate(data):
            fill(s, k, o, e)                                              # (all 17 rows staged: only rows [0, n) may count)
        s.tick(rows, det)
        for k, (o, e) in enumerate(data):
            check_member(s, k, rows[k], det[k], o, e, (step, k))
    s.close()


def test_two_sessions_over_the_same_trainers_and_the_solo_entry_in_between():
    ts = [trainer("sac", (512, 512), 42, 7), trainer("sac", (64,) * 7, 42, 7), trainer("td3", (300, 7, 129), 379, 6)]
    rs = np.random.RandomState(5)
    a, b = Session(ts, [3, 3, 3]), Session(ts, [40, 40, 40])              # different max_rows: different scratch strides
    data = [draws64(rs, 40, t.obs_dim, t.act_dim) for t in ts]
    for rnd in range(2):
        for s, n, det in ((a, 3, True), (b, 40, False), (a, 2, False), (b, 17, True)):
            other = b if s is a else a
            kept = [x.copy() for x in other.obs + other.eps + other.act]
            for k, (o, e) in enumerate(data):
                fill(s, k, o[:s.max_rows[k]], e[:s.max_rows[k]])
            s.tick([n] * 3, [det] * 3)
            got = [x[:n].copy() for x in s.act]
            # the solo entry (the trainers' own scratch, 1000 rows: reallocated under both sessions the first time) ...
            big = [solo(t, np.resize(o, (1000, t.obs_dim)), det, np.resize(e, (1000, t.act_dim))) for t, (o, e) in zip(ts, data)]
            for k, (o, e) in enumerate(data):
                check_member(s, k, n, det, o, e, (rnd, n, det, k))
                assert np.array_equal(bits(got[k]), bits(big[k][:n])), (rnd, n, det, k)
            for x, y in zip(kept, other.obs + other.eps + other.act):
                assert np.array_equal(x, y, equal_nan=True), (rnd, n, det)
    a.close()
    b.close()


# ---- live weights -------------------------------------------------------------------------------------------------------
def _solo_loop(tmp):
    t = fresh("sac", (512, 512), seed=9, B=48)
    buf = filled_buffer(1500, 42, 7, 3)
    return [t], lambda: t.train_loop(buf, 5, batch_size=48)


def _mlp_group(tmp):
    ts = [fresh("sac", (512, 512), seed=30 + i, B=48) for i in range(2)]
    bufs = [filled_buffer(1500, 42, 7, 40 + i) for i in range(2)]
    return ts, lambda: MlpSACTrainerGroup(ts).train_loop(bufs, 5)


def _arch_group(tmp):
    ts = [fresh("sac", h, seed=33 + i, B=48) for i, h in enumerate([(512, 512), (64, 96, 48)])]
    fused = make_pair(42, 7, 48, seed=36)[1]
    bufs = [filled_buffer(1500, 42, 7, 43 + i) for i in range(3)]
    return ts, lambda: ArchSACTrainerGroup([fused] + ts).train_loop(bufs, 5)


def _set_params(tmp):
    t, u = fresh("sac", (300, 7, 129), 379, 6, seed=9), fresh("sac", (300, 7, 129), 379, 6, seed=10)
    return [t], lambda: t._set_params("policy", u.state_dict()["params"]["policy"])


def _checkpoint(tmp):
    from robosuite_benchmark_amd.checkpoint import load_checkpoint, save_checkpoint
    t = fresh("sac", (512, 512), seed=11, B=48)
    buf = filled_buffer(1500, 42, 7, 5)
    t.train_loop(buf, 5, batch_size=48)
    save_checkpoint(str(tmp / "ck"), t, buf)
    t.train_loop(buf, 5, batch_size=48)
    return [t], lambda: load_checkpoint(str(tmp / "ck"), t, buf) and None


LIVE = {"train_loop": _solo_loop, "MlpSACTrainerGroup": _mlp_group, "ArchSACTrainerGroup": _arch_group,
        "sac_set_params": _set_params, "checkpoint load": _checkpoint}


@pytest.mark.parametrize("path", list(LIVE))
def test_a_session_sees_the_weights_behind(path, tmp_path):
    """Act with the session, move the policy, act again with the SAME session: each time it equals the solo entry called
    afterwards (the session itself drains steps nobody waited for), and the second result differs from the first."""
    ts, run = LIVE[path](tmp_path)
    n = 19
    s = Session(ts, [n] * len(ts))
    handles = [t._handle_gen for t in ts]
    rs = np.random.RandomState(6)
    data = [draws64(rs, n, t.obs_dim, t.act_dim) for t in ts]
    seen = []
    for phase in range(2):
        if phase:
            run()
        got = []
        for det in (True, False):
            for k, (o, e) in enumerate(data):
                fill(s, k, o, e)
            s.tick([n] * len(ts), [det] * len(ts))
            got.append([a.copy() for a in s.act])
            for k, (o, e) in enumerate(data):
                check_member(s, k, n, det, o, e, (path, phase, det, k))
        seen.append(got)
    assert [t._handle_gen for t in ts] == handles                         # (the session's handles are still the trainers')
    for k in range(len(ts)):
        for d in range(2):
            assert not np.array_equal(seen[0][d][k], seen[1][d][k]), (path, k, d)
    s.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    lib = _lib.load()
    t0, t1 = trainer("sac", (512, 512), 42, 7), trainer("td3", (1,), 17, 5)
    fused = make_pair(42, 7, 32, seed=1)[1]
    h0, h1 = t0._h.value, t1._h.value
    for hs, mr, text in [([h0, fused._h.value], [1, 1], "sac_actor_create"), ([h0, None], [1, 1], "trainer 1 is null"),
                         ([h0, h1, h0], [1, 1, 1], "trainer 2 is trainer 0 again"),
                         ([h0] * 17, [1] * 17, "takes 1..16 trainers (got 17)"), ([], [], "takes 1..16 trainers (got 0)"),
                         ([h0, h1], [1, 0], "trainer 1: max_rows 0 (1..1024)"),
                         ([h0, h1], [1025, 1], "trainer 0: max_rows 1025 (1..1024)")]:
        rc, a = create(hs, mr)
        assert rc < 0 and a.value is None and text in _lib.last_error(), (text, _lib.last_error())
    a = C.c_void_p(12345)                                                 # *out is null on failure, whatever it held
    assert lib.sac_gactor_create(C.byref(a), (C.c_void_p * 1)(fused._h.value), 1, (C.c_int32 * 1)(4)) < 0 and a.value is None
    assert "trainer 0 has the fused kernels' shapes" in _lib.last_error()
    # sac_actor_create keeps refusing general-step trainers
    a = C.c_void_p()
    assert lib.sac_actor_create(C.byref(a), (C.c_void_p * 1)(h0), 1, (C.c_int32 * 1)(4)) < 0 and not a
    assert "general step" in _lib.last_error()

    s = Session([t0, t1], [5, 3])
    rs = np.random.RandomState(9)
    data = [draws64(rs, m, t.obs_dim, t.act_dim) for t, m in zip(s.ts, s.max_rows)]
    for k, (o, e) in enumerate(data):
        fill(s, k, o, e)
    slab = lambda: [x.copy() for x in s.obs + s.eps + s.act]  # noqa: E731
    kept = slab()
    for rows, text in [((6, 1), "trainer 0: 6 rows (0..5 in this session"), ((1, 4), "trainer 1: 4 rows (0..3 in this session"),
                       ((1, -1), "trainer 1: -1 rows (0..3 in this session"), ((0, 0), "no trainer has rows to act on")]:
        assert s.call(rows, (0, 0)) < 0 and text in _lib.last_error(), (text, _lib.last_error())
        assert all(np.array_equal(x, y) for x, y in zip(kept, slab())), text
    # a member confined to XCDs is refused while it is confined, whether it has rows or not
    confined = fresh("sac", (1,), 17, 5, seed=7)
    sc = Session([t0, confined], [5, 2])
    fill(sc, 0, *data[0])
    _lib.check(lib.sac_trainer_set_xcd_mask(confined._h, 0x0f), "sac_trainer_set_xcd_mask")
    for rows in ((5, 1), (5, 0)):
        assert sc.call(rows, (0, 0)) < 0 and "trainer 1 is confined by sac_trainer_set_xcd[_mask]" in _lib.last_error()
        assert np.all(sc.act[0] == SENTINEL)
    _lib.check(lib.sac_trainer_set_xcd_mask(confined._h, 0xff), "sac_trainer_set_xcd_mask")
    sc.tick((5, 0), (0, 0))
    check_member(sc, 0, 5, False, *data[0], "after the confinement")
    sc.close()
    # ... and a valid call on the first session after all its refusals
    s.tick((5, 3), (0, 1))
    for k, (o, e) in enumerate(data):
        check_member(s, k, s.max_rows[k], bool(k), o, e, ("after refusals", k))
    bad = C.c_void_p()
    assert lib.sac_gactor_arrays(s.a, 2, C.byref(bad), None, None) < 0 and "member 2 of 2" in _lib.last_error()
    assert lib.sac_gactor_act(None, None, None) < 0 and "bad arguments" in _lib.last_error()
    assert lib.sac_gactor_destroy(None) == 0
    s.close()


# ---- GroupActor ---------------------------------------------------------------------------------------------------------
def test_group_actor_with_general_sessions_equals_without():
    ts = [make_pair(42, 7, 32, seed=21)[1], fresh("sac", (512, 512), 42, 7, seed=22), make_td3_pair(46, 7, 32, seed=23)[1],
          fresh("td3", (64, 96, 48), 89, 14, seed=24), fresh("sac", (1,), 17, 5, seed=25)]
    max_rows = [8, 8, 8, 8, 3]
    on = GroupActor(ts, max_rows=max_rows, general="device", general_sessions=True)
    off = GroupActor(ts, max_rows=max_rows, general="device", general_sessions=False)
    assert on.general_sessions and not off.general_sessions
    assert [s.entry for s in on._sessions] == ["sac_actor", "sac_gactor"] and [s.entry for s in off._sessions] == ["sac_actor"]
    assert all(o.dtype == np.float64 and not o.flags["OWNDATA"] for o in on.obs)
    rs = np.random.RandomState(8)

    def both(rows, det):
        data = [draws64(rs, m, t.obs_dim, t.act_dim) for t, m in zip(ts, max_rows)]
        for g in (on, off):
            for i, (o, e) in enumerate(data):
                g.obs[i][...], g.eps[i][...] = o, e
                g.act[i][...] = SENTINEL
            g.act(rows, det)
        for i, (t, n) in enumerate(zip(ts, rows)):
            assert np.array_equal(bits(on.act[i]), bits(off.act[i])), (rows, i)
            assert np.all(on.act[i][n:] == SENTINEL), (rows, i)
            if n and runs_general_step(t):
                d = det if isinstance(det, bool) else det[i]
                assert np.array_equal(bits(on.act[i][:n]), bits(solo(t, data[i][0][:n], d, data[i][1][:n]))), (rows, i)

    both([5, 4, 3, 6, 2], False)
    both([8, 0, 0, 8, 3], [False, True, False, True, False])
    both([0, 1, 0, 0, 0], True)
    # a general member trains at a new batch size between two ticks: its handle is replaced, the sessions are reopened
    t = ts[1]
    gen0, before = t._handle_gen, np.array(on.act[1])
    t.train_loop(filled_buffer(1500, 42, 7, 3), 3, batch_size=64)
    assert t._handle_gen != gen0
    staged = on.obs[3].copy()
    both([0, 1, 0, 0, 0], True)
    both([5, 4, 3, 6, 2], False)
    assert not np.array_equal(before[:1], on.act[1][:1]) and staged.shape == on.obs[3].shape
    on.close()
    off.close()
    with pytest.raises(RuntimeError, match="closed"):
        on.act([1, 1, 1, 1, 1], True)


# ---- drivers ------------------------------------------------------------------------------------------------------------
def test_experiment_group_with_general_sessions_writes_the_rows_and_state_of_without(tmp_path):
    """Progress rows, and through the group checkpoint of the last epoch every member's networks, optimizer state,
    buffer contents (chunk checksums), buffer generator and host generators."""
    from robosuite_benchmark_amd.driver import experiment_group
    from robosuite_benchmark_amd.group_checkpoint import read_manifest
    from tests.test_gpu_device_acting import assert_rows, small_variant
    v = small_variant("Lift-Panda-OSC-POSE-SEED17", (512, 512), batch=100)
    seeds = [17, 18, 19]
    out = {}
    for flag in (True, False):
        ck = str(tmp_path / f"ck{int(flag)}")
        rows = experiment_group(copy.deepcopy(v), seeds=seeds, num_epochs=2, quiet=True, acting="device_all",
                                general_sessions=flag, checkpoint_dir=ck)
        out[flag] = (rows, read_manifest(ck))
    for s in seeds:
        assert_rows(out[True][0][s], out[False][0][s], s)
    assert out[True][1]["members"] == out[False][1]["members"] and len(out[True][1]["members"]) == 3
    default = experiment_group(copy.deepcopy(v), seeds=seeds, num_epochs=2, quiet=True, acting="device_all")
    for s in seeds:
        assert_rows(default[s], out[False][0][s], ("default", s))
