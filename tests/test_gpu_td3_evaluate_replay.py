"""GPU: the TD3 objectives on replay-buffer rows in place -- td3_evaluate_replay_many / td3_evaluate_replay_general_many
(k_eval_rows, csrc/sac_eval_rows.h, unchanged, in front of k_eval_td3 or the first k_eval_layer_td3),
TD3Trainer.evaluate_td3_replay and group.td3_evaluate_replay_many.

There is NO tolerance anywhere.  The reference of every case is the path that existed before, on the same trainer:
evaluate_td3(buffer.gather(idx), eps=the same draw, rows=True, general=..., stats=...).  The nine columns are compared as
uint32, the statistics dicts for equality, the moment records of stats="device" byte for byte.  The buffers hold non-zero
rewards, some terminals == 1 and next_observations distinct from the observations, so a wrong or swapped source array
changes y, tq* or q*."""
import ctypes as C

import numpy as np
import pytest

from robosuite_benchmark_amd import ArchTD3TrainerGroup, EnvReplayBuffer, _lib
from robosuite_benchmark_amd.group import runs_general_step, td3_evaluate_replay_many
from tests.helpers import full_state, make_pair, make_td3_pair, synth_transitions
from tests.td3_eval_reference import ARRAY_COLUMNS, COLUMNS, ROW_COLUMNS, make_td3_trainer

pytestmark = pytest.mark.gpu
ROWS = (1, 15, 16, 17, 1024)                    # around k_eval_rows' 16-row block; one full call
WIDTHS = (1, 63, 64, 65)                        # observation widths around the 64 lanes that walk a row
ENTRY = {False: "td3_evaluate_replay_many", True: "td3_evaluate_replay_general_many"}
OLD_STATS_ENTRY = {False: "td3_evaluate_stats_many", True: "td3_evaluate_general_stats_many"}
FAMILIES = [((32, 16), "host"), ((24, 16, 8), "device")]
FAMILY_IDS = ["fused", "general"]


def make(O, A, hidden=(32, 16), hidden_q=None, seed=5, **kw):
    if hidden_q is None:
        return make_td3_pair(O, A, 32, seed=seed, hidden=tuple(hidden), **kw)[1]
    return make_td3_trainer(O, A, hidden, hidden_q, seed=seed, batch_size=32, policy_learning_rate=1e-3, qf_learning_rate=5e-4,
                            **kw)


def buffer_of(capacity, adds, O, A, seed=3, private=True):
    """A buffer of `capacity` rows after `adds` inserted rows, in two blocks (adds > capacity: wrapped, top in the middle)."""
    obs, act, rew, term, nobs = synth_transitions(adds, O, A, seed=seed, term_frac=0.2)
    assert np.all(rew != 0) and term.any() and not term.all()
    buf = EnvReplayBuffer(capacity, obs_dim=O, action_dim=A)
    cut = (2 * adds) // 3
    for lo, hi in ((0, cut), (cut, adds)):
        buf.add_block(obs[lo:hi], act[lo:hi], rew[lo:hi], nobs[lo:hi], term[lo:hi])
    if private:
        buf.seed(seed)
    return buf


def eps_of(n, A, seed):
    return np.random.RandomState(seed + 7).standard_normal((n, A)).astype(np.float32)


def bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same_columns(got, want):
    return all(bits(got[k], want[k]) for k in COLUMNS)


def check_against_gather(t, buf, idx, eps, where, **kw):
    """evaluate_td3_replay(indices=idx) against evaluate_td3 on the gathered batch, under both values of stats: the columns
    as uint32, the statistics equal."""
    idx = np.asarray(idx, np.int64)
    for stats in ("host", "device"):
        got, cols = t.evaluate_td3_replay(buf, indices=idx, eps=eps, rows=True, stats=stats, **kw)
        want_stats, want = t.evaluate_td3(buf.gather(idx), eps=eps, rows=True, stats=stats, **kw)
        assert same_columns(cols, want), (where, stats)
        assert got == want_stats, (where, stats)
        assert np.array_equal(cols["indices"], idx) and list(cols.keys()) == list(want.keys()) + ["indices"], where
        assert t.evaluate_td3_replay(buf, indices=idx, eps=eps, stats=stats, **kw) == want_stats, (where, stats)
    return cols


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def replay_io(t, n, eps, fill=7.0, rows=True):
    """(td3_eval_io_t with null input arrays, outputs pre-filled with a sentinel, arrays kept alive)."""
    keep = [_lib.f32(eps)]
    out = dict(rows=np.full((len(ROW_COLUMNS), n), fill, np.float32))
    out.update((k, np.full((n, t.act_dim), fill, np.float32)) for k in ARRAY_COLUMNS)
    io = _lib.Td3EvalIO(None, None, None, None, None, keep[0].ctypes.data, out["rows"].ctypes.data if rows else None,
                        *[out[k].ctypes.data for k in ARRAY_COLUMNS])
    return io, out, keep


def replay_c(general, ts, bufs, idxs, ios, stats=False, n_rows=None):
    """The replay entry of one family through the C ABI: (rc, stats array or None)."""
    R = len(ts)
    idxs = [None if i is None else np.ascontiguousarray(i, np.int64) for i in idxs]
    srcs = (_lib.SacEvalSrc * R)(*[_lib.SacEvalSrc(None if b is None else b._h.value, None if i is None else i.ctypes.data)
                                   for b, i in zip(bufs, idxs)])
    arr = (_lib.Td3EvalIO * R)(*ios)
    sts = (_lib.Td3EvalStats * R)() if stats else None
    n_rows = [0 if i is None else len(i) for i in idxs] if n_rows is None else n_rows
    rc = getattr(_lib.load(), ENTRY[general])((C.c_void_p * R)(*[t._h.value for t in ts]), R, (C.c_int32 * R)(*n_rows),
                                              srcs, arr, sts)
    return rc, sts


def old_stats_c(general, t, buf, idx, eps):
    """The *_stats_many entry on the gathered batch: (outputs, the member's td3_eval_stats_t as bytes)."""
    b = buf.gather(idx)
    keep = [_lib.f32(b["observations"]), _lib.f32(b["actions"]), _lib.f32(b["rewards"].reshape(-1)),
            _lib.f32(b["terminals"].reshape(-1)), _lib.f32(b["next_observations"]), _lib.f32(eps)]
    out = dict(rows=np.full((len(ROW_COLUMNS), len(idx)), 7.0, np.float32))
    out.update((k, np.full((len(idx), t.act_dim), 7.0, np.float32)) for k in ARRAY_COLUMNS)
    io = _lib.Td3EvalIO(*[x.ctypes.data for x in keep], out["rows"].ctypes.data, *[out[k].ctypes.data for k in ARRAY_COLUMNS])
    arr, sts = (_lib.Td3EvalIO * 1)(io), (_lib.Td3EvalStats * 1)()
    _lib.check(getattr(_lib.load(), OLD_STATS_ENTRY[general])((C.c_void_p * 1)(t._h.value), 1, (C.c_int32 * 1)(len(idx)),
                                                              arr, sts), OLD_STATS_ENTRY[general])
    return out, bytes(sts[0])


# ---- 1. every width, every row count, both buffer sizes ----------------------------------------------------------------------
@pytest.mark.parametrize("hidden,general", FAMILIES, ids=FAMILY_IDS)
@pytest.mark.parametrize("O", WIDTHS)
def test_columns_statistics_and_records_equal_the_gathered_batch(O, hidden, general):
    A = 3
    t = make(O, A, hidden)
    g = runs_general_step(t)
    assert g == (general == "device")
    for size in (64, 65):
        buf = buffer_of(100, size, O, A, seed=size)
        assert buf.num_steps_can_sample() == size
        rs = np.random.RandomState(O + size)
        for n in ROWS:
            idx = rs.randint(0, size, n)
            idx[0], idx[-1] = size - 1, 0                             # the ends of the storage (one row: row 0)
            if n > 2:
                idx[1] = idx[0]                                       # a repeat
            cols = check_against_gather(t, buf, idx, eps_of(n, A, n), (O, size, n), general=general)
            assert cols["q1"].shape == (n,) and cols["a_smooth"].shape == (n, A)
            if size == 65 and n in (1, 17, 1024):                     # the records of the C entry, byte for byte
                eps = eps_of(n, A, n)
                want_out, want_bytes = old_stats_c(g, t, buf, idx, eps)
                io, out, _keep = replay_io(t, n, eps)
                rc, sts = replay_c(g, [t], [buf], [idx], [io], stats=True)
                assert rc == 0, _lib.last_error()
                assert bytes(sts[0]) == want_bytes and all(bits(out[k], want_out[k]) for k in out), n
                io2, out2, _keep2 = replay_io(t, n, eps, rows=False)  # rows may be NULL with stats: no column comes back
                io2.a_pi = io2.a_target = io2.a_smooth = None
                rc, sts2 = replay_c(g, [t], [buf], [idx], [io2], stats=True)
                assert rc == 0 and bytes(sts2[0]) == want_bytes and np.all(out2["rows"] == 7.0) and np.all(out2["a_pi"] == 7.0)


@pytest.mark.parametrize("hidden,hidden_q,general", [((256, 256), None, "host"), ((512, 512), None, "device"),
                                                     ((24, 16, 8), (32,), "device"), ((512, 512), None, "host")],
                         ids=["256x256", "512x512", "policy deeper than critics", "general step on the host"])
def test_a_wide_first_layer_and_windows_above_1024_rows(hidden, hidden_q, general):
    O, A = 379, 6
    t = make(O, A, hidden, hidden_q)
    buf = buffer_of(400, 300, O, A)
    rs = np.random.RandomState(A)
    for n in (17, 2500) if general == "device" or not runs_general_step(t) else (17,):
        check_against_gather(t, buf, rs.randint(0, 300, n), eps_of(n, A, n), (hidden, n), general=general)


@pytest.mark.parametrize("hidden,general", FAMILIES, ids=FAMILY_IDS)
def test_behind_twenty_steps_and_a_wrapped_buffer(hidden, general):
    O, A = 5, 3
    t = make(O, A, hidden)
    buf = buffer_of(64, 100, O, A)                                    # wrapped: top in the middle
    assert buf.num_steps_can_sample() == 64
    idx = np.random.RandomState(1).permutation(64)
    first = check_against_gather(t, buf, idx, eps_of(64, A, 2), "fresh", general=general)
    t.train_loop(buf, 20, batch_size=32)
    stepped = check_against_gather(t, buf, idx, eps_of(64, A, 2), "20 steps", general=general)
    assert not bits(stepped["q1"], first["q1"]) and not bits(stepped["a_target"], first["a_target"])


# ---- 2. ordering behind the asynchronous ingest -----------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,general", [((256, 256), "host"), ((512, 512), "device")], ids=FAMILY_IDS)
def test_rows_just_added_are_read_behind_their_copies(hidden, general):
    O, A, n = 379, 6, 6000
    t = make(O, A, hidden)
    buf = EnvReplayBuffer(2 * n, obs_dim=O, action_dim=A)
    buf.seed(1)
    seen = []
    for k in range(2):
        obs, act, rew, term, nobs = synth_transitions(n, O, A, seed=20 + k, term_frac=0.2)
        path = dict(observations=obs, actions=act, rewards=rew, next_observations=nobs, terminals=term)
        idx = np.arange(k * n + n - 700, k * n + n)                  # the tail of the block whose copies were just enqueued
        eps = eps_of(len(idx), A, k)
        buf.add_paths([path])
        seen.append((idx, eps, t.evaluate_td3_replay(buf, indices=idx, eps=eps, rows=True, general=general)))      # (no ingest_wait)
    for idx, eps, (stats, cols) in seen:
        want_stats, want = t.evaluate_td3(buf.gather(idx), eps=eps, rows=True, general=general)
        assert same_columns(cols, want) and stats == want_stats


# ---- 3. grouping ------------------------------------------------------------------------------------------------------------
def test_two_families_and_a_shared_buffer_in_one_python_call():
    O, A = 5, 3
    ts = [make(O, A, (32, 16) if i < 3 else (24, 16, 8), seed=40 + i) for i in range(5)]
    assert [runs_general_step(t) for t in ts] == [False] * 3 + [True] * 2
    shared = buffer_of(100, 65, O, A, seed=9)
    bufs = [shared, shared, buffer_of(100, 64, O, A, seed=51), shared, buffer_of(100, 64, O, A, seed=52)]
    counts = [17, 0, 1024, 16, 33]                                    # member 1 sits out
    rs = np.random.RandomState(4)
    idxs = [None if n == 0 else rs.randint(0, 64, n) for n in counts]
    epss = [None if n == 0 else eps_of(n, A, i) for i, n in enumerate(counts)]
    group = ArchTD3TrainerGroup.__new__(ArchTD3TrainerGroup)
    group.trainers = ts
    for stats in ("host", "device"):
        got = td3_evaluate_replay_many(ts, bufs, indices=idxs, eps=epss, rows=True, general="device", stats=stats)
        assert got[1] is None
        for i, t in enumerate(ts):
            if counts[i]:
                solo = t.evaluate_td3_replay(bufs[i], indices=idxs[i], eps=epss[i], rows=True, general="device", stats=stats)
                want = t.evaluate_td3(bufs[i].gather(idxs[i]), eps=epss[i], rows=True, general="device", stats=stats)
                assert same_columns(got[i][1], solo[1]) and got[i][0] == solo[0], (i, stats)
                assert same_columns(got[i][1], want[1]) and got[i][0] == want[0], (i, stats)
                assert np.array_equal(got[i][1]["indices"], idxs[i])
        again = group.td3_evaluate_replay_many(bufs, indices=idxs, eps=epss, general="device", stats=stats)
        assert again == [None if g is None else g[0] for g in got]
    # the C entry: two members on ONE buffer in one call, the member that sits out untouched, records byte for byte
    ios = [replay_io(t, max(n, 1), e if e is not None else eps_of(1, A, 0)) for t, n, e in zip(ts[:3], counts, epss)]
    rc, sts = replay_c(False, ts[:3], [shared] * 3, [idxs[0], None, idxs[2]], [x[0] for x in ios], stats=True)
    assert rc == 0, _lib.last_error()
    assert np.all(ios[1][1]["rows"] == 7.0) and not any(bytes(sts[1]))
    for i in (0, 2):
        want_out, want_bytes = old_stats_c(False, ts[i], shared, idxs[i], epss[i])
        assert bytes(sts[i]) == want_bytes and all(bits(ios[i][1][k], want_out[k]) for k in want_out), i
    # n instead of indices: each member draws from its own rng, the indices in front of the single draw
    got = td3_evaluate_replay_many(ts[:3], bufs[:3], n=[12, 0, 5], rngs=[np.random.RandomState(i) for i in range(3)], rows=True)
    assert got[1] is None
    for i in (0, 2):
        r = np.random.RandomState(i)
        n = (12, 0, 5)[i]
        idx = r.randint(0, bufs[i].num_steps_can_sample(), n)
        want = ts[i].evaluate_td3(bufs[i].gather(idx), eps=r.standard_normal((n, A)), rows=True)
        assert np.array_equal(got[i][1]["indices"], idx) and same_columns(got[i][1], want[1]) and got[i][0] == want[0]


# ---- 4. nothing moves -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,general", FAMILIES, ids=FAMILY_IDS)
def test_training_continues_bit_for_bit(hidden, general):
    O, A = 11, 3

    def run(interleave):
        np.random.seed(77)
        t = make(O, A, hidden, noise_seed=3)
        buf = buffer_of(800, 600, O, A, private=False)                # bound to np.random, as the drivers' buffers
        rs = np.random.RandomState(5)
        seen = []

        def look():
            if interleave:
                idx = rs.randint(0, 600, 40)
                before, ahead = buf.rng_state(), np.random.get_state()
                for stats in ("host", "device"):
                    a = t.evaluate_td3_replay(buf, indices=idx, eps=eps_of(40, A, 1), rows=True, general=general, stats=stats)
                    b = t.evaluate_td3_replay(buf, indices=idx, eps=eps_of(40, A, 1), rows=True, general=general, stats=stats)
                    assert same_columns(a[1], b[1]) and a[0] == b[0]          # a second call: the same bits
                    seen.append(a)
                t.evaluate_td3_replay(buf, n=25, general=general)             # (the private stream: not np.random)
                after, behind = buf.rng_state(), np.random.get_state()
                assert np.array_equal(before[0], after[0]) and before[1] == after[1]
                assert np.array_equal(ahead[1], behind[1]) and ahead[2:] == behind[2:]

        look()
        for k in range(12):                                               # stepwise: the read-ahead is in flight
            t.train(buf.random_batch(32))
            if k % 5 == 2:
                look()
        for k in range(2):                                                # loop calls: the speculative first chunk
            t.train_loop(buf, 12, batch_size=32)
            look()
        for _ in range(3):
            t.train(buf.random_batch(32))
        state = full_state(t, buf) + [t.state_dict()["params"]["target_policy"]]
        st = np.random.get_state()
        return state + [np.asarray(st[1]), np.asarray([st[2]])], len(seen)

    plain, n0 = run(False)                                                # the twin that never evaluated
    mixed, n1 = run(True)
    assert n0 == 0 and n1 >= 10 and len(plain) == len(mixed)
    for x, y in zip(plain, mixed):
        assert np.array_equal(x, y)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
# (Not tested here: the refusal of a buffer that lives on another device than its trainer.  It needs two GPUs and this
# suite runs on one; the check stands next to the dims check in eval_rows_admit_src, in front of anything that changes.)
def test_refusals_write_nothing():
    O, A, n = 5, 3, 8
    a, gen = make(O, A, (32, 16), seed=1), make(O, A, (24, 16, 8), seed=2)
    sac, sacg = make_pair(O, A, 32, seed=3, hidden=(32, 16))[1], make_pair(O, A, 32, seed=3, hidden=(24, 16, 8))[1]
    buf, other, empty = buffer_of(100, 60, O, A), buffer_of(100, 60, O + 1, A), EnvReplayBuffer(50, obs_dim=O, action_dim=A)
    wide = buffer_of(100, 60, O, A + 1)
    idx, eps = np.arange(n, dtype=np.int64), eps_of(n, A, 1)
    state, rng = full_state(a, buf), buf.rng_state()
    want = a.evaluate_td3(buf.gather(idx), eps=eps, rows=True)[1]

    def refused(general, ts, bufs, idxs, message, n_rows=None, drop=None):
        made = [replay_io(t, n, eps) for t in ts]
        if drop:
            setattr(made[-1][0], drop, None)
        for stats in (False, True):
            rc, sts = replay_c(general, ts, bufs, idxs, [m[0] for m in made], stats=stats, n_rows=n_rows)
            assert rc < 0 and message in _lib.last_error(), (message, _lib.last_error())
            assert all(np.all(v == 7.0) for m in made for v in m[1].values()), message
            assert not stats or not any(bytes(sts[0])), message

    size = buf.num_steps_can_sample()
    bad = idx.copy(); bad[5] = size
    refused(False, [a], [buf], [bad], f"trainer 0: index {size} (row 5) out of range [0, {size})")
    bad = idx.copy(); bad[n - 1] = -1
    refused(False, [a], [buf], [bad], "trainer 0: index -1")
    refused(True, [gen], [buf], [bad], "trainer 0: index -1")
    refused(False, [a], [buf], [None], "trainer 0: a null replay buffer or null indices", n_rows=[n])
    refused(False, [a], [None], [idx], "trainer 0: a null replay buffer or null indices")
    refused(False, [a], [other], [idx], f"trainer 0: its replay buffer has dims ({O + 1}, {A}), the trainer ({O}, {A})")
    refused(False, [a], [wide], [idx], "its replay buffer has dims")
    refused(True, [gen], [other], [idx], "its replay buffer has dims")
    refused(False, [a], [empty], [idx], "trainer 0: its replay buffer is empty")
    refused(True, [gen], [empty], [idx], "trainer 0: its replay buffer is empty")
    refused(False, [a], [buf], [idx], "null eps", drop="eps")
    refused(False, [gen], [buf], [idx], "td3_evaluate_replay_general_many is the entry")        # the wrong family
    refused(True, [a], [buf], [idx], "td3_evaluate_replay_many is its entry")
    refused(False, [sac], [buf], [idx], "is a SAC trainer: this entry evaluates the TD3 objective")
    refused(True, [sacg], [buf], [idx], "is a SAC trainer: this entry evaluates the TD3 objective")
    refused(False, [a, a], [buf, buf], [idx, idx], "again")
    refused(False, [a], [buf], [idx], "rows", n_rows=[1025])
    refused(False, [a], [buf], [idx], "no trainer has rows", n_rows=[0])
    # the second member's fault: nothing of the first is written either
    other_a = make(O, A, (32, 16), seed=4)
    bad = idx.copy(); bad[0] = 60
    refused(False, [a, other_a], [buf, buf], [idx, bad], "trainer 1: index 60 (row 0)")
    # rows is needed without stats, and only then
    io, out, _keep = replay_io(a, n, eps, rows=False)
    rc, _ = replay_c(False, [a], [buf], [idx], [io])
    assert rc < 0 and "rows" in _lib.last_error() and np.all(out["a_pi"] == 7.0)
    # nothing moved, and a valid call still gives the right values
    for x, y in zip(full_state(a, buf), state):
        assert np.array_equal(x, y)
    assert np.array_equal(buf.rng_state()[0], rng[0]) and buf.rng_state()[1] == rng[1]
    m1 = replay_io(a, n, eps)
    rc, _ = replay_c(False, [a], [buf], [idx], [m1[0]])
    assert rc == 0, _lib.last_error()
    assert all(bits(m1[1]["rows"][k], want[name]) for k, name in enumerate(ROW_COLUMNS))
    assert all(bits(m1[1][name], want[name]) for name in ARRAY_COLUMNS)
    # Python: a SAC member, bad indices, and the two methods that keep raising
    with pytest.raises(RuntimeError, match="evaluate_replay_many evaluates the SAC objective"):
        td3_evaluate_replay_many([a, sac], [buf, buf], n=4)
    with pytest.raises(RuntimeError, match="out of range"):
        a.evaluate_td3_replay(buf, indices=[0, 60])
    with pytest.raises(NotImplementedError, match="SAC objective"):
        a.evaluate_replay(buf, n=4)
