"""GPU: the replay path at its edges, bit for bit (tables and constructions: tests/replay_edges.py, proved on the CPU by
tests/test_replay_edges_host.py).  Indices against np.random.RandomState -- values, all 624 state words and the position
after every draw; gathered rows against the float64 HostReplayBuffer; the feature-major copy saT through steps on device
batches against steps on host batches of the same rows (the host builds its own saT); the ingest against the host ring and
ndarray.astype(np.float32).  Every comparison is equality; float arrays are compared as uint32."""
import numpy as np
import pytest

from oracle.sac_step_torch import HostReplayBuffer, init_sac_params
from tests import replay_edges as RE
from tests.helpers import flat_of, synth_transitions

pytestmark = pytest.mark.gpu
KEYS = ("observations", "actions", "rewards", "terminals", "next_observations")


# ---- the index stream -----------------------------------------------------------------------------------------------------
def index_buffer(size, bound, capacity=None):
    """A buffer that is only drawn from: one-float rows, its size set through the ring cursor (no row is ever read)."""
    from robosuite_benchmark_amd import EnvReplayBuffer
    buf = EnvReplayBuffer(capacity or size, obs_dim=1, action_dim=1, numpy_global_stream=bound)
    assert buf._bound == bound
    buf.set_cursor(0, size)
    assert buf.num_steps_can_sample() == size
    return buf


class Stream:
    """A buffer's generator next to the reference's.  Private: the buffer owns a copy of `state`.  Bound: the buffer draws
    from np.random itself, and np.random's own state is compared after every draw as well."""

    def __init__(self, buf, bound):
        self.buf, self.bound, self.ref = buf, bound, np.random.RandomState(0)

    def start(self, state):
        self.ref.set_state(state)
        if self.bound:
            np.random.set_state(state)
        else:
            self.buf.set_rng_state(state[1], state[2])

    def check_state(self, where):
        want = self.ref.get_state()
        key, pos = self.buf.rng_state()
        assert pos == want[2], (where, "position", pos, want[2])
        assert np.array_equal(key, want[1]), (where, "state words", int((key != want[1]).sum()))
        if self.bound:
            assert RE.same_state(np.random.get_state(), want), (where, "np.random", np.random.get_state()[2], want[2])

    def draw(self, size, batch, n_batches=1, where=""):
        want = np.stack([self.ref.randint(0, size, batch) for _ in range(n_batches)])
        got = self.buf.sample_indices(batch, n_batches)
        assert got.dtype == np.int64 and got.shape == want.shape, where
        bad = got != want
        assert not bad.any(), (where, f"{int(bad.sum())} of {bad.size} indices differ, first at {np.argwhere(bad)[0].tolist()}")
        self.check_state(where)


@pytest.mark.parametrize("bound", [False, True], ids=["private", "np.random"])
@pytest.mark.parametrize("size", RE.SIZES, ids=RE.size_id)
def test_every_size_draws_numpys_indices_and_leaves_numpys_state(size, bound):
    s = Stream(index_buffer(size, bound), bound)
    for seed in RE.SEEDS:
        s.start(np.random.RandomState(seed).get_state())
        for B in RE.BATCHES:
            s.draw(size, B, where=(size, seed, B))
            s.draw(size, 2000, where=(size, seed, B, "the next 2000"))


@pytest.mark.parametrize("bound", [False, True], ids=["private", "np.random"])
@pytest.mark.parametrize("pos", RE.POSITIONS)
def test_every_start_position_ends_on_the_last_word_and_on_word_zero(pos, bound):
    for size in RE.POSITION_SIZES:
        s = Stream(index_buffer(size, bound), bound)
        for seed in RE.SEEDS:
            st = RE.start_state(seed, pos)
            if size & (size - 1) == 0:
                counts = {RE.MT_N - 1: RE.count_to_last_word(pos), 0: RE.count_to_last_word(pos) + 1}
            else:
                counts = {w: RE.count_ending_on_word(st, size, w) for w in (RE.MT_N - 1, 0)}
            for word, n in counts.items():
                s.start(st)
                s.draw(size, n, where=(size, seed, pos, "last draw on word", word))
                assert s.buf.rng_state()[1] == word + 1              # 624 stays 624: the twist is lazy on both sides
                s.draw(size, 1, where=(size, seed, pos, "one more"))
                s.draw(size, 2000, where=(size, seed, pos, "the next 2000"))


@pytest.mark.parametrize("B", RE.PADDED_BATCHES)
def test_many_padded_batches_in_one_launch(B):
    size = RE.POSITION_SIZES[1]
    s = Stream(index_buffer(size, False), False)
    s.start(np.random.RandomState(59).get_state())
    s.draw(size, B, RE.PADDED_N, where=(B, RE.PADDED_N))             # hundreds of twists (B >= 15), batches at a stride of bp
    s.draw(size, B, 3, where=(B, "again"))
    s.draw(size, 2000, where=(B, "the next 2000"))


@pytest.mark.parametrize("bound", [False, True], ids=["private", "np.random"])
def test_a_size_that_changes_between_draws(bound):
    from robosuite_benchmark_amd import EnvReplayBuffer
    buf = EnvReplayBuffer(2048, obs_dim=1, action_dim=1, numpy_global_stream=bound)
    s = Stream(buf, bound)
    s.start(np.random.RandomState(83).get_state())
    size = 0
    for want in RE.GROWING_SIZES:
        n = want - size
        z = np.zeros((n, 1), np.float32)
        buf.add_block(z, z, z, z, np.zeros(n, np.uint8))
        size = want
        assert buf.num_steps_can_sample() == size
        before = buf.rng_state()
        for B in (16, 17, 256):
            s.draw(size, B, where=("size", size, B))
        s.draw(size, 5, 7, where=("size", size, "5 x 7"))
        if size == 1:                                                # NumPy consumes nothing for one row: all zeros
            assert RE.same_state(before, buf.rng_state())


# ---- the grouped draw -----------------------------------------------------------------------------------------------------
def sac_trainer(O, A, B, seed, hidden=(256, 256), noise_seed=7, **kw):
    from robosuite_benchmark_amd import FlattenMlp, SACTrainer, TanhGaussianPolicy
    nets = init_sac_params(O, A, hidden=hidden, seed=seed)
    pol = TanhGaussianPolicy(list(hidden), O, A)
    qs = [FlattenMlp(list(hidden), 1, O + A) for _ in range(4)]
    pol.load_flat(flat_of(nets["policy"]))
    for q, name in zip(qs, ("qf1", "qf2", "target_qf1", "target_qf2")):
        q.load_flat(flat_of(nets[name]))
    return SACTrainer(policy=pol, qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], batch_size=B,
                      noise_seed=noise_seed, policy_lr=1e-3, qf_lr=5e-4, soft_target_tau=0.005, target_update_period=1, **kw)


def assert_same_training(a, b, where):
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa["params"]:
        assert np.array_equal(sa["params"][k], sb["params"][k]), (where, k)
    for k in sa["opt"]:
        for j, q in enumerate(("exp_avg", "exp_avg_sq")):
            assert np.array_equal(sa["opt"][k][j], sb["opt"][k][j]), (where, k, q)
    assert np.array_equal(sa["scalars"], sb["scalars"]), (where, sa["scalars"], sb["scalars"])


def test_grouped_draw_with_a_one_row_member():
    from robosuite_benchmark_amd import EnvReplayBuffer, MixedSACTrainerGroup
    members = [(5, 2, 1, 16), (11, 3, 1024, 17), (17, 4, 1025, 100), (10, 1, 3300, 256)]       # (O, A, rows, batch)
    steps = 25

    def make(i, O, A, rows, B):
        obs, act, rew, term, nobs = synth_transitions(rows, O, A, seed=40 + i, term_frac=0.1)
        buf = EnvReplayBuffer(4096, obs_dim=O, action_dim=A)
        buf.add_block(obs, act, rew, nobs, term)
        buf.seed(70 + i)
        return sac_trainer(O, A, B, 3 + i, noise_seed=100 + i), buf

    group_side = [make(i, *m) for i, m in enumerate(members)]
    solo_side = [make(i, *m) for i, m in enumerate(members)]
    group = MixedSACTrainerGroup([t for t, _ in group_side])
    group.train_loop([b for _, b in group_side], steps, batch_sizes=[m[3] for m in members])
    for i, ((O, A, rows, B), (t, buf), (ts, bs)) in enumerate(zip(members, group_side, solo_side)):
        ref = np.random.RandomState(70 + i)
        start = ref.get_state()
        for _ in range(steps):
            ref.randint(0, rows, B)
        key, pos = buf.rng_state()
        assert RE.same_state((key, pos), ref.get_state()), (i, rows, B, pos, ref.get_state()[2])
        if rows == 1:
            assert RE.same_state((key, pos), start)
        ts.train_loop(bs, steps, batch_size=B)
        assert_same_training(t, ts, ("member", i))
        assert RE.same_state(bs.rng_state(), (key, pos))


# ---- the gather -----------------------------------------------------------------------------------------------------------
_coded = {}


def coded_pair(O, A, n=RE.GATHER_ROWS):
    """(host buffer, device buffer, private-stream seed) holding the same coded rows; built once per width."""
    from robosuite_benchmark_amd import EnvReplayBuffer
    if (O, A, n) not in _coded:
        _coded.clear()                                               # (one width at a time: the wide ones are 8 MB apiece)
        obs, act, rew, nobs, term = RE.coded_transitions(n, O, A)
        host = HostReplayBuffer(n, O, A)
        host.fill_block(obs, act, rew, term, nobs)
        dev = EnvReplayBuffer(n, obs_dim=O, action_dim=A, numpy_global_stream=False)
        dev.add_block(obs, act, rew, nobs, term)                     # float64 ingest
        _coded[(O, A, n)] = (host, dev)
    return _coded[(O, A, n)]


def host_rows(host, idx):
    return dict(observations=host._obs[idx], actions=host._act[idx], rewards=host._rew[idx], terminals=host._term[idx],
                next_observations=host._next_obs[idx])


def assert_rows(where, got, host, idx):
    want = host_rows(host, idx)
    for k in KEYS:
        RE.assert_bits(f"{where}: {k}", got[k], RE.to_f32(want[k]))


@pytest.mark.parametrize("O,A", RE.GATHER_CASES, ids=lambda v: str(v))
def test_gather_and_random_batch_at_every_width(O, A):
    host, dev = coded_pair(O, A)
    n = RE.GATHER_ROWS
    for what, idx in RE.gather_index_sets(n).items():
        assert_rows((O, A, what), dev.gather(idx), host, idx)
    dev.seed(17)
    ref = np.random.RandomState(17)
    for B in (1, 16, 17, 48):
        got, gidx = dev.random_batch(B, return_indices=True)         # the host-batch entry: gather slots
        idx = ref.randint(0, n, B)
        assert np.array_equal(gidx, idx), (O, A, B)
        assert_rows((O, A, "random_batch", B), got, host, idx)
        lazy = dev.random_batch(B)                                   # the device-batch entry: the ring of slots
        idx = ref.randint(0, n, B)
        assert np.array_equal(lazy.indices(), idx), (O, A, B, "device batch")
        assert_rows((O, A, "device batch", B), lazy, host, idx)
    assert RE.same_state(dev.rng_state(), ref.get_state())


@pytest.mark.parametrize("O,A", RE.SWEEP_CASES, ids=lambda v: str(v))
def test_gather_of_one_two_and_three_trips_of_the_grid(O, A):
    """n slots of one 16-row block each: n blocks over 1024 persistent workgroups -- the first set of the ping-pong alone,
    its second set (blk + stride), the tail test on both sides of 2048, and a third trip.  Every slot is read back."""
    host, dev = coded_pair(O, A)
    rows, B = RE.GATHER_ROWS, RE.RB
    dev.seed(129)
    ref = np.random.RandomState(129)
    want32 = {k: RE.to_f32(v) for k, v in host_rows(host, np.arange(rows)).items()}
    for n in RE.SWEEP_SLOTS:
        dev.sample_gather_device(B, n)
        idx = ref.randint(0, rows, B * n).reshape(n, B)
        got = {k: [] for k in KEYS}
        gidx = np.empty((n, B), np.int64)
        for s in range(n):
            batch, gidx[s] = dev.read_slot(s, B)
            for k in KEYS:
                got[k].append(batch[k])
        bad = np.argwhere((gidx != idx).any(axis=1))
        assert bad.size == 0, (O, A, n, "indices of slots", bad.ravel()[:8].tolist())
        for k in KEYS:
            RE.assert_bits(f"O {O} A {A}, {n} slots: {k} [slot, row, column]", np.stack(got[k]), want32[k][idx])
    assert RE.same_state(dev.rng_state(), ref.get_state())


def test_a_row_wider_than_the_tile_is_refused_and_nothing_else_changes():
    from robosuite_benchmark_amd import EnvReplayBuffer
    A = 1
    O = RE.widest_obs(A) + 1
    assert not RE.gather_accepts(O, A)
    obs, act, rew, nobs, term = RE.coded_transitions(64, O, A)
    wide = EnvReplayBuffer(64, obs_dim=O, action_dim=A, numpy_global_stream=False)
    wide.add_block(obs, act, rew, nobs, term)
    idx = np.arange(16, dtype=np.int64)
    for call in (lambda: wide.gather(idx), lambda: wide.random_batch(16, lazy=False), lambda: wide.random_batch(16)["rewards"],
                 lambda: wide.sample_gather_device(16, 2)):
        with pytest.raises(RuntimeError, match="observation rows too wide for the gather"):
            call()
    # what needs no gather still works on that buffer: its rows and its index stream
    o, a, r, no, t = wide.read_rows(0, 64)
    RE.assert_bits("rows of the refused buffer", o, obs)
    wide.seed(5)
    assert np.array_equal(wide.sample_indices(16)[0], np.random.RandomState(5).randint(0, 64, 16))
    # and the widest sibling that fits is served
    host, dev = coded_pair(RE.widest_obs(A), A)
    idx = RE.gather_index_sets(RE.GATHER_ROWS)["ends and duplicates"]
    assert_rows("widest sibling", dev.gather(idx), host, idx)


# ---- saT through the step ---------------------------------------------------------------------------------------------------
STEP_ROWS = 600


def step_data(O, A):
    obs, act, rew, term, nobs = synth_transitions(STEP_ROWS, O, A, seed=O + A, term_frac=0.1)
    return dict(observations=obs, actions=act, rewards=rew, terminals=term.astype(np.float32), next_observations=nobs)


def step_buffer(data, O, A):
    from robosuite_benchmark_amd import EnvReplayBuffer
    buf = EnvReplayBuffer(STEP_ROWS, obs_dim=O, action_dim=A, numpy_global_stream=False)
    buf.add_block(data["observations"], data["actions"], data["rewards"], data["next_observations"], data["terminals"])
    return buf


def host_steps(data, O, A, B, hidden, ref, steps=2):
    """The reference side: steps on host dicts of the rows RandomState draws (the library builds saT from them on the host)."""
    t = sac_trainer(O, A, B, seed=O, hidden=hidden)
    for _ in range(steps):
        idx = ref.randint(0, STEP_ROWS, B)
        t.train({k: np.ascontiguousarray(v[idx]) for k, v in data.items()})
    return t


@pytest.mark.parametrize("O", RE.STEP_WIDTHS)
def test_steps_on_device_batches_equal_steps_on_host_batches(O):
    for A in RE.STEP_ACTS:
        data = step_data(O, A)
        buf = step_buffer(data, O, A)
        for hidden in RE.STEP_HIDDEN:
            for B in RE.STEP_BATCHES:
                buf.seed(B)
                ref = np.random.RandomState(B)
                dev = sac_trainer(O, A, B, seed=O, hidden=hidden)
                for _ in range(2):
                    batch = buf.random_batch(B)
                    assert batch.on_device
                    dev.train(batch)
                assert (dev.fused_mode() == 3) == (hidden == (32,)), (hidden, dev.fused_mode())
                assert_same_training(dev, host_steps(data, O, A, B, hidden, ref), (O, A, hidden, B))
                assert RE.same_state(buf.rng_state(), ref.get_state())


@pytest.mark.parametrize("entry", ["train_loop", "device batches"])
@pytest.mark.parametrize("hidden", RE.STEP_HIDDEN, ids=["fused", "general"])
def test_one_buffer_through_four_batch_sizes(hidden, entry):
    """48 -> 17 -> 33 -> 16 rows on ONE buffer, a fresh trainer each: every change of the batch size is another slot
    layout inside the same allocation (ensure_slots clears it; the stepwise ring is re-created), so rows of the old layout
    must not show through the pad rows and pad features of saT that the weight gradient contracts."""
    O, A = 61, 3
    data = step_data(O, A)
    buf = step_buffer(data, O, A)
    buf.seed(21)
    ref = np.random.RandomState(21)
    for B in RE.RELAYOUT_BATCHES:
        dev = sac_trainer(O, A, B, seed=O, hidden=hidden)
        if entry == "train_loop":
            dev.train_loop(buf, 2, batch_size=B)
        else:
            for _ in range(2):
                dev.train(buf.random_batch(B))
        assert_same_training(dev, host_steps(data, O, A, B, hidden, ref), (hidden, entry, B))
        assert RE.same_state(buf.rng_state(), ref.get_state()), (hidden, entry, B)


# ---- ingest -----------------------------------------------------------------------------------------------------------------
def test_ingest_at_the_staging_chunk_and_the_rings_end():
    from robosuite_benchmark_amd import EnvReplayBuffer
    cap, O, A, stride = RE.INGEST_CAPACITY, 5, 2, 8
    host = HostReplayBuffer(cap, O, A)
    dev = EnvReplayBuffer(cap, obs_dim=O, action_dim=A, numpy_global_stream=False)
    first = 0
    for j, (what, n) in enumerate(RE.ingest_blocks(cap)):
        obs, act, rew, nobs, term = RE.coded_transitions(n, O, A, first=first, stride=stride)
        first += n
        (host.fill_block if n <= cap else host.add_block)(obs, act, rew, term, nobs)
        if j % 2:                                                    # both entries: float32 rows and the float64 cast
            obs, act, rew, nobs = (RE.to_f32(x) for x in (obs, act, rew, nobs))
        dev.add_block(obs, act, rew, nobs, term)
        assert (dev.top(), dev.num_steps_can_sample(), dev.rows_written()) == (host._top, host._size, first), (what, n)
        m = host._size                                               # (rows beyond the fill level were never written)
        o, a, r, no, t = dev.read_rows(0, m)
        for name, got, want in (("obs", o, host._obs), ("act", a, host._act), ("rew", r, host._rew), ("next_obs", no, host._next_obs)):
            RE.assert_bits(f"after {n} rows ({what}): {name} [ring row, column]", got, RE.to_f32(want[:m]), stride)
        assert t.dtype == np.uint8 and np.array_equal(t, host._term[:m]), (what, n)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_ingest_cast_is_numpys(dtype):
    from robosuite_benchmark_amd import EnvReplayBuffer
    obs, act, rew, nobs, term = RE.cast_edge_block()
    n, O, A = len(obs), obs.shape[1], act.shape[1]
    dev = EnvReplayBuffer(n + 3, obs_dim=O, action_dim=A, numpy_global_stream=False)
    src = [x if dtype is np.float64 else RE.to_f32(x) for x in (obs, act, rew, nobs)]
    assert all(x.dtype == dtype for x in src)
    dev.add_block(src[0], src[1], src[2], src[3], term)
    o, a, r, no, t = dev.read_rows(0, n)
    for name, got, want in (("obs", o, obs), ("act", a, act), ("rew", r, rew), ("next_obs", no, nobs)):
        g, w = got.view(np.uint32), RE.to_f32(want).view(np.uint32)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (name, f"{len(bad)} cells; first {want[tuple(bad[0])]!r} -> {got[tuple(bad[0])]!r}, "
                                     f"NumPy {RE.to_f32(want)[tuple(bad[0])]!r}")
    assert np.array_equal(t, term)
