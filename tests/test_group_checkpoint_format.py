"""Group checkpoints without a GPU: the dirty-chunk range, incremental generations (only changed chunks are written),
kill safety, CRC checks across members and the group identity check -- on stand-ins with the trainer's and the replay
buffer's checkpoint surface (the buffer a NumPy ring with a rows-written counter)."""
import os

import numpy as np
import pytest

from robosuite_benchmark_amd import group_checkpoint as gc
from robosuite_benchmark_amd.group_checkpoint import GroupCheckpoint, GroupMismatchError, dirty_chunks

VARIANT = dict(algorithm="SAC", policy_kwargs=dict(hidden_sizes=[256, 256]), qf_kwargs=dict(hidden_sizes=[256, 256]),
               algorithm_kwargs=dict(num_epochs=10, batch_size=8), replay_buffer_size=10000)


# ---- the dirty range ----------------------------------------------------------------------------------------------
def test_no_previous_save_makes_every_chunk_dirty():
    assert dirty_chunks(10000, 4096, 9000, 9000, 9000, None) == [0, 1, 2]
    assert dirty_chunks(10000, 4096, 0, 0, 0, None) == []


def test_no_wrap():
    # 2 500 rows from row 5 000 on: rows 5000..7499 -> chunk 1 only
    assert dirty_chunks(100000, 4096, 7500, 7500, 7500, (5000, 5000, 5000)) == [1]
    # across a chunk boundary: rows 4000..6499 -> chunks 0, 1
    assert dirty_chunks(100000, 4096, 6500, 6500, 6500, (4000, 4000, 4000)) == [0, 1]
    # nothing written
    assert dirty_chunks(100000, 4096, 6500, 6500, 6500, (6500, 6500, 6500)) == []


def test_a_growing_last_chunk_is_dirty():
    # chunk 2 held rows 8192..8999 at the last save; 10 more rows land in it
    assert dirty_chunks(100000, 4096, 9010, 9010, 12345 + 10, (12345, 9000, 9000)) == [2]
    # one row that opens a new chunk: only that chunk
    assert dirty_chunks(100000, 4096, 8193, 8193, 8193, (8192, 8192, 8192)) == [2]


def test_a_wrap_across_the_end_of_the_ring():
    cap = 10000
    # full ring, top 9 000, 2 500 rows: slots 9000..9999 and 0..1499 -> last chunk (8192..9999) and chunk 0
    assert dirty_chunks(cap, 4096, cap, 1500, 50000 + 2500, (50000, 9000, cap)) == [0, 2]
    # filling up and wrapping in one go: size was 9 000, top 9 000
    assert dirty_chunks(cap, 4096, cap, 1500, 9000 + 2500, (9000, 9000, 9000)) == [0, 2]
    # ending exactly at the end of the ring: top back at 0
    assert dirty_chunks(cap, 4096, cap, 0, 9000 + 1000, (9000, 9000, 9000)) == [2]


def test_writes_of_the_capacity_or_more_make_every_chunk_dirty():
    cap = 10000
    assert dirty_chunks(cap, 4096, cap, 3000, 20000 + cap, (20000, 3000, cap)) == [0, 1, 2]
    assert dirty_chunks(cap, 4096, cap, 3001, 20000 + cap + 1, (20000, 3000, cap)) == [0, 1, 2]
    assert dirty_chunks(cap, 4096, cap, 3000, 20000 + cap - 1, (20000, 3001, cap)) == [0, 1, 2]   # cap - 1: all but one


def test_a_moved_cursor_makes_every_chunk_dirty():
    cap = 10000
    # 100 rows were written, but top is not 100 further on: somebody called set_cursor
    assert dirty_chunks(cap, 4096, 6000, 4000, 6100, (6000, 6000, 6000)) == [0, 1]
    # top where it should be, size not
    assert dirty_chunks(cap, 4096, 3000, 6100, 6100, (6000, 6000, 6000)) == [0]
    # nothing written but the cursor moved
    assert dirty_chunks(cap, 4096, 6000, 10, 6000, (6000, 6000, 6000)) == [0, 1]
    # a counter that went backwards (a foreign baseline)
    assert dirty_chunks(cap, 4096, 6000, 6000, 5000, (6000, 6000, 6000)) == [0, 1]


def test_chunk_rows_that_do_not_divide_the_capacity():
    cap = 1000
    # chunks of 300: [0,300) [300,600) [600,900) [900,1000); slots 950..999 and 0..49
    assert dirty_chunks(cap, 300, cap, 50, 5100, (5000, 950, cap)) == [0, 3]
    assert dirty_chunks(cap, 300, cap, 0, 5050, (5000, 950, cap)) == [3]
    assert dirty_chunks(cap, 300, 620, 620, 620, (590, 590, 590)) == [1, 2]


# ---- stand-ins ------------------------------------------------------------------------------------------------------
class StubTrainer:
    NETS = {"policy": 0, "qf1": 1, "qf2": 2, "target_qf1": 3, "target_qf2": 4}
    discount = reward_scale = policy_lr = qf_lr = soft_target_tau = 0.5
    target_update_period, use_automatic_entropy_tuning, target_entropy = 1, True, -2.0

    def __init__(self, fill, O=5, A=2, batch=8, noise_seed=0):
        self._h, self.obs_dim, self.act_dim, self._batch, self.noise_seed = object(), O, A, batch, noise_seed
        self._num_train_steps = 0
        self.created = []                    # (batch, noise_seed) of every handle built after construction
        self.fill(fill)

    def _create(self, batch):
        self.created.append((int(batch), self.noise_seed))
        self._h, self._batch = object(), int(batch)

    def fill(self, v):
        self.st = dict(params={k: np.full(32, v + i, np.float32) for i, k in enumerate(self.NETS)},
                       opt={k: (np.full(32, v, np.float32), np.full(32, -v, np.float32)) for k in ("policy", "qf1", "qf2")},
                       scalars=np.full(6, v, np.float64))
        self._num_train_steps = int(v * 10)

    def state_dict(self):
        return self.st

    def load_state_dict(self, st):
        self.st = st


class StubBuffer:
    """A NumPy ring with EnvReplayBuffer's insert / cursor / read / generator surface."""

    def __init__(self, capacity, O=5, A=2, seed=0):
        self._max_replay_buffer_size, self._observation_dim, self._action_dim = capacity, O, A
        self.o = np.zeros((capacity, O), np.float32)
        self.a = np.zeros((capacity, A), np.float32)
        self.r = np.zeros((capacity, 1), np.float32)
        self.no = np.zeros((capacity, O), np.float32)
        self.t = np.zeros((capacity, 1), np.uint8)
        self._top = self._size = self._rw = 0
        self.key, self.pos = np.random.RandomState(seed).randint(0, 2 ** 31, 624).astype(np.uint32), seed % 624
        self.reads = []

    def add_block(self, o, a, r, no, t):
        for i in range(len(o)):
            j = self._top
            self.o[j], self.a[j], self.r[j], self.no[j], self.t[j] = o[i], a[i], np.reshape(r[i], 1), no[i], \
                np.reshape(t[i], 1) != 0
            self._top = (self._top + 1) % self._max_replay_buffer_size
            self._size = min(self._size + 1, self._max_replay_buffer_size)
            self._rw += 1

    def fill_random(self, n, rs):
        O, A = self._observation_dim, self._action_dim
        self.add_block(rs.normal(size=(n, O)).astype(np.float32), rs.normal(size=(n, A)).astype(np.float32),
                       rs.normal(size=(n, 1)).astype(np.float32), rs.normal(size=(n, O)).astype(np.float32),
                       (rs.uniform(size=(n, 1)) < 0.1).astype(np.uint8))
        self.pos = (self.pos + n) % 624

    def num_steps_can_sample(self):
        return self._size

    def top(self):
        return self._top

    def rows_written(self):
        return self._rw

    def set_cursor(self, top, size):
        self._top, self._size = int(top), int(size)

    def read_rows(self, start, n):
        self.reads.append((start, n))
        s = slice(start, start + n)
        return self.o[s].copy(), self.a[s].copy(), self.r[s].copy(), self.no[s].copy(), self.t[s].copy()

    def rng_state(self):
        return self.key.copy(), self.pos

    def set_rng_state(self, key, pos):
        self.key, self.pos = np.array(key, np.uint32), int(pos)

    def storage(self):
        n = self._size
        return [x[:n].copy() for x in (self.o, self.a, self.r, self.no, self.t)]


def group(R=3, cap=10000, seeds=None, noise=None, dims=None, batches=None):
    trainers, buffers, ids = [], [], []
    for i in range(R):
        O, A = (dims or {}).get(i, (5, 2))
        t = StubTrainer(1.0 + i, O=O, A=A, batch=(batches or {}).get(i, 8), noise_seed=(noise or {}).get(i, 100 + i))
        b = StubBuffer(cap, O, A, seed=i)
        s = (seeds or list(range(3, 3 + R)))[i]
        trainers.append(t)
        buffers.append(b)
        ids.append(gc.member_identity(f"s{s}", s, VARIANT, t))
    return trainers, buffers, ids


def extras(R, epoch):
    return [dict(epoch=epoch, seed=i) for i in range(R)]


def files_of(d):
    out = {}
    for root, _, names in os.walk(d):
        for n in names:
            p = os.path.join(root, n)
            out[os.path.relpath(p, d)] = os.path.getsize(p)
    return out


def assert_same_member(t, b, t2, b2):
    for k in t.NETS:
        assert np.array_equal(t.st["params"][k], t2.st["params"][k]), k
    for k in ("policy", "qf1", "qf2"):
        for x, y in zip(t.st["opt"][k], t2.st["opt"][k]):
            assert np.array_equal(x, y), k
    assert np.array_equal(t.st["scalars"], t2.st["scalars"]) and t._num_train_steps == t2._num_train_steps
    assert (b.top(), b.num_steps_can_sample()) == (b2.top(), b2.num_steps_can_sample())
    for x, y in zip(b.storage(), b2.storage()):
        assert np.array_equal(x, y)
    (k1, p1), (k2, p2) = b.rng_state(), b2.rng_state()
    assert p1 == p2 and np.array_equal(k1, k2)


# ---- incremental generations ------------------------------------------------------------------------------------------
def test_second_generation_writes_only_the_dirty_chunks_and_loads_back_exactly(tmp_path):
    d, R, cap, C = str(tmp_path / "ck"), 3, 20000, 4096
    rs = np.random.RandomState(0)
    trainers, buffers, ids = group(R, cap)
    for i, b in enumerate(buffers):
        b.fill_random(5000 + 1000 * i, rs)                  # 5000, 6000, 7000 rows: chunk 1 partly filled
    ck = GroupCheckpoint(d, C)
    ck.save(trainers, buffers, ids, extras(R, 0))
    assert ck.last_save["files"] == R + sum(-(-b.num_steps_can_sample() // C) for b in buffers)
    before = files_of(d)
    prev = [(b.rows_written(), b.top(), b.num_steps_can_sample()) for b in buffers]
    for i, (t, b) in enumerate(zip(trainers, buffers)):
        b.fill_random(2500, rs)
        t.fill(10.0 + i)
        b.reads.clear()
    ck.save(trainers, buffers, ids, extras(R, 1))
    after = files_of(d)
    new = {f: n for f, n in after.items() if f.startswith("gen-1/")}
    want_chunks, want_rows = [], 0
    for i, (b, p) in enumerate(zip(buffers, prev)):
        dirty = dirty_chunks(cap, C, b.num_steps_can_sample(), b.top(), b.rows_written(), p)
        assert dirty == ([1] if i == 0 else [1, 2])         # rows 5000..7499 / 6000..8499 / 7000..9499
        want_chunks += [f"gen-1/m{i}.c{k}.bin" for k in dirty]
        want_rows += sum(min(C, b.num_steps_can_sample() - k * C) for k in dirty)
        assert b.reads == [(k * C, min(C, b.num_steps_can_sample() - k * C)) for k in dirty]   # nothing else read back
    state_files = [f"gen-1/m{i}.state.bin" for i in range(R)]
    assert sorted(new) == sorted(want_chunks + state_files + ["gen-1/manifest.json"])
    row_bytes = 4 * (5 + 2 + 1 + 5) + 1
    assert sum(new[f] for f in want_chunks) == row_bytes * want_rows
    assert ck.last_save["files"] == len(want_chunks) + R
    assert ck.last_save["bytes"] == sum(new[f] for f in want_chunks + state_files)
    # the unchanged chunk 0 of every member still lives in gen-0; the replaced gen-0 files are gone
    assert sorted(f for f in after if f.startswith("gen-0/")) == [f"gen-0/m{i}.c0.bin" for i in range(R)]
    assert all(after[f] == before[f] for f in after if f.startswith("gen-0/"))
    # a fresh group loads every member back exactly
    t2, b2, ids2 = group(R, cap)
    for t in t2:
        t.fill(99.0)
    back = GroupCheckpoint(d, C).load(t2, b2, ids2)
    assert [e["epoch"] for e in back] == [1] * R
    for i in range(R):
        assert_same_member(trainers[i], buffers[i], t2[i], b2[i])


def test_a_load_is_the_baseline_of_the_next_save(tmp_path):
    d, C, cap = str(tmp_path / "ck"), 1000, 5000
    rs = np.random.RandomState(1)
    trainers, buffers, ids = group(2, cap)
    for b in buffers:
        b.fill_random(7300, rs)                              # wrapped: top 2300
    GroupCheckpoint(d, C).save(trainers, buffers, ids, extras(2, 0))
    t2, b2, ids2 = group(2, cap)
    ck = GroupCheckpoint(d, C)
    ck.load(t2, b2, ids2)
    for b in b2:                                             # the restored buffers counted the re-inserted rows
        assert b.rows_written() == cap
    for b in b2:
        b.fill_random(900, rs)                               # slots 2300..3199: chunks 2, 3
    ck.save(t2, b2, ids2, extras(2, 1))
    assert sorted(f for f in files_of(d) if f.startswith("gen-1/") and ".c" in f) == [
        f"gen-1/m{i}.c{k}.bin" for i in range(2) for k in (2, 3)]
    man = gc.read_manifest(d)
    assert [m["buffer"]["rows_written"] for m in man["members"]] == [8200, 8200]   # the run's own count goes on
    t3, b3, ids3 = group(2, cap)
    GroupCheckpoint(d, C).load(t3, b3, ids3)
    for i in range(2):
        assert_same_member(t2[i], b2[i], t3[i], b3[i])


def test_a_killed_save_leaves_the_previous_generation_whole(tmp_path, monkeypatch):
    d, R, C = str(tmp_path / "ck"), 3, 4096
    rs = np.random.RandomState(2)
    trainers, buffers, ids = group(R)
    for b in buffers:
        b.fill_random(6000, rs)
    ck = GroupCheckpoint(d, C)
    ck.save(trainers, buffers, ids, extras(R, 0))
    snap = [(dict(params={k: v.copy() for k, v in t.st["params"].items()}), b.storage(), b.top()) for t, b in
            zip(trainers, buffers)]
    for i, (t, b) in enumerate(zip(trainers, buffers)):
        t.fill(20.0 + i)
        b.fill_random(2500, rs)
    real, calls = gc._write, []

    def dying_write(path, arrays):
        calls.append(path)
        if len(calls) == 5:                                  # member 1's first chunk
            raise KeyboardInterrupt("killed half-way through the second save")
        return real(path, arrays)

    monkeypatch.setattr(gc, "_write", dying_write)
    with pytest.raises(KeyboardInterrupt):
        ck.save(trainers, buffers, ids, extras(R, 1))
    monkeypatch.setattr(gc, "_write", real)
    assert os.path.isdir(os.path.join(d, "gen-1"))           # the torn generation is there ...
    t2, b2, ids2 = group(R)
    assert [e["epoch"] for e in GroupCheckpoint(d, C).load(t2, b2, ids2)] == [0] * R     # ... and ignored
    for (params, storage, top), t, b in zip(snap, t2, b2):
        assert all(np.array_equal(params["params"][k], t.st["params"][k]) for k in t.NETS)
        assert b.top() == top and all(np.array_equal(x, y) for x, y in zip(storage, b.storage()))
    ck.save(trainers, buffers, ids, extras(R, 1))            # the next complete save removes the torn files
    assert sorted(x for x in os.listdir(d) if x.startswith("gen-")) == ["gen-0", "gen-2"]
    assert sorted(os.listdir(os.path.join(d, "gen-0"))) == [f"m{i}.c0.bin" for i in range(R)]   # rows 0..4095 unchanged
    t3, b3, ids3 = group(R)
    assert [e["epoch"] for e in GroupCheckpoint(d, C).load(t3, b3, ids3)] == [1] * R
    for i in range(R):
        assert_same_member(trainers[i], buffers[i], t3[i], b3[i])


def test_a_corrupted_chunk_of_the_last_member_leaves_every_member_unchanged(tmp_path):
    d, R = str(tmp_path / "ck"), 4
    rs = np.random.RandomState(3)
    trainers, buffers, ids = group(R)
    for b in buffers:
        b.fill_random(5000, rs)
    GroupCheckpoint(d, 4096).save(trainers, buffers, ids, extras(R, 0))
    man = gc.read_manifest(d)
    path = os.path.join(d, man["members"][-1]["buffer"]["chunks"][1]["file"])
    blob = bytearray(open(path, "rb").read())
    blob[17] ^= 0x40
    open(path, "wb").write(bytes(blob))
    t2, b2, ids2 = group(R)
    for t in t2:
        t.fill(42.0)
    with pytest.raises(ValueError, match="does not match"):
        GroupCheckpoint(d, 4096).load(t2, b2, ids2)
    for t, b in zip(t2, b2):
        assert float(t.st["params"]["policy"][0]) == 42.0 and b.rows_written() == 0 and b.num_steps_can_sample() == 0


@pytest.mark.parametrize("change, member, field", [
    (dict(seeds=[4, 3, 5]), 0, "label"),
    (dict(seeds=[3, 4, 9]), 2, "label"),
    (dict(dims={1: (6, 2)}), 1, "obs_dim"),
    (dict(batches={2: 16}), 2, "batch"),
    (dict(noise={1: 7}), 1, "hparams.noise_seed"),
])
def test_another_group_is_refused_before_any_state_is_touched(tmp_path, change, member, field):
    d, R = str(tmp_path / "ck"), 3
    trainers, buffers, ids = group(R)
    for b in buffers:
        b.fill_random(100, np.random.RandomState(4))
    GroupCheckpoint(d, 64).save(trainers, buffers, ids, extras(R, 0))
    t2, b2, ids2 = group(R, **change)
    for t in t2:
        t.fill(42.0)
    with pytest.raises(GroupMismatchError, match=rf"group member {member} \(.*\): {field} is"):
        GroupCheckpoint(d, 64).load(t2, b2, ids2)
    for t, b in zip(t2, b2):
        assert float(t.st["params"]["policy"][0]) == 42.0 and b.rows_written() == 0
    t3, b3, ids3 = group(R)
    with pytest.raises(GroupMismatchError, match="member 2 .*the group has 2 members, the checkpoint 3"):
        GroupCheckpoint(d, 64).load(t3[:2], b3[:2], ids3[:2])


def test_a_seed_change_alone_is_named():
    t = StubTrainer(1.0)
    a, b = gc.member_identity("x", 3, VARIANT, t), gc.member_identity("x", 4, VARIANT, t)
    man = dict(members=[dict(identity=dict(a))])
    with pytest.raises(GroupMismatchError, match=r"group member 0 \(x\): seed is 4 here, 3 in the checkpoint"):
        gc._check_identity(man, [b])


def test_the_epoch_count_is_not_part_of_the_identity():
    v2 = dict(VARIANT, algorithm_kwargs=dict(VARIANT["algorithm_kwargs"], num_epochs=2000))
    assert gc.variant_hash(v2) == gc.variant_hash(VARIANT)
    v3 = dict(VARIANT, replay_buffer_size=5)
    assert gc.variant_hash(v3) != gc.variant_hash(VARIANT)


def test_load_group_member_into_a_solo_trainer(tmp_path):
    d = str(tmp_path / "ck")
    rs = np.random.RandomState(5)
    trainers, buffers, ids = group(3, 3000)
    for b in buffers:
        b.fill_random(4000, rs)
    GroupCheckpoint(d, 512).save(trainers, buffers, ids, extras(3, 6))
    t, b = StubTrainer(0.0), StubBuffer(3000, seed=9)
    assert gc.load_group_member(d, 2, t, b) == dict(epoch=6, seed=2)
    assert_same_member(trainers[2], buffers[2], t, b)
    # the solo trainer goes on under the member's noise seed: its handle was rebuilt with it (for its own batch size)
    assert t.noise_seed == trainers[2].noise_seed == 102 and t.created == [(8, 102)]
    with pytest.raises(IndexError):
        gc.load_group_member(d, 3, t, b)


def test_no_checkpoint_and_a_dangling_pointer(tmp_path):
    d = str(tmp_path / "ck")
    assert not GroupCheckpoint(d).exists()
    trainers, buffers, ids = group(1)
    GroupCheckpoint(d).save(trainers, buffers, ids, extras(1, 0))
    assert GroupCheckpoint(d).exists()
    with open(os.path.join(d, "latest"), "w") as f:
        f.write("gen-7\n")
    with pytest.raises(FileNotFoundError, match="refusing"):
        GroupCheckpoint(d).exists()


# ---- the drivers still refuse a resume without a directory, before any run is built ----------------------------------
def test_group_drivers_refuse_resume_without_a_checkpoint_dir(monkeypatch):
    from robosuite_benchmark_amd import driver, variant

    def no_runs(*a, **k):
        raise AssertionError("a run was built")

    monkeypatch.setattr(driver, "_group_run", no_runs)
    v = variant.default_variant("Lift", ("Panda",), batch_size=256)
    with pytest.raises(RuntimeError, match="resume"):
        driver.experiment_group(v, seeds=[1, 2], resume=True)
    with pytest.raises(RuntimeError, match="resume"):
        driver.experiment_sweep([(v, 1)], resume=True)


def test_rows_written_is_declared_and_bound():
    from robosuite_benchmark_amd import _lib
    from tests.test_abi_library import declared_symbols
    assert "sac_buffer_rows_written" in declared_symbols() and "sac_buffer_rows_written" in _lib.SYMBOLS
    assert hasattr(_lib.load(), "sac_buffer_rows_written")
