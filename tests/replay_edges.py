"""Edge cases of the replay path (test infrastructure, used by tests/test_gpu_replay_edges.py and checked on the CPU by
tests/test_replay_edges_host.py): the index draw (k_mt_randint, its host mirror mt_skip_accepted, the grouped draw), the row
gather (gather_body<NIT> and its feature-major copy saT) and the ingest of csrc/replay_buffer.hip.

Everything here has an exact reference -- np.random.RandomState for the indices, the float64 HostReplayBuffer of
oracle/sac_step_torch.py for the rows, ndarray.astype(np.float32) for the cast -- so no comparison built on these tables has
a tolerance.  The tables:

  SIZES       buffer sizes.  A power of two has mask == size - 1: no draw is ever rejected.  2^k + 1 has mask == 2^(k+1) - 1:
              about half of all draws are rejected, the most a stream can see.  2^16 - 1 rejects one draw in 2^16.
  POSITIONS   positions of the MT19937 state a draw starts from: the first and last word, both sides of the twist's three
              dependent groups ([0, 227), [227, 454), [454, 624)), and 624, the lazily twisted state.
  OBS_WIDTHS  observation widths: both sides of every boundary of nit = ceil(Ost / 64), the chunks per thread the gather is
              dispatched on (template arms 1, 2, 4, 8), and the widest row its LDS tile takes."""
from __future__ import annotations

import numpy as np

MT_N = 624
MT_GROUPS = (0, 227, 454, 624)           # the twist's three dependent groups (MT_N - MT_M = 227)

SIZES_NO_REJECTION = (2, 16, 1024, 1 << 16, 1 << 20)
SIZES_MOST_REJECTION = (3, 17, 1025, (1 << 16) + 1, (1 << 20) + 1)
SIZES = SIZES_NO_REJECTION + SIZES_MOST_REJECTION + ((1 << 16) - 1,)
SEEDS = (1, 251)
BATCHES = (1, 16, 255, 256, 257, 1024)
POSITIONS = (0, 1, 226, 227, 228, 453, 454, 455, 623, 624)
POSITION_SIZES = (1024, (1 << 16) + 1)   # a size without rejection, a size with the most, for the start positions
PADDED_BATCHES = (1, 15, 17, 255, 257)   # bt != bp for all but none: sample_indices(B, PADDED_N) at size 2^16 + 1
PADDED_N = 700
GROWING_SIZES = (1, 2, 3, 1024, 1025)    # a buffer that grows between draws


def size_id(size):
    for d, tag in ((0, ""), (1, "+1"), (-1, "-1")):
        if size > 32 and (size - d) & (size - d - 1) == 0:
            return f"2^{(size - d).bit_length() - 1}{tag}"
    return str(size)


def mask_of(size):
    """The smallest 2^k - 1 >= size - 1: what NumPy's masked rejection and the kernel AND every draw with."""
    m = int(size) - 1
    for s in (1, 2, 4, 8, 16):
        m |= m >> s
    return m


def start_state(seed, pos):
    """("MT19937", key, pos): the 624 words RandomState(seed) is seeded with, read from word `pos` on."""
    key = np.random.RandomState(seed).get_state()[1].copy()
    return ("MT19937", key, int(pos))


def count_to_last_word(pos):
    """Without rejection: how many indices a draw from `pos` takes to end on word 623 (position 624 afterwards; from the
    lazily twisted 624 that is one whole state)."""
    return MT_N - pos if pos < MT_N else MT_N


def count_ending_on_word(state, size, word, limit=20 * MT_N):
    """The smallest count n >= 1 for which RandomState.randint(0, size, n) from `state` accepts word `word` of the
    generator as its last draw (position word + 1 afterwards) -- found on the reference itself, one index at a time.
    With rejection a given word is accepted only every other state or so: the search runs over as many twists as it takes."""
    rs = np.random.RandomState(0)
    rs.set_state(state)
    for n in range(1, limit + 1):
        rs.randint(0, size, 1)
        if rs.get_state()[2] == word + 1:
            chk = np.random.RandomState(0)
            chk.set_state(state)
            chk.randint(0, size, n)
            assert chk.get_state()[2] == word + 1       # one call of n draws == n calls of one
            return n
    raise AssertionError(f"no count within {limit} ends on word {word}")


def words_consumed(before, after, twists):
    """Words between two get_state() results of one stream that twisted `twists` times in between."""
    return twists * MT_N + int(after[2]) - int(before[2])


def same_state(a, b):
    """Two generator states, (key, pos) or get_state() tuples: all 624 words and the position."""
    ka, pa = (a[1], a[2]) if len(a) > 2 else a
    kb, pb = (b[1], b[2]) if len(b) > 2 else b
    return int(pa) == int(pb) and np.array_equal(np.asarray(ka, np.uint32), np.asarray(kb, np.uint32))


# ---- the gather: widths, and launch_gather's arithmetic restated ----------------------------------------------------------
RB = 16                                   # rows per gather block
GATHER_LDS_LIMIT = 64 * 1024
GATHER_ARMS = (1, 2, 4, 8)
GATHER_GRID = 1024                        # persistent workgroups: the block stride of the two-set ping-pong
ACT_WIDTHS = (1, 3, 4, 5, 7, 16)


def round_up(x, m):
    return (x + m - 1) // m * m


def ost(O):
    """Row stride of the observation storage (floats): 16-byte chunks."""
    return round_up(O, 4)


def gather_nit(O):
    """Observation chunks per thread: ceil(16 rows * (Ost / 4) chunks / 256 threads)."""
    return (RB * (ost(O) // 4) + 255) // 256


def gather_arm(O):
    """The template instance launch_gather dispatches to (0: refused)."""
    nit = gather_nit(O)
    return next((a for a in GATHER_ARMS if nit <= a), 0)


def gather_lds_bytes(O, A):
    return 4 * (2 * RB * ost(O) + RB * round_up(A, 4))


def gather_accepts(O, A):
    """launch_gather's two conditions: the LDS tile and the chunks per thread."""
    return gather_lds_bytes(O, A) <= GATHER_LDS_LIMIT and gather_nit(O) <= GATHER_ARMS[-1]


def widest_obs(A):
    """The widest observation launch_gather takes next to actions of width A."""
    O = max(o for o in range(1, 4096) if gather_accepts(o, A))
    assert not any(gather_accepts(o, A) for o in range(O + 1, 4096))
    return O


# 385 is not a boundary of an arm; it is the first width with seven chunks per thread, which no other entry has
OBS_WIDTHS = (1, 4, 61, 64, 65, 128, 129, 192, 193, 256, 257, 379, 385)
GATHER_CASES = tuple((O, ACT_WIDTHS[i % len(ACT_WIDTHS)]) for i, O in enumerate(OBS_WIDTHS)) + \
    ((widest_obs(1), 1), (widest_obs(16), 16))
SWEEP_CASES = ((61, 3), (193, 4), (257, 7))            # one width per pipeline shape for the slot-count sweep: arms 1, 4, 8
SWEEP_SLOTS = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 3073)      # x 1 block of 16 rows: around 1, 2 and 3 trips of the grid
GATHER_ROWS = 2048
STEP_WIDTHS = (61, 64, 65, 129, 256, 257, 379)         # saT through the step: both write-outs, the obs/action boundary KA
STEP_ACTS = (1, 16)
STEP_BATCHES = (16, 48)
STEP_HIDDEN = ((256, 256), (32,))                      # the fused kernels, the general step
RELAYOUT_BATCHES = (48, 17, 33, 16)                    # one buffer through four slot layouts


def gather_index_sets(n):
    """Index vectors for gather(): both ends, duplicates, a descending run over three blocks, one index repeated."""
    return {
        "ends and duplicates": np.array([0, n - 1, n - 1, 0, 5, 5, 5, 17] * 2, np.int64),
        "descending run": np.arange(n - 1, n - 49, -1, dtype=np.int64),
        "one index": np.full(32, n // 2 + 1, np.int64),
        "odd length": np.array([n - 1, 0, 1, n - 2] * 4 + [n // 3], np.int64),
    }


# ---- rows that name their own place -----------------------------------------------------------------------------------------
def coded_transitions(n, O, A, first=0, stride=512):
    """(obs, act, rew, next_obs, term) of rows first .. first + n - 1, float64, every value exact in float32:
        obs[i, k] = (first + i) * stride + k + 1        next_obs[i, k] = -obs[i, k]
        act[i, k] = -((first + i) * 16 + k) - 0.5       rew[i] = first + i + 0.125
    No two cells of a block are equal, none is 0 (what a cleared pad holds), and locate() reads a value back into the array,
    row and column it belongs to.  stride 512 holds every supported width and 2^14 rows; narrower rows take a smaller one."""
    assert O <= stride and A <= 16 and (first + n) * stride + stride <= 1 << 24, (n, O, A, first, stride)
    i = np.arange(first, first + n, dtype=np.float64)[:, None]
    obs = i * stride + np.arange(O)[None, :] + 1.0
    act = -(i * 16 + np.arange(A)[None, :]) - 0.5
    rew = i + 0.125
    term = (((i.astype(np.int64) % 7) == 3) | ((i.astype(np.int64) % 5) == 0)).astype(np.uint8)
    return obs, act, rew, -obs, term


def locate(value, stride=512):
    """Which cell of coded_transitions holds `value`."""
    v = float(value)
    if v != v or abs(v) >= 1 << 25:
        return f"{v!r} (no coded cell)"
    if v == int(v) and v >= 1:
        return f"obs[{int(v - 1) // stride}, {int(v - 1) % stride}]"
    if v == int(v) and v <= -1:
        return f"next_obs[{int(-v - 1) // stride}, {int(-v - 1) % stride}]"
    if v < 0 and v * 2 == int(v * 2):
        return f"act[{int(-v - 0.5) // 16}, {int(-v - 0.5) % 16}]"
    if v > 0 and v * 8 == int(v * 8):
        return f"rew[{int(v)}]"
    return f"{v!r} (no coded cell)"


def assert_bits(what, got, want, stride=512):
    """Equality of the uint32 views (-0.0 and NaN count); a mismatch is reported as the cell that landed there."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want, np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    if np.any(bad):
        at = tuple(int(x) for x in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} cells differ; first at {at}: holds "
                             f"{locate(got[at], stride)}, wanted {locate(want[at], stride)}")


# ---- the float64 -> float32 cast of the ingest ------------------------------------------------------------------------------
def cast_edge_values():
    """A float64 vector whose float32 cast has to round: ties between float32 neighbours whose lower neighbour has an even
    and an odd last bit (round to even goes down, then up), the doubles next to each tie on both sides, values above
    FLT_MAX (and the tie between FLT_MAX and 2^128, which rounds to inf), the denormal boundary, +-0, inf and NaN."""
    f32 = np.float32
    lows = np.array([1.0, 1.0 + 2.0 ** -23, 3.0, 0.1, 123456.7, 2.0 ** -126, 2.0 ** -140, 3 * 2.0 ** -149], f32)
    lows = np.concatenate([lows, np.nextafter(lows, f32(np.inf))])          # every neighbour pair in both parities
    ties = (lows.astype(np.float64) + np.nextafter(lows, f32(np.inf)).astype(np.float64)) / 2
    fmax = float(np.finfo(f32).max)
    over = np.array([fmax + 2.0 ** 103, np.nextafter(fmax + 2.0 ** 103, 0.0), 3.5e38, 1e39, 1e300, np.finfo(np.float64).max])
    tiny = np.array([1e-45, 7e-46, 2.0 ** -150, np.nextafter(2.0 ** -150, 1.0), 2.0 ** -149, 1e-38, 1.1754943508222875e-38,
                     5e-324])
    body = np.concatenate([ties, np.nextafter(ties, np.inf), np.nextafter(ties, -np.inf), over, tiny])
    return np.concatenate([body, -body, [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -2.5, fmax, -fmax]])


def cast_tie_parities(ties):
    """For float64 values halfway between two float32 neighbours: the last bit of the LOWER neighbour (by magnitude)."""
    t = np.abs(np.asarray(ties, np.float64))
    with np.errstate(over="ignore"):
        lo = t.astype(np.float32)
        lo = np.where(lo.astype(np.float64) > t, np.nextafter(lo, np.float32(0)), lo).astype(np.float32)
    return lo.view(np.uint32) & 1


def to_f32(x):
    """The reference cast: NumPy's, round to nearest even, overflow to inf."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return np.asarray(x).astype(np.float32)


def cast_edge_block(O=8, A=4):
    """The cast-edge values as a block of transitions (float64): every value occurs in every array and column."""
    v = cast_edge_values()
    m = len(v)
    i = np.arange(m)[:, None]
    obs = v[(i + np.arange(O)[None, :]) % m]
    nobs = v[(i + 3 * np.arange(O)[None, :] + 2) % m]
    act = v[(i + 2 * np.arange(A)[None, :] + 1) % m]
    rew = v[:, None].copy()
    term = (np.arange(m) % 3 == 0).astype(np.uint8)[:, None]
    return obs, act, rew, nobs, term


# ---- ingest -------------------------------------------------------------------------------------------------------------------
INGEST_ROWS = 8192                        # rows per pinned staging buffer
INGEST_CAPACITY = 20_000


def ingest_blocks(capacity=INGEST_CAPACITY):
    """[(what, rows)]: block sizes around the staging chunk, blocks that end exactly on the ring's last slot (before and
    after the first wrap), a block of exactly the capacity and one of 2 x capacity + 7."""
    blocks, top = [], 0

    def add(what, n):
        nonlocal top
        blocks.append((what, n))
        top = (top + n) % capacity

    add("one row short of a staging chunk", INGEST_ROWS - 1)
    add("exactly a staging chunk", INGEST_ROWS)
    add("ends on the ring's last slot", capacity - top)
    assert top == 0
    add("a staging chunk and a row", INGEST_ROWS + 1)
    add("two chunks and a row, across the ring's end", 2 * INGEST_ROWS + 1)
    add("exactly the capacity", capacity)
    add("ends on the ring's last slot again", capacity - top)
    assert top == 0
    add("a single row", 1)
    add("twice the capacity and seven", 2 * capacity + 7)
    return blocks
