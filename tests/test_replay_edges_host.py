"""CPU: the tables and constructions of tests/replay_edges.py do what they claim -- on NumPy's RandomState, on the restated
launch arithmetic of the gather and on ndarray.astype -- so that tests/test_gpu_replay_edges.py knows which case it is in."""
import numpy as np
import pytest

from oracle.sac_step_torch import HostReplayBuffer
from tests import replay_edges as RE


def test_the_tables_are_the_ones_the_issue_names():
    assert RE.SIZES == (2, 16, 1024, 65536, 1048576, 3, 17, 1025, 65537, 1048577, 65535)
    assert RE.SEEDS == (1, 251) and RE.BATCHES == (1, 16, 255, 256, 257, 1024)
    assert RE.POSITIONS == (0, 1, 226, 227, 228, 453, 454, 455, 623, 624)
    assert set(RE.MT_GROUPS[1:3]) <= set(RE.POSITIONS)
    assert set(RE.OBS_WIDTHS) >= {1, 4, 61, 64, 65, 128, 129, 192, 193, 256, 257, 379}
    assert {A for _, A in RE.GATHER_CASES} == {1, 3, 4, 5, 7, 16}
    assert RE.SWEEP_SLOTS == (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 3073) and RE.GATHER_ROWS == 2048
    assert RE.STEP_WIDTHS == (61, 64, 65, 129, 256, 257, 379) and RE.RELAYOUT_BATCHES == (48, 17, 33, 16)
    for s in RE.SIZES_NO_REJECTION:
        assert RE.mask_of(s) == s - 1
    for s in RE.SIZES_MOST_REJECTION:
        assert RE.mask_of(s) == 2 * (s - 1) - 1


@pytest.mark.parametrize("size", RE.SIZES_NO_REJECTION)
def test_a_power_of_two_size_consumes_one_word_per_index(size):
    for seed in RE.SEEDS:
        for n in (1, 623, 624, 625, 100_000):
            rs = np.random.RandomState(seed)
            before = rs.get_state()                      # position 624: the first draw twists
            rs.randint(0, size, n)
            twists = (n + RE.MT_N - 1) // RE.MT_N
            assert RE.words_consumed(before, rs.get_state(), twists) == n, (size, seed, n)


@pytest.mark.parametrize("size", RE.SIZES_MOST_REJECTION)
def test_a_size_of_2k_plus_1_rejects_about_half_of_all_draws(size):
    """Counted on the reference: words = twists * 624 + position, with the twists counted by drawing in pieces of at most
    one state's worth of accepted indices (a piece of 300 indices consumes fewer than 2 x 624 words)."""
    n = 100_000
    if size == 3:                                        # mask 3, values 0..2 accepted: the rate is 3/4, not 1/2
        lo, hi = 1.2 * n, 1.5 * n
    else:
        lo, hi = 1.8 * n, 2.2 * n
    for seed in RE.SEEDS:
        rs = np.random.RandomState(seed)
        words, pos = 0, RE.MT_N
        for _ in range(n // 100):
            rs.randint(0, size, 100)
            new = rs.get_state()[2]
            assert new != pos                            # 100 accepted draws never consume exactly 624 words ... twice
            words += new - pos if new > pos else RE.MT_N - pos + new
            pos = new
        assert lo <= words <= hi, (size, seed, words)


@pytest.mark.parametrize("pos", RE.POSITIONS)
def test_start_positions_end_on_the_last_word_and_on_word_zero(pos):
    for seed in RE.SEEDS:
        st = RE.start_state(seed, pos)
        for size in RE.SIZES_NO_REJECTION:
            n = RE.count_to_last_word(pos)
            rs = np.random.RandomState(0); rs.set_state(st)
            rs.randint(0, size, n)
            assert rs.get_state()[2] == RE.MT_N, (seed, pos, size)          # lazy: not twisted yet
            rs = np.random.RandomState(0); rs.set_state(st)
            rs.randint(0, size, n + 1)
            assert rs.get_state()[2] == 1, (seed, pos, size)                # the twist, then word 0
        size = RE.POSITION_SIZES[1]
        for word in (RE.MT_N - 1, 0):
            n = RE.count_ending_on_word(st, size, word)
            rs = np.random.RandomState(0); rs.set_state(st)
            idx = rs.randint(0, size, n)
            assert rs.get_state()[2] == word + 1 and 0 <= idx.min() and idx.max() < size
            if n > 1:                                    # and it is the LAST draw that lands there
                rs = np.random.RandomState(0); rs.set_state(st)
                rs.randint(0, size, n - 1)
                assert rs.get_state()[2] != word + 1 or n - 1 < 1


def test_a_set_state_round_trip_keeps_words_and_position():
    for pos in RE.POSITIONS:
        st = RE.start_state(7, pos)
        rs = np.random.RandomState(0); rs.set_state(st)
        assert RE.same_state(rs.get_state(), st) and RE.same_state((st[1], pos), rs.get_state())
    assert not RE.same_state(RE.start_state(7, 0), RE.start_state(7, 1))
    assert not RE.same_state(RE.start_state(7, 0), RE.start_state(8, 0))


def test_every_chunk_count_and_every_arm_of_the_gather_occurs():
    nits = {RE.gather_nit(O) for O, _ in RE.GATHER_CASES}
    assert nits == set(range(1, 9))
    full = {RE.gather_arm(O) for O, _ in RE.GATHER_CASES if RE.gather_nit(O) == RE.gather_arm(O)}
    part = {RE.gather_arm(O) for O, _ in RE.GATHER_CASES if RE.gather_nit(O) < RE.gather_arm(O)}
    assert full == {1, 2, 4, 8} and part == {4, 8}
    # the exact-fit strides (16 rows x Ost / 4 chunks fill whole passes of 256 threads) and one float beyond each
    for o in (64, 128, 256):
        assert RE.ost(o) == o and (RE.RB * o // 4) % 256 == 0 and RE.gather_nit(o + 1) == RE.gather_nit(o) + 1
        assert o in RE.OBS_WIDTHS and o + 1 in RE.OBS_WIDTHS
    assert all(RE.gather_accepts(O, A) for O, A in RE.GATHER_CASES)
    assert [RE.gather_arm(O) for O, _ in RE.SWEEP_CASES] == [1, 4, 8]
    assert all(RE.gather_arm(O) in (1, 2, 4, 8) for O in RE.STEP_WIDTHS)
    assert {RE.gather_arm(O) == 1 for O in RE.STEP_WIDTHS} == {True, False}          # both saT write-outs
    assert any(O % 16 == 0 for O in RE.STEP_WIDTHS) and any(O % 16 for O in RE.STEP_WIDTHS)   # KA == O and KA > O


def test_the_widest_row_comes_from_the_two_launch_conditions():
    for A in (1, 16):
        O = RE.widest_obs(A)
        assert (O, A) in RE.GATHER_CASES
        assert RE.gather_accepts(O, A) and not RE.gather_accepts(O + 1, A)
        assert RE.gather_nit(O) == 8                     # the LDS tile binds first: nit 8 is reached, 9 never asked for
        assert RE.gather_lds_bytes(O, A) <= RE.GATHER_LDS_LIMIT < RE.gather_lds_bytes(O + 1, A)
    assert RE.widest_obs(16) < RE.widest_obs(1)
    # slot counts on both sides of one, two and three trips of the 1024 persistent workgroups
    for trips in (1, 2):
        assert {trips * RE.GATHER_GRID - 1, trips * RE.GATHER_GRID, trips * RE.GATHER_GRID + 1} <= set(RE.SWEEP_SLOTS)
    assert max(RE.SWEEP_SLOTS) > 3 * RE.GATHER_GRID


@pytest.mark.parametrize("n,O,A,first,stride", [(2048, 508, 1, 0, 512), (2048, 61, 16, 0, 512), (1 << 14, 379, 7, 0, 512),
                                                (40_007, 5, 2, 80_000, 8)])
def test_coded_rows_are_unique_exact_and_name_their_place(n, O, A, first, stride):
    obs, act, rew, nobs, term = RE.coded_transitions(n, O, A, first=first, stride=stride)
    assert obs.shape == nobs.shape == (n, O) and act.shape == (n, A) and rew.shape == term.shape == (n, 1)
    cells = np.concatenate([x.ravel() for x in (obs, act, rew, nobs)])
    assert np.array_equal(cells.astype(np.float32).astype(np.float64), cells)       # exact in float32
    assert np.unique(cells).size == cells.size and not np.any(cells == 0)
    assert 0 < term.mean() < 1
    for i, k in ((0, 0), (n - 1, O - 1), (n // 2, O // 2)):
        assert RE.locate(obs[i, k], stride) == f"obs[{first + i}, {k}]"
        assert RE.locate(nobs[i, k], stride) == f"next_obs[{first + i}, {k}]"
    assert RE.locate(act[n - 1, A - 1]) == f"act[{first + n - 1}, {A - 1}]" and RE.locate(rew[3, 0]) == f"rew[{first + 3}]"
    with pytest.raises(AssertionError, match=rf"holds obs\[{first + 1}, 0\], wanted obs\[{first}, 1\]"):
        bad = obs[:2].astype(np.float32)
        bad[0, 1] = obs[1, 0]
        RE.assert_bits("moved", bad, obs[:2], stride)


def test_coded_rows_survive_the_float64_host_buffer():
    obs, act, rew, nobs, term = RE.coded_transitions(64, 9, 3)
    host = HostReplayBuffer(64, 9, 3)
    host.fill_block(obs, act, rew, term, nobs)
    idx = np.array([63, 0, 0, 17])
    RE.assert_bits("obs", RE.to_f32(host._obs[idx]), obs[idx])
    RE.assert_bits("rew", RE.to_f32(host._rew[idx]), rew[idx])


def test_cast_edges_round_both_ways_overflow_and_flush():
    """astype(np.float32) is the reference of the ingest's cast: round to nearest, ties to even, overflow to inf."""
    with np.errstate(all="ignore"):
        _cast_edge_claims()


def _cast_edge_claims():
    v = RE.cast_edge_values()
    f = RE.to_f32(v)
    back = f.astype(np.float64)
    fin = np.isfinite(v) & np.isfinite(f)
    ties = fin & (back != v) & (np.abs(v - back) == np.abs(v - np.where(back < v, np.nextafter(f, np.float32(np.inf)),
                                                                       np.nextafter(f, np.float32(-np.inf))).astype(np.float64)))
    assert ties.sum() >= 16
    assert np.all(f[ties].view(np.uint32) & 1 == 0)                                  # every tie went to the even neighbour
    par = RE.cast_tie_parities(v[ties])
    assert set(par.tolist()) == {0, 1}                                               # down for one parity, up for the other
    up, down = np.abs(back[ties]) > np.abs(v[ties]), np.abs(back[ties]) < np.abs(v[ties])
    assert np.array_equal(up, par == 1) and np.array_equal(down, par == 0)
    # just off a tie: the nearer neighbour, whatever its parity
    off = fin & ~ties & (back != v) & (np.abs(v) > 1e-30)
    assert off.sum() >= 16
    other = np.where(back < v, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))).astype(np.float64)
    assert np.all(np.abs(v[off] - back[off]) < np.abs(v[off] - other[off]))
    fmax = float(np.finfo(np.float32).max)
    assert np.sum(np.isinf(f) & np.isfinite(v)) >= 10 and np.all(np.abs(v[np.isinf(f) & np.isfinite(v)]) > fmax)
    assert RE.to_f32(fmax + 2.0 ** 103) == np.inf and RE.to_f32(np.nextafter(fmax + 2.0 ** 103, 0.0)) == np.float32(fmax)
    assert RE.to_f32(1e-45).view(np.uint32) == 1 and RE.to_f32(7e-46).view(np.uint32) == 0
    assert RE.to_f32(-7e-46).view(np.uint32) == 0x80000000 and RE.to_f32(2.0 ** -150).view(np.uint32) == 0
    bits = set(f.view(np.uint32).tolist())
    assert {0x00000000, 0x80000000, 0x7f800000, 0xff800000} <= bits and np.isnan(f).sum() == 1
    obs, act, rew, nobs, term = RE.cast_edge_block()
    for x in (obs, act, rew, nobs):
        assert x.dtype == np.float64 and len(x) == len(v)
        for c in range(x.shape[1]):
            assert set(RE.to_f32(x[:, c]).view(np.uint32).tolist()) == bits


def test_ingest_blocks_hit_the_chunk_and_the_ring_end():
    cap, ch = RE.INGEST_CAPACITY, RE.INGEST_ROWS
    sizes = [n for _, n in RE.ingest_blocks()]
    assert {ch - 1, ch, ch + 1, 2 * ch + 1, cap, 2 * cap + 7} <= set(sizes)
    top, ends_on_last, wraps = 0, 0, 0
    for n in sizes:
        if n <= cap and top + n == cap:
            ends_on_last += 1
        if n <= cap and top + n > cap:
            wraps += 1
        top = (top + n) % cap
    assert ends_on_last >= 2 and wraps >= 2
    assert (sum(sizes) + 1) * 8 + 8 <= 1 << 24                                       # coded rows at stride 8 stay exact
