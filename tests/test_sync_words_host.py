"""The hand-off words of the fused launches (csrc/sac_step_plan.h) on the host: where each counter region lies, how much one
launch adds to each counter, and what the test hook sac_debug_set_launch_number writes for a launch number S -- every
counter at units * S modulo 2^32, every tagged word tagged S, the give-up word clear.  The header is compiled with the host
C++ compiler alone, as in test_step_plan_host.py; the expectations below are written out independently, from the
pointer arithmetic of k_abc (sac_fused.h) and k_chain8 (sac_chain.h) and the allocation's size formula."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robosuite_benchmark_amd", "csrc")

WRAPPER = r"""
#include "sac_step_plan.h"
using namespace sac;
extern "C" int stride() { return SYNC_STRIDE; }
extern "C" int regions() { return SYNC_REGIONS; }
extern "C" int region_line(int r, int NB) { return sync_region_line(r, NB); }
extern "C" int region_lines(int r, int NB) { return sync_region_lines(r, NB); }
extern "C" unsigned long long words(int NB) { return (unsigned long long)sync_words(NB); }
extern "C" unsigned units(int kernel, int r, int NB, int wide) { return sync_units(kernel, r, NB, wide != 0); }
extern "C" void fill(unsigned *w, int NB, int kernel, int wide, unsigned seq) { sync_fill(w, NB, kernel, wide != 0, seq); }
extern "C" int stall_hits(unsigned at, unsigned base, unsigned seq) { return test_stall_hits(at, base, seq) ? 1 : 0; }
extern "C" void unit_constants(unsigned *o) {
    o[0] = ABC_UNITS_HEAD; o[1] = ABC_UNITS_QA; o[2] = ABC_UNITS_TQ; o[3] = ABC_UNITS_AC; o[4] = ABC_UNITS_ZX;
    o[5] = CHAIN_UNITS_RB; o[6] = chain_units_lp(34);
}
"""

HEAD, QA, TQ, AC, LP, ABORT, ZX, LP_TAG = range(8)
ABC_SAC, ABC_TD3, CHAIN8 = range(3)
M32 = 1 << 32
# launch numbers around every power of two a target crosses, the wrap, a NaN bit pattern, and the chain's NB * seq crossings
SEQS = [0, 1, 2, 300, 2**28 - 1, 2**28, 2**28 + 1, 2**29 - 4, 2**29, 2**30, 2**30 + 5, 2**31 - 1, 2**31, 2**31 + 1,
        0x7FC00000, 2**32 - 4, 2**32 - 1, 2**31 // 34, 2**31 // 34 + 1, 2**32 // 34, 2**32 // 34 + 1]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("sync_words")
    src, so = d / "sync_wrapper.cpp", d / "libsync_words.so"
    src.write_text(WRAPPER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)])
    L = ctypes.CDLL(str(so))
    L.words.restype = ctypes.c_ulonglong
    L.units.restype = ctypes.c_uint
    return L


def first_lines(NB):
    """The first 128-byte line of each region, as the kernels compute their pointers: head at d.cnt, qa / tq / ac at 2, 3,
    4 NB lines, the chain's log-pi counter at 5 NB, the give-up word one line on, zx at 5 NB + 2, the tagged words at
    11 NB + 2."""
    return {HEAD: 0, QA: 2 * NB, TQ: 3 * NB, AC: 4 * NB, LP: 5 * NB, ABORT: 5 * NB + 1, ZX: 5 * NB + 2, LP_TAG: 11 * NB + 2}


def line_counts(NB):
    return {HEAD: 2 * NB, QA: NB, TQ: NB, AC: NB, LP: 1, ABORT: 1, ZX: 6 * NB, LP_TAG: 1}


def want_units(kernel, region, NB, wide):
    """What one launch adds to a counter: k_abc -- four column parts publish a head, two chains x four parts the qa / tq /
    ac counters of a row-block (the TD3 critic pass has no actor tail), four parts a split first layer; k_chain8 -- one
    item per row-block counter, every P0 item the log-pi counter."""
    if kernel == CHAIN8:
        return {QA: 1, TQ: 1, AC: 1, LP: NB}.get(region, 0)
    return {HEAD: 4, QA: 8, TQ: 8, AC: 8 if kernel == ABC_SAC else 0, ZX: 4 if wide else 0}.get(region, 0)


@pytest.mark.parametrize("NB", [1, 2, 7, 16, 34, 64])
def test_regions_lie_where_the_kernels_point(lib, NB):
    assert lib.stride() == 32 and lib.regions() == 8
    for r in range(8):
        assert lib.region_line(r, NB) == first_lines(NB)[r], r
        assert lib.region_lines(r, NB) == line_counts(NB)[r], r
    # the allocation: sizeof(unsigned) * 32 * (5 NB + 2 + 6 NB + 1) bytes; back to back, nothing overlaps
    assert lib.words(NB) == 32 * (5 * NB + 2 + 6 * NB + 1)
    assert sum(line_counts(NB).values()) * 32 == lib.words(NB)
    # the tagged words (8 bytes per row-block, k_abc: at most 16 row-blocks) fit their one line
    assert 16 * 8 <= 32 * 4


def test_units_per_launch(lib):
    c = (ctypes.c_uint * 7)()
    lib.unit_constants(c)
    assert list(c) == [4, 8, 8, 8, 4, 1, 34]
    for kernel in (ABC_SAC, ABC_TD3, CHAIN8):
        for NB in (1, 16, 34):
            for wide in (0, 1):
                for r in range(8):
                    assert lib.units(kernel, r, NB, wide) == want_units(kernel, r, NB, wide), (kernel, r, NB, wide)


def test_the_kernels_take_their_targets_from_the_table():
    fused = open(os.path.join(CSRC, "sac_fused.h")).read()
    chain = open(os.path.join(CSRC, "sac_chain.h")).read()
    code = "\n".join(re.sub(r"//.*", "", line) for line in (fused + chain).splitlines())
    assert not re.search(r"\b\d+u?\s*\*\s*(sa\.)?seq\b", code)                 # no literal multiple of the launch number
    assert not re.search(r"d\.NB\s*\*\s*sa\.seq", code)
    for name in ("ABC_UNITS_HEAD", "ABC_UNITS_QA", "ABC_UNITS_TQ", "ABC_UNITS_AC", "ABC_UNITS_ZX"):
        assert re.search(name + r"\s*\*\s*seq\b", fused), name
    assert chain.count("CHAIN_UNITS_RB * sa.seq") == 3 and chain.count("chain_units_lp(d.NB) * sa.seq") == 6
    # the early look is said with a flag: no default that reads as a counter value
    assert "peek = 0ull)" in fused and "bool have_peek" in fused and "!have_peek ||" in fused


@pytest.mark.parametrize("kernel, NB, wide", [(ABC_SAC, 16, 0), (ABC_SAC, 1, 0), (ABC_SAC, 4, 1), (ABC_TD3, 8, 0), (ABC_TD3, 2, 1),
                                              (CHAIN8, 34, 0), (CHAIN8, 64, 1)])
def test_fill_for_a_launch_number(lib, kernel, NB, wide):
    n = int(lib.words(NB))
    first, count = first_lines(NB), line_counts(NB)
    for seq in SEQS:
        w = (ctypes.c_uint * n)(*([0xDEADBEEF] * n))
        lib.fill(w, NB, kernel, wide, seq)
        got = list(w)
        want = [0] * n
        for r in (HEAD, QA, TQ, AC, LP, ZX):
            for i in range(count[r]):
                want[32 * (first[r] + i)] = want_units(kernel, r, NB, wide) * seq % M32
        if kernel == ABC_SAC:                       # {value, launch number}: the value in the low word, the tag in the high one
            for i in range(NB):
                want[32 * first[LP_TAG] + 2 * i + 1] = seq
        assert got == want, (seq, [i for i in range(n) if got[i] != want[i]][:8])
        assert got[32 * first[ABORT]] == 0


def test_a_wait_of_the_next_launch_is_not_yet_satisfied_and_is_after_its_adds(lib):
    """The compare the kernels use, (int)(counter - target) >= 0, on the filled words: launch seq + 1 finds every counter
    it waits for short of its target by exactly the units, and at the target once the units have been added -- at every
    launch number, across every wrap."""
    def reached(v, target):
        d = (v - target) % M32
        return d < 2**31
    for kernel, NB, wide in ((ABC_SAC, 16, 1), (ABC_TD3, 16, 1), (CHAIN8, 34, 0)):
        n = int(lib.words(NB))
        first = first_lines(NB)
        for seq in SEQS:
            w = (ctypes.c_uint * n)()
            lib.fill(w, NB, kernel, wide, seq)
            nxt = (seq + 1) % M32
            for r in (HEAD, QA, TQ, AC, LP, ZX):
                u = want_units(kernel, r, NB, wide)
                if u == 0:
                    continue
                v = w[32 * first[r]]
                assert not reached(v, u * nxt % M32), (kernel, r, seq)
                assert reached((v + u) % M32, u * nxt % M32) and not reached((v + u - 1) % M32, u * nxt % M32), (kernel, r, seq)
            if kernel == ABC_SAC:
                assert w[32 * first[LP_TAG] + 1] != nxt


def test_the_stall_counts_from_the_launch_number_last_set(lib):
    assert lib.stall_hits(3, 0, 3) == 1 and lib.stall_hits(3, 0, 2) == 0 and lib.stall_hits(3, 0, 4) == 0
    for seq in range(0, 10):
        assert lib.stall_hits(0, 0, seq) == 0 and lib.stall_hits(0, 7, seq) == 0          # unset: never
    for base in (2**28 - 2, 2**31 - 2, 2**32 - 2, 0x7FC00000 - 3, 2**32 - 1):
        hits = [k for k in range(1, 9) if lib.stall_hits(3, base, (base + k) % M32)]
        assert hits == [3], (base, hits)
