"""The cases of tests/golden/evaluate_entries.npz: what scripts/make_evaluate_golden.py --cases tests.evaluate_entries_cases
wrote with one commit's library and tests/test_gpu_evaluate_entries_golden.py compares, byte for byte, with the library
of now.

The evaluation entries that evaluate_columns.npz and general_layers.npz do not reach: sac_evaluate_replay_many,
td3_evaluate_stats_many and td3_evaluate_replay_many on the fused members SMALL and WIDE of evaluate_golden_cases, and
td3_evaluate_general_many, td3_evaluate_general_stats_many and td3_evaluate_replay_general_many on TD3 trainers of
general_golden_cases' NARROW and DEEP shapes (target_policy_noise 0.3 with clip 0.25, so that the clip binds on part of
the draws).  Two members in ONE grouped call, weights as constructed from fixed seeds and no training step.  Rows per
member: a partial 16-row block, a full one, two blocks with a partial second one, and for the general entries one call in
which the second member has no rows and sits out.

  plain entries    once with every optional output array and once with none
  stats entries    once with a null `rows` and no optional array, once with `rows` and every optional array; the stats
                   struct's bytes are recorded
  replay entries   a buffer of 40 rows; the indices hold row 0, the last row and a repeat; once with null stats, once
                   with stats
  NaN              one case per objective: a NaN in one observation row of the second member (for the replay entry in
                   the storage row that index NAN_ROW names, and no other index does)"""
import ctypes as C

import numpy as np

from robosuite_benchmark_amd import FlattenMlp, TanhMlpPolicy, TD3Trainer, _lib
from tests.evaluate_golden_cases import NAN_ROW, make_inputs, make_members
from tests.general_golden_cases import DEEP, NARROW, replay_buffer

GOLDEN = "evaluate_entries.npz"
ROW_PAIRS = ((1, 17), (16, 1), (17, 16))                          # rows of the two members in one call
SITS_OUT = (17, 0)                                                # the general entries: the second member has no rows
NAN_ROWS, NAN_MEMBER = (16, 17), 1
BUFFER_ROWS = 40                                                  # (general_golden_cases.replay_buffer's)
FUSED = ("sac_evaluate_replay_many", "td3_evaluate_stats_many", "td3_evaluate_replay_many")
GENERAL = ("td3_evaluate_general_many", "td3_evaluate_general_stats_many", "td3_evaluate_replay_general_many")


def _variants(entry):
    """(arrays asked for, stats asked for) of an entry's cases, by name."""
    if "replay" in entry:
        return ("nostats", "stats")
    return ("none", "all")


# (entry, rows, variant, nan)
CASES = [(entry, rows, variant, False) for entry in FUSED for rows in ROW_PAIRS for variant in _variants(entry)] + \
        [(entry, rows, variant, False) for entry in GENERAL for rows in ROW_PAIRS for variant in _variants(entry)] + \
        [(entry, SITS_OUT, _variants(entry)[1], False) for entry in GENERAL] + \
        [("sac_evaluate_replay_many", NAN_ROWS, "stats", True), ("td3_evaluate_general_many", NAN_ROWS, "all", True)]


def case_id(case):
    entry, rows, variant, nan = case
    return f"{entry}-{rows[0]}x{rows[1]}-{variant}{'-nan' if nan else ''}"


def make_general_td3():
    """TD3 trainers of the shapes NARROW and DEEP, general-step, from fixed seeds; no step is taken."""
    out = []
    for seed, (O, A, hidden) in ((60, NARROW), (61, DEEP)):
        rs = np.random.RandomState(seed)
        qs = [FlattenMlp(list(hidden), 1, O + A, rs=rs) for _ in range(4)]
        pols = [TanhMlpPolicy(list(hidden), A, O, rs=rs) for _ in range(2)]
        t = TD3Trainer(policy=pols[0], qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], target_policy=pols[1],
                       batch_size=32, noise_seed=seed, reward_scale=2.5, discount=0.98,
                       target_policy_noise=0.3, target_policy_noise_clip=0.25)
        assert t.fused_mode() == 3
        out.append(t)
    return out


def make_all_members():
    """The members of every entry family, as run() takes them: fused SAC, fused TD3, general TD3."""
    return {"sac": make_members(False), "td3": make_members(True), "td3_general": make_general_td3()}


def replay_indices(n, seed, nan):
    """n storage rows of a BUFFER_ROWS buffer: row 0, the last row and a repeat where n has room for them.  With nan, row 0
    stands at position NAN_ROW and nowhere else."""
    idx = np.random.RandomState(seed).randint(1, BUFFER_ROWS - 1, n).astype(np.int64)
    if nan:
        idx[NAN_ROW] = 0
    elif n >= 4:
        idx[:4] = (0, BUFFER_ROWS - 1, 5, 5)
    else:
        idx[0] = 0
    return idx


def run(all_members, case):
    """One grouped call of `case`: an ordered dict name -> array of everything the call returned for the members with
    rows -- `rows` and the optional arrays asked for (float32), SAC's alpha, and the stats struct's bytes (float64)."""
    entry, rows, variant, nan = case
    td3, replay = entry.startswith("td3"), "replay" in entry
    members = all_members["td3_general" if "general" in entry else "td3" if td3 else "sac"]
    stats = "stats" in entry or variant == "stats"
    arrays = replay or variant == "all"
    want_rows = replay or variant == "all" or "stats" not in entry
    names = _lib.TD3_EVAL_ARRAYS if td3 else _lib.EVAL_ARRAYS
    n_cols = len(_lib.TD3_EVAL_ROWS if td3 else _lib.EVAL_ROWS)
    io_t, stats_t = (_lib.Td3EvalIO, _lib.Td3EvalStats) if td3 else (_lib.SacEvalIO, _lib.SacEvalStats)
    n_in = 6 if td3 else 7
    ios, outs, srcs, keep = [], [], [], []
    for m, (t, n) in enumerate(zip(members, rows)):
        if n == 0:
            ios.append(io_t())
            srcs.append(_lib.SacEvalSrc(None, None))
            outs.append({})
            continue
        nan_here = nan and m == NAN_MEMBER
        ins = make_inputs(t, n, 100 * n + m, nan_here and not replay)[:n_in]
        out = dict(rows=np.full((n_cols, n), 7.0, np.float32)) if want_rows else {}
        if arrays:
            out.update((k, np.full((n, t.act_dim), 7.0, np.float32)) for k in names)
        src = [x.ctypes.data for x in ins]
        if replay:
            src[:5] = [None] * 5
            buf, idx = replay_buffer(t, 70 + m), replay_indices(n, 80 + m, nan_here)
            if nan_here:                                           # (the buffer is full: the next row overwrites storage row 0)
                row = [x[:1].copy() for x in make_inputs(t, 1, 90 + m, False)]
                row[0][0, 2] = np.nan
                buf.add_block(row[0], row[1], row[2].reshape(1, 1), row[4], row[3].reshape(1, 1).astype(np.uint8))
            srcs.append(_lib.SacEvalSrc(buf._h.value, idx.ctypes.data))
            keep += [buf, idx]
        ios.append(io_t(*src, *[out[k].ctypes.data if k in out else None for k in ["rows"] + list(names)]))
        keep.append(ins)
        outs.append(out)
    R = len(members)
    io_arr = (io_t * R)(*ios)
    sts = (stats_t * R)() if stats else None
    args = [(C.c_void_p * R)(*[t._h.value for t in members]), R, (C.c_int32 * R)(*rows)]
    if replay:
        args.append((_lib.SacEvalSrc * R)(*srcs))
    args.append(io_arr)
    if replay or "stats" in entry:
        args.append(sts)
    _lib.check(getattr(_lib.load(), entry)(*args), entry)
    got = {}
    for m, out in enumerate(outs):
        if rows[m] == 0:
            continue
        got.update((f"m{m}.{k}", v) for k, v in out.items())
        if not td3:
            got[f"m{m}.alpha"] = np.array([io_arr[m].alpha], np.float32)
        if stats:
            got[f"m{m}.stats"] = np.frombuffer(bytes(sts[m]), np.float64).copy()
    return got
