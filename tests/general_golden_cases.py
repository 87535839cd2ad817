"""The cases of tests/golden/general_layers.npz: what scripts/make_evaluate_golden.py --cases tests.general_golden_cases
wrote with one commit's library and tests/test_gpu_general_golden.py compares, byte for byte, with the library of now.

The general-shape inference entries (one launch per layer: k_act_layer, k_qval_layer, k_eval_layer, k_act_layer_session,
with k_eval_y and k_unit_moments behind them) on three general-step members in ONE grouped call, weights as constructed
from fixed seeds and no training step, so that nothing depends on a step kernel.  The shapes stand where the layer
schedule can go wrong:

  NARROW  O=3, A=1, hidden (24,)           one hidden layer: its head is launch 1 while the others still have layers;
                                           K % 4 != 0 (vec = 0); N < 64 (a clamped column tile)
  DEEP    O=19, A=3, hidden (72, 40, 136)  three hidden layers: the ping-pong reuses buffer 0; N = 72 is two column tiles
                                           with a partial second one; K = 136 is two reduction chunks with an edge chunk;
                                           the critics' K = 22 goes through the split point
  TWIN    DEEP's shape, a TD3 trainer      acting, Q values and unit statistics take it; evaluation refuses it

Rows per member (NARROW, DEEP, TWIN): a partial 16-row block, a full one, two blocks with a partial second one, and one
call in which the member in the middle has no rows and sits out.  The evaluation entries run NARROW and DEEP."""
import ctypes as C

import numpy as np

from robosuite_benchmark_amd import (EnvReplayBuffer, FlattenMlp, SACTrainer, TanhGaussianPolicy, TanhMlpPolicy, TD3Trainer,
                                     _lib)
from tests.evaluate_golden_cases import NAN_ROW, make_inputs

GOLDEN = "general_layers.npz"
NARROW, DEEP = (3, 1, (24,)), (19, 3, (72, 40, 136))              # (obs_dim, act_dim, hidden sizes)
ROWS = ((1, 17, 16), (16, 1, 17), (17, 16, 1), (17, 0, 5))        # rows of (NARROW, DEEP, TWIN) in one call
NAN_ROWS, NAN_MEMBER = (17, 16, 1), 1                             # the NaN cases: DEEP's observation row NAN_ROW, element 2
Q_MASKS = (0b0001, 0b1010, 0b1111)
# unit statistics: the net masks of (NARROW, DEEP, TWIN): SAC_NET_* bits, bit 5 TD3's target policy
UNIT_MASKS = {"policy": (0b000001, 0b000001, 0b000001), "critic": (0b000100, 0b000100, 0b000100),
              "mixed": (0b001001, 0b001001, 0b100010)}
# (the float64 records and the activations of the wide members are what the file's size is made of: with activations they
# get few rows, and in most cases one of them sits out)
UNIT_ROWS = {("policy", True): (17, 2, 0), ("critic", True): (1, 0, 2), ("mixed", True): (16, 5, 0),
             ("policy", False): (16, 0, 17), ("critic", False): (17, 16, 0), ("mixed", False): ROWS[3]}
SESSION_TICKS = (((17, 16, 1), (0, 1, 0)), ((1, 0, 17), (1, 0, 1)))          # (rows, deterministic) of two ticks
EVAL_ENTRIES = ("sac_evaluate_general_many", "sac_evaluate_general_stats_many", "sac_evaluate_replay_general_many")

# (family, rows, variant, nan)
CASES = [("act", rows, det, False) for rows in ROWS for det in ("det", "stoch")] + \
        [("q", rows, mask, False) for rows, mask in zip(ROWS, Q_MASKS + Q_MASKS[2:])] + \
        [("sac_evaluate_general_many", rows, arrays, False) for rows in ROWS for arrays in ("all", "none")] + \
        [("sac_evaluate_general_stats_many", rows, "none", False) for rows in ROWS[:2]] + \
        [("sac_evaluate_replay_general_many", ROWS[2], "all", False)] + \
        [("units", UNIT_ROWS[nets, acts], (nets, acts), False) for nets in UNIT_MASKS for acts in (True, False)] + \
        [("session", None, "ticks", False)] + \
        [("act", NAN_ROWS, "stoch", True), ("q", NAN_ROWS, 0b1111, True), ("sac_evaluate_general_many", NAN_ROWS, "all", True),
         ("units", UNIT_ROWS["mixed", True], ("mixed", True), True), ("session", None, "ticks", True)]


def case_id(case):
    family, rows, variant, nan = case
    if family == "units":
        variant = f"{variant[0]}-{'acts' if variant[1] else 'noacts'}"
    where = "" if rows is None else "-" + "x".join(map(str, rows))
    return f"{family}{where}-{variant}{'-nan' if nan else ''}"


def make_all_members():
    """[NARROW, DEEP, TWIN]: general-step trainers from fixed seeds; no step is taken."""
    out = []
    for seed, (O, A, hidden), td3 in ((50, NARROW, False), (51, DEEP, False), (52, DEEP, True)):
        rs = np.random.RandomState(seed)
        qs = [FlattenMlp(list(hidden), 1, O + A, rs=rs) for _ in range(4)]
        if td3:
            pols = [TanhMlpPolicy(list(hidden), A, O, rs=rs) for _ in range(2)]
            t = TD3Trainer(policy=pols[0], qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], target_policy=pols[1],
                           batch_size=32, noise_seed=seed, reward_scale=2.5, discount=0.98)
        else:
            pol = TanhGaussianPolicy(list(hidden), O, A, rs=rs, noise=np.random.RandomState(seed))
            t = SACTrainer(policy=pol, qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], batch_size=32,
                           noise_seed=seed, reward_scale=2.5, discount=0.98)
        assert t.fused_mode() == 3
        t.hidden = hidden
        out.append(t)
    return out


def _handles(ts):
    return (C.c_void_p * len(ts))(*[t._h.value for t in ts])


def _ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[None if a is None else a.ctypes.data for a in arrays])


def _inputs(ts, rows, nan):
    """Per member make_inputs' seven arrays (None for a member without rows); the NaN goes into member NAN_MEMBER."""
    return [None if n == 0 else make_inputs(t, n, 100 * n + m, nan and m == NAN_MEMBER) for m, (t, n) in enumerate(zip(ts, rows))]


def _run_act(ts, rows, det, nan):
    ins = _inputs(ts, rows, nan)
    out = [None if n == 0 else np.full((n, t.act_dim), 7.0, np.float32) for t, n in zip(ts, rows)]
    R = len(ts)
    _lib.check(_lib.load().sac_policy_act_general_many(
        _handles(ts), R, (C.c_int32 * R)(*rows), _ptrs([x and x[0] for x in ins]), (C.c_int32 * R)(*[int(det == "det")] * R),
        _ptrs([x and x[5] for x in ins]), _ptrs(out)), "sac_policy_act_general_many")
    return {f"m{m}.act": v for m, v in enumerate(out) if v is not None}


def _run_q(ts, rows, mask, nan):
    ins = _inputs(ts, rows, nan)
    out = [None if n == 0 else np.full((bin(mask).count("1"), n), 7.0, np.float32) for n in rows]
    R = len(ts)
    _lib.check(_lib.load().sac_q_values_general_many(
        _handles(ts), R, (C.c_int32 * R)(*rows), _ptrs([x and x[0] for x in ins]), _ptrs([x and x[1] for x in ins]),
        (C.c_uint32 * R)(*[mask] * R), _ptrs(out)), "sac_q_values_general_many")
    return {f"m{m}.q": v for m, v in enumerate(out) if v is not None}


def replay_buffer(t, seed):
    """A small replay buffer of fixed contents for trainer t."""
    rs = np.random.RandomState(seed)
    O, A, n = t.obs_dim, t.act_dim, 40
    buf = EnvReplayBuffer(n, obs_dim=O, action_dim=A)
    buf.add_block(rs.normal(0, 0.5, (n, O)).astype(np.float32), rs.uniform(-1, 1, (n, A)).astype(np.float32),
                  rs.uniform(0, 1, (n, 1)).astype(np.float32), rs.normal(0, 0.5, (n, O)).astype(np.float32),
                  (rs.uniform(0, 1, (n, 1)) < 0.3).astype(np.uint8))
    return buf


def _run_eval(ts, entry, rows, arrays, nan):
    ts, rows = ts[:2], rows[:2]                                    # (the SAC members)
    stats, replay = entry == "sac_evaluate_general_stats_many", entry == "sac_evaluate_replay_general_many"
    ins = _inputs(ts, rows, nan)
    ios, outs, keep = [], [], []
    for m, (t, n) in enumerate(zip(ts, rows)):
        out = {} if stats or n == 0 else dict(rows=np.full((len(_lib.EVAL_ROWS), n), 7.0, np.float32))
        if arrays == "all" and n:
            out.update((k, np.full((n, t.act_dim), 7.0, np.float32)) for k in _lib.EVAL_ARRAYS)
        src = [None] * 7 if n == 0 else [x.ctypes.data for x in ins[m]]
        if replay:
            src[:5] = [None] * 5
        ios.append(_lib.SacEvalIO(*src, *[out[k].ctypes.data if k in out else None for k in ["rows"] + _lib.EVAL_ARRAYS], -1.0))
        outs.append(out)
    R = len(ts)
    io_arr = (_lib.SacEvalIO * R)(*ios)
    sts = (_lib.SacEvalStats * R)() if stats else None
    args = [_handles(ts), R, (C.c_int32 * R)(*rows)]
    if replay:
        bufs = [replay_buffer(t, 70 + m) for m, t in enumerate(ts)]
        idx = [np.random.RandomState(80 + m).randint(0, 40, n).astype(np.int64) for m, n in enumerate(rows)]
        keep += bufs + idx
        args.append((_lib.SacEvalSrc * R)(*[_lib.SacEvalSrc(b._h.value, i.ctypes.data) for b, i in zip(bufs, idx)]))
    args.append(io_arr)
    if stats or replay:
        args.append(sts)
    _lib.check(getattr(_lib.load(), entry)(*args), entry)
    got = {}
    for m, out in enumerate(outs):
        if rows[m] == 0:
            continue
        got.update((f"m{m}.{k}", v) for k, v in out.items())
        got[f"m{m}.alpha"] = np.array([io_arr[m].alpha], np.float32)
        if stats:
            got[f"m{m}.stats"] = np.frombuffer(bytes(sts[m]), np.float64).copy()
    return got


def unit_widths(t, mask):
    """The hidden widths of every selected net of t, in ascending net id."""
    return [list(t.hidden) for k in range(6) if mask >> k & 1]


def _run_units(ts, rows, variant, nan):
    masks, acts = UNIT_MASKS[variant[0]], variant[1]
    ins = _inputs(ts, rows, nan)
    ios, outs = [], []
    for t, n, mask, x in zip(ts, rows, masks, ins):
        units = sum(sum(w) for w in unit_widths(t, mask))
        mom = np.full((len(_lib.UNIT_FIELDS) * units,), 7.0, np.float64)
        h = np.full((n * units,), 7.0, np.float32) if acts and n else None
        outs.append((mom, h))
        ios.append(_lib.SacUnitsIO(x and x[0].ctypes.data, x and x[1].ctypes.data, mask, 0, mom.ctypes.data,
                                   None if h is None else h.ctypes.data))
    R = len(ts)
    _lib.check(_lib.load().sac_unit_moments_general_many(_handles(ts), R, (C.c_int32 * R)(*rows), (_lib.SacUnitsIO * R)(*ios)),
               "sac_unit_moments_general_many")
    got = {}
    for m, (mom, h) in enumerate(outs):
        if rows[m] == 0:
            continue
        got[f"m{m}.moments"] = mom
        if h is not None:                                          # per selected net and hidden layer (n, N_l), row-major
            off = 0
            for s, widths in enumerate(unit_widths(ts[m], masks[m])):
                for l, N in enumerate(widths):
                    got[f"m{m}.h{s}_{l}"] = h[off:off + rows[m] * N].reshape(rows[m], N).copy()
                    off += rows[m] * N
    return got


def _run_session(ts, nan):
    """One sac_gactor session over the three members and SESSION_TICKS: the actions of every tick."""
    lib, R, cap = _lib.load(), len(ts), 17
    a = C.c_void_p()
    _lib.check(lib.sac_gactor_create(C.byref(a), _handles(ts), R, (C.c_int32 * R)(*[cap] * R)), "sac_gactor_create")
    try:
        views = []
        for m, t in enumerate(ts):
            p = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
            _lib.check(lib.sac_gactor_arrays(a, m, *[C.byref(x) for x in p]), "sac_gactor_arrays")
            views.append([np.ctypeslib.as_array((ct * (cap * cols)).from_address(x.value)).reshape(cap, cols)
                          for x, ct, cols in zip(p, (C.c_double, C.c_float, C.c_float), (t.obs_dim, t.act_dim, t.act_dim))])
        got = {}
        for k, (rows, det) in enumerate(SESSION_TICKS):
            for m, (t, n) in enumerate(zip(ts, rows)):
                rs = np.random.RandomState(200 + 10 * k + m)
                obs, eps, act = views[m]
                obs[:n], eps[:n] = rs.normal(0, 0.4, (n, t.obs_dim)), rs.standard_normal((n, t.act_dim)).astype(np.float32)
                if nan and m == NAN_MEMBER and n > NAN_ROW:
                    obs[NAN_ROW, 2] = np.nan
                act[...] = 7.0
            _lib.check(lib.sac_gactor_act(a, (C.c_int32 * R)(*rows), (C.c_int32 * R)(*det)), "sac_gactor_act")
            got.update((f"t{k}.m{m}.act", views[m][2].copy()) for m in range(R))       # (the rows behind n keep the 7)
        return got
    finally:
        lib.sac_gactor_destroy(a)


def run(members, case):
    """One grouped call (a session: its ticks) of `case` on make_all_members(): an ordered dict name -> array of
    everything the call returned for the members with rows."""
    family, rows, variant, nan = case
    if family == "act":
        return _run_act(members, rows, variant, nan)
    if family == "q":
        return _run_q(members, rows, variant, nan)
    if family == "units":
        return _run_units(members, rows, variant, nan)
    if family == "session":
        return _run_session(members, nan)
    return _run_eval(members, family, rows, variant, nan)
