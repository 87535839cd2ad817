"""GPU: per-tensor statistics of parameters, Adam moments and target gaps on the device -- sac_param_tensors,
sac_param_moments / sac_param_moments_many (k_param_moments and k_param_finish, csrc/sac_params.h),
SACTrainer.param_moments / group.param_moments_many over them, and the drivers' param_diagnostics.

There is NO tolerance: a record is compared as bytes with infer.param_moments_reference of the flat vectors that
sac_get_params and sac_get_opt_state return after the call (tests/param_reference.expected_moments), for both step
families and both algorithms, fresh and behind every path that writes the state; grouped == solo == any subset of nets
== any flags; constructed states are exact; refusals write nothing; the call leaves no trace.  (A record that holds a
NaN -- only the planted ones do -- is compared by value, a NaN equal to a NaN: IEEE 754 leaves a computed NaN's payload
open.)"""
import ctypes as C

import numpy as np
import pytest

from robosuite_benchmark_amd import (ArchSACTrainerGroup, EnvReplayBuffer, FlattenMlp, SACTrainer, TanhGaussianPolicy,
                                     TanhMlpPolicy, TD3Trainer, _lib, driver, infer)
from robosuite_benchmark_amd.checkpoint import load_checkpoint, save_checkpoint
from robosuite_benchmark_amd.group import param_moments_many, param_moments_reference, param_statistics
from robosuite_benchmark_amd.variant import default_variant
from tests.helpers import filled_buffer, full_state, synth_transitions
from tests.param_reference import CH, F, expected_moments, same_bytes, same_values

pytestmark = pytest.mark.gpu
B = 32

# name -> (algorithm, policy hidden, Q hidden (None: the policy's), O, A, the step family expected, SAC_GENERAL)
SHAPES = {
    "fused 1-1 (16,16)": ("sac", (16, 16), None, 1, 1, False, False),
    "fused 42-7 (256,256)": ("sac", (256, 256), None, 42, 7, False, False),
    "fused 379-6 (256,256)": ("sac", (256, 256), None, 379, 6, False, False),          # action columns at KP = 384
    "fused 46-16 (240,256)": ("sac", (240, 256), None, 46, 16, False, False),
    "fused (64,32) under (256,256)": ("sac", (64, 32), (256, 256), 42, 7, False, False),
    "fused td3 (240,256)": ("td3", (240, 256), None, 42, 7, False, False),
    "general (1,)": ("sac", (1,), None, 1, 1, True, False),
    "general (16,)": ("sac", (16,), None, 1, 1, True, False),
    "general (300,7,129)": ("sac", (300, 7, 129), None, 42, 7, True, False),
    "general (64,)x7": ("sac", (64,) * 7, None, 42, 7, True, False),
    "general (4096,)": ("sac", (4096,), None, 42, 7, True, False),
    "general (128,128)": ("sac", (128, 128), None, 42, 7, True, True),                  # fc1.weight: exactly CH elements
    "general (129,127)": ("sac", (129, 127), None, 42, 7, True, True),                  # fc1.weight: CH - 1
    "general (512,512)": ("sac", (512, 512), None, 45, 7, True, False),                 # several chunks, a ragged first layer
    "general td3 (300,200,100)": ("td3", (300, 200, 100), None, 17, 5, True, False),
}
assert 128 * 128 == CH and 127 * 129 == CH - 1


def build(algo, hp, hq, O, A, seed=5, **kw):
    rs = np.random.RandomState(seed)
    hq = list(hq or hp)
    qs = [FlattenMlp(hq, 1, O + A, rs=rs) for _ in range(4)]
    if algo == "td3":
        pols = [TanhMlpPolicy(list(hp), A, O, rs=rs) for _ in range(2)]
        return TD3Trainer(policy=pols[0], qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], target_policy=pols[1],
                          batch_size=B, noise_seed=seed, **kw)
    pol = TanhGaussianPolicy(list(hp), O, A, rs=rs)
    return SACTrainer(policy=pol, qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], batch_size=B, noise_seed=seed,
                      **kw)


def fresh(name, monkeypatch=None, seed=5, **kw):
    algo, hp, hq, O, A, general, forced = SHAPES[name]
    if forced:
        monkeypatch.setenv("SAC_GENERAL", "1")
    t = build(algo, hp, hq, O, A, seed, **kw)
    assert t.runs_general_step() == general, name
    return t


def steps(t, n, seed=50):
    o, a, r, d, no = synth_transitions(B, t.obs_dim, t.act_dim, seed=seed)
    for _ in range(n):
        t.train(dict(observations=o, actions=a, rewards=r, terminals=d, next_observations=no))


def check(t, nets=None, opt=True, gap=True, what=""):
    """param_moments(route="device") against the reference of what the getters return AFTER the call, as bytes."""
    got = t.param_moments(nets=nets, opt=opt, gap=gap)
    want = expected_moments(t, list(got), opt, gap)
    assert list(got) == (list(t.NETS) if nets is None else list(nets))
    for net in got:
        assert got[net].shape == (len(t.param_tensors(net)), 9) and got[net].dtype == np.float64
        assert not np.any(np.isnan(got[net])), (what, net)
        assert same_bytes(got[net], want[net]), (what, net, got[net] - want[net])
    return got


def tensors_c(t, net):
    lib = _lib.load()
    sizes = (C.c_int64 * _lib.PARAM_MAX_TENSORS)()
    n = lib.sac_param_tensors(t._h, net, sizes)
    assert n == lib.sac_param_tensors(t._h, net, None)
    return list(sizes[:n])


# ---- 1. every shape, fresh and behind 20 steps ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_records_are_the_reference_of_the_getters(name, monkeypatch):
    t = fresh(name, monkeypatch)
    for net, k in t.NETS.items():
        assert tensors_c(t, k) == [int(np.prod(s)) for _, s in t.param_tensors(net)], net
        assert sum(tensors_c(t, k)) == int(_lib.load().sac_param_count(t._h, k))
    got = check(t, what="fresh")
    assert all(np.all(got[n][:, 4:8] == 0.0) for n in got)                  # fresh Adam moments, and none on targets
    assert got["qf1"][0, F["gap_sumsq"]] > 0 and np.all(got["target_qf1"][:, 8] == 0.0)
    assert np.all(got["policy"][:, 8] == 0.0) == ("target_policy" not in t.NETS)
    steps(t, 20)
    got = check(t, what="20 steps")
    for net in ("policy", "qf1", "qf2"):
        assert np.all(got[net][:, F["m_sumsq"]] > 0) and np.all(got[net][:, F["v_max"]] > 0), net
    assert np.all(got["target_qf2"][:, 4:] == 0.0)
    # the host route of the same trainer: the same bytes
    host = t.param_moments(route="host")
    assert all(same_bytes(host[n], got[n]) for n in got)


# ---- 2. behind every path that writes the state -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused 42-7 (256,256)", "fused td3 (240,256)", "general (300,7,129)",
                                  "general td3 (300,200,100)"])
def test_behind_every_path_that_moves_the_state(name, tmp_path):
    t, u = fresh(name, seed=7), fresh(name, seed=8)
    O, A = t.obs_dim, t.act_dim
    buf = filled_buffer(1500, O, A, 31)
    last = check(t, what="fresh")

    def moved(last, what):
        now = check(t, what=what)
        assert not same_bytes(now["qf1"], last["qf1"]), what
        return now

    t.train_loop(buf, 6, batch_size=B)
    last = moved(last, "train_loop")
    for _ in range(5):                                   # device batches, stepwise, nothing read and no sac_sync in front
        t.train(buf.random_batch(B))
    last = moved(last, "device-batch steps")
    for net in t.NETS:
        t._set_params(net, u.state_dict()["params"][net])
    last = moved(last, "sac_set_params")
    u.train_loop(buf, 4, batch_size=B)
    t.load_state_dict(u.state_dict())
    last = moved(last, "load_state_dict")
    assert all(same_bytes(a, b) for a, b in zip(last.values(), check(u, what="the donor").values()))
    t.train_loop(buf, 3, batch_size=B)
    save_checkpoint(str(tmp_path / "ck"), t, buf, dict(epoch=0))
    w, wbuf = fresh(name, seed=9), EnvReplayBuffer(1500, obs_dim=O, action_dim=A)
    load_checkpoint(str(tmp_path / "ck"), w, wbuf)
    resumed = check(w, what="resumed")
    assert all(same_bytes(a, b) for a, b in zip(resumed.values(), check(t, what="saved").values()))
    w.train_loop(wbuf, 3, batch_size=B)
    check(w, what="resumed and trained")


# ---- 3. grouped == solo == any subset of nets == any flags -------------------------------------------------------------------
def test_grouped_is_solo_under_any_mask_and_flags(monkeypatch):
    names = [n for n in SHAPES if not SHAPES[n][6]]
    names = (names + names)[:16]
    ts = [fresh(n, seed=20 + i) for i, n in enumerate(names)]
    assert {t.runs_general_step() for t in ts} == {True, False} and {"target_policy" in t.NETS for t in ts} == {True, False}
    for t in ts:
        steps(t, 3, seed=60)
    solo = [check(t, what="solo") for t in ts]
    full = param_moments_many(ts)
    for i, (g, s) in enumerate(zip(full, solo)):
        assert list(g) == list(s) and all(same_bytes(g[n], s[n]) for n in s), names[i]
    # a group's own method, the members in another order
    via = ArchSACTrainerGroup([t for t in ts if "target_policy" not in t.NETS and t.runs_general_step()][::-1])
    for t, g in zip(via.trainers, via.param_moments_many()):
        assert all(same_bytes(g[n], solo[ts.index(t)][n]) for n in g)
    # every flags value and a walk through the masks: a member's selection differs from its neighbours'
    for flags in range(4):
        opt, gap = bool(flags & 1), bool(flags & 2)
        sel = []
        for i, t in enumerate(ts):
            all_nets = list(t.NETS)
            mask = (7 * i + 5 * flags) % (2 ** len(all_nets) - 1) + 1
            sel.append([n for k, n in enumerate(all_nets) if mask >> k & 1][::-1] if i != 3 else None)
        got = param_moments_many(ts, sel, opt=opt, gap=gap)
        assert got[3] is None
        for i, (t, g) in enumerate(zip(ts, got)):
            if g is None:
                continue
            assert list(g) == sel[i]
            one = t.param_moments(nets=sel[i], opt=opt, gap=gap)
            for n in g:
                want = solo[i][n].copy()
                if not opt:
                    want[:, 4:8] = 0.0
                if not gap:
                    want[:, 8] = 0.0
                assert same_bytes(g[n], want) and same_bytes(one[n], want), (names[i], n, flags)


# ---- 4. constructed states ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused 46-16 (240,256)", "general (300,7,129)"])
def test_planted_non_finite_values(name):
    t = fresh(name, seed=11)
    steps(t, 2)
    clean = check(t, what="clean")
    shapes = t.param_tensors("policy")
    names = [n for n, _ in shapes]
    starts = np.concatenate([[0], np.cumsum([int(np.prod(s)) for _, s in shapes])])
    flat0 = t._get_params("policy")
    plant = [("fc0.weight", 17, np.nan), ("fc1.bias", 3, np.inf), ("last_fc_log_std.weight", 5, -np.inf),
             ("last_fc_log_std.bias", t.act_dim - 1, np.nan), ("last_fc.weight", 0, np.inf)]
    for tensor, e, bad in plant:
        flat = flat0.copy()
        j = names.index(tensor)
        flat[starts[j] + e] = bad
        t._set_params("policy", flat)
        got = t.param_moments()
        want = expected_moments(t, list(got))
        for net in got:
            assert same_values(got[net], want[net]), (tensor, net)
            rows = [r for r in range(len(got[net])) if not (net == "policy" and r == j)]
            assert same_bytes(got[net][rows], clean[net][rows]), (tensor, net)           # the other tensors do not move
        rec = got["policy"][j]
        assert rec[F["nonfinite"]] == 1.0 and same_bytes(rec[4:8], clean["policy"][j][4:8])
        if np.isnan(bad):
            assert np.isnan(rec[F["absmax"]]) and np.isnan(rec[F["sum"]])
        else:
            assert rec[F["absmax"]] == np.inf and rec[F["sum"]] == bad
        assert infer.param_statistics(got, {n: [int(np.prod(s)) for _, s in t.param_tensors(n)] for n in got})["Non Finite"] == 1.0
    # three at once in one tensor, in two chunks where it has them
    flat = flat0.copy()
    j = names.index("fc1.weight")
    E = int(starts[j + 1] - starts[j])
    for e, bad in ((0, np.nan), (E // 2, np.inf), (E - 1, -np.inf)):
        flat[starts[j] + e] = bad
    t._set_params("policy", flat)
    rec = t.param_moments(nets=("policy",))["policy"][j]
    assert rec[F["nonfinite"]] == 3.0 and np.isnan(rec[F["absmax"]])
    t._set_params("policy", flat0)
    assert all(same_bytes(a, b) for a, b in zip(check(t, what="restored").values(), clean.values()))


@pytest.mark.parametrize("name", ["fused 379-6 (256,256)", "fused td3 (240,256)", "general (512,512)",
                                  "general td3 (300,200,100)"])
def test_constructed_target_gaps(name):
    t = fresh(name, seed=12)
    steps(t, 2)
    pairs = [(n, infer.param_target(t, n)) for n in t.NETS if infer.param_target(t, n)]
    assert len(pairs) == (3 if "target_policy" in t.NETS else 2)
    for net, target in pairs:
        t._set_params(target, t._get_params(net))
    got = check(t, what="targets equal")
    for net, _ in pairs:
        assert np.all(got[net][:, F["gap_sumsq"]] == 0.0) and not np.any(np.signbit(got[net][:, F["gap_sumsq"]]))
    # one element of one tensor moved by a float32 amount: that amount squared, exactly, and in that tensor alone
    d = np.float32(2.0 ** -9)
    for net, target in pairs:
        shapes = t.param_tensors(net)
        starts = np.concatenate([[0], np.cumsum([int(np.prod(s)) for _, s in shapes])])
        for j in (0, len(shapes) - 2, len(shapes) - 1):          # first weight (a Q net's: an action column), last weight, last bias
            flat = t._get_params(net)
            e = int(starts[j + 1]) - 1
            tg = flat.copy()
            flat[e] = np.float32(0.75)
            tg[e] = np.float32(0.75) + d
            t._set_params(net, flat)
            t._set_params(target, tg)
            got = check(t, nets=(net, target), what=(net, j))
            want = np.zeros(len(shapes))
            want[j] = float(d) * float(d)
            assert np.array_equal(got[net][:, F["gap_sumsq"]], want), (net, j)
            t._set_params(target, flat)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def params_c(ts, ios):
    R = len(ts)
    return _lib.load().sac_param_moments_many((C.c_void_p * R)(*[None if t is None else t._h.value for t in ts]), R,
                                              (_lib.SacParamsIO * R)(*ios))


def test_refusals_write_nothing():
    lib = _lib.load()
    a, g, td3 = fresh("fused 42-7 (256,256)", seed=1), fresh("general (16,)", seed=1), fresh("fused td3 (240,256)", seed=1)
    buf = filled_buffer(500, 42, 7, 2)
    a.train_loop(buf, 3, batch_size=B)
    state = full_state(a, buf)
    mom, mom2 = np.full(9 * 18 * 6, 3.0), np.full(9 * 18 * 6, 3.0)

    def io(m, nets=0x1f, flags=3):
        return _lib.SacParamsIO(nets, flags, None if m is None else m.ctypes.data)

    def refused(rc, what):
        assert rc < 0 and what in _lib.last_error(), (rc, what, _lib.last_error())
        assert np.all(mom == 3.0) and np.all(mom2 == 3.0), what
        for x, y in zip(full_state(a, buf), state):
            assert np.array_equal(x, y), what

    refused(params_c([a, g], [io(mom, 0), io(mom2)]), "nets")
    refused(params_c([a, g], [io(mom), io(mom2, 64)]), "nets")
    refused(params_c([a, g], [io(mom, 1 << 5), io(mom2)]), "only a TD3 trainer")
    refused(params_c([g, a], [io(mom2, 0x3f), io(mom)]), "only a TD3 trainer")
    refused(params_c([a, g], [io(mom), io(None)]), "null moments")
    refused(params_c([a, g], [io(mom, flags=4), io(mom2)]), "flags")
    refused(params_c([a, a], [io(mom), io(mom2)]), "again")
    refused(params_c([a, None], [io(mom), io(mom2)]), "null")
    refused(lib.sac_param_moments_many((C.c_void_p * 17)(*[a._h.value] * 17), 17, (_lib.SacParamsIO * 17)(*[io(mom)] * 17)),
            "1..16")
    refused(lib.sac_param_moments_many((C.c_void_p * 1)(a._h.value), 0, (_lib.SacParamsIO * 1)(io(mom))), "1..16")
    _lib.check(lib.sac_trainer_set_xcd_mask(g._h, 0x0f), "sac_trainer_set_xcd_mask")
    refused(params_c([a, g], [io(mom), io(mom2)]), "trainer 1 is confined by sac_trainer_set_xcd[_mask]")
    _lib.check(lib.sac_trainer_set_xcd_mask(g._h, 0xff), "sac_trainer_set_xcd_mask")
    refused(lib.sac_param_moments(None, C.byref(io(mom))), "bad arguments")
    refused(lib.sac_param_moments(a._h, None), "bad arguments")
    assert lib.sac_param_tensors(None, 0, None) < 0 and lib.sac_param_tensors(a._h, 5, None) < 0
    assert lib.sac_param_tensors(a._h, -1, None) < 0 and lib.sac_param_tensors(td3._h, 5, None) == 6
    # bit 5 on a TD3 handle is served; a valid call -- both families side by side -- gives the right bytes and no more
    m3 = np.full(9 * 6 + 1, 3.0)
    assert params_c([td3], [io(m3, 1 << 5)]) == 0 and m3[-1] == 3.0
    assert same_bytes(m3[:-1].reshape(6, 9), expected_moments(td3, ["target_policy"])["target_policy"])
    one = io(mom, 0x3)
    assert params_c([a, g], [one, io(mom2, 0x10, 0)]) == 0
    want = expected_moments(a, ["policy", "qf1"])
    assert same_bytes(mom[:9 * 14].reshape(14, 9), np.concatenate([want["policy"], want["qf1"]])) and np.all(mom[9 * 14:] == 3.0)
    assert same_bytes(mom2[:9 * 4].reshape(4, 9), expected_moments(g, ["target_qf2"], False, False)["target_qf2"])
    assert np.all(mom2[9 * 4:] == 3.0)


# ---- 6. the call changes nothing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused 42-7 (256,256)", "fused td3 (240,256)", "general (300,7,129)"])
def test_the_call_leaves_no_trace(name):
    a, b = fresh(name, seed=12), fresh(name, seed=12)
    O, A = a.obs_dim, a.act_dim
    ba, bb = filled_buffer(2000, O, A, 8), filled_buffer(2000, O, A, 8)
    for i in range(3):
        a.train_loop(ba, 2, batch_size=B); b.train_loop(bb, 2, batch_size=B)
        a.param_moments(opt=bool(i % 2))
    for i in range(3):
        a.train(ba.random_batch(B)); b.train(bb.random_batch(B))
        param_moments_many([a], [("qf1", "target_qf1")])
    a.param_moments()
    o, ac, r, d, no = synth_transitions(B, O, A, seed=77)
    batch = dict(observations=o, actions=ac, rewards=r, terminals=d, next_observations=no)
    assert np.array_equal(a.train(batch), b.train(batch))                     # the twin that never called it: the same next step
    for x, y in zip(full_state(a, ba), full_state(b, bb)):
        assert np.array_equal(x, y)
    assert list(a.get_diagnostics().items()) == list(b.get_diagnostics().items())
    for t in (a, b):
        pad = t.debug_fetch("pad_nonzero", 16)
        assert pad.size > 0 and not np.any(pad), (name, pad)


# ---- 7. the drivers ------------------------------------------------------------------------------------------------------------
def variant(hidden=(256, 256), algo="SAC"):
    v = default_variant(agent=algo) if algo != "SAC" else default_variant()
    v["algorithm_kwargs"].update(num_epochs=3, num_eval_steps_per_epoch=40, num_expl_steps_per_train_loop=30,
                                 eval_max_path_length=20, expl_max_path_length=20, min_num_steps_before_training=40,
                                 num_trains_per_train_loop=4, batch_size=32)
    v["replay_buffer_size"] = 500
    for kw in ("policy_kwargs", "qf_kwargs"):
        v[kw]["hidden_sizes"] = list(hidden)
    return v


@pytest.mark.parametrize("algo,hidden", [("SAC", (256, 256)), ("TD3", (256, 256)), ("SAC", (64, 64, 64))])
def test_a_group_run_logs_the_params_block(algo, hidden, monkeypatch):
    O, A, seeds = 11, 3, [3, 4]
    kw = dict(obs_dim=O, action_dim=A, quiet=True, num_epochs=3)
    plain = driver.experiment_group(variant(hidden, algo), seeds, **kw)
    seen = []

    def recording(trainers, *a, **k):
        got = param_moments_many(trainers, *a, **k)
        for t, g in zip(trainers, got):                              # a direct call at the same point: the same bytes
            direct, host = t.param_moments(), t.param_moments(route="host")
            assert all(same_bytes(g[n], direct[n]) and same_bytes(g[n], host[n]) for n in g)
            sizes = {n: [int(np.prod(s)) for _, s in t.param_tensors(n)] for n in g}
            targets = tuple(n for n in g if infer.param_target(t, n))
            seen.append(param_statistics(direct, sizes, targets))
        return got

    monkeypatch.setattr(driver, "param_moments_many", recording)
    rows = driver.experiment_group(variant(hidden, algo), seeds, param_diagnostics=True, **kw)
    assert len(seen) == 3 * len(seeds)                               # ONE call per epoch over all runs
    nets = ("Policy", "QF1", "QF2")
    keys = [f"params/{t} {f}" for t in nets for f in infer.PARAM_FIGURES + (("Target Gap",) if t != "Policy" or algo == "TD3" else ())]
    keys.append("params/Non Finite")
    for i, s in enumerate(seeds):
        assert len(rows[s]) == 3
        for e, (row, want) in enumerate(zip(rows[s], plain[s])):
            cols = list(row)
            j = cols.index(keys[0])
            assert cols[j:j + len(keys)] == keys and cols[j + len(keys)] == "time/data storing (s)"
            assert cols[:j] + cols[j + len(keys):] == list(want)
            assert all(k.startswith("time/") or row[k] == want[k] or (row[k] != row[k] and want[k] != want[k]) for k in want)
            stats = seen[e * len(seeds) + i]
            assert [row[k] for k in keys] == [stats[k[len("params/"):]] for k in keys], (s, e)
            assert row["params/Non Finite"] == 0.0 and row["params/QF1 Weight Norm"] > 0
            assert row["params/QF1 Target Gap"] > 0
            assert (row["params/QF1 Adam V Max"] > 0) == (e > 0)     # (epoch 0 is taken in front of the first training block)
    solo = driver.experiment(variant(hidden, algo), seed=3, param_diagnostics=True, **kw)
    assert [[r[k] for k in keys] for r in solo] == [[r[k] for k in keys] for r in rows[3]]
