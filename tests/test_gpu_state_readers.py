"""GPU: every reader (and writer) of trainer state behind fused steps that nobody has settled.

The stepwise loop -- random_batch(); train() on device batches, nobody waiting -- leaves up to 47 fused steps unverified.
Here one of them gives up (SAC_FUSED_TEST_STALL: the n-th fused launch ends in the kernels' own orderly time-out, the
launch returns normally), and then state leaves the library through each of its doors with NO sac_sync in front:
state_dict, save_checkpoint, pickling, get_snapshot, the host acting mirror, a handle rebuilt for another batch size,
load_state_dict / sac_set_scalars, sac_trainer_set_xcd_mask, and a state read after the buffer was dropped.  A
four-launch twin with identical parameters, buffer and generator runs the same script; every comparison is bit for bit.

stall_at == steps: the last step gives up, nothing behind it can have noticed -- is_fused() right before the read and not
after it proves that the reader did the settling.  stall_at == steps - 3: lost steps are queued behind the one that gave up.

Also here, without a stall: every network holder pickles its trained weights, and a resumed run continues on the saved
run's noise stream whatever noise_seed the loading trainer was built with."""
import copy
import gc
import pickle

import numpy as np
import pytest

from robosuite_benchmark_amd import EnvReplayBuffer, FlattenMlp, TanhGaussianPolicy, TanhMlpPolicy, _lib
from robosuite_benchmark_amd import checkpoint as ck
from robosuite_benchmark_amd import group_checkpoint as gc_
from tests.helpers import (_td3_pair_of_hip, filled_buffer, is_td3, make_pair, make_td3_pair, pair_of_hip,
                           synth_transitions)

pytestmark = pytest.mark.gpu

N_ROWS = 3000
# label -> (algo, (O, A, B), steps).  TD3: an odd step count, so the lost steps hold a policy step and adam_t_pi must come
# back right.  Kind 4 (the chained launch with the backward blocks inside) exists only at batch 1024.
PATHS = {"sac-10x3x32": ("sac", (10, 3, 32), 20), "sac-42x7x128": ("sac", (42, 7, 128), 20),
         "td3-10x3x32": ("td3", (10, 3, 32), 21), "sac-kind4": ("kind4", (46, 7, 1024), 8)}
SMALL = ("sac-10x3x32", "td3-10x3x32")


def _pair(label, stall, monkeypatch):
    """(fused trainer whose launch `stall` gives up -- 0: none does --, its four-launch twin, two equal buffers, B, steps)"""
    algo, (O, A, B), steps = PATHS[label]
    env = dict(SAC_FUSED_TEST_STALL=stall) if stall else {}
    if algo == "kind4":
        from tests.test_gpu_large_batch import _chain_pair
        fused, plain = _chain_pair(O, A, B, monkeypatch, **env)
        assert fused.fused_mode() == 4 and plain.fused_mode() == 2
    else:
        fused, plain = (pair_of_hip if algo == "sac" else _td3_pair_of_hip)(O, A, B, seed=4, noise_seed=9, **env)
        assert fused.fused_mode() == 1 and plain.fused_mode() == 0
    return fused, plain, [filled_buffer(N_ROWS, O, A, 8), filled_buffer(N_ROWS, O, A, 8)], B, steps


def _on_fused(t):
    return t.fused_mode() in (1, 4)


def _script(t, buf, B, steps, at=None):
    """One train() that returns diagnostics, then steps - 1 device-batch steps with nobody waiting (at: (k, f) -- f() is
    called in front of step k)."""
    assert t.train(buf.random_batch(B)) is not None
    for k in range(1, steps):
        if at is not None and at[0] == k:
            at[1]()
        batch = buf.random_batch(B)
        assert batch.on_device
        assert t.train(batch) is None


def _state(t):
    st = t.state_dict()
    return ([(f"params {n}", st["params"][n]) for n in t.NETS]
            + [(f"adam {'mv'[i]} {n}", st["opt"][n][i]) for n in ("policy", "qf1", "qf2") for i in (0, 1)]
            + [("scalars", st["scalars"])])


def _same(a, b, what):
    assert [k for k, _ in a] == [k for k, _ in b]
    for (k, x), (_, y) in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}: {k} differs in {int(np.sum(x != y))} of {x.size} elements"


def _same_rng(ba, bb, what):
    (ka, pa), (kb, pb) = ba.rng_state(), bb.rng_state()
    assert pa == pb and np.array_equal(ka, kb), what


def _unsettled(label, stall, monkeypatch):
    """Both trainers behind the script; the fused one has a step that gave up (the last one for stall 0, the third before
    it for -3) and nobody has looked."""
    fused, plain, bufs, B, steps = _pair(label, PATHS[label][2] + stall, monkeypatch)
    _script(fused, bufs[0], B, steps)
    _script(plain, bufs[1], B, steps)
    return fused, plain, bufs, B, steps


class _Settles:
    """Around the reader under test: with the stall on the last step (0), the trainer is still on its fused step in front
    of the reader -- the host has not noticed -- and on the fall-back behind it: the reader settled it."""

    def __init__(self, fused, stall_at):
        self.fused, self.check = fused, stall_at == 0

    def __enter__(self):
        if self.check:
            assert _on_fused(self.fused), "the host noticed the give-up before the reader ran: the test reads a settled trainer"

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None and self.check:
            assert not _on_fused(self.fused), "the reader did not settle the trainer"


# stall_at relative to the script's last step: 0 = the last step, -3 = three lost steps are queued behind it
STALLS = (0, -3)
READ_CASES = [(label, s) for label in PATHS for s in STALLS]
COPY_CASES = [(label, s) for label in PATHS if label != "sac-kind4" for s in STALLS]
_ids = lambda cases: [f"{label}-last{s or ''}" for label, s in cases]      # noqa: E731


@pytest.mark.parametrize("label,stall", READ_CASES, ids=_ids(READ_CASES))
def test_state_dict_behind_a_give_up(label, stall, monkeypatch):
    fused, plain, bufs, B, steps = _unsettled(label, stall, monkeypatch)
    with _Settles(fused, stall):
        got = _state(fused)
    _same(got, _state(plain), "state_dict")
    assert got[-1][1][4] == steps and got[-1][1][3] == steps
    if is_td3(fused):
        assert got[-1][1][0] == (steps + 1) // 2            # the policy's own optimizer steps (every second step)
    _same_rng(bufs[0], bufs[1], "generator behind the script")
    la, lb = fused.train_loop(bufs[0], 5, batch_size=B)[1], plain.train_loop(bufs[1], 5, batch_size=B)[1]
    assert np.array_equal(la, lb)
    _same(_state(fused), _state(plain), "5 loop steps later")
    _same_rng(bufs[0], bufs[1], "generator 5 loop steps later")


def _fresh(label, seed):
    """An undisturbed trainer of the path's algorithm and shape with OTHER initial weights, and an empty buffer."""
    algo, (O, A, B), _ = PATHS[label]
    fresh = (make_pair if algo == "sac" else make_td3_pair)(O, A, B, seed=seed, noise_seed=9)[1]
    return fresh, EnvReplayBuffer(N_ROWS, obs_dim=O, action_dim=A, numpy_global_stream=False)


@pytest.mark.parametrize("label,stall", COPY_CASES, ids=_ids(COPY_CASES))
def test_save_checkpoint_behind_a_give_up(label, stall, monkeypatch, tmp_path):
    fused, plain, bufs, B, steps = _unsettled(label, stall, monkeypatch)
    with _Settles(fused, stall):
        ck.save_checkpoint(str(tmp_path / "ck"), fused, bufs[0])
    resumed, rbuf = _fresh(label, seed=77)
    ck.load_checkpoint(str(tmp_path / "ck"), resumed, rbuf)
    la, lb = resumed.train_loop(rbuf, 10, batch_size=B)[1], plain.train_loop(bufs[1], 10, batch_size=B)[1]
    assert np.array_equal(la, lb)
    _same(_state(resumed), _state(plain), "resumed from a checkpoint taken with no sync")
    assert _state(resumed)[-1][1][4] == steps + 10
    _same_rng(rbuf, bufs[1], "generator of the resumed run")


@pytest.mark.parametrize("how", ["pickle", "deepcopy"])
@pytest.mark.parametrize("label,stall", COPY_CASES, ids=_ids(COPY_CASES))
def test_a_copied_trainer_behind_a_give_up(label, stall, how, monkeypatch):
    fused, plain, bufs, B, steps = _unsettled(label, stall, monkeypatch)
    with _Settles(fused, stall):
        twin = pickle.loads(pickle.dumps(fused)) if how == "pickle" else copy.deepcopy(fused)
    assert twin._h is None and twin is not fused
    twin.train_loop(bufs[0], 5, batch_size=B)
    plain.train_loop(bufs[1], 5, batch_size=B)
    _same(_state(twin), _state(plain), f"{how} of an unsettled trainer, 5 steps later")
    assert _state(twin)[-1][1][4] == steps + 5


@pytest.mark.parametrize("label", SMALL)
def test_get_snapshot_behind_a_give_up(label, monkeypatch):
    fused, plain, _, _, _ = _unsettled(label, 0, monkeypatch)
    with _Settles(fused, 0):
        snap = fused.get_snapshot()
    names = list(fused.NETS) + (["trained_policy"] if is_td3(fused) else [])
    assert set(names) <= set(snap)
    for name in names:
        want = plain._get_params("policy" if name == "trained_policy" else name)
        assert np.array_equal(snap[name].flat().view(np.uint32), want.view(np.uint32)), name


@pytest.mark.parametrize("entry", ["policy_act", "get_action"])
@pytest.mark.parametrize("label", SMALL)
def test_host_acting_behind_a_give_up(label, entry, monkeypatch):
    fused, plain, _, _, _ = _unsettled(label, 0, monkeypatch)
    obs = np.random.RandomState(5).normal(0, 0.4, (4, fused.obs_dim)).astype(np.float32)

    def act(t):
        if entry == "policy_act":
            return t.policy_act(obs, True, None)
        kw = {} if is_td3(t) else dict(deterministic=True)
        return np.stack([t.policy.get_action(o, **kw)[0] for o in obs])

    with _Settles(fused, 0):
        got = act(fused)
    want = act(plain)
    assert got.shape == (4, fused.act_dim) and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("label", SMALL)
def test_a_host_batch_of_another_size_behind_a_give_up(label, monkeypatch):
    """train() on 48 rows rebuilds the handle (made for 32) from the exported state.  Both new handles are created with
    the environment as the pair's constructor restored it; fused and four-launch agree bit for bit anyway."""
    fused, plain, _, B, steps = _unsettled(label, 0, monkeypatch)
    O, A = fused.obs_dim, fused.act_dim
    obs, act, rew, term, nobs = synth_transitions(48, O, A, seed=21, term_frac=0.1)
    batch = dict(observations=obs, actions=act, rewards=rew, terminals=term.astype(np.float32), next_observations=nobs)
    assert _on_fused(fused)
    da = fused.train(batch)
    db = plain.train(batch)
    assert fused._batch == plain._batch == 48 and np.array_equal(da, db)
    _same(_state(fused), _state(plain), "one step on the rebuilt handle")
    assert _state(fused)[-1][1][4] == steps + 1


@pytest.mark.parametrize("label", SMALL)
def test_load_state_dict_behind_a_give_up(label, monkeypatch):
    """S, the twin's state at step 5, goes into both trainers behind the script: the lost steps must not be re-run on top
    of it."""
    fused, plain, bufs, B, steps = _pair(label, PATHS[label][2], monkeypatch)
    S = {}
    _script(fused, bufs[0], B, steps)
    _script(plain, bufs[1], B, steps, at=(5, lambda: S.update(plain.state_dict())))
    assert S["scalars"][4] == 5
    with _Settles(fused, 0):
        fused.load_state_dict(S)
    plain.load_state_dict(S)
    la, lb = fused.train_loop(bufs[0], 6, batch_size=B)[1], plain.train_loop(bufs[1], 6, batch_size=B)[1]
    assert np.array_equal(la, lb)
    _same(_state(fused), _state(plain), "6 loop steps on the loaded state")
    assert _state(fused)[-1][1][4] == 11


def test_set_scalars_alone_behind_a_give_up(monkeypatch):
    """sac_set_scalars by itself (as tests/test_gpu_noise_stream._set_step moves the step counter): the counters it
    writes are the ones the next steps run at, not the ones a late recovery rolls back from."""
    fused, plain, bufs, B, steps = _unsettled("sac-10x3x32", 0, monkeypatch)
    sc = np.ascontiguousarray(plain.state_dict()["scalars"], np.float64)
    sc[4] = 100.0
    with _Settles(fused, 0):
        _lib.check(fused._lib.sac_set_scalars(fused._h, _lib.ptr(sc)), "sac_set_scalars")
    _lib.check(plain._lib.sac_set_scalars(plain._h, _lib.ptr(sc)), "sac_set_scalars")
    fused.train_loop(bufs[0], 6, batch_size=B)
    plain.train_loop(bufs[1], 6, batch_size=B)
    _same(_state(fused), _state(plain), "6 loop steps behind sac_set_scalars")
    assert _state(fused)[-1][1][4] == 106 and _state(fused)[-1][1][3] == steps + 6


@pytest.mark.parametrize("label", SMALL)
def test_set_xcd_mask_behind_a_give_up(label, monkeypatch):
    fused, plain, bufs, B, steps = _unsettled(label, 0, monkeypatch)
    with _Settles(fused, 0):
        assert fused._lib.sac_trainer_set_xcd_mask(fused._h, 0xff) == 0, _lib.last_error()
    _same(_state(fused), _state(plain), "behind sac_trainer_set_xcd_mask")
    for t, b in ((fused, bufs[0]), (plain, bufs[1])):
        for _ in range(5):
            assert t.train(b.random_batch(B)) is None
        assert t._lib.sac_sync(t._h) == 0, _lib.last_error()
    _same(_state(fused), _state(plain), "5 device-batch steps later")
    assert _state(fused)[-1][1][4] == steps + 5


@pytest.mark.parametrize("label", SMALL)
def test_state_dict_after_the_buffer_was_dropped(label, monkeypatch):
    """The lost step is on record by buffer and slot: the trainer keeps the buffer alive until it has settled."""
    fused, plain, bufs, B, steps = _unsettled(label, 0, monkeypatch)
    want = _state(plain)
    del bufs[0]
    gc.collect()
    with _Settles(fused, 0):
        got = _state(fused)
    _same(got, want, "state_dict after del buf")
    assert fused._stepped_buffers == ()


@pytest.mark.parametrize("label", list(PATHS))
def test_control_no_give_up(label, monkeypatch):
    """The same script with no stall: the readers change nothing about an undisturbed run."""
    fused, plain, bufs, B, steps = _pair(label, 0, monkeypatch)
    _script(fused, bufs[0], B, steps)
    _script(plain, bufs[1], B, steps)
    _same(_state(fused), _state(plain), "state_dict")
    assert _on_fused(fused)
    _same_rng(bufs[0], bufs[1], "generator")
    if label == "sac-kind4":
        return
    a, b = pickle.loads(pickle.dumps(fused)), copy.deepcopy(fused)
    bbuf = filled_buffer(N_ROWS, fused.obs_dim, fused.act_dim, 8)         # the deep copy's: bufs[0] as it stands now
    bbuf.set_rng_state(*bufs[0].rng_state())
    a.train_loop(bufs[0], 5, batch_size=B)
    b.train_loop(bbuf, 5, batch_size=B)
    plain.train_loop(bufs[1], 5, batch_size=B)
    _same(_state(a), _state(plain), "pickled copy, 5 steps later")
    _same(_state(b), _state(plain), "deep copy, 5 steps later")


# ---- holders other than the policy pickle their trained weights ------------------------------------------------------
def _host_forward_tanh_mlp(flat, hidden, O, A, obs):
    net = TanhMlpPolicy(list(hidden), A, O)
    net.load_flat(flat)
    return net.get_actions(obs)


@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_every_holder_pickles_its_trained_weights(algo):
    O, A, B = 10, 3, 32
    t = (pair_of_hip if algo == "sac" else _td3_pair_of_hip)(O, A, B, seed=4, noise_seed=9)[0]
    init = {name: getattr(t, name).flat().copy() for name in t.NETS}
    t.train_loop(filled_buffer(N_ROWS, O, A, 8), 7, batch_size=B)
    obs = np.random.RandomState(5).normal(0, 0.4, (4, O)).astype(np.float32)
    if algo == "td3":            # (first: nothing has synced this holder yet)
        want = _host_forward_tanh_mlp(t._get_params("target_policy"), t.target_policy.hidden_sizes, O, A, obs)
        got = t.target_policy.get_actions(obs)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert not np.array_equal(got, _host_forward_tanh_mlp(init["target_policy"], t.target_policy.hidden_sizes, O, A, obs))
    for name in t.NETS:
        for how, copy_of in (("pickle", lambda n: pickle.loads(pickle.dumps(n))), ("deepcopy", copy.deepcopy)):
            holder = getattr(t, name)
            holder.load_flat(init[name])             # the host arrays as before any sync: stale
            assert holder._trainer is t
            loaded = copy_of(holder)
            want = t._get_params(name)
            assert np.array_equal(loaded.flat().view(np.uint32), want.view(np.uint32)), (name, how)
            assert not np.array_equal(loaded.flat(), init[name]), (name, how, "the initial weights")
            assert loaded._trainer is None and loaded is not holder
            assert isinstance(loaded, (FlattenMlp, TanhGaussianPolicy, TanhMlpPolicy))


# ---- a resumed run continues on the SAVED noise stream ---------------------------------------------------------------
S_SEED, K_SAVED = 0x1234_0000_0ABC, 13
O_, A_, B_ = 10, 3, 32


def _make(algo, noise_seed):
    from tests.test_gpu_noise_stream import _zero_head_sac, _zero_head_td3
    return (_zero_head_sac if algo == "sac" else _zero_head_td3)(O_, A_, B_, (256, 256), noise_seed)


def _check_draws(algo, t, step, what):
    from tests.test_gpu_noise_stream import check_sac_step, check_td3_step
    if algo == "sac":
        check_sac_step(t, S_SEED, step, B_, A_, False, what)
    else:
        check_td3_step(t, S_SEED, step, B_, A_, what)


def _straight_and_saved(algo, save):
    t, buf = _make(algo, S_SEED), filled_buffer(N_ROWS, O_, A_, 8)
    t.train_loop(buf, K_SAVED, batch_size=B_)
    save(t, buf)
    t.train_loop(buf, 10, batch_size=B_)
    return _state(t), buf


def _resume_and_check(algo, load, loading, want, sbuf):
    rbuf = EnvReplayBuffer(N_ROWS, obs_dim=O_, action_dim=A_, numpy_global_stream=False)
    load(loading, rbuf)
    assert loading.noise_seed == S_SEED and loading._h is not None
    loading.train_loop(rbuf, 1, batch_size=B_)
    _check_draws(algo, loading, K_SAVED, f"{algo} resumed at step {K_SAVED}")
    loading.train_loop(rbuf, 9, batch_size=B_)
    _same(_state(loading), want, "10 steps behind the resume against the straight run")
    _same_rng(rbuf, sbuf, "generator")


LOADERS = [("sac", "none"), ("sac", "other"), ("sac", "no handle"), ("td3", "none")]


@pytest.mark.parametrize("algo,built", LOADERS, ids=[f"{a}-{b.replace(' ', '-')}" for a, b in LOADERS])
def test_load_checkpoint_adopts_the_saved_noise_seed(algo, built, tmp_path):
    """The loading trainer was built with noise_seed=None (the reference's way: a process-derived value), or with another
    seed and a live handle, or has no handle yet."""
    d = str(tmp_path / "ck")
    want, sbuf = _straight_and_saved(algo, lambda t, b: ck.save_checkpoint(d, t, b))
    loading = _make(algo, None if built == "none" else S_SEED ^ (1 << 40))
    assert loading.noise_seed != S_SEED and loading._h is not None
    if built == "no handle":
        loading._destroy()
    _resume_and_check(algo, lambda t, b: ck.load_checkpoint(d, t, b), loading, want, sbuf)


def test_load_group_member_adopts_the_saved_noise_seed(tmp_path):
    d = str(tmp_path / "ck")
    variant = dict(policy_kwargs=dict(hidden_sizes=[256, 256]), qf_kwargs=dict(hidden_sizes=[256, 256]))

    def save(t, b):
        gc_.GroupCheckpoint(d, 512).save([t], [b], [gc_.member_identity("s0", 0, variant, t)], [dict(epoch=0)])

    want, sbuf = _straight_and_saved("sac", save)
    loading = _make("sac", None)
    assert loading.noise_seed != S_SEED
    _resume_and_check("sac", lambda t, b: gc_.load_group_member(d, 0, t, b), loading, want, sbuf)
