"""GPU: the state the step kernels WRITE, and the next step from it.

Every other float64-referenced check of the step starts from state the host uploaded (sac_set_params writes the forward
copy P and the transposed copy PT of each weight side by side).  Here the trainer first runs train_loop(buf, k) -- the
production path: device batches, device noise, the loop's per-step tables -- for k = 1 and k = 6 (SAC's Polyak has run at
steps 0 and 5, TD3's policy steps at 0, 2, 4; the checked step 6 is a policy step, step 1 a critic-only one), and three
legs run on what the kernels left:

  A  no tolerance: the transposed copy as the backward passes and Adam read it (debug_fetch "pt_<net>": weights from PT)
     equals the forward copy every reader, checkpoint and acting kernel sees (state_dict) bit for bit, and no element of
     the padding of P, PT, MT, VT (general step: P, M, V) and of the targets' P is nonzero ("pad_nonzero") -- the
     kernels run narrow layers as 256-wide ones on that.  Again after leg C's step.
  B  no tolerance: a second trainer gets the state through load_state_dict (the host uploads both copies and the moments);
     both take one train(batch, eps=...) on the same host batch and noise.  Diagnostics, gradients, every per-row output
     and the full state afterwards are bit-equal -- so no device state exists that the readers do not show.
  C  tests/helpers.py check_step_f64, the rule unchanged (max(8 x the fp32 oracle's own error, 1e-5) of each tensor's
     scale against the float64 oracle), with both oracles REBUILT from that state (tests/written_state.py
     oracles_from_state): nothing follows two trajectories.  A stale 16 B of one lane in PT moves fc0.weight's gradient by
     6e-4 to 1e-3 of its scale, a stale tile by 3e-3 (float64 NumPy backward on oracle states) -- 60 times the floor.

Cases: every path of the step-edge tests; the writer's predicates (dw_adam_body stores PT / MT / VT per lane under
own_valid and n < N, P and the Polyak target as a whole tile through LDS under tile_ok) at the smallest shapes that reach
them; the plan's cells (column split, chained, k_bwd8, loop form, RowRegs); TD3; the state a give-up's re-run left; and leg
A on the members of trainer groups, whose launches build their own weight-gradient tables."""
import numpy as np
import pytest

from tests.helpers import F64_ERRORS, SAC_ROWS, TD3_ROWS, check_step_f64, make_pair, make_td3_pair, synth_transitions
from tests.test_gpu_optimizer_step import OPT_PATHS, _batch, _same_state
from tests.test_gpu_step_edges import ENV as EDGE_ENV
from tests.written_state import TRAINED, check_copies_and_pads, copy_differences, oracles_from_state, pad_report

pytestmark = pytest.mark.gpu

ENV = EDGE_ENV + ("SAC_DW_FORM", "SAC_ROW_IMAGES")
H = (256, 256)


def _case(label, algo, shape, env=None, hidden=H, hidden_q=None, kind=1, after=None, ks=(1, 6)):
    """kind / after: fused_mode() in front of the loop and behind it (0 four launches, 1 the fused step -- TD3: its critic
    pass --, 2 chained, 3 the general step, 4 chained with the backward blocks inside)."""
    return dict(label=label, algo=algo, shape=shape, env=env or {}, hidden=hidden, hidden_q=hidden_q, kind=kind,
                after=kind if after is None else after, ks=ks)


def _of_path(p):
    label, algo, env, shape, hidden, kind = p
    if algo == "td3":
        kind = 3 if kind is None else int(kind)
    return _case(label, algo, shape, env, hidden, None, kind)


CASES = [_of_path(p) for p in OPT_PATHS] + [
    # the writer's predicates and the flat map, fused SAC
    _case("sac 48-wide layer, head tile full", "sac", (48, 8, 64)),                  # KP = 48: last k tile; 2A = 16
    _case("sac KQ 80, two head tiles", "sac", (64, 9, 32)),                          # a second strip of one k tile; nth = 2
    _case("sac KQ 128, A 16", "sac", (112, 16, 48)),                                 # the last narrow first layer
    _case("sac KQ 144, one row-block", "sac", (113, 3, 16)),                         # the first wide first layer
    _case("sac O + A below KQ", "sac", (42, 1, 32)),                                 # round_up(O + A) < KQ
    _case("sac 1x1x17", "sac", (1, 1, 17)),
    _case("sac Wipe 379x6", "sac", (379, 6, 64)),
    _case("sac narrow hidden, odd N and K", "sac", (42, 7, 48), hidden=(100, 50), hidden_q=(7, 255)),
    # plan cells
    _case("sac SP 2, loop-form dW", "sac", (42, 7, 288), kind=0),
    _case("sac SP 2, compact 0", "sac", (42, 7, 1040), kind=0),
    _case("sac SP 1 chained, compact 0", "sac", (42, 7, 1056), kind=2),
    _case("sac SP 1 four launches, k_bwd8", "sac", (42, 7, 1024), dict(SAC_CHAIN=0), kind=0),
    _case("sac kind 1, SAC_DW_FORM=loop", "sac", (42, 7, 255), dict(SAC_DW_FORM="loop")),
    _case("sac kind 1, SAC_ROW_IMAGES=0", "sac", (42, 7, 255), dict(SAC_ROW_IMAGES=0)),
    # TD3
    _case("td3 KQ 80", "td3", (64, 9, 32)),
    _case("td3 SP 2", "td3", (42, 7, 288), kind=0),
    _case("td3 SP 1", "td3", (42, 7, 1024), kind=0),                                 # (TD3 never chains)
    # the state a give-up's re-run left: launch 3 of the loop loses a producer, the call re-runs the lost steps
    _case("sac after a give-up", "sac", (42, 7, 255), dict(SAC_FUSED_TEST_STALL=3), after=0, ks=(6,)),
    _case("td3 after a give-up", "td3", (42, 7, 255), dict(SAC_FUSED_TEST_STALL=3), after=0, ks=(6,)),
]
PARAMS = [(c, k) for c in CASES for k in c["ks"]]


def _set_env(env, monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, str(v))


def _trainer(c, noise_seed=41):
    O, A, B = c["shape"]
    if c["algo"] == "sac":
        return make_pair(O, A, B, seed=5, hidden=c["hidden"], hidden_q=c["hidden_q"], noise_seed=noise_seed)[1]
    return make_td3_pair(O, A, B, seed=5, hidden=c["hidden"], noise_seed=noise_seed)[1]


def _buffer(O, A, seed, rows=2000):
    from robosuite_benchmark_amd import EnvReplayBuffer
    obs, act, rew, term, nobs = synth_transitions(rows, O, A, seed=seed, term_frac=0.1)
    buf = EnvReplayBuffer(rows, obs_dim=O, action_dim=A)
    buf.add_block(obs, act, rew, nobs, term)
    buf.seed(seed + 1)
    return buf


def _outputs(t, state, td3, policy_step):
    """What one step leaves for debug_fetch: the gradients it wrote and every per-row output."""
    nets = [n for n in TRAINED if n != "policy" or policy_step]
    out = {"g_" + n: t.debug_fetch("g_" + n, state["params"][n].size) for n in nets}
    out.update({n: t.debug_fetch(n, t._batch * t.act_dim) for n in (TD3_ROWS if td3 else SAC_ROWS)})
    return out


def _written(c, k, monkeypatch):
    """A trainer behind train_loop(buf, k) on its own buffer: (trainer, its state_dict())."""
    label, (O, A, B) = f"{c['label']} k={k}", c["shape"]
    _set_env(c["env"], monkeypatch)
    hip = _trainer(c)
    assert hip.fused_mode() == c["kind"], (label, hip.fused_mode())
    buf = _buffer(O, A, 70)
    first, last = hip.train_loop(buf, k, batch_size=B)
    assert hip.fused_mode() == c["after"], (label, hip.fused_mode())
    assert np.all(np.isfinite(first)) and np.all(np.isfinite(last)), label
    state = hip.state_dict()
    assert state["scalars"][3] == k and state["scalars"][4] == k, (label, state["scalars"])
    return hip, state


def _step_with_twin(c, hip, state):
    """The checked step, train(batch, eps=...) on a host batch with given noise, on the trainer and on a twin that got
    `state` from load_state_dict (the host uploads P, PT and the moments): (twin, batch, eps, diagnostics of both)."""
    (O, A, B), td3 = c["shape"], c["algo"] == "td3"
    twin = _trainer(c)
    twin.load_state_dict(state)
    batch, eps = _batch(O, A, B, 7)
    eps = eps[0] if td3 else eps
    return twin, batch, eps, hip.train(batch, eps=eps), twin.train(batch, eps=eps)


def _leg_b(label, hip, twin, state, diag, diag_twin, td3, policy_step):
    assert np.array_equal(diag, diag_twin, equal_nan=True), (label, "diagnostics of the twin", diag, diag_twin)
    mine, theirs = _outputs(hip, state, td3, policy_step), _outputs(twin, state, td3, policy_step)
    for name in mine:
        assert np.array_equal(mine[name], theirs[name], equal_nan=True), (label, "the twin's", name)
    _same_state(hip, twin, f"{label}, the twin")


def _leg_c(label, hip, state, batch, eps, diag, td3, policy_step):
    o32, o64 = oracles_from_state(hip, state)
    args = (batch["observations"], batch["actions"], batch["rewards"], batch["terminals"], batch["next_observations"])
    args += (eps,) if td3 else tuple(eps)
    want32, want64 = o32.step(*args), o64.step(*args)
    if td3:
        assert bool(o32.last["policy_step"]) == policy_step
    path = f"written state {label}"
    try:
        check_step_f64(hip, o32, o64, diag, want32, want64, path=path)
    finally:
        print(f"{path}: largest kernel error / scale, its tensor, the fp32 oracle's: {F64_ERRORS.get(path)}")


@pytest.mark.parametrize("c,k", PARAMS, ids=[f"{c['label']}-k{k}" for c, k in PARAMS])
def test_step_from_kernel_written_state(c, k, monkeypatch):
    label, td3 = f"{c['label']} k={k}", c["algo"] == "td3"
    hip, state = _written(c, k, monkeypatch)
    policy_step = not td3 or k % 2 == 0                   # (TD3: a policy step every second step; the gradient of another
    #                                                        step's policy pass is no output of this one)
    # A: the kernels' two copies agree, every pad is zero
    check_copies_and_pads(hip, f"{label}, behind the loop")
    # B: a twin that got this state from the readers takes the same step
    twin, batch, eps, diag, diag_twin = _step_with_twin(c, hip, state)
    _leg_b(label, hip, twin, state, diag, diag_twin, td3, policy_step)
    # C: the same step against the float64 oracle rebuilt from that state
    _leg_c(label, hip, state, batch, eps, diag, td3, policy_step)
    # A again, on what this step wrote
    check_copies_and_pads(hip, f"{label}, behind the step")


# ---- groups: leg A on every member -----------------------------------------------------------------------------------------
def _group_case(kind):
    from robosuite_benchmark_amd import MixedSACTrainerGroup, SACTrainerGroup, TD3TrainerGroup
    if kind == "sac":
        shapes, make, group = [(42, 7, 128)] * 3, make_pair, SACTrainerGroup
    elif kind == "td3":
        shapes, make, group = [(42, 7, 128)] * 2, make_td3_pair, TD3TrainerGroup
    else:
        shapes, make, group = [(42, 7, 128), (89, 14, 128)], make_pair, MixedSACTrainerGroup
    members = [make(O, A, B, seed=20 + r, noise_seed=50 + r)[1] for r, (O, A, B) in enumerate(shapes)]
    bufs = [_buffer(O, A, 80 + r) for r, (O, A, B) in enumerate(shapes)]
    return shapes, members, bufs, group(members)


@pytest.mark.parametrize("kind", ["sac", "td3", "mixed"])
def test_group_members_keep_both_copies_and_zero_pads(kind, monkeypatch):
    _set_env({}, monkeypatch)
    shapes, members, bufs, group = _group_case(kind)
    if kind == "mixed":
        group.train_loop(bufs, 6, batch_sizes=[B for _, _, B in shapes])
    else:
        group.train_loop(bufs, 6, batch_size=shapes[0][2])
    for r, t in enumerate(members):
        sc = t.state_dict()["scalars"]
        assert sc[3] == 6 and sc[4] == 6, (kind, r, sc)
        assert t.fused_mode() == 1, (kind, r)
        check_copies_and_pads(t, f"{kind} group member {r}")


# ---- the two readers behind a fused step nobody has settled ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["pt_qf1", "pad_nonzero"])
def test_the_readers_settle_a_trainer_whose_last_step_gave_up(name, monkeypatch):
    """As tests/test_gpu_state_readers.py has it for every other reader: the script's last fused step gives up, nobody has
    looked, and the read itself re-runs the lost step -- the transposed copy it returns is the four-launch twin's weights."""
    from tests.test_gpu_state_readers import _Settles, _unsettled
    fused, plain, bufs, B, steps = _unsettled("sac-42x7x128", 0, monkeypatch)
    want = plain.state_dict()["params"]["qf1"]
    with _Settles(fused, 0):
        got = fused.debug_fetch(name, want.size)
    if name == "pad_nonzero":
        assert pad_report(got, False, False) == {}
    else:
        assert copy_differences(got, want).size == 0
    assert fused.state_dict()["scalars"][4] == steps
