"""CPU: the oracles held to the frozen float64 steps of tests/golden/step_fixtures.npz (written once by
tests/golden/make_step_fixture.py from the cases of tests/step_fixture_cases.py).  The file cannot follow an edit to an
oracle, to the plumbing that builds one from a state, or a change of the installed torch: this test turns red instead.

  checksums    every input the recipe rebuilds has the bytes the file was computed from; every stored array its own
  float64      the live float64 oracle against the file, per tensor max|R_live - R_file| / s <= 1e-6: the stored values are
               float32 roundings (6e-8), a float64 reduction over at most 1024 x 400 terms moves by about 1e-11 between
               thread counts and torch versions, and 1e-6 sits ten times under the kernels' floor
  float32      the live float32 oracle under exactly the rule the kernels get (hold_to_fixture below, which
               tests/test_gpu_step_fixture.py applies to every step path): the reference alone stays within it
  sensitivity  per narrow case the live float64 oracle with ONE hyperparameter or scalar changed by 0.1 % (a period or a
               counter by a step) breaks the rule on a stored quantity: what the file pins, it pins that finely"""
import os

import numpy as np
import pytest
import torch

from tests import step_fixture_cases as cases
from tests.golden import make_step_fixture as gen
from tests.helpers import F64_FACTOR, F64_FLOOR, check_f64_e32

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_fixtures.npz")
LIVE_TOL = 1e-6
WORST = {}                  # path -> (largest kernel error as a fraction of its bound, the tensor), for reporting

_cache = {}


def fixture():
    if "fx" not in _cache:
        _cache["fx"] = cases.Fixture(FIXTURE)
    return _cache["fx"]


def case(name):
    if name not in _cache:
        _cache[name] = cases.build(name)
    return _cache[name]


def live(name, dtype):
    key = (name, dtype)
    if key not in _cache:
        _cache[key] = gen.run(case(name), dtype)
    return _cache[key]


def violations(c, fx, got, path=None):
    """Everything in which the result `got` of one step from case `c` -- dict(diag {name: value}, rows, grads, params, opt,
    scalars) as make_step_fixture.run returns it, a trainer's in the same form -- breaks what the file `fx` pins:
      the rule  max|K - R| / s <= max(8 e32, 1e-5), K == 0 exactly where R is exactly 0 (helpers.check_f64_e32), for every
                diagnostic at its stored scale, every per-row output, every gradient tensor and, narrow cases, the update
                out - in of every parameter and target tensor, both Adam moments, log_alpha and its moments;
      exactly   the counters; and what the case leaves unchanged, against the INPUT bit for bit: targets off their period,
                TD3's policy and its moments off a policy step, log_alpha and its moments where alpha is fixed.
    A list of messages (empty: held)."""
    stored, diag, scalars = fx.case(c)
    bad = []

    def rule(name, K, R, s, e32):
        try:
            eK = check_f64_e32(name, K, R, s, e32, path)
        except AssertionError as e:
            bad.append(str(e))
            return
        frac = eK / max(F64_FACTOR * e32, F64_FLOOR)
        if path is not None and frac >= WORST.get(path, (0.0,))[0]:
            WORST[path] = (frac, name)

    for name, (v, s, e32) in diag.items():
        rule(name, [got["diag"][name]], [v], s, e32)
    grads = {net: got["grads"].get(net, np.full(c.count(net), np.nan)) for net in c.stepped()}
    T = cases.step_tensors(c, got["rows"], grads, got.get("params"), got.get("opt"), got.get("scalars"))
    assert list(T) == list(stored), (c.name, "tensor names differ from the file's")
    for name, (R, s, e32) in stored.items():
        rule(name, cases.stored_view(c, name, T[name]), R, s, e32)
    if c.full:
        return bad
    same = lambda a, b: np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))     # noqa: E731
    for net in c.unchanged_params():
        if not same(got["params"][net], c.params[net]):
            bad.append(f"{net} must stay bit-unchanged")
    for net in cases.TRAINED:
        if net not in c.stepped() and not all(same(a, b) for a, b in zip(got["opt"][net], c.opt[net])):
            bad.append(f"the Adam moments of {net} must stay bit-unchanged")
    sc = np.asarray(got["scalars"], np.float64)
    exact = {3: "adam_t", 4: "n_train_steps_total"}
    if c.td3:
        exact[0] = "adam_t_pi"
    elif not c.auto_alpha():
        if not same(sc[:3], c.scalars[:3]):
            bad.append(f"log_alpha and its moments must stay bit-unchanged under fixed alpha: {sc[:3]} from {c.scalars[:3]}")
    for i, what in exact.items():
        if sc[i] != scalars[i]:
            bad.append(f"{what}: {sc[i]:.0f}, the file has {scalars[i]:.0f}")
    return bad


def hold_to_fixture(c, fx, got, path):
    bad = violations(c, fx, got, path)
    assert not bad, f"{path}: {c.name}: {len(bad)} quantities off the fixture:\n  " + "\n  ".join(bad[:12])


# ---- checksums -----------------------------------------------------------------------------------------------------------
def test_every_stored_array_is_the_one_written():
    fx = fixture()
    want = {f"{name}|{part}" for name in cases.NAMES for part in ("values", "stats", "diag", "scalars")} | {"meta"}
    assert set(fx.arrays) == want
    assert set(fx.meta["sha256"]) == want - {"meta"}
    for key, digest in fx.meta["sha256"].items():
        assert cases.sha256(fx.arrays[key]) == digest, f"{key} is not the array the generator wrote"
    assert fx.meta["grad_stride"] == cases.GRAD_STRIDE and fx.meta["torch"] and fx.meta["numpy"]
    assert os.path.getsize(FIXTURE) <= gen.MAX_BYTES


@pytest.mark.parametrize("name", cases.NAMES)
def test_inputs_have_the_bytes_the_file_was_computed_from(name):
    c, m = case(name), fixture().meta["cases"][name]
    assert dict(c.checksums()) == m["inputs"]
    assert list(c.unchanged_params()) == m["unchanged"] and list(c.stepped()) == m["stepped"]
    assert [int(i) for i in cases.terminal_rows(c)] == m["terminal_rows"] and m["terminal_rows"]
    if not c.full:                     # what the issue asks of a narrow case's inputs
        assert c.B % 16 != 0 or name == "sac chained"          # (the chained launch takes whole pairs of row-blocks only)
        assert all(np.all(m_ != 0) and np.all(v > 0) for m_, v in c.opt.values())
        assert c.td3 or (c.scalars[0] != 0 and c.scalars[1] != 0 and c.scalars[2] > 0)


# ---- the live oracles against the file -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_live_float64_oracle_reproduces_the_file(name):
    c, r = case(name), live(name, torch.float64)
    gen.structure(c, r)
    stored, diag, scalars = fixture().case(c)
    T = gen.tensors_of(c, r)
    assert list(T) == list(stored)
    for k, (R, s, e32) in stored.items():
        assert 8 * e32 <= gen.E32_CAP, (k, e32)
        s_live = float(np.max(np.abs(T[k])))
        assert abs(s_live - s) <= LIVE_TOL * s, (k, s_live, s)
        if s:
            err = float(np.max(np.abs(cases.stored_view(c, k, T[k]) - R))) / s
            assert err <= LIVE_TOL, f"{k}: the live float64 oracle is {err:.3g} of max|R| = {s:.3g} off the file"
        else:
            assert np.all(T[k] == 0), k
    assert list(r["diag"]) == list(diag)
    for k, (v, s, e32) in diag.items():
        assert 8 * e32 <= gen.E32_CAP, (k, e32)
        assert abs(r["scales"][k] - s) <= LIVE_TOL * s, (k, r["scales"][k], s)
        assert abs(r["diag"][k] - v) <= LIVE_TOL * s, (k, r["diag"][k], v)
    assert np.array_equal(r["scalars"][3:], scalars[3:]), (r["scalars"], scalars)
    assert np.all(np.abs(r["scalars"][:3] - scalars[:3]) <= LIVE_TOL * np.abs(scalars[:3])), (r["scalars"], scalars)


@pytest.mark.parametrize("name", cases.NAMES)
def test_live_float32_oracle_stays_within_the_kernels_rule(name):
    hold_to_fixture(case(name), fixture(), live(name, torch.float32), "float32 oracle")


def test_a_terminal_row_takes_no_bootstrap():
    for name in cases.NAMES:
        c = case(name)
        stored = fixture().case(c)[0]
        rows = cases.terminal_rows(c)
        want = (np.float32(c.kw["reward_scale"]) * c.batch["rewards"].ravel()[rows]).astype(np.float32)
        assert np.array_equal(stored["row q_target"][0][rows].astype(np.float32), want), name


# ---- sensitivity ---------------------------------------------------------------------------------------------------------
def _flip_period(c):
    """A period under which the case's step number is on the period where it was off, and off where it was on."""
    n = int(c.scalars[4])
    return next(p for p in range(2, 50) if (n % p == 0) != c.on_period())


def mutations(c):
    """[(label, keyword changes, scalar changes {index: value})]: each hyperparameter times 1.001, the period flipped, each
    counter one step on.  Left out, because the quantity provably does not enter the step:
      target_entropy under fixed alpha (no alpha loss is formed);
      tau / soft_target_tau off the period (no target moves);
      TD3's policy_learning_rate off a policy step (the policy's optimizer does not step)."""
    sc, kw = c.scalars, c.kw
    times = lambda k: (f"{k} x 1.001", {k: kw[k] * 1.001}, {})      # noqa: E731
    out = [times("discount"), times("reward_scale")]
    if c.td3:
        out += [times("qf_learning_rate"), times("target_policy_noise"), times("target_policy_noise_clip")]
        if c.on_period():
            out += [times("tau"), times("policy_learning_rate")]
        out.append(("adam_t_pi + 1", {}, {0: sc[0] + 1}))
        period = "policy_and_target_update_period"
    else:
        out += [times("policy_lr"), times("qf_lr"), ("log_alpha x 1.001", {}, {0: float(np.float32(sc[0] * 1.001))})]
        if c.on_period():
            out.append(times("soft_target_tau"))
        if c.auto_alpha():
            out.append(times("target_entropy"))
        period = "target_update_period"
    out += [(f"{period} -> {_flip_period(c)}", {period: _flip_period(c)}, {}),
            ("n_train_steps_total + 1", {}, {4: sc[4] + 1}), ("adam_t + 1", {}, {3: sc[3] + 1})]
    return out


SENSITIVITY = [(name, m[0]) for name in cases.NARROW_CASES for m in mutations(cases.build(name))]


@pytest.mark.parametrize("name,label", SENSITIVITY, ids=[f"{n}-{m}" for n, m in SENSITIVITY])
def test_one_changed_quantity_breaks_the_rule(name, label):
    c = case(name)
    _, kw, sc_changes = next(m for m in mutations(c) if m[0] == label)
    sc = c.scalars.copy()
    for i, v in sc_changes.items():
        sc[i] = v
    got = gen.run(c, torch.float64, kw=kw, scalars=sc)
    bad = violations(c, fixture(), got)
    assert bad, f"{name}: {label} goes unseen: the file does not pin it"
    if label in ("adam_t + 1", "adam_t_pi + 1") and name in ("sac early", "td3 policy step"):
        # the bias corrections themselves, not just the counter that comes back
        assert any("kernel error" in b for b in bad), (name, label, bad)
