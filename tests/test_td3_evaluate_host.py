"""Host side of TD3Trainer.evaluate_td3 (no GPU): the host path of a trainer without a handle against
tests/td3_eval_reference.py under helpers.check_f64, infer.td3_eval_target / td3_smooth against the float32 torch
reference bit for bit, infer.td3_eval_statistics against hand-computed values, the private noise stream,
td3_evaluate_many on handle-less members, the driver option's refusal, and what stays as it was: TD3Trainer.evaluate /
evaluate_replay and validation=True keep refusing."""
import inspect
import os

import numpy as np
import pytest
import torch

from robosuite_benchmark_amd import _lib, group, infer
from robosuite_benchmark_amd.infer import td3_eval_statistics, td3_eval_target, td3_evaluate_many, td3_smooth
from tests.td3_eval_reference import (ARRAY_COLUMNS, COLUMNS, ROW_COLUMNS, SHAPES, batch_dict, check_columns, column_scales,
                                      conditioned_inputs, inputs, make_td3_trainer, trainer_reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT = ("Mean", "Std", "Max", "Min")
DIAG_KEYS = [k for k in _lib.TD3_DIAG_NAMES if k != "Actor Loss"]
TD_KEYS = [f"TD Error {i} {s}" for i in (1, 2) for s in STAT]


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in COLUMNS)


@pytest.mark.parametrize("O,A,hidden,hidden_q", [(O, A, h, None) for O, A, h in SHAPES] + [(42, 7, (64, 32), (256, 256))])
@pytest.mark.parametrize("n", [1, 17])
def test_the_host_path_against_the_reference(O, A, hidden, hidden_q, n):
    t = make_td3_trainer(O, A, hidden, hidden_q, seed=5, reward_scale=1.5, discount=0.97, target_policy_noise=0.3,
                         target_policy_noise_clip=0.25)
    assert t._h is None
    batch, eps = conditioned_inputs(t, n, O + n, column_scales(t, O))
    stats, cols = t.evaluate_td3(batch_dict(batch), eps=eps, rows=True)
    check_columns(cols, t, batch, eps, (O, A, hidden, hidden_q))
    assert list(cols.keys()) == list(COLUMNS)
    assert all(cols[k].shape == (n,) for k in ROW_COLUMNS) and all(cols[k].shape == (n, A) for k in ARRAY_COLUMNS)
    assert stats == td3_eval_statistics(np.stack([cols[k] for k in ROW_COLUMNS]), cols["a_pi"])
    rew, term = batch[2].ravel(), batch[3].ravel().astype(np.float32)
    y = td3_eval_target(rew, term, cols["tq1"], cols["tq2"], 1.5, 0.97)
    assert np.array_equal(cols["y"], y) and np.array_equal(cols["y"][term == 1], (np.float32(1.5) * rew)[term == 1])
    assert np.array_equal(cols["a_smooth"], td3_smooth(cols["a_target"], eps, 0.3, 0.25))
    assert not np.array_equal(cols["a_target"], cols["a_pi"])        # the target policy is a net of its own
    assert t.evaluate_td3(batch_dict(batch), eps=eps) == stats


def test_target_and_smoothing_are_the_float32_torch_expressions_bit_for_bit():
    rs = np.random.RandomState(3)
    n, A = 4000, 5
    f = lambda *s: rs.standard_normal(s).astype(np.float32)          # noqa: E731
    rew, tq1, tq2 = f(n) * 3, f(n) * 40, f(n) * 40
    term = (rs.uniform(size=n) < 0.3).astype(np.float32)
    y = td3_eval_target(rew, term, tq1, tq2, 2.5, 0.98)
    T = torch.from_numpy
    want = 2.5 * T(rew) + (1.0 - T(term)) * 0.98 * torch.min(T(tq1), T(tq2))
    assert y.dtype == np.float32 and np.array_equal(y, want.numpy())
    assert np.array_equal(y[term == 1], (np.float32(2.5) * rew)[term == 1]) and np.any(term == 1) and np.any(term == 0)
    # NaN follows fminf / np.fmin: a NaN target on one side is dropped, on both sides it stays
    nan = np.float32(np.nan)
    got = td3_eval_target([1.0, 1.0], [0.0, 0.0], [nan, nan], [2.0, nan], 1.0, 0.5)
    assert got[0] == np.float32(2.0) and np.isnan(got[1])
    a, eps = np.tanh(f(n, A)), f(n, A) * 2
    s = td3_smooth(a, eps, 0.3, 0.25)
    want = T(a) + torch.clamp(T(eps) * 0.3, -0.25, 0.25)
    assert s.dtype == np.float32 and np.array_equal(s, want.numpy())
    # a draw beyond clip / sigma lands exactly on a_target +- clip (the sum is not clipped again); a NaN draw stays NaN
    e = np.array([[10.0, -10.0, 0.5, np.nan, 0.0]], np.float32)
    at = np.array([[0.9, -0.9, 0.1, 0.2, 0.3]], np.float32)
    got = td3_smooth(at, e, 0.3, 0.25)[0]
    assert got[0] == np.float32(0.9) + np.float32(0.25) > 1.0 and got[1] == np.float32(-0.9) - np.float32(0.25) < -1.0
    assert got[2] == np.float32(0.1) + np.float32(0.5) * np.float32(0.3) and np.isnan(got[3]) and got[4] == np.float32(0.3)
    clipped = np.abs(eps * np.float32(0.3)) > 0.25
    assert np.any(clipped) and np.any(~clipped)
    assert np.array_equal(np.abs(s - a)[clipped], np.abs((a + np.sign(eps) * np.float32(0.25)) - a)[clipped])


def test_statistics_against_hand_computed_values():
    q1, q2 = np.array([1.0, 2.0, 3.0, 6.0]), np.array([2.0, 2.0, 2.0, 2.0])
    q_pi, y = np.array([0.5, -1.5, 2.0, 3.0]), np.array([2.0, 2.0, 1.0, 4.0])
    z = np.zeros(4)
    a_pi = np.array([[0.5, -0.5], [0.25, 0.75], [-1.0, 1.0], [0.0, 0.0]])
    d = td3_eval_statistics(np.stack([q1, q2, q_pi, z, z, y]).astype(np.float32), a_pi.astype(np.float32))
    assert list(d.keys()) == DIAG_KEYS + TD_KEYS and all(isinstance(v, float) for v in d.values())
    assert d["QF1 Loss"] == (1 + 0 + 4 + 4) / 4 and d["QF2 Loss"] == (0 + 0 + 1 + 4) / 4
    assert d["Policy Loss"] == -float(np.mean(q_pi)) == -1.0
    assert (d["Q1 Predictions Mean"], d["Q1 Predictions Max"], d["Q1 Predictions Min"]) == (3.0, 6.0, 1.0)
    assert d["Q1 Predictions Std"] == float(np.std(q1))
    assert d["Q2 Predictions Std"] == 0.0 and d["Q2 Predictions Mean"] == 2.0          # a constant column: Std exactly 0
    assert (d["Q Targets Mean"], d["Q Targets Max"], d["Q Targets Min"]) == (2.25, 4.0, 1.0)
    assert (d["Bellman Errors 1 Mean"], d["Bellman Errors 1 Max"], d["Bellman Errors 1 Min"]) == (2.25, 4.0, 0.0)
    assert d["Bellman Errors 2 Std"] == float(np.std([0.0, 0.0, 1.0, 4.0]))
    assert (d["Policy Action Mean"], d["Policy Action Max"], d["Policy Action Min"]) == (0.125, 1.0, -1.0)
    assert d["Policy Action Std"] == float(np.std(a_pi))
    assert (d["TD Error 1 Mean"], d["TD Error 1 Max"], d["TD Error 1 Min"]) == (0.75, 2.0, -1.0)       # signed: q - y
    assert d["TD Error 2 Mean"] == -0.25 and d["TD Error 2 Std"] == float(np.std(q2 - y))
    # the key order is get_diagnostics()' of a TD3 trainer: _record fills TD3_DIAG_NAMES without Actor Loss
    t = make_td3_trainer(5, 2, (8, 8))
    t._record(np.arange(len(_lib.TD3_DIAG_NAMES) + 4, dtype=np.float64))
    assert list(t.get_diagnostics().keys()) == list(d.keys())[:-8]


def test_eps_none_is_reproducible_and_leaves_np_random_alone():
    O, A, n = 9, 3, 12
    batch = batch_dict(inputs(n, O, A, 2)[0])
    np.random.seed(123)
    before = np.random.get_state()
    a, b, c = (make_td3_trainer(O, A, (16, 16), noise_seed=s) for s in (7, 7, 8))
    first, second = a.evaluate_td3(batch), a.evaluate_td3(batch)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert first != second                                           # (the private stream moves on)
    assert b.evaluate_td3(batch) == first and b.evaluate_td3(batch) == second
    assert c.evaluate_td3(batch) != first                            # another noise_seed, other draws
    want = np.random.RandomState(5).standard_normal((n, A))
    assert a.evaluate_td3(batch, rng=np.random.RandomState(5)) == a.evaluate_td3(batch, eps=want)
    assert a.get_diagnostics() == {} and a._num_train_steps == 0 and a._need_to_update_eval_statistics is True


def test_many_on_handle_less_members_equals_the_solo_calls():
    dims = [(9, 3, (16, 16)), (5, 2, (8, 8)), (42, 7, (64, 32))]
    ts = [make_td3_trainer(O, A, h, seed=10 + i) for i, (O, A, h) in enumerate(dims)]
    made = [inputs(n, O, A, 20 + i) for i, ((O, A, _), n) in enumerate(zip(dims, (5, 0, 33)))]
    batches = [batch_dict(m[0]) if m[0][0].shape[0] else None for m in made]
    got = td3_evaluate_many(ts, batches, eps=[m[1] for m in made], rows=True)
    assert got[1] is None and td3_evaluate_many(ts[:1], [None]) == [None]
    for i in (0, 2):
        stats, cols = ts[i].evaluate_td3(batches[i], eps=made[i][1], rows=True)
        assert got[i][0] == stats and same(got[i][1], cols), i
    assert group.td3_evaluate_many is infer.td3_evaluate_many
    assert td3_evaluate_many(ts, batches, eps=[m[1] for m in made])[0] == got[0][0]
    with pytest.raises(RuntimeError, match="twice"):
        td3_evaluate_many([ts[0], ts[0]], [batches[0], batches[0]])
    with pytest.raises(RuntimeError, match="per trainer"):
        td3_evaluate_many(ts[:1], [batches[0], batches[0]])
    from robosuite_benchmark_amd import FlattenMlp, SACTrainer, TanhGaussianPolicy
    qs = [FlattenMlp([16, 16], 1, 12) for _ in range(4)]
    sac = SACTrainer(policy=TanhGaussianPolicy([16, 16], 9, 3), qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3])
    with pytest.raises(RuntimeError, match="SAC trainer"):
        td3_evaluate_many([ts[0], sac], [batches[0], batches[0]])
    for kind in (group.TD3TrainerGroup, group.MixedTD3TrainerGroup, group.MlpTD3TrainerGroup, group.ArchTD3TrainerGroup,
                 group.SACTrainerGroup):
        assert callable(kind.td3_evaluate_many)


def test_bad_arguments_raise():
    t = make_td3_trainer(5, 2, (8, 8))
    good = batch_dict(inputs(6, 5, 2, 1)[0])
    for key, bad in (("observations", good["observations"][:, :4]), ("actions", good["actions"][:5]),
                     ("next_observations", good["next_observations"][:3]), ("rewards", good["rewards"][:2])):
        with pytest.raises(ValueError, match="evaluate_td3"):
            t.evaluate_td3(dict(good, **{key: bad}))
    with pytest.raises(ValueError, match="eps"):
        t.evaluate_td3(good, eps=np.zeros((5, 2)))


def test_what_refused_before_still_refuses_and_the_new_option():
    from robosuite_benchmark_amd import driver, variant
    O, A = 5, 2
    t = make_td3_trainer(O, A, (8, 8))
    batch = batch_dict(inputs(4, O, A, 1)[0])
    with pytest.raises(NotImplementedError, match=r"TD3Trainer\.evaluate: evaluate computes the SAC objective .* is not implemented"):
        t.evaluate(batch)
    with pytest.raises(NotImplementedError, match=r"TD3Trainer\.evaluate_replay: evaluate computes the SAC objective"):
        t.evaluate_replay(None, n=4)
    td3 = variant.default_variant(env="Lift", seed=1, batch_size=64, agent="TD3")
    sac = variant.default_variant(env="Lift", seed=1, batch_size=64, agent="SAC")
    for call in (lambda: driver.experiment(td3, seed=1, num_epochs=1, quiet=True, validation=True),
                 lambda: driver.experiment_group(td3, seeds=[1, 2], num_epochs=1, quiet=True, validation=True),
                 lambda: driver.experiment_sweep([(td3, 1)], num_epochs=1, quiet=True, validation=True)):
        with pytest.raises(RuntimeError, match="SAC objective"):
            call()
    # td3_validation: a SAC variant is refused in front of anything that builds a run (no library call, no GPU needed)
    for call in (lambda: driver.experiment(sac, seed=1, num_epochs=1, quiet=True, td3_validation=True),
                 lambda: driver.experiment_group(sac, seeds=[1, 2], num_epochs=1, quiet=True, td3_validation=True),
                 lambda: driver.experiment_sweep([(td3, 1), (sac, 2)], num_epochs=1, quiet=True, td3_validation=True)):
        with pytest.raises(RuntimeError, match=r"td3_validation=True.*validation=True"):
            call()
    for fn in (driver.experiment, driver.experiment_group, driver.experiment_sweep):
        params = inspect.signature(fn).parameters
        assert params["td3_validation"].default is False and list(params)[-1] == "td3_validation", fn.__name__
    assert driver.EvalOptions._field_defaults["td3_validation"] is False and driver.EvalOptions._fields[-1] == "td3_validation"
    opts = driver._options("experiment", [(td3,)], "host", False, "host", False, "host", "host", 0, td3_validation=True)
    assert opts.td3_validation is True and opts.validation is False
    # the columns of an epoch without evaluation paths stay, empty
    empty = driver._td3_validation_columns(None, None)
    assert list(empty.keys()) == ["validation/" + k for k in DIAG_KEYS + TD_KEYS] + ["validation/Num Transitions"]
    assert empty["validation/Num Transitions"] == 0 and all(np.isnan(v) for k, v in empty.items() if k[-11:] != "Transitions")
    # the draw: the first of RandomState([seed, epoch, VALIDATION_STREAM])
    b = batch_dict(inputs(6, O, A, 3)[0])
    want = np.random.RandomState([17, 2, driver.VALIDATION_STREAM]).standard_normal((6, A))
    assert np.array_equal(driver._td3_validation_eps(17, 2, b, A), want) and driver._td3_validation_eps(17, 2, None, A) is None


def test_the_train_script_takes_the_option():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_script", os.path.join(ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    assert ap.parse_args(["--agent", "TD3", "--td3_validation"]).td3_validation is True
    assert ap.parse_args([]).td3_validation is False


def test_bindings_and_header_name_the_feature():
    header = open(os.path.join(ROOT, "include", "sac_hip.h")).read()
    for name in ("td3_evaluate", "td3_evaluate_many"):
        assert name in _lib.SYMBOLS and f"int {name}(" in header
    assert ("enum { TD3_EVAL_Q1, TD3_EVAL_Q2, TD3_EVAL_Q_PI, TD3_EVAL_TQ1, TD3_EVAL_TQ2, TD3_EVAL_Y, TD3_EVAL_ROWS_N };"
            in header)
    assert tuple(_lib.TD3_EVAL_ROWS) == ROW_COLUMNS and tuple(_lib.TD3_EVAL_ARRAYS) == ARRAY_COLUMNS
    assert [f[0] for f in _lib.Td3EvalIO._fields_] == ["obs", "act", "rew", "term", "next_obs", "eps", "rows", "a_pi",
                                                       "a_target", "a_smooth"]
    assert '#include "td3_eval.h"' in open(os.path.join(ROOT, "robosuite_benchmark_amd", "csrc", "sac_trainer.hip")).read()


def test_the_reference_is_the_no_update_half_of_the_oracle_step():
    # the float64 reference's columns are RlkitEquivalentTD3.step's own forward values on the same weights
    from oracle.td3_step_torch import RlkitEquivalentTD3
    from tests.td3_eval_reference import trainer_layers
    O, A, n = 11, 3, 40
    t = make_td3_trainer(O, A, (32, 16), seed=2, reward_scale=2.5, target_policy_noise=0.4, target_policy_noise_clip=0.3)
    batch, eps = inputs(n, O, A, 4)
    o = RlkitEquivalentTD3(trainer_layers(t), A, target_policy_noise=0.4, target_policy_noise_clip=0.3, reward_scale=2.5,
                           dtype=torch.float64)
    obs, act, rew, term, nobs = batch
    o.step(obs, act, rew, term.astype(np.float32), nobs, eps)
    ref = trainer_reference(t, batch, eps, torch.float64)
    for k, key in (("q1", "q1"), ("q2", "q2"), ("tq1", "tq1"), ("tq2", "tq2"), ("y", "y"), ("a_target", "a2"),
                   ("a_smooth", "noisy"), ("a_pi", "pa")):
        want = o.last[key].detach().numpy()
        assert np.array_equal(ref[k], want[:, 0] if k in ROW_COLUMNS else want), k
