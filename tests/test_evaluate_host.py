"""Host side of SACTrainer.evaluate (no GPU): sac.eval_statistics against the float64 oracle's own diagnostics, the host
path of a trainer without a handle against tests/eval_reference.py under helpers.check_f64, the private noise stream,
TD3's refusal and the declarations."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.sac_step_torch import RlkitEquivalentSAC, init_sac_params
from robosuite_benchmark_amd import FlattenMlp, TanhGaussianPolicy, TanhMlpPolicy, TD3Trainer, _lib
from robosuite_benchmark_amd.group import evaluate_many
from robosuite_benchmark_amd.sac import SACTrainer, eval_statistics, eval_target
from tests.eval_reference import COLUMNS, ROW_COLUMNS, SHAPES, batch_dict, check_columns
from tests.helpers import flat_of, synth_transitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD_KEYS = [f"TD Error {i} {s}" for i in (1, 2) for s in ("Mean", "Std", "Max", "Min")]
DIAG_KEYS = [k for k in _lib.DIAG_NAMES if k != "Actor Loss"]


def oracle_rows(o):
    L = o.last
    col = lambda x: x.detach().numpy()[:, 0]                         # noqa: E731
    z = np.zeros(L["q1"].shape[0])                                   # (tq1, tq2, log_pi_next: not read by the statistics)
    rows = [col(L["q1"]), col(L["q2"]), col(L["q1_new"]), col(L["q2_new"]), z, z, col(L["log_pi"]), col(L["log_pi2"]),
            col(L["y"])]
    return np.stack(rows), L["mu"].detach().numpy(), L["log_std"].detach().numpy()


def step_inputs(B, O, A, seed):
    obs, act, rew, term, nobs = synth_transitions(B, O, A, seed=seed, term_frac=0.1)
    rs = np.random.RandomState(seed + 1)
    return (obs, act, rew, term.astype(np.float32), nobs, rs.standard_normal((B, A)).astype(np.float32),
            rs.standard_normal((B, A)).astype(np.float32))


def test_eval_statistics_reproduce_the_float64_step_with_tuning_off():
    # with tuning off the step's alpha is 1 before and after: its diagnostics ARE the evaluation's
    O, A, B = 11, 3, 50
    o = RlkitEquivalentSAC(init_sac_params(O, A, hidden=(32, 16), seed=2), A, use_automatic_entropy_tuning=False,
                           reward_scale=2.5, dtype=torch.float64)
    want = o.step(*step_inputs(B, O, A, 4))
    rows, mu, log_std = oracle_rows(o)
    assert rows.dtype == np.float64
    got = eval_statistics(rows, mu, log_std, 1.0, 0.0, o.target_entropy, False)
    assert list(got.keys()) == DIAG_KEYS + TD_KEYS
    for k in DIAG_KEYS:
        assert isinstance(got[k], float) and got[k] == pytest.approx(want[k], rel=1e-12, abs=0.0), k
    assert got["Alpha"] == 1.0 and got["Alpha Loss"] == 0.0
    td = rows[0] - rows[8]
    assert got["TD Error 1 Mean"] == float(np.mean(td)) < 0          # signed: q - y, the targets above the fresh critics
    assert got["TD Error 1 Min"] == float(np.min(td)) and got["TD Error 1 Max"] == float(np.max(td))
    assert got["TD Error 2 Std"] == float(np.std(rows[1] - rows[8]))
    assert got["QF1 Loss"] == float(np.mean(td ** 2))


def test_alpha_loss_against_the_float64_oracle_before_its_update():
    O, A, B = 7, 2, 40
    o = RlkitEquivalentSAC(init_sac_params(O, A, hidden=(16, 16), seed=3), A, dtype=torch.float64)
    with torch.no_grad():
        o.log_alpha.fill_(0.3)
    want = o.step(*step_inputs(B, O, A, 9))                         # Alpha Loss: from log_alpha = 0.3, before the update
    assert float(o.log_alpha.detach()) != 0.3
    rows, mu, log_std = oracle_rows(o)
    got = eval_statistics(rows, mu, log_std, float(np.exp(0.3)), 0.3, o.target_entropy, True)
    assert got["Alpha Loss"] == pytest.approx(want["Alpha Loss"], rel=1e-12)
    assert got["Alpha Loss"] == float(-np.mean(0.3 * (rows[6] + o.target_entropy)))
    assert got["Alpha"] == float(np.exp(0.3))
    assert got["Log Pis Mean"] == pytest.approx(want["Log Pis Mean"], rel=1e-12)


def handle_less(O, A, hidden, seed=5, **kw):
    """A SACTrainer that was never given a batch size (no handle), on init_sac_params' weights."""
    nets = init_sac_params(O, A, hidden=hidden, seed=seed)
    pol = TanhGaussianPolicy(list(hidden), O, A)
    qs = [FlattenMlp(list(hidden), 1, O + A) for _ in range(4)]
    pol.load_flat(flat_of(nets["policy"]))
    for q, name in zip(qs, ("qf1", "qf2", "target_qf1", "target_qf2")):
        q.load_flat(flat_of(nets[name]))
    kw.setdefault("noise_seed", 7)
    return SACTrainer(policy=pol, qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], **kw)


@pytest.mark.parametrize("O,A,hidden", SHAPES)
@pytest.mark.parametrize("n", [1, 17])
def test_the_host_path_against_the_reference(O, A, hidden, n):
    t = handle_less(O, A, hidden, reward_scale=1.5, discount=0.97)
    assert t._h is None
    batch = synth_transitions(n, O, A, seed=O + n, term_frac=0.1)
    rs = np.random.RandomState(n)
    eps = (rs.standard_normal((n, A)).astype(np.float32), rs.standard_normal((n, A)).astype(np.float32))
    stats, cols = t.evaluate(batch_dict(batch), eps=eps, rows=True)
    check_columns(cols, t, batch, eps, (O, A, hidden))
    assert list(cols.keys()) == list(COLUMNS) + ["alpha"] and cols["alpha"] == 1.0        # (log_alpha 0 at the start)
    assert stats == eval_statistics(np.stack([cols[k] for k in ROW_COLUMNS]), cols["mu"], cols["log_std"], 1.0, 0.0,
                                    t.target_entropy, True)
    term = np.asarray(batch[3]).ravel() != 0
    y = eval_target(batch[2].ravel(), batch[3].ravel(), cols["tq1"], cols["tq2"], cols["log_pi_next"], 1.0, 1.5, 0.97)
    assert np.array_equal(cols["y"], y) and np.array_equal(cols["y"][term], (np.float32(1.5) * batch[2].ravel())[term])
    many = evaluate_many([t], [batch_dict(batch)], eps=[eps], rows=True)
    assert many[0][0] == stats and all(np.array_equal(many[0][1][k], cols[k]) for k in COLUMNS)
    assert evaluate_many([t], [None]) == [None]


def test_eps_none_is_reproducible_and_leaves_np_random_alone():
    O, A, n = 9, 3, 12
    batch = batch_dict(synth_transitions(n, O, A, seed=2, term_frac=0.1))
    np.random.seed(123)
    before = np.random.get_state()
    a, b, c = (handle_less(O, A, (16, 16), noise_seed=s) for s in (7, 7, 8))
    first, second = a.evaluate(batch), a.evaluate(batch)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert first != second                                           # (the private stream moves on)
    assert b.evaluate(batch) == first and b.evaluate(batch) == second
    assert c.evaluate(batch) != first                                # another noise_seed, other draws
    rng = np.random.RandomState(5)
    want = (rng.standard_normal((n, A)), rng.standard_normal((n, A)))
    assert a.evaluate(batch, rng=np.random.RandomState(5)) == a.evaluate(batch, eps=want)
    # evaluate leaves the trainer's own statistics and counters alone
    assert a.get_diagnostics() == {} and a._num_train_steps == 0 and a._need_to_update_eval_statistics is True


def test_bad_arguments_raise():
    t = handle_less(5, 2, (8, 8))
    good = batch_dict(synth_transitions(6, 5, 2, seed=1))
    for key, bad in (("observations", good["observations"][:, :4]), ("actions", good["actions"][:5]),
                     ("next_observations", good["next_observations"][:3]), ("rewards", good["rewards"][:2])):
        with pytest.raises(ValueError, match="evaluate"):
            t.evaluate(dict(good, **{key: bad}))
    with pytest.raises(ValueError, match="eps"):
        t.evaluate(good, eps=(np.zeros((6, 2)), np.zeros((5, 2))))
    with pytest.raises(RuntimeError, match="twice"):
        evaluate_many([t, t], [good, good])
    with pytest.raises(RuntimeError, match="per trainer"):
        evaluate_many([t], [good, good])


def test_td3_refuses():
    O, A = 5, 2
    pols = [TanhMlpPolicy([8, 8], A, O) for _ in range(2)]
    qs = [FlattenMlp([8, 8], 1, O + A) for _ in range(4)]
    t = TD3Trainer(policy=pols[0], qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], target_policy=pols[1])
    with pytest.raises(NotImplementedError, match="SAC objective"):
        t.evaluate(batch_dict(synth_transitions(4, O, A, seed=1)))
    from robosuite_benchmark_amd import driver, variant
    v = variant.default_variant(env="Lift", seed=1, batch_size=64, agent="TD3")
    for call in (lambda: driver.experiment(v, seed=1, num_epochs=1, quiet=True, validation=True),
                 lambda: driver.experiment_group(v, seeds=[1, 2], num_epochs=1, quiet=True, validation=True),
                 lambda: driver.experiment_sweep([(v, 1)], num_epochs=1, quiet=True, validation=True)):
        with pytest.raises(RuntimeError, match="SAC objective"):
            call()


def test_bindings_header_and_drivers_name_the_feature():
    header = open(os.path.join(ROOT, "include", "sac_hip.h")).read()
    for name in ("sac_evaluate", "sac_evaluate_many"):
        assert name in _lib.SYMBOLS and f"int {name}(" in header
    assert ("enum { SAC_EVAL_Q1, SAC_EVAL_Q2, SAC_EVAL_Q1_NEW, SAC_EVAL_Q2_NEW, SAC_EVAL_TQ1, SAC_EVAL_TQ2,\n"
            "       SAC_EVAL_LOG_PI, SAC_EVAL_LOG_PI_NEXT, SAC_EVAL_Y, SAC_EVAL_ROWS_N };") in header
    assert tuple(_lib.EVAL_ROWS) == ROW_COLUMNS and len(_lib.SacEvalIO._fields_) == 13
    assert _lib.SacEvalIO.alpha.offset == 12 * 8                     # twelve pointers, then the float
    from robosuite_benchmark_amd import driver
    for fn in (driver.experiment, driver.experiment_group, driver.experiment_sweep):
        assert inspect.signature(fn).parameters["validation"].default is False, fn.__name__
    assert driver.EvalOptions._field_defaults["validation"] is False
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--help"], capture_output=True,
                         text=True, check=True).stdout
    assert "--validation" in out
