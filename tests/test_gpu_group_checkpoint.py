"""GPU: group checkpoints.  A grouped run saved after some epochs and resumed equals, bit for bit, the same run done
straight -- every non-time progress column, and every member's final parameters, Adam moments, trainer scalars, replay
buffer rows and generator state; a member exported into a solo trainer continues as it would have in the group; the
buffer's rows-written counter counts what it should."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from robosuite_benchmark_amd import EnvReplayBuffer, SACTrainerGroup
from robosuite_benchmark_amd import group_checkpoint as gc
from tests.helpers import make_pair, synth_transitions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small(name, **ak):
    from robosuite_benchmark_amd import variant
    v = variant.load_variant(os.path.join(ROOT, "tests", "golden", name + ".variant.json"))
    v["algorithm_kwargs"].update(min_num_steps_before_training=600, num_eval_steps_per_epoch=200,
                                 num_expl_steps_per_train_loop=400, num_trains_per_train_loop=150,
                                 eval_max_path_length=100, expl_max_path_length=100, num_epochs=3)
    v["algorithm_kwargs"].update(ak)
    v["replay_buffer_size"] = 5000
    return v


def td3_small():
    from robosuite_benchmark_amd.variant import default_variant
    v = default_variant(env="Lift", seed=3, batch_size=128, agent="TD3")
    v["algorithm_kwargs"].update(num_epochs=3, num_trains_per_train_loop=41, num_expl_steps_per_train_loop=100,
                                 num_eval_steps_per_epoch=100, min_num_steps_before_training=200,
                                 expl_max_path_length=50, eval_max_path_length=50)
    v["replay_buffer_size"] = 5000
    return v


def assert_rows_equal(got, want, where):
    assert len(got) == len(want), where
    for rg, rw in zip(got, want):
        assert list(rg.keys()) == list(rw.keys()), where
        for k in rw:
            if not k.startswith("time/"):
                assert rg[k] == rw[k], (where, rg["Epoch"], k)


def saved_members(d):
    """Every member of the newest generation under d: its state arrays, buffer cursor / generator position and rows."""
    man = gc.read_manifest(d)
    out = []
    for m in man["members"]:
        st = gc._split(gc._read(d, m["state"]), m["state"]["layout"])
        bm = m["buffer"]
        rows = b"".join(gc._read(d, c) for c in bm["chunks"])
        out.append((m["identity"]["label"], st, (bm["top"], bm["size"], bm["rng_pos"]), rows, m["trainer"]))
    return out


def assert_same_checkpoints(a, b):
    ma, mb = saved_members(a), saved_members(b)
    assert len(ma) == len(mb)
    for (la, sa, ca, ra, ta), (lb, sb, cb, rb, tb) in zip(ma, mb):
        assert la == lb and ca == cb and ta == tb, (la, ca, cb)
        assert list(sa) == list(sb)
        for k in sa:                                         # params, adam_m / adam_v, trainer scalars, generator key
            assert np.array_equal(sa[k], sb[k]), (la, k)
        assert ra == rb, (la, "buffer rows")


def csv_rows(path):
    with open(path, newline="") as f:
        text = f.read()
    return text, list(csv.DictReader(text.splitlines()))


def test_sac_group_resume_equals_the_straight_run(tmp_path):
    from robosuite_benchmark_amd.driver import experiment_group
    v = small("Lift-Panda-OSC-POSE-SEED17")
    straight = experiment_group(v, seeds=[3, 4], num_epochs=3, log_dir=str(tmp_path / "a"),
                                checkpoint_dir=str(tmp_path / "a" / "ck"), quiet=True)
    first = experiment_group(v, seeds=[3, 4], num_epochs=2, log_dir=str(tmp_path / "b"),
                             checkpoint_dir=str(tmp_path / "b" / "ck"), quiet=True)
    rest = experiment_group(v, seeds=[3, 4], num_epochs=3, log_dir=str(tmp_path / "b"),
                            checkpoint_dir=str(tmp_path / "b" / "ck"), resume=True, quiet=True)
    for s in (3, 4):
        assert [r["Epoch"] for r in rest[s]] == [2]
        assert_rows_equal(first[s] + rest[s], straight[s], s)
        assert all(r["time/saving (s)"] > 0 for r in first[s] + rest[s])
        text, rows = csv_rows(tmp_path / "b" / f"s{s}" / "progress.csv")
        assert text.count("replay_buffer/size") == 1 and len(rows) == 3
        _, want = csv_rows(tmp_path / "a" / f"s{s}" / "progress.csv")
        for rg, rw in zip(rows, want):
            assert {k: x for k, x in rg.items() if not k.startswith("time/")} == \
                   {k: x for k, x in rw.items() if not k.startswith("time/")}
    assert_same_checkpoints(str(tmp_path / "a" / "ck"), str(tmp_path / "b" / "ck"))
    # without a checkpoint directory nothing is saved
    plain = experiment_group(v, seeds=[3, 4], num_epochs=1, quiet=True)
    assert all(r["time/saving (s)"] == 0.0 for r in plain[3])
    # another group is refused, naming the member and the field
    with pytest.raises(gc.GroupMismatchError, match=r"group member 0 \(s4\): label"):
        experiment_group(v, seeds=[4, 3], num_epochs=3, checkpoint_dir=str(tmp_path / "b" / "ck"), resume=True,
                         quiet=True)


def test_td3_group_resumes_in_mid_phase(tmp_path):
    from robosuite_benchmark_amd.driver import experiment_group
    v = td3_small()                                          # 41 steps per epoch: period 2 stops in mid-phase
    straight = experiment_group(v, seeds=[3, 4], num_epochs=3, checkpoint_dir=str(tmp_path / "a"), quiet=True)
    first = experiment_group(v, seeds=[3, 4], num_epochs=1, checkpoint_dir=str(tmp_path / "b"), quiet=True)
    rest = experiment_group(v, seeds=[3, 4], num_epochs=3, checkpoint_dir=str(tmp_path / "b"), resume=True, quiet=True)
    for s in (3, 4):
        assert_rows_equal(first[s] + rest[s], straight[s], s)
        assert "trainer/Policy Loss" in rest[s][-1]
    assert_same_checkpoints(str(tmp_path / "a"), str(tmp_path / "b"))


def test_sweep_resume_with_a_wrapped_ring_and_reused_chunks(tmp_path):
    from robosuite_benchmark_amd.driver import experiment_sweep
    lift, two = small("Lift-Panda-OSC-POSE-SEED17"), small("TwoArmLift-PandaPanda-OSC-POSE-SEED17")
    two["algorithm_kwargs"]["batch_size"] = 256
    lift["algorithm_kwargs"]["batch_size"] = 128
    for v in (lift, two):
        v["replay_buffer_size"] = 1000                       # 600 + 400 rows fill it at epoch 0, epoch 1 wraps
    runs = [(lift, 5), (two, 5), (lift, 6)]
    kw = dict(chunk_rows=96, quiet=True)
    straight = experiment_sweep(runs, num_epochs=3, checkpoint_dir=str(tmp_path / "a"), **kw)
    first = experiment_sweep(runs, num_epochs=2, checkpoint_dir=str(tmp_path / "b"), **kw)
    man = gc.read_manifest(str(tmp_path / "b"))
    for m in man["members"]:
        gens = {c["file"].split("/")[0] for c in m["buffer"]["chunks"]}
        assert m["buffer"]["size"] == 1000 and m["buffer"]["rows_written"] == 1400
        assert "gen-0" in gens and "gen-1" in gens            # wrapped, and chunks of gen 0 reused in gen 1
    rest = experiment_sweep(runs, num_epochs=3, checkpoint_dir=str(tmp_path / "b"), resume=True, **kw)
    for i in range(len(runs)):
        assert_rows_equal(first[i] + rest[i], straight[i], i)
    assert_same_checkpoints(str(tmp_path / "a"), str(tmp_path / "b"))


def test_train_script_group_checkpoint_and_resume(tmp_path):
    vfile = tmp_path / "lift.json"
    vfile.write_text(json.dumps(small("Lift-Panda-OSC-POSE-SEED17")))
    script = os.path.join(ROOT, "scripts", "train.py")

    def run(*args):
        return subprocess.run([sys.executable, script, "--variant", str(vfile), *args], cwd=ROOT, capture_output=True,
                              text=True, timeout=600)

    out = run("--seeds", "3", "4", "--epochs", "3", "--log_dir", str(tmp_path / "a"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert not os.path.exists(tmp_path / "a" / "checkpoint")  # group checkpoints are opt-in
    out = run("--seeds", "3", "4", "--epochs", "2", "--log_dir", str(tmp_path / "b"), "--checkpoint")
    assert out.returncode == 0, out.stderr[-2000:]
    assert gc.checkpoint_exists(str(tmp_path / "b" / "checkpoint"))
    out = run("--seeds", "4", "3", "--epochs", "3", "--resume", str(tmp_path / "b"))
    assert out.returncode != 0 and "group member 0 (s4): label" in out.stderr, out.stderr[-2000:]
    out = run("--seeds", "3", "4", "--epochs", "3", "--resume", str(tmp_path / "b"))
    assert out.returncode == 0, out.stderr[-2000:]
    for s in (3, 4):
        text, rows = csv_rows(tmp_path / "b" / f"s{s}" / "progress.csv")
        _, want = csv_rows(tmp_path / "a" / f"s{s}" / "progress.csv")
        assert text.count("replay_buffer/size") == 1 and len(rows) == len(want) == 3
        for rg, rw in zip(rows, want):
            assert {k: x for k, x in rg.items() if not k.startswith("time/")} == \
                   {k: x for k, x in rw.items() if not k.startswith("time/")}


def test_a_member_exported_to_a_solo_trainer_continues_as_in_the_group(tmp_path):
    O, A, B = 42, 7, 128
    members, bufs, ids = [], [], []
    for i, (seed, n) in enumerate(((3, 3000), (4, 2500), (5, 4100))):
        t = make_pair(O, A, B, seed=seed, noise_seed=1000 + seed)[1]
        obs, act, rew, term, nobs = synth_transitions(n, O, A, seed=50 + i, term_frac=0.1)
        b = EnvReplayBuffer(4000, obs_dim=O, action_dim=A)
        b.add_block(obs, act, rew, nobs, term)
        b.seed(70 + i)
        members.append(t)
        bufs.append(b)
        ids.append(gc.member_identity(f"s{seed}", seed, dict(policy_kwargs=dict(hidden_sizes=[256, 256]),
                                                             qf_kwargs=dict(hidden_sizes=[256, 256])), t))
    group = SACTrainerGroup(members)
    group.train_loop(bufs, 37, batch_size=B)
    d = str(tmp_path / "ck")
    gc.GroupCheckpoint(d, 512).save(members, bufs, ids, [dict(epoch=0, seed=i) for i in range(3)])
    group.train_loop(bufs, 53, batch_size=B)
    for i in range(3):
        solo = make_pair(O, A, B, seed=99, noise_seed=1000 + 3 + i)[1]     # other initial weights: all overwritten
        sbuf = EnvReplayBuffer(4000, obs_dim=O, action_dim=A, numpy_global_stream=False)
        assert gc.load_group_member(d, i, solo, sbuf) == dict(epoch=0, seed=i)
        solo.train_loop(sbuf, 53, batch_size=B)
        st, sst = members[i].state_dict(), solo.state_dict()
        for k in st["params"]:
            assert np.array_equal(st["params"][k], sst["params"][k]), (i, k)
        for k in st["opt"]:
            for x, y in zip(st["opt"][k], sst["opt"][k]):
                assert np.array_equal(x, y), (i, "adam", k)
        assert np.array_equal(st["scalars"], sst["scalars"]), i
        (k1, p1), (k2, p2) = bufs[i].rng_state(), sbuf.rng_state()
        assert p1 == p2 and np.array_equal(k1, k2), i
        assert (sbuf.top(), sbuf.num_steps_can_sample()) == (bufs[i].top(), bufs[i].num_steps_can_sample())


def test_rows_written_counts_every_insert():
    O, A, cap = 11, 3, 1000
    b = EnvReplayBuffer(cap, obs_dim=O, action_dim=A, numpy_global_stream=False)
    assert b.rows_written() == 0
    obs, act, rew, term, nobs = synth_transitions(700, O, A, seed=1)
    b.add_block(obs, act, rew, nobs, term)                   # the pinned async ingest: counted when enqueued
    assert b.rows_written() == 700 and b.top() == 700
    b.ingest_wait()
    b.add_block(obs.astype(np.float64)[:500], act[:500].astype(np.float64), rew[:500], nobs[:500].astype(np.float64),
                term[:500])                                  # the float64 path, wrapping the ring
    assert b.rows_written() == 1200 and b.top() == 200 and b.num_steps_can_sample() == cap
    big = synth_transitions(2300, O, A, seed=2)
    b.add_block(big[0], big[1], big[2], big[4], big[3])      # more than the capacity: the ring moves on by all of it
    assert b.rows_written() == 3500 and b.top() == 3500 % cap
    b.set_cursor(17, 900)
    assert b.rows_written() == 3500 and (b.top(), b.num_steps_can_sample()) == (17, 900)
    b.set_cursor(3500 % cap, cap)
    st = b.state_dict()
    c = EnvReplayBuffer(cap, obs_dim=O, action_dim=A, numpy_global_stream=False)
    c.load_state_dict(st)                                    # a restore re-inserts the rows: cap more
    assert c.rows_written() == cap and c.top() == st["top"]
    assert b.rows_written() == 3500
