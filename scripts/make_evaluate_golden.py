"""Writes a golden file under tests/golden/: every output of the cases of a case module, computed on the GPU by the
library of the checked-out commit, which the file records.

    python scripts/make_evaluate_golden.py [--cases MODULE] [--commit HASH] [--out FILE]

A case module has GOLDEN (the file's name), CASES, case_id(case), make_all_members() and run(members, case) -> {name: array}:

  tests.evaluate_golden_cases (the default)   tests/golden/evaluate_columns.npz pins what k_eval, k_eval_moments and
      k_eval_td3 compute; tests/test_gpu_evaluate_golden.py compares later libraries with it byte for byte.  It was written
      by the commit in front of the one that introduced eval_frame (csrc/sac_eval.h).
  tests.general_golden_cases                  tests/golden/general_layers.npz pins what the general-shape inference
      entries compute (k_act_layer, k_qval_layer, k_eval_layer, k_act_layer_session, k_eval_y, k_unit_moments behind the
      layer launches); tests/test_gpu_general_golden.py compares.  It was written by the commit in front of the one that
      introduced infer_layer_frame and LayerSchedule (csrc/sac_infer.h).
  tests.evaluate_entries_cases                tests/golden/evaluate_entries.npz pins the evaluation entries the other two
      files do not reach (sac_evaluate_replay_many, td3_evaluate_stats_many, td3_evaluate_replay_many and the three
      td3_evaluate_general*_many entries); tests/test_gpu_evaluate_entries_golden.py compares.  It was written by the
      commit in front of the one that gave the SAC and TD3 entries one host body per family (eval_fused_many,
      eval_general_many).

A difference means that a later kernel or host body changed behaviour: regenerate a file only for a change that is meant to change the
bits, from the commit in front of it.  --commit names the commit where no git checkout is at hand (default: git rev-parse
HEAD)."""
from __future__ import annotations

import argparse
import importlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=str, default="tests.evaluate_golden_cases")
    ap.add_argument("--commit", type=str, default=None)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    mod = importlib.import_module(args.cases)
    out = args.out or os.path.join(ROOT, "tests", "golden", mod.GOLDEN)
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    members = mod.make_all_members()
    arrays = {"commit": np.array(commit)}
    for case in mod.CASES:
        for name, value in mod.run(members, case).items():
            arrays[mod.case_id(case) + "/" + name] = value
    np.savez_compressed(out, **arrays)
    print(f"{out}: {len(arrays) - 1} arrays of {len(mod.CASES)} cases, commit {commit}, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
