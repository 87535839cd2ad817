"""Writes tests/golden/evaluate_columns.npz: every output of the cases of tests/evaluate_golden_cases.py, computed on the
GPU by the library of the checked-out commit, which the file records.

    python scripts/make_evaluate_golden.py [--commit HASH] [--out FILE]

The file pins what k_eval, k_eval_moments and k_eval_td3 compute; tests/test_gpu_evaluate_golden.py compares later
libraries with it byte for byte.  It was written by the commit in front of the one that introduced eval_frame
(csrc/sac_eval.h).  A difference means that a later kernel changed behaviour: regenerate the file only for a change that
is meant to change the bits, from the commit in front of it.  --commit names the commit where no git checkout is at hand
(default: git rev-parse HEAD)."""
from __future__ import annotations

import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.evaluate_golden_cases import CASES, GOLDEN, case_id, make_members, run_case  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", type=str, default=None)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "tests", "golden", GOLDEN))
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    members = {False: make_members(False), True: make_members(True)}
    arrays = {"commit": np.array(commit)}
    for case in CASES:
        for name, value in run_case(members[case[0] == "td3_evaluate_many"], case).items():
            arrays[case_id(case) + "/" + name] = value
    np.savez_compressed(args.out, **arrays)
    print(f"{args.out}: {len(arrays) - 1} arrays of {len(CASES)} cases, commit {commit}, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
