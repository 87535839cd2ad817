"""GPU: k_eval, k_eval_moments and k_eval_td3 against tests/golden/evaluate_columns.npz, byte for byte -- the outputs of
the cases of tests/evaluate_golden_cases.py as the commit recorded in the file computed them
(scripts/make_evaluate_golden.py).  The two kernels are instantiations of one frame (eval_frame, csrc/sac_eval.h); the
file was written by the two separate kernels in front of it.  A difference means that the frame changed behaviour."""
import os

import numpy as np
import pytest

from tests.evaluate_golden_cases import CASES, GOLDEN, NAN_ROW, case_id, make_members, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(os.path.dirname(__file__), "golden", GOLDEN)) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def members():
    return {False: make_members(False), True: make_members(True)}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_output_is_the_golden_files_bytes(case, golden, members):
    got = run_case(members[case[0] == "td3_evaluate_many"], case)
    want = {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(case_id(case) + "/")}
    assert set(got) == set(want) and len(want) >= 2
    for name, value in got.items():
        assert value.dtype == want[name].dtype and value.shape == want[name].shape, name
        differ = np.flatnonzero(value.view(np.uint8) != want[name].view(np.uint8))
        assert value.tobytes() == want[name].tobytes(), (name, differ[:8])


def test_the_golden_file_covers_the_cases_and_keeps_a_nan_in_its_row(golden):
    assert len(str(golden["commit"])) == 40
    assert {k.split("/", 1)[0] for k in golden if k != "commit"} == {case_id(c) for c in CASES}
    for case in (c for c in CASES if c[3]):
        cols = {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(case_id(case) + "/")}
        rows = cols["m1.rows"]                                        # (columns, n): the member with the NaN observation
        hit = np.isnan(rows).any(axis=0)
        assert hit[NAN_ROW] and hit.sum() == 1                        # chains Q and P of that row, and no other row
        assert np.isnan(rows[:2, NAN_ROW]).all() and np.isfinite(cols["m0.rows"]).all()
        for name, v in cols.items():
            if name.startswith("m1.") and v.ndim == 2 and name != "m1.rows":
                assert not np.isnan(np.delete(v, NAN_ROW, axis=0)).any(), name
