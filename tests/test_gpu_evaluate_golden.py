"""GPU: k_eval, k_eval_moments and k_eval_td3 against tests/golden/evaluate_columns.npz, byte for byte -- the outputs of
the cases of tests/evaluate_golden_cases.py as the commit recorded in the file computed them
(scripts/make_evaluate_golden.py).  The two kernels are instantiations of one frame (eval_frame, csrc/sac_eval.h); the
file was written by the two separate kernels in front of it.  A difference means that the frame changed behaviour."""
import numpy as np
import pytest

from tests import evaluate_golden_cases as cases
from tests.evaluate_golden_cases import CASES, NAN_ROW, case_id
from tests.golden_compare import case_arrays, check_case, check_covers, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden(cases)


@pytest.fixture(scope="module")
def members():
    return cases.make_all_members()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_output_is_the_golden_files_bytes(case, golden, members):
    check_case(cases, case, golden, members)


def test_the_golden_file_covers_the_cases_and_keeps_a_nan_in_its_row(golden):
    check_covers(cases, golden)
    for case in (c for c in CASES if c[3]):
        cols = case_arrays(cases, golden, case)
        rows = cols["m1.rows"]                                        # (columns, n): the member with the NaN observation
        hit = np.isnan(rows).any(axis=0)
        assert hit[NAN_ROW] and hit.sum() == 1                        # chains Q and P of that row, and no other row
        assert np.isnan(rows[:2, NAN_ROW]).all() and np.isfinite(cols["m0.rows"]).all()
        for name, v in cols.items():
            if name.startswith("m1.") and v.ndim == 2 and name != "m1.rows":
                assert not np.isnan(np.delete(v, NAN_ROW, axis=0)).any(), name
