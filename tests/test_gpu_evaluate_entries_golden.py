"""GPU: the evaluation entries that the other two golden files do not reach against tests/golden/evaluate_entries.npz,
byte for byte -- the outputs of the cases of tests/evaluate_entries_cases.py as the commit recorded in the file computed
them (scripts/make_evaluate_golden.py --cases tests.evaluate_entries_cases).  One host body per family (fixed-shape,
general-step) serves the SAC and the TD3 entries, plain, with statistics and on replay rows; the file was written by the
four separate bodies in front of it.  A difference means that a body, its staging or its tables changed behaviour."""
import numpy as np
import pytest

from tests import evaluate_entries_cases as cases
from tests.evaluate_entries_cases import CASES, FUSED, GENERAL, NAN_MEMBER, NAN_ROW, case_id
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
    assert {c[0] for c in CASES} == set(FUSED + GENERAL)
    nan_cases = [c for c in CASES if c[3]]
    assert {c[0][:3] for c in nan_cases} == {"sac", "td3"}                # one per objective
    for case in nan_cases:
        cols = case_arrays(cases, golden, case)
        rows = cols[f"m{NAN_MEMBER}.rows"]                                # (columns, n): the member with the NaN observation
        hit = np.isnan(rows).any(axis=0)
        assert hit[NAN_ROW] and hit.sum() == 1                            # chains Q and P of that row, and no other row
        assert np.isnan(rows[:2, NAN_ROW]).all()
        for name, v in cols.items():
            leaf = name.rsplit(".", 1)[1]
            if not name.startswith(f"m{NAN_MEMBER}."):
                assert np.isfinite(v).all(), (case_id(case), name)        # the other member, its statistics too
            elif leaf == "stats":
                assert np.isnan(v).any(), (case_id(case), name)           # (sums over the rows)
            elif v.ndim == 2 and leaf != "rows":
                assert not np.isnan(np.delete(v, NAN_ROW, axis=0)).any(), (case_id(case), name)


def test_the_replay_indices_hold_row_0_the_last_row_and_a_repeat():
    for n in (16, 17):
        idx = cases.replay_indices(n, 80, False)
        assert 0 in idx and cases.BUFFER_ROWS - 1 in idx and len(set(idx.tolist())) < n
    idx = cases.replay_indices(17, 81, True)
    assert idx[NAN_ROW] == 0 and (np.delete(idx, NAN_ROW) != 0).all()
