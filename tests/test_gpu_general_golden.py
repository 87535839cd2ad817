"""GPU: the general-shape inference entries against tests/golden/general_layers.npz, byte for byte -- the outputs of the
cases of tests/general_golden_cases.py as the commit recorded in the file computed them
(scripts/make_evaluate_golden.py --cases tests.general_golden_cases).  k_act_layer, k_qval_layer, k_eval_layer<SPLIT> and
k_act_layer_session<F64> are prologues in front of one layer frame (infer_layer_frame, csrc/sac_infer.h) and their job
tables come from one schedule builder (LayerSchedule); the file was written by the separate kernel bodies and the
hand-written layer chains in front of them.  A difference means that the frame or the schedule changed behaviour."""
import ctypes as C

import numpy as np
import pytest

from robosuite_benchmark_amd import _lib
from tests import general_golden_cases as cases
from tests.general_golden_cases import CASES, EVAL_ENTRIES, NAN_MEMBER, NAN_ROW, case_id
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
    nan_cases = [c for c in CASES if c[3]]
    assert {c[0] for c in nan_cases} == {"act", "q", "sac_evaluate_general_many", "units", "session"}
    for case in nan_cases:
        hits = 0
        for name, v in case_arrays(cases, golden, case).items():
            leaf = name.rsplit(".", 1)[1]
            if f"m{NAN_MEMBER}." not in name:
                assert np.isfinite(v).all(), (case_id(case), name)        # the other members
            elif leaf == "moments":
                assert np.isnan(v).any(), (case_id(case), name)           # (a sum over the rows)
            elif leaf != "alpha":
                hit = np.isnan(v).any(axis=0 if leaf in ("rows", "q") else 1)    # per row: (columns, n) or (n, columns)
                assert not np.delete(hit, NAN_ROW).any(), (case_id(case), name)
                hits += int(hit[NAN_ROW])
        assert hits >= 1, case_id(case)


def test_the_evaluation_entries_refuse_the_td3_twin(members):
    twin, n = members[2], 4
    ins = cases.make_inputs(twin, n, 1, False)
    rows = np.full((len(_lib.EVAL_ROWS), n), 7.0, np.float32)
    io = (_lib.SacEvalIO * 1)(_lib.SacEvalIO(*[x.ctypes.data for x in ins], rows.ctypes.data, None, None, None, None, -1.0))
    buf, idx = cases.replay_buffer(twin, 3), np.arange(n, dtype=np.int64)
    src = (_lib.SacEvalSrc * 1)(_lib.SacEvalSrc(buf._h.value, idx.ctypes.data))
    head = [(C.c_void_p * 1)(twin._h.value), 1, (C.c_int32 * 1)(n)]
    tails = ([io], [io, (_lib.SacEvalStats * 1)()], [src, io, None])
    for entry, tail in zip(EVAL_ENTRIES, tails):
        assert getattr(_lib.load(), entry)(*head, *tail) < 0 and "is a TD3 trainer" in _lib.last_error(), entry
    assert np.all(rows == 7.0)
