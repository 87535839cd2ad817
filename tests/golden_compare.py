"""What the golden-file tests share: a case module (tests/evaluate_golden_cases.py, tests/general_golden_cases.py) run by
the library of now against its file under tests/golden/, byte for byte."""
import os

import numpy as np


def load_golden(mod):
    with np.load(os.path.join(os.path.dirname(__file__), "golden", mod.GOLDEN)) as f:
        return {k: f[k] for k in f.files}


def case_arrays(mod, golden, case):
    """The golden file's arrays of one case, without the case's prefix."""
    return {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(mod.case_id(case) + "/")}


def check_case(mod, case, golden, members):
    got = mod.run(members, case)
    want = case_arrays(mod, golden, case)
    assert set(got) == set(want) and len(want) >= 2
    for name, value in got.items():
        assert value.dtype == want[name].dtype and value.shape == want[name].shape, name
        differ = np.flatnonzero(value.view(np.uint8) != want[name].view(np.uint8))
        assert value.tobytes() == want[name].tobytes(), (name, differ[:8])


def check_covers(mod, golden):
    assert len(str(golden["commit"])) == 40
    assert {k.split("/", 1)[0] for k in golden if k != "commit"} == {mod.case_id(c) for c in mod.CASES}
