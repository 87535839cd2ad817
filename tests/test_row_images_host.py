"""Host: where the step plan (csrc/sac_step_plan.h) lets k_abc take its input rows from the slot's row images -- exactly
where the step starts as k_abc; SAC_ROW_IMAGES=0 keeps the converting instance and changes nothing else of the plan."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robosuite_benchmark_amd", "csrc")

WRAPPER = r"""
#include "sac_step_plan.h"
using namespace sac;
// fused: 0 unset, 1 SAC_FUSED=0; images: 0 unset, 1 SAC_ROW_IMAGES=0, 2 SAC_ROW_IMAGES=1
extern "C" void plan_of(int O, int A, int batch, int algo, int cus, int fused, int images, int *out) {
    StepEnv E;
    if (fused) { E.fused.set = true; E.fused.v = 0; }
    if (images) { E.row_images.set = true; E.row_images.v = images - 1; }
    const StepPlan P = step_plan(O, A, batch, algo, cus, E);
    const int v[] = {P.row_images, P.fused, P.chain_bwd, P.chain, P.wide, (int)P.fused_launch.lds, P.fused_launch.grid};
    for (int x : v) *out++ = x;
}
extern "C" int env_row_images() {
    const StepEnv E = step_env_from_environment();
    return E.row_images.set ? E.row_images.v : -1;
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("row_images_plan")
    src, so = d / "wrapper.cpp", d / "libplan.so"
    src.write_text(WRAPPER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)])
    return ctypes.CDLL(str(so))


def plan(lib, O, A, batch, algo=0, cus=256, fused=0, images=0):
    out = (ctypes.c_int * 8)()
    lib.plan_of(O, A, batch, algo, cus, fused, images, out)
    return dict(zip(("row_images", "fused", "chain_bwd", "chain", "wide", "lds", "grid"), list(out)))


@pytest.mark.parametrize("shape, algo, want", [
    ((42, 7, 256), 0, 1), ((42, 7, 1), 0, 1), ((112, 14, 48), 0, 1), ((113, 2, 48), 0, 1), ((379, 6, 256), 0, 1),
    ((42, 7, 256), 1, 1),                      # the TD3 critic pass is k_abc too
    ((42, 7, 272), 0, 0), ((42, 7, 512), 0, 0),          # four launches
    ((46, 7, 544), 0, 0),                      # chained forward launches
    ((46, 7, 1024), 0, 0),                     # fused, but as k_chain8 with the backward inside: it converts the rows itself
])
def test_images_exactly_where_the_step_is_k_abc(lib, shape, algo, want):
    p = plan(lib, *shape, algo=algo)
    assert p["row_images"] == want
    assert p["row_images"] == (1 if p["fused"] and not p["chain_bwd"] else 0)


def test_overrides(lib):
    for shape in [(42, 7, 256), (379, 6, 256), (46, 7, 1024), (42, 7, 512)]:
        on, off = plan(lib, *shape), plan(lib, *shape, images=1)
        assert off["row_images"] == 0 and dict(off, row_images=on["row_images"]) == on      # nothing else moves
        assert plan(lib, *shape, images=2) == on                                            # (1 forces nothing)
    assert plan(lib, 42, 7, 256, fused=1)["row_images"] == 0
    assert plan(lib, 42, 7, 256, cus=128)["row_images"] == 0          # too few CUs for the fused step


def test_the_environment_variable(lib, monkeypatch):
    monkeypatch.delenv("SAC_ROW_IMAGES", raising=False)
    assert lib.env_row_images() == -1
    monkeypatch.setenv("SAC_ROW_IMAGES", "0")
    assert lib.env_row_images() == 0
    for name in sorted(os.listdir(CSRC)):          # read in one place, like the plan's other variables
        if name.endswith((".h", ".hip")) and name != "sac_step_plan.h":
            assert 'getenv("SAC_ROW_IMAGES"' not in open(os.path.join(CSRC, name)).read(), name
