"""The step plan (csrc/sac_step_plan.h) on the host: which step a trainer of the fused kernels' shapes runs -- kernels,
grids, block sizes, LDS -- as a pure function of (obs_dim, act_dim, batch, algo, CU count, environment).  The header is
compiled with the host C++ compiler alone (which also proves it free of HIP) behind a few-line extern "C" wrapper."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robosuite_benchmark_amd", "csrc")

ENV_NAMES = ["SAC_FORCE_SP", "SAC_WIDE_MIN_KQ", "SAC_DW_FORM", "SAC_FUSED", "SAC_FUSED_TEST_STALL", "SAC_CHAIN", "SAC_CHAIN8",
             "SAC_BWD8", "SAC_CHAIN_BWD"]
SCALARS = ["ok", "refusal", "B", "NB", "KP", "KQ", "NH", "nth", "SP", "wide", "wide4", "fused", "chain", "chain8", "bwd8",
           "chain_bwd", "dw_one", "test_stall_at", "compact"]
LAUNCHES = ["a", "b", "c", "fused_launch", "chained", "b2", "c2"]

WRAPPER = r"""
#include "sac_step_plan.h"
using namespace sac;
static void put(const StepPlan &P, int *o) {
    const int v[] = {P.ok, P.refusal, P.B, P.NB, P.KP, P.KQ, P.NH, P.nth, P.SP, P.wide, P.wide4, P.fused, P.chain, P.chain8,
                     P.bwd8, P.chain_bwd, P.dw_one, (int)P.test_stall_at, P.compact};
    for (int x : v) *o++ = x;
    const StepLaunch *L[] = {&P.a, &P.b, &P.c, &P.fused_launch, &P.chained, &P.b2, &P.c2};
    for (const StepLaunch *l : L) { *o++ = l->grid; *o++ = l->threads; *o++ = (int)l->lds; }
}
// set / val: the nine variables in the order of StepEnv (SAC_DW_FORM: val 1 = "loop")
extern "C" void plan_of(int O, int A, int batch, int algo, int cus, const int *set, const int *val, int *out) {
    StepEnv E;
    EnvInt *f[] = {&E.force_sp, &E.wide_min_kq, nullptr, &E.fused, &E.fused_test_stall, &E.chain, &E.chain8, &E.bwd8, &E.chain_bwd};
    for (int i = 0; i < 9; ++i) {
        if (!set[i]) continue;
        if (f[i]) { f[i]->set = true; f[i]->v = val[i]; }
        else E.dw_form_loop = val[i] == 1;
    }
    put(step_plan(O, A, batch, algo, cus, E), out);
}
extern "C" void plan_from_environment(int O, int A, int batch, int algo, int cus, int *out) {
    put(step_plan(O, A, batch, algo, cus, step_env_from_environment()), out);
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("step_plan")
    src, so = d / "plan_wrapper.cpp", d / "libstep_plan.so"
    src.write_text(WRAPPER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)])
    return ctypes.CDLL(str(so))


def _unpack(out):
    p = dict(zip(SCALARS, out))
    for i, name in enumerate(LAUNCHES):
        p[name] = tuple(out[len(SCALARS) + 3 * i: len(SCALARS) + 3 * i + 3])        # (grid, threads, lds)
    # as sac_trainer_step_kind numbers it: 0 four launches, 1 k_abc, 2 chained, 4 chained with the backward inside
    p["kind"] = (4 if p["chain_bwd"] else 1) if p["fused"] else (2 if p["chain"] else 0)
    return p


def plan(lib, O, A, batch, algo=0, cus=256, **env):
    sets, vals = [0] * 9, [0] * 9
    for k, v in env.items():
        i = ENV_NAMES.index(k)
        sets[i], vals[i] = 1, (1 if v == "loop" else 0) if k == "SAC_DW_FORM" else int(v)
    out = (ctypes.c_int * 64)()
    lib.plan_of(O, A, batch, algo, cus, (ctypes.c_int * 9)(*sets), (ctypes.c_int * 9)(*vals), out)
    return _unpack(list(out))


@pytest.mark.parametrize("shape, kind, more", [
    ((42, 7, 256), 1, {}),
    ((42, 7, 1), 1, {}),
    ((112, 7, 64), 1, {"wide": 0}),
    ((113, 7, 64), 1, {"wide": 1}),
    ((379, 6, 256), 1, {}),
    ((496, 16, 256), 1, {"nth": 2}),
    ((42, 7, 272), 0, {"SP": 2}),
    ((42, 7, 512), 0, {"SP": 2}),
    ((42, 7, 1040), 0, {"SP": 2, "NB": 65}),
    ((46, 7, 544), 2, {"SP": 1}),
    ((46, 7, 1024), 4, {}),
    ((86, 14, 1024), 2, {}),
    ((46, 7, 2048), 2, {}),
    ((379, 6, 1024), 0, {}),
])
def test_step_kind_by_shape(lib, shape, kind, more):
    p = plan(lib, *shape)
    assert p["ok"] == 1 and p["kind"] == kind
    for k, v in more.items():
        assert p[k] == v, (k, p[k])


@pytest.mark.parametrize("shape, env, kind, more", [
    ((42, 7, 256), {"SAC_FUSED": 0}, 0, {}),
    ((46, 7, 1024), {"SAC_CHAIN_BWD": 0}, 2, {}),
    ((46, 7, 1024), {"SAC_CHAIN": 0}, 0, {}),
    ((46, 7, 544), {"SAC_CHAIN_BWD": 1}, 4, {}),
    ((379, 6, 1024), {"SAC_CHAIN": 1}, 2, {}),
    ((46, 7, 1024), {"SAC_CHAIN": 1, "SAC_CHAIN8": 0}, 2, {"chained": (256, 256, 43008)}),
])
def test_step_kind_with_overrides(lib, shape, env, kind, more):
    p = plan(lib, *shape, **env)
    assert p["kind"] == kind
    for k, v in more.items():
        assert p[k] == v, (k, p[k])


def test_overrides_that_are_ignored_or_narrow(lib):
    for shape in [(42, 7, 256), (42, 7, 272), (46, 7, 1024), (379, 6, 1040)]:
        assert plan(lib, *shape, SAC_FORCE_SP=3) == plan(lib, *shape)              # not a split
    assert plan(lib, 42, 7, 1040)["NB"] % 2 == 1
    assert plan(lib, 42, 7, 1040, SAC_FORCE_SP=1) == plan(lib, 42, 7, 1040)        # SP * NB must stay even
    assert plan(lib, 42, 7, 1040, SAC_FORCE_SP=4)["SP"] == 4
    assert plan(lib, 42, 7, 256)["dw_one"] == 1 and plan(lib, 42, 7, 272)["dw_one"] == 0
    loop = plan(lib, 42, 7, 256, SAC_DW_FORM="loop")
    assert loop["dw_one"] == 0 and dict(loop, dw_one=1) == plan(lib, 42, 7, 256)
    assert plan(lib, 42, 7, 256, SAC_FUSED_TEST_STALL=3)["test_stall_at"] == 3 and plan(lib, 42, 7, 256)["test_stall_at"] == 0
    assert plan(lib, 42, 7, 64, SAC_WIDE_MIN_KQ=64)["wide"] == 1 and plan(lib, 42, 7, 64)["wide"] == 0


@pytest.mark.parametrize("shape, cus, kind", [((42, 7, 256), 128, 0), ((42, 7, 128), 128, 1), ((46, 7, 1024), 304, 2)])
def test_step_kind_by_cu_count(lib, shape, cus, kind):
    assert plan(lib, *shape, cus=cus)["kind"] == kind


def test_td3(lib):
    assert plan(lib, 42, 7, 256, algo=1)["kind"] == 1
    p = plan(lib, 46, 7, 1024, algo=1)
    assert p["kind"] == 0 and p["bwd8"] == 0 and p["chain"] == 0 and p["SP"] == 1
    assert plan(lib, 46, 16, 256, algo=1)["nth"] == 1 and plan(lib, 46, 16, 256)["nth"] == 2


def test_lds_bytes(lib):
    p = plan(lib, 42, 7, 256)
    assert (p["a"][2], p["b"][2], p["fused_launch"][2]) == (28672, 98304, 102400)
    p = plan(lib, 379, 6, 1024, SAC_CHAIN=1)
    assert (p["a"][2], p["b"][2], p["chained"][2]) == (65536, 65536, 67584)
    assert plan(lib, 379, 6, 1024)["chained"][2] == 67584
    p = plan(lib, 86, 14, 1024)
    assert (p["a"][2], p["b"][2], p["chained"][2]) == (49152, 45056, 51200)
    p = plan(lib, 46, 7, 1024)
    assert p["fused_launch"] == (256, 512, max(43008, 20480))
    for algo in (0, 1):
        for shape in [(42, 7, 1), (42, 7, 256), (496, 16, 256), (46, 7, 544), (46, 7, 1024), (379, 6, 2048)]:
            q = plan(lib, *shape, algo=algo)
            assert q["c"][2] == 20480 and q["ok"] == 1
            if algo:
                assert q["c2"][2] == 20480 and q["b2"][2] == q["b"][2]


@pytest.mark.parametrize("batch", [1, 16, 17, 128, 256, 257, 272, 512, 528, 544, 1024, 1040, 2048])
@pytest.mark.parametrize("dims", [(42, 7), (113, 14), (379, 6)])
def test_grids(lib, dims, batch):
    p = plan(lib, *dims, batch)
    NB, SP = (batch + 15) // 16, p["SP"]
    assert p["NB"] == NB and p["B"] == 16 * NB and SP * NB % 2 == 0
    assert p["a"][:2] == (4 * SP * NB, 256) and p["b"][:2] == (4 * SP * NB, 256)
    compact = 1 if 3 * SP * NB <= 192 else 0
    assert p["compact"] == compact
    assert p["c"][:2] == (4 * SP * NB if compact else 3 * SP * NB, 512 if p["bwd8"] else 256)
    assert p["bwd8"] == (1 if SP == 1 else 0)
    assert p["b2"][0] == 0 and p["c2"][0] == 0
    if p["kind"] == 1:
        assert p["fused_launch"][:2] == (16 * NB, 256)
    if p["kind"] == 4:
        assert p["fused_launch"][:2] == (4 * NB, 512)
    assert p["chained"][:2] == (4 * NB, 512)
    assert plan(lib, *dims, batch, SAC_CHAIN8=0)["chained"][:2] == (4 * NB, 256)
    t = plan(lib, *dims, batch, algo=1)
    g2 = 8 * ((SP * NB + 3) // 4)
    assert t["SP"] == SP and t["compact"] == 0
    assert t["a"][:2] == (4 * SP * NB, 256) and t["b"][:2] == (g2, 256) and t["c"][:2] == (g2, 256)
    assert t["b2"][:2] == (SP * NB, 256) and t["c2"][:2] == (SP * NB, 256)
    if t["kind"] == 1:
        assert t["fused_launch"][:2] == (16 * NB, 256)
    assert t["kind"] in (0, 1)


def test_the_environment_is_read_in_one_place(lib, monkeypatch):
    for name in ENV_NAMES:
        monkeypatch.delenv(name, raising=False)
    out = (ctypes.c_int * 64)()
    lib.plan_from_environment(42, 7, 256, 0, 256, out)
    assert _unpack(list(out)) == plan(lib, 42, 7, 256)
    monkeypatch.setenv("SAC_FUSED", "0")
    monkeypatch.setenv("SAC_DW_FORM", "loop")
    lib.plan_from_environment(42, 7, 256, 0, 256, out)
    assert _unpack(list(out)) == plan(lib, 42, 7, 256, SAC_FUSED=0, SAC_DW_FORM="loop")
    # no other source file asks the environment for one of the nine names
    pat = re.compile(r'getenv\("(%s)"' % "|".join(ENV_NAMES))
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".hip")) and name != "sac_step_plan.h":
            assert not pat.search(open(os.path.join(CSRC, name)).read()), name
    header = open(os.path.join(CSRC, "sac_step_plan.h")).read()
    assert all('"%s"' % name in header for name in ENV_NAMES)


# ---- the step schedule: the plan's launches of one step in launch order (step_schedule) ----------------------------------
WRAPPER += r"""
// out: per stage {kernel, grid, threads, lds, need, arg, tail, last_event}; returns the number of stages
extern "C" int schedule_of(int O, int A, int batch, int algo, int cus, const int *set, const int *val, int fused_now, int *out) {
    StepEnv E;
    EnvInt *f[] = {&E.force_sp, &E.wide_min_kq, nullptr, &E.fused, &E.fused_test_stall, &E.chain, &E.chain8, &E.bwd8, &E.chain_bwd};
    for (int i = 0; i < 9; ++i) {
        if (!set[i]) continue;
        if (f[i]) { f[i]->set = true; f[i]->v = val[i]; }
        else E.dw_form_loop = val[i] == 1;
    }
    StepStage st[STEP_STAGES_MAX];
    const int n = step_schedule(step_plan(O, A, batch, algo, cus, E), fused_now != 0, st);
    for (int i = 0; i < n; ++i) {
        const int v[] = {st[i].kernel, st[i].launch.grid, st[i].launch.threads, (int)st[i].launch.lds, st[i].need, st[i].arg,
                         st[i].tail, st[i].last_event};
        for (int x : v) *out++ = x;
    }
    return n;
}
"""

KERNEL_IDS = ["A", "B", "C", "B2", "C2", "FUSED", "CHAINED", "DW", "DW_Q", "DW_PI"]        # enum StepKernelId, in order
PLAN_LAUNCH = {"A": "a", "B": "b", "C": "c", "B2": "b2", "C2": "c2", "FUSED": "fused_launch", "CHAINED": "chained"}
ACTOR_FOLLOWS = -1                                                                           # TAIL_ACTOR_FOLLOWS


def schedule(lib, O, A, batch, fused_now, algo=0, cus=256, **env):
    """[(kernel name, launch (grid, threads, lds), need, arg, tail, last_event)] of one step"""
    sets, vals = [0] * 9, [0] * 9
    for k, v in env.items():
        i = ENV_NAMES.index(k)
        sets[i], vals[i] = 1, (1 if v == "loop" else 0) if k == "SAC_DW_FORM" else int(v)
    out = (ctypes.c_int * 64)()
    n = lib.schedule_of(O, A, batch, algo, cus, (ctypes.c_int * 9)(*sets), (ctypes.c_int * 9)(*vals), int(fused_now), out)
    assert 0 < n <= 8
    return [(KERNEL_IDS[out[8 * i]], tuple(out[8 * i + 1: 8 * i + 4])) + tuple(out[8 * i + 4: 8 * i + 8]) for i in range(n)]


def _check_launches(lib, sched, shape, algo, env):
    """every stage's launch is the plan's corresponding StepLaunch; a weight-gradient stage: 256 threads, no LDS, no grid"""
    p = plan(lib, *shape, algo=algo, **env)
    for name, launch, *_ in sched:
        assert launch == (p[PLAN_LAUNCH[name]] if name in PLAN_LAUNCH else (0, 256, 0)), (name, launch)
    return p


SAC_FOUR = [("A", 1), ("B", 2), ("C", 4), ("DW", 6)]
SAC_CHAINED = [("CHAINED", 2), ("C", 4), ("DW", 6)]
SAC_FUSED = [("FUSED", 4), ("DW", 6)]


@pytest.mark.parametrize("shape, env, kind, fused_now, want", [
    ((42, 7, 256), {"SAC_FUSED": 0}, 0, True, SAC_FOUR),
    ((42, 7, 256), {"SAC_FUSED": 0}, 0, False, SAC_FOUR),
    ((379, 6, 1024), {}, 0, True, SAC_FOUR),
    ((379, 6, 1024), {}, 0, False, SAC_FOUR),
    ((46, 7, 544), {}, 2, True, SAC_CHAINED),
    ((46, 7, 544), {}, 2, False, SAC_CHAINED),
    ((86, 14, 1024), {}, 2, True, SAC_CHAINED),
    ((86, 14, 1024), {}, 2, False, SAC_CHAINED),
    ((42, 7, 256), {}, 1, True, SAC_FUSED),
    ((46, 7, 1024), {}, 4, True, SAC_FUSED),
    ((42, 7, 256), {}, 1, False, SAC_FOUR),
    ((46, 7, 1024), {}, 4, False, SAC_CHAINED),
])
def test_sac_schedules(lib, shape, env, kind, fused_now, want):
    s = schedule(lib, *shape, fused_now, **env)
    p = _check_launches(lib, s, shape, 0, env)
    assert p["kind"] == kind
    assert [(name, last_event) for name, _, _, _, _, last_event in s] == want
    for name, _, need, arg, tail, _ in s:
        assert (need, arg) == (0, 0)
        assert tail == (p["compact"] if name == "C" else 0), (name, tail)


TD3_ACTOR_PASS = [("B2", 1, 1, 0), ("C2", 2, 1, 0), ("DW_PI", 1, 1, 0)]                       # (kernel, need, arg, tail)
TD3_FOUR = [("A", 0, 0, ACTOR_FOLLOWS), ("B", 0, 0, 0), ("C", 0, 0, 0), ("DW_Q", 0, 0, 0)] + TD3_ACTOR_PASS
TD3_FUSED = [("FUSED", 0, 0, ACTOR_FOLLOWS), ("DW_Q", 0, 0, 0)] + TD3_ACTOR_PASS


@pytest.mark.parametrize("shape, env, kind, fused_now, want", [
    ((46, 7, 1024), {}, 0, True, TD3_FOUR),
    ((46, 7, 1024), {}, 0, False, TD3_FOUR),
    ((42, 7, 256), {"SAC_FUSED": 0}, 0, True, TD3_FOUR),
    ((42, 7, 256), {"SAC_FUSED": 0}, 0, False, TD3_FOUR),
    ((42, 7, 256), {}, 1, True, TD3_FUSED),
    ((42, 7, 256), {}, 1, False, TD3_FOUR),
])
def test_td3_schedules(lib, shape, env, kind, fused_now, want):
    s = schedule(lib, *shape, fused_now, algo=1, **env)
    p = _check_launches(lib, s, shape, 1, env)
    assert p["kind"] == kind and p["compact"] == 0
    assert [(name, need, arg, tail) for name, _, need, arg, tail, _ in s] == want
    assert all(last_event == 0 for *_, last_event in s)            # (the profiling pass instruments the SAC step only)


def test_profile_event_stream_of_a_schedule(lib):
    """e0 in front of the first stage; behind each stage the events after the previous stage's last_event up to its own"""
    def stream(s):
        out, at = ["e0"], 0
        for name, *_, last_event in s:
            out.append(name)
            out += ["e%d" % k for k in range(at + 1, last_event + 1)]
            at = max(at, last_event)
        return out
    assert stream(schedule(lib, 42, 7, 256, True)) == ["e0", "FUSED", "e1", "e2", "e3", "e4", "DW", "e5", "e6"]
    assert stream(schedule(lib, 46, 7, 544, True)) == ["e0", "CHAINED", "e1", "e2", "C", "e3", "e4", "DW", "e5", "e6"]
    assert stream(schedule(lib, 42, 7, 256, False)) == ["e0", "A", "e1", "B", "e2", "C", "e3", "e4", "DW", "e5", "e6"]
