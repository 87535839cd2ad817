"""One SAC / TD3 step per case of tests/step_fixture_cases.py, taken by the float64 oracle and frozen:
tests/golden/step_fixtures.npz.  Runs on the CPU.  Run from the repository root:

    python tests/golden/make_step_fixture.py            (writes the file, prints the report: per case s, e32, size; and
                                                         keeps it in step_fixtures.report.txt)
    python tests/golden/make_step_fixture.py --check    (the report alone; --verbose: a line per tensor)

Per case both oracles are built from the case's inputs the way tests/written_state.py oracles_from_state builds them from a
state_dict() -- nets, log_alpha and its Adam state, n_train_steps_total -- and with the Adam state of EVERY trained
parameter, so that the state behind the step is the oracle's own.  One step in float64 (R), one in float32 (P).  Stored
per case, names and order as step_fixture_cases.step_tensors gives them:
  values   every per-row output, every gradient tensor and -- narrow cases -- the state out: each parameter and target
           tensor as its UPDATE out - in, both Adam moments, log_alpha and its moments.  The float32 rounding of R (at
           most 6e-8 of a value).  A full-size case keeps every 97th element of a gradient tensor and no state out.
  stats    per tensor s = max|R| and e32 = max|P - R| / s over the whole tensor, float64
  diag     per diagnostic the float64 value, its scale (helpers.diag_scales) and e32, float64
  scalars  state_dict()["scalars"][:5] behind the step, float64 (the counters are compared exactly)
and in `meta` (JSON) the tensor names and sizes, the SHA-256 of every input array and of every stored array, and the
torch and NumPy versions that wrote the file.  What the file does not hold is what a case leaves unchanged: the tests
compare that with the input, bit for bit."""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.sac_step_torch import RlkitEquivalentSAC                        # noqa: E402
from oracle.td3_step_torch import RlkitEquivalentTD3                        # noqa: E402
from tests import step_fixture_cases as cases                               # noqa: E402
from tests.helpers import SAC_ROWS, TD3_ROWS, diag_scales, layers_from_flat, oracle_flat_grad      # noqa: E402
from tests.written_state import _adam_entry, _set_net_adam                  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "step_fixtures.npz")
MAX_BYTES = 1 << 20               # no committed file is larger than 1 MiB
E32_CAP = 2.5e-4                  # 8 e32 <= a quarter of the 0.1 % mutations tests/test_step_fixture_host.py must see


def oracle_of(c, dtype, kw=None, scalars=None):
    """The oracle holding the case's state (kw / scalars: these instead of the case's -- the host test's mutations)."""
    kw = dict(c.kw, **(kw or {}))
    sc = [float(x) for x in (c.scalars if scalars is None else scalars)]
    nets = {n: layers_from_flat(c.params[n], c.shapes(n)) for n in c.nets}
    if c.td3:
        o = RlkitEquivalentTD3(nets, c.A, dtype=dtype, **kw)
        steps = dict(policy=sc[0], qf1=sc[3], qf2=sc[3])
    else:
        o = RlkitEquivalentSAC(nets, c.A, dtype=dtype, **kw)
        steps = dict(policy=sc[3], qf1=sc[3], qf2=sc[3])
        if o.auto_alpha:
            with torch.no_grad():
                o.log_alpha.fill_(float(np.float32(sc[0])))
            o.alpha_opt.state[o.log_alpha] = _adam_entry(sc[3], [sc[1]], [sc[2]], dtype)
    for net in cases.TRAINED:
        m, v = c.opt[net]
        _set_net_adam(getattr(o, net + "_opt"), getattr(o, net), c.shapes(net), m, v, steps[net], dtype)
    o.n_train_steps_total = int(sc[4])
    return o


def _flat(net):
    return np.concatenate([np.concatenate([w.detach().numpy().ravel(), b.detach().numpy().ravel()])
                           for w, b in zip(net.ws, net.bs)]).astype(np.float64)


def _flat_opt(opt, net, key):
    return np.concatenate([np.concatenate([opt.state[w][key].numpy().ravel(), opt.state[b][key].numpy().ravel()])
                           for w, b in zip(net.ws, net.bs)]).astype(np.float64)


def run(c, dtype, kw=None, scalars=None):
    """One step of the oracle from the case: dict(diag, scales, rows, grads, params, opt, scalars), everything float64
    arrays of the oracle's own values (a float32 oracle's taken up exactly)."""
    o = oracle_of(c, dtype, kw, scalars)
    sc_in = np.asarray(c.scalars if scalars is None else scalars, np.float64)
    diag = o.step(*c.step_args())
    keys = TD3_ROWS if c.td3 else SAC_ROWS
    rows = {name: o.last[keys[name]].detach().numpy().astype(np.float64).ravel() for name in cases.ROW_NAMES[c.algo]}
    grads = {net: np.asarray(oracle_flat_grad(o.last["g_" + net]), np.float64) for net in cases.TRAINED
             if o.last["g_" + net] is not None}
    params = {net: _flat(getattr(o, net)) for net in c.nets}
    opt = {net: tuple(_flat_opt(getattr(o, net + "_opt"), getattr(o, net), k) for k in ("exp_avg", "exp_avg_sq"))
           for net in cases.TRAINED}
    step_of = lambda net: float(getattr(o, net + "_opt").state[getattr(o, net).ws[0]]["step"])     # noqa: E731
    sc = np.zeros(5, np.float64)
    sc[3], sc[4] = step_of("qf1"), o.n_train_steps_total
    assert step_of("qf2") == sc[3]
    if c.td3:
        sc[0] = step_of("policy")
    else:
        assert step_of("policy") == sc[3]
        sc[:3] = sc_in[:3]             # fixed alpha: log_alpha and its moments are not touched
        if o.auto_alpha:
            st = o.alpha_opt.state[o.log_alpha]
            assert float(st["step"]) == sc[3]
            sc[0], sc[1], sc[2] = float(o.log_alpha.detach()), float(st["exp_avg"]), float(st["exp_avg_sq"])
    return dict(diag=OrderedDict(diag), scales=diag_scales(diag, o), rows=rows, grads=grads, params=params, opt=opt,
                scalars=sc)


def tensors_of(c, r):
    return cases.step_tensors(c, r["rows"], r["grads"], r["params"], r["opt"], r["scalars"])


def structure(c, r):
    """The structural claims of a case in a result `r` (asserted of the float64 step before it is frozen)."""
    for net in c.unchanged_params():
        assert np.array_equal(r["params"][net], c.params[net].astype(np.float64)), (c.name, net, "moved")
    for net in cases.TRAINED:
        if net not in c.stepped():
            for got, was in zip(r["opt"][net], c.opt[net]):
                assert np.array_equal(got, was.astype(np.float64)), (c.name, net, "moments moved")
            assert net not in r["grads"], (c.name, net)
    assert set(r["grads"]) == set(c.stepped()), (c.name, sorted(r["grads"]))
    want = cases.counters_out(c)
    assert r["scalars"][3] == want["adam_t"] and r["scalars"][4] == want["n_train_steps_total"], (c.name, r["scalars"])
    if c.td3:
        assert r["scalars"][0] == want["adam_t_pi"], (c.name, r["scalars"])
    elif not c.auto_alpha():
        assert np.array_equal(r["scalars"][:3], c.scalars[:3]), (c.name, r["scalars"])
    term = cases.terminal_rows(c)
    assert term.size >= 1
    rs = np.float64(np.float32(c.kw["reward_scale"]))
    assert np.allclose(r["rows"]["q_target"][term], rs * c.batch["rewards"].ravel()[term].astype(np.float64), rtol=1e-12, atol=0)


def freeze(c):
    """(arrays of the case, its meta entry, report lines)."""
    r64, r32 = run(c, torch.float64), run(c, torch.float32)
    structure(c, r64)
    T64, T32 = tensors_of(c, r64), tensors_of(c, r32)
    assert list(T64) == list(T32)
    values, stats, names, lines = [], [], [], []
    for name, R in T64.items():
        s = float(np.max(np.abs(R)))
        e32 = float(np.max(np.abs(T32[name] - R))) / s if s else 0.0
        assert 8 * e32 <= E32_CAP, f"{c.name}: {name}: 8 e32 = {8 * e32:.3g} > {E32_CAP:g}: change the case's inputs"
        kept = cases.stored_view(c, name, R).astype(np.float32)
        values.append(kept); stats.append((s, e32)); names.append((name, int(kept.size)))
        lines.append(f"  {name:<46s} n {R.size:>6d} kept {kept.size:>6d}  s {s:.4g}  e32 {e32:.3g}")
    diag = []
    for name, v in r64["diag"].items():
        s = float(r64["scales"][name])
        e32 = abs(r32["diag"][name] - v) / s if s else 0.0
        assert 8 * e32 <= E32_CAP, f"{c.name}: {name}: 8 e32 = {8 * e32:.3g} > {E32_CAP:g}"
        diag.append((v, s, e32))
        lines.append(f"  {name:<46s} value {v:+.6g}  s {s:.4g}  e32 {e32:.3g}")
    arrays = OrderedDict([(c.name + "|values", np.concatenate(values)), (c.name + "|stats", np.asarray(stats, np.float64)),
                          (c.name + "|diag", np.asarray(diag, np.float64)), (c.name + "|scalars", r64["scalars"])])
    meta = dict(tensors=names, diag=list(r64["diag"]), inputs=c.checksums(), unchanged=list(c.unchanged_params()),
                stepped=list(c.stepped()), terminal_rows=[int(i) for i in cases.terminal_rows(c)])
    return arrays, meta, lines


def make():
    arrays, meta, report = OrderedDict(), dict(cases=OrderedDict(), torch=torch.__version__, numpy=np.__version__,
                                               grad_stride=cases.GRAD_STRIDE), []
    for name in cases.NAMES:
        c = cases.build(name)
        a, m, lines = freeze(c)
        arrays.update(a)
        meta["cases"][name] = m
        st = a[name + "|stats"]
        i = int(np.argmax(st[:, 1]))
        pos = st[:, 0][st[:, 0] > 0]
        report.append(f"{name}: {c.algo} {(c.O, c.A, c.B)} hidden {c.hidden} / {c.hidden_q}: {len(m['tensors'])} tensors, "
                      f"{a[name + '|values'].size} float32 kept ({4 * a[name + '|values'].size} bytes), s {pos.min():.3g} .. "
                      f"{pos.max():.3g}, largest e32 {st[i, 1]:.3g} ({m['tensors'][i][0]}), largest e32 of a diagnostic "
                      f"{float(a[name + '|diag'][:, 2].max()):.3g}")
        if "--verbose" in sys.argv:
            report += lines
    meta["sha256"] = OrderedDict((k, cases.sha256(v)) for k, v in arrays.items())
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    return arrays, report


def main():
    arrays, report = make()
    print("\n".join(report))
    print(f"torch {torch.__version__}, numpy {np.__version__}")
    if "--check" in sys.argv:
        return
    np.savez_compressed(PATH, **arrays)
    size = os.path.getsize(PATH)
    print(f"wrote {PATH}: {size} bytes, {len(arrays)} arrays")
    with open(PATH[:-len(".npz")] + ".report.txt", "w") as f:          # the report of the file as committed, next to it
        f.write("\n".join(report + [f"torch {torch.__version__}, numpy {np.__version__}", f"{size} bytes, {len(arrays)} arrays"]) + "\n")
    assert size <= MAX_BYTES, f"{size} bytes > {MAX_BYTES}: shrink the hidden sizes, not the list of cases"


if __name__ == "__main__":
    main()
