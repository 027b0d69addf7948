"""GPU: one training step makes, call for call, the C calls that tests/golden/ops_call_trace.json recorded.

conv_tasnet_amd/ops.py is the one place that decides which entry point runs, with which operands, on which stream.  The bitwise
tests (tests/test_gpu_train.py, tests/test_gpu_h3.py) pin WHAT is computed and into which buffer; this module pins the launches
themselves: the name of every ``lib.call`` of one forward / loss / backward / join_side_stream(), in order, with every scalar
argument (byte counts included), every pointer as null or non-null, every pointer table as its length, every integer table as
its values, every ``bytes`` argument, and every ``stream`` / ``side_stream`` argument as "main", "side" or "null" (compared, at
the time of the call, with ops._side_stream() and torch's current stream).  Addresses are not compared.  The cases of
``mode="stream"`` pin chunked inference the same way: the calls of a streaming.StreamingSeparator over two pushes and the flush.

The fixture pins ONE machine: workspace sizes and partial counts follow the CU count, so it stores torch.version.hip, the device
name and the CU count, and a run anywhere else FAILS with the instruction below (it does not skip).  To re-record, check out the
parent of the commit under review (the fixture in the tree was recorded from the commit before ClnBlock and CumLnBlock became one
node over a record of the norm's calls; its older cases expand to what the fixture before it held; since then only the workspace
byte counts of ctn_tcn_gln_bwd / ctn_tcn_cln_bwd were lowered, by arithmetic on the recorded values, when the second split-K slab
buffer left both workspaces: recorded - align256(max(ctn_pw_wgrad_workspace(M, H, B, Kp), ctn_pw_wgrad_workspace(M, B, H, Kp))) with
the slab size from the parent's library under the case's arithmetic), build it, copy this module over
its own, and run there
    python tests/test_gpu_ops_trace.py --record tests/golden/ops_call_trace.json
never from a tree whose ops.py is the one under review.
"""
import ctypes
import json
import os
import sys

import pytest
import torch

import conftest  # noqa: F401  puts the repository root on sys.path, also when this file runs as a script
from oracle import ctn_oracle as O

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402
from conv_tasnet_amd.optim import FlatAdam  # noqa: E402
from conv_tasnet_amd.streaming import StreamingSeparator  # noqa: E402

DEV = "cuda:0"
FIXTURE = os.path.join(conftest.GOLDEN, "ops_call_trace.json")
NARROW = (32, 20, 16, 32, 3, 4, 2, 2)
WIDE = (64, 20, 64, 128, 3, 3, 2, 2)          # >= 64 rows everywhere: reaches the b6 / h3 piece forms
NORMS = {"gln": ("gLN", False), "cln": ("cLN", True), "bn": ("BN", False), "cumln": ("cumLN", True)}
BASE = dict(dims=WIDE, flat=True, arith="h3", cln_fuse=2, gln_fuse=0, side=True, buckets=False, no_grad=False)


def _cases():
    """{name: settings}.  The base grid, then one setting at a time moved away from BASE on the wide model with sinks."""
    cases = {}

    def add(name, norm, composite, **kw):
        cases["%s_%s_%s" % (norm, "composite" if composite else "perkernel", name)] = dict(BASE, norm=norm, composite=composite, **kw)

    for composite in (True, False):
        for norm in ("gln", "cln"):
            for dims, dname in ((NARROW, "narrow"), (WIDE, "wide")):
                for flat in (True, False):
                    add("%s_%s" % (dname, "sinks" if flat else "autograd"), norm, composite, dims=dims, flat=flat)
            for arith in ("fp32", "b6", "h3"):
                add("arith_" + arith, norm, composite, arith=arith)
            add("side_off", norm, composite, side=False)
            add("buckets2", norm, composite, buckets=True)
            add("no_grad", norm, composite, no_grad=True)
        for level in (0, 1, 2):
            add("cln_fuse%d" % level, "cln", composite, cln_fuse=level)
        for level in (0, 1):
            add("gln_fuse%d" % level, "gln", composite, gln_fuse=level)
    add("narrow_sinks", "bn", False, dims=NARROW)
    # cumLN has no composite stack: per kernel only; ctn_tune("cln_fuse") must not reach it
    for dims, dname in ((NARROW, "narrow"), (WIDE, "wide")):
        for flat in (True, False):
            add("%s_%s" % (dname, "sinks" if flat else "autograd"), "cumln", False, dims=dims, flat=flat)
    for arith in ("fp32", "b6", "h3"):
        add("arith_" + arith, "cumln", False, arith=arith)
    add("side_off", "cumln", False, side=False)
    add("no_grad", "cumln", False, no_grad=True)
    add("cln_fuse0", "cumln", False, cln_fuse=0)
    add("wide_sinks", "bn", False)
    add("narrow_autograd", "bn", False, dims=NARROW, flat=False)
    # chunked inference: StreamingSeparator on the narrow model, eager
    for norm in ("cln", "cumln"):
        cases["%s_stream" % norm] = dict(BASE, norm=norm, composite=False, dims=NARROW, flat=False, mode="stream")
    return cases


CASES = _cases()


class _Buckets:
    """Stand-in for parallel.GradientBuckets, as in tests/test_gpu_optim.py: two blocks per backward call, no collective."""
    blocks_per_bucket = 2

    def __init__(self):
        self.works, self.covered = [], []

    def bucket_ready(self, sinks):
        pass


def _normalise(name, args):
    _, argtypes, argnames = ctn.lib.protos[name]
    assert len(args) == len(argtypes), "%s: %d arguments for %d parameters" % (name, len(args), len(argtypes))
    dev = torch.device(DEV)
    out = [name]
    for a, ty, nm in zip(args, argtypes, argnames):
        if nm in ("stream", "side_stream"):
            side, cur = ops._side_stream(dev).cuda_stream, torch.cuda.current_stream(dev).cuda_stream
            if a == side:
                a = "side"
            elif not a and nm == "side_stream":         # 0 = no second stream (the default stream is 0 as well)
                a = "null"
            elif a == cur:
                a = "main"
            else:
                a = "null" if not a else "other"
        elif isinstance(a, bytes):
            a = {"bytes": a.decode("latin-1")}
        elif isinstance(a, ctypes.Array):
            a = {"table": len(a)} if a._type_ is ctypes.c_void_p else {"ints": list(a)}
        elif ty is ctypes.c_void_p:
            a = "ptr" if a else "nullptr"
        out.append(a)
    return out


def _trace(case, mp):
    """The normalised lib.call sequence of one step under `case`; every switch is put back before it returns."""
    norm_type, causal = NORMS[case["norm"]]
    saved = (ops.gemm_arith(), ctn.lib.ctn_cln_fuse(), ctn.lib.ctn_gln_fuse())
    call, calls = ctn.lib.call, []

    def recorder(name, *args):
        calls.append(_normalise(name, args))
        return call(name, *args)

    try:
        ops.set_gemm_arith(case["arith"])
        call("ctn_tune", b"cln_fuse", case["cln_fuse"])
        call("ctn_tune", b"gln_fuse", case["gln_fuse"])
        ops.set_grad_buckets(_Buckets() if case["buckets"] else None)
        mp.setattr(ops, "_COMPOSITE", case["composite"])
        mp.setattr(ops, "_SIDE_ENABLED", case["side"])
        torch.manual_seed(3)
        m = ctn.ConvTasNet(*case["dims"], norm_type=norm_type, causal=causal).to(DEV)
        opt = FlatAdam(m.parameters(), lr=1e-3) if case["flat"] else None
        mix, lens, src = (t.to(DEV) for t in O.synth_batch(5, 3, 4007))
        if opt is not None:
            opt.zero_grad()
        torch.cuda.synchronize()
        stream = case.get("mode") == "stream"
        if stream:
            sep, hop = StreamingSeparator(m, batch=2), case["dims"][1] // 2
        mp.setattr(ctn.lib, "call", recorder)
        if stream:                                  # a push of 40 hops, one of 7, the flush
            sep.push(mix[:2, :40 * hop])
            sep.push(mix[:2, 40 * hop:47 * hop])
            sep.flush()
        elif case["no_grad"]:
            with torch.no_grad():
                m(mix)
        else:
            ctn.cal_loss(src, m(mix), lens)[0].backward()
            ops.join_side_stream()
        torch.cuda.synchronize()
    finally:
        mp.undo()
        ops.set_grad_buckets(None)
        call("ctn_tune", b"gln_fuse", saved[2])
        call("ctn_tune", b"cln_fuse", saved[1])
        ops.set_gemm_arith(saved[0])
        ops._ws_cache.clear()
    return calls


def _machine():
    p = torch.cuda.get_device_properties(DEV)
    return {"hip_version": str(torch.version.hip), "device": p.name, "compute_units": p.multi_processor_count}


def record(path):
    """{"machine", "calls": every distinct call once, "cases": {name: indices into calls}} -- a step repeats few distinct calls."""
    index, cases = {}, {}
    for name, case in CASES.items():
        with pytest.MonkeyPatch.context() as mp:
            trace = _trace(case, mp)
        cases[name] = [index.setdefault(json.dumps(c), len(index)) for c in trace]
        print("%-40s %4d calls" % (name, len(trace)))
    table = [json.loads(k) for k in index]
    with open(path, "w") as f:
        json.dump({"machine": _machine(), "calls": table, "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print("recorded %d cases, %d distinct calls on %s -> %s (%d bytes)" % (len(cases), len(table), _machine(), path, os.path.getsize(path)))


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_exactly_the_parametrised_cases(recorded):
    assert sorted(recorded["cases"]) == sorted(CASES)
    assert all(len(v) > 0 for v in recorded["cases"].values())


@pytest.mark.parametrize("name", sorted(CASES))
def test_step_makes_the_recorded_calls(recorded, name, monkeypatch):
    assert recorded["machine"] == _machine(), \
        ("tests/golden/ops_call_trace.json was recorded on %s and this is %s: workspace sizes and partial counts follow the machine -- "
         "re-record it from the PARENT commit (python tests/test_gpu_ops_trace.py --record tests/golden/ops_call_trace.json)"
         % (recorded["machine"], _machine()))
    assert sorted(recorded["cases"]) == sorted(CASES), "the fixture and the parametrised cases differ: re-record from the parent commit"
    want = [recorded["calls"][i] for i in recorded["cases"][name]]
    got = json.loads(json.dumps(_trace(CASES[name], monkeypatch)))          # tuples -> lists, as the fixture was stored
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s: call %d differs\n  recorded %s\n  made     %s" % (name, i, w, g)
    n = min(len(got), len(want))
    assert len(got) == len(want), "%s: %d calls made, %d recorded (the first %d agree); the next one is %s" % (
        name, len(got), len(want), n, max(got, want, key=len)[n:n + 1])


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_gpu_ops_trace.py --record PATH.json   (on a build of the parent commit)")
    record(sys.argv[2])
