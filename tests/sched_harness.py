"""Schedule-perturbation harness for the two-stream ordering (tests/test_gpu_sched_stacks.py, tests/test_gpu_sched_step.py).

The same work is run many times, each time with ONE launch held back by a bounded delay on its own stream (ctn_delay /
ctn_delay_arm, include/ctn_hip.h), and every output must have the bits of the unperturbed run.  If a consumer on stream A is not
ordered, directly or transitively, behind its producer on stream B, then holding the producer back for longer than A needs to reach
the consumer makes the consumer read what the buffer held before -- the poison written ahead of every run -- and a writer that
overruns a reader shows the same way.  Sweeping the delay over every launch of both streams exposes every cross-stream dependency
once.  No kernel changes numerically, all accesses stay inside live allocations: a wrong schedule gives NaN or other bits, nothing
else.  Every run is one fixed delay at one fixed place; nothing is retried, and the first failure ends the sweep.

Delay length: D = max(2 ms, 4 x the GPU time of the unperturbed run between two events), at most the library's 20 ms.  The
unperturbed time includes the host's enqueueing, which is what the delayed stream's peer needs to run to the end of the call; it
sizes the delay and is no pass criterion.  Every perturbed run asserts that its delay happened: the count of the hook, GPU time
between the events around the run >= D, and GPU time around the delay itself >= D (two events around ctn_delay on its stream; for
a launch group its own probe record, which the delay sits inside).  A run that fails there is a HarnessError, not a schedule finding.
"""
import contextlib
import ctypes
import re

import torch

import conv_tasnet_amd as ctn
from conv_tasnet_amd import _lib

MIN_DELAY_US, MAX_DELAY_US = 2000, 20000
# family ids of the probe (csrc/ctn_block.hip), in id order
FAMILIES = ("K1", "K2", "K3", "B1", "B2", "B3", "B4", "B5", "B6", "finalize", "prep", "cln_fwd", "cln_bwd", "taps", "-", "frame")
# launch groups that the backward passes issue on the second stream when they have one: both weight gradients and the fixed-order sums
SIDE_FAMILIES = (FAMILIES.index("B2"), FAMILIES.index("B6"), FAMILIES.index("finalize"), FAMILIES.index("taps"))


class HarnessError(AssertionError):
    """The harness itself did not do what it claims (the delay was not issued, or did not last): not a finding about the schedule."""


class ScheduleMismatch(AssertionError):
    """A perturbed run differs from the unperturbed one.  where = ("group", g) | ("call", k) | ("call", k, "group", g)."""

    def __init__(self, where, message):
        super().__init__(message)
        self.where = where


def poison(*tensors):
    """NaN bytes (0xFF: a NaN in fp32 and fp64, -1 in the integer types) into every tensor; lists and tuples are walked."""
    for t in tensors:
        if t is None:
            continue
        if isinstance(t, (list, tuple)):
            poison(*t)
        elif t.numel():
            if t.is_contiguous():
                t.reshape(-1).view(torch.uint8).fill_(0xFF)
            else:
                t.fill_(float("nan") if t.is_floating_point() else -1)


# every way to get uninitialised device memory from Python; tests/test_host_cpu.py checks that the package uses no other
UNINITIALISED = ("empty", "empty_like", "empty_strided")            # torch.*
UNINITIALISED_METHODS = ("new_empty", "new_empty_strided")          # torch.Tensor.*


@contextlib.contextmanager
def poisoned_allocations():
    """While active, every device tensor that Python gets uninitialised (torch.empty, empty_like, empty_strided, Tensor.new_empty,
    new_empty_strided) is born poisoned, filled on the current stream: the buffers that the Python side allocates per call cannot be
    reached from a test, and without this a racing reader would find the bits that the previous, identical run left at the same
    address of the caching allocator."""
    def wrap(real):
        def alloc(*a, **kw):
            t = real(*a, **kw)
            if t.is_cuda:
                poison(t)
            return t
        return alloc

    saved = {nm: getattr(torch, nm) for nm in UNINITIALISED}
    bases = {nm: getattr(torch.Tensor, nm) for nm in UNINITIALISED_METHODS}
    for nm, real in saved.items():
        setattr(torch, nm, wrap(real))
    for nm, real in bases.items():
        setattr(torch.Tensor, nm, wrap(real))
    try:
        yield
    finally:
        for nm, real in saved.items():
            setattr(torch, nm, real)
        for nm in bases:
            delattr(torch.Tensor, nm)           # (the wrapper sat on torch.Tensor over the method of its base class)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def snapshot(outputs):
    return {k: v.detach().clone() for k, v in outputs().items()}


def differences(got, ref):
    """-> one line per output whose bits differ."""
    out = []
    assert sorted(got) == sorted(ref)
    for k in ref:
        if not same_bits(got[k], ref[k]):
            g, r = got[k].reshape(-1), ref[k].reshape(-1)
            bad = int((g.view(torch.uint8) != r.view(torch.uint8)).sum()) if g.shape == r.shape else -1
            nan = int(torch.isnan(g).sum()) if g.is_floating_point() else 0
            out.append("%s: %d of %d bytes differ, %d NaN" % (k, bad, g.numel() * g.element_size(), nan))
    return out


def timed(run):
    """GPU microseconds between two events around run(), which must end with the second stream joined into the current one."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def delay_for(unperturbed_us):
    return int(min(MAX_DELAY_US, max(MIN_DELAY_US, 4.0 * unperturbed_us + 1.0)))


def _disarm():
    L = ctn.lib.load()
    L.ctn_delay_groups()
    L.ctn_probe_enable(0)


def count_groups(run):
    """Dry run with the hook counting only -> (number of launch groups, their family ids in issue order)."""
    L = ctn.lib.load()
    try:
        ctn.lib.call("ctn_probe_enable", 1)
        ctn.lib.call("ctn_delay_arm", -1, 0)
        run()
        torch.cuda.synchronize()
        n = L.ctn_delay_groups()
        fam, us = (ctypes.c_int * 4096)(), (ctypes.c_float * 4096)()
        m = L.ctn_probe_read(fam, us, 4096)
    finally:
        _disarm()
    if n <= 0 or m != n:
        raise HarnessError("the delay hook counted %d launch groups and the probe %d" % (n, m))
    return n, [fam[i] for i in range(n)]


def _fam(fams, g):
    return FAMILIES[fams[g]] if 0 <= fams[g] < len(FAMILIES) else "family %d" % fams[g]


def _probe_read():
    """-> microseconds of every recorded launch group, in issue order; ends the recording (it waits for the events: call it after
    the run, never inside it)."""
    fam, us = (ctypes.c_int * 4096)(), (ctypes.c_float * 4096)()
    m = ctn.lib.load().ctn_probe_read(fam, us, 4096)
    return [us[i] for i in range(min(m, 4096))]


def run_with_group_delay(run, g, micros):
    """One run with the delay ahead of launch group g -> GPU microseconds; HarnessError unless the delay was issued and lasted: the
    hook's count, the delayed group's own probe record (the delay sits behind its first event) and the time around the run."""
    L = ctn.lib.load()
    try:
        ctn.lib.call("ctn_probe_enable", 1)
        ctn.lib.call("ctn_delay_arm", g, micros)
        us = timed(run)
        cnt = L.ctn_delay_groups()
        rec = _probe_read()
    finally:
        _disarm()
    if cnt != g + 1:
        raise HarnessError("group %d: the hook stopped at count %d: the delay was not issued" % (g, cnt))
    if len(rec) <= g or rec[g] < micros or us < micros:
        raise HarnessError("group %d: its own record shows %.0f us and the run %.0f us, delay %d us: the delay did not happen"
                           % (g, rec[g] if len(rec) > g else -1.0, us, micros))
    return us


def sweep_groups(run, outputs, scratch=None, tag=""):
    """run(): one composite call (or several) ending joined; outputs() -> {name: tensor}; scratch() -> tensors to poison before
    every run (outputs, activation slots, gradient destinations, workspaces).  -> the reference snapshot."""
    def fresh():
        if scratch is not None:
            poison(*scratch())

    fresh()
    n, fams = count_groups(run)
    fresh()
    t0 = timed(run)
    ref = snapshot(outputs)
    D = delay_for(t0)
    print("SCHED %s groups=%d unperturbed=%.0fus D=%dus" % (tag, n, t0, D))
    for g in range(n):
        fresh()
        run_with_group_delay(run, g, D)
        bad = differences(snapshot(outputs), ref)
        if bad:
            raise ScheduleMismatch(("group", g), "%s: delay of %d us ahead of launch group %d of %d (%s; issue order %s): %s"
                                   % (tag, D, g, n, _fam(fams, g), " ".join(_fam(fams, i) for i in range(n)), "; ".join(bad)))
    return ref


# ---- one level up: the calls that Python makes -------------------------------------------------------------------------------
def writable_pointers(path=_lib.HEADER):
    """{entry point: names of its pointer parameters that are not pointers to const} -- what a call may write."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    out = {}
    for m in re.finditer(r"\b(ctn_\w+)\s*\(([^)]*)\)\s*;", text):
        names = set()
        for a in m.group(2).split(","):
            a = a.strip()
            if "*" in a and not a.startswith("const "):
                names.add(re.search(r"(\w+)$", a).group(1))
        out[m.group(1)] = names
    return out


class _Tap:
    """Stands in for lib.call.  plan: None = record (and count the launch groups inside every composite call); ("none", -1) = pass
    everything through; ("call", k, D) = ctn_delay on the stream argument of call k, ahead of it; ("group", k, g, D) = the hook armed for group g of call k."""

    def __init__(self, plan):
        self.plan, self.calls, self.first, self.fired, self.events, self.delay_us = plan, [], None, None, None, None
        self.real = ctn.lib.call            # the bound method of the class

    def end_of_first_step(self):
        self.first = len(self.calls)

    def __call__(self, name, *args):
        k = len(self.calls)
        argnames = ctn.lib.protos[name][2]
        stream = args[argnames.index("stream")] if "stream" in argnames else None
        composite = "side_stream" in argnames
        rec = {"name": name, "args": args, "stream": stream, "composite": composite, "groups": None}
        self.calls.append(rec)
        plan, L = self.plan, ctn.lib.load()
        if plan is None and composite:
            self.real("ctn_delay_arm", -1, 0)
            try:
                return self.real(name, *args)
            finally:
                rec["groups"] = L.ctn_delay_groups()
        if plan is not None and plan[1] == k:
            if plan[0] == "call":           # two events around the delay kernel itself, on its stream
                st = torch.cuda.ExternalStream(stream) if stream else torch.cuda.default_stream()
                self.events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                self.events[0].record(st)
                self.real("ctn_delay", stream or 0, plan[2])
                self.events[1].record(st)
                self.fired = name
            else:                           # a recording from here on: record g is launch group g of this call
                self.real("ctn_probe_enable", 1)
                self.real("ctn_delay_arm", plan[2], plan[3])
                try:
                    return self.real(name, *args)
                finally:
                    self.fired = (name, L.ctn_delay_groups())
        return self.real(name, *args)


def _play(step, plan):
    tap = _Tap(plan)
    ctn.lib.call = tap                      # an instance attribute over the method, as monkeypatch.setattr(ctn.lib, "call", ...) does
    try:
        us = timed(lambda: step(tap.end_of_first_step))
        if tap.events is not None:
            tap.delay_us = tap.events[0].elapsed_time(tap.events[1]) * 1e3
        elif plan is not None and plan[0] == "group":
            rec = _probe_read()
            tap.delay_us = rec[plan[2]] if len(rec) > plan[2] else -1.0
    finally:
        del ctn.lib.call
        _disarm()
    if tap.first is None:
        raise HarnessError("the step never called end_of_first_step()")
    return tap, us


def record_calls(step):
    """The lib.call sequence of one unperturbed step -> (the records of every call, the number of calls of the first step)."""
    tap, _ = _play(step, None)
    return tap.calls, tap.first


def _describe(rec, k, side_ptr):
    where = "no stream" if rec["stream"] is None else ("second stream" if side_ptr and rec["stream"] == side_ptr else "main stream")
    return "call %d = %s (%s)" % (k, rec["name"], where)


def sweep_calls(step, outputs, tag="", only=None, side_ptr=None, ref=None):
    """step(end_of_first_step): zero_grad .. the join of the second step, poisoning what it can reach itself; it calls
    end_of_first_step() where the first step ends: the delay falls on the calls before that.  Run k puts ctn_delay on the `stream`
    argument of the k-th lib.call, ahead of it; for a composite call (one with a `side_stream` argument) the launch groups inside it
    are swept through ctn_delay_arm as well.  only: restrict the sweep to these call indices.  ref: compare with this snapshot instead
    of the unperturbed run of `step` (a mutant's own unperturbed run is a race, not a reference).  -> the reference snapshot."""
    calls, first = record_calls(step)
    tap, t0 = _play(step, ("none", -1))     # no delay anywhere
    ref = snapshot(outputs) if ref is None else ref
    D = delay_for(t0)
    ks = [k for k in range(first) if calls[k]["stream"] is not None and (only is None or k in only)]
    ngroups = sum(calls[k]["groups"] or 0 for k in ks)
    print("SCHED %s calls=%d (first step %d, swept %d, launch groups inside composites %d) unperturbed=%.0fus D=%dus"
          % (tag, len(calls), first, len(ks), ngroups, t0, D))
    if [c["name"] for c in tap.calls] != [c["name"] for c in calls]:
        raise HarnessError("%s: two unperturbed runs made different calls" % tag)

    def one(plan, where, what):
        tap, us = _play(step, plan)
        if tap.fired is None or [c["name"] for c in tap.calls] != [c["name"] for c in calls]:
            raise HarnessError("%s: %s: the delay was not issued, or the run made other calls than the recorded ones" % (tag, what))
        if plan[0] == "group" and tap.fired[1] != plan[2] + 1:
            raise HarnessError("%s: %s: the hook stopped at count %d" % (tag, what, tap.fired[1]))
        if us < D or tap.delay_us is None or tap.delay_us < D:
            raise HarnessError("%s: %s: %.0f us of GPU time around the run and %.0f us around the delay itself, delay %d us: the delay "
                               "did not happen" % (tag, what, us, -1.0 if tap.delay_us is None else tap.delay_us, D))
        bad = differences(snapshot(outputs), ref)
        if bad:
            raise ScheduleMismatch(where, "%s: delay of %d us ahead of %s: %s" % (tag, D, what, "; ".join(bad)))

    for k in ks:
        what = _describe(calls[k], k, side_ptr)
        one(("call", k, D), ("call", k), what)
        for g in range(calls[k]["groups"] or 0):
            one(("group", k, g, D), ("call", k, "group", g), "launch group %d of %d inside %s" % (g, calls[k]["groups"], what))
    return ref
