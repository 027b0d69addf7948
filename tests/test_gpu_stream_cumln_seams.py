"""The cumulative fused streaming stack (csrc/ctn_stream.hip: ctn_stream_tcn_cumln, its ragged form, ctn_stream_cum_reset_slots) through
the C ABI against tests/stream_cumln_oracle.py in fp64, on guarded buffers.

What runs (stream_cumln_oracle.CASES, max_frames = 16, three streams: ordinary, quiet, 100 times louder):
    reference  every case in both cuts of stream_oracle.stack_plan (calls of 1 .. 16 frames until every ring has wrapped three times) and
               case 0 over 4096 frames in 16-frame calls, against the fp64 reference within LIMIT["stack_y_cum"]; the records' frame
               counts afterwards; the same bits after a reset of state and records.
    bits       the two cuts; stream 0 alone (M = 1) against stream 0 of the three; the row-split form (M = 3) against the stage form
               (the same streams as slots of M = 130).
    ragged     six slots (and 130, the ragged stage form) with counts 16, 0, 1, 7, 21, -3 rotated from step to step: every slot bitwise a
               plain M = 1 call of its frames; a slot with nf <= 0 keeps y, rings, position word and both banks of its records.
    reset      a slot that carried the loud stream, reset with ctn_stream_reset_slots + ctn_stream_cum_reset_slots, is a fresh slot;
               its neighbours' records are untouched.
    errors     frames = 17, null and misaligned cum: CTN_ERR_ARG and nothing written.
    defect     ctn_stream_tcn_cln (the per-frame kernels) on the same packed weights is far outside the limit on every case.

Limit: stream_cumln_oracle.LIMIT["stack_y_cum"] = 2e-6 of max |ref| per stream: 4x what the fp32 model loses against fp64 on these inputs
(test_stream_cumln_cpu.py), never what the kernels give.

Figures of the first MI355X run (the `CUM` lines of -s), both cuts alike.  A record, not new limits.
    (16, 16, 3, (1, 2)) 1.87e-07   (48, 80, 3, (1, 5, 16)) 4.22e-07   (16, 528, 3, (8, 8)) 7.49e-07   (512, 240, 1, (1, 1)) 8.75e-07
    long plan 2.65e-07 (last 256 frames 1.74e-07); the per-frame kernels on the same weights: 0.29 .. 0.58
"""
import ctypes

import pytest
import torch

import stream_cumln_oracle as CO
import stream_oracle as SO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
F32, I32, I64 = torch.float32, torch.int32, torch.int64
GUARD, SENT = 4096, -7777.0
HDR, TAB = 64, 8
LIM = CO.LIMIT["stack_y_cum"]
WORST = {}
_RUNS = {}
CASES = range(len(CO.CASES))


@pytest.fixture(autouse=True)
def _own_lines():
    print()


def call(name, *args):
    ctn.lib.call(name, *args, ops._stream())


class Guarded:
    """A buffer pre-filled with `fill` between two runs of GUARD sentinel elements of the same allocation."""

    def __init__(self, *shape, fill=NAN, raw=False):
        self.n, self.raw = 1, raw                   # raw: not fp32 values (the records' fp64 bits may read as NaN)
        for s in shape:
            self.n *= s
        self.flat = torch.full((self.n + 2 * GUARD,), SENT, dtype=F32, device=DEV)
        self.t = self.flat[GUARD:GUARD + self.n].view(shape)
        self.t.fill_(fill)

    def ptr(self):
        return self.t.data_ptr()

    def ok(self, where):
        assert bool((self.flat[:GUARD] == SENT).all()) and bool((self.flat[GUARD + self.n:] == SENT).all()), (where, "a guard element was written")
        assert self.raw or not bool(torch.isnan(self.t).any()), (where, "NaN left")
        return self.t


def table(counts):
    t = torch.zeros((len(counts), TAB), dtype=I32)
    t[:, 0] = torch.tensor(counts, dtype=I32)
    t[:, 1] = t[:, 0]
    return t.to(DEV)


class Stack:
    """Packed weights, a guarded zeroed state and guarded zeroed record banks of CASES[ci] for M slots."""

    def __init__(self, ci, M):
        c, (p, _) = CO.CASES[ci], CO.stack_inputs(ci)
        lib = ctn.lib.load()
        self.c, self.M, self.nb = c, M, len(c.dil)
        self.dil = (ctypes.c_int * self.nb)(*c.dil)
        self.state_bytes = lib.ctn_stream_state_bytes(M, c.H, c.P, self.dil, self.nb, c.max_frames)
        self.rings = [SO.ring_len(c.P, d, c.max_frames) for d in c.dil]
        self.state = Guarded(self.state_bytes // 4, fill=0.0)
        self.cum_bytes = lib.ctn_stream_cum_bytes(M, self.nb)
        assert self.cum_bytes == 2 * M * self.nb * 2 * 32
        self.cum = Guarded(self.cum_bytes // 4, fill=0.0, raw=True)
        assert self.cum.ptr() % 16 == 0 and self.state.ptr() % 16 == 0
        self.packed = torch.empty(lib.ctn_stream_pack_bytes(c.B, c.H, c.P, self.nb), dtype=torch.uint8, device=DEV)
        self.params = [getattr(b, k).to(F32).contiguous().to(DEV) for b in p.blocks for k in SO.BLOCK_ORDER]
        call("ctn_stream_pack", ops._ptr_table(self.params), self.nb, c.B, c.H, c.P, self.packed.data_ptr())
        self.pos = torch.zeros(M, dtype=I32, device=DEV)

    def reset(self):
        call("ctn_stream_reset", self.state.ptr(), self.state_bytes)
        self.cum.t.zero_()
        self.pos.zero_()

    def records(self):
        """Both banks as 64-bit words [2 banks, M, nblocks, 2 norms, 4]: C1, C2 (fp64 bits), frames, unused."""
        return self.cum.t.view(I64).view(2, self.M, self.nb, 2, 4)

    def counts(self, bank=0):
        return self.records()[bank, :, :, :, 2]

    def buffer(self, y, counts=None):
        g = Guarded(*y.shape)
        g.t.copy_(y)
        if counts is not None:
            for m, n in enumerate(counts):
                g.t[m, :, n:] = SENT
        return g

    def args(self, g):
        return (self.packed.data_ptr(), self.dil, self.nb, g.ptr(), self.state.ptr())

    def push(self, y, where, fn="ctn_stream_tcn_cumln"):
        """One plain call on y [M, B, f] -> the result (device)."""
        c, g = self.c, self.buffer(y)
        extra = (self.cum.ptr(),) if fn == "ctn_stream_tcn_cumln" else ()
        call(fn, *self.args(g), *extra, self.M, c.B, c.H, c.P, y.shape[2], c.max_frames)
        torch.cuda.synchronize()
        self.state.ok(where), self.cum.ok(where)
        return g.ok(where)

    def push_ragged(self, y, counts, where):
        """One ragged step: y [M, B, F], counts as given to the table (the kernels clamp them to 0 .. F) -> the whole buffer."""
        c, F = self.c, y.shape[2]
        g, tab = self.buffer(y, [min(max(n, 0), F) for n in counts]), table(counts)
        call("ctn_stream_tcn_cumln_ragged", *self.args(g), self.cum.ptr(), tab.data_ptr(), self.pos.data_ptr(), self.M, c.B, c.H, c.P, F, c.max_frames)
        torch.cuda.synchronize()
        self.state.ok(where), self.cum.ok(where)
        return g.ok(where)

    def slot_rings(self, m):
        c, out, off = self.c, [], HDR
        for R in self.rings:
            out.append(self.state.t[off + m * c.H * R:off + (m + 1) * c.H * R])
            off += self.M * c.H * R
        return torch.cat(out)


def run_plan(s, y, plan, where, **kw):
    outs, t0 = [], 0
    for i, n in enumerate(plan):
        outs.append(s.push(y[:, :, t0:t0 + n], where + (i, n), **kw))
        t0 += n
    return torch.cat(outs, 2)


def main_run(ci):
    """cut 0 of a case at M = 3, shared by the tests of this module -> (Stack, y [3, B, T])."""
    if ci not in _RUNS:
        _, y = CO.stack_inputs(ci)
        s = Stack(ci, CO.M_TEST)
        _RUNS[ci] = (s, run_plan(s, y, CO.plans(ci)["cut0"], ("cum stack", ci)))
    return _RUNS[ci]


def note(e, where):
    if e > WORST.get("stack_y_cum", (-1.0,))[0]:
        WORST["stack_y_cum"] = (e, where)


@pytest.mark.parametrize("ci", CASES, ids=CO.CASE_IDS)
def test_stack_against_reference(ci):
    c, (_, y), ref = CO.CASES[ci], CO.stack_inputs(ci), CO.stack_reference(ci)
    s, got = main_run(ci)
    T = y.shape[2]
    e = CO.rel_err(got.cpu(), ref)
    per = [CO.rel_err(got[m:m + 1].cpu(), ref[m:m + 1]) for m in range(3)]
    note(e, "case %s cut0" % (tuple(c[:4]),))
    print("CUM stack %-26s frames %3d  y=%.2e (ordinary %.2e quiet %.2e loud %.2e)  limit %.0e" % (tuple(c[:4]), T, e, *per, LIM))
    assert e < LIM, (ci, e)
    assert bool((s.counts(0) == T).all()) and bool((s.counts(1) == T).all()) and s.pos.sum().item() == 0
    assert int(s.state.t[:1].view(I32).item()) == T
    other = run_plan(Stack(ci, CO.M_TEST), y, CO.plans(ci)["cut1"], ("cut 1", ci))
    e1 = CO.rel_err(other.cpu(), ref)
    print("CUM stack %-26s cut1        y=%.2e" % (tuple(c[:4]), e1))
    assert e1 < LIM and torch.equal(got, other), (ci, "another cut of the same signal")
    s.reset()
    assert float(s.state.t.abs().sum()) == 0.0
    again = run_plan(s, y, CO.plans(ci)["cut0"], ("again", ci))
    assert torch.equal(got, again), (ci, "after a reset of state and records the plan gives other bits")


def test_long_plan_against_reference():
    (_, y), ref = CO.stack_inputs(0, True), CO.stack_reference(0, True)
    s = Stack(0, CO.M_TEST)
    got = run_plan(s, y, CO.plans(0)["long"], ("long",))
    e = CO.rel_err(got.cpu(), ref)
    tail = CO.rel_err(got[:, :, -256:].cpu(), ref[:, :, -256:])
    note(e, "case 0 long")
    print("CUM stack long plan: %d frames in %d calls  y=%.2e (last 256 frames %.2e)  limit %.0e" % (y.shape[2], y.shape[2] // 16, e, tail, LIM))
    assert e < LIM and tail < LIM
    assert bool((s.counts(0) == CO.LONG_FRAMES).all())


@pytest.mark.parametrize("ci", CASES, ids=CO.CASE_IDS)
def test_bits_do_not_depend_on_the_other_streams(ci):
    _, y = CO.stack_inputs(ci)
    _, got = main_run(ci)
    solo = run_plan(Stack(ci, 1), y[:1], CO.plans(ci)["cut1"], ("M = 1", ci))
    assert torch.equal(got[:1], solo), (ci, "stream 0 of M = 3 against M = 1 in another cut")


def test_bits_do_not_depend_on_the_kernel_form():
    """M = 3: two launches per block, up to 16 workgroups per stream.  M = 130: no room for two workgroups per stream, the stage kernel."""
    _, y = CO.stack_inputs(0)
    _, got = main_run(0)
    M = 130
    s = Stack(0, M)
    outs = run_plan(s, y[torch.arange(M) % 3], CO.plans(0)["cut0"], ("stage", 0))
    for m in (0, 1, 2, 64, 65, 127, 128, 129):
        assert torch.equal(outs[m], got[m % 3]), ("stage form", "slot %d" % m)
    assert bool((s.counts(0) == y.shape[2]).all())


@pytest.mark.parametrize("ci,M", [(0, 6), (1, 6), (0, 130)], ids=["B16-H16-rows", "B48-H80-rows", "B16-H16-stage"])
def test_ragged_slots_are_plain_calls(ci, M):
    """Counts 16, 0, 1, 7, 21, -3 rotated by one slot per step (slot m of more than six: the count of slot m % 6).  The first six slots
    have a twin with M = 1 that gets a plain call of the slot's frames."""
    _, y = CO.stack_inputs(ci)
    s, twins, cur = Stack(ci, M), [Stack(ci, 1) for _ in range(6)], [0] * M
    for step, F in enumerate((16, 16, 16, 7, 16, 16)):
        six = SO.ragged_counts(F)
        raw = [six[(m + step) % 6] for m in range(M)]
        eff = [min(max(n, 0), F) for n in raw]
        yin = torch.stack([y[m % 3, :, cur[m]:cur[m] + F] for m in range(M)])
        pos0, rec0 = s.pos.clone(), s.records().clone()
        rings0 = [s.slot_rings(m).clone() for m in range(6)]
        out = s.push_ragged(yin, raw, ("ragged", ci, step))
        rec1 = s.records()
        for m, n in enumerate(eff):
            where = (ci, "step %d" % step, "slot %d" % m, "nf %d of %d" % (n, F))
            assert bool((out[m, :, n:] == SENT).all()), (where, "columns from nf on were written")
            assert int(s.pos[m]) == int(pos0[m]) + n, where
            if n == 0:
                assert torch.equal(rec1[:, m], rec0[:, m]), (where, "records of an idle slot changed")
            else:
                assert bool((rec1[0, m, :, :, 2] == cur[m] + n).all()), (where, "frame counts")
            if m < 6 and n == 0:
                assert torch.equal(s.slot_rings(m), rings0[m]), (where, "rings of an idle slot changed")
            elif m < 6:
                alone = twins[m].push(yin[m:m + 1, :, :n], where)
                assert torch.equal(out[m, :, :n], alone[0]), (where, "differs from the plain M = 1 call")
                assert torch.equal(rec1[0, m], twins[m].records()[0, 0]), (where, "records differ from the plain call's")
            cur[m] += n
    assert min(cur) >= 24


def test_reset_slots_gives_a_fresh_slot_and_leaves_the_neighbours():
    ci = 1
    _, y = CO.stack_inputs(ci)
    c = CO.CASES[ci]
    s = Stack(ci, 3)
    t0 = 0
    for i, n in enumerate((16, 5, 16)):                       # slot 2 carries the loud stream
        s.push_ragged(y[:, :, t0:t0 + n], [n] * 3, ("before", i))
        t0 += n
    before = s.records().clone()
    assert bool((before[:, :, :, :, 2] == t0).all()) and float(s.slot_rings(2).abs().sum()) > 0
    x, tail = Guarded(3, 16, fill=1.0), Guarded(3, 2, 4, fill=1.0)      # the small carries of a pool (L = 8, C = 2): reset along
    one = (ctypes.c_int * 1)(2)
    call("ctn_stream_reset_slots", s.state.ptr(), x.ptr(), 16, tail.ptr(), s.pos.data_ptr(), one, 1, 3, c.H, c.P, s.dil, s.nb, c.max_frames, 2, 8)
    call("ctn_stream_cum_reset_slots", s.cum.ptr(), one, 1, 3, s.nb)
    torch.cuda.synchronize()
    s.state.ok("reset"), s.cum.ok("reset")
    after = s.records()
    assert torch.equal(after[:, :2], before[:, :2]), "the neighbours' records changed"
    assert bool((after[:, 2] == 0).all()) and float(s.slot_rings(2).abs().sum()) == 0.0 and s.pos.tolist() == [t0, t0, 0]
    fresh, u0 = Stack(ci, 1), 0
    for i, n in enumerate((7, 16, 16, 1, 16)):                # slot 2 now gets stream 0 from its start; the others go on
        yin = torch.cat([y[:2, :, t0:t0 + n], y[:1, :, u0:u0 + n]])
        out = s.push_ragged(yin, [n] * 3, ("after", i))
        alone = fresh.push(y[:1, :, u0:u0 + n], ("fresh", i))
        assert torch.equal(out[2], alone[0]), ("call %d after the reset" % i)
        t0 += n
        u0 += n
    assert s.counts(0)[:, 0, 0].tolist() == [t0, t0, u0]


def test_argument_errors_launch_nothing():
    ci = 0
    _, y = CO.stack_inputs(ci)
    c = CO.CASES[ci]
    s = Stack(ci, 3)
    s.push(y[:, :, :16], ("first",))
    state0, cum0 = s.state.t.clone(), s.cum.t.clone()
    lib, err, st = ctn.lib.load(), ctn.lib.ctn_last_error, ops._stream()
    g = s.buffer(y[:, :, :17].contiguous())
    y0 = g.t.clone()
    big = ctn.lib.ctn_stream_state_bytes(3, c.H, c.P, s.dil, s.nb, 32)
    assert big > s.state_bytes
    wide = Guarded(big // 4, fill=0.0)
    assert lib.ctn_stream_tcn_cumln(s.packed.data_ptr(), s.dil, s.nb, g.ptr(), wide.ptr(), s.cum.ptr(), 3, c.B, c.H, c.P, 17, 32, st) == -1
    assert b"at most 16 frames" in err()
    assert lib.ctn_stream_tcn_cumln(*s.args(g), 0, 3, c.B, c.H, c.P, 16, 16, st) == -1 and b"cum" in err()
    assert lib.ctn_stream_tcn_cumln(*s.args(g), s.cum.ptr() + 8, 3, c.B, c.H, c.P, 16, 16, st) == -1 and b"aligned" in err()
    tab = table([16] * 3)
    assert lib.ctn_stream_tcn_cumln_ragged(*s.args(g), s.cum.ptr() + 4, tab.data_ptr(), s.pos.data_ptr(), 3, c.B, c.H, c.P, 16, 16, st) == -1
    torch.cuda.synchronize()
    assert torch.equal(g.t, y0) and torch.equal(s.state.t, state0) and torch.equal(s.cum.t, cum0) and float(wide.t.abs().sum()) == 0.0


@pytest.mark.parametrize("ci", CASES, ids=CO.CASE_IDS)
def test_the_per_frame_kernels_are_far_outside_the_limit(ci):
    """The test can fail: ctn_stream_tcn_cln on the same packed weights, against the cumulative reference."""
    _, y = CO.stack_inputs(ci)
    got = run_plan(Stack(ci, CO.M_TEST), y, CO.plans(ci)["cut0"], ("cln", ci), fn="ctn_stream_tcn_cln")
    e = CO.rel_err(got.cpu(), CO.stack_reference(ci))
    print("CUM defect: per-frame kernels on case %d  y=%.2e  limit %.0e" % (ci, e, LIM))
    assert e > 1000 * LIM


def test_zz_largest_figure():
    for kind, (e, where) in sorted(WORST.items()):
        print("CUM MAX %-12s %.2e  limit %.0e  at %s" % (kind, e, LIM, where))
    _RUNS.clear()
