"""Every kernel of the fused streaming separator (csrc/ctn_stream.hip) through the C ABI against tests/stream_oracle.py in fp64, at
the seams of its tiling, on guarded buffers.

What runs (stream_oracle.STACK_CASES / FRONT_CASES / BACK_CASES; test_stream_oracle_cpu.py checks that they are what they claim):
    stack   ctn_stream_pack + ctn_stream_tcn_cln on (B, H, P) = (16,16,3) (48,80,3) (112,240,2) (496,32,8) (16,528,3) (512,240,1): k-group
            counts 1, 2, 3, 5, 7, 15, 31, 32, 33 (every batch size of gemm_rows, mixed inside one chain), 1 / 2 / 4 / 9 depthwise
            elements per thread (NI = 1, 4, 16, each with clamped last elements), the run-time tap count at P = 1, 2, 8, a dilation
            of one tile exactly and one beyond max_frames, rings with no slack in three cases, a row split with 5 empty slices.  Each case
            pushes a plan of calls of 1, 15, 16, 17 (where max_frames allows; else 16 + 1), max_frames, 2 and 7 frames until every
            ring has wrapped three times; y is compared with the oracle after every call.
    bits    the same signal in another cut; stream 0 of M = 2 against M = 1; the row-split form (M = 1: up to 16 workgroups per
            stream; M = 100: two) against the stage form (M = 129: one workgroup per tile -- the only place where the two-row-tile
            GEMM with a lone last tile and at a mixed batch decomposition runs in the stack); a ring position that starts at
            2^32 - 21 and wraps inside the third call against one that starts at 0 (ragged entry point).
    front   ctn_stream_pack_gemm + ctn_stream_front at (N, L, B) = (16,4,16) (48,16,48) (112,20,16) (528,40,16), 1 / 16 / 17 / 33 frames,
            with 1e30 in the sample buffer beyond the last frame's reach (the packed U has zero columns beyond L; the kernel may not
            read beyond frames + 1 hops).
    back    ctn_stream_back at (N, L, B, C, mask) = (16,4,16,8,softmax) (48,20,48,1,relu) (176,20,16,3,softmax) (112,16,112,2,relu) over four
            calls of 17, 1, 16, 33 frames: decoder frames and samples against the oracle; the overlap-add carry, the carried hop of x
            and out = first half + carried half bitwise from the frames buffer; softmax with scores of +-80 and a column of equal scores.
    ragged  the three ragged compute entry points with six slots of nf = F, 0, 1, 7, F + 5, -3 (rotated from step to step): every
            slot bitwise a plain M = 1 call of nf frames, columns nf .. F - 1 untouched, a slot with nf = 0 untouched altogether
            (y, position word, rings, overlap-add carry, carried hop).
Per call: outputs are pre-filled with NaN (the in / out y: then overwritten with the input; ragged buffers: with the sentinel,
so that untouched columns can be told) inside an allocation with 4096 sentinel elements on either side -- afterwards the sentinels are intact and nothing is NaN; the state (rings + scratch) lies
between sentinels too; after ctn_stream_reset the same plan gives the same bits.

Limits (stream_oracle.LIMIT, of max |ref| per stream): w 5e-7, front y 9e-7, stack y 9e-7, decoder frames 2e-6, samples 1e-6:
4x what an fp32 model in another summation order loses against fp64 on these inputs (test_stream_oracle_cpu.py), never what the
kernels give.

Largest figure per kind over all cases, first MI355X run (the `STREAM MAX` lines of -s).  A record, not new limits.
Run of 2026-10-19:
    kind       largest    limit   at
    w          2.15e-07   5e-7    front (528, 40, 16), 16 frames
    front y    7.67e-07   9e-7    front (528, 40, 16), 1 frame
    stack y    7.26e-07   9e-7    stack (512, 240, 1), dilations 1, 1   ((16, 528, 3): 7.13e-07; (16, 16, 3): 2.23e-07)
    frames     3.82e-07   2e-6    back (112, 16, 112, 2, relu), call 0
    samples    3.33e-07   1e-6    back (112, 16, 112, 2, relu), call 0
"""
import ctypes

import pytest
import torch

import stream_oracle as SO

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
F32, I32 = torch.float32, torch.int32
GUARD, SENT = 4096, -7777.0
HDR, TAB = 64, 8                # floats in front of the rings; ints per slot of a step table (CTN_STREAM_TAB)
WORST = {}
_RUNS = {}


@pytest.fixture(autouse=True)
def _own_lines():
    print()


def call(name, *args):
    ctn.lib.call(name, *args, ops._stream())


def dev(t):
    return t.to(F32).contiguous().to(DEV)


class Guarded:
    """A buffer pre-filled with `fill` between two runs of GUARD sentinel elements of the same allocation."""

    def __init__(self, *shape, fill=NAN):
        self.n = 1
        for s in shape:
            self.n *= s
        self.flat = torch.full((self.n + 2 * GUARD,), SENT, dtype=F32, device=DEV)
        self.t = self.flat[GUARD:GUARD + self.n].view(shape)
        self.t.fill_(fill)

    def ptr(self):
        return self.t.data_ptr()

    def ok(self, where):
        assert bool((self.flat[:GUARD] == SENT).all()) and bool((self.flat[GUARD + self.n:] == SENT).all()), (where, "a guard element was written")
        assert not bool(torch.isnan(self.t).any()), (where, "NaN left")
        return self.t


def note(kind, e, where):
    if e > WORST.get(kind, (-1.0,))[0]:
        WORST[kind] = (e, SO.LIMIT[kind], where)


def packed_gemm(W):
    """ctn_stream_pack_gemm of W [R, Cn] -> the packed buffer (kept alive by the caller)."""
    R, Cn = W.shape
    out = torch.empty(ctn.lib.load().ctn_stream_pack_gemm_bytes(R, Cn), dtype=torch.uint8, device=DEV)
    Wd = dev(W)
    call("ctn_stream_pack_gemm", Wd.data_ptr(), R, Cn, out.data_ptr())
    torch.cuda.synchronize()
    return out


def table(counts):
    t = torch.zeros((len(counts), TAB), dtype=I32)
    t[:, 0] = torch.tensor(counts, dtype=I32)
    t[:, 1] = t[:, 0]
    return t.to(DEV)


# ---- the stack -----------------------------------------------------------------------------------------------------------------------
class Stack:
    """Packed weights and a guarded, zeroed state of STACK_CASES[ci] for M streams."""

    def __init__(self, ci, M):
        c, (p, _) = SO.STACK_CASES[ci], SO.stack_inputs(ci)
        lib = ctn.lib.load()
        self.c, self.M, self.nb = c, M, len(c.dil)
        self.dil = (ctypes.c_int * self.nb)(*c.dil)
        self.state_bytes = lib.ctn_stream_state_bytes(M, c.H, c.P, self.dil, self.nb, c.max_frames)
        self.rings = [SO.ring_len(c.P, d, c.max_frames) for d in c.dil]
        assert self.state_bytes == 4 * (HDR + M * c.H * (sum(self.rings) + 16))
        self.state = Guarded(self.state_bytes // 4, fill=0.0)
        self.packed = torch.empty(lib.ctn_stream_pack_bytes(c.B, c.H, c.P, self.nb), dtype=torch.uint8, device=DEV)
        self.params = [dev(getattr(b, k)) for b in p.blocks for k in SO.BLOCK_ORDER]
        call("ctn_stream_pack", ops._ptr_table(self.params), self.nb, c.B, c.H, c.P, self.packed.data_ptr())
        self.pos = torch.zeros(M, dtype=I32, device=DEV)            # the ragged entry point's position words

    def reset(self):
        call("ctn_stream_reset", self.state.ptr(), self.state_bytes)
        self.pos.zero_()

    def position(self):
        return int(self.state.t[:1].view(I32).item()) & 0xFFFFFFFF

    def buffer(self, y, counts=None):
        """y [M, B, f] (CPU) in a guarded in / out buffer; ragged: F columns per slot, sentinel from the slot's count on."""
        g = Guarded(*y.shape)
        g.t.copy_(y)
        if counts is not None:
            for m, n in enumerate(counts):
                g.t[m, :, n:] = SENT
        return g

    def push(self, y, where):
        """One plain call on y [M, B, f] -> the result (device)."""
        c, f = self.c, y.shape[2]
        g = self.buffer(y)
        call("ctn_stream_tcn_cln", self.packed.data_ptr(), self.dil, self.nb, g.ptr(), self.state.ptr(), self.M, c.B, c.H, c.P, f, c.max_frames)
        torch.cuda.synchronize()
        self.state.ok(where)
        return g.ok(where)

    def push_ragged(self, y, counts, where):
        """One ragged step: y [M, B, F], counts as given to the table (the kernels clamp them to 0 .. F) -> the whole buffer."""
        c, F = self.c, y.shape[2]
        eff = [min(max(n, 0), F) for n in counts]
        g, tab = self.buffer(y, eff), table(counts)
        call("ctn_stream_tcn_cln_ragged", self.packed.data_ptr(), self.dil, self.nb, g.ptr(), self.state.ptr(), tab.data_ptr(), self.pos.data_ptr(),
             self.M, c.B, c.H, c.P, F, c.max_frames)
        torch.cuda.synchronize()
        self.state.ok(where)
        return g.ok(where)

    def slot_rings(self, m):
        """The ring rows of slot m, every block, as one tensor."""
        c, out, off = self.c, [], HDR
        for R in self.rings:
            out.append(self.state.t[off + m * c.H * R:off + (m + 1) * c.H * R])
            off += self.M * c.H * R
        return torch.cat(out)


def run_plan(s, y, plan, where):
    """The calls of `plan` on the signal y [M, B, T] -> [result per call] (device)."""
    outs, t0 = [], 0
    for i, n in enumerate(plan):
        outs.append(s.push(y[:, :, t0:t0 + n], where + (i, n)))
        t0 += n
    return outs


def main_run(ci):
    """Plan 0 of a case at M = 2, shared by the tests of this module: -> (Stack, y after every call, concatenated)."""
    if ci not in _RUNS:
        _, y = SO.stack_inputs(ci)
        s = Stack(ci, SO.M_TEST)
        _RUNS[ci] = (s, torch.cat(run_plan(s, y, SO.stack_plan(s.c), ("stack", ci)), 2))
    return _RUNS[ci]


CASES = range(len(SO.STACK_CASES))
CASE_IDS = ["B%d-H%d-P%d" % c[:3] for c in SO.STACK_CASES]


@pytest.mark.parametrize("ci", CASES, ids=CASE_IDS)
def test_stack_against_oracle(ci):
    c, (_, y), ref = SO.STACK_CASES[ci], SO.stack_inputs(ci), SO.stack_reference(ci)
    s, got = main_run(ci)
    plan, t0, errs = SO.stack_plan(c), 0, []
    assert s.position() == sum(plan)
    for n in plan:
        errs.append(SO.rel_err(got[:, :, t0:t0 + n].cpu(), ref[:, :, t0:t0 + n]))
        t0 += n
    note("stack_y", max(errs), "stack %s" % (tuple(c[:5]),))
    print("STREAM stack %-32s calls %2d frames %3d  y=%.2e" % (tuple(c[:5]), len(plan), t0, max(errs)))
    for i, e in enumerate(errs):
        assert e < SO.LIMIT["stack_y"], (ci, "call %d of %d frames" % (i, plan[i]), e)
    s.reset()
    assert s.position() == 0 and float(s.state.t.abs().sum()) == 0.0
    again = torch.cat(run_plan(s, y, plan, ("stack again", ci)), 2)
    assert torch.equal(got, again), (ci, "after ctn_stream_reset the plan gives other bits")


@pytest.mark.parametrize("ci", CASES, ids=CASE_IDS)
def test_stack_bits_do_not_depend_on_the_cut_or_the_other_streams(ci):
    c, (_, y) = SO.STACK_CASES[ci], SO.stack_inputs(ci)
    _, got = main_run(ci)
    other = torch.cat(run_plan(Stack(ci, SO.M_TEST), y, SO.stack_plan(c, 1), ("cut 1", ci)), 2)
    assert torch.equal(got, other), (ci, "another cut of the same signal")
    solo = torch.cat(run_plan(Stack(ci, 1), y[:1], SO.stack_plan(c), ("M = 1", ci)), 2)
    assert torch.equal(got[:1], solo), (ci, "stream 0 of M = 2 against M = 1")


FORM_PLAN = (16, 16, 7, 16, 1, 9)


@pytest.mark.parametrize("ci", CASES, ids=CASE_IDS)
def test_stack_bits_do_not_depend_on_the_kernel_form(ci):
    """The same frames (calls of at most one tile) through the row-split pair at the largest split (M = 1) and at two workgroups per
    stream (M = 100), and through the stage kernel (M = 129: no room for two workgroups per stream), every stream fed stream 0."""
    c, (_, y) = SO.STACK_CASES[ci], SO.stack_inputs(ci)
    T = sum(FORM_PLAN)
    _, got = main_run(ci)
    base = torch.cat(run_plan(Stack(ci, 1), y[:1, :, :T], FORM_PLAN, ("rows M = 1", ci)), 2)
    assert torch.equal(base, got[:1, :, :T]), (ci, "another cut")
    for M, form in ((100, "rows, two workgroups per stream"), (129, "stage")):
        outs = torch.cat(run_plan(Stack(ci, M), y[:1, :, :T].expand(M, -1, -1), FORM_PLAN, (form, ci)), 2)
        for m in (0, M // 2, M - 1):
            assert torch.equal(outs[m], base[0]), (ci, form, "stream %d" % m)


@pytest.mark.parametrize("ci", CASES, ids=CASE_IDS)
def test_position_word_wraps_at_2_to_the_32(ci):
    """Ragged entry point (the caller owns the position words): slot 0 starts at 2^32 - 21 on a zeroed state and wraps inside the third
    call, slot 1 starts at 0; both are fed stream 0 and must give its bits."""
    c, (_, y) = SO.STACK_CASES[ci], SO.stack_inputs(ci)
    _, got = main_run(ci)
    s = Stack(ci, 2)
    s.pos.copy_(torch.tensor([-21, 0], dtype=I32))                # 2^32 - 21 as a 32-bit word
    plan, t0 = SO.stack_plan(c), 0
    assert plan[0] + plan[1] < 21 < plan[0] + plan[1] + plan[2]
    for i, n in enumerate(plan):
        out = s.push_ragged(y[:1, :, t0:t0 + n].expand(2, -1, -1), [n, n], ("wrap", ci, i))
        for m in (0, 1):
            assert torch.equal(out[m], got[0, :, t0:t0 + n]), (ci, "call %d" % i, "slot %d" % m)
        t0 += n
    assert [int(v) & 0xFFFFFFFF for v in s.pos.tolist()] == [(2 ** 32 - 21 + t0) % 2 ** 32, t0]
    assert s.position() == 0                                       # the state's own position word is not used by the ragged calls


@pytest.mark.parametrize("ci", SO.RAGGED_STACK, ids=[CASE_IDS[i] for i in SO.RAGGED_STACK])
def test_ragged_stack_slots_are_plain_calls(ci):
    """Six slots, counts F, 0, 1, 7, F + 5, -3 rotated by one slot per step; F = max_frames and 16 in turn (case 0: the ragged stage
    kernel and the ragged row-split pair).  Each slot has a twin with M = 1 that gets a plain call of the slot's frames."""
    c, (_, y) = SO.STACK_CASES[ci], SO.stack_inputs(ci)
    M = 6
    s, twins, cur = Stack(ci, M), [Stack(ci, 1) for _ in range(M)], [0] * M
    for step, F in enumerate((c.max_frames, 16, c.max_frames, 16, 7, c.max_frames)):
        raw = SO.ragged_counts(F)
        raw = raw[step % M:] + raw[:step % M]
        eff = [min(max(n, 0), F) for n in raw]
        yin = torch.stack([y[m % 2, :, cur[m]:cur[m] + F] for m in range(M)])
        pos0, rings0 = s.pos.clone(), [s.slot_rings(m).clone() for m in range(M)]
        out = s.push_ragged(yin, raw, ("ragged", ci, step))
        for m, n in enumerate(eff):
            where = (ci, "step %d" % step, "slot %d" % m, "nf %d of %d" % (n, F))
            assert bool((out[m, :, n:] == SENT).all()), (where, "columns from nf on were written")
            assert int(s.pos[m]) == int(pos0[m]) + n, where
            if n == 0:
                assert torch.equal(s.slot_rings(m), rings0[m]), (where, "rings of an idle slot changed")
            else:
                alone = twins[m].push(yin[m:m + 1, :, :n], where)
                assert torch.equal(out[m, :, :n], alone[0]), (where, "differs from the plain M = 1 call")
            cur[m] += n
    assert min(cur) >= 24


# ---- the front end ---------------------------------------------------------------------------------------------------------------------
class Ends:
    """Packed front- and back-end weights."""

    def __init__(self, p):
        self.p = p
        if hasattr(p, "U"):
            self.Up, self.Wbp, self.g0, self.b0 = packed_gemm(p.U), packed_gemm(p.Wb), dev(p.g0), dev(p.b0)
            self.N, self.B = p.U.shape[0], p.Wb.shape[0]
        if hasattr(p, "Wm"):
            self.Wmp, self.Vp = packed_gemm(p.Wm), packed_gemm(p.V)
            self.B, self.N = p.Wm.shape[1], p.V.shape[1]

    def front(self, x, F, M, where, counts=None):
        """x: Guarded [M, xld] -> (w [M, N, F], y [M, B, F]) Guarded."""
        sent = counts is not None
        w, y = Guarded(M, self.N, F, fill=SENT if sent else NAN), Guarded(M, self.B, F, fill=SENT if sent else NAN)
        a = (x.ptr(), x.t.shape[1], self.Up.data_ptr(), self.g0.data_ptr(), self.b0.data_ptr(), self.Wbp.data_ptr(), w.ptr(), y.ptr())
        if sent:
            tab = table(counts)
            call("ctn_stream_front_ragged", *a, tab.data_ptr(), M, self.N, self.p.L, self.B, F)
        else:
            call("ctn_stream_front", *a, M, self.N, self.p.L, self.B, F)
        torch.cuda.synchronize()
        x.ok(where), w.ok(where), y.ok(where)
        return w, y

    def back(self, y, w, tail, x, F, M, C, softmax, where, counts=None):
        """y [M, B, F], w [M, N, F] device tensors; tail, x Guarded (carried) -> (frames [M, C, L, F], out [M, C, F * S]) Guarded."""
        L = self.p.L
        sent = counts is not None
        fr, out = Guarded(M, C, L, F, fill=SENT if sent else NAN), Guarded(M, C, F * (L // 2), fill=SENT if sent else NAN)
        a = (y.data_ptr(), w.data_ptr(), self.Wmp.data_ptr(), self.Vp.data_ptr(), fr.ptr(), out.ptr(), tail.ptr(), x.ptr(), x.t.shape[1])
        if sent:
            tab = table(counts)
            call("ctn_stream_back_ragged", *a, tab.data_ptr(), M, self.N, L, self.B, C, F, int(softmax))
        else:
            call("ctn_stream_back", *a, M, self.N, L, self.B, C, F, int(softmax))
        torch.cuda.synchronize()
        for g in (fr, out, tail, x):
            g.ok(where)
        return fr, out


def sample_buffer(sig, F, S, xld):
    """Guarded [M, xld]: the F + 1 hops that F frames reach, 1e30 beyond."""
    x = Guarded(sig.shape[0], xld, fill=1e30)
    x.t[:, :(F + 1) * S] = sig[:, :(F + 1) * S]
    return x


@pytest.mark.parametrize("case", SO.FRONT_CASES, ids=["N%d-L%d-B%d" % c for c in SO.FRONT_CASES])
def test_front_against_oracle(case):
    N, L, B = case
    (p, sig), (rw, ry) = SO.front_inputs(*case), SO.front_reference(*case)
    S, M = L // 2, sig.shape[0]
    e, xld = Ends(p), (max(SO.FRONT_FRAMES) + 1) * S + 16
    kept = {}
    for F in SO.FRONT_FRAMES:
        where = ("front", case, F)
        w, y = e.front(sample_buffer(sig, F, S, xld), F, M, where)
        ew, ey = SO.rel_err(w.t.cpu(), rw[:, :, :F]), SO.rel_err(y.t.cpu(), ry[:, :, :F])
        note("w", ew, "front %s frames %d" % (case, F))
        note("front_y", ey, "front %s frames %d" % (case, F))
        print("STREAM front N=%-3d L=%-2d B=%-2d frames %2d  w=%.2e y=%.2e" % (N, L, B, F, ew, ey))
        assert ew < SO.LIMIT["w"] and ey < SO.LIMIT["front_y"], (where, ew, ey)
        w2, y2 = e.front(sample_buffer(sig, F, S, xld), F, M, where)
        assert torch.equal(w.t, w2.t) and torch.equal(y.t, y2.t), (where, "second call differs")
        w1, y1 = e.front(sample_buffer(sig[1:], F, S, xld), F, 1, where)
        assert torch.equal(w.t[1:], w1.t) and torch.equal(y.t[1:], y1.t), (where, "stream 1 of M = 2 against M = 1")
        kept[F] = (w.t, y.t)
    for F, G in ((1, 33), (16, 17), (17, 33)):                      # a frame's values do not depend on the call it came in
        assert torch.equal(kept[F][0], kept[G][0][:, :, :F]) and torch.equal(kept[F][1], kept[G][1][:, :, :F]), (case, F, G)


# ---- the back end ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SO.BACK_CASES, ids=["N%d-L%d-B%d-C%d-%s" % (c[:4] + ("softmax" if c[4] else "relu",)) for c in SO.BACK_CASES])
def test_back_against_oracle(case):
    N, L, B, C, soft = case
    (p, y, w, hops), ref = SO.back_inputs(*case), SO.back_reference(case)
    S, M = L // 2, y.shape[0]
    e, xld = Ends(p), (max(SO.BACK_FRAMES) + 1) * S + 16
    tail, x = Guarded(M, C, S, fill=0.0), Guarded(M, xld, fill=SENT)
    x.t[:, :S] = hops[:, :S]
    yd, wd, t0 = dev(y), dev(w), 0
    for i, F in enumerate(SO.BACK_FRAMES):
        where = ("back", case, "call %d" % i, F)
        x.t[:, S:(F + 1) * S] = hops[:, (t0 + 1) * S:(t0 + F + 1) * S]
        x0, tail0 = x.t.clone(), tail.t.clone()
        fr, out = e.back(yd[:, :, t0:t0 + F].contiguous(), wd[:, :, t0:t0 + F].contiguous(), tail, x, F, M, C, soft, where)
        ef, eo = SO.rel_err(fr.t.cpu(), ref[i][0]), SO.rel_err(out.t.cpu(), ref[i][1])
        note("frames", ef, "back %s call %d" % (case, i))
        note("samples", eo, "back %s call %d" % (case, i))
        print("STREAM back N=%-3d L=%-2d B=%-3d C=%d %-7s frames %2d  frames=%.2e samples=%.2e" % (N, L, B, C, "softmax" if soft else "relu", F, ef, eo))
        assert ef < SO.LIMIT["frames"] and eo < SO.LIMIT["samples"], (where, ef, eo)
        # pure copies and one two-term sum: bitwise from the frames buffer
        prev = torch.cat([tail0.unsqueeze(3), fr.t[:, :, S:, :F - 1]], 3)
        assert torch.equal(out.t, (fr.t[:, :, :S, :] + prev).permute(0, 1, 3, 2).reshape(M, C, F * S)), (where, "overlap-add")
        assert torch.equal(tail.t, fr.t[:, :, S:, F - 1]), (where, "the carry is not the second half of the last frame")
        assert torch.equal(x.t[:, :S], x0[:, F * S:(F + 1) * S]) and torch.equal(x.t[:, S:], x0[:, S:]), (where, "the carried hop")
        t0 += F


# ---- the ragged front and back ends ---------------------------------------------------------------------------------------------------
def test_ragged_front_and_back_slots_are_plain_calls():
    N, L, B, C, soft = SO.RAGGED_ENDS
    pf, sig = SO.front_inputs(N, L, B)
    pb = SO.back_inputs(N, L, B, C, soft)[0]
    S, M, Fmax = L // 2, 6, 17
    ef, eb = Ends(pf), Ends(pb)
    xld = (Fmax + 1) * S + 16
    g = torch.Generator().manual_seed(5)
    sigs = torch.randn(M, 64 * S, generator=g)
    x, tail = Guarded(M, xld, fill=SENT), Guarded(M, C, S, fill=0.0)
    x.t[:, :S] = sigs[:, :S]
    xs = [Guarded(1, xld, fill=SENT) for _ in range(M)]
    tails = [Guarded(1, C, S, fill=0.0) for _ in range(M)]
    for m in range(M):
        xs[m].t[:, :S] = sigs[m:m + 1, :S]
    cur = [0] * M
    for step, F in enumerate((Fmax, 16, Fmax, 7, 16, Fmax)):          # six steps: every slot gets every count once
        raw = SO.ragged_counts(F)
        raw = raw[step % M:] + raw[:step % M]
        eff = [min(max(n, 0), F) for n in raw]
        for m, n in enumerate(eff):
            x.t[m, S:(n + 1) * S] = sigs[m, (cur[m] + 1) * S:(cur[m] + n + 1) * S]
            xs[m].t[0, S:(n + 1) * S] = sigs[m, (cur[m] + 1) * S:(cur[m] + n + 1) * S]
        x0, tail0 = x.t.clone(), tail.t.clone()
        w, y = ef.front(x, F, M, ("ragged front", step), counts=raw)
        fr, out = eb.back(y.t, w.t, tail, x, F, M, C, soft, ("ragged back", step), counts=raw)
        for m, n in enumerate(eff):
            where = ("step %d" % step, "slot %d" % m, "nf %d of %d" % (n, F))
            for name, t in (("w", w.t), ("y", y.t), ("frames", fr.t)):
                assert bool((t[m, ..., n:] == SENT).all()), (where, name, "columns from nf on were written")
            assert bool((out.t[m, :, n * S:] == SENT).all()), (where, "samples from nf hops on were written")
            assert torch.equal(x.t[m, S:], x0[m, S:]), (where, "the sample buffer beyond the carried hop changed")
            if n == 0:
                assert torch.equal(tail.t[m], tail0[m]) and torch.equal(x.t[m, :S], x0[m, :S]), (where, "the carries of an idle slot changed")
                continue
            w1, y1 = ef.front(xs[m], n, 1, where)
            fr1, out1 = eb.back(y1.t, w1.t, tails[m], xs[m], n, 1, C, soft, where)
            assert torch.equal(w.t[m, :, :n], w1.t[0]) and torch.equal(y.t[m, :, :n], y1.t[0]), (where, "front differs from the plain M = 1 call")
            assert torch.equal(fr.t[m, :, :, :n], fr1.t[0]) and torch.equal(out.t[m, :, :n * S], out1.t[0]), (where, "back differs from the plain call")
            assert torch.equal(tail.t[m], tails[m].t[0]) and torch.equal(x.t[m, :S], xs[m].t[0, :S]), (where, "carries differ from the plain call")
            cur[m] += n
    assert min(cur) >= 24 and max(cur) + 1 <= sigs.shape[1] // S


def test_zz_largest_figures():
    """Prints the largest figure per kind of output over the cases that ran before it (for the table in the docstring)."""
    for kind, (e, lim, where) in sorted(WORST.items()):
        print("STREAM MAX %-8s %.2e  limit %.0e  at %s" % (kind, e, lim, where))
    _RUNS.clear()
