"""GPU: the two-stream ordering of the composite stacks (ctn_tcn_{gln,cln,cumln}_{fwd,bwd}) under injected delays, through the C ABI.

tests/sched_harness.py: every launch group of a call is held back once, on its own stream, for D = max(2 ms, 4 x the unperturbed
call); every output must keep the bits of the unperturbed call, which in turn must have the bits of the same call with
side_stream = NULL.  Outputs, activation slots, gradient destinations and the workspace are filled with NaN bytes before every run.

Shape: M = 3 (uneven half-batch chains, 1 + 2 utterances, non-zero m0 offsets), B = H = 64 (the smallest widths that reach the piece
forms and h3), K = 130 (Kp = 192: the 62 pad frames must stay exactly 0), P = 3, three blocks with dilations 1, 2, 4 (a first, a
middle and a last block: the one-fork schedule issues dW2 of block i - 1 behind block i).  All three forward entry points take the
second stream (two half-batch chains), so none of the forward cases is dropped.

The mutants show that the harness can see: a backward call with flags = 1 leaves the second stream un-joined, so with the last
launch group of that stream delayed, a copy of the gradients taken on the main stream -- after that stream has idled for twice the
unperturbed call, so that only the delay can keep the second stream behind -- must hold the poison.  If it does not (the two
streams serialised by the runtime, a delay that does not delay), the sweeps above prove nothing and the mutant tests FAIL.

SCHED lines of the first MI355X run (pytest -s; launch groups per call, GPU time of the unperturbed call in us as h3 / b6 / fp32;
D was the 2000 us floor everywhere, 10 to 25 times the call; all 60 cases passed, the module took 6.7 s):
    gln_fwd save=1 / save=0        20 groups   112 / 78 / 82      98 / 78 / 78
    cln_fwd, cumln_fwd             32 groups   137 / 104 / 104    138 / 140 / 141
    gln_bwd gln_fuse=0  1 | 2 forks   23 / 23 / 21 groups   149 | 142   167 | 171   153 | 163
    gln_bwd gln_fuse=1  1 | 2 forks   20 / 20 / 18 groups   142 | 142   160 | 161   131 | 134
    cln_bwd cln_fuse=0  1 | 2 forks   32 / 32 / 30 groups   200 | 162   198 | 187   165 | 170
    cln_bwd cln_fuse=1  1 | 2 forks   29 / 29 / 27 groups   156 | 158   172 | 176   160 | 172
    cln_bwd cln_fuse=2  1 | 2 forks   29 / 29 / 27 groups   157 | 151   180 | 180   157 | 169
    cumln_bwd           1 | 2 forks   29 / 29 / 27 groups   201 | 211   207 | 218   179 | 209
    mutants: the delayed group was the last of the call with one fork (gLN: finalize of block 0, cLN: dW1 of block 0) and the one
    ahead of block 0's B5 with two; the copy held NaN in all 12 cases.
"""
import ctypes
import os

import pytest
import torch

import conftest  # noqa: F401  puts the repository root on sys.path
import sched_harness as SH

pytestmark = pytest.mark.gpu

from conv_tasnet_amd import ops  # noqa: E402
from conv_tasnet_amd._lib import lib  # noqa: E402

DEV = "cuda:0"
F32 = torch.float32
M, B, H, K, P = 3, 64, 64, 130, 3
DIL = [1, 2, 4]
NAMES = ("w1", "a1", "g1", "b1", "D", "a2", "g2", "b2", "w2")          # NPARAM order of include/ctn_hip.h
ACTS = {"gln": ops._gln_acts, "cln": ops._cln_acts, "cumln": ops._cumln_acts}


@pytest.fixture
def switches():
    """Every switch back to its default afterwards, and no cached workspace sized under another setting."""
    saved = (lib.ctn_cln_fuse(), lib.ctn_gln_fuse())
    env = os.environ.get("CTN_BWD_EVENTS", "")          # the library has no getter: its value at first use, as csrc/ctn_block.hip reads it
    try:
        yield
    finally:
        lib.call("ctn_tune", b"bwd_events", int(env[0]) if env[:1] in ("1", "2") else 0)
        lib.call("ctn_tune", b"cln_fuse", saved[0])
        lib.call("ctn_tune", b"gln_fuse", saved[1])
        ops._ws_cache.clear()


class _Stack:
    """Random parameters and inputs of a three-block stack (built as tests/test_gpu_cumln_stack.py builds them) and the buffers of
    its two C calls.  The forward buffers of a backward sweep are written once, by an unperturbed forward call, and then left alone."""

    def __init__(self, kind):
        self.kind, self.entry, self.nb = kind, "ctn_tcn_" + kind, len(DIL)
        self.causal = 0 if kind == "gln" else 1
        self.Kp = Kp = ops.padded_frames(K)
        g = torch.Generator().manual_seed(20 + len(kind))
        r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        params = []
        for _ in DIL:
            params += [r(H, B, 1) / B ** 0.5, torch.tensor([0.25]) + 0.05 * r(1), 1.0 + 0.3 * r(1, H, 1), 0.2 * r(1, H, 1), 0.6 * r(H, 1, P),
                       torch.tensor([0.25]) + 0.05 * r(1), 1.0 + 0.3 * r(1, H, 1), 0.2 * r(1, H, 1), r(B, H, 1) / H ** 0.5]
        self.params = [t.to(DEV).contiguous() for t in params]
        self.grads = [torch.empty_like(t) for t in self.params]
        x0, dout = r(M, B, Kp), r(M, B, Kp)
        x0[..., K:] = 0.0
        dout[..., K:] = 0.0
        self.x0, self.dout = x0.to(DEV), dout.to(DEV)
        self.ptab, self.gtab = ops._ptr_table(self.params), ops._ptr_table(self.grads)
        self.dil = (ctypes.c_int * self.nb)(*DIL)
        self.main = torch.cuda.current_stream().cuda_stream
        self.side = ops._side_stream(torch.device(DEV)).cuda_stream
        assert self.side and self.side != self.main

    def _empty(self, *shape, dtype=F32):
        return torch.empty(shape, dtype=dtype, device=DEV)

    def forward_buffers(self, save):
        nb, Kp = self.nb, self.Kp
        self.save = int(save)
        self.xs = self._empty(nb if save else 2, M, B, Kp)
        self.acts = ACTS[self.kind](nb if save else 1, M, H, Kp, torch.device(DEV))       # under the cln_fuse level of this moment
        self.amax = self._empty(nb, 2, M, ops.AMAX_SLOTS, dtype=torch.int32)
        self.fbytes = getattr(lib, self.entry + "_fwd_workspace")(M, B, H, Kp, nb)
        self.fws = self._empty(max(self.fbytes, 1), dtype=torch.uint8)
        return [self.xs, self.amax, self.fws] + list(self.acts)

    def forward(self, side):
        p = ops._p
        lib.call(self.entry + "_fwd", self.ptab, self.dil, self.nb, p(self.x0), p(self.xs), *[p(t) for t in self.acts], p(self.amax), self.save,
                 M, B, H, K, self.Kp, P, self.causal, p(self.fws), self.fbytes, self.main, side)

    def forward_outputs(self):
        out, seen = {"xs": self.xs}, set()
        for i, t in enumerate(self.acts):
            if t.data_ptr() not in seen:            # (the fused cLN chains hand h1s's pointer for the n1s that they never touch)
                seen.add(t.data_ptr())
                out["act%d" % i] = t
        if ops.gemm_arith() == "h3":                # the tracked maxima: which slot a workgroup merges into is not part of the result
            out["amax"] = self.amax.max(dim=-1).values
        return out

    def backward_buffers(self):
        nb, Kp = self.nb, self.Kp
        self.dxs, self.dh1s = self._empty(nb, M, B, Kp), self._empty(nb, M, H, Kp)
        self.bbytes = getattr(lib, self.entry + "_bwd_workspace")(M, B, H, Kp, P, nb)
        self.bws = self._empty(self.bbytes, dtype=torch.uint8)
        return [self.dxs, self.dh1s, self.bws] + self.grads

    def backward(self, side, flags=0):
        p = ops._p
        lib.call(self.entry + "_bwd", self.ptab, self.gtab, self.dil, self.nb, p(self.x0), p(self.xs), *[p(t) for t in self.acts], p(self.amax),
                 p(self.dout), p(self.dxs), p(self.dh1s), M, B, H, K, self.Kp, P, self.causal, p(self.bws), self.bbytes, self.main, side, flags)

    def gradients(self):
        return {"block%d.%s" % (i // 9, NAMES[i % 9]): t for i, t in enumerate(self.grads)}

    def backward_outputs(self):
        return dict(self.gradients(), dxs=self.dxs, dh1s=self.dh1s)


def _assert_pads_are_zero(tensors):
    for name, t in tensors.items():
        if t.dim() == 4 and t.shape[1:] in ((M, B, ops.padded_frames(K)), (M, H, ops.padded_frames(K))):      # activations and their gradients
            assert t.shape[-1] - K == 62 and float(t[..., K:].abs().max()) == 0.0, "%s: the pad frames do not hold exact zeros" % name


def _assert_finite(ref, names):
    for name in names:
        assert bool(torch.isfinite(ref[name]).all()), "%s of the unperturbed run is not finite: the poison reached it" % name


@pytest.mark.parametrize("kind,save", [("gln", 1), ("gln", 0), ("cln", 1), ("cumln", 1)], ids=["gln-save", "gln-pingpong", "cln", "cumln"])
def test_forward_keeps_its_bits_with_any_launch_group_delayed(gemm_arith, kind, save, switches):
    """The two half-batch chains.  save = 0: two ping-pong x slots and ONE slot of every activation, which both chains and all
    blocks share."""
    s = _Stack(kind)
    scratch = s.forward_buffers(save)
    SH.poison(*scratch)
    s.forward(0)
    torch.cuda.synchronize()
    single = SH.snapshot(s.forward_outputs)
    ref = SH.sweep_groups(lambda: s.forward(s.side), s.forward_outputs, scratch=lambda: scratch,
                          tag="%s_fwd save=%d %s" % (kind, save, gemm_arith))
    assert not SH.differences(ref, single), "two chains against one"
    _assert_finite(ref, ["xs"])
    _assert_pads_are_zero(ref)


BWD = ([("gln", b"gln_fuse", lv) for lv in (0, 1)] + [("cln", b"cln_fuse", lv) for lv in (0, 1, 2)] + [("cumln", None, 0)])


@pytest.mark.parametrize("events", [1, 2], ids=["one-fork", "two-forks"])
@pytest.mark.parametrize("kind,key,level", BWD, ids=["%s%s" % (k, "" if key is None else "-fuse%d" % lv) for k, key, lv in BWD])
def test_backward_keeps_its_bits_with_any_launch_group_delayed(gemm_arith, kind, key, level, events, switches):
    """flags = 0: both weight gradients, the finalize sums and the tap sums of every block on the second stream, behind one or two
    forks per block; the fusion level decides which buffers those kernels read."""
    if key is not None:
        lib.call("ctn_tune", key, level)
    lib.call("ctn_tune", b"bwd_events", events)
    s = _Stack(kind)
    SH.poison(*s.forward_buffers(1))
    s.forward(0)
    scratch = s.backward_buffers()
    SH.poison(*scratch)
    s.backward(0)
    torch.cuda.synchronize()
    single = SH.snapshot(s.backward_outputs)
    ref = SH.sweep_groups(lambda: s.backward(s.side), s.backward_outputs, scratch=lambda: scratch,
                          tag="%s_bwd %s=%d bwd_events=%d %s" % (kind, (key or b"-").decode(), level, events, gemm_arith))
    assert not SH.differences(ref, single), "two streams against one"
    _assert_finite(ref, list(ref))
    _assert_pads_are_zero(ref)
    assert all(float(t.abs().max()) > 0 for t in ref.values())


@pytest.mark.parametrize("events", [1, 2], ids=["one-fork", "two-forks"])
@pytest.mark.parametrize("kind", ["gln", "cln"])
def test_harness_sees_an_unjoined_second_stream(gemm_arith, kind, events, switches):
    """A wrong schedule by construction, with no switch of its own: flags = 1 returns with the second stream un-joined.  With that
    stream's last launch group delayed, the gradients copied on the main stream right after the call must hold the poison; after
    ctn_stream_order(side, main) they have the reference bits (the positive control: the same delay, the edge in place)."""
    lib.call("ctn_tune", b"bwd_events", events)
    s = _Stack(kind)
    SH.poison(*s.forward_buffers(1))
    s.forward(0)
    scratch = s.backward_buffers()

    def joined_by_hand():
        s.backward(s.side, flags=1)
        lib.call("ctn_stream_order", s.side, s.main)

    SH.poison(*scratch)
    n, fams = SH.count_groups(joined_by_hand)
    last = max(i for i, f in enumerate(fams) if f in SH.SIDE_FAMILIES)
    assert last >= n - 2                    # the second stream's last group: the last of the call, or the one ahead of block 0's B5
    SH.poison(*scratch)
    t0 = SH.timed(lambda: s.backward(s.side))
    ref = SH.snapshot(s.backward_outputs)
    D = SH.delay_for(t0)
    print("SCHED %s_bwd mutant bwd_events=%d %s groups=%d delayed=%d (%s) unperturbed=%.0fus D=%dus"
          % (kind, events, gemm_arith, n, last, SH.FAMILIES[fams[last]], t0, D))
    early = {}

    def unjoined_copy():
        s.backward(s.side, flags=1)
        # The main stream first idles for twice the unperturbed call: left alone, the second stream has finished by then, so the copy
        # holds poison only because of the delay (D >= 4 x that call) and not because the second stream happens to be the slower one
        lib.call("ctn_delay", s.main, int(2 * t0))
        early.update(SH.snapshot(s.gradients))              # on the main stream, which nothing has ordered behind the second one
        lib.call("ctn_stream_order", s.side, s.main)        # before anything else touches those buffers

    SH.poison(*scratch)
    SH.run_with_group_delay(unjoined_copy, last, D)
    assert any(bool(torch.isnan(t).any()) for t in early.values()), \
        "the harness is blind: a copy taken ahead of the delayed second stream holds no poison"
    assert SH.differences(early, {k: ref[k] for k in early})
    assert not SH.differences(SH.snapshot(s.backward_outputs), ref), "joined by hand, the same delay must give the reference bits"
