"""GPU: the composite stack of cumLN TemporalBlocks (ctn_tcn_cumln_fwd / _bwd, ops.TcnCumLn) and the two norm passes that track
the h3 maximum of what they store (ctn_cumln_fwd_amax / ctn_cumln_bwd_amax).

Every comparison is torch.equal.  The per-block path (ops.CumLnBlock over ctn_cumln_fwd / ctn_cumln_bwd) is pinned against fp64 by
tests/test_gpu_cumln.py; the stack issues that path's calls from C++ and a maximum is exact, so bitwise equality with it is the whole
accuracy claim and no tolerance appears here."""
import ctypes

import pytest
import torch

import conftest  # noqa: F401  puts the repository root on sys.path
from oracle import ctn_oracle as O

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402
from conv_tasnet_amd._lib import CtnError, lib  # noqa: E402
from conv_tasnet_amd.optim import FlatAdam  # noqa: E402

DEV = "cuda:0"
F32 = torch.float32
P = 3
NARROW, WIDE = (16, 32), (64, 128)          # (B, H): below 64 rows the fp32 forms, from 64 rows the piece forms
CTN_ERR_ARG, CTN_ERR_WORKSPACE = -1, -3


@pytest.fixture
def arith(request):
    ops.set_gemm_arith(request.param)
    yield request.param
    ops.set_gemm_arith(conftest.DEFAULT_ARITH)
    ops._ws_cache.clear()


# ---------------------------------------------------------------------------------------
# the tracked entry points
# ---------------------------------------------------------------------------------------
def _dev(t, mis=False):
    """fp32 on the device; mis: the first element one float off a 16-byte boundary (the scalar / general kernels)."""
    if not mis:
        return t.to(DEV).contiguous()
    buf = torch.empty(t.numel() + 1, dtype=F32, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _slots_max(a):
    """[M, AMAX_SLOTS] bit patterns of non-negative floats -> the maximum per utterance (the slot a workgroup picks is not compared)."""
    return a.max(dim=1).values


@pytest.mark.parametrize("mis", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("prelu", [True, False], ids=["prelu", "plain"])
@pytest.mark.parametrize("padded", [False, True], ids=["K=Kp", "K<Kp"])
@pytest.mark.parametrize("M,Ch,K", [(3, 32, 13), (2, 128, 67), (2, 128, 200)])
def test_tracked_norm_passes_equal_the_untracked_ones_and_absmax_rows(M, Ch, K, padded, prelu, mis):
    """aligned with Kp % 16 == 0: the 16-byte kernels, which take the maximum in the apply pass; K = Kp (13, 67: no multiple of 16) and
    the misaligned inputs: the scalar / general kernels, which finish with a ctn_absmax_rows pass (the stored tensors stay aligned: that
    pass reads 16 bytes at a time)."""
    Kp = ops.padded_frames(K) if padded else K
    g = torch.Generator().manual_seed(100 * K + Ch + M)
    Y = _dev(torch.randn(M, Ch, Kp, generator=g) * 1.7 + 0.3, mis)
    gamma, beta = _dev(torch.randn(Ch, generator=g)), _dev(torch.randn(Ch, generator=g))
    al = torch.tensor([0.21], dtype=F32, device=DEV) if prelu else None
    dOut = torch.randn(M, Ch, Kp, generator=g)
    dOut[..., K:] = 1e30                                                # garbage in the pad frames: it must reach nothing
    dOut = _dev(dOut, mis)
    p, st = ops._p, ops._stream()

    def fwd(entry, *amax):
        out = torch.full((M, Ch, Kp), -7.0, dtype=F32, device=DEV)
        mean, rstd = torch.full((M, Kp), -7.0, dtype=F32, device=DEV), torch.full((M, Kp), -7.0, dtype=F32, device=DEV)
        work = torch.empty(lib.ctn_cumln_work_bytes(M, Kp), dtype=torch.uint8, device=DEV)
        lib.call(entry, p(Y), p(out), p(mean), p(rstd), M, Ch, K, Kp, p(gamma), p(beta), p(al), 0, 0, p(work), *amax, st)
        return out, mean, rstd

    def bwd(entry, mean, rstd, *amax):
        dY = torch.full((M, Ch, Kp), -7.0, dtype=F32, device=DEV)
        pc = torch.zeros(lib.ctn_cln_bwd_pc_floats(M, Ch, Kp), dtype=F32, device=DEV)
        dap = torch.zeros(lib.ctn_cln_bwd_blocks(M, Kp), dtype=F32, device=DEV) if prelu else None
        work = torch.empty(lib.ctn_cumln_work_bytes(M, Kp), dtype=torch.uint8, device=DEV)
        lib.call(entry, p(dOut), p(Y), p(dY), p(mean), p(rstd), M, Ch, K, Kp, p(gamma), p(al), p(dap), p(pc), p(work), *amax, st)
        return dY, pc, dap

    ref = fwd("ctn_cumln_fwd")
    amax = torch.zeros(M, ops.AMAX_SLOTS, dtype=torch.int32, device=DEV)
    got = fwd("ctn_cumln_fwd_amax", p(amax))
    null = fwd("ctn_cumln_fwd_amax", 0)
    for a, b, c in zip(ref, got, null):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert int(amax.min()) >= 0 and torch.equal(_slots_max(amax), _slots_max(ops.absmax_rows(got[0])))
    assert torch.equal(_slots_max(amax), got[0].abs().flatten(1).max(1).values.view(torch.int32))

    mean, rstd = ref[1], ref[2]
    ref = bwd("ctn_cumln_bwd", mean, rstd)
    amax = torch.zeros(M, ops.AMAX_SLOTS, dtype=torch.int32, device=DEV)
    got = bwd("ctn_cumln_bwd_amax", mean, rstd, p(amax))
    null = bwd("ctn_cumln_bwd_amax", mean, rstd, 0)
    for a, b, c in zip(ref, got, null):
        assert (a is None and b is None and c is None) or (torch.equal(a, b) and torch.equal(a, c))
    assert bool(torch.isfinite(got[0]).all()) and (Kp == K or float(got[0][..., K:].abs().max()) == 0.0)
    assert int(amax.min()) >= 0 and torch.equal(_slots_max(amax), _slots_max(ops.absmax_rows(got[0])))
    assert torch.equal(_slots_max(amax), got[0].abs().flatten(1).max(1).values.view(torch.int32))


def test_tracked_maximum_is_merged_into_what_the_slots_hold():
    """The passes merge (atomic max) like every other producer of a tracked maximum: a larger value already there stays."""
    M, Ch, K = 2, 128, 67
    Kp = ops.padded_frames(K)
    g = torch.Generator().manual_seed(5)
    Y, gamma, beta = _dev(torch.randn(M, Ch, Kp, generator=g)), _dev(torch.randn(Ch, generator=g)), _dev(torch.randn(Ch, generator=g))
    out, mean, rstd = torch.empty_like(Y), torch.empty(M, Kp, device=DEV), torch.empty(M, Kp, device=DEV)
    work = torch.empty(lib.ctn_cumln_work_bytes(M, Kp), dtype=torch.uint8, device=DEV)
    big = torch.tensor([1e9], dtype=F32).view(torch.int32).item()
    amax = torch.zeros(M, ops.AMAX_SLOTS, dtype=torch.int32, device=DEV)
    amax[0] = big
    p = ops._p
    lib.call("ctn_cumln_fwd_amax", p(Y), p(out), p(mean), p(rstd), M, Ch, K, Kp, p(gamma), p(beta), 0, 0, 0, p(work), p(amax), ops._stream())
    assert int(amax[0].min()) == big and torch.equal(_slots_max(amax[1:]), _slots_max(ops.absmax_rows(out[1:])))


# ---------------------------------------------------------------------------------------
# the stack against the chain of ops.CumLnBlock
# ---------------------------------------------------------------------------------------
def _stack_inputs(B, H, M, K, nb, seed=0, flat=True):
    """x0 [M,B,Kp] (a leaf), dout, 9 parameters per block in NPARAM order (with FlatAdam's gradient sinks when flat), the optimiser."""
    Kp = ops.padded_frames(K)
    g = torch.Generator().manual_seed(1000 * seed + 10 * K + M)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    params = []
    for _ in range(nb):
        params += [r(H, B, 1) / B ** 0.5, torch.tensor([0.25]) + 0.05 * r(1), 1.0 + 0.3 * r(1, H, 1), 0.2 * r(1, H, 1), 0.6 * r(H, 1, P),
                   torch.tensor([0.25]) + 0.05 * r(1), 1.0 + 0.3 * r(1, H, 1), 0.2 * r(1, H, 1), r(B, H, 1) / H ** 0.5]
    params = [torch.nn.Parameter(t.to(DEV)) for t in params]
    opt = FlatAdam(params, lr=1e-3, direct_grads=flat)
    x0, dout = r(M, B, Kp), r(M, B, Kp)
    x0[..., K:] = 0.0
    dout[..., K:] = 0.0
    return x0.to(DEV).requires_grad_(True), dout.to(DEV), params, opt


def _run(fn, x0, dout, opt):
    """-> (output, dx0, the flat gradient of all parameters) of out = fn(x0); out.backward(dout)."""
    opt.zero_grad()
    x0.grad = None
    out = fn(x0)
    out.backward(dout)
    ops.join_side_stream()
    torch.cuda.synchronize()
    return out.detach().clone(), x0.grad.detach().clone(), opt.flat_grads.clone()


def _chain(params, K, dil):
    def fn(x):
        for i, d in enumerate(dil):
            x = ops.CumLnBlock.apply(x, *params[9 * i:9 * i + 9], K, d, True)
        return x
    return fn


def _stack(params, K, dil):
    return lambda x: ops.TcnCumLn.apply(x, K, dil, True, *params)


def _assert_same(a, b, params, opt):
    assert torch.equal(a[0], b[0]), "stack output"
    assert torch.equal(a[1], b[1]), "dxs[0]"
    for i, (_, o, n) in enumerate(opt._segments()):
        assert torch.equal(a[2][o:o + n], b[2][o:o + n]), "gradient of parameter %d of block %d" % (i % 9, i // 9)
    assert len(opt._segments()) == len(params)


@pytest.mark.parametrize("side", [True, False], ids=["side", "noside"])
@pytest.mark.parametrize("K", [13, 67, 200])
@pytest.mark.parametrize("M", [1, 2, 3])
@pytest.mark.parametrize("width,arith", [(NARROW, "h3"), (WIDE, "h3"), (WIDE, "b6"), (WIDE, "fp32")], indirect=["arith"],
                         ids=["narrow", "wide-h3", "wide-b6", "wide-fp32"])
def test_stack_is_bitwise_the_chain_of_blocks(width, arith, M, K, side, monkeypatch):
    """M = 1: one chain; 2: an even split into two half-batch chains; 3: 1 + 2.  K = 13: less than one 16-frame tile; 67: one crossing of
    the scans' 64-frame block; 200: several and a ragged end.  side off: one stream for everything."""
    monkeypatch.setattr(ops, "_SIDE_ENABLED", side)
    monkeypatch.setattr(ops, "_COMPOSITE", True)
    B, H = width
    dil = [1, 2, 4]
    x0, dout, params, opt = _stack_inputs(B, H, M, K, len(dil))
    ref = _run(_chain(params, K, dil), x0, dout, opt)
    got = _run(_stack(params, K, dil), x0, dout, opt)
    _assert_same(got, ref, params, opt)
    with torch.no_grad():                           # save = 0: two ping-pong x slots, one slot of every activation
        assert torch.equal(ops.tcn_cumln_infer(x0.detach(), K, dil, True, params), ref[0])


@pytest.mark.parametrize("width", [NARROW, WIDE], ids=["narrow", "wide"])
def test_stack_with_plain_autograd_parameters(width):
    """No gradient sinks: the stack returns every gradient to autograd (one scratch buffer, no second stream in the backward pass)."""
    B, H = width
    dil, K, M = [1, 2, 4], 67, 3
    x0, dout, params, opt = _stack_inputs(B, H, M, K, len(dil), flat=False)
    assert all(ops._sink(p) is None for p in params)
    ref = _run(_chain(params, K, dil), x0, dout, opt)
    got = _run(_stack(params, K, dil), x0, dout, opt)
    _assert_same(got, ref, params, opt)


class _Buckets:
    """Stand-in for parallel.GradientBuckets, as in tests/test_gpu_ops_trace.py: two blocks per backward call, no collective."""
    blocks_per_bucket = 2

    def __init__(self):
        self.works, self.covered, self.ready = [], [], []

    def bucket_ready(self, sinks):
        self.ready.append(len(sinks))


@pytest.mark.parametrize("width", [NARROW, WIDE], ids=["narrow", "wide"])
def test_bucketed_backward_equals_one_call(width):
    """A 4-block stack as two backward calls of two blocks (the first leaves the weight-gradient stream un-joined and has a workspace
    of its own) against one call."""
    B, H = width
    dil, K, M = [1, 2, 4, 1], 67, 3
    x0, dout, params, opt = _stack_inputs(B, H, M, K, len(dil))
    one = _run(_stack(params, K, dil), x0, dout, opt)
    gb = _Buckets()
    ops.set_grad_buckets(gb)
    try:
        two = _run(_stack(params, K, dil), x0, dout, opt)
    finally:
        ops.set_grad_buckets(None)
        ops._ws_cache.clear()
    assert gb.ready == [18, 18]
    _assert_same(two, one, params, opt)
    _assert_same(one, _run(_chain(params, K, dil), x0, dout, opt), params, opt)


# ---------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flat", [True, False], ids=["sinks", "autograd"])
def test_model_step_is_bitwise_the_per_block_path(flat, monkeypatch):
    """One step (forward, cal_loss, backward, FlatAdam) of the causal cumLN model with ops._COMPOSITE on and off; under the composite
    the stack is ONE ctn_tcn_cumln_fwd and ONE ctn_tcn_cumln_bwd and Python makes no per-block cumLN call."""
    mix, lens, src = (t.to(DEV) for t in O.synth_batch(5, 3, 4007))
    res, names = [], {}
    for composite in (True, False):
        with monkeypatch.context() as mp:
            mp.setattr(ops, "_COMPOSITE", composite)
            torch.manual_seed(3)
            m = ctn.ConvTasNet(64, 20, 64, 128, 3, 3, 2, 2, norm_type="cumLN", causal=True).to(DEV)
            opt = FlatAdam(m.parameters(), lr=1e-3, direct_grads=flat)
            opt.zero_grad()
            call, made = lib.call, []
            mp.setattr(lib, "call", lambda name, *a: (made.append(name), call(name, *a))[1])
            est = m(mix)
            loss = ctn.cal_loss(src, est, lens)[0]
            loss.backward()
            ops.join_side_stream()
            torch.cuda.synchronize()
            names[composite] = made
            grads = [p.grad.detach().clone() for p in m.parameters()]
            opt.step(max_grad_norm=5.0)
            torch.cuda.synchronize()
            res.append((loss.detach().clone(), est.detach().clone(), grads, [p.detach().clone() for p in m.parameters()]))
    (l1, e1, g1, p1), (l2, e2, g2, p2) = res
    assert torch.equal(l1, l2) and torch.equal(e1, e2)
    assert len(g1) == len(g2) == len(p1) == len(p2) > 0
    for a, b in zip(g1 + p1, g2 + p2):
        assert torch.equal(a, b)
    assert names[True].count("ctn_tcn_cumln_fwd") == 1 and names[True].count("ctn_tcn_cumln_bwd") == 1
    assert not [n for n in names[True] if n.startswith("ctn_cumln_")]
    assert not [n for n in names[False] if n.startswith("ctn_tcn_")] and "ctn_cumln_fwd" in names[False]


# ---------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------
def test_non_causal_stack_is_refused_with_a_message():
    x0, dout, params, opt = _stack_inputs(16, 32, 2, 13, 1)
    with pytest.raises(CtnError, match="ctn_tcn_cumln_fwd.*causal must be 1"):
        ops.tcn_cumln_infer(x0.detach(), 13, [1], False, params)
    # the backward entry point refuses before it touches a pointer: one valid buffer stands in for all of them
    buf = torch.zeros(4096, dtype=F32, device=DEV)
    tab = (ctypes.c_void_p * 9)(*[buf.data_ptr()] * 9)
    b, M, Kp = buf.data_ptr(), 2, ops.padded_frames(13)
    nbytes = lib.ctn_tcn_cumln_bwd_workspace(M, 16, 32, Kp, P, 1)
    rc = lib.ctn_tcn_cumln_bwd(tab, tab, (ctypes.c_int * 1)(1), 1, b, b, b, b, b, b, b, b, b, b, b, M, 16, 32, 13, Kp, P, 0, b, nbytes, 0, 0, 0)
    assert rc == CTN_ERR_ARG and b"causal must be 1" in lib.ctn_last_error()


def test_workspace_one_byte_short_is_refused():
    buf = torch.zeros(4096, dtype=F32, device=DEV)
    tab = (ctypes.c_void_p * 9)(*[buf.data_ptr()] * 9)
    b, M, B, H, K = buf.data_ptr(), 2, 16, 32, 13
    Kp = ops.padded_frames(K)
    dil = (ctypes.c_int * 1)(1)
    need = lib.ctn_tcn_cumln_fwd_workspace(M, B, H, Kp, 1)
    rc = lib.ctn_tcn_cumln_fwd(tab, dil, 1, b, b, b, b, b, b, b, b, 1, M, B, H, K, Kp, P, 1, b, need - 1, 0, 0)
    assert rc == CTN_ERR_WORKSPACE and b"ctn_tcn_cumln_fwd: workspace too small" in lib.ctn_last_error()
    need = lib.ctn_tcn_cumln_bwd_workspace(M, B, H, Kp, P, 1)
    rc = lib.ctn_tcn_cumln_bwd(tab, tab, dil, 1, b, b, b, b, b, b, b, b, b, b, b, M, B, H, K, Kp, P, 1, b, need - 1, 0, 0, 0)
    assert rc == CTN_ERR_WORKSPACE and b"ctn_tcn_cumln_bwd: workspace too small" in lib.ctn_last_error()


def test_second_backward_is_refused():
    x0, dout, params, opt = _stack_inputs(16, 32, 2, 13, 2, flat=False)
    out = ops.TcnCumLn.apply(x0, 13, [1, 2], True, *params)
    out.backward(dout, retain_graph=True)
    with pytest.raises(CtnError, match="backward called twice"):
        out.backward(dout)
    torch.cuda.synchronize()
