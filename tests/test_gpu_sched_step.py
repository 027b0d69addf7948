"""GPU: the two-stream ordering of the training step as Python drives it (ops._wgrad_async / _wgrad_small, the composite stacks'
autograd nodes, the bucketed backward, FlatAdam) under injected delays.

One run is  zero_grad, forward, loss, backward, FlatAdam.step(max_grad_norm=5), zero_grad, forward, loss, backward,
join_side_stream  on a model of two blocks (four in the bucket cases).  tests/sched_harness.py wraps lib.call: run k puts a delay
of D = max(2 ms, 4 x the unperturbed run), at most 20 ms, on the `stream` argument of the k-th call of the FIRST step, ahead of it,
and for a composite call also ahead of every launch group inside it.  Compared bit for bit with the unperturbed run: both losses,
the flat gradient after each backward pass, the flat parameters after the step.  The second step is there for hazards across steps:
cached workspaces, a freed block handed out again (tensor lifetime rests on record_stream), zero_grad or the optimiser's step
against a late second stream.  Every device tensor that the Python side gets uninitialised (torch.empty, empty_like, empty_strided,
Tensor.new_empty: tests/test_host_cpu.py checks that the package uses no other way) is born poisoned (NaN bytes) during a run, and
the cached workspaces and the flat gradient are poisoned ahead of it.

The bucket cases install a stand-in for parallel.GradientBuckets (two blocks per backward call) whose bucket_ready halves every
sink in place on the stream it is called on -- what the all-reduce does to the slice: ordered after the slice is produced and
before anything consumes it.  cumLN runs per kernel, as in tests/test_gpu_ops_trace.py, and through its composite stack
(ops.TcnCumLn, which that trace predates); the wide gLN model runs under h3 both ways: per kernel, _wgrad_async also carries the
tracked maxima to the second stream.

The mutants show that the harness can see: ops._order is patched to skip the fork inside _wgrad_async for ONE weight gradient (a
block's dW1 under each of the three norms, the decoder's dV); with the main-stream producer of that gradient's dOut delayed, the
sweep must report a difference at exactly that call, and with the edge in place the same delay gives the reference bits.

SCHED lines of the first MI355X run (pytest -s; all 18 tests passed, the module took 12.4 s, the longest case 1.9 s):
    case              calls of a run / of the first step   launch groups inside its composites   unperturbed run   D
    gln_composite      49 / 25    28     2942 us   11767 us
    gln_perkernel      85 / 43     0     3572 us   14290 us
    cln_composite      49 / 25    40     3024 us   12095 us
    cln_perkernel     101 / 51     0     3222 us   12888 us
    cumln_perkernel   101 / 51     0     3962 us   15849 us
    gln_wide_h3        57 / 29    30     2608 us   10433 us
    gln_buckets        51 / 26    54     4022 us   16088 us
    cln_buckets        51 / 26    78     3944 us   15778 us
    cumln_composite    49 / 25    40     2409 us    9635 us      (these two from the second run: 22 tests, 14.2 s)
    gln_wide_h3_perkernel  133 / 67     0     4063 us   16251 us
    mutants (gln_perkernel): block dW1 = call 34 (ctn_pw_wgrad), its dOut from call 32 (ctn_gln_prelu_bwd); decoder dV = call 18, its
    dOut from call 16 (ctn_unfold); D 10.8 to 11.7 ms; both reported at exactly that call, both controls kept the reference bits.
    mutants added later (84 tests, 19.3 s): block dW1 of cln_perkernel = call 42, its dOut from call 40 (ctn_cln_bwd), D 12997 us; of
    cumln_perkernel = call 42, its dOut from call 40 (ctn_cumln_bwd), D 13367 us; both reported at that call.
"""
import pytest
import torch

import conftest  # noqa: F401  puts the repository root on sys.path
import sched_harness as SH
from oracle import ctn_oracle as O

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import ops  # noqa: E402
from conv_tasnet_amd.optim import FlatAdam  # noqa: E402

DEV = "cuda:0"
NARROW = (32, 20, 16, 32, 3, 2, 1, 2)           # two blocks: the per-kernel path stays near a hundred calls per step
BUCKETS = (32, 20, 16, 32, 3, 2, 2, 2)          # four blocks: more than blocks_per_bucket
WIDE = (64, 20, 64, 128, 3, 2, 1, 2)            # >= 64 rows everywhere: the h3 entry points, their maxima and atomics
NORMS = {"gln": ("gLN", False), "cln": ("cLN", True), "cumln": ("cumLN", True)}
CASES = {
    "gln_composite": dict(norm="gln", composite=True), "gln_perkernel": dict(norm="gln", composite=False),
    "cln_composite": dict(norm="cln", composite=True), "cln_perkernel": dict(norm="cln", composite=False),
    "cumln_composite": dict(norm="cumln", composite=True), "cumln_perkernel": dict(norm="cumln", composite=False),
    "gln_wide_h3": dict(norm="gln", composite=True, dims=WIDE), "gln_wide_h3_perkernel": dict(norm="gln", composite=False, dims=WIDE),
    "gln_buckets": dict(norm="gln", composite=True, dims=BUCKETS, buckets=True),
    "cln_buckets": dict(norm="cln", composite=True, dims=BUCKETS, buckets=True),
}


class _Buckets:
    """Stand-in for parallel.GradientBuckets: two blocks per backward call; bucket_ready does to the bucket's slice what the
    all-reduce does -- it rewrites every sink in place, on the stream it is called on (the second stream when there is one)."""
    blocks_per_bucket = 2

    def __init__(self):
        self.works, self.covered, self.ready = [], [], 0

    def bucket_ready(self, sinks):
        self.ready += 1
        for s in sinks:
            s.mul_(0.5)


class _Step:
    """The model, the optimiser and the batch of a case; calling it is one run from the same parameters and optimiser state."""

    def __init__(self, case):
        norm_type, causal = NORMS[case["norm"]]
        torch.manual_seed(3)
        self.model = ctn.ConvTasNet(*case.get("dims", NARROW), norm_type=norm_type, causal=causal).to(DEV)
        self.opt = FlatAdam(self.model.parameters(), lr=1e-3)
        self.p0 = self.opt.flat_params.clone()
        self.mix, self.lens, self.src = (t.to(DEV) for t in O.synth_batch(5, 3, 2007))
        self.out = {}
        torch.cuda.synchronize()

    def _backprop(self):
        self.opt.zero_grad()
        loss = ctn.cal_loss(self.src, self.model(self.mix), self.lens)[0]
        loss.backward()
        return loss

    def __call__(self, end_of_first_step=lambda: None):
        opt, out = self.opt, self.out
        with SH.poisoned_allocations():
            opt.flat_params.copy_(self.p0)
            opt.exp_avg.zero_()
            opt.exp_avg_sq.zero_()
            opt._step = 0
            SH.poison(opt.flat_grads, *ops._ws_cache.values())
            loss = self._backprop()
            out["loss1"], out["grads1"] = loss.detach().clone(), opt.flat_grads.clone()       # (the last backward node joined the streams)
            opt.step(max_grad_norm=5.0)
            out["params"] = opt.flat_params.clone()
            end_of_first_step()
            loss = self._backprop()
            ops.join_side_stream()
            out["loss2"], out["grads2"] = loss.detach().clone(), opt.flat_grads.clone()

    def outputs(self):
        return self.out


@pytest.fixture
def case(request, monkeypatch):
    """-> (name, settings) with the case's switches set; all of them, and the cached workspaces, put back afterwards."""
    c = CASES[request.param]
    saved = ops.gemm_arith()
    try:
        ops.set_gemm_arith("h3")                                        # the library default, whatever ran before
        monkeypatch.setattr(ops, "_COMPOSITE", c["composite"])
        monkeypatch.setattr(ops, "_SIDE_ENABLED", True)
        ops.set_grad_buckets(_Buckets() if c.get("buckets") else None)
        yield request.param, c
    finally:
        ops.set_grad_buckets(None)
        ops.set_gemm_arith(saved)
        ops._ws_cache.clear()


def _side_ptr():
    return ops._side_stream(torch.device(DEV)).cuda_stream


def _assert_sane(ref):
    for k, t in ref.items():
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0, "%s of the unperturbed run: the poison reached it" % k
    assert not SH.same_bits(ref["grads1"], ref["grads2"])               # the optimiser's step moved the parameters


@pytest.mark.parametrize("case", sorted(CASES), indirect=True)
def test_reference_is_bitwise_the_single_stream_run(case, monkeypatch):
    """What every sweep below compares with: the unperturbed run on two streams has the bits of the run with the second stream off
    (the bucket cases too: without a second stream the stand-in's bucket_ready runs on the main stream)."""
    name, c = case
    step = _Step(c)
    step()
    torch.cuda.synchronize()
    two = SH.snapshot(step.outputs)
    _assert_sane(two)
    monkeypatch.setattr(ops, "_SIDE_ENABLED", False)
    step()
    torch.cuda.synchronize()
    assert not SH.differences(SH.snapshot(step.outputs), two)


@pytest.mark.parametrize("case", sorted(CASES), indirect=True)
def test_step_keeps_its_bits_with_any_call_delayed(case):
    name, c = case
    step = _Step(c)
    ref = SH.sweep_calls(step, step.outputs, tag=name, side_ptr=_side_ptr())
    _assert_sane(ref)
    if c.get("buckets"):
        assert ops._GRAD_BUCKETS.ready > 0 and ops._GRAD_BUCKETS.ready % 4 == 0        # two buckets per backward pass, two passes per run


# ---- the harness must be shown to see ------------------------------------------------------------------------------------
def _drop_fork(mp, sink):
    """ops._order skips the fork (current stream -> second stream) inside _wgrad_async for the weight gradient that lands in `sink`."""
    real_async, real_order, state = ops._wgrad_async, ops._order, {"skip": False, "dropped": 0}

    def wgrad_async(dOut, X, R, Cn, K, out, **kw):
        state["skip"] = out is not None and out.data_ptr() == sink.data_ptr()
        try:
            return real_async(dOut, X, R, Cn, K, out, **kw)
        finally:
            state["skip"] = False

    def order(src, dst):
        if state["skip"]:
            state["skip"] = False
            state["dropped"] += 1
            return
        real_order(src, dst)

    mp.setattr(ops, "_wgrad_async", wgrad_async)
    mp.setattr(ops, "_order", order)
    return state


def _producer_of_dout(calls, first, sink):
    """-> (index of the weight-gradient call of the first step that writes `sink`, index of the last call before it on the main
    stream that may write that call's dOut: the header declares the pointer it gets there as not const)."""
    writable, main = SH.writable_pointers(), torch.cuda.current_stream().cuda_stream

    def arg(rec, nm):
        return rec["args"][ctn.lib.protos[rec["name"]][2].index(nm)]

    w = [k for k in range(first) if calls[k]["name"].startswith("ctn_pw_wgrad") and arg(calls[k], "dW") == sink.data_ptr()]
    assert len(w) == 1, w
    dout = arg(calls[w[0]], "dOut")
    assert calls[w[0]]["stream"] == _side_ptr()
    ks = [k for k in range(w[0]) if calls[k]["stream"] == main and any(arg(calls[k], nm) == dout for nm in writable[calls[k]["name"]])]
    assert ks, "no producer found"
    return w[0], ks[-1]


W1, V = "separator.network.2.0.0.net.0.weight", "decoder.basis_signals.weight"
# (case, parameter): a block's dW1 under every norm -- its dOut comes from torch.empty (gLN) or torch.empty_like (cLN, cumLN) -- and
# the decoder's dV
MUTANTS = [("gln_perkernel", W1), ("cln_perkernel", W1), ("cumln_perkernel", W1), ("gln_perkernel", V)]


@pytest.mark.parametrize("case,which", MUTANTS, indirect=["case"],
                         ids=["%s-%s" % (c.split("_")[0], "block-dW1" if w == W1 else "decoder-dV") for c, w in MUTANTS])
def test_harness_sees_a_dropped_fork(case, which, monkeypatch):
    name, c = case
    step = _Step(c)
    sink = ops._sink(dict(step.model.named_parameters())[which])
    assert sink is not None
    calls, first = SH.record_calls(step)
    w, k = _producer_of_dout(calls, first, sink)
    what = "%s: dW in call %d (%s), its dOut from call %d (%s)" % (which, w, calls[w]["name"], k, calls[k]["name"])
    # the positive control: the edge in place, the producer delayed -> the reference bits
    ref = SH.sweep_calls(step, step.outputs, tag="%s control %s" % (name, what), only=[k], side_ptr=_side_ptr())
    _assert_sane(ref)
    with monkeypatch.context() as mp:
        state = _drop_fork(mp, sink)
        with pytest.raises(SH.ScheduleMismatch) as e:
            SH.sweep_calls(step, step.outputs, tag="%s mutant %s" % (name, what), only=[k], side_ptr=_side_ptr(), ref=ref)
        assert state["dropped"] > 0
    assert e.value.where == ("call", k), "the harness is blind: " + what
    assert "grads1" in str(e.value)
