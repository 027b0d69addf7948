"""GPU: FusedStreamingSeparator (csrc/ctn_stream.hip) -- the reference's recorded output, bitwise chunk / batch invariance, the fp64
oracle as yardstick against the full forward and against the eager StreamingSeparator, reset / graph replay / refresh.
(Kernel by kernel, at the seams of the tiling and against an fp64 oracle of each entry point: tests/test_gpu_stream_seams.py.)"""
import pytest
import torch

from conftest import DEFAULT_ARITH, load_golden, set_arith
from oracle import ctn_oracle as O

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd.streaming import FusedStreamingSeparator, StreamingSeparator  # noqa: E402

DEV = "cuda:0"
S = 10


def _model(seed=2):
    torch.manual_seed(seed)
    return ctn.ConvTasNet(32, 20, 16, 32, 3, 4, 2, 2, norm_type="cLN", causal=True).to(DEV).eval()     # dilations 1 .. 8


def _run(sep, mix, plan, hop=S):
    outs, pos = [], 0
    for n in plan:
        outs.append(sep.push(mix[:, pos:pos + n * hop]))
        pos += n * hop
    assert pos == mix.shape[1]
    outs.append(sep.flush())
    return outs


def _oracle64(m, cfg, mix):
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    with torch.no_grad():
        return O.forward(cfg, sd, mix.double())


def test_reference_fixture_in_split_chunks():
    """The reference's own causal cLN output (model_tiny_cln_causal, recorded from src/conv_tasnet.py), 3000 samples in chunks of
    17, 100, 3, 180 hops with max_chunk_frames = 64 (100 and 180 are split inside push): the limit of the existing streaming test."""
    gd = load_golden("model_tiny_cln_causal")
    N, L, B, H, P, X, R, C = [int(v) for v in gd["cfg"]]
    mg = ctn.ConvTasNet(N, L, B, H, P, X, R, C, norm_type="cLN", causal=True, mask_nonlinear=str(gd["mask_nonlinear"]))
    mg.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in gd.items() if k.startswith("p:")})
    mg = mg.to(DEV).eval()
    mixg, refg = torch.from_numpy(gd["mixture"])[:, :3000], torch.from_numpy(gd["est_source_raw"])[..., :3000]
    sg = FusedStreamingSeparator(mg, batch=2, max_chunk_frames=64)
    gotg = torch.cat(_run(sg, mixg, (17, 100, 3, 180), L // 2), dim=2).cpu()
    assert gotg.shape == refg.shape
    err, lim = float((gotg - refg).abs().max()), 2e-5 * float(refg.abs().max())
    print("fixture: max|got - ref| = %.3e (limit %.3e)" % (err, lim))
    assert err <= lim
    with pytest.raises(ValueError):
        FusedStreamingSeparator(ctn.ConvTasNet(32, 20, 16, 32, 3, 2, 1, 2).to(DEV))


def _ones_and_twos(total):
    plan, i = [2], 0
    while sum(plan) < total:
        plan.append(min(1 + (i % 3 != 0), total - sum(plan)))       # 1, 2, 2, 1, 2, 2, ...
        i += 1
    return plan


def test_chunk_invariance_is_bitwise():
    """Frame-local fixed-order arithmetic: how the signal is cut into pushes cannot change a single bit (flush included)."""
    m = _model()
    mix, _, _ = O.synth_batch(3, 2, S * 537)
    plans = [(40, 7, 133, 2, 64, 291), _ones_and_twos(537), (537,)]
    assert all(sum(p) == 537 for p in plans) and set(plans[1]) == {1, 2}
    got = [torch.cat(_run(FusedStreamingSeparator(m, batch=2), mix, p), dim=2) for p in plans]
    assert got[0].shape == (2, 2, S * 537)
    assert torch.equal(got[0], got[1])
    assert torch.equal(got[0], got[2])


def test_batch_invariance_is_bitwise():
    """Stream 0 alone == row 0 of a batch of five different streams."""
    m = _model()
    mix, _, _ = O.synth_batch(3, 5, S * 537)
    plan = (40, 7, 133, 2, 64, 291)
    alone = torch.cat(_run(FusedStreamingSeparator(m, batch=1), mix[:1], plan), dim=2)
    five = torch.cat(_run(FusedStreamingSeparator(m, batch=5), mix, plan), dim=2)
    assert torch.equal(alone[0], five[0])
    assert not torch.equal(five[0], five[1])


def test_against_the_full_forward_with_the_fp64_oracle_as_yardstick():
    """e_new (fused separator vs O.forward in float64) <= 2 * e_full (model(full) under the fp32 arithmetic vs the same)."""
    m = _model()
    mix, _, _ = O.synth_batch(3, 2, S * 537)
    cfg = O.Config(32, 20, 16, 32, 3, 4, 2, 2, norm_type="cLN", causal=True)
    ref = _oracle64(m, cfg, mix)
    set_arith("fp32")
    try:
        with torch.no_grad():
            full = m(mix.to(DEV)).cpu().double()
    finally:
        set_arith(DEFAULT_ARITH)
    got = torch.cat(_run(FusedStreamingSeparator(m, batch=2), mix, (40, 7, 133, 2, 64, 291)), dim=2).cpu().double()
    assert got.shape == full.shape == ref.shape
    e_full, e_new = float((full - ref).abs().max()), float((got - ref).abs().max())
    print("vs fp64 oracle: e_full = %.3e  e_new = %.3e  (max|ref| = %.3e)" % (e_full, e_new, float(ref.abs().max())))
    assert e_new <= 2 * e_full


def test_paper_widths_deep_dilations_against_the_eager_separator():
    """N=256, B=256, H=512, X=8, R=4 (dilation 128; the rings wrap several times with max_chunk_frames = 16), one stream of 8000
    samples in chunks of 8 hops.  Yardstick: O.forward in float64.  e_new <= 2 * e_old, e_old = the existing eager
    StreamingSeparator under the fp32 arithmetic on the same input: both are fp32 accumulations of the same lengths in different
    orders."""
    torch.manual_seed(5)
    m = ctn.ConvTasNet(256, 20, 256, 512, 3, 8, 4, 2, norm_type="cLN", causal=True).to(DEV).eval()
    cfg = O.Config(256, 20, 256, 512, 3, 8, 4, 2, norm_type="cLN", causal=True)
    mix, _, _ = O.synth_batch(11, 1, 8000)
    ref = _oracle64(m, cfg, mix)
    plan = [8] * 100
    new = torch.cat(_run(FusedStreamingSeparator(m, batch=1, max_chunk_frames=16), mix, plan), dim=2).cpu().double()
    set_arith("fp32")
    try:
        old = torch.cat(_run(StreamingSeparator(m, batch=1), mix, plan), dim=2).cpu().double()
    finally:
        set_arith(DEFAULT_ARITH)
    assert new.shape == old.shape == ref.shape
    e_old, e_new = float((old - ref).abs().max()), float((new - ref).abs().max())
    print("paper widths vs fp64 oracle: e_old = %.3e  e_new = %.3e  (max|ref| = %.3e)" % (e_old, e_new, float(ref.abs().max())))
    assert e_new <= 2 * e_old


def test_reset_and_graph_replay_are_bitwise():
    """After reset() the same plan reproduces the first run; graph=True replays the step of a length from its second steady-state
    occurrence on and every output equals the eager fused separator's, over two chunk lengths and across a reset()."""
    m = _model(3)
    plan = [40, 40, 40, 40, 7, 40, 40, 7, 7, 7, 40]
    mix, _, _ = O.synth_batch(6, 2, S * sum(plan))
    eager, graphed = FusedStreamingSeparator(m, batch=2), FusedStreamingSeparator(m, batch=2, graph=True)
    runs = []
    for rnd in range(2):
        a, b = _run(eager, mix, plan), _run(graphed, mix, plan)
        for i, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(u, v), (rnd, i)
        assert sorted(graphed._graphs) == ([7, 40] if rnd == 0 else [7, 39, 40])      # 39: the first chunk's second occurrence
        runs.append(torch.cat(a, dim=2))
        eager.reset()
        graphed.reset()                                        # the captured graphs stay valid: the state buffers are the same
    assert torch.equal(runs[0], runs[1])


def test_refresh_repacks_changed_weights():
    m = _model(4)
    mix, _, _ = O.synth_batch(8, 2, S * 90)
    plan = (30, 5, 55)
    s = FusedStreamingSeparator(m, batch=2)
    before = torch.cat(_run(s, mix, plan), dim=2)
    with torch.no_grad():
        m.separator.network[2][1][2].net[3].pointwise().weight.mul_(1.5)       # one block's w2, in place
    s.reset()
    stale = torch.cat(_run(s, mix, plan), dim=2)
    assert torch.equal(stale, before)                           # packed weights are a snapshot ...
    s.reset()
    s.refresh()                                                 # ... until refresh()
    after = torch.cat(_run(s, mix, plan), dim=2)
    fresh = torch.cat(_run(FusedStreamingSeparator(m, batch=2), mix, plan), dim=2)
    assert torch.equal(after, fresh)
    assert not torch.equal(after, before)
