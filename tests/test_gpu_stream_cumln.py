"""GPU: the three fused streaming classes with cumulative=True on a causal cumLN model (the cumulative kernels of csrc/ctn_stream.hip).
The yardsticks: the model's full forward and StreamingSeparator (within 2e-6 of the largest magnitude, the bound of
test_gpu_cumln.py::test_streaming_equals_full_forward), and for everything about chunking, batching, graphs, pools and client rates
FusedStreamingSeparator(cumulative=True) itself on one stream alone, with torch.equal."""
import pytest
import torch

from oracle import ctn_oracle as O

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd import resample  # noqa: E402
from conv_tasnet_amd.streaming import (FusedStreamingSeparator, FusedStreamPool, ResamplingStreamPool,  # noqa: E402
                                       StreamingSeparator)

DEV = "cuda:0"
TINY = (32, 20, 16, 32, 3, 4, 2, 2)
S, L, C = 10, 20, 2
_CACHE = {}


@pytest.fixture(autouse=True)
def _own_lines():
    print()


def _model(seed):
    if seed not in _CACHE:
        torch.manual_seed(seed)
        _CACHE[seed] = ctn.ConvTasNet(*TINY, norm_type="cumLN", causal=True).to(DEV).eval()
    return _CACHE[seed]


def _pushes(s, mix, plan):
    outs, pos = [], 0
    for n in plan:
        outs.append(s.push(mix[:, pos:pos + n * S]))
        pos += n * S
    assert pos == mix.shape[1]
    return torch.cat(outs + [s.flush()], dim=2)


def _alone(m, sig):
    """Stream `sig` [T] alone through the class: one push plus flush() -> [C, T]."""
    s = FusedStreamingSeparator(m, batch=1, max_chunk_frames=16, cumulative=True)
    return torch.cat([s.push(sig[None].to(DEV)), s.flush()], dim=2)[0]


@pytest.mark.usefixtures("gemm_arith")
def test_fused_equals_full_forward():
    """Fails without the cumulative kernels (the constructor refuses the model; per-frame statistics are off by tens of percent)."""
    m = _model(2)
    T, plan = S * 537, (40, 7, 133, 2, 64, 291)
    mix, _, _ = O.synth_batch(3, 2, T)
    mix = mix.to(DEV)
    with torch.no_grad():
        full = m(mix)
    chain = float((_pushes(StreamingSeparator(m, batch=2), mix, plan) - full).abs().max()) / float(full.abs().max())
    s = FusedStreamingSeparator(m, batch=2, max_chunk_frames=16, cumulative=True)
    assert s.cumulative and s.F == 16
    for rnd in range(2):                                            # the second round after reset(): the carry records start again
        got = _pushes(s, mix, plan)
        assert got.shape == full.shape
        err = float((got - full).abs().max()) / float(full.abs().max())
        print("round %d: max |fused - full| / max |full| = %.3e (StreamingSeparator: %.3e; limit 2e-6)" % (rnd, err, chain))
        assert err <= 2e-6
        s.reset()


def test_bits_do_not_depend_on_chunking_batch_or_step_length():
    m = _model(2)
    mix, _, _ = O.synth_batch(3, 2, S * 537)
    mix = mix.to(DEV)

    def run(plan, batch=2, F=16, graph=False):
        s = FusedStreamingSeparator(m, batch=batch, max_chunk_frames=F, graph=graph, cumulative=True)
        assert s.F == 16
        return _pushes(s, mix[:batch], plan)

    small = [2] + [1, 2] * 178 + [1]                                 # the first push must hold a whole frame (L = 2 hops)
    assert sum(small) == 537
    base = run([537])
    assert torch.equal(base, run(small)), "1- and 2-hop pushes"
    assert torch.equal(base, run([16] * 33 + [9])), "16-hop pushes"
    assert torch.equal(base[:1], run([537], batch=1)), "batch 1 against stream 0 of batch 2"
    assert torch.equal(base, run([100, 437], F=64)), "max_chunk_frames = 64 is clamped to 16"


def test_graph_replay_equals_eager():
    """The plan of test_gpu_cumln.py::test_streaming_graph_replay_equals_eager_chunks; the records live on the device and the step's last
    launch commits them, so a replayed step is bitwise the eager one."""
    m = _model(3)
    plan = [40, 40, 40, 40, 7, 40, 40, 7, 7, 7, 40]
    mix, _, _ = O.synth_batch(6, 2, S * sum(plan))
    mix = mix.to(DEV)
    eager = FusedStreamingSeparator(m, batch=2, max_chunk_frames=16, cumulative=True)
    graphed = FusedStreamingSeparator(m, batch=2, max_chunk_frames=16, graph=True, cumulative=True)
    for rnd in range(2):
        pos = 0
        for n in plan:
            a, b = eager.push(mix[:, pos:pos + n * S]), graphed.push(mix[:, pos:pos + n * S])
            assert torch.equal(a, b), (rnd, pos)
            pos += n * S
        assert torch.equal(eager.flush(), graphed.flush())
        assert sorted(graphed._graphs) == [7, 8, 16] and not eager._graphs
        eager.reset()
        graphed.reset()


def _push(pool, sigs, done, hops):
    """One push: slot m delivers hops[m] hops of sigs[m] from hop done[m] on -> the valid part of every slot's output row."""
    M, n = len(hops), max(max(hops), 1)
    chunk = torch.zeros(M, n * S)
    for m, h in enumerate(hops):
        if h:
            chunk[m, :h * S] = sigs[m][done[m] * S:(done[m] + h) * S]
            done[m] += h
    out, lengths = pool.push(chunk.to(DEV), hops)
    for m in range(M):
        assert not out[m, :, lengths[m]:].any()
    return [out[m, :, :lengths[m]] for m in range(M)]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_pool_slots_are_streams_of_their_own(graph):
    """Slot 0 runs throughout with 0, 1 and 40 hops among its pushes; slot 1 opens at the 8th push; slot 2 runs a signal scaled by 100, is
    closed after 5 pushes and reopened at the 10th with another one: a reset that misses a record shows in the second occupant.  Slot 3
    is never opened."""
    m = _model(2)
    mix, _, _ = O.synth_batch(4, 4, S * 260)
    sigs = {0: mix[0], 1: mix[1], 2: mix[2] * 100.0}
    pool = FusedStreamPool(m, slots=4, graph=graph, cumulative=True)
    assert pool.cumulative and pool.F == 16
    assert pool.open() == 0 and pool.open(2) == 2
    got, done, results = {0: [], 1: [], 2: []}, [0] * 4, {}
    for p in range(14):
        if p == 7:
            assert pool.open() == 1
        if p == 5:
            results["loud"] = (torch.cat(got[2] + [pool.close(2)], dim=1), sigs[2][:done[2] * S])
            got[2], done[2] = [], 0
        if p == 9:
            assert pool.open(2) == 2
            sigs[2] = mix[3]
        hops = [[1, 40, 0, 16, 9][p % 5], 0, 0, 0]
        if p >= 7:
            hops[1] = [5, 40, 1][p % 3]
        if p < 5 or p >= 9:
            hops[2] = [16, 3, 40][p % 3]
        outs = _push(pool, sigs, done, hops)
        for i in got:
            got[i].append(outs[i])
    for i in (0, 1, 2):
        results[i] = (torch.cat(got[i] + [pool.close(i)], dim=1), sigs[i][:done[i] * S])
    for key, (res, sig) in results.items():
        assert sig.shape[0] >= 40 * S and torch.equal(res, _alone(m, sig)), key
    assert not pool.is_open[3] and bool(graph) == bool(pool._graphs)


def test_resampling_pool_is_bitwise_the_offline_pipeline():
    """One stream at 16 kHz in ragged pushes: resample -> FusedStreamingSeparator(cumulative=True) -> (no output stage), the contract of
    ResamplingStreamPool."""
    m = _model(2)
    cuts = [163, 0, 7, 2400, 480, 1, 1800, 333]
    mix, _, _ = O.synth_batch(8, 1, sum(cuts))
    x = mix[0]
    pool = ResamplingStreamPool(m, slots=2, input_rate=16000, cumulative=True)
    assert pool.pool.cumulative
    assert pool.open() == 0
    got, at = [], 0
    for n in cuts:
        chunk = torch.full((2, n + 5), float("nan"))
        chunk[0, :n] = x[at:at + n]
        at += n
        out, lengths = pool.push(chunk.to(DEV), [n, 0])
        got.append(out[0, :, :lengths[0]])
    got = torch.cat(got + [pool.close(0)], dim=1)
    x8 = resample.resample(x.to(DEV), 16000, 8000)
    n8 = x8.shape[0]
    padded = torch.zeros(max(L, -(-n8 // S) * S), device=DEV)
    padded[:n8] = x8
    want = _alone(m, padded)[:, :n8]
    assert got.shape == want.shape and torch.equal(got, want)


def test_paper_widths():
    """N = 512, L = 16, B = 128, H = 512, P = 3, X = 8, R = 1: the LDS of the cumulative kernels at paper widths (45440 of 65536
    bytes); the rings of the dilations up to 32 wrap within the 249 frames.  One speaker: the (unchanged) back-end kernel holds
    B + C * N + C * 16 rows of 64 bytes in LDS, which at N = 512 fits for C = 1 only."""
    torch.manual_seed(5)
    m = ctn.ConvTasNet(512, 16, 128, 512, 3, 8, 1, 1, norm_type="cumLN", causal=True).to(DEV).eval()
    hop = 8
    mix, _, _ = O.synth_batch(11, 1, 2000)
    mix = mix.to(DEV)
    fused, chain = FusedStreamingSeparator(m, batch=1, max_chunk_frames=16, cumulative=True), StreamingSeparator(m, batch=1)
    a, b = [], []
    for pos in range(0, 2000, 8 * hop):
        a.append(fused.push(mix[:, pos:pos + 8 * hop]))
        b.append(chain.push(mix[:, pos:pos + 8 * hop]))
    a, b = torch.cat(a + [fused.flush()], dim=2), torch.cat(b + [chain.flush()], dim=2)
    assert a.shape == b.shape == (1, 1, 2000)
    err = float((a - b).abs().max()) / float(b.abs().max())
    print("paper widths: max |fused - StreamingSeparator| / max = %.3e (limit 2e-6)" % err)
    assert err <= 2e-6
