"""GPU: FusedStreamPool (the ragged steps of csrc/ctn_stream.hip) -- streams that join, leave and deliver different amounts per push.
The yardstick in every case is the existing FusedStreamingSeparator(model, batch=1) fed that stream's samples alone in one push plus
flush(); every comparison is torch.equal."""
import pytest
import torch

from oracle import ctn_oracle as O

pytestmark = pytest.mark.gpu

import conv_tasnet_amd as ctn  # noqa: E402
from conv_tasnet_amd.streaming import FusedStreamingSeparator, FusedStreamPool  # noqa: E402

DEV = "cuda:0"
S = 10
_CACHE = {}


def _model(seed=2):
    if seed not in _CACHE:
        torch.manual_seed(seed)
        _CACHE[seed] = ctn.ConvTasNet(32, 20, 16, 32, 3, 4, 2, 2, norm_type="cLN", causal=True).to(DEV).eval()     # dilations 1 .. 8
    return _CACHE[seed]


def _alone(m, sig, F=64):
    """Stream `sig` [T] alone through the existing class: one push plus flush() -> [C, T]."""
    s = FusedStreamingSeparator(m, batch=1, max_chunk_frames=F)
    return torch.cat([s.push(sig[None].to(DEV)), s.flush()], dim=2)[0]


def _push(pool, sigs, done, hops):
    """One push: slot m delivers hops[m] hops of sigs[m] from hop done[m] on.  -> the valid part of every slot's output row."""
    M, n = len(hops), max(max(hops), 1)
    chunk = torch.zeros(M, n * S)
    for m, h in enumerate(hops):
        if h:
            chunk[m, :h * S] = sigs[m][done[m] * S:(done[m] + h) * S]
            done[m] += h
    out, lengths = pool.push(chunk.to(DEV), hops)
    assert out.shape == (M, pool.m.C, max(lengths)) and len(lengths) == M
    for m in range(M):
        assert not out[m, :, lengths[m]:].any()                     # zeros beyond each slot's length
    return [out[m, :, :lengths[m]] for m in range(M)], lengths


def test_ragged_pushes():
    """5 slots opened together, five lengths, five schedules: row-split steps (max <= 16 frames), stage steps (> 16), split pushes
    (> max_chunk_frames = 32), 1 hop beside 40, a first push of a single hop, idle pushes."""
    m = _model()
    sched = [[40, 3, 16, 0, 70, 1, 9],      # slot 0: 40 hops while slot 1 delivers 1; a split push (70 > 33)
             [1, 1, 16, 5, 20, 1, 0],       # slot 1: its first push is a single hop (primes the carry: no output)
             [7, 16, 2, 16, 33, 0, 25],      # slot 2: 25 hops in the last push: one unsplit stage step
             [17, 0, 11, 1, 34, 1, 3],
             [2, 12, 0, 0, 66, 1, 1]]
    total = [sum(s) for s in sched]
    mix, _, _ = O.synth_batch(3, 5, S * max(total))
    sigs = [mix[i, :S * total[i]] for i in range(5)]
    pool = FusedStreamPool(m, slots=5, max_chunk_frames=32)
    assert [pool.open() for _ in range(5)] == [0, 1, 2, 3, 4]
    got, done = [[] for _ in range(5)], [0] * 5
    for p in range(len(sched[0])):
        hops = [s[p] for s in sched]
        assert (max(hops) <= 16) == (p in (1, 2, 3, 5)) and (max(hops) > 33) == (p in (0, 4))      # the forms the plan is meant to take
        outs, lengths = _push(pool, sigs, done, hops)
        assert lengths == [(h - (p == 0 and h > 0)) * S for h in hops]
        for i in range(5):
            got[i].append(outs[i])
    for i in range(5):
        res = torch.cat(got[i] + [pool.close(i)], dim=1)
        assert torch.equal(res, _alone(m, sigs[i])), i


def test_join_and_leave():
    """Slot 0 runs throughout; slot 1 opens at the 8th push; slot 2 runs a signal scaled by 100, is closed after 5 pushes and reopened
    at the 10th with another signal: a reset that misses a ring, a carry or the position shows in the second occupant.  Slots 3 and 4
    are never opened."""
    m = _model()
    mix, _, _ = O.synth_batch(4, 4, S * 200)
    sigs = {0: mix[0], 1: mix[1], 2: mix[2] * 100.0}
    second = mix[3]
    pool = FusedStreamPool(m, slots=5, max_chunk_frames=16)
    assert pool.open() == 0 and pool.open(2) == 2
    got, done, results = {0: [], 1: [], 2: []}, [0] * 5, {}
    for p in range(14):
        if p == 7:
            assert pool.open() == 1                                 # the lowest free slot
        if p == 5:
            results["loud"] = (torch.cat(got[2] + [pool.close(2)], dim=1), sigs[2][:done[2] * S])
            got[2], done[2] = [], 0
        if p == 9:
            assert pool.open(2) == 2
            sigs[2] = second
        hops = [[13, 4, 16, 9][p % 4], 0, 0, 0, 0]
        if p >= 7:
            hops[1] = [5, 16, 1][p % 3]
        if p < 5 or p >= 9:
            hops[2] = [16, 3, 11][p % 3]
        outs, lengths = _push(pool, sigs, done, hops)
        assert lengths[3] == lengths[4] == 0
        for i in got:
            got[i].append(outs[i])
    for i in (0, 1, 2):
        results[i] = (torch.cat(got[i] + [pool.close(i)], dim=1), sigs[i][:done[i] * S])
    for key, (res, sig) in results.items():
        assert sig.shape[0] >= 40 * S and torch.equal(res, _alone(m, sig)), key
    assert not pool.is_open[3] and not pool.is_open[4]


def test_uniform_load_equals_the_existing_class():
    """All slots opened together, equal hops: output by output what FusedStreamingSeparator(batch=5) gives on the same plan."""
    m = _model()
    plan = (40, 7, 133, 2, 16, 64)
    mix, _, _ = O.synth_batch(3, 5, S * sum(plan))
    mix = mix.to(DEV)
    cls = FusedStreamingSeparator(m, batch=5, max_chunk_frames=64)
    pool = FusedStreamPool(m, slots=5, max_chunk_frames=64)
    for _ in range(5):
        pool.open()
    pos = 0
    for i, n in enumerate(plan):
        a = cls.push(mix[:, pos:pos + n * S])
        b, lengths = pool.push(mix[:, pos:pos + n * S], [n] * 5)
        assert lengths == [a.shape[2]] * 5 and torch.equal(a, b), i
        pos += n * S
    tail = cls.flush()
    for s in range(5):
        assert torch.equal(tail[s], pool.close(s))


def test_stage_form_at_16_frames_or_fewer():
    """130 slots: 256 / slots < 2, so steps of <= 16 frames run the stage kernels, most of whose workgroups belong to idle slots."""
    m = _model()
    mix, _, _ = O.synth_batch(5, 3, S * 60)
    where = {0: 0, 1: 77, 2: 129}
    sigs = {where[i]: mix[i] for i in range(3)}
    pool = FusedStreamPool(m, slots=130, max_chunk_frames=16)
    for s in where.values():
        pool.open(s)
    got, done = {s: [] for s in sigs}, [0] * 130
    for a, b, c in ((16, 1, 7), (3, 16, 0), (9, 2, 16), (1, 13, 4)):
        hops = [0] * 130
        hops[0], hops[77], hops[129] = a, b, c
        outs, _ = _push(pool, sigs, done, hops)
        for s in sigs:
            got[s].append(outs[s])
    for s in sigs:
        assert torch.equal(torch.cat(got[s] + [pool.close(s)], dim=1), _alone(m, sigs[s][:done[s] * S])), s


def test_graph_replay():
    """graph=True against the eager pool: the maximum frame count repeats (16 and 5) while the per-slot counts change between replays;
    slot 1 goes idle, slot 2 joins mid-flight.  Every output and every close() tail are equal."""
    m = _model(3)
    mix, _, _ = O.synth_batch(6, 3, S * 200)
    sigs = {i: mix[i] for i in range(3)}
    plan = [(16, 16, 0), (16, 9, 0), (16, 3, 0), (5, 5, 0), (16, 0, 0), (5, 0, 0), (9, 0, 16), (16, 0, 12), (2, 5, 5), (16, 1, 1),
            (5, 2, 0), (3, 16, 16)]
    pools = [FusedStreamPool(m, slots=3, max_chunk_frames=16, graph=g) for g in (False, True)]
    done = [[0] * 3, [0] * 3]
    for pool in pools:
        pool.open(0)
        pool.open(1)
    for p, hops in enumerate(plan):
        if p == 6:
            for pool in pools:
                pool.open(2)
        a, la = _push(pools[0], sigs, done[0], list(hops))
        b, lb = _push(pools[1], sigs, done[1], list(hops))
        assert la == lb
        for i in range(3):
            assert torch.equal(a[i], b[i]), (p, i)
    assert sorted(pools[1]._graphs) == [5, 15, 16] and not pools[0]._graphs     # 15: the first push of slots 0 and 1, again when slot 2 joins
    for i in range(3):
        assert torch.equal(pools[0].close(i), pools[1].close(i))


def test_paper_widths_deep_dilations():
    """N=256, B=256, H=512, X=8, R=4, 2 slots, 8-hop pushes with max_chunk_frames = 16.  Slot 1 joins after slot 0 has run 303 frames:
    more than the 256-frame history of dilation 128, so slot 0's rings have wrapped.  60 pushes in all."""
    torch.manual_seed(5)
    m = ctn.ConvTasNet(256, 20, 256, 512, 3, 8, 4, 2, norm_type="cLN", causal=True).to(DEV).eval()
    mix, _, _ = O.synth_batch(11, 2, S * 480)
    sigs = {0: mix[0], 1: mix[1][:S * 8 * 22]}
    pool = FusedStreamPool(m, slots=2, max_chunk_frames=16)
    pool.open(0)
    got, done = {0: [], 1: []}, [0, 0]
    for p in range(60):
        if p == 38:
            assert done[0] - 1 == 303
            pool.open(1)
        outs, _ = _push(pool, sigs, done, [8, 8 if p >= 38 else 0])
        for i in got:
            got[i].append(outs[i])
    assert done == [480, 176]
    for i in (0, 1):
        assert torch.equal(torch.cat(got[i] + [pool.close(i)], dim=1), _alone(m, sigs[i], 16)), i


def test_errors():
    m = _model()
    pool = FusedStreamPool(m, slots=2, max_chunk_frames=16)
    chunk = torch.zeros(2, 4 * S, device=DEV)
    with pytest.raises(ValueError):
        pool.push(chunk, [1, 0])                    # slot 0 is not open
    assert pool.open() == 0
    with pytest.raises(ValueError):
        pool.open(0)                                # already open
    with pytest.raises(ValueError):
        pool.push(chunk, [1])                       # hops of the wrong length
    with pytest.raises(ValueError):
        pool.push(chunk, [5, 0])                    # the row holds 4 hops
    with pytest.raises(ValueError):
        pool.push(chunk, [1, 1])                    # slot 1 is closed
    assert pool.open() == 1
    with pytest.raises(ValueError):
        pool.open()                                 # no free slot
    pool.close(1)
    with pytest.raises(ValueError):
        pool.close(1)
    with pytest.raises(ValueError):
        pool.push(chunk, [1, 1])                    # pushing to a closed slot
    out, lengths = pool.push(chunk, [0, 0])         # nothing to do: empty output
    assert out.shape == (2, 2, 0) and lengths == [0, 0]
    out, lengths = pool.push(chunk, [4, 0])         # none of the refused calls touched the slot: still its first push
    assert lengths == [3 * S, 0]
    with pytest.raises(ValueError):
        FusedStreamPool(ctn.ConvTasNet(32, 20, 16, 32, 3, 2, 1, 2).to(DEV))
