"""Numpy restatement of the long-recording contract of include/ctn_hip.h ("long-recording separation"): segment counts,
framing, the overlap costs in their 1024-partial order, the chain of permutations, the cross-fade tables and the assembly.
Every float32 operation is written as one numpy float32 operation, so the results are what the device must give bit for bit."""
import itertools

import numpy as np

PART = 1024


def n_segments(T, seg, hop):
    assert T >= 1 and hop >= 1 and 1 <= seg - hop <= hop
    return 1 if T <= seg else 1 + (T - seg + hop - 1) // hop


def seg_ptr(lens, seg, hop):
    return np.concatenate(([0], np.cumsum([n_segments(int(T), seg, hop) for T in lens]))).astype(np.int64)


def frame(x, seg, hop):
    """x float32 [T] -> [n, seg]: segment i = x[i * hop : i * hop + seg], +0 at and beyond T."""
    x = np.asarray(x, dtype=np.float32)
    n = n_segments(len(x), seg, hop)
    out = np.zeros((n, seg), dtype=np.float32)
    for i in range(n):
        part = x[i * hop:i * hop + seg]
        out[i, :len(part)] = part
    return out


def cost_pair(prev, cur):
    """sum_t (prev[t] - cur[t])^2 over float32 [ov] rows: 1024 partial sums filled in ascending t from +0, then the halving tree."""
    prev, cur = np.asarray(prev, dtype=np.float32), np.asarray(cur, dtype=np.float32)
    d = prev - cur
    q = d * d
    assert d.dtype == np.float32 and q.dtype == np.float32
    acc = np.zeros(PART, dtype=np.float32)
    for t0 in range(0, len(q), PART):
        row = q[t0:t0 + PART]
        acc[:len(row)] = acc[:len(row)] + row
    s = PART // 2
    while s >= 1:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s //= 2
    return acc[0]


def costs(est, hop):
    """est float32 [n, C, seg] of ONE recording -> cost [n, C, C]; row 0 is zeros."""
    n, C, seg = est.shape
    out = np.zeros((n, C, C), dtype=np.float32)
    for i in range(1, n):
        for a in range(C):
            for b in range(C):
                out[i, a, b] = cost_pair(est[i - 1, a, hop:], est[i, b, :seg - hop])
    return out


def best_perm(c):
    """The first k (itertools order) that minimises sum_a c[a, perms[k][a]], the sum in float32 from +0, a ascending."""
    C = c.shape[0]
    perms = list(itertools.permutations(range(C)))
    best, bestv = 0, None
    for k, p in enumerate(perms):
        v = np.float32(0.0)
        for a in range(C):
            v = np.float32(v + c[a, p[a]])
        if k == 0 or v < bestv:
            best, bestv = k, v
    return best, perms[best]


def order(cost):
    """cost [n, C, C] of ONE recording -> g int32 [n, C]: g[0] = identity, g[i][a] = perms[q_i][g[i - 1][a]]."""
    n, C, _ = cost.shape
    g = np.zeros((n, C), dtype=np.int32)
    g[0] = np.arange(C)
    for i in range(1, n):
        _, p = best_perm(cost[i])
        g[i] = [p[g[i - 1, a]] for a in range(C)]
    return g


def fade_tables(ov, window="linear"):
    u = (np.arange(ov, dtype=np.float64) + 0.5) / ov
    fi = {"linear": u, "hann": np.sin(np.pi * u / 2.0) ** 2}[window]
    return fi.astype(np.float32), (1.0 - fi).astype(np.float32)


def assemble(est, g, T, hop, fi, fo):
    """est [n, C, seg], g [n, C] of ONE recording of T samples -> out float32 [C, T]."""
    n, C, seg = est.shape
    ov = seg - hop
    assert n == n_segments(T, seg, hop) and len(fi) == len(fo) == ov and fi.dtype == fo.dtype == np.float32
    out = np.empty((C, T), dtype=np.float32)
    for a in range(C):
        for i in range(n):
            end = T if i == n - 1 else (i + 1) * hop
            m = end - i * hop
            out[a, i * hop:end] = est[i, g[i, a], :m]
            if i >= 1:
                k = min(ov, m)
                p1 = fo[:k] * est[i - 1, g[i - 1, a], hop:hop + k]
                p2 = fi[:k] * est[i, g[i, a], :k]
                assert p1.dtype == np.float32 and p2.dtype == np.float32
                out[a, i * hop:i * hop + k] = p1 + p2
    return out


def stitch(est, T, hop, window="linear"):
    """ONE recording: -> (out [C, T], g [n, C], cost [n, C, C])."""
    seg = est.shape[2]
    c = costs(est, hop)
    g = order(c)
    fi, fo = fade_tables(seg - hop, window)
    return assemble(est, g, T, hop, fi, fo), g, c


def permuted_segments(src, seg, hop, rng, noise=0.0):
    """Sources float32 [C, T] cut into segments, every segment's speakers in a drawn order (segment 0: identity).
    -> (est [n, C, seg], local [n, C]): est[i, local[i][a]] = segment i of source a (plus seeded noise)."""
    C, T = src.shape
    fr = np.stack([frame(src[a], seg, hop) for a in range(C)], axis=1)             # [n, C, seg]
    n = fr.shape[0]
    local = np.stack([np.arange(C) if i == 0 else rng.permutation(C) for i in range(n)]).astype(np.int32)
    est = np.empty_like(fr)
    for i in range(n):
        for a in range(C):
            est[i, local[i, a]] = fr[i, a]
    if noise:
        est = (est + noise * rng.standard_normal(est.shape)).astype(np.float32)
    return est, local
