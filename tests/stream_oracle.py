"""The contract of the fused streaming entry points (csrc/ctn_stream.hip; include/ctn_hip.h, "streaming": ctn_stream_front,
ctn_stream_tcn_cln, ctn_stream_back and their ragged forms) in plain torch on the CPU.

`Stream` is stateful across calls like the kernels, but keeps every history as an ordinary growing array: no rings, no tiles, no
fragment order.  dtype float64 is the reference; dtype float32 is the fp32 MODEL: the same mathematics in torch's own fp32
operators (dot products and channel sums as eight interleaved chains, roots and exponentials correctly rounded --
summation orders of its own, and nothing that depends on the host's vector libraries), a sample of what fp32 arithmetic reaches in
another legitimate order.  `wrong` names one deliberate defect (WRONG) that tests/test_stream_oracle_cpu.py uses to show that the
limits tell a defect from rounding.

The module also holds what tests/test_stream_oracle_cpu.py and tests/test_gpu_stream_seams.py share: the case lists, the inputs
(cached: computed once), the chunk plans and the limits.

Limits (LIMIT): per kind of output, relative to max |ref| per stream.  Each is 4x the largest figure of that kind that the fp32
model shows against the fp64 oracle over all cases of the GPU module, on exactly its inputs, rounded up to one significant digit
(FP32_FIGURE: the CPU figures, asserted by test_stream_oracle_cpu.py to stay inside LIMIT / 4).  The factor 4 is the headroom the
GEMM and norm seam modules use between fp32 arithmetic and their limits: room for another legitimate summation order and for
expf / division within a couple of ulp.  They are never derived from what the kernels give.
"""
import collections
import functools
import types

import torch

F64, F32 = torch.float64, torch.float32
EPS = 1e-8                      # CTN_EPS, inside the root
LANES = 8                       # partial sums per dot product of the fp32 model
A1, A2 = 0.1, 0.4               # PReLU slopes: distinguishable (the default 0.25 / 0.25 would hide a swap)
M_TEST = 2
QUIET = 4e-3                    # amplitude of the quiet stream of FRONT_QUIET: column variances of a few hundred eps

# kind -> largest fp32-model figure over all cases (test_stream_oracle_cpu.py::test_fp32_model_stays_four_times_inside prints them)
FP32_FIGURE = {"w": 1.11e-7, "front_y": 2.24e-7, "stack_y": 2.05e-7, "frames": 3.23e-7, "samples": 2.47e-7}
LIMIT = {"w": 5e-7, "front_y": 9e-7, "stack_y": 9e-7, "frames": 2e-6, "samples": 1e-6}

WRONG = ("unbiased_variance", "eps_outside_root", "prelu_after_norm", "taps_reversed", "dilation_plus_one", "future_tap",
         "alphas_swapped", "residual_dropped", "softmax_over_n", "ola_carry_dropped", "history_zeroed")

# ---- the cases ---------------------------------------------------------------------------------------------------------------------
StackCase = collections.namedtuple("StackCase", "B H P dil max_frames seams")
STACK_CASES = (
    StackCase(16, 16, 3, (1, 2), 17, ("one_tile", "G1", "NI1", "NI1_clamp", "tap_inside_tile")),
    StackCase(48, 80, 3, (1, 5, 16), 16, ("G3", "G5", "NI4", "NI4_two_per_thread", "NI4_clamp", "dilation_one_tile")),
    StackCase(112, 240, 2, (3, 40), 24, ("G7", "G15", "NI4", "NI4_four_per_thread", "P2", "dilation_beyond_max_frames")),
    StackCase(496, 32, 8, (1, 2), 18, ("G31", "P8", "P8_fourteen_back")),
    StackCase(16, 528, 3, (8, 8), 16, ("two_tile_odd", "G33", "NI16", "NI16_clamp", "ring_no_slack", "empty_slices")),
    StackCase(512, 240, 1, (1, 1), 16, ("two_tile_mixed", "G15", "P1")),
)
FRONT_CASES = ((16, 4, 16), (48, 16, 48), (112, 20, 16), (528, 40, 16))             # (N, L, B)
FRONT_FRAMES = (1, 16, 17, 33)
FRONT_QUIET = (48, 16, 48)
BACK_CASES = ((16, 4, 16, 8, True), (48, 20, 48, 1, False), (176, 20, 16, 3, True), (112, 16, 112, 2, False))    # (N, L, B, C, softmax)
BACK_FRAMES = (17, 1, 16, 33)           # one call each, in this order: the carries cross three call boundaries
RAGGED_STACK = (0, 1)                   # indices into STACK_CASES
RAGGED_ENDS = (112, 20, 16, 3, True)    # (N, L, B, C, softmax) of the ragged front + back chain


def ragged_counts(F):
    """nf of the six slots of a ragged step: F, 0, 1, 7, one above F (clamped to F) and one negative (clamped to 0)."""
    return [F, 0, 1, 7, F + 5, -3]


def stack_plan(c, cut=0):
    """Frames per call of one stack case.  cut 0: the chunks 1, 15, 16, 17, max_frames, 2, 16, 7 over and over (a chunk above
    max_frames is split as FusedStreamingSeparator.push splits it) until every ring has wrapped three times; cut 1: the same
    number of frames in another cut."""
    total = 3 * max(ring_len(c.P, d, c.max_frames) for d in c.dil) + 16
    if cut == 1:
        total = sum(stack_plan(c, 0))
    chunks = (1, 15, 16, 17, c.max_frames, 2, 16, 7) if cut == 0 else (3, c.max_frames, 16, 5, 1, 1, 14)
    calls, i = [], 0
    while sum(calls) < total:
        n = chunks[i % len(chunks)]
        i += 1
        while n > 0:
            calls.append(min(n, c.max_frames, total - sum(calls) if cut == 1 else n))
            n -= calls[-1]
            if sum(calls) == total:
                break
    return calls


def ring_len(P, d, max_frames):
    n, r = (P - 1) * d + max_frames, 1
    while r < n:
        r <<= 1
    return r


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=F64)


def make_block(g, B, H, P, d):
    """One TemporalBlock's nine parameters (fp32 values): gammas and betas drawn separately and away from 1 / 0, taps not symmetric
    in t, 1x1 weights scaled so that h and the residual branch are of order 1."""
    ramp = 0.2 * torch.arange(1, P + 1, dtype=F64)
    b = types.SimpleNamespace(
        W1=_randn(g, H, B) / B ** 0.5, a1=torch.tensor([A1], dtype=F64), g1=0.5 + 0.4 * _rand(g, H), b1=0.2 + 0.3 * _randn(g, H),
        D=0.5 * _randn(g, H, P) + ramp, a2=torch.tensor([A2], dtype=F64), g2=1.2 + 0.5 * _rand(g, H), b2=-0.2 + 0.3 * _randn(g, H),
        W2=0.5 * _randn(g, B, H) / H ** 0.5, d=int(d))
    for k, v in vars(b).items():
        if k != "d":
            setattr(b, k, v.to(F32))
    return b


BLOCK_ORDER = ("W1", "a1", "g1", "b1", "D", "a2", "g2", "b2", "W2")     # the order of ctn_stream_pack's pointer table


@functools.lru_cache(maxsize=None)
def stack_inputs(ci, M=M_TEST):
    """-> (params, y [M, B, T] fp32) of STACK_CASES[ci]; T = the frames of its plan."""
    c = STACK_CASES[ci]
    g = _gen(1, ci)
    p = types.SimpleNamespace(P=c.P, blocks=[make_block(g, c.B, c.H, c.P, d) for d in c.dil])
    return p, _randn(g, M, c.B, sum(stack_plan(c))).to(F32)


@functools.lru_cache(maxsize=None)
def front_inputs(N, L, B, M=M_TEST):
    """-> (params, samples [M, (33 + 1) * S] fp32).  Stream 1 of FRONT_QUIET is quiet: its column variances are a few hundred eps."""
    g = _gen(2, N, L, B)
    p = types.SimpleNamespace(L=L, U=(_randn(g, N, L) / L ** 0.5).to(F32), g0=(0.6 + 0.3 * _rand(g, N)).to(F32),
                              b0=(0.3 * _randn(g, N) - 0.1).to(F32), Wb=(_randn(g, B, N) / N ** 0.5).to(F32))
    x = _randn(g, M, (max(FRONT_FRAMES) + 1) * (L // 2))
    if (N, L, B) == FRONT_QUIET:
        x[1] *= QUIET
    return p, x.to(F32)


@functools.lru_cache(maxsize=None)
def back_inputs(N, L, B, C, softmax, M=M_TEST):
    """-> (params, y [M, B, T], w [M, N, T] >= 0, hop samples [M, (T + 1) * S]), T = sum(BACK_FRAMES).  Softmax cases: frame 0 of
    stream 0 has scores of exactly +-80 (y is e_0 there and row 0 of y is 0 elsewhere, Wm[:, 0] = +-80), frame 1 has equal scores
    (y = 0)."""
    g = _gen(3, N, L, B, C, int(softmax))
    T = sum(BACK_FRAMES)
    Wm, V = _randn(g, C * N, B) / B ** 0.5, _randn(g, L, N) / N ** 0.5
    y, w = _randn(g, M, B, T), _randn(g, M, N, T).clamp_min(0)
    if softmax:
        y[:, 0, :] = 0
        y[0, :, 0], y[0, 0, 0] = 0, 1
        y[0, :, 1] = 0
        sign = (torch.arange(C * N) // N + torch.arange(C * N) % N) % 2 * 2 - 1      # alternates over speakers and over channels
        Wm[:, 0] = 80.0 * sign
    p = types.SimpleNamespace(L=L, C=C, softmax=bool(softmax), Wm=Wm.to(F32), V=V.to(F32))
    return p, y.to(F32), w.to(F32), _randn(g, M, (T + 1) * (L // 2)).to(F32)


def params_from_state_dict(cfg, sd):
    """oracle.ctn_oracle's flat state_dict of a causal cLN config -> the parameters of `Stream`."""
    from oracle import ctn_oracle as O
    blocks = []
    for r in range(cfg.R):
        for x in range(cfg.X):
            k = O.block_keys(cfg, r, x)
            blocks.append(types.SimpleNamespace(W1=sd[k["w1"]][:, :, 0], a1=sd[k["a1"]], g1=sd[k["g1"]].reshape(-1), b1=sd[k["b1"]].reshape(-1),
                                                D=sd[k["dw"]][:, 0, :], a2=sd[k["a2"]], g2=sd[k["g2"]].reshape(-1), b2=sd[k["b2"]].reshape(-1),
                                                W2=sd[k["w2"]][:, :, 0], d=2 ** x))
    return types.SimpleNamespace(L=cfg.L, C=cfg.C, P=cfg.P, softmax=cfg.mask_nonlinear == "softmax", blocks=blocks,
                                 U=sd["encoder.conv1d_U.weight"][:, 0, :], g0=sd["separator.network.0.gamma"].reshape(-1),
                                 b0=sd["separator.network.0.beta"].reshape(-1), Wb=sd["separator.network.1.weight"][:, :, 0],
                                 Wm=sd["separator.network.3.weight"][:, :, 0], V=sd["decoder.basis_signals.weight"])


# ---- the operation -----------------------------------------------------------------------------------------------------------------
def prelu(t, a):
    return torch.where(t >= 0, t, a * t)


class Stream:
    """front / tcn / back of M streams; the per-block n1 histories and the overlap-add carry persist across calls.
    min_var: the smallest cLN column variance seen so far, per stream."""

    def __init__(self, p, M, dtype=F64, wrong=None):
        assert wrong is None or wrong in WRONG, wrong
        self.p, self.M, self.dt, self.wrong = p, M, dtype, wrong
        self.hist = None
        self.carry = None
        self.min_var = torch.full((M,), float("inf"), dtype=F64)
        self.last_frames = None

    def _c(self, t):
        return t.to(self.dt)

    def mm(self, W, t):
        """W [R, K] . t [M, K, F].  fp64: torch's matmul.  The fp32 model: eight interleaved partial sums per output element, each a
        k-ordered chain of separately rounded products and sums, added pairwise at the end -- elementwise IEEE operations only, so
        the model's figures do not depend on which BLAS kernels a machine has."""
        W = self._c(W)
        if self.dt == F64:
            return torch.matmul(W, t)
        (R, K), (M, _, F) = W.shape, t.shape
        Kp = -(-K // LANES) * LANES
        Wl = torch.nn.functional.pad(W, (0, Kp - K)).view(R, Kp // LANES, LANES)
        tl = torch.nn.functional.pad(t, (0, 0, 0, Kp - K)).view(M, Kp // LANES, LANES, F)
        acc = t.new_zeros(M, R, LANES, F)
        for i in range(Kp // LANES):
            acc = acc + Wl[None, :, i, :, None] * tl[:, None, i, :, :]
        n = LANES
        while n > 1:
            n //= 2
            acc = acc[:, :, :n] + acc[:, :, n:2 * n]
        return acc[:, :, 0]

    def csum(self, t):
        """Sum over the channels (dim 1, kept).  The fp32 model: LANES interleaved chains, as in mm()."""
        if self.dt == F64:
            return t.sum(1, keepdim=True)
        M, Ch, F = t.shape
        Cp = -(-Ch // LANES) * LANES
        tl = torch.nn.functional.pad(t, (0, 0, 0, Cp - Ch)).view(M, Cp // LANES, LANES, F)
        acc = t.new_zeros(M, LANES, F)
        for i in range(Cp // LANES):
            acc = acc + tl[:, i]
        n = LANES
        while n > 1:
            n //= 2
            acc = acc[:, :n] + acc[:, n:2 * n]
        return acc

    def sqrt(self, t):
        """The correctly rounded root in either dtype (torch's fp32 root goes through a vector library on some hosts, whose last bit
        depends on the CPU; the fp64 root rounded once more to fp32 is the correctly rounded fp32 root)."""
        return torch.sqrt(t.to(F64)).to(self.dt)

    def softmax(self, t, dim):
        """fp64: torch's.  The fp32 model: exp(t - max) as the fp64 exponential rounded to fp32 (host-independent), summed in index
        order, one division per element."""
        if self.dt == F64:
            return torch.softmax(t, dim)
        e = torch.exp((t - t.amax(dim, keepdim=True)).to(F64)).to(self.dt)
        den = e.select(dim, 0)
        for i in range(1, t.shape[dim]):
            den = den + e.select(dim, i)
        return e / den.unsqueeze(dim)

    def cln(self, t, gamma, beta):
        """Per frame over the channels: biased variance, eps inside the root."""
        Ch = t.shape[1]
        d = t - self.csum(t) / Ch
        var = self.csum(d * d) / (Ch - 1 if self.wrong == "unbiased_variance" else Ch)
        self.min_var = torch.minimum(self.min_var, var.to(F64).amin((1, 2)))
        rstd = 1.0 / (self.sqrt(var) + EPS) if self.wrong == "eps_outside_root" else 1.0 / self.sqrt(var + EPS)
        return self._c(gamma).view(1, -1, 1) * (d * rstd) + self._c(beta).view(1, -1, 1)

    def front(self, x, frames):
        """x [M, >= (frames + 1) * S]: frame k is x[k * S .. k * S + L) -> (w [M, N, frames], y [M, B, frames])."""
        p, L = self.p, self.p.L
        S = L // 2
        x = self._c(x)
        fr = torch.stack([x[:, k * S:k * S + L] for k in range(frames)], 2)         # [M, L, frames]
        w = self.mm(p.U, fr).clamp_min(0)
        return w, self.mm(p.Wb, self.cln(w, p.g0, p.b0))

    def tcn(self, y, n_new_frames=None):
        """y [M, B, F] -> y after every block, for the first n_new_frames (default: all) columns."""
        p, P, wrong = self.p, self.p.P, self.wrong
        y = self._c(y)
        n = y.shape[2] if n_new_frames is None else n_new_frames
        y = y[:, :, :n]
        if self.hist is None:
            self.hist = [y.new_zeros(self.M, b.W1.shape[0], 0) for b in p.blocks]
        for j, b in enumerate(p.blocks):
            a1, a2 = (b.a2, b.a1) if wrong == "alphas_swapped" else (b.a1, b.a2)
            h = self.mm(b.W1, y)
            if wrong == "prelu_after_norm":
                n1 = prelu(self.cln(h, b.g1, b.b1), self._c(a1))
            else:
                n1 = self.cln(prelu(h, self._c(a1)), b.g1, b.b1)
            past = self.hist[j]
            T0 = past.shape[2]
            self.hist[j] = torch.cat([past, n1], 2)
            src = torch.cat([torch.zeros_like(past), n1], 2) if wrong == "history_zeroed" else self.hist[j]
            d = b.d + 1 if wrong == "dilation_plus_one" else b.d
            z = torch.zeros_like(n1)
            for t in range(P):
                off = (P - 1 - t) * d - (d if wrong == "future_tap" else 0)
                idx = T0 + torch.arange(n) - off
                ok = ((idx >= 0) & (idx < T0 + n)).to(self.dt)                       # zeros before the stream's first frame
                tap = self._c(b.D)[:, P - 1 - t if wrong == "taps_reversed" else t]
                z = z + tap.view(1, -1, 1) * (src[:, :, idx.clamp(0, T0 + n - 1)] * ok)
            n2 = self.cln(prelu(z, self._c(a2)), b.g2, b.b2)
            r = self.mm(b.W2, n2)
            y = r if wrong == "residual_dropped" else y + r
        return y

    def back(self, y, w):
        """y [M, B, F], w [M, N, F] -> (out [M, C, F * S], the new carry [M, C, S]); the decoder frames [M, C, L, F] stay in
        last_frames."""
        p, M, C, L = self.p, self.M, self.p.C, self.p.L
        S, F = L // 2, y.shape[2]
        y, w = self._c(y), self._c(w)
        N = w.shape[1]
        score = self.mm(p.Wm, y).view(M, C, N, F)
        if not p.softmax:
            mask = score.clamp_min(0)
        else:
            mask = self.softmax(score, 2 if self.wrong == "softmax_over_n" else 1)
        fr = self.mm(p.V, (w.unsqueeze(1) * mask).reshape(M * C, N, F)).view(M, C, L, F)
        if self.carry is None or self.wrong == "ola_carry_dropped":
            self.carry = fr.new_zeros(M, C, S)
        prev = torch.cat([self.carry.unsqueeze(3), fr[:, :, S:, :F - 1]], 3)        # the second half of the frame before
        out = (fr[:, :, :S, :] + prev).permute(0, 1, 3, 2).reshape(M, C, F * S)
        self.carry = fr[:, :, S:, F - 1].clone()
        self.last_frames = fr
        return out, self.carry


def rel_err(got, ref):
    """max |got - ref| / max |ref| per stream (dim 0), the largest over the streams."""
    M = ref.shape[0]
    d = (got.to(F64) - ref.to(F64)).abs().reshape(M, -1).amax(1)
    return float((d / ref.to(F64).abs().reshape(M, -1).amax(1)).max())


# ---- every case of the GPU module under one model (dtype, wrong) -> {kind: [(case label, figure)]} --------------------------------------
@functools.lru_cache(maxsize=None)
def stack_reference(ci):
    p, y = stack_inputs(ci)
    return Stream(p, y.shape[0]).tcn(y)


def stack_model(ci, dtype, wrong=None):
    """The whole signal of a stack case, call by call along its plan -> y [M, B, T]."""
    p, y = stack_inputs(ci)
    s, outs, t0 = Stream(p, y.shape[0], dtype, wrong), [], 0
    for n in stack_plan(STACK_CASES[ci]):
        outs.append(s.tcn(y[:, :, t0:t0 + n]))
        t0 += n
    return torch.cat(outs, 2), s


@functools.lru_cache(maxsize=None)
def front_reference(N, L, B):
    p, x = front_inputs(N, L, B)
    return Stream(p, x.shape[0]).front(x, max(FRONT_FRAMES))


def back_model(case, dtype=F64, wrong=None):
    """BACK_FRAMES calls -> [(frames [M,C,L,F], out [M,C,F*S], carry [M,C,S])] per call."""
    p, y, w, _ = back_inputs(*case)
    s, res, t0 = Stream(p, y.shape[0], dtype, wrong), [], 0
    for n in BACK_FRAMES:
        out, carry = s.back(y[:, :, t0:t0 + n], w[:, :, t0:t0 + n])
        res.append((s.last_frames, out, carry))
        t0 += n
    return res


@functools.lru_cache(maxsize=None)
def back_reference(case):
    return back_model(case)


def model_figures(dtype, wrong=None):
    """-> {kind: {case label: figure}}: what a model shows against the fp64 oracle on the GPU module's inputs."""
    fig = collections.defaultdict(dict)
    for ci, c in enumerate(STACK_CASES):
        got, _ = stack_model(ci, dtype, wrong)
        fig["stack_y"]["stack %d" % ci] = rel_err(got, stack_reference(ci))
    for case in FRONT_CASES:
        p, x = front_inputs(*case)
        w, y = Stream(p, x.shape[0], dtype, wrong).front(x, max(FRONT_FRAMES))
        rw, ry = front_reference(*case)
        fig["w"]["front %s" % (case,)] = rel_err(w, rw)
        fig["front_y"]["front %s" % (case,)] = rel_err(y, ry)
    for case in BACK_CASES:
        got, ref = back_model(case, dtype, wrong), back_reference(case)
        fig["frames"]["back %s" % (case,)] = max(rel_err(g[0], r[0]) for g, r in zip(got, ref))
        fig["samples"]["back %s" % (case,)] = max(rel_err(g[1], r[1]) for g, r in zip(got, ref))
    return fig
