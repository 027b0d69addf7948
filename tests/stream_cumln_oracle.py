"""The contract of the cumulative fused streaming stack (csrc/ctn_stream.hip: ctn_stream_tcn_cumln and its ragged form; include/ctn_hip.h)
in plain torch on the CPU, on top of tests/stream_oracle.py (imported, not copied: Stream, its fp32 arithmetic, make_block, stack_plan,
ragged_counts, rel_err).

`CumStream` is stream_oracle.Stream with both norms of every block cumulative: per block and norm it carries (C1, C2, count), the sums
of a and a^2 over all channels of all frames so far and the number of frames, and frame k of a call is normalised by
    C = carry + the sums of this call's frames 0 .. k,  n = Ch (count + k + 1),  mu = C1 / n,  r = 1 / sqrt(max(C2 / n - mu^2, 0) + eps).
Its `front` stays per frame (the encoder-output norm is per frame for every norm_type).  dtype float64 is the reference.  dtype
float32 is the fp32 MODEL: stream_oracle's fp32 GEMM / channel-sum / tap arithmetic, and for the statistics the contract of the
kernels: fp64 from the per-frame sums on, mu and r rounded to fp32 once, the apply in fp32.  `wrong` names one deliberate defect (WRONG).

Cases: (B, H, P, dilations), all with max_frames = 16 and M = 3 streams -- one ordinary, one at stream_oracle.QUIET amplitude, one 100
times louder.  Plans: stream_oracle.stack_plan's two cuts (calls capped at 16 frames) until every ring has wrapped three times; for the
first case also LONG_FRAMES frames in 16-frame calls, so that the carried sums and the count go far beyond one ring.

Limit (LIMIT["stack_y_cum"], of max |ref| per stream): 4x the largest figure the fp32 model shows against the fp64 reference over these
cases and plans, rounded up to one significant digit (FP32_FIGURE: the CPU figure, asserted by test_stream_cumln_cpu.py to stay inside
LIMIT / 4).  The factor 4 is the headroom of stream_oracle's limits.  Never derived from what the kernels give.
"""
import functools
import types

import torch

import stream_oracle as SO
from stream_oracle import F32, F64, EPS, QUIET, rel_err, ragged_counts, stack_plan, ring_len  # noqa: F401  (shared, not copied)

M_TEST = 3
LOUD = 100.0
LONG_FRAMES = 4096

CASES = (
    SO.StackCase(16, 16, 3, (1, 2), 16, ("one_k_group", "tap_inside_tile")),
    SO.StackCase(48, 80, 3, (1, 5, 16), 16, ("two_rows_per_thread", "dilation_one_tile")),
    SO.StackCase(16, 528, 3, (8, 8), 16, ("nine_rows_per_thread", "empty_slices")),
    SO.StackCase(512, 240, 1, (1, 1), 16, ("lds_bound", "P1")),
)
CASE_IDS = ["B%d-H%d-P%d" % c[:3] for c in CASES]

# largest fp32-model figure over all cases and plans (test_stream_cumln_cpu.py::test_fp32_model_stays_four_times_inside prints them)
FP32_FIGURE = {"stack_y_cum": 3.19e-7}           # case (512, 240, 1), either cut; the long plan of case 0: 2.31e-7
LIMIT = {"stack_y_cum": 2e-6}

WRONG = ("per_frame_stats", "carry_dropped", "count_restarts", "count_off_by_one", "norms_share_record", "pad_columns_counted")


def plans(ci):
    """{name: frames per call} of a case: the two cuts, and for case 0 the long plan."""
    c = CASES[ci]
    out = {"cut0": stack_plan(c, 0), "cut1": stack_plan(c, 1)}
    if ci == 0:
        out["long"] = [16] * (LONG_FRAMES // 16)
    assert all(1 <= n <= 16 for p in out.values() for n in p)
    return out


@functools.lru_cache(maxsize=None)
def stack_inputs(ci, long=False):
    """-> (params, y [3, B, T] fp32); T = the frames of the case's cuts, or LONG_FRAMES.  Stream 1 is quiet, stream 2 loud."""
    c = CASES[ci]
    g = SO._gen(7, ci)
    p = types.SimpleNamespace(P=c.P, blocks=[SO.make_block(g, c.B, c.H, c.P, d) for d in c.dil])
    T = LONG_FRAMES if long else sum(stack_plan(c))
    y = SO._randn(SO._gen(8, ci, int(long)), M_TEST, c.B, T)
    y[1] *= QUIET
    y[2] *= LOUD
    return p, y.to(F32)


class CumStream(SO.Stream):
    """stream_oracle.Stream with cumulative block norms.  rec[(block, norm)] = (C1 [M], C2 [M] fp64, frames so far)."""

    def __init__(self, p, M, dtype=F64, wrong=None):
        assert wrong is None or wrong in WRONG, wrong
        super().__init__(p, M, dtype, None)
        self.wrong = wrong
        self.rec = {}

    def cumln(self, t, gamma, beta, key, tile=16):
        """t [M, Ch, F] (after PReLU), the frames of one call, F <= tile for the defect that needs a tile."""
        wrong = self.wrong
        if wrong == "per_frame_stats":
            return self.cln(t, gamma, beta)
        if wrong == "norms_share_record":
            key = (key[0], 0)
        M, Ch, F = t.shape
        s1, s2 = self.csum(t)[:, 0].to(F64), self.csum(t * t)[:, 0].to(F64)           # fp64 from the per-frame sums on
        c1, c2, cnt = self.rec.get(key, (torch.zeros(M, dtype=F64), torch.zeros(M, dtype=F64), 0))
        if wrong == "carry_dropped":
            c1, c2, cnt = torch.zeros_like(c1), torch.zeros_like(c2), 0
        C1, C2 = c1[:, None] + s1.cumsum(1), c2[:, None] + s2.cumsum(1)
        k = torch.arange(F, dtype=F64) + (0 if wrong == "count_restarts" else cnt)
        n = Ch * ((k if wrong == "count_off_by_one" else k + 1).clamp_min(1))
        mu = C1 / n
        r = 1.0 / torch.sqrt((C2 / n - mu * mu).clamp_min(0) + EPS)
        e1, e2 = C1[:, -1], C2[:, -1]
        if wrong == "pad_columns_counted" and F < tile:
            # the columns F .. tile - 1 of the tile enter the carried sums (not the count): modelled as repeats of the last frame
            e1, e2 = e1 + (tile - F) * s1[:, -1], e2 + (tile - F) * s2[:, -1]
        self.rec[key] = (e1, e2, cnt + F)
        mu, r = mu.to(self.dt)[:, None, :], r.to(self.dt)[:, None, :]                 # rounded once (fp64: unchanged)
        return self._c(gamma).view(1, -1, 1) * ((t - mu) * r) + self._c(beta).view(1, -1, 1)

    def tcn(self, y, n_new_frames=None):
        """y [M, B, F] -> y after every block; every carry advanced."""
        p, P = self.p, self.p.P
        y = self._c(y)
        n = y.shape[2] if n_new_frames is None else n_new_frames
        y = y[:, :, :n]
        if self.hist is None:
            self.hist = [y.new_zeros(self.M, b.W1.shape[0], 0) for b in p.blocks]
        for j, b in enumerate(p.blocks):
            n1 = self.cumln(SO.prelu(self.mm(b.W1, y), self._c(b.a1)), b.g1, b.b1, (j, 0))
            T0 = self.hist[j].shape[2]
            self.hist[j] = torch.cat([self.hist[j], n1], 2)
            z = torch.zeros_like(n1)
            for t in range(P):
                idx = T0 + torch.arange(n) - (P - 1 - t) * b.d
                ok = (idx >= 0).to(self.dt)                                           # zeros before the stream's first frame
                z = z + self._c(b.D)[:, t].view(1, -1, 1) * (self.hist[j][:, :, idx.clamp_min(0)] * ok)
            n2 = self.cumln(SO.prelu(z, self._c(b.a2)), b.g2, b.b2, (j, 1))
            y = y + self.mm(b.W2, n2)
        return y


@functools.lru_cache(maxsize=None)
def stack_reference(ci, long=False):
    """fp64, the whole signal in one call."""
    p, y = stack_inputs(ci, long)
    return CumStream(p, y.shape[0]).tcn(y)


def stack_model(ci, plan, dtype, wrong=None, long=False):
    """The signal of a case, call by call along `plan` -> y [M, B, T]."""
    p, y = stack_inputs(ci, long)
    s, outs, t0 = CumStream(p, y.shape[0], dtype, wrong), [], 0
    for n in plan:
        outs.append(s.tcn(y[:, :, t0:t0 + n]))
        t0 += n
    assert t0 == y.shape[2]
    return torch.cat(outs, 2)


def model_figures(dtype, wrong=None):
    """-> {(case, plan name): figure} of a model against the fp64 reference."""
    fig = {}
    for ci in range(len(CASES)):
        for name, plan in plans(ci).items():
            long = name == "long"
            fig[(ci, name)] = rel_err(stack_model(ci, plan, dtype, wrong, long), stack_reference(ci, long))
    return fig
