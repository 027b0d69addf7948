"""Chunked (streaming) inference for the causal / cLN variant.

With ``causal=True, norm_type='cLN'`` every layer of the reference is frame-local (1x1 convs, PReLU, the
per-frame cLN of src/conv_tasnet.py:313-335 -- which is NOT cumulative) except the depthwise conv,
which looks (P-1)*dilation frames into the past (src/conv_tasnet.py:182,253-256,281-295).  So a stream can be
separated chunk by chunk, exactly, by carrying per block the last (P-1)*dilation frames of the depthwise input,
plus the encoder's L-S input samples and the decoder's L-S overlap-add samples.  Total left context is
R*(P-1)*(2^X-1) frames (2040 at the paper config) -- but it is state, not recomputation.

``norm_type='cumLN'`` (the paper's cumulative layer norm, csrc/ctn_cumln.hip) adds one more kind of state: per norm the prefix sums
of the frames so far and their count, kept in device memory and advanced by the scan kernel itself (so a captured graph replays
it); the order of the prefix sums is fixed by the absolute frame index, so the statistics do not depend on the chunking.
`StreamingSeparator` serves such models with the training kernels; the fused classes below serve them with ``cumulative=True``: the
fused kernels then carry one (sum, sum of squares, frame count) record per stream, block and norm in a device buffer of their own
and run at most 16 frames (one tile) per stream and step, because a tile's statistics need the sums of the tiles before it.

All arithmetic runs through the same HIP entry points as training (ops.py); torch only slices / concatenates.
"""
import functools

import torch

from . import ops
from ._lib import lib
from .resample import ZEROS


def _padded(t, K):
    """[M,Ch,K] (any stride) -> contiguous zero-padded [M,Ch,Kp]."""
    Kp = ops.padded_frames(K)
    out = t.new_zeros(t.shape[:-1] + (Kp,))
    out[..., :K] = t
    return out


class StreamingSeparator:
    """Stateful chunk-wise separation with a causal ConvTasNet (norm_type 'cLN' or 'cumLN').

        s = StreamingSeparator(model, batch=1)
        for chunk in stream:            # chunk: [M, n*S] samples, S = L//2, n >= 1
            out = s.push(chunk)         # [M, C, n*S]  (delayed by L-S samples)
        tail = s.flush()                # [M, C, L-S]
    Concatenating every `out` and `tail` reproduces ``model(full_mixture)`` on the whole signal.

    ``graph=True``: a chunk is ~300 small launches issued from Python (4 ms of host time for 100 ms of audio); every chunk after
    the first has the same shape, so from the third chunk of a given length on the whole step -- kernels, state updates, the
    copies between them -- is replayed as ONE HIP graph (the second chunk runs eagerly and sizes the workspaces).  The state
    lives in fixed buffers updated in place, so eager and replayed chunks can be mixed; same kernels, same order: same bits.
    """

    def __init__(self, model, batch=1, graph=False):
        if not model.causal or model.norm_type not in ("cLN", "cumLN"):
            raise ValueError("streaming needs the causal cLN or cumLN variant (gLN statistics span the whole utterance)")
        self.cum = model.norm_type == "cumLN"
        self.m = model
        self.M = batch
        self.L, self.S = model.L, model.L // 2
        self.dev = next(model.parameters()).device
        self.soft = model.separator.softmax_mask()
        self.use_graph = bool(graph) and self.dev.type == "cuda"
        self.reset()

    def reset(self):
        m, dev, M = self.m, self.dev, self.M
        if getattr(self, "hist", None) is None:         # fixed buffers: a captured graph keeps their addresses
            self.in_tail = torch.zeros((M, self.L - self.S), device=dev)
            self.ola_tail = torch.zeros((M, m.C, self.L - self.S), device=dev)
            self.hist = []
            for rep in m.separator.network[2]:
                for blk in rep:
                    halo = (m.P - 1) * blk.dilation
                    self.hist.append(torch.zeros((M, m.H, halo), device=dev))
            # cumLN: per norm the prefix sums and the frame count so far, on the device (the scan kernel advances them: graph replay)
            self.cum_state = [ops.cumln_state(M, dev) for _ in range(2 * len(self.hist))] if self.cum else []
            # the norm pass of norm j (block i: 2i and 2i + 1): cln_fwd, or cumln_fwd bound to that norm's state
            self.norms = [functools.partial(ops.cumln_fwd, state=st) for st in self.cum_state] or [ops.cln_fwd] * (2 * len(self.hist))
            self._graphs = {}            # chunk length -> (graph, static chunk, static output)
            self._seen = {}              # chunk length -> eager steady-state chunks so far
        else:
            self.in_tail.zero_()
            self.ola_tail.zero_()
            for h in self.hist:
                h.zero_()
            for carry, count in self.cum_state:
                carry.zero_()
                count.zero_()
        self.first = True

    @torch.no_grad()
    def push(self, chunk):
        S, L, M = self.S, self.L, self.M
        assert chunk.shape[0] == M and chunk.shape[1] % S == 0 and chunk.shape[1] >= L
        chunk = chunk.to(self.dev, torch.float32)
        if self.first:
            self.first = False
            return self._step(chunk, True).clone()      # the very first frame starts at sample 0
        n = chunk.shape[1]
        if not self.use_graph:
            return self._step(chunk, False).clone()
        if n not in self._graphs:
            if self._seen.get(n, 0) < 1:                 # one eager chunk of this length first: workspaces, allocator
                self._seen[n] = self._seen.get(n, 0) + 1
                return self._step(chunk, False).clone()
            static_in = chunk.clone()
            torch.cuda.synchronize(self.dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):                   # records, does not run: the state is untouched until the replay
                static_out = self._step(static_in, False)
            self._graphs[n] = (g, static_in, static_out)
        g, static_in, static_out = self._graphs[n]
        static_in.copy_(chunk)
        g.replay()
        return static_out.clone()

    def _step(self, chunk, first):
        """One chunk through the network; carried state updated in place.  Returns a view of this step's output buffer."""
        m, S, L, M = self.m, self.S, self.L, self.M
        x = chunk if first else torch.cat([self.in_tail, chunk], dim=1)
        self.in_tail.copy_(x[:, x.shape[1] - (L - S):])
        T = x.shape[1]
        K = (T - L) // S + 1
        Kp = ops.padded_frames(K)
        sep = m.separator
        # encoder -> input cLN -> bottleneck
        xcol = torch.empty((M, L, Kp), device=self.dev)
        x = x.contiguous()
        lib.call("ctn_im2col", x.data_ptr(), xcol.data_ptr(), M, T, L, L, K, Kp, ops._stream())
        w, _ = ops.pw_gemm(m.encoder.conv1d_U.weight, xcol, m.N, L, K, relu_out=True)
        y, _, _ = ops.cln_fwd(w, sep.network[0].gamma, sep.network[0].beta, None, K)
        y, _ = ops.pw_gemm(sep.network[1].weight, y, m.B, m.N, K)
        # temporal blocks with carried depthwise history
        i = 0
        for rep in sep.network[2]:
            for blk in rep:
                ds = blk.net[3]
                halo = (m.P - 1) * blk.dilation
                h, _ = ops.pw_gemm(blk.net[0].weight, y, m.H, m.B, K)
                n1, _, _ = self.norms[2 * i](h, blk.net[2].gamma, blk.net[2].beta, blk.net[1].weight, K)
                cat = torch.cat([self.hist[i], n1[..., :K]], dim=2)          # [M, H, halo + K]
                self.hist[i].copy_(cat[..., cat.shape[2] - halo:])
                Kc = halo + K
                z, _ = ops.dw_fwd(_padded(cat, Kc), ds.net[0].weight, Kc, blk.dilation, True)
                z = _padded(z[..., halo:Kc], K)
                n2, _, _ = self.norms[2 * i + 1](z, ds.norm().gamma, ds.norm().beta, ds.prelu().weight, K)
                y, _ = ops.pw_gemm(ds.pointwise().weight, n2, m.B, m.H, K, residual=y)
                i += 1
        # mask -> decoder frames -> overlap-add with carry
        score, _ = ops.pw_gemm(sep.network[3].weight, y, m.C * m.N, m.B, K)
        sw = ops.mask_apply(score, w, m.C, self.soft)
        fr, _ = ops.pw_gemm(m.decoder.basis_signals.weight, sw.view(M * m.C, m.N, Kp), L, m.N, K)
        Tc = (K - 1) * S + L
        est = torch.empty((M, m.C, Tc), device=self.dev)
        lib.call("ctn_ola", fr.data_ptr(), est.data_ptr(), M * m.C, Tc, L, L, K, Kp, ops._stream())
        est[..., : L - S] += self.ola_tail
        self.ola_tail.copy_(est[..., K * S:])
        return est[..., : K * S]

    @torch.no_grad()
    def flush(self):
        """The last L-S output samples (their second overlap-add tap never arrives)."""
        out = self.ola_tail.clone()
        self.ola_tail.zero_()
        return out


CUM_STEP = 16    # frames per stream and step of the cumulative kernels: one tile (ctn_stream_tcn_cumln in include/ctn_hip.h)


def check_fused_model(model, cumulative):
    """-> bool(cumulative) if the fused streaming kernels serve `model` in that mode, else ValueError (pure host code, no GPU)."""
    if not model.causal or model.norm_type not in ("cLN", "cumLN"):
        raise ValueError("the fused streaming kernels need the causal cLN or cumLN variant (gLN statistics span the whole utterance)")
    if model.norm_type == "cumLN" and not cumulative:
        raise ValueError("a cumLN model needs cumulative=True here (or StreamingSeparator): the cumulative kernels are opt-in because "
                         "they keep a carry record per stream, block and norm and run at most %d frames per stream and step "
                         "(longer pushes are cut into such steps)" % CUM_STEP)
    if cumulative and model.norm_type != "cumLN":
        raise ValueError("cumulative=True is for norm_type 'cumLN'; this model has norm_type %r" % (model.norm_type,))
    return bool(cumulative)


class _FusedBase:
    """What FusedStreamingSeparator and FusedStreamPool share: the checks, the packed weights and the fixed buffers of a chunk step."""

    def _setup(self, model, batch, max_chunk_frames, graph, cumulative=False):
        import ctypes
        self.cumulative = check_fused_model(model, cumulative)
        if max_chunk_frames < 1 or batch < 1:
            raise ValueError("batch and max_chunk_frames must be positive")
        m = self.m = model
        self.M, self.F = int(batch), int(max_chunk_frames)
        if self.cumulative:
            self.F = min(self.F, CUM_STEP)       # one tile per stream and step; push / plan_steps cut longer pushes at self.F
        self.L, self.S = m.L, m.L // 2
        if m.L % 4 or m.N % 16 or m.B % 16 or m.H % 16:
            raise ValueError("the fused streaming kernels need L % 4 == 0 and N, B, H multiples of 16")
        self.dev = dev = next(model.parameters()).device
        self.soft = int(m.separator.softmax_mask())
        self.use_graph = bool(graph) and dev.type == "cuda"
        self.blocks = [blk for rep in m.separator.network[2] for blk in rep]
        nb = self.nb = len(self.blocks)
        self.dil = (ctypes.c_int * nb)(*[int(b.dilation) for b in self.blocks])
        M, F, S = self.M, self.F, self.S
        u8 = dict(dtype=torch.uint8, device=dev)
        self.state_bytes = lib.ctn_stream_state_bytes(M, m.H, m.P, self.dil, nb, F)
        self.state = torch.zeros(self.state_bytes, **u8)
        # cumLN: the carry records of every slot, block and norm (two banks); zeros = the start of a stream
        self.cum = torch.zeros(lib.ctn_stream_cum_bytes(M, nb), **u8) if self.cumulative else None
        self.packed = torch.empty(lib.ctn_stream_pack_bytes(m.B, m.H, m.P, nb), **u8)
        self.Up = torch.empty(lib.ctn_stream_pack_gemm_bytes(m.N, m.L), **u8)
        self.Wbp = torch.empty(lib.ctn_stream_pack_gemm_bytes(m.B, m.N), **u8)
        self.Wmp = torch.empty(lib.ctn_stream_pack_gemm_bytes(m.C * m.N, m.B), **u8)
        self.Vp = torch.empty(lib.ctn_stream_pack_gemm_bytes(m.L, m.N), **u8)
        # fixed buffers: a captured graph keeps their addresses
        self.xld = (F + 1) * S
        self.x = torch.zeros((M, self.xld), device=dev)              # [carried S samples | chunk]
        self.w = torch.empty((M * m.N * F,), device=dev)
        self.y = torch.empty((M * m.B * F,), device=dev)
        self.fr = torch.empty((M * m.C * m.L * F,), device=dev)
        self.out = torch.empty((M * m.C * F * S,), device=dev)
        self.ola_tail = torch.zeros((M, m.C, self.L - S), device=dev)
        self._graphs = {}            # frames -> graph
        self._seen = set()           # frames of the steady-state steps run eagerly so far
        self.refresh()

    @torch.no_grad()
    def refresh(self):
        """Re-pack the model's weights (after a load_state_dict / an optimiser step); the stream state is untouched."""
        m, sep = self.m, self.m.separator
        params = []
        for blk in self.blocks:
            ds = blk.net[3]
            params += [blk.net[0].weight, blk.net[1].weight, blk.net[2].gamma, blk.net[2].beta, ds.net[0].weight,
                       ds.prelu().weight, ds.norm().gamma, ds.norm().beta, ds.pointwise().weight]
        self._params = [ops._c(p.detach().to(torch.float32)) for p in params]
        ops._chk(*self._params)
        st = ops._stream()
        lib.call("ctn_stream_pack", ops._ptr_table(self._params), self.nb, m.B, m.H, m.P, self.packed.data_ptr(), st)
        self._small = [ops._c(t.detach().to(torch.float32)) for t in
                       (m.encoder.conv1d_U.weight, sep.network[1].weight, sep.network[3].weight, m.decoder.basis_signals.weight,
                        sep.network[0].gamma, sep.network[0].beta)]
        ops._chk(*self._small)
        U, Wb, Wm, V = self._small[:4]
        lib.call("ctn_stream_pack_gemm", U.data_ptr(), m.N, m.L, self.Up.data_ptr(), st)
        lib.call("ctn_stream_pack_gemm", Wb.data_ptr(), m.B, m.N, self.Wbp.data_ptr(), st)
        lib.call("ctn_stream_pack_gemm", Wm.data_ptr(), m.C * m.N, m.B, self.Wmp.data_ptr(), st)
        lib.call("ctn_stream_pack_gemm", V.data_ptr(), m.L, m.N, self.Vp.data_ptr(), st)

    def _run(self, frames):
        if not self.use_graph:
            return self._step(frames).clone()
        if frames not in self._graphs:
            if frames not in self._seen:                 # one eager step of this length first (module load, allocator)
                self._seen.add(frames)
                return self._step(frames).clone()
            torch.cuda.synchronize(self.dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):                    # records, does not run: the state is untouched until the replay
                self._step(frames)
            self._graphs[frames] = g
        self._graphs[frames].replay()
        return self._out_view(frames).clone()

    def _out_view(self, frames):
        m = self.m
        return self.out[: self.M * m.C * frames * self.S].view(self.M, m.C, frames * self.S)


class FusedStreamingSeparator(_FusedBase):
    """Low-latency, many-stream form of `StreamingSeparator`: same contract, one fused launch per block boundary.

        s = FusedStreamingSeparator(model, batch=32, max_chunk_frames=16)
        out = s.push(chunk)             # chunk [M, n*S] -> [M, C, n*S] (the very first push: [M, C, (n-1)*S], and needs n*S >= L)
        tail = s.flush()                # [M, C, L-S]
    Concatenating every `out` and `tail` reproduces ``model(full_mixture)``.

    A chunk costs nblocks + 5 launches (csrc/ctn_stream.hip) on unpadded [M, Ch, frames] activations: front end, one stage per
    block boundary with the depthwise history in per-block ring buffers, back end with the overlap-add carry; chunks of at most 16
    frames run each block as two launches spread over up to 16 workgroups per stream (2 * nblocks + 4 launches).  The arithmetic is
    frame-local and in a fixed order (exact fp32 MFMA chains; it does not follow `set_gemm_arith`), so the output samples are
    BITWISE independent of how the signal was cut into chunks and of the other streams of the batch.  Every push after the first
    accepts any n >= 1; a chunk of more than `max_chunk_frames` frames is split inside `push`.

    The weights are packed into the kernels' fragment order at construction: call `refresh()` after the model's parameters changed.
    ``graph=True`` replays the chunk step of a given length as one HIP graph from its second occurrence on (same kernels: same bits).

    Every stream of the batch starts on the same push and delivers the same number of hops; streams that join, leave, reset or
    deliver different amounts per push are served by `FusedStreamPool` (below; same kernels, same bits).  Out of scope: gLN /
    non-causal models (ValueError), training (no autograd).

    ``cumulative=True`` serves a causal cumLN model (the paper's cumulative layer norm) on the cumulative forms of the same kernels
    (ctn_stream_tcn_cumln): `max_chunk_frames` is clamped to 16, a step is the same 2 * nblocks + 4 launches (the one that advances
    the ring position also commits the carry records), a longer push is cut into consecutive 16-frame steps inside `push`, and the
    same bitwise independence of the chunking and of the other streams holds.  It is opt-in: a cumLN model without the keyword, and the
    keyword with any other model, is a ValueError.
    """

    def __init__(self, model, batch=1, max_chunk_frames=64, graph=False, cumulative=False):
        self._setup(model, batch, max_chunk_frames, graph, cumulative)
        self.first = True

    def reset(self):
        """Back to the start of a stream (every stream of the batch); packed weights and captured graphs stay valid."""
        lib.call("ctn_stream_reset", self.state.data_ptr(), self.state_bytes, ops._stream())
        if self.cumulative:
            self.cum.zero_()
        self.x.zero_()
        self.ola_tail.zero_()
        self.first = True

    @torch.no_grad()
    def push(self, chunk):
        S, L, M = self.S, self.L, self.M
        if chunk.dim() != 2 or chunk.shape[0] != M or chunk.shape[1] % S or chunk.shape[1] < (L if self.first else S):
            raise ValueError("chunk must be [%d, n*%d] with n*%d >= %d" % (M, S, S, L if self.first else S))
        chunk = chunk.to(self.dev, torch.float32)
        outs, pos, n = [], 0, chunk.shape[1] // S
        while pos < n:
            if self.first:               # the very first frame starts at sample 0: n hops hold n - 1 frames
                hops = min(n - pos, self.F + 1)
                self.x[:, :hops * S].copy_(chunk[:, pos * S:(pos + hops) * S])
                frames = hops - 1
                self.first = False
            else:
                hops = frames = min(n - pos, self.F)
                self.x[:, S:(hops + 1) * S].copy_(chunk[:, pos * S:(pos + hops) * S])
            pos += hops
            if frames:
                outs.append(self._run(frames))
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=2)

    def _step(self, frames):
        """`frames` frames of the sample buffer through the network; every carry updated in place.  Returns a view of the output buffer."""
        m, M, st = self.m, self.M, ops._stream()
        g0, b0 = self._small[4], self._small[5]
        lib.call("ctn_stream_front", self.x.data_ptr(), self.xld, self.Up.data_ptr(), g0.data_ptr(), b0.data_ptr(), self.Wbp.data_ptr(),
                 self.w.data_ptr(), self.y.data_ptr(), M, m.N, m.L, m.B, frames, st)
        if self.cumulative:
            lib.call("ctn_stream_tcn_cumln", self.packed.data_ptr(), self.dil, self.nb, self.y.data_ptr(), self.state.data_ptr(),
                     self.cum.data_ptr(), M, m.B, m.H, m.P, frames, self.F, st)
        else:
            lib.call("ctn_stream_tcn_cln", self.packed.data_ptr(), self.dil, self.nb, self.y.data_ptr(), self.state.data_ptr(),
                     M, m.B, m.H, m.P, frames, self.F, st)
        lib.call("ctn_stream_back", self.y.data_ptr(), self.w.data_ptr(), self.Wmp.data_ptr(), self.Vp.data_ptr(), self.fr.data_ptr(),
                 self.out.data_ptr(), self.ola_tail.data_ptr(), self.x.data_ptr(), self.xld, M, m.N, m.L, m.B, m.C, frames, self.soft, st)
        return self._out_view(frames)

    @torch.no_grad()
    def flush(self):
        """The last L-S output samples (their second overlap-add tap never arrives)."""
        out = self.ola_tail.clone()
        self.ola_tail.zero_()
        return out


TAB = 8      # ints per slot of a step table (CTN_STREAM_TAB in include/ctn_hip.h): nf, nh, src, dst, out, 3 unused


def plan_steps(hops, fresh, F):
    """Cut one ragged push into steps of at most `F` frames per slot (pure host code, no GPU).

    hops[m]: hops slot m delivers with this push; fresh[m]: its stream starts with this push (its first hop only primes the carry:
    h hops hold h - 1 frames, and they land at offset 0 of the sample buffer instead of behind the carried hop).
    -> list of (frames, max_hops, rows): rows[m] = [nf, nh, src, dst, out, 0, 0, 0] in hops (the table of include/ctn_hip.h),
    frames = max nf, max_hops = max nh.  Step i holds every slot's i-th piece; slots that ran out have nf = nh = 0.
    """
    M = len(hops)
    left, new = [int(h) for h in hops], [bool(f) for f in fresh]
    src, out = [0] * M, [0] * M
    steps = []
    while any(left):
        rows = []
        for m in range(M):
            if new[m] and left[m]:
                nh = min(left[m], F + 1)
                nf, dst = nh - 1, 0
                new[m] = False
            else:
                nh = nf = min(left[m], F)
                dst = 1
            rows.append([nf, nh, src[m], dst, out[m], 0, 0, 0])
            left[m] -= nh
            src[m] += nh
            out[m] += nf
        steps.append((max(r[0] for r in rows), max(r[1] for r in rows), rows))
    return steps


class FusedStreamPool(_FusedBase):
    """`slots` independent streams on the kernels of `FusedStreamingSeparator`, each with a life of its own.

        pool = FusedStreamPool(model, slots=32, max_chunk_frames=16)
        s = pool.open()                         # a free slot (or pool.open(slot)), reset on the device
        out, lengths = pool.push(chunk, hops)   # chunk [slots, n*S]; slot m delivers hops[m] hops = the first hops[m]*S samples of its row
        tail = pool.close(s)                    # [C, L-S]: the slot's last overlap-add samples; the slot is free again
    `hops` may be any mix of values: 0 (nothing this time), 1 on a slot's very first push (its first hop only primes the carry),
    more than `max_chunk_frames` (split inside `push`).  out is [slots, C, max(lengths)] with zeros beyond lengths[m] = hops[m]*S
    (minus S on the push that carries the slot's first hop).  out[m, :, :lengths[m]] of every push of a slot and its `close()` tail,
    concatenated, are BITWISE what `FusedStreamingSeparator(model, batch=1)` gives for that stream alone, whatever the other slots do.

    A step is a per-slot table (`plan_steps`) uploaded to a fixed device tensor, then the ragged forms of the same launches
    (include/ctn_hip.h, "ragged steps"): one copy of the chunk rows into the sample buffer, front, stack, back, one copy into the
    padded output rows: two launches and one small upload more than the class, none of them per slot.  ``graph=True`` replays
    front + stack + back as one HIP graph per maximum frame count from its second occurrence on; the per-slot counts live in the
    table, never in a graph; `open` / `close` and both copies stay outside the graphs.

    ``cumulative=True``: a cumLN model, as for `FusedStreamingSeparator` (steps of at most 16 frames per slot); `open` also zeroes
    the slot's carry records, and a slot that delivers nothing in a step keeps them bit for bit.
    """

    def __init__(self, model, slots=1, max_chunk_frames=16, graph=False, cumulative=False):
        self._setup(model, slots, max_chunk_frames, graph, cumulative)
        dev, M = self.dev, self.M
        self.pos = torch.zeros(M, dtype=torch.int32, device=dev)
        self.tab = torch.zeros((M, TAB), dtype=torch.int32, device=dev)
        self.is_open, self.fresh = [False] * M, [False] * M
        # pinned staging for the table upload: a ring, each entry with the event of its last copy (never rewritten before that completed)
        self._stage, self._stage_i = [], 0
        if dev.type == "cuda":
            self._stage = [[torch.zeros((M, TAB), dtype=torch.int32).pin_memory(), None] for _ in range(4)]

    def open(self, slot=None):
        """Take a free slot (the lowest, or `slot`) and reset it on the device; returns its index."""
        import ctypes
        if slot is None:
            free = [i for i, o in enumerate(self.is_open) if not o]
            if not free:
                raise ValueError("no free slot (all %d are open)" % self.M)
            slot = free[0]
        slot = int(slot)
        if not 0 <= slot < self.M:
            raise ValueError("slot %d is outside 0..%d" % (slot, self.M - 1))
        if self.is_open[slot]:
            raise ValueError("slot %d is already open" % slot)
        m = self.m
        lib.call("ctn_stream_reset_slots", self.state.data_ptr(), self.x.data_ptr(), self.xld, self.ola_tail.data_ptr(), self.pos.data_ptr(),
                 (ctypes.c_int * 1)(slot), 1, self.M, m.H, m.P, self.dil, self.nb, self.F, m.C, m.L, ops._stream())
        if self.cumulative:
            lib.call("ctn_stream_cum_reset_slots", self.cum.data_ptr(), (ctypes.c_int * 1)(slot), 1, self.M, self.nb, ops._stream())
        self.is_open[slot], self.fresh[slot] = True, True
        return slot

    @torch.no_grad()
    def close(self, slot):
        """The slot's last L-S output samples [C, L-S] (their second overlap-add tap never arrives); the slot is free again."""
        slot = int(slot)
        if not 0 <= slot < self.M or not self.is_open[slot]:
            raise ValueError("slot %r is not open" % (slot,))
        tail = self.ola_tail[slot].clone()
        self.is_open[slot] = self.fresh[slot] = False
        return tail

    def _upload(self, rows):
        """The step table -> the fixed device tensor, through pinned staging on the current stream."""
        if not self._stage:
            self.tab.copy_(torch.tensor(rows, dtype=torch.int32))
            return
        buf = self._stage[self._stage_i]
        self._stage_i = (self._stage_i + 1) % len(self._stage)
        if buf[1] is not None:
            buf[1].synchronize()                 # its previous copy has completed (long ago, as a rule)
        else:
            buf[1] = torch.cuda.Event()
        buf[0].copy_(torch.tensor(rows, dtype=torch.int32))
        self.tab.copy_(buf[0], non_blocking=True)
        buf[1].record()

    @torch.no_grad()
    def push(self, chunk, hops):
        S, M, m = self.S, self.M, self.m
        hops = [int(h) for h in hops]
        if len(hops) != M:
            raise ValueError("hops must have one entry per slot (%d), got %d" % (M, len(hops)))
        if chunk.dim() != 2 or chunk.shape[0] != M:
            raise ValueError("chunk must be [%d, n*%d]" % (M, S))
        for i, h in enumerate(hops):
            if h < 0:
                raise ValueError("hops[%d] is negative" % i)
            if h and not self.is_open[i]:
                raise ValueError("slot %d is not open but hops[%d] = %d" % (i, i, h))
            if h * S > chunk.shape[1]:
                raise ValueError("chunk rows hold %d samples, slot %d needs hops[%d]*%d = %d" % (chunk.shape[1], i, i, S, h * S))
        steps = plan_steps(hops, self.fresh, self.F)
        lengths = [(h - (1 if f and h else 0)) * S for h, f in zip(hops, self.fresh)]
        for i, h in enumerate(hops):
            if h:
                self.fresh[i] = False
        out = torch.zeros((M, m.C, max(lengths)), device=self.dev)
        if not steps:
            return out, lengths
        chunk = chunk.to(self.dev, torch.float32)
        if chunk.stride(1) != 1 or (M > 1 and chunk.stride(0) < chunk.shape[1]):
            chunk = chunk.contiguous()
        cld = chunk.stride(0) if M > 1 else chunk.shape[1]       # rows of a wider tensor are read in place
        for frames, max_hops, rows in steps:
            st = ops._stream()
            self._upload(rows)
            lib.call("ctn_stream_load_ragged", chunk.data_ptr(), cld, chunk.shape[1] // S, self.x.data_ptr(), self.xld,
                     self.tab.data_ptr(), M, S, max_hops, st)
            if frames:                           # 0: only first hops that prime their carries
                self._run_step(frames)
                lib.call("ctn_stream_store_ragged", self.out.data_ptr(), out.data_ptr(), out.shape[2], self.tab.data_ptr(),
                         M, m.C, S, frames, st)
        return out, lengths

    def _run_step(self, frames):
        if not self.use_graph:
            return self._step(frames)
        if frames not in self._graphs:
            if frames not in self._seen:                 # one eager step of this maximum first (module load, allocator)
                self._seen.add(frames)
                return self._step(frames)
            torch.cuda.synchronize(self.dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):                    # records, does not run; the table is read at replay, not baked in
                self._step(frames)
            self._graphs[frames] = g
        self._graphs[frames].replay()

    def _step(self, frames):
        """One ragged step of at most `frames` frames per slot, by the table in `self.tab`; every carry updated in place."""
        m, M, st = self.m, self.M, ops._stream()
        g0, b0, tab = self._small[4], self._small[5], self.tab.data_ptr()
        lib.call("ctn_stream_front_ragged", self.x.data_ptr(), self.xld, self.Up.data_ptr(), g0.data_ptr(), b0.data_ptr(),
                 self.Wbp.data_ptr(), self.w.data_ptr(), self.y.data_ptr(), tab, M, m.N, m.L, m.B, frames, st)
        if self.cumulative:
            lib.call("ctn_stream_tcn_cumln_ragged", self.packed.data_ptr(), self.dil, self.nb, self.y.data_ptr(), self.state.data_ptr(),
                     self.cum.data_ptr(), tab, self.pos.data_ptr(), M, m.B, m.H, m.P, frames, self.F, st)
        else:
            lib.call("ctn_stream_tcn_cln_ragged", self.packed.data_ptr(), self.dil, self.nb, self.y.data_ptr(), self.state.data_ptr(),
                     tab, self.pos.data_ptr(), M, m.B, m.H, m.P, frames, self.F, st)
        lib.call("ctn_stream_back_ragged", self.y.data_ptr(), self.w.data_ptr(), self.Wmp.data_ptr(), self.Vp.data_ptr(),
                 self.fr.data_ptr(), self.out.data_ptr(), self.ola_tail.data_ptr(), self.x.data_ptr(), self.xld, tab,
                 M, m.N, m.L, m.B, m.C, frames, self.soft, st)


def plan_rate_push(rem, new, S):
    """(hops, rem'): a slot that carries `rem` < S model-rate samples and receives `new` more feeds (rem + new) // S whole hops to
    the pool and carries the rest (pure host code, no GPU)."""
    rem, new, S = int(rem), int(new), int(S)
    if not 0 <= rem < S or new < 0:
        raise ValueError("a remainder in 0..%d and a count >= 0 expected, got %d and %d" % (S - 1, rem, new))
    return (rem + new) // S, (rem + new) % S


def plan_rate_close(fed_hops, rem, S, L):
    """(hops, pad): the last push of a stream of n = fed_hops * S + rem model-rate samples (rem may be S or more here: it holds the
    resampler's flush): `pad` zeros take it to max(L, the next multiple of S), fed as `hops` hops.  (0, 0) for an empty stream."""
    fed_hops, rem, S, L = int(fed_hops), int(rem), int(S), int(L)
    n = fed_hops * S + rem
    if n == 0:
        return 0, 0
    total = max(L, -(-n // S) * S)
    return (total - fed_hops * S) // S, total - n


class ResamplingStreamPool:
    """`FusedStreamPool` for clients at another sample rate: samples in at `input_rate`, separated audio out at `output_rate`
    (None: at the model's rate, no output stage), resampled on the device by two `resample.StreamResampler`s.

        pool = ResamplingStreamPool(model, slots=32, max_chunk_frames=16, input_rate=16000, output_rate=16000)
        s = pool.open()
        out, lengths = pool.push(chunk, counts)     # chunk [slots, n]: slot m delivers counts[m] SAMPLES at input_rate, any values
        tail = pool.close(s)                        # [C, n]: everything not yet delivered; the slot is free again
    out is [slots, C, max(lengths)] with zeros beyond lengths[m].

    A push, in order: the input resampler writes every slot's new model-rate samples behind the slot's remainder (fewer than S
    samples) in a device staging buffer; (remainder + new) // S whole hops per slot go to the pool; the leftover moves to the front of
    the staging rows; the pool's [slots, C, .] output goes through the output resampler (slots * C rows, groups = C).  No launch or
    copy is per slot, nothing is read back and nothing synchronises: all counting is host arithmetic (`plan_rate_push`,
    `resample.plan_stream_resample`, `plan_steps`).  `close` flushes the input resampler, zero-pads what is left to a whole hop (and
    the stream to L samples if it was shorter), pushes it, takes the pool's tail, cuts the model-rate result to
    n8 = ceil(N * model_rate / input_rate) samples, feeds and flushes the output resampler.  A stream of 0 samples gives [C, 0].

    For every slot, all `push` outputs plus the `close` tail are BITWISE what this offline pipeline gives for the slot's signal x:
        x8 = resample(x, input_rate, model_rate)
        x8 zero-padded to max(L, the next multiple of S), through FusedStreamingSeparator(model, batch=1) as one push plus flush()
        the result cut to len(x8), then resample(., model_rate, output_rate)
    whatever the cuts and whatever the other slots do (for zeros != 32 read `resample` as the same sum with that filter).
    `zeros` sets the resamplers' look-ahead (see StreamResampler); ``graph`` and ``cumulative`` are the pool's: the resample launches
    stay outside its graphs.
    """

    def __init__(self, model, slots=1, max_chunk_frames=16, model_rate=8000, input_rate=8000, output_rate=None, zeros=ZEROS, graph=False,
                 cumulative=False):
        from . import resample as rs
        check_fused_model(model, cumulative)                   # ValueError on a model / mode mismatch before anything is built
        rs.ratio(input_rate, model_rate)                       # ValueError on a bad rate before anything is built
        if output_rate is not None:
            rs.ratio(model_rate, output_rate)
        self.pool = pool = FusedStreamPool(model, slots, max_chunk_frames, graph, cumulative)
        self.M, self.S, self.L, self.C, self.dev = pool.M, pool.S, pool.L, model.C, pool.dev
        piece = pool.F * pool.S                                  # model-rate samples of one pool step
        self.in_rs = rs.StreamResampler(self.M, input_rate, model_rate, max(1, piece * int(input_rate) // int(model_rate)), zeros=zeros,
                                        device=self.dev)
        self.out_rs = None
        if output_rate is not None:
            self.out_rs = rs.StreamResampler(self.M * self.C, model_rate, output_rate, piece, zeros=zeros, groups=self.C, device=self.dev)
        self.rem, self.fed = [0] * self.M, [0] * self.M          # carried model-rate samples; hops fed to the pool so far
        self.stage = torch.zeros((self.M, 4 * piece + 2 * self.S), device=self.dev)

    @property
    def is_open(self):
        return self.pool.is_open

    def _room(self, width):
        """Staging rows of at least `width` samples; the carried remainders move along."""
        if width > self.stage.shape[1]:
            grown = torch.zeros((self.M, 2 * width), device=self.dev)
            grown[:, :self.S] = self.stage[:, :self.S]
            self.stage = grown

    def open(self, slot=None):
        slot = self.pool.open(slot)
        self.in_rs.open(slot)
        if self.out_rs is not None:
            self.out_rs.open(slot)
        self.rem[slot] = self.fed[slot] = 0
        return slot

    @torch.no_grad()
    def push(self, chunk, counts):
        M, S, C = self.M, self.S, self.C
        counts = self.in_rs._check_counts(counts)
        if not any(counts):
            return torch.zeros((M, C, 0), device=self.dev), [0] * M
        new = self.in_rs.plan(counts)
        plan = [plan_rate_push(r, n, S) for r, n in zip(self.rem, new)]
        hops = [h for h, _ in plan]
        self._room(max(r + n for r, n in zip(self.rem, new)) + S)
        self.in_rs.run(chunk, counts, self.stage, self.stage.shape[1], self.rem, spare=[h * S for h in hops])
        if any(hops):
            out, lengths = self.pool.push(self.stage[:, :max(hops) * S], hops)
            # the leftover of every row to its front: row m from hops[m] * S on (the table's spare entry), one launch for all
            lib.call("ctn_stream_carry", self.stage.data_ptr(), self.stage.shape[1], M, self.in_rs.tab.data_ptr(), S - 1, ops._stream())
        else:
            out, lengths = torch.zeros((M, C, 0), device=self.dev), [0] * M
        for m, (h, r) in enumerate(plan):
            self.fed[m] += h
            self.rem[m] = r
        if self.out_rs is None:
            return out, lengths
        y, lengths = self.out_rs.push(out.view(M * C, out.shape[2]), lengths)
        return y.view(M, C, y.shape[1]), lengths

    @torch.no_grad()
    def close(self, slot):
        """Everything of the slot's stream not yet delivered, [C, n] at the output rate; the slot is free again."""
        slot = int(slot)
        if not 0 <= slot < self.M or not self.pool.is_open[slot]:
            raise ValueError("slot %r is not open" % (slot,))
        M, S, C = self.M, self.S, self.C
        none = [0] * M
        flush = self.in_rs.plan(none, (slot,))[slot]
        self._room(self.rem[slot] + flush + self.L + S)
        total_in = self.in_rs.n[slot]
        self.in_rs.run(None, none, self.stage, self.stage.shape[1], self.rem, final=(slot,))
        rem = self.rem[slot] + flush
        n8, fed = self.fed[slot] * S + rem, self.fed[slot]
        assert n8 == self.in_rs.out_total(total_in)
        hops, pad = plan_rate_close(fed, rem, S, self.L)
        self.rem[slot] = self.fed[slot] = 0
        if n8 == 0:
            self.pool.close(slot)
            if self.out_rs is not None:
                self.out_rs.close(slot)
            return torch.zeros((C, 0), device=self.dev)
        if pad:
            self.stage[slot, rem:rem + pad] = 0
        feed = list(none)
        feed[slot] = hops
        out, lengths = self.pool.push(self.stage[:, :hops * S], feed)
        rest = torch.cat([out[slot, :, :lengths[slot]], self.pool.close(slot)], dim=1)
        rest = rest[:, :n8 - max(fed - 1, 0) * S]                # the model-rate result cut to n8 samples in all
        if self.out_rs is None:
            return rest.contiguous()
        buf = torch.zeros((M * C, rest.shape[1]), device=self.dev)
        buf[slot * C:(slot + 1) * C] = rest
        feed[slot] = rest.shape[1]
        y, lengths = self.out_rs.push(buf, feed)
        return torch.cat([y[slot * C:(slot + 1) * C, :lengths[slot]], self.out_rs.close(slot)], dim=1)
