"""Chunked (streaming) inference for the causal / cLN variant.

With ``causal=True, norm_type='cLN'`` every layer of the reference is frame-local (1x1 convs, PReLU, the
per-frame cLN of src/conv_tasnet.py:313-335 -- which is NOT cumulative) except the depthwise conv,
which looks (P-1)*dilation frames into the past (src/conv_tasnet.py:182,253-256,281-295).  So a stream can be
separated chunk by chunk, exactly, by carrying per block the last (P-1)*dilation frames of the depthwise input,
plus the encoder's L-S input samples and the decoder's L-S overlap-add samples.  Total left context is
R*(P-1)*(2^X-1) frames (2040 at the paper config) -- but it is state, not recomputation.

All arithmetic runs through the same HIP entry points as training (ops.py); torch only slices / concatenates.
"""
import torch

from . import ops
from ._lib import lib


def _padded(t, K):
    """[M,Ch,K] (any stride) -> contiguous zero-padded [M,Ch,Kp]."""
    Kp = ops.padded_frames(K)
    out = t.new_zeros(t.shape[:-1] + (Kp,))
    out[..., :K] = t
    return out


class StreamingSeparator:
    """Stateful chunk-wise separation with a causal ConvTasNet.

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
        if not model.causal or model.norm_type != "cLN":
            raise ValueError("streaming needs the causal cLN variant (gLN statistics span the whole utterance)")
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
            self._graphs = {}            # chunk length -> (graph, static chunk, static output)
            self._seen = {}              # chunk length -> eager steady-state chunks so far
        else:
            self.in_tail.zero_()
            self.ola_tail.zero_()
            for h in self.hist:
                h.zero_()
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
                n1, _, _ = ops.cln_fwd(h, blk.net[2].gamma, blk.net[2].beta, blk.net[1].weight, K)
                cat = torch.cat([self.hist[i], n1[..., :K]], dim=2)          # [M, H, halo + K]
                self.hist[i].copy_(cat[..., cat.shape[2] - halo:])
                Kc = halo + K
                z, _ = ops.dw_fwd(_padded(cat, Kc), ds.net[0].weight, Kc, blk.dilation, True)
                z = _padded(z[..., halo:Kc], K)
                n2, _, _ = ops.cln_fwd(z, ds.norm().gamma, ds.norm().beta, ds.prelu().weight, K)
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


class FusedStreamingSeparator:
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

    Out of scope: per-stream reset and streams joining mid-flight (the first chunk has one frame fewer, for every stream of the batch
    at once), gLN / non-causal models (ValueError), training (no autograd).
    """

    def __init__(self, model, batch=1, max_chunk_frames=64, graph=False):
        import ctypes
        if not model.causal or model.norm_type != "cLN":
            raise ValueError("streaming needs the causal cLN variant (gLN statistics span the whole utterance)")
        if max_chunk_frames < 1 or batch < 1:
            raise ValueError("batch and max_chunk_frames must be positive")
        m = self.m = model
        self.M, self.F = int(batch), int(max_chunk_frames)
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
        self.first = True
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

    def reset(self):
        """Back to the start of a stream (every stream of the batch); packed weights and captured graphs stay valid."""
        lib.call("ctn_stream_reset", self.state.data_ptr(), self.state_bytes, ops._stream())
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

    def _step(self, frames):
        """`frames` frames of the sample buffer through the network; every carry updated in place.  Returns a view of the output buffer."""
        m, M, st = self.m, self.M, ops._stream()
        g0, b0 = self._small[4], self._small[5]
        lib.call("ctn_stream_front", self.x.data_ptr(), self.xld, self.Up.data_ptr(), g0.data_ptr(), b0.data_ptr(), self.Wbp.data_ptr(),
                 self.w.data_ptr(), self.y.data_ptr(), M, m.N, m.L, m.B, frames, st)
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
