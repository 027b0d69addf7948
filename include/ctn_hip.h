/* libctn_hip.so -- C ABI of the MI355X (gfx950) Conv-TasNet hot path.
 *
 * The reference (OfekCohen1/Conv-TasNet) has no FFI of its own: its hot path is torch.nn
 * modules.  This header is the boundary a maintainer binds instead (ctypes
 * stub in INTEGRATION.md); each entry point names the reference code it replaces, paths
 * relative to the reference root.
 *
 * Conventions
 *  - plain pointers + sizes only; every pointer is DEVICE memory unless marked "host".
 *  - the caller owns and allocates every buffer, workspaces included; the library never
 *    allocates, frees or retains a pointer, and never synchronises the device.
 *  - every launch goes to `stream` (a hipStream_t passed as void*; NULL = default stream).
 *  - return 0 on success, <0 on error (CTN_ERR_*); ctn_last_error() gives the message
 *    for the calling thread.  Nothing throws across the boundary.
 *  - activations are fp32 [M, Ch, Kp], frames fastest; Kp = ctn_padded_frames(K); columns
 *    k in [K, Kp) hold exact zeros in every activation / gradient tensor (every kernel keeps
 *    that invariant).  Channel counts must be multiples of 4; tensors 16-byte aligned.
 *  - all reductions have a fixed order: same inputs -> bitwise same outputs.
 */
#ifndef CTN_HIP_H
#define CTN_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTN_OK 0
#define CTN_ERR_ARG (-1)
#define CTN_ERR_LAUNCH (-2)
#define CTN_ERR_WORKSPACE (-3)
#define CTN_AMAX_SLOTS 64      /* words per utterance of a tracked-maximum array (h3 arithmetic, below) */

int ctn_version(void);
const char* ctn_last_error(void);
int ctn_padded_frames(int K);               /* K rounded up to a multiple of 64 */
/* Orders two HIP streams of the current device: work enqueued on `from` so far completes before work enqueued on `to`
 * after the call.  Device-scope event (no timing, no system-scope fence): the cheap form of
 * torch.cuda.Stream.wait_stream for the weight-gradient stream of the backward pass. */
int ctn_stream_order(void* from, void* to);

/* ---- 1x1 convolutions = GEMMs on the matrix cores, fp32-faithful ------------------------
 * replaces nn.Conv1d(*, *, 1, bias=False): src/conv_tasnet.py:174 (bottleneck), :191 (mask),
 * :223 and :262 (TemporalBlock), and the Linear of the decoder (:128,:143); autograd's
 * convolution_backward for the same layers. */

/* Out[m] = op(W) . f(X[m])  (+ residual[m]),   X:[M,Cn,Kp]  Out:[M,R,Kp]
 *   trans_w = 0: W is [R,Cn] (forward);  trans_w = 1: W is [Cn,R] (input gradient, or forward on a transposed copy:
 *     the fast form of the fp32-MFMA arithmetic -- ctn_transpose_batch);  trans_w = 2: W is a block of pre-split bf16 pieces
 *     from ctn_split_b3_batch (b6 arithmetic, R >= 64: the fast form there).
 *   pro_part != NULL: f(x)[i,k] = gamma[i]*((prelu(x,alpha)-mean_m)*rstd_m)+beta[i]
 *     for k < K, 0 otherwise; (mean_m, rstd_m) are finalised from the [M, pro_nparts, 2] fp64
 *     (sum, sum of squares) partials of prelu(x) -- global LayerNorm, src/conv_tasnet.py:358-360 --
 *     and written to pro_ms_out [M,2] when that is non-NULL.
 *   residual != NULL: TemporalBlock's "out + residual" (src/conv_tasnet.py:243).
 *   epi_part != NULL: also emits the partials of prelu(Out, epi_alpha) for the NEXT gLN,
 *     layout [M, ctn_pw_stats_parts(M,R,Kp), 2] fp64.
 *   relu_out != 0: Out = relu(.)  (encoder, src/conv_tasnet.py:120). */
int ctn_pw_gemm(const float* W, const float* X, float* Out, int M, int R, int Cn, int K, int Kp, int trans_w,
                const double* pro_part, int pro_nparts, const float* pro_gamma, const float* pro_beta,
                const float* pro_alpha, float* pro_ms_out,
                const float* residual, const float* epi_alpha, double* epi_part, int relu_out, void* stream);
int ctn_pw_stats_parts(int M, int R, int Kp);

/* dst[i] = src[i]^T for n equally shaped [rows, cols] fp32 matrices (HOST arrays of device pointers): the forward pass
 * keeps a [I, O] copy of every 1x1 weight [O, I] so that ctn_pw_gemm(trans_w = 1) -- 16-byte row writes into LDS, no
 * transposing scatter -- serves forward and input gradient alike (src/conv_tasnet.py:223,262). */
int ctn_transpose_batch(const void* const* src, void* const* dst, int n, int rows, int cols, void* stream);

/* dN[m] = W^T . dOut[m]   (W:[Cn,R] as stored by the forward layer, dOut:[M,Cn,Kp], dN:[M,R,Kp])
 * and, fused, the two sums gLN backward needs per utterance, as partials
 * sums_part [M, ctn_pw_stats_parts(M,R,Kp), 2] fp64:  S1 = sum gamma*dN,  S2 = sum gamma*dN*xhat,
 * xhat = (prelu(y,alpha)-ms[m][0])*ms[m][1],  y:[M,R,Kp] the pre-activation input of that norm. */
int ctn_pw_dgrad_gln(const float* W, const float* dOut, float* dN, int M, int R, int Cn, int K, int Kp,
                     const float* y, const float* gamma, const float* alpha, const float* ms, double* sums_part,
                     void* stream);

/* dW[R,Cn] = sum_{m,k} dOut[m,r,k] * f(X[m,c,k]);  f as above when pro_ms ([M,2]) != NULL.
 * workspace: ctn_pw_wgrad_workspace() bytes of split-K slabs, summed in a fixed order. */
int ctn_pw_wgrad(const float* dOut, const float* X, float* dW, int M, int R, int Cn, int K, int Kp,
                 const float* pro_gamma, const float* pro_beta, const float* pro_alpha, const float* pro_ms,
                 void* workspace, size_t workspace_bytes, void* stream);
size_t ctn_pw_wgrad_workspace(int M, int R, int Cn, int Kp);
/* Library switches (process-global; the library is driven by ONE host thread at a time: set them from that thread, between
 * steps -- workspace sizes and statistics layouts depend on them).  Keys: "arith" (below); "b3_tile" / "b3_tile_k3" 0|1|2|3 =
 * 128x128 / 128x64 / 256x64 / 256x64 on 8 waves: tile of the split forward / input-gradient kernels (the prologue + residual form has its
 * own); "b3_wgrad_blocks", "wgrad_blocks": target workgroups per weight-gradient launch (split-bf16 / fp32 MFMA);
 * "pw_tile" -1|0..3: tile of the fp32-MFMA forward kernel (also CTN_PW_TILE); "cln_fr" 16|32: frames per workgroup of the channel-wise LayerNorm backward
 * kernel (16: three 256-thread workgroups per CU; changes ctn_cln_bwd_blocks()); "cln_lean" 0|1 (default 1): ctn_cln_bwd at 512 channels with PReLU and without `add` /
 * `relu_ref` runs a kernel specialised for that form (same bits, 11 % faster alone); "cln_fuse" 0|1|2 (default 2): 1 = the
 * composite cLN stacks run the second norm's backward inside the input-gradient GEMM's epilogue and the depthwise backward
 * (ctn_pw_dgrad_cln / ctn_cln_bwd_frame / ctn_dw_bwd_cln) instead of as a ctn_cln_bwd pass; 2 = also the first norm's forward
 * inside the first 1x1 conv's epilogue and the depthwise kernel's prologue (ctn_pw_gemm_cln / ctn_cln_stats_frame / ctn_dw_fwd_cln:
 * n1s is then neither written nor read; set it between steps, forward and backward under the same value; CTN_CLN_FUSE=0|1|2 at first
 * use); ctn_cln_fuse() reads it;
 * "bwd_events" 0|1|2 (default 0 = gLN stacks 1, cLN stacks 2; CTN_BWD_EVENTS=1|2 at first use): forks of the weight-gradient stream
 * per block of the composite backward passes -- 2: dW2 behind B1 and dW1 behind the norm backward; 1: one fork behind B5 (dW1 and the
 * sums of that block, then dW2 of the next block, which needs only that B5's output); same gradients bit for bit; "gln_fuse" 0|1
 * (default 0; CTN_GLN_FUSE at first use; ctn_gln_fuse() reads it): 1 = the composite gLN stacks run without the gLN-1' / PReLU-1' pass
 * (ctn_pw_dgrad_gln2 + ctn_dw_bwd_gln2 instead of ctn_pw_dgrad_gln + ctn_dw_bwd + ctn_gln_prelu_bwd): three tensor passes of 20 less, same
 * gradients to fp32 rounding -- and 1.7 % SLOWER in the step (profiles/README.md r04_m): a tested option.  Defaults are the
 * measured best. */
int ctn_tune(const char* key, int value);
int ctn_cln_fuse(void);
int ctn_gln_fuse(void);
/* Arithmetic of the 1x1-convolution GEMMs (ctn_pw_gemm, ctn_pw_dgrad_gln, ctn_pw_wgrad and the composites over them):
 *   3 = "h3" (default): the GEMMs of the composite stacks (ctn_tcn_*) run on the ctn_*_h3 entry points below -- two fp16 pieces
 *       per fp32 operand under a tracked power-of-two scale, three f16 MFMAs, fp32 accumulation; every other GEMM as b6;
 *   2 = "b6": every fp32 operand is split EXACTLY into three bf16 pieces (a = a0 + a1 + a2, round-to-nearest-even)
 *       and a.b is formed from the six piece-products of weight >= 2^-17 on v_mfma_f32_32x32x16_bf16 with fp32 accumulation;
 *       the dropped terms are <= 2^-23 |a.b| -- one fp32 rounding of the product.  Measured against fp64 the error of every
 *       GEMM form is that of the fp32 MFMA (3.4e-7 vs 4.0e-7 of sum |a||b|, profiles/r03_a_b6_check.txt);
 *   0 = fp32 MFMA (v_mfma_f32_32x32x2_f32), bit-exact fp32 FMA chains;
 *   (1 was round 2's two-piece bf16 "b3", ~16-bit products: removed -- h3 costs the same three MFMAs at reference precision.)
 * Selected by CTN_GEMM_ARITH=h3|b6|fp32 at first use or ctn_tune("arith", 3|2|0) between steps; layers with fewer than 64
 * output rows (and weight gradients with a side below 32) always use the fp32-MFMA kernels. */
int ctn_gemm_arith(void);
/* b6 arithmetic (also the plain entry points under h3): the weight operand pre-split once per step.  dst[i] receives the bf16 pieces of the GEMM operand
 * A [R, Cn] (rows = output channels of THAT GEMM, Cn = its contraction) in MFMA fragment order, zero-filled to multiples
 * of 32: ctn_split_b3_bytes(R, Cn) bytes each (three pieces), 16-byte aligned.  k_major = 0: src[i] is
 * stored [R, Cn] (forward layers); k_major = 1: src[i] is stored [Cn, R] and used transposed (input gradients of the same
 * layers).  HOST arrays of device pointers, any n.  ctn_pw_gemm(trans_w = 2) and ctn_pw_dgrad_gln_planes take such a block as
 * W: no conversion work and no LDS traffic for the weights inside the GEMM; results are bitwise those of the fp32-weight forms. */
size_t ctn_split_b3_bytes(int R, int Cn);
int ctn_split_b3_batch(const void* const* src, void* const* dst, int n, int R, int Cn, int k_major, void* stream);
int ctn_pw_dgrad_gln_planes(const void* Wp, const float* dOut, float* dN, int M, int R, int Cn, int K, int Kp,
                            const float* y, const float* gamma, const float* alpha, const float* ms, double* sums_part,
                            void* stream);

/* ---- "h3" arithmetic: fp32-faithful products from TWO fp16 pieces per operand (three f16 MFMAs instead of b6's six) ------
 * replaces the same fp32 nn.Conv1d(*, *, 1) layers (src/conv_tasnet.py:223,262) inside the composite stacks.
 *   a s = a0 + a1 + r,  a0 = fp16_rne(a s), a1 = fp16_rne(a s - a0):  two 11-bit significands + the sign of a1 hold 22-23 bits,
 *   |a1| <= 2^-11 |a s|, |r| <= 2^-23 |a s|;   a.b ~= (a1.b0 + a0.b1 + a0.b0) / (s_a s_b)  on v_mfma_f32_32x32x16_f16, fp32
 *   accumulation; dropped per product: a1.b1 + r_a.b + a.r_b, <= 8 * 2^-24 |a.b| in the worst case (4.8e-7), 1.2 * 2^-24 rms (b6
 *   drops 2 * 2^-24).  A single product is thus NOT better than an fp32 one; the GEMM is, because the f16 MFMA rounds its fp32
 *   accumulator once per 16-deep step where the fp32 MFMA rounds it every 2-deep step (measured rms error of every form 1.3e-8
 *   of sum |a||b| against 2.8e-8, max 1.5e-7 against 3.8e-7).  Coherent worst case (all operands positive, each just below a
 *   rounding midpoint): 2.4e-7 .. 4.8e-7 of sum |a||b|, tested (tests/test_gpu_h3.py).
 * fp16 has 5 exponent bits, so every operand is brought into range by an exact power-of-two scale s derived from a bound on
 * its magnitude: the weight's own maximum (computed by ctn_split_h3_batch), and for activations the per-utterance maximum
 * max |X[m]| TRACKED BY THE KERNEL THAT PRODUCED X -- `amax` arrays: [M][CTN_AMAX_SLOTS] unsigned, bit patterns of non-negative
 * floats; a producer workgroup merges its maximum into one of an utterance's slots with an atomic max (exact, order-free: results
 * stay bitwise reproducible; 64 slots because 1000 atomics on one address cost a producer 5-9 us), a consumer takes the maximum
 * over the slots; the caller zeroes the array before the producer runs.  Producers: ctn_absmax_rows (any tensor), ctn_pw_gemm_h3 (residual epilogue, out_amax), ctn_dw_fwd and
 * ctn_gln_prelu_bwd (amax_out).  With an operand prologue the scale comes from the bound
 * max|gamma| * rstd * (max(1,|alpha|) * amax + |mean|) + max|beta|  (pro_gbmax = {max|gamma|, max|beta|}: ctn_absmax_batch).
 * Scaled values stay below 2^15 (fp16 holds 65504).  The bounds above hold for every element down to 2^-27 of its operand's bound
 * (the low piece is stored times 2^11 and accumulated separately, so it stays a normal fp16 number); smaller elements lose RELATIVE
 * precision gracefully (absolute error <= 2^-50 of the bound).  The scale is per UTTERANCE (per weight matrix): an element far below
 * its utterance's maximum is covered by that window, not by a scale of its own.  Same tiles, statistics
 * layouts (ctn_pw_stats_parts of the split arithmetics), epilogues and fixed-order reductions as the plain entry points.
 * These entry points do not depend on ctn_tune("arith"); R >= 64 (weight gradient: both sides >= 32). */
size_t ctn_split_h3_bytes(int R, int Cn);
int ctn_split_h3_batch(const void* const* src, void* const* dst, int n, int R, int Cn, int k_major, void* stream);
/* dst[i][0] = bit pattern of max |src[i][0 .. len)|  (HOST arrays of device pointers; dst[i]: 4 bytes) */
int ctn_absmax_batch(const void* const* src, void* const* dst, int n, int len, void* stream);
/* slots of amax[m] <- bits of max |x[m][0 .. n)|,  x: [M, n] fp32, n % 4 == 0, amax: [M][CTN_AMAX_SLOTS] */
int ctn_absmax_rows(const float* x, int M, long long n, unsigned* amax, void* stream);
/* ctn_pw_gemm(trans_w = 2) on h3 pieces.  x_amax: maximum of X as stored; pro_gbmax with the prologue; out_amax
 * (optional, with residual): receives the maximum of Out. */
int ctn_pw_gemm_h3(const void* Wp, const float* X, float* Out, int M, int R, int Cn, int K, int Kp,
                   const double* pro_part, int pro_nparts, const float* pro_gamma, const float* pro_beta,
                   const float* pro_alpha, float* pro_ms_out, const float* residual, const float* epi_alpha, double* epi_part,
                   const unsigned* x_amax, const float* pro_gbmax, unsigned* out_amax, void* stream);
int ctn_pw_dgrad_gln_h3(const void* Wp, const float* dOut, float* dN, int M, int R, int Cn, int K, int Kp,
                        const float* y, const float* gamma, const float* alpha, const float* ms, double* sums_part,
                        const unsigned* g_amax, void* stream);
int ctn_pw_wgrad_h3(const float* dOut, const float* X, float* dW, int M, int R, int Cn, int K, int Kp,
                    const float* pro_gamma, const float* pro_beta, const float* pro_alpha, const float* pro_ms,
                    const unsigned* g_amax, const unsigned* x_amax, const float* pro_gbmax,
                    void* workspace, size_t workspace_bytes, void* stream);
size_t ctn_pw_wgrad_h3_workspace(int M, int R, int Cn, int Kp);

/* ---- depthwise dilated conv (+ fused PReLU / gLN) ---------------------------------------
 * replaces DepthwiseSeparableConv.net[0] (+Chomp1d), src/conv_tasnet.py:253-256,281-295, with the
 * PReLU (:224,:259) and GlobalLayerNorm (:225,:260,:338-361) on either side fused in. */

/* Z[m,h,k] = sum_j D[h,j] * n[m,h,k + j*dilation - pad_left],  zeros outside [0,K);
 *   pad_left = (P-1)*dilation/2 (non-causal "same") or (P-1)*dilation (causal, = pad + Chomp1d).
 *   pro_part != NULL: n = gLN(prelu(Y)) as in ctn_pw_gemm; else n = Y.
 *   epi_part != NULL: partials of prelu(Z, epi_alpha), layout [M, H, 2] fp64;
 *   amax_out != NULL (with epi_part): [M][CTN_AMAX_SLOTS], receives max |Z[m]| -- see the h3 section. */
int ctn_dw_fwd(const float* Y, float* Z, const float* D, int M, int H, int K, int Kp, int P, int dilation, int causal,
               const double* pro_part, int pro_nparts, const float* pro_gamma, const float* pro_beta,
               const float* pro_alpha, float* pro_ms_out, const float* epi_alpha, double* epi_part, unsigned* amax_out,
               void* stream);

/* Backward of the above.  fused = 1 walks  gLN2 <- PReLU2 <- depthwise <- (gLN1 output)  in one pass:
 *   in : dN2 (grad of gLN2's output), Dz (= Z of the forward), Y1 (= Y of the forward),
 *        (g1,b1,a1,ms1) / (g2,a2,ms2) of the two norms, sums2_part from ctn_pw_dgrad_gln
 *   out: dN1 (grad of gLN1's output), sums1_part [M,H,2] fp64 (S1,S2 for gLN1's backward) and
 *        pc [F, M, H] per-(utterance, channel) partials, F = ctn_dw_bwd_rows(P, fused):
 *        rows 0..P-1 dD taps; fused adds P: dgamma2, P+1: dbeta2, P+2: dgamma1, P+3: dbeta1, P+4: dalpha2.
 * fused = 0: dN2 = dZ, Y1 = the forward input; outputs dN1 = dY and pc rows 0..P-1.
 * fused takes 0 and 1 only.  The other two forms have entry points of their own, and this one refuses their numbers with
 * CTN_ERR_ARG and a message that names the one to call: 2 = the channel-wise LayerNorm form, ctn_dw_bwd_cln; 3 = the gLN form
 * with the first norm's backward applied, ctn_dw_bwd_gln2 (both below).  ctn_dw_bwd_rows still answers for 0..3. */
int ctn_dw_bwd(const float* dN2, const float* Dz, const float* Y1, float* dN1, const float* D,
               int M, int H, int K, int Kp, int P, int dilation, int causal, int fused,
               const float* g1, const float* b1, const float* a1, const float* ms1,
               const float* g2, const float* a2, const float* ms2,
               const double* sums2_part, int sums2_nparts, float* pc, double* sums1_part, void* stream);
int ctn_dw_bwd_rows(int P, int fused);
/* Fixed-order finish of the fused backward's partials: pc [P+5,M,H] -> dD [H,P] (the depthwise weight's layout),
 * dgamma2, dbeta2, dgamma1, dbeta1 [H] and dalpha2 [1]; when dalpha1_part (the [n_dalpha1] per-row partials of
 * ctn_gln_prelu_bwd) is non-NULL the same launch also sums dalpha1 [1].  Destinations may be views into a flat
 * gradient buffer. */
int ctn_dw_bwd_finalize(const float* pc, int P, int M, int H, float* dD, float* dgamma2, float* dbeta2,
                        float* dgamma1, float* dbeta1, float* dalpha2, const float* dalpha1_part, int n_dalpha1,
                        float* dalpha1, void* stream);

/* gLN block WITHOUT the gLN-1' / PReLU-1' pass (round 4; GlobalLayerNorm backward of src/conv_tasnet.py:338-361 inside a TemporalBlock,
 * :223-225).  The first norm's backward needs S1' = sum gamma1 dN1 and S2' = sum gamma1 dN1 xhat1 over the utterance, dN1 being the
 * depthwise conv's input gradient.  The conv's adjoint moves both sums onto its OUTPUT gradient dd:
 *     S1' = sum_{c,k} dd[c,k] gamma1[c] V[c,k],   S2' = sum_{c,k} dd[c,k] (d[c,k] - beta1[c] V[c,k])
 * (d = the forward depthwise output = dw(gamma1 xhat1 + beta1), V[c,k] = sum of the taps of frame k that stay inside [0, K)), and
 * dd = prelu'(d) rstd2 (gamma2 dN2 - c1 - xhat2 c2) is affine in the second norm's (c1, c2) -- so six more per-utterance sums of
 * quantities that the second 1x1 conv's input-gradient GEMM already holds in its epilogue give S1', S2' BEFORE the depthwise
 * backward runs:   ctn_pw_dgrad_gln2 = ctn_pw_dgrad_gln with sums_part [M, ctn_pw_stats_parts(M,R,Kp), 8]
 *     (S1, S2, sum u t g1V, sum u g1V, sum u xh2 g1V, sum u t e, sum u e, sum u xh2 e;  u = prelu'(d), t = gamma2 dN, g1V = gamma1 V,
 *      e = d - beta1 V; W / w_form as ctn_pw_dgrad_cln; gamma1, beta1 [R], D [R,P], P, dilation, causal: the depthwise conv),
 * and ctn_dw_bwd_gln2 = ctn_dw_bwd(fused = 1) that applies the first norm's backward to its result on the fly: it writes
 *     dY1 = rstd1 (gamma1 dN1 - S1'/n - xhat1 S2'/n) prelu'(Y1)   instead of dN1,
 * the dalpha1 partials as row P+5 of pc [P+6, M, H] (ctn_dw_bwd_rows(P, 3); finish with ctn_dw_bwd_finalize, dalpha1_part = that
 * row) and, with amax_out != NULL, max |dY1[m]| (h3 section).  ctn_gln_prelu_bwd (three tensor passes) is not needed then. */
int ctn_pw_dgrad_gln2(const void* W, int w_form, const float* dOut, float* dN, int M, int R, int Cn, int K, int Kp,
                      const float* y, const float* gamma, const float* alpha, const float* ms,
                      const float* gamma1, const float* beta1, const float* D, int P, int dilation, int causal,
                      double* sums_part, const unsigned* g_amax, void* stream);
int ctn_dw_bwd_gln2(const float* dN2, const float* Dz, const float* Y1, float* dY1, const float* D,
                    int M, int H, int K, int Kp, int P, int dilation, int causal,
                    const float* g1, const float* b1, const float* a1, const float* ms1,
                    const float* g2, const float* a2, const float* ms2,
                    const double* sums2_part, int sums2_nparts, float* pc, unsigned* amax_out, void* stream);

/* Fixed-order finish of the UN-fused ctn_dw_bwd's tap partials: pc [P, M, H] -> dD [H, P] (the depthwise weight's layout). */
int ctn_dw_bwd_taps(const float* pc, int P, int M, int H, float* dD, void* stream);

/* cLN form of the backward (round 4; ChannelwiseLayerNorm, src/conv_tasnet.py:313-335, on the causal config's blocks :257-266):
 * walks  cLN2 <- PReLU2 <- depthwise  in one pass, i.e. the second norm's whole backward rides in the depthwise kernel:
 *   in : dN2 (grad of cLN2's output, from ctn_pw_dgrad_cln), Dz (= Z of the forward = cLN2's input), X1 (= the forward's input =
 *        cLN1's output), gamma2 / alpha2, fc [M][4][Kp] per-frame constants from ctn_cln_bwd_frame;
 *        g1 != NULL: the first norm's output was never stored -- X1 is its INPUT (the first 1x1 conv's output) and the kernel recomputes
 *        cLN1(prelu(X1, a1)) from (g1, b1, a1) and the per-frame statistics mean1, rstd1 [M,Kp]; else pass NULL for all five
 *   out: dN1 (grad of X1) and pc [P+3, M, H]: rows 0..P-1 dD taps, P: dgamma2, P+1: dbeta2, P+2: dalpha2 partials
 *        (ctn_dw_bwd_rows(P, 2) rows), finished in fixed order by ctn_dw_bwd_cln_finalize: dD [H,P], dgamma2 / dbeta2 [H], dalpha2 [1]. */
int ctn_dw_bwd_cln(const float* dN2, const float* Dz, const float* X1, float* dN1, const float* D,
                   int M, int H, int K, int Kp, int P, int dilation, int causal,
                   const float* g2, const float* a2, const float* fc,
                   const float* g1, const float* b1, const float* a1, const float* mean1, const float* rstd1,
                   float* pc, void* stream);
int ctn_dw_bwd_cln_finalize(const float* pc, int P, int M, int H, float* dD, float* dgamma2, float* dbeta2, float* dalpha2,
                            void* stream);

/* dY = rstd*(gamma*dN - S1/n - xhat*S2/n) * prelu'(Y);  dalpha_part [M*H] = per-row sum over Y<0 of (..)*Y.
 * Backward of  gLN(prelu(Y)), src/conv_tasnet.py:224-225.  dY may alias dN.
 * amax_out != NULL: [M][CTN_AMAX_SLOTS], receives max |dY[m]| -- see the h3 section. */
int ctn_gln_prelu_bwd(const float* dN, const float* Y, float* dY, int M, int H, int K, int Kp,
                      const float* gamma, const float* alpha, const float* ms, const double* sums_part, int nparts,
                      float* dalpha_part, unsigned* amax_out, void* stream);

/* First pass of the STAND-ALONE gLN(prelu(Y)) backward (GlobalLayerNorm used as a module of its own,
 * src/conv_tasnet.py:338-361; inside a TemporalBlock these sums come out of the GEMM / depthwise epilogues):
 * sums_part [M, H, 2] fp64 per-row (S1 = sum gamma*dN, S2 = sum gamma*dN*xhat) for ctn_gln_prelu_bwd, and
 * pc [2, M, H]: row 0 the dgamma partials (sum dN*xhat), row 1 the dbeta partials (sum dN) -> ctn_reduce_mid. */
int ctn_gln_bwd_sums(const float* dN, const float* Y, int M, int H, int K, int Kp, const float* gamma, const float* alpha,
                     const float* ms, double* sums_part, float* pc, void* stream);

/* ---- composite: the whole stack of gLN TemporalBlocks in one call ---------------------------------
 * replaces `temporal_conv_net = nn.Sequential(*repeats)`, src/conv_tasnet.py:176-186, i.e. nblocks = X*R
 * TemporalBlock.forward calls (:233-243) and their autograd backward.  The host side of a block (3 launches forward,
 * 8 backward) is issued from C++ in exactly the order of the per-kernel entry points above, so results are bitwise
 * those of calling them one by one.
 *   params  : HOST array [nblocks][9] of device pointers, per block in the order
 *             w1 [H,B], alpha1 [1], gamma1 [H], beta1 [H], D [H,P], alpha2 [1], gamma2 [H], beta2 [H], w2 [B,H]
 *             (src/conv_tasnet.py:223-225 and :253-262).   grads: the same layout, gradient destinations.
 *   dilation: HOST int [nblocks] (2^x, :170).
 *   x0 [M,B,Kp]: input of block 0.  Forward writes, backward reads (all device, caller-owned):
 *     xs  [nblocks][M,B,Kp]  block outputs (xs[nblocks-1] is the stack's output),
 *     h1s [nblocks][M,H,Kp]  first 1x1 outputs,  ds [nblocks][M,H,Kp] depthwise outputs,
 *     ms  [nblocks][2][M][2] (mean, rstd) of the two gLNs,
 *     amax [nblocks][2][M][CTN_AMAX_SLOTS] unsigned (h3 arithmetic; may be NULL otherwise): the tracked maxima of every block's input and of
 *          its depthwise output (see the h3 section); written by the forward pass (which zeroes it first), read by backward.
 *     save = 0 (inference): xs needs 2 slots, h1s / ds / ms one slot each (amax all nblocks); the output is xs[(nblocks-1) & 1].
 *   forward with side_stream != NULL and M >= 2: the batch runs as two half-batch chains on the two streams (utterances are
 *     independent; one half's HBM-bound phases overlap the other half's MFMA phases); same values bit for bit; on return `stream`
 *     is ordered after both.
 *   backward: dout [M,B,Kp] gradient of the stack's output; dxs [nblocks][M,B,Kp] receives the gradient of every
 *     block's input (dxs[0] = gradient w.r.t. x0); dn1s [nblocks][M,H,Kp] scratch (one slot per block, read by the
 *     weight-gradient stream).  side_stream != NULL: weight-gradient GEMMs and the fixed-order parameter-gradient sums go
 *     there (forked / joined with ctn_stream_order); on return `stream` is ordered after all of them -- unless flags bit 0
 *     is set: then the second stream is left un-joined, so that the caller can put more work behind this call's gradients
 *     (a data-parallel trainer: the all-reduce of this bucket of blocks) while `stream` already runs the next call; such a
 *     call needs a workspace of its own, and the caller joins the streams itself (ctn_stream_order) before the gradients
 *     are read on `stream`.  A stack may be run as several calls over consecutive block ranges (last blocks first).
 *   workspace: ctn_tcn_gln_{fwd,bwd}_workspace() bytes, 256-byte aligned. */
int ctn_tcn_gln_fwd(const void* const* params, const int* dilation, int nblocks, const float* x0,
                    float* xs, float* h1s, float* ds, float* ms, unsigned* amax, int save,
                    int M, int B, int H, int K, int Kp, int P, int causal,
                    void* workspace, size_t workspace_bytes, void* stream, void* side_stream);
size_t ctn_tcn_gln_fwd_workspace(int M, int B, int H, int Kp, int nblocks);
int ctn_tcn_gln_bwd(const void* const* params, void* const* grads, const int* dilation, int nblocks,
                    const float* x0, const float* xs, const float* h1s, const float* ds, const float* ms, const unsigned* amax,
                    const float* dout, float* dxs, float* dn1s,
                    int M, int B, int H, int K, int Kp, int P, int causal,
                    void* workspace, size_t workspace_bytes, void* stream, void* side_stream, int flags);
size_t ctn_tcn_gln_bwd_workspace(int M, int B, int H, int Kp, int P, int nblocks);

/* Measurement hook for the composite stacks (bench.py's roofline leg): ctn_probe_enable(1) makes every launch group issued
 * by ctn_tcn_*_fwd / _bwd on this thread's process record a HIP-event pair on the stream it is launched to;
 * ctn_probe_read waits for them, fills fam[i] (0..15: K1 K2 K3 B1 B2 B3 B4 B5 B6 finalize weight-prep cln_fwd cln_bwd taps last-slab-sums cln-frame-constants)
 * and us[i] (microseconds) in issue order for up to cap groups, returns the number recorded and ends the recording.
 * Off by default: no events, no overhead. */
int ctn_probe_enable(int on);
int ctn_probe_read(int* fam, float* us, int cap);

/* Schedule-perturbation hook for the tests of the two-stream ordering (tests/sched_harness.py); nothing in the package calls it.
 * ctn_delay enqueues a delay kernel on `stream`: one wave that stores nothing and polls the constant-rate wall clock until `micros`
 * microseconds have passed (0 <= micros <= 20000, CTN_ERR_ARG otherwise; a fixed cap on the polls ends it whatever the clock says).
 * ctn_delay_arm(group, micros) resets a counter of the launch groups that ctn_tcn_*_fwd / _bwd issue (the groups of the probe above)
 * and, with group >= 0, puts that delay ahead of the group-th one issued from now on, on the stream that group is launched to; the
 * hook then disarms itself, the count staying at group + 1.  group = -1 only counts, until ctn_delay_groups.  ctn_delay_groups returns
 * the count since the last arm and disarms (CTN_ERR_LAUNCH if the armed delay could not be launched).  Independent of
 * ctn_probe_enable: no probe record is added (while a recording is on, the delayed group's own record includes the delay: it is
 * enqueued behind that record's first event).  Disarmed (the default): one branch per launch group, no launch. */
int ctn_delay(void* stream, int micros);
int ctn_delay_arm(int group, int micros);
int ctn_delay_groups(void);

/* The same for a stack of cLN TemporalBlocks (norm_type = 'cLN': the causal BASELINE config), un-fused norms: per block
 * forward  1x1 -> cLN(PReLU) -> depthwise -> cLN(PReLU) -> 1x1 + residual,  backward the adjoint chain with the two weight
 * gradients on side_stream.  Saved by forward (slot per block): xs [nblocks][M,B,Kp]; h1s, n1s, ds, n2s [nblocks][M,H,Kp]
 * (1x1 output, first norm output, depthwise output, second norm output); st [nblocks][4][M,Kp] = mean1, rstd1, mean2, rstd2.
 * amax [nblocks][2][M][CTN_AMAX_SLOTS] (h3 arithmetic; may be NULL otherwise): tracked maxima of every block's input and of its
 * second norm's output, written by forward, read by backward.
 * save = 0: two x slots, one slot of everything else (amax all nblocks).  backward scratch: dxs [nblocks][M,B,Kp], dh1s [nblocks][M,H,Kp]. */
int ctn_tcn_cln_fwd(const void* const* params, const int* dilation, int nblocks, const float* x0,
                    float* xs, float* h1s, float* n1s, float* ds, float* n2s, float* st, unsigned* amax, int save,
                    int M, int B, int H, int K, int Kp, int P, int causal,
                    void* workspace, size_t workspace_bytes, void* stream, void* side_stream);
size_t ctn_tcn_cln_fwd_workspace(int M, int B, int H, int Kp, int nblocks);
int ctn_tcn_cln_bwd(const void* const* params, void* const* grads, const int* dilation, int nblocks,
                    const float* x0, const float* xs, const float* h1s, const float* n1s, const float* ds, const float* n2s,
                    const float* st, const unsigned* amax, const float* dout, float* dxs, float* dh1s,
                    int M, int B, int H, int K, int Kp, int P, int causal,
                    void* workspace, size_t workspace_bytes, void* stream, void* side_stream, int flags);
size_t ctn_tcn_cln_bwd_workspace(int M, int B, int H, int Kp, int P, int nblocks);

/* ---- channel-wise LayerNorm, src/conv_tasnet.py:313-335 (per frame, biased variance) -----
 * Out = gamma*((a-mean_k)*rstd_k)+beta with a = prelu(Y,alpha) if alpha != NULL else Y.
 * mean, rstd: [M,Kp] saved for backward.  amax_out != NULL: [M][CTN_AMAX_SLOTS], receives max |Out[m]| (h3 section). */
int ctn_cln_fwd(const float* Y, float* Out, float* mean, float* rstd, int M, int Ch, int K, int Kp,
                const float* gamma, const float* beta, const float* alpha, unsigned* amax_out, void* stream);
/* dY = [cLN/PReLU backward of dOut  (+ add)] masked by (relu_ref > 0) when relu_ref != NULL -- and, in the same pass, the
 * parameter-gradient partials: pc [2][ctn_cln_bwd_blocks(M,Kp)][Ch] (ctn_cln_bwd_pc_floats() floats: dgamma, dbeta of every
 * workgroup's 16 frames -- 32 with ctn_tune("cln_fr", 32) --) and dalpha_part [ctn_cln_bwd_blocks(M,Kp)]; ctn_cln_bwd_finalize
 * sums them in fixed order.  Size both with the functions below AFTER any ctn_tune("cln_fr", ...).
 * amax_out != NULL: [M][CTN_AMAX_SLOTS], receives max |dY[m]| (h3 section). */
int ctn_cln_bwd(const float* dOut, const float* Y, float* dY, const float* mean, const float* rstd,
                int M, int Ch, int K, int Kp, const float* gamma, const float* alpha,
                const float* add, const float* relu_ref, float* dalpha_part, float* pc, unsigned* amax_out, void* stream);
int ctn_cln_bwd_blocks(int M, int Kp);
size_t ctn_cln_bwd_pc_floats(int M, int Ch, int Kp);
/* cLN backward WITHOUT a pass of its own (round 4), for a norm that sits between a 1x1 conv and the depthwise conv
 * (src/conv_tasnet.py:257-266): the input-gradient GEMM of the 1x1 conv produces, besides dN = W^T . dOut, the two per-frame sums
 * over channels that the norm's backward needs,
 *     S1[k] = sum_c gamma_c dN[c,k],   S2[k] = sum_c gamma_c dN[c,k] xhat[c,k],   xhat = (prelu(y, alpha) - mean[k]) rstd[k],
 * as column partials of its row tiles: col_part [M][ctn_pw_col_parts(M,R,Kp,w_form)][Kp][2] fp64 (fixed order inside a tile);
 * ctn_cln_bwd_frame sums them over the row tiles and writes fc [M][4][Kp] = (rstd, mean rstd, rstd S1/Ch, rstd S2/Ch)[k], from which
 * ctn_dw_bwd_cln forms  dy = rstd (gamma dN - S1/Ch - xhat S2/Ch) prelu'(y)  on the fly.
 *   W / w_form: 1 = the stored fp32 [Cn, R] matrix used transposed (arithmetic by ctn_tune("arith")), 2 = b6 pieces
 *   (ctn_split_b3_batch, k_major = 1), 3 = h3 pieces (ctn_split_h3_batch, k_major = 1; g_amax = tracked maximum of dOut, else NULL).
 *   y: the norm's input [M,R,Kp]; mean, rstd: [M,Kp] saved by ctn_cln_fwd. */
int ctn_pw_dgrad_cln(const void* W, int w_form, const float* dOut, float* dN, int M, int R, int Cn, int K, int Kp,
                     const float* y, const float* gamma, const float* alpha, const float* mean, const float* rstd,
                     double* col_part, const unsigned* g_amax, void* stream);
int ctn_pw_col_parts(int M, int R, int Kp, int w_form);
/* cLN forward WITHOUT a pass of its own (round 4), for the norm between the first 1x1 conv and the depthwise conv
 * (src/conv_tasnet.py:223-225 with norm_type = 'cLN'): ctn_pw_gemm_cln is the 1x1 conv Out = op(W) . X that also leaves, per frame,
 * (sum_c p, sum_c p^2), p = prelu(Out, alpha), as column partials of its row tiles (col_part as above; w_form 0 = fp32 [R, Cn],
 * 1 = fp32 [Cn, R] used transposed, 2 = b6 pieces, 3 = h3 pieces with x_amax = tracked maximum of X); ctn_cln_stats_frame sums them
 * over the row tiles into mean, rstd [M,Kp] (fp64, biased variance, eps as ctn_cln_fwd); ctn_dw_fwd_cln is ctn_dw_fwd with
 * n = gamma ((prelu(Y, alpha) - mean[k]) rstd[k]) + beta applied while the row is staged: the norm's output is never stored. */
int ctn_pw_gemm_cln(const void* W, int w_form, const float* X, float* Out, int M, int R, int Cn, int K, int Kp,
                    const float* alpha, double* col_part, const unsigned* x_amax, void* stream);
int ctn_cln_stats_frame(const double* col_part, int nparts, float* mean, float* rstd, int M, int Ch, int Kp, void* stream);
int ctn_dw_fwd_cln(const float* Y, float* Z, const float* D, int M, int H, int K, int Kp, int P, int dilation, int causal,
                   const float* mean, const float* rstd, const float* gamma, const float* beta, const float* alpha, void* stream);
int ctn_cln_bwd_frame(const double* col_part, int nparts, const float* mean, const float* rstd, float* fc, int M, int Ch, int Kp,
                      void* stream);
/* One launch that finishes the partials above in fixed order: dgamma[Ch], dbeta[Ch] from pc, and dalpha[1] from
 * dalpha_part [ctn_cln_bwd_blocks(M,Kp)] when that is non-NULL. */
int ctn_cln_bwd_finalize(const float* pc, const float* dalpha_part, int M, int Ch, int Kp, float* dgamma, float* dbeta,
                         float* dalpha, void* stream);

/* ---- cumulative LayerNorm (the causal norm of Luo & Mesgarani 2019, eq. 12-14; not in src/conv_tasnet.py) -----
 * Frame k is normalised by the statistics of all channels of all frames 0..k of its utterance (a = prelu(Y, alpha) or Y):
 *     mean_k = sum_{j<=k} sum_c a[c,j] / n_k,  n_k = Ch (k + 1),  rstd_k = 1 / sqrt(max(E_k[a^2] - mean_k^2, 0) + eps),
 *     Out = gamma (a - mean_k) rstd_k + beta.
 * Per frame that is the channel-wise norm's affine form, so ctn_pw_gemm_cln / ctn_dw_fwd_cln and ctn_pw_dgrad_cln / ctn_dw_bwd_cln
 * serve it unchanged; only the per-frame kernels between them differ:
 *   ctn_cumln_stats_frame: col_part as for ctn_cln_stats_frame -> mean, rstd [M,Kp]; frames k >= K get (0, 1/sqrt(eps)).
 *   ctn_cumln_bwd_frame  : col_part as for ctn_cln_bwd_frame (the sums taken with the cumulative mean / rstd) ->
 *       fc [M][4][Kp] = (rstd, mean rstd, U - W + mean V, V / rstd)[k] with the suffix sums over the valid frames
 *       (U, V, W)_j = sum_{j<=k<K} (rstd_k S1_k, rstd_k^2 S2_k, rstd_k^2 S2_k mean_k) / n_k, which ctn_dw_bwd_cln turns into
 *       da = rstd gamma dN - U + W - a V.
 * The prefix sums run in fp64 in ONE order fixed by the absolute frame index (64-frame blocks sequentially inside, block prefixes
 * sequentially), so a stream cut into calls anywhere gives the bits of one call.  carry [M][4] fp64 + count [M] long long hold
 * the state across calls IN DEVICE MEMORY (zero both to start a stream; the kernel advances them, so a captured graph replays it);
 * NULL for both: whole utterances starting at frame 0.  The backward has no chunked form.
 *   ctn_cumln_fwd: the norm as passes of its own (per-frame sums in fp64 -> scan -> apply: three tensor passes); any alignment and
 *       any Kp (16-byte accesses when the rows allow).  work: ctn_cumln_work_bytes(M, Kp) bytes, 16-byte aligned.
 *   ctn_cumln_bwd: dY = cumLN/PReLU backward of dOut (sums + parameter partials -> suffix scans -> apply: five tensor passes).
 *       Frames k >= K of dOut may hold anything; those of dY are written as zeros.  dY may alias dOut.  pc and dalpha_part
 *       (required with alpha) have ctn_cln_bwd's layout and sizes: finish them with ctn_cln_bwd_finalize. */
int ctn_cumln_stats_frame(const double* col_part, int nparts, float* mean, float* rstd, double* carry, long long* count,
                          int M, int Ch, int K, int Kp, void* stream);
int ctn_cumln_bwd_frame(const double* col_part, int nparts, const float* mean, const float* rstd, float* fc,
                        int M, int Ch, int K, int Kp, void* stream);
size_t ctn_cumln_work_bytes(int M, int Kp);
int ctn_cumln_fwd(const float* Y, float* Out, float* mean, float* rstd, int M, int Ch, int K, int Kp,
                  const float* gamma, const float* beta, const float* alpha, double* carry, long long* count,
                  void* work, void* stream);
int ctn_cumln_bwd(const float* dOut, const float* Y, float* dY, const float* mean, const float* rstd,
                  int M, int Ch, int K, int Kp, const float* gamma, const float* alpha,
                  float* dalpha_part, float* pc, void* work, void* stream);
/* The two passes with the h3 maximum of what they store tracked on the way (what the composite cumLN stack calls): the same
 * arguments plus amax_out [M][CTN_AMAX_SLOTS] -- its slots receive max |Out[m]| (forward) / max |dY[m]| (backward), merged into what
 * they hold, bit for bit what ctn_absmax_rows of the stored tensor gives.  The 16-byte forms take the maximum in their apply pass (a
 * few VALU max per element, one atomic per workgroup); the scalar / general forms finish with a ctn_absmax_rows pass (the stored
 * tensor must then be 16-byte aligned with Ch * Kp % 4 == 0).  Every other output has the bits of the untracked entry points, which
 * are these with amax_out = NULL. */
int ctn_cumln_fwd_amax(const float* Y, float* Out, float* mean, float* rstd, int M, int Ch, int K, int Kp,
                       const float* gamma, const float* beta, const float* alpha, double* carry, long long* count,
                       void* work, unsigned* amax_out, void* stream);
int ctn_cumln_bwd_amax(const float* dOut, const float* Y, float* dY, const float* mean, const float* rstd,
                       int M, int Ch, int K, int Kp, const float* gamma, const float* alpha,
                       float* dalpha_part, float* pc, void* work, unsigned* amax_out, void* stream);

/* The stack of cumLN TemporalBlocks (norm_type = 'cumLN': the paper's causal model) behind one call per direction: the parameter
 * lists, the params / grads layout, the saved activations, amax, save, flags, the streams and the half-batch chains of the cLN stack
 * above.  Per block it is the cLN stack's fully fused chain whatever ctn_tune("cln_fuse") says, with the per-frame kernels of the
 * cumulative norm:
 *   forward : ctn_pw_gemm_cln -> ctn_cumln_stats_frame (whole utterances: carry = count = NULL) -> ctn_dw_fwd_cln ->
 *             ctn_cumln_fwd_amax (second norm; n2's maximum tracked) -> 1x1 + residual
 *   backward: ctn_pw_dgrad_cln -> [dW2] -> ctn_cumln_bwd_frame -> ctn_dw_bwd_cln (first norm applied on the fly) ->
 *             ctn_cumln_bwd_amax (first norm; dh1's maximum tracked) -> [ctn_dw_bwd_cln_finalize, ctn_cln_bwd_finalize, dW1] -> 1x1 + dy
 * ([..]: on side_stream when given) -- the calls of ops.CumLnBlock, so the results are bitwise the per-block path's.
 * n1s is never written or read (may be NULL).  causal must be 1 (CTN_ERR_ARG otherwise).  The workspaces are the cLN stack's
 * layouts followed by ctn_cumln_work_bytes(M, Kp) regions: two forward (one per chain), one backward. */
int ctn_tcn_cumln_fwd(const void* const* params, const int* dilation, int nblocks, const float* x0,
                      float* xs, float* h1s, float* n1s, float* ds, float* n2s, float* st, unsigned* amax, int save,
                      int M, int B, int H, int K, int Kp, int P, int causal,
                      void* workspace, size_t workspace_bytes, void* stream, void* side_stream);
size_t ctn_tcn_cumln_fwd_workspace(int M, int B, int H, int Kp, int nblocks);
int ctn_tcn_cumln_bwd(const void* const* params, void* const* grads, const int* dilation, int nblocks,
                      const float* x0, const float* xs, const float* h1s, const float* n1s, const float* ds, const float* n2s,
                      const float* st, const unsigned* amax, const float* dout, float* dxs, float* dh1s,
                      int M, int B, int H, int K, int Kp, int P, int causal,
                      void* workspace, size_t workspace_bytes, void* stream, void* side_stream, int flags);
size_t ctn_tcn_cumln_bwd_workspace(int M, int B, int H, int Kp, int P, int nblocks);

/* ---- BatchNorm1d over (utterances, frames) per channel, optionally behind PReLU ------------------
 * replaces nn.BatchNorm1d as returned by chose_norm's else-branch, src/conv_tasnet.py:305-309, at its two uses
 * (:225 after PReLU :224, :260 after PReLU :259).  gamma/beta are nn.BatchNorm1d's weight/bias [Ch].
 *   training != 0: batch statistics over the M*K valid frames (biased variance for the normalisation); when
 *     running_mean/running_var are non-NULL they are updated in place with `momentum` (unbiased variance), as
 *     torch does.  part: [Ch*M*2] fp64 workspace.
 *   training == 0: normalises with running_mean / running_var.
 *   alpha != NULL: the input is prelu(Y, alpha) (fused), else Y itself.
 *   mr [Ch,2] out: the (mean, 1/sqrt(var+eps)) actually used -- saved for ctn_bn_bwd.  Frames >= K are written 0. */
int ctn_bn_fwd(const float* Y, float* Out, const float* alpha, const float* gamma, const float* beta,
               float* running_mean, float* running_var, int training, float eps, float momentum,
               int M, int Ch, int K, int Kp, double* part, float* mr, void* stream);
/* dY (may alias dOut) = gradient w.r.t. Y (through the PReLU when alpha != NULL); dgamma/dbeta [Ch];
 * dalpha_part [M*Ch] per-row partials (sum them in order for dalpha);  part [Ch*M*2] fp64 and coef [Ch,2] workspaces. */
int ctn_bn_bwd(const float* dOut, const float* Y, float* dY, const float* alpha, const float* gamma, const float* mr,
               int training, int M, int Ch, int K, int Kp, double* part, float* coef, float* dgamma, float* dbeta,
               float* dalpha_part, void* stream);

/* out[f][i] = sum_r in[f][r][i]  -- fixed-order finish of the per-(m,c) partials above */
int ctn_reduce_mid(const float* in, float* out, int F, int Mid, int Inner, void* stream);

/* ---- encoder / decoder glue -----------------------------------------------------------
 * encoder  src/conv_tasnet.py:106-121 : ctn_encoder_fwd (forward); ctn_im2col + ctn_pw_wgrad (basis gradient)
 * decoder  src/conv_tasnet.py:140-145 : ctn_mask_apply + ctn_pw_gemm + ctn_ola (src/utils.py:9-47)
 * mask non-linearity src/conv_tasnet.py:208-214 (relu | softmax over speakers). */
int ctn_im2col(const float* mix, float* xcol, int M, int T, int L, int Lp, int K, int Kp, void* stream);
/* The encoder in one kernel (forward): w[m,n,k] = relu(sum_l U[n,l] * mix[m, k*L/2 + l]), zero for k >= K; the L-sample
 * sliding windows of 256 frames and the basis rows are staged in LDS, no im2col buffer.  U: [N, L] (the Conv1d weight
 * [N,1,L]); w: [M,N,Kp].  Filter lengths compiled in: ctn_encoder_supported(L) (16, 20, 32, 40); other lengths and the
 * weight gradient use ctn_im2col + the GEMM entry points. */
int ctn_encoder_supported(int L);
int ctn_encoder_fwd(const float* mix, const float* U, float* w, int M, int T, int N, int L, int K, int Kp, void* stream);
/* softmax: 0 = relu, 1 = softmax over speakers, 2 = identity (sw = w * score: the stand-alone Decoder.forward, :140) */
int ctn_mask_apply(const float* score, const float* w, float* sw, int M, int C, int N, int Kp, int softmax, void* stream);
int ctn_mask_apply_bwd(const float* dsw, const float* score, const float* w, float* dscore, float* dw,
                       int M, int C, int N, int Kp, int softmax, void* stream);
/* est[b, t] = sum_{k*S+l = t} frames[b, l, k]; zeros for t >= (K-1)S+L (the F.pad of :59). frames:[Bn,Lp,Kp] */
int ctn_ola(const float* frames, float* est, int Bn, int T, int L, int Lp, int K, int Kp, void* stream);
int ctn_unfold(const float* dest, float* dframes, int Bn, int T, int L, int Lp, int K, int Kp, void* stream);
/* overlap_and_add(signal, frame_step) for ANY frame_step, src/utils.py:9-47 (the reference splits frames into
 * gcd(frame_length, frame_step) sub-frames and index_add_s them; here a deterministic gather in ascending frame order):
 * signal [Bn, frames, frame_length] row-major -> out [Bn, (frames-1)*frame_step + frame_length]; _bwd is its adjoint. */
int ctn_overlap_add(const float* signal, float* out, int Bn, int frames, int frame_length, int frame_step, void* stream);
int ctn_overlap_add_bwd(const float* dout, float* dsignal, int Bn, int frames, int frame_length, int frame_step, void* stream);

/* ---- PIT SI-SNR loss, src/pit_criterion.py:12-77 -----------------------------------------
 * source, estimate: [B,C,T]; lengths: [B] int64; perms: [nperm,C] int32 in itertools order.
 * estimate is masked IN PLACE for t >= len (reference :38).  Outputs: max_snr [B], best_idx [B] int64,
 * loss [1] = -mean(max_snr), snr_out [B,C,C] (optional), and the backward tables coef [B,C,4], jsel [B,C].
 * Source samples at t >= len are never read: every sum, the source mean included, runs over t < len.  The reference
 * instead divides the source's full-length sum by len (:41), so the two agree only for a source that is zero at
 * t >= len, which is what every loader here produces. */
int ctn_sisnr_pit_fwd(const float* source, float* estimate, const long long* lengths, const int* perms, int nperm,
                      int B, int C, int T, float* max_snr, long long* best_idx, float* loss, float* snr_out,
                      float* coef, int* jsel, void* workspace, size_t workspace_bytes, void* stream);
size_t ctn_sisnr_workspace(int B, int C, int T);
int ctn_sisnr_chunks(int T);
/* d_estimate = dloss/d estimate for upstream grads g_loss [1] and/or g_max [B] (either may be NULL) */
int ctn_sisnr_pit_bwd(const float* source, const float* estimate, const long long* lengths, const float* coef,
                      const int* jsel, const float* g_loss, const float* g_max, int B, int C, int T, float* d_estimate,
                      void* stream);

/* ---- optimiser tail, src/solver.py:194-196 (clip_grad_norm_ + Adam.step) on flat buffers ---
 * g' = grad_scale*g; total = ||g'||2 -> total_norm_out; g' *= min(1, max_norm/(total+1e-6)) if max_norm > 0;
 * torch.optim.Adam update (no weight decay / amsgrad) with bias corrections for `step` (1-based).
 * workspace: ctn_optim_parts() doubles. */
int ctn_clip_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n,
                       float grad_scale, float max_norm, float lr, float beta1, float beta2, float eps, int step,
                       float* total_norm_out, double* workspace, void* stream);
int ctn_optim_parts(void);
/* The same clip (the norm is of the clipped gradient g' only; the decay term comes after it, as the reference Solver clips
 * before optimizer.step() adds it), then the torch.optim.SGD update of src/train.py:87-91 (optimizer_type 'sgd',
 * momentum, weight_decay = l2):  d = g' + weight_decay*p;  with momentum != 0:  buf = first_step ? d :
 * momentum*buf + (1-dampening)*d,  d = nesterov ? d + momentum*buf : buf;  p -= lr*d.
 * momentum_buf may be NULL (and is never touched) when momentum == 0; nesterov needs momentum > 0, dampening == 0.
 * params, grads, momentum_buf 16-byte aligned.  workspace: ctn_optim_parts() doubles. */
int ctn_clip_sgd_step(float* params, const float* grads, float* momentum_buf, long long n, float grad_scale,
                      float max_norm, float lr, float momentum, float dampening, float weight_decay, int nesterov,
                      int first_step, float* total_norm_out, double* workspace, void* stream);
/* ctn_clip_adam_step with coupled L2 (src/train.py:92-95 with weight_decay = l2 > 0, torch.optim.Adam(weight_decay=...),
 * not AdamW): the Adam update of g' + weight_decay*p.  All four buffers 16-byte aligned. */
int ctn_clip_adam_l2_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n,
                          float grad_scale, float max_norm, float lr, float beta1, float beta2, float eps, int step,
                          float weight_decay, float* total_norm_out, double* workspace, void* stream);

/* ---- BSS Eval v3: SDR / SIR / SAR in fp64 ------------------------------------------------------------------------------
 * replaces mir_eval.separation.bss_eval_sources(reference_sources, estimated_sources) (compute_permutation=True, 512-tap
 * distortion filters) as called by cal_SDRi, src/evaluate.py:76-91, and by the calc_sdr branch of evaluate, :62-72.
 * ref: [B,C,T] fp32 references, est: [B,E,T] fp32 estimate rows (cal_SDRi's mixture anchor can be one extra row), lengths:
 * [B] int64; samples at t >= lengths[b] count as zero in both.  2 <= C <= 4, E >= 1, T >= 1; all arithmetic fp64.
 * The time partition of every reduction depends on lengths[b] only: an utterance scores bitwise the same in any batch.
 *   ctn_bss_eval: everything below in one call -> sdr, sir, sar [B,E,C] fp64 (row e scored against reference j; the SIR
 *     permutation choice over them is the caller's), status [B,C] int32 (0: factorised; else 1 + the first pivot that was
 *     not finite or not above dim*eps*max diag: [b,0] = G (C*512 square, whose leading block also serves G_00), [b,j] = G_jj;
 *     an utterance with a non-zero status has undefined numbers and must be redone another way).
 *     workspace: ctn_bss_workspace() bytes, grows as B*(C*512)^2*8.
 * The stages, each on caller buffers:
 *   ctn_bss_corr: r [B,C,C,512] r[b,i,k,tau] = sum_t s_i[t] s_k[t+tau]; d [B,E,C,512] d[b,e,i,a] = sum_t s_i[t] e[t+a];
 *     enorm [B,E] = sum_t e[t]^2.  workspace: ctn_bss_corr_workspace() bytes.
 *   ctn_bss_factor: Gram matrices from r and their Cholesky factors (lower triangle) in factors (ctn_bss_factor_doubles()
 *     doubles: B matrices of (C*512)^2, then B*(C-1) of 512^2 for G_11.. G_{C-1,C-1}), status as above.
 *   ctn_bss_solve: coef_all [B,E,C*512] = G^-1 d[b,e];  coef_own [B,E,C,512] = G_jj^-1 d[b,e,j].
 *   ctn_bss_project: P_all e, P_j e as 512-tap FIRs of the references over the n+511 samples of the padded signals; the
 *     residual energies accumulated explicitly -> sdr, sir, sar; energies [B,E,3C+2] (nullable): per j ||P_j e||^2,
 *     ||e - P_j e||^2, ||P_all e - P_j e||^2, then ||P_all e||^2, ||e - P_all e||^2.  workspace: ctn_bss_project_workspace().
 *   sdr = 10 log10(||P_j e||^2 / ||e - P_j e||^2), sir = 10 log10(||P_j e||^2 / ||P_all e - P_j e||^2),
 *   sar = 10 log10(||P_all e||^2 / ||e - P_all e||^2); a zero denominator gives +inf. */
#define CTN_BSS_FLEN 512
size_t ctn_bss_workspace(long long B, int C, long long E, long long T);
int ctn_bss_eval(const float* ref, const float* est, const long long* lengths, long long B, int C, long long E, long long T,
                 double* sdr, double* sir, double* sar, int* status, void* workspace, size_t workspace_bytes, void* stream);
size_t ctn_bss_corr_workspace(long long B, int C, long long E, long long T);
int ctn_bss_corr(const float* ref, const float* est, const long long* lengths, long long B, int C, long long E, long long T,
                 double* r, double* d, double* enorm, void* workspace, size_t workspace_bytes, void* stream);
size_t ctn_bss_factor_doubles(long long B, int C);
int ctn_bss_factor(const double* r, long long B, int C, double* factors, int* status, void* stream);
int ctn_bss_solve(const double* factors, const double* d, long long B, int C, long long E, double* coef_all, double* coef_own,
                  void* stream);
size_t ctn_bss_project_workspace(long long B, int C, long long E, long long T);
int ctn_bss_project(const float* ref, const float* est, const long long* lengths, const double* coef_all, const double* coef_own,
                    long long B, int C, long long E, long long T, double* sdr, double* sir, double* sar, double* energies,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- fused low-latency streaming inference of the causal cLN model (csrc/ctn_stream.hip) -----------------------------
 * Chunk-wise TemporalConvNet.forward (src/conv_tasnet.py:176-186 with causal = True, norm_type = 'cLN') on UNPADDED chunks:
 * activations here are [M, Ch, F] with F = the frames of this chunk (no 64-frame padding).  One workgroup carries a tile of 16
 * frame columns of one stream through a whole block boundary in LDS; the depthwise history of block j is a ring buffer
 * ring[j] [M,H,Rj], Rj = the power of two >= (P-1)*dilation[j] + max_frames, inside `state`, whose first word is the write
 * position (device memory: a captured step replays without new arguments).  nblocks + 1 stage launches + one that advances the
 * position (frames <= 16 and M <= 128: two launches per block whose workgroups split the GEMMs' output rows, bitwise the same
 * values); a straight chain on `stream`.  Arithmetic is frame-local and in a fixed order (exact fp32 MFMA chains, two-pass
 * per-frame cLN): a frame's values do not depend on the chunk it arrived in, its position in the chunk, or the other streams.
 *   ctn_stream_state_bytes: host-only; 256 bytes of header + 4*M*H*(sum_j Rj + 16: one tile of scratch per stream).  A zeroed state
 *     = the start of a stream.
 *   ctn_stream_pack: the stack's parameters (`params` HOST [nblocks][9] device pointers in the order of ctn_tcn_cln_fwd)
 *     -> `packed` (ctn_stream_pack_bytes): per block the two 1x1 weights in MFMA fragment order, then the small vectors.
 *     Weights are constants at inference: pack once, again after they change.
 *   ctn_stream_tcn_cln: y [M,B,frames] in place through the nblocks blocks, state advanced.  B, H multiples of 16 with
 *     (B + H + 64) * 64 bytes of LDS <= 64 KiB, 1 <= P <= 8, any dilation >= 1, 1 <= frames <= max_frames (the value
 *     the state was sized with).
 *   ctn_stream_pack_gemm: one weight W [R,Cn] row-major -> fragment order (rows / contraction zero-filled to multiples of 16).
 *   ctn_stream_front: frames k = x[m][k*S .. k*S+L), S = L/2, of the sample buffer x [M][xld] -> w = relu(U frame) [M,N,frames]
 *     -> cLN(g0, b0) -> bottleneck 1x1 -> y [M,B,frames]   (src/conv_tasnet.py:96-99, :152-156).  Up, Wbp: packed [N,L], [B,N].
 *   ctn_stream_back: mask 1x1 (Wmp packed [C*N,B]) -> relu (softmax = 0) or softmax over speakers (1) -> * w -> basis (Vp packed
 *     [L,N]) -> fr [M,C,L,frames] (scratch) -> overlap-add with the carried half frame ola_tail [M,C,S] -> out [M,C,frames*S];
 *     then the carries: ola_tail = second half of the last frame, x[m][0..S) = x[m][frames*S .. frames*S+S)
 *     (src/conv_tasnet.py:118-132, :199-211).  N, B multiples of 16, L a multiple of 4, C <= 8. */
size_t ctn_stream_state_bytes(int M, int H, int P, const int* dilation, int nblocks, int max_frames);
size_t ctn_stream_pack_bytes(int B, int H, int P, int nblocks);
int ctn_stream_pack(const void* const* params, int nblocks, int B, int H, int P, void* packed, void* stream);
int ctn_stream_tcn_cln(const void* packed, const int* dilation, int nblocks, float* y, void* state, int M, int B, int H, int P,
                       int frames, int max_frames, void* stream);
int ctn_stream_reset(void* state, size_t bytes, void* stream);
size_t ctn_stream_pack_gemm_bytes(int R, int Cn);
int ctn_stream_pack_gemm(const float* W, int R, int Cn, void* packed, void* stream);
int ctn_stream_front(const float* x, int xld, const void* Up, const float* g0, const float* b0, const void* Wbp, float* w, float* y,
                     int M, int N, int L, int B, int frames, void* stream);
int ctn_stream_back(const float* y, const float* w, const void* Wmp, const void* Vp, float* fr, float* out, float* ola_tail,
                    float* x, int xld, int M, int N, int L, int B, int C, int frames, int softmax, void* stream);

/* ---- ragged steps of the same kernels: a slot pool whose streams join, leave and deliver different amounts (csrc/ctn_stream.hip) ----
 * One step serves M slots; slot m computes nf[m] frames, 0 <= nf[m] <= frames.  `frames` (the maximum over the slots) sizes the grid
 * and is the leading dimension of w, y, fr and the step output, exactly as in the calls above; a workgroup whose tile starts at or
 * beyond nf[m] returns before its first load.  The same device functions run the same per-element FMA chains and cLN sums: a frame's
 * values are bitwise those of the calls above.  Two caller-owned device arrays replace the scalar count and the state's position word:
 *   tab  int [M][CTN_STREAM_TAB], rewritten by the caller before every step; offsets in hops of S = L/2 samples:
 *        [0] nf   frames to compute                      [1] nh   hops to load (nf, or nf + 1 for a stream that starts with this step)
 *        [2] src  first hop in the caller's chunk row    [3] dst  where they land in the sample buffer row: 0 for a stream that
 *        [4] out  first hop in the caller's output row        starts with this step (its first frame begins at its sample 0), else 1
 *        [5..7] unused.  The kernels clamp nf to 0..frames and the copies to their rows: a bad table cannot write out of bounds.
 *   pos  unsigned [M]: ring position per slot (the position word in `state`'s header is unused by these calls).
 * `state` is laid out and sized as above (ctn_stream_state_bytes).  A step is  load -> front -> tcn_cln -> back -> store  on `stream`:
 * 2 more launches than the calls above, none of them per slot.
 *   ctn_stream_load_ragged: x[m][(dst+h)*S ..] = chunk[m][(src+h)*S ..], h < nh[m]; chunk: M rows of chunk_hops hops, row stride cld
 *     samples; max_hops >= every nh (grid size).
 *   ctn_stream_front_ragged / _tcn_cln_ragged / _back_ragged: as ctn_stream_front / _tcn_cln / _back with nf[m] valid frames for
 *     slot m; tcn_cln advances pos[m] by nf[m]; back writes the step output out [M,C,frames*S] (nf[m]*S samples valid per row), and a
 *     slot with nf[m] = 0 keeps its ola_tail and its carried hop.
 *   ctn_stream_store_ragged: dst[m][c][(out+k)*S ..] = step output frames k < nf[m]; dst [M,C,dld] (the caller's padded rows).
 *   ctn_stream_reset_slots: the `nslots` slots listed in `slots` (HOST array) back to the start of a stream: their part of every
 *     ring, their carried hop x[m][0..S), ola_tail [M,C,S] row and pos[m] are zeroed, in one launch per 64 blocks x 32 slots. */
#define CTN_STREAM_TAB 8
int ctn_stream_load_ragged(const float* chunk, long long cld, int chunk_hops, float* x, int xld, const int* tab, int M, int S, int max_hops,
                           void* stream);
int ctn_stream_front_ragged(const float* x, int xld, const void* Up, const float* g0, const float* b0, const void* Wbp, float* w, float* y,
                            const int* tab, int M, int N, int L, int B, int frames, void* stream);
int ctn_stream_tcn_cln_ragged(const void* packed, const int* dilation, int nblocks, float* y, void* state, const int* tab, void* pos,
                              int M, int B, int H, int P, int frames, int max_frames, void* stream);
int ctn_stream_back_ragged(const float* y, const float* w, const void* Wmp, const void* Vp, float* fr, float* out, float* ola_tail,
                           float* x, int xld, const int* tab, int M, int N, int L, int B, int C, int frames, int softmax, void* stream);
int ctn_stream_store_ragged(const float* out, float* dst, long long dld, const int* tab, int M, int C, int S, int frames, void* stream);
int ctn_stream_reset_slots(void* state, float* x, int xld, float* ola_tail, void* pos, const int* slots, int nslots, int M, int H, int P,
                           const int* dilation, int nblocks, int max_frames, int C, int L, void* stream);

/* ---- the same stack with the cumulative layer norm (norm_type 'cumLN', csrc/ctn_stream.hip) -------------------------------------------
 * ctn_stream_tcn_cumln / _ragged are ctn_stream_tcn_cln / _ragged with both norms of every block cumulative, under the contract of
 * ctn_cumln_fwd: with a = prelu(input),  s1 = sum_ch a[ch,k],  s2 = sum_ch a[ch,k]^2  of the frame's own channels and C1, C2 their
 * running sums over the stream's frames 0 .. k,   n = Ch (k + 1),  mu = C1 / n,  r = 1 / sqrt(max(C2 / n - mu^2, 0) + 1e-8),
 * out = gamma (a - mu) r + beta.  Everything from the first addition to mu and r is fp64; mu and r are rounded to fp32 once and applied
 * in fp32.  The prefix is the plain chain C_k = C_(k-1) + s_k continued from the carried sums, so a frame's statistics depend on its
 * absolute index and the stream's past only: not on the chunking, the column, the kernel form or the other slots.  `packed`, `state`,
 * `tab` and `pos` are those of the cLN calls (ctn_stream_pack serves both norms); front and back end are the same calls.
 *   cum: caller-owned device buffer of ctn_stream_cum_bytes(M, nblocks) bytes, 16-byte aligned: two banks (current, pending) of
 *        [M][nblocks][2 norms] records of 32 bytes: { double C1; double C2; uint64 frames; uint64 unused }.  All zeros = the start
 *        of a stream (zero the whole buffer with a memset, or listed slots with ctn_stream_cum_reset_slots).  The kernels of a step read
 *        the current bank and one workgroup per slot writes the pending one; the step's last launch, which also advances the ring
 *        position(s), copies pending over current for every slot that computed frames (ragged: nf[m] > 0; a slot with nf[m] = 0 keeps
 *        both banks bit for bit).  The frame count is the record's own 64-bit word, not the 32-bit ring position.
 *   frames <= 16: a tile's prefix needs the sums of the stream's earlier tiles and no kernel here waits on another workgroup, so a step
 *        is at most ONE 16-frame tile per slot; the caller cuts longer chunks into consecutive steps.  max_frames is what `state` was
 *        sized with, as above.  LDS: (B + H) * 64 + 4480 bytes <= 64 KiB (the fp64 partial sums of both moments, per wave).
 *   ctn_stream_cum_reset_slots: both banks of the `nslots` slots listed in `slots` (HOST array) zeroed, one launch per 32 slots. */
size_t ctn_stream_cum_bytes(int M, int nblocks);
int ctn_stream_tcn_cumln(const void* packed, const int* dilation, int nblocks, float* y, void* state, void* cum,
                         int M, int B, int H, int P, int frames, int max_frames, void* stream);
int ctn_stream_tcn_cumln_ragged(const void* packed, const int* dilation, int nblocks, float* y, void* state, void* cum,
                                const int* tab, void* pos, int M, int B, int H, int P, int frames, int max_frames, void* stream);
int ctn_stream_cum_reset_slots(void* cum, const int* slots, int nslots, int M, int nblocks, void* stream);

/* ---- on-device dynamic mixing: a resident single-speaker corpus and the minibatch sampler (csrc/ctn_dynmix.hip) ---------
 * replaces the offline mixture set of the reference's recipe: the list tools/create_txt_file_like_wsj0.py draws (two
 * speakers, snr_1 = randrange(1, 250) / 100 dB, snr_2 = -snr_1) and tools/matlab-code/create_wav_2speakers.m builds
 * (sources at unit level, weighted by 10^(snr/20), added, everything rescaled to a peak of 0.9), with a fresh draw every step.
 * corpus: one flat fp32 buffer of num_samples samples holding U utterances back to back; offsets [U], lens [U] int64.
 *   ctn_dynmix_levels: meansq [U] fp64 = the mean of the squares of every utterance, one workgroup per utterance: thread t
 *     of 256 sums samples t, t + 256, ... in fp64, then a fixed-order block sum.  The partition depends on the utterance's own
 *     length only, so a value does not depend on the neighbours or on U.  An entry outside [0, num_samples) gives -1.
 *   ctn_dynmix_plan: the plan of one minibatch, then *step += 1 ON THE DEVICE (the host passes the same arguments every
 *     step: a captured call replays).  plan_utt [B,C] int32, plan_start [B,C] int64, plan_q [B,C] int32, gain [B,C] fp32.
 *     Tables: spk_ptr [S+1] int32 (CSR over speakers), utt_ids [spk_ptr[S]] int32: the ELIGIBLE utterances of every speaker
 *     (lens[u] >= seg_len and meansq[u] > 0; every speaker has at least one), inv_rms [U] fp32 = 1 / sqrt(meansq[u]),
 *     w [499] fp32 = 10^(q / 2000) for q = -249 .. 249, both rounded from fp64 on the host: no pow or sqrt on the device.
 *     The draw is a pure function of (seed, rank, epoch, step, b) through Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57,
 *     key increments 0x9E3779B9, 0xBB67AE85):
 *         counter = (c, b, step, epoch)      key = (seed bits 0..31, seed bits 32..47 | rank << 16)
 *     one block of four words per source c of mixture b; 0 <= seed < 2^48, 0 <= rank < 2^16, epoch >= 0.  An integer in [0, n)
 *     from a word r is (uint64(r) * n) >> 32 (bias below n / 2^32).  Of the block of source c:
 *         word 0  speaker: s in [0, S - c), then stepped over the c speakers already taken, in ascending order (C distinct
 *                 speakers, uniform without replacement, no rejection loop)
 *         word 1  utterance: uniform among the speaker's eligible ones
 *         word 2  start: uniform in [0, lens[u] - seg_len]
 *         word 3  level q_c in hundredths of a dB: c = 0: 1 + [0, 249); c = 1: q_1 = -q_0 (word unused); c >= 2: v in [0, 498),
 *                 q_c = 1 + v for v < 249, -(1 + v - 249) otherwise (uniform magnitude in [1, 250), random sign)
 *     gain[b,c] = w[q_c + 249] * inv_rms[u]: one fp32 multiply.  2 <= C <= 4, S >= C.
 *   ctn_dynmix_gather: the minibatch of a plan (the sampler's or the caller's); mixture [B,T], sources [B,C,T] fp32 (16-byte
 *     aligned), peak [B], T = seg_len.  Every operation is one fp32 rounding, in this order:
 *         s_c[t] = gain[b,c] * corpus[offsets[u_c] + start_c + t]
 *         mix[t] = ((s_0[t] + s_1[t]) + s_2[t]) + ...
 *         a      = max_t max(|mix[t]|, |s_0[t]|, ..., |s_{C-1}[t]|)          (create_wav_2speakers.m:111)
 *         scale  = a > 0 ? 0.9f / a : 1.0f                                   (:112, IEEE division)
 *         mixture[b,t] = scale * mix[t];  sources[b,c,t] = scale * s_c[t];  peak[b] = a
 *     max is order-free, so the outputs are a bitwise function of the plan and the corpus, whatever the launch geometry.
 *     mode 0: two launches of (ceil(T / 1024), B) workgroups (per-workgroup maxima into `workspace`,
 *     ctn_dynmix_gather_workspace() bytes; then the scaled samples); mode 1: one launch of B workgroups that read their
 *     segments twice (no workspace).  Same values.  A plan entry outside its utterance (u outside [0, U), start < 0 or
 *     start + T > lens[u]) is never read: that source counts as silence and peak[b] = -1.
 * The 0-dB level behind inv_rms is the caller's: the plain RMS of the whole utterance (ctn_dynmix_levels) or, as
 * create_wav_2speakers.m:89-97 has it, the ITU-T P.56 active level (ctn_active_level below: inv_rms = 1 / sqrt(level)).
 * Deliberate difference from create_wav_2speakers.m: the peak rescale is per drawn segment, not per whole utterance. */
int ctn_dynmix_levels(const float* corpus, long long num_samples, const long long* offsets, const long long* lens, long long U,
                      double* meansq, void* stream);
int ctn_dynmix_plan(const int* spk_ptr, const int* utt_ids, int S, const long long* lens, const float* inv_rms, const float* w,
                    long long seed, int epoch, int rank, unsigned* step, int B, int C, int seg_len, int* plan_utt,
                    long long* plan_start, int* plan_q, float* gain, void* stream);
size_t ctn_dynmix_gather_workspace(int B, int T);
int ctn_dynmix_gather(const float* corpus, const long long* offsets, const long long* lens, long long U, const int* plan_utt,
                      const long long* plan_start, const float* gain, int B, int C, int T, float* mixture, float* sources,
                      float* peak, void* workspace, size_t workspace_bytes, int mode, void* stream);

/* ---- on-device sinc resampling: corpora at any rate, speed perturbation (csrc/ctn_resample.hip, csrc/ctn_dynmix.hip) ------
 * what librosa.load(path, sr=sample_rate) does for the reference's loaders, for ragged rows in device memory.
 * Filter (designed on the host in fp64, rounded once to fp32: resample.design_filter): up / down in lowest terms,
 *     fc = rolloff * min(1, up / down),  W = ceil(zeros / fc)                 (zeros = 32, rolloff = 0.95, beta = 14.77)
 *     h [up][2W]: for phase p in [0, up) and tap j in [0, 2W), tau = (j - W + 1) - p / up,
 *     h[p][j] = fc * sinc(fc * tau) * I0(beta * sqrt(1 - (tau / W)^2)) / I0(beta), 0 where |tau| >= W   (sinc(v) = sin(pi v) / (pi v));
 *     every phase is then divided by its own sum, so a constant stays constant.
 * Output sample t of a row sits at input position t * down / up: i = floor(t * down / up), p = (t * down) mod up,
 *     y[t] = sum_{j = 0}^{2W - 1} h[p][j] * x[i + j - W + 1]            n_out = ceil(n_in * up / down)
 *     acc = +0; for j ascending: acc = acc + h[p][j] * x[..]: every product and every add is one fp32 rounding (no fused
 *     multiply-add).  x outside [0, n_in) of its OWN row reads as zero.  The output is a bitwise function of the table and the
 *     input, whatever the launch geometry.
 *   ctn_resample_ragged: U rows of one flat buffer x (x_samples floats; in_offsets, in_lens [U] int64 in device memory)
 *     into rows of the flat buffer y (y_samples floats; out_offsets, out_lens [U]), out_lens[r] = ceil(in_lens[r] * up / down).
 *     host_tables [4][U] int64 in HOST memory holds the same four tables (in_offsets, in_lens, out_offsets, out_lens): sizes and
 *     every row are checked against the two buffers before the launch (CTN_ERR_ARG, nothing launched), and the grid is sized
 *     from them.  The kernel checks the device tables again: a row outside its buffer is neither read nor written and
 *     status[r] = -1 (0 otherwise; status [U] int32 may be null).  1 <= up, down <= 2^20, gcd(up, down) = 1, rows of 1 .. 2^40
 *     samples.  One workgroup of 256 threads per 1024 consecutive outputs of a row (fewer where down / up is large) stages
 *     their input span, and the bank when it fits, in LDS.  ctn_resample_span(up, down, W, chunk) = that span in floats,
 *     floor((up - 1 + (chunk - 1) * down) / up) + 2W (0 for arguments out of range, chunk <= 1024).
 *   ctn_dynmix_plan_speed: ctn_dynmix_plan plus a table pct [n] int32 of speed percents in device memory (1 <= n <= 151, every
 *     entry in [50, 200]).  For source c of mixture b ONE MORE Philox block under the same key,
 *         counter = (c + 256, b, step, epoch)        word 0: plan_pct[b,c] = pct[(uint64(word 0) * n) >> 32]
 *     The block (c, b, step, epoch) draws speaker, utterance and level exactly as ctn_dynmix_plan does; its word 2 draws the start
 *     uniform in [0, lens[u] - need] with need = ceil(seg_len * pct / 100), the input samples the segment spans.  Eligible
 *     utterances (spk_ptr / utt_ids): lens[u] >= ceil(seg_len * max(pct) / 100) and meansq[u] > 0.  *step += 1 on the device.
 *   ctn_dynmix_speed_segments: seg [B,C,T] fp32 = the unit-gain segments of a plan with speeds.  Source (b,c) is utterance u
 *     replayed at pct % of its speed: resampled by up / down = 100 / pct in lowest terms, output sample 0 at input sample
 *     plan_start,  seg[b,c,t] = sum_j h[p][j] * x_u[plan_start + i + j - W + 1]  with the sum above; x_u outside [0, lens[u]) reads
 *     as zero, inside it (before plan_start, or past plan_start + need) it reads the utterance.  pct = 100 is a plain copy,
 *     seg[b,c,t] = x_u[plan_start + t], whatever the tables say.  banks: the fp32 tables of all configured percents in one flat
 *     buffer of bank_floats floats; bank_tab [151][4] int32, row pct - 50 = (up, down, W, offset of h in banks), W = 0 for a
 *     percent that is not configured.  span_cap, bank_cap: LDS floats for the input span of 1024 outputs (>= the largest
 *     ctn_resample_span(up, down, W, 1024) configured) and for a staged bank (a bank of more than bank_cap / (2W + 1) phases is
 *     read through the cache); 4 * (span_cap + bank_cap) <= 61440.  An entry that is never read -- u outside [0, U), start < 0,
 *     start + need > lens[u], pct outside [50, 200] or not configured, a table row outside banks -- gives a segment of zeros
 *     and seg_utt[b,c] = -1; every other entry gives seg_utt[b,c] = b * C + c.
 *   The mix: ctn_dynmix_gather over seg as a corpus of B * C utterances of T samples (offsets = arange * T, lens = T), with
 *     plan_utt = seg_utt and plan_start = 0: gains, sum order, peak and the 0.9 rescale are the contract above, both modes, and
 *     a flagged entry gives peak[b] = -1 as there. */
size_t ctn_resample_span(int up, int down, int W, int chunk);
int ctn_resample_ragged(const float* x, long long x_samples, const long long* in_offsets, const long long* in_lens, long long U, int up,
                        int down, const float* h, int W, float* y, long long y_samples, const long long* out_offsets,
                        const long long* out_lens, const long long* host_tables, int* status, void* stream);
int ctn_dynmix_plan_speed(const int* spk_ptr, const int* utt_ids, int S, const long long* lens, const float* inv_rms, const float* w,
                          const int* pct, int n, long long seed, int epoch, int rank, unsigned* step, int B, int C, int seg_len,
                          int* plan_utt, long long* plan_start, int* plan_q, float* gain, int* plan_pct, void* stream);
int ctn_dynmix_speed_segments(const float* corpus, const long long* offsets, const long long* lens, long long U, const int* plan_utt,
                              const long long* plan_start, const int* plan_pct, int B, int C, int T, const float* banks,
                              long long bank_floats, const int* bank_tab, int span_cap, int bank_cap, float* seg, int* seg_utt,
                              void* stream);

/* ---- streaming sinc resampling: the sum above over signals that arrive push by push (csrc/ctn_resample.hip) -----------------
 * `rows` independent streams.  The filter, (i, p) and the tap sum are those of the section above, taken over the WHOLE stream of a
 * row: x before sample 0 and beyond the end of the stream reads as zero, so every output is bitwise what ctn_resample_ragged gives
 * for the whole signal, however it was cut into pushes and whatever the other rows do.  The arithmetic the caller keeps on the host:
 *     after N input samples exactly E(N) = ceil((N - W) * up / down) outputs are computable for N > W, 0 otherwise (output t reads
 *     up to input i_t + W); a push that takes a row from N to N + k samples emits outputs [E(N), E(N + k)); the first tap of output
 *     E(N) is at index >= N - 2W + 1; closing a row emits [E(N), ceil(N * up / down)) with zeros for the missing future.
 * State: hist [2][rows][2W - 1] fp32, the last 2W - 1 samples of every row, twice: a push reads half `parity` and writes the other
 * half, so no workgroup reads what another one of the same launch writes; the caller flips a row's parity after every push with
 * n_new > 0.  A stream starts with n_old = 0 (history entries before sample 0 are never read; zeroing them is the caller's choice).
 *   tab  int64 [rows][CTN_STREAM_RS_TAB] in device memory, rewritten by the caller before every call:
 *        [0] n_old   samples of the row received before this call      [1] n_new   new samples with this call (0: none, a flush)
 *        [2] t0      first output to emit                              [3] n_out   outputs to emit
 *        [4] src     offset of the row's new samples in `chunk`        [5] dst     offset of the row's first output in `y`
 *        [6] parity  half of hist that holds the row's history (0, 1)  [7] spare
 *   ctn_stream_resample: y[dst + k] = output t0 + k of the row for k < n_out, then hist[1 - parity][row] = the last 2W - 1 samples
 *     of the n_old + n_new received (zeros before sample 0) when n_new > 0.  Sample g of the row reads as zero for g < 0 and
 *     g >= n_old + n_new, chunk[src + g - n_old] for g >= n_old, hist[parity][row][g - n_old + 2W - 1] otherwise: the kernel never
 *     touches chunk beyond a row's n_new.  A row with n_new = n_out = 0 is neither read nor written, whatever its other entries.
 *     Every other row needs: all entries >= 0, parity 0 or 1, n_old + n_new <= 2^40, [src, src + n_new) inside chunk
 *     (chunk_samples floats), [dst, dst + n_out) inside y (y_samples floats), t0 + n_out <= ceil((n_old + n_new) * up / down), and
 *     for n_out > 0 the first tap of output t0 inside the history: floor(t0 * down / up) - W + 1 >= n_old - (2W - 1).
 *     host_tab: the same table in HOST memory; every row is checked before the launch (CTN_ERR_ARG, nothing launched) and the grid
 *     is sized from it.  The kernel checks the device table again: a row that breaks the contract is neither read nor written and
 *     status[r] = -1 (0 otherwise; status [rows] int32 may be null).  One workgroup of 256 threads per 1024 consecutive outputs
 *     of a row (fewer where down / up is large) stages the input span, and the bank when it fits, in LDS as ctn_resample_ragged
 *     does, plus one workgroup per row for the history: a long push spreads over the device.  1 <= up, down <= 2^20 in lowest
 *     terms, 1 <= W <= 2^16, 1 <= rows < 2^31.
 *   ctn_stream_carry: buf [rows][ld] fp32; row r moves its samples [off, off + n) to its front, buf[r][k] = buf[r][off + k] for
 *     k < n, off = tab[r][7] (the spare entry of the table above): what a caller that consumes whole hops from the front of
 *     staging rows carries over to the next push.  One workgroup per row reads all n samples before it writes any (the spans may
 *     overlap).  A row with off <= 0 or off + n > ld is left alone.  1 <= n <= 1024, ld >= n. */
#define CTN_STREAM_RS_TAB 8
int ctn_stream_resample(const float* chunk, long long chunk_samples, float* hist, long long rows, int up, int down, const float* h, int W,
                        float* y, long long y_samples, const long long* tab, const long long* host_tab, int* status, void* stream);
int ctn_stream_carry(float* buf, long long ld, long long rows, const long long* tab, int n, void* stream);

/* ---- noisy and reverberant dynamic mixing (csrc/ctn_dynmix_aug.hip) ------------------------------------------------------
 * what WHAM!, WHAMR! and noisy LibriMix add to wsj0-2mix, drawn on the device: a noise recording at a drawn SNR under every
 * mixture, every source convolved with a drawn room impulse response (RIR).  The conventions are those of the two sections
 * above: draws are pure functions of (seed, rank, epoch, step, b) through Philox4x32-10 under the same key, no pow or sqrt on the
 * device, every fp32 operation is one rounding in a stated order, outputs are a bitwise function of plan and data whatever the
 * launch geometry, and an entry that breaks its tables is never read and is flagged.
 * RIR bank: R responses back to back in one flat fp32 buffer of bank_floats floats; rir_offsets [R] int64, rir_lens [R],
 *   rir_direct [R], rir_early [R] int32.  Response r has n_r = rir_lens[r] taps, 1 <= n_r <= 8192; d_r = rir_direct[r] in
 *   [0, n_r) is its direct path (the host takes the first index of max |h|); rir_early[r] in [0, n_r] is the number of leading
 *   taps that make the training target (direct path and early reflections; n_r: the fully reverberant source).  The host may
 *   divide every response by sqrt(sum h^2) in fp64 before the one rounding to fp32 (rir.RirBank(normalize=True)): the
 *   reverberant source then keeps ROUGHLY the level the plan gave it (its RMS; the active level, where the corpus was built with
 *   it, moves with the reverberation's tail) -- a deliberate approximation: exact for white sources only, and the early-taps target is below it by the energy of the late taps.
 * Noise: an ordinary corpus (noise, noise_offsets, noise_lens [Un], noise_inv_rms [Un]; speaker labels play no part).
 *   noise_ids [Nn] int32: the eligible noise utterances, lens[v] >= seg_len and meansq[v] > 0.  SNR in integer tenths of a dB,
 *   lo10 .. lo10 + nsnr - 1 (1 <= nsnr <= 1024), table wn [nsnr] fp32, wn[i] = 10^(-(lo10 + i) / 200) rounded from fp64 on the
 *   host.  The SNR is relative to the sources' 0-dB REFERENCE level -- unit RMS, before the +-q hundredths of a dB the plan gives
 *   each source -- not to the level of the louder source or of their sum.
 *   ctn_dynmix_plan_aug: the extra draws of one minibatch; launched BEFORE ctn_dynmix_plan / ctn_dynmix_plan_speed on the same
 *     stream, it reads *step and leaves it alone (the kernel behind it advances it).  Same key; the blocks at counters
 *     (c, ..) and (c + 256, ..) are not touched, so speaker, utterance, start, level and speed draws of a seed are what they are
 *     without this call.  New blocks:
 *         RIR of source c of mixture b     counter = (c + 512, b, step, epoch)   plan_rir[b,c] = (uint64(word 0) * R) >> 32
 *         noise of mixture b               counter = (768, b, step, epoch)
 *             word 0  noise_utt[b] = v = noise_ids[(uint64(word 0) * Nn) >> 32]
 *             word 1  noise_start[b]: uniform in [0, noise_lens[v] - seg_len]
 *             word 2  k = (uint64(word 2) * nsnr) >> 32,  snr10[b] = lo10 + k
 *         ngain[b] = wn[k] * noise_inv_rms[v]: one fp32 multiply.
 *     plan_rir [B,C] int32; noise_utt, snr10 [B] int32, noise_start [B] int64, ngain [B] fp32.  Either half is skipped when its
 *     pointers are null (plan_rir; the eight noise arrays together); both null is an error.  A noise_ids entry outside [0, Un)
 *     or shorter than seg_len gives noise_utt[b] = -1, ngain[b] = 0: an entry the mix flags.
 *   ctn_dynmix_reverb: rows i in [0, N), N = B * C, of the "corpus + plan" form ctn_dynmix_gather reads.  The dry segment of row
 *     i is x_i[t] = corpus[offsets[u] + plan_start[i] + t] for t in [0, T), u = plan_utt[i], and reads as ZERO outside [0, T):
 *     the reverberation sees the drawn segment only, not the utterance before it -- the same thing as convolving a cut segment,
 *     and what lets the stage run over the speed-perturbed segment buffer as a corpus (seg, offsets = arange * T, lens = T,
 *     plan_utt = seg_utt, plan_start = 0).  With r = plan_rir[i], n = rir_lens[r], d = rir_direct[r], h = bank + rir_offsets[r]:
 *         wet[i,t] = sum_{j=0}^{n-1} h[j] * x_i[t + d - j]
 *         acc = +0; for j ascending: acc = acc + h[j] * x: the product and the add are one fp32 rounding each
 *         tgt[i,t] = acc after the taps j < rir_early[r]                    (so tgt == wet where rir_early[r] == n)
 *     wet, tgt [N,T] fp32 at unit gain (16-byte aligned); tgt may be null (then only wet is computed).  The shift by d keeps the
 *     target time-aligned with the dry source.  Taps whose sample lies outside [0, T) may be skipped or added as zeros: acc
 *     starts at +0 and can never become -0, so both give the same bits.  A row is written as zeros with out_utt[i] = -1 when its
 *     plan entry is outside its utterance (u outside [0, U) -- a segment the speed stage flagged has u = -1 --, start < 0,
 *     start + T > lens[u]), plan_rir[i] is outside [0, R), or the response's table entry is outside the bank buffer or breaks
 *     1 <= n <= 8192, 0 <= d < n, 0 <= early <= n; every other row gives out_utt[i] = i.  One workgroup of 256 threads per 1024
 *     consecutive outputs of a row, 4 per thread in registers; taps are staged in LDS 1024 at a time beside their input span.
 *   ctn_dynmix_gather_aug: ctn_dynmix_gather (chunked form, two launches, ctn_dynmix_gather_workspace() bytes) with targets that
 *     differ from the mixture components and a noise row.  tgt_corpus: same layout and plan as corpus (null: the targets are the
 *     mixture components); noise null: no noise, and no noise term in the sum.
 *         r_c[t] = gain[b,c] * corpus[..]        g_c[t] = gain[b,c] * tgt_corpus[..]        (g_c = r_c when tgt_corpus is null)
 *         n[t]   = ngain[b] * noise[noise_offsets[v] + noise_start[b] + t]                  v = noise_utt[b]
 *         mix[t] = (((r_0[t] + r_1[t]) + r_2[t] ...) + n[t])
 *         a      = max_t max(|mix[t]|, |g_0[t]|, ..., |g_{C-1}[t]|)          scale = a > 0 ? 0.9f / a : 1.0f
 *         mixture[b,t] = scale * mix[t];  sources[b,c,t] = scale * g_c[t];  peak[b] = a
 *     A source entry outside its utterance (as ctn_dynmix_gather defines it; both r_c and g_c) or a noise entry outside its
 *     utterance (v outside [0, Un), start < 0, start + T > noise_lens[v]) is never read, counts as silence and gives peak[b] = -1.
 *   The pipeline of one step: plan_aug -> plan | plan_speed -> speed_segments (with speeds) -> reverb over the corpus or over seg
 *     (with RIRs) -> gather_aug over (wet, tgt) as corpora of B * C utterances of T samples, plan_utt = out_utt, plan_start = 0. */
int ctn_dynmix_plan_aug(long long seed, int epoch, int rank, const unsigned* step, int B, int C, int seg_len, int R, int* plan_rir,
                        const int* noise_ids, int Nn, const long long* noise_lens, long long Un, const float* noise_inv_rms,
                        const float* wn, int nsnr, int lo10, int* noise_utt, long long* noise_start, int* snr10, float* ngain,
                        void* stream);
int ctn_dynmix_reverb(const float* corpus, const long long* offsets, const long long* lens, long long U, const int* plan_utt,
                      const long long* plan_start, int N, int T, const float* bank, long long bank_floats, const long long* rir_offsets,
                      const int* rir_lens, const int* rir_direct, const int* rir_early, int R, const int* plan_rir, float* wet, float* tgt,
                      int* out_utt, void* stream);
int ctn_dynmix_gather_aug(const float* corpus, const long long* offsets, const long long* lens, long long U, const int* plan_utt,
                          const long long* plan_start, const float* gain, int B, int C, int T, const float* tgt_corpus,
                          const float* noise, const long long* noise_offsets, const long long* noise_lens, long long Un,
                          const int* noise_utt, const long long* noise_start, const float* ngain, float* mixture, float* sources,
                          float* peak, void* workspace, size_t workspace_bytes, void* stream);

/* ---- long-recording separation: segments framed and stitched on the device (csrc/ctn_longform.hip) -------------------------
 * what users of the non-causal gLN model do with a meeting or a podcast: cut it into overlapping segments of the training length,
 * separate the segments as a batch, bring every segment's speakers into the order of its predecessor by comparing the overlaps
 * (PIT leaves the order arbitrary per segment), and cross-fade.  R recordings at the model's rate; segment length seg, hop hop,
 * overlap ov = seg - hop with 1 <= ov <= hop, so hop < seg <= 2 * hop: never more than two segments over one sample.
 * Segments of a recording of T >= 1 samples: n = 1 if T <= seg, else n = 1 + ceil((T - seg) / hop) (ctn_longform_nseg; 0 for
 *   arguments out of range).  Segment i covers samples [i * hop, i * hop + seg) and reads zero at and beyond T; only the last one
 *   is ever padded: (n - 2) * hop + seg < T and (n - 1) * hop < T.  All recordings' segments form one list of Nseg rows;
 *   seg_ptr [R + 1] int64 gives each recording's range (seg_ptr[0] = 0, seg_ptr[R] = Nseg).
 * Framing (ctn_longform_frame): segs[s, u] = x[in_off[r] + i * hop + u] where i * hop + u < T[r], else +0, for s = seg_ptr[r] + i.
 *   Bit copies.  segs [Nseg][seg] fp32.
 * Costs (ctn_longform_costs): for every segment i >= 1 of a recording and speakers a, b < C,
 *       cost[s, a, b] = sum_{t < ov} (est[s - 1, a, hop + t] - est[s, b, t])^2          est [Nseg][C][seg], cost [Nseg][C][C] fp32
 *   in a fixed order that does not depend on the launch geometry: d = prev - cur, q = d * d, acc[j] = acc[j] + q, three separate
 *   fp32 roundings (no fused multiply-add).  There are 1024 partial sums: acc[t mod 1024] takes the elements t in ascending order,
 *   starting from +0; then for s = 512, 256, ..., 1: acc[j] += acc[j + s] for j < s; cost = acc[0].  Rows of first segments
 *   are written as zeros.
 * Order (ctn_longform_order): perms = the C! permutations in lexicographic (itertools) order, 2 <= C <= 4.  q_s = the first k
 *   that minimises sum_a cost[s, a, perms[k][a]], the sum taken in fp32 from +0 with a ascending; a strict < keeps the earlier k
 *   on a tie (and k = 0 when a sum is NaN).  g[first segment] = identity, g[s][a] = perms[q_s][ g[s - 1][a] ]: g[s][a] is the
 *   local channel of segment s that carries output channel a.  g [Nseg][C] int32.  A recording's chain is a scan of permutations.
 * Assembly (ctn_longform_assemble): for output channel a and sample t < T: i = min(t div hop, n - 1), u = t - i * hop.
 *       i >= 1 and u < ov:   out = fo[u] * est[i - 1, g[i - 1][a], hop + u] + fi[u] * est[i, g[i][a], u]
 *                            two products and one sum, each one fp32 rounding, in that order
 *       otherwise            out = the bit copy of est[i, g[i][a], u]
 *   fi, fo [ov] fp32 tables designed on the host in fp64 and rounded once (longform.fade_tables):
 *       'linear'  fi[u] = (u + 0.5) / ov                     fo[u] = 1 - (u + 0.5) / ov
 *       'hann'    fi[u] = sin^2(pi * (u + 0.5) / (2 * ov))   fo[u] = 1 - that
 *   Channel a of recording r starts at out_off[r] + a * T[r] in the flat buffer out (out_samples floats).  Nothing outside those
 *   ranges is written.  An entry of g outside [0, C) never forms an address: what would have read it -- that channel of the segment's
 *   own samples, and of the chunk of its successor that holds the cross-fade -- is left unwritten.
 * Conventions (those of ctn_resample_ragged): plain pointers and an explicit stream; seg_ptr, T, in_off / out_off as int64 in
 *   device memory; host_tables in HOST memory = seg_ptr [R + 1], T [R], in_off or out_off [R] back to back (host_seg_ptr: the
 *   first of the three), checked against the contract and the buffer sizes before anything is launched (CTN_ERR_ARG), the grid
 *   sized from them.  The kernels check the device copy again: a recording whose range, length or offset breaks the contract is
 *   neither read nor written and status[r] = -1 (0 otherwise; status [R] int32 may be null).  1 <= R <= Nseg < 2^31,
 *   seg <= 2^30, T <= 2^40.  The C ABI takes any seg and hop within 1 <= ov <= hop; 16-byte loads and stores are used where the
 *   addresses allow (seg and hop multiples of 4 on 16-byte aligned buffers), 4-byte ones elsewhere, with the same bits.
 *   256-thread workgroups: one per 2048 samples of a segment (frame, assemble), one per segment pair (costs: the 2 * C overlap
 *   rows are loaded once for all C * C costs, the tree runs through LDS), one per recording (order).  No atomics. */
long long ctn_longform_nseg(long long T, int seg, int hop);
int ctn_longform_frame(const float* x, long long x_samples, const long long* seg_ptr, const long long* T, const long long* in_off,
                       long long R, long long Nseg, int seg, int hop, float* segs, const long long* host_tables, int* status,
                       void* stream);
int ctn_longform_costs(const float* est, const long long* seg_ptr, long long R, long long Nseg, int C, int seg, int hop, float* cost,
                       const long long* host_seg_ptr, void* stream);
int ctn_longform_order(const float* cost, const long long* seg_ptr, long long R, long long Nseg, int C, int* g,
                       const long long* host_seg_ptr, int* status, void* stream);
int ctn_longform_assemble(const float* est, const int* g, const long long* seg_ptr, const long long* T, const long long* out_off,
                          long long R, long long Nseg, int C, int seg, int hop, const float* fi, const float* fo, float* out,
                          long long out_samples, const long long* host_tables, int* status, void* stream);

/* ---- STOI / ESTOI intelligibility scores in fp64 (csrc/ctn_stoi.hip) ---------------------------------------------------------
 * C. H. Taal, R. C. Hendriks, R. Heusdens, J. Jensen, "An Algorithm for Intelligibility Prediction of Time-Frequency Weighted Noisy
 * Speech", IEEE TASLP 19(7), 2011 (STOI) and J. Jensen, C. H. Taal, "An Algorithm for Predicting the Intelligibility of Speech
 * Masked by Modulated Noise Maskers", IEEE/ACM TASLP 24(11), 2016 (ESTOI), with the conventions of the authors' MATLAB code and of
 * pystoi.  Constants: 10 kHz input, frames of 256 at hop 128 starting at i < n - 256 (strict: the frame that ends on the last
 * sample is dropped), window hanning(258)[1:-1], 512-point DFT, 15 third-octave bands from 150 Hz (bins 7 .. 218), segments of
 * 30 frames, beta = -15 dB, 40 dB dynamic range, eps = DBL_EPSILON, 1e-5 for fewer than 30 frames.
 * ref: [B,C,T] fp32 references, est: [B,E,T] fp32 estimate rows (the mixture can be one more row: the anchor in the same call),
 * lengths: [B] int64, all ALREADY AT 10 kHz; samples at t >= lengths[b] are never read.  C >= 1, E >= 1, 1 <= T <= 2^30.  All
 * arithmetic fp64 from the fp32 samples, every reduction in a fixed order that depends on the utterance alone (bitwise the same
 * in any batch); no host read-back, no synchronisation, no atomics: graph-capturable.  NF = ctn_stoi_max_frames(T) =
 * max(1, first-pass frames of T samples), MF = max(1, NF - 1).
 *   ctn_stoi_eval: everything below in one call -> d_stoi, d_estoi [B,E,C] fp64 (estimate e against reference c), m_out, k_out
 *     [B,E,C] int32 (nullable): the frames M after silent-frame removal and the kept first-pass frames K of that pair.
 *     workspace: ctn_stoi_workspace() bytes.
 * The stages, each on caller buffers:
 *   ctn_stoi_frames: per reference row energy [B,C,NF] = 20 log10(||w * frame|| + eps) (0 beyond the row's frames), the keep
 *     mask energy > max - 40 and its exclusive scan: keep_idx [B,C,NF] int32 = the kept frame indices in order (-1 beyond
 *     them), kcount [B,C] int32 = K.  The mask belongs to the reference: an estimate paired with reference c uses c's table.
 *   ctn_stoi_bands: env [B, C + E*C, 15, MF] fp64: set c < C = reference c, set C + e*C + c = estimate e compacted by the table of
 *     reference c.  The compacted signal (overlap-add of the kept windowed frames at hop 128) is rebuilt on the fly, framed and
 *     windowed again, its DFT taken as a DFT-matrix product on v_mfma_f64_16x16x4_f64; env = sqrt of the band sums of |X|^2.
 *     Frame m < M = max(K - 1, 0) of a set is written, nothing beyond.
 *   ctn_stoi_score: per pair and segment the 15 x 30 normalise / clip / correlate of STOI and the row / column normalisation
 *     of ESTOI in one pass, then the sum over segments -> d; M < 30 gives 1e-5 for both.  workspace: ctn_stoi_score_workspace().
 * Arguments are checked before any launch (CTN_ERR_ARG); the workspace functions return 0 for arguments out of range. */
#define CTN_STOI_FS 10000
#define CTN_STOI_FRAME 256
#define CTN_STOI_HOP 128
#define CTN_STOI_NFFT 512
#define CTN_STOI_BANDS 15
#define CTN_STOI_SEGMENT 30
int ctn_stoi_max_frames(long long T);
size_t ctn_stoi_workspace(long long B, int C, long long E, long long T);
int ctn_stoi_eval(const float* ref, const float* est, const long long* lengths, long long B, int C, long long E, long long T,
                  double* d_stoi, double* d_estoi, int* m_out, int* k_out, void* workspace, size_t workspace_bytes, void* stream);
int ctn_stoi_frames(const float* ref, const long long* lengths, long long B, int C, long long T, double* energy, int* keep_idx,
                    int* kcount, void* stream);
int ctn_stoi_bands(const float* ref, const float* est, const long long* lengths, const int* keep_idx, const int* kcount,
                   long long B, int C, long long E, long long T, double* env, void* stream);
size_t ctn_stoi_score_workspace(long long B, int C, long long E, long long T);
int ctn_stoi_score(const double* env, const int* kcount, long long B, int C, long long E, long long T, double* d_stoi,
                   double* d_estoi, int* m_out, int* k_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- STOI / ESTOI as a training loss: the backward pass in fp64 (csrc/ctn_stoi_grad.hip) -----------------------------------------
 * The gradient of the scores above with respect to the ESTIMATE's samples (M. Kolbaek et al., "Monaural Speech Enhancement Using
 * Deep Neural Networks by Maximizing a Short-Time Objective Intelligibility Measure", ICASSP 2018; S.-W. Fu et al., "End-to-End
 * Waveform Utterance Enhancement for Direct Evaluation Metrics Optimization", IEEE/ACM TASLP 26(9), 2018).  Only chosen pairs are
 * differentiated: est_of_ref [B,C] int32 on the device pairs reference c of utterance b with estimate row est_of_ref[b,c] (clamped
 * to [0, E); the rows need not form a permutation).  A pair is laid out as an utterance of its own: P = B * C pair rows p = b C + c
 * of one reference and one estimate, so the stage buffers are those of the forward stages called with (B, C, E) = (P, 1, 1):
 * keep_idx [P,NF], kcount [P], env [P,2,15,MF] (set 0 the reference, set 1 the estimate), and the forward values are bitwise
 * ctn_stoi_eval's for that pair.  Everything that depends on the reference alone is constant (energies, keep mask, index table,
 * reference envelopes, clip bound); a cell the forward clipped (alpha y > bound) passes nothing through alpha y, the dependence
 * of alpha on y is differentiated; a norm or an envelope that is exactly 0 passes 0; the eps terms are the forward's; a pair with
 * M < 30 has gradient 0; samples at t >= lengths[b] are never read and get gradient 0.  All arithmetic fp64, every sum in a fixed
 * order that depends on the pair alone; no atomics, no host read-back, no synchronisation: graph-capturable.
 *   ctn_stoi_score_bwd: g_env [P,15,MF] fp64 = d(w_stoi[p] stoi_p + w_estoi[p] estoi_p) / d env[p,1] (0 at frames >= M); w_stoi,
 *     w_estoi [P] fp64 on the device; a weight of 0 skips that measure.  One thread per segment writes the 15 x 30 cell gradients
 *     of its segment, a second kernel sums the segments over a frame in ascending order.  workspace: ctn_stoi_score_bwd_workspace().
 *   ctn_stoi_bands_bwd: g10 [P,T] fp64, the gradient with respect to the pair's 10 kHz estimate row est_p [P,T] fp32 (lengths_p
 *     [P] int64).  The compacted windowed frames are rebuilt and their spectra recomputed as in ctn_stoi_bands; g_X = g_env X / env;
 *     the transposed DFT-matrix product on v_mfma_f64_16x16x4_f64; then window, overlap-add and compaction are undone in gather
 *     form (ascending frame order).  workspace: ctn_stoi_bands_bwd_workspace().
 *   ctn_resample_rows_adjoint_f64: g_est [B,E,T] fp32 (and g_sum [B,E,T] fp64, nullable: the value before the one rounding):
 *     g_est[b,e,i] = sum over c with est_of_ref[b,c] = e, ascending, of sum_t h[(t down) % up][i - (t down) / up + W - 1] g10[b,c,t],
 *     t ascending, fp64 fused multiply-adds: the transpose of ctn_resample_ragged's tap table h [up, 2W] as a linear map from T
 *     samples to T10 = ceil(T up / down).  lengths [B] are at the estimate's rate; i >= lengths[b] gives 0.  up = down = 1
 *     (T10 = T, h unused): the sum over c alone.  It needs no workspace: ctn_resample_rows_adjoint_workspace() is 0 for every size
 *     and stands beside the other stages' workspace functions.
 *   ctn_stoi_pairs_fwd: ref [B,C,T], est [B,E,T], lengths [B], all at 10 kHz -> d_stoi, d_estoi [B,C] fp64, m_out [B,C] int32
 *     (nullable); workspace (ctn_stoi_pairs_workspace(B, C, T) bytes) keeps what the backward pass needs.
 *   ctn_stoi_pairs_bwd: score, bands and adjoint in one call from the forward's workspace (sized for T10) -> g_est [B,E,T] at the
 *     estimate's own rate; workspace: ctn_stoi_pairs_bwd_workspace(B, C, T10).
 * B * C <= 65535, B * E <= 65535, C <= 64, T, T10 <= 2^30, up / down in lowest terms.  Arguments are checked before any launch. */
size_t ctn_stoi_score_bwd_workspace(long long P, long long T);
int ctn_stoi_score_bwd(const double* env, const int* kcount, const double* w_stoi, const double* w_estoi, long long P, long long T,
                       double* g_env, void* workspace, size_t workspace_bytes, void* stream);
size_t ctn_stoi_bands_bwd_workspace(long long P, long long T);
int ctn_stoi_bands_bwd(const float* est_p, const long long* lengths_p, const int* keep_idx, const int* kcount, const double* env,
                       const double* g_env, long long P, long long T, double* g10, void* workspace, size_t workspace_bytes,
                       void* stream);
size_t ctn_resample_rows_adjoint_workspace(long long B, int C, long long E, long long T);
int ctn_resample_rows_adjoint_f64(const double* g10, const int* est_of_ref, const long long* lengths, long long B, int C, long long E,
                                  long long T, long long T10, int up, int down, const float* h, int W, float* g_est, double* g_sum,
                                  void* stream);
size_t ctn_stoi_pairs_workspace(long long B, int C, long long T);
size_t ctn_stoi_pairs_bwd_workspace(long long B, int C, long long T);
int ctn_stoi_pairs_fwd(const float* ref, const float* est, const long long* lengths, const int* est_of_ref, long long B, int C,
                       long long E, long long T, double* d_stoi, double* d_estoi, int* m_out, void* workspace,
                       size_t workspace_bytes, void* stream);
int ctn_stoi_pairs_bwd(const void* fwd_workspace, size_t fwd_workspace_bytes, const double* w_stoi, const double* w_estoi,
                       const int* est_of_ref, const long long* lengths, long long B, int C, long long E, long long T, long long T10,
                       int up, int down, const float* h, int W, float* g_est, void* workspace, size_t workspace_bytes, void* stream);

/* ---- mixture invariant training loss (csrc/ctn_mixit.hip) --------------------------------------------------------------------
 * S. Wisdom et al., "Unsupervised Sound Separation Using Mixture Invariant Training", NeurIPS 2020 (MixIT), with the paper's
 * soft-thresholded SNR (no mean removal: SNR, not SI-SNR).  mixtures: [B,2,T] fp32, the two reference mixtures; estimates:
 * [B,M,T] fp32, 2 <= M <= 8, NOT modified; lengths: [B] int64, clamped to [0, T], only t < len counts; tau = 10^(-snr_max/10)
 * >= 0 (0: no threshold).  An assignment a in [0, 2^M) sends source i to mixture (a >> i) & 1 (a mixture may get no source):
 *     err_n = sum_t (sum_{i in A_n} e_i - x_n)^2,  Xx_n = sum_t x_n^2,  l_n = 10 log10((err_n + tau Xx_n + 1e-8) / (Xx_n + 1e-8)),
 *     L(a) = (l_0 + l_1) / 2;  assign [B] int64 = the first a, ascending, that attains min_a L(a) (fp64, strict <),
 *     per_utt [B] = L(assign), snr [B,2] = -l_n(assign), loss [1] = mean_b per_utt (fp64 mean, rounded once),
 *     coef [B,2] = c_n = (10 / ln 10) / (err_n + tau Xx_n + 1e-8): the backward table.  len = 0: per_utt = 0, assign = 0.
 * Forward: one sweep collects the fp64 moments G = e e^T (upper triangle), Xe = x e^T and Xx per utterance and time chunk
 * (ctn_sisnr_chunks(T) chunks: the partition depends on T alone, so an utterance's result is bitwise the same in any batch, at
 * any batch index and for any pointer alignment), then the 2^M assignments are scored on those scalars.  Rows are read 16 bytes
 * per lane when T % 4 == 0 and the base pointers are 16-byte aligned.  workspace: ctn_mixit_workspace() bytes (0: bad sizes).
 * Backward: d_estimates[b,i,t] = [t < len] * scale_b * c_n * (sum_{k in A_n} e_k[t] - x_n[t]), n = bit i of assign[b], the
 * remix added in fp32 in ascending k; scale_b = g_loss[0] / B + g_per[b] for upstream gradients g_loss [1] of loss and g_per [B]
 * of per_utt (either may be NULL).  Fixed-order reductions, no atomics, no read-back, no synchronisation: graph-capturable.
 * Arguments are checked before any launch (CTN_ERR_ARG). */
size_t ctn_mixit_workspace(int B, int M, int T);
int ctn_mixit_fwd(const float* mixtures, const float* estimates, const long long* lengths, int B, int M, int T, double tau,
                  float* per_utt, long long* assign, float* snr, float* loss, float* coef, void* workspace,
                  size_t workspace_bytes, void* stream);
int ctn_mixit_bwd(const float* mixtures, const float* estimates, const long long* lengths, const long long* assign,
                  const float* coef, const float* g_loss, const float* g_per, int B, int M, int T, float* d_estimates,
                  void* stream);

/* ---- PIT with inactive sources: variable speaker counts (csrc/ctn_varpit.hip) ---------------------------------------------------
 * A C-output model trained on mixtures of 1 .. C speakers: S. Wisdom et al., "What's all the FUSS about free universal sound
 * separation data?", ICASSP 2021.  sources: [B,C,T] fp32, a reference row may be all zeros; estimates: [B,C,T] fp32, NOT modified;
 * lengths: [B] int64, clamped to [0, T], only t < len counts; 2 <= C <= 6; perms: [C!,C] int32 in itertools.permutations order,
 * nperm = C!, perm[i] = j pairs estimate i with reference j; tau = 10^(-snr_max/10) >= 0, tau0 = 10^(-inactive_snr_max/10) >= 0.
 * Moments over t < len, no mean removal (SNR, not SI-SNR):
 *     Ss_j = sum s_j^2,  Ee_i = sum e_i^2,  Es_ij = sum e_i s_j,  Xx = sum_t (sum_j s_j[t])^2  (inner sum in fp64, ascending j):
 *     the energy of the clean mixture, so the criterion needs nothing beyond (sources, estimates, lengths).
 * Reference j is active iff Ss_j > 0.  Pair losses:
 *     active:    l_ij = 10 log10((max(Ss_j - 2 Es_ij + Ee_i, 0) + tau Ss_j + 1e-8) / (Ss_j + 1e-8))
 *     inactive:  l_ij = 10 log10((Ee_i + tau0 Xx + 1e-8) / (Xx + 1e-8))                 (the same value for every inactive j)
 *     L(p) = (sum_i l_{i,p(i)}) / C in fp64, ascending i;  perm_idx [B] int64 = the first p in table order that attains min_p L(p)
 *     (strict <).  Permutations that differ only in which inactive reference an output takes add the same values in the same
 *     order: their sums are bitwise equal, the tie is exact and the first one wins.
 *     per_utt [B] = L(perm_idx), pair [B,C,C] = l as fp32, active [B,C] int32, loss [1] = mean_b per_utt (fp64 mean, rounded once),
 *     coef [B,C,2] = (c_i, a_i): c_i = (20 / ln 10) / D_i with D_i the numerator argument of the chosen pair of estimate i, a_i = 1
 *     for an active reference and 0 for an inactive one: the backward table.  len = 0: per_utt = 0, perm_idx = 0.
 * Forward: one sweep collects the C^2 + 2C + 1 fp64 moments per utterance and time chunk (ctn_sisnr_chunks(T) chunks: the
 * partition depends on T alone, so an utterance's result is bitwise the same in any batch, at any batch index and for any
 * pointer alignment), then one wave per utterance scores the C! permutations on those scalars.  Rows are read 16 bytes per lane
 * when T % 4 == 0 and the base pointers are 16-byte aligned.  workspace: ctn_varpit_workspace() bytes (0: bad sizes).
 * Backward: d_estimates[b,i,t] = [t < len] * (scale_b / C) * c_i * (e_i[t] - a_i s_j[t]), j = perms[perm_idx[b]][i]; scale_b =
 * g_loss[0] / B + g_per[b] for upstream gradients g_loss [1] of loss and g_per [B] of per_utt (either may be NULL); every fp32
 * operation rounded once.  Fixed-order reductions, no atomics, no read-back, no synchronisation: graph-capturable.
 * Arguments are checked before any launch (CTN_ERR_ARG). */
size_t ctn_varpit_workspace(int B, int C, int T);
int ctn_varpit_fwd(const float* sources, const float* estimates, const long long* lengths, const int* perms, int nperm, int B,
                   int C, int T, double tau, double tau0, float* per_utt, long long* perm_idx, float* pair, int* active,
                   float* loss, float* coef, void* workspace, size_t workspace_bytes, void* stream);
int ctn_varpit_bwd(const float* sources, const float* estimates, const long long* lengths, const int* perms,
                   const long long* perm_idx, const float* coef, const float* g_loss, const float* g_per, int B, int C, int T,
                   float* d_estimates, void* stream);

/* ---- variable speaker counts in the dynamic mixer (csrc/ctn_dynmix_active.hip) ---------------------------------------------------
 * ctn_dynmix_plan_active: n_active[b] = min_speakers + below(r.w[0], C - min_speakers + 1) with r = philox4x32_10(1024, b, step,
 *   epoch, k0, k1), key and below() as in ctn_dynmix_plan; 1 <= min_speakers <= C.  The c0 words 0 .. 3, 256 + c, 512 + c and 768
 *   belong to the other draws, which are untouched.  Launched BEFORE ctn_dynmix_plan / ctn_dynmix_plan_speed on the same stream:
 *   it reads the step word and leaves it alone.
 * ctn_dynmix_mask_active: gain[b,c] = +0 for c >= n_active[b], launched behind the plan.  The gather, speed, reverberation and
 *   noise kernels then run unchanged: a masked source row is zeros and adds nothing to the mixture or its peak. */
int ctn_dynmix_plan_active(long long seed, int epoch, int rank, const unsigned* step, int B, int C, int min_speakers, int* n_active,
                           void* stream);
int ctn_dynmix_mask_active(const int* n_active, int B, int C, float* gain, void* stream);

/* ---- active speech level, ITU-T P.56 method B (csrc/ctn_levels.hip) ---------------------------------------------------------------
 * what tools/matlab-code/create_wav_2speakers.m:89-97 normalises every source with (activlev(s, fs, 'n'), default mode), for U
 * ragged utterances in device memory: samples [num_samples] fp32, offsets [U], lens [U] int64 as for ctn_dynmix_levels.
 * Of utterance u the device produces  ssq [U] fp64, ns [U] int64, emax [U] int32, counts [U, 20] int64;  the level itself is a
 * few fp64 operations per utterance on the host (levels.level_from_counts).  For one utterance x[0 .. len), all in fp64:
 *   padding   nz zeros are appended (ceil(0.35 fs)); N = len + nz samples are processed and ns = N.
 *   band      x -> y through a first-order section, two biquads and, if use_lp, one 5th-order section (the 200 Hz high-pass and
 *             the 5.5 kHz low-pass, 5th-order Chebyshev-II, designed on the host: levels.design), every section direct form II
 *             transposed from zero state, every product and every sum ONE rounding, no contraction, in this order:
 *                 first order   y = b0 x + z0;  z0 = b1 x - a1 y
 *                 biquad        y = b0 v + z1;  z1 = (b1 v + z2) - a1 y;  z2 = b2 v - a2 y                  (v: the section's input)
 *                 5th order     y = b0 v + z1;  zk = (bk v + z(k+1)) - ak y, k = 1 .. 4;  z5 = b5 v - a5 y
 *   energy    p = p + y y per sample, in order, from 0 at the start of every chunk; ssq = ((0 + p_0) + p_1) + ..., chunks ascending.
 *   envelope  s = b0 |y| + z1;  z1 = z2 - a1 s;  z2 = -(a2 s)      (b0 = (1 - g)^2, a1 = -2 g, a2 = g^2, g = exp(-1 / (0.03 fs)))
 *   exponent  e[n] = the frexp exponent of the one-rounding product s s (fp64 denormals kept); -32768 stands for -inf where it is 0.
 *   hangover  h[n] = max e[n - nh + 1 .. n], indices below 0 absent (nh = ceil(0.2 fs) + 1;  CH <= nh <= 9601: the device form
 *             splits a window once, at a chunk seam, so a window shorter than a chunk is CTN_ERR_ARG: rates from 5.12 kHz up).
 *   bins      emax = max h + 1 (-32767 if every e is -inf);  counts[j - 1] = the samples with j = min(emax - h[n], 20), j = 1 .. 20.
 * The device form: an utterance is cut into chunks of CH = ctn_active_level_chunk() samples by its own sample index.  Every chunk
 * runs from zero state and leaves its end state z_c (band: 5 values, 10 with the low-pass, in section order; envelope: 2); one
 * carry per utterance forms the true start states
 *     s_0 = 0;   s_(c+1)[r] = (((T[r][0] s_c[0] + T[r][1] s_c[1]) + ...) + T[r][S-1] s_c[S-1]) + z_c[r]
 * with T = A^CH (column k: the state CH zero-input samples after the unit state e_k) from the host; then every chunk is rerun from
 * s_c.  By linearity that is the sequential filter in exact arithmetic; in fp64 it is THIS computation (tests/levels_oracle.py
 * restates both).  No pow, tan, exp or log on the device.
 * table [131] fp64: [0,3) first-order b0 b1 a1; [3,8), [8,13) biquads b0 b1 b2 a1 a2; [13,24) 5th-order b0..b5 a1..a5 (zeros without
 * it); [24,27) envelope b0 a1 a2; [27,127) T of the band filter, row-major S x S (S = 5 or 10); [127,131) T of the envelope.
 * chunk_ptr [U + 1] int64: chunk_ptr[0] = 0, chunk_ptr[u + 1] - chunk_ptr[u] = ceil((lens[u] + nz) / CH), total_chunks = chunk_ptr[U].
 * Determinism: counts and maxima are integers (their atomics are order-free) and ssq has the fixed order above, so
 * (ssq, ns, emax, counts) of an utterance is a bitwise function of its own samples, the table, nz, nh and CH: independent of the
 * neighbours, of U, of the launch geometry and of how a caller groups utterances into calls to bound the workspace.
 * An entry outside the buffer (offset < 0, len < 0, offset + len > num_samples) or a chunk range that is not the one its length asks
 * for is never read: ns[u] = -1, ssq = 0, emax = -32767, counts = 0, and nothing else changes.
 * workspace: ctn_active_level_workspace(total_chunks, U) bytes (8-byte aligned; 2 bytes per sample for the exponents, the chunk
 * states and energy partials; a function of total_chunks alone, U is only checked to be positive).  U <= total_chunks <= 2^24 - 1
 * per call (one workgroup per chunk in the last launch: 17 G samples, a workspace of 36 GB; group the utterances beyond that).
 * Six launches on `stream`; bad sizes are CTN_ERR_ARG before any launch. */
int ctn_active_level_chunk(void);
size_t ctn_active_level_workspace(long long total_chunks, long long U);
int ctn_active_level(const float* samples, long long num_samples, const long long* offsets, const long long* lens,
                     const long long* chunk_ptr, long long U, long long total_chunks, const double* table, int use_lp, int nz, int nh,
                     double* ssq, long long* ns, int* emax, long long* counts, void* workspace, size_t workspace_bytes, void* stream);

/* ---- optimal-assignment PIT: the SI-SNR loss for 2 .. 16 speakers, and the assignment solver (csrc/ctn_assign.hip) ---------------
 * The loss of ctn_sisnr_pit_fwd with the C! enumeration replaced by an exact linear-assignment solver (Kuhn's Hungarian method in
 * its shortest-augmenting-path form with row and column potentials, O(C^3)), as in Dovrat, Nachmani & Wolf, "Many-speakers single
 * channel speech separation with optimal permutation training", 2021.  source, estimate: [B,C,T] fp32, 2 <= C <= 16; the estimate is
 * NOT modified (unlike ctn_sisnr_pit_fwd's in-place mask); lengths: [B] int64, clamped to [0, T], only t < len counts.
 *   pair    [B,C,C] fp32   pair[b,i,j] = (float) snr_ij, the SI-SNR in dB of estimate i against reference j: ctn_sisnr_pit_fwd's
 *                          algebra on the centred fp64 moments, with its three EPS
 *   perm    [B,C] int32    perm[b,i] = j: estimate i is matched to reference j; the permutation maximising sum_i pair[b,i,perm[i]]
 *                          over the STORED fp32 values widened to fp64, so perm is a function of pair alone
 *   max_snr [B] fp32       (float)((sum_i snr_{i,perm[i]} in fp64, ascending i) / C): one rounding
 *   loss    [1] fp32       -(float)(mean_b of the fp64 values above, in a fixed order)
 *   coef    [B,C,4] fp32   {A, B, mean e_i, mean s_j} of the matched pairs, for the backward pass
 * The solver: rows enter in index order; a row's search grows an alternating tree over the reduced costs (c_ij - u_i) - v_j with
 * c = -score when maximising, each step taking the FIRST column of least slack, until it meets a free column, and the path is
 * flipped.  Its arithmetic is fp64 additions, subtractions and comparisons only, so tests/assign_oracle.py's solve() gives the same
 * permutation bit for bit, ties included.  Every loop has a trip count fixed by C (at most C search steps per row, at most C
 * steps back): NaN or infinite scores still end with some valid permutation.
 * Forward: one sweep collects the 4C + C^2 fp64 moments per utterance and time chunk (ctn_sisnr_chunks(T) chunks; the cross
 * moments on v_mfma_f64_16x16x4_f64 from tiles staged through LDS, 16-byte loads when T % 4 == 0 and the bases are aligned), then
 * one wave per utterance sums the chunks, scores the pairs and solves.  An utterance's results are bitwise the same in any batch,
 * at any batch index and for any pointer alignment.  workspace: ctn_sisnr_assign_workspace() bytes (0: bad sizes).
 * Backward: d_estimate[b,i,t] = [t < len] * scale_b * (A (s_j[t] - mean s_j) + B (e_i[t] - mean e_i)), j = perm[b,i], scale_b =
 * (-g_loss[0] / B + g_max[b]) / C for upstream gradients g_loss [1] and g_max [B] (either may be NULL); every fp32 operation rounded
 * once.  Fixed-order reductions, no atomics, no read-back, no synchronisation: graph-capturable.
 * ctn_assign_solve: the same device routine over N matrices score [N,C,C] fp32, 1 <= C <= 16, maximising (maximize != 0) or
 * minimising -> perm [N,C] int32, one wave per matrix.
 * Arguments are checked before any launch (CTN_ERR_ARG, CTN_ERR_WORKSPACE). */
size_t ctn_sisnr_assign_workspace(int B, int C, int T);
int ctn_sisnr_assign_fwd(const float* source, const float* estimate, const long long* lengths, int B, int C, int T, float* max_snr,
                         int* perm, float* loss, float* pair, float* coef, void* workspace, size_t workspace_bytes, void* stream);
int ctn_sisnr_assign_bwd(const float* source, const float* estimate, const long long* lengths, const int* perm, const float* coef,
                         const float* g_loss, const float* g_max, int B, int C, int T, float* d_estimate, void* stream);
int ctn_assign_solve(const float* score, int N, int C, int maximize, int* perm, void* stream);

/* ---- multi-resolution STFT loss in fp64, forward and backward (csrc/ctn_mrstft.hip) -----------------------------------------------
 * Spectral convergence, log-magnitude and linear-magnitude distance (Yamamoto et al., "Parallel WaveGAN", ICASSP 2020; auraloss
 * MultiResolutionSTFTLoss) of reference row c of utterance b against estimate row est_of_ref[b,c] (clamped to [0, E)), over R
 * resolutions; resolutions: HOST pointer to R triples (n_fft, hop, win_length) of int, read before any launch.
 * ref [B,C,T], est [B,E,T] fp32; lengths [B] int64, clamped to [0, T]: samples at t >= n = lengths[b] are never read.
 * Accepted: 1 <= R <= 8; n_fft a power of two in 64 .. 2048; 1 <= win_length <= n_fft; 1 <= hop, ceil(win_length / hop) <= 64;
 * B * C and B * E in 1 .. 65535, C <= 64, T in 1 .. 2^24; eps > 0.  Anything else: CTN_ERR_ARG before any launch.
 * The transform of a row: torch.stft(x[:n], n_fft, hop, win_length, hann_window(win_length), center=True, pad_mode='reflect'):
 * the periodic Hann window zero-padded to n_fft with (n_fft - win_length) / 2 zeros on the left, reflect padding of n_fft / 2
 * samples about samples 0 and n - 1, F = 1 + n / hop frames.  |X| = sqrt(max(re^2 + im^2, eps)).  Over the F (n_fft / 2 + 1) bins
 * of a (pair, resolution) cell, with D = sum (|S| - |S^|)^2 and A = sum |S|^2:
 *   terms [B,C,R,3] fp64 = { sqrt(D) / sqrt(A) (0 where D = 0),  mean | log|S| - log|S^| |,  mean | |S| - |S^| | }.
 * A cell with n <= n_fft / 2 (reflect padding undefined) has terms and gradient exactly 0.
 * Forward: a radix-2 FFT in LDS (reference and estimate frame packed as one complex input), per-frame partial sums, then a
 * fixed-order sum over a cell's frames; no spectrogram goes to memory.  workspace: ctn_mrstft_workspace() bytes; it keeps the
 * twiddle and window tables (built on the device by the first launch of the call) and the cells' sums for the backward pass.
 * Backward: g_terms [B,C,R,3] fp64 upstream -> g_est [B,E,T] fp32 = d sum(g_terms * terms) / d est: spectra recomputed per frame,
 * the adjoint transform and window into a per-frame fp64 workspace (ctn_mrstft_bwd_workspace() bytes), then per sample t < n the
 * frames that cover it and its mirror images in the padding, over the references that chose the row and the resolutions, in a
 * fixed order in fp64, rounded once.  A clamped bin (re^2 + im^2 < eps) and a bin with |S| = |S^| pass no gradient; exactly 0 at
 * t >= n and for rows no reference chose.  ref, est, lengths, est_of_ref, resolutions and eps must be those of the forward call.
 * A pair's terms and gradient are bitwise the same alone or in any batch.  Fixed-order reductions, no atomics, no read-back, no
 * synchronisation: graph-capturable.  The workspace functions return 0 for sizes or resolutions out of range. */
size_t ctn_mrstft_workspace(long long B, int C, long long T, int R, const int* resolutions);
size_t ctn_mrstft_bwd_workspace(long long B, int C, long long T, int R, const int* resolutions);
int ctn_mrstft_pairs_fwd(const float* ref, const float* est, const long long* lengths, const int* est_of_ref, long long B, int C,
                         long long E, long long T, const int* resolutions, int R, double eps, double* terms, void* workspace,
                         size_t workspace_bytes, void* stream);
int ctn_mrstft_pairs_bwd(const void* fwd_workspace, size_t fwd_workspace_bytes, const float* ref, const float* est,
                         const long long* lengths, const int* est_of_ref, long long B, int C, long long E, long long T,
                         const int* resolutions, int R, double eps, const double* g_terms, float* g_est, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- image-source room simulator: shoebox rooms for the reverberant mixer (csrc/ctn_ism.hip) ---------------------------------------
 * The image-source method of Allen & Berkley (JASA 65, 1979) for a rectangular room, one omnidirectional microphone, frequency-
 * independent walls: R responses of n_taps taps each, h [R][n_taps] fp64, that rir.RirBank turns into a bank for ctn_dynmix_reverb.
 * All device arithmetic is fp64, every operation ONE rounding in the order written here (no contraction into fused multiply-adds,
 * IEEE division and square root), the device calls no transcendental function and uses no floating-point atomic: h is a BITWISE
 * function of the tables, whatever the launch geometry.  tests/ism_oracle.py restates this text in numpy.
 * Tables (fp64, prepared on the host; `tables` is ONE buffer of ctn_ism_table_doubles(G, R, K, Q, W) doubles, the four parts back
 * to back; integers are stored as doubles):
 *   room  [G][16]     L[3] the dimensions in metres, mic[3], beta[6] the wall reflection coefficients in the order x0, x1, y0, y1,
 *                     z0, z1, each in [0, 1], N[3] the lattice bounds, N[a] = ceil(n_taps / fs * c / (2 L[a])) + 1 <= 4096, one 0.
 *   pw    [G][6][K]   pw[g][w][0] = 1, pw[g][w][k] = pw[g][w][k-1] * beta[w]: the repeated product, K >= max N + 2.
 *   resp  [R][4]      the room index g and src[3].  (A room of P source positions holds responses g * P .. g * P + P - 1.)
 *   frac  [Q][2W]     the fractional-delay table: with tau = (j - W + 1) - q / Q, frac[q][j] = sinc(tau) * 0.5 * (1 + cos(pi tau / W)),
 *                     0 where |tau| >= W (rir.design_fractional_delay).  1 <= Q <= 4096, 1 <= W <= 32.
 *   scalars           fs_over_c = fs / c, four_pi = 4 pi as a double, 1 <= n_taps <= 8192.
 * Images of response r in room g: the index ascends with nx outermost over [-N[0], N[0]], then ny, then nz, then
 * p = 4 px + 2 py + pz over 0 .. 7, innermost.  For one image:
 *   R_a  = ((1 - 2 p_a) * src[a] - mic[a]) + (2 * n_a) * L[a]                      per axis a
 *   d2   = (Rx * Rx + Ry * Ry) + Rz * Rz;   d = sqrt(d2), correctly rounded
 *   amp  = (((pw[0][|nx - px|] * pw[1][|nx|]) * (pw[2][|ny - py|] * pw[3][|ny|])) * (pw[4][|nz - pz|] * pw[5][|nz|])) / (d * four_pi)
 *   tau  = d * fs_over_c;   i = floor(tau);   q = int(floor((tau - i) * Q))
 *   (q < Q: tau - i <= 1 - 2^-52, and for Q = m * 2^e, 1 <= m < 2, the product lies within (m / 2) ulp < 1 ulp below Q and rounds
 *   below it.)  An image with i >= n_taps contributes nothing.  Otherwise, for j in [0, 2W), tap k = i + j - W + 1 receives
 *   amp * frac[q][j] when 0 <= k < n_taps.
 * Taps: h[r][k] starts at +0 and the contributions are added in ascending image index, acc = acc + amp * frac[q][j], the product and
 * the add one rounding each.  Images with amp == 0 may be skipped or added: their terms are +-0, and acc + (+-0) == acc bit for bit
 * unless acc is -0, which it never is -- acc starts at +0, (+0) + (-0) = +0, two non-zero terms that cancel give +0 under
 * round-to-nearest, and a non-zero acc plus a zero keeps its bits.  (The kernel skips them.)
 * ctn_ism_simulate: tables_host is the HOST copy of the same buffer.  Every row is checked there before the launch and nothing is
 *   launched on an error (CTN_ERR_ARG): the sizes above, the room index, 0 < L, N[a] an integer in [0, min(4096, K - 2)], at most 2^28
 *   lattice entries 8 (2 N[0] + 1) (2 N[1] + 1) (2 N[2] + 1) per room (a walk stays within seconds), mic and src strictly inside the room, |src - mic| >= 1e-3 m, beta in [0, 1].  The kernel checks the device copy again: a bad row is
 *   written as zeros with status[r] = -1, every other row gives status[r] = 0.  status [R] int32.
 *   stats: null, or two int64 the CALLER zeroed: [0] += lattice entries the pruned walks visited (summed over the workgroups),
 *   [1] += images that contributed (i < n_taps, amp != 0; each counted once).  Integer atomics; h does not depend on them.
 *   Gather form: one workgroup of 256 threads per (response, ctn_ism_chunk_taps() consecutive taps), one tap per thread.  It walks
 *   the lattice in index order, pruned to the spherical shell the chunk's images lie in (a tap wider on either side than the
 *   arithmetic above can reach, so only images that contribute nothing to the chunk are skipped), compacts the images whose span
 *   meets the chunk into an LDS list of ctn_ism_list_capacity() entries in that order (ballot and prefix, waves in fixed order),
 *   and drains the list in order, whenever it is full and at the end (the products amp * frac[q][j] of a few images at a time are
 *   staged in LDS, then every thread adds its tap's product or +0 per image).  No workspace, no read-back, no synchronisation.
 * ctn_dynmix_plan_rooms: the RIR half of ctn_dynmix_plan_aug for a bank of G rooms with P source positions each (R = G * P): all
 *   sources of a mixture in ONE room at DISTINCT positions.  Same key and counters as ctn_dynmix_plan_aug:
 *       room of mixture b      g = (uint64(word 0 of block (512, b, step, epoch)) * G) >> 32
 *       source c               k_c = (uint64(word 1 of block (c + 512, b, step, epoch)) * (P - c)) >> 32
 *       pos_c = the k_c-th position, in ascending order, that sources 0 .. c - 1 have not taken;  plan_rir[b,c] = g * P + pos_c
 *   2 <= C <= P <= 64.  It reads *step and leaves it alone.  It replaces only the RIR half: the noise half is still drawn by
 *   ctn_dynmix_plan_aug with a null plan_rir, and every other draw of a seed keeps its bits. */
int ctn_ism_list_capacity(void);
int ctn_ism_chunk_taps(void);
long long ctn_ism_table_doubles(int G, int R, int K, int Q, int W);
int ctn_ism_simulate(const double* tables_host, const double* tables, int G, int R, int K, int Q, int W, int n_taps, double fs_over_c,
                     double four_pi, double* h, int* status, long long* stats, void* stream);
int ctn_dynmix_plan_rooms(long long seed, int epoch, int rank, const unsigned* step, int B, int C, int G, int P, int* plan_rir,
                          void* stream);

/* ---- integrated loudness, ITU-R BS.1770-4, mono (csrc/ctn_loudness.hip) -------------------------------------------------------------
 * what the LibriMix recipe normalises every source and noise file with, for U ragged utterances in device memory: samples
 * [num_samples] fp32, offsets [U], lens [U] int64 as for ctn_dynmix_levels.  Of utterance u the device produces  ns, n_blocks, n_abs,
 * n_rel [U] int64 and sum_all, sum_abs, sum_rel [U] fp64;  the loudness itself is one division and one logarithm per utterance on the
 * host (loudness.loudness_from_stats).  For one utterance x[0 .. len), all in fp64, nothing appended, ns = len:
 *   weighting  x -> y through two biquads (the high shelf, then the high-pass; designed on the host from the analog prototype by the
 *              bilinear transform: loudness.design), direct form II transposed from zero state at sample 0, every product and every
 *              sum ONE rounding, no contraction, in this order:
 *                  y = b0 v + z1;  z1 = (b1 v + z2) - a1 y;  z2 = b2 v - a2 y                              (v: the section's input)
 *   sub-blocks h = hop = fs / 10 samples (800 <= h <= 4800), sub-block i = samples [i h, (i + 1) h), i < nsub = floor(len / h).  A chunk
 *              (below) meets at most three sub-blocks; a PIECE is what a chunk and a sub-block share, its sum p = p + y y per sample,
 *              in order, from 0.  S_i = ((0 + p) + p') + ..., the pieces of sub-block i, chunks ascending.
 *   blocks     n_blocks = max(nsub - 3, 0);  z_j = (((S_j + S_(j+1)) + S_(j+2)) + S_(j+3)) / (4 h): 400 ms every 100 ms in exact
 *              integers, a trailing partial block is dropped.
 *   gates      absolute: z_j > Ga (table[26] = 10^((-70 + 0.691) / 10), from the host);  relative: z_j > Ga and
 *              z_j > (sum_abs / n_abs) / 10.0 (none if n_abs = 0).  Both strict, in the power domain.
 *   sums       sum_all over all blocks, sum_abs over the absolute-gated ones, sum_rel over those that pass both; n_abs, n_rel count
 *              them.  Each sum: lane l = j mod 64 adds its blocks from 0, j ascending, then ((lane 0 + lane 1) + ...) + lane 63.
 * The device form: an utterance is cut into chunks of CH = ctn_loudness_chunk() samples by its own sample index.  Every chunk runs
 * from zero state and leaves its end state z_c (4 values, section order); one carry per utterance forms the true start states
 *     s_0 = 0;   s_(c+1)[r] = (((T[r][0] s_c[0] + T[r][1] s_c[1]) + T[r][2] s_c[2]) + T[r][3] s_c[3]) + z_c[r]
 * with T = A^CH (column k: the state CH zero-input samples after the unit state e_k) from the host; then every chunk is rerun from
 * s_c.  By linearity that is the sequential filter in exact arithmetic; in fp64 it is THIS computation (tests/loudness_oracle.py
 * restates it).  No pow, tan, exp or log on the device, no atomics on device memory, no read-back.
 * table [27] fp64: [0,5) shelf b0 b1 b2 a1 a2; [5,10) high-pass b0 b1 b2 a1 a2; [10,26) T row-major 4 x 4; [26] Ga.
 * chunk_ptr [U + 1] int64: chunk_ptr[0] = 0, chunk_ptr[u + 1] - chunk_ptr[u] = ceil(lens[u] / CH), total_chunks = chunk_ptr[U] (0 is
 * allowed: empty utterances only).
 * Determinism: the seven statistics of an utterance are a bitwise function of its own samples, the table, hop and CH: independent of
 * the neighbours, of U, of the launch geometry and of how a caller groups utterances into calls to bound the workspace.
 * An entry outside the buffer (offset < 0, len < 0, offset + len > num_samples) or a chunk range that is not the one its length asks
 * for is never read: ns[u] = -1, the other six are 0, and nothing else changes.
 * workspace: ctn_loudness_workspace(total_chunks, U) bytes (8-byte aligned; 7 fp64 words per chunk: a function of total_chunks alone,
 * U is only checked to be positive).  total_chunks <= 2^31 - 65 per call.  Four launches on `stream` (one if total_chunks = 0); bad
 * sizes are CTN_ERR_ARG before any launch. */
int ctn_loudness_chunk(void);
size_t ctn_loudness_workspace(long long total_chunks, long long U);
int ctn_loudness(const float* samples, long long num_samples, const long long* offsets, const long long* lens,
                 const long long* chunk_ptr, long long U, long long total_chunks, const double* table, int hop, long long* ns,
                 long long* n_blocks, long long* n_abs, long long* n_rel, double* sum_all, double* sum_abs, double* sum_rel,
                 void* workspace, size_t workspace_bytes, void* stream);

/* ---- LibriMix-recipe mixing: absolute loudness per source, a noise loudness, rescale only what clips ------------------------------
 * (csrc/ctn_dynmix_loudness.hip, the gathers of csrc/ctn_dynmix.hip and csrc/ctn_dynmix_aug.hip).  The corpus' inv_rms is
 * float32(1 / sqrt(gated K-weighted power)) from ctn_loudness: an utterance times inv_rms reads 0.691 dB above 0 LUFS.
 * ctn_dynmix_plan_loudness: launched BEHIND ctn_dynmix_plan / ctn_dynmix_plan_speed on the same stream (and before
 *   ctn_dynmix_mask_active): those have advanced the step word, so the minibatch's step is *step - 1, which it reads and leaves alone.
 *       i = below(r.w[0], nl),  r = philox4x32_10(1280 + c, b, *step - 1, epoch, k0, k1), key and below() as in ctn_dynmix_plan
 *       plan_l10[b,c] = lo10 + i (tenths of a LU);   gain[b,c] = wl[i] * inv_rms[plan_utt[b,c]]  (one fp32 multiply; 0 for a
 *       flagged entry, plan_utt outside [0, U))
 *   wl [nl] fp32, 1 <= nl <= 1024, from the host: wl[i] = float32(10^(((lo10 + i) / 10 + 0.691) / 20)).  It OVERWRITES the gains of
 *   the plan; plan_q is still drawn and plays no part.  The c0 words c, 256 + c, 512 + c, 768 and 1024 belong to the other draws,
 *   which keep their bits; 1280 + c is used by no other draw.
 * The noise loudness needs no entry point of its own: ctn_dynmix_plan_aug with wn = the loudness table of the noise range
 *   (wn[k] = float32(10^(((lo10 + k) / 10 + 0.691) / 20))), so the word that chooses the SNR chooses the noise loudness, snr10 holds
 *   its tenths of a LU and ngain = wn[k] * noise_inv_rms[v] with the noise corpus' loudness inv_rms.
 * ctn_dynmix_gather_peak / ctn_dynmix_gather_aug_peak: ctn_dynmix_gather / ctn_dynmix_gather_aug with the peak rule as an argument:
 *       peak_mode 0   scale = a > 0 ? 0.9f / a : 1      every mixture to a peak of 0.9: what the plain entry points do (they forward)
 *       peak_mode 1   scale = a > 0.9f ? 0.9f / a : 1   only a mixture that would clip (the LibriMix rule)
 *   a = peak[b], the unscaled maximum, is stored as before; every other word of their contracts holds. */
int ctn_dynmix_plan_loudness(const int* plan_utt, const float* inv_rms, long long U, const float* wl, int nl, int lo10, long long seed,
                             int epoch, int rank, const unsigned* step, int B, int C, int* plan_l10, float* gain, void* stream);
int ctn_dynmix_gather_peak(const float* corpus, const long long* offsets, const long long* lens, long long U, const int* plan_utt,
                           const long long* plan_start, const float* gain, int B, int C, int T, float* mixture, float* sources,
                           float* peak, void* workspace, size_t workspace_bytes, int mode, int peak_mode, void* stream);
int ctn_dynmix_gather_aug_peak(const float* corpus, const long long* offsets, const long long* lens, long long U, const int* plan_utt,
                               const long long* plan_start, const float* gain, int B, int C, int T, const float* tgt_corpus,
                               const float* noise, const long long* noise_offsets, const long long* noise_lens, long long Un,
                               const int* noise_utt, const long long* noise_start, const float* ngain, float* mixture, float* sources,
                               float* peak, void* workspace, size_t workspace_bytes, int peak_mode, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CTN_HIP_H */
