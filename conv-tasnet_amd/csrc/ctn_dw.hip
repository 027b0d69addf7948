// Row kernels of the temporal-conv blocks, gfx950: one wave owns one (utterance, channel) row.
//
//  * depthwise dilated conv forward/backward (src/conv_tasnet.py:247-295) with the
//    neighbouring PReLU + global-LayerNorm (:224-225, :259-260, :338-361) fused in:
//    frames on the lanes (coalesced 256-B / 1-KiB wave accesses), the P-tap dilated window is served from an
//    LDS copy of the row segment (+halo) that already holds the normalised values.
//  * element-wise gLN+PReLU backward.
//  * small fixed-order reductions for per-channel parameter gradients.
//
// (The channel-wise LayerNorm kernels of the causal variant are in ctn_cln.hip.)
//
// All cross-lane / cross-block sums have a fixed order (no float atomics), so a step is bitwise reproducible run to run.
#include "ctn_common.h"
#include <stdlib.h>
#include <type_traits>

namespace {

constexpr int NT = 256;
constexpr int ROWS = 4;          // one wave per row
constexpr int MAXP = 8;          // max depthwise kernel size supported
// LDS floats per wave for the row segment (+halo).  Small buffers when the receptive field is short (more
// workgroups per CU in flight = more HBM requests outstanding), large ones when the halo would dominate.
constexpr int FWD_BUF_S = 1024, FWD_BUF_L = 3584;    // forward: 16 / 56 KiB per workgroup
constexpr int BWD_BUF_S = 768, BWD_BUF_M = 1280, BWD_BUF_L = 1792;     // backward (two arrays): 24 / 40 / 56 KiB per workgroup

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ int floor4(int v) { return (v >> 2) << 2; }  // arithmetic shift: floors negatives

// Early loads.  The row kernels below issue a whole batch of a wave's 16-byte loads before they use the first of them, so a
// wave pays one memory round trip per batch and its bandwidth does not hang on how many sibling waves the CU still holds.
// Such a load is issued before the code that decides whether the frame exists, so it must not be able to fault: every
// wave reads through a buffer resource that spans exactly its own row (no bytes at all for a dead wave), and a frame outside
// [0, Kp) is sent to ROW_OOB, an offset past the end of any row: the hardware range check answers 0 and no address outside
// the tensor is formed.  (make_rsrc / buf_ld4 as in ctn_gemm_common.h, whose other names collide with this file's.)
typedef float f32x4v __attribute__((ext_vector_type(4)));
constexpr int ROW_OOB = (int)0x80000000u;
constexpr int CHUNK = 256;       // frames that one wave covers with one float4 per lane
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ float4 buf_ld4(__amdgpu_buffer_rsrc_t r, int voff) {
    const f32x4v f = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0));
    return make_float4(f.x, f.y, f.z, f.w);
}
__device__ __forceinline__ float uni(float v) {      // a wave-uniform value into a scalar register
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
// byte offset of frame k (a multiple of 4) in a row of Kp frames; `in` = the lane takes part in this chunk at all
__device__ __forceinline__ int row_voff(int k, int Kp, bool in) { return (in && k >= 0 && k < Kp) ? k * 4 : ROW_OOB; }

// ---------------------------------------------------------------------------
// depthwise forward:  z[k] = sum_j D[c,j] * n[k + j*dil - padl],  n = (PRO ? gLN(prelu(y)) : y)
// ---------------------------------------------------------------------------
struct DwFwdArgs {
    const float* Y; float* Z; const float* D;
    int M, H, K, Kp, P, dil, padl, seg;
    const double* pro_part; int pro_nparts;
    const float* pro_gamma; const float* pro_beta; const float* pro_alpha; float* pro_ms_out;
    const float* epi_alpha; double* epi_part;   // [M, H, 2]
    unsigned* amax_out;                         // EPI: [M][CTN_AMAX_SLOTS] max |Z[m]| (h3 arithmetic of the GEMM that reads Z), optional
    const float* cln_mean; const float* cln_rstd;   // PRO = 2: [M][Kp] per-frame statistics of the channel-wise LayerNorm
};

// PRO: 0 n = y, 1 n = gLN(prelu(y)) (per-utterance statistics), 2 n = cLN(prelu(y)) (per-frame statistics, round 4)
template <int PRO, bool EPI, int FWD_BUF, bool VEC4, int PT>      // PT: compile-time kernel size (3) or 0 = a.P at run time
__global__ __launch_bounds__(NT) void dw_fwd_kernel(DwFwdArgs a) {
    __shared__ __attribute__((aligned(16))) float buf[ROWS][FWD_BUF];
    __shared__ double red[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (scalar: the row and its buffer resources are wave-uniform)
    const int hb = (a.H + ROWS - 1) / ROWS;
    const int m = blockIdx.x / hb;
    const int c = (blockIdx.x % hb) * ROWS + wave;
    const bool live = c < a.H;
    const size_t row = ((size_t)m * a.H + (live ? c : 0)) * a.Kp;
    const float* __restrict__ y = a.Y + row;
    float* __restrict__ z = a.Z + row;
    float* __restrict__ L = buf[wave];
    const unsigned rbytes = live ? (unsigned)a.Kp * 4u : 0u;
    const __amdgpu_buffer_rsrc_t rsY = make_rsrc(y, rbytes);

    float mean = 0.f, rstd = 1.f, alpha = 0.f, g = 1.f, b = 0.f;
    const float* __restrict__ cmu = PRO == 2 ? a.cln_mean + (size_t)m * a.Kp : nullptr;
    const float* __restrict__ crs = PRO == 2 ? a.cln_rstd + (size_t)m * a.Kp : nullptr;
    const __amdgpu_buffer_rsrc_t rsMu = make_rsrc(cmu, PRO == 2 ? rbytes : 0u), rsRs = make_rsrc(crs, PRO == 2 ? rbytes : 0u);
    if constexpr (PRO == 2) {
        alpha = a.pro_alpha[0];
        if (live) { g = a.pro_gamma[c]; b = a.pro_beta[c]; }
    }
    if constexpr (PRO == 1) {
        finalize_stats<NT>(a.pro_part + (size_t)m * a.pro_nparts * 2, a.pro_nparts, (double)a.H * (double)a.K, red,
                           mean, rstd);
        alpha = a.pro_alpha[0];
        if (live) { g = a.pro_gamma[c]; b = a.pro_beta[c]; }
        if (a.pro_ms_out != nullptr && (blockIdx.x % hb) == 0 && tid == 0) {
            a.pro_ms_out[2 * m] = mean;
            a.pro_ms_out[2 * m + 1] = rstd;
        }
    }
    const float gs = g * rstd, cc = b - gs * mean, gn = gs * alpha;
    constexpr int NP = PT ? PT : MAXP;
    const int P_ = PT ? PT : a.P;
    float taps[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) taps[j] = (live && j < P_) ? a.D[(size_t)c * P_ + j] : 0.f;
    float e_alpha = 0.f;
    if constexpr (EPI) e_alpha = a.epi_alpha[0];
    const int halo = (P_ - 1) * a.dil;
    float s1 = 0.f, s2 = 0.f, amax = 0.f;

    // The image of a segment is filled in batches of NB chunks: all loads of a batch first, then the arithmetic and the LDS
    // writes chunk by chunk.  The small patch is one batch.  On the float4 tap path the first batch of the next segment is
    // issued before this segment's taps and stores, so its round trip runs beside them; on the scalar tap path (64-frame
    // groups, 4 times as many tap iterations per segment) that measured 4 % slower alone (profiles/README.md), so there
    // the batch is issued where it is used.
    constexpr int NB = 4;
    float4 rv[NB], rmu[NB], rrs[NB];
    auto issue = [&](int base, int j0, int nfill) {        // chunk i of the batch: image floats j0 + CHUNK i + 4 lane ..+3
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int j = j0 + CHUNK * i + lane * 4;
            const int off = row_voff(base + j, a.Kp, j < nfill);
            rv[i] = buf_ld4(rsY, off);
            if constexpr (PRO == 2) { rmu[i] = buf_ld4(rsMu, off); rrs[i] = buf_ld4(rsRs, off); }
        }
    };
    auto consume = [&](int base, int j0, int nfill) {
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int j = j0 + CHUNK * i + lane * 4;
            if (j >= nfill) continue;
            const int k = base + j;
            float4 v = rv[i];                               // 0 outside the row
            if (live && k >= 0 && k < a.Kp) {
                if constexpr (PRO == 2) {  // gamma ((prelu(x) - mean[k]) rstd[k]) + beta: the order of cln_fwd_v4_kernel
                    const float4 mu = rmu[i], rs = rrs[i];
                    v.x = k + 0 < a.K ? g * ((prelu_f(v.x, alpha) - mu.x) * rs.x) + b : 0.f;
                    v.y = k + 1 < a.K ? g * ((prelu_f(v.y, alpha) - mu.y) * rs.y) + b : 0.f;
                    v.z = k + 2 < a.K ? g * ((prelu_f(v.z, alpha) - mu.z) * rs.z) + b : 0.f;
                    v.w = k + 3 < a.K ? g * ((prelu_f(v.w, alpha) - mu.w) * rs.w) + b : 0.f;
                }
                if constexpr (PRO == 1) {  // gamma*((prelu(x)-mean)*rstd)+beta as one select + one FMA per element
                    v.x = fmaf(v.x, v.x >= 0.f ? gs : gn, cc);
                    v.y = fmaf(v.y, v.y >= 0.f ? gs : gn, cc);
                    v.z = fmaf(v.z, v.z >= 0.f ? gs : gn, cc);
                    v.w = fmaf(v.w, v.w >= 0.f ? gs : gn, cc);
                    if (k + 3 >= a.K) {
                        if (k + 0 >= a.K) v.x = 0.f;
                        if (k + 1 >= a.K) v.y = 0.f;
                        if (k + 2 >= a.K) v.z = 0.f;
                        if (k + 3 >= a.K) v.w = 0.f;
                    }
                }
            }
            *reinterpret_cast<float4*>(L + j) = v;
        }
    };
    auto nfill_of = [&](int k0) { return (min(k0 + a.seg, a.Kp) - k0) + halo + 4; };   // covers idx up to (kend-1-base-padl)+halo

    constexpr bool AHEAD = VEC4;
    if (AHEAD) issue(floor4(-a.padl), 0, nfill_of(0));
    for (int k0 = 0; k0 < a.Kp; k0 += a.seg) {
        const int kend = min(k0 + a.seg, a.Kp);
        const int base = floor4(k0 - a.padl);
        const int nfill = nfill_of(k0);
        if (!AHEAD) issue(base, 0, nfill);
        consume(base, 0, nfill);
        for (int j0 = CHUNK * NB; j0 < nfill; j0 += CHUNK * NB) {
            issue(base, j0, nfill);
            consume(base, j0, nfill);
        }
        __builtin_amdgcn_wave_barrier();   // the LDS patch is private to this wave; DS ops of one wave retire in order
        if (AHEAD && k0 + a.seg < a.Kp) issue(floor4(k0 + a.seg - a.padl), 0, nfill_of(k0 + a.seg));
        if constexpr (VEC4) {
            // dilation and pad are multiples of 4: every tap of 4 consecutive frames is one aligned 16-byte LDS read
            // and the result leaves as a float4 (1 KiB per wave store)
            for (int k = k0 + lane * 4; k < kend; k += 256) {
                const int idx = k - base - a.padl;
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int j = 0; j < NP; ++j)
                    if (PT || j < a.P) {
                        const float4 t = *reinterpret_cast<const float4*>(L + idx + j * a.dil);
                        acc.x += taps[j] * t.x; acc.y += taps[j] * t.y; acc.z += taps[j] * t.z; acc.w += taps[j] * t.w;
                    }
                if (k + 3 >= a.K) {
                    if (k + 0 >= a.K) acc.x = 0.f;
                    if (k + 1 >= a.K) acc.y = 0.f;
                    if (k + 2 >= a.K) acc.z = 0.f;
                    if (k + 3 >= a.K) acc.w = 0.f;
                }
                if constexpr (EPI) {
                    const float p0 = prelu_f(acc.x, e_alpha), p1 = prelu_f(acc.y, e_alpha);
                    const float p2 = prelu_f(acc.z, e_alpha), p3 = prelu_f(acc.w, e_alpha);
                    s1 += (p0 + p1) + (p2 + p3);
                    s2 += (p0 * p0 + p1 * p1) + (p2 * p2 + p3 * p3);
                    amax = fmaxf(fmaxf(amax, fmaxf(fabsf(acc.x), fabsf(acc.y))), fmaxf(fabsf(acc.z), fabsf(acc.w)));
                }
                if (live) *reinterpret_cast<float4*>(z + k) = acc;
            }
        } else {
        for (int k = k0 + lane; k < kend; k += 64) {
            const int idx = k - base - a.padl;
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < NP; ++j)
                if (PT || j < a.P) acc += taps[j] * L[idx + j * a.dil];
            if (k >= a.K) acc = 0.f;
            if constexpr (EPI) {
                const float p = prelu_f(acc, e_alpha);
                s1 += p;
                s2 += p * p;
                amax = fmaxf(amax, fabsf(acc));
            }
            if (live) z[k] = acc;
        }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if constexpr (EPI) {
        const double d1 = wave_sum((double)s1), d2 = wave_sum((double)s2);
        if (live && lane == 0) {
            double* dst = a.epi_part + ((size_t)m * a.H + c) * 2;
            dst[0] = d1;
            dst[1] = d2;
        }
        if (a.amax_out != nullptr) block_amax_atomic<NT>(amax, red, a.amax_out + (size_t)m * CTN_AMAX_SLOTS, blockIdx.x % hb);      // (dead waves hold 0)
    }
}

// ---------------------------------------------------------------------------
// depthwise backward.
//   FUSED: given dN2 (grad of the 2nd norm's output), d (= dw output, pre-PReLU) and h1
//          (= first 1x1 output, pre-PReLU):
//            xh2 = (prelu(d)-mean2)*rstd2 ; da2 = rstd2*(g2*dN2 - S1/n - xh2*S2/n) ; dd = da2*prelu'(d)
//            n1  = g1*xh1+b1, xh1 = (prelu(h1)-mean1)*rstd1
//            dN1[k] = sum_j D[j]*dd[k - j*dil + padl] ;  dD[j] = sum_k dd[k]*n1[k + j*dil - padl]
//          plus every per-channel / per-utterance sum the two norms and PReLUs need.
//   PLAIN: dd = dZ, n1 = X as stored.
//   CLN (round 4; channel-wise LayerNorm, the causal config): dd as in FUSED but with PER-FRAME constants of the second norm --
//          fc [M][4][Kp] = (rstd2, mean2 rstd2, rstd2 S1/H, rstd2 S2/H)[k] from ctn_cln_bwd_frame (S1, S2: the per-frame sums over
//          channels that the input-gradient GEMM's epilogue produced) -- and n1 = X as stored (the first norm's output):
//            xh2 = prelu(d) fc0 - fc1 ; da2 = g2 fc0 dN2 - fc2 - xh2 fc3 ; dd = da2 * prelu'(d)
//          i.e. the whole stand-alone cLN-backward pass of the second norm (three tensor passes) rides in this kernel's dd image.
// Template: DDM = how dd is formed (0 plain, 1 gLN, 2 cLN), XM = how the x image is formed (0 as stored, 1 gLN-1 recomputed from h1,
// 2 cLN-1 recomputed from h1 with its per-frame statistics: the first norm's output is never stored; 3 (with DDM = 1, round 4) as 1 AND
// the first norm's own backward applied to the result: the kernel writes dh1 = gLN1' . PReLU1'(dn1) instead of dn1 -- its two sums
// S1', S2' are known BEFORE this kernel runs (ctn_pw_dgrad_gln2: sums2_part is [M, parts, 8]), so the gln_prelu_bwd pass is gone;
// pc gets a row P+5 with the dalpha1 partials).
// per-row float outputs pc[f][m][c]:  f = 0..P-1: dD ; (DDM, XM) = (1, 1) adds P: dgamma2, P+1: dbeta2,
//   P+2: dgamma1, P+3: dbeta1, P+4: dalpha2 ; (2, 0) adds P: dgamma2, P+1: dbeta2, P+2: dalpha2
// ---------------------------------------------------------------------------
struct DwBwdArgs {
    const float* dN2; const float* Dz; const float* Y1; float* dN1; const float* D;
    int M, H, K, Kp, P, dil, padl, seg;
    const float* g1; const float* b1; const float* a1; const float* ms1;
    const float* g2; const float* a2; const float* ms2;
    const double* sums2_part; int sums2_nparts;
    float* pc;             // [F, M, H]
    double* sums1_part;    // [M, H, 2]
    const float* fc2;      // DDM = 2: [M][4][Kp] per-frame constants of the second norm's backward
    const float* mean1f; const float* rstd1f;      // XM = 2: [M][Kp] per-frame statistics of the first (channel-wise) norm
    unsigned* amax_out;    // XM = 3: [M][CTN_AMAX_SLOTS] max |dY1[m]| (h3 arithmetic of the GEMMs that read it), optional
};

// registers of one batch of N chunks (the members a form does not load are never touched and cost nothing)
template <int N_> struct DdRegs { static constexpr int N = N_; float4 n[N_], d[N_], f0[N_], f1[N_], f2[N_], f3[N_]; };
template <int N_> struct XRegs { static constexpr int N = N_; float4 v[N_], mu[N_], rs[N_]; };

template <int DDM, int XM, int BWD_BUF, bool VEC4, int PT>
__global__ __launch_bounds__(NT) void dw_bwd_kernel(DwBwdArgs a) {
    static_assert((DDM == 0 && XM == 0) || (DDM == 1 && (XM == 1 || XM == 3)) || (DDM == 2 && (XM == 0 || XM == 2)), "supported forms");
    constexpr bool APPLY = XM == 3;         // write dh1 (first norm's backward applied) instead of dn1
    constexpr bool FUSED = DDM == 1;        // (the gLN form couples both images)
    constexpr bool XHAT = XM != 0;          // the x image holds xhat1: gamma1 / beta1 are applied where it is read
    __shared__ __attribute__((aligned(16))) float bufA[ROWS][BWD_BUF];  // dd
    __shared__ __attribute__((aligned(16))) float bufB[ROWS][BWD_BUF];  // xh1 (FUSED) or x (PLAIN)
    __shared__ double red[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (scalar: the row and its buffer resources are wave-uniform)
    const int hb = (a.H + ROWS - 1) / ROWS;
    const int m = blockIdx.x / hb;
    const int c = (blockIdx.x % hb) * ROWS + wave;
    const bool live = c < a.H;
    const size_t row = ((size_t)m * a.H + (live ? c : 0)) * a.Kp;
    const float* __restrict__ dn2 = a.dN2 + row;
    const float* __restrict__ dz = DDM != 0 ? a.Dz + row : nullptr;
    const float* __restrict__ fcm = DDM == 2 ? a.fc2 + (size_t)m * 4 * a.Kp : nullptr;
    const float* __restrict__ y1 = a.Y1 + row;
    float* __restrict__ dn1 = a.dN1 + row;
    float* __restrict__ LA = bufA[wave];
    float* __restrict__ LB = bufB[wave];

    float mean1 = 0.f, rstd1 = 1.f, mean2 = 0.f, rstd2 = 1.f, al1 = 0.f, al2 = 0.f;
    float g1 = 1.f, b1 = 0.f, g2 = 1.f, c1 = 0.f, c2 = 0.f;
    float c1p = 0.f, c2p = 0.f;            // APPLY: S1' / n, S2' / n of the first norm
    if constexpr (FUSED) {
        constexpr int NS = APPLY ? 8 : 2;
        double S[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) S[q] = 0.0;
        for (int i = tid; i < a.sums2_nparts; i += NT)
#pragma unroll
            for (int q = 0; q < NS; ++q) S[q] += a.sums2_part[((size_t)m * a.sums2_nparts + i) * NS + q];
        if constexpr (APPLY) {          // the eight sums in one reduction (two barriers): fp64 over the lanes, then over the waves in order
            __shared__ double red8[8][NT / 64];
#pragma unroll
            for (int q = 0; q < NS; ++q) S[q] = wave_sum(S[q]);
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < NS; ++q) red8[q][wave] = S[q];
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                double r = red8[q][0];
#pragma unroll
                for (int w2 = 1; w2 < NT / 64; ++w2) r += red8[q][w2];
                S[q] = r;
            }
        } else {
#pragma unroll
            for (int q = 0; q < NS; ++q) S[q] = block_sum<double, NT>(S[q], red);
        }
        const double n = (double)a.H * (double)a.K;
        const double d1 = S[0] / n, d2 = S[1] / n;
        c1 = (float)d1;
        c2 = (float)d2;
        if constexpr (APPLY) {          // S1' = rstd2 (A1 - c1 B1 - c2 C1), S2' = rstd2 (A2 - c1 B2 - c2 C2)   (ctn_pw_dgrad_gln2)
            const double r2 = (double)a.ms2[2 * m + 1];
            c1p = (float)(r2 * (S[2] - d1 * S[3] - d2 * S[4]) / n);
            c2p = (float)(r2 * (S[5] - d1 * S[6] - d2 * S[7]) / n);
        }
        mean1 = a.ms1[2 * m]; rstd1 = a.ms1[2 * m + 1];
        mean2 = a.ms2[2 * m]; rstd2 = a.ms2[2 * m + 1];
        al1 = a.a1[0]; al2 = a.a2[0];
        if (live) { g1 = a.g1[c]; b1 = a.b1[c]; g2 = a.g2[c]; }
    }
    if constexpr (DDM == 2) {
        al2 = a.a2[0];
        if (live) g2 = a.g2[c];
    }
    const float* __restrict__ mu1f = XM == 2 ? a.mean1f + (size_t)m * a.Kp : nullptr;
    const float* __restrict__ rs1f = XM == 2 ? a.rstd1f + (size_t)m * a.Kp : nullptr;
    if constexpr (XM == 2) {
        al1 = a.a1[0];
        if (live) { g1 = a.g1[c]; b1 = a.b1[c]; }
    }
    // buffer resources of the early loads: the wave's own rows, and the utterance's per-frame vectors of the cLN forms
    const unsigned rbytes = live ? (unsigned)a.Kp * 4u : 0u;
    const __amdgpu_buffer_rsrc_t rsN = make_rsrc(dn2, rbytes), rsD = make_rsrc(dz, DDM != 0 ? rbytes : 0u), rsY = make_rsrc(y1, rbytes);
    const __amdgpu_buffer_rsrc_t rsF = make_rsrc(fcm, DDM == 2 && live ? (unsigned)a.Kp * 16u : 0u);
    const __amdgpu_buffer_rsrc_t rsMu = make_rsrc(mu1f, XM == 2 ? rbytes : 0u), rsRs = make_rsrc(rs1f, XM == 2 ? rbytes : 0u);
    constexpr int NP = PT ? PT : MAXP;
    const int P_ = PT ? PT : a.P;
    float taps[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) taps[j] = (live && j < P_) ? a.D[(size_t)c * P_ + j] : 0.f;
    const int halo = (P_ - 1) * a.dil;

    // folded constants of the two norms: xh = x*(x>=0 ? rstd : alpha*rstd) - mean*rstd ;  da = rg2*dn2 - rc1 - xh*rc2
    // (all wave-uniform, but computed by the vector ALU: uni() hands them to the scalar register file, which takes the float4
    // gLN variants from 97 to 92 vector registers.  Those variants then sit at the scalar-register cap: 13 scalar values are
    // spilled to lanes of one vector register, which the 92 include, and come back by v_readlane in the fill.  uni() on any
    // subset of the constants gave 94-95 registers and 8-11 spills: profiles/dw_batched_resources.txt)
    const float ar1 = uni(al1 * rstd1), mr1 = uni(mean1 * rstd1), ar2 = uni(al2 * rstd2), mr2 = uni(mean2 * rstd2);
    const float rg2 = uni(rstd2 * g2), rc1 = uni(rstd2 * c1), rc2 = uni(rstd2 * c2);
    float dD[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) dD[j] = 0.f;
    float dg2 = 0.f, db2 = 0.f, dal2 = 0.f, dg1 = 0.f, db1 = 0.f, t1 = 0.f, t2 = 0.f;
    float dal1 = 0.f, amax1 = 0.f;
    const float rg1 = uni(rstd1 * g1), rc1p = uni(rstd1 * c1p), rc2p = uni(rstd1 * c2p);       // APPLY: da1 = rstd1 (g1 dn1 - c1' - xh1 c2')
    // dh1 of one element: dn = dn1[k], xh = xhat1[k], h = h1[k] (its sign selects the PReLU branch); k < K
    auto apply1 = [&](float dn, float xh, float h) -> float {
        const float da = fmaf(-xh, rc2p, fmaf(rg1, dn, -rc1p));
        if (h < 0.f) dal1 += da * h;
        const float o = h >= 0.f ? da : al1 * da;
        amax1 = fmaxf(amax1, fabsf(o));
        return o;
    };

    for (int k0 = 0; k0 < a.Kp; k0 += a.seg) {
        const int kend = min(k0 + a.seg, a.Kp);
        // dd is needed on [k0 + padl - halo, kend-1 + padl]; x on [k0 - padl, kend-1 - padl + halo]
        const int baseA = floor4(k0 + a.padl - halo);
        const int baseB = floor4(k0 - a.padl);
        const int nfill = (kend - k0) + halo + 4;
        // dd image.  Frames of [k0, kend) belong to this segment: their parameter-gradient sums are taken here, and
        // when the segment lies inside [0, K) -- a uniform condition -- nothing in the loop is predicated.  The halo
        // frames on either side are transformed only (the neighbouring segment owns their sums).
        //
        // Loads come in batches of chunks (CHUNK frames, one float4 per lane and tensor): issue_dd / issue_x put a batch's loads
        // in flight, use_dd / use_x then run the arithmetic and the LDS writes on it chunk by chunk, in the order of frames, so
        // every per-lane sum adds its terms in the order it always did.  The gLN and plain forms take a segment in two batches
        // (below); the cLN forms carry six vectors per dd chunk and go range by range, a chunk at a time.
        auto issue_dd = [&](int kq, int ke, auto& r) {         // chunk i of the batch: frames kq + CHUNK i + 4 lane ..+3, below ke
#pragma unroll
            for (int i = 0; i < r.N; ++i) {
                const int k = kq + CHUNK * i + lane * 4;
                const int off = row_voff(k, a.Kp, k < ke);
                r.n[i] = buf_ld4(rsN, off);
                if constexpr (DDM != 0) r.d[i] = buf_ld4(rsD, off);
                if constexpr (DDM == 2) {
                    // (a.Kp * 4 bytes from one vector of fc to the next: an out-of-range frame must stay out of range)
                    const int p4 = off == ROW_OOB ? 0 : a.Kp * 4;
                    r.f0[i] = buf_ld4(rsF, off); r.f1[i] = buf_ld4(rsF, off + p4);
                    r.f2[i] = buf_ld4(rsF, off + 2 * p4); r.f3[i] = buf_ld4(rsF, off + 3 * p4);
                }
            }
        };
        auto use_dd = [&](int kq, int ke, const auto& r, const bool own, const bool all_valid) {
#pragma unroll
            for (int i = 0; i < r.N; ++i) {
                const int k = kq + CHUNK * i + lane * 4;
                if (k >= ke) continue;
                float4 v = r.n[i];                              // 0 outside the row
                if (live && k >= 0 && k < a.Kp) {
                    if constexpr (FUSED) {
                        const float4 d = r.d[i];
                        float vv[4] = {v.x, v.y, v.z, v.w};
                        const float dd_[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const bool valid = all_valid || (k + e) < a.K;
                            const float xh = fmaf(dd_[e], dd_[e] >= 0.f ? rstd2 : ar2, -mr2);    // (prelu(d)-mean2)*rstd2
                            const float da = fmaf(-xh, rc2, fmaf(rg2, vv[e], -rc1));            // rstd2*(g2*dn2 - c1 - xh*c2)
                            if (own && valid) {
                                dg2 += vv[e] * xh;
                                db2 += vv[e];
                                dal2 += dd_[e] < 0.f ? da * dd_[e] : 0.f;
                            }
                            vv[e] = valid ? (dd_[e] >= 0.f ? da : al2 * da) : 0.f;
                        }
                        v = make_float4(vv[0], vv[1], vv[2], vv[3]);
                    }
                    if constexpr (DDM == 2) {
                        const float4 d = r.d[i];
                        const float4 f0 = r.f0[i], f1 = r.f1[i], f2 = r.f2[i], f3 = r.f3[i];
                        float vv[4] = {v.x, v.y, v.z, v.w};
                        const float dd_[4] = {d.x, d.y, d.z, d.w};
                        const float q0[4] = {f0.x, f0.y, f0.z, f0.w}, q1[4] = {f1.x, f1.y, f1.z, f1.w};
                        const float q2[4] = {f2.x, f2.y, f2.z, f2.w}, q3[4] = {f3.x, f3.y, f3.z, f3.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const bool valid = all_valid || (k + e) < a.K;
                            const float xh = fmaf(dd_[e], dd_[e] >= 0.f ? q0[e] : al2 * q0[e], -q1[e]);      // (prelu(d) - mean2[k]) rstd2[k]
                            const float da = fmaf(-xh, q3[e], fmaf(q0[e] * g2, vv[e], -q2[e]));               // rstd2 (g2 dn2 - S1/H - xh S2/H)
                            if (own && valid) {
                                dg2 += vv[e] * xh;
                                db2 += vv[e];
                                dal2 += dd_[e] < 0.f ? da * dd_[e] : 0.f;
                            }
                            vv[e] = valid ? (dd_[e] >= 0.f ? da : al2 * da) : 0.f;
                        }
                        v = make_float4(vv[0], vv[1], vv[2], vv[3]);
                    }
                }
                *reinterpret_cast<float4*>(LA + (k - baseA)) = v;
            }
        };
        auto issue_x = [&](int j0, auto& r) {                  // chunk i of the batch: image floats j0 + CHUNK i + 4 lane ..+3
#pragma unroll
            for (int i = 0; i < r.N; ++i) {
                const int j = j0 + CHUNK * i + lane * 4;
                const int off = row_voff(baseB + j, a.Kp, j < nfill);
                r.v[i] = buf_ld4(rsY, off);
                if constexpr (XM == 2) { r.mu[i] = buf_ld4(rsMu, off); r.rs[i] = buf_ld4(rsRs, off); }
            }
        };
        auto use_x = [&](int j0, const auto& r) {
#pragma unroll
            for (int i = 0; i < r.N; ++i) {
                const int j = j0 + CHUNK * i + lane * 4;
                if (j >= nfill) continue;
                const int k = baseB + j;
                float4 v = r.v[i];                              // 0 outside the row
                if (live && k >= 0 && k < a.Kp) {
                    if constexpr (XM == 2) {
                        const float4 mu = r.mu[i], rs = r.rs[i];
                        v.x = (prelu_f(v.x, al1) - mu.x) * rs.x;
                        v.y = (prelu_f(v.y, al1) - mu.y) * rs.y;
                        v.z = (prelu_f(v.z, al1) - mu.z) * rs.z;
                        v.w = (prelu_f(v.w, al1) - mu.w) * rs.w;
                    }
                    if constexpr (FUSED) {
                        v.x = fmaf(v.x, v.x >= 0.f ? rstd1 : ar1, -mr1);
                        v.y = fmaf(v.y, v.y >= 0.f ? rstd1 : ar1, -mr1);
                        v.z = fmaf(v.z, v.z >= 0.f ? rstd1 : ar1, -mr1);
                        v.w = fmaf(v.w, v.w >= 0.f ? rstd1 : ar1, -mr1);
                    }
                }
                *reinterpret_cast<float4*>(LB + j) = v;
            }
        };
        // the batches of a range past its first one, each issued and used in turn
        auto rest_dd = [&](int kb, int ke, auto& r, const bool own, const bool all_valid) {
            for (int kq = kb + CHUNK * r.N; kq < ke; kq += CHUNK * r.N) {
                issue_dd(kq, ke, r);
                use_dd(kq, ke, r, own, all_valid);
            }
        };
        auto rest_x = [&](auto& r) {
            for (int j0 = CHUNK * r.N; j0 < nfill; j0 += CHUNK * r.N) {
                issue_x(j0, r);
                use_x(j0, r);
            }
        };
        const int endA = baseA + ((nfill + 3) & ~3);
        const int kown = max(k0, baseA);
        const bool all_valid = kend <= a.K;
        if constexpr (DDM == 2) {
            DdRegs<1> r;
            XRegs<XM == 2 ? 2 : 4> rx;
            issue_dd(baseA, k0, r);     use_dd(baseA, k0, r, false, false);   rest_dd(baseA, k0, r, false, false);
            issue_dd(kown, kend, r);
            if (all_valid) { use_dd(kown, kend, r, true, true);   rest_dd(kown, kend, r, true, true); }
            else           { use_dd(kown, kend, r, true, false);  rest_dd(kown, kend, r, true, false); }
            issue_dd(kend, endA, r);    use_dd(kend, endA, r, false, false);  rest_dd(kend, endA, r, false, false);
            issue_x(0, rx);             use_x(0, rx);                         rest_x(rx);
        } else {
            // Two round trips per small-patch segment: the segment's own frames (at most 704 = 3 chunks of two tensors), then
            // both halos (a chunk each) together with the x image (at most 764 floats = 3 chunks).  All of it in one batch
            // would be 13 float4 per lane and takes 127 registers; two waves per SIMD beside a weight-gradient workgroup
            // need 92 or fewer (profiles/dw_batched_resources.txt).  The scalar tap path needs more registers for its taps
            // and batches 2 chunks.  Larger patches run further batches of the same size (rest_dd / rest_x).
            constexpr int NBO = VEC4 ? 3 : 2;
            DdRegs<NBO> ro;
            issue_dd(kown, kend, ro);
            if (all_valid) { use_dd(kown, kend, ro, true, true);   rest_dd(kown, kend, ro, true, true); }
            else           { use_dd(kown, kend, ro, true, false);  rest_dd(kown, kend, ro, true, false); }
            DdRegs<1> rl, rr;
            XRegs<NBO> rx;
            issue_dd(baseA, k0, rl);
            issue_dd(kend, endA, rr);
            issue_x(0, rx);
            use_dd(baseA, k0, rl, false, false);    rest_dd(baseA, k0, rl, false, false);
            use_dd(kend, endA, rr, false, false);   rest_dd(kend, endA, rr, false, false);
            use_x(0, rx);                           rest_x(rx);
        }
        __builtin_amdgcn_wave_barrier();   // wave-private LDS patches
        if constexpr (VEC4) {
            for (int k = k0 + lane * 4; k < kend; k += 256) {
                const int ia = k + a.padl - baseA;
                float accv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < NP; ++j)
                    if (PT || j < a.P) {
                        const float4 t = *reinterpret_cast<const float4*>(LA + ia - j * a.dil);
                        accv[0] += taps[j] * t.x; accv[1] += taps[j] * t.y; accv[2] += taps[j] * t.z; accv[3] += taps[j] * t.w;
                    }
                const float4 dq = *reinterpret_cast<const float4*>(LA + (k - baseA));
                const float ddv[4] = {dq.x, dq.y, dq.z, dq.w};
                const int ib = k - a.padl - baseB;
#pragma unroll
                for (int j = 0; j < NP; ++j)
                    if (PT || j < a.P) {
                        const float4 xq = *reinterpret_cast<const float4*>(LB + ib + j * a.dil);
                        float xv[4] = {xq.x, xq.y, xq.z, xq.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            if constexpr (XHAT) {
                                const int kk = k + e - a.padl + j * a.dil;
                                xv[e] = (kk >= 0 && kk < a.K) ? g1 * xv[e] + b1 : 0.f;
                            }
                            dD[j] += ddv[e] * xv[e];
                        }
                    }
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k + e >= a.K) accv[e] = 0.f;
                if constexpr (FUSED) {
                    const float4 hq = *reinterpret_cast<const float4*>(LB + (k - baseB));
                    const float xh[4] = {hq.x, hq.y, hq.z, hq.w};
                    float4 hr = make_float4(0.f, 0.f, 0.f, 0.f);
                    if constexpr (APPLY) { if (live) hr = ld4(y1 + k); }       // (the raw h1: its sign; the lines were just read for the image)
                    const float hv[4] = {hr.x, hr.y, hr.z, hr.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (k + e < a.K) {
                            dg1 += accv[e] * xh[e];
                            db1 += accv[e];
                            if constexpr (APPLY) accv[e] = apply1(accv[e], xh[e], hv[e]);
                            else {
                                const float t = g1 * accv[e];
                                t1 += t;
                                t2 += t * xh[e];
                            }
                        }
                }
                if (live) *reinterpret_cast<float4*>(dn1 + k) = make_float4(accv[0], accv[1], accv[2], accv[3]);
            }
        } else {
        for (int kg = k0; kg < kend; kg += 64) {
            const int k = kg + lane;
            // a 64-frame group whose taps all stay inside [0, K) (uniform test) needs no per-lane predicates
            if (kg - a.padl >= 0 && kg + 63 - a.padl + halo < a.K && kg + 63 < kend) {
                float acc = 0.f;
                const int ia = k + a.padl - baseA, ib = k - a.padl - baseB;
#pragma unroll
                for (int j = 0; j < NP; ++j)
                    if (PT || j < a.P) {
                        acc += taps[j] * LA[ia - j * a.dil];
                        float xv = LB[ib + j * a.dil];
                        if constexpr (XHAT) xv = g1 * xv + b1;
                        dD[j] += LA[k - baseA] * xv;
                    }
                if constexpr (FUSED) {
                    const float xh1 = LB[k - baseB];
                    dg1 += acc * xh1;
                    db1 += acc;
                    if constexpr (APPLY) acc = apply1(acc, xh1, live ? y1[k] : 0.f);
                    else {
                        const float t = g1 * acc;
                        t1 += t;
                        t2 += t * xh1;
                    }
                }
                if (live) dn1[k] = acc;
                continue;
            }
            if (k >= kend) continue;
            // input gradient: transposed taps
            float acc = 0.f;
            const int ia = k + a.padl - baseA;
#pragma unroll
            for (int j = 0; j < NP; ++j)
                if (PT || j < a.P) acc += taps[j] * LA[ia - j * a.dil];
            if (k >= a.K) acc = 0.f;
            // tap gradients
            const float ddk = LA[k - baseA];
            const int ib = k - a.padl - baseB;
#pragma unroll
            for (int j = 0; j < NP; ++j)
                if (PT || j < a.P) {
                    const int kk = k - a.padl + j * a.dil;
                    float xv = LB[ib + j * a.dil];
                    if constexpr (XHAT) xv = (kk >= 0 && kk < a.K) ? g1 * xv + b1 : 0.f;
                    dD[j] += ddk * xv;
                }
            if constexpr (FUSED) {
                if (k < a.K) {
                    const float xh1 = LB[k - baseB];
                    dg1 += acc * xh1;
                    db1 += acc;
                    if constexpr (APPLY) acc = apply1(acc, xh1, live ? y1[k] : 0.f);
                    else {
                        const float t = g1 * acc;
                        t1 += t;
                        t2 += t * xh1;
                    }
                }
            }
            if (live) dn1[k] = acc;
        }
        }
        __builtin_amdgcn_wave_barrier();
    }
    const size_t MH = (size_t)a.M * a.H, rc = (size_t)m * a.H + c;
#pragma unroll
    for (int j = 0; j < NP; ++j)
        if (PT || j < a.P) {
            const float v = wave_sum(dD[j]);
            if (live && lane == 0) a.pc[(size_t)j * MH + rc] = v;
        }
    if constexpr (DDM == 2) {
        const float v0 = wave_sum(dg2), v1 = wave_sum(db2), v4 = wave_sum(dal2);
        if (live && lane == 0) {
            a.pc[(size_t)(P_ + 0) * MH + rc] = v0;
            a.pc[(size_t)(P_ + 1) * MH + rc] = v1;
            a.pc[(size_t)(P_ + 2) * MH + rc] = v4;
        }
    }
    if constexpr (FUSED) {
        const float v0 = wave_sum(dg2), v1 = wave_sum(db2), v2 = wave_sum(dg1), v3 = wave_sum(db1), v4 = wave_sum(dal2);
        const double w1 = wave_sum((double)t1), w2 = wave_sum((double)t2);
        if (live && lane == 0) {
            a.pc[(size_t)(P_ + 0) * MH + rc] = v0;
            a.pc[(size_t)(P_ + 1) * MH + rc] = v1;
            a.pc[(size_t)(P_ + 2) * MH + rc] = v2;
            a.pc[(size_t)(P_ + 3) * MH + rc] = v3;
            a.pc[(size_t)(P_ + 4) * MH + rc] = v4;
            if constexpr (!APPLY) {
                a.sums1_part[rc * 2] = w1;
                a.sums1_part[rc * 2 + 1] = w2;
            }
        }
        if constexpr (APPLY) {
            const float v5 = wave_sum(dal1);
            if (live && lane == 0) a.pc[(size_t)(P_ + 5) * MH + rc] = v5;
            // (a dead wave's image is 0, but apply1 still gives it -rstd1 S1'/n: it must not reach the maximum)
            if (a.amax_out != nullptr) block_amax_atomic<NT>(live ? amax1 : 0.f, red, a.amax_out + (size_t)m * CTN_AMAX_SLOTS, blockIdx.x % hb);
        }
    }
}

// ---------------------------------------------------------------------------
// dY = rstd*(g*dN - S1/n - xh*S2/n) * prelu'(y),  xh = (prelu(y)-mean)*rstd ; dalpha partial per row
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void gln_prelu_bwd_kernel(const float* __restrict__ dN, const float* __restrict__ Y,
                                                           float* __restrict__ dY, int M, int H, int K, int Kp,
                                                           const float* __restrict__ gamma, const float* __restrict__ alpha_p,
                                                           const float* __restrict__ ms, const double* __restrict__ sums_part,
                                                           int nparts, float* __restrict__ dalpha_part,
                                                           unsigned* __restrict__ amax_out) {
    __shared__ double red[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (scalar: the row and its buffer resources are wave-uniform)
    const int hb = (H + ROWS - 1) / ROWS;
    const int m = blockIdx.x / hb;
    const int c = (blockIdx.x % hb) * ROWS + wave;
    double S1 = 0.0, S2 = 0.0;
    for (int i = tid; i < nparts; i += NT) {
        S1 += sums_part[((size_t)m * nparts + i) * 2];
        S2 += sums_part[((size_t)m * nparts + i) * 2 + 1];
    }
    S1 = block_sum<double, NT>(S1, red);
    S2 = block_sum<double, NT>(S2, red);
    const bool live = c < H;
    const double n = (double)H * (double)K;
    const float c1 = (float)(S1 / n), c2 = (float)(S2 / n);
    const float mean = ms[2 * m], rstd = ms[2 * m + 1], al = alpha_p[0], g = live ? gamma[c] : 0.f;
    const float ar = al * rstd, mr = mean * rstd, rg = rstd * g, rc1 = rstd * c1, rc2 = rstd * c2;
    const size_t row = ((size_t)m * H + (live ? c : 0)) * Kp;
    const unsigned rbytes = live ? (unsigned)Kp * 4u : 0u;
    const __amdgpu_buffer_rsrc_t rsN = make_rsrc(dN + row, rbytes), rsY = make_rsrc(Y + row, rbytes);
    float dal = 0.f, amax = 0.f;
    // The row goes in batches of NB chunks through a ring of NB register slots: the 2 NB loads of the first batch are issued
    // before the first use, and a slot is reloaded for the next batch as soon as its chunk has been stored, so 2 NB loads
    // stay in flight.  Arithmetic and stores run chunk by chunk in the order of frames (dal and amax take their terms as
    // before).  dY may be dN: a lane only ever writes frames that it has read, and reads every frame before it writes it.
    constexpr int NB = 4;
    float4 rn[NB], ry[NB];
    auto issue = [&](int i, int k) {
        const int off = row_voff(k, Kp, true);
        rn[i] = buf_ld4(rsN, off);
        ry[i] = buf_ld4(rsY, off);
    };
    auto batch = [&](int kq, const bool full) {             // full: all NB chunks lie inside the row (uniform)
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int k = kq + CHUNK * i + lane * 4;
            if (full || k < Kp) {
                const float dv[4] = {rn[i].x, rn[i].y, rn[i].z, rn[i].w};
                const float yv[4] = {ry[i].x, ry[i].y, ry[i].z, ry[i].w};
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float xh = fmaf(yv[e], yv[e] >= 0.f ? rstd : ar, -mr);
                    const float da = fmaf(-xh, rc2, fmaf(rg, dv[e], -rc1));
                    const bool valid = (k + e) < K;
                    if (valid && yv[e] < 0.f) dal += da * yv[e];
                    o[e] = valid ? (yv[e] >= 0.f ? da : al * da) : 0.f;
                }
                amax = fmaxf(fmaxf(amax, fmaxf(fabsf(o[0]), fabsf(o[1]))), fmaxf(fabsf(o[2]), fabsf(o[3])));
                *reinterpret_cast<float4*>(dY + row + k) = make_float4(o[0], o[1], o[2], o[3]);
            }
            if (full) issue(i, k + CHUNK * NB);              // (past the row: offset out of range, reads 0, never used)
        }
    };
    if (live) {
#pragma unroll
        for (int i = 0; i < NB; ++i) issue(i, CHUNK * i + lane * 4);
        int kq = 0;
        for (; kq + CHUNK * NB <= Kp; kq += CHUNK * NB) batch(kq, true);
        if (kq < Kp) batch(kq, false);                      // the ragged tail: chunks past the row hold 0 and store nothing
    }
    dal = wave_sum(dal);
    if (live && lane == 0) dalpha_part[(size_t)m * H + c] = dal;
    if (amax_out != nullptr) block_amax_atomic<NT>(amax, red, amax_out + (size_t)m * CTN_AMAX_SLOTS, blockIdx.x % hb);
}

// ---------------------------------------------------------------------------
// Stand-alone gLN(prelu(Y)) backward, first pass (the fused path gets these sums from the GEMM / depthwise epilogues):
// per (utterance, channel) row  S1 = sum_k g*dN, S2 = sum_k g*dN*xh  -> sums_part [M, H, 2] fp64, and the parameter-
// gradient partials  pc[0] = sum_k dN*xh (dgamma), pc[1] = sum_k dN (dbeta)  -> pc [2, M, H].
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void gln_bwd_sums_kernel(const float* __restrict__ dN, const float* __restrict__ Y,
                                                          int M, int H, int K, int Kp, const float* __restrict__ gamma,
                                                          const float* __restrict__ alpha_p, const float* __restrict__ ms,
                                                          double* __restrict__ sums_part, float* __restrict__ pc) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hb = (H + ROWS - 1) / ROWS;
    const int m = blockIdx.x / hb;
    const int c = (blockIdx.x % hb) * ROWS + wave;
    if (c >= H) return;
    const float mean = ms[2 * m], rstd = ms[2 * m + 1], al = alpha_p[0], g = gamma[c];
    const size_t row = ((size_t)m * H + c) * Kp;
    float sdn = 0.f, sdx = 0.f;
    for (int k = lane * 4; k < Kp; k += 256) {
        const float4 dn = ld4(dN + row + k);
        const float4 y = ld4(Y + row + k);
        const float dv[4] = {dn.x, dn.y, dn.z, dn.w};
        const float yv[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < K) {
                const float xh = (prelu_f(yv[e], al) - mean) * rstd;
                sdn += dv[e];
                sdx = fmaf(dv[e], xh, sdx);
            }
    }
    const double d1 = wave_sum((double)sdn), d2 = wave_sum((double)sdx);
    if (lane == 0) {
        sums_part[((size_t)m * H + c) * 2] = (double)g * d1;
        sums_part[((size_t)m * H + c) * 2 + 1] = (double)g * d2;
        pc[(size_t)m * H + c] = (float)d2;
        pc[(size_t)(M + m) * H + c] = (float)d1;
    }
}

// out[f][i] = sum_mid in[f][mid][i]   (fixed order).  mode 0: thread per output; mode 1: workgroup per output.
__global__ __launch_bounds__(NT) void reduce_mid_kernel(const float* __restrict__ in, int F, int Mid, int Inner,
                                                        float* __restrict__ out, int wave_mode) {
    if (!wave_mode) {
        const long long o = (long long)blockIdx.x * NT + threadIdx.x;
        if (o >= (long long)F * Inner) return;
        const int f = (int)(o / Inner), i = (int)(o % Inner);
        float s = 0.f;
        for (int r = 0; r < Mid; ++r) s += in[((size_t)f * Mid + r) * Inner + i];
        out[o] = s;
    } else {                                        // one workgroup per output
        __shared__ float red[NT / 64];
        const long long o = blockIdx.x;
        const int f = (int)(o / Inner), i = (int)(o % Inner);
        float s = 0.f;
        for (int r = threadIdx.x; r < Mid; r += NT) s += in[((size_t)f * Mid + r) * Inner + i];
        s = block_sum<float, NT>(s, red);
        if (threadIdx.x == 0) out[o] = s;
    }
}

// Finish the per-(m,c) partials of dw_bwd<FUSED>:  pc [P+5, M, H] -> dD [H,P], dgamma2, dbeta2, dgamma1, dbeta1 [H],
// dalpha2 [1].  Blocks 0..nb-2 do the per-channel sums over m (thread per (f,h)); the last block sums dalpha2.
__global__ __launch_bounds__(NT) void dw_bwd_finalize_kernel(const float* __restrict__ pc, int P, int M, int H,
                                                             float* __restrict__ dD, float* __restrict__ dg2,
                                                             float* __restrict__ db2, float* __restrict__ dg1,
                                                             float* __restrict__ db1, float* __restrict__ da2,
                                                             const float* __restrict__ da1_part, int n_da1,
                                                             float* __restrict__ da1) {
    __shared__ float red[NT / 64];
    const size_t MH = (size_t)M * H;
    if (blockIdx.x == gridDim.x - 1) {                 // dalpha1 from gln_prelu_bwd's per-row partials (optional)
        if (da1_part == nullptr) return;
        float s = 0.f;
        for (int i = threadIdx.x; i < n_da1; i += NT) s += da1_part[i];
        s = block_sum<float, NT>(s, red);
        if (threadIdx.x == 0) da1[0] = s;
        return;
    }
    if (blockIdx.x == gridDim.x - 2) {
        float s = 0.f;
        const float* src = pc + (size_t)(P + 4) * MH;
        for (size_t i = threadIdx.x; i < MH; i += NT) s += src[i];
        s = block_sum<float, NT>(s, red);
        if (threadIdx.x == 0) da2[0] = s;
        return;
    }
    const int o = blockIdx.x * NT + threadIdx.x;
    if (o >= (P + 4) * H) return;
    const int f = o / H, h = o % H;
    float s = 0.f;
    for (int m = 0; m < M; ++m) s += pc[(size_t)f * MH + (size_t)m * H + h];
    if (f < P) dD[(size_t)h * P + f] = s;
    else if (f == P) dg2[h] = s;
    else if (f == P + 1) db2[h] = s;
    else if (f == P + 2) dg1[h] = s;
    else db1[h] = s;
}

// Finish the per-(m,c) partials of dw_bwd<CLN>: pc [P+3, M, H] -> dD [H,P], dgamma2, dbeta2 [H] (sums over m in a fixed order), dalpha2 [1]
// (last workgroup).
__global__ __launch_bounds__(NT) void dw_bwd_cln_finalize_kernel(const float* __restrict__ pc, int P, int M, int H, float* __restrict__ dD,
                                                                 float* __restrict__ dg2, float* __restrict__ db2, float* __restrict__ da2) {
    __shared__ float red[NT / 64];
    const size_t MH = (size_t)M * H;
    if (blockIdx.x == gridDim.x - 1) {
        float s = 0.f;
        const float* src = pc + (size_t)(P + 2) * MH;
        for (size_t i = threadIdx.x; i < MH; i += NT) s += src[i];
        s = block_sum<float, NT>(s, red);
        if (threadIdx.x == 0) da2[0] = s;
        return;
    }
    const int o = blockIdx.x * NT + threadIdx.x;
    if (o >= (P + 2) * H) return;
    const int f = o / H, h = o % H;
    float s = 0.f;
    for (int m = 0; m < M; ++m) s += pc[(size_t)f * MH + (size_t)m * H + h];
    if (f < P) dD[(size_t)h * P + f] = s;
    else if (f == P) dg2[h] = s;
    else db2[h] = s;
}

// pc [P, M, H] (the un-fused ctn_dw_bwd's tap partials) -> dD [H, P], summed over m in a fixed order
__global__ __launch_bounds__(NT) void dw_bwd_taps_kernel(const float* __restrict__ pc, int P, int M, int H, float* __restrict__ dD) {
    const int o = blockIdx.x * NT + threadIdx.x;
    if (o >= P * H) return;
    const int j = o / H, h = o % H;
    float s = 0.f;
    for (int m = 0; m < M; ++m) s += pc[((size_t)j * M + m) * H + h];
    dD[(size_t)h * P + j] = s;
}

}  // namespace

// ---------------------------------------------------------------------------
// host side of the depthwise kernels: one geometry check for all five entry points, one typed launcher per direction
// ---------------------------------------------------------------------------
enum DwPatch { DW_SMALL, DW_MEDIUM, DW_LARGE };         // LDS patch class, chosen from the halo (DW_MEDIUM: backward only)
// how dw_bwd_kernel forms its two images: the (DDM, XM) pair of the kernel's template
enum class DwBwdForm {
    PLAIN,          // (0, 0)
    GLN,            // (1, 1)
    GLN_APPLY,      // (1, 3): gLN with the first norm's backward applied to the result
    CLN,            // (2, 0)
    CLN_RECOMPUTE   // (2, 2): cLN with the first norm's output recomputed from its input
};

// Sizes, kernel size and halo parity of a depthwise call, its patch class and segment length; fills a.M .. a.seg.
// `who` is the entry point that the caller called: every message names it.
template <class Args>
static int dw_geometry(const char* who, bool bwd, int M, int H, int K, int Kp, int P, int dilation, int causal, Args& a, DwPatch* patch) {
    CTN_REQUIRE(M > 0 && H > 0 && K > 0 && Kp >= K && Kp % 4 == 0, "%s: bad sizes", who);
    CTN_REQUIRE(P >= 1 && P <= MAXP && dilation >= 1, "%s: kernel size %d unsupported (max %d)", who, P, MAXP);
    const int halo = (P - 1) * dilation;
    CTN_REQUIRE(causal || halo % 2 == 0, "%s: non-causal 'same' padding needs (P-1)*dilation even", who);
    int seg;
    if (!bwd) {
        const bool small = halo <= 192;
        *patch = small ? DW_SMALL : DW_LARGE;
        seg = (((small ? FWD_BUF_S : FWD_BUF_L) - halo - 8) / 64) * 64;
    } else {
        // patch size by halo: the dilation-128 blocks of the paper stack (halo 256) ran at 107 us with the 1792-float patches
        // (2 workgroups per CU) against 52 us for the others; 1280 floats = 960-frame segments at 4 workgroups per CU
        const bool small = halo <= 128, medium = !small && halo <= 256;
        *patch = small ? DW_SMALL : (medium ? DW_MEDIUM : DW_LARGE);
        seg = (((small ? BWD_BUF_S : (medium ? BWD_BUF_M : BWD_BUF_L)) - halo - 8) / 64) * 64;
    }
    CTN_REQUIRE(seg >= 64, "%s: receptive field (P-1)*dilation=%d too large", who, halo);
    a.M = M; a.H = H; a.K = K; a.Kp = Kp; a.P = P; a.dil = dilation;
    a.padl = causal ? halo : halo / 2; a.seg = seg;
    return CTN_OK;
}

template <int V> using DwInt = std::integral_constant<int, V>;

// patch size x float4 tap path x kernel size (3, every configuration of the paper, is compiled in; other sizes take the
// run-time-P variant) of one forward form
template <int PRO, bool EPI>
static void dw_fwd_pick(const DwFwdArgs& a, DwPatch patch, bool vec4, dim3 grid, hipStream_t st) {
    auto launch = [&](auto buf, auto v4, auto pt) {
        hipLaunchKernelGGL((dw_fwd_kernel<PRO, EPI, decltype(buf)::value, decltype(v4)::value, decltype(pt)::value>), grid, dim3(NT), 0, st, a);
    };
    auto by_p = [&](auto buf, auto v4) { if (a.P == 3) launch(buf, v4, DwInt<3>{}); else launch(buf, v4, DwInt<0>{}); };
    auto by_vec4 = [&](auto buf) { if (vec4) by_p(buf, std::true_type{}); else by_p(buf, std::false_type{}); };
    if (patch == DW_SMALL) by_vec4(DwInt<FWD_BUF_S>{});
    else by_vec4(DwInt<FWD_BUF_L>{});
}

// pro: 0 n = y, 1 gLN prologue, 2 cLN prologue; epi: the statistics epilogue (forms 0 and 1)
static int dw_fwd_launch(const char* who, const DwFwdArgs& a, int pro, bool epi, DwPatch patch, void* stream) {
    const dim3 grid((unsigned)(a.M * ctn_cdiv(a.H, ROWS)));
    hipStream_t st = (hipStream_t)stream;
    const bool vec4 = (a.dil % 4 == 0) && (a.padl % 4 == 0);
    if (pro == 2) dw_fwd_pick<2, false>(a, patch, vec4, grid, st);
    else if (pro && epi) dw_fwd_pick<1, true>(a, patch, vec4, grid, st);
    else if (pro) dw_fwd_pick<1, false>(a, patch, vec4, grid, st);
    else if (epi) dw_fwd_pick<0, true>(a, patch, vec4, grid, st);
    else dw_fwd_pick<0, false>(a, patch, vec4, grid, st);
    CTN_CHECK_LAUNCH(who);
    return CTN_OK;
}

// the same choice for one backward form
template <int DDM, int XM>
static void dw_bwd_pick(const DwBwdArgs& a, DwPatch patch, bool vec4, dim3 grid, hipStream_t st) {
    auto launch = [&](auto buf, auto v4, auto pt) {
        hipLaunchKernelGGL((dw_bwd_kernel<DDM, XM, decltype(buf)::value, decltype(v4)::value, decltype(pt)::value>), grid, dim3(NT), 0, st, a);
    };
    auto by_p = [&](auto buf, auto v4) { if (a.P == 3) launch(buf, v4, DwInt<3>{}); else launch(buf, v4, DwInt<0>{}); };
    auto by_vec4 = [&](auto buf) { if (vec4) by_p(buf, std::true_type{}); else by_p(buf, std::false_type{}); };
    if (patch == DW_SMALL) by_vec4(DwInt<BWD_BUF_S>{});
    else if (patch == DW_MEDIUM) by_vec4(DwInt<BWD_BUF_M>{});
    else by_vec4(DwInt<BWD_BUF_L>{});
}

static int dw_bwd_launch(const char* who, const DwBwdArgs& a, DwBwdForm form, DwPatch patch, void* stream) {
    const dim3 grid((unsigned)(a.M * ctn_cdiv(a.H, ROWS)));
    hipStream_t st = (hipStream_t)stream;
    // float4 compute path whenever the tap offsets keep 16-byte alignment (dilation and left pad multiples of 4): with the
    // kernel size compiled in it also wins for the small-patch variant (44.7 vs 48.5 us at dilation 4..32)
    const bool vec4 = (a.dil % 4 == 0) && (a.padl % 4 == 0);
    switch (form) {
    case DwBwdForm::PLAIN: dw_bwd_pick<0, 0>(a, patch, vec4, grid, st); break;
    case DwBwdForm::GLN: dw_bwd_pick<1, 1>(a, patch, vec4, grid, st); break;
    case DwBwdForm::GLN_APPLY: dw_bwd_pick<1, 3>(a, patch, vec4, grid, st); break;
    case DwBwdForm::CLN: dw_bwd_pick<2, 0>(a, patch, vec4, grid, st); break;
    case DwBwdForm::CLN_RECOMPUTE: dw_bwd_pick<2, 2>(a, patch, vec4, grid, st); break;
    }
    CTN_CHECK_LAUNCH(who);
    return CTN_OK;
}

extern "C" {

int ctn_dw_fwd(const float* Y, float* Z, const float* D, int M, int H, int K, int Kp, int P, int dilation, int causal,
               const double* pro_part, int pro_nparts, const float* pro_gamma, const float* pro_beta,
               const float* pro_alpha, float* pro_ms_out, const float* epi_alpha, double* epi_part, unsigned* amax_out,
               void* stream) {
    CTN_REQUIRE(Y && Z && D, "ctn_dw_fwd: null pointer");
    CTN_REQUIRE(!amax_out || epi_part, "ctn_dw_fwd: amax_out comes with the statistics epilogue");
    DwFwdArgs a{};
    DwPatch patch;
    if (const int rc = dw_geometry("ctn_dw_fwd", false, M, H, K, Kp, P, dilation, causal, a, &patch)) return rc;
    CTN_REQUIRE(ctn_aligned16(Y) && ctn_aligned16(Z), "ctn_dw_fwd: pointers must be 16-byte aligned");
    CTN_REQUIRE(!pro_part || (pro_gamma && pro_beta && pro_alpha && pro_nparts > 0), "ctn_dw_fwd: incomplete prologue arguments");
    CTN_REQUIRE(!epi_part || epi_alpha, "ctn_dw_fwd: stats epilogue needs alpha");
    a.Y = Y; a.Z = Z; a.D = D;
    a.pro_part = pro_part; a.pro_nparts = pro_nparts; a.pro_gamma = pro_gamma; a.pro_beta = pro_beta;
    a.pro_alpha = pro_alpha; a.pro_ms_out = pro_ms_out; a.epi_alpha = epi_alpha; a.epi_part = epi_part;
    a.amax_out = amax_out;
    return dw_fwd_launch("ctn_dw_fwd", a, pro_part ? 1 : 0, epi_part != nullptr, patch, stream);
}

// channel-wise LayerNorm form (round 4): n = gamma ((prelu(Y, alpha) - mean[k]) rstd[k]) + beta with the per-frame statistics that
// ctn_cln_stats_frame made of the producing GEMM's column partials; no separate norm pass, the norm's output is never stored
int ctn_dw_fwd_cln(const float* Y, float* Z, const float* D, int M, int H, int K, int Kp, int P, int dilation, int causal,
                   const float* mean, const float* rstd, const float* gamma, const float* beta, const float* alpha, void* stream) {
    CTN_REQUIRE(Y && Z && D && mean && rstd && gamma && beta && alpha, "ctn_dw_fwd_cln: null pointer");
    DwFwdArgs a{};
    DwPatch patch;
    if (const int rc = dw_geometry("ctn_dw_fwd_cln", false, M, H, K, Kp, P, dilation, causal, a, &patch)) return rc;
    CTN_REQUIRE(ctn_aligned16(Y) && ctn_aligned16(Z) && ctn_aligned16(mean) && ctn_aligned16(rstd), "ctn_dw_fwd_cln: pointers must be 16-byte aligned");
    a.Y = Y; a.Z = Z; a.D = D;
    a.pro_gamma = gamma; a.pro_beta = beta; a.pro_alpha = alpha; a.cln_mean = mean; a.cln_rstd = rstd;
    return dw_fwd_launch("ctn_dw_fwd_cln", a, 2, false, patch, stream);
}

int ctn_dw_bwd_rows(int P, int fused) { return fused == 1 ? P + 5 : (fused == 2 ? P + 3 : (fused == 3 ? P + 6 : P)); }

// see include/ctn_hip.h.  pc is [F, M, H] with F = ctn_dw_bwd_rows(P, fused)
int ctn_dw_bwd(const float* dN2, const float* Dz, const float* Y1, float* dN1, const float* D,
               int M, int H, int K, int Kp, int P, int dilation, int causal, int fused,
               const float* g1, const float* b1, const float* a1, const float* ms1,
               const float* g2, const float* a2, const float* ms2,
               const double* sums2_part, int sums2_nparts, float* pc, double* sums1_part, void* stream) {
    CTN_REQUIRE(fused != 2, "ctn_dw_bwd: fused = 2 (the cLN form) has an entry point of its own: ctn_dw_bwd_cln");
    CTN_REQUIRE(fused != 3, "ctn_dw_bwd: fused = 3 (gLN + the first norm's backward) has an entry point of its own: ctn_dw_bwd_gln2");
    CTN_REQUIRE(fused == 0 || fused == 1, "ctn_dw_bwd: fused must be 0 (plain) or 1 (gLN)");
    CTN_REQUIRE(dN2 && Y1 && dN1 && D && pc, "ctn_dw_bwd: null pointer");
    DwBwdArgs a{};
    DwPatch patch;
    if (const int rc = dw_geometry("ctn_dw_bwd", true, M, H, K, Kp, P, dilation, causal, a, &patch)) return rc;
    CTN_REQUIRE(ctn_aligned16(dN2) && ctn_aligned16(Y1) && ctn_aligned16(dN1) && (!fused || ctn_aligned16(Dz)), "ctn_dw_bwd: alignment");
    if (fused)
        CTN_REQUIRE(Dz && g1 && b1 && a1 && ms1 && g2 && a2 && ms2 && sums2_part && sums2_nparts > 0 && sums1_part,
                    "ctn_dw_bwd: fused mode needs every norm argument");
    a.dN2 = dN2; a.Dz = Dz; a.Y1 = Y1; a.dN1 = dN1; a.D = D;
    a.g1 = g1; a.b1 = b1; a.a1 = a1; a.ms1 = ms1; a.g2 = g2; a.a2 = a2; a.ms2 = ms2;
    a.sums2_part = sums2_part; a.sums2_nparts = sums2_nparts; a.pc = pc; a.sums1_part = sums1_part;
    return dw_bwd_launch("ctn_dw_bwd", a, fused ? DwBwdForm::GLN : DwBwdForm::PLAIN, patch, stream);
}

int ctn_dw_bwd_finalize(const float* pc, int P, int M, int H, float* dD, float* dgamma2, float* dbeta2,
                        float* dgamma1, float* dbeta1, float* dalpha2, const float* dalpha1_part, int n_dalpha1,
                        float* dalpha1, void* stream) {
    CTN_REQUIRE(pc && dD && dgamma2 && dbeta2 && dgamma1 && dbeta1 && dalpha2, "ctn_dw_bwd_finalize: null pointer");
    CTN_REQUIRE(P >= 1 && P <= MAXP && M > 0 && H > 0, "ctn_dw_bwd_finalize: bad sizes");
    CTN_REQUIRE(!dalpha1_part || (dalpha1 && n_dalpha1 > 0), "ctn_dw_bwd_finalize: incomplete dalpha1 arguments");
    const unsigned nb = (unsigned)ctn_cdiv((P + 4) * H, NT) + 2;
    hipLaunchKernelGGL(dw_bwd_finalize_kernel, dim3(nb), dim3(NT), 0, (hipStream_t)stream, pc, P, M, H, dD, dgamma2,
                       dbeta2, dgamma1, dbeta1, dalpha2, dalpha1_part, n_dalpha1, dalpha1);
    CTN_CHECK_LAUNCH("ctn_dw_bwd_finalize");
    return CTN_OK;
}

// gLN form with the first norm's backward applied (round 4): see include/ctn_hip.h.  sums2_part [M, nparts, 8] from ctn_pw_dgrad_gln2;
// dY1 = gLN1' . PReLU1'(dN1) [M,H,Kp]; pc [P+6, M, H] (rows as fused = 1, plus P+5: dalpha1 partials); amax_out optional (h3).
int ctn_dw_bwd_gln2(const float* dN2, const float* Dz, const float* Y1, float* dY1, const float* D,
                    int M, int H, int K, int Kp, int P, int dilation, int causal,
                    const float* g1, const float* b1, const float* a1, const float* ms1,
                    const float* g2, const float* a2, const float* ms2,
                    const double* sums2_part, int sums2_nparts, float* pc, unsigned* amax_out, void* stream) {
    CTN_REQUIRE(dN2 && Y1 && dY1 && D && pc, "ctn_dw_bwd_gln2: null pointer");
    DwBwdArgs a{};
    DwPatch patch;
    if (const int rc = dw_geometry("ctn_dw_bwd_gln2", true, M, H, K, Kp, P, dilation, causal, a, &patch)) return rc;
    CTN_REQUIRE(ctn_aligned16(dN2) && ctn_aligned16(Y1) && ctn_aligned16(dY1) && ctn_aligned16(Dz), "ctn_dw_bwd_gln2: alignment");
    CTN_REQUIRE(Dz && g1 && b1 && a1 && ms1 && g2 && a2 && ms2 && sums2_part && sums2_nparts > 0,
                "ctn_dw_bwd_gln2: needs every norm argument");
    a.dN2 = dN2; a.Dz = Dz; a.Y1 = Y1; a.dN1 = dY1; a.D = D;
    a.g1 = g1; a.b1 = b1; a.a1 = a1; a.ms1 = ms1; a.g2 = g2; a.a2 = a2; a.ms2 = ms2;
    a.sums2_part = sums2_part; a.sums2_nparts = sums2_nparts; a.pc = pc; a.amax_out = amax_out;
    return dw_bwd_launch("ctn_dw_bwd_gln2", a, DwBwdForm::GLN_APPLY, patch, stream);
}

// cLN form (round 4): see include/ctn_hip.h
int ctn_dw_bwd_cln(const float* dN2, const float* Dz, const float* X1, float* dN1, const float* D,
                   int M, int H, int K, int Kp, int P, int dilation, int causal,
                   const float* g2, const float* a2, const float* fc,
                   const float* g1, const float* b1, const float* a1, const float* mean1, const float* rstd1,
                   float* pc, void* stream) {
    CTN_REQUIRE((g1 == nullptr) == (mean1 == nullptr) && (g1 == nullptr) == (rstd1 == nullptr), "ctn_dw_bwd_cln: first-norm arguments come together");
    CTN_REQUIRE(dN2 && X1 && dN1 && D && pc, "ctn_dw_bwd_cln: null pointer");
    DwBwdArgs a{};
    DwPatch patch;
    if (const int rc = dw_geometry("ctn_dw_bwd_cln", true, M, H, K, Kp, P, dilation, causal, a, &patch)) return rc;
    CTN_REQUIRE(ctn_aligned16(dN2) && ctn_aligned16(X1) && ctn_aligned16(dN1) && ctn_aligned16(Dz), "ctn_dw_bwd_cln: alignment");
    CTN_REQUIRE(Dz && g2 && a2 && fc && ctn_aligned16(fc), "ctn_dw_bwd_cln: null or unaligned argument");
    const bool recompute = g1 != nullptr;       // the first norm's output is recomputed from X1 = its input
    CTN_REQUIRE(!recompute || (b1 && a1 && ctn_aligned16(mean1) && ctn_aligned16(rstd1)), "ctn_dw_bwd_cln: incomplete first-norm arguments");
    a.dN2 = dN2; a.Dz = Dz; a.Y1 = X1; a.dN1 = dN1; a.D = D;
    a.g1 = g1; a.b1 = b1; a.a1 = a1; a.g2 = g2; a.a2 = a2; a.pc = pc;
    a.fc2 = fc; a.mean1f = mean1; a.rstd1f = rstd1;
    return dw_bwd_launch("ctn_dw_bwd_cln", a, recompute ? DwBwdForm::CLN_RECOMPUTE : DwBwdForm::CLN, patch, stream);
}

int ctn_dw_bwd_cln_finalize(const float* pc, int P, int M, int H, float* dD, float* dgamma2, float* dbeta2, float* dalpha2,
                            void* stream) {
    CTN_REQUIRE(pc && dD && dgamma2 && dbeta2 && dalpha2, "ctn_dw_bwd_cln_finalize: null pointer");
    CTN_REQUIRE(P >= 1 && P <= MAXP && M > 0 && H > 0, "ctn_dw_bwd_cln_finalize: bad sizes");
    const unsigned nb = (unsigned)ctn_cdiv((P + 2) * H, NT) + 1;
    hipLaunchKernelGGL(dw_bwd_cln_finalize_kernel, dim3(nb), dim3(NT), 0, (hipStream_t)stream, pc, P, M, H, dD, dgamma2, dbeta2, dalpha2);
    CTN_CHECK_LAUNCH("ctn_dw_bwd_cln_finalize");
    return CTN_OK;
}

int ctn_dw_bwd_taps(const float* pc, int P, int M, int H, float* dD, void* stream) {
    CTN_REQUIRE(pc && dD && P >= 1 && P <= MAXP && M > 0 && H > 0, "ctn_dw_bwd_taps: bad arguments");
    hipLaunchKernelGGL(dw_bwd_taps_kernel, dim3((unsigned)ctn_cdiv(P * H, NT)), dim3(NT), 0, (hipStream_t)stream, pc, P, M, H, dD);
    CTN_CHECK_LAUNCH("ctn_dw_bwd_taps");
    return CTN_OK;
}

int ctn_gln_prelu_bwd(const float* dN, const float* Y, float* dY, int M, int H, int K, int Kp,
                      const float* gamma, const float* alpha, const float* ms, const double* sums_part, int nparts,
                      float* dalpha_part, unsigned* amax_out, void* stream) {
    CTN_REQUIRE(dN && Y && dY && gamma && alpha && ms && sums_part && dalpha_part && nparts > 0, "ctn_gln_prelu_bwd: null pointer");
    CTN_REQUIRE(M > 0 && H > 0 && K > 0 && Kp >= K && Kp % 4 == 0, "ctn_gln_prelu_bwd: bad sizes");
    CTN_REQUIRE(ctn_aligned16(dN) && ctn_aligned16(Y) && ctn_aligned16(dY), "ctn_gln_prelu_bwd: alignment");
    hipLaunchKernelGGL(gln_prelu_bwd_kernel, dim3((unsigned)(M * ctn_cdiv(H, ROWS))), dim3(NT), 0, (hipStream_t)stream,
                       dN, Y, dY, M, H, K, Kp, gamma, alpha, ms, sums_part, nparts, dalpha_part, amax_out);
    CTN_CHECK_LAUNCH("ctn_gln_prelu_bwd");
    return CTN_OK;
}

int ctn_gln_bwd_sums(const float* dN, const float* Y, int M, int H, int K, int Kp, const float* gamma, const float* alpha,
                     const float* ms, double* sums_part, float* pc, void* stream) {
    CTN_REQUIRE(dN && Y && gamma && alpha && ms && sums_part && pc, "ctn_gln_bwd_sums: null pointer");
    CTN_REQUIRE(M > 0 && H > 0 && K > 0 && Kp >= K && Kp % 4 == 0, "ctn_gln_bwd_sums: bad sizes");
    CTN_REQUIRE(ctn_aligned16(dN) && ctn_aligned16(Y), "ctn_gln_bwd_sums: alignment");
    hipLaunchKernelGGL(gln_bwd_sums_kernel, dim3((unsigned)(M * ctn_cdiv(H, ROWS))), dim3(NT), 0, (hipStream_t)stream,
                       dN, Y, M, H, K, Kp, gamma, alpha, ms, sums_part, pc);
    CTN_CHECK_LAUNCH("ctn_gln_bwd_sums");
    return CTN_OK;
}

 // ctn_tune("gln_fuse", 0 | 1): composite gLN stacks without the gLN-1' / PReLU-1' pass (ctn_pw_dgrad_gln2 + ctn_dw_bwd_gln2)
int g_ctn_gln_fuse = -1;
int ctn_gln_fuse(void) {         // (CTN_GLN_FUSE=0|1 at first use; default below)
    if (g_ctn_gln_fuse < 0) {
        const char* e = getenv("CTN_GLN_FUSE");
        g_ctn_gln_fuse = (e && (*e == '0' || *e == '1') && !e[1]) ? *e - '0' : 0;      // measured slower in the step (profiles/README.md r04_m): off
    }
    return g_ctn_gln_fuse;
}

int ctn_reduce_mid(const float* in, float* out, int F, int Mid, int Inner, void* stream) {
    CTN_REQUIRE(in && out && F > 0 && Mid > 0 && Inner > 0, "ctn_reduce_mid: bad arguments");
    const long long n = (long long)F * Inner;
    const int wave_mode = (Mid >= 256 && n <= 4096) ? 1 : 0;
    const unsigned blocks = wave_mode ? (unsigned)n : (unsigned)ctn_cdivll(n, NT);
    hipLaunchKernelGGL(reduce_mid_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, in, F, Mid, Inner, out, wave_mode);
    CTN_CHECK_LAUNCH("ctn_reduce_mid");
    return CTN_OK;
}

}  // extern "C"
