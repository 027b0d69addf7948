// Channel-wise LayerNorm (src/conv_tasnet.py:313-335) of the causal variant and the input norm (:172), gfx950.
//
//  * forward / backward in three generations: the 16-byte "v4" kernels that the stacks run, and the register-resident and
//    generic kernels behind them for very wide layers or unaligned frames.
//  * the fixed-order finish of the parameter-gradient partials.
//  * the per-frame statistics / backward constants made of a GEMM epilogue's column partials, for the forms in which the norm
//    rides inside its neighbours (ctn_pw_gemm_cln / ctn_dw_fwd_cln, ctn_pw_dgrad_cln / ctn_dw_bwd_cln).
//
// All cross-lane / cross-block sums have a fixed order (no float atomics), so a step is bitwise reproducible run to run.
#include "ctn_common.h"
#include <stdlib.h>

namespace {

constexpr int NT = 256;
constexpr int ROWS = 4;          // one wave per row (cln_bwd_params_kernel)

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// ---------------------------------------------------------------------------
// channel-wise LayerNorm (optionally after PReLU), per (m, frame) over channels.
// block = 64 frames x 4 channel-groups (one wave each).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void cln_fwd_kernel(const float* __restrict__ Y, float* __restrict__ Out,
                                                     float* __restrict__ mean_o, float* __restrict__ rstd_o,
                                                     int M, int Ch, int K, int Kp, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, const float* __restrict__ alpha_p) {
    __shared__ float sh[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kb = (Kp + 63) / 64;
    const int m = blockIdx.x / kb, k = (blockIdx.x % kb) * 64 + lane;
    const bool in = k < Kp;
    const bool has_a = alpha_p != nullptr;
    const float al = has_a ? alpha_p[0] : 1.f;
    const float* __restrict__ y = Y + (size_t)m * Ch * Kp + (in ? k : 0);
    float s = 0.f;
    for (int c = wave; c < Ch; c += 4) {
        float v = in ? y[(size_t)c * Kp] : 0.f;
        if (has_a) v = prelu_f(v, al);
        s += v;
    }
    sh[wave][lane] = s;
    __syncthreads();
    const float mu = (sh[0][lane] + sh[1][lane] + sh[2][lane] + sh[3][lane]) / (float)Ch;
    __syncthreads();
    float q = 0.f;
    for (int c = wave; c < Ch; c += 4) {
        float v = in ? y[(size_t)c * Kp] : 0.f;
        if (has_a) v = prelu_f(v, al);
        q += (v - mu) * (v - mu);
    }
    sh[wave][lane] = q;
    __syncthreads();
    const float var = (sh[0][lane] + sh[1][lane] + sh[2][lane] + sh[3][lane]) / (float)Ch;
    const float rs = 1.0f / sqrtf(var + CTN_EPS);
    if (wave == 0 && in) {
        mean_o[(size_t)m * Kp + k] = mu;
        rstd_o[(size_t)m * Kp + k] = rs;
    }
    if (!in) return;
    float* __restrict__ o = Out + (size_t)m * Ch * Kp + k;
    const bool valid = k < K;
    for (int c = wave; c < Ch; c += 4) {
        float v = y[(size_t)c * Kp];
        if (has_a) v = prelu_f(v, al);
        o[(size_t)c * Kp] = valid ? gamma[c] * ((v - mu) * rs) + beta[c] : 0.f;
    }
}

// dY = [ rstd*(t - mean_c(t) - xh*mean_c(t*xh)) * prelu'(y) + add ] * (relu_ref > 0)
__global__ __launch_bounds__(NT) void cln_bwd_dx_kernel(const float* __restrict__ dOut, const float* __restrict__ Y,
                                                        float* __restrict__ dY, const float* __restrict__ mean_i,
                                                        const float* __restrict__ rstd_i, int M, int Ch, int K, int Kp,
                                                        const float* __restrict__ gamma, const float* __restrict__ alpha_p,
                                                        const float* __restrict__ add, const float* __restrict__ relu_ref,
                                                        float* __restrict__ dalpha_part) {
    __shared__ float sh[2][4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kb = (Kp + 63) / 64;
    const int m = blockIdx.x / kb, k = (blockIdx.x % kb) * 64 + lane;
    const bool in = k < Kp, valid = k < K;
    const bool has_a = alpha_p != nullptr;
    const float al = has_a ? alpha_p[0] : 1.f;
    const size_t off = (size_t)m * Ch * Kp + (in ? k : 0);
    const float mu = in ? mean_i[(size_t)m * Kp + k] : 0.f, rs = in ? rstd_i[(size_t)m * Kp + k] : 0.f;
    float s1 = 0.f, s2 = 0.f;
    for (int c = wave; c < Ch; c += 4) {
        if (valid) {
            float v = Y[off + (size_t)c * Kp];
            if (has_a) v = prelu_f(v, al);
            const float t = gamma[c] * dOut[off + (size_t)c * Kp];
            s1 += t;
            s2 += t * ((v - mu) * rs);
        }
    }
    sh[0][wave][lane] = s1;
    sh[1][wave][lane] = s2;
    __syncthreads();
    const float m1 = (sh[0][0][lane] + sh[0][1][lane] + sh[0][2][lane] + sh[0][3][lane]) / (float)Ch;
    const float m2 = (sh[1][0][lane] + sh[1][1][lane] + sh[1][2][lane] + sh[1][3][lane]) / (float)Ch;
    float dal = 0.f;
    if (in) {
        for (int c = wave; c < Ch; c += 4) {
            const size_t o = off + (size_t)c * Kp;
            float r = 0.f;
            if (valid) {
                const float yv = Y[o];
                const float v = has_a ? prelu_f(yv, al) : yv;
                const float xh = (v - mu) * rs;
                const float da = rs * (gamma[c] * dOut[o] - m1 - xh * m2);
                if (has_a && yv < 0.f) dal += da * yv;
                r = (has_a && yv < 0.f) ? al * da : da;
                if (add != nullptr) r += add[o];
                if (relu_ref != nullptr && !(relu_ref[o] > 0.f)) r = 0.f;
            }
            dY[o] = r;
        }
    }
    if (dalpha_part != nullptr) {
        __syncthreads();
        dal = wave_sum(dal);
        if (lane == 0) sh[0][wave][0] = dal;
        __syncthreads();
        if (tid == 0) dalpha_part[blockIdx.x] = sh[0][0][0] + sh[0][1][0] + sh[0][2][0] + sh[0][3][0];
    }
}

// ---------------------------------------------------------------------------
// Register-resident channel-wise LayerNorm: a 1024-thread workgroup owns FR frames x all channels.  Lane l of wave w
// holds frame l % FR for channel group g = w * (64/FR) + l / FR, i.e. channels g, g + NG, ... (NG = 1024/FR groups,
// CPT channels per thread), so the tensor is read ONCE for the two-pass statistics and the normalisation (the generic
// kernels above re-read it per pass with 4 waves per 64 frames: 1.6 TB/s).  FR = 32 keeps 128-byte row segments.
// ---------------------------------------------------------------------------
constexpr int CLN_NT = 1024, CLN_FR = 32;

template <int FR, int CPT>
__global__ __launch_bounds__(CLN_NT) __attribute__((amdgpu_waves_per_eu(8, 8))) void cln_fwd_reg_kernel(const float* __restrict__ Y, float* __restrict__ Out,
                                                             float* __restrict__ mean_o, float* __restrict__ rstd_o,
                                                             int M, int Ch, int K, int Kp, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ alpha_p) {
    constexpr int NG = CLN_NT / FR;
    __shared__ float sh[NG][FR];
    const int fr = threadIdx.x % FR, g = threadIdx.x / FR;
    const int kb = (Kp + FR - 1) / FR;
    const int m = blockIdx.x / kb, k = (blockIdx.x % kb) * FR + fr;
    const bool in = k < Kp;
    const bool has_a = alpha_p != nullptr;
    const float al = has_a ? alpha_p[0] : 1.f;
    const float* __restrict__ y = Y + (size_t)m * Ch * Kp + (in ? k : 0);
    float v[CPT];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int c = g + NG * j;
        float t = (in && c < Ch) ? y[(size_t)c * Kp] : 0.f;
        if (has_a) t = prelu_f(t, al);
        v[j] = t;
        s += t;
    }
    sh[g][fr] = s;
    __syncthreads();
    float mu = 0.f;
    for (int w = 0; w < NG; ++w) mu += sh[w][fr];
    mu /= (float)Ch;
    __syncthreads();
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < CPT; ++j)
        if (g + NG * j < Ch) q += (v[j] - mu) * (v[j] - mu);
    sh[g][fr] = q;
    __syncthreads();
    float var = 0.f;
    for (int w = 0; w < NG; ++w) var += sh[w][fr];
    var /= (float)Ch;
    const float rs = 1.0f / sqrtf(var + CTN_EPS);
    if (!in) return;
    if (g == 0) {
        mean_o[(size_t)m * Kp + k] = mu;
        rstd_o[(size_t)m * Kp + k] = rs;
    }
    float* __restrict__ o = Out + (size_t)m * Ch * Kp + k;
    const bool valid = k < K;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int c = g + NG * j;
        if (c < Ch) o[(size_t)c * Kp] = valid ? gamma[c] * ((v[j] - mu) * rs) + beta[c] : 0.f;
    }
}

template <int FR, int CPT, int NTB>     // NTB threads per workgroup (512 or 1024)
__global__ __launch_bounds__(NTB) void cln_bwd_dx_reg_kernel(const float* __restrict__ dOut, const float* __restrict__ Y,
                                                                float* __restrict__ dY, const float* __restrict__ mean_i,
                                                                const float* __restrict__ rstd_i, int M, int Ch, int K, int Kp,
                                                                const float* __restrict__ gamma, const float* __restrict__ alpha_p,
                                                                const float* __restrict__ add, const float* __restrict__ relu_ref,
                                                                float* __restrict__ dalpha_part) {
    constexpr int NG = NTB / FR;
    __shared__ float sh[2][NG][FR];
    __shared__ float red[NTB / 64];
    const int fr = threadIdx.x % FR, g = threadIdx.x / FR;
    const int kb = (Kp + FR - 1) / FR;
    const int m = blockIdx.x / kb, k = (blockIdx.x % kb) * FR + fr;
    const bool in = k < Kp, valid = k < K;
    const bool has_a = alpha_p != nullptr;
    const float al = has_a ? alpha_p[0] : 1.f;
    const size_t off = (size_t)m * Ch * Kp + (in ? k : 0);
    const float mu = in ? mean_i[(size_t)m * Kp + k] : 0.f, rs = in ? rstd_i[(size_t)m * Kp + k] : 0.f;
    float t[CPT], yv[CPT];           // gamma * dOut and the raw input of this thread's channels
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int c = g + NG * j;
        const bool ok = valid && c < Ch;
        yv[j] = ok ? Y[off + (size_t)c * Kp] : 0.f;
        t[j] = ok ? gamma[c] * dOut[off + (size_t)c * Kp] : 0.f;
        const float v = has_a ? prelu_f(yv[j], al) : yv[j];
        s1 += t[j];
        s2 += ok ? t[j] * ((v - mu) * rs) : 0.f;
    }
    sh[0][g][fr] = s1;
    sh[1][g][fr] = s2;
    __syncthreads();
    float m1 = 0.f, m2 = 0.f;
    for (int w = 0; w < NG; ++w) { m1 += sh[0][w][fr]; m2 += sh[1][w][fr]; }
    m1 /= (float)Ch;
    m2 /= (float)Ch;
    float dal = 0.f;
    if (in) {
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            const int c = g + NG * j;
            if (c < Ch) {
                const size_t o = off + (size_t)c * Kp;
                float r = 0.f;
                if (valid) {
                    const float v = has_a ? prelu_f(yv[j], al) : yv[j];
                    const float xh = (v - mu) * rs;
                    const float da = rs * (t[j] - m1 - xh * m2);
                    if (has_a && yv[j] < 0.f) dal += da * yv[j];
                    r = (has_a && yv[j] < 0.f) ? al * da : da;
                    if (add != nullptr) r += add[o];
                    if (relu_ref != nullptr && !(relu_ref[o] > 0.f)) r = 0.f;
                }
                dY[o] = r;
            }
        }
    }
    if (dalpha_part != nullptr) {
        dal = block_sum<float, NTB>(dal, red);
        if (threadIdx.x == 0) dalpha_part[blockIdx.x] = dal;
    }
}

// ---------------------------------------------------------------------------
// Round-2 channel-wise LayerNorm ("v4"): 16-byte accesses along frames and ONE backward pass.
// A 512-thread workgroup owns 32 frames x all channels: thread t holds the frame quad q = t % 8 (frames 4q..4q+3) of channel
// group g = t / 8, i.e. channels g, g + 64, ... (CPT per thread).  A wave instruction then moves 8 rows x 128 bytes with
// 64 float4 accesses instead of 4-byte ones.  Per-frame sums over channels: three xor-shuffles over the 8 groups of a wave,
// then 8 float4 partials through LDS.  The backward kernel also produces the parameter-gradient partials: dgamma / dbeta of
// a channel over this workgroup's 32 frames (its 4 frames per thread, then three xor-shuffles over the 8 quads), written to
// pc [2][blocks][Ch] and summed in fixed order by cln_bwd_finalize -- the separate cln_bwd_params pass (a third read of both
// tensors) is gone.
// ---------------------------------------------------------------------------
constexpr int C4_NT = 512, C4_FR = 32, C4_NG = C4_NT / (C4_FR / 4);      // 64 channel groups

template <int FR = C4_FR>
__device__ __forceinline__ float4 quad_group_sum(float4 v) {              // sum over the channel groups of a wave (lane bits above the FR / 4 frame quads)
#pragma unroll
    for (int o = FR / 4; o < 64; o <<= 1) {
        v.x += __shfl_xor(v.x, o, 64); v.y += __shfl_xor(v.y, o, 64);
        v.z += __shfl_xor(v.z, o, 64); v.w += __shfl_xor(v.w, o, 64);
    }
    return v;
}
// sum of `v` over all channel groups of the workgroup, result for this thread's frame quad in every thread
template <int NW = C4_NT / 64, int FR = C4_FR>
__device__ __forceinline__ float4 block_group_sum(float4 v, float4 (*sh)[FR / 4], int wave, int q, int lane) {
    v = quad_group_sum<FR>(v);
    __syncthreads();                                 // sh may still be read by a previous call
    if (lane < FR / 4) sh[wave][q] = v;
    __syncthreads();
    float4 r = sh[0][q];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
        const float4 t = sh[w][q];
        r.x += t.x; r.y += t.y; r.z += t.z; r.w += t.w;
    }
    return r;
}

// (NTB, FR) = (512, 32) or (256, 16): the same channel groups and per-thread work; the small form fits more independent workgroups on a CU
template <int CPT, int NTB = C4_NT, int FR = C4_FR>
__global__ __launch_bounds__(NTB) void cln_fwd_v4_kernel(const float* __restrict__ Y, float* __restrict__ Out,
                                                           float* __restrict__ mean_o, float* __restrict__ rstd_o,
                                                           int M, int Ch, int K, int Kp, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ alpha_p,
                                                           unsigned* __restrict__ amax_out) {
    constexpr int NW = NTB / 64, NQ = FR / 4, C4_NG = NTB / NQ;
    static_assert(C4_NG == 64, "64 channel groups");
    __shared__ float4 sh[NW][NQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = tid % NQ, g = tid / NQ;
    const int kb = Kp / FR;
    const int bx = FR == 32 ? (int)blockIdx.x : xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int m = bx / kb, k0 = (bx % kb) * FR + 4 * q;
    float amax = 0.f;
    const bool has_a = alpha_p != nullptr;
    const float al = has_a ? alpha_p[0] : 1.f;
    const size_t off = (size_t)m * Ch * Kp + k0;
    float4 v[CPT];
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int c = g + C4_NG * j;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < Ch) t = ld4(Y + off + (size_t)c * Kp);
        if (has_a) { t.x = prelu_f(t.x, al); t.y = prelu_f(t.y, al); t.z = prelu_f(t.z, al); t.w = prelu_f(t.w, al); }
        v[j] = t;
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    float4 mu = block_group_sum<NW, FR>(s, sh, wave, q, lane);
    const float inv = 1.f / (float)Ch;
    mu.x *= inv; mu.y *= inv; mu.z *= inv; mu.w *= inv;
    float4 d2 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < CPT; ++j)
        if (g + C4_NG * j < Ch) {
            d2.x += (v[j].x - mu.x) * (v[j].x - mu.x); d2.y += (v[j].y - mu.y) * (v[j].y - mu.y);
            d2.z += (v[j].z - mu.z) * (v[j].z - mu.z); d2.w += (v[j].w - mu.w) * (v[j].w - mu.w);
        }
    const float4 var = block_group_sum<NW, FR>(d2, sh, wave, q, lane);
    const float4 rs = make_float4(1.0f / sqrtf(var.x * inv + CTN_EPS), 1.0f / sqrtf(var.y * inv + CTN_EPS),
                                  1.0f / sqrtf(var.z * inv + CTN_EPS), 1.0f / sqrtf(var.w * inv + CTN_EPS));
    if (g == 0) {
        *reinterpret_cast<float4*>(mean_o + (size_t)m * Kp + k0) = mu;
        *reinterpret_cast<float4*>(rstd_o + (size_t)m * Kp + k0) = rs;
    }
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int c = g + C4_NG * j;
        if (c < Ch) {
            const float ga = gamma[c], be = beta[c];
            float4 o;
            o.x = k0 + 0 < K ? ga * ((v[j].x - mu.x) * rs.x) + be : 0.f;
            o.y = k0 + 1 < K ? ga * ((v[j].y - mu.y) * rs.y) + be : 0.f;
            o.z = k0 + 2 < K ? ga * ((v[j].z - mu.z) * rs.z) + be : 0.f;
            o.w = k0 + 3 < K ? ga * ((v[j].w - mu.w) * rs.w) + be : 0.f;
            amax = fmaxf(fmaxf(amax, fmaxf(fabsf(o.x), fabsf(o.y))), fmaxf(fabsf(o.z), fabsf(o.w)));
            *reinterpret_cast<float4*>(Out + off + (size_t)c * Kp) = o;
        }
    }
    if (amax_out != nullptr)        // h3 arithmetic of the GEMM that reads Out: its maximum per utterance
        block_amax_atomic<NTB>(amax, reinterpret_cast<double*>(&sh[0][0]), amax_out + (size_t)m * CTN_AMAX_SLOTS, bx % kb);
}

// NTB threads = NTB/8 channel groups.  CPT = 8 at 512 threads needs 161 VGPRs (one workgroup = 2 waves per SIMD) and is
// still the fastest form for 512 channels: 1024 threads x CPT 4 (4 waves per SIMD) measured 84 us against 55 us, capping
// the registers at 128 (re-reading dOut in the second phase) 59 us.
// FR = frames per workgroup.  (512 threads, 32 frames) holds ONE workgroup per CU (161 VGPRs x 8 waves): it loads 128 KiB, reduces,
// then stores 64 KiB, and nothing on the CU overlaps those phases.  (256 threads, 16 frames) has the same channel groups, registers
// and instruction stream per thread, but three independent workgroups fit a CU; its 64-byte row pieces pair up into whole
// 128-byte lines with the neighbouring workgroup, which the XCD-contiguous block order keeps on the same L2.
// LEAN: the form the composite stacks launch -- every channel group full (Ch == NG * CPT), PReLU fused, no added gradient, no ReLU
// mask: the per-channel and per-element option tests become compile-time (1481 -> ~1000 VALU instructions per wave; the kernel spends
// about a third of its time issuing them).  Same arithmetic, same order: bitwise the general form.
template <int CPT, int NTB, int FR = C4_FR, bool LEAN = false>
__global__ __launch_bounds__(NTB) void cln_bwd_v4_kernel(const float* __restrict__ dOut, const float* __restrict__ Y,
                                                           float* __restrict__ dY, const float* __restrict__ mean_i,
                                                           const float* __restrict__ rstd_i, int M, int Ch, int K, int Kp,
                                                           const float* __restrict__ gamma, const float* __restrict__ alpha_p,
                                                           const float* __restrict__ add, const float* __restrict__ relu_ref,
                                                           float* __restrict__ dalpha_part, float* __restrict__ pc,
                                                           unsigned* __restrict__ amax_out) {
    constexpr int NW = NTB / 64, NQ = FR / 4, NG = NTB / NQ;
    __shared__ float4 sh[NW][NQ];
    __shared__ float red[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = tid % NQ, g = tid / NQ;
    const int kb = Kp / FR, nblk = M * kb;
    const int bx = FR == C4_FR ? (int)blockIdx.x : xcd_remap((int)blockIdx.x, nblk);        // FR 16: the two halves of a 128-byte line on one XCD
    const int m = bx / kb, k0 = (bx % kb) * FR + 4 * q;
    const bool has_a = LEAN || alpha_p != nullptr;
    const float al = has_a ? alpha_p[0] : 1.f;
    const size_t off = (size_t)m * Ch * Kp + k0;
    const float4 mu = ld4(mean_i + (size_t)m * Kp + k0), rs = ld4(rstd_i + (size_t)m * Kp + k0);
    const float vm[4] = {k0 + 0 < K ? 1.f : 0.f, k0 + 1 < K ? 1.f : 0.f, k0 + 2 < K ? 1.f : 0.f, k0 + 3 < K ? 1.f : 0.f};
    float4 t[CPT], yv[CPT];           // gamma * dOut (0 for frames >= K) and the raw input of this thread's channels
    float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int c = g + NG * j;
        float4 y = make_float4(0.f, 0.f, 0.f, 0.f), d = y;
        float ga = 0.f;
        if (LEAN || c < Ch) {
            y = ld4(Y + off + (size_t)c * Kp);
            d = ld4(dOut + off + (size_t)c * Kp);
            ga = gamma[c];
        }
        d.x *= vm[0]; d.y *= vm[1]; d.z *= vm[2]; d.w *= vm[3];
        const float4 v = has_a ? make_float4(prelu_f(y.x, al), prelu_f(y.y, al), prelu_f(y.z, al), prelu_f(y.w, al)) : y;
        const float4 xh = make_float4((v.x - mu.x) * rs.x, (v.y - mu.y) * rs.y, (v.z - mu.z) * rs.z, (v.w - mu.w) * rs.w);
        // parameter-gradient partials of channel c over this workgroup's frames: its 4 frames here, the 8 quads by shuffles
        float pg = (d.x * xh.x + d.y * xh.y) + (d.z * xh.z + d.w * xh.w), pb = (d.x + d.y) + (d.z + d.w);
#pragma unroll
        for (int o = 1; o < NQ; o <<= 1) { pg += __shfl_xor(pg, o, 64); pb += __shfl_xor(pb, o, 64); }
        if (q == 0 && (LEAN || c < Ch)) {
            pc[(size_t)bx * Ch + c] = pg;
            pc[((size_t)nblk + bx) * Ch + c] = pb;
        }
        yv[j] = y;
        t[j] = make_float4(ga * d.x, ga * d.y, ga * d.z, ga * d.w);
        s1.x += t[j].x; s1.y += t[j].y; s1.z += t[j].z; s1.w += t[j].w;
        s2.x += t[j].x * xh.x; s2.y += t[j].y * xh.y; s2.z += t[j].z * xh.z; s2.w += t[j].w * xh.w;
    }
    float4 m1 = block_group_sum<NW, FR>(s1, sh, wave, q, lane), m2 = block_group_sum<NW, FR>(s2, sh, wave, q, lane);
    const float inv = 1.f / (float)Ch;
    m1.x *= inv; m1.y *= inv; m1.z *= inv; m1.w *= inv;
    m2.x *= inv; m2.y *= inv; m2.z *= inv; m2.w *= inv;
    float dal = 0.f, amax = 0.f;
    const float mm[4] = {mu.x, mu.y, mu.z, mu.w}, rr[4] = {rs.x, rs.y, rs.z, rs.w};
    const float a1[4] = {m1.x, m1.y, m1.z, m1.w}, a2[4] = {m2.x, m2.y, m2.z, m2.w};
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int c = g + NG * j;
        if (LEAN || c < Ch) {
            const size_t o = off + (size_t)c * Kp;
            const float yy[4] = {yv[j].x, yv[j].y, yv[j].z, yv[j].w}, tt[4] = {t[j].x, t[j].y, t[j].z, t[j].w};
            float4 ad = make_float4(0.f, 0.f, 0.f, 0.f), rf = make_float4(1.f, 1.f, 1.f, 1.f);
            if constexpr (!LEAN) {
                if (add != nullptr) ad = ld4(add + o);
                if (relu_ref != nullptr) rf = ld4(relu_ref + o);
            }
            const float av[4] = {ad.x, ad.y, ad.z, ad.w}, rv[4] = {rf.x, rf.y, rf.z, rf.w};
            float r[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = has_a ? prelu_f(yy[e], al) : yy[e];
                const float xh = (v - mm[e]) * rr[e];
                const float da = rr[e] * (tt[e] - a1[e] - xh * a2[e]);
                float x = 0.f;
                if (vm[e] != 0.f) {
                    if (has_a && yy[e] < 0.f) dal += da * yy[e];
                    x = (has_a && yy[e] < 0.f) ? al * da : da;
                    if constexpr (!LEAN) {
                        x += av[e];
                        if (!(rv[e] > 0.f)) x = 0.f;
                    }
                }
                r[e] = x;
            }
            amax = fmaxf(fmaxf(amax, fmaxf(fabsf(r[0]), fabsf(r[1]))), fmaxf(fabsf(r[2]), fabsf(r[3])));
            *reinterpret_cast<float4*>(dY + o) = make_float4(r[0], r[1], r[2], r[3]);
        }
    }
    if (dalpha_part != nullptr) {
        dal = block_sum<float, NTB>(dal, red);
        if (tid == 0) dalpha_part[bx] = dal;
    }
    if (amax_out != nullptr)
        block_amax_atomic<NTB>(amax, reinterpret_cast<double*>(&sh[0][0]), amax_out + (size_t)m * CTN_AMAX_SLOTS, bx % kb);
}

// per-(m,c) partial of dgamma = sum_k dOut*xh and dbeta = sum_k dOut ; pc[2][rows][Ch], rows >= M (fallback of the v4 kernel)
__global__ __launch_bounds__(NT) void cln_bwd_params_kernel(const float* __restrict__ dOut, const float* __restrict__ Y,
                                                            const float* __restrict__ mean_i, const float* __restrict__ rstd_i,
                                                            int M, int Ch, int K, int Kp, const float* __restrict__ alpha_p,
                                                            float* __restrict__ pc, int rows) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hb = (Ch + ROWS - 1) / ROWS;
    const int m = blockIdx.x / hb;
    const int c = (blockIdx.x % hb) * ROWS + wave;
    if (c >= Ch) return;
    const bool has_a = alpha_p != nullptr;
    const float al = has_a ? alpha_p[0] : 1.f;
    const size_t row = ((size_t)m * Ch + c) * Kp;
    float dg = 0.f, db = 0.f;
    for (int k = lane * 4; k < Kp; k += 256) {
        const float4 d = ld4(dOut + row + k), y = ld4(Y + row + k);
        const float4 mu = ld4(mean_i + (size_t)m * Kp + k), rs = ld4(rstd_i + (size_t)m * Kp + k);
        const float dv[4] = {d.x, d.y, d.z, d.w}, yv[4] = {y.x, y.y, y.z, y.w};
        const float mv[4] = {mu.x, mu.y, mu.z, mu.w}, rv[4] = {rs.x, rs.y, rs.z, rs.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < K) {
                const float v = has_a ? prelu_f(yv[e], al) : yv[e];
                dg += dv[e] * ((v - mv[e]) * rv[e]);
                db += dv[e];
            }
    }
    dg = wave_sum(dg);
    db = wave_sum(db);
    if (lane == 0) {
        pc[(size_t)m * Ch + c] = dg;
        pc[(size_t)rows * Ch + (size_t)m * Ch + c] = db;
    }
}

// Finish ctn_cln_bwd's partials in one launch: pc [2][rows][Ch] -> dgamma[Ch], dbeta[Ch].  A workgroup owns 64 channels of one
// of the two outputs: lanes along channels (256-byte coalesced rows), the four waves take rows w, w+4, ... and their sums are
// added in wave order (fixed order: bitwise reproducible).  rows = workgroups of the backward kernel (800 at the paper shape).
// The last workgroup sums the nblk per-workgroup dalpha partials.
__global__ __launch_bounds__(NT) void cln_bwd_finalize_kernel(const float* __restrict__ pc, const float* __restrict__ dap,
                                                              int rows, int Ch, int nblk, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta, float* __restrict__ dalpha) {
    __shared__ float red[NT / 64];
    __shared__ float part[NT / 64][64];
    if (blockIdx.x == gridDim.x - 1) {
        if (dap == nullptr) return;
        float s = 0.f;
        for (int i = threadIdx.x; i < nblk; i += NT) s += dap[i];
        s = block_sum<float, NT>(s, red);
        if (threadIdx.x == 0) dalpha[0] = s;
        return;
    }
    const int cb = (Ch + 63) / 64;
    const int f = blockIdx.x / cb, c = (blockIdx.x % cb) * 64 + (threadIdx.x & 63), wave = threadIdx.x >> 6;
    float s = 0.f;
    if (c < Ch) {
        const float* __restrict__ p = pc + (size_t)f * rows * Ch + c;
        int r = wave;
        for (; r + 252 < rows; r += 256) {               // 64 independent loads in flight per lane: the kernel is load latency, a
            float v[64];                                 // few MB over nine workgroups; the adds keep their row order
#pragma unroll
            for (int j = 0; j < 64; ++j) v[j] = p[(size_t)(r + 4 * j) * Ch];
#pragma unroll
            for (int j = 0; j < 64; ++j) s += v[j];
        }
        for (; r + 28 < rows; r += 32) {                 // eight
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = p[(size_t)(r + 4 * j) * Ch];
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[j];
        }
        for (; r < rows; r += 4) s += p[(size_t)r * Ch];
    }
    part[wave][threadIdx.x & 63] = s;
    __syncthreads();
    if (wave == 0 && c < Ch)
        (f == 0 ? dgamma : dbeta)[c] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
}

// Per-frame statistics of a channel-wise LayerNorm from the column partials of ctn_pw_gemm_cln: (sum p, sum p^2) over the row tiles
// in fixed order (fp64) -> mean, rstd = 1 / sqrt(E[p^2] - mean^2 + eps) (fp64 until the last step; biased variance).
__global__ __launch_bounds__(NT) void cln_stats_frame_kernel(const double* __restrict__ part, int nparts, float* __restrict__ mean,
                                                             float* __restrict__ rstd, int M, int Ch, int Kp) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= (long long)M * Kp) return;
    const int m = (int)(i / Kp), k = (int)(i % Kp);
    double s1 = 0.0, s2 = 0.0;
    for (int t = 0; t < nparts; ++t) {
        const double2 q = *reinterpret_cast<const double2*>(part + (((size_t)m * nparts + t) * Kp + k) * 2);
        s1 += q.x;
        s2 += q.y;
    }
    const double mu = s1 / (double)Ch;
    double var = s2 / (double)Ch - mu * mu;
    if (var < 0.0) var = 0.0;
    mean[i] = (float)mu;
    rstd[i] = (float)(1.0 / sqrt(var + (double)CTN_EPS));
}

// Per-frame constants of a channel-wise LayerNorm's backward from the column partials of ctn_pw_dgrad_cln:
//   S1[k] = sum_t part[m][t][k][0], S2[k] = sum_t part[m][t][k][1]  (t = row tiles, fixed order, fp64)
//   fc[m][0..3][k] = (rstd, mean rstd, rstd S1 / Ch, rstd S2 / Ch)
__global__ __launch_bounds__(NT) void cln_bwd_frame_kernel(const double* __restrict__ part, int nparts, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, float* __restrict__ fc, int M, int Ch, int Kp) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= (long long)M * Kp) return;
    const int m = (int)(i / Kp), k = (int)(i % Kp);
    double s1 = 0.0, s2 = 0.0;
    for (int t = 0; t < nparts; ++t) {
        const double2 q = *reinterpret_cast<const double2*>(part + (((size_t)m * nparts + t) * Kp + k) * 2);
        s1 += q.x;
        s2 += q.y;
    }
    const float rs = rstd[i], mu = mean[i];
    float* const o = fc + (size_t)m * 4 * Kp + k;
    o[0] = rs;
    o[(size_t)Kp] = mu * rs;
    o[(size_t)2 * Kp] = rs * (float)(s1 / (double)Ch);
    o[(size_t)3 * Kp] = rs * (float)(s2 / (double)Ch);
}

}  // namespace

extern "C" {

int ctn_cln_bwd_frame(const double* col_part, int nparts, const float* mean, const float* rstd, float* fc, int M, int Ch, int Kp,
                      void* stream) {
    CTN_REQUIRE(col_part && mean && rstd && fc && nparts > 0 && M > 0 && Ch > 0 && Kp > 0, "ctn_cln_bwd_frame: bad arguments");
    CTN_REQUIRE(ctn_aligned16(col_part), "ctn_cln_bwd_frame: col_part must be 16-byte aligned");
    hipLaunchKernelGGL(cln_bwd_frame_kernel, dim3((unsigned)ctn_cdivll((long long)M * Kp, NT)), dim3(NT), 0, (hipStream_t)stream,
                       col_part, nparts, mean, rstd, fc, M, Ch, Kp);
    CTN_CHECK_LAUNCH("ctn_cln_bwd_frame");
    return CTN_OK;
}

int ctn_cln_stats_frame(const double* col_part, int nparts, float* mean, float* rstd, int M, int Ch, int Kp, void* stream) {
    CTN_REQUIRE(col_part && mean && rstd && nparts > 0 && M > 0 && Ch > 0 && Kp > 0, "ctn_cln_stats_frame: bad arguments");
    CTN_REQUIRE(ctn_aligned16(col_part), "ctn_cln_stats_frame: col_part must be 16-byte aligned");
    hipLaunchKernelGGL(cln_stats_frame_kernel, dim3((unsigned)ctn_cdivll((long long)M * Kp, NT)), dim3(NT), 0, (hipStream_t)stream,
                       col_part, nparts, mean, rstd, M, Ch, Kp);
    CTN_CHECK_LAUNCH("ctn_cln_stats_frame");
    return CTN_OK;
}

// frames per workgroup of the cln_*_v4 kernels: 16 (256 threads, three and more workgroups per CU; default since round 4) or 32
// (512 threads); ctn_tune("cln_fr", 16 | 32).  The backward partial buffers are sized and summed by this count for every kernel
// of the family.
int g_ctn_cln_fr = 16;
int g_ctn_cln_fuse = -1;         // ctn_tune("cln_fuse", 0 | 1 | 2): 1 = composite cLN stacks run the second norm's backward inside the input-gradient
                                 // GEMM's epilogue (per-frame sums) and the depthwise backward's dd image instead of as a pass of its own
int ctn_cln_fuse(void) {         // (-1: not read yet; CTN_CLN_FUSE=0|1|2 at first use, for fresh-process A/B runs; default 2)
    if (g_ctn_cln_fuse < 0) {
        const char* e = getenv("CTN_CLN_FUSE");
        g_ctn_cln_fuse = (e && *e >= '0' && *e <= '2' && !e[1]) ? *e - '0' : 2;
    }
    return g_ctn_cln_fuse;
}
int g_ctn_cln_lean = 1;          // ctn_tune("cln_lean", 0 | 1): the specialised backward kernel for the stacks' form

static bool cln_v4_ok(int Ch, int Kp, const void* a, const void* b, const void* c) {
    return Ch <= 8 * C4_NG && Kp % C4_FR == 0 && ctn_aligned16(a) && ctn_aligned16(b) && ctn_aligned16(c);
}

int ctn_cln_fwd(const float* Y, float* Out, float* mean, float* rstd, int M, int Ch, int K, int Kp,
                const float* gamma, const float* beta, const float* alpha, unsigned* amax_out, void* stream) {
    CTN_REQUIRE(Y && Out && mean && rstd && gamma && beta, "ctn_cln_fwd: null pointer");
    CTN_REQUIRE(M > 0 && Ch > 0 && K > 0 && Kp >= K, "ctn_cln_fwd: bad sizes");
    hipStream_t st = (hipStream_t)stream;
    if (cln_v4_ok(Ch, Kp, Y, Out, mean) && ctn_aligned16(rstd)) {     // 16-byte accesses along frames (round 2)
        const bool small = g_ctn_cln_fr == 16;                     // (Kp % 32 == 0 was checked: 16 divides it)
        const dim3 grid((unsigned)(M * (Kp / (small ? 16 : C4_FR))));
#define CTN_CLN_FWD4(CPT_) do { if (small) hipLaunchKernelGGL((cln_fwd_v4_kernel<CPT_, 256, 16>), grid, dim3(256), 0, st, Y, Out, mean, rstd, M, Ch, K, Kp, gamma, beta, alpha, amax_out); \
                                else hipLaunchKernelGGL((cln_fwd_v4_kernel<CPT_>), grid, dim3(C4_NT), 0, st, Y, Out, mean, rstd, M, Ch, K, Kp, gamma, beta, alpha, amax_out); } while (0)
        const int cpt = ctn_cdiv(Ch, C4_NG);
        if (cpt <= 1) CTN_CLN_FWD4(1);
        else if (cpt <= 2) CTN_CLN_FWD4(2);
        else if (cpt <= 4) CTN_CLN_FWD4(4);
        else CTN_CLN_FWD4(8);
#undef CTN_CLN_FWD4
        CTN_CHECK_LAUNCH("ctn_cln_fwd");
        return CTN_OK;
    }
    const dim3 grid_r((unsigned)(M * ctn_cdiv(Kp, CLN_FR)));
#define CTN_CLN_FWD(CPT_) hipLaunchKernelGGL((cln_fwd_reg_kernel<CLN_FR, CPT_>), grid_r, dim3(CLN_NT), 0, st, Y, Out, mean, rstd, M, Ch, K, Kp, gamma, beta, alpha)
    const int cpt = ctn_cdiv(Ch, CLN_NT / CLN_FR);
    if (cpt <= 2) CTN_CLN_FWD(2);
    else if (cpt <= 4) CTN_CLN_FWD(4);
    else if (cpt <= 8) CTN_CLN_FWD(8);
    else if (cpt <= 16) CTN_CLN_FWD(16);
    else if (cpt <= 32) CTN_CLN_FWD(32);
    else hipLaunchKernelGGL(cln_fwd_kernel, dim3((unsigned)(M * ctn_cdiv(Kp, 64))), dim3(NT), 0, st, Y, Out, mean, rstd, M, Ch, K, Kp,
                            gamma, beta, alpha);
#undef CTN_CLN_FWD
    CTN_CHECK_LAUNCH("ctn_cln_fwd");
    if (amax_out != nullptr) return ctn_absmax_rows(Out, M, (long long)Ch * Kp, amax_out, stream);     // fallback kernels: a pass of its own
    return CTN_OK;
}

int ctn_cln_bwd_blocks(int M, int Kp) { return M * ctn_cdiv(Kp, g_ctn_cln_fr); }   // rows of the parameter-gradient partials
size_t ctn_cln_bwd_pc_floats(int M, int Ch, int Kp) { return (size_t)2 * ctn_cln_bwd_blocks(M, Kp) * Ch; }

// see include/ctn_hip.h.  pc is [2][ctn_cln_bwd_blocks(M, Kp)][Ch]
int ctn_cln_bwd(const float* dOut, const float* Y, float* dY, const float* mean, const float* rstd,
                int M, int Ch, int K, int Kp, const float* gamma, const float* alpha,
                const float* add, const float* relu_ref, float* dalpha_part, float* pc, unsigned* amax_out, void* stream) {
    CTN_REQUIRE(dOut && Y && dY && mean && rstd && gamma && pc, "ctn_cln_bwd: null pointer");
    CTN_REQUIRE(M > 0 && Ch > 0 && K > 0 && Kp >= K && Kp % 4 == 0, "ctn_cln_bwd: bad sizes");
    CTN_REQUIRE(!alpha || dalpha_part, "ctn_cln_bwd: dalpha_part required with alpha");
    CTN_REQUIRE(ctn_aligned16(dOut) && ctn_aligned16(Y) && ctn_aligned16(mean) && ctn_aligned16(rstd), "ctn_cln_bwd: alignment");
    hipStream_t st = (hipStream_t)stream;
    float* const dap = alpha ? dalpha_part : nullptr;
    const int rows = ctn_cln_bwd_blocks(M, Kp);
    if (cln_v4_ok(Ch, Kp, dOut, Y, dY) && Kp % g_ctn_cln_fr == 0 && (!add || ctn_aligned16(add)) && (!relu_ref || ctn_aligned16(relu_ref))) {
        // one pass: input gradient AND the parameter-gradient partials (dY may alias dOut: each thread reads its elements
        // of dOut before it writes them)
        const dim3 grid((unsigned)rows);
#define CTN_CLN_BWD4(CPT_) do { if (g_ctn_cln_fr == 16) hipLaunchKernelGGL((cln_bwd_v4_kernel<CPT_, 256, 16>), grid, dim3(256), 0, st, dOut, Y, dY, mean, rstd, M, Ch, K, Kp, gamma, alpha, add, relu_ref, dap, pc, amax_out); \
                                else hipLaunchKernelGGL((cln_bwd_v4_kernel<CPT_, C4_NT, C4_FR>), grid, dim3(C4_NT), 0, st, dOut, Y, dY, mean, rstd, M, Ch, K, Kp, gamma, alpha, add, relu_ref, dap, pc, amax_out); } while (0)
        // the stacks' form (every channel group full, PReLU fused, no added gradient, no ReLU mask) has a kernel of its own
        const bool lean = g_ctn_cln_lean && Ch == 8 * C4_NG && g_ctn_cln_fr == 16 && alpha && !add && !relu_ref;
        if (lean) hipLaunchKernelGGL((cln_bwd_v4_kernel<8, 256, 16, true>), grid, dim3(256), 0, st, dOut, Y, dY, mean, rstd, M, Ch, K, Kp, gamma, alpha, add, relu_ref, dap, pc, amax_out);
        else if (Ch <= C4_NG) CTN_CLN_BWD4(1);
        else if (Ch <= 2 * C4_NG) CTN_CLN_BWD4(2);
        else if (Ch <= 4 * C4_NG) CTN_CLN_BWD4(4);
        else CTN_CLN_BWD4(8);
#undef CTN_CLN_BWD4
        CTN_CHECK_LAUNCH("ctn_cln_bwd");
        return CTN_OK;
    }
    // fallback (very wide layers / unaligned frames): parameter partials first (dY may alias dOut), into the first M rows of pc;
    // these kernels work in 32-frame blocks whatever g_ctn_cln_fr is: the partial rows they do not write stay zero
    hipMemsetAsync(pc, 0, sizeof(float) * ctn_cln_bwd_pc_floats(M, Ch, Kp), st);
    if (dap) hipMemsetAsync(dap, 0, sizeof(float) * (size_t)rows, st);
    hipLaunchKernelGGL(cln_bwd_params_kernel, dim3((unsigned)(M * ctn_cdiv(Ch, ROWS))), dim3(NT), 0, st,
                       dOut, Y, mean, rstd, M, Ch, K, Kp, alpha, pc, rows);
    CTN_CHECK_LAUNCH("ctn_cln_bwd/params");
    const dim3 grid_r((unsigned)(M * ctn_cdiv(Kp, CLN_FR)));
#define CTN_CLN_BWD(CPT_, NTB_) hipLaunchKernelGGL((cln_bwd_dx_reg_kernel<CLN_FR, CPT_, NTB_>), grid_r, dim3(NTB_), 0, st, dOut, Y, dY, mean, rstd, M, Ch, K, Kp, gamma, alpha, add, relu_ref, dap)
    if (Ch <= 32) CTN_CLN_BWD(2, 512);
    else if (Ch <= 64) CTN_CLN_BWD(4, 512);
    else if (Ch <= 128) CTN_CLN_BWD(8, 512);
    else if (Ch <= 256) CTN_CLN_BWD(16, 512);
    else if (Ch <= 512) CTN_CLN_BWD(16, 1024);
    else {      // generic kernel; it fills only the first M*ceil(Kp/64) partials of the buffer
        hipLaunchKernelGGL(cln_bwd_dx_kernel, dim3((unsigned)(M * ctn_cdiv(Kp, 64))), dim3(NT), 0, st, dOut, Y, dY, mean, rstd, M,
                           Ch, K, Kp, gamma, alpha, add, relu_ref, dap);
    }
#undef CTN_CLN_BWD
    CTN_CHECK_LAUNCH("ctn_cln_bwd/dx");
    if (amax_out != nullptr) return ctn_absmax_rows(dY, M, (long long)Ch * Kp, amax_out, stream);      // fallback kernels: a pass of its own
    return CTN_OK;
}

int ctn_cln_bwd_finalize(const float* pc, const float* dalpha_part, int M, int Ch, int Kp, float* dgamma, float* dbeta,
                         float* dalpha, void* stream) {
    CTN_REQUIRE(pc && dgamma && dbeta && M > 0 && Ch > 0 && Kp > 0, "ctn_cln_bwd_finalize: bad arguments");
    CTN_REQUIRE(!dalpha_part || dalpha, "ctn_cln_bwd_finalize: dalpha required with dalpha_part");
    const int rows = ctn_cln_bwd_blocks(M, Kp);
    const unsigned nb = (unsigned)(2 * ctn_cdiv(Ch, 64)) + 1;
    hipLaunchKernelGGL(cln_bwd_finalize_kernel, dim3(nb), dim3(NT), 0, (hipStream_t)stream, pc, dalpha_part, rows, Ch, rows,
                       dgamma, dbeta, dalpha);
    CTN_CHECK_LAUNCH("ctn_cln_bwd_finalize");
    return CTN_OK;
}

}  // extern "C"
