// Fused low-latency streaming inference for the causal cLN and cumLN models (include/ctn_hip.h, "streaming" section).
//
// Everything of the causal stack except the depthwise taps is frame-local, so one workgroup carries a tile of ST_TC frame columns of
// ONE stream through   depthwise -> PReLU -> cLN -> 1x1 + residual -> next block's 1x1 -> PReLU -> cLN   in LDS (a "stage").  The only
// data that crosses workgroups is the depthwise history; it lives in one ring buffer per block, written by stage j and read by
// stage j+1 (the next launch).  nblocks + 1 stage launches per chunk instead of 9 per block, no cat / pad copies, no 64-frame padding.
// Chunks of at most one tile per stream (the low-latency case) run the same block boundary as two launches whose workgroups split
// the GEMMs' output rows, so that one stream's weights are streamed by up to 16 CUs instead of one (stream_rows_a / _b below).
//
// Arithmetic is frame-local and fixed-order: every output value of frame k of stream m is a k-ordered fp32 FMA chain
// (v_mfma_f32_16x16x4_f32) or a fixed-order sum over the channels of that frame alone, so it does not depend on the chunk the frame
// arrived in, on its column position in a tile, or on the other streams.
// The cumulative norm (cumLN) adds fp64 running sums per stream, block and norm, continued in the order of the absolute frame index
// from a carried record (tile_cumln): the same independence, at one tile per stream and step.
#include "ctn_common.h"
#include <algorithm>
#include <type_traits>

namespace {

constexpr int ST_NT = 1024;       // threads per workgroup: 4 waves per SIMD hide the weight-load latency of the one resident tile
constexpr int ST_NW = ST_NT / 64; // waves
constexpr int ST_TC = 16;         // frame columns per tile (the N of the 16x16x4 MFMA)
constexpr int ST_GRP = ST_NT / ST_TC;   // channel groups of the cLN partial sums
constexpr int ST_MAXP = 8;        // depthwise taps
constexpr int ST_MAXC = 8;        // speakers (softmax mask)
constexpr int ST_HDR = 64;        // floats in front of the rings: word 0 = frame position
constexpr int ST_TAB = 8;         // ints per slot of a ragged step table (CTN_STREAM_TAB): nf, nh, src, dst, out hop offsets, 3 spare
constexpr int ST_RST_SLOTS = 32;  // slots / rings per launch of the per-slot reset
constexpr int ST_RST_RINGS = 64;
constexpr size_t ST_MAX_LDS = 64 * 1024;

typedef float f32x4 __attribute__((ext_vector_type(4)));

inline int c16(int n) { return (n + 15) / 16; }
inline long long pow2ceil(long long n) { long long r = 1; while (r < n) r <<= 1; return r; }
inline long long ring_len(int P, int d, int max_frames) { return pow2ceil((long long)(P - 1) * d + max_frames); }
// one block of the packed stack: W1 fragments [H,B], W2 fragments [B,H], (alpha1, alpha2, 0, 0), gamma1, beta1, gamma2, beta2 [H], D [H,P]
inline size_t block_floats(int B, int H, int P) { return (size_t)2 * H * B + 4 + (size_t)4 * H + (size_t)H * P; }

enum { EPI_STORE = 0, EPI_ADD = 1, EPI_RELU = 2 };

// Frames slot m computes in this step: the call's `frames` (F), or with RAGGED its own count from the step table, clamped to 0 .. F
// (F is the leading dimension of every activation of the step: a bad table cannot index past a row).
template <bool RAGGED>
__device__ __forceinline__ int slot_frames(const int* __restrict__ tab, int m, int F) {
    return RAGGED ? min(max(tab[m * ST_TAB], 0), F) : F;
}

// ---- weights -> MFMA fragment order --------------------------------------------------------------------------------
// W [R, Cn] row-major -> float4 [ceil(R/16)][ceil(Cn/16)][64 lanes]: element i of lane l in (row tile rt, k group g) is
// W[rt*16 + (l & 15)][g*16 + i*4 + (l >> 4)] = the A operand of k-step g*4+i; rows / columns past R / Cn are exact zeros.
__global__ __launch_bounds__(256) void stream_pack_kernel(const float* __restrict__ W, float* __restrict__ out, int R, int Cn) {
    const int Rt = (R + 15) / 16, G = (Cn + 15) / 16;
    const long long n = (long long)Rt * G * 256;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int i = (int)(e & 3), l = (int)((e >> 2) & 63);
        const long long t = e >> 8;
        const int g = (int)(t % G), rt = (int)(t / G);
        const int row = rt * 16 + (l & 15), k = g * 16 + i * 4 + (l >> 4);
        out[e] = (row < R && k < Cn) ? W[(size_t)row * Cn + k] : 0.f;
    }
}

__global__ __launch_bounds__(256) void stream_pack_vec_kernel(const float* __restrict__ a1, const float* __restrict__ g1,
                                                             const float* __restrict__ b1, const float* __restrict__ D,
                                                             const float* __restrict__ a2, const float* __restrict__ g2,
                                                             const float* __restrict__ b2, float* __restrict__ out, int H, int P) {
    const int n = 4 + 4 * H + H * P;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        float v;
        if (e < 4) v = e == 0 ? a1[0] : e == 1 ? a2[0] : 0.f;
        else if (e < 4 + H) v = g1[e - 4];
        else if (e < 4 + 2 * H) v = b1[e - 4 - H];
        else if (e < 4 + 3 * H) v = g2[e - 4 - 2 * H];
        else if (e < 4 + 4 * H) v = b2[e - 4 - 3 * H];
        else v = D[e - 4 - 4 * H];
        out[e] = v;
    }
}

// ---- tile primitives (all operands in LDS as [channels][ST_TC]) -----------------------------------------------------
// NB k groups (16 k values each) of NTILE row tiles: every weight fragment of the batch is requested before the first MFMA, so a
// wave has NB * NTILE KB in flight and pays one memory latency per batch, not per k group (the loads return in order, the MFMAs wait
// with counted vmcnt).  No conditional around a load.  The B operand of k-step s is act[4s + (l>>4)][l&15] = 64 consecutive floats.
template <int NTILE, int NB>
__device__ __forceinline__ void gemm_batch(const float4* __restrict__ ap, int G, const float* b, f32x4 (&c)[NTILE]) {
    float4 a[NTILE][NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int t = 0; t < NTILE; ++t) a[t][i] = ap[((size_t)t * G + i) * 64];
    __builtin_amdgcn_sched_barrier(0);      // the scheduler otherwise sinks every load to just in front of its MFMAs
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const float b0 = b[i * 256], b1 = b[i * 256 + 64], b2 = b[i * 256 + 128], b3 = b[i * 256 + 192];
#pragma unroll
        for (int t = 0; t < NTILE; ++t) c[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][i].x, b0, c[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NTILE; ++t) c[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][i].y, b1, c[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NTILE; ++t) c[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][i].z, b2, c[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NTILE; ++t) c[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][i].w, b3, c[t], 0, 0, 0);
    }
}

// NTILE consecutive row tiles from rt on: one k-ordered FMA chain per output element, whatever NTILE and the batch sizes are.
template <int EPI, int NTILE>
__device__ __forceinline__ void gemm_rows(const float4* __restrict__ Wp, int rt, int G, const float* act, float* out) {
    const int lane = threadIdx.x & 63;
    const float4* __restrict__ ap = Wp + (size_t)rt * G * 64 + lane;
    const float* b = act + lane;
    f32x4 c[NTILE];
#pragma unroll
    for (int t = 0; t < NTILE; ++t) c[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    int g = 0;
    if (NTILE == 1)
        for (; g + 16 <= G; g += 16) gemm_batch<NTILE, 16>(ap + (size_t)g * 64, G, b + g * 256, c);
    for (; g + 8 <= G; g += 8) gemm_batch<NTILE, 8>(ap + (size_t)g * 64, G, b + g * 256, c);
    if (g + 4 <= G) { gemm_batch<NTILE, 4>(ap + (size_t)g * 64, G, b + g * 256, c); g += 4; }
    if (g + 2 <= G) { gemm_batch<NTILE, 2>(ap + (size_t)g * 64, G, b + g * 256, c); g += 2; }
    if (g < G) gemm_batch<NTILE, 1>(ap + (size_t)g * 64, G, b + g * 256, c);
    // C/D map: column = lane & 15, row = (lane >> 4) * 4 + register
#pragma unroll
    for (int t = 0; t < NTILE; ++t) {
        float* o = out + ((size_t)(rt + t) * 16 + (lane >> 4) * 4) * ST_TC + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (EPI == EPI_ADD) o[r * ST_TC] += c[t][r];
            else o[r * ST_TC] = EPI == EPI_RELU ? fmaxf(c[t][r], 0.f) : c[t][r];
        }
    }
}

// out[Rt tiles of 16 rows][ST_TC] (op)= Wp . act[G*16][ST_TC].  A wave owns two row tiles at a time when there are enough of them (two
// independent accumulators cover the 40-cycle dependent latency of the 32-cycle MFMA), else one, so that no wave idles.
template <int EPI>
__device__ __forceinline__ void tile_gemm(const float* __restrict__ Wp_, int Rt, int G, const float* act, float* out) {
    const float4* __restrict__ Wp = reinterpret_cast<const float4*>(Wp_);
    const int wave = threadIdx.x >> 6;
    if (Rt >= 2 * ST_NW) {
        int rt = wave * 2;
        for (; rt + 1 < Rt; rt += ST_NW * 2) gemm_rows<EPI, 2>(Wp, rt, G, act, out);
        if (rt < Rt) gemm_rows<EPI, 1>(Wp, rt, G, act, out);
    } else {
        for (int rt = wave; rt < Rt; rt += ST_NW) gemm_rows<EPI, 1>(Wp, rt, G, act, out);
    }
}

// In place: t = gamma * ((prelu(t) - mean) * rstd) + beta per column over the Ch rows (src/conv_tasnet.py:313-335: biased variance,
// eps 1e-8), two passes over the values held in LDS.  Thread (group g, column c) sums rows g, g+ST_GRP, ...; the ST_GRP partials of a
// column are then added in ascending group order by every thread: one fixed order for every column.  part: ST_GRP*ST_TC floats.
// Starts and ends with a workgroup barrier.
__device__ __forceinline__ void tile_cln(float* t, int Ch, const float* __restrict__ alpha_p, const float* __restrict__ gamma,
                                         const float* __restrict__ beta, float* part) {
    const int col = threadIdx.x & (ST_TC - 1), grp = threadIdx.x / ST_TC;
    const bool has_a = alpha_p != nullptr;
    const float al = has_a ? alpha_p[0] : 1.f;
    __syncthreads();
    float s = 0.f;
    for (int r = grp; r < Ch; r += ST_GRP) {
        float v = t[r * ST_TC + col];
        if (has_a) { v = prelu_f(v, al); t[r * ST_TC + col] = v; }
        s += v;
    }
    part[grp * ST_TC + col] = s;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < ST_GRP; ++i) tot += part[i * ST_TC + col];
    const float mu = tot / (float)Ch;
    __syncthreads();
    float q = 0.f;
    for (int r = grp; r < Ch; r += ST_GRP) {
        const float v = t[r * ST_TC + col] - mu;
        q += v * v;
    }
    part[grp * ST_TC + col] = q;
    __syncthreads();
    tot = 0.f;
#pragma unroll
    for (int i = 0; i < ST_GRP; ++i) tot += part[i * ST_TC + col];
    const float rs = 1.0f / sqrtf(tot / (float)Ch + CTN_EPS);
    for (int r = grp; r < Ch; r += ST_GRP) t[r * ST_TC + col] = gamma[r] * ((t[r * ST_TC + col] - mu) * rs) + beta[r];
    __syncthreads();
}

// ---- cumulative layer norm (norm_type 'cumLN'; the contract of ctn_cumln_fwd) -----------------------------------------------------------
// One carry record per slot, block and norm: the sums of a and a^2 over all channels of all frames so far, and the number of frames.
// `cum` holds two banks of [M][nblocks][2] records: the current one, which the kernels of a step only read, and the pending one, which
// one workgroup per slot writes and the step's last launch copies over the current one (stream_advance_cum_kernel).
struct CumRec {
    double c1, c2;
    unsigned long long count, spare;
};
static_assert(sizeof(CumRec) == 32, "CumRec is 32 bytes in the C ABI (ctn_stream_cum_bytes)");

// LDS behind the [B + H][ST_TC] tiles of a cumulative kernel: the (sum, sum of squares) partials of every wave and column, the ST_TC
// column sums, the ST_TC (mean, rstd) pairs.
constexpr size_t ST_CUM_LDS = (size_t)(ST_NW + 1) * ST_TC * sizeof(double2) + ST_TC * sizeof(float2);

// In place: t = gamma * ((prelu(t) - mu_c) * r_c) + beta with the statistics of column c taken over all channels of the stream's frames
// up to and including that column: C = rec + the sums of columns 0 .. c, n = Ch * (rec.count + c + 1), mu = C1 / n,
// r = 1 / sqrt(max(C2 / n - mu^2, 0) + eps).  fp64 from the first addition to mu and r, which are rounded to fp32 once; the last line is
// tile_cln's.  Thread (group g, column c) sums rows g, g+ST_GRP, ...; the four groups of a wave are added by two exchanges across the
// lanes of a column, (g0 + g1) + (g2 + g3), which leaves the same bits in all four (the partials stay in registers: 4 KB of LDS
// instead of 16); lane c of the first 16 adds the ST_NW wave partials of its column in ascending order, then runs the chain
// C_i = C_{i-1} + s_i from the record to its own column: the same additions in the same order whatever the column, the call and the
// workgroup.  Columns >= nvalid add nothing and are left without statistics (mu = r = 0).
// pend != null: this workgroup stores the advanced record.  part: ST_CUM_LDS bytes, 16-byte aligned.  Starts and ends with a barrier.
__device__ __forceinline__ void tile_cumln(float* t, int Ch, const float* __restrict__ alpha_p, const float* __restrict__ gamma,
                                           const float* __restrict__ beta, double2* part, const CumRec* __restrict__ rec,
                                           CumRec* __restrict__ pend, int nvalid) {
    const int col = threadIdx.x & (ST_TC - 1), grp = threadIdx.x / ST_TC;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double2* colsum = part + ST_NW * ST_TC;
    float2* stat = reinterpret_cast<float2*>(colsum + ST_TC);
    const bool has_a = alpha_p != nullptr;
    const float al = has_a ? alpha_p[0] : 1.f;
    __syncthreads();
    double s1 = 0.0, s2 = 0.0;
    for (int r = grp; r < Ch; r += ST_GRP) {
        float v = t[r * ST_TC + col];
        if (has_a) { v = prelu_f(v, al); t[r * ST_TC + col] = v; }
        s1 += (double)v;
        s2 = fma((double)v, (double)v, s2);
    }
    s1 += __shfl_xor(s1, ST_TC);
    s2 += __shfl_xor(s2, ST_TC);
    s1 += __shfl_xor(s1, 2 * ST_TC);
    s2 += __shfl_xor(s2, 2 * ST_TC);
    if (lane < ST_TC) part[wave * ST_TC + col] = double2{s1, s2};
    __syncthreads();
    if (threadIdx.x < ST_TC) {
        double a1 = 0.0, a2 = 0.0;
#pragma unroll
        for (int i = 0; i < ST_NW; ++i) {
            const double2 p = part[i * ST_TC + col];
            a1 += p.x;
            a2 += p.y;
        }
        colsum[col] = double2{a1, a2};
    }
    __syncthreads();
    if (threadIdx.x < ST_TC) {
        float2 st = float2{0.f, 0.f};
        if (col < nvalid) {
            double c1 = rec->c1, c2 = rec->c2;
            const unsigned long long cnt = rec->count;
            for (int i = 0; i <= col; ++i) {
                c1 += colsum[i].x;
                c2 += colsum[i].y;
            }
            const double n = (double)Ch * (double)(cnt + (unsigned long long)col + 1ull);
            const double mu = c1 / n;
            double var = c2 / n - mu * mu;
            if (var < 0.0) var = 0.0;
            st = float2{(float)mu, (float)(1.0 / sqrt(var + (double)CTN_EPS))};
            if (pend != nullptr && col == nvalid - 1) {
                pend->c1 = c1;
                pend->c2 = c2;
                pend->count = cnt + (unsigned long long)nvalid;
            }
        }
        stat[col] = st;
    }
    __syncthreads();
    const float mu = stat[col].x, rs = stat[col].y;
    for (int r = grp; r < Ch; r += ST_GRP) t[r * ST_TC + col] = gamma[r] * ((t[r * ST_TC + col] - mu) * rs) + beta[r];
    __syncthreads();
}

// global [rows][ld] columns k0 .. k0+nvalid-1 <-> LDS [rows][ST_TC]; columns past nvalid are zeros in LDS and are never stored
__device__ __forceinline__ void tile_load(float* t, const float* __restrict__ g, int rows, int ld, int k0, int nvalid) {
    for (int e = threadIdx.x; e < rows * ST_TC; e += ST_NT) {
        const int r = e / ST_TC, c = e & (ST_TC - 1);
        const float v = g[(size_t)r * ld + k0 + min(c, nvalid - 1)];      // unconditional (clamped) load, then select: no branch per element
        t[e] = c < nvalid ? v : 0.f;
    }
}
__device__ __forceinline__ void tile_store(const float* t, float* __restrict__ g, int rows, int ld, int k0, int nvalid) {
    for (int e = threadIdx.x; e < rows * ST_TC; e += ST_NT) {
        const int r = e / ST_TC, c = e & (ST_TC - 1);
        if (c < nvalid) g[(size_t)r * ld + k0 + c] = t[e];
    }
}

// Causal depthwise taps of a tile: z[h][c] = sum_t D[h,t] * n1[h][frame(c) - (P-1-t)*d], the current frame (t = P-1) and the past, one
// ascending-t FMA chain per element.  n1 comes from the block's ring; with INTILE the frames of this tile are taken from `cur`
// (LDS [H][ST_TC], column 0 = frame pos) instead, because the ring does not hold them yet (same values either way).  Every ring load
// is unconditional (clamped) and issued before the first FMA: one memory latency for the whole tile.  Thread t owns elements
// t, t + ST_NT, ...: z[i] (NI = ceil(H * ST_TC / ST_NT)); PT = P when specialised, 0 = run-time tap count.
template <int NI, int PT, bool INTILE>
__device__ __forceinline__ void tile_dw(float (&z)[NI], const float* __restrict__ ring, int R, unsigned pos, int d, int H, int P,
                                        const float* __restrict__ D, const float* cur) {
    const unsigned mask = (unsigned)R - 1u;
    const int last = H * ST_TC - 1;
    if (PT > 0) {
        float v[NI][PT > 0 ? PT : 1], w[NI][PT > 0 ? PT : 1];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int e = min((int)threadIdx.x + i * ST_NT, last), h = e / ST_TC, c = e & (ST_TC - 1);
#pragma unroll
            for (int t = 0; t < PT; ++t) {
                v[i][t] = ring[(size_t)h * R + ((pos + (unsigned)c - (unsigned)((PT - 1 - t) * d)) & mask)];
                w[i][t] = D[h * PT + t];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int e = min((int)threadIdx.x + i * ST_NT, last), c = e & (ST_TC - 1);
            float acc = 0.f;
#pragma unroll
            for (int t = 0; t < PT; ++t) {
                const int off = (PT - 1 - t) * d;
                float x = v[i][t];
                if (INTILE && off <= c) x = cur[e - off];
                acc = fmaf(w[i][t], x, acc);
            }
            z[i] = acc;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int e = min((int)threadIdx.x + i * ST_NT, last), h = e / ST_TC, c = e & (ST_TC - 1);
            float acc = 0.f;
            for (int t = 0; t < P; ++t) {
                const int off = (P - 1 - t) * d;
                float x = ring[(size_t)h * R + ((pos + (unsigned)c - (unsigned)off) & mask)];
                if (INTILE && off <= c) x = cur[e - off];
                acc = fmaf(D[h * P + t], x, acc);
            }
            z[i] = acc;
        }
    }
}

// dst (LDS [H][ST_TC]) = taps; dst may be `cur` (the values are held in registers across a barrier).
template <int NI, bool INTILE>
__device__ __forceinline__ void tile_dw_to(float* dst, const float* __restrict__ ring, int R, unsigned pos, int d, int H, int P,
                                           const float* __restrict__ D, const float* cur) {
    float z[NI];
    if (P == 3) tile_dw<NI, 3, INTILE>(z, ring, R, pos, d, H, P, D, cur);
    else tile_dw<NI, 0, INTILE>(z, ring, R, pos, d, H, P, D, cur);
    if (INTILE) __syncthreads();
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int e = (int)threadIdx.x + i * ST_NT;
        if (e < H * ST_TC) dst[e] = z[i];
    }
}
template <bool INTILE>
__device__ __forceinline__ void tile_dw_any(float* dst, const float* __restrict__ ring, int R, unsigned pos, int d, int H, int P,
                                            const float* __restrict__ D, const float* cur) {
    const int ni = (H * ST_TC + ST_NT - 1) / ST_NT;        // H <= 1024: at most 16 elements per thread
    if (ni <= 1) tile_dw_to<1, INTILE>(dst, ring, R, pos, d, H, P, D, cur);
    else if (ni <= 4) tile_dw_to<4, INTILE>(dst, ring, R, pos, d, H, P, D, cur);
    else if (ni <= 8) tile_dw_to<8, INTILE>(dst, ring, R, pos, d, H, P, D, cur);
    else tile_dw_to<16, INTILE>(dst, ring, R, pos, d, H, P, D, cur);
}

__device__ __forceinline__ void ring_store(float* __restrict__ ring, int R, unsigned pos, const float* t, int H, int nvalid) {
    const unsigned mask = (unsigned)R - 1u;
    for (int e = threadIdx.x; e < H * ST_TC; e += ST_NT) {
        const int h = e / ST_TC, c = e & (ST_TC - 1);
        if (c < nvalid) ring[(size_t)h * R + ((pos + (unsigned)c) & mask)] = t[e];
    }
}

// ---- stage j of the stack -------------------------------------------------------------------------------------------
struct StageArgs {
    const float* prev;      // packed block j-1 (null for j = 0)
    const float* cur;       // packed block j   (null for j = nblocks)
    float* y;               // [M,B,F], in place
    const float* ring_prev; // [M,H,Rp]   (j >= 1)
    float* ring_cur;        // [M,H,Rc]   (j < nblocks)
    const unsigned* pos;    // device word: index of this chunk's first frame (RAGGED: one word per slot)
    const int* tab;         // RAGGED: step table [M][ST_TAB]
    int Rp, dp, Rc;
    int B, H, P, F, tiles;
};

// The cumulative forms take the record banks as well: stage / block j reads cur[(m * nblocks + j) * 2 + norm] and writes pend[same].
struct CumArgs {
    const CumRec* cur;
    CumRec* pend;
    int nblocks, j;         // j: the stage (StageArgs: blocks j-1 and j) or the block (RowsArgs)
};
struct StageArgsCum : StageArgs { CumArgs c; };
template <bool CUM> using stage_args_t = std::conditional_t<CUM, StageArgsCum, StageArgs>;

// RAGGED (every kernel of a step): slot m computes nf[m] <= F frames from its own ring position; a workgroup whose tile starts at or
// beyond nf[m] returns before its first load and barrier (blockIdx and the table only: uniform over the workgroup).
// CUM: cumulative statistics (tile_cumln) in place of the per-frame ones; tiles == 1, and this workgroup stores the pending records.
template <bool RAGGED, bool CUM>
__global__ __launch_bounds__(ST_NT) void stream_stage_kernel(stage_args_t<CUM> a) {
    extern __shared__ float lds[];
    float* ybuf = lds;                              // [B][16]
    float* hbuf = ybuf + (size_t)a.B * ST_TC;       // [H][16]
    float* part = hbuf + (size_t)a.H * ST_TC;       // [ST_GRP][16]  (CUM: ST_CUM_LDS bytes)
    const int m = blockIdx.x / a.tiles, k0 = (blockIdx.x % a.tiles) * ST_TC;
    const int nf = slot_frames<RAGGED>(a.tab, m, a.F);
    if (RAGGED && k0 >= nf) return;
    const int nvalid = min(ST_TC, nf - k0);
    const unsigned pos = a.pos[RAGGED ? m : 0] + (unsigned)k0;
    const int B = a.B, H = a.H, P = a.P;
    float* yg = a.y + (size_t)m * B * a.F;
    tile_load(ybuf, yg, B, a.F, k0, nvalid);
    if (a.prev) {
        const float* vec = a.prev + (size_t)2 * H * B;
        tile_dw_any<false>(hbuf, a.ring_prev + (size_t)m * H * a.Rp, a.Rp, pos, a.dp, H, P, vec + 4 + 4 * H, nullptr);
        if constexpr (CUM) {
            const size_t r = ((size_t)m * a.c.nblocks + (a.c.j - 1)) * 2 + 1;
            tile_cumln(hbuf, H, vec + 1, vec + 4 + 2 * H, vec + 4 + 3 * H, reinterpret_cast<double2*>(part), a.c.cur + r, a.c.pend + r, nvalid);
        } else {
            tile_cln(hbuf, H, vec + 1, vec + 4 + 2 * H, vec + 4 + 3 * H, part);
        }
        tile_gemm<EPI_ADD>(a.prev + (size_t)H * B, B / 16, H / 16, hbuf, ybuf);
        __syncthreads();
        tile_store(ybuf, yg, B, a.F, k0, nvalid);
    }
    if (a.cur) {
        const float* vec = a.cur + (size_t)2 * H * B;
        __syncthreads();
        tile_gemm<EPI_STORE>(a.cur, H / 16, B / 16, ybuf, hbuf);
        if constexpr (CUM) {
            const size_t r = ((size_t)m * a.c.nblocks + a.c.j) * 2;
            tile_cumln(hbuf, H, vec, vec + 4, vec + 4 + H, reinterpret_cast<double2*>(part), a.c.cur + r, a.c.pend + r, nvalid);
        } else {
            tile_cln(hbuf, H, vec, vec + 4, vec + 4 + H, part);
        }
        ring_store(a.ring_cur + (size_t)m * H * a.Rc, a.Rc, pos, hbuf, H, nvalid);
    }
}

// ---- the same block boundary for chunks of at most one tile per stream, spread over `nsplit` workgroups per stream ------------------
// One workgroup per tile leaves a single stream on ONE CU, which then streams 2*H*B weights by itself.  With at most ST_TC frames per
// stream a block is two launches whose workgroups each own a slice of a GEMM's output rows (= of its weights):
//   rows_a:  h[slice] = W1[slice] . y                                              -> hraw [M,H,F] (scratch behind the rings)
//   rows_b:  n1 = cLN(PReLU(h)) (every workgroup, from the whole hraw column; slice 0 stores it in the ring) -> taps -> cLN(PReLU)
//            -> y[slice] += W2[slice] . n2
// Same device functions, same per-element FMA chains and sum orders as the stage kernel: bitwise the same values.
struct RowsArgs {
    const float* blk;       // packed block
    float* y;               // [M,B,F]
    float* hraw;            // [M,H,F]
    float* ring;            // [M,H,R]
    const unsigned* pos;
    const int* tab;         // RAGGED: step table
    int R, d;
    int B, H, P, F, nsplit;
};

template <bool RAGGED>
__global__ __launch_bounds__(ST_NT) void stream_rows_a_kernel(RowsArgs a) {
    extern __shared__ float lds[];
    float* ybuf = lds;
    float* hbuf = ybuf + (size_t)a.B * ST_TC;
    const int m = blockIdx.x / a.nsplit, sp = blockIdx.x % a.nsplit, wave = threadIdx.x >> 6;
    const int Rt = a.H / 16, per = (Rt + a.nsplit - 1) / a.nsplit, rt0 = min(sp * per, Rt), rt1 = min(rt0 + per, Rt);
    const int nf = slot_frames<RAGGED>(a.tab, m, a.F);     // a.F: leading dimension; nf: valid columns
    if (RAGGED && nf == 0) return;
    tile_load(ybuf, a.y + (size_t)m * a.B * a.F, a.B, a.F, 0, nf);
    __syncthreads();
    for (int rt = rt0 + wave; rt < rt1; rt += ST_NW) gemm_rows<EPI_STORE, 1>(reinterpret_cast<const float4*>(a.blk), rt, a.B / 16, ybuf, hbuf);
    __syncthreads();
    tile_store(hbuf + (size_t)rt0 * 16 * ST_TC, a.hraw + ((size_t)m * a.H + rt0 * 16) * a.F, (rt1 - rt0) * 16, a.F, 0, nf);
}

struct RowsArgsCum : RowsArgs { CumArgs c; };
template <bool CUM> using rows_args_t = std::conditional_t<CUM, RowsArgsCum, RowsArgs>;

// CUM: every one of the slot's nsplit workgroups reads the same two current records and forms the same statistics in the same order;
// slice 0 alone stores the pending ones.
template <bool RAGGED, bool CUM>
__global__ __launch_bounds__(ST_NT) void stream_rows_b_kernel(rows_args_t<CUM> a) {
    extern __shared__ float lds[];
    float* ybuf = lds;
    float* hbuf = ybuf + (size_t)a.B * ST_TC;
    float* part = hbuf + (size_t)a.H * ST_TC;
    const int m = blockIdx.x / a.nsplit, sp = blockIdx.x % a.nsplit, wave = threadIdx.x >> 6;
    const int B = a.B, H = a.H;
    const int Rt = B / 16, per = (Rt + a.nsplit - 1) / a.nsplit, rt0 = min(sp * per, Rt), rt1 = min(rt0 + per, Rt);
    const int nf = slot_frames<RAGGED>(a.tab, m, a.F);
    if (RAGGED && nf == 0) return;
    const unsigned pos = a.pos[RAGGED ? m : 0];
    const float* vec = a.blk + (size_t)2 * H * B;
    float* yg = a.y + ((size_t)m * B + rt0 * 16) * a.F;
    float* ring = a.ring + (size_t)m * H * a.R;
    tile_load(hbuf, a.hraw + (size_t)m * H * a.F, H, a.F, 0, nf);
    tile_load(ybuf + (size_t)rt0 * 16 * ST_TC, yg, (rt1 - rt0) * 16, a.F, 0, nf);
    if constexpr (CUM) {
        const size_t r = ((size_t)m * a.c.nblocks + a.c.j) * 2;
        tile_cumln(hbuf, H, vec, vec + 4, vec + 4 + H, reinterpret_cast<double2*>(part), a.c.cur + r, sp == 0 ? a.c.pend + r : nullptr, nf);
    } else {
        tile_cln(hbuf, H, vec, vec + 4, vec + 4 + H, part);
    }
    if (sp == 0) ring_store(ring, a.R, pos, hbuf, H, nf);
    tile_dw_any<true>(hbuf, ring, a.R, pos, a.d, H, a.P, vec + 4 + 4 * H, hbuf);
    if constexpr (CUM) {
        const size_t r = ((size_t)m * a.c.nblocks + a.c.j) * 2 + 1;
        tile_cumln(hbuf, H, vec + 1, vec + 4 + 2 * H, vec + 4 + 3 * H, reinterpret_cast<double2*>(part), a.c.cur + r,
                   sp == 0 ? a.c.pend + r : nullptr, nf);
    } else {
        tile_cln(hbuf, H, vec + 1, vec + 4 + 2 * H, vec + 4 + 3 * H, part);
    }
    for (int rt = rt0 + wave; rt < rt1; rt += ST_NW)
        gemm_rows<EPI_ADD, 1>(reinterpret_cast<const float4*>(a.blk + (size_t)H * B), rt, H / 16, hbuf, ybuf);
    __syncthreads();
    tile_store(ybuf + (size_t)rt0 * 16 * ST_TC, yg, (rt1 - rt0) * 16, a.F, 0, nf);
}

__global__ void stream_advance_kernel(unsigned* pos, int frames) {
    if (threadIdx.x == 0 && blockIdx.x == 0) pos[0] += (unsigned)frames;
}

__global__ __launch_bounds__(256) void stream_advance_ragged_kernel(unsigned* __restrict__ pos, const int* __restrict__ tab, int M, int F) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m < M) pos[m] += (unsigned)slot_frames<true>(tab, m, F);
}

// The last launch of a cumulative step: the pending records of every slot that computed frames become its current ones (`per` records per
// slot), and the ring position(s) advance as in the two kernels above.  Until here no kernel of the step has written a current record.
template <bool RAGGED>
__global__ __launch_bounds__(256) void stream_advance_cum_kernel(unsigned* __restrict__ pos, const int* __restrict__ tab, int M, int F,
                                                                 CumRec* __restrict__ cur, const CumRec* __restrict__ pend, int per) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < (long long)M * per && slot_frames<RAGGED>(tab, (int)(i / per), F) > 0) cur[i] = pend[i];
    if (RAGGED) {
        if (i < M) pos[i] += (unsigned)slot_frames<true>(tab, (int)i, F);
    } else if (i == 0) {
        pos[0] += (unsigned)F;
    }
}

// The listed slots' records, current and pending, back to zero: blockIdx.y = entry of the list, `per` records per slot and bank.
struct CumResetArgs {
    int slot[ST_RST_SLOTS];
};
__global__ __launch_bounds__(64) void stream_cum_reset_slots_kernel(CumRec* __restrict__ cum, CumResetArgs a, int M, int per) {
    const int m = a.slot[blockIdx.y];
    for (int i = blockIdx.x * 64 + threadIdx.x; i < 2 * per; i += gridDim.x * 64) {
        const size_t r = (size_t)(i / per) * M * per + (size_t)m * per + i % per;
        cum[r] = CumRec{0.0, 0.0, 0ull, 0ull};
    }
}

// ---- front end: frames of the sample buffer -> relu(U x) = w -> cLN -> bottleneck 1x1 = y ---------------------------
struct FrontArgs {
    const float* x; int xld;        // [M][xld] samples; frame k = x[k*S .. k*S+L)
    const float* Up; const float* g0; const float* b0; const float* Wbp;
    float* w; float* y;             // [M,N,F], [M,B,F]
    const int* tab;                 // RAGGED: step table
    int N, L, B, F, tiles;
};

template <bool RAGGED>
__global__ __launch_bounds__(ST_NT) void stream_front_kernel(FrontArgs a) {
    extern __shared__ float lds[];
    const int Lp = (a.L + 15) / 16 * 16, S = a.L / 2;
    float* xin = lds;                               // [Lp][16]
    float* wbuf = xin + (size_t)Lp * ST_TC;         // [N][16]
    float* ybuf = wbuf + (size_t)a.N * ST_TC;       // [B][16]
    float* part = ybuf + (size_t)a.B * ST_TC;
    const int m = blockIdx.x / a.tiles, k0 = (blockIdx.x % a.tiles) * ST_TC;
    const int nf = slot_frames<RAGGED>(a.tab, m, a.F);
    if (RAGGED && k0 >= nf) return;
    const int nvalid = min(ST_TC, nf - k0);
    const float* xg = a.x + (size_t)m * a.xld;
    for (int e = threadIdx.x; e < Lp * ST_TC; e += ST_NT) {
        const int i = e / ST_TC, c = e & (ST_TC - 1);
        const float v = xg[(size_t)(k0 + min(c, nvalid - 1)) * S + min(i, a.L - 1)];
        xin[e] = (i < a.L && c < nvalid) ? v : 0.f;
    }
    __syncthreads();
    tile_gemm<EPI_RELU>(a.Up, a.N / 16, Lp / 16, xin, wbuf);
    __syncthreads();
    tile_store(wbuf, a.w + (size_t)m * a.N * a.F, a.N, a.F, k0, nvalid);
    tile_cln(wbuf, a.N, nullptr, a.g0, a.b0, part);
    tile_gemm<EPI_STORE>(a.Wbp, a.B / 16, a.N / 16, wbuf, ybuf);
    __syncthreads();
    tile_store(ybuf, a.y + (size_t)m * a.B * a.F, a.B, a.F, k0, nvalid);
}

// ---- back end: mask 1x1 -> relu / softmax over speakers -> * w -> decoder basis -> frames [M,C,L,F] -----------------
struct BackArgs {
    const float* y; const float* w; const float* Wmp; const float* Vp;
    float* fr;                      // [M,C,L,F]
    const int* tab;                 // RAGGED: step table
    int N, L, B, C, F, tiles, softmax;
};

template <bool RAGGED>
__global__ __launch_bounds__(ST_NT) void stream_back_kernel(BackArgs a) {
    extern __shared__ float lds[];
    const int Lp = (a.L + 15) / 16 * 16, N = a.N, C = a.C;
    float* ybuf = lds;                                  // [B][16]
    float* sbuf = ybuf + (size_t)a.B * ST_TC;           // [C*N][16]
    float* fbuf = sbuf + (size_t)C * N * ST_TC;         // [C][Lp][16]
    const int m = blockIdx.x / a.tiles, k0 = (blockIdx.x % a.tiles) * ST_TC;
    const int nf = slot_frames<RAGGED>(a.tab, m, a.F);
    if (RAGGED && k0 >= nf) return;
    const int nvalid = min(ST_TC, nf - k0);
    tile_load(ybuf, a.y + (size_t)m * a.B * a.F, a.B, a.F, k0, nvalid);
    __syncthreads();
    tile_gemm<EPI_STORE>(a.Wmp, C * N / 16, a.B / 16, ybuf, sbuf);
    __syncthreads();
    const float* wg = a.w + (size_t)m * N * a.F;
    for (int e = threadIdx.x; e < N * ST_TC; e += ST_NT) {
        const int n = e / ST_TC, c = e & (ST_TC - 1);
        const float wl = wg[(size_t)n * a.F + k0 + min(c, nvalid - 1)];
        const float wv = c < nvalid ? wl : 0.f;
        if (!a.softmax) {
            for (int s = 0; s < C; ++s) sbuf[(size_t)s * N * ST_TC + e] = wv * fmaxf(sbuf[(size_t)s * N * ST_TC + e], 0.f);
        } else {
            float mx = -INFINITY, den = 0.f;
            for (int s = 0; s < C; ++s) mx = fmaxf(mx, sbuf[(size_t)s * N * ST_TC + e]);
            for (int s = 0; s < C; ++s) {
                const float ex = expf(sbuf[(size_t)s * N * ST_TC + e] - mx);
                sbuf[(size_t)s * N * ST_TC + e] = ex;
                den += ex;
            }
            for (int s = 0; s < C; ++s) sbuf[(size_t)s * N * ST_TC + e] = wv * (sbuf[(size_t)s * N * ST_TC + e] / den);
        }
    }
    __syncthreads();
    for (int s = 0; s < C; ++s) tile_gemm<EPI_STORE>(a.Vp, Lp / 16, N / 16, sbuf + (size_t)s * N * ST_TC, fbuf + (size_t)s * Lp * ST_TC);
    __syncthreads();
    for (int s = 0; s < C; ++s)
        tile_store(fbuf + (size_t)s * Lp * ST_TC, a.fr + ((size_t)m * C + s) * a.L * a.F, a.L, a.F, k0, nvalid);
}

// Overlap-add with the carried half frame (L = 2S: at most two frames meet in a sample, and a two-term sum commutes), then the carries:
// tail = second half of the last frame; the first S samples of the sample buffer = its last S consumed ones.  One thread per (row, r).
// RAGGED: nf[m] frames per row of slot m (F stays the leading dimension of fr and out); a slot with nf = 0 keeps both of its carries.
template <bool RAGGED>
__global__ __launch_bounds__(256) void stream_ola_kernel(const float* __restrict__ fr, float* __restrict__ out, float* __restrict__ tail,
                                                         float* __restrict__ x, int xld, int M, int MC, int L, int F,
                                                         const int* __restrict__ tab) {
    const int S = L / 2;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < MC * S) {
        const int mc = e / S, r = e % S;
        const int nf = slot_frames<RAGGED>(tab, mc / (MC / M), F);
        if (!RAGGED || nf > 0) {
            const float* f = fr + (size_t)mc * L * F;
            float prev = tail[e];
            float* o = out + (size_t)mc * F * S + r;
            for (int k = 0; k < nf; ++k) {
                o[(size_t)k * S] = f[(size_t)r * F + k] + prev;
                prev = f[(size_t)(r + S) * F + k];
            }
            tail[e] = prev;
        }
    }
    if (e < M * S) {
        const int m = e / S, i = e % S;
        const int nf = slot_frames<RAGGED>(tab, m, F);
        if (!RAGGED || nf > 0) x[(size_t)m * xld + i] = x[(size_t)m * xld + (size_t)nf * S + i];
    }
}

// ---- ragged steps: the caller's rows <-> the fixed buffers of a step, by the step table (all offsets in hops of S samples) ------------
// x[m][(dst + h) * S ..] = chunk[m][(src + h) * S ..] for h < nh[m]; nh is clamped to what fits in either row.
__global__ __launch_bounds__(256) void stream_load_ragged_kernel(const float* __restrict__ chunk, long long cld, int chunk_hops,
                                                                 float* __restrict__ x, int xld, const int* __restrict__ tab, int S) {
    const int m = blockIdx.y;
    const int* t = tab + m * ST_TAB;
    const int src = max(t[2], 0), dst = max(t[3], 0);
    const int room = min(xld / S - dst, chunk_hops - src);
    const long long n = (long long)min(max(t[1], 0), max(room, 0)) * S;
    const float* c = chunk + (size_t)m * cld + (size_t)src * S;
    float* o = x + (size_t)m * xld + (size_t)dst * S;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) o[i] = c[i];
}

// dst[m][c][(out + k) * S ..] = step output [M,C,F*S] frames k < nf[m]; clamped to the destination row.
__global__ __launch_bounds__(256) void stream_store_ragged_kernel(const float* __restrict__ out, float* __restrict__ dst, long long dld,
                                                                  const int* __restrict__ tab, int C, int S, int F) {
    const int mc = blockIdx.y, m = mc / C;
    const int off = max(tab[m * ST_TAB + 4], 0);
    const long long n = min((long long)slot_frames<true>(tab, m, F), max(dld / S - off, 0LL)) * S;
    const float* s = out + (size_t)mc * F * S;
    float* o = dst + (size_t)mc * dld + (size_t)off * S;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) o[i] = s[i];
}

// ---- per-slot reset: the listed slots' part of every ring, their carried hop, overlap-add carry and position word ----------------------
struct ResetArgs {
    float* ring0;                       // first ring of this launch
    float* x; float* tail; unsigned* pos;
    long long off[ST_RST_RINGS];        // ring j of this launch starts at ring0 + off[j]
    int R[ST_RST_RINGS];
    int slot[ST_RST_SLOTS];
    int nrings, H, xld, S, CS;          // CS = C * S; blockIdx.y == nrings: the small carries (only in the launch that has x != null)
};

__global__ __launch_bounds__(256) void stream_reset_slots_kernel(ResetArgs a) {
    const int j = blockIdx.y, m = a.slot[blockIdx.z];
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    if (j < a.nrings) {
        const size_t n4 = (size_t)a.H * a.R[j] / 4;         // H % 16 == 0 and the rings start 16-byte aligned
        float4* p = reinterpret_cast<float4*>(a.ring0 + a.off[j] + (size_t)m * a.H * a.R[j]);
        for (size_t i = t; i < n4; i += step) p[i] = float4{0.f, 0.f, 0.f, 0.f};
    } else if (a.x) {
        for (size_t i = t; i < (size_t)a.S; i += step) a.x[(size_t)m * a.xld + i] = 0.f;
        for (size_t i = t; i < (size_t)a.CS; i += step) a.tail[(size_t)m * a.CS + i] = 0.f;
        if (t == 0) a.pos[m] = 0u;
    }
}

}  // namespace

// =====================================================================================================================
extern "C" {

size_t ctn_stream_state_bytes(int M, int H, int P, const int* dilation, int nblocks, int max_frames) {
    if (M < 1 || H < 1 || P < 1 || !dilation || nblocks < 1 || max_frames < 1) return 0;
    size_t n = ST_HDR;
    for (int j = 0; j < nblocks; ++j) {
        if (dilation[j] < 1) return 0;
        n += (size_t)M * H * (size_t)ring_len(P, dilation[j], max_frames);
    }
    n += (size_t)M * H * ST_TC;      // hraw: one tile of first-1x1 outputs per stream (row-split form)
    return n * sizeof(float);
}

size_t ctn_stream_pack_gemm_bytes(int R, int Cn) {
    if (R < 1 || Cn < 1) return 0;
    return (size_t)c16(R) * c16(Cn) * 256 * sizeof(float);
}

int ctn_stream_pack_gemm(const float* W, int R, int Cn, void* packed, void* stream) {
    CTN_REQUIRE(W && packed, "ctn_stream_pack_gemm: null pointer");
    CTN_REQUIRE(R > 0 && Cn > 0, "ctn_stream_pack_gemm: bad sizes");
    CTN_REQUIRE(ctn_aligned16(packed), "ctn_stream_pack_gemm: packed must be 16-byte aligned");
    const long long n = (long long)c16(R) * c16(Cn) * 256;
    hipLaunchKernelGGL(stream_pack_kernel, dim3((unsigned)ctn_cdivll(n, 256)), dim3(256), 0, (hipStream_t)stream, W, (float*)packed, R, Cn);
    CTN_CHECK_LAUNCH("ctn_stream_pack_gemm");
    return CTN_OK;
}

size_t ctn_stream_pack_bytes(int B, int H, int P, int nblocks) {
    if (B < 1 || H < 1 || P < 1 || nblocks < 1 || B % 16 || H % 16) return 0;
    return (size_t)nblocks * block_floats(B, H, P) * sizeof(float);
}

int ctn_stream_pack(const void* const* params, int nblocks, int B, int H, int P, void* packed, void* stream) {
    CTN_REQUIRE(params && packed, "ctn_stream_pack: null pointer");
    CTN_REQUIRE(nblocks > 0 && B > 0 && H > 0 && B % 16 == 0 && H % 16 == 0, "ctn_stream_pack: B and H must be positive multiples of 16");
    CTN_REQUIRE(P >= 1 && P <= ST_MAXP, "ctn_stream_pack: kernel size must be 1..%d", ST_MAXP);
    CTN_REQUIRE(ctn_aligned16(packed), "ctn_stream_pack: packed must be 16-byte aligned");
    for (int i = 0; i < nblocks * 9; ++i) CTN_REQUIRE(params[i], "ctn_stream_pack: block %d parameter %d is null", i / 9, i % 9);
    const size_t bf = block_floats(B, H, P);
    for (int i = 0; i < nblocks; ++i) {
        const float* const* p = (const float* const*)(params + (size_t)i * 9);
        float* o = (float*)packed + (size_t)i * bf;
        const unsigned g = (unsigned)ctn_cdivll((long long)H * B, 256);
        hipLaunchKernelGGL(stream_pack_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, p[0], o, H, B);
        hipLaunchKernelGGL(stream_pack_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, p[8], o + (size_t)H * B, B, H);
        hipLaunchKernelGGL(stream_pack_vec_kernel, dim3((unsigned)ctn_cdiv(4 + 4 * H + H * P, 256)), dim3(256), 0, (hipStream_t)stream,
                           p[1], p[2], p[3], p[4], p[5], p[6], p[7], o + (size_t)2 * H * B, H, P);
    }
    CTN_CHECK_LAUNCH("ctn_stream_pack");
    return CTN_OK;
}

int ctn_stream_reset(void* state, size_t bytes, void* stream) {
    CTN_REQUIRE(state, "ctn_stream_reset: null pointer");
    CTN_REQUIRE(bytes >= ST_HDR * sizeof(float), "ctn_stream_reset: state smaller than its header");
    if (hipMemsetAsync(state, 0, bytes, (hipStream_t)stream) != hipSuccess) {
        ctn_set_error("ctn_stream_reset: %s", hipGetErrorString(hipGetLastError()));
        return CTN_ERR_LAUNCH;
    }
    return CTN_OK;
}

}  // extern "C"

namespace {

// tab == null: one frame count and the state's own position word; else the ragged step (table + one position word per slot).
// CUM: the cumulative kernels on the record banks in `cum` (frames <= ST_TC: one tile per slot), committed by the step's last launch.
template <bool CUM>
int tcn_launch(const void* packed, const int* dilation, int nblocks, float* y, void* state, void* cum, const int* tab, unsigned* pos_m,
               int M, int B, int H, int P, int frames, int max_frames, void* stream) {
    const size_t lds = (size_t)(B + H) * ST_TC * sizeof(float) + (CUM ? ST_CUM_LDS : ST_GRP * ST_TC * sizeof(float));
    const int tiles = ctn_cdiv(frames, ST_TC);
    const size_t bf = block_floats(B, H, P);
    float* ring = (float*)state + ST_HDR;
    const unsigned* pos = tab ? pos_m : (const unsigned*)state;
    const int per = nblocks * 2;                    // records per slot and bank
    CumArgs ca;
    ca.cur = (const CumRec*)cum; ca.pend = (CumRec*)cum + (size_t)M * per; ca.nblocks = nblocks; ca.j = 0;
    // at most one tile per stream and room for >= 2 workgroups per stream in one round of the CUs: two row-split launches per block
    const int cap = 256 / M;
    if (frames <= ST_TC && cap >= 2) {
        float* hraw = ring;
        for (int j = 0; j < nblocks; ++j) hraw += (size_t)M * H * (size_t)ring_len(P, dilation[j], max_frames);
        for (int j = 0; j < nblocks; ++j) {
            rows_args_t<CUM> a;
            a.blk = (const float*)packed + (size_t)j * bf;
            a.y = y; a.hraw = hraw; a.ring = ring; a.pos = pos; a.tab = tab;
            a.R = (int)ring_len(P, dilation[j], max_frames); a.d = dilation[j];
            a.B = B; a.H = H; a.P = P; a.F = frames;
            if constexpr (CUM) { a.c = ca; a.c.j = j; }
            a.nsplit = std::max(1, std::min(std::min(H / 16, 16), cap));
            const RowsArgs& ra = a;                 // rows_a has no norm: one kernel for both
            if (tab) hipLaunchKernelGGL(stream_rows_a_kernel<true>, dim3((unsigned)(M * a.nsplit)), dim3(ST_NT), lds, (hipStream_t)stream, ra);
            else hipLaunchKernelGGL(stream_rows_a_kernel<false>, dim3((unsigned)(M * a.nsplit)), dim3(ST_NT), lds, (hipStream_t)stream, ra);
            a.nsplit = std::max(1, std::min(std::min(B / 16, 16), cap));
            if (tab) hipLaunchKernelGGL((stream_rows_b_kernel<true, CUM>), dim3((unsigned)(M * a.nsplit)), dim3(ST_NT), lds, (hipStream_t)stream, a);
            else hipLaunchKernelGGL((stream_rows_b_kernel<false, CUM>), dim3((unsigned)(M * a.nsplit)), dim3(ST_NT), lds, (hipStream_t)stream, a);
            ring += (size_t)M * H * a.R;
        }
    } else {
        float* ring_prev = nullptr;
        int Rp = 0;
        for (int j = 0; j <= nblocks; ++j) {
            stage_args_t<CUM> a;
            a.prev = j >= 1 ? (const float*)packed + (size_t)(j - 1) * bf : nullptr;
            a.cur = j < nblocks ? (const float*)packed + (size_t)j * bf : nullptr;
            a.y = y;
            a.ring_prev = ring_prev;
            a.Rp = Rp;
            a.dp = j >= 1 ? dilation[j - 1] : 0;
            a.ring_cur = j < nblocks ? ring : nullptr;
            a.Rc = j < nblocks ? (int)ring_len(P, dilation[j], max_frames) : 0;
            a.pos = pos; a.tab = tab;
            a.B = B; a.H = H; a.P = P; a.F = frames; a.tiles = tiles;
            if constexpr (CUM) { a.c = ca; a.c.j = j; }
            if (tab) hipLaunchKernelGGL((stream_stage_kernel<true, CUM>), dim3((unsigned)(M * tiles)), dim3(ST_NT), lds, (hipStream_t)stream, a);
            else hipLaunchKernelGGL((stream_stage_kernel<false, CUM>), dim3((unsigned)(M * tiles)), dim3(ST_NT), lds, (hipStream_t)stream, a);
            ring_prev = ring;
            Rp = a.Rc;
            ring += (size_t)M * H * a.Rc;
        }
    }
    if constexpr (CUM) {
        const dim3 g((unsigned)ctn_cdivll((long long)M * per, 256));
        if (tab) hipLaunchKernelGGL(stream_advance_cum_kernel<true>, g, dim3(256), 0, (hipStream_t)stream, pos_m, tab, M, frames, (CumRec*)cum, (const CumRec*)ca.pend, per);
        else hipLaunchKernelGGL(stream_advance_cum_kernel<false>, g, dim3(256), 0, (hipStream_t)stream, (unsigned*)state, tab, M, frames, (CumRec*)cum, (const CumRec*)ca.pend, per);
    } else if (tab) {
        hipLaunchKernelGGL(stream_advance_ragged_kernel, dim3((unsigned)ctn_cdiv(M, 256)), dim3(256), 0, (hipStream_t)stream, pos_m, tab, M, frames);
    } else {
        hipLaunchKernelGGL(stream_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned*)state, frames);
    }
    return CTN_OK;
}

// The argument checks every stack entry point shares (`fn`: its name in the messages).
int tcn_check(const char* fn, const void* packed, const int* dilation, int nblocks, const float* y, const void* state, int M, int B, int H,
              int P, int frames, int max_frames) {
    CTN_REQUIRE(packed && dilation && y && state, "%s: null pointer", fn);
    CTN_REQUIRE(nblocks > 0 && M > 0, "%s: bad sizes", fn);
    CTN_REQUIRE(B > 0 && H > 0 && B % 16 == 0 && H % 16 == 0, "%s: B and H must be positive multiples of 16 (got %d, %d)", fn, B, H);
    CTN_REQUIRE(P >= 1 && P <= ST_MAXP, "%s: kernel size must be 1..%d (got %d)", fn, ST_MAXP, P);
    CTN_REQUIRE(max_frames >= 1 && max_frames <= (1 << 20), "%s: bad max_frames", fn);
    CTN_REQUIRE(frames >= 1 && frames <= max_frames, "%s: frames must be 1..max_frames (got %d, max_frames %d)", fn, frames, max_frames);
    CTN_REQUIRE(ctn_aligned16(packed) && ctn_aligned16(state), "%s: packed and state must be 16-byte aligned", fn);
    for (int j = 0; j < nblocks; ++j)
        CTN_REQUIRE(dilation[j] >= 1 && dilation[j] <= (1 << 20), "%s: bad dilation %d of block %d", fn, dilation[j], j);
    return CTN_OK;
}

// ... and what the cumulative ones add: one tile per step, the record banks, the LDS of tile_cumln.
int tcn_check_cum(const char* fn, const void* cum, int B, int H, int frames) {
    CTN_REQUIRE(frames <= ST_TC, "%s: at most %d frames per step (got %d): cut longer chunks into consecutive steps", fn, ST_TC, frames);
    CTN_REQUIRE(cum, "%s: null record buffer (cum)", fn);
    CTN_REQUIRE(ctn_aligned16(cum), "%s: cum must be 16-byte aligned", fn);
    const size_t lds = (size_t)(B + H) * ST_TC * sizeof(float) + ST_CUM_LDS;
    CTN_REQUIRE(lds <= ST_MAX_LDS, "%s: B + H = %d needs %zu bytes of LDS per tile with the fp64 partial sums (limit %zu)", fn, B + H, lds, ST_MAX_LDS);
    return CTN_OK;
}

}  // namespace

extern "C" {

int ctn_stream_tcn_cln(const void* packed, const int* dilation, int nblocks, float* y, void* state, int M, int B, int H, int P,
                       int frames, int max_frames, void* stream) {
    if (int rc = tcn_check("ctn_stream_tcn_cln", packed, dilation, nblocks, y, state, M, B, H, P, frames, max_frames)) return rc;
    const size_t lds = ((size_t)(B + H) * ST_TC + ST_GRP * ST_TC) * sizeof(float);
    CTN_REQUIRE(lds <= ST_MAX_LDS, "ctn_stream_tcn_cln: B + H = %d needs %zu bytes of LDS per tile (limit %zu)", B + H, lds, ST_MAX_LDS);
    tcn_launch<false>(packed, dilation, nblocks, y, state, nullptr, nullptr, nullptr, M, B, H, P, frames, max_frames, stream);
    CTN_CHECK_LAUNCH("ctn_stream_tcn_cln");
    return CTN_OK;
}

int ctn_stream_front(const float* x, int xld, const void* Up, const float* g0, const float* b0, const void* Wbp, float* w, float* y,
                     int M, int N, int L, int B, int frames, void* stream) {
    CTN_REQUIRE(x && Up && g0 && b0 && Wbp && w && y, "ctn_stream_front: null pointer");
    CTN_REQUIRE(M > 0 && frames > 0, "ctn_stream_front: bad sizes");
    CTN_REQUIRE(N > 0 && B > 0 && N % 16 == 0 && B % 16 == 0, "ctn_stream_front: N and B must be positive multiples of 16 (got %d, %d)", N, B);
    CTN_REQUIRE(L >= 4 && L % 4 == 0, "ctn_stream_front: L must be a multiple of 4 (got %d)", L);
    CTN_REQUIRE((long long)xld >= (long long)(frames + 1) * (L / 2), "ctn_stream_front: sample buffer row shorter than frames + 1 hops");
    CTN_REQUIRE(ctn_aligned16(Up) && ctn_aligned16(Wbp), "ctn_stream_front: packed weights must be 16-byte aligned");
    const size_t lds = ((size_t)(c16(L) * 16 + N + B) * ST_TC + ST_GRP * ST_TC) * sizeof(float);
    CTN_REQUIRE(lds <= ST_MAX_LDS, "ctn_stream_front: N + B = %d needs %zu bytes of LDS per tile (limit %zu)", N + B, lds, ST_MAX_LDS);
    FrontArgs a;
    a.x = x; a.xld = xld; a.Up = (const float*)Up; a.g0 = g0; a.b0 = b0; a.Wbp = (const float*)Wbp; a.w = w; a.y = y; a.tab = nullptr;
    a.N = N; a.L = L; a.B = B; a.F = frames; a.tiles = ctn_cdiv(frames, ST_TC);
    hipLaunchKernelGGL(stream_front_kernel<false>, dim3((unsigned)(M * a.tiles)), dim3(ST_NT), lds, (hipStream_t)stream, a);
    CTN_CHECK_LAUNCH("ctn_stream_front");
    return CTN_OK;
}

int ctn_stream_back(const float* y, const float* w, const void* Wmp, const void* Vp, float* fr, float* out, float* ola_tail,
                    float* x, int xld, int M, int N, int L, int B, int C, int frames, int softmax, void* stream) {
    CTN_REQUIRE(y && w && Wmp && Vp && fr && out && ola_tail && x, "ctn_stream_back: null pointer");
    CTN_REQUIRE(M > 0 && frames > 0 && C > 0, "ctn_stream_back: bad sizes");
    CTN_REQUIRE(N > 0 && B > 0 && N % 16 == 0 && B % 16 == 0, "ctn_stream_back: N and B must be positive multiples of 16 (got %d, %d)", N, B);
    CTN_REQUIRE(L >= 4 && L % 4 == 0, "ctn_stream_back: L must be a multiple of 4 (got %d)", L);
    CTN_REQUIRE(softmax == 0 || softmax == 1, "ctn_stream_back: mask must be 0 (relu) or 1 (softmax)");
    CTN_REQUIRE(C <= ST_MAXC, "ctn_stream_back: at most %d speakers", ST_MAXC);
    CTN_REQUIRE((long long)xld >= (long long)(frames + 1) * (L / 2), "ctn_stream_back: sample buffer row shorter than frames + 1 hops");
    CTN_REQUIRE(ctn_aligned16(Wmp) && ctn_aligned16(Vp), "ctn_stream_back: packed weights must be 16-byte aligned");
    const size_t lds = ((size_t)B + (size_t)C * N + (size_t)C * c16(L) * 16) * ST_TC * sizeof(float);
    CTN_REQUIRE(lds <= ST_MAX_LDS, "ctn_stream_back: B + C*N = %d needs %zu bytes of LDS per tile (limit %zu)", B + C * N, lds, ST_MAX_LDS);
    BackArgs a;
    a.y = y; a.w = w; a.Wmp = (const float*)Wmp; a.Vp = (const float*)Vp; a.fr = fr; a.tab = nullptr;
    a.N = N; a.L = L; a.B = B; a.C = C; a.F = frames; a.tiles = ctn_cdiv(frames, ST_TC); a.softmax = softmax;
    hipLaunchKernelGGL(stream_back_kernel<false>, dim3((unsigned)(M * a.tiles)), dim3(ST_NT), lds, (hipStream_t)stream, a);
    hipLaunchKernelGGL(stream_ola_kernel<false>, dim3((unsigned)ctn_cdiv(M * C * (L / 2), 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)fr, out, ola_tail, x, xld, M, M * C, L, frames, (const int*)nullptr);
    CTN_CHECK_LAUNCH("ctn_stream_back");
    return CTN_OK;
}

// ---- ragged steps (a slot pool): the same launches driven by a per-slot step table ------------------------------------------------------
int ctn_stream_load_ragged(const float* chunk, long long cld, int chunk_hops, float* x, int xld, const int* tab, int M, int S, int max_hops,
                           void* stream) {
    CTN_REQUIRE(chunk && x, "ctn_stream_load_ragged: null pointer");
    CTN_REQUIRE(tab, "ctn_stream_load_ragged: null step table (tab)");
    CTN_REQUIRE(M > 0 && M <= 65535, "ctn_stream_load_ragged: M must be 1..65535 (got %d)", M);
    CTN_REQUIRE(S > 0, "ctn_stream_load_ragged: S must be positive (got %d)", S);
    CTN_REQUIRE(xld >= S && xld % S == 0, "ctn_stream_load_ragged: xld must be a positive multiple of S (got %d)", xld);
    CTN_REQUIRE(chunk_hops >= 1 && cld >= (long long)chunk_hops * S, "ctn_stream_load_ragged: chunk row stride (cld) shorter than chunk_hops hops");
    CTN_REQUIRE(max_hops >= 1 && max_hops <= xld / S, "ctn_stream_load_ragged: max_hops must be 1..xld/S (got %d)", max_hops);
    const unsigned gx = (unsigned)std::min(ctn_cdivll((long long)max_hops * S, 256), 64LL);
    hipLaunchKernelGGL(stream_load_ragged_kernel, dim3(gx, (unsigned)M), dim3(256), 0, (hipStream_t)stream, chunk, cld, chunk_hops, x, xld, tab, S);
    CTN_CHECK_LAUNCH("ctn_stream_load_ragged");
    return CTN_OK;
}

int ctn_stream_store_ragged(const float* out, float* dst, long long dld, const int* tab, int M, int C, int S, int frames, void* stream) {
    CTN_REQUIRE(out && dst, "ctn_stream_store_ragged: null pointer");
    CTN_REQUIRE(tab, "ctn_stream_store_ragged: null step table (tab)");
    CTN_REQUIRE(M > 0 && C > 0 && (long long)M * C <= 65535, "ctn_stream_store_ragged: M * C must be 1..65535");
    CTN_REQUIRE(S > 0 && frames > 0, "ctn_stream_store_ragged: S and frames must be positive");
    CTN_REQUIRE(dld >= S, "ctn_stream_store_ragged: destination row (dld) shorter than one hop");
    const unsigned gx = (unsigned)std::min(ctn_cdivll((long long)frames * S, 256), 64LL);
    hipLaunchKernelGGL(stream_store_ragged_kernel, dim3(gx, (unsigned)(M * C)), dim3(256), 0, (hipStream_t)stream, out, dst, dld, tab, C, S, frames);
    CTN_CHECK_LAUNCH("ctn_stream_store_ragged");
    return CTN_OK;
}

int ctn_stream_front_ragged(const float* x, int xld, const void* Up, const float* g0, const float* b0, const void* Wbp, float* w, float* y,
                            const int* tab, int M, int N, int L, int B, int frames, void* stream) {
    CTN_REQUIRE(x && Up && g0 && b0 && Wbp && w && y, "ctn_stream_front_ragged: null pointer");
    CTN_REQUIRE(tab, "ctn_stream_front_ragged: null step table (tab)");
    CTN_REQUIRE(M > 0 && frames > 0, "ctn_stream_front_ragged: M and frames must be positive (got %d, %d)", M, frames);
    CTN_REQUIRE(N > 0 && B > 0 && N % 16 == 0 && B % 16 == 0, "ctn_stream_front_ragged: N and B must be positive multiples of 16 (got %d, %d)", N, B);
    CTN_REQUIRE(L >= 4 && L % 4 == 0, "ctn_stream_front_ragged: L must be a multiple of 4 (got %d)", L);
    CTN_REQUIRE((long long)xld >= (long long)(frames + 1) * (L / 2), "ctn_stream_front_ragged: sample buffer row shorter than frames + 1 hops");
    CTN_REQUIRE(ctn_aligned16(Up) && ctn_aligned16(Wbp), "ctn_stream_front_ragged: packed weights must be 16-byte aligned");
    const size_t lds = ((size_t)(c16(L) * 16 + N + B) * ST_TC + ST_GRP * ST_TC) * sizeof(float);
    CTN_REQUIRE(lds <= ST_MAX_LDS, "ctn_stream_front_ragged: N + B = %d needs %zu bytes of LDS per tile (limit %zu)", N + B, lds, ST_MAX_LDS);
    FrontArgs a;
    a.x = x; a.xld = xld; a.Up = (const float*)Up; a.g0 = g0; a.b0 = b0; a.Wbp = (const float*)Wbp; a.w = w; a.y = y; a.tab = tab;
    a.N = N; a.L = L; a.B = B; a.F = frames; a.tiles = ctn_cdiv(frames, ST_TC);
    hipLaunchKernelGGL(stream_front_kernel<true>, dim3((unsigned)(M * a.tiles)), dim3(ST_NT), lds, (hipStream_t)stream, a);
    CTN_CHECK_LAUNCH("ctn_stream_front_ragged");
    return CTN_OK;
}

int ctn_stream_tcn_cln_ragged(const void* packed, const int* dilation, int nblocks, float* y, void* state, const int* tab, void* pos,
                              int M, int B, int H, int P, int frames, int max_frames, void* stream) {
    if (int rc = tcn_check("ctn_stream_tcn_cln_ragged", packed, dilation, nblocks, y, state, M, B, H, P, frames, max_frames)) return rc;
    CTN_REQUIRE(tab, "ctn_stream_tcn_cln_ragged: null step table (tab)");
    CTN_REQUIRE(pos, "ctn_stream_tcn_cln_ragged: null position array (pos)");
    const size_t lds = ((size_t)(B + H) * ST_TC + ST_GRP * ST_TC) * sizeof(float);
    CTN_REQUIRE(lds <= ST_MAX_LDS, "ctn_stream_tcn_cln_ragged: B + H = %d needs %zu bytes of LDS per tile (limit %zu)", B + H, lds, ST_MAX_LDS);
    tcn_launch<false>(packed, dilation, nblocks, y, state, nullptr, tab, (unsigned*)pos, M, B, H, P, frames, max_frames, stream);
    CTN_CHECK_LAUNCH("ctn_stream_tcn_cln_ragged");
    return CTN_OK;
}

int ctn_stream_back_ragged(const float* y, const float* w, const void* Wmp, const void* Vp, float* fr, float* out, float* ola_tail,
                           float* x, int xld, const int* tab, int M, int N, int L, int B, int C, int frames, int softmax, void* stream) {
    CTN_REQUIRE(y && w && Wmp && Vp && fr && out && ola_tail && x, "ctn_stream_back_ragged: null pointer");
    CTN_REQUIRE(tab, "ctn_stream_back_ragged: null step table (tab)");
    CTN_REQUIRE(M > 0 && frames > 0 && C > 0, "ctn_stream_back_ragged: M, C and frames must be positive (got %d, %d, %d)", M, C, frames);
    CTN_REQUIRE(N > 0 && B > 0 && N % 16 == 0 && B % 16 == 0, "ctn_stream_back_ragged: N and B must be positive multiples of 16 (got %d, %d)", N, B);
    CTN_REQUIRE(L >= 4 && L % 4 == 0, "ctn_stream_back_ragged: L must be a multiple of 4 (got %d)", L);
    CTN_REQUIRE(softmax == 0 || softmax == 1, "ctn_stream_back_ragged: mask must be 0 (relu) or 1 (softmax)");
    CTN_REQUIRE(C <= ST_MAXC, "ctn_stream_back_ragged: at most %d speakers", ST_MAXC);
    CTN_REQUIRE((long long)xld >= (long long)(frames + 1) * (L / 2), "ctn_stream_back_ragged: sample buffer row shorter than frames + 1 hops");
    CTN_REQUIRE(ctn_aligned16(Wmp) && ctn_aligned16(Vp), "ctn_stream_back_ragged: packed weights must be 16-byte aligned");
    const size_t lds = ((size_t)B + (size_t)C * N + (size_t)C * c16(L) * 16) * ST_TC * sizeof(float);
    CTN_REQUIRE(lds <= ST_MAX_LDS, "ctn_stream_back_ragged: B + C*N = %d needs %zu bytes of LDS per tile (limit %zu)", B + C * N, lds, ST_MAX_LDS);
    BackArgs a;
    a.y = y; a.w = w; a.Wmp = (const float*)Wmp; a.Vp = (const float*)Vp; a.fr = fr; a.tab = tab;
    a.N = N; a.L = L; a.B = B; a.C = C; a.F = frames; a.tiles = ctn_cdiv(frames, ST_TC); a.softmax = softmax;
    hipLaunchKernelGGL(stream_back_kernel<true>, dim3((unsigned)(M * a.tiles)), dim3(ST_NT), lds, (hipStream_t)stream, a);
    hipLaunchKernelGGL(stream_ola_kernel<true>, dim3((unsigned)ctn_cdiv(M * C * (L / 2), 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)fr, out, ola_tail, x, xld, M, M * C, L, frames, tab);
    CTN_CHECK_LAUNCH("ctn_stream_back_ragged");
    return CTN_OK;
}

int ctn_stream_reset_slots(void* state, float* x, int xld, float* ola_tail, void* pos, const int* slots, int nslots, int M, int H, int P,
                           const int* dilation, int nblocks, int max_frames, int C, int L, void* stream) {
    CTN_REQUIRE(state && x && ola_tail && pos && slots && dilation, "ctn_stream_reset_slots: null pointer");
    CTN_REQUIRE(M > 0 && nblocks > 0 && C > 0, "ctn_stream_reset_slots: bad sizes");
    CTN_REQUIRE(nslots >= 1 && nslots <= M, "ctn_stream_reset_slots: nslots must be 1..M (got %d, M %d)", nslots, M);
    CTN_REQUIRE(H > 0 && H % 16 == 0, "ctn_stream_reset_slots: H must be a positive multiple of 16 (got %d)", H);
    CTN_REQUIRE(P >= 1 && P <= ST_MAXP, "ctn_stream_reset_slots: kernel size must be 1..%d (got %d)", ST_MAXP, P);
    CTN_REQUIRE(max_frames >= 1 && max_frames <= (1 << 20), "ctn_stream_reset_slots: bad max_frames");
    CTN_REQUIRE(L >= 4 && L % 4 == 0 && xld >= L / 2, "ctn_stream_reset_slots: L must be a multiple of 4 and xld at least one hop");
    CTN_REQUIRE(ctn_aligned16(state), "ctn_stream_reset_slots: state must be 16-byte aligned");
    for (int j = 0; j < nblocks; ++j)
        CTN_REQUIRE(dilation[j] >= 1 && dilation[j] <= (1 << 20), "ctn_stream_reset_slots: bad dilation %d of block %d", dilation[j], j);
    for (int i = 0; i < nslots; ++i)
        CTN_REQUIRE(slots[i] >= 0 && slots[i] < M, "ctn_stream_reset_slots: slot %d (entry %d of the list) is outside 0..%d", slots[i], i, M - 1);
    ResetArgs a;
    a.x = nullptr; a.tail = ola_tail; a.pos = (unsigned*)pos;
    a.H = H; a.xld = xld; a.S = L / 2; a.CS = C * (L / 2);
    float* ring = (float*)state + ST_HDR;
    for (int j0 = 0; j0 < nblocks; j0 += ST_RST_RINGS) {
        a.ring0 = ring;
        a.nrings = std::min(ST_RST_RINGS, nblocks - j0);
        long long off = 0, rmax = 0;
        for (int j = 0; j < a.nrings; ++j) {
            a.off[j] = off;
            a.R[j] = (int)ring_len(P, dilation[j0 + j], max_frames);
            rmax = std::max(rmax, (long long)a.R[j]);
            off += (long long)M * H * a.R[j];
        }
        ring += off;
        const bool last = j0 + ST_RST_RINGS >= nblocks;     // the small carries ride on the last group of rings
        a.x = last ? x : nullptr;
        const unsigned gx = (unsigned)std::min(ctn_cdivll((long long)H * rmax / 4, 256 * 4), 64LL);
        for (int s0 = 0; s0 < nslots; s0 += ST_RST_SLOTS) {
            const int ns = std::min(ST_RST_SLOTS, nslots - s0);
            for (int i = 0; i < ns; ++i) a.slot[i] = slots[s0 + i];
            hipLaunchKernelGGL(stream_reset_slots_kernel, dim3(std::max(gx, 1u), (unsigned)(a.nrings + (last ? 1 : 0)), (unsigned)ns), dim3(256),
                               0, (hipStream_t)stream, a);
        }
    }
    CTN_CHECK_LAUNCH("ctn_stream_reset_slots");
    return CTN_OK;
}

// ---- the cumLN stack: the same launches with cumulative statistics, one carry record per slot, block and norm in `cum` ------------------
size_t ctn_stream_cum_bytes(int M, int nblocks) {
    if (M < 1 || nblocks < 1) return 0;
    return (size_t)2 * M * nblocks * 2 * sizeof(CumRec);
}

int ctn_stream_tcn_cumln(const void* packed, const int* dilation, int nblocks, float* y, void* state, void* cum, int M, int B, int H, int P,
                         int frames, int max_frames, void* stream) {
    const char* fn = "ctn_stream_tcn_cumln";
    if (int rc = tcn_check(fn, packed, dilation, nblocks, y, state, M, B, H, P, frames, max_frames)) return rc;
    if (int rc = tcn_check_cum(fn, cum, B, H, frames)) return rc;
    tcn_launch<true>(packed, dilation, nblocks, y, state, cum, nullptr, nullptr, M, B, H, P, frames, max_frames, stream);
    CTN_CHECK_LAUNCH("ctn_stream_tcn_cumln");
    return CTN_OK;
}

int ctn_stream_tcn_cumln_ragged(const void* packed, const int* dilation, int nblocks, float* y, void* state, void* cum, const int* tab,
                                void* pos, int M, int B, int H, int P, int frames, int max_frames, void* stream) {
    const char* fn = "ctn_stream_tcn_cumln_ragged";
    if (int rc = tcn_check(fn, packed, dilation, nblocks, y, state, M, B, H, P, frames, max_frames)) return rc;
    CTN_REQUIRE(tab, "%s: null step table (tab)", fn);
    CTN_REQUIRE(pos, "%s: null position array (pos)", fn);
    if (int rc = tcn_check_cum(fn, cum, B, H, frames)) return rc;
    tcn_launch<true>(packed, dilation, nblocks, y, state, cum, tab, (unsigned*)pos, M, B, H, P, frames, max_frames, stream);
    CTN_CHECK_LAUNCH("ctn_stream_tcn_cumln_ragged");
    return CTN_OK;
}

int ctn_stream_cum_reset_slots(void* cum, const int* slots, int nslots, int M, int nblocks, void* stream) {
    CTN_REQUIRE(cum && slots, "ctn_stream_cum_reset_slots: null pointer");
    CTN_REQUIRE(ctn_aligned16(cum), "ctn_stream_cum_reset_slots: cum must be 16-byte aligned");
    CTN_REQUIRE(M > 0 && nblocks > 0, "ctn_stream_cum_reset_slots: bad sizes");
    CTN_REQUIRE(nslots >= 1 && nslots <= M, "ctn_stream_cum_reset_slots: nslots must be 1..M (got %d, M %d)", nslots, M);
    for (int i = 0; i < nslots; ++i)
        CTN_REQUIRE(slots[i] >= 0 && slots[i] < M, "ctn_stream_cum_reset_slots: slot %d (entry %d of the list) is outside 0..%d", slots[i], i, M - 1);
    const int per = nblocks * 2;
    for (int s0 = 0; s0 < nslots; s0 += ST_RST_SLOTS) {
        const int ns = std::min(ST_RST_SLOTS, nslots - s0);
        CumResetArgs a;
        for (int i = 0; i < ST_RST_SLOTS; ++i) a.slot[i] = slots[s0 + std::min(i, ns - 1)];
        hipLaunchKernelGGL(stream_cum_reset_slots_kernel, dim3((unsigned)std::min(ctn_cdiv(2 * per, 64), 64), (unsigned)ns), dim3(64), 0,
                           (hipStream_t)stream, (CumRec*)cum, a, M, per);
    }
    CTN_CHECK_LAUNCH("ctn_stream_cum_reset_slots");
    return CTN_OK;
}

}  // extern "C"
