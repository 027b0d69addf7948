// Cumulative LayerNorm ("cLN" of Luo & Mesgarani 2019, eq. 12-14; CumLN elsewhere) of the causal model, gfx950: frame k is
// normalised by the mean and variance of ALL channels of ALL frames 0..k of its utterance.
//
//   forward :  s1_k = sum_c a[c,k], s2_k = sum_c a[c,k]^2 (a = prelu(y)), C1_k / C2_k their prefix sums, n_k = Ch (k+1),
//              mean_k = C1_k / n_k, rstd_k = 1 / sqrt(max(C2_k / n_k - mean_k^2, 0) + eps), out = gamma (a - mean_k) rstd_k + beta
//   backward:  t = gamma dOut, xh = (a - mean_k) rstd_k, p1_k = sum_c t, p2_k = sum_c t xh,
//              u_k = rstd_k p1_k / n_k, v_k = rstd_k^2 p2_k / n_k, (U, V, W)_j = sum_{j <= k < K} (u_k, v_k, v_k mean_k),
//              da[c,j] = rstd_j t - U_j + W_j - a V_j
//
// Per frame this is the affine form of the per-frame channel-wise norm with other constants, so inside a TemporalBlock the kernels
// around the norm stay (ctn_pw_gemm_cln / ctn_dw_fwd_cln, ctn_pw_dgrad_cln / ctn_dw_bwd_cln) and only the two small per-frame
// kernels between them are replaced by the scans here (ctn_cumln_stats_frame, ctn_cumln_bwd_frame).  The norm that has passes of
// its own gets ctn_cumln_fwd (sums, scan, apply: three tensor passes) and ctn_cumln_bwd (sums, scan, apply: five).
//
// Canonical order of the forward scan.  A frame's statistics must not depend on how a stream was cut into calls, so the fp64
// additions are ordered by the ABSOLUTE frame index a (frames of earlier calls + k): inside an aligned block of 64 absolute frames
// q_a = q_{a-1} + s_a runs sequentially from q = 0; the block prefixes run sequentially, P_{b+1} = P_b + q_{64b+63}; C_a = P_{a/64} +
// q_a.  The carry across calls -- (P1, P2, q1, q2) and the frame count, per utterance -- lives in device memory and is advanced by
// the scan kernel itself (a captured graph replays it).  The per-frame sums depend only on the frame's own Ch values, reduced in one
// fixed tree whatever the frame's position in the call: the 16-byte kernel and its scalar fallback share that tree.
//
// Nothing here waits on another workgroup (no flags, no look-back, no grid sync): a row's scan is ONE workgroup, the passes are
// separate launches in stream order.  No float atomics: bitwise reproducible run to run.
#include "ctn_common.h"

namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// ---------------------------------------------------------------------------
// the scans: one 1024-thread workgroup per utterance
// ---------------------------------------------------------------------------
constexpr int SC_NT = 1024, SC_NW = SC_NT / 64, SC_B = 64, SC_NB = 56, SC_LD = SC_B + 1;     // 56 blocks = 3584 frames per round
constexpr int SC_SLOTS = SC_NB * SC_B, SC_SPT = (SC_SLOTS + SC_NT - 1) / SC_NT;             // (rows of 65 doubles: a lane per block, no bank conflicts)

// part [M][nparts][Kp][2] fp64: (s1, s2) of frame k as nparts partials, summed here in the order of t.
// A round stages the sums of 56 blocks in LDS (slot = position inside its absolute block; the slots outside the call hold 0, which
// changes no sum).  Then ONE LANE per block runs that block's 64-step chain in place (wave 0: s1, wave 1: s2 -- the chains of different
// blocks are independent, so the longest dependent chain of a round is 64 additions), one thread per moment walks the block totals'
// prefix in block order, and all threads turn C = P + q into (mean, rstd).
__global__ __launch_bounds__(SC_NT) void cumln_scan_kernel(const double* __restrict__ part, int nparts, float* __restrict__ mean,
                                                           float* __restrict__ rstd, double* __restrict__ carry,
                                                           long long* __restrict__ count, int M, int Ch, int K, int Kp) {
    __shared__ double S[2][SC_NB][SC_LD];       // per-frame sums, then the chains q
    __shared__ double PB[2][SC_NB + 1];         // block prefixes of the round; [SC_NB]: the prefix the next round starts from
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = blockIdx.x;
    const long long a0 = count != nullptr ? count[m] : 0ll;
    double P[2] = {0.0, 0.0}, cq[2] = {0.0, 0.0};
    if (carry != nullptr) { P[0] = carry[4 * m]; P[1] = carry[4 * m + 1]; cq[0] = carry[4 * m + 2]; cq[1] = carry[4 * m + 3]; }
    const int o = (int)(a0 & (SC_B - 1));
    if (o == 0) { P[0] += cq[0]; P[1] += cq[1]; cq[0] = 0.0; cq[1] = 0.0; }     // the previous call ended a block: fold it (0 + 0 at the start)
    const long long nb = ((long long)o + K + SC_B - 1) / SC_B;         // 64-frame blocks this call touches
    const double* __restrict__ pm = part + (size_t)m * nparts * Kp * 2;
    for (long long b0 = 0; b0 < nb; b0 += SC_NB) {
#pragma unroll
        for (int u = 0; u < SC_SPT; ++u) {
            const int slot = tid + u * SC_NT;
            const long long k = b0 * SC_B + slot - o;
            double s1 = 0.0, s2 = 0.0;
            if (slot < SC_SLOTS && k >= 0 && k < K) {
#pragma unroll 4
                for (int t = 0; t < nparts; ++t) {
                    const double2 v = *reinterpret_cast<const double2*>(pm + ((size_t)t * Kp + (size_t)k) * 2);
                    s1 += v.x;
                    s2 += v.y;
                }
            }
            if (slot < SC_SLOTS) { S[0][slot / SC_B][slot % SC_B] = s1; S[1][slot / SC_B][slot % SC_B] = s2; }
        }
        __syncthreads();
        if (wave < 2 && lane < SC_NB) {
            double* const row = S[wave][lane];
            double r = (b0 == 0 && lane == 0) ? cq[wave] : 0.0;         // the block a previous call left unfinished
#pragma unroll 8
            for (int i = 0; i < SC_B; ++i) {
                r += row[i];
                row[i] = r;
            }
        }
        __syncthreads();
        if (tid < 2) {
            double p = P[tid];
            for (int b = 0; b < SC_NB; ++b) {
                PB[tid][b] = p;
                p += S[tid][b][SC_B - 1];
            }
            PB[tid][SC_NB] = p;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < SC_SPT; ++u) {
            const int slot = tid + u * SC_NT;
            const long long k = b0 * SC_B + slot - o;
            if (slot < SC_SLOTS && k >= 0 && k < K) {
                const int b = slot / SC_B, i = slot % SC_B;
                const double p1 = PB[0][b], p2 = PB[1][b], q1 = S[0][b][i], q2 = S[1][b][i];
                const double n = (double)Ch * (double)(a0 + k + 1);
                const double mu = (p1 + q1) / n;
                double var = (p2 + q2) / n - mu * mu;
                if (var < 0.0) var = 0.0;
                mean[(size_t)m * Kp + k] = (float)mu;
                rstd[(size_t)m * Kp + k] = (float)(1.0 / sqrt(var + (double)CTN_EPS));
                if (k == K - 1 && carry != nullptr) {
                    carry[4 * m] = p1; carry[4 * m + 1] = p2; carry[4 * m + 2] = q1; carry[4 * m + 3] = q2;
                }
            }
        }
        P[0] = PB[0][SC_NB]; P[1] = PB[1][SC_NB];
        __syncthreads();                                                // S and PB are written again in the next round
    }
    const float rpad = (float)(1.0 / sqrt((double)CTN_EPS));           // what the per-frame kernels give a frame of zeros
    for (int k = K + tid; k < Kp; k += SC_NT) {
        mean[(size_t)m * Kp + k] = 0.f;
        rstd[(size_t)m * Kp + k] = rpad;
    }
    if (tid == 0 && count != nullptr) count[m] = a0 + K;
}

// EXCLUSIVE prefix sums of three values over the workgroup's threads in thread order, each on top of its running total (fixed order)
__device__ __forceinline__ void block_scan3(double (&x)[3], double (&run)[3], double (*sh)[SC_NW], int lane, int wave) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            const double t = __shfl_up(x[f], o, 64);
            if (lane >= o) x[f] += t;
        }
    }
    __syncthreads();                                                    // sh may still be read by a previous call
    if (lane == 63) {
#pragma unroll
        for (int f = 0; f < 3; ++f) sh[f][wave] = x[f];
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        double base = run[f], all = run[f];
#pragma unroll
        for (int w = 0; w < SC_NW; ++w) {
            if (w == wave) base = all;
            all += sh[f][w];
        }
        run[f] = all;
        const double prev = __shfl_up(x[f], 1, 64);                     // the wave's inclusive sum up to the lane before
        x[f] = lane == 0 ? base : base + prev;
    }
}

// part [M][nparts][Kp][2] fp64: (p1, p2) of frame k.  Suffix sums over the valid frames as prefix sums of the reversed row: a thread
// takes 4 consecutive frames of a round of 4096 (sequentially), the threads' totals are scanned across the workgroup.
// fc [M][4][Kp] = (rstd, mean rstd, U - W + mean V, V / rstd): ctn_dw_bwd_cln's (and cumln_bwd_apply's) form
//   xh = a fc0 - fc1 ; da = gamma fc0 dN - fc2 - xh fc3   ( = rstd t - U + W - a V )
constexpr int BS_EPT = 4;
__global__ __launch_bounds__(SC_NT) void cumln_bwd_scan_kernel(const double* __restrict__ part, int nparts, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, float* __restrict__ fc, int M, int Ch,
                                                               int K, int Kp) {
    __shared__ double sh[3][SC_NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = blockIdx.x;
    const double* __restrict__ pm = part + (size_t)m * nparts * Kp * 2;
    float* const fo = fc + (size_t)m * 4 * Kp;
    double run[3] = {0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < K; c0 += SC_NT * BS_EPT) {
        double loc[BS_EPT][3], mu[BS_EPT], rs[BS_EPT], tot[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int e = 0; e < BS_EPT; ++e) {
            const int k = K - 1 - (c0 + tid * BS_EPT + e);
            double u = 0.0, v = 0.0, w = 0.0;
            mu[e] = 0.0; rs[e] = 1.0;
            if (k >= 0) {
                double p1 = 0.0, p2 = 0.0;
#pragma unroll 4
                for (int t = 0; t < nparts; ++t) {
                    const double2 q = *reinterpret_cast<const double2*>(pm + ((size_t)t * Kp + (size_t)k) * 2);
                    p1 += q.x;
                    p2 += q.y;
                }
                mu[e] = (double)mean[(size_t)m * Kp + k];
                rs[e] = (double)rstd[(size_t)m * Kp + k];
                const double n = (double)Ch * (double)(k + 1);
                u = rs[e] * p1 / n;
                v = rs[e] * rs[e] * p2 / n;
                w = v * mu[e];
            }
            tot[0] += u; tot[1] += v; tot[2] += w;
            loc[e][0] = tot[0]; loc[e][1] = tot[1]; loc[e][2] = tot[2];
        }
        double base[3] = {tot[0], tot[1], tot[2]};
        block_scan3(base, run, sh, lane, wave);                         // what the threads before and the rounds before add up to
#pragma unroll
        for (int e = 0; e < BS_EPT; ++e) {
            const int k = K - 1 - (c0 + tid * BS_EPT + e);
            if (k >= 0) {
                const double U = base[0] + loc[e][0], V = base[1] + loc[e][1], W = base[2] + loc[e][2];
                fo[k] = (float)rs[e];
                fo[(size_t)Kp + k] = (float)(mu[e] * rs[e]);
                fo[(size_t)2 * Kp + k] = (float)(U - W + mu[e] * V);
                fo[(size_t)3 * Kp + k] = (float)(V / rs[e]);
            }
        }
    }
    for (int k = K + tid; k < Kp; k += SC_NT) {                         // pad frames: the consumers mask them; keep them finite
        fo[k] = rstd[(size_t)m * Kp + k];
        fo[(size_t)Kp + k] = 0.f;
        fo[(size_t)2 * Kp + k] = 0.f;
        fo[(size_t)3 * Kp + k] = 0.f;
    }
}

// ---------------------------------------------------------------------------
// streaming passes of the forward.  256 threads = 64 channel groups x 4 frame slots; thread t holds slot q = t % 4 of channel
// group g = t / 4, i.e. channels g, g + 64, ...  VEC = 4: a slot is a frame quad (16 frames a workgroup, 16-byte accesses, the
// cln_*_v4 tiling); VEC = 1: a slot is one frame (unaligned rows, Kp % 16 != 0).  The reduction tree of a frame is the same in both:
// the thread's channels in order, xor-shuffles over the 16 groups of a wave, the 4 waves in order.
// ---------------------------------------------------------------------------
constexpr int CU_NT = 256, CU_NQ = 4, CU_NG = CU_NT / CU_NQ, CU_NW = CU_NT / 64;

template <int VEC>
__device__ __forceinline__ void ld_slot(const float* p, float (&v)[VEC]) {
    if constexpr (VEC == 4) { const float4 t = ld4(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else v[0] = p[0];
}
template <int VEC>
__device__ __forceinline__ void st_slot(float* p, const float (&v)[VEC]) {
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}

// per-frame (sum a, sum a^2) in fp64 -> work [M][Kp][2]
template <int VEC>
__global__ __launch_bounds__(CU_NT) void cumln_sums_kernel(const float* __restrict__ Y, double* __restrict__ work, int M, int Ch,
                                                           int K, int Kp, const float* __restrict__ alpha_p) {
    constexpr int FR = CU_NQ * VEC;
    __shared__ double sh[2][CU_NW][FR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = tid % CU_NQ, g = tid / CU_NQ;
    const int kb = (Kp + FR - 1) / FR;
    const int bx = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int m = bx / kb, kw = (bx % kb) * FR, k0 = kw + VEC * q;
    const bool has_a = alpha_p != nullptr;
    const float al = has_a ? alpha_p[0] : 1.f;
    double s1[VEC], s2[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) { s1[e] = 0.0; s2[e] = 0.0; }
    if (k0 < Kp) {
        const float* __restrict__ y = Y + (size_t)m * Ch * Kp + k0;
#pragma unroll 4
        for (int c = g; c < Ch; c += CU_NG) {
            float v[VEC];
            ld_slot<VEC>(y + (size_t)c * Kp, v);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const double a = (double)(has_a ? prelu_f(v[e], al) : v[e]);
                s1[e] += a;
                s2[e] += a * a;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
#pragma unroll
        for (int o = CU_NQ; o < 64; o <<= 1) { s1[e] += __shfl_xor(s1[e], o, 64); s2[e] += __shfl_xor(s2[e], o, 64); }
    }
    if (lane < CU_NQ) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) { sh[0][wave][VEC * q + e] = s1[e]; sh[1][wave][VEC * q + e] = s2[e]; }
    }
    __syncthreads();
    if (tid < FR && kw + tid < Kp) {
        double r1 = sh[0][0][tid], r2 = sh[1][0][tid];
#pragma unroll
        for (int w = 1; w < CU_NW; ++w) { r1 += sh[0][w][tid]; r2 += sh[1][w][tid]; }
        *reinterpret_cast<double2*>(work + ((size_t)m * Kp + kw + tid) * 2) = make_double2(r1, r2);
    }
}

// TRACK (16-byte form only: no thread of it leaves early): the maximum of |Out| per utterance, merged into amax_out [M][CTN_AMAX_SLOTS]
// as cln_fwd_v4_kernel does (h3 arithmetic of the GEMM that reads Out).  The stores are those of the untracked form.
template <int VEC, bool TRACK = false>
__global__ __launch_bounds__(CU_NT) void cumln_apply_kernel(const float* __restrict__ Y, float* __restrict__ Out,
                                                            const float* __restrict__ mean_i, const float* __restrict__ rstd_i, int M,
                                                            int Ch, int K, int Kp, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ alpha_p,
                                                            unsigned* __restrict__ amax_out) {
    static_assert(!TRACK || VEC == 4, "tracked maxima: the 16-byte form");
    constexpr int FR = CU_NQ * VEC;
    const int tid = threadIdx.x, q = tid % CU_NQ, g = tid / CU_NQ;
    const int kb = (Kp + FR - 1) / FR;
    const int bx = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int m = bx / kb, k0 = (bx % kb) * FR + VEC * q;
    if (k0 >= Kp) return;
    const bool has_a = alpha_p != nullptr;
    const float al = has_a ? alpha_p[0] : 1.f;
    float mu[VEC], rs[VEC];
    ld_slot<VEC>(mean_i + (size_t)m * Kp + k0, mu);
    ld_slot<VEC>(rstd_i + (size_t)m * Kp + k0, rs);
    const size_t off = (size_t)m * Ch * Kp + k0;
    float amax = 0.f;
#pragma unroll 4
    for (int c = g; c < Ch; c += CU_NG) {
        float v[VEC], r[VEC];
        ld_slot<VEC>(Y + off + (size_t)c * Kp, v);
        const float ga = gamma[c], be = beta[c];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float a = has_a ? prelu_f(v[e], al) : v[e];
            r[e] = k0 + e < K ? ga * ((a - mu[e]) * rs[e]) + be : 0.f;
            if constexpr (TRACK) amax = fmaxf(amax, fabsf(r[e]));
        }
        st_slot<VEC>(Out + off + (size_t)c * Kp, r);
    }
    if constexpr (TRACK) {
        __shared__ double sc[CU_NW];
        block_amax_atomic<CU_NT>(amax, sc, amax_out + (size_t)m * CTN_AMAX_SLOTS, bx % kb);
    }
}

// ---------------------------------------------------------------------------
// streaming passes of the backward, 16-byte form: NTB threads = 64 channel groups x NTB / 64 frame quads, i.e. the workgroups, the
// parameter-gradient partials pc [2][workgroups][Ch] and the dalpha partials of ctn_cln_bwd (ctn_cln_bwd_finalize finishes them):
// (256, 16 frames) or, under ctn_tune("cln_fr", 32), (512, 32 frames).
// ---------------------------------------------------------------------------
template <int NTB>
__global__ __launch_bounds__(NTB) void cumln_bwd_sums_kernel(const float* __restrict__ dOut, const float* __restrict__ Y,
                                                             const float* __restrict__ mean_i, const float* __restrict__ rstd_i,
                                                             double* __restrict__ work, int M, int Ch, int K, int Kp,
                                                             const float* __restrict__ gamma, const float* __restrict__ alpha_p,
                                                             float* __restrict__ pc) {
    constexpr int NQ = NTB / 64, FR = 4 * NQ, NW = NTB / 64;
    __shared__ double sh[2][NW][FR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = tid % NQ, g = tid / NQ;
    const int kb = Kp / FR, nblk = M * kb;
    const int bx = xcd_remap((int)blockIdx.x, nblk);
    const int m = bx / kb, kw = (bx % kb) * FR, k0 = kw + 4 * q;
    const bool has_a = alpha_p != nullptr;
    const float al = has_a ? alpha_p[0] : 1.f;
    const size_t off = (size_t)m * Ch * Kp + k0;
    float mu[4], rs[4];
    ld_slot<4>(mean_i + (size_t)m * Kp + k0, mu);
    ld_slot<4>(rstd_i + (size_t)m * Kp + k0, rs);
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
    for (int c = g; c < Ch; c += 64) {
        float y[4], d[4];
        ld_slot<4>(Y + off + (size_t)c * Kp, y);
        ld_slot<4>(dOut + off + (size_t)c * Kp, d);
        const float ga = gamma[c];
        float pg = 0.f, pb = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float dv = k0 + e < K ? d[e] : 0.f;                   // a pad frame of dOut may hold anything: select, never multiply
            const float a = has_a ? prelu_f(y[e], al) : y[e];
            const float xh = (a - mu[e]) * rs[e];
            pg += dv * xh;
            pb += dv;
            const float t = ga * dv;
            s1[e] += (double)t;
            s2[e] += (double)t * (double)xh;
        }
#pragma unroll
        for (int o = 1; o < NQ; o <<= 1) { pg += __shfl_xor(pg, o, 64); pb += __shfl_xor(pb, o, 64); }
        if (q == 0) {
            pc[(size_t)bx * Ch + c] = pg;
            pc[((size_t)nblk + bx) * Ch + c] = pb;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int o = NQ; o < 64; o <<= 1) { s1[e] += __shfl_xor(s1[e], o, 64); s2[e] += __shfl_xor(s2[e], o, 64); }
    }
    if (lane < NQ) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { sh[0][wave][4 * q + e] = s1[e]; sh[1][wave][4 * q + e] = s2[e]; }
    }
    __syncthreads();
    if (tid < FR) {
        double r1 = sh[0][0][tid], r2 = sh[1][0][tid];
#pragma unroll
        for (int w = 1; w < NW; ++w) { r1 += sh[0][w][tid]; r2 += sh[1][w][tid]; }
        *reinterpret_cast<double2*>(work + ((size_t)m * Kp + kw + tid) * 2) = make_double2(r1, r2);
    }
}

// TRACK: the maximum of |dY| per utterance, merged into amax_out [M][CTN_AMAX_SLOTS] as cln_bwd_v4_kernel does; same stores and partials
template <int NTB, bool TRACK = false>
__global__ __launch_bounds__(NTB) void cumln_bwd_apply_kernel(const float* __restrict__ dOut, const float* __restrict__ Y,
                                                              float* __restrict__ dY, const float* __restrict__ fc, int M, int Ch, int K,
                                                              int Kp, const float* __restrict__ gamma, const float* __restrict__ alpha_p,
                                                              float* __restrict__ dalpha_part, unsigned* __restrict__ amax_out) {
    constexpr int NQ = NTB / 64, FR = 4 * NQ;
    __shared__ float red[NTB / 64];
    const int tid = threadIdx.x, q = tid % NQ, g = tid / NQ;
    const int kb = Kp / FR, nblk = M * kb;
    const int bx = xcd_remap((int)blockIdx.x, nblk);
    const int m = bx / kb, k0 = (bx % kb) * FR + 4 * q;
    const bool has_a = alpha_p != nullptr;
    const float al = has_a ? alpha_p[0] : 1.f;
    const size_t off = (size_t)m * Ch * Kp + k0;
    const float* const fm = fc + (size_t)m * 4 * Kp + k0;
    float f0[4], f1[4], f2[4], f3[4];
    ld_slot<4>(fm, f0);
    ld_slot<4>(fm + (size_t)Kp, f1);
    ld_slot<4>(fm + (size_t)2 * Kp, f2);
    ld_slot<4>(fm + (size_t)3 * Kp, f3);
    float dal = 0.f, amax = 0.f;
#pragma unroll 2
    for (int c = g; c < Ch; c += 64) {
        float y[4], d[4], r[4];
        ld_slot<4>(Y + off + (size_t)c * Kp, y);
        ld_slot<4>(dOut + off + (size_t)c * Kp, d);             // (dY may alias dOut: read before this thread's store)
        const float ga = gamma[c];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float x = 0.f;
            if (k0 + e < K) {
                const float a = has_a ? prelu_f(y[e], al) : y[e];
                const float xh = a * f0[e] - f1[e];
                const float da = ga * f0[e] * d[e] - f2[e] - xh * f3[e];
                const bool neg = has_a && y[e] < 0.f;
                if (neg) dal += da * y[e];
                x = neg ? al * da : da;
            }
            r[e] = x;
            if constexpr (TRACK) amax = fmaxf(amax, fabsf(x));
        }
        st_slot<4>(dY + off + (size_t)c * Kp, r);
    }
    if (dalpha_part != nullptr) {
        dal = block_sum<float, NTB>(dal, red);
        if (tid == 0) dalpha_part[bx] = dal;
    }
    if constexpr (TRACK) {
        __shared__ double sc[NTB / 64];
        block_amax_atomic<NTB>(amax, sc, amax_out + (size_t)m * CTN_AMAX_SLOTS, bx % kb);
    }
}

// ---------------------------------------------------------------------------
// backward, generic form (unaligned rows, Kp no multiple of the frame tile): 64 frames x 4 waves over the channels; the parameter
// partials go to the first M rows of pc and the first M * ceil(Kp / 64) dalpha partials, the rest of both buffers is zeroed.
// ---------------------------------------------------------------------------
constexpr int GN_NT = 256;

__global__ __launch_bounds__(GN_NT) void cumln_bwd_sums_gen_kernel(const float* __restrict__ dOut, const float* __restrict__ Y,
                                                                   const float* __restrict__ mean_i, const float* __restrict__ rstd_i,
                                                                   double* __restrict__ work, int M, int Ch, int K, int Kp,
                                                                   const float* __restrict__ gamma, const float* __restrict__ alpha_p) {
    __shared__ double sh[2][4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kb = (Kp + 63) / 64;
    const int m = blockIdx.x / kb, k = (blockIdx.x % kb) * 64 + lane;
    const bool valid = k < K;
    const bool has_a = alpha_p != nullptr;
    const float al = has_a ? alpha_p[0] : 1.f;
    double s1 = 0.0, s2 = 0.0;
    if (valid) {
        const size_t off = (size_t)m * Ch * Kp + k;
        const float mu = mean_i[(size_t)m * Kp + k], rs = rstd_i[(size_t)m * Kp + k];
        for (int c = wave; c < Ch; c += 4) {
            const float yv = Y[off + (size_t)c * Kp];
            const float a = has_a ? prelu_f(yv, al) : yv;
            const float t = gamma[c] * dOut[off + (size_t)c * Kp];
            s1 += (double)t;
            s2 += (double)t * (double)((a - mu) * rs);
        }
    }
    sh[0][wave][lane] = s1;
    sh[1][wave][lane] = s2;
    __syncthreads();
    if (wave == 0 && k < Kp)
        *reinterpret_cast<double2*>(work + ((size_t)m * Kp + k) * 2) =
            make_double2(((sh[0][0][lane] + sh[0][1][lane]) + sh[0][2][lane]) + sh[0][3][lane],
                         ((sh[1][0][lane] + sh[1][1][lane]) + sh[1][2][lane]) + sh[1][3][lane]);
}

// dgamma / dbeta of one (m, c) row per wave -> pc [2][rows][Ch], row m
__global__ __launch_bounds__(GN_NT) void cumln_bwd_params_gen_kernel(const float* __restrict__ dOut, const float* __restrict__ Y,
                                                                     const float* __restrict__ mean_i, const float* __restrict__ rstd_i,
                                                                     int M, int Ch, int K, int Kp, const float* __restrict__ alpha_p,
                                                                     float* __restrict__ pc, int rows) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hb = (Ch + 3) / 4;
    const int m = blockIdx.x / hb, c = (blockIdx.x % hb) * 4 + wave;
    if (c >= Ch) return;
    const bool has_a = alpha_p != nullptr;
    const float al = has_a ? alpha_p[0] : 1.f;
    const size_t row = ((size_t)m * Ch + c) * Kp;
    float dg = 0.f, db = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float yv = Y[row + k], dv = dOut[row + k];
        const float a = has_a ? prelu_f(yv, al) : yv;
        dg += dv * ((a - mean_i[(size_t)m * Kp + k]) * rstd_i[(size_t)m * Kp + k]);
        db += dv;
    }
    dg = wave_sum(dg);
    db = wave_sum(db);
    if (lane == 0) {
        pc[(size_t)m * Ch + c] = dg;
        pc[((size_t)rows + m) * Ch + c] = db;
    }
}

__global__ __launch_bounds__(GN_NT) void cumln_bwd_apply_gen_kernel(const float* __restrict__ dOut, const float* __restrict__ Y,
                                                                    float* __restrict__ dY, const float* __restrict__ fc, int M, int Ch,
                                                                    int K, int Kp, const float* __restrict__ gamma,
                                                                    const float* __restrict__ alpha_p, float* __restrict__ dalpha_part) {
    __shared__ float red[GN_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kb = (Kp + 63) / 64;
    const int m = blockIdx.x / kb, k = (blockIdx.x % kb) * 64 + lane;
    const bool has_a = alpha_p != nullptr;
    const float al = has_a ? alpha_p[0] : 1.f;
    float dal = 0.f;
    if (k < Kp) {
        const size_t off = (size_t)m * Ch * Kp + k;
        const float* const fm = fc + (size_t)m * 4 * Kp + k;
        const float f0 = fm[0], f1 = fm[(size_t)Kp], f2 = fm[(size_t)2 * Kp], f3 = fm[(size_t)3 * Kp];
        for (int c = wave; c < Ch; c += 4) {
            float x = 0.f;
            if (k < K) {
                const float yv = Y[off + (size_t)c * Kp];
                const float a = has_a ? prelu_f(yv, al) : yv;
                const float xh = a * f0 - f1;
                const float da = gamma[c] * f0 * dOut[off + (size_t)c * Kp] - f2 - xh * f3;
                const bool neg = has_a && yv < 0.f;
                if (neg) dal += da * yv;
                x = neg ? al * da : da;
            }
            dY[off + (size_t)c * Kp] = x;
        }
    }
    if (dalpha_part != nullptr) {
        dal = block_sum<float, GN_NT>(dal, red);
        if (tid == 0) dalpha_part[blockIdx.x] = dal;
    }
}

}  // namespace

extern "C" {

int ctn_cln_bwd_blocks(int M, int Kp);                  // csrc/ctn_cln.hip: rows of the parameter-gradient partials
size_t ctn_cln_bwd_pc_floats(int M, int Ch, int Kp);

int ctn_cumln_stats_frame(const double* col_part, int nparts, float* mean, float* rstd, double* carry, long long* count, int M, int Ch,
                          int K, int Kp, void* stream) {
    CTN_REQUIRE(col_part && mean && rstd && nparts > 0 && M > 0 && Ch > 0 && K > 0 && Kp >= K, "ctn_cumln_stats_frame: bad arguments");
    CTN_REQUIRE(ctn_aligned16(col_part), "ctn_cumln_stats_frame: col_part must be 16-byte aligned");
    CTN_REQUIRE((carry == nullptr) == (count == nullptr), "ctn_cumln_stats_frame: carry and count come together");
    hipLaunchKernelGGL(cumln_scan_kernel, dim3((unsigned)M), dim3(SC_NT), 0, (hipStream_t)stream, col_part, nparts, mean, rstd, carry,
                       count, M, Ch, K, Kp);
    CTN_CHECK_LAUNCH("ctn_cumln_stats_frame");
    return CTN_OK;
}

int ctn_cumln_bwd_frame(const double* col_part, int nparts, const float* mean, const float* rstd, float* fc, int M, int Ch, int K, int Kp,
                        void* stream) {
    CTN_REQUIRE(col_part && mean && rstd && fc && nparts > 0 && M > 0 && Ch > 0 && K > 0 && Kp >= K, "ctn_cumln_bwd_frame: bad arguments");
    CTN_REQUIRE(ctn_aligned16(col_part), "ctn_cumln_bwd_frame: col_part must be 16-byte aligned");
    hipLaunchKernelGGL(cumln_bwd_scan_kernel, dim3((unsigned)M), dim3(SC_NT), 0, (hipStream_t)stream, col_part, nparts, mean, rstd, fc, M,
                       Ch, K, Kp);
    CTN_CHECK_LAUNCH("ctn_cumln_bwd_frame");
    return CTN_OK;
}

// work: [M][Kp][2] fp64 per-frame sums, then (backward) fc [M][4][Kp] fp32
size_t ctn_cumln_work_bytes(int M, int Kp) { return (size_t)M * Kp * (2 * sizeof(double) + 4 * sizeof(float)); }

// amax_out != NULL: the slots of amax_out[m] also receive the bits of max |Out[m]| (merged: the caller zeroes them), from the apply pass
// itself in the 16-byte form, from a ctn_absmax_rows pass behind the scalar form (as ctn_cln_fwd's fallbacks)
int ctn_cumln_fwd_amax(const float* Y, float* Out, float* mean, float* rstd, int M, int Ch, int K, int Kp, const float* gamma,
                       const float* beta, const float* alpha, double* carry, long long* count, void* work, unsigned* amax_out,
                       void* stream) {
    CTN_REQUIRE(Y && Out && mean && rstd && gamma && beta && work, "ctn_cumln_fwd: null pointer");
    CTN_REQUIRE(M > 0 && Ch > 0 && K > 0 && Kp >= K, "ctn_cumln_fwd: bad sizes");
    CTN_REQUIRE(ctn_aligned16(work), "ctn_cumln_fwd: work must be 16-byte aligned");
    CTN_REQUIRE((carry == nullptr) == (count == nullptr), "ctn_cumln_fwd: carry and count come together");
    hipStream_t st = (hipStream_t)stream;
    double* const sums = (double*)work;
    const bool v4 = Kp % 16 == 0 && ctn_aligned16(Y) && ctn_aligned16(Out) && ctn_aligned16(mean) && ctn_aligned16(rstd);
    const dim3 grid((unsigned)(M * ctn_cdiv(Kp, v4 ? 16 : 4)));
    if (v4) hipLaunchKernelGGL(cumln_sums_kernel<4>, grid, dim3(CU_NT), 0, st, Y, sums, M, Ch, K, Kp, alpha);
    else hipLaunchKernelGGL(cumln_sums_kernel<1>, grid, dim3(CU_NT), 0, st, Y, sums, M, Ch, K, Kp, alpha);
    CTN_CHECK_LAUNCH("ctn_cumln_fwd/sums");
    hipLaunchKernelGGL(cumln_scan_kernel, dim3((unsigned)M), dim3(SC_NT), 0, st, sums, 1, mean, rstd, carry, count, M, Ch, K, Kp);
    CTN_CHECK_LAUNCH("ctn_cumln_fwd/scan");
    if (v4 && amax_out != nullptr)
        hipLaunchKernelGGL((cumln_apply_kernel<4, true>), grid, dim3(CU_NT), 0, st, Y, Out, mean, rstd, M, Ch, K, Kp, gamma, beta, alpha, amax_out);
    else if (v4) hipLaunchKernelGGL((cumln_apply_kernel<4>), grid, dim3(CU_NT), 0, st, Y, Out, mean, rstd, M, Ch, K, Kp, gamma, beta, alpha, nullptr);
    else hipLaunchKernelGGL((cumln_apply_kernel<1>), grid, dim3(CU_NT), 0, st, Y, Out, mean, rstd, M, Ch, K, Kp, gamma, beta, alpha, nullptr);
    CTN_CHECK_LAUNCH("ctn_cumln_fwd/apply");
    if (!v4 && amax_out != nullptr) return ctn_absmax_rows(Out, M, (long long)Ch * Kp, amax_out, stream);      // scalar form: a pass of its own
    return CTN_OK;
}

int ctn_cumln_fwd(const float* Y, float* Out, float* mean, float* rstd, int M, int Ch, int K, int Kp, const float* gamma,
                  const float* beta, const float* alpha, double* carry, long long* count, void* work, void* stream) {
    return ctn_cumln_fwd_amax(Y, Out, mean, rstd, M, Ch, K, Kp, gamma, beta, alpha, carry, count, work, nullptr, stream);
}

// pc [2][ctn_cln_bwd_blocks(M, Kp)][Ch] and dalpha_part [ctn_cln_bwd_blocks(M, Kp)]: ctn_cln_bwd's layout, finished by ctn_cln_bwd_finalize
// amax_out != NULL: the slots of amax_out[m] also receive the bits of max |dY[m]| (merged), as for ctn_cumln_fwd_amax
int ctn_cumln_bwd_amax(const float* dOut, const float* Y, float* dY, const float* mean, const float* rstd, int M, int Ch, int K, int Kp,
                       const float* gamma, const float* alpha, float* dalpha_part, float* pc, void* work, unsigned* amax_out,
                       void* stream) {
    CTN_REQUIRE(dOut && Y && dY && mean && rstd && gamma && pc && work, "ctn_cumln_bwd: null pointer");
    CTN_REQUIRE(M > 0 && Ch > 0 && K > 0 && Kp >= K, "ctn_cumln_bwd: bad sizes");
    CTN_REQUIRE(!alpha || dalpha_part, "ctn_cumln_bwd: dalpha_part required with alpha");
    CTN_REQUIRE(ctn_aligned16(work), "ctn_cumln_bwd: work must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float* const dap = alpha ? dalpha_part : nullptr;
    double* const sums = (double*)work;
    float* const fc = (float*)(sums + (size_t)M * Kp * 2);
    const int rows = ctn_cln_bwd_blocks(M, Kp), fr = g_ctn_cln_fr;
    const bool v4 = Kp % fr == 0 && ctn_aligned16(dOut) && ctn_aligned16(Y) && ctn_aligned16(dY) && ctn_aligned16(mean) && ctn_aligned16(rstd);
    if (v4) {                                                           // rows == M * Kp / fr workgroups
        if (fr == 16) hipLaunchKernelGGL(cumln_bwd_sums_kernel<256>, dim3((unsigned)rows), dim3(256), 0, st, dOut, Y, mean, rstd, sums, M, Ch, K, Kp, gamma, alpha, pc);
        else hipLaunchKernelGGL(cumln_bwd_sums_kernel<512>, dim3((unsigned)rows), dim3(512), 0, st, dOut, Y, mean, rstd, sums, M, Ch, K, Kp, gamma, alpha, pc);
    } else {
        hipMemsetAsync(pc, 0, sizeof(float) * ctn_cln_bwd_pc_floats(M, Ch, Kp), st);
        if (dap) hipMemsetAsync(dap, 0, sizeof(float) * (size_t)rows, st);
        hipLaunchKernelGGL(cumln_bwd_params_gen_kernel, dim3((unsigned)(M * ctn_cdiv(Ch, 4))), dim3(GN_NT), 0, st, dOut, Y, mean, rstd, M, Ch,
                           K, Kp, alpha, pc, rows);
        CTN_CHECK_LAUNCH("ctn_cumln_bwd/params");
        hipLaunchKernelGGL(cumln_bwd_sums_gen_kernel, dim3((unsigned)(M * ctn_cdiv(Kp, 64))), dim3(GN_NT), 0, st, dOut, Y, mean, rstd, sums, M,
                           Ch, K, Kp, gamma, alpha);
    }
    CTN_CHECK_LAUNCH("ctn_cumln_bwd/sums");
    hipLaunchKernelGGL(cumln_bwd_scan_kernel, dim3((unsigned)M), dim3(SC_NT), 0, st, sums, 1, mean, rstd, fc, M, Ch, K, Kp);
    CTN_CHECK_LAUNCH("ctn_cumln_bwd/scan");
    if (v4) {
        const dim3 grid((unsigned)rows);
        if (amax_out != nullptr) {
            if (fr == 16) hipLaunchKernelGGL((cumln_bwd_apply_kernel<256, true>), grid, dim3(256), 0, st, dOut, Y, dY, fc, M, Ch, K, Kp, gamma, alpha, dap, amax_out);
            else hipLaunchKernelGGL((cumln_bwd_apply_kernel<512, true>), grid, dim3(512), 0, st, dOut, Y, dY, fc, M, Ch, K, Kp, gamma, alpha, dap, amax_out);
        } else if (fr == 16) hipLaunchKernelGGL((cumln_bwd_apply_kernel<256>), grid, dim3(256), 0, st, dOut, Y, dY, fc, M, Ch, K, Kp, gamma, alpha, dap, nullptr);
        else hipLaunchKernelGGL((cumln_bwd_apply_kernel<512>), grid, dim3(512), 0, st, dOut, Y, dY, fc, M, Ch, K, Kp, gamma, alpha, dap, nullptr);
    } else {
        hipLaunchKernelGGL(cumln_bwd_apply_gen_kernel, dim3((unsigned)(M * ctn_cdiv(Kp, 64))), dim3(GN_NT), 0, st, dOut, Y, dY, fc, M, Ch, K, Kp,
                           gamma, alpha, dap);
    }
    CTN_CHECK_LAUNCH("ctn_cumln_bwd/apply");
    if (!v4 && amax_out != nullptr) return ctn_absmax_rows(dY, M, (long long)Ch * Kp, amax_out, stream);       // general form: a pass of its own
    return CTN_OK;
}

int ctn_cumln_bwd(const float* dOut, const float* Y, float* dY, const float* mean, const float* rstd, int M, int Ch, int K, int Kp,
                  const float* gamma, const float* alpha, float* dalpha_part, float* pc, void* work, void* stream) {
    return ctn_cumln_bwd_amax(dOut, Y, dY, mean, rstd, M, Ch, K, Kp, gamma, alpha, dalpha_part, pc, work, nullptr, stream);
}

}  // extern "C"
