// Mixture invariant training loss (MixIT: Wisdom et al., "Unsupervised Sound Separation Using Mixture Invariant Training",
// NeurIPS 2020) with the soft-thresholded SNR of the paper, gfx950.
//
// x [B,2,T] are two reference mixtures, e [B,M,T] the model's M outputs (2 <= M <= 8).  An assignment a in [0, 2^M) sends
// source i to mixture (a >> i) & 1; per mixture n
//     err_n = sum_t (sum_{i in A_n} e_i - x_n)^2,   l_n = 10 log10((err_n + tau Xx_n + EPS) / (Xx_n + EPS)),   L = (l_0 + l_1) / 2
// and the loss of an utterance is the minimum of L over the 2^M assignments (first minimum in ascending a).
//
// Pass 1 (HBM-bound): one sweep over x and e accumulating, per utterance and time chunk, the fp64 second-order moments over
//   t < len: the upper triangle of G[i][k] = sum e_i e_k, Xe[n][i] = sum x_n e_i, Xx[n] = sum x_n^2  (54 values at M = 8).
// Pass 2 (scalars): one wave per utterance sums the chunk partials in a fixed order, evaluates
//   err_n(a) = Xx_n - 2 sum_{i in A_n} Xe[n][i] + sum_{i,k in A_n} G[i][k] for every a (the lanes share the 2^M assignments),
//   keeps the first minimum and emits per_utt, assign, snr, the mean loss and the backward coefficients c_n.
// Backward: d_e[b,i,t] = [t < len] * scale_b * c_n * (sum_{k in A_n} e_k[t] - x_n[t]),  n = bit i of assign_b.
//
// The textbook form materialises the [B, 2^M, 2, T] remixes; this one needs none.  The time partition and the lane that owns
// a sample depend on T alone, and the aligned (16 bytes per lane) and the scalar load paths add the same values in the same
// order, so an utterance's result is bitwise the same in any batch, at any batch index and at any alignment.
#include "ctn_common.h"

extern "C" int ctn_sisnr_chunks(int T);      // csrc/ctn_loss.hip: the time partition, a function of T alone

namespace {

constexpr int NT = 256;            // moments and backward kernels
constexpr int NTA = 1024;          // assignment kernel: 16 waves, one utterance per wave at a time
constexpr int MINM = 2, MAXM = 8;
constexpr double EPSD = 1e-8;

__host__ __device__ constexpr int nmom(int M) { return M * (M + 1) / 2 + 2 * M + 2; }
__host__ __device__ constexpr int g_at(int M, int i, int k) { return i * M - i * (i - 1) / 2 + (k - i); }   // k >= i
__host__ __device__ constexpr int xe_at(int M, int n, int i) { return M * (M + 1) / 2 + n * M + i; }
__host__ __device__ constexpr int xx_at(int M, int n) { return M * (M + 1) / 2 + 2 * M + n; }

struct Quad { float v[4]; };

// four consecutive samples of one row starting at t (t % 4 == 0); samples at or beyond `len` read as 0 and are not touched
template <bool VEC>
__device__ __forceinline__ Quad load4(const float* __restrict__ row, int t, int len) {
    Quad q;
    if (VEC && t + 4 <= len) {
        const float4 f = *reinterpret_cast<const float4*>(row + t);
        q.v[0] = f.x; q.v[1] = f.y; q.v[2] = f.z; q.v[3] = f.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) q.v[j] = t + j < len ? row[t + j] : 0.f;
    }
    return q;
}

// partial[b][chunk][nmom(M)]; chunk % 4 == 0.  Lane tid owns the quads (t0 + 4 tid) + 4 NT k of its chunk, in ascending k.
template <int M, bool VEC>
__global__ __launch_bounds__(NT) void mixit_moments_kernel(const float* __restrict__ x, const float* __restrict__ e,
                                                           const long long* __restrict__ lens, int T, int chunk, int nchunk,
                                                           double* __restrict__ partial) {
    constexpr int NV = nmom(M);
    __shared__ double red[NT / 64][NV];
    const int b = blockIdx.x / nchunk, ch = blockIdx.x % nchunk;
    const int tid = threadIdx.x;
    long long ll = lens[b];
    if (ll > T) ll = T;
    if (ll < 0) ll = 0;
    const int len = (int)ll;
    const int t0 = ch * chunk, t1 = min(min(t0 + chunk, T), len);
    const float* __restrict__ xb = x + (size_t)b * 2 * T;
    const float* __restrict__ eb = e + (size_t)b * M * T;
    double acc[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) acc[q] = 0.0;
    for (int t = t0 + 4 * tid; t < t1; t += 4 * NT) {
        Quad xv[2], ev[M];
#pragma unroll
        for (int n = 0; n < 2; ++n) xv[n] = load4<VEC>(xb + (size_t)n * T, t, len);
#pragma unroll
        for (int i = 0; i < M; ++i) ev[i] = load4<VEC>(eb + (size_t)i * T, t, len);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int i = 0; i < M; ++i) {
                const double ei = (double)ev[i].v[j];
#pragma unroll
                for (int k = i; k < M; ++k) acc[g_at(M, i, k)] += ei * (double)ev[k].v[j];
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[xe_at(M, n, i)] += (double)xv[n].v[j] * ei;
            }
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[xx_at(M, n)] += (double)xv[n].v[j] * (double)xv[n].v[j];
        }
    }
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const double v = wave_sum(acc[q]);
        if ((tid & 63) == 0) red[tid >> 6][q] = v;
    }
    __syncthreads();
    if (tid < NV) {
        double s = red[0][tid];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) s += red[w][tid];
        partial[((size_t)b * nchunk + ch) * NV + tid] = s;
    }
}

// One block of 16 waves; wave w takes utterances w, w + 16, ...  coef [B,2], snr [B,2].
__global__ __launch_bounds__(NTA) void mixit_assign_kernel(const double* __restrict__ partial, int B, int M, int nchunk,
                                                           double tau, float* __restrict__ per_utt,
                                                           long long* __restrict__ assign, float* __restrict__ snr,
                                                           float* __restrict__ loss, float* __restrict__ coef) {
    constexpr int NW = NTA / 64;
    __shared__ double mo[NW][nmom(MAXM)];
    __shared__ double wsum[NW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nv = nmom(M), na = 1 << M;
    double local = 0.0;                       // lane 0: sum of this wave's per-utterance losses, ascending b
    for (int b0 = 0; b0 < B; b0 += NW) {      // block-uniform trip count: the barriers below are reached by every wave
        const int b = b0 + w;
        __syncthreads();                      // mo[w] may still be read for the previous utterance
        if (b < B && lane < nv) {
            double s = 0.0;
            for (int ch = 0; ch < nchunk; ++ch) s += partial[((size_t)b * nchunk + ch) * nv + lane];
            mo[w][lane] = s;
        }
        __syncthreads();
        if (b >= B) continue;
        const double* m = mo[w];
        const double xx0 = m[xx_at(M, 0)], xx1 = m[xx_at(M, 1)];
        double bestL = 0.0, bl0 = 0.0, bl1 = 0.0, be0 = 0.0, be1 = 0.0;
        int besta = na;                       // na: this lane has seen no assignment yet
        for (int a = lane; a < na; a += 64) {
            double err[2] = {xx0, xx1};
            for (int i = 0; i < M; ++i) {
                const int n = (a >> i) & 1;
                double s = m[g_at(M, i, i)] - 2.0 * m[xe_at(M, n, i)];
                for (int k = i + 1; k < M; ++k)
                    if (((a >> k) & 1) == n) s += 2.0 * m[g_at(M, i, k)];
                err[n] += s;
            }
            const double e0 = fmax(err[0], 0.0), e1 = fmax(err[1], 0.0);
            const double l0 = 10.0 * log10((e0 + tau * xx0 + EPSD) / (xx0 + EPSD));
            const double l1 = 10.0 * log10((e1 + tau * xx1 + EPSD) / (xx1 + EPSD));
            const double L = (l0 + l1) * 0.5;
            if (besta == na || L < bestL) { bestL = L; besta = a; bl0 = l0; bl1 = l1; be0 = e0; be1 = e1; }
        }
        // first minimum over the wave: smaller L wins, equal L -> smaller a (lanes without an assignment carry a = na)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double oL = __shfl_xor(bestL, o, 64), ol0 = __shfl_xor(bl0, o, 64), ol1 = __shfl_xor(bl1, o, 64);
            const double oe0 = __shfl_xor(be0, o, 64), oe1 = __shfl_xor(be1, o, 64);
            const int oa = __shfl_xor(besta, o, 64);
            const bool take = oa < na && (besta == na || oL < bestL || (oL == bestL && oa < besta));
            if (take) { bestL = oL; besta = oa; bl0 = ol0; bl1 = ol1; be0 = oe0; be1 = oe1; }
        }
        if (lane == 0) {
            per_utt[b] = (float)bestL;
            assign[b] = (long long)besta;
            snr[2 * (size_t)b] = (float)(0.0 - bl0);
            snr[2 * (size_t)b + 1] = (float)(0.0 - bl1);
            const double c10 = 10.0 / log(10.0);
            coef[2 * (size_t)b] = (float)(c10 / (be0 + tau * xx0 + EPSD));
            coef[2 * (size_t)b + 1] = (float)(c10 / (be1 + tau * xx1 + EPSD));
            local += bestL;
        }
    }
    if (lane == 0) wsum[w] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = wsum[0];
#pragma unroll
        for (int k = 1; k < NW; ++k) tot += wsum[k];
        loss[0] = (float)(tot / (double)B);
    }
}

// Each lane takes four consecutive samples of one utterance: reads the M + 2 rows, writes the M rows of d_e.
template <int M, bool VEC>
__global__ __launch_bounds__(NT) void mixit_bwd_kernel(const float* __restrict__ x, const float* __restrict__ e,
                                                       const long long* __restrict__ lens, const long long* __restrict__ assign,
                                                       const float* __restrict__ coef, const float* __restrict__ g_loss,
                                                       const float* __restrict__ g_per, int B, int T, int ntile,
                                                       float* __restrict__ de) {
#pragma clang fp contract(off)
    const int b = blockIdx.x / ntile, tile = blockIdx.x % ntile;
    const int t = (tile * NT + threadIdx.x) * 4;
    if (t >= T) return;
    long long ll = lens[b];
    if (ll > T) ll = T;
    if (ll < 0) ll = 0;
    const int len = (int)ll;
    const int a = (int)assign[b];
    float scale = 0.f;
    if (g_loss != nullptr) scale = g_loss[0] / (float)B;
    if (g_per != nullptr) scale += g_per[b];
    const float wn[2] = {scale * coef[2 * (size_t)b], scale * coef[2 * (size_t)b + 1]};
    const float* __restrict__ xb = x + (size_t)b * 2 * T;
    const float* __restrict__ eb = e + (size_t)b * M * T;
    float* __restrict__ db = de + (size_t)b * M * T;
    Quad mix[2], ev[M];
#pragma unroll
    for (int j = 0; j < 4; ++j) mix[0].v[j] = mix[1].v[j] = 0.f;
    if (t < len) {
#pragma unroll
        for (int i = 0; i < M; ++i) ev[i] = load4<VEC>(eb + (size_t)i * T, t, len);
#pragma unroll
        for (int i = 0; i < M; ++i) {          // ascending source index, one rounding per add (x + 0 is exact)
            const bool one = (a >> i) & 1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                mix[0].v[j] += one ? 0.f : ev[i].v[j];
                mix[1].v[j] += one ? ev[i].v[j] : 0.f;
            }
        }
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const Quad xv = load4<VEC>(xb + (size_t)n * T, t, len);
#pragma unroll
            for (int j = 0; j < 4; ++j) mix[n].v[j] = wn[n] * (mix[n].v[j] - xv.v[j]);     // samples >= len: fixed below
        }
    }
#pragma unroll
    for (int i = 0; i < M; ++i) {
        const int n = (a >> i) & 1;
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = t + j < len ? (n ? mix[1].v[j] : mix[0].v[j]) : 0.f;
        float* __restrict__ dst = db + (size_t)i * T + t;
        if (VEC) {                              // T % 4 == 0: the whole quad is inside the row
            *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (t + j < T) dst[j] = o[j];
        }
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

inline int mixit_chunk(int T, int nchunk) { return ctn_cdiv(ctn_cdiv(T, nchunk), 4) * 4; }

template <int M>
void launch_moments(bool vec, unsigned grid, hipStream_t st, const float* x, const float* e, const long long* lens, int T,
                    int chunk, int nchunk, double* partial) {
    if (vec)
        hipLaunchKernelGGL((mixit_moments_kernel<M, true>), dim3(grid), dim3(NT), 0, st, x, e, lens, T, chunk, nchunk, partial);
    else
        hipLaunchKernelGGL((mixit_moments_kernel<M, false>), dim3(grid), dim3(NT), 0, st, x, e, lens, T, chunk, nchunk, partial);
}

template <int M>
void launch_bwd(bool vec, unsigned grid, hipStream_t st, const float* x, const float* e, const long long* lens,
                const long long* assign, const float* coef, const float* g_loss, const float* g_per, int B, int T, int ntile,
                float* de) {
    if (vec)
        hipLaunchKernelGGL((mixit_bwd_kernel<M, true>), dim3(grid), dim3(NT), 0, st, x, e, lens, assign, coef, g_loss, g_per, B, T,
                           ntile, de);
    else
        hipLaunchKernelGGL((mixit_bwd_kernel<M, false>), dim3(grid), dim3(NT), 0, st, x, e, lens, assign, coef, g_loss, g_per, B, T,
                           ntile, de);
}

#define MIXIT_DISPATCH(M, CALL)                 \
    switch (M) {                                \
        case 2: CALL(2); break;                 \
        case 3: CALL(3); break;                 \
        case 4: CALL(4); break;                 \
        case 5: CALL(5); break;                 \
        case 6: CALL(6); break;                 \
        case 7: CALL(7); break;                 \
        default: CALL(8); break;                \
    }

}  // namespace

extern "C" {

size_t ctn_mixit_workspace(int B, int M, int T) {
    if (B <= 0 || M < MINM || M > MAXM || T <= 0) return 0;
    return (size_t)B * ctn_sisnr_chunks(T) * nmom(M) * sizeof(double);
}

// see include/ctn_hip.h
int ctn_mixit_fwd(const float* mixtures, const float* estimates, const long long* lengths, int B, int M, int T, double tau,
                  float* per_utt, long long* assign, float* snr, float* loss, float* coef, void* workspace,
                  size_t workspace_bytes, void* stream) {
    CTN_REQUIRE(mixtures && estimates && lengths && per_utt && assign && snr && loss && coef, "ctn_mixit_fwd: null pointer");
    CTN_REQUIRE(M >= MINM && M <= MAXM, "ctn_mixit_fwd: M = %d outside %d .. %d", M, MINM, MAXM);
    CTN_REQUIRE(B > 0 && T > 0 && tau >= 0.0, "ctn_mixit_fwd: bad sizes (B = %d, T = %d) or tau < 0", B, T);
    const int nchunk = ctn_sisnr_chunks(T);
    CTN_REQUIRE((long long)B * nchunk < (1ll << 31) && (long long)T + 4 * NT < (1ll << 31), "ctn_mixit_fwd: B * chunks or T too large");
    if (workspace == nullptr || workspace_bytes < ctn_mixit_workspace(B, M, T)) {
        ctn_set_error("ctn_mixit_fwd: workspace too small");
        return CTN_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (T % 4 == 0) && aligned16(mixtures) && aligned16(estimates);
    const int chunk = mixit_chunk(T, nchunk);
    const unsigned grid = (unsigned)(B * nchunk);
#define CALL(MM) launch_moments<MM>(vec, grid, st, mixtures, estimates, lengths, T, chunk, nchunk, (double*)workspace)
    MIXIT_DISPATCH(M, CALL)
#undef CALL
    CTN_CHECK_LAUNCH("ctn_mixit_fwd/moments");
    hipLaunchKernelGGL(mixit_assign_kernel, dim3(1), dim3(NTA), 0, st, (const double*)workspace, B, M, nchunk, tau, per_utt,
                       assign, snr, loss, coef);
    CTN_CHECK_LAUNCH("ctn_mixit_fwd/assign");
    return CTN_OK;
}

int ctn_mixit_bwd(const float* mixtures, const float* estimates, const long long* lengths, const long long* assign,
                  const float* coef, const float* g_loss, const float* g_per, int B, int M, int T, float* d_estimates,
                  void* stream) {
    CTN_REQUIRE(mixtures && estimates && lengths && assign && coef && d_estimates, "ctn_mixit_bwd: null pointer");
    CTN_REQUIRE(M >= MINM && M <= MAXM, "ctn_mixit_bwd: M = %d outside %d .. %d", M, MINM, MAXM);
    CTN_REQUIRE(B > 0 && T > 0, "ctn_mixit_bwd: bad sizes (B = %d, T = %d)", B, T);
    const int ntile = ctn_cdiv(ctn_cdiv(T, 4), NT);
    CTN_REQUIRE((long long)B * ntile < (1ll << 31) && (long long)T + 4 * NT < (1ll << 31), "ctn_mixit_bwd: B * tiles or T too large");
    const bool vec = (T % 4 == 0) && aligned16(mixtures) && aligned16(estimates) && aligned16(d_estimates);
    const unsigned grid = (unsigned)(B * ntile);
    hipStream_t st = (hipStream_t)stream;
#define CALL(MM) launch_bwd<MM>(vec, grid, st, mixtures, estimates, lengths, assign, coef, g_loss, g_per, B, T, ntile, d_estimates)
    MIXIT_DISPATCH(M, CALL)
#undef CALL
    CTN_CHECK_LAUNCH("ctn_mixit_bwd");
    return CTN_OK;
}

}  // extern "C"
