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
// The textbook form materialises the [B, 2^M, 2, T] remixes; this one needs none.  The sweep, the reductions, the first-minimum
// rule and the load and store paths are the skeleton of ctn_moment_loss.h, shared with ctn_varpit.hip; it keeps the promise that
// an utterance's result is bitwise the same in any batch, at any batch index and at any alignment.  This file holds MixIT's own
// algebra: which moments, the 2^M enumeration, the coefficients and the backward body.
#include "ctn_moment_loss.h"

namespace {

constexpr int MINM = 2, MAXM = 8;
constexpr double EPSD = 1e-8;

__host__ __device__ constexpr int nmom(int M) { return M * (M + 1) / 2 + 2 * M + 2; }
__host__ __device__ constexpr int g_at(int M, int i, int k) { return i * M - i * (i - 1) / 2 + (k - i); }   // k >= i
__host__ __device__ constexpr int xe_at(int M, int n, int i) { return M * (M + 1) / 2 + n * M + i; }
__host__ __device__ constexpr int xx_at(int M, int n) { return M * (M + 1) / 2 + 2 * M + n; }

// the sweep's policy: the rows x [2,T] and e [M,T] of an utterance, sample j of the loaded quads
template <int M>
struct MixitMoments {
    static constexpr int NREF = 2, NEST = M, NV = nmom(M);
    static __device__ __forceinline__ void accumulate(double (&acc)[NV], const Quad (&xv)[2], const Quad (&ev)[M], int j) {
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
};

// One block of 16 waves; wave w takes utterances w, w + 16, ...  coef [B,2], snr [B,2].
__global__ __launch_bounds__(NTA) void mixit_assign_kernel(const double* __restrict__ partial, int B, int M, int nchunk,
                                                           double tau, float* __restrict__ per_utt,
                                                           long long* __restrict__ assign, float* __restrict__ snr,
                                                           float* __restrict__ loss, float* __restrict__ coef) {
    constexpr int NW = NTA / 64;
    __shared__ double mo[NW][nmom(MAXM)];
    __shared__ double wsum[NW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int na = 1 << M;
    double local = 0.0;                       // lane 0: sum of this wave's per-utterance losses, ascending b
    for (int b0 = 0; b0 < B; b0 += NW) {      // block-uniform trip count: the barriers of sum_chunks_to_lds are reached by every wave
        const int b = b0 + w;
        sum_chunks_to_lds(partial, b, B, nmom(M), nchunk, mo[w]);
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
        wave_first_min(bestL, besta, na);
        const int src = besta & 63;           // the lane whose own first minimum is the winner: its l_n and err_n are the winner's
        bl0 = __shfl(bl0, src, 64), bl1 = __shfl(bl1, src, 64), be0 = __shfl(be0, src, 64), be1 = __shfl(be1, src, 64);
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
    mean_over_waves(local, wsum, B, loss);
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
    const int len = clamped_len(lens, b, T);
    const int a = (int)assign[b];
    const float scale = upstream_scale(g_loss, g_per, b, B);
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
        store4<VEC>(db + (size_t)i * T + t, o, t, T);
    }
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
    if (const int rc = grid_guard("ctn_mixit_fwd", "chunks", B, nchunk, T)) return rc;
    if (const int rc = workspace_guard("ctn_mixit_fwd", workspace, workspace_bytes, ctn_mixit_workspace(B, M, T))) return rc;
    hipStream_t st = (hipStream_t)stream;
    dispatch_n<MINM, MAXM>(M, [&](auto m) {
        launch_moment_sweep<MixitMoments<decltype(m)::value>>(mixtures, estimates, lengths, B, T, nchunk, (double*)workspace, st);
    });
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
    const int ntile = bwd_tiles(T);
    if (const int rc = grid_guard("ctn_mixit_bwd", "tiles", B, ntile, T)) return rc;
    const bool vec = (T % 4 == 0) && ctn_aligned16(mixtures) && ctn_aligned16(estimates) && ctn_aligned16(d_estimates);
    dispatch_n<MINM, MAXM>(M, [&](auto m) {
        constexpr int MM = decltype(m)::value;
        auto kernel = vec ? &mixit_bwd_kernel<MM, true> : &mixit_bwd_kernel<MM, false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)(B * ntile)), dim3(NT), 0, (hipStream_t)stream, mixtures, estimates, lengths, assign,
                           coef, g_loss, g_per, B, T, ntile, d_estimates);
    });
    CTN_CHECK_LAUNCH("ctn_mixit_bwd");
    return CTN_OK;
}

}  // extern "C"
