// Pairwise SI-SNR + permutation-invariant loss (src/pit_criterion.py:12-77), gfx950.
//
// Pass 1 (HBM-bound): one sweep over source/estimate accumulating, per utterance, the raw
//   second-order moments over t < len  (sum s_j, sum e_i, sum s_j^2, sum e_i^2, sum e_i s_j)
//   in fp64; it also zeroes the estimate for t >= len like the reference's in-place mask (:38).
// Pass 2 (C x C scalars): centre the moments, form snr[i][j] with the three EPS of :57,:62,:63,
//   enumerate the C! permutations (table from the host, itertools order, first max wins = argmax),
//   emit max_snr, the arg-max index, loss = -mean, and the per-(b,i) coefficients of the gradient.
// Backward: de[b,i,t] = [t<len] * scale_b * (A*(s_j[t]-mean s_j) + B*(e_i[t]-mean e_i)), j = perm_b(i).
//
// The reference materialises four [B,C,C,T] temporaries; the moment form needs none.  Algebra:
//   sum proj^2  = dot^2 * En / En'^2,   sum noise^2 = Ee - 2 dot^2/En' + dot^2 En/En'^2,  En' = En + EPS
// evaluated in fp64 so the cancellation at high SNR stays far below the 1e-3 dB budget.
#include "ctn_common.h"

namespace {

constexpr int NT = 256;
constexpr int MAXC = 6;
constexpr double EPSD = 1e-8;

__device__ __forceinline__ int nmom(int C) { return 4 * C + C * C; }

// partial[b][chunk][nmom]
__global__ __launch_bounds__(NT) void sisnr_moments_kernel(const float* __restrict__ src, float* __restrict__ est,
                                                           const long long* __restrict__ lens, int B, int C, int T,
                                                           int chunk, int nchunk, double* __restrict__ partial) {
    __shared__ double red[NT / 64];
    const int b = blockIdx.x / nchunk, ch = blockIdx.x % nchunk;
    const int tid = threadIdx.x;
    long long len = lens[b];
    if (len > T) len = T;
    if (len < 0) len = 0;
    const int t0 = ch * chunk, t1 = min(t0 + chunk, T);
    double ss[MAXC], se[MAXC], qs[MAXC], qe[MAXC], x[MAXC][MAXC];
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        ss[i] = se[i] = qs[i] = qe[i] = 0.0;
#pragma unroll
        for (int j = 0; j < MAXC; ++j) x[i][j] = 0.0;
    }
    const float* __restrict__ sb = src + (size_t)b * C * T;
    float* __restrict__ eb = est + (size_t)b * C * T;
    for (int t = t0 + tid; t < t1; t += NT) {
        if (t < len) {
            float sv[MAXC], ev[MAXC];
#pragma unroll
            for (int i = 0; i < MAXC; ++i)
                if (i < C) { sv[i] = sb[(size_t)i * T + t]; ev[i] = eb[(size_t)i * T + t]; }
#pragma unroll
            for (int i = 0; i < MAXC; ++i)
                if (i < C) {
                    ss[i] += sv[i]; se[i] += ev[i];
                    qs[i] += (double)sv[i] * sv[i]; qe[i] += (double)ev[i] * ev[i];
#pragma unroll
                    for (int j = 0; j < MAXC; ++j)
                        if (j < C) x[i][j] += (double)ev[i] * sv[j];
                }
        } else {
            for (int i = 0; i < C; ++i) eb[(size_t)i * T + t] = 0.f;   // estimate_source *= mask
        }
    }
    double* __restrict__ out = partial + ((size_t)b * nchunk + ch) * nmom(C);
#pragma unroll
    for (int i = 0; i < MAXC; ++i)
        if (i < C) {
            double v;
            v = block_sum<double, NT>(ss[i], red); if (tid == 0) out[i] = v;
            v = block_sum<double, NT>(se[i], red); if (tid == 0) out[C + i] = v;
            v = block_sum<double, NT>(qs[i], red); if (tid == 0) out[2 * C + i] = v;
            v = block_sum<double, NT>(qe[i], red); if (tid == 0) out[3 * C + i] = v;
#pragma unroll
            for (int j = 0; j < MAXC; ++j)
                if (j < C) { v = block_sum<double, NT>(x[i][j], red); if (tid == 0) out[4 * C + i * C + j] = v; }
        }
}

// coef[b][i][4] = {A, Bc, mean_e_i, mean_s_j}; jsel[b][i] = j
// One workgroup.  The nchunk-long sums of the nmom(C) moments are latency, not bytes: a pass of PIT_UB utterances puts one
// (utterance, moment) pair on every lane, issues its chunk loads eight at a time and adds them in chunk order into LDS; then
// thread b % NT does utterance b's algebra and permutation search, so every thread's share of the batch mean is summed in the
// order of one thread per utterance.
constexpr int PIT_UB = 32;      // utterances per pass (divides NT)
__global__ __launch_bounds__(NT) void sisnr_pit_kernel(const double* __restrict__ partial, const long long* __restrict__ lens,
                                                       const int* __restrict__ perms, int nperm, int B, int C, int T,
                                                       int nchunk, float* __restrict__ max_snr, long long* __restrict__ idx_out,
                                                       float* __restrict__ loss, float* __restrict__ snr_out,
                                                       float* __restrict__ coef, int* __restrict__ jsel) {
    __shared__ double red[NT / 64];
    __shared__ double mom[PIT_UB * (4 * MAXC + MAXC * MAXC)];
    double local = 0.0;
    const int nm = nmom(C);
    for (int b0 = 0; b0 < B; b0 += PIT_UB) {
        const int nb = min(PIT_UB, B - b0);
        __syncthreads();        // the previous pass has read mom
        for (int it = threadIdx.x; it < nb * nm; it += NT) {
            const double* __restrict__ p = partial + ((size_t)(b0 + it / nm) * nchunk) * nm + it % nm;
            double s = 0.0;
            int ch = 0;
            for (; ch + 8 <= nchunk; ch += 8) {
                double v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = p[(size_t)(ch + j) * nm];
#pragma unroll
                for (int j = 0; j < 8; ++j) s += v[j];
            }
            for (; ch < nchunk; ++ch) s += p[(size_t)ch * nm];
            mom[it] = s;
        }
        __syncthreads();
        const int off = (int)threadIdx.x - b0 % NT;
        if (off < 0 || off >= nb) continue;
        const int b = b0 + off;
        const double* mo = mom + off * nm;
        long long len = lens[b];
        if (len > T) len = T;
        const double n = (double)len;
        double ms[MAXC], me[MAXC], En[MAXC], Ee[MAXC];
        for (int i = 0; i < C; ++i) {
            ms[i] = mo[i] / n;
            me[i] = mo[C + i] / n;
            En[i] = fmax(mo[2 * C + i] - n * ms[i] * ms[i], 0.0);
            Ee[i] = fmax(mo[3 * C + i] - n * me[i] * me[i], 0.0);
        }
        double snr[MAXC][MAXC], dA[MAXC][MAXC], dB[MAXC][MAXC];
        for (int i = 0; i < C; ++i)
            for (int j = 0; j < C; ++j) {
                const double dot = mo[4 * C + i * C + j] - n * me[i] * ms[j];
                const double Enp = En[j] + EPSD;
                const double P = dot * dot * En[j] / (Enp * Enp);
                const double Nz = fmax(Ee[i] - 2.0 * dot * dot / Enp + P, 0.0);
                const double ratio = P / (Nz + EPSD);
                snr[i][j] = 10.0 * log10(ratio + EPSD);
                const double dsnr = (10.0 / log(10.0)) / (ratio + EPSD);
                const double dP = 2.0 * dot * En[j] / (Enp * Enp);
                const double dNz = -4.0 * dot / Enp + dP;
                dA[i][j] = dsnr * (dP / (Nz + EPSD) - P / ((Nz + EPSD) * (Nz + EPSD)) * dNz);
                dB[i][j] = 2.0 * dsnr * (-P / ((Nz + EPSD) * (Nz + EPSD)));
                if (snr_out != nullptr) snr_out[((size_t)b * C + i) * C + j] = (float)snr[i][j];
            }
        int best = 0;
        float bestv = 0.f;
        for (int p = 0; p < nperm; ++p) {
            float s = 0.f;   // fp32 sum over i, like the reference's einsum on fp32 snr
            for (int i = 0; i < C; ++i) s += (float)snr[i][perms[p * C + i]];
            if (p == 0 || s > bestv) { bestv = s; best = p; }
        }
        const float mx = bestv / (float)C;
        max_snr[b] = mx;
        idx_out[b] = best;
        local += (double)mx;
        for (int i = 0; i < C; ++i) {
            const int j = perms[best * C + i];
            float* cf = coef + ((size_t)b * C + i) * 4;
            cf[0] = (float)dA[i][j];
            cf[1] = (float)dB[i][j];
            cf[2] = (float)me[i];
            cf[3] = (float)ms[j];
            jsel[b * C + i] = j;
        }
    }
    const double tot = block_sum<double, NT>(local, red);
    if (threadIdx.x == 0) loss[0] = (float)(0.0 - tot / (double)B);
}

// g_loss: scalar upstream grad of loss (nullable); g_max: [B] upstream grad of max_snr (nullable)
__global__ __launch_bounds__(NT) void sisnr_bwd_kernel(const float* __restrict__ src, const float* __restrict__ est,
                                                       const long long* __restrict__ lens, const float* __restrict__ coef,
                                                       const int* __restrict__ jsel, const float* __restrict__ g_loss,
                                                       const float* __restrict__ g_max, int B, int C, int T,
                                                       float* __restrict__ dest) {
    const long long n = (long long)B * C * T;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
        const int t = (int)(i % T);
        const int bi = (int)(i / T);
        const int b = bi / C;
        float v = 0.f;
        if (t < lens[b]) {
            float scale = 0.f;
            if (g_loss != nullptr) scale -= g_loss[0] / (float)B;
            if (g_max != nullptr) scale += g_max[b];
            scale /= (float)C;
            const float* cf = coef + (size_t)bi * 4;
            const int j = jsel[bi];
            const float s = src[((size_t)b * C + j) * T + t];
            v = scale * (cf[0] * (s - cf[3]) + cf[1] * (est[i] - cf[2]));
        }
        dest[i] = v;
    }
}

}  // namespace

extern "C" {

int ctn_sisnr_chunks(int T) { int c = ctn_cdiv(T, 2048); return c < 1 ? 1 : (c > 64 ? 64 : c); }

size_t ctn_sisnr_workspace(int B, int C, int T) { return (size_t)B * ctn_sisnr_chunks(T) * (4 * C + C * C) * sizeof(double); }

// see include/ctn_hip.h
int ctn_sisnr_pit_fwd(const float* source, float* estimate, const long long* lengths, const int* perms, int nperm,
                      int B, int C, int T, float* max_snr, long long* best_idx, float* loss, float* snr_out,
                      float* coef, int* jsel, void* workspace, size_t workspace_bytes, void* stream) {
    CTN_REQUIRE(source && estimate && lengths && perms && max_snr && best_idx && loss && coef && jsel, "ctn_sisnr_pit_fwd: null pointer");
    CTN_REQUIRE(B > 0 && C > 0 && C <= MAXC && T > 0 && nperm > 0, "ctn_sisnr_pit_fwd: bad sizes (C <= %d)", MAXC);
    const int nchunk = ctn_sisnr_chunks(T);
    if (workspace == nullptr || workspace_bytes < ctn_sisnr_workspace(B, C, T)) {
        ctn_set_error("ctn_sisnr_pit_fwd: workspace too small");
        return CTN_ERR_WORKSPACE;
    }
    const int chunk = ctn_cdiv(T, nchunk);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sisnr_moments_kernel, dim3((unsigned)(B * nchunk)), dim3(NT), 0, st, source, estimate, lengths, B, C, T,
                       chunk, nchunk, (double*)workspace);
    CTN_CHECK_LAUNCH("ctn_sisnr_pit_fwd/moments");
    hipLaunchKernelGGL(sisnr_pit_kernel, dim3(1), dim3(NT), 0, st, (const double*)workspace, lengths, perms, nperm, B, C, T,
                       nchunk, max_snr, best_idx, loss, snr_out, coef, jsel);
    CTN_CHECK_LAUNCH("ctn_sisnr_pit_fwd/pit");
    return CTN_OK;
}

int ctn_sisnr_pit_bwd(const float* source, const float* estimate, const long long* lengths, const float* coef,
                      const int* jsel, const float* g_loss, const float* g_max, int B, int C, int T, float* d_estimate,
                      void* stream) {
    CTN_REQUIRE(source && estimate && lengths && coef && jsel && d_estimate, "ctn_sisnr_pit_bwd: null pointer");
    CTN_REQUIRE(B > 0 && C > 0 && C <= MAXC && T > 0, "ctn_sisnr_pit_bwd: bad sizes");
    long long nb = ctn_cdivll((long long)B * C * T, NT);
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(sisnr_bwd_kernel, dim3((unsigned)nb), dim3(NT), 0, (hipStream_t)stream, source, estimate, lengths, coef,
                       jsel, g_loss, g_max, B, C, T, d_estimate);
    CTN_CHECK_LAUNCH("ctn_sisnr_pit_bwd");
    return CTN_OK;
}

}  // extern "C"
