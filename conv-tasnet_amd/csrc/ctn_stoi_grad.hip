// Backward pass of the STOI / ESTOI scores of ctn_stoi.hip in fp64, gfx950: the gradient of d(estimate, reference) with respect
// to the estimate's samples, for a training loss (Kolbaek et al., ICASSP 2018; Fu et al., TASLP 2018).
//
// Only the chosen pairs are differentiated: reference row c of utterance b is paired with estimate row est_of_ref[b, c].  A pair
// is laid out as an utterance of its own (P = B * C pair rows, one reference and one estimate each), so the forward is the
// forward chain of ctn_stoi.hip on P rows and its values are the bits ctn_stoi_eval gives for that pair.
// Everything that depends on the reference alone is a constant: frame energies, keep mask, kept-index table, the reference
// envelopes and the clip bound.  A cell that the forward clipped (alpha y > bound, strictly) passes no gradient through alpha y;
// the dependence of alpha on y is differentiated.  A norm that is exactly 0 passes gradient 0.
//   score bwd   one thread per pair and segment: d STOI / d y and d ESTOI / d y of its 15 x 30 cells, scaled by the pair's upstream
//               weights, into a tile of its own; a second kernel sums the (at most 30) tiles over a frame in segment order
//               -> g_env [P][15][MF].
//   bands bwd   per 16 output frames: the compacted windowed frames are rebuilt in LDS and their spectra on bins 7 .. 230 recomputed
//               as in stoi_bands_kernel; g_X = g_env[band] X / env[band] (0 where env = 0); the transposed DFT-matrix product on
//               v_mfma_f64_16x16x4_f64 (A = 16 samples x 4 bins of the cos / sin matrix, B = 4 bins x 16 frames) and the window
//               -> the gradient of every second-pass frame [P][MF][256]; a gather kernel undoes the second-pass overlap-add and the
//               compaction: a 10 kHz sample lies in at most two first-pass frames, a compacted sample in at most two second-pass
//               frames, summed in ascending frame order -> g10 [P][T].
//   adjoint     g_est[b, e, i] = float(sum over c with est_of_ref[b, c] = e, ascending, of sum_t h[(t down) % up, j] g10[b, c, t]),
//               j = i - (t down) / up + W - 1 in [0, 2W), t ascending, fp64 fused multiply-adds: the transpose of the resampler's
//               fp32 tap table.  up = down: the plain sum over c.  Samples at i >= lengths[b] get exactly 0.
// Fixed-order reductions that depend on the pair alone, no atomics, no host read-back, no synchronisation: graph-capturable.
#include "ctn_stoi_common.h"

extern "C" {
int ctn_stoi_frames(const float* ref, const long long* lengths, long long B, int C, long long T, double* energy, int* keep_idx,
                    int* kcount, void* stream);
int ctn_stoi_bands(const float* ref, const float* est, const long long* lengths, const int* keep_idx, const int* kcount,
                   long long B, int C, long long E, long long T, double* env, void* stream);
size_t ctn_stoi_score_workspace(long long B, int C, long long E, long long T);
int ctn_stoi_score(const double* env, const int* kcount, long long B, int C, long long E, long long T, double* d_stoi,
                   double* d_estoi, int* m_out, int* k_out, void* workspace, size_t workspace_bytes, void* stream);
}

namespace {

constexpr int TILE = NBAND * NSEG;            // cells of one segment
constexpr int RS_MAX_TERM = 1 << 20;          // as ctn_resample.hip

__device__ __forceinline__ int clamp_row(int e, int E) { return e < 0 ? 0 : (e >= E ? E - 1 : e); }

// ---- pair rows: est_p[p] = est[b, est_of_ref[b, c]] over t < n_b (zeros beyond), lens_p[p] = n_b; grid (ceil(T / 256), P) --------
__global__ __launch_bounds__(NT) void stoi_pair_rows_kernel(const float* __restrict__ est, const long long* __restrict__ lens,
                                                            const int* __restrict__ est_of_ref, int C, int E, long long T,
                                                            float* __restrict__ est_p, long long* __restrict__ lens_p) {
    const long long p = blockIdx.y, b = p / C;
    const long long n = clamp_len(lens, b, T);
    const int e = clamp_row(est_of_ref[p], E);
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i == 0) lens_p[p] = n;
    if (i < T) est_p[p * T + i] = i < n ? est[(b * E + e) * T + i] : 0.0f;
}

// ---- score backward: grid (chunk of 64 segments, pair), one wave; thread = segment ------------------------------------------------
// tiles [P][nchunk][TILE][SEGT]: cell (k, t) of segment s0 + lane at [(k * NSEG + t) * SEGT + lane].  The ESTOI half first leaves
// the gradient of the row-normalised cells there (a thread reads back only what it wrote itself), the pass over the bands then
// replaces it by the sum of the two measures' gradients.
__global__ __launch_bounds__(SEGT) void stoi_score_bwd_kernel(const double* __restrict__ env, const int* __restrict__ kcount,
                                                              const double* __restrict__ w_stoi, const double* __restrict__ w_estoi,
                                                              int NF, int MF, int nchunk, double clipmul, double* __restrict__ tiles) {
    __shared__ double ex[NBAND][SFR];
    __shared__ double ey[NBAND][SFR];
    const int tid = threadIdx.x, ch = blockIdx.x;
    const long long p = blockIdx.y;
    int K = kcount[p];
    K = K < 0 ? 0 : (K > NF ? NF : K);
    const int M = K > 0 ? K - 1 : 0, S = M - NSEG + 1;
    const int s0 = ch * SEGT;
    if (s0 >= S) return;
    const double* __restrict__ gx = env + (size_t)p * 2 * NBAND * MF;
    const double* __restrict__ gy = gx + (size_t)NBAND * MF;
    for (int i = tid; i < NBAND * SFR; i += SEGT) {
        const int k = i / SFR, f = i % SFR;
        const bool in = s0 + f < M;
        ex[k][f] = in ? gx[(size_t)k * MF + s0 + f] : 0.0;
        ey[k][f] = in ? gy[(size_t)k * MF + s0 + f] : 0.0;
    }
    __syncthreads();
    if (s0 + tid >= S) return;
    const double ws = w_stoi[p] / ((double)S * NBAND), we = w_estoi[p] / ((double)S * NSEG);
    double* __restrict__ tl = tiles + ((size_t)p * nchunk + ch) * TILE * SEGT + tid;
    if (we != 0.0) {
        // the forward's row statistics, then per frame the column normalisation and its backward
        double mx[NBAND], dx[NBAND], my[NBAND], dy[NBAND];
        for (int k = 0; k < NBAND; ++k) {
            double sx = 0.0, sy = 0.0;
            for (int t = 0; t < NSEG; ++t) { sx += ex[k][tid + t]; sy += ey[k][tid + t]; }
            const double mxk = sx / NSEG, myk = sy / NSEG;
            double nx = 0.0, ny = 0.0;
            for (int t = 0; t < NSEG; ++t) {
                const double a = ex[k][tid + t] - mxk, v = ey[k][tid + t] - myk;
                nx = fma(a, a, nx); ny = fma(v, v, ny);
            }
            mx[k] = mxk; dx[k] = 1.0 / (sqrt(nx) + DBL_EPSILON); my[k] = myk; dy[k] = 1.0 / (sqrt(ny) + DBL_EPSILON);
        }
        for (int t = 0; t < NSEG; ++t) {
            double u[NBAND], v[NBAND], su = 0.0, sv = 0.0;
#pragma unroll
            for (int k = 0; k < NBAND; ++k) {
                u[k] = (ex[k][tid + t] - mx[k]) * dx[k];
                v[k] = (ey[k][tid + t] - my[k]) * dy[k];
                su += u[k]; sv += v[k];
            }
            const double mu = su / NBAND, mv = sv / NBAND;
            double qu = 0.0, qv = 0.0;
#pragma unroll
            for (int k = 0; k < NBAND; ++k) {
                u[k] -= mu; v[k] -= mv;
                qu = fma(u[k], u[k], qu); qv = fma(v[k], v[k], qv);
            }
            const double nv = sqrt(qv);
            const double ru = we / (sqrt(qu) + DBL_EPSILON), rv = 1.0 / (nv + DBL_EPSILON);
            // V = v rv, d = sum u ru V: g_V = u ru; g_v = rv g_V - (sum g_V v) rv^2 v / |v|; then the centring
            double a = 0.0;
#pragma unroll
            for (int k = 0; k < NBAND; ++k) { u[k] *= ru; a = fma(u[k], v[k], a); }
            const double coef = nv > 0.0 ? a * rv * rv / nv : 0.0;
            double sg = 0.0;
#pragma unroll
            for (int k = 0; k < NBAND; ++k) { u[k] = rv * u[k] - coef * v[k]; sg += u[k]; }
            const double mg = sg / NBAND;
#pragma unroll
            for (int k = 0; k < NBAND; ++k) tl[(size_t)(k * NSEG + t) * SEGT] = u[k] - mg;
        }
    }
    for (int k = 0; k < NBAND; ++k) {
        double sx = 0.0, sy = 0.0, qx = 0.0, qy = 0.0;
        for (int t = 0; t < NSEG; ++t) {
            const double a = ex[k][tid + t], v = ey[k][tid + t];
            sx += a; sy += v;
            qx = fma(a, a, qx); qy = fma(v, v, qy);
        }
        // ESTOI, the row normalisation r = (y - my) dy backwards: g_z = dy g_r - (sum g_r z) dy^2 z / |z|, then the centring
        const double myk = sy / NSEG;
        double e_dy = 0.0, e_coef = 0.0, e_mean = 0.0;
        if (we != 0.0) {
            double ny = 0.0, sz = 0.0, sg = 0.0, a = 0.0;
            for (int t = 0; t < NSEG; ++t) {
                const double z = ey[k][tid + t] - myk, g = tl[(size_t)(k * NSEG + t) * SEGT];
                ny = fma(z, z, ny); sz += z; sg += g; a = fma(g, z, a);
            }
            const double nz = sqrt(ny);
            e_dy = 1.0 / (nz + DBL_EPSILON);
            e_coef = nz > 0.0 ? a * e_dy * e_dy / nz : 0.0;
            e_mean = (e_dy * sg - e_coef * sz) / NSEG;
        }
        // STOI: p = min(alpha y, bound), v = p - mean p, corr = sum a v / (|v| + eps) with a the normalised centred reference row
        double scale = 0.0, mxk = 0.0, mp = 0.0, rdx = 0.0, rdp = 0.0, c2 = 0.0, mgv = 0.0, dalpha = 0.0, G = 0.0;
        if (ws != 0.0) {
            const double nyq = sqrt(qy), nxq = sqrt(qx);
            scale = nxq / (nyq + DBL_EPSILON);
            mxk = sx / NSEG;
            double sp = 0.0;
            for (int t = 0; t < NSEG; ++t) sp += fmin(ey[k][tid + t] * scale, ex[k][tid + t] * clipmul);
            mp = sp / NSEG;
            double nx = 0.0, np_ = 0.0;
            for (int t = 0; t < NSEG; ++t) {
                const double a = ex[k][tid + t] - mxk;
                const double v = fmin(ey[k][tid + t] * scale, ex[k][tid + t] * clipmul) - mp;
                nx = fma(a, a, nx); np_ = fma(v, v, np_);
            }
            const double nrm = sqrt(np_);
            rdx = 1.0 / (sqrt(nx) + DBL_EPSILON);
            rdp = 1.0 / (nrm + DBL_EPSILON);
            double av = 0.0, sa = 0.0, sv = 0.0;
            for (int t = 0; t < NSEG; ++t) {
                const double a = (ex[k][tid + t] - mxk) * rdx;
                const double v = fmin(ey[k][tid + t] * scale, ex[k][tid + t] * clipmul) - mp;
                av = fma(a, v, av); sa += a; sv += v;
            }
            c2 = nrm > 0.0 ? av * rdp * rdp / nrm : 0.0;
            mgv = (rdp * sa - c2 * sv) / NSEG;
            // through alpha = |x| / (|y| + eps): d alpha / d y_t = dalpha y_t, fed by the unclipped cells
            dalpha = nyq > 0.0 ? -nxq / ((nyq + DBL_EPSILON) * (nyq + DBL_EPSILON) * nyq) : 0.0;
            for (int t = 0; t < NSEG; ++t) {
                const double y = ey[k][tid + t], bound = ex[k][tid + t] * clipmul;
                if (!(y * scale > bound)) {
                    const double a = (ex[k][tid + t] - mxk) * rdx, v = y * scale - mp;
                    G = fma(rdp * a - c2 * v - mgv, y, G);
                }
            }
        }
        for (int t = 0; t < NSEG; ++t) {
            const double x = ex[k][tid + t], y = ey[k][tid + t];
            double g = 0.0;
            if (ws != 0.0) {
                g = dalpha * y * G;
                if (!(y * scale > x * clipmul)) g = fma(scale, rdp * ((x - mxk) * rdx) - c2 * (y * scale - mp) - mgv, g);
                g *= ws;
            }
            if (we != 0.0) g += e_dy * tl[(size_t)(k * NSEG + t) * SEGT] - e_coef * (y - myk) - e_mean;
            tl[(size_t)(k * NSEG + t) * SEGT] = g;
        }
    }
}

// g_env[p][k][m] = the tiles' cells over frame m in segment order; grid (ceil(MF / 256), band, pair)
__global__ __launch_bounds__(NT) void stoi_score_gather_kernel(const double* __restrict__ tiles, const int* __restrict__ kcount,
                                                               int NF, int MF, int nchunk, double* __restrict__ g_env) {
    const int m = blockIdx.x * NT + threadIdx.x, k = blockIdx.y;
    const long long p = blockIdx.z;
    if (m >= MF) return;
    int K = kcount[p];
    K = K < 0 ? 0 : (K > NF ? NF : K);
    const int M = K > 0 ? K - 1 : 0, S = M - NSEG + 1;
    double acc = 0.0;
    if (S >= 1 && m < M) {
        const int lo = m - (NSEG - 1) > 0 ? m - (NSEG - 1) : 0, hi = m < S - 1 ? m : S - 1;
        for (int s = lo; s <= hi; ++s)
            acc += tiles[(((size_t)p * nchunk + (s / SEGT)) * TILE + k * NSEG + (m - s)) * SEGT + (s % SEGT)];
    }
    g_env[((size_t)p * NBAND + k) * MF + m] = acc;
}

// ---- bands backward: grid (tile of 16 output frames, pair) ---------------------------------------------------------------------------
// buf holds the compacted samples z (ZPAD doubles) for the forward product, then, once every wave has its spectra in registers, the
// gradients of the spectra [re | im][NBINS][FT]: a B operand of the transposed product is 64 consecutive doubles (no bank conflict).
__global__ __launch_bounds__(NT) void stoi_bands_bwd_kernel(const float* __restrict__ est_p, const long long* __restrict__ lens,
                                                            const int* __restrict__ keep_idx, const int* __restrict__ kcount,
                                                            const double* __restrict__ env, const double* __restrict__ g_env,
                                                            long long T, int NF, int MF, double* __restrict__ g_frames) {
    __shared__ double win[FL];
    __shared__ double tcos[512];
    __shared__ double tsin[512];
    __shared__ double fac[NBAND + 1][FT];
    __shared__ double buf[2 * NBINS * FT];
    __shared__ int band_of[NBINS];
    static_assert(ZPAD <= 2 * NBINS * FT, "z fits the buffer of the spectra");
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long p = blockIdx.y;
    const int m0 = blockIdx.x * FT;
    int K = kcount[p];
    K = K < 0 ? 0 : (K > NF ? NF : K);
    const int M = K > 0 ? K - 1 : 0;
    if (m0 >= M || M < NSEG) return;                 // a pair without a segment has no gradient: the gather writes its zeros
    const long long n = clamp_len(lens, p, T);
    const float* __restrict__ x = est_p + (size_t)p * T;
    const int* __restrict__ idx = keep_idx + (size_t)p * NF;
    win[tid] = window_at(tid);
    for (int j = tid; j < 512; j += NT) {
        tcos[j] = cospi((double)j / 256.0);
        tsin[j] = sinpi((double)j / 256.0);
    }
    if (tid < NBINS) {
        int k = NBAND;                                // bins 219 .. 230 belong to no band: row NBAND of fac is zero
        for (int q = 0; q < NBAND; ++q)
            if (tid + BIN0 >= BAND_FIRST[q] && tid + BIN0 < BAND_FIRST[q] + BAND_WIDTH[q]) k = q;
        band_of[tid] = k;
    }
    {
        const int f = tid % FT, k = tid / FT;         // 256 threads = 16 rows of fac
        double v = 0.0;
        if (k < NBAND && m0 + f < M) {
            const double e = env[((size_t)p * 2 + 1) * NBAND * MF + (size_t)k * MF + m0 + f];
            if (e != 0.0) v = g_env[((size_t)p * NBAND + k) * MF + m0 + f] / e;
        }
        fac[k][f] = v;
    }
    __syncthreads();                                  // win (read below by other waves than its writers), the twiddles, fac, band_of
    // z as in stoi_bands_kernel
    for (int q = tid; q < ZLEN; q += NT) {
        const int j = m0 + (q >> 7), r = q & (HOP - 1);
        double v = 0.0;
        if (j >= 1 && j - 1 < K) {
            const long long f = idx[j - 1];
            if (f >= 0 && f * HOP + FL <= n) v = win[r + HOP] * (double)x[f * HOP + r + HOP];
        }
        if (j < K) {
            const long long f = idx[j];
            if (f >= 0 && f * HOP + FL <= n) v += win[r] * (double)x[f * HOP + r];
        }
        buf[zpos(q)] = v;
    }
    __syncthreads();
    const int col = lane & 15, kk = lane >> 4;
    double4_t ac[4], as[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ac[i] = {0.0, 0.0, 0.0, 0.0};
        as[i] = {0.0, 0.0, 0.0, 0.0};
        const int bt = w + 4 * i;
        if (bt < NTILE) {
            const int bin = BIN0 + 16 * bt + col;
#pragma unroll 4
            for (int ks = 0; ks < FL / 4; ++ks) {
                const int s = 4 * ks + kk;
                const int t = (bin * s) & 511;
                const double bv = win[s] * buf[zpos(col * HOP + s)];
                ac[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(tcos[t], bv, ac[i], 0, 0, 0);
                as[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(tsin[t], bv, as[i], 0, 0, 0);
            }
        }
    }
    __syncthreads();                                  // every wave has read z: the buffer now takes the spectra's gradients
    double* const gre = buf;
    double* const gim = buf + NBINS * FT;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int bt = w + 4 * i;
        if (bt < NTILE) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int bl = 16 * bt + kk + 4 * r;
                const double f = fac[band_of[bl]][col];
                gre[bl * FT + col] = ac[i][r] * f;
                gim[bl * FT + col] = as[i][r] * f;
            }
        }
    }
    __syncthreads();
    // transposed product: D[sample][frame] = sum_bin cos(bin * sample) g_re[bin][frame] + sin(bin * sample) g_im[bin][frame]
    for (int nt = w; nt < FL / 16; nt += NT / 64) {
        const int smp = 16 * nt + col;                // A row of this lane
        double4_t dc = {0.0, 0.0, 0.0, 0.0}, ds = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int ks = 0; ks < NBINS / 4; ++ks) {
            const int bl = 4 * ks + kk;
            const int t = ((BIN0 + bl) * smp) & 511;
            dc = __builtin_amdgcn_mfma_f64_16x16x4f64(tcos[t], gre[bl * FT + col], dc, 0, 0, 0);
            ds = __builtin_amdgcn_mfma_f64_16x16x4f64(tsin[t], gim[bl * FT + col], ds, 0, 0, 0);
        }
        if (m0 + col < M) {
            double* __restrict__ out = g_frames + ((size_t)p * MF + m0 + col) * FL;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = 16 * nt + kk + 4 * r;
                out[s] = win[s] * (dc[r] + ds[r]);
            }
        }
    }
}

// position of first-pass frame f in the kept-index table (ascending), or -1
__device__ __forceinline__ int kept_rank(const int* __restrict__ idx, int K, int f) {
    int lo = 0, hi = K - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1, v = idx[mid];
        if (v == f) return mid;
        if (v < f) lo = mid + 1; else hi = mid - 1;
    }
    return -1;
}

// g10[p][i]: the first-pass frames over sample i in ascending order, each through its window to the compacted sample, whose
// gradient is that of the (at most two) second-pass frames over it in ascending order.  grid (ceil(T / 256), pair)
__global__ __launch_bounds__(NT) void stoi_frames_bwd_kernel(const double* __restrict__ g_frames, const long long* __restrict__ lens,
                                                             const int* __restrict__ keep_idx, const int* __restrict__ kcount,
                                                             long long T, int NF, int MF, double* __restrict__ g10) {
    const long long p = blockIdx.y, i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= T) return;
    const long long n = clamp_len(lens, p, T);
    const int nf = (int)frames_of(n);
    int K = kcount[p];
    K = K < 0 ? 0 : (K > NF ? NF : K);
    const int M = K > 0 ? K - 1 : 0;
    const int* __restrict__ idx = keep_idx + (size_t)p * NF;
    const double* __restrict__ gf = g_frames + (size_t)p * MF * FL;
    double acc = 0.0;
    if (i < n && M >= NSEG) {
        const int f1 = (int)(i >> 7);
        for (int f = f1 - 1; f <= f1; ++f) {
            if (f < 0 || f >= nf) continue;
            const int j = kept_rank(idx, K, f);
            if (j < 0) continue;
            const int r = (int)(i - (long long)f * HOP);
            const int pos = j * HOP + r, mhi = pos >> 7, mlo = mhi - 1;
            double gz = 0.0;
            if (mlo >= 0 && mlo < M) gz = gf[(size_t)mlo * FL + pos - mlo * HOP];
            if (mhi < M) gz += gf[(size_t)mhi * FL + pos - mhi * HOP];
            acc = fma(window_at(r), gz, acc);
        }
    }
    g10[(size_t)p * T + i] = acc;
}

// ---- the resampler's adjoint and the sum over the references of one estimate: grid (ceil(T / 256), B * E) -----------------------------
__global__ __launch_bounds__(NT) void resample_adjoint_kernel(const double* __restrict__ g10, const int* __restrict__ est_of_ref,
                                                              const long long* __restrict__ lens, int C, int E, long long T,
                                                              long long T10, int up, int down, const float* __restrict__ h, int W,
                                                              float* __restrict__ g_est, double* __restrict__ g_sum) {
    const long long row = blockIdx.y, b = row / E, i = (long long)blockIdx.x * NT + threadIdx.x;
    const int e = (int)(row - b * E);
    if (i >= T) return;
    const long long n = clamp_len(lens, b, T);
    long long n10 = up == down ? n : (n * up + down - 1) / down;
    n10 = n10 > T10 ? T10 : n10;
    double acc = 0.0;
    if (i < n) {
        for (int c = 0; c < C; ++c) {
            if (clamp_row(est_of_ref[b * C + c], E) != e) continue;
            const double* __restrict__ g = g10 + (size_t)(b * C + c) * T10;
            double s = 0.0;
            if (up == down) {
                if (i < n10) s = g[i];
            } else {
                // outputs t with i - W <= (t down) / up <= i + W - 1
                const long long a = (i - W) * up, z = (i + W) * up;
                long long lo = a <= 0 ? 0 : (a + down - 1) / down;
                long long hi = (z + down - 1) / down - 1;
                hi = hi > n10 - 1 ? n10 - 1 : hi;
                for (long long t = lo; t <= hi; ++t) {
                    const long long q = t * down / up;
                    const int ph = (int)(t * down - q * up), j = (int)(i - q) + W - 1;
                    if (j >= 0 && j < 2 * W) s = fma((double)h[(size_t)ph * 2 * W + j], g[t], s);
                }
            }
            acc += s;
        }
    }
    g_est[row * T + i] = (float)acc;
    if (g_sum != nullptr) g_sum[row * T + i] = acc;
}

bool pairs_ok(long long P, long long T) { return P >= 1 && P <= 65535 && T >= 1 && T <= (1LL << 30); }

size_t tiles_bytes(long long P, long long T) { return aligned((size_t)P * seg_chunks(T) * TILE * SEGT * sizeof(double)); }
size_t genv_bytes(long long P, long long T) { return aligned((size_t)P * NBAND * env_frames(T) * sizeof(double)); }
size_t gframes_bytes(long long P, long long T) { return aligned((size_t)P * env_frames(T) * FL * sizeof(double)); }
size_t g10_bytes(long long P, long long T) { return aligned((size_t)P * T * sizeof(double)); }

// the forward's buffers, kept for the backward pass
struct PairsLayout {
    float* est_p; long long* lens_p; double* energy; int* keep_idx; int* kcount; double* env; double* part;
    size_t total;
};

PairsLayout pairs_layout(void* workspace, long long P, long long T) {
    char* w = (char*)workspace;
    PairsLayout l;
    l.est_p = (float*)w;        w += aligned((size_t)P * T * sizeof(float));
    l.lens_p = (long long*)w;   w += aligned((size_t)P * sizeof(long long));
    l.energy = (double*)w;      w += aligned((size_t)P * alloc_frames(T) * sizeof(double));
    l.keep_idx = (int*)w;       w += aligned((size_t)P * alloc_frames(T) * sizeof(int));
    l.kcount = (int*)w;         w += aligned((size_t)P * sizeof(int));
    l.env = (double*)w;         w += aligned((size_t)P * 2 * NBAND * env_frames(T) * sizeof(double));
    l.part = (double*)w;        w += aligned(ctn_stoi_score_workspace(P, 1, 1, T));
    l.total = (size_t)(w - (char*)workspace);
    return l;
}

int launch_score_bwd(const double* env, const int* kcount, const double* w_stoi, const double* w_estoi, long long P, long long T,
                     double* g_env, double* tiles, hipStream_t st) {
    const int nchunk = seg_chunks(T), NF = alloc_frames(T), MF = env_frames(T);
    const double clipmul = 1.0 + pow(10.0, 15.0 / 20.0);
    hipLaunchKernelGGL(stoi_score_bwd_kernel, dim3((unsigned)nchunk, (unsigned)P), dim3(SEGT), 0, st, env, kcount, w_stoi, w_estoi, NF,
                       MF, nchunk, clipmul, tiles);
    CTN_CHECK_LAUNCH("ctn_stoi_score_bwd");
    hipLaunchKernelGGL(stoi_score_gather_kernel, dim3((unsigned)ctn_cdiv(MF, NT), NBAND, (unsigned)P), dim3(NT), 0, st, tiles, kcount,
                       NF, MF, nchunk, g_env);
    CTN_CHECK_LAUNCH("ctn_stoi_score_bwd/gather");
    return CTN_OK;
}

int launch_bands_bwd(const float* est_p, const long long* lens_p, const int* keep_idx, const int* kcount, const double* env,
                     const double* g_env, long long P, long long T, double* g10, double* g_frames, hipStream_t st) {
    const int NF = alloc_frames(T), MF = env_frames(T);
    hipLaunchKernelGGL(stoi_bands_bwd_kernel, dim3((unsigned)ctn_cdiv(MF, FT), (unsigned)P), dim3(NT), 0, st, est_p, lens_p, keep_idx,
                       kcount, env, g_env, T, NF, MF, g_frames);
    CTN_CHECK_LAUNCH("ctn_stoi_bands_bwd");
    hipLaunchKernelGGL(stoi_frames_bwd_kernel, dim3((unsigned)ctn_cdivll(T, NT), (unsigned)P), dim3(NT), 0, st, g_frames, lens_p,
                       keep_idx, kcount, T, NF, MF, g10);
    CTN_CHECK_LAUNCH("ctn_stoi_bands_bwd/frames");
    return CTN_OK;
}

int check_ratio(const char* fn, long long T, long long T10, int up, int down, const float* h, int W) {
    CTN_REQUIRE(up >= 1 && down >= 1 && up <= RS_MAX_TERM && down <= RS_MAX_TERM, "%s: ratio %d / %d (terms in 1 .. 2^20)", fn, up, down);
    if (up == down) {
        CTN_REQUIRE(up == 1 && T10 == T, "%s: equal rates are 1 / 1 with T10 = T, got %d / %d and %lld vs %lld", fn, up, down, T10, T);
        return CTN_OK;
    }
    int a = up, b = down;
    while (b) { const int t = a % b; a = b; b = t; }
    CTN_REQUIRE(a == 1, "%s: ratio %d / %d is not in lowest terms", fn, up, down);
    CTN_REQUIRE(h != nullptr && W >= 1 && W <= (1 << 16), "%s: a filter bank with W = %d taps to either side (1 .. 2^16) is needed", fn, W);
    CTN_REQUIRE(T10 == (T * up + down - 1) / down, "%s: T10 = %lld, ceil(%lld * %d / %d) expected", fn, T10, T, up, down);
    return CTN_OK;
}

int launch_adjoint(const double* g10, const int* est_of_ref, const long long* lengths, long long B, int C, int E, long long T,
                   long long T10, int up, int down, const float* h, int W, float* g_est, double* g_sum, hipStream_t st) {
    hipLaunchKernelGGL(resample_adjoint_kernel, dim3((unsigned)ctn_cdivll(T, NT), (unsigned)(B * E)), dim3(NT), 0, st, g10, est_of_ref,
                       lengths, C, E, T, T10, up, down, h, W, g_est, g_sum);
    CTN_CHECK_LAUNCH("ctn_resample_rows_adjoint_f64");
    return CTN_OK;
}

#define PAIRS_CHECK_SIZES(fn, B, C, E, T)                                                                                          \
    CTN_REQUIRE((B) >= 1 && (C) >= 1 && (C) <= 64 && (long long)(B) * (C) <= 65535, fn ": B = %lld, C = %d (B * C in 1..65535, C <= 64)", \
                (long long)(B), (int)(C));                                                                                         \
    CTN_REQUIRE((E) >= 1 && (long long)(B) * (E) <= 65535, fn ": E = %lld (B * E in 1..65535)", (long long)(E));                    \
    CTN_REQUIRE((T) >= 1 && (T) <= (1LL << 30), fn ": T = %lld outside 1..2^30", (long long)(T))

}  // namespace

extern "C" {

// see include/ctn_hip.h
size_t ctn_stoi_score_bwd_workspace(long long P, long long T) { return pairs_ok(P, T) ? tiles_bytes(P, T) : 0; }

int ctn_stoi_score_bwd(const double* env, const int* kcount, const double* w_stoi, const double* w_estoi, long long P, long long T,
                       double* g_env, void* workspace, size_t workspace_bytes, void* stream) {
    CTN_REQUIRE(env && kcount && w_stoi && w_estoi && g_env, "ctn_stoi_score_bwd: null pointer");
    CTN_REQUIRE(pairs_ok(P, T), "ctn_stoi_score_bwd: P = %lld pairs (1..65535) of T = %lld samples (1..2^30)", P, T);
    if (workspace == nullptr || workspace_bytes < tiles_bytes(P, T)) {
        ctn_set_error("ctn_stoi_score_bwd: workspace too small");
        return CTN_ERR_WORKSPACE;
    }
    return launch_score_bwd(env, kcount, w_stoi, w_estoi, P, T, g_env, (double*)workspace, (hipStream_t)stream);
}

size_t ctn_stoi_bands_bwd_workspace(long long P, long long T) { return pairs_ok(P, T) ? gframes_bytes(P, T) : 0; }

int ctn_stoi_bands_bwd(const float* est_p, const long long* lengths_p, const int* keep_idx, const int* kcount, const double* env,
                       const double* g_env, long long P, long long T, double* g10, void* workspace, size_t workspace_bytes,
                       void* stream) {
    CTN_REQUIRE(est_p && lengths_p && keep_idx && kcount && env && g_env && g10, "ctn_stoi_bands_bwd: null pointer");
    CTN_REQUIRE(pairs_ok(P, T), "ctn_stoi_bands_bwd: P = %lld pairs (1..65535) of T = %lld samples (1..2^30)", P, T);
    if (workspace == nullptr || workspace_bytes < gframes_bytes(P, T)) {
        ctn_set_error("ctn_stoi_bands_bwd: workspace too small");
        return CTN_ERR_WORKSPACE;
    }
    return launch_bands_bwd(est_p, lengths_p, keep_idx, kcount, env, g_env, P, T, g10, (double*)workspace, (hipStream_t)stream);
}

size_t ctn_resample_rows_adjoint_workspace(long long, int, long long, long long) { return 0; }   // the gather needs none

int ctn_resample_rows_adjoint_f64(const double* g10, const int* est_of_ref, const long long* lengths, long long B, int C, long long E,
                                  long long T, long long T10, int up, int down, const float* h, int W, float* g_est, double* g_sum,
                                  void* stream) {
    CTN_REQUIRE(g10 && est_of_ref && lengths && g_est, "ctn_resample_rows_adjoint_f64: null pointer");
    PAIRS_CHECK_SIZES("ctn_resample_rows_adjoint_f64", B, C, E, T);
    CTN_REQUIRE(T10 >= 1 && T10 <= (1LL << 30), "ctn_resample_rows_adjoint_f64: T10 = %lld outside 1..2^30", T10);
    const int rc = check_ratio("ctn_resample_rows_adjoint_f64", T, T10, up, down, h, W);
    if (rc != CTN_OK) return rc;
    return launch_adjoint(g10, est_of_ref, lengths, B, C, (int)E, T, T10, up, down, h, W, g_est, g_sum, (hipStream_t)stream);
}

size_t ctn_stoi_pairs_workspace(long long B, int C, long long T) {
    if (B < 1 || C < 1 || C > 64 || !pairs_ok(B * C, T)) return 0;
    return pairs_layout(nullptr, B * C, T).total;
}

size_t ctn_stoi_pairs_bwd_workspace(long long B, int C, long long T) {
    if (B < 1 || C < 1 || C > 64 || !pairs_ok(B * C, T)) return 0;
    const long long P = B * C;
    return tiles_bytes(P, T) + genv_bytes(P, T) + gframes_bytes(P, T) + g10_bytes(P, T);
}

int ctn_stoi_pairs_fwd(const float* ref, const float* est, const long long* lengths, const int* est_of_ref, long long B, int C,
                       long long E, long long T, double* d_stoi, double* d_estoi, int* m_out, void* workspace,
                       size_t workspace_bytes, void* stream) {
    CTN_REQUIRE(ref && est && lengths && est_of_ref && d_stoi && d_estoi, "ctn_stoi_pairs_fwd: null pointer");
    PAIRS_CHECK_SIZES("ctn_stoi_pairs_fwd", B, C, E, T);
    const long long P = B * C;
    if (workspace == nullptr || workspace_bytes < pairs_layout(nullptr, P, T).total) {
        ctn_set_error("ctn_stoi_pairs_fwd: workspace too small");
        return CTN_ERR_WORKSPACE;
    }
    const PairsLayout l = pairs_layout(workspace, P, T);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(stoi_pair_rows_kernel, dim3((unsigned)ctn_cdivll(T, NT), (unsigned)P), dim3(NT), 0, st, est, lengths, est_of_ref,
                       C, (int)E, T, l.est_p, l.lens_p);
    CTN_CHECK_LAUNCH("ctn_stoi_pairs_fwd/rows");
    // every pair as an utterance of one reference and one estimate: the bits of ctn_stoi_eval for that pair
    int rc = ctn_stoi_frames(ref, l.lens_p, P, 1, T, l.energy, l.keep_idx, l.kcount, stream);
    if (rc == CTN_OK) rc = ctn_stoi_bands(ref, l.est_p, l.lens_p, l.keep_idx, l.kcount, P, 1, 1, T, l.env, stream);
    if (rc == CTN_OK)
        rc = ctn_stoi_score(l.env, l.kcount, P, 1, 1, T, d_stoi, d_estoi, m_out, nullptr, l.part, ctn_stoi_score_workspace(P, 1, 1, T), stream);
    return rc;
}

int ctn_stoi_pairs_bwd(const void* fwd_workspace, size_t fwd_workspace_bytes, const double* w_stoi, const double* w_estoi,
                       const int* est_of_ref, const long long* lengths, long long B, int C, long long E, long long T, long long T10,
                       int up, int down, const float* h, int W, float* g_est, void* workspace, size_t workspace_bytes, void* stream) {
    CTN_REQUIRE(fwd_workspace && w_stoi && w_estoi && est_of_ref && lengths && g_est, "ctn_stoi_pairs_bwd: null pointer");
    PAIRS_CHECK_SIZES("ctn_stoi_pairs_bwd", B, C, E, T);
    CTN_REQUIRE(T10 >= 1 && T10 <= (1LL << 30), "ctn_stoi_pairs_bwd: T10 = %lld outside 1..2^30", T10);
    int rc = check_ratio("ctn_stoi_pairs_bwd", T, T10, up, down, h, W);
    if (rc != CTN_OK) return rc;
    const long long P = B * C;
    if (fwd_workspace_bytes < pairs_layout(nullptr, P, T10).total || workspace == nullptr ||
        workspace_bytes < ctn_stoi_pairs_bwd_workspace(B, C, T10)) {
        ctn_set_error("ctn_stoi_pairs_bwd: workspace too small");
        return CTN_ERR_WORKSPACE;
    }
    const PairsLayout l = pairs_layout(const_cast<void*>(fwd_workspace), P, T10);
    char* w = (char*)workspace;
    double* tiles = (double*)w;     w += tiles_bytes(P, T10);
    double* g_env = (double*)w;     w += genv_bytes(P, T10);
    double* g_frames = (double*)w;  w += gframes_bytes(P, T10);
    double* g10 = (double*)w;
    hipStream_t st = (hipStream_t)stream;
    rc = launch_score_bwd(l.env, l.kcount, w_stoi, w_estoi, P, T10, g_env, tiles, st);
    if (rc == CTN_OK) rc = launch_bands_bwd(l.est_p, l.lens_p, l.keep_idx, l.kcount, l.env, g_env, P, T10, g10, g_frames, st);
    if (rc == CTN_OK) rc = launch_adjoint(g10, est_of_ref, lengths, B, C, (int)E, T, T10, up, down, h, W, g_est, nullptr, st);
    return rc;
}

}  // extern "C"
