// STOI and ESTOI intelligibility scores in fp64, gfx950.
//   C. H. Taal, R. C. Hendriks, R. Heusdens, J. Jensen, "An Algorithm for Intelligibility Prediction of Time-Frequency
//   Weighted Noisy Speech", IEEE TASLP 19(7), 2011 (STOI); J. Jensen, C. H. Taal, "An Algorithm for Predicting the
//   Intelligibility of Speech Masked by Modulated Noise Maskers", IEEE/ACM TASLP 24(11), 2016 (ESTOI); conventions of the
//   authors' MATLAB code and of pystoi.  Input is 10 kHz fp32 (stoi.py resamples with ctn_resample_ragged first).
//
// One utterance b has C references and E estimate rows of length n_b <= T; every estimate is scored against every reference.
//   frames   first-pass frames of 256 samples at hop 128, starts i < n_b - 256 (strict).  Per reference row: the energies
//            20 log10(||w * frame|| + eps), their maximum, the keep mask e > max - 40 and its exclusive scan -> the table of
//            kept frame indices and their count K.  The mask belongs to the reference: an estimate paired with reference c is
//            compacted by c's table.
//   bands    envelope sets per utterance: set c < C = reference c, set C + e*C + c = estimate e under the table of reference c.
//            The compacted signal z[p] = sum of the (at most two) windowed kept frames over sample p is rebuilt in LDS for 16
//            output frames at a time and never written to memory; frame m = w * z[128 m .. 128 m + 256), its 512-point DFT on
//            bins 7 .. 230 as a DFT-matrix product on v_mfma_f64_16x16x4_f64 (A = 16 bins x 4 samples of the cos / sin
//            matrix from an LDS twiddle table, B = 4 samples x 16 frames), |X|^2, the 15 third-octave band sums in bin
//            order and the square root -> env [B][C + E*C][15][MF].  M = K - 1 frames (K >= 1).
//   score    per (b, e, c) and segment of 30 frames one thread: STOI (scale, clip, mean / norm normalise, correlate per
//            band) and ESTOI (normalise along time, then along bands, correlate) from the two envelope sets staged in LDS;
//            64 segments per workgroup summed by a fixed shuffle tree, the workgroups' partials summed in order by the
//            finish kernel -> d.  M < 30 gives 1e-5 for both.
// Every reduction has a fixed order that depends on the utterance alone: it scores bitwise the same in any batch.  Samples at
// t >= n_b are never read.  No host read-back, no synchronisation, no atomics.
#include "ctn_stoi_common.h"

namespace {

// ---- frames: one workgroup of 16 waves per reference row ------------------------------------------------------------------
__global__ __launch_bounds__(NTF) void stoi_frames_kernel(const float* __restrict__ ref, const long long* __restrict__ lens,
                                                         int C, long long T, int NF, double* __restrict__ energy,
                                                         int* __restrict__ keep_idx, int* __restrict__ kcount) {
    __shared__ double win[FL];
    __shared__ double wmax[NTF / 64];
    __shared__ int wcnt[NTF / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long row = blockIdx.x, b = row / C;
    const long long n = clamp_len(lens, b, T);
    const int nf = (int)frames_of(n);
    const float* __restrict__ x = ref + (size_t)row * T;
    double* __restrict__ en = energy + (size_t)row * NF;
    int* __restrict__ idx = keep_idx + (size_t)row * NF;
    if (tid < FL) win[tid] = window_at(tid);
    __syncthreads();
    // one wave per frame: a lane squares four adjacent samples in order, the wave sums by the shuffle tree
    double mx = -INFINITY;
    for (int f = w; f < nf; f += NTF / 64) {
        const float* __restrict__ fr = x + (size_t)f * HOP + 4 * lane;
        double q = 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double v = win[4 * lane + u] * (double)fr[u];
            q = fma(v, v, q);
        }
        q = wave_sum(q);
        const double e = 20.0 * log10(sqrt(q) + DBL_EPSILON);
        if (lane == 0) en[f] = e;
        mx = fmax(mx, e);
    }
    if (lane == 0) wmax[w] = mx;
    __threadfence_block();
    __syncthreads();
    mx = wmax[0];
    for (int k = 1; k < NTF / 64; ++k) mx = fmax(mx, wmax[k]);
    const double thr = mx - 40.0;
    // exclusive scan of the keep mask, 1024 frames at a time
    int base = 0;
    for (int f0 = 0; f0 < nf; f0 += NTF) {
        const int f = f0 + tid;
        const bool keep = f < nf && en[f] > thr;
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        __syncthreads();                       // wcnt of the previous round has been read
        if (lane == 0) wcnt[w] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int k = 0; k < w; ++k) off += wcnt[k];
        if (keep) idx[off + before] = f;
        for (int k = 0; k < NTF / 64; ++k) base += wcnt[k];
    }
    for (int j = base + tid; j < NF; j += NTF) idx[j] = -1;
    for (int f = nf + tid; f < NF; f += NTF) en[f] = 0.0;
    if (tid == 0) kcount[row] = base;
}

// ---- band envelopes: grid (tile of 16 output frames, envelope set, b) ------------------------------------------------------
__global__ __launch_bounds__(NT) void stoi_bands_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                        const long long* __restrict__ lens, const int* __restrict__ keep_idx,
                                                        const int* __restrict__ kcount, int C, int E, long long T, int NF,
                                                        int MF, double* __restrict__ env) {
    __shared__ double win[FL];
    __shared__ double tcos[512];
    __shared__ double tsin[512];
    __shared__ double z[ZPAD];
    __shared__ double pw[FT][NBINS + 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int set = blockIdx.y, nset = C + E * C;
    const long long b = blockIdx.z;
    const int c = set < C ? set : (set - C) % C;
    const int m0 = blockIdx.x * FT;
    int K = kcount[b * C + c];
    K = K < 0 ? 0 : (K > NF ? NF : K);
    const int M = K > 0 ? K - 1 : 0;
    if (m0 >= M) return;
    const long long n = clamp_len(lens, b, T);
    const float* __restrict__ x = set < C ? ref + ((size_t)b * C + set) * T : est + ((size_t)b * E + (set - C) / C) * T;
    const int* __restrict__ idx = keep_idx + ((size_t)b * C + c) * NF;
    win[tid] = window_at(tid);
    for (int j = tid; j < 512; j += NT) {
        tcos[j] = cospi((double)j / 256.0);
        tsin[j] = sinpi((double)j / 256.0);
    }
    __syncthreads();
    // z[p] for p in [128 m0, 128 m0 + 17 * 128): kept frame j - 1 first, then kept frame j = p / 128 (the overlap-add order)
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
        z[zpos(q)] = v;
    }
    __syncthreads();
    // DFT-matrix product: D[bin][frame] = sum_n tw[bin * n mod 512] * (w[n] z[128 frame + n]).  A: lane holds A[l & 15][l >> 4],
    // B: B[l >> 4][l & 15], D: column l & 15, rows (l >> 4) + 4 r.
    const int col = lane & 15, kk = lane >> 4;
    for (int bt = w; bt < NTILE; bt += NT / 64) {
        const int bin = BIN0 + 16 * bt + col;              // A row of this lane
        double4_t ac = {0.0, 0.0, 0.0, 0.0}, as = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int ks = 0; ks < FL / 4; ++ks) {
            const int s = 4 * ks + kk;
            const int t = (bin * s) & 511;
            const double bv = win[s] * z[zpos(col * HOP + s)];
            ac = __builtin_amdgcn_mfma_f64_16x16x4f64(tcos[t], bv, ac, 0, 0, 0);
            as = __builtin_amdgcn_mfma_f64_16x16x4f64(tsin[t], bv, as, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) pw[col][16 * bt + kk + 4 * r] = fma(ac[r], ac[r], as[r] * as[r]);
    }
    __syncthreads();
    if (tid < FT * NBAND) {
        const int f = tid % FT, k = tid / FT;
        if (m0 + f < M) {
            const int first = BAND_FIRST[k] - BIN0, wd = BAND_WIDTH[k];
            double s = 0.0;
            for (int q = 0; q < wd; ++q) s += pw[f][first + q];
            env[(((size_t)b * nset + set) * NBAND + k) * MF + m0 + f] = sqrt(s);
        }
    }
}

// ---- scores: grid (chunk of 64 segments, pair e*C + c, b), one wave ----------------------------------------------------------
__global__ __launch_bounds__(SEGT) void stoi_score_kernel(const double* __restrict__ env, const int* __restrict__ kcount, int C,
                                                          int E, int NF, int MF, int nchunk, double clipmul,
                                                          double* __restrict__ part) {
    __shared__ double ex[NBAND][SFR];
    __shared__ double ey[NBAND][SFR];
    const int tid = threadIdx.x;
    const int ch = blockIdx.x, pair = blockIdx.y, c = pair % C, nset = C + E * C;
    const long long b = blockIdx.z;
    int K = kcount[b * C + c];
    K = K < 0 ? 0 : (K > NF ? NF : K);
    const int M = K > 0 ? K - 1 : 0, S = M - NSEG + 1;
    const int s0 = ch * SEGT;
    if (s0 >= S) return;
    const double* __restrict__ gx = env + ((size_t)b * nset + c) * NBAND * MF;
    const double* __restrict__ gy = env + ((size_t)b * nset + C + pair) * NBAND * MF;
    for (int i = tid; i < NBAND * SFR; i += SEGT) {
        const int k = i / SFR, f = i % SFR;
        const bool in = s0 + f < M;
        ex[k][f] = in ? gx[(size_t)k * MF + s0 + f] : 0.0;
        ey[k][f] = in ? gy[(size_t)k * MF + s0 + f] : 0.0;
    }
    __syncthreads();
    double dst = 0.0, dex = 0.0;
    if (s0 + tid < S) {
        double mx[NBAND], dx[NBAND], my[NBAND], dy[NBAND];          // per band: the means and 1 / (norm + eps) of the centred rows
        for (int k = 0; k < NBAND; ++k) {
            double sx = 0.0, sy = 0.0, qx = 0.0, qy = 0.0;
            for (int t = 0; t < NSEG; ++t) {
                const double a = ex[k][tid + t], v = ey[k][tid + t];
                sx += a; sy += v;
                qx = fma(a, a, qx); qy = fma(v, v, qy);
            }
            // STOI: scale y to x's norm, clip, remove the means, normalise, correlate
            const double scale = sqrt(qx) / (sqrt(qy) + DBL_EPSILON);
            const double mxk = sx / NSEG;
            double sp = 0.0;
            for (int t = 0; t < NSEG; ++t) sp += fmin(ey[k][tid + t] * scale, ex[k][tid + t] * clipmul);
            const double mp = sp / NSEG;
            double nx = 0.0, np_ = 0.0;
            for (int t = 0; t < NSEG; ++t) {
                const double a = ex[k][tid + t] - mxk;
                const double v = fmin(ey[k][tid + t] * scale, ex[k][tid + t] * clipmul) - mp;
                nx = fma(a, a, nx); np_ = fma(v, v, np_);
            }
            // one reciprocal per norm instead of a division per cell (an fp64 division is ~30 instructions)
            const double rdx = 1.0 / (sqrt(nx) + DBL_EPSILON), rdp = 1.0 / (sqrt(np_) + DBL_EPSILON);
            double corr = 0.0;
            for (int t = 0; t < NSEG; ++t) {
                const double a = (ex[k][tid + t] - mxk) * rdx;
                const double v = (fmin(ey[k][tid + t] * scale, ex[k][tid + t] * clipmul) - mp) * rdp;
                corr = fma(a, v, corr);
            }
            dst += corr;
            // ESTOI, along time: the mean and the norm of the centred row of each signal
            const double myk = sy / NSEG;
            double ny = 0.0;
            for (int t = 0; t < NSEG; ++t) { const double v = ey[k][tid + t] - myk; ny = fma(v, v, ny); }
            mx[k] = mxk; dx[k] = rdx; my[k] = myk; dy[k] = 1.0 / (sqrt(ny) + DBL_EPSILON);
        }
        // ESTOI, along bands: per frame the 15 row-normalised values are centred, normalised and correlated
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
            const double ru = 1.0 / (sqrt(qu) + DBL_EPSILON), rv = 1.0 / (sqrt(qv) + DBL_EPSILON);
            double corr = 0.0;
#pragma unroll
            for (int k = 0; k < NBAND; ++k) corr = fma(u[k] * ru, v[k] * rv, corr);
            dex += corr / NSEG;
        }
    }
    dst = wave_sum(dst);
    dex = wave_sum(dex);
    if (tid == 0) {
        double* __restrict__ out = part + (((size_t)b * E * C + pair) * nchunk + ch) * 2;
        out[0] = dst;
        out[1] = dex;
    }
}

// one thread per (b, e, c): chunk partials in order -> d
__global__ __launch_bounds__(NT) void stoi_finish_kernel(const double* __restrict__ part, const int* __restrict__ kcount,
                                                         long long B, int C, int E, int NF, int nchunk,
                                                         double* __restrict__ d_stoi, double* __restrict__ d_estoi,
                                                         int* __restrict__ m_out, int* __restrict__ k_out) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= B * E * C) return;
    const long long b = i / ((long long)E * C);
    const int c = (int)(i % C);
    int K = kcount[b * C + c];
    K = K < 0 ? 0 : (K > NF ? NF : K);
    const int M = K > 0 ? K - 1 : 0, S = M - NSEG + 1;
    double ds = TOO_SHORT, de = TOO_SHORT;
    if (S >= 1) {
        const int nc = (S + SEGT - 1) / SEGT;
        double a = 0.0, e = 0.0;
        for (int ch = 0; ch < nc; ++ch) {
            a += part[((size_t)i * nchunk + ch) * 2];
            e += part[((size_t)i * nchunk + ch) * 2 + 1];
        }
        ds = a / ((double)S * NBAND);
        de = e / (double)S;
    }
    d_stoi[i] = ds;
    d_estoi[i] = de;
    if (m_out != nullptr) m_out[i] = M;
    if (k_out != nullptr) k_out[i] = K;
}

#define STOI_CHECK_SIZES(fn, B, C, E, T)                                                                                \
    CTN_REQUIRE((B) >= 1 && (B) <= 65535, fn ": B = %lld outside 1..65535", (long long)(B));                              \
    CTN_REQUIRE((C) >= 1 && (C) <= 64, fn ": C = %d outside 1..64", (int)(C));                                            \
    CTN_REQUIRE((E) >= 1 && (long long)(C) * ((E) + 1) <= 65535, fn ": E = %lld outside 1..%d", (long long)(E),           \
                65535 / (int)(C) - 1);                                                                                    \
    CTN_REQUIRE((T) >= 1 && (T) <= (1LL << 30), fn ": T = %lld outside 1..2^30", (long long)(T))

int launch_frames(const float* ref, const long long* lengths, long long B, int C, long long T, double* energy, int* keep_idx,
                  int* kcount, hipStream_t st) {
    hipLaunchKernelGGL(stoi_frames_kernel, dim3((unsigned)(B * C)), dim3(NTF), 0, st, ref, lengths, C, T, alloc_frames(T), energy,
                       keep_idx, kcount);
    CTN_CHECK_LAUNCH("ctn_stoi_frames");
    return CTN_OK;
}

int launch_bands(const float* ref, const float* est, const long long* lengths, const int* keep_idx, const int* kcount,
                 long long B, int C, int E, long long T, double* env, hipStream_t st) {
    const int MF = env_frames(T);
    hipLaunchKernelGGL(stoi_bands_kernel, dim3((unsigned)ctn_cdiv(MF, FT), (unsigned)(C + E * C), (unsigned)B), dim3(NT), 0, st,
                       ref, est, lengths, keep_idx, kcount, C, E, T, alloc_frames(T), MF, env);
    CTN_CHECK_LAUNCH("ctn_stoi_bands");
    return CTN_OK;
}

int launch_score(const double* env, const int* kcount, long long B, int C, int E, long long T, double* d_stoi, double* d_estoi,
                 int* m_out, int* k_out, double* part, hipStream_t st) {
    const int nchunk = seg_chunks(T);
    const double clipmul = 1.0 + pow(10.0, 15.0 / 20.0);          // 1 + 10^(-beta / 20), beta = -15 dB
    hipLaunchKernelGGL(stoi_score_kernel, dim3((unsigned)nchunk, (unsigned)(E * C), (unsigned)B), dim3(SEGT), 0, st, env, kcount,
                       C, E, alloc_frames(T), env_frames(T), nchunk, clipmul, part);
    CTN_CHECK_LAUNCH("ctn_stoi_score");
    hipLaunchKernelGGL(stoi_finish_kernel, dim3((unsigned)ctn_cdivll(B * E * C, NT)), dim3(NT), 0, st, part, kcount, B, C, E,
                       alloc_frames(T), nchunk, d_stoi, d_estoi, m_out, k_out);
    CTN_CHECK_LAUNCH("ctn_stoi_score/finish");
    return CTN_OK;
}

size_t energy_bytes(long long B, int C, long long T) { return aligned((size_t)B * C * alloc_frames(T) * sizeof(double)); }
size_t index_bytes(long long B, int C, long long T) { return aligned((size_t)B * C * alloc_frames(T) * sizeof(int)); }
size_t count_bytes(long long B, int C) { return aligned((size_t)B * C * sizeof(int)); }
size_t env_bytes(long long B, int C, long long E, long long T) {
    return aligned((size_t)B * (C + E * C) * NBAND * env_frames(T) * sizeof(double));
}
size_t part_bytes(long long B, int C, long long E, long long T) { return aligned((size_t)B * E * C * seg_chunks(T) * 2 * sizeof(double)); }

bool sizes_ok(long long B, int C, long long E, long long T) {
    return B >= 1 && B <= 65535 && C >= 1 && C <= 64 && E >= 1 && (long long)C * (E + 1) <= 65535 && T >= 1 && T <= (1LL << 30);
}

}  // namespace

extern "C" {

// see include/ctn_hip.h
int ctn_stoi_max_frames(long long T) {
    if (T < 1 || T > (1LL << 30)) return 0;
    return alloc_frames(T);
}

size_t ctn_stoi_score_workspace(long long B, int C, long long E, long long T) {
    if (!sizes_ok(B, C, E, T)) return 0;
    return part_bytes(B, C, E, T);
}

size_t ctn_stoi_workspace(long long B, int C, long long E, long long T) {
    if (!sizes_ok(B, C, E, T)) return 0;
    return energy_bytes(B, C, T) + index_bytes(B, C, T) + count_bytes(B, C) + env_bytes(B, C, E, T) + part_bytes(B, C, E, T);
}

int ctn_stoi_frames(const float* ref, const long long* lengths, long long B, int C, long long T, double* energy, int* keep_idx,
                    int* kcount, void* stream) {
    CTN_REQUIRE(ref && lengths && energy && keep_idx && kcount, "ctn_stoi_frames: null pointer");
    STOI_CHECK_SIZES("ctn_stoi_frames", B, C, 1, T);
    return launch_frames(ref, lengths, B, C, T, energy, keep_idx, kcount, (hipStream_t)stream);
}

int ctn_stoi_bands(const float* ref, const float* est, const long long* lengths, const int* keep_idx, const int* kcount,
                   long long B, int C, long long E, long long T, double* env, void* stream) {
    CTN_REQUIRE(ref && est && lengths && keep_idx && kcount && env, "ctn_stoi_bands: null pointer");
    STOI_CHECK_SIZES("ctn_stoi_bands", B, C, E, T);
    return launch_bands(ref, est, lengths, keep_idx, kcount, B, C, (int)E, T, env, (hipStream_t)stream);
}

int ctn_stoi_score(const double* env, const int* kcount, long long B, int C, long long E, long long T, double* d_stoi,
                   double* d_estoi, int* m_out, int* k_out, void* workspace, size_t workspace_bytes, void* stream) {
    CTN_REQUIRE(env && kcount && d_stoi && d_estoi, "ctn_stoi_score: null pointer");
    STOI_CHECK_SIZES("ctn_stoi_score", B, C, E, T);
    if (workspace == nullptr || workspace_bytes < part_bytes(B, C, E, T)) {
        ctn_set_error("ctn_stoi_score: workspace too small");
        return CTN_ERR_WORKSPACE;
    }
    return launch_score(env, kcount, B, C, (int)E, T, d_stoi, d_estoi, m_out, k_out, (double*)workspace, (hipStream_t)stream);
}

int ctn_stoi_eval(const float* ref, const float* est, const long long* lengths, long long B, int C, long long E, long long T,
                  double* d_stoi, double* d_estoi, int* m_out, int* k_out, void* workspace, size_t workspace_bytes,
                  void* stream) {
    CTN_REQUIRE(ref && est && lengths && d_stoi && d_estoi, "ctn_stoi_eval: null pointer");
    STOI_CHECK_SIZES("ctn_stoi_eval", B, C, E, T);
    if (workspace == nullptr || workspace_bytes < ctn_stoi_workspace(B, C, E, T)) {
        ctn_set_error("ctn_stoi_eval: workspace too small");
        return CTN_ERR_WORKSPACE;
    }
    char* w = (char*)workspace;
    double* energy = (double*)w;   w += energy_bytes(B, C, T);
    int* keep_idx = (int*)w;       w += index_bytes(B, C, T);
    int* kcount = (int*)w;         w += count_bytes(B, C);
    double* env = (double*)w;      w += env_bytes(B, C, E, T);
    double* part = (double*)w;
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_frames(ref, lengths, B, C, T, energy, keep_idx, kcount, st);
    if (rc == CTN_OK) rc = launch_bands(ref, est, lengths, keep_idx, kcount, B, C, (int)E, T, env, st);
    if (rc == CTN_OK) rc = launch_score(env, kcount, B, C, (int)E, T, d_stoi, d_estoi, m_out, k_out, part, st);
    return rc;
}

}  // extern "C"
