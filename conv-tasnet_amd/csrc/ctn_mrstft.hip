// Multi-resolution STFT loss in fp64, gfx950: spectral convergence, log-magnitude and linear-magnitude distance of chosen
// (reference, estimate) pairs over up to 8 analysis resolutions, and the gradient with respect to the estimate's samples
// (Yamamoto et al., "Parallel WaveGAN", ICASSP 2020; auraloss MultiResolutionSTFTLoss).  See include/ctn_hip.h for the definition.
//
// The transform is a decimation-in-frequency FFT in LDS.  A workgroup of 256 threads holds SLAB = 2048 complex points, i.e.
// 2048 / n_fft frames of one (pair, resolution) side by side, so a stage is 1024 butterflies whatever n_fft is.  A frame's
// complex input is (windowed reference) + i (windowed estimate): one transform gives both real spectra,
//     S[k] = (Z[k] + conj Z[N-k]) / 2,   S^[k] = (Z[k] - conj Z[N-k]) / 2i,
// which is the arithmetic of two N/2-point complex transforms.  The output stays in bit-reversed order: the bin loop reads it
// through __brev, so there is no reordering pass.
//   stages       three stages at a time in registers: a thread loads the 8 points d0 + s q (q the smallest half-span of the three)
//                that the stages close over, does the 12 butterflies and stores them back: log2 N = 6 .. 11 stages cost 2 .. 4 LDS
//                round trips.  The one or two stages left over run first as a radix-2 or radix-4 pass.
//   LDS layout   re[] and im[] apart, point d at d + (d >> 5): one double of padding per 32.  A ds_read_b64 is served in two groups
//                of 32 lanes over 64 four-byte banks, so the 32 doubles of a group must differ mod 32.  q >= 64: a group reads 32
//                consecutive points.  q = 1: every eighth point, which the padding spreads over all banks.  q = 8: a group takes
//                8 offsets of every fourth 64-point block, whose padded starts lie 8 banks apart.  Conflict-free reads in every
//                pass; the 8-byte stores (groups of 16 lanes) are at worst 2-way.
//   twiddles     one fp64 table of 2048 entries, entry h + o = exp(-i pi o / h) for h = 1, 2, .. 1024: a stage reads it with unit
//                stride and the same table serves every n_fft.  Built on the device by the first launch of a forward call into the
//                caller's workspace together with the zero-padded Hann windows; there is no sincos in a butterfly.
//   forward      gather (reflect padding about the utterance's own ends, window) -> FFT -> per frame the four sums of the
//                definition by a fixed tree over the frame's threads -> part [P][frames][4]; a second kernel sums a cell's frames
//                in a fixed order -> terms [P][R][3] and the cell's (D, A) for the backward pass.  No spectrogram goes to memory.
//   backward     the frame's spectra are recomputed; G[k] = dL/d|S^| S^/|S^| per bin; its Hermitian extension H goes back into LDS
//                and the same FFT on conj H gives the real time-domain gradient (Re FFT(conj H) = sum_k H[k] e^{+2 pi i k m / N});
//                times the window -> gframes [P][frames][win_length] fp64.  A gather kernel then gives every sample t < n of an
//                estimate row the sum of the frames that cover it and of the frames that cover its mirror images in the reflect
//                padding, over the references that chose the row and the resolutions, in a fixed order in fp64, rounded once.
// Fixed-order reductions that depend on the pair alone, no atomics, no host read-back, no synchronisation: graph-capturable.
#include "ctn_common.h"
#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int SLAB = 2048;                    // complex points per workgroup = the largest n_fft
constexpr int LOG_SLAB = 11;
constexpr int LDSN = SLAB + SLAB / 32;        // with one double of padding per 32
constexpr int MAX_RES = 8;
constexpr int MIN_FFT = 64;
constexpr int MAX_COVER = 64;                 // frames over one sample: ceil(win_length / hop)
constexpr long long MAX_T = 1LL << 24;
constexpr size_t ALIGN = 256;

struct ResTab {
    int R;
    int nfft[MAX_RES], logn[MAX_RES], hop[MAX_RES], win[MAX_RES], off[MAX_RES];
    long long foff[MAX_RES];                  // first frame slot of resolution r within a pair's FT slots
    long long goff[MAX_RES];                  // first double of resolution r within a pair's GT doubles of frame gradients
    long long FT, GT;
    int maxpass;                              // the largest number of workgroups along x that a resolution needs
};

struct FwdLayout {
    double2* tw;       // [SLAB]
    double* wtab;      // [R][SLAB]
    double* part;      // [P][FT][4]
    double* sums;      // [P][R][4]: D, A, sum |log|, sum |lin|
    size_t total;
};

inline size_t aligned(size_t bytes) { return (bytes + ALIGN - 1) / ALIGN * ALIGN; }

FwdLayout fwd_layout(void* base, long long P, const ResTab& t) {
    FwdLayout l;
    char* w = (char*)base;
    size_t o = 0;
    l.tw = (double2*)(w + o);    o += aligned(sizeof(double2) * SLAB);
    l.wtab = (double*)(w + o);   o += aligned(sizeof(double) * SLAB * t.R);
    l.part = (double*)(w + o);   o += aligned(sizeof(double) * 4 * (size_t)P * (size_t)t.FT);
    l.sums = (double*)(w + o);   o += aligned(sizeof(double) * 4 * (size_t)P * t.R);
    l.total = o;
    return l;
}

// -> false with `why` set: a resolution outside the accepted set
bool make_tab(int R, const int* res, long long T, ResTab& t, const char** why) {
    if (R < 1 || R > MAX_RES) { *why = "1 .. 8 resolutions"; return false; }
    t.R = R;
    t.FT = t.GT = 0;
    t.maxpass = 1;
    for (int r = 0; r < R; ++r) {
        const int N = res[3 * r], hop = res[3 * r + 1], win = res[3 * r + 2];
        if (N < MIN_FFT || N > SLAB || (N & (N - 1)) != 0) { *why = "n_fft must be a power of two in 64 .. 2048"; return false; }
        if (win < 1 || win > N) { *why = "1 <= win_length <= n_fft"; return false; }
        if (hop < 1 || (win + hop - 1) / hop > MAX_COVER) { *why = "1 <= hop and ceil(win_length / hop) <= 64"; return false; }
        int lg = 0;
        while ((1 << lg) < N) ++lg;
        t.nfft[r] = N; t.logn[r] = lg; t.hop[r] = hop; t.win[r] = win; t.off[r] = (N - win) / 2;
        const long long maxf = 1 + T / hop;
        t.foff[r] = t.FT; t.FT += maxf;
        t.goff[r] = t.GT; t.GT += maxf * win;
        const long long pass = (maxf + (SLAB / N) - 1) / (SLAB / N);
        if (pass > t.maxpass) t.maxpass = (int)pass;
    }
    return true;
}

__device__ __forceinline__ int pos(int d) { return d + (d >> 5); }
__device__ __forceinline__ int clamp_row(int e, int E) { return e < 0 ? 0 : (e >= E ? E - 1 : e); }
__device__ __forceinline__ long long clamp_len(const long long* lens, long long b, long long T) {
    const long long n = lens[b];
    return n < 0 ? 0 : (n > T ? T : n);
}
__device__ __forceinline__ int brev_n(int k, int logn) { return (int)(__brev((unsigned)k) >> (32 - logn)); }

// ---- tables: block 0 the twiddles, block 1 + r the window of resolution r zero-padded to n_fft ------------------------------------
__global__ __launch_bounds__(NT) void mrstft_tables_kernel(ResTab t, double2* __restrict__ tw, double* __restrict__ wtab) {
    const int blk = blockIdx.x;
    if (blk == 0) {
        for (int i = threadIdx.x; i < SLAB; i += NT) {
            double s = 0.0, c = 1.0;
            if (i > 0) {
                const int h = 1 << (31 - __clz(i));
                sincospi((double)(i - h) / (double)h, &s, &c);
            }
            tw[i] = make_double2(c, -s);
        }
        return;
    }
    const int r = blk - 1, win = t.win[r], off = t.off[r];
    for (int m = threadIdx.x; m < SLAB; m += NT) {
        const int j = m - off;
        wtab[(size_t)r * SLAB + m] = (j >= 0 && j < win) ? 0.5 - 0.5 * cospi(2.0 * (double)j / (double)win) : 0.0;
    }
}

// ---- the frames f0 .. f0 + SLAB / N - 1 of one row pair, windowed, into LDS: re = reference, im = estimate ------------------------
__device__ __forceinline__ void load_frames(double* __restrict__ re, double* __restrict__ im, const float* __restrict__ x,
                                            const float* __restrict__ y, long long n, int N, int logn, int hop, long long f0,
                                            long long F, const double* __restrict__ w, int win, int off) {
#pragma unroll
    for (int q = 0; q < SLAB / NT; ++q) {
        const int d = threadIdx.x + q * NT, m = d & (N - 1);
        const long long f = f0 + (d >> logn);
        double xr = 0.0, xi = 0.0;
        if (f < F && m >= off && m < off + win) {              // the taps under the window: the three loads depend on no other
            long long j = f * hop + m - (N >> 1);              // reflect about samples 0 and n - 1: n > N / 2, one fold suffices
            j = j < 0 ? -j : (j >= n ? 2 * (n - 1) - j : j);
            const double wm = w[m];
            xr = wm * (double)x[j];
            xi = wm * (double)y[j];
        }
        re[pos(d)] = xr;
        im[pos(d)] = xi;
    }
    __syncthreads();
}

// ---- SLAB / N transforms of N points side by side, in place, natural order in, bit-reversed order out ----------------------------
// One butterfly of half-span h at offset o within its half: (a, b) -> (a + b, (a - b) exp(-i pi o / h)).
__device__ __forceinline__ void butterfly(double& ar, double& ai, double& br, double& bi, const double2 w) {
    const double dr = ar - br, di = ai - bi;
    ar += br;
    ai += bi;
    br = dr * w.x - di * w.y;
    bi = dr * w.y + di * w.x;
}

// K consecutive stages (half-spans h, h / 2, .. q = h >> (K - 1)) on the 2^K points d0 + s q that they close over, in registers:
// one LDS round trip per K stages.  A thread takes 8 >> K such units.
template <int K>
__device__ __forceinline__ void fft_pass(double* __restrict__ re, double* __restrict__ im, int h, const double2* __restrict__ tw) {
    constexpr int PTS = 1 << K;
    const int q = h >> (K - 1), lq = 31 - __clz(q);
#pragma unroll
    for (int j = 0; j < (8 >> K); ++j) {
        const int u = threadIdx.x + j * NT;
        int o, d0;
        if (K < 3 || q >= 64 || q == 1) {                      // a lane group reads 32 consecutive points, or every eighth one
            o = u & (q - 1);
            d0 = ((u - o) << K) + o;
        } else {                                               // blocks of 8 q points, 32 / q of them per lane group: every fourth
            const int g = u >> 5, l = u & 31;                  // block, whose padded starts lie q banks apart
            o = l & (q - 1);
            d0 = ((((g >> 2) << 2) << (5 - lq)) + (g & 3) + ((l >> lq) << 2)) * (q << 3) + o;
        }
        double xr[PTS], xi[PTS];
#pragma unroll
        for (int s = 0; s < PTS; ++s) {
            const int p = pos(d0 + s * q);
            xr[s] = re[p];
            xi[s] = im[p];
        }
        if (K == 3) {
#pragma unroll
            for (int s = 0; s < 4; ++s) butterfly(xr[s], xi[s], xr[s + 4], xi[s + 4], tw[h + o + s * q]);
            const double2 w0 = tw[(h >> 1) + o], w1 = tw[(h >> 1) + o + q];
            butterfly(xr[0], xi[0], xr[2], xi[2], w0);
            butterfly(xr[1], xi[1], xr[3], xi[3], w1);
            butterfly(xr[4], xi[4], xr[6], xi[6], w0);
            butterfly(xr[5], xi[5], xr[7], xi[7], w1);
        } else if (K == 2) {
            butterfly(xr[0], xi[0], xr[2], xi[2], tw[h + o]);
            butterfly(xr[1], xi[1], xr[3], xi[3], tw[h + o + q]);
        }
        const double2 wq = tw[q + o];
#pragma unroll
        for (int s = 0; s < PTS; s += 2) butterfly(xr[s], xi[s], xr[s + 1], xi[s + 1], wq);
#pragma unroll
        for (int s = 0; s < PTS; ++s) {
            const int p = pos(d0 + s * q);
            re[p] = xr[s];
            im[p] = xi[s];
        }
    }
    __syncthreads();
}

// log2 N = 6 .. 11 stages as radix-8 passes, the one or two stages left over first, where the spans are widest.  The radix-8 passes
// then fall on quarter-spans q = 64, 8 and 1 only.
__device__ __forceinline__ void fft_slab(double* __restrict__ re, double* __restrict__ im, int N, int logn,
                                         const double2* __restrict__ tw) {
    int h = N >> 1;
    const int rem = logn % 3;
    if (rem == 1) {
        fft_pass<1>(re, im, h, tw);
        h >>= 1;
    } else if (rem == 2) {
        fft_pass<2>(re, im, h, tw);
        h >>= 2;
    }
    for (; h >= 4; h >>= 3) fft_pass<3>(re, im, h, tw);
}

// the two spectra of bin k of the frame at LDS base `base` from the packed transform
__device__ __forceinline__ void bin_spectra(const double* __restrict__ re, const double* __restrict__ im, int base, int k, int N,
                                            int logn, double& sr, double& si, double& er, double& ei) {
    const int pk = pos(base + brev_n(k, logn)), pn = pos(base + brev_n((N - k) & (N - 1), logn));
    const double zr = re[pk], zi = im[pk], nr = re[pn], ni = im[pn];
    sr = 0.5 * (zr + nr); si = 0.5 * (zi - ni);
    er = 0.5 * (zi + ni); ei = 0.5 * (nr - zr);
}

// ---- forward: grid (pass, R, P) -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void mrstft_fwd_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                        const long long* __restrict__ lens, const int* __restrict__ est_of_ref,
                                                        int C, int E, long long T, ResTab t, double eps,
                                                        const double2* __restrict__ tw, const double* __restrict__ wtab,
                                                        double* __restrict__ part) {
    __shared__ double re[LDSN];
    __shared__ double im[LDSN];
    const int r = blockIdx.y, tid = threadIdx.x;
    const long long p = blockIdx.z, b = p / C;
    const int N = t.nfft[r], logn = t.logn[r], hop = t.hop[r];
    const long long n = clamp_len(lens, b, T);
    if (n <= (N >> 1)) return;
    const long long F = 1 + n / hop, f0 = (long long)blockIdx.x << (LOG_SLAB - logn);
    if (f0 >= F) return;
    const float* __restrict__ x = ref + (size_t)p * T;
    const float* __restrict__ y = est + ((size_t)b * E + clamp_row(est_of_ref[p], E)) * T;
    load_frames(re, im, x, y, n, N, logn, hop, f0, F, wtab + (size_t)r * SLAB, t.win[r], t.off[r]);
    fft_slab(re, im, N, logn, tw);
    const int tpf = N >> 3, g = tid >> (logn - 3), lt = tid & (tpf - 1);       // N / 8 threads per frame
    const long long f = f0 + g;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (f < F) {
        for (int k = lt; k <= (N >> 1); k += tpf) {
            double sr, si, er, ei;
            bin_spectra(re, im, g << logn, k, N, logn, sr, si, er, ei);
            const double ps = fmax(sr * sr + si * si, eps), pe = fmax(er * er + ei * ei, eps);
            const double ms = sqrt(ps), me = sqrt(pe), d = ms - me;
            a0 = fma(d, d, a0);
            a1 += ps;
            a2 += fabs(0.5 * log(ps) - 0.5 * log(pe));
            a3 += fabs(d);
        }
    }
    __syncthreads();                                           // the spectra are consumed: re[] becomes the reduction's scratch
    re[tid] = a0; re[NT + tid] = a1; re[2 * NT + tid] = a2; re[3 * NT + tid] = a3;
    __syncthreads();
    for (int s = tpf >> 1; s >= 1; s >>= 1) {
        if (lt < s) {
#pragma unroll
            for (int q = 0; q < 4; ++q) re[q * NT + tid] += re[q * NT + tid + s];
        }
        __syncthreads();
    }
    if (lt == 0 && f < F) {
        double* __restrict__ o = part + ((size_t)p * t.FT + t.foff[r] + f) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = re[q * NT + tid];
    }
}

// ---- a cell's frames in a fixed order: grid (R, P) --------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void mrstft_terms_kernel(const double* __restrict__ part, const long long* __restrict__ lens, int C,
                                                          long long T, ResTab t, double* __restrict__ terms,
                                                          double* __restrict__ sums) {
    __shared__ double scratch[NT / 64];
    const int r = blockIdx.x, tid = threadIdx.x;
    const long long p = blockIdx.y, n = clamp_len(lens, p / C, T);
    const int N = t.nfft[r];
    const long long F = n > (N >> 1) ? 1 + n / t.hop[r] : 0;
    const double* __restrict__ in = part + ((size_t)p * t.FT + t.foff[r]) * 4;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long f = tid; f < F; f += NT) {
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] += in[f * 4 + q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] = block_sum<double, NT>(s[q], scratch);
    if (tid == 0) {
        const double M = (double)F * (double)((N >> 1) + 1);
        double* __restrict__ o = terms + ((size_t)p * t.R + r) * 3;
        o[0] = (F > 0 && s[0] > 0.0) ? sqrt(s[0]) / sqrt(s[1]) : 0.0;
        o[1] = F > 0 ? s[2] / M : 0.0;
        o[2] = F > 0 ? s[3] / M : 0.0;
        double* __restrict__ k = sums + ((size_t)p * t.R + r) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) k[q] = s[q];
    }
}

// ---- backward, frames: grid (pass, R, P) -> gframes [P][GT] -----------------------------------------------------------------------
__global__ __launch_bounds__(NT) void mrstft_bwd_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                        const long long* __restrict__ lens, const int* __restrict__ est_of_ref,
                                                        int C, int E, long long T, ResTab t, double eps,
                                                        const double2* __restrict__ tw, const double* __restrict__ wtab,
                                                        const double* __restrict__ sums, const double* __restrict__ g_terms,
                                                        double* __restrict__ gframes) {
    __shared__ double re[LDSN];
    __shared__ double im[LDSN];
    const int r = blockIdx.y, tid = threadIdx.x;
    const long long p = blockIdx.z, b = p / C;
    const int N = t.nfft[r], logn = t.logn[r], hop = t.hop[r], win = t.win[r], off = t.off[r];
    const long long n = clamp_len(lens, b, T);
    if (n <= (N >> 1)) return;
    const long long F = 1 + n / hop, f0 = (long long)blockIdx.x << (LOG_SLAB - logn);
    if (f0 >= F) return;
    const float* __restrict__ x = ref + (size_t)p * T;
    const float* __restrict__ y = est + ((size_t)b * E + clamp_row(est_of_ref[p], E)) * T;
    const double* __restrict__ w = wtab + (size_t)r * SLAB;
    load_frames(re, im, x, y, n, N, logn, hop, f0, F, w, win, off);
    fft_slab(re, im, N, logn, tw);
    // d loss / d |S^| of a bin = c_sc (|S^| - |S|) + sign(|S^| - |S|) (c_log / |S^| + c_lin)
    const double D = sums[((size_t)p * t.R + r) * 4], A = sums[((size_t)p * t.R + r) * 4 + 1];
    const double invM = 1.0 / ((double)F * (double)((N >> 1) + 1));
    const double* __restrict__ gt = g_terms + ((size_t)p * t.R + r) * 3;
    const double c_sc = D > 0.0 ? gt[0] / (sqrt(D) * sqrt(A)) : 0.0, c_log = gt[1] * invM, c_lin = gt[2] * invM;
    const int tpf = N >> 3, g = tid >> (logn - 3), lt = tid & (tpf - 1), base = g << logn;
    const bool live = f0 + g < F;
    double hr[5], hi[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int k = lt + i * tpf;
        hr[i] = hi[i] = 0.0;
        if (live && k <= (N >> 1)) {
            double sr, si, er, ei;
            bin_spectra(re, im, base, k, N, logn, sr, si, er, ei);
            const double pe = er * er + ei * ei;
            if (pe >= eps) {                                   // a clamped bin passes no gradient
                const double ms = sqrt(fmax(sr * sr + si * si, eps)), me = sqrt(pe), d = me - ms;
                const double sg = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
                const double c = (c_sc * d + sg * (c_log / me + c_lin)) / me;
                hr[i] = c * er;
                hi[i] = c * ei;
            }
        }
    }
    __syncthreads();
    // conj H in natural order: H[k] = G[k] / 2, H[N - k] = conj G[k] / 2 for 0 < k < N / 2; H[0] = Re G[0], H[N/2] = Re G[N/2]
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int k = lt + i * tpf;
        if (k <= (N >> 1)) {
            if (k == 0 || k == (N >> 1)) {
                re[pos(base + k)] = hr[i];
                im[pos(base + k)] = 0.0;
            } else {
                re[pos(base + k)] = 0.5 * hr[i];
                im[pos(base + k)] = -0.5 * hi[i];
                re[pos(base + N - k)] = 0.5 * hr[i];
                im[pos(base + N - k)] = 0.5 * hi[i];
            }
        }
    }
    __syncthreads();
    fft_slab(re, im, N, logn, tw);
    double* __restrict__ out = gframes + (size_t)p * t.GT + t.goff[r];
#pragma unroll
    for (int q = 0; q < SLAB / NT; ++q) {
        const int d = tid + q * NT, m = d & (N - 1), j = m - off;
        const long long f = f0 + (d >> logn);
        if (f < F && j >= 0 && j < win) out[f * win + j] = w[m] * re[pos((d - m) + brev_n(m, logn))];
    }
}

// the frames of one resolution over padded position i, ascending
__device__ __forceinline__ double cover_sum(const double* __restrict__ gf, long long i, int hop, int win, int off, long long F) {
    const long long a = i - off;                               // position within the frame at hop 0 of the window's first tap
    if (a < 0) return 0.0;
    long long hi = a / hop, lo = a - win + 1 <= 0 ? 0 : (a - win + hop) / hop;
    if (hi > F - 1) hi = F - 1;
    double s = 0.0;
    for (long long f = lo; f <= hi; ++f) s += gf[f * win + (a - f * hop)];
    return s;
}

// ---- backward, samples: grid (ceil(T / 256), B * E) -> g_est [B][E][T] ------------------------------------------------------------
__global__ __launch_bounds__(NT) void mrstft_gather_kernel(const double* __restrict__ gframes, const long long* __restrict__ lens,
                                                           const int* __restrict__ est_of_ref, int C, int E, long long T, ResTab t,
                                                           float* __restrict__ g_est) {
    const long long row = blockIdx.y, b = row / E, e = row % E;
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= T) return;
    const long long n = clamp_len(lens, b, T);
    double acc = 0.0;
    if (i < n) {
        for (int c = 0; c < C; ++c) {
            if (clamp_row(est_of_ref[b * C + c], E) != e) continue;
            const double* __restrict__ gp = gframes + (size_t)(b * C + c) * t.GT;
            for (int r = 0; r < t.R; ++r) {
                const int N = t.nfft[r], hop = t.hop[r], win = t.win[r], off = t.off[r], half = N >> 1;
                if (n <= half) continue;
                const long long F = 1 + n / hop;
                const double* __restrict__ gf = gp + t.goff[r];
                double s = cover_sum(gf, i + half, hop, win, off, F);                  // the sample itself
                if (i >= 1 && i <= half) s += cover_sum(gf, half - i, hop, win, off, F);            // its image before sample 0
                if (i <= n - 2) s += cover_sum(gf, 2 * (n - 1) - i + half, hop, win, off, F);       // its image beyond sample n - 1
                acc += s;
            }
        }
    }
    g_est[row * T + i] = (float)acc;
}

#define MRSTFT_CHECK_SIZES(fn, B, C, E, T)                                                                                         \
    CTN_REQUIRE((B) >= 1 && (C) >= 1 && (C) <= 64 && (long long)(B) * (C) <= 65535, fn ": B = %lld, C = %d (B * C in 1..65535, C <= 64)", \
                (long long)(B), (int)(C));                                                                                         \
    CTN_REQUIRE((E) >= 1 && (long long)(B) * (E) <= 65535, fn ": E = %lld (B * E in 1..65535)", (long long)(E));                    \
    CTN_REQUIRE((T) >= 1 && (T) <= MAX_T, fn ": T = %lld outside 1..2^24", (long long)(T))

bool sizes_ok(long long B, int C, long long T) { return B >= 1 && C >= 1 && C <= 64 && B * C <= 65535 && T >= 1 && T <= MAX_T; }

}  // namespace

extern "C" {

// see include/ctn_hip.h
size_t ctn_mrstft_workspace(long long B, int C, long long T, int R, const int* resolutions) {
    ResTab t;
    const char* why;
    if (!resolutions || !sizes_ok(B, C, T) || !make_tab(R, resolutions, T, t, &why)) return 0;
    return fwd_layout(nullptr, B * C, t).total;
}

size_t ctn_mrstft_bwd_workspace(long long B, int C, long long T, int R, const int* resolutions) {
    ResTab t;
    const char* why;
    if (!resolutions || !sizes_ok(B, C, T) || !make_tab(R, resolutions, T, t, &why)) return 0;
    return aligned(sizeof(double) * (size_t)(B * C) * (size_t)t.GT);
}

int ctn_mrstft_pairs_fwd(const float* ref, const float* est, const long long* lengths, const int* est_of_ref, long long B, int C,
                         long long E, long long T, const int* resolutions, int R, double eps, double* terms, void* workspace,
                         size_t workspace_bytes, void* stream) {
    CTN_REQUIRE(ref && est && lengths && est_of_ref && resolutions && terms, "ctn_mrstft_pairs_fwd: null pointer");
    MRSTFT_CHECK_SIZES("ctn_mrstft_pairs_fwd", B, C, E, T);
    CTN_REQUIRE(eps > 0.0, "ctn_mrstft_pairs_fwd: eps = %g must be positive", eps);
    ResTab t;
    const char* why = "";
    CTN_REQUIRE(make_tab(R, resolutions, T, t, &why), "ctn_mrstft_pairs_fwd: resolution out of range: %s", why);
    const long long P = B * C;
    if (workspace == nullptr || workspace_bytes < fwd_layout(nullptr, P, t).total) {
        ctn_set_error("ctn_mrstft_pairs_fwd: workspace too small");
        return CTN_ERR_WORKSPACE;
    }
    const FwdLayout l = fwd_layout(workspace, P, t);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mrstft_tables_kernel, dim3(1 + R), dim3(NT), 0, st, t, l.tw, l.wtab);
    CTN_CHECK_LAUNCH("ctn_mrstft_pairs_fwd/tables");
    hipLaunchKernelGGL(mrstft_fwd_kernel, dim3((unsigned)t.maxpass, (unsigned)R, (unsigned)P), dim3(NT), 0, st, ref, est, lengths,
                       est_of_ref, C, (int)E, T, t, eps, l.tw, l.wtab, l.part);
    CTN_CHECK_LAUNCH("ctn_mrstft_pairs_fwd");
    hipLaunchKernelGGL(mrstft_terms_kernel, dim3((unsigned)R, (unsigned)P), dim3(NT), 0, st, l.part, lengths, C, T, t, terms, l.sums);
    CTN_CHECK_LAUNCH("ctn_mrstft_pairs_fwd/terms");
    return CTN_OK;
}

int ctn_mrstft_pairs_bwd(const void* fwd_workspace, size_t fwd_workspace_bytes, const float* ref, const float* est,
                         const long long* lengths, const int* est_of_ref, long long B, int C, long long E, long long T,
                         const int* resolutions, int R, double eps, const double* g_terms, float* g_est, void* workspace,
                         size_t workspace_bytes, void* stream) {
    CTN_REQUIRE(fwd_workspace && ref && est && lengths && est_of_ref && resolutions && g_terms && g_est,
                "ctn_mrstft_pairs_bwd: null pointer");
    MRSTFT_CHECK_SIZES("ctn_mrstft_pairs_bwd", B, C, E, T);
    CTN_REQUIRE(eps > 0.0, "ctn_mrstft_pairs_bwd: eps = %g must be positive", eps);
    ResTab t;
    const char* why = "";
    CTN_REQUIRE(make_tab(R, resolutions, T, t, &why), "ctn_mrstft_pairs_bwd: resolution out of range: %s", why);
    const long long P = B * C;
    if (fwd_workspace_bytes < fwd_layout(nullptr, P, t).total || workspace == nullptr ||
        workspace_bytes < aligned(sizeof(double) * (size_t)P * (size_t)t.GT)) {
        ctn_set_error("ctn_mrstft_pairs_bwd: workspace too small");
        return CTN_ERR_WORKSPACE;
    }
    const FwdLayout l = fwd_layout(const_cast<void*>(fwd_workspace), P, t);
    double* gframes = (double*)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mrstft_bwd_kernel, dim3((unsigned)t.maxpass, (unsigned)R, (unsigned)P), dim3(NT), 0, st, ref, est, lengths,
                       est_of_ref, C, (int)E, T, t, eps, l.tw, l.wtab, l.sums, g_terms, gframes);
    CTN_CHECK_LAUNCH("ctn_mrstft_pairs_bwd");
    hipLaunchKernelGGL(mrstft_gather_kernel, dim3((unsigned)ctn_cdivll(T, NT), (unsigned)(B * E)), dim3(NT), 0, st, gframes, lengths,
                       est_of_ref, C, (int)E, T, t, g_est);
    CTN_CHECK_LAUNCH("ctn_mrstft_pairs_bwd/gather");
    return CTN_OK;
}

}  // extern "C"
