// Noisy and reverberant dynamic mixing: the plan's extra draws (one RIR per source, one noise segment and SNR per mixture),
// the reverberation of the drawn segments (direct convolution with a room impulse response, early-taps target), and the mix
// with separate target rows and a noise row.
// Contract: include/ctn_hip.h ("noisy and reverberant dynamic mixing"); executable restatement: tests/dynmix_aug_oracle.py.
// Every float32 operation is ONE rounding in a stated order (no contraction into fused multiply-adds, IEEE division), so the
// outputs are a bitwise function of the plan and the data, whatever the launch geometry.
#include "ctn_dynmix_common.h"

#pragma clang fp contract(off)

namespace {

// One rounding each.  Written here, under the pragma above, in plain operators: __fmul_rn / __fadd_rn are inline functions of a
// header compiled under the default contraction mode, and a product whose only use is the add behind it is fused there.
__device__ __forceinline__ float am_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float am_add(float a, float b) { return a + b; }

constexpr int RV_PT = 4;                // consecutive outputs per thread: the sliding window of x is RV_PT + 4 registers
constexpr int RV_TILE = RV_PT * DM_NT;  // 1024 outputs of one row per workgroup
constexpr int RV_JC = 1024;             // taps staged in LDS at a time
constexpr int RV_MAX_TAPS = 8192;       // longest response
constexpr int AUG_MAX_SNR = 1024;       // most entries of the SNR table

// ---- plan ----------------------------------------------------------------------------------------------------------------
// One workgroup; thread b draws mixture b (and b + NT, ...).  Reads the step word and leaves it alone: ctn_dynmix_plan /
// ctn_dynmix_plan_speed, launched behind this kernel on the same stream, advance it.
__global__ __launch_bounds__(DM_NT) void dynmix_plan_aug_kernel(unsigned k0, unsigned k1, unsigned epoch, const unsigned* __restrict__ step_word,
                                                                int B, int C, int seg_len, int R, int* __restrict__ plan_rir,
                                                                const int* __restrict__ noise_ids, int Nn, const long long* __restrict__ noise_lens,
                                                                int Un, const float* __restrict__ noise_inv_rms, const float* __restrict__ wn,
                                                                int nsnr, int lo10, int* __restrict__ noise_utt,
                                                                long long* __restrict__ noise_start, int* __restrict__ snr10,
                                                                float* __restrict__ ngain) {
    const unsigned step = *step_word;
    for (int b = threadIdx.x; b < B; b += DM_NT) {
        if (plan_rir != nullptr) {
            for (int c = 0; c < C; ++c) {
                const Philox4 r = philox4x32_10((unsigned)c + 512u, (unsigned)b, step, epoch, k0, k1);
                plan_rir[b * C + c] = (int)below(r.w[0], (unsigned long long)R);
            }
        }
        if (noise_utt != nullptr) {
            const Philox4 r = philox4x32_10(768u, (unsigned)b, step, epoch, k0, k1);
            const int v = noise_ids[below(r.w[0], (unsigned long long)Nn)];
            const int k = (int)below(r.w[2], (unsigned long long)nsnr);
            if (v < 0 || v >= Un || noise_lens[v] < seg_len) {   // tables that break their contract: an entry the mix flags (peak = -1)
                noise_utt[b] = -1;
                noise_start[b] = 0;
                snr10[b] = lo10 + k;
                ngain[b] = 0.0f;
                continue;
            }
            noise_utt[b] = v;
            noise_start[b] = (long long)below(r.w[1], (unsigned long long)(noise_lens[v] - seg_len + 1));
            snr10[b] = lo10 + k;
            ngain[b] = am_mul(wn[k], noise_inv_rms[v]);
        }
    }
}

// ---- reverberation -------------------------------------------------------------------------------------------------------
// acc[k] += sum over taps j in [jbeg, jend), ascending, of h[j] * x[t + d - j] for the thread's outputs t = t0 + RV_PT * tid + k;
// x outside [0, T) reads as zero.
//
// Taps whose samples lie outside [0, T) for EVERY output of the tile are skipped, the others meet staged zeros.  Both give the
// bits of the contract's full sum: such a term is h * 0 = +-0, and acc + (+-0) == acc bit for bit unless acc is -0 -- which it
// never is: acc starts at +0, (+0) + (-0) = +0, a sum of two non-zero floats that cancel is +0 under round-to-nearest, and a
// non-zero acc plus a zero keeps its bits.
//
// Per chunk of up to RV_JC taps starting at jc, xs[m] = x[t0 + d - jc - RV_JC + m]: the sample of tap jc + jj and output
// t0 + o sits at xs[RV_JC + o - jj].  A thread keeps the RV_PT samples of the current tap in registers; four taps further on the
// window has moved down by one aligned float4, so one 16-byte read of x and one broadcast 16-byte read of h feed
// 4 * RV_PT multiply-adds.  The taps left over (fewer than four) read their samples one by one.
__device__ __forceinline__ void rv_taps(const float* __restrict__ xrow, int T, const float* __restrict__ h, int jbeg, int jend, int t0, int d,
                                        float* __restrict__ xs, float* __restrict__ hs, float (&acc)[RV_PT]) {
    const int lo = max(jbeg, t0 + d - T + 1), hi = min(jend, t0 + RV_TILE + d);
    const float* const xw = xs + RV_JC + RV_PT * (int)threadIdx.x;
    const float4* const xw4 = reinterpret_cast<const float4*>(xs) + RV_JC / 4 + (int)threadIdx.x;
    const float4* const hs4 = reinterpret_cast<const float4*>(hs);
    for (int jc = lo; jc < hi; jc += RV_JC) {
        const int len = min(RV_JC, hi - jc), len4 = len & ~3;
        __syncthreads();                                                // the chunk before this one has been read
        for (int jj = threadIdx.x; jj < len; jj += DM_NT) hs[jj] = h[jc + jj];
        const int gbase = t0 + d - jc - RV_JC;
        for (int m = RV_JC - len + (int)threadIdx.x; m < RV_TILE + RV_JC; m += DM_NT) {
            const int g = gbase + m;
            xs[m] = (g >= 0 && g < T) ? xrow[g] : 0.0f;
        }
        __syncthreads();
        float4 w = xw4[0];
#pragma unroll 2
        for (int q = 0; q < len4 / 4; ++q) {
            const float4 p = xw4[-q - 1];
            const float4 hh = hs4[q];
            const float v[8] = {p.x, p.y, p.z, p.w, w.x, w.y, w.z, w.w};
            const float hv[4] = {hh.x, hh.y, hh.z, hh.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int k = 0; k < RV_PT; ++k) acc[k] = am_add(acc[k], am_mul(hv[u], v[4 + k - u]));
            }
            w = p;
        }
        for (int jj = len4; jj < len; ++jj) {
            const float hv = hs[jj];
#pragma unroll
            for (int k = 0; k < RV_PT; ++k) acc[k] = am_add(acc[k], am_mul(hv, xw[k - jj]));
        }
    }
}

// the thread's RV_PT outputs of one row; 16-byte stores where the rows are 16-byte aligned (T % 4 == 0)
__device__ __forceinline__ void rv_store(float* __restrict__ row, int T, int t, const float (&acc)[RV_PT]) {
    static_assert(RV_PT == 4, "rv_store writes one float4 per thread");
    if ((T & 3) == 0 && t + 4 <= T) {
        *reinterpret_cast<float4*>(row + t) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
#pragma unroll
        for (int k = 0; k < RV_PT; ++k)
            if (t + k < T) row[t + k] = acc[k];
    }
}

// grid (ceil(T / RV_TILE), N).  A row whose plan entry or response breaks its tables is never read: zeros, out_utt = -1.
__global__ __launch_bounds__(DM_NT) void dynmix_reverb_kernel(const float* __restrict__ corpus, const long long* __restrict__ offsets,
                                                              const long long* __restrict__ lens, int U, const int* __restrict__ plan_utt,
                                                              const long long* __restrict__ plan_start, int T, const float* __restrict__ bank,
                                                              long long bank_floats, const long long* __restrict__ rir_offsets,
                                                              const int* __restrict__ rir_lens, const int* __restrict__ rir_direct,
                                                              const int* __restrict__ rir_early, int R, const int* __restrict__ plan_rir,
                                                              float* __restrict__ wet, float* __restrict__ tgt, int* __restrict__ out_utt) {
    __shared__ __align__(16) float xs[RV_TILE + RV_JC];
    __shared__ __align__(16) float hs[RV_JC];
    const int i = blockIdx.y, t0 = blockIdx.x * RV_TILE, t = t0 + RV_PT * (int)threadIdx.x;
    const int u = plan_utt[i], r = plan_rir[i];
    const long long st = plan_start[i];
    bool ok = u >= 0 && u < U && st >= 0 && r >= 0 && r < R;
    if (ok) ok = st + (long long)T <= lens[u];
    long long ho = 0;
    int n = 0, d = 0, e = 0;
    if (ok) {
        ho = rir_offsets[r]; n = rir_lens[r]; d = rir_direct[r]; e = rir_early[r];
        ok = ho >= 0 && n >= 1 && n <= RV_MAX_TAPS && ho + n <= bank_floats && d >= 0 && d < n && e >= 0 && e <= n;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out_utt[i] = ok ? i : -1;      // the mix flags -1 entries: peak[b] = -1
    float acc[RV_PT];
#pragma unroll
    for (int k = 0; k < RV_PT; ++k) acc[k] = 0.0f;
    float* const wrow = wet + (long long)i * T;
    float* const trow = tgt != nullptr ? tgt + (long long)i * T : nullptr;
    if (!ok) {
        rv_store(wrow, T, t, acc);
        if (trow != nullptr) rv_store(trow, T, t, acc);
        return;
    }
    const float* __restrict__ xrow = corpus + offsets[u] + st;
    const float* __restrict__ h = bank + ho;
    if (trow != nullptr) {                                                  // the tap loop is split at `early`: the snapshot is free
        rv_taps(xrow, T, h, 0, e, t0, d, xs, hs, acc);
        rv_store(trow, T, t, acc);
        rv_taps(xrow, T, h, e, n, t0, d, xs, hs, acc);
    } else {
        rv_taps(xrow, T, h, 0, n, t0, d, xs, hs, acc);
    }
    rv_store(wrow, T, t, acc);
}

// ---- the mix ---------------------------------------------------------------------------------------------------------------
template <int C>
struct AugRows {
    const float* src[C];    // first sample of the mixture component of source c
    const float* tg[C];     // first sample of its target (== src[c] without a target corpus)
    float g[C];
    const float* nz;        // first sample of the noise segment
    float ng;
    bool split, noisy;      // a target corpus / a noise corpus is configured
    bool bad;               // a source or noise entry points outside its utterance: it reads as silence, peak[b] = -1
};

#define AUG_GATHER_ARGS                                                                                                          \
    const float *__restrict__ corpus, const long long *__restrict__ offsets, const long long *__restrict__ lens, int U,         \
        const int *__restrict__ plan_utt, const long long *__restrict__ plan_start, const float *__restrict__ gain, int T,      \
        const float *__restrict__ tgt_corpus, const float *__restrict__ noise, const long long *__restrict__ noise_offsets,     \
        const long long *__restrict__ noise_lens, int Un, const int *__restrict__ noise_utt,                                    \
        const long long *__restrict__ noise_start, const float *__restrict__ ngain
#define AUG_GATHER_PASS                                                                                                          \
    corpus, offsets, lens, U, plan_utt, plan_start, gain, T, tgt_corpus, noise, noise_offsets, noise_lens, Un, noise_utt,       \
        noise_start, ngain

template <int C>
__device__ __forceinline__ AugRows<C> aug_load_rows(AUG_GATHER_ARGS, int b) {
    AugRows<C> r;
    r.bad = false;
    r.split = tgt_corpus != nullptr;
    r.noisy = noise != nullptr;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int u = plan_utt[b * C + c];
        const long long st = plan_start[b * C + c];
        const bool ok = u >= 0 && u < U && st >= 0 && st + (long long)T <= lens[u < 0 || u >= U ? 0 : u];
        r.src[c] = ok ? corpus + offsets[u] + st : nullptr;
        r.tg[c] = ok && r.split ? tgt_corpus + offsets[u] + st : r.src[c];
        r.g[c] = gain[b * C + c];
        r.bad = r.bad || !ok;
    }
    r.nz = nullptr;
    r.ng = 0.0f;
    if (r.noisy) {
        const int v = noise_utt[b];
        const long long st = noise_start[b];
        const bool ok = v >= 0 && v < Un && st >= 0 && st + (long long)T <= noise_lens[v < 0 || v >= Un ? 0 : v];
        r.nz = ok ? noise + noise_offsets[v] + st : nullptr;
        r.ng = ngain[b];
        r.bad = r.bad || !ok;
    }
    return r;
}

// g_c[t] and mix[t] of one sample, each operation rounded once
template <int C>
__device__ __forceinline__ float aug_one(const AugRows<C>& r, int t, float (&g)[C]) {
    float s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        s[c] = r.src[c] != nullptr ? am_mul(r.g[c], r.src[c][t]) : 0.0f;
        g[c] = r.split ? (r.tg[c] != nullptr ? am_mul(r.g[c], r.tg[c][t]) : 0.0f) : s[c];
    }
    float m = am_add(s[0], s[1]);
#pragma unroll
    for (int c = 2; c < C; ++c) m = am_add(m, s[c]);
    if (r.noisy) m = am_add(m, r.nz != nullptr ? am_mul(r.ng, r.nz[t]) : 0.0f);
    return m;
}

// launch 1: wgmax[b, chunk] = the maximum of |mix| and every |g_c| over this workgroup's DM_CHUNK samples.  grid (nchunk, B)
template <int C>
__global__ __launch_bounds__(DM_NT) void dynmix_aug_peak_kernel(AUG_GATHER_ARGS, float* __restrict__ wgmax) {
    __shared__ float scratch[DM_NT / 64];
    const int b = blockIdx.y, t0 = blockIdx.x * DM_CHUNK, t1 = min(T, t0 + DM_CHUNK);
    const AugRows<C> r = aug_load_rows<C>(AUG_GATHER_PASS, b);
    float a = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int t = t0 + 4 * (int)threadIdx.x + k;
        if (t < t1) {
            float g[C];
            a = fmaxf(a, fabsf(aug_one<C>(r, t, g)));
#pragma unroll
            for (int c = 0; c < C; ++c) a = fmaxf(a, fabsf(g[c]));
        }
    }
    a = block_max<DM_NT>(a, scratch);
    if (threadIdx.x == 0) wgmax[(long long)b * gridDim.x + blockIdx.x] = a;
}

// launch 2: the maximum over the mixture's workgroup maxima, then the scaled samples, recomputed with the same roundings
template <int C>
__global__ __launch_bounds__(DM_NT) void dynmix_aug_write_kernel(AUG_GATHER_ARGS, const float* __restrict__ wgmax, float over,
                                                                 float* __restrict__ mixture, float* __restrict__ sources,
                                                                 float* __restrict__ peak) {
    __shared__ float scratch[DM_NT / 64];
    const int b = blockIdx.y, t0 = blockIdx.x * DM_CHUNK, t1 = min(T, t0 + DM_CHUNK), nchunk = gridDim.x;
    const AugRows<C> r = aug_load_rows<C>(AUG_GATHER_PASS, b);
    float a = 0.0f;
    for (int i = threadIdx.x; i < nchunk; i += DM_NT) a = fmaxf(a, wgmax[(long long)b * nchunk + i]);
    a = block_max<DM_NT>(a, scratch);
    if (blockIdx.x == 0 && threadIdx.x == 0) peak[b] = r.bad ? -1.0f : a;
    const float scale = peak_scale(a, over);
    float* const mixrow = mixture + (long long)b * T;
    float* const srcrows = sources + (long long)b * C * T;
    const int t4 = t0 + 4 * (int)threadIdx.x;
    if ((T & 3) == 0 && t4 + 4 <= t1) {                      // 16-byte stores where the rows are 16-byte aligned
        float m[4], g[4][C];
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = am_mul(scale, aug_one<C>(r, t4 + k, g[k]));
        *reinterpret_cast<float4*>(mixrow + t4) = make_float4(m[0], m[1], m[2], m[3]);
#pragma unroll
        for (int c = 0; c < C; ++c)
            *reinterpret_cast<float4*>(srcrows + (long long)c * T + t4) =
                make_float4(am_mul(scale, g[0][c]), am_mul(scale, g[1][c]), am_mul(scale, g[2][c]), am_mul(scale, g[3][c]));
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (t4 + k < t1) {
                float g[C];
                mixrow[t4 + k] = am_mul(scale, aug_one<C>(r, t4 + k, g));
#pragma unroll
                for (int c = 0; c < C; ++c) srcrows[(long long)c * T + t4 + k] = am_mul(scale, g[c]);
            }
        }
    }
}

template <int C>
int aug_gather_launch(AUG_GATHER_ARGS, int B, float* mixture, float* sources, float* peak, float* wgmax, float over, hipStream_t st) {
    const dim3 grid(ctn_cdiv(T, DM_CHUNK), B);
    dynmix_aug_peak_kernel<C><<<grid, dim3(DM_NT), 0, st>>>(AUG_GATHER_PASS, wgmax);
    CTN_CHECK_LAUNCH("ctn_dynmix_gather_aug (peak)");
    dynmix_aug_write_kernel<C><<<grid, dim3(DM_NT), 0, st>>>(AUG_GATHER_PASS, wgmax, over, mixture, sources, peak);
    CTN_CHECK_LAUNCH("ctn_dynmix_gather_aug (write)");
    return CTN_OK;
}

}  // namespace

extern "C" {

int ctn_dynmix_plan_aug(long long seed, int epoch, int rank, const unsigned* step, int B, int C, int seg_len, int R, int* plan_rir,
                        const int* noise_ids, int Nn, const long long* noise_lens, long long Un, const float* noise_inv_rms,
                        const float* wn, int nsnr, int lo10, int* noise_utt, long long* noise_start, int* snr10, float* ngain,
                        void* stream) {
    const bool rir = plan_rir != nullptr;
    const bool any = noise_ids || noise_lens || noise_inv_rms || wn || noise_utt || noise_start || snr10 || ngain;
    const bool all = noise_ids && noise_lens && noise_inv_rms && wn && noise_utt && noise_start && snr10 && ngain;
    CTN_REQUIRE(step != nullptr, "ctn_dynmix_plan_aug: null pointer (step)");
    CTN_REQUIRE(rir || any, "ctn_dynmix_plan_aug: null pointer (neither plan_rir nor the noise half is given)");
    CTN_REQUIRE(!any || all, "ctn_dynmix_plan_aug: null pointer (the noise half needs all of its eight arrays)");
    CTN_REQUIRE(C >= 2 && C <= 4, "ctn_dynmix_plan_aug: C = %d sources per mixture (2 .. 4)", C);
    CTN_REQUIRE(B >= 1 && B <= (1 << 20), "ctn_dynmix_plan_aug: B = %d mixtures (1 .. 2^20)", B);
    CTN_REQUIRE(seg_len >= 1, "ctn_dynmix_plan_aug: seg_len = %d", seg_len);
    CTN_REQUIRE(seed >= 0 && seed < (1LL << 48), "ctn_dynmix_plan_aug: seed %lld outside [0, 2^48)", seed);
    CTN_REQUIRE(rank >= 0 && rank < (1 << 16), "ctn_dynmix_plan_aug: rank %d outside [0, 2^16)", rank);
    CTN_REQUIRE(epoch >= 0, "ctn_dynmix_plan_aug: epoch %d", epoch);
    if (rir) CTN_REQUIRE(R >= 1, "ctn_dynmix_plan_aug: R = %d responses", R);
    if (any) {
        CTN_REQUIRE(Nn >= 1, "ctn_dynmix_plan_aug: Nn = %d eligible noise utterances", Nn);
        CTN_REQUIRE(Un >= 1 && Un <= 0x7fffffffLL, "ctn_dynmix_plan_aug: Un = %lld noise utterances (1 .. 2^31 - 1)", Un);
        CTN_REQUIRE(nsnr >= 1 && nsnr <= AUG_MAX_SNR, "ctn_dynmix_plan_aug: nsnr = %d SNR values (1 .. %d)", nsnr, AUG_MAX_SNR);
    }
    const unsigned k0 = (unsigned)(seed & 0xffffffffLL), k1 = (unsigned)(seed >> 32) | ((unsigned)rank << 16);
    dynmix_plan_aug_kernel<<<dim3(1), dim3(DM_NT), 0, (hipStream_t)stream>>>(k0, k1, (unsigned)epoch, step, B, C, seg_len, R, plan_rir, noise_ids,
                                                                             Nn, noise_lens, (int)Un, noise_inv_rms, wn, nsnr, lo10, noise_utt,
                                                                             noise_start, snr10, ngain);
    CTN_CHECK_LAUNCH("ctn_dynmix_plan_aug");
    return CTN_OK;
}

int ctn_dynmix_reverb(const float* corpus, const long long* offsets, const long long* lens, long long U, const int* plan_utt,
                      const long long* plan_start, int N, int T, const float* bank, long long bank_floats, const long long* rir_offsets,
                      const int* rir_lens, const int* rir_direct, const int* rir_early, int R, const int* plan_rir, float* wet, float* tgt,
                      int* out_utt, void* stream) {
    CTN_REQUIRE(corpus && offsets && lens && plan_utt && plan_start && bank && rir_offsets && rir_lens && rir_direct && rir_early &&
                    plan_rir && wet && out_utt,
                "ctn_dynmix_reverb: null pointer");
    CTN_REQUIRE(N >= 1 && N <= 65535, "ctn_dynmix_reverb: N = %d rows (1 .. 65535)", N);
    CTN_REQUIRE(T >= 1 && T <= (1 << 30), "ctn_dynmix_reverb: seg_len = %d (1 .. 2^30)", T);
    CTN_REQUIRE(U >= 1 && U <= 0x7fffffffLL, "ctn_dynmix_reverb: U = %lld utterances (1 .. 2^31 - 1)", U);
    CTN_REQUIRE(R >= 1, "ctn_dynmix_reverb: R = %d responses", R);
    CTN_REQUIRE(bank_floats >= 1, "ctn_dynmix_reverb: bank_floats = %lld", bank_floats);
    CTN_REQUIRE((((size_t)wet | (size_t)tgt) & 15) == 0, "ctn_dynmix_reverb: wet and tgt must be 16-byte aligned");
    dynmix_reverb_kernel<<<dim3(ctn_cdiv(T, RV_TILE), N), dim3(DM_NT), 0, (hipStream_t)stream>>>(
        corpus, offsets, lens, (int)U, plan_utt, plan_start, T, bank, bank_floats, rir_offsets, rir_lens, rir_direct, rir_early, R, plan_rir,
        wet, tgt, out_utt);
    CTN_CHECK_LAUNCH("ctn_dynmix_reverb");
    return CTN_OK;
}

int ctn_dynmix_gather_aug_peak(const float* corpus, const long long* offsets, const long long* lens, long long U, const int* plan_utt,
                               const long long* plan_start, const float* gain, int B, int C, int T, const float* tgt_corpus,
                               const float* noise, const long long* noise_offsets, const long long* noise_lens, long long Un,
                               const int* noise_utt, const long long* noise_start, const float* ngain, float* mixture, float* sources,
                               float* peak, void* workspace, size_t workspace_bytes, int peak_mode, void* stream);

// peak mode 0: the rule of every mixture before the LibriMix recipe, the same launches and bits
int ctn_dynmix_gather_aug(const float* corpus, const long long* offsets, const long long* lens, long long U, const int* plan_utt,
                          const long long* plan_start, const float* gain, int B, int C, int T, const float* tgt_corpus,
                          const float* noise, const long long* noise_offsets, const long long* noise_lens, long long Un,
                          const int* noise_utt, const long long* noise_start, const float* ngain, float* mixture, float* sources,
                          float* peak, void* workspace, size_t workspace_bytes, void* stream) {
    return ctn_dynmix_gather_aug_peak(corpus, offsets, lens, U, plan_utt, plan_start, gain, B, C, T, tgt_corpus, noise, noise_offsets,
                                      noise_lens, Un, noise_utt, noise_start, ngain, mixture, sources, peak, workspace, workspace_bytes, 0,
                                      stream);
}

// see include/ctn_hip.h ("LibriMix-recipe mixing")
int ctn_dynmix_gather_aug_peak(const float* corpus, const long long* offsets, const long long* lens, long long U, const int* plan_utt,
                               const long long* plan_start, const float* gain, int B, int C, int T, const float* tgt_corpus,
                               const float* noise, const long long* noise_offsets, const long long* noise_lens, long long Un,
                               const int* noise_utt, const long long* noise_start, const float* ngain, float* mixture, float* sources,
                               float* peak, void* workspace, size_t workspace_bytes, int peak_mode, void* stream) {
    CTN_REQUIRE(peak_mode == 0 || peak_mode == 1, "ctn_dynmix_gather_aug: peak_mode %d (0: always rescale; 1: only what would clip)",
                peak_mode);
    CTN_REQUIRE(corpus && offsets && lens && plan_utt && plan_start && gain && mixture && sources && peak,
                "ctn_dynmix_gather_aug: null pointer");
    if (noise != nullptr) {
        CTN_REQUIRE(noise_offsets && noise_lens && noise_utt && noise_start && ngain, "ctn_dynmix_gather_aug: null pointer (noise tables)");
        CTN_REQUIRE(Un >= 1 && Un <= 0x7fffffffLL, "ctn_dynmix_gather_aug: Un = %lld noise utterances (1 .. 2^31 - 1)", Un);
    }
    CTN_REQUIRE(C >= 2 && C <= 4, "ctn_dynmix_gather_aug: C = %d sources per mixture (2 .. 4)", C);
    CTN_REQUIRE(T >= 1, "ctn_dynmix_gather_aug: seg_len = %d", T);
    CTN_REQUIRE(B >= 1 && B <= 65535, "ctn_dynmix_gather_aug: B = %d mixtures (1 .. 65535)", B);
    CTN_REQUIRE(U >= 1 && U <= 0x7fffffffLL, "ctn_dynmix_gather_aug: U = %lld utterances (1 .. 2^31 - 1)", U);
    CTN_REQUIRE((((size_t)mixture | (size_t)sources) & 15) == 0, "ctn_dynmix_gather_aug: mixture and sources must be 16-byte aligned");
    CTN_REQUIRE(workspace != nullptr, "ctn_dynmix_gather_aug: null workspace");
    const size_t need = sizeof(float) * (size_t)B * (size_t)ctn_cdiv(T, DM_CHUNK);     // == ctn_dynmix_gather_workspace(B, T)
    if (workspace_bytes < need) {
        ctn_set_error("ctn_dynmix_gather_aug: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return CTN_ERR_WORKSPACE;
    }
    const hipStream_t st = (hipStream_t)stream;
    float* const wg = (float*)workspace;
    const int Ui = (int)U, Uni = noise != nullptr ? (int)Un : 0;
    const float over = peak_over(peak_mode);
    switch (C) {
        case 2: return aug_gather_launch<2>(corpus, offsets, lens, Ui, plan_utt, plan_start, gain, T, tgt_corpus, noise, noise_offsets, noise_lens,
                                            Uni, noise_utt, noise_start, ngain, B, mixture, sources, peak, wg, over, st);
        case 3: return aug_gather_launch<3>(corpus, offsets, lens, Ui, plan_utt, plan_start, gain, T, tgt_corpus, noise, noise_offsets, noise_lens,
                                            Uni, noise_utt, noise_start, ngain, B, mixture, sources, peak, wg, over, st);
        default: return aug_gather_launch<4>(corpus, offsets, lens, Ui, plan_utt, plan_start, gain, T, tgt_corpus, noise, noise_offsets,
                                             noise_lens, Uni, noise_utt, noise_start, ngain, B, mixture, sources, peak, wg, over, st);
    }
}

}  // extern "C"
