// ITU-T P.56 active speech level (method B) of ragged utterances: the band filter, the envelope, its octave exponents, the 0.2 s
// hangover and the 20-bin occupancy, all on the device.  Contract: include/ctn_hip.h ("active speech level"); executable
// restatement: tests/levels_oracle.py.
// Both filters are linear, so every utterance is cut into chunks of LV_CH samples by its own sample index: pass 1 runs every chunk
// from zero state, a carry per utterance turns the end states into true start states (s_{c+1} = T s_c + z_c, T = A^CH from the
// host), pass 2 reruns every chunk from its true state.  One lane per chunk; a wave stages 64 chunks x 32 samples through LDS so
// that the global loads and the exponent stores are whole rows.
// Every fp64 product and sum is ONE rounding in the written order (no contraction), counts and maxima are integers: the statistics
// of an utterance are a bitwise function of its own samples, the tables and LV_CH.
#include "ctn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int LV_CH = 1024;           // samples per chunk (ctn_active_level_chunk)
constexpr int LV_TS = 32;             // samples of every chunk staged per round (8.4 KB of LDS per wave: several waves per SIMD)
constexpr int LV_LPR = LV_TS / 4;     // lanes per staged row (4 samples each)
constexpr int LV_RPI = 64 / LV_LPR;   // rows per load instruction
constexpr int LV_ROWS = 64;           // chunks per workgroup of the filter passes: one wave, one lane per chunk
constexpr int LV_NH_MAX = 9601;       // hangover at 48 kHz
constexpr int LV_NH_MIN = LV_CH;      // levels_hang_kernel splits a window ONCE, at its chunk's first sample: a window must not
                                      // lie inside a chunk, so nh >= LV_CH (1601 at 8 kHz; a larger LV_CH needs another kernel)
constexpr long long LV_G_MAX = (1ll << 24) - 1;      // levels_hang_kernel: one workgroup of 256 per chunk, grid x block < 2^32
static_assert(LV_NH_MIN <= 1601, "the hangover at 8 kHz (1601 samples) must span a chunk: see levels_hang_kernel");
constexpr int LV_NBIN = 20;
constexpr int LV_EMPTY = -32768;      // exponent of a zero: stands for -inf
constexpr int LV_SLOTS = 12;          // fp64 state words per chunk in the workspace: 10 band + 2 envelope
constexpr int LV_HANG_NT = 256;
// the table (fp64): sections, then the transition matrices
constexpr int LT_HP1 = 0, LT_BQ1 = 3, LT_BQ2 = 8, LT_LP = 13, LT_ENV = 24, LT_TBAND = 27, LT_TENV = 127, LT_SIZE = 131;

typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));       // four samples from a 4-byte aligned address
typedef short short4v __attribute__((ext_vector_type(4)));

struct Utt {
    long long off, len, n, cp0;       // first sample, samples, samples with the appended zeros, first chunk
    long long nch;
    bool ok;
};

// An utterance whose samples lie inside the buffer and whose chunk range is the one its length asks for; anything else is
// flagged and never read.
__device__ __forceinline__ Utt utt_info(long long u, const long long* __restrict__ offsets, const long long* __restrict__ lens,
                                        const long long* __restrict__ chunk_ptr, long long num_samples, long long G, int nz) {
    Utt r;
    r.off = offsets[u];
    r.len = lens[u];
    r.cp0 = chunk_ptr[u];
    const long long cp1 = chunk_ptr[u + 1];
    r.ok = r.off >= 0 && r.len >= 0 && r.len <= num_samples && r.off <= num_samples - r.len;
    r.n = r.ok ? r.len + nz : 0;
    r.nch = (r.n + LV_CH - 1) / LV_CH;
    r.ok = r.ok && r.n >= 1 && r.cp0 >= 0 && cp1 <= G && cp1 - r.cp0 == r.nch;
    return r;
}

// the utterance whose chunk range holds chunk g: the last u with chunk_ptr[u] <= g
__device__ __forceinline__ long long utt_of_chunk(long long g, const long long* __restrict__ chunk_ptr, long long U) {
    long long lo = 0, hi = U - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (chunk_ptr[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// frexp exponent of v >= 0 (v = f 2^e, 0.5 <= f < 1), denormals included; LV_EMPTY for zero
__device__ __forceinline__ int exponent_of(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const int be = (int)((b >> 52) & 0x7ffull);
    const unsigned long long mant = b & ((1ull << 52) - 1ull);
    if (be != 0) return be - 1022;
    if (mant == 0ull) return LV_EMPTY;
    return -1010 - __clzll((long long)mant);
}

// ---- the filter passes -------------------------------------------------------------------------------------------------
// MODE 1: band filter from zero state, keeps the end state.
// MODE 2: band filter from the true state; ssq partial of the chunk; envelope from zero state, keeps its end state.
// MODE 3: both from their true states; the exponents into the workspace, the utterance's maximum by an integer atomic.
template <int MODE, bool LP>
__global__ __launch_bounds__(LV_ROWS) void levels_chunk_kernel(const float* __restrict__ samples, long long num_samples,
                                                               const long long* __restrict__ offsets, const long long* __restrict__ lens,
                                                               const long long* __restrict__ chunk_ptr, long long U, long long G,
                                                               const double* __restrict__ tab, int nz, double* state,
                                                               double* __restrict__ ssq_part, short* __restrict__ ews, int* emax) {
    __shared__ float tile[LV_ROWS][LV_TS + 1];
    __shared__ __attribute__((aligned(8))) short etile[MODE == 3 ? LV_ROWS : 1][LV_TS + 4];      // rows of 72 bytes: 8-byte reads
    __shared__ long long r_off[LV_ROWS], r_len[LV_ROWS], r_n0[LV_ROWS];
    __shared__ int r_w[LV_ROWS];
    __shared__ int w_max;
    const int lane = threadIdx.x;
    const long long g0 = (long long)blockIdx.x * LV_ROWS, g = g0 + lane;
    long long u = -1;
    int W = 0;
    r_off[lane] = 0;
    r_len[lane] = 0;
    r_n0[lane] = 0;
    if (lane == 0) w_max = 0;
    if (g < G) {
        u = utt_of_chunk(g, chunk_ptr, U);
        const Utt info = utt_info(u, offsets, lens, chunk_ptr, num_samples, G, nz);
        const long long c = g - info.cp0;
        if (info.ok && c >= 0 && c < info.nch) {
            const long long n0 = c * LV_CH;
            W = (int)(info.n - n0 < LV_CH ? info.n - n0 : LV_CH);
            r_off[lane] = info.off;
            r_len[lane] = info.len;
            r_n0[lane] = n0;
        }
    }
    r_w[lane] = W;
    __syncthreads();
    atomicMax(&w_max, W);
    // sections
    const double h_b0 = tab[LT_HP1], h_b1 = tab[LT_HP1 + 1], h_a1 = tab[LT_HP1 + 2];
    double q[2][5], lp[11];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        q[0][k] = tab[LT_BQ1 + k];
        q[1][k] = tab[LT_BQ2 + k];
    }
#pragma unroll
    for (int k = 0; k < 11; ++k) lp[k] = LP ? tab[LT_LP + k] : 0.0;
    const double e_b0 = tab[LT_ENV], e_a1 = tab[LT_ENV + 1], e_a2 = tab[LT_ENV + 2];
    constexpr int SB = LP ? 10 : 5;
    double z[SB], ze[2] = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < SB; ++k) z[k] = (MODE != 1 && W > 0) ? state[g * LV_SLOTS + k] : 0.0;
    if (MODE == 3 && W > 0) {
        ze[0] = state[g * LV_SLOTS + 10];
        ze[1] = state[g * LV_SLOTS + 11];
    }
    double ssq = 0.0;
    int me = LV_EMPTY;
    __syncthreads();
    const int rounds = (w_max + LV_TS - 1) / LV_TS;
    for (int t = 0; t < rounds; ++t) {
        __syncthreads();
        for (int r = lane / LV_LPR; r < LV_ROWS; r += LV_RPI) {     // row r of the tile: LV_TS consecutive samples of chunk g0 + r;
            const int col = (lane % LV_LPR) * 4;            // LV_LPR lanes per row, 4 samples each: LV_RPI rows per load instruction
            const long long n = r_n0[r] + (long long)t * LV_TS + col, len = r_len[r];
            const float* __restrict__ src = samples + r_off[r] + n;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};          // the appended zeros are never loaded
            if (n + 3 < len) {
                const float4u w4 = *reinterpret_cast<const float4u*>(src);      // rows start anywhere: 4-byte aligned only
                v[0] = w4.x; v[1] = w4.y; v[2] = w4.z; v[3] = w4.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (n + k < len) v[k] = src[k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) tile[r][col + k] = v[k];
        }
        __syncthreads();
        const int cnt = min(LV_TS, max(0, W - t * LV_TS));
        auto step = [&](float xf, int i) {
            const double x = (double)xf;
            // first-order section
            double y = h_b0 * x + z[0];
            z[0] = h_b1 * x - h_a1 * y;
            // two biquads
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const double v = y;
                y = q[s][0] * v + z[1 + 2 * s];
                z[1 + 2 * s] = (q[s][1] * v + z[2 + 2 * s]) - q[s][3] * y;
                z[2 + 2 * s] = q[s][2] * v - q[s][4] * y;
            }
            if (LP) {                                       // the 5th-order low-pass, one section
                const double v = y;
                y = lp[0] * v + z[SB - 5];
#pragma unroll
                for (int k = 1; k < 5; ++k) z[SB - 5 + k - 1] = (lp[k] * v + z[SB - 5 + k]) - lp[5 + k] * y;
                z[SB - 1] = lp[5] * v - lp[10] * y;
            }
            if (MODE >= 2) {
                if (MODE == 2) ssq = ssq + y * y;
                const double s = e_b0 * fabs(y) + ze[0];
                ze[0] = ze[1] - e_a1 * s;
                ze[1] = -(e_a2 * s);
                if (MODE == 3) {
                    const int e = exponent_of(s * s);
                    me = max(me, e);
                    etile[lane][i] = (short)e;
                }
            }
        };
        if (cnt == LV_TS) {                                 // a whole tile: the LDS reads of 8 samples ahead of their 8 steps
            for (int i0 = 0; i0 < LV_TS; i0 += 8) {
                float xv[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) xv[k] = tile[lane][i0 + k];
#pragma unroll
                for (int k = 0; k < 8; ++k) step(xv[k], i0 + k);
            }
        } else {
            for (int i = 0; i < cnt; ++i) step(tile[lane][i], i);
        }
        if (MODE == 3) {
            __syncthreads();
            for (int r = lane / LV_LPR; r < LV_ROWS; r += LV_RPI) {     // LV_LPR lanes per row, 4 exponents (8 aligned bytes) each
                const int col = (lane % LV_LPR) * 4, idx = t * LV_TS + col, w = r_w[r];
                short* __restrict__ dst = ews + (g0 + r) * LV_CH + idx;
                if (idx + 3 < w) {
                    *reinterpret_cast<short4v*>(dst) = *reinterpret_cast<const short4v*>(&etile[r][col]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (idx + k < w) dst[k] = etile[r][col + k];
                }
            }
        }
    }
    if (W > 0) {
        if (MODE == 1) {
#pragma unroll
            for (int k = 0; k < SB; ++k) state[g * LV_SLOTS + k] = z[k];
        }
        if (MODE == 2) {
            state[g * LV_SLOTS + 10] = ze[0];
            state[g * LV_SLOTS + 11] = ze[1];
            ssq_part[g] = ssq;
        }
        if (MODE == 3) atomicMax(&emax[u], me + 1);               // emax = max e + 1 = max h + 1
    }
}

// ---- the carry ---------------------------------------------------------------------------------------------------------
// 16 lanes per utterance, lane r < S owns component r of the state.  Slot c of the workspace holds z_c (the end state of chunk c
// run from zero) on entry and s_c (its true start state) on exit (a slot is loaded before it is stored to):
//     s_0 = 0;   s_{c+1}[r] = (((T[r][0] s_c[0] + T[r][1] s_c[1]) + ...) + T[r][S-1] s_c[S-1]) + z_c[r]
// INIT (band carry): lane 0 also writes the utterance's ns (or the flag) and clears its other outputs.
// SSQ (envelope carry): lane 15 also sums the chunks' ssq partials, chunks ascending.
template <int S, bool INIT, bool SSQ>
__global__ __launch_bounds__(64) void levels_carry_kernel(const long long* __restrict__ offsets, const long long* __restrict__ lens,
                                                          const long long* __restrict__ chunk_ptr, long long num_samples, long long U,
                                                          long long G, int nz, const double* __restrict__ T, double* state, int slot0,
                                                          const double* __restrict__ ssq_part, double* __restrict__ ssq_out,
                                                          long long* __restrict__ ns_out, int* __restrict__ emax,
                                                          long long* __restrict__ counts) {
    constexpr int BLK = 16;
    const int sub = threadIdx.x & 15;
    const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 4);
    if (u >= U) return;
    const Utt info = utt_info(u, offsets, lens, chunk_ptr, num_samples, G, nz);
    if (INIT && sub == 0) {
        ns_out[u] = info.ok ? info.n : -1;
        emax[u] = LV_EMPTY + 1;
        ssq_out[u] = 0.0;
        for (int j = 0; j < LV_NBIN; ++j) counts[u * LV_NBIN + j] = 0;
    }
    if (!info.ok) return;
    const bool mine = sub < S;
    double trow[S];
#pragma unroll
    for (int k = 0; k < S; ++k) trow[k] = mine ? T[sub * S + k] : 0.0;
    double s = 0.0, total = 0.0;
    double za[BLK], zb[BLK], pa[BLK], pb[BLK];             // two blocks of z_c (and ssq partials): one in use, one in flight
    double* const slot = state + info.cp0 * LV_SLOTS + slot0 + (mine ? sub : 0);
    const double* const part = SSQ ? ssq_part + info.cp0 : nullptr;
    auto load = [&](double (&zv)[BLK], double (&pv)[BLK], long long c0) {
#pragma unroll
        for (int j = 0; j < BLK; ++j) {
            const long long c = c0 + j;
            zv[j] = (mine && c < info.nch) ? slot[c * LV_SLOTS] : 0.0;
            pv[j] = (SSQ && sub == 15 && c < info.nch) ? part[c] : 0.0;
        }
    };
    auto run = [&](const double (&zv)[BLK], const double (&pv)[BLK], long long c0) {
#pragma unroll
        for (int j = 0; j < BLK; ++j) {
            const long long c = c0 + j;
            if (c < info.nch) {                             // uniform over the 16 lanes of an utterance
                if (mine) slot[c * LV_SLOTS] = s;
                double acc = trow[0] * __shfl(s, 0, 16);
#pragma unroll
                for (int k = 1; k < S; ++k) acc = acc + trow[k] * __shfl(s, k, 16);
                s = acc + zv[j];
                if (SSQ) total = total + pv[j];
            }
        }
    };
    // a block's loads are issued a whole block of the chain ahead of their use, and always before the stores to their own slots
    load(za, pa, 0);
    for (long long c0 = 0; c0 < info.nch; c0 += 2 * BLK) {
        load(zb, pb, c0 + BLK);
        run(za, pa, c0);
        load(za, pa, c0 + 2 * BLK);
        run(zb, pb, c0 + BLK);
    }
    if (SSQ && sub == 15) ssq_out[u] = total;
}

// ---- hangover and occupancy ----------------------------------------------------------------------------------------------
// max over the threads before this one of m (LV_EMPTY for thread 0): a wave scan by shuffles, then the waves' totals
__device__ __forceinline__ int block_max_before(int m, int* wtot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int v = m;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (lane >= d) v = max(v, o);
    }
    if (lane == 63) wtot[wave] = v;
    int before = __shfl_up(v, 1, 64);
    if (lane == 0) before = LV_EMPTY;
    __syncthreads();
    for (int k = 0; k < wave; ++k) before = max(before, wtot[k]);
    return before;
}

// In-place running maxima in LDS, 3 compares per element: of left[0 .. nl) from its END backwards and of right[0 .. nr) forwards.
// Every thread scans its own run of each, the runs' totals are scanned across the workgroup, then every run takes what came
// before it.
__device__ __forceinline__ void scan_max_pair(short* left, int nl, short* right, int nr, int* wtot) {
    const int tid = threadIdx.x;
    const int segl = (nl + LV_HANG_NT - 1) / LV_HANG_NT, segr = (nr + LV_HANG_NT - 1) / LV_HANG_NT;
    const int lo_l = min(nl, tid * segl), hi_l = min(nl, lo_l + segl);
    const int lo_r = min(nr, tid * segr), hi_r = min(nr, lo_r + segr);
    int ml = LV_EMPTY, mr = LV_EMPTY;
    for (int i = lo_l; i < hi_l; ++i) {
        ml = max(ml, (int)left[nl - 1 - i]);
        left[nl - 1 - i] = (short)ml;
    }
    for (int i = lo_r; i < hi_r; ++i) {
        mr = max(mr, (int)right[i]);
        right[i] = (short)mr;
    }
    const int bl = block_max_before(ml, wtot), br = block_max_before(mr, wtot + LV_HANG_NT / 64);
    for (int i = lo_l; i < hi_l; ++i) left[nl - 1 - i] = (short)max((int)left[nl - 1 - i], bl);
    for (int i = lo_r; i < hi_r; ++i) right[i] = (short)max((int)right[i], br);
    __syncthreads();
}

// One workgroup per chunk: h[n] = max e[n - nh + 1 .. n] for the chunk's samples [n0, n0 + W), split at n0 (van Herk): the running
// maximum backwards over the nh - 1 samples before n0 and forwards over the chunk.  Then bin j = min(emax - h, 20).
// One split is enough because nh >= LV_CH (the entry point refuses less): every window of the chunk reaches back to n0 or
// beyond it (or to sample 0 in the first chunk), so the forward maximum from n0 never covers a sample outside the window.
__global__ __launch_bounds__(LV_HANG_NT) void levels_hang_kernel(const long long* __restrict__ offsets, const long long* __restrict__ lens,
                                                                 const long long* __restrict__ chunk_ptr, long long num_samples,
                                                                 long long U, long long G, int nz, int nh, const short* __restrict__ ews,
                                                                 const int* __restrict__ emax, unsigned long long* __restrict__ counts) {
    __shared__ short buf[LV_NH_MAX - 1 + LV_CH];
    __shared__ int wtot[2 * LV_HANG_NT / 64];
    __shared__ unsigned hist[LV_NBIN];
    const int tid = threadIdx.x;
    const long long g = blockIdx.x;
    const long long u = utt_of_chunk(g, chunk_ptr, U);
    const Utt info = utt_info(u, offsets, lens, chunk_ptr, num_samples, G, nz);
    const long long c = g - info.cp0;
    if (!info.ok || c < 0 || c >= info.nch) return;         // uniform over the workgroup
    const long long n0 = c * LV_CH;
    const int W = (int)(info.n - n0 < LV_CH ? info.n - n0 : LV_CH);
    const long long left0 = n0 - (nh - 1) > 0 ? n0 - (nh - 1) : 0;
    const int Lh = (int)(n0 - left0);                       // <= nh - 1 <= LV_NH_MAX - 1
    const short* __restrict__ e = ews + info.cp0 * LV_CH + left0;
    for (int i = tid; i < Lh + W; i += LV_HANG_NT) buf[i] = e[i];
    if (tid < LV_NBIN) hist[tid] = 0u;
    __syncthreads();
    scan_max_pair(buf, Lh, buf + Lh, W, wtot);
    const int top = emax[u];
    for (int i = tid; i < W; i += LV_HANG_NT) {
        int h = buf[Lh + i];
        const long long lo = n0 + i - (nh - 1);             // first sample of the window, clipped to the utterance
        if (lo < n0 && Lh > 0) h = max(h, (int)buf[lo > left0 ? (int)(lo - left0) : 0]);
        atomicAdd(&hist[min(top - h, LV_NBIN) - 1], 1u);
    }
    __syncthreads();
    if (tid < LV_NBIN && hist[tid] != 0u) atomicAdd(&counts[u * LV_NBIN + tid], (unsigned long long)hist[tid]);
}

template <bool LP>
int levels_launch(const float* samples, long long num_samples, const long long* offsets, const long long* lens, const long long* chunk_ptr,
                  long long U, long long G, const double* tab, int nz, int nh, double* ssq, long long* ns, int* emax, long long* counts,
                  double* state, double* ssq_part, short* ews, hipStream_t st) {
    constexpr int SB = LP ? 10 : 5;
    const dim3 cgrid((unsigned)ctn_cdivll(G, LV_ROWS)), ugrid((unsigned)ctn_cdivll(U, 4));
    levels_chunk_kernel<1, LP><<<cgrid, dim3(LV_ROWS), 0, st>>>(samples, num_samples, offsets, lens, chunk_ptr, U, G, tab, nz, state,
                                                               ssq_part, ews, emax);
    CTN_CHECK_LAUNCH("ctn_active_level (band pass 1)");
    levels_carry_kernel<SB, true, false><<<ugrid, dim3(64), 0, st>>>(offsets, lens, chunk_ptr, num_samples, U, G, nz, tab + LT_TBAND, state,
                                                                     0, ssq_part, ssq, ns, emax, counts);
    CTN_CHECK_LAUNCH("ctn_active_level (band carry)");
    levels_chunk_kernel<2, LP><<<cgrid, dim3(LV_ROWS), 0, st>>>(samples, num_samples, offsets, lens, chunk_ptr, U, G, tab, nz, state,
                                                               ssq_part, ews, emax);
    CTN_CHECK_LAUNCH("ctn_active_level (band pass 2, envelope pass 1)");
    levels_carry_kernel<2, false, true><<<ugrid, dim3(64), 0, st>>>(offsets, lens, chunk_ptr, num_samples, U, G, nz, tab + LT_TENV, state,
                                                                    10, ssq_part, ssq, ns, emax, counts);
    CTN_CHECK_LAUNCH("ctn_active_level (envelope carry)");
    levels_chunk_kernel<3, LP><<<cgrid, dim3(LV_ROWS), 0, st>>>(samples, num_samples, offsets, lens, chunk_ptr, U, G, tab, nz, state,
                                                               ssq_part, ews, emax);
    CTN_CHECK_LAUNCH("ctn_active_level (envelope pass 2)");
    levels_hang_kernel<<<dim3((unsigned)G), dim3(LV_HANG_NT), 0, st>>>(offsets, lens, chunk_ptr, num_samples, U, G, nz, nh, ews, emax,
                                                                        (unsigned long long*)counts);
    CTN_CHECK_LAUNCH("ctn_active_level (hangover)");
    return CTN_OK;
}

}  // namespace

extern "C" {

int ctn_active_level_chunk(void) { return LV_CH; }

size_t ctn_active_level_workspace(long long total_chunks, long long U) {
    if (total_chunks < 1 || U < 1) return 0;
    return (size_t)total_chunks * (sizeof(double) * (LV_SLOTS + 1) + sizeof(short) * LV_CH);
}

int ctn_active_level(const float* samples, long long num_samples, const long long* offsets, const long long* lens,
                     const long long* chunk_ptr, long long U, long long total_chunks, const double* table, int use_lp, int nz, int nh,
                     double* ssq, long long* ns, int* emax, long long* counts, void* workspace, size_t workspace_bytes, void* stream) {
    CTN_REQUIRE(samples && offsets && lens && chunk_ptr && table && ssq && ns && emax && counts && workspace,
                "ctn_active_level: null pointer");
    CTN_REQUIRE(num_samples >= 1, "ctn_active_level: num_samples = %lld", num_samples);
    CTN_REQUIRE(U >= 1 && U <= 0x7fffffffLL, "ctn_active_level: U = %lld utterances (1 .. 2^31 - 1)", U);
    CTN_REQUIRE(total_chunks >= U && total_chunks <= LV_G_MAX, "ctn_active_level: total_chunks = %lld for %lld utterances (U .. 2^24 - 1)",
                total_chunks, U);
    CTN_REQUIRE(use_lp == 0 || use_lp == 1, "ctn_active_level: use_lp = %d (0 or 1)", use_lp);
    CTN_REQUIRE(nz >= 0 && nz <= (1 << 20), "ctn_active_level: nz = %d appended zeros (0 .. 2^20)", nz);
    CTN_REQUIRE(nh >= LV_NH_MIN && nh <= LV_NH_MAX, "ctn_active_level: nh = %d hangover samples (%d .. %d: a window spans a chunk)", nh,
                LV_NH_MIN, LV_NH_MAX);
    CTN_REQUIRE(((size_t)workspace & 7) == 0, "ctn_active_level: the workspace must be 8-byte aligned");
    if (workspace_bytes < ctn_active_level_workspace(total_chunks, U)) {
        ctn_set_error("ctn_active_level: workspace of %zu bytes, %zu needed", workspace_bytes, ctn_active_level_workspace(total_chunks, U));
        return CTN_ERR_WORKSPACE;
    }
    double* const state = (double*)workspace;
    double* const ssq_part = state + (size_t)total_chunks * LV_SLOTS;
    short* const ews = (short*)(ssq_part + total_chunks);
    const hipStream_t st = (hipStream_t)stream;
    if (use_lp)
        return levels_launch<true>(samples, num_samples, offsets, lens, chunk_ptr, U, total_chunks, table, nz, nh, ssq, ns, emax, counts,
                                   state, ssq_part, ews, st);
    return levels_launch<false>(samples, num_samples, offsets, lens, chunk_ptr, U, total_chunks, table, nz, nh, ssq, ns, emax, counts,
                                state, ssq_part, ews, st);
}

}  // extern "C"
