// ITU-R BS.1770-4 integrated loudness (mono) of ragged utterances: the K-weighting, the 400 ms blocks at 75 % overlap and both
// gates, all on the device.  Contract: include/ctn_hip.h ("integrated loudness"); executable restatement: tests/loudness_oracle.py.
// The K-weighting is linear, so every utterance is cut into chunks of LD_CH samples by its own sample index, as the P.56 meter does
// (ctn_levels.hip): pass 1 runs every chunk from zero state, a carry per utterance turns the end states into true start states
// (s_{c+1} = T s_c + z_c, T = A^CH from the host), pass 2 reruns every chunk from its true state and sums y y over the pieces the
// 100 ms sub-blocks cut it into.  One lane per chunk; a wave stages 64 chunks x 32 samples through LDS so that the global loads are
// whole rows.  The last launch, one wave per utterance, forms the blocks and gates them in the power domain.
// Every fp64 product and sum is ONE rounding in the written order (no contraction), the counts are integers, no atomics: the
// statistics of an utterance are a bitwise function of its own samples, the table, h and LD_CH.
#include "ctn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int LD_CH = 1024;           // samples per chunk (ctn_loudness_chunk)
constexpr int LD_TS = 32;             // samples of every chunk staged per round (8.4 KB of LDS per wave: several waves per SIMD)
constexpr int LD_LPR = LD_TS / 4;     // lanes per staged row (4 samples each)
constexpr int LD_RPI = 64 / LD_LPR;   // rows per load instruction
constexpr int LD_ROWS = 64;           // chunks per workgroup of the filter passes: one wave, one lane per chunk
constexpr int LD_NP = 3;              // pieces of a chunk: a chunk meets at most 3 sub-blocks while 2 h + 2 > LD_CH
constexpr int LD_H_MIN = 800, LD_H_MAX = 4800;       // the 100 ms hop at 8 and 48 kHz
static_assert(2 * LD_H_MIN + 2 > LD_CH, "a chunk must not meet more than LD_NP sub-blocks");
constexpr int LD_SLOTS = 4 + LD_NP;   // fp64 words per chunk in the workspace: 4 filter states, LD_NP piece sums
constexpr long long LD_G_MAX = (1ll << 31) - 1 - LD_ROWS;
// the table (fp64): the two biquads (b0 b1 b2 a1 a2), the transition matrix, the absolute gate as a power
constexpr int LT_SHELF = 0, LT_HP = 5, LT_T = 10, LT_GATE = 26, LT_SIZE = 27;

typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));       // four samples from a 4-byte aligned address

struct Utt {
    long long off, len, cp0, nch;
    bool ok;
};

// An utterance whose samples lie inside the buffer and whose chunk range is the one its length asks for; anything else is
// flagged and never read.
__device__ __forceinline__ Utt utt_info(long long u, const long long* __restrict__ offsets, const long long* __restrict__ lens,
                                        const long long* __restrict__ chunk_ptr, long long num_samples, long long G) {
    Utt r;
    r.off = offsets[u];
    r.len = lens[u];
    r.cp0 = chunk_ptr[u];
    const long long cp1 = chunk_ptr[u + 1];
    r.ok = r.off >= 0 && r.len >= 0 && r.len <= num_samples && r.off <= num_samples - r.len;
    r.nch = r.ok ? (r.len + LD_CH - 1) / LD_CH : 0;
    r.ok = r.ok && r.cp0 >= 0 && cp1 <= G && cp1 - r.cp0 == r.nch;
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

// ---- the filter passes -------------------------------------------------------------------------------------------------
// MODE 1: K-weighting from zero state, keeps the end state.
// MODE 2: from the true state; the sums of y y over the chunk's pieces.
template <int MODE>
__global__ __launch_bounds__(LD_ROWS) void loudness_chunk_kernel(const float* __restrict__ samples, long long num_samples,
                                                                 const long long* __restrict__ offsets, const long long* __restrict__ lens,
                                                                 const long long* __restrict__ chunk_ptr, long long U, long long G,
                                                                 const double* __restrict__ tab, int h, double* ws) {
    __shared__ float tile[LD_ROWS][LD_TS + 1];
    __shared__ long long r_off[LD_ROWS], r_len[LD_ROWS], r_n0[LD_ROWS];
    __shared__ int w_max;
    const int lane = threadIdx.x;
    const long long g0 = (long long)blockIdx.x * LD_ROWS, g = g0 + lane;
    int W = 0, b1 = LD_CH, b2 = LD_CH;
    r_off[lane] = 0;
    r_len[lane] = 0;
    r_n0[lane] = 0;
    if (lane == 0) w_max = 0;
    if (g < G) {
        const long long u = utt_of_chunk(g, chunk_ptr, U);
        const Utt info = utt_info(u, offsets, lens, chunk_ptr, num_samples, G);
        const long long c = g - info.cp0;
        if (info.ok && c >= 0 && c < info.nch) {
            const long long n0 = c * LD_CH;
            W = (int)(info.len - n0 < LD_CH ? info.len - n0 : LD_CH);
            b1 = h - (int)(n0 % h);                         // the chunk's first sample of its second and third sub-block
            b2 = b1 + h;
            r_off[lane] = info.off;
            r_len[lane] = info.len;
            r_n0[lane] = n0;
        }
    }
    __syncthreads();
    atomicMax(&w_max, W);                                   // LDS, an integer maximum: order-free
    double q[2][5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        q[0][k] = tab[LT_SHELF + k];
        q[1][k] = tab[LT_HP + k];
    }
    double z[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) z[k] = (MODE == 2 && W > 0) ? ws[g * LD_SLOTS + k] : 0.0;
    double acc = 0.0, p0 = 0.0, p1 = 0.0, p2 = 0.0;
    __syncthreads();
    const int rounds = (w_max + LD_TS - 1) / LD_TS;
    for (int t = 0; t < rounds; ++t) {
        __syncthreads();
        for (int r = lane / LD_LPR; r < LD_ROWS; r += LD_RPI) {     // row r of the tile: LD_TS consecutive samples of chunk g0 + r;
            const int col = (lane % LD_LPR) * 4;            // LD_LPR lanes per row, 4 samples each: LD_RPI rows per load instruction
            const long long n = r_n0[r] + (long long)t * LD_TS + col, len = r_len[r];
            const float* __restrict__ src = samples + r_off[r] + n;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
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
        const int cnt = min(LD_TS, max(0, W - t * LD_TS));
        auto step = [&](float xf, int pos) {
            double y = (double)xf;
#pragma unroll
            for (int s = 0; s < 2; ++s) {                   // shelf, then high-pass: direct form II transposed
                const double v = y;
                y = q[s][0] * v + z[2 * s];
                z[2 * s] = (q[s][1] * v + z[2 * s + 1]) - q[s][3] * y;
                z[2 * s + 1] = q[s][2] * v - q[s][4] * y;
            }
            if (MODE == 2) {
                if (pos == b1) { p0 = acc; acc = 0.0; }
                if (pos == b2) { p1 = acc; acc = 0.0; }
                acc = acc + y * y;
            }
        };
        if (cnt == LD_TS) {                                 // a whole tile: the LDS reads of 8 samples ahead of their 8 steps
            for (int i0 = 0; i0 < LD_TS; i0 += 8) {
                float xv[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) xv[k] = tile[lane][i0 + k];
#pragma unroll
                for (int k = 0; k < 8; ++k) step(xv[k], t * LD_TS + i0 + k);
            }
        } else {
            for (int i = 0; i < cnt; ++i) step(tile[lane][i], t * LD_TS + i);
        }
    }
    if (W > 0) {
        if (MODE == 1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) ws[g * LD_SLOTS + k] = z[k];
        } else {
            if (W - 1 < b1) p0 = acc; else if (W - 1 < b2) p1 = acc; else p2 = acc;      // the piece of the last sample
            ws[g * LD_SLOTS + 4] = p0;
            ws[g * LD_SLOTS + 5] = p1;
            ws[g * LD_SLOTS + 6] = p2;
        }
    }
}

// ---- the carry ---------------------------------------------------------------------------------------------------------
// 4 lanes per utterance, lane r owns component r of the state.  Slot c of the workspace holds z_c (the end state of chunk c run
// from zero) on entry and s_c (its true start state) on exit (a slot is loaded before it is stored to):
//     s_0 = 0;   s_{c+1}[r] = (((T[r][0] s_c[0] + T[r][1] s_c[1]) + T[r][2] s_c[2]) + T[r][3] s_c[3]) + z_c[r]
__global__ __launch_bounds__(64) void loudness_carry_kernel(const long long* __restrict__ offsets, const long long* __restrict__ lens,
                                                            const long long* __restrict__ chunk_ptr, long long num_samples, long long U,
                                                            long long G, const double* __restrict__ T, double* ws) {
    constexpr int BLK = 16;
    const int sub = threadIdx.x & 3;
    const long long u = (long long)blockIdx.x * 16 + (threadIdx.x >> 2);
    if (u >= U) return;
    const Utt info = utt_info(u, offsets, lens, chunk_ptr, num_samples, G);
    if (!info.ok) return;
    double trow[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) trow[k] = T[sub * 4 + k];
    double s = 0.0;
    double za[BLK], zb[BLK];                                // two blocks of z_c: one in use, one in flight
    double* const slot = ws + info.cp0 * LD_SLOTS + sub;
    auto load = [&](double (&zv)[BLK], long long c0) {
#pragma unroll
        for (int j = 0; j < BLK; ++j) zv[j] = c0 + j < info.nch ? slot[(c0 + j) * LD_SLOTS] : 0.0;
    };
    auto run = [&](const double (&zv)[BLK], long long c0) {
#pragma unroll
        for (int j = 0; j < BLK; ++j) {
            if (c0 + j < info.nch) {                        // uniform over the 4 lanes of an utterance
                slot[(c0 + j) * LD_SLOTS] = s;
                double acc = trow[0] * __shfl(s, 0, 4);
#pragma unroll
                for (int k = 1; k < 4; ++k) acc = acc + trow[k] * __shfl(s, k, 4);
                s = acc + zv[j];
            }
        }
    };
    // a block's loads are issued a whole block of the chain ahead of their use, and always before the stores to their own slots
    load(za, 0);
    for (long long c0 = 0; c0 < info.nch; c0 += 2 * BLK) {
        load(zb, c0 + BLK);
        run(za, c0);
        load(za, c0 + 2 * BLK);
        run(zb, c0 + BLK);
    }
}

// ---- blocks and gates ----------------------------------------------------------------------------------------------------
// S_i of sub-block i (samples [i h, (i + 1) h)): its pieces, chunks ascending
__device__ __forceinline__ double sub_block(const double* __restrict__ wsu, long long i, int h) {
    const long long c_lo = i * h / LD_CH, c_hi = ((i + 1) * h - 1) / LD_CH;
    double s = 0.0;
    for (long long c = c_lo; c <= c_hi; ++c) s = s + wsu[c * LD_SLOTS + 4 + (int)(i - c * LD_CH / h)];
    return s;
}

__device__ __forceinline__ double block_power(const double* __restrict__ wsu, long long j, int h, double n) {
    const double s = ((sub_block(wsu, j, h) + sub_block(wsu, j + 1, h)) + sub_block(wsu, j + 2, h)) + sub_block(wsu, j + 3, h);
    return s / n;
}

// lanes ascending: ((v_0 + v_1) + v_2) + ... + v_63, the same value in every lane
__device__ __forceinline__ double lanes_in_order(double v) {
    double t = __shfl(v, 0, 64);
    for (int k = 1; k < 64; ++k) t = t + __shfl(v, k, 64);
    return t;
}

__device__ __forceinline__ long long wave_count(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave per utterance.  Lane l sums the blocks j = l, l + 64, ... in ascending order, then the lanes are summed in ascending
// order: an order fixed by the block index.  Two rounds: all blocks and the absolute gate, then the relative gate.
__global__ __launch_bounds__(64) void loudness_gate_kernel(const long long* __restrict__ offsets, const long long* __restrict__ lens,
                                                           const long long* __restrict__ chunk_ptr, long long num_samples, long long U,
                                                           long long G, const double* __restrict__ tab, int h, const double* __restrict__ ws,
                                                           long long* __restrict__ ns, long long* __restrict__ n_blocks,
                                                           long long* __restrict__ n_abs, long long* __restrict__ n_rel,
                                                           double* __restrict__ sum_all, double* __restrict__ sum_abs,
                                                           double* __restrict__ sum_rel) {
    const long long u = blockIdx.x;
    const int lane = threadIdx.x;
    const Utt info = utt_info(u, offsets, lens, chunk_ptr, num_samples, G);
    const long long nsub = info.ok ? info.len / h : 0, nb = nsub >= 4 ? nsub - 3 : 0;
    const double* __restrict__ wsu = ws + (info.ok ? info.cp0 : 0) * LD_SLOTS;
    const double n = (double)(4 * h), gate = tab[LT_GATE];
    double a_all = 0.0, a_abs = 0.0;
    long long c_abs = 0;
    for (long long j = lane; j < nb; j += 64) {
        const double zj = block_power(wsu, j, h, n);
        a_all = a_all + zj;
        if (zj > gate) {
            a_abs = a_abs + zj;
            ++c_abs;
        }
    }
    a_all = lanes_in_order(a_all);
    a_abs = lanes_in_order(a_abs);
    c_abs = wave_count(c_abs);
    double a_rel = 0.0;
    long long c_rel = 0;
    if (c_abs > 0) {                                        // uniform over the wave
        const double rel = (a_abs / (double)c_abs) / 10.0;
        for (long long j = lane; j < nb; j += 64) {
            const double zj = block_power(wsu, j, h, n);
            if (zj > gate && zj > rel) {
                a_rel = a_rel + zj;
                ++c_rel;
            }
        }
    }
    a_rel = lanes_in_order(a_rel);
    c_rel = wave_count(c_rel);
    if (lane == 0) {
        ns[u] = info.ok ? info.len : -1;
        n_blocks[u] = nb;
        n_abs[u] = c_abs;
        n_rel[u] = c_rel;
        sum_all[u] = a_all;
        sum_abs[u] = a_abs;
        sum_rel[u] = a_rel;
    }
}

}  // namespace

extern "C" {

int ctn_loudness_chunk(void) { return LD_CH; }

size_t ctn_loudness_workspace(long long total_chunks, long long U) {
    if (total_chunks < 0 || U < 1) return 0;
    return (size_t)total_chunks * sizeof(double) * LD_SLOTS;
}

int ctn_loudness(const float* samples, long long num_samples, const long long* offsets, const long long* lens,
                 const long long* chunk_ptr, long long U, long long total_chunks, const double* table, int hop, long long* ns,
                 long long* n_blocks, long long* n_abs, long long* n_rel, double* sum_all, double* sum_abs, double* sum_rel,
                 void* workspace, size_t workspace_bytes, void* stream) {
    CTN_REQUIRE(samples && offsets && lens && chunk_ptr && table && ns && n_blocks && n_abs && n_rel && sum_all && sum_abs && sum_rel,
                "ctn_loudness: null pointer");
    CTN_REQUIRE(num_samples >= 1, "ctn_loudness: num_samples = %lld", num_samples);
    CTN_REQUIRE(U >= 1 && U <= 0x7fffffffLL, "ctn_loudness: U = %lld utterances (1 .. 2^31 - 1)", U);
    CTN_REQUIRE(total_chunks >= 0 && total_chunks <= LD_G_MAX, "ctn_loudness: total_chunks = %lld (0 .. 2^31 - 65)", total_chunks);
    CTN_REQUIRE(hop >= LD_H_MIN && hop <= LD_H_MAX, "ctn_loudness: hop = %d samples of 100 ms (%d .. %d: 8 .. 48 kHz)", hop, LD_H_MIN,
                LD_H_MAX);
    CTN_REQUIRE(total_chunks == 0 || workspace != nullptr, "ctn_loudness: null workspace");
    CTN_REQUIRE(((size_t)workspace & 7) == 0, "ctn_loudness: the workspace must be 8-byte aligned");
    if (workspace_bytes < ctn_loudness_workspace(total_chunks, U)) {
        ctn_set_error("ctn_loudness: workspace of %zu bytes, %zu needed", workspace_bytes, ctn_loudness_workspace(total_chunks, U));
        return CTN_ERR_WORKSPACE;
    }
    double* const ws = (double*)workspace;
    const hipStream_t st = (hipStream_t)stream;
    const long long G = total_chunks;
    if (G > 0) {
        const dim3 cgrid((unsigned)ctn_cdivll(G, LD_ROWS));
        loudness_chunk_kernel<1><<<cgrid, dim3(LD_ROWS), 0, st>>>(samples, num_samples, offsets, lens, chunk_ptr, U, G, table, hop, ws);
        CTN_CHECK_LAUNCH("ctn_loudness (pass 1)");
        loudness_carry_kernel<<<dim3((unsigned)ctn_cdivll(U, 16)), dim3(64), 0, st>>>(offsets, lens, chunk_ptr, num_samples, U, G,
                                                                                      table + LT_T, ws);
        CTN_CHECK_LAUNCH("ctn_loudness (carry)");
        loudness_chunk_kernel<2><<<cgrid, dim3(LD_ROWS), 0, st>>>(samples, num_samples, offsets, lens, chunk_ptr, U, G, table, hop, ws);
        CTN_CHECK_LAUNCH("ctn_loudness (pass 2)");
    }
    loudness_gate_kernel<<<dim3((unsigned)U), dim3(64), 0, st>>>(offsets, lens, chunk_ptr, num_samples, U, G, table, hop, ws, ns, n_blocks,
                                                                 n_abs, n_rel, sum_all, sum_abs, sum_rel);
    CTN_CHECK_LAUNCH("ctn_loudness (gates)");
    return CTN_OK;
}

}  // extern "C"
