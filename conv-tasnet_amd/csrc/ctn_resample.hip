// On-device sinc resampling: a Kaiser-windowed-sinc polyphase resampler for ragged batches in device memory, and the
// speed-perturbed segments of the dynamic mixer, which are the same sum started at plan_start.
// Contract: include/ctn_hip.h ("on-device sinc resampling"); executable restatement: tests/resample_oracle.py.
// Every product and every add of the tap sum is ONE float32 rounding in ascending tap order (no contraction into fused
// multiply-adds), so an output is a bitwise function of the table and the input, whatever the launch geometry.
#include "ctn_common.h"

#pragma clang fp contract(off)

namespace {

// One rounding each.  Written here, under the pragma above, in plain operators: __fmul_rn / __fadd_rn are inline functions of a
// header compiled under the default contraction mode, and a product whose only use is the add behind it is fused there.
__device__ __forceinline__ float rs_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float rs_add(float a, float b) { return a + b; }

constexpr int RS_NT = 256;                 // threads per workgroup
constexpr int RS_CHUNK = 4 * RS_NT;        // most outputs of one row per workgroup (4 per thread, RS_NT apart: 256-byte stores per wave)
constexpr int RS_LDS_BYTES = 60 * 1024;    // dynamic LDS of one workgroup at most: the input span, then the filter bank when it fits
constexpr int RS_MAX_TERM = 1 << 20;       // up, down <= 2^20: (up - 1) + 1023 * down stays below 2^31
constexpr long long RS_MAX_LEN = 1LL << 40;
constexpr int RS_PCT_LO = 50, RS_PCT_HI = 200;

// LDS floats of the input span of `chunk` consecutive outputs: the last output's first tap is at most
// floor((up - 1 + (chunk - 1) * down) / up) samples behind the first output's, and every output reads 2W samples
__host__ __device__ inline long long rs_span(int up, int down, int W, int chunk) {
    return ((long long)(up - 1) + (long long)(chunk - 1) * down) / up + 2LL * W;
}

// outputs [0, n) of one chunk from the staged span xs; output lt reads xs[di + j] * hb[ph * hstride + j], j = 0 .. 2W - 1,
// (di, ph) = divmod(r0 + lt * down, up).  Idle lanes recompute output 0 and drop it (every address stays inside the span).
__device__ __forceinline__ void rs_taps(const float* __restrict__ xs, const float* __restrict__ hb, int hstride, unsigned up, unsigned down,
                                        int W, unsigned r0, int n, float* __restrict__ yrow) {
    for (int base = 0; base < n; base += 4 * RS_NT) {
        const float* xp[4];
        const float* hp[4];
        float acc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int lt = base + (int)threadIdx.x + k * RS_NT;
            const unsigned a = r0 + (unsigned)(lt < n ? lt : 0) * down;
            const unsigned di = a / up, ph = a - di * up;
            xp[k] = xs + di;
            hp[k] = hb + (size_t)ph * hstride;
            acc[k] = 0.0f;
        }
        for (int j = 0; j < 2 * W; ++j) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = rs_add(acc[k], rs_mul(hp[k][j], xp[k][j]));
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int lt = base + (int)threadIdx.x + k * RS_NT;
            if (lt < n) yrow[lt] = acc[k];
        }
    }
}

// outputs [t0, t0 + n) of one row: y[t] = sum_j h[phi][j] * x[base + i + j - W + 1], x outside [0, len) of its row reads as zero.
// lds: `span` floats for the input, then up * (2W + 1) for the bank when bank_lds (row stride 2W + 1: an odd number of words,
// so lanes on different phase rows fall on different banks).
__device__ __forceinline__ void rs_chunk(const float* __restrict__ xrow, long long len, long long base, int up, int down,
                                         const float* __restrict__ h, int W, bool bank_lds, int span, float* lds, float* __restrict__ yrow,
                                         long long t0, int n) {
    const long long p = t0 * down, q0 = p / up;
    const unsigned r0 = (unsigned)(p - q0 * up);
    float* const xs = lds;
    float* const hs = lds + span;
    const long long g0 = base + q0 - W + 1;
    for (int k = threadIdx.x; k < span; k += RS_NT) {
        const long long g = g0 + k;
        xs[k] = (g >= 0 && g < len) ? xrow[g] : 0.0f;
    }
    if (bank_lds) {
        const int taps = 2 * W, total = up * taps;
        for (int idx = threadIdx.x; idx < total; idx += RS_NT) {
            const int ph = idx / taps;
            hs[ph * (taps + 1) + (idx - ph * taps)] = h[idx];
        }
    }
    __syncthreads();
    if (bank_lds)
        rs_taps(xs, hs, 2 * W + 1, (unsigned)up, (unsigned)down, W, r0, n, yrow + t0);
    else
        rs_taps(xs, h, 2 * W, (unsigned)up, (unsigned)down, W, r0, n, yrow + t0);
}

// ---- ragged rows ---------------------------------------------------------------------------------------------------------
// workgroup id = row * nchunk + chunk.  A row whose tables break their contract is flagged and neither read nor written.
__global__ __launch_bounds__(RS_NT) void resample_ragged_kernel(const float* __restrict__ x, long long x_samples,
                                                                const long long* __restrict__ in_offsets,
                                                                const long long* __restrict__ in_lens, int up, int down,
                                                                const float* __restrict__ h, int W, float* __restrict__ y, long long y_samples,
                                                                const long long* __restrict__ out_offsets,
                                                                const long long* __restrict__ out_lens, int nchunk, int chunk, int span,
                                                                int bank_lds, int* __restrict__ status) {
    extern __shared__ float rs_lds[];
    const long long row = blockIdx.x / (unsigned)nchunk;
    const int ch = (int)(blockIdx.x - (unsigned)row * (unsigned)nchunk);
    const long long io = in_offsets[row], ni = in_lens[row], oo = out_offsets[row], no = out_lens[row];
    const bool ok = io >= 0 && ni >= 1 && ni <= RS_MAX_LEN && ni <= x_samples && io <= x_samples - ni && oo >= 0 && no >= 0 &&
                    no <= y_samples && oo <= y_samples - no && no == (ni * up + down - 1) / down;
    if (ch == 0 && threadIdx.x == 0 && status != nullptr) status[row] = ok ? 0 : -1;
    if (!ok) return;
    const long long t0 = (long long)ch * chunk;
    if (t0 >= no) return;
    const int n = (int)(no - t0 < (long long)chunk ? no - t0 : (long long)chunk);
    rs_chunk(x + io, ni, 0, up, down, h, W, bank_lds != 0, span, rs_lds, y + oo, t0, n);
}

// ---- speed-perturbed segments of the dynamic mixer -----------------------------------------------------------------------
// grid (ceil(T / RS_CHUNK), B * C).  bank_tab row pct - 50 = (up, down, W, offset into banks); W = 0: not configured.
__global__ __launch_bounds__(RS_NT) void dynmix_speed_segments_kernel(const float* __restrict__ corpus, const long long* __restrict__ offsets,
                                                                      const long long* __restrict__ lens, int U,
                                                                      const int* __restrict__ plan_utt, const long long* __restrict__ plan_start,
                                                                      const int* __restrict__ plan_pct, int T, const float* __restrict__ banks,
                                                                      long long bank_floats, const int* __restrict__ bank_tab, int span_cap,
                                                                      int bank_cap, float* __restrict__ seg, int* __restrict__ seg_utt) {
    extern __shared__ float rs_lds[];
    const int o = blockIdx.y;
    const int t0 = blockIdx.x * RS_CHUNK;
    const int n = min(RS_CHUNK, T - t0);
    float* const yrow = seg + (long long)o * T;
    const int u = plan_utt[o], pct = plan_pct[o];
    const long long st = plan_start[o];
    bool ok = u >= 0 && u < U && st >= 0 && pct >= RS_PCT_LO && pct <= RS_PCT_HI;
    int up = 1, down = 1, W = 0;
    long long boff = 0;
    if (ok) {
        const long long need = ((long long)T * pct + 99) / 100;
        ok = st + need <= lens[u];
    }
    if (ok && pct != 100) {
        const int* row = bank_tab + 4 * (pct - RS_PCT_LO);
        up = row[0]; down = row[1]; W = row[2]; boff = row[3];
        ok = W >= 1 && up >= 1 && down >= 1 && up <= RS_MAX_TERM && down <= RS_MAX_TERM && boff >= 0 &&
             boff + (long long)up * 2 * W <= bank_floats && rs_span(up, down, W, RS_CHUNK) <= (long long)span_cap;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) seg_utt[o] = ok ? o : -1;   // the gather flags -1 entries: peak[b] = -1
    if (!ok) {                                                            // never read: the segment is silence
        for (int lt = threadIdx.x; lt < n; lt += RS_NT) yrow[t0 + lt] = 0.0f;
        return;
    }
    const float* __restrict__ xrow = corpus + offsets[u];
    if (pct == 100) {                                                     // a plain copy
        for (int lt = threadIdx.x; lt < n; lt += RS_NT) yrow[t0 + lt] = xrow[st + t0 + lt];
        return;
    }
    const int span = (int)rs_span(up, down, W, RS_CHUNK);
    const bool bank_lds = (long long)up * (2 * W + 1) <= (long long)bank_cap;
    rs_chunk(xrow, lens[u], st, up, down, banks + boff, W, bank_lds, span, rs_lds, yrow, t0, n);
}

// ---- streaming rows: the same sum over a signal that arrives push by push -------------------------------------------------
// tab row (int64 [RS_STAB]): n_old, n_new, t0, n_out, src, dst, parity, spare (include/ctn_hip.h, "streaming sinc resampling").
// Global sample g of a row: zero for g < 0 and g >= n_old + n_new, the chunk for g >= n_old, else the row's history of the last
// 2W - 1 samples.  hist [2][rows][2W - 1]: a push reads the half `parity` and writes the other one, so the workgroup that moves
// the history on never races with those that still read it.
constexpr int RS_STAB = 8;

// a row's table entry against the two buffers and the contract; a row with n_new = n_out = 0 has nothing to check
__host__ __device__ inline bool rs_stream_row_ok(const long long* e, int up, int down, int W, long long chunk_samples, long long y_samples) {
    const long long n_old = e[0], n_new = e[1], t0 = e[2], n_out = e[3], src = e[4], dst = e[5], par = e[6];
    if (n_new == 0 && n_out == 0) return true;
    if (n_old < 0 || n_new < 0 || t0 < 0 || n_out < 0 || src < 0 || dst < 0 || (par != 0 && par != 1)) return false;
    if (n_old > RS_MAX_LEN || n_new > RS_MAX_LEN || n_old + n_new > RS_MAX_LEN) return false;
    if (n_new > chunk_samples || src > chunk_samples - n_new || n_out > y_samples || dst > y_samples - n_out) return false;
    if (t0 > RS_MAX_LEN || n_out > RS_MAX_LEN || t0 + n_out > ((n_old + n_new) * up + down - 1) / down) return false;
    // the first tap of the first output lies inside the history
    return n_out == 0 || (t0 * down) / up - W + 1 >= n_old - (2LL * W - 1);
}

__device__ __forceinline__ float rs_stream_fetch(const float* __restrict__ hrow, const float* __restrict__ crow, long long g, long long n_old,
                                                 long long n_tot, int H) {
    if (g < 0 || g >= n_tot) return 0.0f;
    if (g >= n_old) return crow[g - n_old];
    const long long k = g - (n_old - H);
    return k >= 0 ? hrow[k] : 0.0f;
}

// workgroup id = row * (nchunk + 1) + ch: ch < nchunk computes outputs [t0 + ch * chunk, ..) of the row, ch == nchunk moves the
// row's history on.  A row whose table breaks the contract is flagged and neither read nor written.
__global__ __launch_bounds__(RS_NT) void stream_resample_kernel(const float* __restrict__ chunkbuf, long long chunk_samples, float* hist,
                                                                long long rows, int up, int down, const float* __restrict__ h, int W,
                                                                float* __restrict__ y, long long y_samples, const long long* __restrict__ tab,
                                                                int nchunk, int chunk, int span, int bank_lds, int* __restrict__ status) {
    extern __shared__ float rs_lds[];
    const unsigned per = (unsigned)nchunk + 1u;
    const long long row = blockIdx.x / per;
    const int ch = (int)(blockIdx.x - (unsigned)row * per);
    const long long* const e = tab + row * RS_STAB;
    const long long n_old = e[0], n_new = e[1], t0 = e[2], n_out = e[3];
    const bool ok = rs_stream_row_ok(e, up, down, W, chunk_samples, y_samples);
    if (ch == 0 && threadIdx.x == 0 && status != nullptr) status[row] = ok ? 0 : -1;
    if (!ok || (n_new == 0 && n_out == 0)) return;
    const int H = 2 * W - 1;
    const long long par = e[6], n_tot = n_old + n_new;
    const float* const hrow = hist + (par * rows + row) * H;
    const float* const crow = chunkbuf + e[4];
    if (ch == nchunk) {
        if (n_new == 0) return;                                           // a flush: the history stays
        float* const hnew = hist + ((1 - par) * rows + row) * H;
        for (int k = threadIdx.x; k < H; k += RS_NT) hnew[k] = rs_stream_fetch(hrow, crow, n_tot - H + k, n_old, n_tot, H);
        return;
    }
    const long long l0 = (long long)ch * chunk;
    if (l0 >= n_out) return;
    const int n = (int)(n_out - l0 < (long long)chunk ? n_out - l0 : (long long)chunk);
    const long long p = (t0 + l0) * down, q0 = p / up;
    const unsigned r0 = (unsigned)(p - q0 * up);
    float* const xs = rs_lds;
    float* const hs = rs_lds + span;
    const long long g0 = q0 - W + 1;
    const int need = (int)rs_span(up, down, W, n);                        // <= span: the staged part of n <= chunk outputs
    for (int k = threadIdx.x; k < need; k += RS_NT) xs[k] = rs_stream_fetch(hrow, crow, g0 + k, n_old, n_tot, H);
    if (bank_lds) {
        const int taps = 2 * W, total = up * taps;
        for (int idx = threadIdx.x; idx < total; idx += RS_NT) {
            const int ph = idx / taps;
            hs[ph * (taps + 1) + (idx - ph * taps)] = h[idx];
        }
    }
    __syncthreads();
    float* const yrow = y + e[5] + l0;
    if (bank_lds)
        rs_taps(xs, hs, 2 * W + 1, (unsigned)up, (unsigned)down, W, r0, n, yrow);
    else
        rs_taps(xs, h, 2 * W, (unsigned)up, (unsigned)down, W, r0, n, yrow);
}

// buf[r][k] = buf[r][off + k], k < n <= 4 * RS_NT, off = the spare entry of row r's table: one workgroup per row reads everything
// before it writes anything (the two spans may overlap).  off <= 0 or off + n > ld: the row is left alone.
__global__ __launch_bounds__(RS_NT) void stream_carry_kernel(float* __restrict__ buf, long long ld, const long long* __restrict__ tab, int n) {
    const long long off = tab[(long long)blockIdx.x * RS_STAB + 7];
    if (off <= 0 || off > ld - n) return;                                 // uniform over the workgroup
    float* const row = buf + (long long)blockIdx.x * ld;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = (int)threadIdx.x + k * RS_NT;
        v[k] = i < n ? row[off + i] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = (int)threadIdx.x + k * RS_NT;
        if (i < n) row[i] = v[k];
    }
}

int rs_gcd(int a, int b) {
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}

}  // namespace

extern "C" {

size_t ctn_resample_span(int up, int down, int W, int chunk) {
    if (up < 1 || down < 1 || W < 1 || chunk < 1 || chunk > RS_CHUNK || up > RS_MAX_TERM || down > RS_MAX_TERM) return 0;
    return (size_t)rs_span(up, down, W, chunk);
}

int ctn_resample_ragged(const float* x, long long x_samples, const long long* in_offsets, const long long* in_lens, long long U, int up,
                        int down, const float* h, int W, float* y, long long y_samples, const long long* out_offsets,
                        const long long* out_lens, const long long* host_tables, int* status, void* stream) {
    CTN_REQUIRE(x && in_offsets && in_lens && h && y && out_offsets && out_lens && host_tables, "ctn_resample_ragged: null pointer");
    CTN_REQUIRE(U >= 1 && U <= 0x7fffffffLL, "ctn_resample_ragged: U = %lld rows (1 .. 2^31 - 1)", U);
    CTN_REQUIRE(up >= 1 && down >= 1 && up <= RS_MAX_TERM && down <= RS_MAX_TERM, "ctn_resample_ragged: ratio %d / %d (terms in 1 .. 2^20)",
                up, down);
    CTN_REQUIRE(rs_gcd(up, down) == 1, "ctn_resample_ragged: ratio %d / %d is not in lowest terms", up, down);
    CTN_REQUIRE(W >= 1 && W <= (1 << 16), "ctn_resample_ragged: W = %d taps to either side (1 .. 2^16)", W);
    CTN_REQUIRE(x_samples >= 1 && y_samples >= 1, "ctn_resample_ragged: buffers of %lld and %lld samples", x_samples, y_samples);
    const long long *hio = host_tables, *hni = host_tables + U, *hoo = host_tables + 2 * U, *hno = host_tables + 3 * U;
    long long longest = 0;
    for (long long r = 0; r < U; ++r) {
        CTN_REQUIRE(hni[r] >= 1 && hni[r] <= RS_MAX_LEN, "ctn_resample_ragged: row %lld has %lld samples (1 .. 2^40)", r, hni[r]);
        CTN_REQUIRE(hio[r] >= 0 && hni[r] <= x_samples && hio[r] <= x_samples - hni[r],
                    "ctn_resample_ragged: row %lld (offset %lld, %lld samples) lies outside the input buffer of %lld samples", r, hio[r], hni[r],
                    x_samples);
        CTN_REQUIRE(hno[r] == (hni[r] * up + down - 1) / down, "ctn_resample_ragged: row %lld: %lld output samples, ceil(%lld * %d / %d) expected", r,
                    hno[r], hni[r], up, down);
        CTN_REQUIRE(hoo[r] >= 0 && hno[r] <= y_samples && hoo[r] <= y_samples - hno[r],
                    "ctn_resample_ragged: row %lld (offset %lld, %lld samples) lies outside the output buffer of %lld samples", r, hoo[r], hno[r],
                    y_samples);
        if (hno[r] > longest) longest = hno[r];
    }
    // the largest chunk (a multiple of 256 outputs, 1024 at most) whose input span fits the LDS
    int chunk = RS_CHUNK;
    while (chunk > 0 && 4 * rs_span(up, down, W, chunk) > RS_LDS_BYTES) chunk -= RS_NT;
    CTN_REQUIRE(chunk > 0, "ctn_resample_ragged: the input span of 256 outputs at %d / %d with W = %d does not fit %d bytes of LDS", up, down, W,
                RS_LDS_BYTES);
    const long long span = rs_span(up, down, W, chunk), padded = (long long)up * (2 * W + 1);
    const int bank_lds = 4 * (span + padded) <= RS_LDS_BYTES;
    const long long nchunk = ctn_cdivll(longest, chunk);
    CTN_REQUIRE(nchunk * U <= 0x7fffffffLL, "ctn_resample_ragged: %lld rows of up to %lld chunks exceed one launch", U, nchunk);
    const size_t lds = 4 * (size_t)(span + (bank_lds ? padded : 0));
    resample_ragged_kernel<<<dim3((unsigned)(nchunk * U)), dim3(RS_NT), lds, (hipStream_t)stream>>>(
        x, x_samples, in_offsets, in_lens, up, down, h, W, y, y_samples, out_offsets, out_lens, (int)nchunk, chunk, (int)span, bank_lds, status);
    CTN_CHECK_LAUNCH("ctn_resample_ragged");
    return CTN_OK;
}

int ctn_stream_resample(const float* chunk, long long chunk_samples, float* hist, long long rows, int up, int down, const float* h, int W,
                        float* y, long long y_samples, const long long* tab, const long long* host_tab, int* status, void* stream) {
    CTN_REQUIRE(chunk && hist && h && y && tab && host_tab, "ctn_stream_resample: null pointer");
    CTN_REQUIRE(rows >= 1 && rows <= 0x7fffffffLL, "ctn_stream_resample: %lld rows (1 .. 2^31 - 1)", rows);
    CTN_REQUIRE(up >= 1 && down >= 1 && up <= RS_MAX_TERM && down <= RS_MAX_TERM, "ctn_stream_resample: ratio %d / %d (terms in 1 .. 2^20)",
                up, down);
    CTN_REQUIRE(rs_gcd(up, down) == 1, "ctn_stream_resample: ratio %d / %d is not in lowest terms", up, down);
    CTN_REQUIRE(W >= 1 && W <= (1 << 16), "ctn_stream_resample: W = %d taps to either side (1 .. 2^16)", W);
    CTN_REQUIRE(chunk_samples >= 1 && y_samples >= 1, "ctn_stream_resample: buffers of %lld and %lld samples", chunk_samples, y_samples);
    long long longest = 0;
    for (long long r = 0; r < rows; ++r) {
        const long long* e = host_tab + r * RS_STAB;
        CTN_REQUIRE(rs_stream_row_ok(e, up, down, W, chunk_samples, y_samples),
                    "ctn_stream_resample: row %lld (n_old %lld, n_new %lld, t0 %lld, n_out %lld, src %lld, dst %lld, parity %lld) breaks its "
                    "contract or lies outside the buffers of %lld and %lld samples", r, e[0], e[1], e[2], e[3], e[4], e[5], e[6], chunk_samples,
                    y_samples);
        if (e[3] > longest) longest = e[3];
    }
    // the largest chunk (a multiple of 256 outputs, 1024 at most) whose input span fits the LDS, as in ctn_resample_ragged
    int chunkn = RS_CHUNK;
    while (chunkn > 0 && 4 * rs_span(up, down, W, chunkn) > RS_LDS_BYTES) chunkn -= RS_NT;
    CTN_REQUIRE(chunkn > 0, "ctn_stream_resample: the input span of 256 outputs at %d / %d with W = %d does not fit %d bytes of LDS", up, down, W,
                RS_LDS_BYTES);
    const long long span = rs_span(up, down, W, chunkn), padded = (long long)up * (2 * W + 1);
    const int bank_lds = 4 * (span + padded) <= RS_LDS_BYTES;
    const long long nchunk = ctn_cdivll(longest, chunkn);
    CTN_REQUIRE((nchunk + 1) * rows <= 0x7fffffffLL, "ctn_stream_resample: %lld rows of up to %lld chunks exceed one launch", rows, nchunk);
    const size_t lds = 4 * (size_t)(span + (bank_lds ? padded : 0));
    stream_resample_kernel<<<dim3((unsigned)((nchunk + 1) * rows)), dim3(RS_NT), lds, (hipStream_t)stream>>>(
        chunk, chunk_samples, hist, rows, up, down, h, W, y, y_samples, tab, (int)nchunk, chunkn, (int)span, bank_lds, status);
    CTN_CHECK_LAUNCH("ctn_stream_resample");
    return CTN_OK;
}

int ctn_stream_carry(float* buf, long long ld, long long rows, const long long* tab, int n, void* stream) {
    CTN_REQUIRE(buf && tab, "ctn_stream_carry: null pointer");
    CTN_REQUIRE(rows >= 1 && rows <= 0x7fffffffLL, "ctn_stream_carry: %lld rows (1 .. 2^31 - 1)", rows);
    CTN_REQUIRE(n >= 1 && n <= RS_CHUNK && ld >= n, "ctn_stream_carry: n = %d samples (1 .. %d) in rows of %lld", n, RS_CHUNK, ld);
    stream_carry_kernel<<<dim3((unsigned)rows), dim3(RS_NT), 0, (hipStream_t)stream>>>(buf, ld, tab, n);
    CTN_CHECK_LAUNCH("ctn_stream_carry");
    return CTN_OK;
}

int ctn_dynmix_speed_segments(const float* corpus, const long long* offsets, const long long* lens, long long U, const int* plan_utt,
                              const long long* plan_start, const int* plan_pct, int B, int C, int T, const float* banks,
                              long long bank_floats, const int* bank_tab, int span_cap, int bank_cap, float* seg, int* seg_utt,
                              void* stream) {
    CTN_REQUIRE(corpus && offsets && lens && plan_utt && plan_start && plan_pct && banks && bank_tab && seg && seg_utt,
                "ctn_dynmix_speed_segments: null pointer");
    CTN_REQUIRE(C >= 2 && C <= 4, "ctn_dynmix_speed_segments: C = %d sources per mixture (2 .. 4)", C);
    CTN_REQUIRE(T >= 1, "ctn_dynmix_speed_segments: seg_len = %d", T);
    CTN_REQUIRE(B >= 1 && (long long)B * C <= 65535, "ctn_dynmix_speed_segments: B = %d mixtures (B * C in 1 .. 65535)", B);
    CTN_REQUIRE(U >= 1 && U <= 0x7fffffffLL, "ctn_dynmix_speed_segments: U = %lld utterances (1 .. 2^31 - 1)", U);
    CTN_REQUIRE(bank_floats >= 1, "ctn_dynmix_speed_segments: bank_floats = %lld", bank_floats);
    CTN_REQUIRE(span_cap >= 1 && bank_cap >= 0 && 4 * ((long long)span_cap + bank_cap) <= RS_LDS_BYTES,
                "ctn_dynmix_speed_segments: span_cap %d + bank_cap %d floats of LDS (span_cap >= 1, %d bytes at most)", span_cap, bank_cap,
                RS_LDS_BYTES);
    const size_t lds = 4 * ((size_t)span_cap + (size_t)bank_cap);
    dynmix_speed_segments_kernel<<<dim3(ctn_cdiv(T, RS_CHUNK), B * C), dim3(RS_NT), lds, (hipStream_t)stream>>>(
        corpus, offsets, lens, (int)U, plan_utt, plan_start, plan_pct, T, banks, bank_floats, bank_tab, span_cap, bank_cap, seg, seg_utt);
    CTN_CHECK_LAUNCH("ctn_dynmix_speed_segments");
    return CTN_OK;
}

}  // extern "C"
