// Long-recording separation: recordings cut into overlapping segments, and the segments' estimates brought into one speaker
// order and cross-faded back into recordings, all in device memory.
// Contract: include/ctn_hip.h ("long-recording separation"); executable restatement: tests/longform_oracle.py.
// Every product and every add is ONE float32 rounding in a stated order (no contraction into fused multiply-adds), and the
// order of every sum is a function of the data alone, so cost, g and out are bitwise functions of est whatever the launch
// geometry.  Everything here is bound by memory traffic: 16-byte loads and stores wherever the addresses allow.
#include "ctn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int LF_NT = 256;                 // threads per workgroup
constexpr int LF_PART = 1024;              // partial sums of one cost (4 per thread)
constexpr int LF_CHUNK = 2048;             // samples of one segment per workgroup in frame / assemble (2 float4 per thread)
constexpr int LF_MAX_C = 4;
constexpr long long LF_MAX_LEN = 1LL << 40;
constexpr int LF_MAX_SEG = 1 << 30;

// the C! permutations in itertools (lexicographic) order
__device__ const unsigned char LF_PERM2[2][2] = {{0, 1}, {1, 0}};
__device__ const unsigned char LF_PERM3[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
__device__ const unsigned char LF_PERM4[24][4] = {
    {0, 1, 2, 3}, {0, 1, 3, 2}, {0, 2, 1, 3}, {0, 2, 3, 1}, {0, 3, 1, 2}, {0, 3, 2, 1}, {1, 0, 2, 3}, {1, 0, 3, 2},
    {1, 2, 0, 3}, {1, 2, 3, 0}, {1, 3, 0, 2}, {1, 3, 2, 0}, {2, 0, 1, 3}, {2, 0, 3, 1}, {2, 1, 0, 3}, {2, 1, 3, 0},
    {2, 3, 0, 1}, {2, 3, 1, 0}, {3, 0, 1, 2}, {3, 0, 2, 1}, {3, 1, 0, 2}, {3, 1, 2, 0}, {3, 2, 0, 1}, {3, 2, 1, 0}};

template <int C> __device__ __forceinline__ int lf_perm(int k, int a) {
    if constexpr (C == 2) return LF_PERM2[k][a];
    else if constexpr (C == 3) return LF_PERM3[k][a];
    else return LF_PERM4[k][a];
}
template <int C> constexpr int lf_nperm() { return C == 2 ? 2 : C == 3 ? 6 : 24; }

// segments of a recording of T >= 1 samples
__host__ __device__ inline long long lf_nseg(long long T, long long seg, long long hop) {
    return T <= seg ? 1 : 1 + (T - seg + hop - 1) / hop;
}

// the recording r in [0, R) with seg_ptr[r] <= s < seg_ptr[r + 1], or -1 when the device table has no such entry (only entries
// 0 .. R of seg_ptr are read, whatever they hold)
__device__ __forceinline__ long long lf_find_rec(const long long* __restrict__ seg_ptr, long long R, long long s) {
    long long lo = 0, hi = R;                                               // invariant wanted: seg_ptr[lo] <= s < seg_ptr[hi]
    while (hi - lo > 1) {
        const long long mid = lo + (hi - lo) / 2;
        if (seg_ptr[mid] <= s) lo = mid; else hi = mid;
    }
    return (seg_ptr[lo] <= s && s < seg_ptr[lo + 1]) ? lo : -1;
}

// a recording's device tables against the contract: its segment range inside [0, Nseg] with the count its length asks for
__device__ __forceinline__ bool lf_rec_ok(long long lo, long long hi, long long T, long long Nseg, int seg, int hop) {
    return T >= 1 && T <= LF_MAX_LEN && lo >= 0 && hi <= Nseg && lo < hi && hi - lo == lf_nseg(T, seg, hop);
}

// ---- framing ---------------------------------------------------------------------------------------------------------------
// workgroup id = s * nchunk + chunk: samples [chunk * LF_CHUNK, ..) of segment s.  segs[s, u] = x[in_off + i * hop + u] below T, else +0.
__global__ __launch_bounds__(LF_NT) void longform_frame_kernel(const float* __restrict__ x, long long x_samples,
                                                               const long long* __restrict__ seg_ptr, const long long* __restrict__ Tt,
                                                               const long long* __restrict__ in_off, long long R, long long Nseg, int seg,
                                                               int hop, int nchunk, float* __restrict__ segs, int* __restrict__ status) {
    const long long s = blockIdx.x / (unsigned)nchunk;
    const int ch = (int)(blockIdx.x - (unsigned)s * (unsigned)nchunk);
    const long long r = lf_find_rec(seg_ptr, R, s);
    if (r < 0) return;
    const long long lo = seg_ptr[r], hi = seg_ptr[r + 1], T = Tt[r], io = in_off[r];
    const bool ok = lf_rec_ok(lo, hi, T, Nseg, seg, hop) && io >= 0 && T <= x_samples && io <= x_samples - T;
    if (s == lo && ch == 0 && threadIdx.x == 0 && status != nullptr) status[r] = ok ? 0 : -1;
    if (!ok) return;
    const long long i = s - lo;
    const int u0 = ch * LF_CHUNK;
    const int n = min(LF_CHUNK, seg - u0);
    const long long left = T - i * hop - u0;                                // samples of the recording from u0 on (may be <= 0)
    const float* __restrict__ src = x + io + i * hop + u0;
    float* __restrict__ dst = segs + s * seg + u0;
    if (ctn_aligned16(src) && ctn_aligned16(dst)) {
        for (int k = 4 * threadIdx.x; k < n; k += 4 * LF_NT) {
            if (k + 4 <= n && k + 4 <= left) {
                *reinterpret_cast<float4*>(dst + k) = *reinterpret_cast<const float4*>(src + k);
            } else if (k + 4 <= n && k >= left) {
                *reinterpret_cast<float4*>(dst + k) = make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                for (int e = k; e < min(k + 4, n); ++e) dst[e] = e < left ? src[e] : 0.0f;
            }
        }
    } else {
        for (int k = threadIdx.x; k < n; k += LF_NT) dst[k] = k < left ? src[k] : 0.0f;
    }
}

// ---- costs -----------------------------------------------------------------------------------------------------------------
// four consecutive samples of a row: one 16-byte load where the address allows, else four 4-byte loads; elements at or beyond
// `left` are not read
__device__ __forceinline__ void lf_load4(const float* __restrict__ p, bool vec, int left, float v[4]) {
    if (vec && left >= 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = e < left ? p[e] : 0.0f;
    }
}

// One workgroup per segment s.  A first segment writes zeros.  Otherwise thread x keeps partial sums j = 4x .. 4x + 3 of all C * C
// costs: every round of 1024 overlap samples loads the C rows of the predecessor's tail and the C rows of this segment's head
// once, for all C * C pairs.  Then, pair by pair, the 1024 partials go through LDS into the order the tree wants (thread x takes
// j = x, x + 256, x + 512, x + 768: the steps 512 and 256 are in registers), the steps 128 and 64 read LDS, the rest is one wave.
template <int C>
__global__ __launch_bounds__(LF_NT) void longform_costs_kernel(const float* __restrict__ est, const long long* __restrict__ seg_ptr,
                                                               long long R, long long Nseg, int seg, int hop, float* __restrict__ cost) {
    __shared__ __attribute__((aligned(16))) float part[LF_PART];
    __shared__ float red[C * C][LF_NT];
    const long long s = blockIdx.x;
    const long long r = lf_find_rec(seg_ptr, R, s);
    float* const crow = cost + s * (C * C);
    if (r < 0 || s == seg_ptr[r] || s == 0) {                               // a first segment (s == 0 has no predecessor, whatever the table says)
        if (threadIdx.x < C * C) crow[threadIdx.x] = 0.0f;
        return;
    }
    const int ov = seg - hop;
    const float* const prev = est + (s - 1) * C * seg + hop;                // row a: prev + a * seg
    const float* const cur = est + s * C * seg;                             // row b: cur + b * seg
    const bool pvec = ctn_aligned16(prev) && (seg & 3) == 0;
    const bool cvec = ctn_aligned16(cur) && (seg & 3) == 0;
    float acc[C * C][4];
#pragma unroll
    for (int p = 0; p < C * C; ++p)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[p][e] = 0.0f;
    for (int t0 = 4 * (int)threadIdx.x; t0 < ov; t0 += LF_PART) {
        const int left = ov - t0;
        float pv[C][4], cv[C][4];
#pragma unroll
        for (int a = 0; a < C; ++a) lf_load4(prev + (long long)a * seg + t0, pvec, left, pv[a]);
#pragma unroll
        for (int b = 0; b < C; ++b) lf_load4(cur + (long long)b * seg + t0, cvec, left, cv[b]);
#pragma unroll
        for (int a = 0; a < C; ++a)
#pragma unroll
            for (int b = 0; b < C; ++b)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float d = pv[a][e] - cv[b][e];
                    const float q = d * d;
                    if (e < left) acc[a * C + b][e] = acc[a * C + b][e] + q;
                }
    }
#pragma unroll
    for (int p = 0; p < C * C; ++p) {
        __syncthreads();                                                    // the previous pair's reads of part
        *reinterpret_cast<float4*>(part + 4 * threadIdx.x) = make_float4(acc[p][0], acc[p][1], acc[p][2], acc[p][3]);
        __syncthreads();
        const float a0 = part[threadIdx.x] + part[threadIdx.x + 512];       // step 512, j = x and j = x + 256
        const float a1 = part[threadIdx.x + 256] + part[threadIdx.x + 768];
        red[p][threadIdx.x] = a0 + a1;                                      // step 256
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int p = wave; p < C * C; p += LF_NT / 64) {
        const float b0 = red[p][lane] + red[p][lane + 128];                 // step 128, j = lane and j = lane + 64
        const float b1 = red[p][lane + 64] + red[p][lane + 192];
        float v = b0 + b1;                                                  // step 64
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = v + __shfl_down(v, o, 64);     // steps 32 .. 1: lane j < o adds lane j + o
        if (lane == 0) crow[p] = v;
    }
}

// ---- order -----------------------------------------------------------------------------------------------------------------
// A permutation of C <= 4 channels in one word, 2 bits per entry.
__device__ __forceinline__ unsigned lf_pack_identity() { return 0xE4u; }   // 3 2 1 0
__device__ __forceinline__ unsigned lf_get(unsigned p, int a) { return (p >> (2 * a)) & 3u; }
// (later after earlier)(a) = later[earlier[a]]
__device__ __forceinline__ unsigned lf_compose(unsigned later, unsigned earlier) {
    unsigned o = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) o |= lf_get(later, (int)lf_get(earlier, a)) << (2 * a);
    return o;
}

// the first k that minimises sum_a cost[a][perms[k][a]], the sum in fp32 from +0 with a ascending
template <int C> __device__ __forceinline__ int lf_best_perm(const float* __restrict__ c) {
    float cc[C * C];
#pragma unroll
    for (int p = 0; p < C * C; ++p) cc[p] = c[p];
    int best = 0;
    float bestv = 0.0f;
#pragma unroll
    for (int k = 0; k < lf_nperm<C>(); ++k) {
        float v = 0.0f;
#pragma unroll
        for (int a = 0; a < C; ++a) v = v + cc[a * C + lf_perm<C>(k, a)];
        if (k == 0 || v < bestv) { best = k; bestv = v; }
    }
    return best;
}

template <int C> __device__ __forceinline__ unsigned lf_pack_perm(int k) {
    unsigned o = lf_pack_identity();
#pragma unroll
    for (int a = 0; a < C; ++a) o = (o & ~(3u << (2 * a))) | ((unsigned)lf_perm<C>(k, a) << (2 * a));
    return o;
}

// One workgroup per recording.  Thread x takes a run of consecutive segments: it finds their q_s and composes them, the 256 runs
// are scanned in LDS, and the thread walks its run again from the scanned prefix.  g[s][0] holds q_s between the two walks (the
// same thread writes and reads it).
template <int C>
__global__ __launch_bounds__(LF_NT) void longform_order_kernel(const float* __restrict__ cost, const long long* __restrict__ seg_ptr,
                                                               long long Nseg, int* __restrict__ g, int* __restrict__ status) {
    __shared__ unsigned scan[2][LF_NT];
    const long long r = blockIdx.x;
    const long long lo = seg_ptr[r], hi = seg_ptr[r + 1];
    const bool ok = lo >= 0 && lo < hi && hi <= Nseg;
    if (threadIdx.x == 0 && status != nullptr) status[r] = ok ? 0 : -1;
    if (!ok) return;
    const long long n = hi - lo, run = (n + LF_NT - 1) / LF_NT;
    const long long i0 = min(n, (long long)threadIdx.x * run), i1 = min(n, i0 + run);
    unsigned mine = lf_pack_identity();
    for (long long i = i0; i < i1; ++i) {
        const int q = i == 0 ? 0 : lf_best_perm<C>(cost + (lo + i) * (C * C));
        g[(lo + i) * C] = q;
        mine = lf_compose(lf_pack_perm<C>(q), mine);
    }
    int w = 0;
    scan[0][threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < LF_NT; d <<= 1) {
        unsigned v = scan[w][threadIdx.x];
        if ((int)threadIdx.x >= d) v = lf_compose(v, scan[w][threadIdx.x - d]);
        scan[w ^ 1][threadIdx.x] = v;
        w ^= 1;
        __syncthreads();
    }
    unsigned at = threadIdx.x == 0 ? lf_pack_identity() : scan[w][threadIdx.x - 1];
    for (long long i = i0; i < i1; ++i) {
        at = lf_compose(lf_pack_perm<C>(g[(lo + i) * C]), at);
#pragma unroll
        for (int a = 0; a < C; ++a) g[(lo + i) * C + a] = (int)lf_get(at, a);
    }
}

// ---- assembly --------------------------------------------------------------------------------------------------------------
// workgroup id = s * nchunk + chunk.  Segment i of a recording owns the output samples [i * hop, (i + 1) * hop), the last one
// [i * hop, T): the chunk is samples [chunk * LF_CHUNK, ..) of that range, all C channels.  u < ov of a segment i >= 1 is the
// cross-fade with the predecessor's tail: fo * prev + fi * cur, two products and one sum.
__global__ __launch_bounds__(LF_NT) void longform_assemble_kernel(const float* __restrict__ est, const int* __restrict__ g,
                                                                  const long long* __restrict__ seg_ptr, const long long* __restrict__ Tt,
                                                                  const long long* __restrict__ out_off, long long R, long long Nseg, int C,
                                                                  int seg, int hop, int nchunk, const float* __restrict__ fi,
                                                                  const float* __restrict__ fo, float* __restrict__ out, long long out_samples,
                                                                  int* __restrict__ status) {
    const long long s = blockIdx.x / (unsigned)nchunk;
    const int ch = (int)(blockIdx.x - (unsigned)s * (unsigned)nchunk);
    const long long r = lf_find_rec(seg_ptr, R, s);
    if (r < 0) return;
    const long long lo = seg_ptr[r], hi = seg_ptr[r + 1], T = Tt[r], oo = out_off[r];
    const bool ok = lf_rec_ok(lo, hi, T, Nseg, seg, hop) && oo >= 0 && T <= out_samples / C && oo <= out_samples - T * C;
    if (s == lo && ch == 0 && threadIdx.x == 0 && status != nullptr) status[r] = ok ? 0 : -1;
    if (!ok) return;
    const long long i = s - lo;
    const long long own = (s == hi - 1) ? T - i * hop : (long long)hop;    // <= seg: the last segment reaches T
    const long long u0 = (long long)ch * LF_CHUNK;
    if (u0 >= own) return;
    const int n = (int)min((long long)LF_CHUNK, own - u0);
    const int ov = seg - hop;
    const int nfade = i >= 1 ? (int)max(0LL, min((long long)n, ov - u0)) : 0;   // leading samples of this chunk that are cross-faded
    const bool tvec = ctn_aligned16(fi + u0) && ctn_aligned16(fo + u0);
    for (int a = 0; a < C; ++a) {
        const int gc = g[s * C + a];
        if ((unsigned)gc >= (unsigned)C) continue;                          // never an address from a bad order entry
        const float* __restrict__ cur = est + (s * C + gc) * seg + u0;
        float* __restrict__ dst = out + oo + a * T + i * hop + u0;
        const float* __restrict__ prv = cur;
        if (nfade > 0) {
            const int gp = g[(s - 1) * C + a];
            if ((unsigned)gp >= (unsigned)C) continue;
            prv = est + ((s - 1) * C + gp) * seg + hop + u0;
        }
        const bool vec = ctn_aligned16(cur) && ctn_aligned16(dst) && (nfade == 0 || (tvec && ctn_aligned16(prv)));
        if (vec) {
            const int nf4 = nfade & ~3, n4 = n & ~3;                        // whole float4 groups of the fade and of the chunk
            for (int k = 4 * threadIdx.x; k < n4; k += 4 * LF_NT) {
                float4 c = *reinterpret_cast<const float4*>(cur + k);
                if (k < nf4) {
                    const float4 p = *reinterpret_cast<const float4*>(prv + k);
                    const float4 wi = *reinterpret_cast<const float4*>(fi + u0 + k);
                    const float4 wo = *reinterpret_cast<const float4*>(fo + u0 + k);
                    float x0 = wo.x * p.x, y0 = wi.x * c.x; c.x = x0 + y0;
                    float x1 = wo.y * p.y, y1 = wi.y * c.y; c.y = x1 + y1;
                    float x2 = wo.z * p.z, y2 = wi.z * c.z; c.z = x2 + y2;
                    float x3 = wo.w * p.w, y3 = wi.w * c.w; c.w = x3 + y3;
                } else if (k < nfade) {                                     // the group the fade ends in
                    float v[4] = {c.x, c.y, c.z, c.w};
                    for (int e = 0; e < nfade - k; ++e) {
                        const float x0 = fo[u0 + k + e] * prv[k + e], y0 = fi[u0 + k + e] * v[e];
                        v[e] = x0 + y0;
                    }
                    c = make_float4(v[0], v[1], v[2], v[3]);
                }
                *reinterpret_cast<float4*>(dst + k) = c;
            }
            for (int k = n4 + threadIdx.x; k < n; k += LF_NT) {
                float c = cur[k];
                if (k < nfade) {
                    const float x0 = fo[u0 + k] * prv[k], y0 = fi[u0 + k] * c;
                    c = x0 + y0;
                }
                dst[k] = c;
            }
        } else {
            for (int k = threadIdx.x; k < n; k += LF_NT) {
                float c = cur[k];
                if (k < nfade) {
                    const float x0 = fo[u0 + k] * prv[k], y0 = fi[u0 + k] * c;
                    c = x0 + y0;
                }
                dst[k] = c;
            }
        }
    }
}

// seg_ptr in host memory: R + 1 ascending entries from 0 to Nseg, no empty recording
bool lf_seg_ptr_ok(const long long* sp, long long R, long long Nseg) {
    if (sp[0] != 0 || sp[R] != Nseg) return false;
    for (long long r = 0; r < R; ++r)
        if (sp[r + 1] <= sp[r]) return false;
    return true;
}

}  // namespace

#define LF_REQUIRE_GEOMETRY(name)                                                                                                      \
    CTN_REQUIRE(hop >= 1 && seg > hop && seg <= LF_MAX_SEG && seg - hop <= hop,                                                        \
                name ": seg = %d, hop = %d (1 <= seg - hop <= hop, seg <= 2^30: at most two segments over one sample)", seg, hop);    \
    CTN_REQUIRE(R >= 1 && R <= 0x7fffffffLL && Nseg >= R && Nseg <= 0x7fffffffLL, name ": %lld recordings in %lld segments", R, Nseg)

extern "C" {

long long ctn_longform_nseg(long long T, int seg, int hop) {
    if (T < 1 || T > LF_MAX_LEN || hop < 1 || seg <= hop || seg - hop > hop) return 0;
    return lf_nseg(T, seg, hop);
}

int ctn_longform_frame(const float* x, long long x_samples, const long long* seg_ptr, const long long* T, const long long* in_off,
                       long long R, long long Nseg, int seg, int hop, float* segs, const long long* host_tables, int* status,
                       void* stream) {
    CTN_REQUIRE(x && seg_ptr && T && in_off && segs && host_tables, "ctn_longform_frame: null pointer");
    LF_REQUIRE_GEOMETRY("ctn_longform_frame");
    CTN_REQUIRE(x_samples >= 1, "ctn_longform_frame: a buffer of %lld samples", x_samples);
    const long long *hsp = host_tables, *hT = host_tables + R + 1, *hoff = host_tables + 2 * R + 1;
    CTN_REQUIRE(lf_seg_ptr_ok(hsp, R, Nseg), "ctn_longform_frame: seg_ptr does not ascend from 0 to Nseg = %lld", Nseg);
    for (long long r = 0; r < R; ++r) {
        CTN_REQUIRE(hT[r] >= 1 && hT[r] <= LF_MAX_LEN, "ctn_longform_frame: recording %lld has %lld samples (1 .. 2^40)", r, hT[r]);
        CTN_REQUIRE(hsp[r + 1] - hsp[r] == lf_nseg(hT[r], seg, hop), "ctn_longform_frame: recording %lld: %lld segments, %lld expected for %lld samples",
                    r, hsp[r + 1] - hsp[r], lf_nseg(hT[r], seg, hop), hT[r]);
        CTN_REQUIRE(hoff[r] >= 0 && hT[r] <= x_samples && hoff[r] <= x_samples - hT[r],
                    "ctn_longform_frame: recording %lld (offset %lld, %lld samples) lies outside the input buffer of %lld samples", r, hoff[r],
                    hT[r], x_samples);
    }
    const long long nchunk = ctn_cdiv(seg, LF_CHUNK);
    CTN_REQUIRE(nchunk * Nseg <= 0x7fffffffLL, "ctn_longform_frame: %lld segments of %lld chunks exceed one launch", Nseg, nchunk);
    longform_frame_kernel<<<dim3((unsigned)(nchunk * Nseg)), dim3(LF_NT), 0, (hipStream_t)stream>>>(
        x, x_samples, seg_ptr, T, in_off, R, Nseg, seg, hop, (int)nchunk, segs, status);
    CTN_CHECK_LAUNCH("ctn_longform_frame");
    return CTN_OK;
}

int ctn_longform_costs(const float* est, const long long* seg_ptr, long long R, long long Nseg, int C, int seg, int hop, float* cost,
                       const long long* host_seg_ptr, void* stream) {
    CTN_REQUIRE(est && seg_ptr && cost && host_seg_ptr, "ctn_longform_costs: null pointer");
    CTN_REQUIRE(C >= 2 && C <= LF_MAX_C, "ctn_longform_costs: C = %d speakers (2 .. 4)", C);
    LF_REQUIRE_GEOMETRY("ctn_longform_costs");
    CTN_REQUIRE(lf_seg_ptr_ok(host_seg_ptr, R, Nseg), "ctn_longform_costs: seg_ptr does not ascend from 0 to Nseg = %lld", Nseg);
    const dim3 grid((unsigned)Nseg), block(LF_NT);
    hipStream_t st = (hipStream_t)stream;
    if (C == 2) longform_costs_kernel<2><<<grid, block, 0, st>>>(est, seg_ptr, R, Nseg, seg, hop, cost);
    else if (C == 3) longform_costs_kernel<3><<<grid, block, 0, st>>>(est, seg_ptr, R, Nseg, seg, hop, cost);
    else longform_costs_kernel<4><<<grid, block, 0, st>>>(est, seg_ptr, R, Nseg, seg, hop, cost);
    CTN_CHECK_LAUNCH("ctn_longform_costs");
    return CTN_OK;
}

int ctn_longform_order(const float* cost, const long long* seg_ptr, long long R, long long Nseg, int C, int* g,
                       const long long* host_seg_ptr, int* status, void* stream) {
    CTN_REQUIRE(cost && seg_ptr && g && host_seg_ptr, "ctn_longform_order: null pointer");
    CTN_REQUIRE(C >= 2 && C <= LF_MAX_C, "ctn_longform_order: C = %d speakers (2 .. 4)", C);
    CTN_REQUIRE(R >= 1 && R <= 0x7fffffffLL && Nseg >= R && Nseg <= 0x7fffffffLL, "ctn_longform_order: %lld recordings in %lld segments", R, Nseg);
    CTN_REQUIRE(lf_seg_ptr_ok(host_seg_ptr, R, Nseg), "ctn_longform_order: seg_ptr does not ascend from 0 to Nseg = %lld", Nseg);
    const dim3 grid((unsigned)R), block(LF_NT);
    hipStream_t st = (hipStream_t)stream;
    if (C == 2) longform_order_kernel<2><<<grid, block, 0, st>>>(cost, seg_ptr, Nseg, g, status);
    else if (C == 3) longform_order_kernel<3><<<grid, block, 0, st>>>(cost, seg_ptr, Nseg, g, status);
    else longform_order_kernel<4><<<grid, block, 0, st>>>(cost, seg_ptr, Nseg, g, status);
    CTN_CHECK_LAUNCH("ctn_longform_order");
    return CTN_OK;
}

int ctn_longform_assemble(const float* est, const int* g, const long long* seg_ptr, const long long* T, const long long* out_off,
                          long long R, long long Nseg, int C, int seg, int hop, const float* fi, const float* fo, float* out,
                          long long out_samples, const long long* host_tables, int* status, void* stream) {
    CTN_REQUIRE(est && g && seg_ptr && T && out_off && fi && fo && out && host_tables, "ctn_longform_assemble: null pointer");
    CTN_REQUIRE(C >= 2 && C <= LF_MAX_C, "ctn_longform_assemble: C = %d speakers (2 .. 4)", C);
    LF_REQUIRE_GEOMETRY("ctn_longform_assemble");
    CTN_REQUIRE(out_samples >= 1, "ctn_longform_assemble: a buffer of %lld samples", out_samples);
    const long long *hsp = host_tables, *hT = host_tables + R + 1, *hoff = host_tables + 2 * R + 1;
    CTN_REQUIRE(lf_seg_ptr_ok(hsp, R, Nseg), "ctn_longform_assemble: seg_ptr does not ascend from 0 to Nseg = %lld", Nseg);
    for (long long r = 0; r < R; ++r) {
        CTN_REQUIRE(hT[r] >= 1 && hT[r] <= LF_MAX_LEN, "ctn_longform_assemble: recording %lld has %lld samples (1 .. 2^40)", r, hT[r]);
        CTN_REQUIRE(hsp[r + 1] - hsp[r] == lf_nseg(hT[r], seg, hop),
                    "ctn_longform_assemble: recording %lld: %lld segments, %lld expected for %lld samples", r, hsp[r + 1] - hsp[r],
                    lf_nseg(hT[r], seg, hop), hT[r]);
        CTN_REQUIRE(hoff[r] >= 0 && hT[r] <= out_samples / C && hoff[r] <= out_samples - hT[r] * C,
                    "ctn_longform_assemble: recording %lld (offset %lld, %d channels of %lld samples) lies outside the output buffer of %lld samples",
                    r, hoff[r], C, hT[r], out_samples);
    }
    const long long nchunk = ctn_cdiv(seg, LF_CHUNK);
    CTN_REQUIRE(nchunk * Nseg <= 0x7fffffffLL, "ctn_longform_assemble: %lld segments of %lld chunks exceed one launch", Nseg, nchunk);
    longform_assemble_kernel<<<dim3((unsigned)(nchunk * Nseg)), dim3(LF_NT), 0, (hipStream_t)stream>>>(
        est, g, seg_ptr, T, out_off, R, Nseg, C, seg, hop, (int)nchunk, fi, fo, out, out_samples, status);
    CTN_CHECK_LAUNCH("ctn_longform_assemble");
    return CTN_OK;
}

}  // extern "C"
