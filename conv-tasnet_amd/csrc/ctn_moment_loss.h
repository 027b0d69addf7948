// The skeleton of the moment-form losses (ctn_mixit.hip, ctn_varpit.hip), gfx950.  Such a loss runs
//   1. moment_sweep_kernel: one sweep over the reference and estimate rows collecting fp64 moments per utterance and time chunk,
//   2. a one-block assignment kernel, one wave per utterance: sum_chunks_to_lds, the loss's own scalars, wave_first_min, mean_over_waves,
//   3. a backward of four samples per lane: clamped_len, upstream_scale, load4, the loss's own arithmetic, store4.
// A loss supplies a moment policy (below), its assignment kernel between the shared prologue and epilogue, and its backward body.
//
// The bitwise promise of these losses is kept HERE, once: the time partition (ctn_sisnr_chunks, moment_chunk) and the lane that
// owns a sample depend on T alone, every reduction adds in one fixed order, and the aligned (16 bytes per lane) and the scalar
// load and store paths move the same values, so an utterance's result is bitwise the same in any batch, at any batch index and at
// any alignment.  The kernels of ctn_loss.hip share the partition only: their reduction order is another.
#pragma once
#include <type_traits>

#include "ctn_common.h"

extern "C" int ctn_sisnr_chunks(int T);      // csrc/ctn_loss.hip: the time partition, a function of T alone

namespace {

constexpr int NT = 256;            // moment sweep and backward kernels
constexpr int NTA = 1024;          // assignment kernels: 16 waves, one utterance per wave at a time

// The device helpers below are inlined into kernels whose own parameters are __restrict__.  Apart from load4 they add no such
// qualifier of their own: it would only give the compiler further alias scopes to schedule by.
struct Quad { float v[4]; };

// four consecutive samples of one row starting at t (t % 4 == 0); samples at or beyond `len` read as 0 and are not touched
template <bool VEC>
__device__ __forceinline__ Quad load4(const float* __restrict__ row, int t, int len) {
    Quad q;
    if (VEC && t + 4 <= len) {
        const float4 f = *reinterpret_cast<const float4*>(row + t);
        q.v[0] = f.x; q.v[1] = f.y; q.v[2] = f.z; q.v[3] = f.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) q.v[j] = t + j < len ? row[t + j] : 0.f;
    }
    return q;
}

// o[0 .. 3] to dst = row + t.  VEC implies T % 4 == 0: the whole quad is inside the row.
template <bool VEC>
__device__ __forceinline__ void store4(float* dst, const float (&o)[4], int t, int T) {
    if (VEC) {
        *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (t + k < T) dst[k] = o[k];
    }
}

__device__ __forceinline__ int clamped_len(const long long* lens, int b, int T) {
    long long ll = lens[b];
    if (ll > T) ll = T;
    if (ll < 0) ll = 0;
    return (int)ll;
}

// Block sum of NV values per lane: the waves' sums go through LDS and lane q < NV adds those of value q in ascending wave order
// and returns the total (the other lanes return 0).
template <int NV>
__device__ __forceinline__ double reduce_partials(const double (&acc)[NV], double (&red)[NT / 64][NV]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const double v = wave_sum(acc[q]);
        if ((tid & 63) == 0) red[tid >> 6][q] = v;
    }
    __syncthreads();
    double s = 0.0;
    if (tid < NV) {
        s = red[0][tid];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) s += red[w][tid];
    }
    return s;
}

// partial[b][chunk][P::NV]; chunk % 4 == 0.  Lane tid owns the quads (t0 + 4 tid) + 4 NT k of its chunk, in ascending k.
// The policy P of a loss: NREF and NEST, the rows per utterance of `refs` and `est`; NV, its number of moments; and
// accumulate(acc, ref quads, est quads, k), which adds sample k (0 .. 3) of the loaded quads to the NV moments.
template <class P, bool VEC>
__global__ __launch_bounds__(NT) void moment_sweep_kernel(const float* __restrict__ refs, const float* __restrict__ est,
                                                          const long long* __restrict__ lens, int T, int chunk, int nchunk,
                                                          double* __restrict__ partial) {
    constexpr int NV = P::NV;
    __shared__ double red[NT / 64][NV];
    const int b = blockIdx.x / nchunk, ch = blockIdx.x % nchunk;
    const int tid = threadIdx.x;
    const int len = clamped_len(lens, b, T);
    const int t0 = ch * chunk, t1 = min(min(t0 + chunk, T), len);
    const float* __restrict__ rb = refs + (size_t)b * P::NREF * T;
    const float* __restrict__ eb = est + (size_t)b * P::NEST * T;
    double acc[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) acc[q] = 0.0;
    for (int t = t0 + 4 * tid; t < t1; t += 4 * NT) {
        Quad rv[P::NREF], ev[P::NEST];
#pragma unroll
        for (int j = 0; j < P::NREF; ++j) rv[j] = load4<VEC>(rb + (size_t)j * T, t, len);
#pragma unroll
        for (int i = 0; i < P::NEST; ++i) ev[i] = load4<VEC>(eb + (size_t)i * T, t, len);
#pragma unroll
        for (int k = 0; k < 4; ++k) P::accumulate(acc, rv, ev, k);
    }
    const double s = reduce_partials<NV>(acc, red);
    if (tid < NV) partial[((size_t)b * nchunk + ch) * NV + tid] = s;
}

// The head of an iteration `for (b0 = 0; b0 < B; b0 += NTA / 64) { b = b0 + wave; ...` of an assignment kernel: lanes < nv of the
// wave sum moment `lane` of utterance b over the chunks, ascending, into mo_w[lane].  Both barriers are reached by every wave, so
// the loop's trip count must be block-uniform, and a wave without an utterance (b >= B) may only `continue` after the last barrier
// of its iteration.
__device__ __forceinline__ void sum_chunks_to_lds(const double* partial, int b, int B, int nv, int nchunk,
                                                  double* mo_w) {
    const int lane = threadIdx.x & 63;
    __syncthreads();                          // mo_w and what was derived from it may still be read for the previous utterance
    if (b < B && lane < nv) {
        double s = 0.0;
        for (int ch = 0; ch < nchunk; ++ch) s += partial[((size_t)b * nchunk + ch) * nv + lane];
        mo_w[lane] = s;
    }
    __syncthreads();
}

// First minimum over the wave: smaller L wins, equal L -> smaller idx; lanes without a candidate carry idx = none.  Every lane
// returns the winner.  A lane that enumerates its candidates lane, lane + 64, ... in ascending order and keeps ITS first minimum
// holds the winner's other results too when it is lane idx & 63: the winner is the first of all candidates to attain the minimum,
// hence also the first of that lane's, and so the lane's own pick.  A payload is fetched from there afterwards
// (__shfl(v, idx & 63, 64)) rather than carried through the butterfly.
__device__ __forceinline__ void wave_first_min(double& L, int& idx, int none) {
    double bestL = L;
    int best = idx;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double oL = __shfl_xor(bestL, o, 64);
        const int oi = __shfl_xor(best, o, 64);
        const bool take = oi < none && (best == none || oL < bestL || (oL == bestL && oi < best));
        if (take) { bestL = oL; best = oi; }
    }
    L = bestL;
    idx = best;
}

// The tail of an assignment kernel: `local` is lane 0's sum of its wave's per-utterance losses in ascending b; loss[0] = their
// sum over the waves, ascending, over B.
__device__ __forceinline__ void mean_over_waves(double local, double (&wsum)[NTA / 64], int B, float* loss) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wsum[w] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = wsum[0];
#pragma unroll
        for (int k = 1; k < NTA / 64; ++k) tot += wsum[k];
        loss[0] = (float)(tot / (double)B);
    }
}

// d objective / d per_utt[b] of g_loss * loss + sum g_per * per_utt; either pointer may be null.  One rounding per operation.
__device__ __forceinline__ float upstream_scale(const float* g_loss, const float* g_per, int b, int B) {
    float scale = 0.f;
    if (g_loss != nullptr) scale = g_loss[0] / (float)B;
    if (g_per != nullptr) scale += g_per[b];
    return scale;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
inline int moment_chunk(int T, int nchunk) { return ctn_cdiv(ctn_cdiv(T, nchunk), 4) * 4; }
inline int bwd_tiles(int T) { return ctn_cdiv(ctn_cdiv(T, 4), NT); }

// f(std::integral_constant<int, N>) for N = n; n outside LO .. HI (the callers have refused it already) takes HI
template <int LO, int HI, class F>
inline void dispatch_n(int n, F&& f) {
    if constexpr (LO < HI) {
        if (n == LO) return f(std::integral_constant<int, LO>{});
        dispatch_n<LO + 1, HI>(n, f);
    } else {
        f(std::integral_constant<int, HI>{});
    }
}

template <class P>
void launch_moment_sweep(const float* refs, const float* est, const long long* lens, int B, int T, int nchunk, double* partial,
                         hipStream_t st) {
    const bool vec = (T % 4 == 0) && ctn_aligned16(refs) && ctn_aligned16(est);
    auto kernel = vec ? &moment_sweep_kernel<P, true> : &moment_sweep_kernel<P, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(B * nchunk)), dim3(NT), 0, st, refs, est, lens, T, moment_chunk(T, nchunk), nchunk,
                       partial);
}

// The guards the entry points share.  grid_guard: a grid of B * blocks (`what` names them) and T + 4 NT fit an int.
// workspace_guard: the forward's workspace is there and holds `need` bytes.
inline int grid_guard(const char* fn, const char* what, int B, int blocks, int T) {
    CTN_REQUIRE((long long)B * blocks < (1ll << 31) && (long long)T + 4 * NT < (1ll << 31), "%s: B * %s or T too large", fn, what);
    return CTN_OK;
}
inline int workspace_guard(const char* fn, const void* workspace, size_t workspace_bytes, size_t need) {
    if (workspace == nullptr || workspace_bytes < need) {
        ctn_set_error("%s: workspace too small", fn);
        return CTN_ERR_WORKSPACE;
    }
    return CTN_OK;
}

}  // namespace
