// On-device dynamic mixing: levels of a ragged corpus, the minibatch plan (Philox4x32-10), the gather / mix / peak-rescale.
// Contract: include/ctn_hip.h ("on-device dynamic mixing"); executable restatement: tests/dynmix_oracle.py.
// Every float32 operation of the gather is ONE rounding in a stated order (no contraction into fused multiply-adds, IEEE
// division), so the minibatch is a bitwise function of the plan and the corpus.
#include "ctn_dynmix_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int DM_WIDE_NT = 1024;    // threads of the one-workgroup-per-mixture gather

// ---- levels ------------------------------------------------------------------------------------------------------------
// One workgroup per utterance.  Thread t sums the squares of samples t, t + NT, t + 2 NT, ... in fp64, then the fixed-order
// block sum: the partition is a function of the utterance's own length only.
__global__ __launch_bounds__(DM_NT) void dynmix_levels_kernel(const float* __restrict__ corpus, const long long* __restrict__ offsets,
                                                              const long long* __restrict__ lens, long long num_samples,
                                                              double* __restrict__ meansq) {
    __shared__ double scratch[DM_NT / 64];
    const long long u = blockIdx.x;
    const long long n = lens[u], off = offsets[u];
    if (off < 0 || n < 0 || off + n > num_samples) {        // a table entry outside the corpus buffer: flagged, never read
        if (threadIdx.x == 0) meansq[u] = -1.0;
        return;
    }
    const float* __restrict__ x = corpus + off;
    double acc = 0.0;
    for (long long i = threadIdx.x; i < n; i += DM_NT) {
        const double v = (double)x[i];
        acc += v * v;
    }
    acc = block_sum<double, DM_NT>(acc, scratch);
    if (threadIdx.x == 0) meansq[u] = n > 0 ? acc / (double)n : 0.0;
}

// ---- plan --------------------------------------------------------------------------------------------------------------
// One workgroup; thread b draws mixture b (and b + NT, ...).  Every thread reads the step word before the barrier, thread 0
// advances it behind the barrier.
__global__ __launch_bounds__(DM_NT) void dynmix_plan_kernel(const int* __restrict__ spk_ptr, const int* __restrict__ utt_ids, int S,
                                                            const long long* __restrict__ lens, const float* __restrict__ inv_rms,
                                                            const float* __restrict__ w, unsigned k0, unsigned k1, unsigned epoch,
                                                            unsigned* step_word, int B, int C, int seg_len,
                                                            int* __restrict__ plan_utt, long long* __restrict__ plan_start,
                                                            int* __restrict__ plan_q, float* __restrict__ gain) {
    const unsigned step = *step_word;
    for (int b = threadIdx.x; b < B; b += DM_NT) {
        int taken[4];
        int q0 = 0;
        for (int c = 0; c < C; ++c) {
            const Philox4 r = philox4x32_10((unsigned)c, (unsigned)b, step, epoch, k0, k1);
            // speaker: uniform among the S - c not taken yet; step over the taken ones in ascending order
            int s = (int)below(r.w[0], (unsigned long long)(S - c));
            for (int i = 0; i < c; ++i)
                if (s >= taken[i]) ++s;
            int pos = c;                              // keep `taken` ascending
            while (pos > 0 && taken[pos - 1] > s) { taken[pos] = taken[pos - 1]; --pos; }
            taken[pos] = s;
            const int first = spk_ptr[s], count = spk_ptr[s + 1] - first;
            const int o = b * C + c;
            const int u = count > 0 ? utt_ids[first + (int)below(r.w[1], (unsigned long long)count)] : -1;
            if (u < 0 || lens[u] < seg_len) {         // tables that break their contract: an entry the gather flags (peak = -1)
                plan_utt[o] = -1;
                plan_start[o] = 0;
                plan_q[o] = 0;
                gain[o] = 0.0f;
                continue;
            }
            const long long start = (long long)below(r.w[2], (unsigned long long)(lens[u] - seg_len + 1));
            int q;
            if (c == 0) {
                q = q0 = 1 + (int)below(r.w[3], 249ull);
            } else if (c == 1) {
                q = -q0;
            } else {
                const int v = (int)below(r.w[3], 498ull);
                q = v < 249 ? 1 + v : -(1 + (v - 249));
            }
            plan_utt[o] = u;
            plan_start[o] = start;
            plan_q[o] = q;
            gain[o] = __fmul_rn(w[q + 249], inv_rms[u]);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) *step_word = step + 1u;
}

// The plan with speed perturbation: the draws of dynmix_plan_kernel from the same Philox block, plus one more block per source,
// counter (c + 256, b, step, epoch), whose word 0 picks the speed percent.  The start is drawn over the
// need = ceil(seg_len * pct / 100) input samples the resampled segment spans.
__global__ __launch_bounds__(DM_NT) void dynmix_plan_speed_kernel(const int* __restrict__ spk_ptr, const int* __restrict__ utt_ids, int S,
                                                                  const long long* __restrict__ lens, const float* __restrict__ inv_rms,
                                                                  const float* __restrict__ w, const int* __restrict__ pct_tab, int npct,
                                                                  unsigned k0, unsigned k1, unsigned epoch, unsigned* step_word, int B, int C,
                                                                  int seg_len, int* __restrict__ plan_utt, long long* __restrict__ plan_start,
                                                                  int* __restrict__ plan_q, float* __restrict__ gain, int* __restrict__ plan_pct) {
    const unsigned step = *step_word;
    for (int b = threadIdx.x; b < B; b += DM_NT) {
        int taken[4];
        int q0 = 0;
        for (int c = 0; c < C; ++c) {
            const Philox4 r = philox4x32_10((unsigned)c, (unsigned)b, step, epoch, k0, k1);
            const Philox4 rs = philox4x32_10((unsigned)c + 256u, (unsigned)b, step, epoch, k0, k1);
            const int pct = pct_tab[below(rs.w[0], (unsigned long long)npct)];
            const long long need = ((long long)seg_len * pct + 99) / 100;
            int s = (int)below(r.w[0], (unsigned long long)(S - c));
            for (int i = 0; i < c; ++i)
                if (s >= taken[i]) ++s;
            int pos = c;                              // keep `taken` ascending
            while (pos > 0 && taken[pos - 1] > s) { taken[pos] = taken[pos - 1]; --pos; }
            taken[pos] = s;
            const int first = spk_ptr[s], count = spk_ptr[s + 1] - first;
            const int o = b * C + c;
            const int u = count > 0 ? utt_ids[first + (int)below(r.w[1], (unsigned long long)count)] : -1;
            if (u < 0 || need < 1 || lens[u] < need) { // tables that break their contract: an entry the segments kernel flags
                plan_utt[o] = -1;
                plan_start[o] = 0;
                plan_q[o] = 0;
                gain[o] = 0.0f;
                plan_pct[o] = 100;
                continue;
            }
            const long long start = (long long)below(r.w[2], (unsigned long long)(lens[u] - need + 1));
            int q;
            if (c == 0) {
                q = q0 = 1 + (int)below(r.w[3], 249ull);
            } else if (c == 1) {
                q = -q0;
            } else {
                const int v = (int)below(r.w[3], 498ull);
                q = v < 249 ? 1 + v : -(1 + (v - 249));
            }
            plan_utt[o] = u;
            plan_start[o] = start;
            plan_q[o] = q;
            gain[o] = __fmul_rn(w[q + 249], inv_rms[u]);
            plan_pct[o] = pct;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) *step_word = step + 1u;
}

// ---- gather ------------------------------------------------------------------------------------------------------------
template <int C>
struct Rows {
    const float* src[C];    // first sample of the segment of source c
    float g[C];
    bool bad;               // a plan entry points outside its utterance: the source reads as silence, peak[b] = -1
};

template <int C>
__device__ __forceinline__ Rows<C> load_rows(const float* __restrict__ corpus, const long long* __restrict__ offsets,
                                             const long long* __restrict__ lens, int U, const int* __restrict__ plan_utt,
                                             const long long* __restrict__ plan_start, const float* __restrict__ gain, int b, int T) {
    Rows<C> r;
    r.bad = false;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int u = plan_utt[b * C + c];
        const long long st = plan_start[b * C + c];
        const bool ok = u >= 0 && u < U && st >= 0 && st + (long long)T <= lens[u < 0 || u >= U ? 0 : u];
        r.src[c] = ok ? corpus + offsets[u] + st : nullptr;
        r.g[c] = gain[b * C + c];
        r.bad = r.bad || !ok;
    }
    return r;
}

// s_c[t] and mix[t] of one sample, each operation rounded once
template <int C>
__device__ __forceinline__ float mix_one(const Rows<C>& r, int t, float (&s)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = r.src[c] != nullptr ? __fmul_rn(r.g[c], r.src[c][t]) : 0.0f;
    float m = __fadd_rn(s[0], s[1]);
#pragma unroll
    for (int c = 2; c < C; ++c) m = __fadd_rn(m, s[c]);
    return m;
}

// max over samples [t0, t1) of |mix| and every |s_c|, this thread's share: 4 consecutive samples per thread and round
template <int C>
__device__ __forceinline__ float range_absmax(const Rows<C>& r, int t0, int t1, int nt) {
    float a = 0.0f;
    for (int t4 = t0 + 4 * (int)threadIdx.x; t4 < t1; t4 += 4 * nt) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (t4 + k < t1) {
                float s[C];
                a = fmaxf(a, fabsf(mix_one<C>(r, t4 + k, s)));
#pragma unroll
                for (int c = 0; c < C; ++c) a = fmaxf(a, fabsf(s[c]));
            }
        }
    }
    return a;
}

// mixture[b, t] and sources[b, c, t] for samples [t0, t1); 16-byte stores where the rows are 16-byte aligned (T % 4 == 0)
template <int C>
__device__ __forceinline__ void range_write(const Rows<C>& r, float scale, int t0, int t1, int nt, int T, float* __restrict__ mixrow,
                                            float* __restrict__ srcrows) {
    const bool wide = (T & 3) == 0;
    for (int t4 = t0 + 4 * (int)threadIdx.x; t4 < t1; t4 += 4 * nt) {
        if (wide && t4 + 4 <= t1) {
            float m[4], s[4][C];
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = __fmul_rn(scale, mix_one<C>(r, t4 + k, s[k]));
            *reinterpret_cast<float4*>(mixrow + t4) = make_float4(m[0], m[1], m[2], m[3]);
#pragma unroll
            for (int c = 0; c < C; ++c)
                *reinterpret_cast<float4*>(srcrows + (long long)c * T + t4) =
                    make_float4(__fmul_rn(scale, s[0][c]), __fmul_rn(scale, s[1][c]), __fmul_rn(scale, s[2][c]), __fmul_rn(scale, s[3][c]));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (t4 + k < t1) {
                    float s[C];
                    mixrow[t4 + k] = __fmul_rn(scale, mix_one<C>(r, t4 + k, s));
#pragma unroll
                    for (int c = 0; c < C; ++c) srcrows[(long long)c * T + t4 + k] = __fmul_rn(scale, s[c]);
                }
            }
        }
    }
}

#define DM_GATHER_ARGS                                                                                                          \
    const float *__restrict__ corpus, const long long *__restrict__ offsets, const long long *__restrict__ lens, int U,         \
        const int *__restrict__ plan_utt, const long long *__restrict__ plan_start, const float *__restrict__ gain, int T

// chunked form, launch 1: wgmax[b, chunk] = the maximum over this workgroup's DM_CHUNK samples.  grid (nchunk, B)
template <int C>
__global__ __launch_bounds__(DM_NT) void dynmix_peak_kernel(DM_GATHER_ARGS, float* __restrict__ wgmax) {
    __shared__ float scratch[DM_NT / 64];
    const int b = blockIdx.y, t0 = blockIdx.x * DM_CHUNK;
    const Rows<C> r = load_rows<C>(corpus, offsets, lens, U, plan_utt, plan_start, gain, b, T);
    const float a = block_max<DM_NT>(range_absmax<C>(r, t0, min(T, t0 + DM_CHUNK), DM_NT), scratch);
    if (threadIdx.x == 0) wgmax[(long long)b * gridDim.x + blockIdx.x] = a;
}

// chunked form, launch 2: the maximum over the mixture's workgroup maxima, then the scaled samples (recomputed from the
// corpus: the same roundings, and 2 MB of re-reads that hit in L2 instead of 3 MB of unscaled outputs written and read back)
template <int C>
__global__ __launch_bounds__(DM_NT) void dynmix_write_kernel(DM_GATHER_ARGS, const float* __restrict__ wgmax, float over,
                                                             float* __restrict__ mixture, float* __restrict__ sources,
                                                             float* __restrict__ peak) {
    __shared__ float scratch[DM_NT / 64];
    const int b = blockIdx.y, t0 = blockIdx.x * DM_CHUNK, nchunk = gridDim.x;
    const Rows<C> r = load_rows<C>(corpus, offsets, lens, U, plan_utt, plan_start, gain, b, T);
    float a = 0.0f;
    for (int i = threadIdx.x; i < nchunk; i += DM_NT) a = fmaxf(a, wgmax[(long long)b * nchunk + i]);
    a = block_max<DM_NT>(a, scratch);
    if (blockIdx.x == 0 && threadIdx.x == 0) peak[b] = r.bad ? -1.0f : a;
    range_write<C>(r, peak_scale(a, over), t0, min(T, t0 + DM_CHUNK), DM_NT, T, mixture + (long long)b * T, sources + (long long)b * C * T);
}

// one-launch form: one workgroup per mixture, both phases in it
template <int C>
__global__ __launch_bounds__(DM_WIDE_NT) void dynmix_gather_wg_kernel(DM_GATHER_ARGS, float over, float* __restrict__ mixture,
                                                                      float* __restrict__ sources, float* __restrict__ peak) {
    __shared__ float scratch[DM_WIDE_NT / 64];
    const int b = blockIdx.x;
    const Rows<C> r = load_rows<C>(corpus, offsets, lens, U, plan_utt, plan_start, gain, b, T);
    const float a = block_max<DM_WIDE_NT>(range_absmax<C>(r, 0, T, DM_WIDE_NT), scratch);
    if (threadIdx.x == 0) peak[b] = r.bad ? -1.0f : a;
    range_write<C>(r, peak_scale(a, over), 0, T, DM_WIDE_NT, T, mixture + (long long)b * T, sources + (long long)b * C * T);
}

template <int C>
int gather_launch(DM_GATHER_ARGS, int B, float* mixture, float* sources, float* peak, float* wgmax, int mode, float over, hipStream_t st) {
    if (mode == 1) {
        dynmix_gather_wg_kernel<C><<<dim3(B), dim3(DM_WIDE_NT), 0, st>>>(corpus, offsets, lens, U, plan_utt, plan_start, gain, T, over,
                                                                        mixture, sources, peak);
        CTN_CHECK_LAUNCH("ctn_dynmix_gather");
        return CTN_OK;
    }
    const dim3 grid(ctn_cdiv(T, DM_CHUNK), B);
    dynmix_peak_kernel<C><<<grid, dim3(DM_NT), 0, st>>>(corpus, offsets, lens, U, plan_utt, plan_start, gain, T, wgmax);
    CTN_CHECK_LAUNCH("ctn_dynmix_gather (peak)");
    dynmix_write_kernel<C><<<grid, dim3(DM_NT), 0, st>>>(corpus, offsets, lens, U, plan_utt, plan_start, gain, T, wgmax, over, mixture,
                                                        sources, peak);
    CTN_CHECK_LAUNCH("ctn_dynmix_gather (write)");
    return CTN_OK;
}

}  // namespace

extern "C" {

int ctn_dynmix_levels(const float* corpus, long long num_samples, const long long* offsets, const long long* lens, long long U,
                      double* meansq, void* stream) {
    CTN_REQUIRE(corpus && offsets && lens && meansq, "ctn_dynmix_levels: null pointer");
    CTN_REQUIRE(U >= 1 && U <= 0x7fffffffLL, "ctn_dynmix_levels: U = %lld utterances (1 .. 2^31 - 1)", U);
    CTN_REQUIRE(num_samples >= 1, "ctn_dynmix_levels: num_samples = %lld", num_samples);
    dynmix_levels_kernel<<<dim3((unsigned)U), dim3(DM_NT), 0, (hipStream_t)stream>>>(corpus, offsets, lens, num_samples, meansq);
    CTN_CHECK_LAUNCH("ctn_dynmix_levels");
    return CTN_OK;
}

int ctn_dynmix_plan(const int* spk_ptr, const int* utt_ids, int S, const long long* lens, const float* inv_rms, const float* w,
                    long long seed, int epoch, int rank, unsigned* step, int B, int C, int seg_len, int* plan_utt,
                    long long* plan_start, int* plan_q, float* gain, void* stream) {
    CTN_REQUIRE(spk_ptr && utt_ids && lens && inv_rms && w && step && plan_utt && plan_start && plan_q && gain,
                "ctn_dynmix_plan: null pointer");
    CTN_REQUIRE(C >= 2 && C <= 4, "ctn_dynmix_plan: C = %d sources per mixture (2 .. 4)", C);
    CTN_REQUIRE(S >= C, "ctn_dynmix_plan: %d speakers for mixtures of %d", S, C);
    CTN_REQUIRE(B >= 1 && B <= (1 << 20), "ctn_dynmix_plan: B = %d mixtures (1 .. 2^20)", B);
    CTN_REQUIRE(seg_len >= 1, "ctn_dynmix_plan: seg_len = %d", seg_len);
    CTN_REQUIRE(seed >= 0 && seed < (1LL << 48), "ctn_dynmix_plan: seed %lld outside [0, 2^48)", seed);
    CTN_REQUIRE(rank >= 0 && rank < (1 << 16), "ctn_dynmix_plan: rank %d outside [0, 2^16)", rank);
    CTN_REQUIRE(epoch >= 0, "ctn_dynmix_plan: epoch %d", epoch);
    const unsigned k0 = (unsigned)(seed & 0xffffffffLL), k1 = (unsigned)(seed >> 32) | ((unsigned)rank << 16);
    dynmix_plan_kernel<<<dim3(1), dim3(DM_NT), 0, (hipStream_t)stream>>>(spk_ptr, utt_ids, S, lens, inv_rms, w, k0, k1, (unsigned)epoch, step,
                                                                         B, C, seg_len, plan_utt, plan_start, plan_q, gain);
    CTN_CHECK_LAUNCH("ctn_dynmix_plan");
    return CTN_OK;
}

int ctn_dynmix_plan_speed(const int* spk_ptr, const int* utt_ids, int S, const long long* lens, const float* inv_rms, const float* w,
                          const int* pct, int n, long long seed, int epoch, int rank, unsigned* step, int B, int C, int seg_len,
                          int* plan_utt, long long* plan_start, int* plan_q, float* gain, int* plan_pct, void* stream) {
    CTN_REQUIRE(spk_ptr && utt_ids && lens && inv_rms && w && pct && step && plan_utt && plan_start && plan_q && gain && plan_pct,
                "ctn_dynmix_plan_speed: null pointer");
    CTN_REQUIRE(n >= 1 && n <= 151, "ctn_dynmix_plan_speed: n = %d speed percents (1 .. 151)", n);
    CTN_REQUIRE(C >= 2 && C <= 4, "ctn_dynmix_plan_speed: C = %d sources per mixture (2 .. 4)", C);
    CTN_REQUIRE(S >= C, "ctn_dynmix_plan_speed: %d speakers for mixtures of %d", S, C);
    CTN_REQUIRE(B >= 1 && B <= (1 << 20), "ctn_dynmix_plan_speed: B = %d mixtures (1 .. 2^20)", B);
    CTN_REQUIRE(seg_len >= 1, "ctn_dynmix_plan_speed: seg_len = %d", seg_len);
    CTN_REQUIRE(seed >= 0 && seed < (1LL << 48), "ctn_dynmix_plan_speed: seed %lld outside [0, 2^48)", seed);
    CTN_REQUIRE(rank >= 0 && rank < (1 << 16), "ctn_dynmix_plan_speed: rank %d outside [0, 2^16)", rank);
    CTN_REQUIRE(epoch >= 0, "ctn_dynmix_plan_speed: epoch %d", epoch);
    const unsigned k0 = (unsigned)(seed & 0xffffffffLL), k1 = (unsigned)(seed >> 32) | ((unsigned)rank << 16);
    dynmix_plan_speed_kernel<<<dim3(1), dim3(DM_NT), 0, (hipStream_t)stream>>>(spk_ptr, utt_ids, S, lens, inv_rms, w, pct, n, k0, k1,
                                                                               (unsigned)epoch, step, B, C, seg_len, plan_utt, plan_start,
                                                                               plan_q, gain, plan_pct);
    CTN_CHECK_LAUNCH("ctn_dynmix_plan_speed");
    return CTN_OK;
}

size_t ctn_dynmix_gather_workspace(int B, int T) {
    if (B < 1 || T < 1) return 0;
    return sizeof(float) * (size_t)B * (size_t)ctn_cdiv(T, DM_CHUNK);
}

int ctn_dynmix_gather_peak(const float* corpus, const long long* offsets, const long long* lens, long long U, const int* plan_utt,
                           const long long* plan_start, const float* gain, int B, int C, int T, float* mixture, float* sources,
                           float* peak, void* workspace, size_t workspace_bytes, int mode, int peak_mode, void* stream);

// peak mode 0: the rule of every mixture before the LibriMix recipe, the same launches and bits
int ctn_dynmix_gather(const float* corpus, const long long* offsets, const long long* lens, long long U, const int* plan_utt,
                      const long long* plan_start, const float* gain, int B, int C, int T, float* mixture, float* sources,
                      float* peak, void* workspace, size_t workspace_bytes, int mode, void* stream) {
    return ctn_dynmix_gather_peak(corpus, offsets, lens, U, plan_utt, plan_start, gain, B, C, T, mixture, sources, peak, workspace,
                                  workspace_bytes, mode, 0, stream);
}

// see include/ctn_hip.h ("LibriMix-recipe mixing")
int ctn_dynmix_gather_peak(const float* corpus, const long long* offsets, const long long* lens, long long U, const int* plan_utt,
                           const long long* plan_start, const float* gain, int B, int C, int T, float* mixture, float* sources,
                           float* peak, void* workspace, size_t workspace_bytes, int mode, int peak_mode, void* stream) {
    CTN_REQUIRE(peak_mode == 0 || peak_mode == 1, "ctn_dynmix_gather: peak_mode %d (0: always rescale; 1: only what would clip)", peak_mode);
    CTN_REQUIRE(corpus && offsets && lens && plan_utt && plan_start && gain && mixture && sources && peak,
                "ctn_dynmix_gather: null pointer");
    CTN_REQUIRE(C >= 2 && C <= 4, "ctn_dynmix_gather: C = %d sources per mixture (2 .. 4)", C);
    CTN_REQUIRE(T >= 1, "ctn_dynmix_gather: seg_len = %d", T);
    CTN_REQUIRE(B >= 1 && B <= 65535, "ctn_dynmix_gather: B = %d mixtures (1 .. 65535)", B);
    CTN_REQUIRE(U >= 1 && U <= 0x7fffffffLL, "ctn_dynmix_gather: U = %lld utterances (1 .. 2^31 - 1)", U);
    CTN_REQUIRE(mode == 0 || mode == 1, "ctn_dynmix_gather: mode %d (0: chunked, two launches; 1: one workgroup per mixture)", mode);
    CTN_REQUIRE((((size_t)mixture | (size_t)sources) & 15) == 0, "ctn_dynmix_gather: mixture and sources must be 16-byte aligned");
    if (mode == 0) {
        CTN_REQUIRE(workspace != nullptr, "ctn_dynmix_gather: null workspace");
        if (workspace_bytes < ctn_dynmix_gather_workspace(B, T)) {
            ctn_set_error("ctn_dynmix_gather: workspace of %zu bytes, %zu needed", workspace_bytes, ctn_dynmix_gather_workspace(B, T));
            return CTN_ERR_WORKSPACE;
        }
    }
    const hipStream_t st = (hipStream_t)stream;
    float* const wg = (float*)workspace;
    const float over = peak_over(peak_mode);
    switch (C) {
        case 2: return gather_launch<2>(corpus, offsets, lens, (int)U, plan_utt, plan_start, gain, T, B, mixture, sources, peak, wg, mode, over, st);
        case 3: return gather_launch<3>(corpus, offsets, lens, (int)U, plan_utt, plan_start, gain, T, B, mixture, sources, peak, wg, mode, over, st);
        default: return gather_launch<4>(corpus, offsets, lens, (int)U, plan_utt, plan_start, gain, T, B, mixture, sources, peak, wg, mode, over, st);
    }
}

}  // extern "C"
