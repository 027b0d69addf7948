// Permutation invariant training with inactive sources: a C-output model trained on mixtures of 1 .. C speakers (Wisdom et al.,
// "What's all the FUSS about free universal sound separation data?", ICASSP 2021), gfx950.
//
// s [B,C,T] are the references (a row may be all zeros), e [B,C,T] the model's outputs, 2 <= C <= 6.  Reference j is active iff
// Ss_j = sum s_j^2 > 0.  Estimate i against reference j costs
//     active:    l_ij = 10 log10((max(Ss_j - 2 Es_ij + Ee_i, 0) + tau Ss_j + EPS) / (Ss_j + EPS))     the soft-thresholded -SNR
//     inactive:  l_ij = 10 log10((Ee_i + tau0 Xx + EPS) / (Xx + EPS))                                  the output's level in the mixture
// with Xx = sum_t (sum_j s_j[t])^2 the energy of the clean mixture, and the loss of an utterance is the minimum over the C!
// permutations p of L(p) = sum_i l_{i,p(i)} / C (first minimum in table order).
//
// Pass 1 (HBM-bound): one sweep over s and e accumulating, per utterance and time chunk, the fp64 moments over t < len:
//   Es[i][j] = sum e_i s_j, Ss[j], Ee[i], Xx  (C^2 + 2C + 1 values, 49 at C = 6).
// Pass 2 (scalars): one wave per utterance sums the chunk partials in a fixed order, lanes < C^2 evaluate the pair losses, the lanes
//   share the C! permutations, the first minimum is kept, and per_utt, idx, pair, active, the mean loss and the backward
//   coefficients are emitted.
// Backward: d_e[b,i,t] = [t < len] * scale_b / C * c_i * (e_i[t] - a_i s_j[t]),  j = perm_idx(i).
//
// The time partition and the lane that owns a sample depend on T alone, and the aligned (16 bytes per lane) and the scalar load
// paths add the same values in the same order, so an utterance's result is bitwise the same in any batch, at any batch index and
// at any alignment.
#include "ctn_common.h"

extern "C" int ctn_sisnr_chunks(int T);      // csrc/ctn_loss.hip: the time partition, a function of T alone

namespace {

constexpr int NT = 256;            // moments and backward kernels
constexpr int NTA = 1024;          // assignment kernel: 16 waves, one utterance per wave at a time
constexpr int MINC = 2, MAXC = 6;
constexpr double EPSD = 1e-8;

__host__ __device__ constexpr int nmom(int C) { return C * C + 2 * C + 1; }
__host__ __device__ constexpr int es_at(int C, int i, int j) { return i * C + j; }
__host__ __device__ constexpr int ss_at(int C, int j) { return C * C + j; }
__host__ __device__ constexpr int ee_at(int C, int i) { return C * C + C + i; }
__host__ __device__ constexpr int xx_at(int C) { return C * C + 2 * C; }
constexpr int nfact(int C) { return C <= 1 ? 1 : C * nfact(C - 1); }

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

// acc + m * m in two roundings.  Every other product of the sweep is one of two fp32 values and exact in fp64, so a fused and an
// unfused multiply-add give the same bits there; this one is not, and is kept unfused in both load paths.
__device__ __forceinline__ double add_square(double acc, double m) {
#pragma clang fp contract(off)
    const double p = m * m;
    return acc + p;
}

// partial[b][chunk][nmom(C)]; chunk % 4 == 0.  Lane tid owns the quads (t0 + 4 tid) + 4 NT k of its chunk, in ascending k.
template <int C, bool VEC>
__global__ __launch_bounds__(NT) void varpit_moments_kernel(const float* __restrict__ s, const float* __restrict__ e,
                                                            const long long* __restrict__ lens, int T, int chunk, int nchunk,
                                                            double* __restrict__ partial) {
    constexpr int NV = nmom(C);
    __shared__ double red[NT / 64][NV];
    const int b = blockIdx.x / nchunk, ch = blockIdx.x % nchunk;
    const int tid = threadIdx.x;
    long long ll = lens[b];
    if (ll > T) ll = T;
    if (ll < 0) ll = 0;
    const int len = (int)ll;
    const int t0 = ch * chunk, t1 = min(min(t0 + chunk, T), len);
    const float* __restrict__ sb = s + (size_t)b * C * T;
    const float* __restrict__ eb = e + (size_t)b * C * T;
    double acc[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) acc[q] = 0.0;
    for (int t = t0 + 4 * tid; t < t1; t += 4 * NT) {
        Quad sv[C], ev[C];
#pragma unroll
        for (int j = 0; j < C; ++j) sv[j] = load4<VEC>(sb + (size_t)j * T, t, len);
#pragma unroll
        for (int i = 0; i < C; ++i) ev[i] = load4<VEC>(eb + (size_t)i * T, t, len);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double sd[C];
            double mix = 0.0;
#pragma unroll
            for (int j = 0; j < C; ++j) {
                sd[j] = (double)sv[j].v[k];
                mix += sd[j];                                       // the clean mixture: ascending j
                acc[ss_at(C, j)] += sd[j] * sd[j];
            }
            acc[xx_at(C)] = add_square(acc[xx_at(C)], mix);
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const double ei = (double)ev[i].v[k];
                acc[ee_at(C, i)] += ei * ei;
#pragma unroll
                for (int j = 0; j < C; ++j) acc[es_at(C, i, j)] += ei * sd[j];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const double v = wave_sum(acc[q]);
        if ((tid & 63) == 0) red[tid >> 6][q] = v;
    }
    __syncthreads();
    if (tid < NV) {
        double r = red[0][tid];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) r += red[w][tid];
        partial[((size_t)b * nchunk + ch) * NV + tid] = r;
    }
}

// One block of 16 waves; wave w takes utterances w, w + 16, ...  pair [B,C,C], active [B,C], coef [B,C,2].
__global__ __launch_bounds__(NTA) void varpit_assign_kernel(const double* __restrict__ partial, const int* __restrict__ perms,
                                                            int nperm, int B, int C, int nchunk, double tau, double tau0,
                                                            float* __restrict__ per_utt, long long* __restrict__ idx,
                                                            float* __restrict__ pair, int* __restrict__ active,
                                                            float* __restrict__ loss, float* __restrict__ coef) {
    constexpr int NW = NTA / 64;
    __shared__ double mo[NW][nmom(MAXC)];
    __shared__ double pl[NW][MAXC * MAXC];    // l_ij
    __shared__ double pd[NW][MAXC * MAXC];    // D_ij: the numerator argument of l_ij
    __shared__ double wsum[NW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nv = nmom(C), cc = C * C;
    double local = 0.0;                       // lane 0: sum of this wave's per-utterance losses, ascending b
    for (int b0 = 0; b0 < B; b0 += NW) {      // block-uniform trip count: the barriers below are reached by every wave
        const int b = b0 + w;
        __syncthreads();                      // mo[w], pl[w], pd[w] may still be read for the previous utterance
        if (b < B && lane < nv) {
            double r = 0.0;
            for (int ch = 0; ch < nchunk; ++ch) r += partial[((size_t)b * nchunk + ch) * nv + lane];
            mo[w][lane] = r;
        }
        __syncthreads();
        const double* m = mo[w];
        if (b < B && lane < cc) {
            const int i = lane / C, j = lane % C;
            const double ss = m[ss_at(C, j)], ee = m[ee_at(C, i)], xx = m[xx_at(C)];
            double d, den;
            if (ss > 0.0) {
                d = fmax(ss - 2.0 * m[es_at(C, i, j)] + ee, 0.0) + tau * ss + EPSD;
                den = ss + EPSD;
            } else {                          // the same value for every inactive j
                d = ee + tau0 * xx + EPSD;
                den = xx + EPSD;
            }
            const double l = 10.0 * log10(d / den);
            pl[w][lane] = l;
            pd[w][lane] = d;
            pair[(size_t)b * cc + lane] = (float)l;
        }
        __syncthreads();
        if (b >= B) continue;
        double bestL = 0.0;
        int bestp = nperm;                    // nperm: this lane has seen no permutation yet
        for (int p = lane; p < nperm; p += 64) {
            double sum = 0.0;
            for (int i = 0; i < C; ++i) {     // ascending i: permutations of one tie class add the same values in the same order
                const int j = min(max(perms[p * C + i], 0), C - 1);
                sum += pl[w][i * C + j];
            }
            const double L = sum / (double)C;
            if (bestp == nperm || L < bestL) { bestL = L; bestp = p; }
        }
        // first minimum over the wave: smaller L wins, equal L -> smaller p (lanes without a permutation carry p = nperm)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double oL = __shfl_xor(bestL, o, 64);
            const int op = __shfl_xor(bestp, o, 64);
            const bool take = op < nperm && (bestp == nperm || oL < bestL || (oL == bestL && op < bestp));
            if (take) { bestL = oL; bestp = op; }
        }
        if (lane < C) {
            const int j = min(max(perms[bestp * C + lane], 0), C - 1);
            const bool act = m[ss_at(C, j)] > 0.0;
            const double c20 = 20.0 / log(10.0);
            coef[2 * ((size_t)b * C + lane)] = (float)(c20 / pd[w][lane * C + j]);
            coef[2 * ((size_t)b * C + lane) + 1] = act ? 1.f : 0.f;
            active[(size_t)b * C + lane] = m[ss_at(C, lane)] > 0.0 ? 1 : 0;
        }
        if (lane == 0) {
            per_utt[b] = (float)bestL;
            idx[b] = (long long)bestp;
            local += bestL;
        }
    }
    if (lane == 0) wsum[w] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = wsum[0];
#pragma unroll
        for (int k = 1; k < NW; ++k) tot += wsum[k];
        loss[0] = (float)(tot / (double)B);
    }
}

// Each lane takes four consecutive samples of one utterance: reads the C estimate rows and the paired active reference rows,
// writes the C rows of d_e.  One rounding per operation.
template <int C, bool VEC>
__global__ __launch_bounds__(NT) void varpit_bwd_kernel(const float* __restrict__ s, const float* __restrict__ e,
                                                        const long long* __restrict__ lens, const int* __restrict__ perms,
                                                        const long long* __restrict__ idx, const float* __restrict__ coef,
                                                        const float* __restrict__ g_loss, const float* __restrict__ g_per, int B,
                                                        int T, int ntile, float* __restrict__ de) {
#pragma clang fp contract(off)
    const int b = blockIdx.x / ntile, tile = blockIdx.x % ntile;
    const int t = (tile * NT + threadIdx.x) * 4;
    if (t >= T) return;
    long long ll = lens[b];
    if (ll > T) ll = T;
    if (ll < 0) ll = 0;
    const int len = (int)ll;
    long long p = idx[b];
    if (p < 0) p = 0;
    if (p >= nfact(C)) p = nfact(C) - 1;
    float scale = 0.f;
    if (g_loss != nullptr) scale = g_loss[0] / (float)B;
    if (g_per != nullptr) scale += g_per[b];
    scale = scale / (float)C;
    const float* __restrict__ sb = s + (size_t)b * C * T;
    const float* __restrict__ eb = e + (size_t)b * C * T;
    float* __restrict__ db = de + (size_t)b * C * T;
#pragma unroll
    for (int i = 0; i < C; ++i) {
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if (t < len) {
            const int j = min(max(perms[(int)p * C + i], 0), C - 1);
            const float wi = scale * coef[2 * ((size_t)b * C + i)];
            const bool act = coef[2 * ((size_t)b * C + i) + 1] != 0.f;
            const Quad ev = load4<VEC>(eb + (size_t)i * T, t, len);
            Quad sv;
#pragma unroll
            for (int k = 0; k < 4; ++k) sv.v[k] = 0.f;
            if (act) sv = load4<VEC>(sb + (size_t)j * T, t, len);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float r = act ? ev.v[k] - sv.v[k] : ev.v[k];
                o[k] = t + k < len ? wi * r : 0.f;
            }
        }
        float* __restrict__ dst = db + (size_t)i * T + t;
        if (VEC) {                              // T % 4 == 0: the whole quad is inside the row
            *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (t + k < T) dst[k] = o[k];
        }
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

inline int varpit_chunk(int T, int nchunk) { return ctn_cdiv(ctn_cdiv(T, nchunk), 4) * 4; }

template <int C>
void launch_moments(bool vec, unsigned grid, hipStream_t st, const float* s, const float* e, const long long* lens, int T,
                    int chunk, int nchunk, double* partial) {
    if (vec)
        hipLaunchKernelGGL((varpit_moments_kernel<C, true>), dim3(grid), dim3(NT), 0, st, s, e, lens, T, chunk, nchunk, partial);
    else
        hipLaunchKernelGGL((varpit_moments_kernel<C, false>), dim3(grid), dim3(NT), 0, st, s, e, lens, T, chunk, nchunk, partial);
}

template <int C>
void launch_bwd(bool vec, unsigned grid, hipStream_t st, const float* s, const float* e, const long long* lens, const int* perms,
                const long long* idx, const float* coef, const float* g_loss, const float* g_per, int B, int T, int ntile,
                float* de) {
    if (vec)
        hipLaunchKernelGGL((varpit_bwd_kernel<C, true>), dim3(grid), dim3(NT), 0, st, s, e, lens, perms, idx, coef, g_loss, g_per,
                           B, T, ntile, de);
    else
        hipLaunchKernelGGL((varpit_bwd_kernel<C, false>), dim3(grid), dim3(NT), 0, st, s, e, lens, perms, idx, coef, g_loss, g_per,
                           B, T, ntile, de);
}

#define VARPIT_DISPATCH(C, CALL)                \
    switch (C) {                                \
        case 2: CALL(2); break;                 \
        case 3: CALL(3); break;                 \
        case 4: CALL(4); break;                 \
        case 5: CALL(5); break;                 \
        default: CALL(6); break;                \
    }

inline int host_fact(int C) { int f = 1; for (int k = 2; k <= C; ++k) f *= k; return f; }

}  // namespace

extern "C" {

size_t ctn_varpit_workspace(int B, int C, int T) {
    if (B <= 0 || C < MINC || C > MAXC || T <= 0) return 0;
    return (size_t)B * ctn_sisnr_chunks(T) * nmom(C) * sizeof(double);
}

// see include/ctn_hip.h
int ctn_varpit_fwd(const float* sources, const float* estimates, const long long* lengths, const int* perms, int nperm, int B,
                   int C, int T, double tau, double tau0, float* per_utt, long long* perm_idx, float* pair, int* active,
                   float* loss, float* coef, void* workspace, size_t workspace_bytes, void* stream) {
    CTN_REQUIRE(sources && estimates && lengths && perms && per_utt && perm_idx && pair && active && loss && coef,
                "ctn_varpit_fwd: null pointer");
    CTN_REQUIRE(C >= MINC && C <= MAXC, "ctn_varpit_fwd: C = %d outside %d .. %d", C, MINC, MAXC);
    CTN_REQUIRE(nperm == host_fact(C), "ctn_varpit_fwd: nperm = %d, C! = %d permutations are needed", nperm, host_fact(C));
    CTN_REQUIRE(B > 0 && T > 0 && tau >= 0.0 && tau0 >= 0.0, "ctn_varpit_fwd: bad sizes (B = %d, T = %d) or a threshold < 0", B, T);
    const int nchunk = ctn_sisnr_chunks(T);
    CTN_REQUIRE((long long)B * nchunk < (1ll << 31) && (long long)T + 4 * NT < (1ll << 31), "ctn_varpit_fwd: B * chunks or T too large");
    if (workspace == nullptr || workspace_bytes < ctn_varpit_workspace(B, C, T)) {
        ctn_set_error("ctn_varpit_fwd: workspace too small");
        return CTN_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (T % 4 == 0) && aligned16(sources) && aligned16(estimates);
    const int chunk = varpit_chunk(T, nchunk);
    const unsigned grid = (unsigned)(B * nchunk);
#define CALL(CC) launch_moments<CC>(vec, grid, st, sources, estimates, lengths, T, chunk, nchunk, (double*)workspace)
    VARPIT_DISPATCH(C, CALL)
#undef CALL
    CTN_CHECK_LAUNCH("ctn_varpit_fwd/moments");
    hipLaunchKernelGGL(varpit_assign_kernel, dim3(1), dim3(NTA), 0, st, (const double*)workspace, perms, nperm, B, C, nchunk, tau,
                       tau0, per_utt, perm_idx, pair, active, loss, coef);
    CTN_CHECK_LAUNCH("ctn_varpit_fwd/assign");
    return CTN_OK;
}

int ctn_varpit_bwd(const float* sources, const float* estimates, const long long* lengths, const int* perms,
                   const long long* perm_idx, const float* coef, const float* g_loss, const float* g_per, int B, int C, int T,
                   float* d_estimates, void* stream) {
    CTN_REQUIRE(sources && estimates && lengths && perms && perm_idx && coef && d_estimates, "ctn_varpit_bwd: null pointer");
    CTN_REQUIRE(C >= MINC && C <= MAXC, "ctn_varpit_bwd: C = %d outside %d .. %d", C, MINC, MAXC);
    CTN_REQUIRE(B > 0 && T > 0, "ctn_varpit_bwd: bad sizes (B = %d, T = %d)", B, T);
    const int ntile = ctn_cdiv(ctn_cdiv(T, 4), NT);
    CTN_REQUIRE((long long)B * ntile < (1ll << 31) && (long long)T + 4 * NT < (1ll << 31), "ctn_varpit_bwd: B * tiles or T too large");
    const bool vec = (T % 4 == 0) && aligned16(sources) && aligned16(estimates) && aligned16(d_estimates);
    const unsigned grid = (unsigned)(B * ntile);
    hipStream_t st = (hipStream_t)stream;
#define CALL(CC) launch_bwd<CC>(vec, grid, st, sources, estimates, lengths, perms, perm_idx, coef, g_loss, g_per, B, T, ntile, d_estimates)
    VARPIT_DISPATCH(C, CALL)
#undef CALL
    CTN_CHECK_LAUNCH("ctn_varpit_bwd");
    return CTN_OK;
}

}  // extern "C"
