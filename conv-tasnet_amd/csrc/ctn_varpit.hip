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
// The sweep, the reductions, the first-minimum rule and the load and store paths are the skeleton of ctn_moment_loss.h, shared
// with ctn_mixit.hip; it keeps the promise that an utterance's result is bitwise the same in any batch, at any batch index and at
// any alignment.  This file holds this loss's own algebra: which moments, the pair losses and active flags, the C! enumeration,
// the coefficients and the backward body.
#include "ctn_moment_loss.h"

namespace {

constexpr int MINC = 2, MAXC = 6;
constexpr double EPSD = 1e-8;

__host__ __device__ constexpr int nmom(int C) { return C * C + 2 * C + 1; }
__host__ __device__ constexpr int es_at(int C, int i, int j) { return i * C + j; }
__host__ __device__ constexpr int ss_at(int C, int j) { return C * C + j; }
__host__ __device__ constexpr int ee_at(int C, int i) { return C * C + C + i; }
__host__ __device__ constexpr int xx_at(int C) { return C * C + 2 * C; }
constexpr int nfact(int C) { return C <= 1 ? 1 : C * nfact(C - 1); }

// acc + m * m in two roundings.  Every other product of the sweep is one of two fp32 values and exact in fp64, so a fused and an
// unfused multiply-add give the same bits there; this one is not, and is kept unfused in both load paths.
__device__ __forceinline__ double add_square(double acc, double m) {
#pragma clang fp contract(off)
    const double p = m * m;
    return acc + p;
}

// the sweep's policy: the rows s [C,T] and e [C,T] of an utterance, sample k of the loaded quads
template <int C>
struct VarpitMoments {
    static constexpr int NREF = C, NEST = C, NV = nmom(C);
    static __device__ __forceinline__ void accumulate(double (&acc)[NV], const Quad (&sv)[C], const Quad (&ev)[C], int k) {
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
};

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
        sum_chunks_to_lds(partial, b, B, nv, nchunk, mo[w]);      // its first barrier also guards pl[w], pd[w]
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
        wave_first_min(bestL, bestp, nperm);
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
    mean_over_waves(local, wsum, B, loss);
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
    const int len = clamped_len(lens, b, T);
    long long p = idx[b];
    if (p < 0) p = 0;
    if (p >= nfact(C)) p = nfact(C) - 1;
    const float scale = upstream_scale(g_loss, g_per, b, B) / (float)C;
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
        store4<VEC>(db + (size_t)i * T + t, o, t, T);
    }
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
    if (const int rc = grid_guard("ctn_varpit_fwd", "chunks", B, nchunk, T)) return rc;
    if (const int rc = workspace_guard("ctn_varpit_fwd", workspace, workspace_bytes, ctn_varpit_workspace(B, C, T))) return rc;
    hipStream_t st = (hipStream_t)stream;
    dispatch_n<MINC, MAXC>(C, [&](auto c) {
        launch_moment_sweep<VarpitMoments<decltype(c)::value>>(sources, estimates, lengths, B, T, nchunk, (double*)workspace, st);
    });
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
    const int ntile = bwd_tiles(T);
    if (const int rc = grid_guard("ctn_varpit_bwd", "tiles", B, ntile, T)) return rc;
    const bool vec = (T % 4 == 0) && ctn_aligned16(sources) && ctn_aligned16(estimates) && ctn_aligned16(d_estimates);
    dispatch_n<MINC, MAXC>(C, [&](auto c) {
        constexpr int CC = decltype(c)::value;
        auto kernel = vec ? &varpit_bwd_kernel<CC, true> : &varpit_bwd_kernel<CC, false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)(B * ntile)), dim3(NT), 0, (hipStream_t)stream, sources, estimates, lengths, perms,
                           perm_idx, coef, g_loss, g_per, B, T, ntile, d_estimates);
    });
    CTN_CHECK_LAUNCH("ctn_varpit_bwd");
    return CTN_OK;
}

}  // extern "C"
