// Optimal-assignment PIT: the SI-SNR loss of ctn_loss.hip for 2 <= C <= 16 speakers, and the linear-assignment solver it is built
// on (Kuhn's Hungarian method in its shortest-augmenting-path form, O(C^3), in place of the C! enumeration), gfx950.
//
// s [B,C,T] are the references, e [B,C,T] the model's outputs; the estimate is NOT modified (as in ctn_mixit.hip, ctn_varpit.hip).
//
// Pass 1 (HBM-bound): per utterance and time chunk the raw fp64 moments over t < len: sum s_j, sum e_i, sum s_j^2, sum e_i^2 and
//   the C x C cross moments sum e_i s_j.  A tile of TK samples of the 2C rows goes through LDS (16-byte loads along t where the
//   rows are aligned, the scalar path of load4 where not); the cross moments are the [16 x TK] . [TK x 16] product on
//   v_mfma_f64_16x16x4_f64, rows >= C being zeros, and the row sums and squares are added in fp64 by the lanes that load the
//   row, in a fixed order.  Every product of two fp32 values is exact in fp64 and a zero sample adds an exact zero, so samples
//   at t >= len, the tail of a chunk and the rows >= C change no bit.
// Pass 2 (scalars): one wave per utterance sums the chunk partials in chunk order, centres the moments and forms snr[i][j] with
//   the algebra and the three EPS of sisnr_pit_kernel (ctn_loss.hip), stores pair = (float)snr, and solves the assignment on the
//   fp32-rounded matrix widened to fp64 (assign_solve below).  max_snr, loss = -mean, the backward coefficients and perm follow.
// Backward: de[b,i,t] = [t < len] * scale_b * (A (s_j[t] - mean s_j) + B (e_i[t] - mean e_i)), j = perm[b][i].
//
// The time partition, the first-minimum rule, the load and store paths and the fixed-order reductions are those of
// ctn_moment_loss.h: an utterance's result is bitwise the same in any batch, at any batch index and at any alignment.
#include "ctn_moment_loss.h"

namespace {

constexpr int MINC = 2, MAXC = 16;
constexpr int TK = 256;                  // samples per LDS tile: 64 k-steps of the MFMA
constexpr int LDW = TK + 4;              // row stride of a tile in floats: rows stay 16-byte aligned, 16 rows x 4 columns spread over the banks
constexpr int RPW = 2 * MAXC / (NT / 64);  // rows of a tile per wave
constexpr double EPSD = 1e-8;

typedef double double4_t __attribute__((ext_vector_type(4)));

// partial[b][chunk][nmom(C)]: the layout of ctn_loss.hip
__host__ __device__ constexpr int nmom(int C) { return 4 * C + C * C; }

// Wave w's rows (w, w + 4, ...; rows < C are references, rows C .. 2C - 1 estimates) of the tile at tt, one quad per lane.
template <bool VEC>
__device__ __forceinline__ void load_tile(const float* __restrict__ sb, const float* __restrict__ eb, int C, int T, int tt, int t1,
                                          Quad (&qv)[RPW]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int r = w + (NT / 64) * k;
        if (r < 2 * C) {
            const float* __restrict__ row = r < C ? sb + (size_t)r * T : eb + (size_t)(r - C) * T;
            qv[k] = load4<VEC>(row, tt + 4 * lane, t1);          // samples at or beyond t1 are zeros and are not read
        }
    }
}

// One block per (utterance, chunk).  The four waves take the k-steps w, w + 4, ... of every tile; their fragments are added in
// wave order at the end.  A row's sum and sum of squares are kept by the lanes that load it (wave r % 4, one quad per lane and
// tile, fp64, tiles ascending) and added over the wave once at the end: four more MFMAs per k-step would give them too (the
// diagonals of e e^T and s s^T, a column of e 1^T), and were measured 11 us slower at C = 2.
template <bool VEC>
__global__ __launch_bounds__(NT) void assign_moments_kernel(const float* __restrict__ src, const float* __restrict__ est,
                                                            const long long* __restrict__ lens, int C, int T, int chunk,
                                                            int nchunk, double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float ts[MAXC][LDW];
    __shared__ __attribute__((aligned(16))) float te[MAXC][LDW];
    __shared__ double red[NT / 64][MAXC * MAXC];
    __shared__ double rowm[4 * MAXC];                             // [0, 2C): the rows' sums, [2C, 4C): their sums of squares
    const int b = blockIdx.x / nchunk, ch = blockIdx.x % nchunk;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int len = clamped_len(lens, b, T);
    const int t0 = ch * chunk, t1 = min(min(t0 + chunk, T), len);
    const float* __restrict__ sb = src + (size_t)b * C * T;
    const float* __restrict__ eb = est + (size_t)b * C * T;
    for (int q = C * LDW + tid; q < MAXC * LDW; q += NT) {        // rows >= C stay zeros; the others are written whole every tile
        (&ts[0][0])[q] = 0.f;
        (&te[0][0])[q] = 0.f;
    }
    double4_t x = {0.0, 0.0, 0.0, 0.0};
    double rs[RPW], rq[RPW];
#pragma unroll
    for (int k = 0; k < RPW; ++k) rs[k] = rq[k] = 0.0;
    const int row = lane & 15, kk = lane >> 4;
    Quad qv[RPW];
    if (t0 < t1) load_tile<VEC>(sb, eb, C, T, t0, t1, qv);
    for (int tt = t0; tt < t1; tt += TK) {
        __syncthreads();                                          // the zeros above; the previous tile has been read
#pragma unroll
        for (int k = 0; k < RPW; ++k) {
            const int r = w + (NT / 64) * k;
            if (r < 2 * C) {
                float* dst = (r < C ? &ts[r][0] : &te[r - C][0]) + 4 * lane;
                *reinterpret_cast<float4*>(dst) = make_float4(qv[k].v[0], qv[k].v[1], qv[k].v[2], qv[k].v[3]);
                const double v0 = qv[k].v[0], v1 = qv[k].v[1], v2 = qv[k].v[2], v3 = qv[k].v[3];
                rs[k] += ((v0 + v1) + v2) + v3;
                rq[k] = fma(v3, v3, fma(v2, v2, fma(v1, v1, fma(v0, v0, rq[k]))));       // exact products: fused or not, the same bits
            }
        }
        __syncthreads();
        if (tt + TK < t1) load_tile<VEC>(sb, eb, C, T, tt + TK, t1, qv);      // the next tile's loads fly under the MFMAs
        const int nks = min(TK / 4, (t1 - tt + 3) / 4);        // the k-steps beyond hold zeros only
        for (int ks = w; ks < nks; ks += NT / 64) {
            // A: lane holds A[l & 15][l >> 4], B: B[l >> 4][l & 15], D: column l & 15, rows (l >> 4) + 4 r  (as in ctn_stoi.hip)
            const double sv = (double)ts[row][4 * ks + kk], ev = (double)te[row][4 * ks + kk];
            x = __builtin_amdgcn_mfma_f64_16x16x4f64(ev, sv, x, 0, 0, 0);        // x[i][j] = sum e_i s_j
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = kk + 4 * r, j = row;
        if (i < C && j < C) red[w][i * C + j] = x[r];
    }
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int r = w + (NT / 64) * k;                          // wave-uniform
        if (r < 2 * C) {
            const double s = wave_sum(rs[k]), q = wave_sum(rq[k]);
            if (lane == 0) { rowm[r] = s; rowm[2 * C + r] = q; }
        }
    }
    __syncthreads();
    double* __restrict__ out = partial + ((size_t)b * nchunk + ch) * nmom(C);
    for (int q = tid; q < nmom(C); q += NT) {
        double s;
        if (q < 4 * C) {
            s = rowm[q];                                          // rows 0 .. C - 1 are s, C .. 2C - 1 are e: ctn_loss.hip's order
        } else {
            s = red[0][q - 4 * C];
#pragma unroll
            for (int k = 1; k < NT / 64; ++k) s += red[k][q - 4 * C];
        }
        out[q] = s;
    }
}

// sum_chunks_to_lds of the skeleton for more than 64 moments: lane takes the moments lane, lane + 64, ... (at most MROUND of
// them); the same two barriers, the same sum in chunk order.  The sums are latency, not bytes (ctn_loss.hip says the same of its
// own): the loads of CB chunks of every moment of the lane are issued together, then added in chunk order.
constexpr int MROUND = (nmom(MAXC) + 63) / 64, CB = 4;
__device__ __forceinline__ void sum_chunks_to_lds_wide(const double* __restrict__ partial, int b, int B, int nv, int nchunk,
                                                       double* mo_w) {
    const int lane = threadIdx.x & 63;
    __syncthreads();
    if (b < B) {
        const double* __restrict__ p = partial + (size_t)b * nchunk * nv;
        double s[MROUND];
#pragma unroll
        for (int r = 0; r < MROUND; ++r) s[r] = 0.0;
        for (int c0 = 0; c0 < nchunk; c0 += CB) {
            double v[MROUND][CB];
#pragma unroll
            for (int r = 0; r < MROUND; ++r)
#pragma unroll
                for (int j = 0; j < CB; ++j) {
                    const int q = lane + 64 * r;
                    v[r][j] = q < nv && c0 + j < nchunk ? p[(size_t)(c0 + j) * nv + q] : 0.0;
                }
#pragma unroll
            for (int r = 0; r < MROUND; ++r)
#pragma unroll
                for (int j = 0; j < CB; ++j)
                    if (c0 + j < nchunk) s[r] += v[r][j];
        }
#pragma unroll
        for (int r = 0; r < MROUND; ++r)
            if (lane + 64 * r < nv) mo_w[lane + 64 * r] = s[r];
    }
    __syncthreads();
}

// snr[i][j] and its derivatives from the raw moments `mo` of an utterance of n samples: sisnr_pit_kernel's algebra (ctn_loss.hip).
struct PairTerms { double snr, dA, dB, me, ms; };
__device__ __forceinline__ PairTerms pair_terms(const double* mo, int C, double n, int i, int j) {
    PairTerms r;
    r.ms = mo[j] / n;
    r.me = mo[C + i] / n;
    const double En = fmax(mo[2 * C + j] - n * r.ms * r.ms, 0.0);
    const double Ee = fmax(mo[3 * C + i] - n * r.me * r.me, 0.0);
    const double dot = mo[4 * C + i * C + j] - n * r.me * r.ms;
    const double Enp = En + EPSD;
    const double P = dot * dot * En / (Enp * Enp);
    const double Nz = fmax(Ee - 2.0 * dot * dot / Enp + P, 0.0);
    const double ratio = P / (Nz + EPSD);
    r.snr = 10.0 * log10(ratio + EPSD);
    const double dsnr = (10.0 / log(10.0)) / (ratio + EPSD);
    const double dP = 2.0 * dot * En / (Enp * Enp);
    const double dNz = -4.0 * dot / Enp + dP;
    r.dA = dsnr * (dP / (Nz + EPSD) - P / ((Nz + EPSD) * (Nz + EPSD)) * dNz);
    r.dB = 2.0 * dsnr * (-P / ((Nz + EPSD) * (Nz + EPSD)));
    return r;
}

// First minimum over lanes 0 .. 15 (the columns): smaller L wins, equal L -> smaller idx; a lane without a candidate carries
// idx = MAXC.  Every lane returns lane 0's result, so the wave agrees on one winner whatever the values are (NaN included), and
// the winner is a candidate whenever there is one: a lane without one takes any candidate it meets.
__device__ __forceinline__ void first_min16(double& L, int& idx) {
    double bestL = L;
    int best = idx;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        const double oL = __shfl_xor(bestL, o, 64);
        const int oi = __shfl_xor(best, o, 64);
        const bool take = oi < MAXC && (best == MAXC || oL < bestL || (oL == bestL && oi < best));
        if (take) { bestL = oL; best = oi; }
    }
    L = __shfl(bestL, 0, 64);
    idx = __shfl(best, 0, 64);
}

// The assignment of one C x C matrix by one wave: perm of row `lane` (lanes < C) maximising (maximize != 0) or minimising
// sum_i m[i * C + perm[i]].  Shortest augmenting paths with row potentials u (lane = row) and column potentials v (lane = column):
// rows enter in index order; a row's search grows a tree from the row over reduced costs (c[i][j] - u[i]) - v[j], each step
// taking the FIRST column of least slack, until it meets a free column; then the path is flipped back to the row.
// The arithmetic is fp64 additions, subtractions and comparisons of the widened fp32 entries only (the negation for `maximize` is
// exact), so tests/assign_oracle.py's solve() follows it bit for bit, ties included.
// EVERY LOOP HAS A TRIP COUNT FIXED BY C.  A search step picks an unused column whatever the data is (first_min16 returns a
// candidate whenever one exists), a picked column is marked used, and the search ends at the first free column; the columns in
// use are matched ones, fewer than C, so at most C steps run.  way[j] is the column the search stood on when j's slack was
// last lowered (-1: the row itself), which was marked used earlier than j, so the walk back strictly descends in that order and
// takes at most C steps.  With NaN or infinite entries the comparisons may choose differently, but these counts and the
// bijection do not depend on any value: some valid permutation comes out.
// m: global or LDS.  Wave-uniform control flow; no barrier.  Returns perm[lane] for lane < C (undefined elsewhere).
__device__ __forceinline__ int assign_solve(const float* m, int C, bool maximize) {
    const int lane = threadIdx.x & 63;
    const double INF = __builtin_huge_val();
    double u = 0.0, v = 0.0;                 // u: potential of row `lane`; v: of column `lane`
    int p = -1;                              // the row matched to column `lane`
    for (int i = 0; i < C; ++i) {
        double minv = INF;
        int way = -1;
        bool used = false;                   // column `lane` is in the tree
        bool intree = lane == i;             // row `lane` is in the tree
        int j0 = -1, i0 = i;                 // the column the search stands on (-1: none yet) and its row
        bool done = false;
        for (int step = 0; step < C; ++step) {
            if (done) continue;
            if (lane == j0) used = true;
            const double ui0 = __shfl(u, i0, 64);
            const bool cand = lane < C && !used;
            if (cand) {
                const double c = (double)m[i0 * C + lane];
                const double cur = ((maximize ? -c : c) - ui0) - v;
                if (cur < minv) { minv = cur; way = j0; }
            }
            double delta = minv;
            int j1 = cand ? lane : MAXC;
            first_min16(delta, j1);
            if (intree) u += delta;
            if (used) v -= delta;
            else minv -= delta;
            j0 = j1 < C ? j1 : 0;            // (a candidate exists while fewer than C columns are used: always)
            i0 = __shfl(p, j0, 64);
            done = i0 < 0;
            if (!done && lane == i0) intree = true;
            if (done) i0 = 0;
        }
        for (int step = 0; step < C; ++step) {   // flip the path: column j0 takes the row of the column before it, back to row i
            if (j0 < 0) continue;
            const int j1 = __shfl(way, j0, 64);
            const int pj1 = __shfl(p, j1 < 0 ? 0 : j1, 64);
            if (lane == j0) p = j1 < 0 ? i : pj1;
            j0 = j1;
        }
    }
    // invert: perm[row] = column.  p is a bijection of the columns < C onto the rows < C.
    int perm = 0;
    for (int j = 0; j < C; ++j) {
        const int pj = __shfl(p, j, 64);
        if (pj == lane) perm = j;
    }
    return perm;
}

// One block of 16 waves; wave w takes utterances w, w + 16, ...  pair [B,C,C], perm [B,C], coef [B,C,4] = {dA, dB, mean e_i, mean s_j}.
__global__ __launch_bounds__(NTA) void sisnr_assign_kernel(const double* __restrict__ partial, const long long* __restrict__ lens,
                                                           int B, int C, int T, int nchunk, float* __restrict__ max_snr,
                                                           int* __restrict__ perm, float* __restrict__ loss,
                                                           float* __restrict__ pair, float* __restrict__ coef) {
    constexpr int NW = NTA / 64;
    __shared__ double mo[NW][nmom(MAXC)];
    __shared__ float cost[NW][MAXC * MAXC];   // pair[b] as stored: what the solver sees
    __shared__ double wsum[NW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nv = nmom(C), cc = C * C;
    double local = 0.0;                       // lane 0: sum of this wave's max_snr in fp64, ascending b
    for (int b0 = 0; b0 < B; b0 += NW) {      // block-uniform trip count: the barriers below are reached by every wave
        const int b = b0 + w;
        sum_chunks_to_lds_wide(partial, b, B, nv, nchunk, mo[w]);      // its first barrier also guards cost[w]
        if (b >= B) continue;                 // (after the last barrier of the iteration)
        const double n = (double)clamped_len(lens, b, T);
        for (int q = lane; q < cc; q += 64) {
            const float f = (float)pair_terms(mo[w], C, n, q / C, q % C).snr;
            cost[w][q] = f;
            pair[(size_t)b * cc + q] = f;
        }
        // cost[w] is written and read by this wave alone: the LDS operations of a wave complete in order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int j = assign_solve(cost[w], C, true);
        double mine = 0.0;
        if (lane < C) {
            const PairTerms t = pair_terms(mo[w], C, n, lane, j);
            float* cf = coef + ((size_t)b * C + lane) * 4;
            cf[0] = (float)t.dA;
            cf[1] = (float)t.dB;
            cf[2] = (float)t.me;
            cf[3] = (float)t.ms;
            perm[(size_t)b * C + lane] = j;
            mine = t.snr;
        }
        double tot = 0.0;                     // fp64 sum of the matched snr in ascending i, on every lane
        for (int i = 0; i < C; ++i) tot += __shfl(mine, i, 64);
        const double mx = tot / (double)C;
        if (lane == 0) {
            max_snr[b] = (float)mx;
            local += mx;
        }
    }
    // mean_over_waves writes the mean; the loss is its negative (an exact sign flip of the fp32 value)
    mean_over_waves(local, wsum, B, loss);
    if (threadIdx.x == 0) loss[0] = -loss[0];
}

// One wave per matrix: score [N,C,C] -> perm [N,C].
__global__ __launch_bounds__(NT) void assign_solve_kernel(const float* __restrict__ score, int N, int C, int maximize,
                                                          int* __restrict__ perm) {
    const int lane = threadIdx.x & 63;
    const long long n = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (n >= N) return;                       // wave-uniform; no barrier in this kernel
    const int j = assign_solve(score + (size_t)n * C * C, C, maximize != 0);
    if (lane < C) perm[(size_t)n * C + lane] = j;
}

// Each lane takes four consecutive samples of one utterance: reads the C estimate rows and their matched reference rows, writes
// the C rows of d_e.  One rounding per operation.
template <bool VEC>
__global__ __launch_bounds__(NT) void sisnr_assign_bwd_kernel(const float* __restrict__ s, const float* __restrict__ e,
                                                              const long long* __restrict__ lens, const int* __restrict__ perm,
                                                              const float* __restrict__ coef, const float* __restrict__ g_loss,
                                                              const float* __restrict__ g_max, int B, int C, int T, int ntile,
                                                              float* __restrict__ de) {
#pragma clang fp contract(off)
    const int b = blockIdx.x / ntile, tile = blockIdx.x % ntile;
    const int t = (tile * NT + threadIdx.x) * 4;
    if (t >= T) return;
    const int len = clamped_len(lens, b, T);
    // d objective / d max_snr[b]: loss = -mean max_snr
    const float scale = (upstream_scale(nullptr, g_max, b, B) - upstream_scale(g_loss, nullptr, b, B)) / (float)C;
    const float* __restrict__ sb = s + (size_t)b * C * T;
    const float* __restrict__ eb = e + (size_t)b * C * T;
    float* __restrict__ db = de + (size_t)b * C * T;
    for (int i = 0; i < C; ++i) {
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if (t < len) {
            const int j = min(max(perm[(size_t)b * C + i], 0), C - 1);
            const float* cf = coef + ((size_t)b * C + i) * 4;
            const float cA = cf[0], cB = cf[1], me = cf[2], ms = cf[3];
            const Quad ev = load4<VEC>(eb + (size_t)i * T, t, len);
            const Quad sv = load4<VEC>(sb + (size_t)j * T, t, len);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float a = cA * (sv.v[k] - ms), c = cB * (ev.v[k] - me);
                o[k] = t + k < len ? scale * (a + c) : 0.f;
            }
        }
        store4<VEC>(db + (size_t)i * T + t, o, t, T);
    }
}

}  // namespace

extern "C" {

size_t ctn_sisnr_assign_workspace(int B, int C, int T) {
    if (B <= 0 || C < MINC || C > MAXC || T <= 0) return 0;
    return (size_t)B * ctn_sisnr_chunks(T) * nmom(C) * sizeof(double);
}

// see include/ctn_hip.h
int ctn_sisnr_assign_fwd(const float* source, const float* estimate, const long long* lengths, int B, int C, int T, float* max_snr,
                         int* perm, float* loss, float* pair, float* coef, void* workspace, size_t workspace_bytes, void* stream) {
    CTN_REQUIRE(source && estimate && lengths && max_snr && perm && loss && pair && coef, "ctn_sisnr_assign_fwd: null pointer");
    CTN_REQUIRE(C >= MINC && C <= MAXC, "ctn_sisnr_assign_fwd: C = %d outside %d .. %d", C, MINC, MAXC);
    CTN_REQUIRE(B > 0 && T > 0, "ctn_sisnr_assign_fwd: bad sizes (B = %d, T = %d)", B, T);
    const int nchunk = ctn_sisnr_chunks(T);
    if (const int rc = grid_guard("ctn_sisnr_assign_fwd", "chunks", B, nchunk, T)) return rc;
    if (const int rc = workspace_guard("ctn_sisnr_assign_fwd", workspace, workspace_bytes, ctn_sisnr_assign_workspace(B, C, T)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (T % 4 == 0) && ctn_aligned16(source) && ctn_aligned16(estimate);
    auto kernel = vec ? &assign_moments_kernel<true> : &assign_moments_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(B * nchunk)), dim3(NT), 0, st, source, estimate, lengths, C, T, moment_chunk(T, nchunk),
                       nchunk, (double*)workspace);
    CTN_CHECK_LAUNCH("ctn_sisnr_assign_fwd/moments");
    hipLaunchKernelGGL(sisnr_assign_kernel, dim3(1), dim3(NTA), 0, st, (const double*)workspace, lengths, B, C, T, nchunk, max_snr,
                       perm, loss, pair, coef);
    CTN_CHECK_LAUNCH("ctn_sisnr_assign_fwd/assign");
    return CTN_OK;
}

int ctn_sisnr_assign_bwd(const float* source, const float* estimate, const long long* lengths, const int* perm, const float* coef,
                         const float* g_loss, const float* g_max, int B, int C, int T, float* d_estimate, void* stream) {
    CTN_REQUIRE(source && estimate && lengths && perm && coef && d_estimate, "ctn_sisnr_assign_bwd: null pointer");
    CTN_REQUIRE(C >= MINC && C <= MAXC, "ctn_sisnr_assign_bwd: C = %d outside %d .. %d", C, MINC, MAXC);
    CTN_REQUIRE(B > 0 && T > 0, "ctn_sisnr_assign_bwd: bad sizes (B = %d, T = %d)", B, T);
    const int ntile = bwd_tiles(T);
    if (const int rc = grid_guard("ctn_sisnr_assign_bwd", "tiles", B, ntile, T)) return rc;
    const bool vec = (T % 4 == 0) && ctn_aligned16(source) && ctn_aligned16(estimate) && ctn_aligned16(d_estimate);
    auto kernel = vec ? &sisnr_assign_bwd_kernel<true> : &sisnr_assign_bwd_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(B * ntile)), dim3(NT), 0, (hipStream_t)stream, source, estimate, lengths, perm, coef,
                       g_loss, g_max, B, C, T, ntile, d_estimate);
    CTN_CHECK_LAUNCH("ctn_sisnr_assign_bwd");
    return CTN_OK;
}

int ctn_assign_solve(const float* score, int N, int C, int maximize, int* perm, void* stream) {
    CTN_REQUIRE(score && perm, "ctn_assign_solve: null pointer");
    CTN_REQUIRE(C >= 1 && C <= MAXC, "ctn_assign_solve: C = %d outside 1 .. %d", C, MAXC);
    CTN_REQUIRE(N > 0, "ctn_assign_solve: bad sizes (N = %d)", N);
    hipLaunchKernelGGL(assign_solve_kernel, dim3((unsigned)ctn_cdiv(N, NT / 64)), dim3(NT), 0, (hipStream_t)stream, score, N, C,
                       maximize, perm);
    CTN_CHECK_LAUNCH("ctn_assign_solve");
    return CTN_OK;
}

}  // extern "C"
