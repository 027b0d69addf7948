// BSS Eval v3 (SDR / SIR / SAR) in fp64, gfx950: mir_eval.separation.bss_eval_sources as called by cal_SDRi,
// src/evaluate.py:76-91, and by evaluate's calc_sdr branch, :62-72.
//
// One utterance b has C references s_i and E estimate rows e (the mixture anchor of cal_SDRi can be one of them), all of
// length n_b <= T; samples at t >= n_b count as zero.  F = 512 is the distortion-filter length of bss_eval_sources.
//   corr     r_ik(tau) = sum_t s_i[t] s_k[t+tau],  D[e,i,a] = sum_t s_i[t] e[t+a],  ||e||^2     (tau, a in [0,F))
//            per-time-chunk partials (chunk = 2048 samples of the utterance, so the partition depends on n_b only),
//            summed in chunk order by corr_reduce
//   gram     G (C*F square, block (i,k) Toeplitz: G[iF+a, kF+b] = r_ik(a-b)) and G_jj for j >= 1; G_00 is the leading
//            block of G and its Cholesky factor the leading block of chol(G)
//   chol     right-looking blocked Cholesky, 64-wide panels: per step one panel launch (every workgroup factors the
//            64x64 diagonal tile and solves its own tile below it) and one trailing-update launch over every 64x64 tile
//            of the trailing lower triangle; all matrices of all utterances in the same launches
//   solve    forward + back substitution, one workgroup per (utterance, matrix): E right-hand sides D[e] on G -> coef_all,
//            D[e, j] on G_jj -> coef_own[e, j]
//   project  P_all e = sum_i coef_all_i * s_i, P_j e = coef_own_j * s_j over u in [0, n_b+F-1) (chunks of 1024 samples),
//            the five residual energies accumulated explicitly (never as ||e||^2 - c.D, which cancels SAR/10 digits)
//   finish   energies summed in chunk order -> dB.  sdr = ||P_j e||^2 / ||e - P_j e||^2, sir = ||P_j e||^2 / ||P_all e -
//            P_j e||^2, sar = ||P_all e||^2 / ||e - P_all e||^2; a zero denominator gives +inf, as mir_eval's _safe_db.
// Every reduction has a fixed order, so the same utterance gives bitwise the same numbers in any batch.
#include "ctn_common.h"
#include <float.h>

namespace {

constexpr int F = 512;        // distortion-filter length, fixed in bss_eval_sources
constexpr int NB = 64;        // Cholesky panel width = tile edge
constexpr int MAXC = 4;
constexpr int TC = 2048;      // correlation time chunk
constexpr int TU = 1024;      // projection time chunk
constexpr int NT = 256;
constexpr int NR = 3;         // right-hand sides per solve pass

__host__ __device__ __forceinline__ long long cdiv64(long long a, long long b) { return (a + b - 1) / b; }

__device__ __forceinline__ long long clamp_len(const long long* lens, long long b, long long T) {
    long long n = lens[b];
    return n < 0 ? 0 : (n > T ? T : n);
}

// matrix mi of utterance b: 0 = G (dim C*F), j >= 1 = G_jj (dim F)
__device__ __forceinline__ double* mat_ptr(double* fac, long long b, int mi, long long B, int C) {
    const size_t big = (size_t)C * F * C * F;
    if (mi == 0) return fac + (size_t)b * big;
    return fac + (size_t)B * big + ((size_t)b * (C - 1) + (mi - 1)) * F * F;
}

// ---- correlations: grid (chunk, signal x in [0, C+E), b) -----------------------------------------------------------
// part[b][ch][x][i][tau] = sum_{t in chunk} s_i[t] x[t+tau];  epart[b][ch][e] = sum_{t in chunk} e[t]^2
__global__ __launch_bounds__(NT) void bss_corr_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                      const long long* __restrict__ lens, int C, int E, long long T, int nch,
                                                      double* __restrict__ part, double* __restrict__ epart) {
    __shared__ float srow[MAXC][TC];
    __shared__ float slag[TC + F];
    __shared__ double red[NT / 64];
    const int ch = blockIdx.x, x = blockIdx.y, tid = threadIdx.x;
    const long long b = blockIdx.z;
    const long long n = clamp_len(lens, b, T);
    const long long t0 = (long long)ch * TC;
    if (t0 >= n) return;                                    // past this utterance: never read by corr_reduce
    const float* __restrict__ xs = x < C ? ref + ((size_t)b * C + x) * T : est + ((size_t)b * E + (x - C)) * T;
    for (int i = 0; i < C; ++i)
        for (int u = tid; u < TC; u += NT) srow[i][u] = t0 + u < n ? ref[((size_t)b * C + i) * T + t0 + u] : 0.f;
    for (int u = tid; u < TC + F; u += NT) slag[u] = t0 + u < n ? xs[t0 + u] : 0.f;
    __syncthreads();
    double a0[MAXC], a1[MAXC];
#pragma unroll
    for (int i = 0; i < MAXC; ++i) a0[i] = a1[i] = 0.0;
#pragma unroll 4
    for (int u = 0; u < TC; ++u) {
        const double x0 = (double)slag[u + tid], x1 = (double)slag[u + tid + NT];
#pragma unroll
        for (int i = 0; i < MAXC; ++i)
            if (i < C) {
                const double si = (double)srow[i][u];
                a0[i] = fma(si, x0, a0[i]);
                a1[i] = fma(si, x1, a1[i]);
            }
    }
    double* __restrict__ out = part + (((size_t)b * nch + ch) * (C + E) + x) * C * F;
#pragma unroll
    for (int i = 0; i < MAXC; ++i)
        if (i < C) { out[(size_t)i * F + tid] = a0[i]; out[(size_t)i * F + tid + NT] = a1[i]; }
    if (x >= C) {
        double q = 0.0;
        for (int u = tid; u < TC; u += NT) { const double v = (double)slag[u]; q = fma(v, v, q); }
        q = block_sum<double, NT>(q, red);
        if (tid == 0) epart[((size_t)b * nch + ch) * E + (x - C)] = q;
    }
}

// grid (cdiv(per, NT), b): sum the chunk partials of one utterance in chunk order.  r [B,C,C,F], d [B,E,C,F], enorm [B,E]
__global__ __launch_bounds__(NT) void bss_corr_reduce_kernel(const double* __restrict__ part, const double* __restrict__ epart,
                                                             const long long* __restrict__ lens, int C, int E, long long T,
                                                             int nch, double* __restrict__ r, double* __restrict__ d,
                                                             double* __restrict__ enorm) {
    const long long b = blockIdx.y;
    const long long per = (long long)(C + E) * C * F;
    const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
    const long long n = clamp_len(lens, b, T);
    const int nc = (int)cdiv64(n, TC);
    if (idx < per) {
        double s = 0.0;
        for (int ch = 0; ch < nc; ++ch) s += part[((size_t)b * nch + ch) * per + idx];
        const int tau = (int)(idx % F), i = (int)((idx / F) % C), x = (int)(idx / ((long long)C * F));
        if (x < C) r[(((size_t)b * C + i) * C + x) * F + tau] = s;
        else d[(((size_t)b * E + (x - C)) * C + i) * F + tau] = s;
    } else if (idx < per + E) {
        const int e = (int)(idx - per);
        double s = 0.0;
        for (int ch = 0; ch < nc; ++ch) s += epart[((size_t)b * nch + ch) * E + e];
        enorm[(size_t)b * E + e] = s;
    }
}

// ---- Gram matrices: grid (blocks, mi in [0,C), b); full square (both triangles) -------------------------------------
__global__ __launch_bounds__(NT) void bss_gram_kernel(const double* __restrict__ r, long long B, int C,
                                                      double* __restrict__ fac, int* __restrict__ status) {
    const int mi = blockIdx.y;
    const long long b = blockIdx.z;
    const int dim = mi == 0 ? C * F : F;
    double* __restrict__ A = mat_ptr(fac, b, mi, B, C);
    const double* __restrict__ rb = r + (size_t)b * C * C * F;
    const long long tot = (long long)dim * dim;
    for (long long idx = (long long)blockIdx.x * NT + threadIdx.x; idx < tot; idx += (long long)gridDim.x * NT) {
        const int p = (int)(idx / dim), q = (int)(idx % dim);
        const int i = mi == 0 ? p / F : mi, k = mi == 0 ? q / F : mi, a = p % F, c = q % F;
        A[idx] = a >= c ? rb[((size_t)i * C + k) * F + (a - c)] : rb[((size_t)k * C + i) * F + (c - a)];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) status[b * C + mi] = 0;
}

__device__ __forceinline__ double pivot_threshold(const double* __restrict__ r, long long b, int mi, int C, int dim) {
    const double* rb = r + (size_t)b * C * C * F;
    double mx = 0.0;
    if (mi == 0) {
        for (int i = 0; i < C; ++i) mx = fmax(mx, rb[((size_t)i * C + i) * F]);
    } else {
        mx = rb[((size_t)mi * C + mi) * F];
    }
    return (double)dim * DBL_EPSILON * mx;
}

// Unblocked right-looking Cholesky of the diagonal tile Dt (transposed in LDS: Dt[q][r] = A[s*64+r][s*64+q]) and, with
// `panel`, the solve L_is L_ss^T = A_is of the tile Pt below it.  The same operations in every workgroup that calls it:
// bitwise the same L_ss.  Returns the first pivot that is not finite or not above `thresh` (-1: none).
__device__ int chol_tile(double (*Dt)[NB], double (*Pt)[NB], bool panel, double thresh) {
    const int tid = threadIdx.x, rr = tid & 63, g = tid >> 6;
    int bad = -1;
    for (int c = 0; c < NB; ++c) {
        __syncthreads();
        const double piv = Dt[c][c];
        const bool ok = piv > thresh && piv <= DBL_MAX;
        if (!ok && bad < 0) bad = c;
        const double dg = ok ? sqrt(piv) : 1.0;
        const double inv = 1.0 / dg;
        __syncthreads();
        if (g == 0) {
            if (rr > c) Dt[c][rr] *= inv;
            else if (rr == c) Dt[c][c] = dg;
        } else if (g == 1 && panel) {
            Pt[c][rr] *= inv;
        }
        __syncthreads();
        for (int q = c + 1 + g; q < NB; q += 4) {
            const double lq = Dt[c][q];
            if (rr >= q) Dt[q][rr] = fma(-Dt[c][rr], lq, Dt[q][rr]);
            if (panel) Pt[q][rr] = fma(-Pt[c][rr], lq, Pt[q][rr]);
        }
    }
    __syncthreads();
    return bad;
}

__device__ void load_tile_t(double (*Dt)[NB], const double* __restrict__ A, size_t off, int dim) {
    for (int idx = threadIdx.x; idx < NB * NB; idx += NT) {
        const int rr = idx / NB, q = idx % NB;
        Dt[q][rr] = A[off + (size_t)rr * dim + q];
    }
}

__device__ void store_lower_t(double* __restrict__ A, const double (*Dt)[NB], size_t off, int dim) {
    for (int idx = threadIdx.x; idx < NB * NB; idx += NT) {
        const int rr = idx / NB, q = idx % NB;
        if (rr >= q) A[off + (size_t)rr * dim + q] = Dt[q][rr];
    }
}

// ---- Cholesky panel at step s: grid (tile row i - s, mi, b) ------------------------------------------------------------
// Every workgroup factors the diagonal tile A_ss and, for i > s, writes L_is.  L_ss itself is written by the trailing-update
// launch of the same step (its extra workgroup), since the panel workgroups of this launch still read A_ss; only at a
// matrix's last step, where the panel launch has one workgroup for it, is it written here.
// status[b][mi] = 1 + the first pivot that is not finite or not above dim*eps*max diag (0: factorised).
__global__ __launch_bounds__(NT) void bss_chol_panel_kernel(const double* __restrict__ r, long long B, int C, int s,
                                                            double* __restrict__ fac, int* __restrict__ status) {
    __shared__ double Dt[NB][NB];
    __shared__ double Pt[NB][NB];
    const int mi = blockIdx.y, tid = threadIdx.x;
    const long long b = blockIdx.z;
    const int dim = mi == 0 ? C * F : F, nblk = dim / NB;
    const int i = s + blockIdx.x;
    if (i >= nblk) return;
    double* __restrict__ A = mat_ptr(fac, b, mi, B, C);
    const bool panel = i > s;
    const size_t d0 = (size_t)s * NB * dim + (size_t)s * NB, p0 = (size_t)i * NB * dim + (size_t)s * NB;
    load_tile_t(Dt, A, d0, dim);
    if (panel) load_tile_t(Pt, A, p0, dim);
    const int bad = chol_tile(Dt, Pt, panel, pivot_threshold(r, b, mi, C, dim));
    if (panel) {
        for (int idx = tid; idx < NB * NB; idx += NT) {
            const int r2 = idx / NB, q = idx % NB;
            A[p0 + (size_t)r2 * dim + q] = Pt[q][r2];
        }
    } else if (s == nblk - 1) {
        store_lower_t(A, Dt, d0, dim);
    }
    if (!panel && tid == 0 && bad >= 0 && status[b * C + mi] == 0) status[b * C + mi] = s * NB + bad + 1;
}

// ---- trailing update at step s: grid (tile of the trailing lower triangle, mi, b) -------------------------------------
// A_ij -= L_is L_js^T for s < j <= i, the 64-deep product summed in order p = 0..63
// The workgroup after the last tile of a matrix factors A_ss again (bitwise what the panel launch used) and writes L_ss.
__global__ __launch_bounds__(NT) void bss_chol_update_kernel(const double* __restrict__ r, long long B, int C, int s,
                                                             double* __restrict__ fac) {
    __shared__ double sm[NB][NB];
    double (*Li)[NB] = sm;              // rows 0..31: L_is, p-major, half of the 64-deep product at a time
    double (*Lj)[NB] = sm + NB / 2;     // rows 32..63: L_js
    const int mi = blockIdx.y, tid = threadIdx.x;
    const long long b = blockIdx.z;
    const int dim = mi == 0 ? C * F : F, nblk = dim / NB;
    const int m = nblk - s - 1;
    int idx = blockIdx.x;
    if (m <= 0 || idx > m * (m + 1) / 2) return;
    if (idx == m * (m + 1) / 2) {
        double (*Dt)[NB] = sm;
        double* __restrict__ A = mat_ptr(fac, b, mi, B, C);
        const size_t d0 = (size_t)s * NB * dim + (size_t)s * NB;
        load_tile_t(Dt, A, d0, dim);
        chol_tile(Dt, Dt, false, pivot_threshold(r, b, mi, C, dim));
        store_lower_t(A, Dt, d0, dim);
        return;
    }
    int ii = 0;
    while (idx > ii) { idx -= ii + 1; ++ii; }
    const int i = s + 1 + ii, j = s + 1 + idx;
    double* __restrict__ A = mat_ptr(fac, b, mi, B, C);
    const int tc = tid & 15, tr = tid >> 4;
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    for (int h = 0; h < 2; ++h) {
        __syncthreads();
        for (int e = tid; e < NB * NB / 2; e += NT) {
            const int row = e / (NB / 2), p = e % (NB / 2);
            Li[p][row] = A[((size_t)i * NB + row) * dim + (size_t)s * NB + h * (NB / 2) + p];
            Lj[p][row] = A[((size_t)j * NB + row) * dim + (size_t)s * NB + h * (NB / 2) + p];
        }
        __syncthreads();
#pragma unroll 4
        for (int p = 0; p < NB / 2; ++p) {
            double a[4], bb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { a[u] = Li[p][tr + 16 * u]; bb[u] = Lj[p][tc + 16 * u]; }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fma(a[u], bb[v], acc[u][v]);
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            double* p = A + ((size_t)i * NB + tr + 16 * u) * dim + (size_t)j * NB + tc + 16 * v;
            *p = *p - acc[u][v];
        }
}

// ---- solves: grid (problem, b), problem 0 = G (dim C*F), 1 + j = G_jj (dim F; j = 0 reads chol(G)'s leading block) ----
__global__ __launch_bounds__(NT) void bss_solve_kernel(const double* __restrict__ fac, const double* __restrict__ d, long long B,
                                                       int C, int E, double* __restrict__ coef_all, double* __restrict__ coef_own) {
    __shared__ double v[NR][MAXC * F];
    __shared__ double part[4][NR][NB];
    const int pi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long b = blockIdx.y;
    const int j = pi - 1;
    const int dim = pi == 0 ? C * F : F;
    const int lda = pi <= 1 ? C * F : F;
    const double* __restrict__ L = pi <= 1 ? mat_ptr(const_cast<double*>(fac), b, 0, B, C)
                                           : mat_ptr(const_cast<double*>(fac), b, j, B, C);
    const int nblk = dim / NB;
    const size_t rstride = (size_t)C * F;                  // D[b,e,:,:]: one row of C*F per estimate
    for (int e0 = 0; e0 < E; e0 += NR) {
        const int nr = min(NR, E - e0);
        __syncthreads();
        for (int k = 0; k < nr; ++k) {
            const double* __restrict__ rhs = d + ((size_t)b * E + e0 + k) * rstride + (pi == 0 ? 0 : (size_t)j * F);
            for (int p = tid; p < dim; p += NT) v[k][p] = rhs[p];
        }
        // forward: L y = rhs, block row by block row
        for (int kb = 0; kb < nblk; ++kb) {
            const int R0 = kb * NB;
            __syncthreads();
            for (int rr = w * 16; rr < w * 16 + 16; ++rr) {
                const double* __restrict__ Lr = L + (size_t)(R0 + rr) * lda;
                double acc[NR] = {0.0, 0.0, 0.0};
                for (int p = lane; p < R0; p += 64) {
                    const double l = Lr[p];
#pragma unroll
                    for (int k = 0; k < NR; ++k) acc[k] = fma(l, v[k][p], acc[k]);
                }
#pragma unroll
                for (int k = 0; k < NR; ++k) {
                    const double sum = wave_sum(acc[k]);
                    if (lane == 0) part[0][k][rr] = sum;
                }
            }
            __syncthreads();
            if (w == 0) {
                double lrow[NB];
                const double* __restrict__ Lr = L + (size_t)(R0 + lane) * lda + R0;
#pragma unroll
                for (int c = 0; c < NB; ++c) lrow[c] = c <= lane ? Lr[c] : 0.0;
                const double dinv = 1.0 / Lr[lane];
                double z[NR];
#pragma unroll
                for (int k = 0; k < NR; ++k) z[k] = v[k][R0 + lane] - part[0][k][lane];
#pragma unroll
                for (int c = 0; c < NB; ++c)
#pragma unroll
                    for (int k = 0; k < NR; ++k) {
                        const double yc = __shfl(z[k] * dinv, c, 64);
                        if (lane > c) z[k] = fma(-lrow[c], yc, z[k]);
                        else if (lane == c) z[k] = yc;
                    }
#pragma unroll
                for (int k = 0; k < NR; ++k) v[k][R0 + lane] = z[k];
            }
        }
        // backward: L^T c = y, from the last block row up; v holds c below the current block
        for (int kb = nblk - 1; kb >= 0; --kb) {
            const int R0 = kb * NB;
            __syncthreads();
            double acc[NR] = {0.0, 0.0, 0.0};
            for (int rr = R0 + NB + w; rr < dim; rr += 4) {
                const double l = L[(size_t)rr * lda + R0 + lane];
#pragma unroll
                for (int k = 0; k < NR; ++k) acc[k] = fma(l, v[k][rr], acc[k]);
            }
#pragma unroll
            for (int k = 0; k < NR; ++k) part[w][k][lane] = acc[k];
            __syncthreads();
            if (w == 0) {
                double lcol[NB];
#pragma unroll
                for (int q = 0; q < NB; ++q) lcol[q] = q >= lane ? L[(size_t)(R0 + q) * lda + R0 + lane] : 0.0;
                const double dinv = 1.0 / L[(size_t)(R0 + lane) * lda + R0 + lane];
                double z[NR];
#pragma unroll
                for (int k = 0; k < NR; ++k)
                    z[k] = v[k][R0 + lane] - (((part[0][k][lane] + part[1][k][lane]) + part[2][k][lane]) + part[3][k][lane]);
#pragma unroll
                for (int q = NB - 1; q >= 0; --q)
#pragma unroll
                    for (int k = 0; k < NR; ++k) {
                        const double cq = __shfl(z[k] * dinv, q, 64);
                        if (lane < q) z[k] = fma(-lcol[q], cq, z[k]);
                        else if (lane == q) z[k] = cq;
                    }
#pragma unroll
                for (int k = 0; k < NR; ++k) v[k][R0 + lane] = z[k];
            }
        }
        __syncthreads();
        for (int k = 0; k < nr; ++k) {
            double* __restrict__ out = pi == 0 ? coef_all + ((size_t)b * E + e0 + k) * C * F
                                               : coef_own + (((size_t)b * E + e0 + k) * C + j) * F;
            for (int p = tid; p < dim; p += NT) out[p] = v[k][p];
        }
    }
}

// ---- projections + energies: grid (chunk of u, e, b) ------------------------------------------------------------------
// epart[b][e][ch][k]: k = 3j + {0: ||P_j e||^2, 1: ||e - P_j e||^2, 2: ||P_all e - P_j e||^2}, 3C: ||P_all e||^2,
// 3C+1: ||e - P_all e||^2, over u in the chunk and u < n_b + F - 1
__global__ __launch_bounds__(NT) void bss_project_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                         const long long* __restrict__ lens, const double* __restrict__ coef_all,
                                                         const double* __restrict__ coef_own, int C, int E, long long T, int nch,
                                                         double* __restrict__ epart) {
    __shared__ double ca[MAXC][F];
    __shared__ double cj[MAXC][F];
    __shared__ float win[MAXC][TU + F];
    __shared__ double red[NT / 64];
    const int ch = blockIdx.x, e = blockIdx.y, tid = threadIdx.x;
    const long long b = blockIdx.z;
    const long long n = clamp_len(lens, b, T);
    const long long u0 = (long long)ch * TU, nu = n + F - 1;
    if (u0 >= nu) return;
    for (int i = 0; i < C; ++i) {
        for (int a = tid; a < F; a += NT) {
            ca[i][a] = coef_all[(((size_t)b * E + e) * C + i) * F + a];
            cj[i][a] = coef_own[(((size_t)b * E + e) * C + i) * F + a];
        }
        // win[i][w] = s_i[u0 - (F-1) + w]
        for (int w = tid; w < TU + F - 1; w += NT) {
            const long long t = u0 - (F - 1) + w;
            win[i][w] = t >= 0 && t < n ? ref[((size_t)b * C + i) * T + t] : 0.f;
        }
    }
    __syncthreads();
    double pall[4], pj[MAXC][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        pall[q] = 0.0;
#pragma unroll
        for (int i = 0; i < MAXC; ++i) pj[i][q] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < MAXC; ++i)
        if (i < C) {
            for (int a = 0; a < F; ++a) {
                const double wa = ca[i][a], wj = cj[i][a];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double sv = (double)win[i][tid + NT * q + (F - 1) - a];
                    pall[q] = fma(wa, sv, pall[q]);
                    pj[i][q] = fma(wj, sv, pj[i][q]);
                }
            }
        }
    double acc[3 * MAXC + 2];
#pragma unroll
    for (int k = 0; k < 3 * MAXC + 2; ++k) acc[k] = 0.0;
    const float* __restrict__ eb = est + ((size_t)b * E + e) * T;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long long u = u0 + tid + NT * q;
        if (u < nu) {
            const double ev = u < n ? (double)eb[u] : 0.0;
            const double pa = pall[q];
#pragma unroll
            for (int i = 0; i < MAXC; ++i)
                if (i < C) {
                    const double p = pj[i][q], r1 = ev - p, r2 = pa - p;
                    acc[3 * i] = fma(p, p, acc[3 * i]);
                    acc[3 * i + 1] = fma(r1, r1, acc[3 * i + 1]);
                    acc[3 * i + 2] = fma(r2, r2, acc[3 * i + 2]);
                }
            const double r3 = ev - pa;
            acc[3 * MAXC] = fma(pa, pa, acc[3 * MAXC]);
            acc[3 * MAXC + 1] = fma(r3, r3, acc[3 * MAXC + 1]);
        }
    }
    const int nk = 3 * C + 2;
    double* __restrict__ out = epart + (((size_t)b * E + e) * nch + ch) * nk;
#pragma unroll
    for (int k = 0; k < 3 * MAXC + 2; ++k) {
        const bool used = k < 3 * C || k >= 3 * MAXC;
        if (!used) continue;
        const double s = block_sum<double, NT>(acc[k], red);
        if (tid == 0) out[k < 3 * MAXC ? k : 3 * C + (k - 3 * MAXC)] = s;
    }
}

__device__ __forceinline__ double safe_db(double num, double den) { return den == 0.0 ? INFINITY : 10.0 * log10(num / den); }

// one thread per (b, e): energies summed in chunk order -> sdr / sir / sar [B,E,C]; energies [B,E,3C+2] (nullable)
__global__ __launch_bounds__(NT) void bss_finish_kernel(const double* __restrict__ epart, const long long* __restrict__ lens,
                                                        long long B, int C, int E, long long T, int nch, double* __restrict__ sdr,
                                                        double* __restrict__ sir, double* __restrict__ sar,
                                                        double* __restrict__ energies) {
    const long long be = (long long)blockIdx.x * NT + threadIdx.x;
    if (be >= B * E) return;
    const long long b = be / E;
    const long long n = clamp_len(lens, b, T);
    const int nc = (int)cdiv64(n + F - 1, TU), nk = 3 * C + 2;
    double en[3 * MAXC + 2];
    for (int k = 0; k < nk; ++k) {
        double s = 0.0;
        for (int ch = 0; ch < nc; ++ch) s += epart[((size_t)be * nch + ch) * nk + k];
        en[k] = s;
        if (energies != nullptr) energies[(size_t)be * nk + k] = s;
    }
    for (int j = 0; j < C; ++j) {
        sdr[(size_t)be * C + j] = safe_db(en[3 * j], en[3 * j + 1]);
        sir[(size_t)be * C + j] = safe_db(en[3 * j], en[3 * j + 2]);
        sar[(size_t)be * C + j] = safe_db(en[3 * C], en[3 * C + 1]);
    }
}

constexpr size_t ALIGN = 256;
size_t aligned(size_t bytes) { return (bytes + ALIGN - 1) / ALIGN * ALIGN; }

int corr_chunks(long long T) { return (int)ctn_cdivll(T, TC); }
int proj_chunks(long long T) { return (int)ctn_cdivll(T + F - 1, TU); }

size_t corr_ws(long long B, int C, long long E, long long T) {
    return aligned((size_t)B * corr_chunks(T) * (C + E) * C * F * sizeof(double)) +
           aligned((size_t)B * corr_chunks(T) * E * sizeof(double));
}
size_t proj_ws(long long B, int C, long long E, long long T) {
    return aligned((size_t)B * E * proj_chunks(T) * (3 * C + 2) * sizeof(double));
}
size_t factor_doubles(long long B, int C) { return (size_t)B * ((size_t)C * F * C * F + (size_t)(C - 1) * F * F); }

#define BSS_CHECK_SIZES(fn, B, C, E, T)                                                                              \
    CTN_REQUIRE((C) >= 2 && (C) <= MAXC, fn ": C = %d outside 2..%d", (int)(C), MAXC);                                 \
    CTN_REQUIRE((B) >= 1 && (B) <= 65535, fn ": B = %lld outside 1..65535", (long long)(B));                           \
    CTN_REQUIRE((E) >= 1 && (E) <= 4096, fn ": E = %lld outside 1..4096", (long long)(E));                             \
    CTN_REQUIRE((T) >= 1 && (T) <= (1LL << 40), fn ": T = %lld < 1", (long long)(T))

int launch_corr(const float* ref, const float* est, const long long* lengths, long long B, int C, long long E, long long T,
                double* r, double* d, double* enorm, void* ws, hipStream_t st) {
    const int nch = corr_chunks(T);
    double* part = (double*)ws;
    double* epart = (double*)((char*)ws + aligned((size_t)B * nch * (C + E) * C * F * sizeof(double)));
    hipLaunchKernelGGL(bss_corr_kernel, dim3(nch, (unsigned)(C + E), (unsigned)B), dim3(NT), 0, st, ref, est, lengths, C,
                       (int)E, T, nch, part, epart);
    CTN_CHECK_LAUNCH("ctn_bss_corr");
    const long long per = (C + E) * C * F + E;
    hipLaunchKernelGGL(bss_corr_reduce_kernel, dim3((unsigned)ctn_cdivll(per, NT), (unsigned)B), dim3(NT), 0, st, part, epart,
                       lengths, C, (int)E, T, nch, r, d, enorm);
    CTN_CHECK_LAUNCH("ctn_bss_corr/reduce");
    return CTN_OK;
}

int launch_factor(const double* r, long long B, int C, double* fac, int* status, hipStream_t st) {
    hipLaunchKernelGGL(bss_gram_kernel, dim3(256, (unsigned)C, (unsigned)B), dim3(NT), 0, st, r, B, C, fac, status);
    CTN_CHECK_LAUNCH("ctn_bss_factor/gram");
    const int nblk = C * F / NB;
    for (int s = 0; s < nblk; ++s) {
        hipLaunchKernelGGL(bss_chol_panel_kernel, dim3((unsigned)(nblk - s), (unsigned)C, (unsigned)B), dim3(NT), 0, st, r, B,
                           C, s, fac, status);
        CTN_CHECK_LAUNCH("ctn_bss_factor/panel");
        const int m = nblk - s - 1;
        if (m > 0) {
            hipLaunchKernelGGL(bss_chol_update_kernel, dim3((unsigned)(m * (m + 1) / 2 + 1), (unsigned)C, (unsigned)B), dim3(NT),
                               0, st, r, B, C, s, fac);
            CTN_CHECK_LAUNCH("ctn_bss_factor/update");
        }
    }
    return CTN_OK;
}

int launch_solve(const double* fac, const double* d, long long B, int C, long long E, double* coef_all, double* coef_own,
                 hipStream_t st) {
    hipLaunchKernelGGL(bss_solve_kernel, dim3((unsigned)(C + 1), (unsigned)B), dim3(NT), 0, st, fac, d, B, C, (int)E, coef_all,
                       coef_own);
    CTN_CHECK_LAUNCH("ctn_bss_solve");
    return CTN_OK;
}

int launch_project(const float* ref, const float* est, const long long* lengths, const double* coef_all, const double* coef_own,
                   long long B, int C, long long E, long long T, double* sdr, double* sir, double* sar, double* energies,
                   void* ws, hipStream_t st) {
    const int nch = proj_chunks(T);
    double* epart = (double*)ws;
    hipLaunchKernelGGL(bss_project_kernel, dim3(nch, (unsigned)E, (unsigned)B), dim3(NT), 0, st, ref, est, lengths, coef_all,
                       coef_own, C, (int)E, T, nch, epart);
    CTN_CHECK_LAUNCH("ctn_bss_project");
    hipLaunchKernelGGL(bss_finish_kernel, dim3((unsigned)ctn_cdivll(B * E, NT)), dim3(NT), 0, st, epart, lengths, B, C, (int)E, T,
                       nch, sdr, sir, sar, energies);
    CTN_CHECK_LAUNCH("ctn_bss_project/finish");
    return CTN_OK;
}

}  // namespace

extern "C" {

// see include/ctn_hip.h
size_t ctn_bss_corr_workspace(long long B, int C, long long E, long long T) {
    if (B < 1 || C < 2 || C > MAXC || E < 1 || T < 1) return 0;
    return corr_ws(B, C, E, T);
}

size_t ctn_bss_factor_doubles(long long B, int C) {
    if (B < 1 || C < 2 || C > MAXC) return 0;
    return factor_doubles(B, C);
}

size_t ctn_bss_project_workspace(long long B, int C, long long E, long long T) {
    if (B < 1 || C < 2 || C > MAXC || E < 1 || T < 1) return 0;
    return proj_ws(B, C, E, T);
}

size_t ctn_bss_workspace(long long B, int C, long long E, long long T) {
    if (B < 1 || C < 2 || C > MAXC || E < 1 || T < 1) return 0;
    const size_t cf = (size_t)C * F;
    size_t s = aligned((size_t)B * C * cf * sizeof(double));                 // r
    s += aligned((size_t)B * E * cf * sizeof(double));                       // d
    s += aligned((size_t)B * E * sizeof(double));                            // enorm
    s += 2 * aligned((size_t)B * E * cf * sizeof(double));                   // coef_all, coef_own
    s += aligned(factor_doubles(B, C) * sizeof(double));                     // factors
    const size_t c = corr_ws(B, C, E, T), p = proj_ws(B, C, E, T);
    return s + (c > p ? c : p);                                              // chunk partials (corr, then projection)
}

int ctn_bss_corr(const float* ref, const float* est, const long long* lengths, long long B, int C, long long E, long long T,
                 double* r, double* d, double* enorm, void* workspace, size_t workspace_bytes, void* stream) {
    CTN_REQUIRE(ref && est && lengths && r && d && enorm, "ctn_bss_corr: null pointer");
    BSS_CHECK_SIZES("ctn_bss_corr", B, C, E, T);
    if (workspace == nullptr || workspace_bytes < corr_ws(B, C, E, T)) {
        ctn_set_error("ctn_bss_corr: workspace too small");
        return CTN_ERR_WORKSPACE;
    }
    return launch_corr(ref, est, lengths, B, C, E, T, r, d, enorm, workspace, (hipStream_t)stream);
}

int ctn_bss_factor(const double* r, long long B, int C, double* factors, int* status, void* stream) {
    CTN_REQUIRE(r && factors && status, "ctn_bss_factor: null pointer");
    BSS_CHECK_SIZES("ctn_bss_factor", B, C, 1, 1);
    return launch_factor(r, B, C, factors, status, (hipStream_t)stream);
}

int ctn_bss_solve(const double* factors, const double* d, long long B, int C, long long E, double* coef_all, double* coef_own,
                  void* stream) {
    CTN_REQUIRE(factors && d && coef_all && coef_own, "ctn_bss_solve: null pointer");
    BSS_CHECK_SIZES("ctn_bss_solve", B, C, E, 1);
    return launch_solve(factors, d, B, C, E, coef_all, coef_own, (hipStream_t)stream);
}

int ctn_bss_project(const float* ref, const float* est, const long long* lengths, const double* coef_all, const double* coef_own,
                    long long B, int C, long long E, long long T, double* sdr, double* sir, double* sar, double* energies,
                    void* workspace, size_t workspace_bytes, void* stream) {
    CTN_REQUIRE(ref && est && lengths && coef_all && coef_own && sdr && sir && sar, "ctn_bss_project: null pointer");
    BSS_CHECK_SIZES("ctn_bss_project", B, C, E, T);
    if (workspace == nullptr || workspace_bytes < proj_ws(B, C, E, T)) {
        ctn_set_error("ctn_bss_project: workspace too small");
        return CTN_ERR_WORKSPACE;
    }
    return launch_project(ref, est, lengths, coef_all, coef_own, B, C, E, T, sdr, sir, sar, energies, workspace,
                          (hipStream_t)stream);
}

int ctn_bss_eval(const float* ref, const float* est, const long long* lengths, long long B, int C, long long E, long long T,
                 double* sdr, double* sir, double* sar, int* status, void* workspace, size_t workspace_bytes, void* stream) {
    CTN_REQUIRE(ref && est && lengths && sdr && sir && sar && status, "ctn_bss_eval: null pointer");
    BSS_CHECK_SIZES("ctn_bss_eval", B, C, E, T);
    if (workspace == nullptr || workspace_bytes < ctn_bss_workspace(B, C, E, T)) {
        ctn_set_error("ctn_bss_eval: workspace too small");
        return CTN_ERR_WORKSPACE;
    }
    const size_t cf = (size_t)C * F;
    char* w = (char*)workspace;
    double* r = (double*)w;          w += aligned((size_t)B * C * cf * sizeof(double));
    double* d = (double*)w;          w += aligned((size_t)B * E * cf * sizeof(double));
    double* enorm = (double*)w;      w += aligned((size_t)B * E * sizeof(double));
    double* coef_all = (double*)w;   w += aligned((size_t)B * E * cf * sizeof(double));
    double* coef_own = (double*)w;   w += aligned((size_t)B * E * cf * sizeof(double));
    double* fac = (double*)w;        w += aligned(factor_doubles(B, C) * sizeof(double));
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_corr(ref, est, lengths, B, C, E, T, r, d, enorm, w, st);
    if (rc == CTN_OK) rc = launch_factor(r, B, C, fac, status, st);
    if (rc == CTN_OK) rc = launch_solve(fac, d, B, C, E, coef_all, coef_own, st);
    if (rc == CTN_OK) rc = launch_project(ref, est, lengths, coef_all, coef_own, B, C, E, T, sdr, sir, sar, nullptr, w, st);
    return rc;
}

}  // extern "C"
