// Shoebox image-source room simulator (Allen & Berkley 1979) and the same-room RIR draw of the dynamic mixer.
// Contract: include/ctn_hip.h ("image-source room simulator"); executable restatement: tests/ism_oracle.py.
// Every fp64 operation is ONE rounding in the stated order (no contraction into fused multiply-adds, IEEE division and square
// root), no transcendental function, no floating-point atomic: h is a bitwise function of the tables, whatever the launch geometry.
//
// Gather form.  One workgroup of 256 threads owns ISM_CHUNK consecutive taps of one response, one tap per thread.  It walks the
// image lattice in index order, compacts the images whose span meets its taps into an LDS list in that order, and every thread
// drains the list in order into its own accumulator: the additions of a tap happen in ascending image index, as the contract
// asks, without atomics.  LDS: 32 KB of list, 16 KB of staged products, 3 KB of walk tables: 51 KB.
//
// The walk is pruned to the spherical shell the chunk's images lie in.  Rows are the (nx, ny) pairs of the bounding rectangle,
// 256 at a time, one per thread: a row's nz range is the outer sphere's chord minus the inner sphere's (both from bounds on
// Rx^2 + Ry^2 over the four parities), counted, prefix-summed over the workgroup, and the candidates of the 256 rows are then dealt
// to the threads 256 at a time in index order (binary search of the prefix).  The bounds are conservative by a whole tap (about
// 4 cm at 8 kHz) where the fp64 rounding of the pruning arithmetic is below 1e-12 m, so only images that contribute nothing to
// the chunk are skipped; the contract's arithmetic is evaluated for every candidate, and it alone decides what is added.
#include "ctn_dynmix_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int ISM_NT = 256;            // threads per workgroup
constexpr int ISM_CHUNK = ISM_NT;      // taps per workgroup, one per thread
constexpr int ISM_LIST = 2048;         // images in the LDS list before it is drained: 16 bytes each, 32 KB
constexpr int ISM_STAGE = 2048;        // doubles of the drain's staging buffer (16 KB): the products of ISM_STAGE / 2W images
constexpr int ISM_MAX_TAPS = 8192;
constexpr int ISM_MAX_Q = 4096;
constexpr int ISM_MAX_W = 32;
constexpr int ISM_MAX_N = 4096;        // largest lattice bound per axis
constexpr int ISM_ROOM = 16;           // doubles per room row: L[3], mic[3], beta[6], N[3], one unused
constexpr int ISM_RESP = 4;            // doubles per response row: room index, src[3]
constexpr double ISM_MIN_DIST2 = 1e-6; // |src - mic| >= 1e-3 m
constexpr double ISM_MAX_LATTICE = 268435456.0;    // 2^28 lattice entries per room: a walk stays within seconds

struct IsmLayout { long long room, pw, resp, frac, total; };

__host__ __device__ inline IsmLayout ism_layout(int G, int R, int K, int Q, int W) {
    IsmLayout l;
    l.room = 0;
    l.pw = l.room + (long long)G * ISM_ROOM;
    l.resp = l.pw + (long long)G * 6 * K;
    l.frac = l.resp + (long long)R * ISM_RESP;
    l.total = l.frac + (long long)Q * 2 * W;
    return l;
}

// The row checks, the same on the host (before the launch) and in the kernel (again): every comparison is written so that a NaN fails.
__host__ __device__ inline bool ism_row_ok(const double* __restrict__ tb, const IsmLayout& l, int G, int K, int r) {
    const double* rs = tb + l.resp + (long long)r * ISM_RESP;
    if (!(rs[0] >= 0.0 && rs[0] < (double)G) || rs[0] != (double)(int)rs[0]) return false;
    const double* rm = tb + l.room + (long long)(int)rs[0] * ISM_ROOM;
    double d2 = 0.0, lattice = 8.0;
    for (int a = 0; a < 3; ++a) {
        const double L = rm[a], mic = rm[3 + a], src = rs[1 + a], N = rm[12 + a];
        if (!(L > 0.0 && L <= 1e6)) return false;
        if (!(mic > 0.0 && mic < L && src > 0.0 && src < L)) return false;
        if (!(N >= 0.0 && N <= (double)ISM_MAX_N && N + 2.0 <= (double)K) || N != (double)(int)N) return false;
        d2 += (src - mic) * (src - mic);
        lattice *= 2.0 * N + 1.0;
    }
    if (!(lattice <= ISM_MAX_LATTICE)) return false;
    for (int w = 0; w < 6; ++w)
        if (!(rm[6 + w] >= 0.0 && rm[6 + w] <= 1.0)) return false;
    return d2 >= ISM_MIN_DIST2;
}

// exclusive prefix sum of one int per thread over the workgroup, waves in fixed order; total in every thread
__device__ __forceinline__ int ism_block_scan(int v, int* __restrict__ wsum, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                   // wsum may still be read by the call before this one
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < ISM_NT / 64; ++w) {
        if (w < wave) base += wsum[w];
        tot += wsum[w];
    }
    total = tot;
    return base + inc - v;
}

// acc += amp * frac[q][j] for the list's images in order; the product and the add are one rounding each.  Every thread of the
// workgroup calls it with the same n.
// The products of ISM_STAGE / 2W images at a time are staged in LDS first, 2W threads per image: the table rows are read by
// independent, coalesced loads that are all in flight together, where a load inside the ordered loop would wait out its latency
// once per image.  A thread whose tap lies outside an image's span adds +0 instead of branching: acc is never -0 (ctn_hip.h), so
// acc + (+0) keeps its bits.
__device__ __forceinline__ double ism_drain(const double* __restrict__ lamp, const int* __restrict__ li, const int* __restrict__ lq, int n,
                                            const double* __restrict__ frac, int W, int k, double* __restrict__ stage, double acc) {
    const int kw = k + W - 1, w2 = 2 * W, per = ISM_STAGE / w2;
    const int te = (int)threadIdx.x / w2, tj = (int)threadIdx.x - te * w2, estep = ISM_NT / w2;
    for (int b0 = 0; b0 < n; b0 += per) {
        const int m = min(per, n - b0);
        if (te < estep)
            for (int e = te; e < m; e += estep) stage[e * w2 + tj] = lamp[b0 + e] * frac[lq[b0 + e] * w2 + tj];
        __syncthreads();
#pragma unroll 4
        for (int e = 0; e < m; ++e) {
            const int j = kw - li[b0 + e];
            const bool in = (unsigned)j < (unsigned)w2;
            const double v = stage[e * w2 + (in ? j : 0)];
            acc = acc + (in ? v : 0.0);
        }
        __syncthreads();                                // the stage is free again (and, after the last round, so is the list)
    }
    return acc;
}

// grid (R * nchunk): workgroup id -> response id % R, chunk nchunk - 1 - id / R (the late chunks hold the most images: they start first)
__global__ __launch_bounds__(ISM_NT) void ism_kernel(const double* __restrict__ tb, int G, int R, int K, int Q, int W, int n_taps,
                                                     double fs_over_c, double four_pi, int nchunk, double* __restrict__ h,
                                                     int* __restrict__ status, long long* __restrict__ stats) {
    __shared__ double lamp[ISM_LIST];
    __shared__ int li[ISM_LIST];
    __shared__ int lq[ISM_LIST];
    __shared__ double stage[ISM_STAGE];
    __shared__ int prefix[ISM_NT + 1];
    __shared__ int row_hi[ISM_NT];
    __shared__ int row_in[ISM_NT];
    __shared__ int wsum[ISM_NT / 64];
    __shared__ int wcnt[ISM_NT / 64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = (int)(blockIdx.x % (unsigned)R), chunk = nchunk - 1 - (int)(blockIdx.x / (unsigned)R);
    const int k0 = chunk * ISM_CHUNK, kend = min(k0 + ISM_CHUNK, n_taps), k = k0 + tid;
    const IsmLayout lay = ism_layout(G, R, K, Q, W);
    double* const hrow = h + (long long)r * n_taps;

    const bool ok = ism_row_ok(tb, lay, G, K, r);               // the same answer in every thread
    if (chunk == 0 && tid == 0) status[r] = ok ? 0 : -1;
    if (!ok) {
        if (k < kend) hrow[k] = 0.0;
        return;
    }
    const double* const rs = tb + lay.resp + (long long)r * ISM_RESP;
    const int g = (int)rs[0];
    const double* const rm = tb + lay.room + (long long)g * ISM_ROOM;
    const double* const pw = tb + lay.pw + (long long)g * 6 * K;
    const double* const frac = tb + lay.frac;
    const double Lx = rm[0], Ly = rm[1], Lz = rm[2], mx = rm[3], my = rm[4], mz = rm[5];
    const double sx = rs[1], sy = rs[2], sz = rs[3];
    const int Nx = (int)rm[12], Ny = (int)rm[13], Nz = (int)rm[14];
    const double Qd = (double)Q;

    // the shell of this chunk, a tap wider on either side than the images that can reach it: i in [k0 - W, min(kend + W - 1, n_taps))
    const double dhi = (double)(min(kend + W, n_taps) + 1) / fs_over_c;
    const double dlo = k0 - W - 1 > 0 ? (double)(k0 - W - 1) / fs_over_c : 0.0;
    const double dhi2 = dhi * dhi, dlo2 = dlo * dlo;
    // |R_a| >= 2 |n_a| L_a - (src_a + mic_a): beyond these bounds no image lies inside the outer sphere
    const double bx = (dhi + sx + mx) / (2.0 * Lx), by = (dhi + sy + my) / (2.0 * Ly);
    const int nxm = bx >= (double)Nx ? Nx : (int)bx, nym = by >= (double)Ny ? Ny : (int)by;
    const int nyspan = 2 * nym + 1;
    const long long nrows = (long long)(2 * nxm + 1) * nyspan;

    double acc = 0.0;
    int list_n = 0;
    long long visited = 0, counted = 0;

    for (long long row0 = 0; row0 < nrows; row0 += ISM_NT) {
        // ---- the rows of this tile: nz ranges and candidate counts ----
        int hi = -1, in = -1, cnt = 0;
        const long long row = row0 + tid;
        if (row < nrows) {
            const int nx = -nxm + (int)(row / nyspan), ny = -nym + (int)(row % nyspan);
            const double ax = 2.0 * nx * Lx, ay = 2.0 * ny * Ly;
            const double x0 = (sx - mx) + ax, x1 = (-sx - mx) + ax, y0 = (sy - my) + ay, y1 = (-sy - my) + ay;
            const double x02 = x0 * x0, x12 = x1 * x1, y02 = y0 * y0, y12 = y1 * y1;
            const double m = fmin(x02, x12) + fmin(y02, y12), M = fmax(x02, x12) + fmax(y02, y12);
            if (dhi2 > m) {
                const double v = (sqrt(dhi2 - m) + sz + mz) / (2.0 * Lz);
                hi = v >= (double)Nz ? Nz : (int)v;
                if (dlo2 > M) {                                 // |R_z| <= 2 |nz| L_z + (src_z + mic_z): inside the inner sphere for every parity
                    const double u = (sqrt(dlo2 - M) - (sz + mz)) / (2.0 * Lz);
                    if (u > 0.0) in = min((int)ceil(fmin(u, (double)ISM_MAX_N + 2.0)) - 1, hi);
                }
                cnt = 8 * (in >= 0 ? 2 * (hi - in) : 2 * hi + 1);
            }
        }
        int total;
        const int excl = ism_block_scan(cnt, wsum, total);
        prefix[tid] = excl;
        row_hi[tid] = hi;
        row_in[tid] = in;
        if (tid == 0) prefix[ISM_NT] = total;
        __syncthreads();
        visited += total;

        // ---- the candidates of the tile in index order, 256 at a time ----
        for (int base = 0; base < total; base += ISM_NT) {
            if (list_n + ISM_NT > ISM_LIST) {                   // the next batch may not fit: drain (every thread takes this branch)
                acc = ism_drain(lamp, li, lq, list_n, frac, W, k, stage, acc);
                list_n = 0;
                __syncthreads();
            }
            const int t = base + tid;
            bool keep = false;
            double amp = 0.0;
            int ii = 0, qq = 0;
            if (t < total) {
                int lo = 0, up = ISM_NT;                        // the row with prefix[row] <= t < prefix[row + 1]
                while (up - lo > 1) {
                    const int mid = (lo + up) >> 1;
                    if (prefix[mid] <= t) lo = mid; else up = mid;
                }
                const long long rw = row0 + lo;
                const int nx = -nxm + (int)(rw / nyspan), ny = -nym + (int)(rw % nyspan);
                const int u = t - prefix[lo], zi = u >> 3, p = u & 7;
                const int rh = row_hi[lo], ri = row_in[lo];
                const int nz = (ri < 0 || zi < rh - ri) ? -rh + zi : ri + 1 + (zi - (rh - ri));
                const int px = p >> 2, py = (p >> 1) & 1, pz = p & 1;
                // the contract's arithmetic, one rounding per operation
                const double Rx = ((px ? -sx : sx) - mx) + (double)(2 * nx) * Lx;
                const double Ry = ((py ? -sy : sy) - my) + (double)(2 * ny) * Ly;
                const double Rz = ((pz ? -sz : sz) - mz) + (double)(2 * nz) * Lz;
                const double d2 = (Rx * Rx + Ry * Ry) + Rz * Rz;
                const double d = sqrt(d2);
                const double tau = d * fs_over_c;
                const double fi = floor(tau);
                if (fi < (double)n_taps) {
                    ii = (int)fi;
                    if (ii + W >= k0 && ii - W + 1 < kend) {
                        const double bpx = pw[0 * K + abs(nx - px)] * pw[1 * K + abs(nx)];
                        const double bpy = pw[2 * K + abs(ny - py)] * pw[3 * K + abs(ny)];
                        const double bpz = pw[4 * K + abs(nz - pz)] * pw[5 * K + abs(nz)];
                        amp = ((bpx * bpy) * bpz) / (d * four_pi);
                        qq = min((int)floor((tau - fi) * Qd), Q - 1);          // < Q by the arithmetic (ctn_hip.h); clamped all the same
                        keep = amp != 0.0;                                     // a zero image adds +-0: the same bits (ctn_hip.h)
                        if (keep && ii >= k0 && ii < kend) ++counted;
                    }
                }
            }
            const unsigned long long ball = __ballot(keep);
            if (lane == 0) wcnt[wave] = __popcll(ball);
            __syncthreads();
            int off = list_n, tot = 0;
#pragma unroll
            for (int w = 0; w < ISM_NT / 64; ++w) {
                if (w < wave) off += wcnt[w];
                tot += wcnt[w];
            }
            if (keep) {
                off += __popcll(ball & ((1ull << lane) - 1ull));
                lamp[off] = amp;
                li[off] = ii;
                lq[off] = qq;
            }
            list_n += tot;
            __syncthreads();                                    // the list is written, wcnt and (after the last batch) prefix are free
        }
        __syncthreads();
    }
    acc = ism_drain(lamp, li, lq, list_n, frac, W, k, stage, acc);
    if (k < kend) hrow[k] = acc;
    if (stats != nullptr) {
        if (tid == 0) atomicAdd(reinterpret_cast<unsigned long long*>(stats), (unsigned long long)visited);
        if (counted != 0) atomicAdd(reinterpret_cast<unsigned long long*>(stats) + 1, (unsigned long long)counted);
    }
}

// One workgroup; thread b draws mixture b (and b + NT, ...).  Reads the step word and leaves it alone.
__global__ __launch_bounds__(DM_NT) void dynmix_plan_rooms_kernel(unsigned k0, unsigned k1, unsigned epoch, const unsigned* __restrict__ step_word,
                                                                  int B, int C, int G, int P, int* __restrict__ plan_rir) {
    const unsigned step = *step_word;
    for (int b = threadIdx.x; b < B; b += DM_NT) {
        const int g = (int)below(philox4x32_10(512u, (unsigned)b, step, epoch, k0, k1).w[0], (unsigned long long)G);
        int taken[4];                                           // the positions of sources 0 .. c - 1, ascending
        for (int c = 0; c < C; ++c) {
            const Philox4 rw = philox4x32_10((unsigned)c + 512u, (unsigned)b, step, epoch, k0, k1);
            int s = (int)below(rw.w[1], (unsigned long long)(P - c));
            int at = 0;
            for (; at < c && s >= taken[at]; ++at) ++s;         // the s-th position not yet taken
            for (int m = c; m > at; --m) taken[m] = taken[m - 1];
            taken[at] = s;
            plan_rir[b * C + c] = g * P + s;
        }
    }
}

}  // namespace

extern "C" {

int ctn_ism_list_capacity(void) { return ISM_LIST; }
int ctn_ism_chunk_taps(void) { return ISM_CHUNK; }

long long ctn_ism_table_doubles(int G, int R, int K, int Q, int W) {
    if (G < 1 || R < 1 || K < 2 || K > ISM_MAX_N + 2 || Q < 1 || Q > ISM_MAX_Q || W < 1 || W > ISM_MAX_W) return 0;
    return ism_layout(G, R, K, Q, W).total;
}

int ctn_ism_simulate(const double* tables_host, const double* tables, int G, int R, int K, int Q, int W, int n_taps, double fs_over_c,
                     double four_pi, double* h, int* status, long long* stats, void* stream) {
    CTN_REQUIRE(tables_host && tables && h && status, "ctn_ism_simulate: null pointer");
    CTN_REQUIRE(G >= 1 && G <= (1 << 20), "ctn_ism_simulate: G = %d rooms (1 .. 2^20)", G);
    CTN_REQUIRE(R >= 1 && R <= (1 << 20), "ctn_ism_simulate: R = %d responses (1 .. 2^20)", R);
    CTN_REQUIRE(K >= 2 && K <= ISM_MAX_N + 2, "ctn_ism_simulate: K = %d powers per wall (2 .. %d)", K, ISM_MAX_N + 2);
    CTN_REQUIRE(Q >= 1 && Q <= ISM_MAX_Q, "ctn_ism_simulate: Q = %d phases (1 .. %d)", Q, ISM_MAX_Q);
    CTN_REQUIRE(W >= 1 && W <= ISM_MAX_W, "ctn_ism_simulate: W = %d (1 .. %d)", W, ISM_MAX_W);
    CTN_REQUIRE(n_taps >= 1 && n_taps <= ISM_MAX_TAPS, "ctn_ism_simulate: n_taps = %d (1 .. %d)", n_taps, ISM_MAX_TAPS);
    CTN_REQUIRE(fs_over_c > 0.0 && fs_over_c <= 1e9, "ctn_ism_simulate: fs_over_c = %g", fs_over_c);
    CTN_REQUIRE(four_pi > 0.0 && four_pi <= 1e9, "ctn_ism_simulate: four_pi = %g", four_pi);
    const IsmLayout lay = ism_layout(G, R, K, Q, W);
    for (int r = 0; r < R; ++r)
        CTN_REQUIRE(ism_row_ok(tables_host, lay, G, K, r),
                    "ctn_ism_simulate: response %d breaks its tables (room index, dimensions, lattice bounds against K = %d and 2^28 "
                    "entries, positions strictly inside the room, |src - mic| >= 1e-3 m, beta in [0, 1])", r, K);
    const int nchunk = ctn_cdiv(n_taps, ISM_CHUNK);
    ism_kernel<<<dim3((unsigned)R * (unsigned)nchunk), dim3(ISM_NT), 0, (hipStream_t)stream>>>(tables, G, R, K, Q, W, n_taps, fs_over_c,
                                                                                                four_pi, nchunk, h, status, stats);
    CTN_CHECK_LAUNCH("ctn_ism_simulate");
    return CTN_OK;
}

int ctn_dynmix_plan_rooms(long long seed, int epoch, int rank, const unsigned* step, int B, int C, int G, int P, int* plan_rir,
                          void* stream) {
    CTN_REQUIRE(step && plan_rir, "ctn_dynmix_plan_rooms: null pointer");
    CTN_REQUIRE(C >= 2 && C <= 4, "ctn_dynmix_plan_rooms: C = %d sources per mixture (2 .. 4)", C);
    CTN_REQUIRE(B >= 1 && B <= (1 << 20), "ctn_dynmix_plan_rooms: B = %d mixtures (1 .. 2^20)", B);
    CTN_REQUIRE(P >= C && P <= 64, "ctn_dynmix_plan_rooms: P = %d positions per room (C = %d .. 64)", P, C);
    CTN_REQUIRE(G >= 1 && (long long)G * P <= 0x7fffffffLL, "ctn_dynmix_plan_rooms: G = %d rooms of %d positions", G, P);
    CTN_REQUIRE(seed >= 0 && seed < (1LL << 48), "ctn_dynmix_plan_rooms: seed %lld outside [0, 2^48)", seed);
    CTN_REQUIRE(rank >= 0 && rank < (1 << 16), "ctn_dynmix_plan_rooms: rank %d outside [0, 2^16)", rank);
    CTN_REQUIRE(epoch >= 0, "ctn_dynmix_plan_rooms: epoch %d", epoch);
    const unsigned k0 = (unsigned)(seed & 0xffffffffLL), k1 = (unsigned)(seed >> 32) | ((unsigned)rank << 16);
    dynmix_plan_rooms_kernel<<<dim3(1), dim3(DM_NT), 0, (hipStream_t)stream>>>(k0, k1, (unsigned)epoch, step, B, C, G, P, plan_rir);
    CTN_CHECK_LAUNCH("ctn_dynmix_plan_rooms");
    return CTN_OK;
}

}  // extern "C"
