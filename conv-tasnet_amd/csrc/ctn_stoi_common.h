// Constants and small helpers shared by the STOI / ESTOI forward kernels (ctn_stoi.hip) and their backward pass
// (ctn_stoi_grad.hip).  Library-internal.
#pragma once
#include "ctn_common.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int FL = 256;       // frame length
constexpr int HOP = 128;
constexpr int NSEG = 30;      // frames per segment
constexpr int NBAND = 15;
constexpr int BIN0 = 7;       // first bin of band 0
constexpr int NTILE = 14;     // 16-bin tiles: bins 7 .. 230 cover the bands' 7 .. 218
constexpr int NBINS = 16 * NTILE;
constexpr int FT = 16;        // output frames per workgroup of the band kernel
constexpr int ZLEN = (FT + 1) * HOP;          // compacted samples under 16 consecutive frames
constexpr int ZPAD = ZLEN + 2 * (FT + 1);     // two doubles of padding per 128: the 16 frames of a B operand hit different banks
constexpr int NT = 256;
constexpr int NTF = 1024;     // threads of the frame kernel: a row's frames are dealt to its 16 waves
constexpr int SEGT = 64;      // segments per workgroup of the score kernel
constexpr int SFR = SEGT + NSEG - 1;
constexpr double TOO_SHORT = 1e-5;

__constant__ int BAND_FIRST[NBAND] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174};
__constant__ int BAND_WIDTH[NBAND] = {2, 2, 3, 3, 5, 5, 7, 9, 12, 14, 18, 22, 29, 36, 45};

typedef double double4_t __attribute__((ext_vector_type(4)));

__host__ __device__ __forceinline__ long long frames_of(long long n) { return n > FL ? (n - FL + HOP - 1) / HOP : 0; }

__device__ __forceinline__ long long clamp_len(const long long* lens, long long b, long long T) {
    const long long n = lens[b];
    return n < 0 ? 0 : (n > T ? T : n);
}

// np.hanning(258)[1:-1]
__device__ __forceinline__ double window_at(int n) { return 0.5 - 0.5 * cospi(2.0 * (double)(n + 1) / 257.0); }

__device__ __forceinline__ int zpos(int p) { return p + 2 * (p >> 7); }

constexpr size_t ALIGN = 256;
inline size_t aligned(size_t bytes) { return (bytes + ALIGN - 1) / ALIGN * ALIGN; }

inline int max_frames(long long T) { return (int)frames_of(T); }
inline int env_frames(long long T) { const int nf = max_frames(T); return nf > 1 ? nf - 1 : 1; }
inline int alloc_frames(long long T) { const int nf = max_frames(T); return nf > 1 ? nf : 1; }
inline int seg_chunks(long long T) { const int s = env_frames(T) - NSEG + 1; return s > 0 ? (s + SEGT - 1) / SEGT : 1; }

}  // namespace
