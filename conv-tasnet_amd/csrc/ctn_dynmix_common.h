// What the dynamic mixer's kernel files share (ctn_dynmix.hip, ctn_dynmix_aug.hip): the Philox4x32-10 block, the integer draw,
// the order-free block maximum and the peak rescale.  Contract: include/ctn_hip.h ("on-device dynamic mixing").
#pragma once
#include "ctn_common.h"

namespace {

constexpr int DM_NT = 256;          // threads per workgroup of every kernel of the mixer
constexpr int DM_CHUNK = 4 * DM_NT; // samples per workgroup of the chunked gather (4 consecutive samples per thread)

struct Philox4 { unsigned w[4]; };

__device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
        const unsigned n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        const unsigned n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ unsigned below(unsigned r, unsigned long long n) { return (unsigned)(((unsigned long long)r * n) >> 32); }

template <int NT>
__device__ __forceinline__ float block_max(float v, float* scratch) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = scratch[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) r = fmaxf(r, scratch[w]);
    return r;
}

// The peak rule: 0.9 / a where the peak a lies above `over`, 1 elsewhere.  over = 0: every mixture is rescaled to a peak of 0.9
// (peak mode 0, "always"); over = 0.9: only a mixture that would clip is (peak mode 1, "clip", the LibriMix rule).
__device__ __forceinline__ float peak_scale(float a, float over) { return a > over ? __fdiv_rn(0.9f, a) : 1.0f; }
static inline float peak_over(int peak_mode) { return peak_mode == 1 ? 0.9f : 0.0f; }

}  // namespace
