// Variable speaker counts for the dynamic mixer: one more draw per mixture, the number of active sources n_b in [m, C], and the
// masking of the plan's gains behind it.  Contract: include/ctn_hip.h ("variable speaker counts"); executable restatement:
// tests/dynmix_active_oracle.py.
//
// The speaker, utterance, start, level, speed, RIR and noise draws keep their Philox blocks (c0 = c, 256 + c, 512 + c, 768); the
// count takes c0 = 1024.  Only gain[b, c >= n_b] changes, to +0: the gather, speed, reverberation and noise kernels run unchanged
// and a masked row comes out as zeros that add nothing to the mixture or its peak.
#include "ctn_dynmix_common.h"

namespace {

// One workgroup; thread b draws mixture b (and b + NT, ...).  Reads the step word and leaves it alone: ctn_dynmix_plan /
// ctn_dynmix_plan_speed, launched behind this kernel on the same stream, advance it.
__global__ __launch_bounds__(DM_NT) void dynmix_plan_active_kernel(unsigned k0, unsigned k1, unsigned epoch,
                                                                   const unsigned* __restrict__ step_word, int B, int C, int m,
                                                                   int* __restrict__ n_active) {
    const unsigned step = *step_word;
    for (int b = threadIdx.x; b < B; b += DM_NT) {
        const Philox4 r = philox4x32_10(1024u, (unsigned)b, step, epoch, k0, k1);
        n_active[b] = m + (int)below(r.w[0], (unsigned long long)(C - m + 1));
    }
}

// gain [B,C]: entries c >= n_active[b] become +0
__global__ __launch_bounds__(DM_NT) void dynmix_mask_active_kernel(const int* __restrict__ n_active, int B, int C,
                                                                   float* __restrict__ gain) {
    const int k = blockIdx.x * DM_NT + threadIdx.x;
    if (k >= B * C) return;
    if (k % C >= n_active[k / C]) gain[k] = 0.0f;
}

}  // namespace

extern "C" {

// see include/ctn_hip.h
int ctn_dynmix_plan_active(long long seed, int epoch, int rank, const unsigned* step, int B, int C, int min_speakers, int* n_active,
                           void* stream) {
    CTN_REQUIRE(step && n_active, "ctn_dynmix_plan_active: null pointer");
    CTN_REQUIRE(C >= 2 && C <= 4, "ctn_dynmix_plan_active: C = %d sources per mixture (2 .. 4)", C);
    CTN_REQUIRE(min_speakers >= 1 && min_speakers <= C, "ctn_dynmix_plan_active: min_speakers = %d outside 1 .. %d", min_speakers, C);
    CTN_REQUIRE(B >= 1 && B <= (1 << 20), "ctn_dynmix_plan_active: B = %d mixtures (1 .. 2^20)", B);
    CTN_REQUIRE(seed >= 0 && seed < (1LL << 48), "ctn_dynmix_plan_active: seed %lld outside [0, 2^48)", seed);
    CTN_REQUIRE(rank >= 0 && rank < (1 << 16), "ctn_dynmix_plan_active: rank %d outside [0, 2^16)", rank);
    CTN_REQUIRE(epoch >= 0, "ctn_dynmix_plan_active: epoch %d", epoch);
    const unsigned k0 = (unsigned)(seed & 0xffffffffLL), k1 = (unsigned)(seed >> 32) | ((unsigned)rank << 16);
    dynmix_plan_active_kernel<<<dim3(1), dim3(DM_NT), 0, (hipStream_t)stream>>>(k0, k1, (unsigned)epoch, step, B, C, min_speakers,
                                                                                n_active);
    CTN_CHECK_LAUNCH("ctn_dynmix_plan_active");
    return CTN_OK;
}

int ctn_dynmix_mask_active(const int* n_active, int B, int C, float* gain, void* stream) {
    CTN_REQUIRE(n_active && gain, "ctn_dynmix_mask_active: null pointer");
    CTN_REQUIRE(C >= 2 && C <= 4, "ctn_dynmix_mask_active: C = %d sources per mixture (2 .. 4)", C);
    CTN_REQUIRE(B >= 1 && B <= (1 << 20), "ctn_dynmix_mask_active: B = %d mixtures (1 .. 2^20)", B);
    dynmix_mask_active_kernel<<<dim3((unsigned)ctn_cdiv(B * C, DM_NT)), dim3(DM_NT), 0, (hipStream_t)stream>>>(n_active, B, C, gain);
    CTN_CHECK_LAUNCH("ctn_dynmix_mask_active");
    return CTN_OK;
}

}  // extern "C"
