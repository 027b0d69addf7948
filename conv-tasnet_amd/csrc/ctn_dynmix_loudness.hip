// LibriMix-recipe levels for the dynamic mixer: one more draw per source, its absolute loudness, and the gain that brings the
// utterance there.  Contract: include/ctn_hip.h ("LibriMix-recipe mixing"); executable restatement:
// tests/dynmix_loudness_oracle.py.
//
// The speaker, utterance, start, level, speed, RIR, noise and count draws keep their Philox blocks (c0 = c, 256 + c, 512 + c, 768,
// 1024); the loudness takes c0 = 1280 + c.  Only gain[b, c] changes: the gather, speed, reverberation and noise kernels run
// unchanged.  The peak rule of the recipe (rescale only what would clip) is peak mode 1 of ctn_dynmix_gather_peak /
// ctn_dynmix_gather_aug_peak.
#include "ctn_dynmix_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int DL_MAX = 1024;        // most entries of the loudness table

// One workgroup; thread b draws mixture b (and b + NT, ...).  Launched BEHIND ctn_dynmix_plan / ctn_dynmix_plan_speed, which have
// advanced the step word: the minibatch's step is *step_word - 1.
__global__ __launch_bounds__(DM_NT) void dynmix_plan_loudness_kernel(const int* __restrict__ plan_utt, const float* __restrict__ inv_rms,
                                                                     int U, const float* __restrict__ wl, int nl, int lo10, unsigned k0,
                                                                     unsigned k1, unsigned epoch, const unsigned* __restrict__ step_word,
                                                                     int B, int C, int* __restrict__ plan_l10, float* __restrict__ gain) {
    const unsigned step = *step_word - 1u;
    for (int b = threadIdx.x; b < B; b += DM_NT) {
        for (int c = 0; c < C; ++c) {
            const Philox4 r = philox4x32_10(1280u + (unsigned)c, (unsigned)b, step, epoch, k0, k1);
            const int i = (int)below(r.w[0], (unsigned long long)nl);
            const int o = b * C + c, u = plan_utt[o];
            plan_l10[o] = lo10 + i;
            gain[o] = (u >= 0 && u < U) ? wl[i] * inv_rms[u] : 0.0f;      // a flagged plan entry keeps gain 0
        }
    }
}

}  // namespace

extern "C" {

// see include/ctn_hip.h
int ctn_dynmix_plan_loudness(const int* plan_utt, const float* inv_rms, long long U, const float* wl, int nl, int lo10, long long seed,
                             int epoch, int rank, const unsigned* step, int B, int C, int* plan_l10, float* gain, void* stream) {
    CTN_REQUIRE(plan_utt && inv_rms && wl && step && plan_l10 && gain, "ctn_dynmix_plan_loudness: null pointer");
    CTN_REQUIRE(U >= 1 && U <= 0x7fffffffLL, "ctn_dynmix_plan_loudness: U = %lld utterances (1 .. 2^31 - 1)", U);
    CTN_REQUIRE(nl >= 1 && nl <= DL_MAX, "ctn_dynmix_plan_loudness: nl = %d loudness values (1 .. %d)", nl, DL_MAX);
    CTN_REQUIRE(C >= 2 && C <= 4, "ctn_dynmix_plan_loudness: C = %d sources per mixture (2 .. 4)", C);
    CTN_REQUIRE(B >= 1 && B <= (1 << 20), "ctn_dynmix_plan_loudness: B = %d mixtures (1 .. 2^20)", B);
    CTN_REQUIRE(seed >= 0 && seed < (1LL << 48), "ctn_dynmix_plan_loudness: seed %lld outside [0, 2^48)", seed);
    CTN_REQUIRE(rank >= 0 && rank < (1 << 16), "ctn_dynmix_plan_loudness: rank %d outside [0, 2^16)", rank);
    CTN_REQUIRE(epoch >= 0, "ctn_dynmix_plan_loudness: epoch %d", epoch);
    const unsigned k0 = (unsigned)(seed & 0xffffffffLL), k1 = (unsigned)(seed >> 32) | ((unsigned)rank << 16);
    dynmix_plan_loudness_kernel<<<dim3(1), dim3(DM_NT), 0, (hipStream_t)stream>>>(plan_utt, inv_rms, (int)U, wl, nl, lo10, k0, k1,
                                                                                  (unsigned)epoch, step, B, C, plan_l10, gain);
    CTN_CHECK_LAUNCH("ctn_dynmix_plan_loudness");
    return CTN_OK;
}

}  // extern "C"
