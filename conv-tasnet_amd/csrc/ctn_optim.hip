// Flat-buffer optimiser step (src/solver.py:194-196 with Adam from src/train.py:92-95), gfx950.
//
// The whole model lives in one flat fp32 buffer (and so do its gradient and the two Adam
// moments), so the per-step tail of the training loop is three streaming kernels instead of
// 294 x (norm, clip-scale, 4 Adam ops):  sum-of-squares partials -> clip coefficient + Adam.
// The same flat gradient is the single RCCL all-reduce payload in data-parallel runs.
// torch.optim.SGD (momentum / dampening / nesterov) and coupled-L2 Adam reuse the same partials: src/train.py:87-98.
#include "ctn_common.h"

namespace {

constexpr int NT = 256;
constexpr int MAXPART = 1024;

__global__ __launch_bounds__(NT) void sumsq_kernel(const float* __restrict__ g, long long n, double* __restrict__ part) {
    __shared__ double red[NT / 64];
    double s = 0.0;
    const long long n4 = n / 4;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long long)gridDim.x * NT) {
        const float4 v = *reinterpret_cast<const float4*>(g + 4 * i);
        s += (double)(v.x * v.x + v.y * v.y) + (double)(v.z * v.z + v.w * v.w);
    }
    if (blockIdx.x == 0)
        for (long long i = n4 * 4 + threadIdx.x; i < n; i += NT) s += (double)g[i] * g[i];
    s = block_sum<double, NT>(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// grad_scale multiplies g before everything (1/world after a sum all-reduce).
// total_norm_out[0] = ||grad_scale * g||_2 ; coef = min(1, max_norm / (norm + 1e-6)) as clip_grad_norm_.
__global__ __launch_bounds__(NT) void clip_adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v, long long n,
                                                       const double* __restrict__ part, int nparts, float grad_scale,
                                                       float max_norm, float lr, float b1, float b2, float eps,
                                                       float bc1, float bc2_sqrt, float* __restrict__ total_norm_out) {
    __shared__ double red[NT / 64];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += NT) s += part[i];
    s = block_sum<double, NT>(s, red);
    const float total = (float)sqrt(s) * fabsf(grad_scale);
    float coef = 1.f;
    if (max_norm > 0.f) coef = fminf(max_norm / (total + 1e-6f), 1.f);
    if (blockIdx.x == 0 && threadIdx.x == 0 && total_norm_out != nullptr) total_norm_out[0] = total;
    const float gs = grad_scale * coef;
    const float step = lr / bc1;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
        const float gi = g[i] * gs;
        const float mi = m[i] * b1 + gi * (1.f - b1);
        const float vi = v[i] * b2 + (gi * gi) * (1.f - b2);
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p[i] = p[i] - step * (mi / denom);
    }
}

// ---- SGD and coupled-L2 Adam (torch.optim.SGD / torch.optim.Adam(weight_decay=...)) ---------------------------------
// Same clip as clip_adam_kernel: every block re-sums the sumsq partials in the same order (no atomics), so all blocks
// see the same coefficient and the result is bitwise reproducible.  The weight-decay term is added AFTER the clip
// (the reference Solver clips before optimizer.step() adds it) and does not enter the norm.
__device__ __forceinline__ float clip_scale(const double* __restrict__ part, int nparts, float grad_scale, float max_norm,
                                            float* __restrict__ total_norm_out, double* red) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += NT) s += part[i];
    s = block_sum<double, NT>(s, red);
    const float total = (float)sqrt(s) * fabsf(grad_scale);
    float coef = 1.f;
    if (max_norm > 0.f) coef = fminf(max_norm / (total + 1e-6f), 1.f);
    if (blockIdx.x == 0 && threadIdx.x == 0 && total_norm_out != nullptr) total_norm_out[0] = total;
    return grad_scale * coef;
}

// d = g*gs + wd*p; with momentum: buf = first ? d : mom*buf + (1-damp)*d; d = nesterov ? d + mom*buf : buf; p -= lr*d
template <bool MOM, bool NEST>
__device__ __forceinline__ float sgd_elem(float p, float g, float& b, float gs, float lr, float mom, float damp1, float wd,
                                          bool first) {
    float d = g * gs + wd * p;
    if (MOM) {
        b = first ? d : b * mom + d * damp1;
        d = NEST ? d + mom * b : b;
    }
    return p - lr * d;
}

// float4 body over n/4 vectors (grid-stride), scalar tail of n%4 elements in block 0.  momentum_buf untouched if !MOM.
template <bool MOM, bool NEST>
__global__ __launch_bounds__(NT) void clip_sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                      float* __restrict__ buf, long long n, const double* __restrict__ part,
                                                      int nparts, float grad_scale, float max_norm, float lr, float mom,
                                                      float dampening, float wd, int first_step,
                                                      float* __restrict__ total_norm_out) {
    __shared__ double red[NT / 64];
    const float gs = clip_scale(part, nparts, grad_scale, max_norm, total_norm_out, red);
    const float damp1 = 1.f - dampening;
    const bool first = first_step != 0;
    const long long n4 = n / 4;
    float4* __restrict__ p4 = reinterpret_cast<float4*>(p);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    float4* __restrict__ b4 = reinterpret_cast<float4*>(buf);
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long long)gridDim.x * NT) {
        float4 pv = p4[i];
        const float4 gv = g4[i];
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (MOM && !first) bv = b4[i];
        pv.x = sgd_elem<MOM, NEST>(pv.x, gv.x, bv.x, gs, lr, mom, damp1, wd, first);
        pv.y = sgd_elem<MOM, NEST>(pv.y, gv.y, bv.y, gs, lr, mom, damp1, wd, first);
        pv.z = sgd_elem<MOM, NEST>(pv.z, gv.z, bv.z, gs, lr, mom, damp1, wd, first);
        pv.w = sgd_elem<MOM, NEST>(pv.w, gv.w, bv.w, gs, lr, mom, damp1, wd, first);
        if (MOM) b4[i] = bv;
        p4[i] = pv;
    }
    if (blockIdx.x == 0)
        for (long long i = n4 * 4 + threadIdx.x; i < n; i += NT) {
            float b = (MOM && !first) ? buf[i] : 0.f;
            p[i] = sgd_elem<MOM, NEST>(p[i], g[i], b, gs, lr, mom, damp1, wd, first);
            if (MOM) buf[i] = b;
        }
}

// the clip_adam_kernel update with gi = g*gs + wd*p (coupled L2 as torch.optim.Adam(weight_decay=wd); not AdamW)
__device__ __forceinline__ float adam_l2_elem(float p, float g, float& m, float& v, float gs, float wd, float b1,
                                              float b2, float eps, float step, float bc2_sqrt) {
    const float gi = g * gs + wd * p;
    m = m * b1 + gi * (1.f - b1);
    v = v * b2 + (gi * gi) * (1.f - b2);
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    return p - step * (m / denom);
}

__global__ __launch_bounds__(NT) void clip_adam_l2_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v, long long n,
                                                          const double* __restrict__ part, int nparts, float grad_scale,
                                                          float max_norm, float lr, float b1, float b2, float eps,
                                                          float bc1, float bc2_sqrt, float wd,
                                                          float* __restrict__ total_norm_out) {
    __shared__ double red[NT / 64];
    const float gs = clip_scale(part, nparts, grad_scale, max_norm, total_norm_out, red);
    const float step = lr / bc1;
    const long long n4 = n / 4;
    float4* __restrict__ p4 = reinterpret_cast<float4*>(p);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    float4* __restrict__ m4 = reinterpret_cast<float4*>(m);
    float4* __restrict__ v4 = reinterpret_cast<float4*>(v);
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long long)gridDim.x * NT) {
        float4 pv = p4[i], mv = m4[i], vv = v4[i];
        const float4 gv = g4[i];
        pv.x = adam_l2_elem(pv.x, gv.x, mv.x, vv.x, gs, wd, b1, b2, eps, step, bc2_sqrt);
        pv.y = adam_l2_elem(pv.y, gv.y, mv.y, vv.y, gs, wd, b1, b2, eps, step, bc2_sqrt);
        pv.z = adam_l2_elem(pv.z, gv.z, mv.z, vv.z, gs, wd, b1, b2, eps, step, bc2_sqrt);
        pv.w = adam_l2_elem(pv.w, gv.w, mv.w, vv.w, gs, wd, b1, b2, eps, step, bc2_sqrt);
        m4[i] = mv;
        v4[i] = vv;
        p4[i] = pv;
    }
    if (blockIdx.x == 0)
        for (long long i = n4 * 4 + threadIdx.x; i < n; i += NT) {
            float mi = m[i], vi = v[i];
            p[i] = adam_l2_elem(p[i], g[i], mi, vi, gs, wd, b1, b2, eps, step, bc2_sqrt);
            m[i] = mi;
            v[i] = vi;
        }
}

// sumsq partials of the clip, shared by the SGD and Adam+L2 entry points; -> number of partials
inline int launch_sumsq(const float* grads, long long n, double* workspace, hipStream_t st) {
    long long nb = ctn_cdivll(n / 4 + 1, NT);
    if (nb > MAXPART) nb = MAXPART;
    hipLaunchKernelGGL(sumsq_kernel, dim3((unsigned)nb), dim3(NT), 0, st, grads, n, workspace);
    return (int)nb;
}

// update grid: one float4 per thread, capped at 2048 blocks and grid-strided beyond
inline unsigned update_blocks(long long n) {
    long long nb = ctn_cdivll(n / 4 + 1, NT);
    return (unsigned)(nb > 2048 ? 2048 : nb);
}

}  // namespace

extern "C" {

int ctn_optim_parts(void) { return MAXPART; }

// workspace: ctn_optim_parts() doubles
int ctn_clip_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n,
                       float grad_scale, float max_norm, float lr, float beta1, float beta2, float eps, int step,
                       float* total_norm_out, double* workspace, void* stream) {
    CTN_REQUIRE(params && grads && exp_avg && exp_avg_sq && workspace, "ctn_clip_adam_step: null pointer");
    CTN_REQUIRE(n > 0 && step >= 1, "ctn_clip_adam_step: bad sizes");
    CTN_REQUIRE((reinterpret_cast<uintptr_t>(grads) & 15) == 0, "ctn_clip_adam_step: grads must be 16-byte aligned");
    long long nb = ctn_cdivll(n / 4 + 1, NT);
    if (nb > MAXPART) nb = MAXPART;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sumsq_kernel, dim3((unsigned)nb), dim3(NT), 0, st, grads, n, workspace);
    CTN_CHECK_LAUNCH("ctn_clip_adam_step/sumsq");
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    long long nb2 = ctn_cdivll(n, NT);
    if (nb2 > 2048) nb2 = 2048;
    hipLaunchKernelGGL(clip_adam_kernel, dim3((unsigned)nb2), dim3(NT), 0, st, params, grads, exp_avg, exp_avg_sq, n,
                       (const double*)workspace, (int)nb, grad_scale, max_norm, lr, beta1, beta2, eps, (float)bc1,
                       (float)sqrt(bc2), total_norm_out);
    CTN_CHECK_LAUNCH("ctn_clip_adam_step/adam");
    return CTN_OK;
}

int ctn_clip_sgd_step(float* params, const float* grads, float* momentum_buf, long long n, float grad_scale,
                      float max_norm, float lr, float momentum, float dampening, float weight_decay, int nesterov,
                      int first_step, float* total_norm_out, double* workspace, void* stream) {
    CTN_REQUIRE(params && grads && workspace, "ctn_clip_sgd_step: null pointer");
    CTN_REQUIRE(momentum == 0.f || momentum_buf, "ctn_clip_sgd_step: null pointer (momentum_buf with momentum != 0)");
    CTN_REQUIRE(n > 0, "ctn_clip_sgd_step: bad sizes");
    CTN_REQUIRE(ctn_aligned16(grads) && ctn_aligned16(params) && (momentum == 0.f || ctn_aligned16(momentum_buf)),
                "ctn_clip_sgd_step: grads, params and momentum_buf must be 16-byte aligned");
    CTN_REQUIRE(!nesterov || (momentum > 0.f && dampening == 0.f),
                "ctn_clip_sgd_step: nesterov momentum requires a momentum and zero dampening");
    hipStream_t st = (hipStream_t)stream;
    const int nb = launch_sumsq(grads, n, workspace, st);
    CTN_CHECK_LAUNCH("ctn_clip_sgd_step/sumsq");
    const dim3 grid(update_blocks(n)), block(NT);
    const double* part = workspace;
    if (momentum == 0.f)
        hipLaunchKernelGGL((clip_sgd_kernel<false, false>), grid, block, 0, st, params, grads, nullptr, n, part, nb,
                           grad_scale, max_norm, lr, 0.f, dampening, weight_decay, first_step, total_norm_out);
    else if (nesterov)
        hipLaunchKernelGGL((clip_sgd_kernel<true, true>), grid, block, 0, st, params, grads, momentum_buf, n, part, nb,
                           grad_scale, max_norm, lr, momentum, dampening, weight_decay, first_step, total_norm_out);
    else
        hipLaunchKernelGGL((clip_sgd_kernel<true, false>), grid, block, 0, st, params, grads, momentum_buf, n, part, nb,
                           grad_scale, max_norm, lr, momentum, dampening, weight_decay, first_step, total_norm_out);
    CTN_CHECK_LAUNCH("ctn_clip_sgd_step/sgd");
    return CTN_OK;
}

int ctn_clip_adam_l2_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n,
                          float grad_scale, float max_norm, float lr, float beta1, float beta2, float eps, int step,
                          float weight_decay, float* total_norm_out, double* workspace, void* stream) {
    CTN_REQUIRE(params && grads && exp_avg && exp_avg_sq && workspace, "ctn_clip_adam_l2_step: null pointer");
    CTN_REQUIRE(n > 0 && step >= 1, "ctn_clip_adam_l2_step: bad sizes");
    CTN_REQUIRE(ctn_aligned16(grads) && ctn_aligned16(params) && ctn_aligned16(exp_avg) && ctn_aligned16(exp_avg_sq),
                "ctn_clip_adam_l2_step: grads, params, exp_avg and exp_avg_sq must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int nb = launch_sumsq(grads, n, workspace, st);
    CTN_CHECK_LAUNCH("ctn_clip_adam_l2_step/sumsq");
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(clip_adam_l2_kernel, dim3(update_blocks(n)), dim3(NT), 0, st, params, grads, exp_avg, exp_avg_sq, n,
                       (const double*)workspace, nb, grad_scale, max_norm, lr, beta1, beta2, eps, (float)bc1,
                       (float)sqrt(bc2), weight_decay, total_norm_out);
    CTN_CHECK_LAUNCH("ctn_clip_adam_l2_step/adam");
    return CTN_OK;
}

}  // extern "C"
