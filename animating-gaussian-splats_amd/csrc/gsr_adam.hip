// gsr_adam.hip -- one-launch Adam step over every per-Gaussian parameter tensor (SURVEY.md 8(f)
// row 3), replacing torch.optim.Adam (densify.py:68-86: one named group per parameter, eps 1e-15,
// betas (0.9, 0.999), no weight decay) whose foreach path runs ~8 elementwise kernels per group, each
// streaming the parameter / gradient / moments through HBM again.
//
// k_adam: blocks walk a table of up to kAdamMaxTensors tensors (block -> tensor by a prefix of block
// counts, passed in the kernel arguments); each thread updates 4 consecutive elements (float4 when
// the tensor is 16-byte aligned) with the operation order of torch's _multi_tensor_adam:
//   m = lerp(m, g, 1 - beta1)                   = m + w (g - m)            (w < 0.5 form, fused)
//   v = v * beta2;  v = v + (1 - beta2) (g g)   (addcmul, fused)
//   d = sqrt(v) / sqrt(1 - beta2^t) + eps
//   p = p + step_size * (m / d),  step_size = -lr / (1 - beta1^t)           (addcdiv, fused)
// Per-tensor scalars are computed on the host in double exactly as torch does and rounded to float.
// Algorithmic HBM bytes: 28 per element (read p, g, m, v; write p, m, v).
//
// Gradient norm (train.py:432-443 calculate_gradient_norm, one .norm(2).pow(2) and one host read per
// parameter there): every block also reduces its gradients' squares, in double, to one partial
// (k_adam<true>, or k_grad_sumsq without the update), and k_norm_final sums the partials per tensor and
// the tensors in slot order.  Fixed orders throughout and no atomics: the result is bitwise repeatable and
// the same from both kernels.
#include "gsr_common.h"
#include "gsr_internal.h"

namespace gsr {

__device__ inline void adam_elem(float &p, float g, float &m, float &v, float w1, float b2, float omb2,
                                 float eps, float step_size, float bc2s) {
    m = fmaf(w1, g - m, m);
    const float vb = v * b2;
    v = fmaf(omb2, g * g, vb);  // addcmul: self + value * (t1 * t2), contracted
    const float d = sqrtf(v) / bc2s + eps;
    p = fmaf(step_size, m / d, p);
}

// ---- gradient norm (include/gsr.h gsr_grad_norm / gsr_adam_step_norm) ---------------------------
// One thread's four elements: each float converted to double and squared (exact: 48 significant bits),
// added in element order.  The float4 and the scalar branch add in the same order, so a tensor's
// partials do not depend on which branch a caller's alignment selects.
__device__ inline double sumsq4(float x, float y, float z, float w) {
    const double a = (double)x, b = (double)y, c = (double)z, d = (double)w;
    return a * a + b * b + c * c + d * d;
}

__device__ inline double thread_sumsq(const float *__restrict__ grad, long long n, int vec4, long long e0) {
    if (e0 >= n) return 0.0;
    if (vec4 && e0 + 4 <= n) {
        const float4 g = *reinterpret_cast<const float4 *>(grad + e0);
        return sumsq4(g.x, g.y, g.z, g.w);
    }
    double s = 0.0;
    for (long long e = e0; e < e0 + 4 && e < n; ++e) s += (double)grad[e] * (double)grad[e];
    return s;
}

// A block's share of a gradient tensor (kAdamPerBlock elements, `sq` = each thread's four) as ONE partial
// sum of squares: butterfly within the wave, then the four waves' sums through LDS, added in wave order.
// Every thread of the block calls it (threads past the tensor's end with 0).  No atomics: the partial is
// a pure function of the block's elements.
__device__ inline void block_sumsq(double sq, double *__restrict__ out) {
    __shared__ double s_wave[kAdamThreads / 64];
    for (int d = 32; d > 0; d >>= 1) sq += __shfl_xor(sq, d, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sq;
    lds_barrier();
    if (threadIdx.x == 0) *out = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

// kNorm: the update as without it, plus the block's partial sum of squared gradients into
// partials[blockIdx.x] (the instantiation without it is gsr_adam_step's kernel and never reads `partials`).
template <bool kNorm>
__global__ __launch_bounds__(kAdamThreads) void k_adam(AdamTable tab, double *__restrict__ partials) {
    int t = 0;
    while (t + 1 < tab.n && (int)blockIdx.x >= tab.block_start[t + 1]) ++t;
    const AdamTensor &T = tab.t[t];
    const long long e0 = (long long)((int)blockIdx.x - tab.block_start[t]) * kAdamPerBlock + 4ll * threadIdx.x;
    double sq = 0.0;  // threads past the tensor's end contribute 0 and still reach block_sumsq's barrier
    if (e0 < T.n) {
        if (T.vec4 && e0 + 4 <= T.n) {
            float4 p = *reinterpret_cast<const float4 *>(T.param + e0);
            const float4 g = *reinterpret_cast<const float4 *>(T.grad + e0);
            float4 m = *reinterpret_cast<const float4 *>(T.exp_avg + e0);
            float4 v = *reinterpret_cast<const float4 *>(T.exp_avg_sq + e0);
            adam_elem(p.x, g.x, m.x, v.x, tab.w1, tab.b2, tab.omb2, tab.eps, T.step_size, T.bc2_sqrt);
            adam_elem(p.y, g.y, m.y, v.y, tab.w1, tab.b2, tab.omb2, tab.eps, T.step_size, T.bc2_sqrt);
            adam_elem(p.z, g.z, m.z, v.z, tab.w1, tab.b2, tab.omb2, tab.eps, T.step_size, T.bc2_sqrt);
            adam_elem(p.w, g.w, m.w, v.w, tab.w1, tab.b2, tab.omb2, tab.eps, T.step_size, T.bc2_sqrt);
            *reinterpret_cast<float4 *>(T.param + e0) = p;
            *reinterpret_cast<float4 *>(T.exp_avg + e0) = m;
            *reinterpret_cast<float4 *>(T.exp_avg_sq + e0) = v;
            if (kNorm) sq = sumsq4(g.x, g.y, g.z, g.w);
        } else {
            for (long long e = e0; e < e0 + 4 && e < T.n; ++e) {
                float p = T.param[e], m = T.exp_avg[e], v = T.exp_avg_sq[e];
                const float g = T.grad[e];
                adam_elem(p, g, m, v, tab.w1, tab.b2, tab.omb2, tab.eps, T.step_size, T.bc2_sqrt);
                T.param[e] = p; T.exp_avg[e] = m; T.exp_avg_sq[e] = v;
                if (kNorm) sq += (double)g * (double)g;
            }
        }
    }
    if (kNorm) block_sumsq(sq, partials + blockIdx.x);
}

// The reduction alone, over a table of gradient tensors walked like k_adam's.
__global__ __launch_bounds__(kAdamThreads) void k_grad_sumsq(NormTable tab, double *__restrict__ partials) {
    int t = 0;
    while (t + 1 < tab.n && (int)blockIdx.x >= tab.block_start[t + 1]) ++t;
    const NormTensor &T = tab.t[t];
    const long long e0 = (long long)((int)blockIdx.x - tab.block_start[t]) * kAdamPerBlock + 4ll * threadIdx.x;
    block_sumsq(thread_sumsq(T.grad, T.n, T.vec4, e0), partials + blockIdx.x);
}

// One block per table: wave w sums the partials of the table's tensors w, w + 4, ... (lane l takes
// partials l, l + 64, ... in order, then the butterfly), then thread 0 stores each tensor's sum in its
// slot -- as a double for the total, rounded to float32 for the caller.  On the call's last table thread 0
// adds the slots' doubles 0 .. nslots-1 in slot order (every slot was written by this launch or by an
// earlier one on the stream) and writes the total and its square root.
__global__ __launch_bounds__(kAdamThreads) void k_norm_final(NormFinal f, const double *__restrict__ partials,
                                                             double *tensor_sums, double *total,
                                                             float *__restrict__ out_sqnorms,
                                                             float *__restrict__ out_norm) {
    __shared__ double s_sum[kAdamMaxTensors];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int t = wave; t < f.n; t += kAdamThreads / 64) {
        double a = 0.0;
        for (int i = f.part_start[t] + lane; i < f.part_start[t + 1]; i += 64) a += partials[i];
        for (int d = 32; d > 0; d >>= 1) a += __shfl_xor(a, d, 64);
        if (lane == 0) s_sum[t] = a;
    }
    lds_barrier();
    if (threadIdx.x != 0) return;
    for (int t = 0; t < f.n; ++t) {
        tensor_sums[f.slot[t]] = s_sum[t];
        if (out_sqnorms) out_sqnorms[f.slot[t]] = (float)s_sum[t];
    }
    if (!f.last) return;
    __threadfence();  // this thread's slot stores above are read back below
    double sum = 0.0;
    for (int k = 0; k < f.nslots; ++k) sum += tensor_sums[k];
    *total = sum;
    *out_norm = (float)sqrt(sum);
}

int adam_blocks(long long n) { return (int)((n + kAdamPerBlock - 1) / kAdamPerBlock); }

hipError_t launch_adam(const AdamTable &tab, hipStream_t s) {
    const int nb = tab.block_start[tab.n];
    if (nb == 0) return hipSuccess;
    k_adam<false><<<nb, kAdamThreads, 0, s>>>(tab, nullptr);
    return hipGetLastError();
}

hipError_t launch_adam_norm(const AdamTable &tab, double *partials, hipStream_t s) {
    const int nb = tab.block_start[tab.n];
    if (nb == 0) return hipSuccess;
    k_adam<true><<<nb, kAdamThreads, 0, s>>>(tab, partials);
    return hipGetLastError();
}

hipError_t launch_grad_sumsq(const NormTable &tab, double *partials, hipStream_t s) {
    const int nb = tab.block_start[tab.n];
    if (nb == 0) return hipSuccess;
    k_grad_sumsq<<<nb, kAdamThreads, 0, s>>>(tab, partials);
    return hipGetLastError();
}

hipError_t launch_norm_final(const NormFinal &f, const double *partials, double *tensor_sums, double *total,
                             float *out_sqnorms, float *out_norm, hipStream_t s) {
    k_norm_final<<<1, kAdamThreads, 0, s>>>(f, partials, tensor_sums, total, out_sqnorms, out_norm);
    return hipGetLastError();
}

}  // namespace gsr
