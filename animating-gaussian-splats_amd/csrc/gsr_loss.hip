// gsr_loss.hip -- fused L1 + SSIM image loss (forward and backward) for the render call sites.
//
// Replaces, at train.py:354-364 / densify.py:127-129,149-151, the pair
//     torch.nn.functional.l1_loss(img1, img2)   and   calc_ssim(img1, img2)   (external.py:68-110)
// where calc_ssim runs five grouped 11x11 conv2d (window = outer product of a normalised 1-D
// Gaussian, sigma 1.5, zero padding 5) and a dozen elementwise kernels, each with its own autograd
// node.  Here the window is applied separably out of LDS and everything else is fused:
//
//   k_ssim_fwd   one wave64 per 64-column x 32-row strip of one image plane, 4 independent waves per
//                block: rows stream through wave-private LDS (11-tap horizontal pass of
//                (x, y, x^2, y^2, xy)) into an 11-row register ring (vertical pass), then per pixel
//                the SSIM value, three derivative maps dS/dmu1, dS/d<x^2>, dS/d<xy> + 2 dS/d<x^2> (stored
//                for the backward) and |x - y|.  Per-wave partial sums, no atomics.
//   k_ssim_sum   one block: fixed-order (double) sum of the block partials -> (mean |x-y|, mean S).
//   k_ssim_eval  the forward-only form for scoring V image pairs (train.py:598-613): the same strip body
//                (ssim_fwd_strip<false>) without the derivative maps, plus sum (x-y)^2; k_scores_sum (one
//                block per view) and k_scores_mean turn the partials into (l1, ssim, mse, image_loss) per
//                view and the mean image_loss.  8 B per pixel instead of 20.
//   k_ssim_bwd   same strips: blur the three stored derivative maps (the window is symmetric, so the
//                adjoint of the zero-padded correlation is the same correlation) and combine
//                dL/dx = gS/N (blur(dS/dmu1) + 2 x blur(dS/d<x^2>) + y blur(dS/d<xy>)) + gL1/N sign(x-y)
//                with the upstream gradients gL1, gS read from device memory (no host sync).
//                dS/d<x^2> = -S / D and dS/d<xy> = 2 A / (C D) are each ~ 1 / c2 = 1111 on a flat region and
//                cancel to ~ 0 where the render matches its target, so their fp32 roundings (7e-5 each)
//                would be the whole result there.  The third map therefore holds the sum
//                dS/d<xy> + 2 dS/d<x^2> = 2 (A - S C) / (C D), cancelled before it is rounded, and the
//                backward combines 2 (x - y) blur(dS/d<x^2>) + y blur(third map): the same gradient.
//
// Algorithmic HBM bytes: forward 2 reads + 3 writes per pixel (20 B), backward 3 + 2 reads + 1
// write (24 B); the 10 halo rows per 32-row strip and the 10 halo columns re-read through L2.
#include "gsr_common.h"
#include "gsr_internal.h"

namespace gsr {

constexpr int kSsR = 5;                 // window radius (window_size 11)
constexpr int kSsTaps = 2 * kSsR + 1;
constexpr int kSsRH = 32;               // output rows per wave strip (64 columns = one per lane)
constexpr int kSsWaves = 4;             // independent waves per 256-thread block
constexpr int kSsRowBuf = 80;           // staged row: 64 + 2 * 5 halo columns (+ pad)
constexpr float kSsC1 = 0.01f * 0.01f, kSsC2 = 0.03f * 0.03f;
constexpr int kSsEvalViews = 32;        // image pairs per k_ssim_eval launch (their pointers are kernel arguments)

// Strip of wave `gw`: plane, first column x0, first output row y0.
struct SsStrip { int plane, x0, y0; };
__device__ inline SsStrip ss_strip(int gw, int sx, int sy) {
    SsStrip t;
    t.plane = gw / (sx * sy);
    const int r = gw - t.plane * sx * sy;
    t.y0 = (r / sx) * kSsRH;
    t.x0 = (r % sx) * 64;
    return t;
}

// Stage input row `gy` of one plane, columns [x0 - 5, x0 + 69), into the wave's LDS row (zero outside
// the image: conv2d zero padding).  Lane l holds column x0 - 5 + l, lanes 0..9 also x0 + 59 + l.
__device__ inline void ss_load_row(const float *__restrict__ src, int H, int W, int x0, int gy, int lane,
                                   float &lo, float &hi) {
    const bool row_ok = gy >= 0 && gy < H;
    const int ca = x0 - kSsR + lane, cb = x0 + 64 - kSsR + lane;
    lo = (row_ok && ca >= 0 && ca < W) ? src[(size_t)gy * W + ca] : 0.f;
    hi = (row_ok && lane < 2 * kSsR && cb < W) ? src[(size_t)gy * W + cb] : 0.f;
}

// ------------------------------------------------------------------------------------------
// Forward.  Each wave streams down a 64-column strip: per input row it stages the row (+ halo) of
// both images in wave-private LDS, forms the 5 horizontal window sums of (x, y, x^2, y^2, xy) for
// its lane's column, and keeps the last 11 rows of those sums in a register ring (slot = row mod
// 11, resolved at compile time by unrolling 2 x 11 rows; the next two rows' loads are in flight); once 11 rows are in, the vertical window gives
// mu1, mu2, <x^2>, <y^2>, <xy> of the output row 5 above.  No block barriers.
//
// One strip's body, shared by k_ssim_fwd and k_ssim_eval.  SAVE: store the three derivative maps (the
// training forward).  Without it (the scoring path, nothing differentiates) no map is written and
// (x - y)^2 is summed as well; lsum and ssum take the same operations in the same order either way, so
// they are bitwise the same.  The sums come back reduced over the wave.
template <bool SAVE>
__device__ __forceinline__ void ssim_fwd_strip(int planes, int H, int W, const SsStrip st, int lane,
                                               float *ra, float *rb, const float *__restrict__ img1,
                                               const float *__restrict__ img2, const SsimWindow &w,
                                               float *__restrict__ maps, size_t plane_stride, float &lsum,
                                               float &ssum, float &qsum) {
    const float *a = img1 + st.plane * plane_stride, *b = img2 + st.plane * plane_stride;
    [[maybe_unused]] float *m0 = SAVE ? maps + st.plane * plane_stride : nullptr;
    [[maybe_unused]] const size_t map_stride = plane_stride * planes;  // the three maps are [3][planes][H][W]
    const int gx = st.x0 + lane;
    const int nin = min(kSsRH, H - st.y0) + 2 * kSsR;  // input rows this strip streams
    float h[kSsTaps][5];   // ring of horizontal sums
    ssum = 0.f; lsum = 0.f; qsum = 0.f;
    // input rows prefetched 2 ahead into statically named registers (unroll by 2 x 11)
    float pf[2][4];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        ss_load_row(a, H, W, st.x0, st.y0 - kSsR + d, lane, pf[d][0], pf[d][1]);
        ss_load_row(b, H, W, st.x0, st.y0 - kSsR + d, lane, pf[d][2], pf[d][3]);
    }
    for (int base = 0; base < nin; base += 2 * kSsTaps) {
#pragma unroll
        for (int k = 0; k < 2 * kSsTaps; ++k) {
            const int i = base + k;  // input row index within the strip (wave-uniform)
            if (i >= nin) continue;
            const int slot = k % kSsTaps, d = k & 1;
            ra[lane] = pf[d][0]; rb[lane] = pf[d][2];
            if (lane < 16) { ra[64 + lane] = pf[d][1]; rb[64 + lane] = pf[d][3]; }
            if (i + 2 < nin) {
                ss_load_row(a, H, W, st.x0, st.y0 - kSsR + i + 2, lane, pf[d][0], pf[d][1]);
                ss_load_row(b, H, W, st.x0, st.y0 - kSsR + i + 2, lane, pf[d][2], pf[d][3]);
            }
            wave_lds_sync();
#pragma unroll
            for (int q = 0; q < 5; ++q) h[slot][q] = 0.f;
#pragma unroll
            for (int t = 0; t < kSsTaps; ++t) {
                const float x = ra[lane + t], y = rb[lane + t];
                // the centre pixel of input row i lies in output row i - 5 (L1 term)
                if (t == kSsR && i >= kSsR && i < nin - kSsR && gx < W) {
                    lsum += fabsf(x - y);
                    if constexpr (!SAVE) qsum += (x - y) * (x - y);
                }
                h[slot][0] = fmaf(w.w[t], x, h[slot][0]);
                h[slot][1] = fmaf(w.w[t], y, h[slot][1]);
                h[slot][2] = fmaf(w.w[t], x * x, h[slot][2]);
                h[slot][3] = fmaf(w.w[t], y * y, h[slot][3]);
                h[slot][4] = fmaf(w.w[t], x * y, h[slot][4]);
            }
            wave_lds_sync();  // the row buffer is rewritten next iteration
            if (i >= 2 * kSsR) {  // output row o = i - 10: window rows i - 10 .. i
                float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < kSsTaps; ++t) {
                    const int rs = (k + 1 + t) % kSsTaps;  // ring slot of row i - 10 + t
#pragma unroll
                    for (int q = 0; q < 5; ++q) acc[q] = fmaf(w.w[t], h[rs][q], acc[q]);
                }
                [[maybe_unused]] const int gy = st.y0 + i - 2 * kSsR;
                if (gx < W) {
                    const float mu1 = acc[0], mu2 = acc[1];
                    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
                    const float sigma1_sq = acc[2] - mu1_sq, sigma2_sq = acc[3] - mu2_sq, sigma12 = acc[4] - mu1_mu2;
                    const float A = 2.f * mu1_mu2 + kSsC1, B = 2.f * sigma12 + kSsC2;
                    const float C = mu1_sq + mu2_sq + kSsC1, D = sigma1_sq + sigma2_sq + kSsC2;
                    const float inv = 1.f / (C * D);
                    const float S = (A * B) * inv;
                    ssum += S;
                    if constexpr (SAVE) {
                        // S = A B / (C D): dS/dmu1 = (2 mu2 (B - A) - 2 mu1 S (D - C)) / (C D),
                        // dS/d<x^2> = -S / D, dS/d<xy> = 2 A / (C D); the third map is dS/d<xy> + 2 dS/d<x^2>
                        const size_t p = (size_t)gy * W + gx;
                        // S multiplies one rounded product, not 2 mu1 first: where mu1 = mu2, A = C and B = D the two
                        // terms are then the same float and their difference is (1 - S) of it, not a rounding of 2 mu1 S
                        m0[p] = 2.f * fmaf(-S, mu1 * (D - C), mu2 * (B - A)) * inv;
                        m0[map_stride + p] = -S / D;
                        m0[2 * map_stride + p] = 2.f * fmaf(-S, C, A) * inv;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        ssum += __shfl_xor(ssum, d, 64);
        lsum += __shfl_xor(lsum, d, 64);
        if constexpr (!SAVE) qsum += __shfl_xor(qsum, d, 64);
    }
}

__global__ __launch_bounds__(256) void k_ssim_fwd(int planes, int H, int W, int sx, int sy,
                                                  const float *__restrict__ img1, const float *__restrict__ img2,
                                                  SsimWindow w, float *__restrict__ maps, size_t plane_stride,
                                                  float2 *__restrict__ partial) {
    __shared__ float s_row[kSsWaves][2][kSsRowBuf];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gw = blockIdx.x * kSsWaves + wv;
    if (gw >= planes * sx * sy) return;
    float lsum, ssum, qsum;
    ssim_fwd_strip<true>(planes, H, W, ss_strip(gw, sx, sy), lane, s_row[wv][0], s_row[wv][1], img1, img2, w, maps,
                         plane_stride, lsum, ssum, qsum);
    if (lane == 0) partial[gw] = make_float2(lsum, ssum);
}

// Scoring (forward only) of up to kSsEvalViews image pairs of one size: the same strips over view blockIdx.y,
// whose two image pointers come by value in the kernel arguments (every render is a tensor of its own: no
// stacked copy, no pointer upload).  partial: [view of this launch][wave][3] = (sum |x-y|, sum S, sum (x-y)^2).
struct SsViewPtrs { const float *a[kSsEvalViews], *b[kSsEvalViews]; };
__global__ __launch_bounds__(256) void k_ssim_eval(int planes, int H, int W, int sx, int sy, SsViewPtrs vp,
                                                   SsimWindow w, size_t plane_stride, float *__restrict__ partial) {
    __shared__ float s_row[kSsWaves][2][kSsRowBuf];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gw = blockIdx.x * kSsWaves + wv, nw = planes * sx * sy;
    if (gw >= nw) return;
    const int v = blockIdx.y;
    float lsum, ssum, qsum;
    ssim_fwd_strip<false>(planes, H, W, ss_strip(gw, sx, sy), lane, s_row[wv][0], s_row[wv][1], vp.a[v], vp.b[v], w,
                          nullptr, plane_stride, lsum, ssum, qsum);
    if (lane == 0) {
        float *p = partial + ((size_t)v * nw + gw) * 3;
        p[0] = lsum; p[1] = ssum; p[2] = qsum;
    }
}

// One block per view, the sums of k_ssim_sum (same order, so l1 and ssim are bitwise its results) and the
// squared error: out_scores[view] = (l1, ssim, mse, 0.8 l1 + 0.2 (1 - ssim)), the last in float32 in the
// expression order of train.py:391-392.
__global__ __launch_bounds__(256) void k_scores_sum(int nw, const float *__restrict__ partial, double inv_n,
                                                    float *__restrict__ out_scores) {
    __shared__ double s_l[256], s_s[256], s_q[256];
    const float *p = partial + (size_t)blockIdx.x * nw * 3;
    double l = 0, s = 0, q = 0;
    for (int i = threadIdx.x; i < nw; i += 256) { l += p[3 * (size_t)i]; s += p[3 * (size_t)i + 1]; q += p[3 * (size_t)i + 2]; }
    s_l[threadIdx.x] = l; s_s[threadIdx.x] = s; s_q[threadIdx.x] = q;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            s_l[threadIdx.x] += s_l[threadIdx.x + d]; s_s[threadIdx.x] += s_s[threadIdx.x + d];
            s_q[threadIdx.x] += s_q[threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float l1 = (float)(s_l[0] * inv_n), ssim = (float)(s_s[0] * inv_n);
        float *o = out_scores + 4 * (size_t)blockIdx.x;
        o[0] = l1; o[1] = ssim; o[2] = (float)(s_q[0] * inv_n);
        o[3] = 0.8f * l1 + 0.2f * (1.0f - ssim);
    }
}

// One block: the mean of the views' image_loss, summed in double in a fixed order.
__global__ __launch_bounds__(256) void k_scores_mean(int views, const float *__restrict__ scores,
                                                     float *__restrict__ out_mean) {
    __shared__ double s_m[256];
    double m = 0;
    for (int v = threadIdx.x; v < views; v += 256) m += scores[4 * (size_t)v + 3];
    s_m[threadIdx.x] = m;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) s_m[threadIdx.x] += s_m[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out_mean = (float)(s_m[0] / (double)views);
}

// One block: *out_l1 = mean |x - y|, *out_ssim = mean S over n pixels (double accumulation, fixed order).
__global__ __launch_bounds__(256) void k_ssim_sum(int nb, const float2 *__restrict__ partial, double inv_n,
                                                  float *__restrict__ out_l1, float *__restrict__ out_ssim) {
    __shared__ double s_l[256], s_s[256];
    double l = 0, s = 0;
    for (int i = threadIdx.x; i < nb; i += 256) { l += partial[i].x; s += partial[i].y; }
    s_l[threadIdx.x] = l; s_s[threadIdx.x] = s;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) { s_l[threadIdx.x] += s_l[threadIdx.x + d]; s_s[threadIdx.x] += s_s[threadIdx.x + d]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { *out_l1 = (float)(s_l[0] * inv_n); *out_ssim = (float)(s_s[0] * inv_n); }
}

// ------------------------------------------------------------------------------------------
// Backward, same strips: stream the three derivative maps through the horizontal + register-ring
// vertical window and combine at each output pixel.
__global__ __launch_bounds__(256) void k_ssim_bwd(int planes, int H, int W, int sx, int sy,
                                                  const float *__restrict__ img1, const float *__restrict__ img2,
                                                  SsimWindow w, const float *__restrict__ maps, size_t plane_stride,
                                                  const float *__restrict__ g_l1, const float *__restrict__ g_ssim,
                                                  float inv_n, float *__restrict__ dimg1) {
    __shared__ float s_row[kSsWaves][3][kSsRowBuf];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gw = blockIdx.x * kSsWaves + wv;
    if (gw >= planes * sx * sy) return;
    const SsStrip st = ss_strip(gw, sx, sy);
    const size_t map_stride = plane_stride * planes;
    const float gs = g_ssim ? g_ssim[0] * inv_n : 0.f;
    const float gl = g_l1 ? g_l1[0] * inv_n : 0.f;
    const float *a = img1 + st.plane * plane_stride, *b = img2 + st.plane * plane_stride;
    const float *mp = maps + st.plane * plane_stride;
    float *dst = dimg1 + st.plane * plane_stride;
    const int gx = st.x0 + lane;
    const int nout = min(kSsRH, H - st.y0);
    if (!g_ssim) {  // L1 term only
        if (gx < W)
            for (int o = 0; o < nout; ++o) {
                const size_t p = (size_t)(st.y0 + o) * W + gx;
                const float d = a[p] - b[p];
                dst[p] = gl * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
            }
        return;
    }
    const int nin = nout + 2 * kSsR;
    float *r0 = s_row[wv][0], *r1 = s_row[wv][1], *r2 = s_row[wv][2];
    float h[kSsTaps][3];
    float pf[2][3][2];  // map rows prefetched 2 ahead (lo, hi halo)
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            ss_load_row(mp + j * map_stride, H, W, st.x0, st.y0 - kSsR + d, lane, pf[d][j][0], pf[d][j][1]);
    for (int base = 0; base < nin; base += 2 * kSsTaps) {
#pragma unroll
        for (int k = 0; k < 2 * kSsTaps; ++k) {
            const int i = base + k;
            if (i >= nin) continue;
            const int slot = k % kSsTaps, d = k & 1;
            r0[lane] = pf[d][0][0]; r1[lane] = pf[d][1][0]; r2[lane] = pf[d][2][0];
            if (lane < 16) { r0[64 + lane] = pf[d][0][1]; r1[64 + lane] = pf[d][1][1]; r2[64 + lane] = pf[d][2][1]; }
            if (i + 2 < nin) {
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    ss_load_row(mp + j * map_stride, H, W, st.x0, st.y0 - kSsR + i + 2, lane, pf[d][j][0], pf[d][j][1]);
            }
            wave_lds_sync();
#pragma unroll
            for (int q = 0; q < 3; ++q) h[slot][q] = 0.f;
#pragma unroll
            for (int t = 0; t < kSsTaps; ++t) {
                h[slot][0] = fmaf(w.w[t], r0[lane + t], h[slot][0]);
                h[slot][1] = fmaf(w.w[t], r1[lane + t], h[slot][1]);
                h[slot][2] = fmaf(w.w[t], r2[lane + t], h[slot][2]);
            }
            wave_lds_sync();
            if (i >= 2 * kSsR) {
                float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < kSsTaps; ++t) {
                    const int rs = (k + 1 + t) % kSsTaps;
#pragma unroll
                    for (int q = 0; q < 3; ++q) acc[q] = fmaf(w.w[t], h[rs][q], acc[q]);
                }
                if (gx < W) {
                    const size_t p = (size_t)(st.y0 + i - 2 * kSsR) * W + gx;
                    const float x = a[p], y = b[p];
                    const float dd = x - y;
                    const float sgn = dd > 0.f ? 1.f : (dd < 0.f ? -1.f : 0.f);
                    dst[p] = gs * (acc[0] + 2.f * dd * acc[1] + y * acc[2]) + gl * sgn;
                }
            }
        }
    }
}

// ==========================================================================================
size_t ssim_partials(int planes, int H, int W) {
    return (size_t)planes * div_up(W, 64) * div_up(H, kSsRH);
}

hipError_t launch_ssim_fwd(int planes, int H, int W, const float *img1, const float *img2, const SsimWindow &w,
                           float *maps, float2 *partial, float *out_l1, float *out_ssim, hipStream_t s) {
    const int sx = div_up(W, 64), sy = div_up(H, kSsRH);
    const int nw = planes * sx * sy;
    const size_t ps = (size_t)H * W;
    k_ssim_fwd<<<div_up(nw, kSsWaves), 64 * kSsWaves, 0, s>>>(planes, H, W, sx, sy, img1, img2, w, maps, ps, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_ssim_sum<<<1, 256, 0, s>>>(nw, partial, 1.0 / ((double)planes * ps), out_l1, out_ssim);
    return hipGetLastError();
}

hipError_t launch_image_scores(int views, int planes, int H, int W, const float *const *img1,
                               const float *const *img2, const SsimWindow &w, float *partial, float *out_scores,
                               float *out_mean, hipStream_t s) {
    const int sx = div_up(W, 64), sy = div_up(H, kSsRH);
    const int nw = planes * sx * sy;
    const size_t ps = (size_t)H * W;
    for (int v0 = 0; v0 < views; v0 += kSsEvalViews) {  // kSsEvalViews pointer pairs per launch
        const int n = min(kSsEvalViews, views - v0);
        SsViewPtrs vp;
        for (int k = 0; k < kSsEvalViews; ++k) {
            vp.a[k] = k < n ? img1[v0 + k] : nullptr;
            vp.b[k] = k < n ? img2[v0 + k] : nullptr;
        }
        k_ssim_eval<<<dim3(div_up(nw, kSsWaves), n), 64 * kSsWaves, 0, s>>>(planes, H, W, sx, sy, vp, w, ps,
                                                                            partial + (size_t)v0 * nw * 3);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    k_scores_sum<<<views, 256, 0, s>>>(nw, partial, 1.0 / ((double)planes * ps), out_scores);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !out_mean) return e;
    k_scores_mean<<<1, 256, 0, s>>>(views, out_scores, out_mean);
    return hipGetLastError();
}

hipError_t launch_ssim_bwd(int planes, int H, int W, const float *img1, const float *img2, const SsimWindow &w,
                           const float *maps, const float *g_l1, const float *g_ssim, float *dimg1,
                           hipStream_t s) {
    const int sx = div_up(W, 64), sy = div_up(H, kSsRH);
    const int nw = planes * sx * sy;
    const size_t ps = (size_t)H * W;
    k_ssim_bwd<<<div_up(nw, kSsWaves), 64 * kSsWaves, 0, s>>>(planes, H, W, sx, sy, img1, img2, w, maps, ps,
                                                              g_l1, g_ssim, (float)(1.0 / ((double)planes * ps)), dimg1);
    return hipGetLastError();
}

}  // namespace gsr
