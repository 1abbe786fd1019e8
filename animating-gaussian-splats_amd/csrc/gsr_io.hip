// gsr_io.hip -- the pixel side of the data path: decoded 8-bit camera frames
// and segmentation masks of one timestep, uploaded as ONE u8 batch, become the float tensors the
// reference's load_timestep_views builds (shared.py:127-171) per view with ~6 torch ops each:
//   image = torch.tensor(u8 HWC).float().cuda().permute(2, 0, 1) / 255      (shared.py:152-160)
//   mask  = torch.stack((m, zeros_like(m), 1 - m)),  m = float(u8 HW)        (shared.py:131-143,161-168)
// On the GPU torch divides by a Python scalar as a multiply by its float reciprocal
// (x * (1.0f / 255.0f)); the kernel does exactly that, so the result is bitwise the reference's.
//
// k_views_pack: grid.y = frame, one thread per 4 consecutive pixels: three dword loads give the 12
// interleaved RGB bytes (wave: 768 contiguous bytes), one dword gives 4 mask bytes; the planar
// outputs are float4 stores (coalesced per plane).  Byte work, HBM-bound: 4 B read + 24 B written per
// pixel with a mask (12 B without).
//
// The output side (SURVEY.md component 9): a rendered planar float image becomes the interleaved 8-bit
// frame of render_and_export_frame (train.py:534-545),
//   frame = (255 * np.clip(image, 0, 1)).astype(np.uint8).transpose(1, 2, 0)
// k_frames_pack: the same thread shape the other way round: one float4 load per plane (coalesced),
// three dword stores of the 12 interleaved bytes (wave: 768 contiguous bytes); 12 B read + 3 B written
// per pixel.  A byte is clamp to [0, 1], ONE float multiply by 255.0f, truncation; NaN gives 0.
#include "gsr_common.h"
#include "gsr_internal.h"

namespace gsr {

constexpr int kPackThreads = 256;
constexpr int kPackMaxFrames = 65535;  // grid.y limit

__device__ inline float u8f(uint32_t w, int k) { return (float)((w >> (8 * k)) & 0xFFu); }

__global__ __launch_bounds__(kPackThreads) void k_views_pack(int HW, const uint8_t *__restrict__ rgb,
                                                             const uint8_t *__restrict__ seg,
                                                             float *__restrict__ img, float *__restrict__ msk) {
    const int f = blockIdx.y;
    const int p0 = 4 * (blockIdx.x * kPackThreads + threadIdx.x);
    if (p0 >= HW) return;
    const float inv = 1.0f / 255.0f;
    const uint8_t *src = rgb + (size_t)f * HW * 3;
    float *dst = img + (size_t)f * 3 * HW;
    if ((HW & 3) == 0) {  // 4 whole pixels, 4-byte aligned loads, 16-byte aligned stores
        const uint32_t *s32 = reinterpret_cast<const uint32_t *>(src + 3 * (size_t)p0);
        const uint32_t w0 = s32[0], w1 = s32[1], w2 = s32[2];  // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        const float4 R = make_float4(u8f(w0, 0) * inv, u8f(w0, 3) * inv, u8f(w1, 2) * inv, u8f(w2, 1) * inv);
        const float4 G = make_float4(u8f(w0, 1) * inv, u8f(w1, 0) * inv, u8f(w1, 3) * inv, u8f(w2, 2) * inv);
        const float4 B = make_float4(u8f(w0, 2) * inv, u8f(w1, 1) * inv, u8f(w2, 0) * inv, u8f(w2, 3) * inv);
        *reinterpret_cast<float4 *>(dst + p0) = R;
        *reinterpret_cast<float4 *>(dst + HW + p0) = G;
        *reinterpret_cast<float4 *>(dst + 2 * (size_t)HW + p0) = B;
        if (seg) {
            const uint32_t m = *reinterpret_cast<const uint32_t *>(seg + (size_t)f * HW + p0);
            float *md = msk + (size_t)f * 3 * HW;
            const float4 M = make_float4(u8f(m, 0), u8f(m, 1), u8f(m, 2), u8f(m, 3));
            *reinterpret_cast<float4 *>(md + p0) = M;
            *reinterpret_cast<float4 *>(md + HW + p0) = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4 *>(md + 2 * (size_t)HW + p0) =
                make_float4(1.f - M.x, 1.f - M.y, 1.f - M.z, 1.f - M.w);
        }
        return;
    }
    for (int p = p0; p < min(p0 + 4, HW); ++p) {  // ragged frame: byte loads, scalar stores
        dst[p] = (float)src[3 * (size_t)p] * inv;
        dst[HW + p] = (float)src[3 * (size_t)p + 1] * inv;
        dst[2 * (size_t)HW + p] = (float)src[3 * (size_t)p + 2] * inv;
        if (seg) {
            const float m = (float)seg[(size_t)f * HW + p];
            float *md = msk + (size_t)f * 3 * HW;
            md[p] = m;
            md[HW + p] = 0.f;
            md[2 * (size_t)HW + p] = 1.f - m;
        }
    }
}

hipError_t launch_views_pack(int frames, int HW, const uint8_t *rgb, const uint8_t *seg, float *img, float *msk,
                             hipStream_t s) {
    const dim3 grid(div_up(div_up(HW, 4), kPackThreads), frames);
    hipLaunchKernelGGL(k_views_pack, grid, dim3(kPackThreads), 0, s, HW, rgb, seg, img, msk);
    return hipGetLastError();
}

// (255 * clip(x, 0, 1)).astype(uint8): the comparisons send NaN, -0.0 and every negative to +0 and
// everything >= 1 to 1, so the product lies in [0, 255] and the conversion truncates in range.
__device__ inline uint32_t f8u(float x) {
    const float c = x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f;
    return (uint32_t)(c * 255.0f);
}

__global__ __launch_bounds__(kPackThreads) void k_frames_pack(int HW, int vec, const float *__restrict__ img,
                                                              uint8_t *__restrict__ rgb) {
    const int f = blockIdx.y;
    const int p0 = 4 * (blockIdx.x * kPackThreads + threadIdx.x);
    if (p0 >= HW) return;
    const float *src = img + (size_t)f * 3 * HW;
    uint8_t *dst = rgb + (size_t)f * HW * 3;
    if (vec) {  // HW % 4 == 0, img 16-byte and rgb 4-byte aligned: 4 whole pixels
        const float4 R = *reinterpret_cast<const float4 *>(src + p0);
        const float4 G = *reinterpret_cast<const float4 *>(src + HW + p0);
        const float4 B = *reinterpret_cast<const float4 *>(src + 2 * (size_t)HW + p0);
        uint32_t *d32 = reinterpret_cast<uint32_t *>(dst + 3 * (size_t)p0);
        d32[0] = f8u(R.x) | f8u(G.x) << 8 | f8u(B.x) << 16 | f8u(R.y) << 24;  // r0 g0 b0 r1
        d32[1] = f8u(G.y) | f8u(B.y) << 8 | f8u(R.z) << 16 | f8u(G.z) << 24;  // g1 b1 r2 g2
        d32[2] = f8u(B.z) | f8u(R.w) << 8 | f8u(G.w) << 16 | f8u(B.w) << 24;  // b2 r3 g3 b3
        return;
    }
    for (int p = p0; p < min(p0 + 4, HW); ++p) {  // ragged or misaligned frame: scalar loads, byte stores
        dst[3 * (size_t)p] = (uint8_t)f8u(src[p]);
        dst[3 * (size_t)p + 1] = (uint8_t)f8u(src[HW + p]);
        dst[3 * (size_t)p + 2] = (uint8_t)f8u(src[2 * (size_t)HW + p]);
    }
}

hipError_t launch_frames_pack(int frames, int HW, const float *img, uint8_t *rgb, hipStream_t s) {
    const int vec = (HW & 3) == 0 && ((uintptr_t)img & 15) == 0 && ((uintptr_t)rgb & 3) == 0;
    const int gx = div_up(div_up(HW, 4), kPackThreads);
    for (int f0 = 0; f0 < frames; f0 += kPackMaxFrames) {  // grid.y holds 65535 frames: the rest in further launches
        const dim3 grid(gx, min(frames - f0, kPackMaxFrames));
        hipLaunchKernelGGL(k_frames_pack, grid, dim3(kPackThreads), 0, s, HW, vec, img + (size_t)f0 * 3 * HW,
                           rgb + (size_t)f0 * HW * 3);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace gsr
