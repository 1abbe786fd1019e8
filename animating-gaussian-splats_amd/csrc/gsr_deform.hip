// gsr_deform.hip -- the input side of train.py's deformation network.
//
// Every step the reference re-encodes the previous cloud (normalize_and_encode_means_and_rotations,
// train.py:185-204: a dozen torch kernels over (P, C, 2L) temporaries), repeats the progress encoding
// over P rows, concatenates both with the initial encoding into a (P, 192) matrix and multiplies it by
// fc_in (train.py:96-104).  All 192 columns are a function of 14 floats per Gaussian, 14 column ranges
// per cloud and one scalar, so the kernels here rebuild them where they are consumed.
//
// Encoding (PositionalEncoding, train.py:113-127, of columns normalised to [-1, 1]):
//     n = x - lo_c;  xn = (2 n) / hi_c - 1     (fp32, this order, IEEE division; hi_c = max_P n)
//     f_l = 2^l pi (fp32);  s = sin(f_l xn);  feature (2l) C + c = s,  feature (2l + 1) C + c = cos(s)
// -- the cosine of the stored SINE: the reference's second in-place assignment reads the slots the first
// one overwrote.  L = 10 for the 3 mean columns, 4 for the 4 quaternion columns and for the progress.
// 192 columns: [initial means 60 | initial quats 32 | previous means 60 | previous quats 32 | progress 8].
//
//   k_posenc            one lane per (row, argument): the (P, 92) encoding of one (means, quats) pair.
//   k_deform_in_fwd     Y[P, H] = X[P, 192] W^T + b.  A workgroup of 8 waves takes 64 rows: it
//                       normalises their 14 columns into LDS, evaluates each (row, argument) once into a
//                       64 x 184 fp32 LDS tile (row stride 185: conflict-free for the per-row writes and
//                       for the MFMA A reads), then runs v_mfma_f32_32x32x2_f32 over K = 184 in four
//                       chunks of 46 with the matching slice of W staged through LDS (k-major, zero
//                       columns past H).  Wave w owns rows 32 (w & 1) .. + 31 and every fourth 32-column
//                       tile; the 8 progress columns and the bias enter as one constant per column.
//                       blockIdx.y splits H above 128 columns.  K order is fixed: bitwise repeatable.
//                       At most 71 KB of LDS: two workgroups per CU, so one's sine phase overlaps the
//                       other's MFMA phase (128 rows per workgroup, one per CU, measured 13-20 % slower;
//                       GSR_DEFORM_FWD_ROWS / _THREADS are the A/B knobs of `make variant`).
//   k_deform_in_bwd     dW[H, 192] = dY^T X and db = sum_rows dY, X recomputed.  A fixed grid of
//                       persistent workgroups; each walks row tiles of 64 (tile = block, block + grid,
//                       ...), stages X as above plus a ones column (184) whose "gradient" is db, and dY
//                       into LDS, and accumulates v_mfma_f32_16x16x4_f32 products in registers: wave w
//                       owns feature columns 48 (w & 3) .. + 47 and half of the H rows.  One partial
//                       (H x 185) per workgroup goes to the workspace.
//   k_deform_in_reduce  sums the partials in workgroup order (no float atomics) and writes
//                       dW[:, 184 + j] = enc(progress)_j db.
#include "gsr_common.h"
#include "gsr_internal.h"
#include "gsr_mlp.h"

namespace gsr {

namespace {
constexpr int kEncArgs = 46;    // (column, frequency) pairs of one (means, quats) pair: 3 * 10 + 4 * 4
constexpr int kEncCols = 92;    // features of one pair: a sine and a cosine each
constexpr int kXCols = 184;     // per-row features (two pairs); the 8 progress columns are per-call constants
constexpr int kXStride = 185;   // LDS row stride of the feature tile (odd: lanes of a row-per-lane access hit 32 banks)
constexpr int kInCols = 192;    // fc_in's input width
constexpr float kPi = 3.14159265358979323846f;

#ifndef GSR_DEFORM_FWD_ROWS
#define GSR_DEFORM_FWD_ROWS 64
#endif
#ifndef GSR_DEFORM_FWD_THREADS
#define GSR_DEFORM_FWD_THREADS 512
#endif
constexpr int kFwdRows = GSR_DEFORM_FWD_ROWS, kFwdThreads = GSR_DEFORM_FWD_THREADS, kWChunk = 46;
constexpr int kFwdMTiles = kFwdRows / 32;                    // 32-row tiles of a workgroup
constexpr int kFwdNGroups = kFwdThreads / 64 / kFwdMTiles;   // waves that share a row tile split the column tiles
static_assert(kFwdMTiles * 32 == kFwdRows && kFwdNGroups * kFwdMTiles * 64 == kFwdThreads && kFwdNGroups >= 1, "forward tiling");
constexpr int kBwdRows = 64, kBwdThreads = 512;

// argument a in [0, 46) of a pair: its input column (0-2 means, 3-6 quaternion), frequency index and the
// feature slots of its sine and of the cosine of that sine
__device__ inline void enc_slot(int a, int &col, int &l, int &sin_at, int &cos_at) {
    if (a < 30) {
        l = a / 3;
        col = a - 3 * l;
        sin_at = 6 * l + col;
        cos_at = sin_at + 3;
    } else {
        a -= 30;
        l = a >> 2;
        col = 3 + (a & 3);
        sin_at = 60 + 8 * l + (a & 3);
        cos_at = sin_at + 4;
    }
}

__device__ inline float norm_col(float x, float lo, float hi) {
    const float n = x - lo;
    return (2.0f * n) / hi - 1.0f;  // 0 / 0 = NaN for a constant column, as in the reference
}

__device__ inline void enc_pair(float x, int l, float &s, float &c) {
    const float arg = ((float)(1 << l) * kPi) * x;
    s = sinf(arg);
    c = cosf(s);
}

__device__ inline void progress_enc(float progress, float pe[8]) {
#pragma unroll
    for (int l = 0; l < 4; ++l) enc_pair(progress, l, pe[2 * l], pe[2 * l + 1]);
}

struct DeformIn {
    int P, H;
    const float *im, *iq, *ir;  // initial means (P, 3), quaternions (P, 4), ranges lo[7], hi[7]
    const float *pm, *pq, *pr;  // previous
    float progress;
};

// Rows [row0, row0 + ROWS) of X into LDS: xn (14, ROWS) scratch, X (ROWS, kXStride).  Rows past P are
// zeros.  Ends with X written but not yet visible: the caller's next lds_barrier() publishes it.
template <int ROWS, int THREADS>
__device__ inline void stage_x(const DeformIn &a, int row0, float *xn, float *X) {
    const int t = threadIdx.x;
    for (int i = t; i < 14 * ROWS; i += THREADS) {
        const int c14 = i / ROWS, r = i - c14 * ROWS;
        const int set = c14 >= 7, col = c14 - 7 * set;
        const int row = row0 + r;
        float v = 0.f;
        if (row < a.P) {
            const float *m = set ? a.pm : a.im, *q = set ? a.pq : a.iq, *rg = set ? a.pr : a.ir;
            const float x = col < 3 ? m[(size_t)row * 3 + col] : q[(size_t)row * 4 + col - 3];
            v = norm_col(x, rg[col], rg[7 + col]);
        }
        xn[i] = v;
    }
    lds_barrier();
    for (int i = t; i < kEncCols * ROWS; i += THREADS) {
        const int a92 = i / ROWS, r = i - a92 * ROWS;
        const int set = a92 >= kEncArgs;
        int col, l, sa, ca;
        enc_slot(a92 - kEncArgs * set, col, l, sa, ca);
        float s = 0.f, c = 0.f;
        if (row0 + r < a.P) enc_pair(xn[(7 * set + col) * ROWS + r], l, s, c);
        float *xr = X + r * kXStride + kEncCols * set;
        xr[sa] = s;
        xr[ca] = c;
    }
}
}  // namespace

// min / max that keep a NaN once seen, like torch's reductions
__device__ inline float nan_min(float m, float x) { return (x < m || x != x) ? x : m; }
__device__ inline float nan_max(float m, float x) { return (x > m || x != x) ? x : m; }

// Column minima and maxima of rows blockIdx.x * 256 + t, + gridDim.x * 256, ...: partial[block][14]
// (7 minima, 7 maxima).  Minimum and maximum do not depend on the order they are taken in.
__global__ __launch_bounds__(256) void k_posenc_ranges(int P, const float *__restrict__ means,
                                                       const float *__restrict__ quats, float *__restrict__ partial) {
    __shared__ float s_part[4][14];
    float v[14];
#pragma unroll
    for (int c = 0; c < 7; ++c) { v[c] = INFINITY; v[7 + c] = -INFINITY; }
    for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < P; row += (long long)gridDim.x * 256) {
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            const float x = c < 3 ? means[row * 3 + c] : quats[row * 4 + c - 3];
            v[c] = nan_min(v[c], x);
            v[7 + c] = nan_max(v[7 + c], x);
        }
    }
#pragma unroll
    for (int c = 0; c < 14; ++c)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float other = __shfl_xor(v[c], o);
            v[c] = c < 7 ? nan_min(v[c], other) : nan_max(v[c], other);
        }
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int c = 0; c < 14; ++c) s_part[threadIdx.x >> 6][c] = v[c];
    lds_barrier();
    if (threadIdx.x < 14) {
        float r = s_part[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) r = threadIdx.x < 7 ? nan_min(r, s_part[w][threadIdx.x]) : nan_max(r, s_part[w][threadIdx.x]);
        partial[blockIdx.x * 14 + threadIdx.x] = r;
    }
}

// ranges = lo[7], hi[7] with hi = max_P (x - lo) = (max_P x) - lo: the fp32 subtraction is monotone in x
__global__ __launch_bounds__(64) void k_posenc_ranges_final(int nb, const float *__restrict__ partial,
                                                            float *__restrict__ ranges) {
    const int c = threadIdx.x;
    if (c >= 7) return;
    float lo = partial[c], mx = partial[7 + c];
    for (int b = 1; b < nb; ++b) {
        lo = nan_min(lo, partial[b * 14 + c]);
        mx = nan_max(mx, partial[b * 14 + 7 + c]);
    }
    ranges[c] = lo;
    ranges[7 + c] = mx - lo;
}

__global__ __launch_bounds__(256) void k_posenc(int P, const float *__restrict__ means, const float *__restrict__ quats,
                                                const float *__restrict__ ranges, float *__restrict__ out) {
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    if (item >= (long long)P * kEncArgs) return;
    const int row = (int)(item / kEncArgs);
    int col, l, sa, ca;
    enc_slot((int)(item - (long long)row * kEncArgs), col, l, sa, ca);
    const float x = col < 3 ? means[(size_t)row * 3 + col] : quats[(size_t)row * 4 + col - 3];
    float s, c;
    enc_pair(norm_col(x, ranges[col], ranges[7 + col]), l, s, c);
    out[(size_t)row * kEncCols + sa] = s;
    out[(size_t)row * kEncCols + ca] = c;
}

// NT: 32-column tiles of this workgroup's slice of H (blockIdx.y selects the slice)
template <int NT>
__global__ __launch_bounds__(kFwdThreads) void k_deform_in_fwd(DeformIn a, const float *__restrict__ W,
                                                               const float *__restrict__ bias, float *__restrict__ Y) {
    extern __shared__ __attribute__((aligned(16))) float s_lds[];
    constexpr int WS = NT * 32 + 1;  // k-major W slice: odd stride, the transposing store is conflict-free
    float *X = s_lds;                         // kFwdRows * kXStride
    float *Ws = s_lds + kFwdRows * kXStride;  // max(14 * kFwdRows, kWChunk * WS): xn first, then W slices
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int mt = w % kFwdMTiles, nh = w / kFwdMTiles;
    const int row0 = blockIdx.x * kFwdRows, h0 = blockIdx.y * (NT * 32);
    constexpr int NW = (NT + kFwdNGroups - 1) / kFwdNGroups;
    f32x16 acc[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    stage_x<kFwdRows, kFwdThreads>(a, row0, Ws, X);
    const float *xa = X + (mt * 32 + (lane & 31)) * kXStride + (lane >> 5);
    const float *wb = Ws + (lane >> 5) * WS + (lane & 31);
    for (int kc = 0; kc < kXCols; kc += kWChunk) {
        lds_barrier();  // X is visible and xn consumed / the previous W slice has been consumed
        for (int i = t; i < NT * 32 * kWChunk; i += kFwdThreads) {
            const int col = i / kWChunk, k = i - col * kWChunk;
            const int h = h0 + col;
            Ws[k * WS + col] = h < a.H ? W[(size_t)h * kInCols + kc + k] : 0.f;
        }
        lds_barrier();
#pragma unroll 23
        for (int k = 0; k < kWChunk; k += 2) {
            const float av = xa[kc + k];
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const int nt = nh + kFwdNGroups * j;
                if (nt < NT) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, wb[k * WS + nt * 32], acc[j], 0, 0, 0);
            }
        }
    }

    float pe[8];
    progress_enc(a.progress, pe);
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const int nt = nh + kFwdNGroups * j;
        const int h = h0 + nt * 32 + (lane & 31);
        if (nt >= NT || h >= a.H) continue;
        float c = bias[h];
#pragma unroll
        for (int q = 0; q < 8; ++q) c = fmaf(W[(size_t)h * kInCols + kXCols + q], pe[q], c);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row0 + mt * 32 + acc_row(r, lane);
            if (row < a.P) Y[(size_t)row * a.H + h] = acc[j][r] + c;
        }
    }
}

// MT: 32-row tiles of this workgroup's slice of H (= 2 MT 16-row MFMA tiles, MT per wave half)
template <int MT>
__global__ __launch_bounds__(kBwdThreads) void k_deform_in_bwd(DeformIn a, int tiles, const float *__restrict__ dY,
                                                               float *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float s_lds[];
    constexpr int HC = MT * 32;
    constexpr int SD = HC + 16;  // dY tile stride = 16 mod 32: the 2 rows x 16 columns a 32-lane group reads hit 32 banks
    float *X = s_lds;                          // kBwdRows * kXStride
    float *xn = X + kBwdRows * kXStride;       // 14 * kBwdRows
    float *dYs = xn + 14 * kBwdRows;           // kBwdRows * SD
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int ns = w & 3, mh = w >> 2;
    const int h0 = blockIdx.y * HC;
    f32x4 acc[MT][3];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int n = 0; n < 3; ++n) acc[i][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int row0 = tile * kBwdRows;
        lds_barrier();  // the previous tile has been consumed
        stage_x<kBwdRows, kBwdThreads>(a, row0, xn, X);
        if (t < kBwdRows) X[t * kXStride + kXCols] = row0 + t < a.P ? 1.f : 0.f;  // the column whose gradient is db
        for (int i = t; i < kBwdRows * HC; i += kBwdThreads) {
            const int r = i / HC, c = i - r * HC;
            const int row = row0 + r, h = h0 + c;
            dYs[r * SD + c] = row < a.P && h < a.H ? dY[(size_t)row * a.H + h] : 0.f;
        }
        lds_barrier();
#pragma unroll 4
        for (int k = 0; k < kBwdRows; k += 4) {
            const int r = k + (lane >> 4);
            float b[3];
#pragma unroll
            for (int n = 0; n < 3; ++n) {
                const int f = ns * 48 + n * 16 + (lane & 15);
                b[n] = f <= kXCols ? X[r * kXStride + f] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const float av = dYs[r * SD + (mh * MT + i) * 16 + (lane & 15)];
#pragma unroll
                for (int n = 0; n < 3; ++n) acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[n], acc[i][n], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int n = 0; n < 3; ++n) {
            const int f = ns * 48 + n * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int h = h0 + (mh * MT + i) * 16 + (lane >> 4) * 4 + r;
                if (h < a.H && f <= kXCols) partial[((size_t)blockIdx.x * a.H + h) * kXStride + f] = acc[i][n][r];
            }
        }
}

__global__ __launch_bounds__(256) void k_deform_in_reduce(int H, int nb, const float *__restrict__ partial, float progress,
                                                          float *__restrict__ dW, float *__restrict__ db) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= H * kInCols) return;
    const int h = idx / kInCols, f = idx - h * kInCols;
    const float *p = partial + (size_t)h * kXStride + (f < kXCols ? f : kXCols);
    float s = 0.f;
    for (int b = 0; b < nb; ++b) s += p[(size_t)b * H * kXStride];
    if (f >= kXCols) {
        if (f == kXCols && db) db[h] = s;
        float pe[8];
        progress_enc(progress, pe);
        s = pe[f - kXCols] * s;
    }
    if (dW) dW[idx] = s;
}

// ---- host launchers --------------------------------------------------------------------------
namespace {
DeformIn deform_in(int P, int H, const float *im, const float *iq, const float *ir, const float *pm, const float *pq,
                   const float *pr, float progress) {
    DeformIn a;
    a.P = P; a.H = H;
    a.im = im; a.iq = iq; a.ir = ir;
    a.pm = pm; a.pq = pq; a.pr = pr;
    a.progress = progress;
    return a;
}

// H split into ny slices of nt 32-wide tiles each (nt <= 4: what the accumulators hold)
void split_h(int H, int &ny, int &nt) {
    ny = div_up(H, 128);
    nt = div_up(div_up(H, 32), ny);
}

int deform_in_blocks(int P, int max_blocks) { return persistent_blocks(P, kBwdRows, max_blocks, kDeformAutoBlocks); }
}  // namespace

hipError_t launch_posenc_ranges(int P, const float *means, const float *quats, float *partial, float *ranges,
                                hipStream_t s) {
    const int nb = div_up(P, 256) < kPosencRangeBlocks ? div_up(P, 256) : kPosencRangeBlocks;
    k_posenc_ranges<<<nb, 256, 0, s>>>(P, means, quats, partial);
    k_posenc_ranges_final<<<1, 64, 0, s>>>(nb, partial, ranges);
    return hipGetLastError();
}

hipError_t launch_posenc(int P, const float *means, const float *quats, const float *ranges, float *out, hipStream_t s) {
    const long long items = (long long)P * kEncArgs;
    k_posenc<<<(unsigned)((items + 255) / 256), 256, 0, s>>>(P, means, quats, ranges, out);
    return hipGetLastError();
}

hipError_t launch_deform_in_fwd(int P, int H, const float *im, const float *iq, const float *ir, const float *pm,
                                const float *pq, const float *pr, float progress, const float *W, const float *bias,
                                float *Y, hipStream_t s) {
    const DeformIn a = deform_in(P, H, im, iq, ir, pm, pq, pr, progress);
    int ny, nt;
    split_h(H, ny, nt);
    return dispatch_tiles(nt, [&](auto n) {
        constexpr int NT = decltype(n)::value, WS = NT * 32 + 1;
        constexpr int second = 14 * kFwdRows > kWChunk * WS ? 14 * kFwdRows : kWChunk * WS;
        return launch_lds(k_deform_in_fwd<NT>, dim3(div_up(P, kFwdRows), ny), kFwdThreads,
                          sizeof(float) * (kFwdRows * kXStride + second), s, a, W, bias, Y);
    });
}

size_t deform_in_partial_floats(int P, int H, int max_blocks) {
    return (size_t)deform_in_blocks(P, max_blocks) * (size_t)H * kXStride;
}

hipError_t launch_deform_in_bwd(int P, int H, const float *im, const float *iq, const float *ir, const float *pm,
                                const float *pq, const float *pr, float progress, const float *dY, float *partial,
                                int max_blocks, float *dW, float *db, hipStream_t s) {
    const DeformIn a = deform_in(P, H, im, iq, ir, pm, pq, pr, progress);
    const int nb = deform_in_blocks(P, max_blocks), tiles = div_up(P, kBwdRows);
    int ny, mt;
    split_h(H, ny, mt);
    hipError_t e = dispatch_tiles(mt, [&](auto m) {
        constexpr int MT = decltype(m)::value;
        return launch_lds(k_deform_in_bwd<MT>, dim3(nb, ny), kBwdThreads,
                          sizeof(float) * (kBwdRows * kXStride + 14 * kBwdRows + kBwdRows * (MT * 32 + 16)), s, a, tiles,
                          dY, partial);
    });
    if (e != hipSuccess) return e;
    k_deform_in_reduce<<<div_up(H * kInCols, 256), 256, 0, s>>>(H, nb, partial, progress, dW, db);
    return hipGetLastError();
}

}  // namespace gsr
