// gsr_head.hip -- the output side of train.py's deformation network (train.py:106-108):
//     out = (x W^T + b) + [initial means | initial quaternions]
// with W (7, H) and b (7) of nn.Linear(H, 7).  The (P, 7) concatenation is never written: the two arrays
// are read where they are added.  With 7 output columns there are 7 fmaf per loaded float: a streaming
// problem on the vector ALU, not an MFMA one.  All fp32, no float atomics, every summation order fixed.
//
// Both kernels read and write the (P, H) tensors straight from and to global memory, 16 bytes per lane where
// H % 4 == 0, consecutive lanes consecutive addresses: a thread owns 4 consecutive columns of some rows.
//
//   k_head_fwd<VEC, ONE>  16 lanes share a row; a workgroup of 4 waves has 16 row slots and takes 64-row tiles
//                       (4 consecutive ones per workgroup), 4 rows per slot.  Lane l owns columns 64 c + 4 l ..
//                       + 3 of every 64-column chunk c: per row and output column one fmaf chain over its
//                       columns in ascending order.  ONE (H <= 64): its 28 weights stay in registers; otherwise
//                       each chunk's come from a zero-padded LDS copy of W, read once for the 4 rows.  The 16
//                       lanes' sums are added by four DPP stages inside their row of lanes (lane ^ 1, lane ^ 2,
//                       then the mirrored 4 and the mirrored 8: every lane ends with the same tree), then lane
//                       j < 7 adds bias[j], then the initial value, and stores column j.  No LDS traffic for x,
//                       no barrier after the weights are staged.
//   k_head_bwd<VEC>     a fixed grid of persistent workgroups; each walks row tiles of 64 (tile = block,
//                       block + grid, ...).  A thread owns 4 consecutive columns (its 28 weights in registers)
//                       and every RP-th row of a tile (RP = 256 / ceil(H / 4) rows are in flight at once).
//                       The tile's 64 x 7 upstream gradients are staged in LDS (two buffers: one barrier per
//                       tile).  dL_dx = one 7-term fmaf chain per element; dL_dweight's 28 and dL_dbias' 7
//                       running sums stay in registers over all tiles, are added over the RP row slots in slot
//                       order through LDS, and leave as one (7 H + 7) partial per workgroup.  Outputs that are
//                       not wanted are neither computed nor stored, and x is read only for dL_dweight.
//   k_head_reduce       sums the partials in workgroup order (double; one wave per element: lanes take
//                       consecutive chunks of workgroups, then neighbours merge) into dL_dweight and dL_dbias.
//                       A wave, not a thread, per element: one thread walking 1024 partials is a serial chain
//                       of loads that takes longer than k_head_bwd itself.
#include "gsr_common.h"
#include "gsr_internal.h"
#include "gsr_mlp.h"

namespace gsr {

namespace {
constexpr int kRows = 64, kThreads = 256, kChunk = 64;
constexpr int kSlots = kThreads / 16;       // the forward's row slots
constexpr int kPasses = kRows / kSlots;     // rows of a tile per slot
constexpr int kFwdTiles = 4;                // consecutive row tiles of a forward workgroup
constexpr int kTileOut = kRows * 7;         // upstream gradients of a row tile

// sum over the 16 lanes of a DPP row, the same tree in every lane
__device__ inline float row16_sum(float v) {
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, false));   // lane ^ 1
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, false));   // lane ^ 2
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, false));  // 7 - i of 8 lanes
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, false));  // 15 - i of 16 lanes
    return v;
}
}  // namespace

template <bool VEC, bool ONE>
__global__ __launch_bounds__(kThreads) void k_head_fwd(int P, int H, int tiles, const float *__restrict__ X,
                                                       const float *__restrict__ W, const float *__restrict__ bias,
                                                       const float *__restrict__ im, const float *__restrict__ iq,
                                                       float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float s_lds[];  // !ONE: W as 7 x HP, zeros past H
    const int NC = ONE ? 1 : div_up(H, kChunk), HP = NC * kChunk;
    const int t = threadIdx.x, l = t & 15, slot = t >> 4;

    float4 w[7];
    if (ONE) {
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int c = 4 * l;
            w[j].x = c < H ? W[(size_t)j * H + c] : 0.f;
            w[j].y = c + 1 < H ? W[(size_t)j * H + c + 1] : 0.f;
            w[j].z = c + 2 < H ? W[(size_t)j * H + c + 2] : 0.f;
            w[j].w = c + 3 < H ? W[(size_t)j * H + c + 3] : 0.f;
        }
    } else {
        for (int i = t; i < 7 * HP; i += kThreads) {
            const int j = i / HP, c = i - j * HP;
            s_lds[i] = c < H ? W[(size_t)j * H + c] : 0.f;
        }
        lds_barrier();
    }
    const float bj = l < 7 ? bias[l] : 0.f;

    const int first = blockIdx.x * kFwdTiles, last = first + kFwdTiles < tiles ? first + kFwdTiles : tiles;
    for (int tile = first; tile < last; ++tile) {
        const int row0 = tile * kRows + slot;  // this slot's rows: row0, + kSlots, ...
        float acc[kPasses][7];
#pragma unroll
        for (int u = 0; u < kPasses; ++u)
#pragma unroll
            for (int j = 0; j < 7; ++j) acc[u][j] = 0.f;
#pragma unroll 2
        for (int c = 0; c < NC; ++c) {
            const int col = c * kChunk + 4 * l;
            float4 xv[kPasses];
#pragma unroll
            for (int u = 0; u < kPasses; ++u) {
                const int row = row0 + u * kSlots;
                xv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < P) {
                    const float *xr = X + (size_t)row * H + col;
                    if (VEC) {
                        if (col < H) xv[u] = *(const float4 *)xr;  // H % 4 == 0: col + 3 < H
                    } else {
                        if (col < H) xv[u].x = xr[0];
                        if (col + 1 < H) xv[u].y = xr[1];
                        if (col + 2 < H) xv[u].z = xr[2];
                        if (col + 3 < H) xv[u].w = xr[3];
                    }
                }
            }
            if (!ONE) {
#pragma unroll
                for (int j = 0; j < 7; ++j) w[j] = *(const float4 *)(s_lds + j * HP + col);
            }
#pragma unroll
            for (int u = 0; u < kPasses; ++u)
#pragma unroll
                for (int j = 0; j < 7; ++j) {
                    float a = acc[u][j];
                    a = fmaf(xv[u].x, w[j].x, a);
                    a = fmaf(xv[u].y, w[j].y, a);
                    a = fmaf(xv[u].z, w[j].z, a);
                    acc[u][j] = fmaf(xv[u].w, w[j].w, a);
                }
        }
#pragma unroll
        for (int u = 0; u < kPasses; ++u) {
            float s = 0.f;  // lane j keeps column j
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const float r = row16_sum(acc[u][j]);
                if (l == j) s = r;
            }
            const size_t row = (size_t)(row0 + u * kSlots);
            if (l < 7 && row < (size_t)P) {
                const float init = l < 3 ? im[row * 3 + l] : iq[row * 4 + l - 3];
                out[row * 7 + l] = (s + bj) + init;
            }
        }
    }
}

// partial == NULL: neither dL_dweight nor dL_dbias; want_w == 0: x is not read and the dL_dweight part of the
// partial is not written; dX == NULL: nothing of size (P, H) is written.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_head_bwd(int P, int H, int tiles, const float *__restrict__ X,
                                                       const float *__restrict__ W, const float *__restrict__ G,
                                                       float *__restrict__ dX, float *__restrict__ partial, int want_w) {
    extern __shared__ __attribute__((aligned(16))) float s_lds[];
    const int CG = div_up(H, 4), HP = 4 * CG;
    const int RP = kThreads / CG < kRows ? kThreads / CG : kRows;  // row slots
    float *gs = s_lds;                  // 2 x kRows x 8: the tile's upstream gradients, [row][7] is never read
    float *red = gs + 2 * kRows * 8;    // RP x 7 x HP
    float *redb = red + RP * 7 * HP;    // RP x 7
    const int t = threadIdx.x, rl = t / CG, col = 4 * (t - rl * CG);
    const bool active = rl < RP, want_x = dX != nullptr, sums = partial != nullptr;

    float w[7][4], acc[7][4], accb[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        accb[j] = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[j][e] = 0.f;
            w[j][e] = want_x && active && col + e < H ? W[(size_t)j * H + col + e] : 0.f;
        }
    }

    // the next tile's upstream gradients wait in registers while this one is worked on
    constexpr int NG = (kTileOut + kThreads - 1) / kThreads;
    float gp[NG];
    auto fetch_g = [&](int tile) {
#pragma unroll
        for (int n = 0; n < NG; ++n) {
            const int e = t + n * kThreads;
            gp[n] = e < kTileOut && tile * kRows + e / 7 < P ? G[(size_t)tile * kTileOut + e] : 0.f;
        }
    };
    if ((int)blockIdx.x < tiles) fetch_g(blockIdx.x);

    int buf = 0;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x, buf ^= 1) {
        const int row0 = tile * kRows;
        float *g = gs + buf * kRows * 8;
#pragma unroll
        for (int n = 0; n < NG; ++n) {
            const int e = t + n * kThreads, rr = e / 7;
            if (e < kTileOut) g[rr * 8 + (e - rr * 7)] = gp[n];
        }
        lds_barrier();  // two buffers: the tile before the previous one has been consumed by now
        if (tile + (int)gridDim.x < tiles) fetch_g(tile + gridDim.x);
#pragma unroll 4
        for (int rr = rl; rr < (active ? kRows : 0); rr += RP) {
            const int row = row0 + rr;
            if (row >= P) break;
            float gr[7];
#pragma unroll
            for (int j = 0; j < 7; ++j) gr[j] = g[rr * 8 + j];
            const size_t at = (size_t)row * H + col;
            if (want_w) {
                float xv[4];
                if (VEC) {
                    const float4 v = *(const float4 *)(X + at);
                    xv[0] = v.x; xv[1] = v.y; xv[2] = v.z; xv[3] = v.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) xv[e] = col + e < H ? X[at + e] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < 7; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(gr[j], xv[e], acc[j][e]);
            }
            if (sums) {
#pragma unroll
                for (int j = 0; j < 7; ++j) accb[j] += gr[j];
            }
            if (want_x) {
                float d[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    d[e] = gr[0] * w[0][e];
#pragma unroll
                    for (int j = 1; j < 7; ++j) d[e] = fmaf(gr[j], w[j][e], d[e]);
                }
                if (VEC) {
                    *(float4 *)(dX + at) = make_float4(d[0], d[1], d[2], d[3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (col + e < H) dX[at + e] = d[e];
                }
            }
        }
    }
    if (!sums) return;

    // the row slots' sums, added in slot order
    if (active) {
        if (want_w) {
#pragma unroll
            for (int j = 0; j < 7; ++j)
                *(float4 *)(red + (rl * 7 + j) * HP + col) = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
        }
        if (col == 0) {
#pragma unroll
            for (int j = 0; j < 7; ++j) redb[rl * 7 + j] = accb[j];
        }
    }
    lds_barrier();
    float *mine = partial + (size_t)blockIdx.x * (7 * H + 7);
    if (want_w)
        for (int i = t; i < 7 * H; i += kThreads) {
            const int j = i / H, c = i - j * H;
            float s = 0.f;
            for (int k = 0; k < RP; ++k) s += red[(k * 7 + j) * HP + c];
            mine[i] = s;
        }
    if (t < 7) {
        float s = 0.f;
        for (int k = 0; k < RP; ++k) s += redb[k * 7 + t];
        mine[7 * H + t] = s;
    }
}

// one wave per element of the (7 H + 7) partials (dW = [0, 7 H), db the rest), summed over the workgroups in
// their order: lanes take consecutive chunks, then neighbours merge
__global__ __launch_bounds__(64) void k_head_reduce(int H, int nb, const float *__restrict__ partial,
                                                    float *__restrict__ dW, float *__restrict__ db) {
    const int n = 7 * H + 7, i = blockIdx.x, lane = threadIdx.x;
    float *dst = i < 7 * H ? (dW ? dW + i : nullptr) : (db ? db + (i - 7 * H) : nullptr);
    if (!dst) return;
    const int chunk = div_up(nb, 64);
    double s = 0.0;
    for (int b = lane * chunk; b < nb && b < (lane + 1) * chunk; ++b) s += (double)partial[(size_t)b * n + i];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
    if (lane == 0) *dst = (float)s;
}

// ---- host launchers --------------------------------------------------------------------------
namespace {
size_t bwd_lds(int H) {
    const int CG = div_up(H, 4), RP = kThreads / CG < kRows ? kThreads / CG : kRows;
    return sizeof(float) * ((size_t)2 * kRows * 8 + (size_t)RP * 7 * 4 * CG + (size_t)RP * 7);
}

template <bool VEC>
void run_fwd(int nb, int P, int H, int tiles, const float *x, const float *W, const float *bias, const float *im,
             const float *iq, float *out, hipStream_t s) {
    if (H <= kChunk) k_head_fwd<VEC, true><<<nb, kThreads, 0, s>>>(P, H, tiles, x, W, bias, im, iq, out);
    else k_head_fwd<VEC, false><<<nb, kThreads, sizeof(float) * 7 * div_up(H, kChunk) * kChunk, s>>>(P, H, tiles, x, W, bias,
                                                                                                   im, iq, out);
}

int head_blocks(int P, int max_blocks) { return persistent_blocks(P, kRows, max_blocks, kHeadAutoBlocks); }
}  // namespace

hipError_t launch_head_fwd(int P, int H, const float *x, const float *W, const float *bias, const float *im,
                           const float *iq, float *out, hipStream_t s) {
    const int tiles = div_up(P, kRows), nb = div_up(tiles, kFwdTiles);
    if (H % 4 == 0 && aligned16(x)) run_fwd<true>(nb, P, H, tiles, x, W, bias, im, iq, out, s);
    else run_fwd<false>(nb, P, H, tiles, x, W, bias, im, iq, out, s);
    return hipGetLastError();
}

size_t head_partial_floats(int P, int H, int max_blocks) { return (size_t)head_blocks(P, max_blocks) * (7 * (size_t)H + 7); }

hipError_t launch_head_bwd(int P, int H, const float *x, const float *W, const float *g, float *partial, int max_blocks,
                           float *dx, float *dW, float *db, hipStream_t s) {
    const int nb = head_blocks(P, max_blocks), tiles = div_up(P, kRows);
    const bool sums = dW || db;
    const bool vec = H % 4 == 0 && (!dW || aligned16(x)) && (!dx || aligned16(dx));
    if (vec) k_head_bwd<true><<<nb, kThreads, bwd_lds(H), s>>>(P, H, tiles, x, W, g, dx, sums ? partial : nullptr, dW != nullptr);
    else k_head_bwd<false><<<nb, kThreads, bwd_lds(H), s>>>(P, H, tiles, x, W, g, dx, sums ? partial : nullptr, dW != nullptr);
    if (sums) k_head_reduce<<<7 * H + 7, 64, 0, s>>>(H, nb, partial, dW, db);
    return hipGetLastError();
}

}  // namespace gsr
