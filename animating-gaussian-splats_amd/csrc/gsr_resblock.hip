// gsr_resblock.hip -- the residual blocks of train.py's deformation network (train.py:57-77), fused:
//     y1 = x W1^T;  a1 = gelu(bn1(y1));  y2 = a1 W2^T;  out = gelu(bn2(y2) + x)
// with both BatchNorms on the batch statistics (the reference never calls .eval()), GELU in the exact erf
// form.  All fp32 on v_mfma_f32_32x32x2_f32 (bit for bit a k-ordered fmaf chain); no float atomics: every
// reduction over rows is one partial per workgroup, combined in workgroup order, so two runs are bitwise equal.
//
// A workgroup of 8 waves takes 64-row tiles (tile = block, block + grid, ...).  H is padded to HP = 32 NT
// columns (NT = 1 .. 4) with zeros; LDS row strides are HP + 1 (odd: the 32 rows a lane group reads for the
// MFMA A operand hit 32 banks; B operands and the staging stores are consecutive floats).  The GEMM kernels
// load the next tile's rows into registers before they multiply the current one, so the loads' latency is
// behind the MFMAs even with one workgroup per CU (H > 64).
//
//   k_res_gemm<NT, PRO>      Y = A W^T with A = X (PRO = false) or gelu(bn(X)) applied on the way into LDS
//                            (PRO = true).  W staged once, k-major.  Wave w owns rows 32 (w & 1) .. + 31 and
//                            column tile w >> 1.  Per tile each wave reduces its 32 x 32 result to a per-column
//                            (mean, M2) about its own mean in registers; the workgroup merges them over its
//                            tiles with Chan's formula in double and writes one (count, mean, M2) per column.
//   k_res_stats              merges the workgroups' partials (Chan, double, workgroup order: lanes take
//                            consecutive chunks, then neighbours merge) into mean and 1 / sqrt(var + eps), and
//                            blends the running statistics (unbiased variance) as torch does.
//   k_res_out                out = gelu(bn2(y2) + x), float4 where H % 4 == 0.
//   k_res_bwd_out            g_s = g_out gelu'(bn2(y2) + x) and per-workgroup column sums of g_s and g_s xhat2,
//                            over column chunks of a power of two (any H).
//   k_res_colsum             those partials (double) summed in workgroup order: dbeta, dgamma.
//   k_res_bwd_gemm<NT, ST>   G = BN-backward of (g_in, y) formed into LDS; dW += G^T A accumulated in registers
//                            over the workgroup's tiles (A = gelu(bn1(y1)) recomputed for stage 2, x for stage
//                            1), one H x H partial per workgroup; R = G W, then stage 2 writes g_z1 = R gelu'(bn1(y1))
//                            and the column sums of g_z1 and g_z1 xhat1, stage 1 writes g_x = R + g_s.
//   k_res_reduce_w           sums the dW partials in workgroup order.
//
// The above is H <= 128, where the whole weight stays in LDS.  128 < H <= 512 runs the k_res_*_wide kernels
// further down (128-column blocks of the output, k panels of 128, dW in a kernel of its own) with the same
// k_res_stats, k_res_out, k_res_bwd_out, k_res_colsum and k_res_reduce_w.  The two halves differ in their main
// loops (how the operands reach LDS); the mathematics around them is one set of device helpers: Bn (a column's
// BatchNorm, forward), BnBack / bn_back_apply (its backward), merge_tile_stats (the forward GEMM's Chan merge)
// and bwd_r_epilogue / store_stage2_sums (the epilogue of R = G W).  The forward GEMM's store of Y with the
// wave's (mean, M2), and the final partial store, stay written out in k_res_gemm and k_res_gemm_wide: behind a
// shared function k_res_gemm<4, false> compiled to 92 VGPRs and lost an occupancy step.  k_res_gemm_wide keeps
// them out of caution only, so that the H > 128 forward runs the device code it ran before; no cost of the shared
// form was isolated for it.  On the host one resblock_grid() sizes every grid and the workspace, and gemm<PRO> /
// stage<STAGE> choose between the halves.
#include "gsr_common.h"
#include "gsr_internal.h"
#include "gsr_mlp.h"

namespace gsr {

namespace {
constexpr int kRows = 64, kThreads = 512, kEwThreads = 256;
constexpr int kOutBlocks = 1024;  // workgroups of k_res_bwd_out when the caller sets no bound

struct BnCols { const float *mean, *invstd, *gamma, *beta; };

__device__ inline float gelu_f(float t) { return (t * 0.5f) * (1.0f + erff(t * 0.70710678118654752440f)); }
// Phi(t) + t phi(t)
__device__ inline float gelu_grad(float t) {
    const float cdf = 0.5f * (1.0f + erff(t * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * expf(-0.5f * (t * t));
    return cdf + t * pdf;
}

// (n, mean, M2) of a set followed by (nb, mb, m2b) of the next
__device__ inline void chan(double &n, double &mean, double &m2, double nb, double mb, double m2b) {
    if (nb == 0.0) return;
    if (n == 0.0) { n = nb; mean = mb; m2 = m2b; return; }
    const double tot = n + nb, d = mb - mean;
    mean = mean + d * (nb / tot);
    m2 = m2 + m2b + d * d * (n * nb / tot);
    n = tot;
}

// one column's BatchNorm
struct Bn {
    float mean, invstd, gamma, beta;
    __device__ float xhat(float v) const { return (v - mean) * invstd; }
    __device__ float bn_apply(float v) const { return xhat(v) * gamma + beta; }
};
// column c of bn, zeros past H
__device__ inline Bn bn_load(const BnCols &bn, int c, int H) {
    Bn k = {0.f, 0.f, 0.f, 0.f};
    if (c < H) {
        k.mean = bn.mean[c];
        k.invstd = bn.invstd[c];
        k.gamma = bn.gamma[c];
        k.beta = bn.beta[c];
    }
    return k;
}
// column i into cols[0 .. 4 HP), HP floats per member, and column c back from there
template <int HP>
__device__ inline void stage_bn(float *cols, const BnCols &bn, int i, int H) {
    const Bn k = bn_load(bn, i, H);
    cols[i] = k.mean;
    cols[HP + i] = k.invstd;
    cols[2 * HP + i] = k.gamma;
    cols[3 * HP + i] = k.beta;
}
template <int HP>
__device__ inline Bn bn_staged(const float *cols, int c) {
    return {cols[c], cols[HP + c], cols[2 * HP + c], cols[3 * HP + c]};
}
template <int HP>
__device__ inline float bn_gelu(float v, const float *cols, int c) {
    return gelu_f(bn_staged<HP>(cols, c).bn_apply(v));
}

// the BatchNorm backward's constants of one column: mean, invstd, gamma invstd, dbeta / P, dgamma / P
struct BnBack { float mean, invstd, scale, db, dg; };
__device__ inline BnBack bn_back(const BnCols &bn, const float *sums, int c, int H, int P) {
    BnBack k = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (c < H) {
        k.mean = bn.mean[c];
        k.invstd = bn.invstd[c];
        k.scale = bn.gamma[c] * k.invstd;
        k.db = sums[c] / (float)P;
        k.dg = sums[H + c] / (float)P;
    }
    return k;
}
__device__ inline float bn_back_apply(const BnBack &k, float g, float y) {
    const float xh = (y - k.mean) * k.invstd;
    return k.scale * ((g - k.db) - xh * k.dg);
}

// The two row halves' (mean, M2) of column c of the tile at row0, st[(2 h, 2 h + 1) * stride + c], merged onto the
// thread's running (rn, rmean, rm2).
__device__ inline void merge_tile_stats(double &rn, double &rmean, double &rm2, const float *st, int stride, int c, int row0,
                                        int P) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        int nv = P - (row0 + h * 32);
        nv = nv < 0 ? 0 : (nv > 32 ? 32 : nv);
        chan(rn, rmean, rm2, (double)nv, (double)st[(h * 2 + 0) * stride + c], (double)st[(h * 2 + 1) * stride + c]);
    }
}

// Epilogue of R = G W for the wave's 32 x 32 result (rows rbase .., column col).  Stage 2: g_z1 = R gelu'(bn1(y1)),
// a_in = y1, and this lane's sums of g_z1 and g_z1 xhat1 onto (ps0, ps1).  Stage 1: g_x = R + g_s.  bn1_of() gives
// bn1 of column col and is asked per row: the narrow kernel reads its staged columns there, which keeps four
// registers free across the loads (an occupancy step of k_res_bwd_gemm<1, 2>); the wide one holds them anyway.
template <int STAGE, class BnOf>
__device__ inline void bwd_r_epilogue(const f32x16 &acc, int rbase, int lane, int col, int H, int P,
                                      const float *__restrict__ a_in, BnOf bn1_of, const float *__restrict__ g_s,
                                      float *__restrict__ g_out, double &ps0, double &ps1) {
    if (col >= H) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = rbase + acc_row(r, lane);
        if (row >= P) continue;
        const size_t at = (size_t)row * H + col;
        if (STAGE == 2) {
            const Bn bn1 = bn1_of();
            const float y = a_in[at];
            const float gz = acc[r] * gelu_grad(bn1.bn_apply(y));
            g_out[at] = gz;
            ps0 += (double)gz;
            ps1 += (double)(gz * bn1.xhat(y));
        } else {
            g_out[at] = acc[r] + g_s[at];
        }
    }
}
// Stage 2's sums of a workgroup: the lanes' (ps0, ps1) of column lc of the workgroup's `stride` columns, through
// red[2 row halves][2 sums][stride] (the LDS of the operand tiles), to partialS at column col0 + lc.  All threads call it.
__device__ inline void store_stage2_sums(double ps0, double ps1, double *red, int stride, int lc, int mt, int lane, int H,
                                         double *__restrict__ partialS, int col0) {
    const int t = threadIdx.x;
    ps0 += __shfl_xor(ps0, 32);
    ps1 += __shfl_xor(ps1, 32);
    lds_barrier();  // every wave is done with the last tile
    if (lc < stride && lane < 32) {
        red[(mt * 2 + 0) * stride + lc] = ps0;
        red[(mt * 2 + 1) * stride + lc] = ps1;
    }
    lds_barrier();
    if (t < stride && col0 + t < H) {
        partialS[((size_t)blockIdx.x * 2 + 0) * H + col0 + t] = red[t] + red[2 * stride + t];
        partialS[((size_t)blockIdx.x * 2 + 1) * H + col0 + t] = red[stride + t] + red[3 * stride + t];
    }
}

// prefetch slot q of thread t: row r and column c of the kRows x HP tile
template <int HP>
__device__ inline void slot_rc(int t, int q, int &r, int &c) {
    const int i = t + q * kThreads;
    r = i / HP;
    c = i - r * HP;
}
}  // namespace

template <int NT, bool PRO>
__global__ __launch_bounds__(kThreads) void k_res_gemm(int P, int H, int tiles, const float *__restrict__ X,
                                                       const float *__restrict__ W, BnCols bn, float *__restrict__ Y,
                                                       double *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float s_lds[];
    constexpr int HP = NT * 32, XS = HP + 1, WS = HP + 1;
    float *Xs = s_lds;               // kRows * XS
    float *Ws = Xs + kRows * XS;     // HP * WS, k-major: Ws[k][j] = W[j][k]
    float *cols = Ws + HP * WS;      // 4 * HP: mean, invstd, gamma, beta of the prologue's BatchNorm
    float *st = cols + 4 * HP;       // 2 x (mean, M2) x HP: the two row halves of the tile
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, mt = w & 1, nt = w >> 1;
    const int KP = (H + 1) & ~1;

    for (int i = t; i < HP * HP; i += kThreads) {
        const int j = i / HP, k = i - j * HP;
        Ws[k * WS + j] = j < H && k < H ? W[(size_t)j * H + k] : 0.f;
    }
    if (PRO)
        for (int i = t; i < HP; i += kThreads) stage_bn<HP>(cols, bn, i, H);
    double rn = 0.0, rmean = 0.0, rm2 = 0.0;  // thread t < H: column t over this workgroup's tiles
    const float *xa = Xs + (mt * 32 + (lane & 31)) * XS + (lane >> 5);
    const float *wb = Ws + (lane >> 5) * WS + nt * 32 + (lane & 31);

    // the next tile's rows wait in registers while this one is multiplied
    constexpr int NL = kRows * HP / kThreads;
    float pre[NL];
    auto fetch = [&](int tile) {
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            int r, c;
            slot_rc<HP>(t, q, r, c);
            const int row = tile * kRows + r;
            pre[q] = row < P && c < H ? X[(size_t)row * H + c] : 0.f;
        }
    };
    if ((int)blockIdx.x < tiles) fetch(blockIdx.x);

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int row0 = tile * kRows;
        lds_barrier();  // W and the column constants are visible / the previous tile has been consumed
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            int r, c;
            slot_rc<HP>(t, q, r, c);
            float v = pre[q];
            if (PRO && row0 + r < P && c < H) v = bn_gelu<HP>(v, cols, c);
            Xs[r * XS + c] = v;
        }
        lds_barrier();
        if (tile + (int)gridDim.x < tiles) fetch(tile + gridDim.x);
        if (nt < NT) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            for (int k = 0; k < KP; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[k], wb[k * WS], acc, 0, 0, 0);
            const int col = nt * 32 + (lane & 31);
            const int rbase = row0 + mt * 32;
            float sum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rbase + acc_row(r, lane);
                if (row < P) {
                    if (col < H) Y[(size_t)row * H + col] = acc[r];
                    sum += acc[r];
                }
            }
            sum += __shfl_xor(sum, 32);
            int nv = P - rbase;
            nv = nv < 0 ? 0 : (nv > 32 ? 32 : nv);
            const float mean = nv > 0 ? sum / (float)nv : 0.f;
            float m2 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float d = acc[r] - mean;
                if (rbase + acc_row(r, lane) < P) m2 += d * d;
            }
            m2 += __shfl_xor(m2, 32);
            if (lane < 32) {
                st[(mt * 2 + 0) * HP + col] = mean;
                st[(mt * 2 + 1) * HP + col] = m2;
            }
        }
        lds_barrier();
        if (t < H) merge_tile_stats(rn, rmean, rm2, st, HP, t, row0, P);
    }
    if (t < H) {
        double *p = partial + (size_t)blockIdx.x * 3 * H;
        p[t] = rn;
        p[H + t] = rmean;
        p[2 * H + t] = rm2;
    }
}

// one wave per column
__global__ __launch_bounds__(64) void k_res_stats(int P, int H, int nb, const double *__restrict__ partial, float eps,
                                                  float momentum, float *__restrict__ mean_out, float *__restrict__ invstd_out,
                                                  float *__restrict__ running_mean, float *__restrict__ running_var) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int chunk = div_up(nb, 64);
    double n = 0.0, mean = 0.0, m2 = 0.0;
    for (int b = lane * chunk; b < nb && b < (lane + 1) * chunk; ++b) {
        const double *p = partial + (size_t)b * 3 * H;
        chan(n, mean, m2, p[c], p[H + c], p[2 * H + c]);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {  // neighbours merge, the lower lanes' rows first
        const double on = __shfl_xor(n, o), om = __shfl_xor(mean, o), o2 = __shfl_xor(m2, o);
        if (lane & o) {
            double an = on, am = om, a2 = o2;
            chan(an, am, a2, n, mean, m2);
            n = an; mean = am; m2 = a2;
        } else {
            chan(n, mean, m2, on, om, o2);
        }
    }
    if (lane != 0) return;
    const double var = m2 / (double)P;
    mean_out[c] = (float)mean;
    invstd_out[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * (float)mean;
    if (running_var) running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (float)(m2 / (double)(P - 1));
}

template <bool VEC>
__global__ __launch_bounds__(kEwThreads) void k_res_out(size_t n, int H, const float *__restrict__ y2,
                                                        const float *__restrict__ x, BnCols bn, float *__restrict__ out) {
    const size_t stride = (size_t)gridDim.x * kEwThreads;
    for (size_t i = (size_t)blockIdx.x * kEwThreads + threadIdx.x; i < n; i += stride) {
        if (VEC) {
            const int c = (int)((i * 4) % (size_t)H);
            const float4 y = ((const float4 *)y2)[i], xi = ((const float4 *)x)[i];
            const float4 m = *(const float4 *)(bn.mean + c), is = *(const float4 *)(bn.invstd + c);
            const float4 g = *(const float4 *)(bn.gamma + c), b = *(const float4 *)(bn.beta + c);
            float4 o;
            o.x = gelu_f((((y.x - m.x) * is.x) * g.x + b.x) + xi.x);
            o.y = gelu_f((((y.y - m.y) * is.y) * g.y + b.y) + xi.y);
            o.z = gelu_f((((y.z - m.z) * is.z) * g.z + b.z) + xi.z);
            o.w = gelu_f((((y.w - m.w) * is.w) * g.w + b.w) + xi.w);
            ((float4 *)out)[i] = o;
        } else {
            const int c = (int)(i % (size_t)H);
            out[i] = gelu_f((((y2[i] - bn.mean[c]) * bn.invstd[c]) * bn.gamma[c] + bn.beta[c]) + x[i]);
        }
    }
}

// CW: a power of two, at most 256: the columns are walked in chunks of CW (one chunk of the power of two >= H for
// H <= 128, chunks of 128 above); thread t takes column t & (CW - 1) of each chunk and rows t / CW, + 256 / CW, ...
__global__ __launch_bounds__(kEwThreads) void k_res_bwd_out(int P, int H, int tiles, int CW, const float *__restrict__ g_out,
                                                            const float *__restrict__ y2, const float *__restrict__ x,
                                                            BnCols bn, float *__restrict__ g_s, double *__restrict__ partial) {
    __shared__ double s_red[2][kEwThreads];
    const int t = threadIdx.x, rl = t / CW, RW = kEwThreads / CW;
    for (int c0 = 0; c0 < H; c0 += CW) {
        const int c = c0 + (t & (CW - 1));
        const bool in = c < H;
        const Bn k = bn_load(bn, c, H);
        double s0 = 0.0, s1 = 0.0;
        for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
            const int row0 = tile * kRows;
            for (int r = rl; r < kRows; r += RW) {
                const int row = row0 + r;
                if (row < P && in) {
                    const size_t i = (size_t)row * H + c;
                    const float y = y2[i];
                    const float gs = g_out[i] * gelu_grad(k.bn_apply(y) + x[i]);
                    g_s[i] = gs;
                    s0 += (double)gs;
                    s1 += (double)(gs * k.xhat(y));
                }
            }
        }
        s_red[0][t] = s0;
        s_red[1][t] = s1;
        lds_barrier();
        if (t < CW && in) {
            double a0 = 0.0, a1 = 0.0;
            for (int q = 0; q < RW; ++q) {
                a0 += s_red[0][q * CW + t];
                a1 += s_red[1][q * CW + t];
            }
            partial[((size_t)blockIdx.x * 2 + 0) * H + c] = a0;
            partial[((size_t)blockIdx.x * 2 + 1) * H + c] = a1;
        }
        lds_barrier();  // s_red is free for the next chunk
    }
}

// one wave per column: sums[c] = sum_b partial[b][0][c], sums[H + c] = sum_b partial[b][1][c], in a fixed order
__global__ __launch_bounds__(64) void k_res_colsum(int H, int nb, const double *__restrict__ partial, float *__restrict__ sums,
                                                   float *__restrict__ dbeta, float *__restrict__ dgamma) {
    const int c = blockIdx.x, lane = threadIdx.x;
    double a0 = 0.0, a1 = 0.0;
    for (int b = lane; b < nb; b += 64) {
        a0 += partial[((size_t)b * 2 + 0) * H + c];
        a1 += partial[((size_t)b * 2 + 1) * H + c];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a0 += __shfl_xor(a0, o);
        a1 += __shfl_xor(a1, o);
    }
    if (lane != 0) return;
    sums[c] = (float)a0;
    sums[H + c] = (float)a1;
    if (dbeta) dbeta[c] = (float)a0;
    if (dgamma) dgamma[c] = (float)a1;
}

// STAGE 2: g_in = g_s, yn = y2 (bn2), A = gelu(bn1(y1)), W = W2, g_out = g_z1 (+ column sums for bn1)
// STAGE 1: g_in = g_z1, yn = y1 (bn1), A = x, W = W1, g_out = g_x = G W1 + g_s
// g_out == NULL: G W is not computed; partialW == NULL: dW is not computed.
template <int NT, int STAGE>
__global__ __launch_bounds__(kThreads) void k_res_bwd_gemm(int P, int H, int tiles, const float *__restrict__ g_in,
                                                           const float *__restrict__ yn, BnCols bnG,
                                                           const float *__restrict__ sums, const float *__restrict__ a_in,
                                                           BnCols bnA, const float *__restrict__ W,
                                                           const float *__restrict__ g_s, float *__restrict__ g_out,
                                                           float *__restrict__ partialW, double *__restrict__ partialS) {
    extern __shared__ __attribute__((aligned(16))) float s_lds[];
    constexpr int HP = NT * 32, XS = HP + 1, WS = HP + 1;
    constexpr int NQ = (NT * NT + 7) / 8;  // 32 x 32 tiles of dW per wave
    float *Gs = s_lds;                // kRows * XS (+ 1: an even float count, As stays 8-byte aligned)
    float *As = Gs + kRows * XS + (kRows * XS & 1);
    float *colsG = As + kRows * XS;   // 5 * HP: mean, invstd, gamma invstd, dbeta / P, dgamma / P
    float *colsA = colsG + 5 * HP;    // 4 * HP: mean, invstd, gamma, beta of bn1 (stage 2)
    float *Wn = colsA + 4 * HP;       // HP * WS, as stored: Wn[j][k] = W[j][k]
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, mt = w & 1, nt = w >> 1;
    const int KP = (H + 1) & ~1;
    const bool want_g = g_out != nullptr, want_w = partialW != nullptr;

    if (want_g)
        for (int i = t; i < HP * HP; i += kThreads) {
            const int j = i / HP, k = i - j * HP;
            Wn[j * WS + k] = j < H && k < H ? W[(size_t)j * H + k] : 0.f;
        }
    for (int i = t; i < HP; i += kThreads) {
        const BnBack k = bn_back(bnG, sums, i, H, P);
        colsG[i] = k.mean;
        colsG[HP + i] = k.invstd;
        colsG[2 * HP + i] = k.scale;
        colsG[3 * HP + i] = k.db;
        colsG[4 * HP + i] = k.dg;
        if (STAGE == 2) stage_bn<HP>(colsA, bnA, i, H);
    }
    f32x16 dw[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) dw[q][r] = 0.f;
    double ps0 = 0.0, ps1 = 0.0;  // stage 2: this lane's rows of column nt * 32 + (lane & 31)

    // the next tile's rows wait in registers while this one is multiplied
    constexpr int NL = kRows * HP / kThreads;
    float pg[NL], py[NL], pa[NL];
    auto fetch = [&](int tile) {
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            int r, c;
            slot_rc<HP>(t, q, r, c);
            const int row = tile * kRows + r;
            const bool in = row < P && c < H;
            const size_t at = (size_t)row * H + c;
            pg[q] = in ? g_in[at] : 0.f;
            py[q] = in ? yn[at] : 0.f;
            pa[q] = in && want_w ? a_in[at] : 0.f;
        }
    };
    if ((int)blockIdx.x < tiles) fetch(blockIdx.x);

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int row0 = tile * kRows;
        lds_barrier();  // W and the column constants are visible / the previous tile has been consumed
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            int r, c;
            slot_rc<HP>(t, q, r, c);
            float gy = 0.f, a = 0.f;
            if (row0 + r < P && c < H) {
                const BnBack k = {colsG[c], colsG[HP + c], colsG[2 * HP + c], colsG[3 * HP + c], colsG[4 * HP + c]};
                gy = bn_back_apply(k, pg[q], py[q]);
                a = pa[q];
                if (STAGE == 2 && want_w) a = bn_gelu<HP>(a, colsA, c);
            }
            Gs[r * XS + c] = gy;
            As[r * XS + c] = a;
        }
        lds_barrier();
        if (tile + (int)gridDim.x < tiles) fetch(tile + gridDim.x);
        if (want_w) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int id = w + 8 * q;
                if (id < NT * NT) {
                    const float *ga = Gs + (lane >> 5) * XS + (id / NT) * 32 + (lane & 31);
                    const float *ab = As + (lane >> 5) * XS + (id % NT) * 32 + (lane & 31);
#pragma unroll 4
                    for (int k = 0; k < kRows; k += 2)
                        dw[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[k * XS], ab[k * XS], dw[q], 0, 0, 0);
                }
            }
        }
        if (want_g && nt < NT) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            const float *ga = Gs + (mt * 32 + (lane & 31)) * XS + (lane >> 5);
            const float *wb = Wn + (lane >> 5) * WS + nt * 32 + (lane & 31);
            for (int j = 0; j < KP; j += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[j], wb[j * WS], acc, 0, 0, 0);
            const int col = nt * 32 + (lane & 31);
            bwd_r_epilogue<STAGE>(acc, row0 + mt * 32, lane, col, H, P, a_in, [&] { return bn_staged<HP>(colsA, col); }, g_s,
                                  g_out, ps0, ps1);
        }
    }

    if (want_w) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int id = w + 8 * q;
            if (id >= NT * NT) continue;
            const int k = (id % NT) * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = (id / NT) * 32 + acc_row(r, lane);
                if (j < H && k < H) partialW[((size_t)blockIdx.x * H + j) * H + k] = dw[q][r];
            }
        }
    }
    if (STAGE == 2 && want_g)  // red over the G tile
        store_stage2_sums(ps0, ps1, (double *)s_lds, HP, nt * 32 + (lane & 31), mt, lane, H, partialS, 0);
}

__global__ __launch_bounds__(256) void k_res_reduce_w(int n, int nb, const float *__restrict__ partial, float *__restrict__ dW) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += (double)partial[(size_t)b * n + i];
    dW[i] = (float)s;
}

// ---- 128 < H <= 512 ------------------------------------------------------------------------------
// An H x H weight no longer fits LDS and an H x H dW no longer fits a workgroup's registers, so the grid
// gets a second dimension over 128-column blocks of the output and the reduction dimension is walked in
// panels of 128: per panel the workgroup stages 64 x 128 of the left operand and 128 x 128 of the weight and
// multiplies on into the same accumulators, so every output element is still one fmaf chain over ascending k.
// Staging slot q of thread t is row (t >> 7) + 4 q of panel column t & 127: a thread's column is fixed within
// a panel and its BatchNorm constants travel in registers with the prefetched values.
//
//   k_res_gemm_wide<PRO>     k_res_gemm for column block blockIdx.y; a column belongs to one block, so the
//                            statistics partials keep their (workgroup along the rows, 3, H) layout.
//   k_res_bwd_r_wide<ST>     R = G W for column block blockIdx.y with the epilogues of k_res_bwd_gemm.
//   k_res_bwd_w_wide<ST>     dW = G^T A: workgroup (row group, 128 x 128 block of dW) forms the G and A panels
//                            of the block's columns per 64-row tile, each wave two 32 x 32 accumulators; one
//                            partial per row group, summed by k_res_reduce_w in row-group order.
namespace {
constexpr int kPanel = 128, kPS = kPanel + 1;    // columns per block / k per panel; LDS row stride
constexpr int kRowStep = kThreads / kPanel;      // rows between a thread's staging slots
constexpr int kNX = kRows * kPanel / kThreads;   // staging slots per thread of a 64 x 128 panel
constexpr int kNW = kPanel * kPanel / kThreads;  // ... of a 128 x 128 weight panel

// base[r H + c] from the last row for r >= rows and from column 0 unless `cin` (c < H): an unconditional load, so a
// thread's loads issue back to back without a branch each.  The value of a clamped slot is some element of the
// matrix.  Where the slot's index along the reduction is past H it is replaced by 0 on its way into LDS (one
// predicate per thread and panel, no mask per prefetched value kept alive across the multiply); a slot of a row
// past P or of an output column past H only feeds results that are neither stored nor counted in a sum.
__device__ inline float load_clamped(const float *base, int r, int rows, int H, int c, bool cin) {
    return base[(unsigned)((r < rows ? r : rows - 1) * H + (cin ? c : 0))];
}
}  // namespace

template <bool PRO>
__global__ __launch_bounds__(kThreads) void k_res_gemm_wide(int P, int H, int tiles, const float *__restrict__ X,
                                                            const float *__restrict__ W, BnCols bn,
                                                            float *__restrict__ Y, double *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float s_lds[];
    float *Xs = s_lds;              // kRows * kPS
    float *Ws = Xs + kRows * kPS;   // kPanel * kPS, k-major: Ws[k][j] = W[col0 + j][k0 + k]
    float *st = Ws + kPanel * kPS;  // 2 x (mean, M2) x kPanel: the two row halves of the tile
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, mt = w & 1, nt = w >> 1;
    const int col0 = blockIdx.y * kPanel, panels = div_up(H, kPanel), KP = (H + 1) & ~1;
    const int pc = t & (kPanel - 1), pr = t >> 7;
    const bool live = col0 + nt * 32 < H;  // this wave's column tile holds a column of the matrix

    float px[kNX], pw[kNW];
    Bn kb = {0.f, 0.f, 0.f, 0.f};  // the prologue's BatchNorm of the prefetched panel's column
    auto fetch = [&](int tile, int kp) {
        const int k = kp * kPanel + pc;
        const bool kin = k < H;
        const float *xt = X + (size_t)tile * kRows * H, *wt = W + (size_t)col0 * H;  // uniform bases, 32-bit offsets
        const int rows = P - tile * kRows, cols = H - col0;
#pragma unroll
        for (int q = 0; q < kNX; ++q) px[q] = load_clamped(xt, pr + q * kRowStep, rows, H, k, kin);
#pragma unroll
        for (int q = 0; q < kNW; ++q) pw[q] = load_clamped(wt, pr + q * kRowStep, cols, H, k, kin);
        if (PRO && kin) kb = bn_load(bn, k, H);
    };
    if ((int)blockIdx.x < tiles) fetch(blockIdx.x, 0);

    double rn = 0.0, rmean = 0.0, rm2 = 0.0;  // thread t < 128: column col0 + t over this workgroup's tiles
    const float *xa = Xs + (mt * 32 + (lane & 31)) * kPS + (lane >> 5);
    const float *wb = Ws + (lane >> 5) * kPS + nt * 32 + (lane & 31);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int row0 = tile * kRows;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int kp = 0; kp < panels; ++kp) {
            const bool kin = kp * kPanel + pc < H;
            lds_barrier();  // the previous panel has been consumed
#pragma unroll
            for (int q = 0; q < kNX; ++q) {
                const int r = pr + q * kRowStep;
                float v = px[q];
                if (PRO) v = gelu_f(kb.bn_apply(v));
                Xs[r * kPS + pc] = kin ? v : 0.f;
            }
#pragma unroll
            for (int q = 0; q < kNW; ++q) Ws[pc * kPS + pr + q * kRowStep] = kin ? pw[q] : 0.f;
            lds_barrier();
            const bool last = kp + 1 == panels;
            if (!last || tile + (int)gridDim.x < tiles) fetch(last ? tile + gridDim.x : tile, last ? 0 : kp + 1);
            if (live) {
                const int kn = KP - kp * kPanel < kPanel ? KP - kp * kPanel : kPanel;
                for (int k = 0; k < kn; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[k], wb[k * kPS], acc, 0, 0, 0);
            }
        }
        if (live) {
            const int lc = nt * 32 + (lane & 31), col = col0 + lc;
            const int rbase = row0 + mt * 32;
            float sum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rbase + acc_row(r, lane);
                if (row < P) {
                    if (col < H) Y[(size_t)row * H + col] = acc[r];
                    sum += acc[r];
                }
            }
            sum += __shfl_xor(sum, 32);
            int nv = P - rbase;
            nv = nv < 0 ? 0 : (nv > 32 ? 32 : nv);
            const float mean = nv > 0 ? sum / (float)nv : 0.f;
            float m2 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float d = acc[r] - mean;
                if (rbase + acc_row(r, lane) < P) m2 += d * d;
            }
            m2 += __shfl_xor(m2, 32);
            if (lane < 32) {
                st[(mt * 2 + 0) * kPanel + lc] = mean;
                st[(mt * 2 + 1) * kPanel + lc] = m2;
            }
        }
        lds_barrier();
        if (t < kPanel && col0 + t < H) merge_tile_stats(rn, rmean, rm2, st, kPanel, t, row0, P);
    }
    if (t < kPanel && col0 + t < H) {
        double *p = partial + (size_t)blockIdx.x * 3 * H + col0 + t;
        p[0] = rn;
        p[H] = rmean;
        p[2 * H] = rm2;
    }
}

// stages as k_res_bwd_gemm; grid (workgroups along the rows, column blocks of g_out)
template <int STAGE>
__global__ __launch_bounds__(kThreads) void k_res_bwd_r_wide(int P, int H, int tiles, const float *__restrict__ g_in,
                                                             const float *__restrict__ yn, BnCols bnG,
                                                             const float *__restrict__ sums, const float *__restrict__ a_in,
                                                             BnCols bnA, const float *__restrict__ W,
                                                             const float *__restrict__ g_s, float *__restrict__ g_out,
                                                             double *__restrict__ partialS) {
    extern __shared__ __attribute__((aligned(16))) float s_lds[];
    float *Gs = s_lds;             // kRows * kPS
    float *Wn = Gs + kRows * kPS;  // kPanel * kPS, as stored: Wn[j][k] = W[j0 + j][col0 + k]
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, mt = w & 1, nt = w >> 1;
    const int col0 = blockIdx.y * kPanel, panels = div_up(H, kPanel), KP = (H + 1) & ~1;
    const int pc = t & (kPanel - 1), pr = t >> 7;
    const int lc = nt * 32 + (lane & 31), col = col0 + lc;
    const bool live = col0 + nt * 32 < H;

    const Bn bn1 = bn_load(bnA, col, H);  // bn1 of this lane's output column; stage 1 does not use it and the loads go
    double ps0 = 0.0, ps1 = 0.0;          // stage 2: this lane's rows of column col

    float pg[kNX], py[kNX], pw[kNW];
    BnBack kb = {0.f, 0.f, 0.f, 0.f, 0.f};
    auto fetch = [&](int tile, int jp) {
        const int j = jp * kPanel + pc;
        const size_t base = (size_t)tile * kRows * H;  // uniform bases, 32-bit offsets
        const float *gt = g_in + base, *yt = yn + base, *wt = W + (size_t)jp * kPanel * H + col0;
        const int rows = P - tile * kRows, wrows = H - jp * kPanel;
#pragma unroll
        for (int q = 0; q < kNX; ++q) {
            pg[q] = load_clamped(gt, pr + q * kRowStep, rows, H, j, j < H);
            py[q] = load_clamped(yt, pr + q * kRowStep, rows, H, j, j < H);
        }
#pragma unroll
        for (int q = 0; q < kNW; ++q) {
            pw[q] = load_clamped(wt, pr + q * kRowStep, wrows, H, pc, col0 + pc < H);
        }
        kb = bn_back(bnG, sums, j, H, P);
    };
    if ((int)blockIdx.x < tiles) fetch(blockIdx.x, 0);

    const float *ga = Gs + (mt * 32 + (lane & 31)) * kPS + (lane >> 5);
    const float *wb = Wn + (lane >> 5) * kPS + lc;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int row0 = tile * kRows;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int jp = 0; jp < panels; ++jp) {
            const bool jin = jp * kPanel + pc < H;
            lds_barrier();  // the previous panel has been consumed
#pragma unroll
            for (int q = 0; q < kNX; ++q) {
                const int r = pr + q * kRowStep;
                Gs[r * kPS + pc] = jin ? bn_back_apply(kb, pg[q], py[q]) : 0.f;
            }
#pragma unroll
            for (int q = 0; q < kNW; ++q) {
                const int j = pr + q * kRowStep;
                Wn[j * kPS + pc] = jp * kPanel + j < H ? pw[q] : 0.f;
            }
            lds_barrier();
            const bool last = jp + 1 == panels;
            if (!last || tile + (int)gridDim.x < tiles) fetch(last ? tile + gridDim.x : tile, last ? 0 : jp + 1);
            if (live) {
                const int jn = KP - jp * kPanel < kPanel ? KP - jp * kPanel : kPanel;
                for (int j = 0; j < jn; j += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[j], wb[j * kPS], acc, 0, 0, 0);
            }
        }
        bwd_r_epilogue<STAGE>(acc, row0 + mt * 32, lane, col, H, P, a_in, [&] { return bn1; }, g_s, g_out, ps0, ps1);
    }
    if (STAGE == 2) store_stage2_sums(ps0, ps1, (double *)s_lds, kPanel, lc, mt, lane, H, partialS, col0);  // red over the G panel
}

// grid (row groups, CB * CB blocks of dW): block blockIdx.y = jb * CB + kb is dW[128 jb .., 128 kb ..]
template <int STAGE>
__global__ __launch_bounds__(kThreads) void k_res_bwd_w_wide(int P, int H, int tiles, int CB, const float *__restrict__ g_in,
                                                             const float *__restrict__ yn, BnCols bnG,
                                                             const float *__restrict__ sums, const float *__restrict__ a_in,
                                                             BnCols bnA, float *__restrict__ partialW) {
    extern __shared__ __attribute__((aligned(16))) float s_lds[];
    float *Gs = s_lds;             // kRows * kPS: columns j0 ..
    float *As = Gs + kRows * kPS;  // kRows * kPS: columns k0 ..
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int j0 = ((int)blockIdx.y / CB) * kPanel, k0 = ((int)blockIdx.y % CB) * kPanel;
    const int pc = t & (kPanel - 1), pr = t >> 7;
    const int cj = j0 + pc, ck = k0 + pc;
    const BnBack kb = bn_back(bnG, sums, cj, H, P);
    const Bn bn1 = bn_load(bnA, ck, H);  // bn1 of column ck; stage 1 does not use it and the loads go

    f32x16 dw[2];  // 32 x 32 tiles w and w + 8 of the block's 4 x 4
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) dw[q][r] = 0.f;

    float pg[kNX], py[kNX], pa[kNX];
    auto fetch = [&](int tile) {
        const size_t base = (size_t)tile * kRows * H;  // uniform bases, 32-bit offsets
        const float *gt = g_in + base, *yt = yn + base, *at = a_in + base;
        const int rows = P - tile * kRows;
#pragma unroll
        for (int q = 0; q < kNX; ++q) {
            pg[q] = load_clamped(gt, pr + q * kRowStep, rows, H, cj, cj < H);
            py[q] = load_clamped(yt, pr + q * kRowStep, rows, H, cj, cj < H);
            pa[q] = load_clamped(at, pr + q * kRowStep, rows, H, ck, ck < H);
        }
    };
    if ((int)blockIdx.x < tiles) fetch(blockIdx.x);

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int row0 = tile * kRows;
        lds_barrier();  // the previous tile has been consumed
#pragma unroll
        for (int q = 0; q < kNX; ++q) {
            const int r = pr + q * kRowStep;
            const bool rin = row0 + r < P;
            float a = pa[q];
            if (STAGE == 2) a = gelu_f(bn1.bn_apply(a));
            Gs[r * kPS + pc] = rin && cj < H ? bn_back_apply(kb, pg[q], py[q]) : 0.f;
            As[r * kPS + pc] = rin && ck < H ? a : 0.f;
        }
        lds_barrier();
        if (tile + (int)gridDim.x < tiles) fetch(tile + gridDim.x);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int id = w + 8 * q, jt = id >> 2, kt = id & 3;
            if (j0 + jt * 32 < H && k0 + kt * 32 < H) {
                const float *ga = Gs + (lane >> 5) * kPS + jt * 32 + (lane & 31);
                const float *ab2 = As + (lane >> 5) * kPS + kt * 32 + (lane & 31);
#pragma unroll 4
                for (int k = 0; k < kRows; k += 2)
                    dw[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[k * kPS], ab2[k * kPS], dw[q], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int id = w + 8 * q, jt = id >> 2, kt = id & 3;
        const int k = k0 + kt * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + jt * 32 + acc_row(r, lane);
            if (j < H && k < H) partialW[((size_t)blockIdx.x * H + j) * H + k] = dw[q][r];
        }
    }
}

// ---- host launchers --------------------------------------------------------------------------
namespace {
int res_nt(int H) { return div_up(H, 32); }

size_t fwd_lds(int nt) {
    const int HP = nt * 32;
    return sizeof(float) * ((size_t)kRows * (HP + 1) + (size_t)HP * (HP + 1) + 8 * HP);
}
size_t bwd_lds(int nt) {
    const int HP = nt * 32, tile = kRows * (HP + 1);
    return sizeof(float) * ((size_t)2 * tile + (tile & 1) + 9 * HP + (size_t)HP * (HP + 1));
}

constexpr size_t kWideFwdLds = sizeof(float) * ((size_t)kRows * kPS + (size_t)kPanel * kPS + 4 * kPanel);
constexpr size_t kWideRLds = sizeof(float) * ((size_t)kRows * kPS + (size_t)kPanel * kPS);
constexpr size_t kWideWLds = sizeof(float) * ((size_t)2 * kRows * kPS);

bool wide(int H) { return H > kResblockNarrowH; }
int wide_cb(int H) { return div_up(H, kPanel); }  // column blocks; 1 for H <= 128

// The grids of one (P, H, max_blocks), which the workspace's carving and both launchers share.
//   nb  workgroups along the rows of the forward and backward GEMM kernels.  H <= 64: two fit a CU's LDS.  H > 128:
//       with the CB column blocks about one per CU (their LDS admits no second).
//   ng  row groups of dW = G^T A, one partial each.  H <= 128: dW comes from the same workgroups, ng = nb.  H > 128:
//       with the CB x CB blocks of dW about one workgroup per CU as well, which bounds the dW partials by
//       kResblockAutoBlocks x 128 x 128 floats (16 MB) for every H and P.
//   no  workgroups of k_res_bwd_out.
struct ResblockGrid { int nb, ng, no; };
ResblockGrid resblock_grid(int P, int H, int max_blocks) {
    const int cb = wide_cb(H), per_cu = H <= 64 ? 2 : 1;
    return {persistent_blocks(P, kRows, max_blocks, kResblockAutoBlocks * per_cu / cb),
            persistent_blocks(P, kRows, max_blocks, kResblockAutoBlocks * per_cu / (cb * cb)),
            persistent_blocks(P, kRows, max_blocks, kOutBlocks)};
}

// Y = A W^T and its statistics partials, A = X or gelu(bn(X))
template <bool PRO>
hipError_t gemm(const ResblockGrid &g, int P, int H, const float *X, const float *W, const BnCols &bn, float *Y,
                double *partial, hipStream_t s) {
    const int tiles = div_up(P, kRows);
    if (wide(H))
        return launch_lds(k_res_gemm_wide<PRO>, dim3(g.nb, wide_cb(H)), kThreads, kWideFwdLds, s, P, H, tiles, X, W, bn, Y,
                          partial);
    return dispatch_tiles(res_nt(H), [&](auto n) {
        constexpr int NT = decltype(n)::value;
        return launch_lds(k_res_gemm<NT, PRO>, g.nb, kThreads, fwd_lds(NT), s, P, H, tiles, X, W, bn, Y, partial);
    });
}

// stage STAGE of the backward: R = G W into g_out (unless NULL) and dW into dW (unless NULL)
template <int STAGE>
hipError_t stage(const ResblockGrid &g, int P, int H, const float *g_in, const float *yn, const BnCols &bnG,
                 const float *sums, const float *a_in, const BnCols &bnA, const float *W, const float *g_s, float *g_out,
                 float *partialW, float *dW, double *partialS, hipStream_t s) {
    const int tiles = div_up(P, kRows), cb = wide_cb(H);
    hipError_t e = hipSuccess;
    if (!wide(H)) {
        e = dispatch_tiles(res_nt(H), [&](auto n) {
            constexpr int NT = decltype(n)::value;
            return launch_lds(k_res_bwd_gemm<NT, STAGE>, g.nb, kThreads, bwd_lds(NT), s, P, H, tiles, g_in, yn, bnG, sums,
                              a_in, bnA, W, g_s, g_out, dW ? partialW : nullptr, partialS);
        });
    } else {
        if (g_out)
            e = launch_lds(k_res_bwd_r_wide<STAGE>, dim3(g.nb, cb), kThreads, kWideRLds, s, P, H, tiles, g_in, yn, bnG, sums,
                           a_in, bnA, W, g_s, g_out, partialS);
        if (e == hipSuccess && dW)
            e = launch_lds(k_res_bwd_w_wide<STAGE>, dim3(g.ng, cb * cb), kThreads, kWideWLds, s, P, H, tiles, cb, g_in, yn,
                           bnG, sums, a_in, bnA, partialW);
    }
    if (e != hipSuccess) return e;
    if (dW) k_res_reduce_w<<<div_up(H * H, 256), 256, 0, s>>>(H * H, g.ng, partialW, dW);
    return hipGetLastError();
}
}  // namespace

ResblockWorkspace::ResblockWorkspace(int P, int H, int max_blocks, bool backward) {
    const ResblockGrid g = resblock_grid(P, H, max_blocks);
    const size_t nb = (size_t)g.nb, ng = (size_t)g.ng, no = (size_t)g.no;
    const size_t h = (size_t)H, ph = (size_t)P * h;
    size_t o = 0;
    partial_s = o; o = align256(o + sizeof(double) * 3 * h * (nb > no ? nb : no));
    partial_w = sums = g_s = g_z1 = o;
    if (backward) {
        partial_w = o; o = align256(o + sizeof(float) * ng * h * h);
        sums = o;      o = align256(o + sizeof(float) * 4 * h);
        g_s = o;       o = align256(o + sizeof(float) * ph);
        g_z1 = o;      o = align256(o + sizeof(float) * ph);
    }
    total = o;
}

hipError_t launch_resblock_fwd(int P, int H, const float *x, const float *W1, const float *gamma1, const float *beta1,
                               const float *W2, const float *gamma2, const float *beta2, float eps1, float eps2,
                               float momentum1, float momentum2, float *running_mean1, float *running_var1,
                               float *running_mean2, float *running_var2, char *ws, int max_blocks, float *y1, float *y2,
                               float *out, float *stats, hipStream_t s) {
    const ResblockWorkspace L(P, H, max_blocks, false);
    const ResblockGrid g = resblock_grid(P, H, max_blocks);
    double *partial = (double *)(ws + L.partial_s);
    const BnCols none = {nullptr, nullptr, nullptr, nullptr};
    const BnCols bn1 = {stats, stats + H, gamma1, beta1}, bn2 = {stats + 2 * H, stats + 3 * H, gamma2, beta2};
    hipError_t e = gemm<false>(g, P, H, x, W1, none, y1, partial, s);
    if (e != hipSuccess) return e;
    k_res_stats<<<H, 64, 0, s>>>(P, H, g.nb, partial, eps1, momentum1, stats, stats + H, running_mean1, running_var1);
    e = gemm<true>(g, P, H, y1, W2, bn1, y2, partial, s);
    if (e != hipSuccess) return e;
    k_res_stats<<<H, 64, 0, s>>>(P, H, g.nb, partial, eps2, momentum2, stats + 2 * H, stats + 3 * H, running_mean2, running_var2);
    const size_t n = (size_t)P * H;
    const bool vec = H % 4 == 0 && aligned16(y2) && aligned16(x) && aligned16(out) && aligned16(stats) &&
                     aligned16(gamma2) && aligned16(beta2);
    const size_t items = vec ? n / 4 : n;
    const size_t want = (items + kEwThreads - 1) / kEwThreads;
    const unsigned grid = (unsigned)(want < 8192 ? want : 8192);
    if (vec) k_res_out<true><<<grid, kEwThreads, 0, s>>>(items, H, y2, x, bn2, out);
    else k_res_out<false><<<grid, kEwThreads, 0, s>>>(items, H, y2, x, bn2, out);
    return hipGetLastError();
}

hipError_t launch_resblock_bwd(int P, int H, const float *x, const float *y1, const float *y2, const float *stats,
                               const float *W1, const float *gamma1, const float *beta1, const float *W2,
                               const float *gamma2, const float *beta2, const float *g_out, char *ws, int max_blocks,
                               float *dx, float *dW1, float *dgamma1, float *dbeta1, float *dW2, float *dgamma2,
                               float *dbeta2, hipStream_t s) {
    const ResblockWorkspace L(P, H, max_blocks, true);
    const ResblockGrid g = resblock_grid(P, H, max_blocks);
    double *partial_s = (double *)(ws + L.partial_s);
    float *partial_w = (float *)(ws + L.partial_w), *sums = (float *)(ws + L.sums);
    float *g_s = (float *)(ws + L.g_s), *g_z1 = (float *)(ws + L.g_z1);
    const BnCols bn1 = {stats, stats + H, gamma1, beta1}, bn2 = {stats + 2 * H, stats + 3 * H, gamma2, beta2};
    const bool below = dx || dW1 || dgamma1 || dbeta1;  // anything past a1
    int CW = 8;  // k_res_bwd_out's column chunk: the power of two >= H, 128 for H > 128
    while (CW < H && CW < kPanel) CW <<= 1;
    k_res_bwd_out<<<g.no, kEwThreads, 0, s>>>(P, H, div_up(P, kRows), CW, g_out, y2, x, bn2, g_s, partial_s);
    k_res_colsum<<<H, 64, 0, s>>>(H, g.no, partial_s, sums, dbeta2, dgamma2);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (dW2 || below) {
        e = stage<2>(g, P, H, g_s, y2, bn2, sums, y1, bn1, W2, nullptr, below ? g_z1 : nullptr, partial_w, dW2, partial_s, s);
        if (e != hipSuccess) return e;
        if (below) k_res_colsum<<<H, 64, 0, s>>>(H, g.nb, partial_s, sums + 2 * H, dbeta1, dgamma1);
    }
    if (dx || dW1) {
        e = stage<1>(g, P, H, g_z1, y1, bn1, sums + 2 * H, x, bn1, W1, g_s, dx, partial_w, dW1, nullptr, s);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

}  // namespace gsr
