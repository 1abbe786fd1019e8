// gsr_rigidity.hip -- the rigidity term of train.py and the neighbour search that feeds it.
//
// Replaces, per training step, calculate_rigidity_loss (train.py:325-351: an int64 index gather,
// F x k broadcast 3x3 mat-vecs, an elementwise tail and an autograd backward that scatters into the
// neighbour rows) and, once per sequence, compute_knn_indices_and_squared_distances (shared.py:45-61:
// a per-point Python loop over a CPU KD-tree).
//
//   k_knn        exact brute force.  One lane per query point; candidates stream through LDS in tiles
//                of 256 (every lane reads the same LDS word: a broadcast), squared distances in float64
//                from the fp32 coordinates (shared.py:50 widens to float64), each lane's current best K
//                kept sorted in registers.  Self is excluded by index.  Candidates are visited in
//                ascending index order and a candidate displaces an entry only when strictly closer,
//                so equal distances keep the lower index first: the result is fully defined, also for
//                the coincident means densification's clones start from.
//   k_rigid_fwd  one lane per foreground Gaussian i, looping over its k neighbour slots j:
//                    q = raw_q / max(|raw_q|, 1e-12);  rel = q (x) pinv_i;  R = build_rotation(rel)
//                    v_ij = R^T (m_nbr - m_i);  term_ij = sqrt(|v_ij - o_prev_ij|^2 w_ij + 1e-20)
//                The (k, F) neighbour-major arrays (row of the neighbour, weight, previous offset) are
//                read lane-adjacent; only the neighbour means are a random 12-byte gather.  When a
//                backward will follow it also stores d(sum of terms)/d(everything): per edge the
//                world-space vector u_ij = d/dm_nbr, per Gaussian -sum_j u_ij and the gradient of its
//                raw quaternion (through both normalisations).  Per-block double partial sums.
//                A second instantiation also stores the state the NEXT timestep compares with, from
//                the q and m_nbr - m_i it already holds.
//   k_foreground_info  that state alone (create_foreground_info, train.py:228-248): one lane per
//                foreground Gaussian, conj(q) as one float4 and the k offsets in the (k, 3, F) layout
//                k_rigid_fwd reads.
//   k_rigid_sum  one block: fixed-order sum of the block partials -> mean over the F k terms.
//   k_rigid_bwd  one lane per row of the full (P, .) parameter arrays: a foreground row adds the stored
//                u of the edges that list it (reverse adjacency, CSR, fixed order: no float atomics)
//                to its own part and scales by the upstream gradient read from device memory;
//                background rows get zeros.
#include "gsr_common.h"
#include "gsr_internal.h"

namespace gsr {

constexpr int kKnnBlock = 256;  // queries per block = candidates per LDS tile
constexpr int kRigBlock = 256;

// ------------------------------------------------------------------------------------------
// Queries [q0, q1) of n points against all n points; out_idx / out_d2 are (n, k) row-major.
template <int K>
__global__ __launch_bounds__(kKnnBlock) void k_knn(int n, int q0, int q1, int k, const float *__restrict__ pts,
                                                   int *__restrict__ out_idx, double *__restrict__ out_d2) {
    __shared__ double s_x[kKnnBlock], s_y[kKnnBlock], s_z[kKnnBlock];
    const int q = q0 + blockIdx.x * kKnnBlock + threadIdx.x;
    const bool live = q < q1;
    const int qq = live ? q : q1 - 1;  // idle lanes of the last block follow its last query (barriers)
    const double qx = pts[3 * (size_t)qq], qy = pts[3 * (size_t)qq + 1], qz = pts[3 * (size_t)qq + 2];
    double bd[K];
    int bi[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { bd[j] = __builtin_huge_val(); bi[j] = -1; }
    for (int base = 0; base < n; base += kKnnBlock) {
        const int c = base + threadIdx.x;
        lds_barrier();  // the previous tile has been consumed
        if (c < n) {
            s_x[threadIdx.x] = pts[3 * (size_t)c];
            s_y[threadIdx.x] = pts[3 * (size_t)c + 1];
            s_z[threadIdx.x] = pts[3 * (size_t)c + 2];
        }
        lds_barrier();
        const int m = min(kKnnBlock, n - base);
#pragma unroll 2
        for (int t = 0; t < m; ++t) {
            const double dx = s_x[t] - qx, dy = s_y[t] - qy, dz = s_z[t] - qz;
            const double d = dx * dx + dy * dy + dz * dz;
            if (d < bd[K - 1] && base + t != qq) {
                const int ci = base + t;
#pragma unroll
                for (int j = K - 1; j > 0; --j) {  // top down: bd[j - 1] is still the old entry
                    const bool shift = d < bd[j - 1], here = d < bd[j];
                    bi[j] = shift ? bi[j - 1] : (here ? ci : bi[j]);
                    bd[j] = shift ? bd[j - 1] : (here ? d : bd[j]);
                }
                if (d < bd[0]) { bd[0] = d; bi[0] = ci; }
            }
        }
    }
    if (live) {
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j < k) {
                out_idx[(size_t)q * k + j] = bi[j];
                out_d2[(size_t)q * k + j] = bd[j];
            }
    }
}

// ------------------------------------------------------------------------------------------
// Sum of v over the block in a fixed order (lanes by xor-halving, then waves in index order), valid in
// thread 0.  `s_w`: one double per wave.
__device__ inline double block_sum_fixed(double v, double *s_w) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    lds_barrier();
    double t = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += s_w[w];
    return t;
}

// The state the next timestep's rigidity term compares with (create_foreground_info, train.py:228-248),
// from values a lane of foreground Gaussian i holds: the conjugate of its normalised quaternion, and
// the offset to its j-th neighbour in the (k, 3, F) layout k_rigid_fwd reads as prev_off (lane-adjacent
// stores).
__device__ inline float4 inverted_rotation(float4 q) { return make_float4(q.x, -q.y, -q.z, -q.w); }
__device__ inline void store_offset(float *__restrict__ out_off, int F, int j, int i, float d0, float d1, float d2) {
    const size_t o = (3 * (size_t)j) * F + i;
    out_off[o] = d0; out_off[o + F] = d1; out_off[o + 2 * (size_t)F] = d2;
}

// One lane per foreground Gaussian: the state alone, where no loss precedes it (a sequence's first
// timestep, inference).  Either output may be NULL: it is then neither computed nor stored.  Only
// foreground rows of means / quats are read.
__global__ __launch_bounds__(kRigBlock) void k_foreground_info(int F, int k, const float *__restrict__ means,
                                                               const float *__restrict__ quats,
                                                               const int *__restrict__ fg_rows,
                                                               const int *__restrict__ nbr_rows,
                                                               float4 *__restrict__ out_inv, float *__restrict__ out_off) {
    const int i = blockIdx.x * kRigBlock + threadIdx.x;
    if (i >= F) return;
    const size_t row = (size_t)fg_rows[i];
    if (out_inv) {
        const float4 raw = reinterpret_cast<const float4 *>(quats)[row];
        out_inv[i] = inverted_rotation(act_normalize(raw, quat_norm(raw)));
    }
    if (out_off) {
        const float mx = means[3 * row], my = means[3 * row + 1], mz = means[3 * row + 2];
#pragma unroll 4
        for (int j = 0; j < k; ++j) {
            const size_t nr = (size_t)nbr_rows[(size_t)j * F + i];
            store_offset(out_off, F, j, i, means[3 * nr] - mx, means[3 * nr + 1] - my, means[3 * nr + 2] - mz);
        }
    }
}

// save_* (all three or none): d(sum of the F k terms)/d(neighbour mean) per edge (k, F, 3), its negated
// sum over a Gaussian's own edges (F, 3) and d/d(raw quaternion) (F, 4).
// kState: also store this cloud's state (next_inv (F, 4), next_off (k, 3, F), both required) from the q
// and d0..d2 the loss is evaluated with; the other instantiation holds none of that code.
template <bool kState>
__global__ __launch_bounds__(kRigBlock) void k_rigid_fwd(int F, int k, const float *__restrict__ means,
                                                         const float *__restrict__ quats, const int *__restrict__ fg_rows,
                                                         const int *__restrict__ nbr_rows, const float *__restrict__ weights,
                                                         const float *__restrict__ prev_off, const float4 *__restrict__ prev_inv,
                                                         double *__restrict__ partial, float *__restrict__ save_u,
                                                         float *__restrict__ save_m, float4 *__restrict__ save_q,
                                                         float4 *__restrict__ next_inv, float *__restrict__ next_off) {
    __shared__ double s_w[kRigBlock / 64];
    const int i = blockIdx.x * kRigBlock + threadIdx.x;
    double sum = 0;
    if (i < F) {
        const size_t row = (size_t)fg_rows[i];
        const float mx = means[3 * row], my = means[3 * row + 1], mz = means[3 * row + 2];
        const float4 raw = reinterpret_cast<const float4 *>(quats)[row];
        const float4 p = prev_inv[i];
        const float nraw = quat_norm(raw);
        const float4 q = act_normalize(raw, nraw);
        if constexpr (kState) next_inv[i] = inverted_rotation(q);
        // quat_mult(q, p), train.py:311-318 (components (w, x, y, z) = (.x, .y, .z, .w))
        const float4 rel = make_float4(q.x * p.x - q.y * p.y - q.z * p.z - q.w * p.w,
                                       q.x * p.y + q.y * p.x + q.z * p.w - q.w * p.z,
                                       q.x * p.z - q.y * p.w + q.z * p.x + q.w * p.y,
                                       q.x * p.w + q.y * p.z - q.z * p.y + q.w * p.x);
        // build_rotation, external.py:27-46: normalises again (no epsilon), rows R[r][c]
        const float nrel = quat_norm(rel);
        const float r = rel.x / nrel, x = rel.y / nrel, y = rel.z / nrel, z = rel.w / nrel;
        const float R00 = 1.f - 2.f * (y * y + z * z), R01 = 2.f * (x * y - r * z), R02 = 2.f * (x * z + r * y);
        const float R10 = 2.f * (x * y + r * z), R11 = 1.f - 2.f * (x * x + z * z), R12 = 2.f * (y * z - r * x);
        const float R20 = 2.f * (x * z - r * y), R21 = 2.f * (y * z + r * x), R22 = 1.f - 2.f * (x * x + y * y);
        float G[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // d/dR[r][c] = sum_j d_r a_c
        float ux = 0.f, uy = 0.f, uz = 0.f;
        for (int j = 0; j < k; ++j) {
            const size_t e = (size_t)j * F + i;
            const size_t nr = (size_t)nbr_rows[e];
            const float w = weights[e];
            const float ox = prev_off[(3 * (size_t)j) * F + i], oy = prev_off[(3 * (size_t)j + 1) * F + i],
                        oz = prev_off[(3 * (size_t)j + 2) * F + i];
            const float d0 = means[3 * nr] - mx, d1 = means[3 * nr + 1] - my, d2 = means[3 * nr + 2] - mz;
            if constexpr (kState) store_offset(next_off, F, j, i, d0, d1, d2);
            const float e0 = (R00 * d0 + R10 * d1 + R20 * d2) - ox;
            const float e1 = (R01 * d0 + R11 * d1 + R21 * d2) - oy;
            const float e2 = (R02 * d0 + R12 * d1 + R22 * d2) - oz;
            const float t = sqrtf((e0 * e0 + e1 * e1 + e2 * e2) * w + 1e-20f);
            sum += (double)t;
            if (save_u) {
                // d t / d v = w (v - o) / t (exactly 0 for a zero weight); back to the world frame: R a
                const float a0 = w * e0 / t, a1 = w * e1 / t, a2 = w * e2 / t;
                const float u0 = R00 * a0 + R01 * a1 + R02 * a2;
                const float u1 = R10 * a0 + R11 * a1 + R12 * a2;
                const float u2 = R20 * a0 + R21 * a1 + R22 * a2;
                save_u[3 * e] = u0; save_u[3 * e + 1] = u1; save_u[3 * e + 2] = u2;
                ux += u0; uy += u1; uz += u2;
                G[0] += d0 * a0; G[1] += d0 * a1; G[2] += d0 * a2;
                G[3] += d1 * a0; G[4] += d1 * a1; G[5] += d1 * a2;
                G[6] += d2 * a0; G[7] += d2 * a1; G[8] += d2 * a2;
            }
        }
        if (save_u) {
            save_m[3 * (size_t)i] = -ux; save_m[3 * (size_t)i + 1] = -uy; save_m[3 * (size_t)i + 2] = -uz;
            // d/d(normalised rel) through build_rotation's entries
            float4 gn;
            gn.x = 2.f * (-z * G[1] + y * G[2] + z * G[3] - x * G[5] - y * G[6] + x * G[7]);
            gn.y = 2.f * (y * G[1] + z * G[2] + y * G[3] - 2.f * x * G[4] - r * G[5] + z * G[6] + r * G[7] - 2.f * x * G[8]);
            gn.z = 2.f * (-2.f * y * G[0] + x * G[1] + r * G[2] + x * G[3] + z * G[5] - r * G[6] + z * G[7] - 2.f * y * G[8]);
            gn.w = 2.f * (-2.f * z * G[0] - r * G[1] + x * G[2] + r * G[3] - 2.f * z * G[4] + y * G[5] + x * G[6] + y * G[7]);
            // build_rotation's division by |rel|
            const float dn = r * gn.x + x * gn.y + y * gn.z + z * gn.w;
            const float4 gr = make_float4((gn.x - r * dn) / nrel, (gn.y - x * dn) / nrel, (gn.z - y * dn) / nrel,
                                          (gn.w - z * dn) / nrel);
            // quat_mult's first argument
            const float4 gq = make_float4(gr.x * p.x + gr.y * p.y + gr.z * p.z + gr.w * p.w,
                                          -gr.x * p.y + gr.y * p.x - gr.z * p.w + gr.w * p.z,
                                          -gr.x * p.z + gr.y * p.w + gr.z * p.x - gr.w * p.y,
                                          -gr.x * p.w - gr.y * p.z + gr.z * p.y + gr.w * p.x);
            save_q[i] = act_normalize_bwd(q, nraw, gq);  // F.normalize of the raw quaternion
        }
    }
    const double tot = block_sum_fixed(sum, s_w);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void k_rigid_sum(int nb, const double *__restrict__ partial, double inv_n,
                                                   float *__restrict__ out_loss) {
    __shared__ double s_w[4];
    double v = 0;
    for (int b = threadIdx.x; b < nb; b += 256) v += partial[b];
    const double tot = block_sum_fixed(v, s_w);
    if (threadIdx.x == 0) *out_loss = (float)(tot * inv_n);
}

__global__ __launch_bounds__(kRigBlock) void k_rigid_bwd(int P, const int *__restrict__ row_to_fg,
                                                         const int *__restrict__ rev_off, const int *__restrict__ rev_edge,
                                                         const float *__restrict__ save_u, const float *__restrict__ save_m,
                                                         const float4 *__restrict__ save_q, const float *__restrict__ g_loss,
                                                         float inv_n, float *__restrict__ dmeans, float *__restrict__ dquats) {
    const int row = blockIdx.x * kRigBlock + threadIdx.x;
    if (row >= P) return;
    const int i = row_to_fg[row];
    float gx = 0.f, gy = 0.f, gz = 0.f;
    float4 gq = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i >= 0) {
        const float gs = g_loss[0] * inv_n;
        if (dmeans) {
            float sx = save_m[3 * (size_t)i], sy = save_m[3 * (size_t)i + 1], sz = save_m[3 * (size_t)i + 2];
            const int e1 = rev_off[i + 1];
            for (int s = rev_off[i]; s < e1; ++s) {  // the edges that list this Gaussian, in stored order
                const size_t e = (size_t)rev_edge[s];
                sx += save_u[3 * e]; sy += save_u[3 * e + 1]; sz += save_u[3 * e + 2];
            }
            gx = gs * sx; gy = gs * sy; gz = gs * sz;
        }
        if (dquats) {
            const float4 t = save_q[i];
            gq = make_float4(gs * t.x, gs * t.y, gs * t.z, gs * t.w);
        }
    }
    if (dmeans) { dmeans[3 * (size_t)row] = gx; dmeans[3 * (size_t)row + 1] = gy; dmeans[3 * (size_t)row + 2] = gz; }
    if (dquats) reinterpret_cast<float4 *>(dquats)[row] = gq;
}

// ==========================================================================================
// One launch covers at most kKnnPairs (query, candidate) pairs, so that no launch holds the device
// for long at a million points (the queries of a launch are independent of the other launches').
constexpr long long kKnnPairs = 1ll << 37;

hipError_t launch_knn(int n, const float *pts, int k, int *out_idx, double *out_d2, hipStream_t s) {
    long long per = kKnnPairs / (n > 0 ? n : 1);
    per = per / kKnnBlock * kKnnBlock;
    if (per < kKnnBlock) per = kKnnBlock;
    for (long long q0 = 0; q0 < n; q0 += per) {
        const int q1 = (int)(q0 + per < n ? q0 + per : n);
        const int nb = div_up(q1 - (int)q0, kKnnBlock);
        if (k == 20)
            k_knn<20><<<nb, kKnnBlock, 0, s>>>(n, (int)q0, q1, k, pts, out_idx, out_d2);
        else
            k_knn<32><<<nb, kKnnBlock, 0, s>>>(n, (int)q0, q1, k, pts, out_idx, out_d2);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

int rigid_blocks(int F) { return div_up(F, kRigBlock); }

hipError_t launch_rigid_fwd(int F, int k, const float *means, const float *quats, const int *fg_rows,
                            const int *nbr_rows, const float *weights, const float *prev_off, const float *prev_inv,
                            double *partial, float *save_u, float *save_m, float *save_q, float *out_loss,
                            float *next_inv, float *next_off, hipStream_t s) {
    const int nb = rigid_blocks(F);
    const float4 *pinv = reinterpret_cast<const float4 *>(prev_inv);
    float4 *sq = reinterpret_cast<float4 *>(save_q);
    if (next_inv && next_off)
        k_rigid_fwd<true><<<nb, kRigBlock, 0, s>>>(F, k, means, quats, fg_rows, nbr_rows, weights, prev_off, pinv, partial,
                                                   save_u, save_m, sq, reinterpret_cast<float4 *>(next_inv), next_off);
    else
        k_rigid_fwd<false><<<nb, kRigBlock, 0, s>>>(F, k, means, quats, fg_rows, nbr_rows, weights, prev_off, pinv, partial,
                                                    save_u, save_m, sq, nullptr, nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_rigid_sum<<<1, 256, 0, s>>>(nb, partial, 1.0 / ((double)F * k), out_loss);
    return hipGetLastError();
}

hipError_t launch_foreground_info(int F, int k, const float *means, const float *quats, const int *fg_rows,
                                  const int *nbr_rows, float *out_inv, float *out_off, hipStream_t s) {
    k_foreground_info<<<rigid_blocks(F), kRigBlock, 0, s>>>(F, k, means, quats, fg_rows, nbr_rows,
                                                            reinterpret_cast<float4 *>(out_inv), out_off);
    return hipGetLastError();
}

hipError_t launch_rigid_bwd(int P, int F, int k, const int *row_to_fg, const int *rev_off, const int *rev_edge,
                            const float *save_u, const float *save_m, const float *save_q, const float *g_loss,
                            float *dmeans, float *dquats, hipStream_t s) {
    k_rigid_bwd<<<div_up(P, kRigBlock), kRigBlock, 0, s>>>(P, row_to_fg, rev_off, rev_edge, save_u, save_m,
                                                          reinterpret_cast<const float4 *>(save_q), g_loss,
                                                          (float)(1.0 / ((double)F * k)), dmeans, dquats);
    return hipGetLastError();
}

}  // namespace gsr
