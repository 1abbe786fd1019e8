// gsr_api_aux.hip -- C ABI of libgsr (declared in include/gsr.h): the entry points beside the
// rasterizer -- fused L1 + SSIM, k-nearest neighbours and the rigidity loss, the deformation network's
// input layer, residual blocks and output head, densification, fused Adam with the gradient norm and the
// camera-frame packing.
// Argument validation and workspace carving; the kernels are in gsr_loss.hip, gsr_rigidity.hip, gsr_deform.hip,
// gsr_resblock.hip, gsr_head.hip, gsr_densify.hip, gsr_adam.hip and gsr_io.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/gsr.h"
#include "gsr_common.h"
#include "gsr_internal.h"
#include "gsr_host.h"

using namespace gsr;

namespace {
struct SsimScratch {
    size_t maps, partial, total;
    SsimScratch(int planes, int H, int W) {
        const size_t n = (size_t)planes * H * W;
        maps = 0;
        partial = align256(sizeof(float) * 3 * n);
        total = align256(partial + sizeof(float2) * ssim_partials(planes, H, W));
    }
};

// The window of calc_ssim: gaussian(11, 1.5) (external.py:48-55) evaluates exp() in double, stores
// float32 and normalises by the float32 sum.
SsimWindow ssim_window() {
    SsimWindow w;
    float sum = 0.f;
    for (int x = 0; x < 11; ++x) {
        w.w[x] = (float)std::exp(-(double)((x - 5) * (x - 5)) / (2.0 * 1.5 * 1.5));
        sum += w.w[x];
    }
    for (int x = 0; x < 11; ++x) w.w[x] = w.w[x] / sum;
    return w;
}

int check_ssim(int planes, int H, int W, const float *img1, const float *img2) {
    if (planes < 0 || H < 0 || W < 0) return fail(GSR_ERR_ARG, "l1_ssim: negative size");
    if ((size_t)planes * H * W > 0 && (!img1 || !img2)) return fail(GSR_ERR_ARG, "l1_ssim: null image");
    if ((size_t)planes * H * W >= (size_t)1 << 31) return fail(GSR_ERR_UNSUPPORTED, "l1_ssim: image too large");
    if (planes > 65535) return fail(GSR_ERR_UNSUPPORTED, "l1_ssim: more than 65535 planes");
    return GSR_OK;
}

constexpr int kKnnMaxK = 32;
struct RigidScratch {
    size_t partial, save_m, save_q, save_u, total;
    RigidScratch(int F, int k, bool save) {
        const size_t f = (size_t)F;
        partial = 0;
        size_t o = align256(sizeof(double) * (size_t)rigid_blocks(F));
        save_m = o; if (save) o = align256(o + sizeof(float) * 3 * f);
        save_q = o; if (save) o = align256(o + sizeof(float) * 4 * f);
        save_u = o; if (save) o = align256(o + sizeof(float) * 3 * f * (size_t)k);
        total = o;
    }
};
int check_rigid(int P, int F, int k) {
    if (P < 0 || F < 0 || k < 0) return fail(GSR_ERR_ARG, "rigidity: negative size");
    if (F > P) return fail(GSR_ERR_ARG, "rigidity: %d foreground rows of %d Gaussians", F, P);
    if ((size_t)F * (size_t)k >= (size_t)1 << 31) return fail(GSR_ERR_UNSUPPORTED, "rigidity: more than 2^31 edges");
    return GSR_OK;
}
// the entry points that write a foreground state: a non-empty foreground and the neighbour search's k
int check_foreground(int P, int F, int k) {
    if (F <= 0) return fail(GSR_ERR_ARG, "foreground_info: F must be > 0 (got %d)", F);
    if (k < 1 || k > kKnnMaxK) return fail(GSR_ERR_ARG, "foreground_info: k = %d (1 to %d supported)", k, kKnnMaxK);
    return check_rigid(P, F, k);
}

// the deformation network's units: `what` is deform_in, resblock or deform_out
int check_blocks(const char *what, int max_blocks) {
    if (max_blocks < 0) return fail(GSR_ERR_ARG, "%s: max_blocks must be >= 0 (0: automatic)", what);
    return GSR_OK;
}

int check_layer(const char *what, int P, int H, int max_h) {
    if (P < 0) return fail(GSR_ERR_ARG, "%s: P must be >= 0", what);
    if (H < 1 || H > max_h) return fail(GSR_ERR_UNSUPPORTED, "%s: hidden dimension %d (1 to %d supported)", what, H, max_h);
    return GSR_OK;
}

int check_resblock(int P, int H, int max_blocks) {
    if (P < 2) return fail(GSR_ERR_ARG, "resblock: batch statistics need P >= 2 rows (got %d)", P);
    if (H < 1 || H > kResblockMaxH)
        return fail(GSR_ERR_ARG, "resblock: hidden dimension %d (1 to %d supported)", H, kResblockMaxH);
    return check_blocks("resblock", max_blocks);
}

int dens_args(const gsr_densify_settings *st, DensArgs &a) {
    if (!st) return fail(GSR_ERR_ARG, "densify: null settings");
    if (st->P < 0) return fail(GSR_ERR_ARG, "densify: P must be >= 0");
    if (st->P > 0 && (!st->grad_accum || !st->vis_count || !st->log_scales || !st->opacity_logits ||
                      !st->rotation_quaternions))
        return fail(GSR_ERR_ARG, "densify: statistics / log_scales / opacity_logits / rotations required");
    if (!(st->split_divisor > 0.f)) return fail(GSR_ERR_ARG, "densify: split_divisor must be > 0");
    a.P = st->P; a.prune_big = st->prune_big;
    a.grad_threshold = st->grad_threshold; a.small_scale = st->small_scale; a.big_scale = st->big_scale;
    a.remove_opacity = st->remove_opacity;
    // torch evaluates tensor / python-scalar on the GPU as tensor * (1 / scalar) in float
    a.inv_split_div = 1.0f / st->split_divisor;
    a.grad_accum = st->grad_accum; a.vis_count = st->vis_count; a.log_scales = st->log_scales;
    a.opacity_logits = st->opacity_logits; a.rotations = st->rotation_quaternions;
    return GSR_OK;
}

// fused Adam: the tensor list's checks (before anything is launched), and the launch table
constexpr long long kAdamMaxNumel = (1ll << 30) * kAdamPerBlock;  // 2^30 blocks, the most one launch takes
int check_adam(int ntensors, const gsr_adam_tensor *tensors) {
    if (ntensors < 0 || (ntensors > 0 && !tensors)) return fail(GSR_ERR_ARG, "adam: bad tensor list");
    for (int k = 0; k < ntensors; ++k) {
        const gsr_adam_tensor &a = tensors[k];
        if (a.numel < 0) return fail(GSR_ERR_ARG, "adam: tensor %d: negative numel", k);
        if (a.numel > 0 && (!a.param || !a.grad || !a.exp_avg || !a.exp_avg_sq))
            return fail(GSR_ERR_ARG, "adam: tensor %d: null pointer", k);
        if (a.numel > 0 && !(a.step >= 1.0)) return fail(GSR_ERR_ARG, "adam: tensor %d: step must be >= 1", k);
        if (a.numel > kAdamMaxNumel) return fail(GSR_ERR_UNSUPPORTED, "adam: tensor %d too large", k);
    }
    return GSR_OK;
}
void adam_table_reset(AdamTable &tab, double beta1, double beta2, double eps) {
    memset(&tab, 0, sizeof(tab));
    tab.w1 = (float)(1.0 - beta1);
    tab.b2 = (float)beta2;
    tab.omb2 = (float)(1.0 - beta2);
    tab.eps = (float)eps;
}
// the table's next entry: tensor `a`, whose first block is the table's block `nb`
void adam_table_add(AdamTable &tab, const gsr_adam_tensor &a, double beta1, double beta2, int nb) {
    const double bc1 = 1.0 - std::pow(beta1, a.step), bc2 = 1.0 - std::pow(beta2, a.step);
    AdamTensor &t = tab.t[tab.n];
    t.param = a.param; t.grad = a.grad; t.exp_avg = a.exp_avg; t.exp_avg_sq = a.exp_avg_sq;
    t.n = a.numel;
    t.step_size = (float)((a.lr / bc1) * -1.0);
    t.bc2_sqrt = (float)std::pow(bc2, 0.5);
    const uintptr_t al = (uintptr_t)a.param | (uintptr_t)a.grad | (uintptr_t)a.exp_avg | (uintptr_t)a.exp_avg_sq;
    t.vec4 = (al & 15) == 0;
    tab.block_start[tab.n] = nb;
    ++tab.n;
}

// The gradient norm's side of a call: the workspace (doubles: the total, one sum per slot, one partial per
// block of the call) and the table k_norm_final gets after each reducing launch.  A table takes up to
// kAdamMaxTensors tensors of the list, the empty ones included (they own a slot and no partials).
struct NormRun {
    hipStream_t s;
    double *total, *sums, *partials;
    float *out_sq, *out_norm;
    int last;
    NormFinal f;
    long long base = 0;  // blocks of the call's earlier tables
    int nb = 0;          // blocks of this table so far
    NormRun(hipStream_t s_, void *ws, int nslots, int last_, float *out_sq_, float *out_norm_)
        : s(s_), total((double *)ws), sums((double *)ws + 1), partials((double *)ws + 1 + nslots), out_sq(out_sq_),
          out_norm(out_norm_), last(last_) {
        memset(&f, 0, sizeof(f));
        f.nslots = nslots;
    }
    bool full(int blocks) const { return f.n == kAdamMaxTensors || nb + (long long)blocks > (1ll << 30); }
    double *table_partials() const { return partials + base; }
    void add(int slot, int blocks) {
        f.slot[f.n] = slot;
        f.part_start[f.n] = nb;
        nb += blocks;
        f.part_start[++f.n] = nb;
    }
    hipError_t flush(bool end_of_call) {
        f.last = end_of_call && last;
        hipError_t e = launch_norm_final(f, table_partials(), sums, total, out_sq, out_norm, s);
        base += nb;
        nb = 0;
        const int nslots = f.nslots;
        memset(&f, 0, sizeof(f));
        f.nslots = nslots;
        return e;
    }
};
}  // namespace

extern "C" {

// ---- fused L1 + SSIM ----------------------------------------------------------------------
size_t gsr_ssim_scratch_bytes(int planes, int H, int W) {
    return SsimScratch(planes < 0 ? 0 : planes, H < 0 ? 0 : H, W < 0 ? 0 : W).total;
}

int gsr_l1_ssim_forward(int planes, int H, int W, const float *img1, const float *img2, void *scratch,
                        float *out_l1, float *out_ssim, void *stream) {
    int rc = check_ssim(planes, H, W, img1, img2);
    if (rc) return rc;
    if (!out_l1 || !out_ssim) return fail(GSR_ERR_ARG, "l1_ssim: null output");
    if ((size_t)planes * H * W == 0) return fail(GSR_ERR_ARG, "l1_ssim: empty image (the mean is undefined)");
    if (!scratch) return fail(GSR_ERR_ARG, "l1_ssim: null scratch");
    hipStream_t s = (hipStream_t)stream;
    const SsimScratch L(planes, H, W);
    char *base = (char *)scratch;
    Phase ph(s, "ssim_fwd");
    HIP_TRY(launch_ssim_fwd(planes, H, W, img1, img2, ssim_window(), (float *)(base + L.maps),
                            (float2 *)(base + L.partial), out_l1, out_ssim, s));
    return GSR_OK;
}

int gsr_l1_ssim_backward(int planes, int H, int W, const float *img1, const float *img2, const void *scratch,
                         const float *dL_dl1, const float *dL_dssim, float *dL_dimg1, void *stream) {
    int rc = check_ssim(planes, H, W, img1, img2);
    if (rc) return rc;
    if ((size_t)planes * H * W == 0) return GSR_OK;
    if (!dL_dimg1 || !scratch) return fail(GSR_ERR_ARG, "l1_ssim: null gradient output / scratch");
    hipStream_t s = (hipStream_t)stream;
    const SsimScratch L(planes, H, W);
    Phase ph(s, "ssim_bwd");
    HIP_TRY(launch_ssim_bwd(planes, H, W, img1, img2, ssim_window(), (const float *)((const char *)scratch + L.maps),
                            dL_dl1, dL_dssim, dL_dimg1, s));
    return GSR_OK;
}

// ---- scores of a timestep's views (forward only) --------------------------------------------
size_t gsr_image_scores_workspace_bytes(int views, int planes, int H, int W) {
    if (views < 0 || planes < 0 || H < 0 || W < 0) return 0;
    return (size_t)views * (sizeof(float) * 3 * ssim_partials(planes, H, W));
}

int gsr_image_scores(int views, int planes, int H, int W, const float *const *img1, const float *const *img2,
                     void *workspace, float *out_scores, float *out_mean, void *stream) {
    if (views < 0 || planes < 0 || H < 0 || W < 0) return fail(GSR_ERR_ARG, "image_scores: negative size");
    if (views > 0 && (!img1 || !img2)) return fail(GSR_ERR_ARG, "image_scores: null image array");
    hipStream_t s = (hipStream_t)stream;
    if (views == 0) {  // the mean of an empty list
        if (out_mean) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)out_mean, 0x7FC00000, 1, s));
        return GSR_OK;
    }
    if ((size_t)planes * H * W == 0) return fail(GSR_ERR_ARG, "image_scores: empty image (the means are undefined)");
    if ((size_t)planes * H * W >= (size_t)1 << 31) return fail(GSR_ERR_UNSUPPORTED, "image_scores: image too large");
    if (planes > 65535) return fail(GSR_ERR_UNSUPPORTED, "image_scores: more than 65535 planes per view");
    for (int v = 0; v < views; ++v)
        if (!img1[v] || !img2[v]) return fail(GSR_ERR_ARG, "image_scores: null image (view %d)", v);
    if (!workspace || !out_scores) return fail(GSR_ERR_ARG, "image_scores: null workspace / output");
    Phase ph(s, "image_scores");
    HIP_TRY(launch_image_scores(views, planes, H, W, img1, img2, ssim_window(), (float *)workspace, out_scores,
                                out_mean, s));
    return GSR_OK;
}

// ---- rigidity loss + k-nearest neighbours ---------------------------------------------------
int gsr_knn(int n, const float *points, int k, int *out_indices, double *out_sq_distances, void *stream) {
    if (n < 0 || k < 1) return fail(GSR_ERR_ARG, "knn: n must be >= 0 and k >= 1 (got n = %d, k = %d)", n, k);
    if (k > kKnnMaxK) return fail(GSR_ERR_UNSUPPORTED, "knn: k = %d (at most %d supported)", k, kKnnMaxK);
    if (n <= k) return fail(GSR_ERR_ARG, "knn: %d points have no %d other points each", n, k);
    if ((size_t)n * (size_t)k >= (size_t)1 << 31) return fail(GSR_ERR_UNSUPPORTED, "knn: more than 2^31 results");
    if (!points || !out_indices || !out_sq_distances) return fail(GSR_ERR_ARG, "knn: null pointer");
    hipStream_t s = (hipStream_t)stream;
    Phase ph(s, "knn");
    HIP_TRY(launch_knn(n, points, k, out_indices, out_sq_distances, s));
    return GSR_OK;
}

size_t gsr_rigidity_scratch_bytes(int F, int k, int save_for_backward) {
    return RigidScratch(F < 0 ? 0 : F, k < 0 ? 0 : k, save_for_backward != 0).total;
}

// gsr_rigidity_forward, and with next_* (both) gsr_rigidity_forward_state
static int rigidity_forward(int P, int F, int k, const float *means, const float *rotation_quaternions,
                            const int *foreground_rows, const int *neighbor_rows, const float *weights,
                            const float *previous_offsets, const float *previous_inverted_rotations, void *scratch,
                            int save_for_backward, float *out_loss, float *next_inv, float *next_off, void *stream) {
    int rc = check_rigid(P, F, k);
    if (rc) return rc;
    if (F == 0 || k == 0) return fail(GSR_ERR_ARG, "rigidity: no foreground edges (the mean is undefined)");
    if (!means || !rotation_quaternions || !foreground_rows || !neighbor_rows || !weights || !previous_offsets ||
        !previous_inverted_rotations || !scratch || !out_loss)
        return fail(GSR_ERR_ARG, "rigidity: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const RigidScratch L(F, k, save_for_backward != 0);
    char *base = (char *)scratch;
    const bool sv = save_for_backward != 0;
    Phase ph(s, "rigidity_fwd");
    HIP_TRY(launch_rigid_fwd(F, k, means, rotation_quaternions, foreground_rows, neighbor_rows, weights,
                             previous_offsets, previous_inverted_rotations, (double *)(base + L.partial),
                             sv ? (float *)(base + L.save_u) : nullptr, sv ? (float *)(base + L.save_m) : nullptr,
                             sv ? (float *)(base + L.save_q) : nullptr, out_loss, next_inv, next_off, s));
    return GSR_OK;
}

int gsr_rigidity_forward(int P, int F, int k, const float *means, const float *rotation_quaternions,
                         const int *foreground_rows, const int *neighbor_rows, const float *weights,
                         const float *previous_offsets, const float *previous_inverted_rotations, void *scratch,
                         int save_for_backward, float *out_loss, void *stream) {
    return rigidity_forward(P, F, k, means, rotation_quaternions, foreground_rows, neighbor_rows, weights,
                            previous_offsets, previous_inverted_rotations, scratch, save_for_backward, out_loss, nullptr,
                            nullptr, stream);
}

int gsr_rigidity_forward_state(int P, int F, int k, const float *means, const float *rotation_quaternions,
                               const int *foreground_rows, const int *neighbor_rows, const float *weights,
                               const float *previous_offsets, const float *previous_inverted_rotations, void *scratch,
                               int save_for_backward, float *out_loss, float *next_inverted_rotations,
                               float *next_offsets, void *stream) {
    int rc = check_foreground(P, F, k);
    if (rc) return rc;
    if (!next_inverted_rotations || !next_offsets)
        return fail(GSR_ERR_ARG, "rigidity: the state outputs are both required (gsr_rigidity_forward computes none)");
    return rigidity_forward(P, F, k, means, rotation_quaternions, foreground_rows, neighbor_rows, weights,
                            previous_offsets, previous_inverted_rotations, scratch, save_for_backward, out_loss,
                            next_inverted_rotations, next_offsets, stream);
}

int gsr_foreground_info(int P, int F, int k, const float *means, const float *rotation_quaternions,
                        const int *foreground_rows, const int *neighbor_rows, float *out_inverted_rotations,
                        float *out_offsets, void *stream) {
    int rc = check_foreground(P, F, k);
    if (rc) return rc;
    if (!foreground_rows || (out_inverted_rotations && !rotation_quaternions) ||
        (out_offsets && (!means || !neighbor_rows)))
        return fail(GSR_ERR_ARG, "foreground_info: null pointer");
    if (!out_inverted_rotations && !out_offsets) return GSR_OK;
    hipStream_t s = (hipStream_t)stream;
    Phase ph(s, "foreground_info");
    HIP_TRY(launch_foreground_info(F, k, means, rotation_quaternions, foreground_rows, neighbor_rows,
                                   out_inverted_rotations, out_offsets, s));
    return GSR_OK;
}

int gsr_rigidity_backward(int P, int F, int k, const int *row_to_foreground, const int *reverse_offsets,
                          const int *reverse_edges, const void *scratch, const float *dL_dloss, float *dL_dmeans,
                          float *dL_drotation_quaternions, void *stream) {
    int rc = check_rigid(P, F, k);
    if (rc) return rc;
    if (P == 0 || (!dL_dmeans && !dL_drotation_quaternions)) return GSR_OK;
    if (F == 0 || k == 0) return fail(GSR_ERR_ARG, "rigidity: no foreground edges");
    if (!row_to_foreground || !reverse_offsets || !reverse_edges || !scratch || !dL_dloss)
        return fail(GSR_ERR_ARG, "rigidity: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const RigidScratch L(F, k, true);
    const char *base = (const char *)scratch;
    Phase ph(s, "rigidity_bwd");
    HIP_TRY(launch_rigid_bwd(P, F, k, row_to_foreground, reverse_offsets, reverse_edges,
                             (const float *)(base + L.save_u), (const float *)(base + L.save_m),
                             (const float *)(base + L.save_q), dL_dloss, dL_dmeans, dL_drotation_quaternions, s));
    return GSR_OK;
}

// ---- deformation network input layer ----------------------------------------------------------
static_assert(kPosencRangeBlocks == GSR_POSENC_RANGE_BLOCKS, "the header's workspace size follows the kernel's grid");

int gsr_posenc_ranges(int P, const float *means, const float *rotation_quaternions, float *partial,
                      float *out_ranges, void *stream) {
    if (P < 1) return fail(GSR_ERR_ARG, "posenc: the ranges of an empty cloud are undefined (P = %d)", P);
    if (!means || !rotation_quaternions || !partial || !out_ranges) return fail(GSR_ERR_ARG, "posenc: null pointer");
    hipStream_t s = (hipStream_t)stream;
    Phase ph(s, "posenc_ranges");
    HIP_TRY(launch_posenc_ranges(P, means, rotation_quaternions, partial, out_ranges, s));
    return GSR_OK;
}

int gsr_posenc_forward(int P, const float *means, const float *rotation_quaternions, const float *ranges,
                       float *out_encoding, void *stream) {
    if (P < 0) return fail(GSR_ERR_ARG, "posenc: P must be >= 0");
    if (P == 0) return GSR_OK;
    if (!means || !rotation_quaternions || !ranges || !out_encoding) return fail(GSR_ERR_ARG, "posenc: null pointer");
    hipStream_t s = (hipStream_t)stream;
    Phase ph(s, "posenc");
    HIP_TRY(launch_posenc(P, means, rotation_quaternions, ranges, out_encoding, s));
    return GSR_OK;
}

int gsr_deform_in_forward(int P, int H, const float *initial_means, const float *initial_rotation_quaternions,
                          const float *initial_ranges, const float *previous_means,
                          const float *previous_rotation_quaternions, const float *previous_ranges, float progress,
                          const float *weight, const float *bias, float *out, void *stream) {
    int rc = check_layer("deform_in", P, H, kDeformMaxH);
    if (rc) return rc;
    if (P == 0) return GSR_OK;
    if (!initial_means || !initial_rotation_quaternions || !initial_ranges || !previous_means ||
        !previous_rotation_quaternions || !previous_ranges || !weight || !bias || !out)
        return fail(GSR_ERR_ARG, "deform_in: null pointer");
    hipStream_t s = (hipStream_t)stream;
    Phase ph(s, "deform_in_fwd");
    HIP_TRY(launch_deform_in_fwd(P, H, initial_means, initial_rotation_quaternions, initial_ranges, previous_means,
                                 previous_rotation_quaternions, previous_ranges, progress, weight, bias, out, s));
    return GSR_OK;
}

size_t gsr_deform_in_workspace_bytes(int P, int H, int max_blocks) {
    if (P <= 0 || H <= 0) return 0;
    return align256(sizeof(float) * deform_in_partial_floats(P, H, max_blocks));
}

int gsr_deform_in_backward(int P, int H, const float *initial_means, const float *initial_rotation_quaternions,
                           const float *initial_ranges, const float *previous_means,
                           const float *previous_rotation_quaternions, const float *previous_ranges, float progress,
                           const float *dL_dout, void *workspace, int max_blocks, float *dL_dweight,
                           float *dL_dbias, void *stream) {
    int rc = check_layer("deform_in", P, H, kDeformMaxH);
    if (!rc) rc = check_blocks("deform_in", max_blocks);
    if (rc) return rc;
    if (!dL_dweight && !dL_dbias) return GSR_OK;
    if (P == 0) return fail(GSR_ERR_ARG, "deform_in: no rows to sum the gradient over");
    if (!initial_means || !initial_rotation_quaternions || !initial_ranges || !previous_means ||
        !previous_rotation_quaternions || !previous_ranges || !dL_dout || !workspace)
        return fail(GSR_ERR_ARG, "deform_in: null pointer");
    hipStream_t s = (hipStream_t)stream;
    Phase ph(s, "deform_in_bwd");
    HIP_TRY(launch_deform_in_bwd(P, H, initial_means, initial_rotation_quaternions, initial_ranges, previous_means,
                                 previous_rotation_quaternions, previous_ranges, progress, dL_dout, (float *)workspace,
                                 max_blocks, dL_dweight, dL_dbias, s));
    return GSR_OK;
}

// ---- deformation network residual blocks ------------------------------------------------------
size_t gsr_resblock_workspace_bytes(int P, int H, int max_blocks, int backward) {
    if (P < 2 || H < 1 || H > kResblockMaxH || max_blocks < 0) return 0;
    return ResblockWorkspace(P, H, max_blocks, backward != 0).total;
}

int gsr_resblock_forward(int P, int H, const float *x, const float *fc1_weight, const float *bn1_weight,
                         const float *bn1_bias, const float *fc2_weight, const float *bn2_weight,
                         const float *bn2_bias, float eps1, float eps2, float momentum1, float momentum2,
                         float *bn1_running_mean, float *bn1_running_var, float *bn2_running_mean,
                         float *bn2_running_var, void *workspace, int max_blocks, float *y1, float *y2, float *out,
                         float *stats, void *stream) {
    int rc = check_resblock(P, H, max_blocks);
    if (rc) return rc;
    if (!x || !fc1_weight || !bn1_weight || !bn1_bias || !fc2_weight || !bn2_weight || !bn2_bias || !workspace ||
        !y1 || !y2 || !out || !stats)
        return fail(GSR_ERR_ARG, "resblock: null pointer");
    hipStream_t s = (hipStream_t)stream;
    Phase ph(s, "resblock_fwd");
    HIP_TRY(launch_resblock_fwd(P, H, x, fc1_weight, bn1_weight, bn1_bias, fc2_weight, bn2_weight, bn2_bias, eps1, eps2,
                                momentum1, momentum2, bn1_running_mean, bn1_running_var, bn2_running_mean,
                                bn2_running_var, (char *)workspace, max_blocks, y1, y2, out, stats, s));
    return GSR_OK;
}

int gsr_resblock_backward(int P, int H, const float *x, const float *y1, const float *y2, const float *stats,
                          const float *fc1_weight, const float *bn1_weight, const float *bn1_bias,
                          const float *fc2_weight, const float *bn2_weight, const float *bn2_bias,
                          const float *dL_dout, void *workspace, int max_blocks, float *dL_dx, float *dL_dfc1_weight,
                          float *dL_dbn1_weight, float *dL_dbn1_bias, float *dL_dfc2_weight, float *dL_dbn2_weight,
                          float *dL_dbn2_bias, void *stream) {
    int rc = check_resblock(P, H, max_blocks);
    if (rc) return rc;
    if (!dL_dx && !dL_dfc1_weight && !dL_dbn1_weight && !dL_dbn1_bias && !dL_dfc2_weight && !dL_dbn2_weight &&
        !dL_dbn2_bias)
        return GSR_OK;
    if (!x || !y1 || !y2 || !stats || !fc1_weight || !bn1_weight || !bn1_bias || !fc2_weight || !bn2_weight ||
        !bn2_bias || !dL_dout || !workspace)
        return fail(GSR_ERR_ARG, "resblock: null pointer");
    hipStream_t s = (hipStream_t)stream;
    Phase ph(s, "resblock_bwd");
    HIP_TRY(launch_resblock_bwd(P, H, x, y1, y2, stats, fc1_weight, bn1_weight, bn1_bias, fc2_weight, bn2_weight,
                                bn2_bias, dL_dout, (char *)workspace, max_blocks, dL_dx, dL_dfc1_weight, dL_dbn1_weight,
                                dL_dbn1_bias, dL_dfc2_weight, dL_dbn2_weight, dL_dbn2_bias, s));
    return GSR_OK;
}

// ---- deformation network output head ----------------------------------------------------------
int gsr_deform_out_forward(int P, int H, const float *x, const float *weight, const float *bias,
                           const float *initial_means, const float *initial_rotation_quaternions, float *out,
                           void *stream) {
    int rc = check_layer("deform_out", P, H, kHeadMaxH);
    if (rc) return rc;
    if (P == 0) return GSR_OK;
    if (!x || !weight || !bias || !initial_means || !initial_rotation_quaternions || !out)
        return fail(GSR_ERR_ARG, "deform_out: null pointer");
    hipStream_t s = (hipStream_t)stream;
    Phase ph(s, "deform_out_fwd");
    HIP_TRY(launch_head_fwd(P, H, x, weight, bias, initial_means, initial_rotation_quaternions, out, s));
    return GSR_OK;
}

size_t gsr_deform_out_workspace_bytes(int P, int H, int max_blocks) {
    if (P <= 0 || H < 1 || H > kHeadMaxH || max_blocks < 0) return 0;
    return align256(sizeof(float) * head_partial_floats(P, H, max_blocks));
}

int gsr_deform_out_backward(int P, int H, const float *x, const float *weight, const float *dL_dout, void *workspace,
                            int max_blocks, float *dL_dx, float *dL_dweight, float *dL_dbias, void *stream) {
    int rc = check_layer("deform_out", P, H, kHeadMaxH);
    if (!rc) rc = check_blocks("deform_out", max_blocks);
    if (rc) return rc;
    if (!dL_dx && !dL_dweight && !dL_dbias) return GSR_OK;
    hipStream_t s = (hipStream_t)stream;
    if (P == 0) {  // empty sums: no kernel
        if (dL_dweight) HIP_TRY(hipMemsetAsync(dL_dweight, 0, sizeof(float) * 7 * (size_t)H, s));
        if (dL_dbias) HIP_TRY(hipMemsetAsync(dL_dbias, 0, sizeof(float) * 7, s));
        return GSR_OK;
    }
    if (!dL_dout || (dL_dx && !weight) || (dL_dweight && !x) || ((dL_dweight || dL_dbias) && !workspace))
        return fail(GSR_ERR_ARG, "deform_out: null pointer");
    Phase ph(s, "deform_out_bwd");
    HIP_TRY(launch_head_bwd(P, H, x, weight, dL_dout, (float *)workspace, max_blocks, dL_dx, dL_dweight, dL_dbias, s));
    return GSR_OK;
}

// ---- densification --------------------------------------------------------------------------
int gsr_densify_update_radii(int P, const int *radii, float *max_radii, uint8_t *visible, void *stream) {
    if (P < 0) return fail(GSR_ERR_ARG, "densify: P must be >= 0");
    if (P > 0 && (!radii || !max_radii || !visible)) return fail(GSR_ERR_ARG, "densify: null pointer");
    HIP_TRY(launch_dens_radii(P, radii, max_radii, visible, (hipStream_t)stream));
    return GSR_OK;
}

int gsr_densify_accumulate_grads(int P, const uint8_t *visible, const float *means2D_grad, float *grad_accum,
                                 float *vis_count, void *stream) {
    if (P < 0) return fail(GSR_ERR_ARG, "densify: P must be >= 0");
    if (P > 0 && (!visible || !means2D_grad || !grad_accum || !vis_count))
        return fail(GSR_ERR_ARG, "densify: null pointer");
    HIP_TRY(launch_dens_grads(P, visible, means2D_grad, grad_accum, vis_count, (hipStream_t)stream));
    return GSR_OK;
}

size_t gsr_densify_workspace_bytes(int P) { return DensWorkspace(P < 0 ? 0 : P).total; }

int gsr_densify_plan(const gsr_densify_settings *st, void *workspace, gsr_densify_counts *counts, void *stream) {
    DensArgs a;
    int rc = dens_args(st, a);
    if (rc) return rc;
    if (!workspace || !counts) return fail(GSR_ERR_ARG, "densify: null workspace / counts");
    memset(counts, 0, sizeof(*counts));
    if (a.P == 0) return GSR_OK;
    hipStream_t s = (hipStream_t)stream;
    const DensWorkspace L(a.P);
    { Phase ph(s, "densify_plan"); HIP_TRY(launch_dens_plan(a, (char *)workspace, s)); }
    uint32_t tot[4];
    HIP_TRY(hipMemcpyAsync(tot, (char *)workspace + L.totals, sizeof(tot), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    counts->n_keep_orig = (int)tot[0];
    counts->n_keep_clone = (int)tot[1];
    counts->n_split = (int)tot[2];
    counts->n_keep_split = (int)tot[3];
    const long long po = (long long)tot[0] + tot[1] + 2ll * tot[3];
    if (po > 0x7FFFFFFF) return fail(GSR_ERR_UNSUPPORTED, "densify: output too large");
    counts->P_out = (int)po;
    return GSR_OK;
}

int gsr_densify_split_stds(const gsr_densify_settings *st, const void *workspace, float *stds, void *stream) {
    DensArgs a;
    int rc = dens_args(st, a);
    if (rc) return rc;
    if (a.P == 0) return GSR_OK;
    if (!workspace || !stds) return fail(GSR_ERR_ARG, "densify: null workspace / stds");
    HIP_TRY(launch_dens_stds(a, (const char *)workspace, stds, (hipStream_t)stream));
    return GSR_OK;
}

int gsr_densify_apply(const gsr_densify_settings *st, const void *workspace, const gsr_densify_counts *counts,
                      const float *samples, int ncols, const gsr_densify_column *cols, void *stream) {
    DensArgs a;
    int rc = dens_args(st, a);
    if (rc) return rc;
    if (ncols < 0 || ncols > kDensMaxColumns) return fail(GSR_ERR_ARG, "densify: 0..%d columns", kDensMaxColumns);
    if (a.P == 0 || ncols == 0) return GSR_OK;
    if (!workspace || !cols || !counts) return fail(GSR_ERR_ARG, "densify: null workspace / counts / columns");
    if (counts->n_split > 0 && !samples) return fail(GSR_ERR_ARG, "densify: %d splits need samples", counts->n_split);
    DensColumns dc;
    memset(&dc, 0, sizeof(dc));
    dc.n = ncols;
    for (int k = 0; k < ncols; ++k) {
        const gsr_densify_column &c = cols[k];
        if (c.width <= 0 || !c.src || !c.dst) return fail(GSR_ERR_ARG, "densify: column %d has no data", k);
        if ((c.exp_avg == nullptr) != (c.exp_avg_sq == nullptr) || (c.exp_avg == nullptr) != (c.dst_exp_avg == nullptr) ||
            (c.dst_exp_avg == nullptr) != (c.dst_exp_avg_sq == nullptr))
            return fail(GSR_ERR_ARG, "densify: column %d: Adam moments must be given together", k);
        if (c.role == GSR_DENS_MEANS && c.width != 3) return fail(GSR_ERR_ARG, "densify: means need width 3");
        if (c.role == GSR_DENS_LOG_SCALES && c.width != 3) return fail(GSR_ERR_ARG, "densify: log_scales need width 3");
        dc.c[k] = DensColumn{c.width, c.role, c.src, c.exp_avg, c.exp_avg_sq, c.dst, c.dst_exp_avg, c.dst_exp_avg_sq};
    }
    hipStream_t s = (hipStream_t)stream;
    Phase ph(s, "densify_apply");
    HIP_TRY(launch_dens_apply(a, (const char *)workspace, samples, dc, s));
    return GSR_OK;
}

int gsr_adam_step(int ntensors, const gsr_adam_tensor *tensors, double beta1, double beta2, double eps,
                  void *stream) {
    int rc = check_adam(ntensors, tensors);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    Phase ph(s, "adam");
    AdamTable tab;
    adam_table_reset(tab, beta1, beta2, eps);
    int nb = 0;
    for (int k = 0; k < ntensors; ++k) {
        const gsr_adam_tensor &a = tensors[k];
        if (a.numel == 0) continue;
        const int b = adam_blocks(a.numel);
        if (tab.n == kAdamMaxTensors || nb + (long long)b > (1ll << 30)) {  // table full: launch it
            tab.block_start[tab.n] = nb;
            HIP_TRY(launch_adam(tab, s));
            adam_table_reset(tab, beta1, beta2, eps);
            nb = 0;
        }
        adam_table_add(tab, a, beta1, beta2, nb);
        nb += b;
    }
    if (tab.n) {
        tab.block_start[tab.n] = nb;
        HIP_TRY(launch_adam(tab, s));
    }
    return GSR_OK;
}

// ---- gradient norm --------------------------------------------------------------------------------
size_t gsr_grad_norm_workspace_bytes(int ntensors, const long long *numels) {
    if (ntensors < 0 || (ntensors > 0 && !numels)) return 0;
    size_t doubles = 1 + (size_t)ntensors;
    for (int k = 0; k < ntensors; ++k) {
        if (numels[k] < 0) return 0;
        doubles += (size_t)(numels[k] / kAdamPerBlock) + (numels[k] % kAdamPerBlock != 0);
    }
    return sizeof(double) * doubles;
}

int gsr_grad_norm(int ntensors, const gsr_grad_tensor *tensors, void *workspace, float *out_sqnorms,
                  float *out_norm, void *stream) {
    if (ntensors < 0 || (ntensors > 0 && !tensors)) return fail(GSR_ERR_ARG, "grad_norm: bad tensor list");
    for (int k = 0; k < ntensors; ++k) {  // validate everything before launching anything
        if (tensors[k].numel < 0) return fail(GSR_ERR_ARG, "grad_norm: tensor %d: negative numel", k);
        if (tensors[k].numel > 0 && !tensors[k].grad) return fail(GSR_ERR_ARG, "grad_norm: tensor %d: null gradient", k);
        if (tensors[k].numel > kAdamMaxNumel) return fail(GSR_ERR_UNSUPPORTED, "grad_norm: tensor %d too large", k);
    }
    if (!workspace || !out_norm) return fail(GSR_ERR_ARG, "grad_norm: null workspace / out_norm");
    hipStream_t s = (hipStream_t)stream;
    Phase ph(s, "grad_norm");
    if (ntensors == 0) {  // the norm of nothing
        HIP_TRY(hipMemsetAsync(out_norm, 0, sizeof(float), s));
        return GSR_OK;
    }
    NormRun run(s, workspace, ntensors, 1, out_sqnorms, out_norm);
    NormTable tab;
    memset(&tab, 0, sizeof(tab));
    for (int k = 0; k < ntensors; ++k) {
        const gsr_grad_tensor &a = tensors[k];
        const int b = adam_blocks(a.numel);
        if (run.full(b)) {  // table full: reduce it, sum its tensors
            tab.block_start[tab.n] = run.nb;
            HIP_TRY(launch_grad_sumsq(tab, run.table_partials(), s));
            HIP_TRY(run.flush(false));
            memset(&tab, 0, sizeof(tab));
        }
        if (a.numel > 0) {
            tab.t[tab.n] = NormTensor{a.grad, a.numel, ((uintptr_t)a.grad & 15) == 0};
            tab.block_start[tab.n++] = run.nb;
        }
        run.add(k, b);
    }
    tab.block_start[tab.n] = run.nb;
    HIP_TRY(launch_grad_sumsq(tab, run.table_partials(), s));
    HIP_TRY(run.flush(true));
    return GSR_OK;
}

int gsr_adam_step_norm(int ntensors, const gsr_adam_tensor *tensors, double beta1, double beta2, double eps,
                       void *workspace, const int *slots, int nslots, int last, float *out_sqnorms,
                       float *out_norm, void *stream) {
    int rc = check_adam(ntensors, tensors);
    if (rc) return rc;
    if (nslots < 0 || (!slots && ntensors > nslots))
        return fail(GSR_ERR_ARG, "adam_norm: %d tensors but %d slots", ntensors, nslots);
    for (int k = 0; slots && k < ntensors; ++k)
        if (slots[k] < 0 || slots[k] >= nslots)
            return fail(GSR_ERR_ARG, "adam_norm: tensor %d: slot %d outside [0, %d)", k, slots[k], nslots);
    if (!workspace || !out_norm) return fail(GSR_ERR_ARG, "adam_norm: null workspace / out_norm");
    hipStream_t s = (hipStream_t)stream;
    Phase ph(s, "adam");
    if (nslots == 0) {  // the norm of nothing
        if (last) HIP_TRY(hipMemsetAsync(out_norm, 0, sizeof(float), s));
        return GSR_OK;
    }
    NormRun run(s, workspace, nslots, last, out_sqnorms, out_norm);
    AdamTable tab;
    adam_table_reset(tab, beta1, beta2, eps);
    for (int k = 0; k < ntensors; ++k) {
        const gsr_adam_tensor &a = tensors[k];
        const int b = adam_blocks(a.numel);
        if (run.full(b)) {  // table full: update it, sum its tensors
            tab.block_start[tab.n] = run.nb;
            HIP_TRY(launch_adam_norm(tab, run.table_partials(), s));
            HIP_TRY(run.flush(false));
            adam_table_reset(tab, beta1, beta2, eps);
        }
        if (a.numel > 0) adam_table_add(tab, a, beta1, beta2, run.nb);
        run.add(slots ? slots[k] : k, b);
    }
    tab.block_start[tab.n] = run.nb;
    HIP_TRY(launch_adam_norm(tab, run.table_partials(), s));
    if (run.f.n || last) HIP_TRY(run.flush(true));
    return GSR_OK;
}

int gsr_views_pack(int frames, int H, int W, const uint8_t *rgb, const uint8_t *seg, float *images,
                   float *seg_masks, void *stream) {
    if (frames < 0 || H < 0 || W < 0) return fail(GSR_ERR_ARG, "views_pack: negative size");
    if (frames == 0 || H == 0 || W == 0) return GSR_OK;
    if ((long long)H * W > (1ll << 29)) return fail(GSR_ERR_UNSUPPORTED, "views_pack: frame of %d x %d too large", H, W);
    if (frames > 65535) return fail(GSR_ERR_UNSUPPORTED, "views_pack: more than 65535 frames in one call");
    if (!rgb || !images) return fail(GSR_ERR_ARG, "views_pack: null rgb / images");
    if ((seg == nullptr) != (seg_masks == nullptr))
        return fail(GSR_ERR_ARG, "views_pack: seg and seg_masks must be given together");
    const int HW = H * W;
    if (HW % 4 == 0) {  // the vector path's alignment contract
        if (((uintptr_t)rgb & 3) || (seg && ((uintptr_t)seg & 3)) || ((uintptr_t)images & 15) ||
            (seg_masks && ((uintptr_t)seg_masks & 15)))
            return fail(GSR_ERR_ARG, "views_pack: rgb / seg must be 4-byte and outputs 16-byte aligned");
    }
    hipStream_t s = (hipStream_t)stream;
    Phase ph(s, "views_pack");
    HIP_TRY(launch_views_pack(frames, HW, rgb, seg, images, seg_masks, s));
    return GSR_OK;
}

int gsr_frames_pack(int frames, int H, int W, const float *images, uint8_t *rgb, void *stream) {
    if (frames < 0 || H < 0 || W < 0) return fail(GSR_ERR_ARG, "frames_pack: negative size");
    if (frames == 0 || H == 0 || W == 0) return GSR_OK;
    if ((long long)H * W > (1ll << 29)) return fail(GSR_ERR_UNSUPPORTED, "frames_pack: frame of %d x %d too large", H, W);
    if (!images || !rgb) return fail(GSR_ERR_ARG, "frames_pack: null images / rgb");
    hipStream_t s = (hipStream_t)stream;
    Phase ph(s, "frames_pack");
    HIP_TRY(launch_frames_pack(frames, H * W, images, rgb, s));
    return GSR_OK;
}

}  // extern "C"
