// gsr_internal.h -- argument bundles and host launchers shared by the libgsr translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {

// One view's inputs, shared by the forward's and the backward's argument bundles: the frame and its
// tile grid, the camera, and the Gaussians' parameter arrays (opacities: the forward only).
struct ViewIn {
    int P, D, M, W, H, gx, gy, act;
    float scale_modifier, tan_fovx, tan_fovy, focal_x, focal_y;
    const float *means3D, *scales, *rotations, *opacities, *shs, *colors_precomp, *cov3D_precomp;
    const float *viewmatrix, *projmatrix, *campos, *bg;
    CamStrides cs;
};

struct FwdArgs {
    ViewIn v;
    // geom
    float *depth; float4 *rec; uint2 *rect; uint32_t *tiles; uint32_t *goff; uint8_t *clampm;
    // image
    uint2 *ranges; float4 *pix_end; uint32_t *n_contrib; uint32_t *tile_maxc;
    uint32_t *tile_order_f; uint32_t *seg_off; uint32_t *sort_lists; uint32_t *tile_count;
    uint32_t *tile_cursor; uint32_t *block_sums; uint32_t *block_off; uint32_t *meta; uint32_t *chunk_off;
    uint32_t *items_ws; uint32_t *scan_ws; uint32_t *tile_rank;
    // exact-threshold mode: per tile, the count of near-threshold weights k_render_fwd re-evaluated, and
    // their records (kNearCap per tile: key (list position << 8 | pixel), power, G, alpha)
    uint32_t *tile_flag; float4 *near_rec;
    // exact-threshold mode: pixels whose final T lies within t_window of 1e-4, redone by k_render_tsat
    // (count in items_ws[kTSatCtr])
    uint32_t *tsat_list;
    // binning
    uint4 *pairs; uint32_t *point_list; uint32_t *slot_emit; float4 *seg_state;
    // outputs
    int *radii; float *out_color; float *out_depth;
    // speculative enqueue (gsr_forward_info with speculate): the BINNING capacity the post-scan kernels
    // were queued with before the host read K (0: exact path), and the device flag they check
    // (meta + 1, written by k_bin_scan; nullptr: exact path)
    uint32_t spec_cap; const uint32_t *spec_ok;
    uint32_t spec_sort_blocks;  // grid of the speculative k_tile_sort (<= kSpecSortBlocks; 0: that bound)
    // asynchronous forward (gsr_forward_async): the gate word the speculative render's first wave waits
    // on when the speculation failed, the value that opens it, the forward's timeout error word (set to
    // gate_seq when the gate is abandoned) and the timeout (s_memrealtime ticks, 100 MHz)
    const uint32_t *gate; uint32_t gate_seq; uint32_t *gate_err; uint64_t gate_timeout;
    // exact-threshold mode (gsr_set_exact_thresholds, on by default): near-threshold weights
    // re-evaluated in the reference's expression order
    int exact;
};
// blocks of the speculative k_tile_sort launch (they loop over the device-side list count)
constexpr int kSpecSortBlocks = 512;

// The per-Gaussian gradient outputs the two backward kernels share (NULL: not requested) and the
// gsr_grad_bits of the outputs added into instead of overwritten (gsr_grads.accumulate).
struct GaussGrads {
    float *dL_dcolors, *dL_dopacity, *dL_dmeans3D, *dL_dcov3D, *dL_dsh, *dL_dscales, *dL_drot;
    int accm;
};

struct BwdArgs : GaussGrads {
    ViewIn v;
    int K;
    const int *radii;
    // saved state
    const float4 *rec; const uint2 *rect; const uint8_t *clampm;
    const uint32_t *goff; const uint2 *ranges; const float4 *pix_end; const uint32_t *n_contrib;
    const uint32_t *tile_maxc; const uint32_t *tile_flag; const float4 *near_rec; const uint32_t *seg_off; const uint32_t *meta; uint32_t *items_ws;
    const uint32_t *point_list; const uint32_t *slot_emit; const float4 *seg_state;
    uint2 *items; uint32_t max_items;
    // scratch
    float4 *part;
    // upstream gradient
    const float *dL_dcolor;
    float *dL_dmeans2D;  // the screen-space output (the others: GaussGrads)
    const uint32_t *spec_ok;  // speculative render half (pair count unknown): kernels return when the forward's speculation failed
};

hipError_t launch_preprocess(const FwdArgs &a, hipStream_t s);
hipError_t launch_bin_count(const FwdArgs &a, hipStream_t s);
hipError_t launch_bin_scan(const FwdArgs &a, uint32_t *host_words, hipStream_t s);
hipError_t launch_bin_emit(const FwdArgs &a, int K, hipStream_t s);
hipError_t launch_tile_sort(const FwdArgs &a, uint32_t n_mid, uint32_t n_vlong, uint32_t max_n, uint4 *tmp,
                            hipStream_t s);
hipError_t launch_render_fwd(const FwdArgs &a, hipStream_t s);
hipError_t launch_zero(float *p, size_t n, hipStream_t s);
hipError_t launch_mark_visible(int P, const float *means3D, const float *viewmatrix, uint8_t *present,
                               hipStream_t s);

hipError_t launch_bwd_items(const BwdArgs &a, hipStream_t s);
hipError_t launch_bwd_items_raw(int K, int T, int P, const uint2 *ranges, const uint32_t *tile_maxc,
                                const uint32_t *tile_flag, uint2 *items, uint32_t *ws, hipStream_t s,
                                const uint32_t *spec_ok = nullptr);
hipError_t launch_render_bwd(const BwdArgs &a, hipStream_t s);
hipError_t launch_gauss_bwd(const BwdArgs &a, hipStream_t s);
// Each Gaussian's per-pair records of one view summed in emission order into kPartial x P SoA sums
// (the deferred multi-view pass reads these instead of walking the records itself).
hipError_t launch_sum_records(int P, const uint32_t *goff, const float4 *part, float *sums, hipStream_t s,
                              const uint32_t *spec_ok, const float *viewmatrix, const float *projmatrix,
                              const float *campos, CamStrides cs, int W, int H);

// Per-Gaussian backward over several views of the same Gaussians (gsr_backward_gaussians): one
// launch reads the parameters and read-modify-writes every gradient once for up to kMultiViews views.
constexpr int kMultiViews = 8;
struct MultiView {
    const float *viewmatrix, *projmatrix, *campos;
    CamStrides cs;
    float tan_fovx, tan_fovy, focal_x, focal_y;
    const int *radii;
    const float4 *rec;      // the view's render records (GEOM): the activated opacity (sigmoid chain)
    const uint8_t *clampm;  // the view's SH clamp masks (GEOM)
    const float *sums;      // the view's per-Gaussian record sums, kPartial x P SoA (SUMS, gsr_backward_render)
    float *dL_dmeans2D;     // the view's screen-space gradient (P,3) or NULL
    int acc2;               // add into dL_dmeans2D instead of overwriting
};
struct MultiArgs : GaussGrads {
    int P, D, M, nv, act;
    float scale_modifier;
    const float *means3D, *scales, *rotations, *shs, *cov3D_precomp;
    MultiView v[kMultiViews];
};
hipError_t launch_gauss_bwd_multi(const MultiArgs &a, hipStream_t s);

// fused L1 + SSIM (gsr_loss.hip): normalised 1-D window of calc_ssim (external.py:48-65)
struct SsimWindow { float w[11]; };
size_t ssim_partials(int planes, int H, int W);
hipError_t launch_ssim_fwd(int planes, int H, int W, const float *img1, const float *img2, const SsimWindow &w,
                           float *maps, float2 *partial, float *out_l1, float *out_ssim, hipStream_t s);
// forward-only scoring of `views` image pairs (host arrays of device pointers); partial: views x
// ssim_partials x 3 floats; out_scores (views, 4); out_mean may be null.  views >= 1.
hipError_t launch_image_scores(int views, int planes, int H, int W, const float *const *img1,
                               const float *const *img2, const SsimWindow &w, float *partial, float *out_scores,
                               float *out_mean, hipStream_t s);
hipError_t launch_ssim_bwd(int planes, int H, int W, const float *img1, const float *img2, const SsimWindow &w,
                           const float *maps, const float *g_l1, const float *g_ssim, float *dimg1,
                           hipStream_t s);

// rigidity loss + exact k-nearest neighbours (gsr_rigidity.hip)
hipError_t launch_knn(int n, const float *pts, int k, int *out_idx, double *out_d2, hipStream_t s);
int rigid_blocks(int F);
hipError_t launch_rigid_fwd(int F, int k, const float *means, const float *quats, const int *fg_rows,
                            const int *nbr_rows, const float *weights, const float *prev_off, const float *prev_inv,
                            double *partial, float *save_u, float *save_m, float *save_q, float *out_loss,
                            float *next_inv, float *next_off, hipStream_t s);  // next_*: both or neither
hipError_t launch_foreground_info(int F, int k, const float *means, const float *quats, const int *fg_rows,
                                  const int *nbr_rows, float *out_inv, float *out_off, hipStream_t s);
hipError_t launch_rigid_bwd(int P, int F, int k, const int *row_to_fg, const int *rev_off, const int *rev_edge,
                            const float *save_u, const float *save_m, const float *save_q, const float *g_loss,
                            float *dmeans, float *dquats, hipStream_t s);

// deformation network input layer (gsr_deform.hip): i* initial, p* previous (means, quats, ranges)
constexpr int kDeformAutoBlocks = 256;  // persistent backward workgroups when the caller sets no bound (one per CU)
constexpr int kDeformMaxH = 512;
constexpr int kPosencRangeBlocks = 256;  // = GSR_POSENC_RANGE_BLOCKS: workgroups (partials) of the range reduction
hipError_t launch_posenc_ranges(int P, const float *means, const float *quats, float *partial, float *ranges,
                                hipStream_t s);
hipError_t launch_posenc(int P, const float *means, const float *quats, const float *ranges, float *out, hipStream_t s);
hipError_t launch_deform_in_fwd(int P, int H, const float *im, const float *iq, const float *ir, const float *pm,
                                const float *pq, const float *pr, float progress, const float *W, const float *bias,
                                float *Y, hipStream_t s);
size_t deform_in_partial_floats(int P, int H, int max_blocks);
hipError_t launch_deform_in_bwd(int P, int H, const float *im, const float *iq, const float *ir, const float *pm,
                                const float *pq, const float *pr, float progress, const float *dY, float *partial,
                                int max_blocks, float *dW, float *db, hipStream_t s);

// deformation network residual blocks (gsr_resblock.hip): stats = mean1, invstd1, mean2, invstd2 (4 H)
constexpr int kResblockAutoBlocks = 256;  // persistent workgroups when the caller sets no bound (one per CU; twice that for H <= 64)
constexpr int kResblockNarrowH = 128;  // up to here the weight stays in LDS; wider blocks walk 128-column blocks and k panels
constexpr int kResblockMaxH = 512;
struct ResblockWorkspace {  // byte offsets; the backward's also holds the two transient (P, H) gradients
    size_t partial_s, partial_w, sums, g_s, g_z1, total;
    ResblockWorkspace(int P, int H, int max_blocks, bool backward);
};
hipError_t launch_resblock_fwd(int P, int H, const float *x, const float *W1, const float *gamma1, const float *beta1,
                               const float *W2, const float *gamma2, const float *beta2, float eps1, float eps2,
                               float momentum1, float momentum2, float *running_mean1, float *running_var1,
                               float *running_mean2, float *running_var2, char *ws, int max_blocks, float *y1, float *y2,
                               float *out, float *stats, hipStream_t s);
hipError_t launch_resblock_bwd(int P, int H, const float *x, const float *y1, const float *y2, const float *stats,
                               const float *W1, const float *gamma1, const float *beta1, const float *W2,
                               const float *gamma2, const float *beta2, const float *g_out, char *ws, int max_blocks,
                               float *dx, float *dW1, float *dgamma1, float *dbeta1, float *dW2, float *dgamma2,
                               float *dbeta2, hipStream_t s);

// deformation network output head (gsr_head.hip): fc_out and the "+ initial" update; im / iq the initial
// means (P, 3) and quaternions (P, 4)
constexpr int kHeadAutoBlocks = 1024;  // persistent backward workgroups when the caller sets no bound (four per CU)
constexpr int kHeadMaxH = 512;
hipError_t launch_head_fwd(int P, int H, const float *x, const float *W, const float *bias, const float *im,
                           const float *iq, float *out, hipStream_t s);
size_t head_partial_floats(int P, int H, int max_blocks);
hipError_t launch_head_bwd(int P, int H, const float *x, const float *W, const float *g, float *partial, int max_blocks,
                           float *dx, float *dW, float *db, hipStream_t s);

// densification (gsr_densify.hip)
struct DensArgs {
    int P, prune_big;
    float grad_threshold, small_scale, big_scale, remove_opacity, inv_split_div;
    const float *grad_accum, *vis_count, *log_scales, *opacity_logits, *rotations;
};
struct DensColumn {
    int width, role;
    const float *src, *m_src, *v_src;
    float *dst, *m_dst, *v_dst;
};
constexpr int kDensMaxColumns = 8;
struct DensColumns { int n; DensColumn c[kDensMaxColumns]; };
struct DensWorkspace {
    int NB;
    size_t flags, bsum, boff, totals, total;
    explicit DensWorkspace(int P);
};
hipError_t launch_dens_radii(int P, const int *radii, float *max_radii, uint8_t *visible, hipStream_t s);
hipError_t launch_dens_grads(int P, const uint8_t *visible, const float *m2grad, float *grad_accum,
                             float *vis_count, hipStream_t s);
hipError_t launch_dens_plan(const DensArgs &a, char *ws, hipStream_t s);
hipError_t launch_dens_stds(const DensArgs &a, const char *ws, float *stds, hipStream_t s);
hipError_t launch_dens_apply(const DensArgs &a, const char *ws, const float *samples, const DensColumns &cols,
                             hipStream_t s);

// fused Adam (gsr_adam.hip)
struct AdamTensor {
    float *param; const float *grad; float *exp_avg; float *exp_avg_sq;
    long long n; float step_size, bc2_sqrt; int vec4;
};
constexpr int kAdamMaxTensors = 16;
constexpr int kAdamThreads = 256;
constexpr int kAdamPerBlock = kAdamThreads * 4;  // elements per block: 4 per thread
struct AdamTable {
    int n; float w1, b2, omb2, eps;
    AdamTensor t[kAdamMaxTensors];
    int block_start[kAdamMaxTensors + 1];
};
int adam_blocks(long long n);
hipError_t launch_adam(const AdamTable &tab, hipStream_t s);
// gradient norm (gsr_adam.hip): one double per block of kAdamPerBlock elements at partials[block in
// the table], by the update itself (launch_adam_norm) or by a reduction-only pass (launch_grad_sumsq);
// launch_norm_final sums each table entry's partials [part_start[k], part_start[k + 1]) into
// tensor_sums[slot[k]] (and out_sqnorms[slot[k]] when given) and, on the call's last table, the slots
// 0 .. nslots-1 in order into *total and sqrt(*total) into *out_norm.  An entry may have no partials (an
// empty tensor: its sum is 0).
struct NormTensor { const float *grad; long long n; int vec4; };
struct NormTable {
    int n;
    NormTensor t[kAdamMaxTensors];
    int block_start[kAdamMaxTensors + 1];
};
struct NormFinal {
    int n, nslots, last;
    int slot[kAdamMaxTensors];
    int part_start[kAdamMaxTensors + 1];
};
hipError_t launch_adam_norm(const AdamTable &tab, double *partials, hipStream_t s);
hipError_t launch_grad_sumsq(const NormTable &tab, double *partials, hipStream_t s);
hipError_t launch_norm_final(const NormFinal &f, const double *partials, double *tensor_sums, double *total,
                             float *out_sqnorms, float *out_norm, hipStream_t s);

// camera frames -> view tensors (gsr_io.hip)
hipError_t launch_views_pack(int frames, int HW, const uint8_t *rgb, const uint8_t *seg, float *img, float *msk,
                             hipStream_t s);
// rendered images -> 8-bit frames (gsr_io.hip); any alignment, any frame count
hipError_t launch_frames_pack(int frames, int HW, const float *img, uint8_t *rgb, hipStream_t s);

}  // namespace gsr
