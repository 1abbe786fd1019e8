"""One densify.py iteration on the native path (the caller side of SURVEY.md 8(a) + rows 8(f) 1-3).

``densify_iteration`` is the body of densify.py's loop (densify.py:218-247) with every piece on the
HIP kernels of ``libgsr.so``:

=====================================================  ============================================
reference (densify.py / external.py / shared.py)       here
=====================================================  ============================================
create_render_arguments + Renderer (image)  :110-126    rasterize_parameters (activations fused)
0.8 l1 + 0.2 (1 - calc_ssim)                :127-129    splat_loss.image_loss (fused L1 + SSIM)
segmentation render + loss                  :132-151    rasterize_parameters(colors = masks) + loss
update_max_2d_radii_and_visibility_mask     :154-162    splat_densify (statistics kernel)
total_loss.backward()                       :237        same (native backward kernels)
densify_gaussians                           :239-245    splat_densify.densify_gaussians
optimizer.step(); zero_grad(set_to_none)    :246-247    splat_adam.FusedAdam (one launch)
=====================================================  ============================================

``train_step_loss`` is the loss of one train.py step (train.py:395-418): the views' renders and image
losses as above plus the rigidity term of ``splat_rigidity``, evaluated once per step.
``advance_timestep`` hands a finished timestep's cloud and rigidity state to the next (train.py:251-266).
``evaluate_views`` is the comparison half of an inference timestep (train.py:598-613) and ``ScoreLog`` takes
its numbers to the host without a synchronisation.  ``step_metrics`` packs what a training step logs
(train.py:419-428, :769-772) for the same ``ScoreLog``; the gradient norm in it comes from
``splat_adam.gradient_norm`` or ``FusedAdam.step(grad_norm=True)``.

``View`` restates shared.py:13-18.  The image-render ``means2D`` is a leaf that receives the same
screen-space (NDC) gradient the reference reads through ``retain_grad`` (densify.py:119).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

import splat_densify
import splat_loss
import splat_rigidity
from diff_gaussian_rasterization import GaussianRasterizationSettings, rasterize_parameters

__all__ = ["View", "densify_iteration", "create_densification_variables", "train_step_loss", "advance_timestep",
           "evaluate_views", "ScoreLog", "step_metrics", "STEP_METRIC_NAMES"]


@dataclass
class View:
    """shared.py:13-18."""
    camera_index: int
    render_settings: GaussianRasterizationSettings
    image: torch.Tensor
    segmentation_mask: torch.Tensor


def create_densification_variables(params):
    """densify.py:89-106."""
    P = params["means"].shape[0]
    dev = params["means"].device
    return splat_densify.DensificationVariables(visibility_count=torch.zeros(P, device=dev),
                                                mean_2d_gradients_accumulated=torch.zeros(P, device=dev),
                                                max_2d_radii=torch.zeros(P, device=dev))


def densify_iteration(params, view, densification_variables, optimizer, scene_radius, i, sample_fn=None):
    """densify.py:218-247 for one view.  Returns (total_loss, image_loss, segmentation_loss) as
    detached scalars (no host sync) and the densify row counts when this iteration densified."""
    rs = view.render_settings
    dv = densification_variables
    means2D = torch.zeros_like(params["means"], requires_grad=True)
    image, radii, _ = rasterize_parameters(params, rs, means2D=means2D)
    image_loss = splat_loss.image_loss(image, view.image)
    seg_params = dict(params)
    seg_params["colors"] = params["segmentation_masks"]
    seg, _, _ = rasterize_parameters(seg_params, rs)
    segmentation_loss = splat_loss.image_loss(seg, view.segmentation_mask)
    dv.means_2d = means2D  # gradient only from the colour render (densify.py:130-133)
    splat_densify.update_max_2d_radii_and_visibility_mask(radii, dv)
    total = image_loss + 3 * segmentation_loss
    total.backward()
    with torch.no_grad():
        info = splat_densify.densify_gaussians(params, dv, scene_radius, optimizer, i, sample_fn=sample_fn)
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)
    return (total.detach(), image_loss.detach(), segmentation_loss.detach()), info


def train_step_loss(params, views, neighbor_info, foreground_info, next_foreground_info=False):
    """train.py:395-418 ``calculate_loss`` without the logging: every view rendered
    (``rasterize_parameters``) and compared (fused L1 + SSIM), plus the rigidity term.  The reference
    evaluates the rigidity term once per view although it does not depend on the view; here it is
    evaluated once and multiplied by ``V = len(views)``.  Returns ``(0.8 sum l1 + 0.2 sum (1 - ssim) +
    3 V rigidity, sum l1, sum (1 - ssim), V rigidity)``; call ``backward()`` on the first.

    ``next_foreground_info``: a fifth element, the ``ForegroundInfo`` of ``params`` -- what the next
    timestep's rigidity term compares with (train.py:759-765 builds it after the loss) -- stored by the
    rigidity forward kernel itself (``calculate_rigidity_loss_and_state``; DESIGN.md 6 has the timing
    against a separate ``splat_rigidity.foreground_info`` launch)."""
    if not views:
        raise ValueError("train_step_loss: no views")
    l1_sum = ssim_sum = None
    for view in views:
        image, _, _ = rasterize_parameters(params, view.render_settings)
        l1, ssim_loss = splat_loss.l1_and_ssim_loss(image, view.image)
        l1_sum = l1 if l1_sum is None else l1_sum + l1
        ssim_sum = ssim_loss if ssim_sum is None else ssim_sum + ssim_loss
    if next_foreground_info:
        rigidity, state = splat_rigidity.calculate_rigidity_loss_and_state(params, neighbor_info, foreground_info)
    else:
        rigidity = splat_rigidity.calculate_rigidity_loss(params, neighbor_info, foreground_info)
    rigidity_sum = len(views) * rigidity
    total = 0.8 * l1_sum + 0.2 * ssim_sum + 3 * rigidity_sum
    if next_foreground_info:
        return total, l1_sum, ssim_sum, rigidity_sum, state
    return total, l1_sum, ssim_sum, rigidity_sum


STEP_METRIC_NAMES = ("train-loss/total", "train-loss/l1", "train-loss/ssim", "train-loss/image",
                     "train-loss/rigidity", "gradient-norm")


def step_metrics(losses, gradient_norm):
    """What a train.py step logs (train.py:419-428 and :769-772) as ONE float32 tensor of six values in
    ``STEP_METRIC_NAMES`` order, for ``ScoreLog.put(step, ...)``: the reference reads each of them with its
    own ``.item()``.  ``losses`` is ``train_step_loss``'s tuple, ``gradient_norm`` the scalar of
    ``splat_adam.gradient_norm`` or ``FusedAdam.step(grad_norm=True)``.  ``image`` is
    ``0.8 l1_sum + 0.2 ssim_sum`` in float32 (train.py:391-392).  Torch operations only; nothing is
    synchronised."""
    total, l1_sum, ssim_sum, rigidity_sum = (x.detach().float() for x in losses[:4])
    image = 0.8 * l1_sum + 0.2 * ssim_sum
    return torch.stack([total, l1_sum, ssim_sum, image, rigidity_sum,
                        gradient_norm.detach().float().to(total.device)]).reshape(6)


def evaluate_views(params, views):
    """train.py:598-613 without the loading and the logging: every view of a timestep rendered under
    ``no_grad`` (``rasterize_parameters``) and all of them compared with their images in one forward-only
    pass.  Returns ``splat_loss.image_scores``' result: per view ``l1``, ``ssim``, ``mse``, ``psnr`` and
    ``image_loss = 0.8 l1 + 0.2 (1 - ssim)``, and ``mean_image_loss``, the reference's ``mean-image-loss``.
    Device tensors; nothing is synchronised (``ScoreLog`` takes them to the host)."""
    if not views:
        raise ValueError("evaluate_views: no views")
    with torch.no_grad():
        renders = [rasterize_parameters(params, view.render_settings)[0] for view in views]
    return splat_loss.image_scores(renders, [view.image for view in views])


class ScoreLog:
    """The metric's way to the host without a synchronisation: a ring of ``depth`` pinned host slots,
    modelled on ``splat_export.FrameWriter``.

    ``put(step, scores)``: ``scores`` is ``image_scores``' result or one tensor; its values are packed and
    copied into the next slot asynchronously, with an event behind the copy.  ``drain()`` returns the
    ``(step, values)`` pairs whose copies have landed, in the order they were put, without blocking;
    ``values`` is an ``ImageScores`` of host tensors, or a host tensor.  A full ring makes ``put`` wait for
    its oldest slot, whose pair is kept for the next ``drain``.  ``close()`` waits for the rest and returns it."""

    def __init__(self, depth: int = 8):
        if depth < 1:
            raise ValueError(f"ScoreLog: got depth={depth}, expected at least 1")
        self.depth = depth
        self._slots = [None] * depth   # (step, staging view, event, views V or None) of a copy in flight
        self._staging = [None] * depth
        self._head = self._count = 0   # oldest slot in flight, slots in flight
        self._done = []
        self._closed = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __len__(self):
        """Pairs not yet returned by ``drain``."""
        return self._count + len(self._done)

    def _finish_oldest(self):
        step, staged, event, V = self._slots[self._head]
        if event is not None:
            event.synchronize()
        host = staged.clone()  # the slot is reused
        if V is None:
            values = host
        else:
            rows = host[:5 * V].view(5, V)
            values = splat_loss.ImageScores(rows[0], rows[1], rows[2], rows[3], rows[4], host[5 * V])
        self._done.append((step, values))
        self._slots[self._head] = None
        self._head = (self._head + 1) % self.depth
        self._count -= 1

    def put(self, step, scores):
        if self._closed:
            raise RuntimeError("ScoreLog: put after close()")
        if isinstance(scores, splat_loss.ImageScores):
            V = scores.l1.numel()
            packed = torch.cat([torch.stack(scores[:5]).reshape(-1), scores.mean_image_loss.reshape(1)])
        elif isinstance(scores, torch.Tensor):
            V, packed = None, scores.detach()
        else:
            raise TypeError(f"ScoreLog.put: got {type(scores).__name__}, expected image_scores' result or a tensor")
        if self._count == self.depth:
            self._finish_oldest()  # blocks on the oldest copy; its pair waits in _done
        k = (self._head + self._count) % self.depth
        n = packed.numel()
        st = self._staging[k]
        if st is None or st.numel() < n or st.dtype != packed.dtype:
            st = self._staging[k] = torch.empty(max(n, 1), dtype=packed.dtype, pin_memory=torch.cuda.is_available())
        staged = st[:n].view(packed.shape)
        event = None
        if packed.is_cuda:
            staged.copy_(packed, non_blocking=True)
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(packed.device))
        else:
            staged.copy_(packed)
        self._slots[k] = (step, staged, event, V)
        self._count += 1

    def drain(self):
        while self._count:
            event = self._slots[self._head][2]
            if event is not None and not event.query():
                break  # later copies are behind it on the stream
            self._finish_oldest()
        done, self._done = self._done, []
        return done

    def close(self):
        self._closed = True
        while self._count:
            self._finish_oldest()
        done, self._done = self._done, []
        return done


def advance_timestep(updated_params, neighbor_info, foreground_info=None):
    """train.py:251-266 ``compute_encoded_normalized_means_and_rotations_and_foreground_info`` between two
    timesteps: ``(previous_params, ForegroundInfo)`` for the next one.  ``previous_params`` is every entry
    of ``updated_params`` detached; nothing is encoded here, ``splat_deform.deform_input_layer`` takes the
    dict.  The state is ``foreground_info`` when given (the one ``train_step_loss(...,
    next_foreground_info=True)`` returned for the same cloud), else ``splat_rigidity.foreground_info`` of
    the updated cloud: one launch, no host synchronisation."""
    previous_params = {name: value.detach() for name, value in updated_params.items()}
    if foreground_info is None:
        foreground_info = splat_rigidity.foreground_info(previous_params, neighbor_info)
    return previous_params, foreground_info
