"""Fused L1 + SSIM image loss on the HIP kernels of ``libgsr.so``.

Drop-ins for the loss the reference computes after every render:

* ``calc_ssim(img1, img2, window_size=11, size_average=True)`` -- external.py:68-76 (+ ``_ssim``,
  external.py:79-110): mean SSIM with an 11x11 Gaussian window (sigma 1.5), zero padding.
* ``calculate_l1_and_ssim_loss``-style pair ``l1_and_ssim_loss(rendered, target)`` ->
  ``(l1_loss, 1 - ssim)`` as train.py:354-364 returns it, and ``image_loss(rendered, target)`` =
  ``0.8 * l1 + 0.2 * (1 - ssim)`` (train.py:391-392, densify.py:127-129,149-151).

* ``image_scores(renders, targets)``: the scoring loop of ``inference`` (train.py:598-613) over all views of
  a timestep in one forward-only pass -- per view ``l1``, ``ssim``, ``mse``, ``psnr`` and ``image_loss``,
  and their mean image loss, with no derivative maps written and nothing synchronised.  ``l1_and_ssim``
  takes the same kernels wherever no gradient can follow; its values do not change by a bit.

One forward kernel computes both means and keeps the per-pixel SSIM derivatives; one backward
kernel blurs them and adds the L1 sign term, taking the upstream gradients from device memory.
Gradients flow to ``img1`` (the render) only; the target ``img2`` is data in every reference call
site, so a target that requires grad is rejected rather than silently given none.  There is no CPU
path: CPU tensors or a missing ``libgsr.so`` raise.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch

from diff_gaussian_rasterization import _C

__all__ = ["calc_ssim", "l1_and_ssim", "l1_and_ssim_loss", "image_loss", "image_scores", "ImageScores"]


def _planes(img):
    if img.dim() < 2:
        raise RuntimeError("l1_ssim: expected an image of shape (..., H, W)")
    H, W = img.shape[-2], img.shape[-1]
    planes = img.numel() // max(H * W, 1)
    return planes, H, W


class _L1SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2):
        L = _C.load_library()
        if img1.shape != img2.shape:
            raise RuntimeError(f"l1_ssim: image shapes differ: {tuple(img1.shape)} vs {tuple(img2.shape)}")
        a, b = img1.contiguous(), img2.contiguous()
        for t in (a, b):
            _C._ptr(t)  # GPU + float32 checks (no CPU path)
        planes, H, W = _planes(a)
        dev = a.device
        scratch = torch.empty(L.gsr_ssim_scratch_bytes(planes, H, W), dtype=torch.uint8, device=dev)
        l1 = torch.empty((), dtype=torch.float32, device=dev)
        ssim = torch.empty((), dtype=torch.float32, device=dev)
        _C._check(L.gsr_l1_ssim_forward(planes, H, W, a.data_ptr(), b.data_ptr(), scratch.data_ptr(),
                                        l1.data_ptr(), ssim.data_ptr(), _C._stream_ptr(dev)))
        ctx.save_for_backward(a, b, scratch)
        ctx.shape = img1.shape
        ctx.set_materialize_grads(False)
        return l1, ssim

    @staticmethod
    def backward(ctx, g_l1, g_ssim):
        if g_l1 is None and g_ssim is None:
            return None, None
        L = _C.load_library()
        a, b, scratch = ctx.saved_tensors
        planes, H, W = _planes(a)
        gl = g_l1.contiguous().float() if g_l1 is not None else None
        gs = g_ssim.contiguous().float() if g_ssim is not None else None
        grad = torch.empty_like(a)
        _C._check(L.gsr_l1_ssim_backward(planes, H, W, a.data_ptr(), b.data_ptr(), scratch.data_ptr(),
                                         gl.data_ptr() if gl is not None else None,
                                         gs.data_ptr() if gs is not None else None, grad.data_ptr(),
                                         _C._stream_ptr(a.device)))
        return grad.view(ctx.shape), None


def _score(L, views1, views2, planes, H, W, dev, mean):
    """gsr_image_scores over contiguous float32 GPU views of one size: the (V, 4) scores tensor and, with
    ``mean``, the 0-d mean image loss."""
    V = len(views1)
    scores = torch.empty((V, 4), dtype=torch.float32, device=dev)
    out_mean = torch.empty((), dtype=torch.float32, device=dev) if mean else None
    work = torch.empty(L.gsr_image_scores_workspace_bytes(V, planes, H, W), dtype=torch.uint8, device=dev)
    p1 = (ctypes.c_void_p * V)(*[t.data_ptr() for t in views1]) if V else None
    p2 = (ctypes.c_void_p * V)(*[t.data_ptr() for t in views2]) if V else None
    with _C._device_guard(dev):
        _C._check(L.gsr_image_scores(V, planes, H, W, p1, p2, work.data_ptr() if V else None,
                                     scores.data_ptr() if V else None,
                                     out_mean.data_ptr() if mean else None, _C._stream_ptr(dev)))
    return scores, out_mean


def _l1_ssim_forward_only(img1, img2):
    """_L1SSIM.forward without a backward to prepare: no derivative maps are written or allocated; the same
    values bitwise (the scoring kernel runs the training forward's per-pixel code and sums)."""
    L = _C.feature_library("scores")
    if img1.shape != img2.shape:
        raise RuntimeError(f"l1_ssim: image shapes differ: {tuple(img1.shape)} vs {tuple(img2.shape)}")
    a, b = img1.detach().contiguous(), img2.contiguous()
    for t in (a, b):
        _C._ptr(t)  # GPU + float32 checks (no CPU path)
    planes, H, W = _planes(a)
    if planes * H * W == 0:
        raise RuntimeError("l1_ssim: empty image (the mean is undefined)")
    scores, _ = _score(L, [a], [b], planes, H, W, a.device, False)
    return scores[0, 0], scores[0, 1]


def l1_and_ssim(img1, img2):
    """``(torch.nn.functional.l1_loss(img1, img2), calc_ssim(img1, img2))`` from one kernel pair.  Where
    no gradient can follow (``torch.no_grad()``, or an ``img1`` that does not require one) the forward-only
    kernel gives the same two values without the derivative scratch."""
    if img2.requires_grad:
        raise NotImplementedError("l1_ssim: gradients flow to img1 (the render) only; detach the target")
    if not (torch.is_grad_enabled() and img1.requires_grad):
        return _l1_ssim_forward_only(img1, img2)
    return _L1SSIM.apply(img1, img2)


class ImageScores(NamedTuple):
    """``image_scores``' result: ``(V,)`` float32 device tensors and the 0-d mean of ``image_loss``."""
    l1: torch.Tensor
    ssim: torch.Tensor
    mse: torch.Tensor
    psnr: torch.Tensor
    image_loss: torch.Tensor
    mean_image_loss: torch.Tensor


def _view_list(x, side):
    if isinstance(x, torch.Tensor):
        if x.dim() != 4:
            raise RuntimeError(f"image_scores: {side}: expected a (V, C, H, W) batch or a sequence of (C, H, W) "
                               f"images, got a tensor of shape {tuple(x.shape)}")
        return list(x.unbind(0))
    views = list(x)
    for k, t in enumerate(views):
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise RuntimeError(f"image_scores: {side}[{k}]: expected a (C, H, W) tensor")
    return views


def image_scores(renders, targets):
    """Scores of a timestep's views, train.py:598-613 without the renders: per view ``l1``, ``ssim``,
    ``mse``, ``psnr = -10 log10(mse)`` (``+inf`` for equal images) and ``image_loss = 0.8 l1 + 0.2 (1 -
    ssim)``, and ``mean_image_loss`` over the views, from one forward-only pass (``gsr_image_scores``).

    ``renders`` / ``targets``: each a sequence of ``(C, H, W)`` tensors (separately allocated renders are
    read where they are, no stacked copy) or a ``(V, C, H, W)`` batch; all of one size, float32, on one GPU.
    Inputs are detached: nothing here is differentiable.  Nothing is synchronised.  ``l1`` and ``ssim``
    are bitwise what ``l1_and_ssim`` gives for the view alone."""
    a, b = _view_list(renders, "renders"), _view_list(targets, "targets")
    if len(a) != len(b):
        raise RuntimeError(f"image_scores: {len(a)} renders but {len(b)} targets")
    if any(t.requires_grad for t in b):
        raise NotImplementedError("image_scores: a target requires grad; targets are data, detach them")
    if not a:
        if not isinstance(renders, torch.Tensor):
            raise ValueError("image_scores: got an empty list, expected at least one view (or an empty batch)")
        first = renders[:0]
    else:
        first = a[0]
    for k, (x, y) in enumerate(zip(a, b)):
        if x.shape != first.shape or y.shape != first.shape:
            raise RuntimeError(f"image_scores: view {k}: image shapes differ: render {tuple(x.shape)}, target "
                               f"{tuple(y.shape)}, view 0 {tuple(first.shape)}")
    for t in (first, *a, *b):
        if t.dtype != torch.float32:
            raise RuntimeError(f"image_scores: expected float32, got {t.dtype}")
        if not t.is_cuda:
            raise RuntimeError("image_scores: tensors must be on the GPU (no CPU path)")
        if t.device != first.device:
            raise RuntimeError(f"image_scores: views on {t.device} and {first.device}")
    L = _C.feature_library("scores")
    planes, H, W = (int(s) for s in first.shape[-3:])
    if a and planes * H * W == 0:
        raise RuntimeError("image_scores: empty images (the means are undefined)")
    a = [t.detach().contiguous() for t in a]
    b = [t.contiguous() for t in b]
    scores, mean = _score(L, a, b, planes, H, W, first.device, True)
    mse = scores[:, 2]
    return ImageScores(scores[:, 0], scores[:, 1], mse, -10.0 * torch.log10(mse), scores[:, 3], mean)


def calc_ssim(img1, img2, window_size=11, size_average=True):
    """external.py:68-76.  Only the configuration the reference uses is supported: window 11 with the
    scalar mean (``size_average=False`` cannot be evaluated on the reference's (3,H,W) renders)."""
    if window_size != 11 or not size_average:
        raise NotImplementedError("calc_ssim: only window_size=11, size_average=True (the reference's use)")
    return l1_and_ssim(img1, img2)[1]


def l1_and_ssim_loss(rendered, target):
    """train.py:354-364 ``calculate_l1_and_ssim_loss`` minus the render: ``(l1_loss, 1 - ssim)``."""
    l1, ssim = l1_and_ssim(rendered, target)
    return l1, 1.0 - ssim


def image_loss(rendered, target):
    """0.8 * l1 + 0.2 * (1 - ssim): train.py:391-392 and densify.py:127-129,149-151."""
    l1, ssim = l1_and_ssim(rendered, target)
    return 0.8 * l1 + 0.2 * (1.0 - ssim)
