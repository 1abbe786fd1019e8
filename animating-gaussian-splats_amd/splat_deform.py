"""The deformation network of train.py with its input side, its residual blocks and its output head on the
HIP kernels of ``libgsr.so``.

Every step the reference re-encodes the previous cloud (``normalize_and_encode_means_and_rotations``,
train.py:185-204), repeats the progress encoding over all rows, ``torch.cat``s both with the initial
encoding into a (P, 192) matrix and feeds it to ``fc_in`` (train.py:96-104, 269-294).  Here that matrix
never exists: ``deform_input_layer`` computes ``fc_in``'s output straight from the 14 floats per
Gaussian (csrc/gsr_deform.hip), and its backward recomputes the features for ``dW``.

* ``encode_means_and_rotations(params)`` -- train.py:185-204, the (P, 92) encoding as a tensor;
* ``deform_input_layer(weight, bias, initial_params, previous_params, progress)`` -- ``fc_in`` applied
  to ``[enc(initial) | enc(previous) | enc(progress)]``; gradients flow to ``weight`` and ``bias`` only
  (the reference detaches the encoded parameters, train.py:255-258);
* ``residual_block(x, fc1_weight, bn1, fc2_weight, bn2)`` -- one ResidualBlock (train.py:57-77) with
  training-mode BatchNorm, fused (csrc/gsr_resblock.hip) for H <= 512: three (P, H) tensors stay alive for
  the backward; ``set_fused_residual_blocks(False)`` sends ``ResidualBlock`` back to the torch ops, and
  ``set_fused_residual_block_width(max_hidden)`` sets the widest H that ``ResidualBlock`` routes to the
  kernels by itself (128 by default, up to 512);
* ``deform_output_layer(x, weight, bias, initial_params)`` -- ``fc_out`` and the ``+ [initial means | initial
  quaternions]`` that follows it (train.py:106-108) in one kernel (csrc/gsr_head.hip), the (P, 7) concatenation
  never built; gradients flow to ``x``, ``weight`` and ``bias`` (and to the initial values if they require one);
  ``set_fused_output_head(False)`` sends ``DeformationNetwork`` back to the two torch lines;
* ``DeformationNetwork`` -- train.py:80-110 with the reference's ``state_dict`` names and shapes; its
  residual blocks run fused when eligible (training mode, H <= the fused width, 128 by default), its
  output head in either mode;
* ``update_gaussian_cloud_parameters`` -- train.py:269-308; the ``* 0.01`` update stays in torch.

All fp32.  There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

import torch
from torch import nn

from diff_gaussian_rasterization import _C

__all__ = ["encode_means_and_rotations", "encoding_ranges", "deform_input_layer", "residual_block",
           "set_fused_residual_blocks", "set_fused_residual_block_width", "deform_output_layer",
           "set_fused_output_head", "ResidualBlock", "DeformationNetwork", "update_gaussian_cloud_parameters",
           "MAX_HIDDEN", "MAX_FUSED_HIDDEN"]

MAX_HIDDEN = 512
MAX_FUSED_HIDDEN = 128  # widest hidden dimension ResidualBlock sends to the fused kernels by default
ENCODING_WIDTH = 92  # 3 means x 10 frequencies x (sin, cos) + 4 quaternion components x 4 x 2
INPUT_WIDTH = 192    # two encodings + the 8 progress columns
RANGE_BLOCKS = 256   # GSR_POSENC_RANGE_BLOCKS of include/gsr.h


def _param_tensors(params, what, P=None):
    """The (P, 3) means and (P, 4) raw quaternions of ``params`` as they are (attached), checked to be fp32 and
    to have ``P`` rows (None: as many as the means have)."""
    means, quats = params["means"], params["rotation_quaternions"]
    rows = "P" if P is None else P
    if P is None:
        P = means.shape[0] if means.dim() else -1
    if tuple(means.shape) != (P, 3) or tuple(quats.shape) != (P, 4):
        raise ValueError(f"{what}: means {tuple(means.shape)} / rotation_quaternions {tuple(quats.shape)}, "
                         f"expected ({rows}, 3) / ({rows}, 4)")
    for t in (means, quats):
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: expected float32 parameters, got {t.dtype}")
    return means, quats


def _means_and_rotations(params, what):
    """The (P, 3) means and (P, 4) raw quaternions of ``params``, detached, fp32, contiguous."""
    means, quats = _param_tensors(params, what)
    return means.detach().contiguous(), quats.detach().contiguous()


def _check_activation(x, what, max_hidden):
    """(P, H) of ``x``, checked to be a float32 matrix with 1 <= H <= ``max_hidden``."""
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"{what}: x {tuple(x.shape)} {x.dtype}, expected float32 (P, H)")
    P, H = x.shape
    if not 1 <= H <= max_hidden:
        raise ValueError(f"{what}: hidden dimension {H} outside [1, {max_hidden}]")
    return P, H


def _check_blocks(max_blocks, what):
    if max_blocks < 0:
        raise ValueError(f"{what}: max_blocks must be >= 0")


def _need_gpu(what, *tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"splat_deform: {what} must be on the GPU (no CPU path)")


def _eligible(x, *params):
    """The tensor tests of the fused paths: a contiguous (P, H) activation, and it and ``params`` float32 on the GPU."""
    return x.dim() == 2 and x.is_contiguous() and all(t.is_cuda and t.dtype == torch.float32 for t in (x, *params))


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _workspace(nbytes, dev):
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)


def _call(dev, fn, *args):
    """The entry point ``fn`` of libgsr on ``dev`` and its current stream (every entry point's last argument)."""
    with _C._device_guard(dev):
        _C._check(fn(*args, _C._stream_ptr(dev)))


def encoding_ranges(means, quats):
    """The 14 floats the normalisation needs: per column (means xyz, quaternion wxyz) the minimum and
    the maximum of ``x - minimum`` (train.py:190-197), exact in fp32: one pass over the (P >= 1) rows."""
    L = _C.feature_library("deform")
    dev = means.device
    if means.shape[0] == 0:
        return torch.zeros(14, dtype=torch.float32, device=dev)
    buf = torch.empty(14 * (RANGE_BLOCKS + 1), dtype=torch.float32, device=dev)  # the ranges, then the partials
    _call(dev, L.gsr_posenc_ranges, means.shape[0], means.data_ptr(), quats.data_ptr(), buf[14:].data_ptr(),
          buf.data_ptr())
    return buf[:14]


def encode_means_and_rotations(params):
    """train.py:185-204 ``normalize_and_encode_means_and_rotations``: (P, 92) float32."""
    means, quats = _means_and_rotations(params, "encode_means_and_rotations")
    _need_gpu("params", means, quats)
    L = _C.feature_library("deform")
    P, dev = means.shape[0], means.device
    out = torch.empty((P, ENCODING_WIDTH), dtype=torch.float32, device=dev)
    if P == 0:
        return out
    ranges = encoding_ranges(means, quats)
    _call(dev, L.gsr_posenc_forward, P, means.data_ptr(), quats.data_ptr(), ranges.data_ptr(), out.data_ptr())
    return out


class _DeformIn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, bias, im, iq, ir, pm, pq, pr, progress, max_blocks, save):
        L = _C.feature_library("deform")
        w, b = weight.detach().contiguous(), bias.detach().contiguous()
        P, H, dev = im.shape[0], w.shape[0], im.device
        out = torch.empty((P, H), dtype=torch.float32, device=dev)
        _call(dev, L.gsr_deform_in_forward, P, H, im.data_ptr(), iq.data_ptr(), ir.data_ptr(), pm.data_ptr(),
              pq.data_ptr(), pr.data_ptr(), progress, w.data_ptr(), b.data_ptr(), out.data_ptr())
        if save:
            ctx.save_for_backward(im, iq, ir, pm, pq, pr)
            ctx.progress, ctx.max_blocks, ctx.H = progress, max_blocks, H
        return out

    @staticmethod
    def backward(ctx, g):
        L = _C.feature_library("deform")
        im, iq, ir, pm, pq, pr = ctx.saved_tensors
        P, H, dev = im.shape[0], ctx.H, im.device
        g = g.contiguous().float()
        dw = torch.empty((H, INPUT_WIDTH), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        db = torch.empty((H,), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        if P == 0:
            return (dw.zero_() if dw is not None else None, db.zero_() if db is not None else None) + (None,) * 9
        ws = _workspace(L.gsr_deform_in_workspace_bytes(P, H, ctx.max_blocks), dev)
        _call(dev, L.gsr_deform_in_backward, P, H, im.data_ptr(), iq.data_ptr(), ir.data_ptr(), pm.data_ptr(),
              pq.data_ptr(), pr.data_ptr(), ctx.progress, g.data_ptr(), ws.data_ptr(), ctx.max_blocks, _ptr(dw),
              _ptr(db))
        return (dw, db) + (None,) * 9


def _check_layer(weight, bias):
    if weight.dim() != 2 or weight.shape[1] != INPUT_WIDTH:
        raise ValueError(f"deform_input_layer: weight {tuple(weight.shape)}, expected (H, {INPUT_WIDTH})")
    H = weight.shape[0]
    if not 1 <= H <= MAX_HIDDEN:
        raise ValueError(f"deform_input_layer: hidden dimension {H} outside [1, {MAX_HIDDEN}]")
    if tuple(bias.shape) != (H,):
        raise ValueError(f"deform_input_layer: bias {tuple(bias.shape)}, expected ({H},)")
    for t in (weight, bias):
        if t.dtype != torch.float32:
            raise ValueError(f"deform_input_layer: expected float32 weights, got {t.dtype}")


def deform_input_layer(weight, bias, initial_params, previous_params, progress, max_blocks=0):
    """``fc_in`` of the deformation network on its never-materialised input: (P, H) =
    ``[enc(initial) 92 | enc(previous) 92 | enc(progress) 8] @ weight.T + bias`` with ``weight`` (H, 192)
    and ``bias`` (H) as in ``nn.Linear(192, H)``, ``progress`` = timestep / timestep_count.  The
    parameter dicts are detached (no gradient reaches them).  ``max_blocks``: upper bound on the
    backward's persistent workgroups (0: automatic)."""
    _check_layer(weight, bias)
    im, iq = _means_and_rotations(initial_params, "deform_input_layer (initial)")
    pm, pq = _means_and_rotations(previous_params, "deform_input_layer (previous)")
    if pm.shape[0] != im.shape[0]:
        raise ValueError(f"deform_input_layer: {im.shape[0]} initial and {pm.shape[0]} previous Gaussians")
    _check_blocks(max_blocks, "deform_input_layer")
    _need_gpu("weight, bias and params", weight, bias, im, iq, pm, pq)
    ir, pr = encoding_ranges(im, iq), encoding_ranges(pm, pq)
    # the reference builds the scalar as torch.tensor(timestep / timestep_count): rounded to fp32 once
    progress = float(torch.tensor(float(progress), dtype=torch.float32))
    save = torch.is_grad_enabled() and (weight.requires_grad or bias.requires_grad)  # nothing under no_grad
    return _DeformIn.apply(weight, bias, im, iq, ir, pm, pq, pr, progress, int(max_blocks), save)


_FUSED_RESBLOCKS = True


def set_fused_residual_blocks(on):
    """Whether ``ResidualBlock.forward`` runs eligible calls on the fused kernels (default) or always on
    the torch ops (the A/B switch of tools/bench_resblock.py).  Process-wide; returns the previous setting."""
    global _FUSED_RESBLOCKS
    previous, _FUSED_RESBLOCKS = _FUSED_RESBLOCKS, bool(on)
    return previous


_FUSED_RESBLOCK_WIDTH = MAX_FUSED_HIDDEN


def set_fused_residual_block_width(max_hidden):
    """The widest hidden dimension at which ``ResidualBlock.forward`` runs eligible calls on the fused kernels:
    ``MAX_FUSED_HIDDEN`` (128, the default) to ``MAX_HIDDEN`` (512); wider blocks run the torch ops.  An explicit
    ``residual_block`` call runs the kernels at any H <= 512, and ``set_fused_residual_blocks(False)`` wins over
    this.  Process-wide (the A/B switch of tools/bench_resblock.py's wide legs); returns the previous value."""
    global _FUSED_RESBLOCK_WIDTH
    if isinstance(max_hidden, bool) or not isinstance(max_hidden, int) or not MAX_FUSED_HIDDEN <= max_hidden <= MAX_HIDDEN:
        raise ValueError(f"set_fused_residual_block_width: {max_hidden!r} outside [{MAX_FUSED_HIDDEN}, {MAX_HIDDEN}]")
    previous, _FUSED_RESBLOCK_WIDTH = _FUSED_RESBLOCK_WIDTH, max_hidden
    return previous


class _ResBlock(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, g1, b1, w2, g2, b2, bn1, bn2, max_blocks, save):
        L = _C.feature_library("resblock")
        P, H, dev = x.shape[0], x.shape[1], x.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731 - every element is written
        y1, y2, out, stats = new(P, H), new(P, H), new(P, H), new(4 * H)
        ws = _workspace(L.gsr_resblock_workspace_bytes(P, H, max_blocks, 0), dev)
        running = [_ptr(t) for t in (bn1.running_mean, bn1.running_var, bn2.running_mean, bn2.running_var)]
        _call(dev, L.gsr_resblock_forward, P, H, x.data_ptr(), w1.data_ptr(), g1.data_ptr(), b1.data_ptr(),
              w2.data_ptr(), g2.data_ptr(), b2.data_ptr(), bn1.eps, bn2.eps, bn1.momentum, bn2.momentum, *running,
              ws.data_ptr(), max_blocks, y1.data_ptr(), y2.data_ptr(), out.data_ptr(), stats.data_ptr())
        if save:
            ctx.save_for_backward(x, y1, y2, stats, w1, g1, b1, w2, g2, b2)
            ctx.max_blocks = max_blocks
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        L = _C.feature_library("resblock")
        x, y1, y2, stats, w1, g1, b1, w2, g2, b2 = ctx.saved_tensors
        P, H, dev = x.shape[0], x.shape[1], x.device
        g = g.contiguous().float()
        grads = [torch.empty_like(t) if need else None
                 for t, need in zip((x, w1, g1, b1, w2, g2, b2), ctx.needs_input_grad[:7])]
        ws = _workspace(L.gsr_resblock_workspace_bytes(P, H, ctx.max_blocks, 1), dev)
        _call(dev, L.gsr_resblock_backward, P, H, x.data_ptr(), y1.data_ptr(), y2.data_ptr(), stats.data_ptr(),
              w1.data_ptr(), g1.data_ptr(), b1.data_ptr(), w2.data_ptr(), g2.data_ptr(), b2.data_ptr(), g.data_ptr(),
              ws.data_ptr(), ctx.max_blocks, *[_ptr(t) for t in grads])
        return tuple(grads) + (None,) * 4


def _check_bn(bn, H, name):
    if not isinstance(bn, nn.BatchNorm1d) or bn.num_features != H:
        raise ValueError(f"residual_block: {name} must be a BatchNorm1d over {H} features")
    if not bn.affine or bn.momentum is None:
        raise ValueError(f"residual_block: {name} must be affine with a momentum (no cumulative average)")
    for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError(f"residual_block: {name} must hold contiguous float32 tensors")


def residual_block(x, fc1_weight, bn1, fc2_weight, bn2, max_blocks=0):
    """One ResidualBlock of train.py:57-77 on the kernels of csrc/gsr_resblock.hip:
    ``gelu(bn2(gelu(bn1(x @ fc1_weight.T)) @ fc2_weight.T) + x)`` for ``x`` (P >= 2, H <= 512) float32 on
    the GPU, ``fc*_weight`` (H, H) and ``bn*`` the two ``nn.BatchNorm1d`` modules, always normalising with
    the batch statistics (training mode).  Their running statistics are blended and
    ``num_batches_tracked`` incremented as ``F.batch_norm`` does.  Gradients flow to ``x``, both weights and
    both BatchNorms' affine parameters; the graph keeps ``x``, the two GEMM outputs and 4 H statistics.
    ``max_blocks``: upper bound on the persistent workgroups along the rows (0: automatic).  H <= 128 keeps
    the weights in LDS; wider blocks run the kernels that walk 128-column blocks and k panels."""
    P, H = _check_activation(x, "residual_block", MAX_HIDDEN)
    if P < 2:
        raise ValueError(f"residual_block: batch statistics need more than one row (got {P})")
    for w, name in ((fc1_weight, "fc1_weight"), (fc2_weight, "fc2_weight")):
        if tuple(w.shape) != (H, H) or w.dtype != torch.float32:
            raise ValueError(f"residual_block: {name} {tuple(w.shape)} {w.dtype}, expected float32 ({H}, {H})")
    _check_bn(bn1, H, "bn1")
    _check_bn(bn2, H, "bn2")
    _check_blocks(max_blocks, "residual_block")
    params = (fc1_weight, bn1.weight, bn1.bias, fc2_weight, bn2.weight, bn2.bias)
    _need_gpu("x, the weights and the BatchNorms", x, *params,
              *(t for bn in (bn1, bn2) for t in (bn.running_mean, bn.running_var) if t is not None))
    save = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
    out = _ResBlock.apply(x.contiguous(), fc1_weight.contiguous(), bn1.weight, bn1.bias, fc2_weight.contiguous(),
                          bn2.weight, bn2.bias, bn1, bn2, int(max_blocks), save)
    with torch.no_grad():
        for bn in (bn1, bn2):
            if bn.num_batches_tracked is not None:
                bn.num_batches_tracked += 1
    return out


class ResidualBlock(nn.Module):
    """train.py:57-77.  A training-mode call on a contiguous float32 GPU (P >= 2, H <= 128, or up to what
    ``set_fused_residual_block_width`` allows) input runs ``residual_block`` (unless
    ``set_fused_residual_blocks(False)``); every other call the torch ops."""

    def __init__(self, dimension):
        super().__init__()
        self.fc1 = nn.Linear(dimension, dimension, bias=False)
        self.bn1 = nn.BatchNorm1d(dimension)
        self.fc2 = nn.Linear(dimension, dimension, bias=False)
        self.bn2 = nn.BatchNorm1d(dimension)

    def _fused(self, x):
        if not (_FUSED_RESBLOCKS and self.training and x.dim() == 2 and x.shape[0] >= 2
                and x.shape[1] <= _FUSED_RESBLOCK_WIDTH):
            return False
        if tuple(self.fc1.weight.shape) != (x.shape[1],) * 2 or tuple(self.fc2.weight.shape) != (x.shape[1],) * 2:
            return False
        for bn in (self.bn1, self.bn2):
            if not (isinstance(bn, nn.BatchNorm1d) and bn.affine and bn.track_running_stats and bn.momentum is not None
                    and bn.running_mean is not None):
                return False
        params = (self.fc1.weight, self.fc2.weight, self.bn1.weight, self.bn1.bias, self.bn2.weight, self.bn2.bias,
                  self.bn1.running_mean, self.bn1.running_var, self.bn2.running_mean, self.bn2.running_var)
        return _eligible(x, *params) and all(t.is_contiguous() for t in params)

    def forward(self, x):
        if self._fused(x):
            return residual_block(x, self.fc1.weight, self.bn1, self.fc2.weight, self.bn2)
        identity = x
        x = nn.functional.gelu(self.bn1(self.fc1(x)))
        x = self.bn2(self.fc2(x))
        x = x + identity
        return nn.functional.gelu(x)


_FUSED_HEAD = True


def set_fused_output_head(on):
    """Whether ``DeformationNetwork.forward`` runs ``fc_out`` and the ``+ initial`` update of eligible calls
    on the fused kernels (default) or always on the torch ops (the A/B switch of tools/bench_head.py).
    Process-wide; returns the previous setting."""
    global _FUSED_HEAD
    previous, _FUSED_HEAD = _FUSED_HEAD, bool(on)
    return previous


class _DeformOut(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, means, quats, max_blocks, save):
        L = _C.feature_library("head")
        x, w, b = x.detach().contiguous(), weight.detach().contiguous(), bias.detach().contiguous()
        im, iq = means.detach().contiguous(), quats.detach().contiguous()
        P, H, dev = x.shape[0], x.shape[1], x.device
        out = torch.empty((P, 7), dtype=torch.float32, device=dev)
        _call(dev, L.gsr_deform_out_forward, P, H, x.data_ptr(), w.data_ptr(), b.data_ptr(), im.data_ptr(),
              iq.data_ptr(), out.data_ptr())
        ctx.saved = save
        if save:
            ctx.save_for_backward(x, w)
            ctx.max_blocks = max_blocks
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        need = ctx.needs_input_grad
        # the initial values are added as they are: their gradient is the upstream gradient's columns
        gm = g[:, :3] if need[3] else None
        gq = g[:, 3:] if need[4] else None
        if not ctx.saved or not any(need[:3]):
            return None, None, None, gm, gq, None, None
        L = _C.feature_library("head")
        x, w = ctx.saved_tensors
        P, H, dev = x.shape[0], x.shape[1], x.device
        g = g.contiguous().float()
        dx = torch.empty_like(x) if need[0] else None
        dw = torch.empty_like(w) if need[1] else None
        db = torch.empty((7,), dtype=torch.float32, device=dev) if need[2] else None
        sums = dw is not None or db is not None
        ws = _workspace(L.gsr_deform_out_workspace_bytes(P, H, ctx.max_blocks) if sums else 0, dev)
        _call(dev, L.gsr_deform_out_backward, P, H, x.data_ptr(), w.data_ptr(), g.data_ptr(), ws.data_ptr(),
              ctx.max_blocks, _ptr(dx), _ptr(dw), _ptr(db))
        return dx, dw, db, gm, gq, None, None


def deform_output_layer(x, weight, bias, initial_params, max_blocks=0):
    """``fc_out`` of the deformation network and the update that follows it (train.py:106-108) on the kernels
    of csrc/gsr_head.hip: (P, 7) = ``(x @ weight.T + bias) + [initial means | initial quaternions]`` for ``x``
    (P, H <= 512) float32 on the GPU, ``weight`` (7, H) and ``bias`` (7) as in ``nn.Linear(H, 7)``; the (P, 7)
    concatenation is never built.  Gradients flow to ``x``, ``weight`` and ``bias``, and to the initial means
    and quaternions when they require one (the upstream gradient's columns, as from ``out + torch.cat(...)``);
    the graph keeps ``x`` and ``weight``.  ``max_blocks``: upper bound on the backward's persistent workgroups
    (0: automatic)."""
    P, H = _check_activation(x, "deform_output_layer", MAX_HIDDEN)
    if tuple(weight.shape) != (7, H) or weight.dtype != torch.float32:
        raise ValueError(f"deform_output_layer: weight {tuple(weight.shape)} {weight.dtype}, expected float32 (7, {H})")
    if tuple(bias.shape) != (7,) or bias.dtype != torch.float32:
        raise ValueError(f"deform_output_layer: bias {tuple(bias.shape)} {bias.dtype}, expected float32 (7,)")
    means, quats = _param_tensors(initial_params, "deform_output_layer", P)  # attached: gradients reach them
    _check_blocks(max_blocks, "deform_output_layer")
    _need_gpu("x, weight, bias and params", x, weight, bias, means, quats)
    save = torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or bias.requires_grad)
    return _DeformOut.apply(x, weight, bias, means, quats, int(max_blocks), save)


class DeformationNetwork(nn.Module):
    """train.py:80-110 with the reference's parameter names (``fc_in``, ``residual_blocks.N.*``,
    ``fc_out``), so its checkpoints load.  ``forward`` takes the parameter dicts instead of their
    encodings: the input layer encodes on the fly.  ``fc_out`` and the ``+ initial`` update run
    ``deform_output_layer`` on a contiguous float32 GPU (P, H) activation with float32 GPU parameters, in
    training and eval mode alike (unless ``set_fused_output_head(False)``); every other call the torch ops."""

    def __init__(self, hidden_dimension, residual_block_count):
        super().__init__()
        if not 1 <= hidden_dimension <= MAX_HIDDEN:
            raise ValueError(f"DeformationNetwork: hidden dimension {hidden_dimension} outside [1, {MAX_HIDDEN}]")
        self.fc_in = nn.Linear(INPUT_WIDTH, hidden_dimension)
        self.residual_blocks = nn.Sequential(*(ResidualBlock(hidden_dimension) for _ in range(residual_block_count)))
        self.fc_out = nn.Linear(hidden_dimension, 7)

    def _fused_head(self, x):
        w, b = self.fc_out.weight, self.fc_out.bias
        return (_FUSED_HEAD and b is not None and _eligible(x, w, b) and tuple(w.shape) == (7, x.shape[1])
                and x.shape[1] <= MAX_HIDDEN)

    def forward(self, initial_params, previous_params, timestep, timestep_count):
        out = deform_input_layer(self.fc_in.weight, self.fc_in.bias, initial_params, previous_params,
                                 timestep / timestep_count)
        out = self.residual_blocks(out)
        if self._fused_head(out):
            return deform_output_layer(out, self.fc_out.weight, self.fc_out.bias, initial_params)
        out = self.fc_out(out)
        return out + torch.cat((initial_params["means"], initial_params["rotation_quaternions"]), dim=1)


def update_gaussian_cloud_parameters(network, initial_params, previous_params, timestep, timestep_count):
    """train.py:269-308: the cloud of this timestep -- the initial means and quaternions (detached) plus
    0.01 of the network's output, every other entry passed through."""
    delta = network(initial_params, previous_params, timestep, timestep_count)
    updated = dict(initial_params)
    updated["means"] = initial_params["means"].detach() + delta[:, :3] * 0.01
    updated["rotation_quaternions"] = initial_params["rotation_quaternions"].detach() + delta[:, 3:] * 0.01
    return updated
