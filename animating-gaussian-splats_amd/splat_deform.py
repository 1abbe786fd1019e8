"""The deformation network of train.py with its input side on the HIP kernels of ``libgsr.so``.

Every step the reference re-encodes the previous cloud (``normalize_and_encode_means_and_rotations``,
train.py:185-204), repeats the progress encoding over all rows, ``torch.cat``s both with the initial
encoding into a (P, 192) matrix and feeds it to ``fc_in`` (train.py:96-104, 269-294).  Here that matrix
never exists: ``deform_input_layer`` computes ``fc_in``'s output straight from the 14 floats per
Gaussian (csrc/gsr_deform.hip), and its backward recomputes the features for ``dW``.

* ``encode_means_and_rotations(params)`` -- train.py:185-204, the (P, 92) encoding as a tensor;
* ``deform_input_layer(weight, bias, initial_params, previous_params, progress)`` -- ``fc_in`` applied
  to ``[enc(initial) | enc(previous) | enc(progress)]``; gradients flow to ``weight`` and ``bias`` only
  (the reference detaches the encoded parameters, train.py:255-258);
* ``DeformationNetwork`` -- train.py:80-110 with the reference's ``state_dict`` names and shapes; the
  residual blocks (training-mode BatchNorm over all rows, H x H GEMMs) and ``fc_out`` stay torch;
* ``update_gaussian_cloud_parameters`` -- train.py:269-308.

All fp32.  There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

import torch
from torch import nn

from diff_gaussian_rasterization import _C

__all__ = ["encode_means_and_rotations", "encoding_ranges", "deform_input_layer", "ResidualBlock",
           "DeformationNetwork", "update_gaussian_cloud_parameters", "MAX_HIDDEN"]

MAX_HIDDEN = 512
ENCODING_WIDTH = 92  # 3 means x 10 frequencies x (sin, cos) + 4 quaternion components x 4 x 2
INPUT_WIDTH = 192    # two encodings + the 8 progress columns
RANGE_BLOCKS = 256   # GSR_POSENC_RANGE_BLOCKS of include/gsr.h


def _means_and_rotations(params, what):
    """The (P, 3) means and (P, 4) raw quaternions of ``params``, detached, fp32, contiguous."""
    means, quats = params["means"], params["rotation_quaternions"]
    P = means.shape[0] if means.dim() else -1
    if tuple(means.shape) != (P, 3) or tuple(quats.shape) != (P, 4):
        raise ValueError(f"{what}: means {tuple(means.shape)} / rotation_quaternions {tuple(quats.shape)}, "
                         f"expected (P, 3) / (P, 4)")
    for t in (means, quats):
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: expected float32 parameters, got {t.dtype}")
    return means.detach().contiguous(), quats.detach().contiguous()


def _need_gpu(what, *tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"splat_deform: {what} must be on the GPU (no CPU path)")


def encoding_ranges(means, quats):
    """The 14 floats the normalisation needs: per column (means xyz, quaternion wxyz) the minimum and
    the maximum of ``x - minimum`` (train.py:190-197), exact in fp32: one pass over the (P >= 1) rows."""
    L = _C.deform_library()
    dev = means.device
    if means.shape[0] == 0:
        return torch.zeros(14, dtype=torch.float32, device=dev)
    buf = torch.empty(14 * (RANGE_BLOCKS + 1), dtype=torch.float32, device=dev)  # the ranges, then the partials
    with _C._device_guard(dev):
        _C._check(L.gsr_posenc_ranges(means.shape[0], means.data_ptr(), quats.data_ptr(), buf[14:].data_ptr(),
                                      buf.data_ptr(), _C._stream_ptr(dev)))
    return buf[:14]


def encode_means_and_rotations(params):
    """train.py:185-204 ``normalize_and_encode_means_and_rotations``: (P, 92) float32."""
    means, quats = _means_and_rotations(params, "encode_means_and_rotations")
    _need_gpu("params", means, quats)
    L = _C.deform_library()
    P, dev = means.shape[0], means.device
    out = torch.empty((P, ENCODING_WIDTH), dtype=torch.float32, device=dev)
    if P == 0:
        return out
    ranges = encoding_ranges(means, quats)
    with _C._device_guard(dev):
        _C._check(L.gsr_posenc_forward(P, means.data_ptr(), quats.data_ptr(), ranges.data_ptr(), out.data_ptr(),
                                       _C._stream_ptr(dev)))
    return out


class _DeformIn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, bias, im, iq, ir, pm, pq, pr, progress, max_blocks, save):
        L = _C.deform_library()
        w, b = weight.detach().contiguous(), bias.detach().contiguous()
        P, H, dev = im.shape[0], w.shape[0], im.device
        out = torch.empty((P, H), dtype=torch.float32, device=dev)
        with _C._device_guard(dev):
            _C._check(L.gsr_deform_in_forward(P, H, im.data_ptr(), iq.data_ptr(), ir.data_ptr(), pm.data_ptr(),
                                              pq.data_ptr(), pr.data_ptr(), progress, w.data_ptr(), b.data_ptr(),
                                              out.data_ptr(), _C._stream_ptr(dev)))
        if save:
            ctx.save_for_backward(im, iq, ir, pm, pq, pr)
            ctx.progress, ctx.max_blocks, ctx.H = progress, max_blocks, H
        return out

    @staticmethod
    def backward(ctx, g):
        L = _C.deform_library()
        im, iq, ir, pm, pq, pr = ctx.saved_tensors
        P, H, dev = im.shape[0], ctx.H, im.device
        g = g.contiguous().float()
        dw = torch.empty((H, INPUT_WIDTH), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        db = torch.empty((H,), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        if P == 0:
            return (dw.zero_() if dw is not None else None, db.zero_() if db is not None else None) + (None,) * 9
        ws = torch.empty(max(L.gsr_deform_in_workspace_bytes(P, H, ctx.max_blocks), 1), dtype=torch.uint8, device=dev)
        with _C._device_guard(dev):
            _C._check(L.gsr_deform_in_backward(P, H, im.data_ptr(), iq.data_ptr(), ir.data_ptr(), pm.data_ptr(),
                                               pq.data_ptr(), pr.data_ptr(), ctx.progress, g.data_ptr(), ws.data_ptr(),
                                               ctx.max_blocks, dw.data_ptr() if dw is not None else None,
                                               db.data_ptr() if db is not None else None, _C._stream_ptr(dev)))
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
    if max_blocks < 0:
        raise ValueError("deform_input_layer: max_blocks must be >= 0")
    _need_gpu("weight, bias and params", weight, bias, im, iq, pm, pq)
    ir, pr = encoding_ranges(im, iq), encoding_ranges(pm, pq)
    # the reference builds the scalar as torch.tensor(timestep / timestep_count): rounded to fp32 once
    progress = float(torch.tensor(float(progress), dtype=torch.float32))
    save = torch.is_grad_enabled() and (weight.requires_grad or bias.requires_grad)  # nothing under no_grad
    return _DeformIn.apply(weight, bias, im, iq, ir, pm, pq, pr, progress, int(max_blocks), save)


class ResidualBlock(nn.Module):
    """train.py:57-77."""

    def __init__(self, dimension):
        super().__init__()
        self.fc1 = nn.Linear(dimension, dimension, bias=False)
        self.bn1 = nn.BatchNorm1d(dimension)
        self.fc2 = nn.Linear(dimension, dimension, bias=False)
        self.bn2 = nn.BatchNorm1d(dimension)

    def forward(self, x):
        identity = x
        x = nn.functional.gelu(self.bn1(self.fc1(x)))
        x = self.bn2(self.fc2(x))
        x = x + identity
        return nn.functional.gelu(x)


class DeformationNetwork(nn.Module):
    """train.py:80-110 with the reference's parameter names (``fc_in``, ``residual_blocks.N.*``,
    ``fc_out``), so its checkpoints load.  ``forward`` takes the parameter dicts instead of their
    encodings: the input layer encodes on the fly."""

    def __init__(self, hidden_dimension, residual_block_count):
        super().__init__()
        if not 1 <= hidden_dimension <= MAX_HIDDEN:
            raise ValueError(f"DeformationNetwork: hidden dimension {hidden_dimension} outside [1, {MAX_HIDDEN}]")
        self.fc_in = nn.Linear(INPUT_WIDTH, hidden_dimension)
        self.residual_blocks = nn.Sequential(*(ResidualBlock(hidden_dimension) for _ in range(residual_block_count)))
        self.fc_out = nn.Linear(hidden_dimension, 7)

    def forward(self, initial_params, previous_params, timestep, timestep_count):
        out = deform_input_layer(self.fc_in.weight, self.fc_in.bias, initial_params, previous_params,
                                 timestep / timestep_count)
        out = self.residual_blocks(out)
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
