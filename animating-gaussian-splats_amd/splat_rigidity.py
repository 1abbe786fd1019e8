"""Rigidity loss and neighbour search of train.py on the HIP kernels of ``libgsr.so``.

Drop-ins for the three rigidity call sites of the reference's ``train.py``:

* ``create_neighbor_info(params, k=20)`` -- train.py:166-182, with ``knn`` in place of the open3d
  KD-tree loop of ``compute_knn_indices_and_squared_distances`` (shared.py:45-61);
* ``create_foreground_info(params, indices)`` -- train.py:228-248;
* ``calculate_rigidity_loss(params, neighbor_info, foreground_info)`` -- train.py:325-351, one forward
  kernel and one backward kernel (csrc/gsr_rigidity.hip) instead of a dozen torch ops over
  ``(F, k, 3)`` intermediates and an autograd scatter.

The state a timestep hands to the next one (what ``create_foreground_info`` restates with torch ops) also
comes from the kernels, in one launch and without a host synchronisation:

* ``foreground_info(params, neighbor_info)`` -- the state of a cloud on its own (a sequence's first
  timestep, inference), from the packed neighbour lists;
* ``calculate_rigidity_loss_and_state(params, neighbor_info, foreground_info)`` -- the loss and, as a side
  output of its forward kernel, the state of the cloud it evaluated.

Both return a ``ForegroundInfo`` whose ``(F, k, 3)`` offsets are a view of the kernels' ``(k, 3, F)`` buffer.

``knn`` is exact (brute force, float64 distances from the fp32 coordinates).  A point is excluded from
its own list BY INDEX -- the reference drops "the first result" of a (k + 1)-query, which is the query
point only when no other point coincides with it -- and equal distances are ordered by the lower
index, so the result is defined for the coincident means densification's clones start from (there the
reference returns whatever its KD-tree happens to visit first).

The kernels read a neighbour-major packed form of the neighbour lists (``PackedNeighbors``), built
once by ``create_neighbor_info``; an object with only the reference's fields (``indices`` (F, k) int64,
``weights`` (F, k)) is packed on first use.  Gradients flow to ``params["means"]`` and
``params["rotation_quaternions"]`` only.  There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from diff_gaussian_rasterization import _C

__all__ = ["knn", "NeighborInfo", "ForegroundInfo", "PackedNeighbors", "pack_neighbors", "create_neighbor_info",
           "create_foreground_info", "calculate_rigidity_loss", "foreground_info",
           "calculate_rigidity_loss_and_state"]

MAX_K = 32


def _need_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"splat_rigidity: {what} must be on the GPU (no CPU path)")


def knn(points, k=20):
    """The ``k`` nearest other points of each of ``points`` (n, 3) float32: ``(indices int64 (n, k),
    squared_distances float64 (n, k))``, ascending in distance, ties by the lower index, self excluded
    by index (shared.py:45-61 ``compute_knn_indices_and_squared_distances``)."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"knn: expected points of shape (n, 3), got {tuple(points.shape)}")
    n = points.shape[0]
    if not 1 <= k <= MAX_K:
        raise ValueError(f"knn: k must be in [1, {MAX_K}], got {k}")
    if n <= k:
        raise ValueError(f"knn: {n} points have no {k} other points each (the reference would build ragged lists)")
    _need_gpu(points, "points")
    pts = points.detach().contiguous()
    _C._ptr(pts)  # float32 check
    if not bool(torch.isfinite(pts).all()):
        raise ValueError("knn: points must be finite")
    L = _C.load_library()
    idx = torch.empty((n, k), dtype=torch.int32, device=pts.device)
    d2 = torch.empty((n, k), dtype=torch.float64, device=pts.device)
    with _C._device_guard(pts.device):
        _C._check(L.gsr_knn(n, pts.data_ptr(), int(k), idx.data_ptr(), d2.data_ptr(), _C._stream_ptr(pts.device)))
    return idx.long(), d2


@dataclass
class PackedNeighbors:
    """What the kernels read.  ``foreground_rows`` (F) int32: row of foreground Gaussian i in the
    (P, .) parameter arrays, ``row_to_foreground`` (P) int32 its inverse (-1: background);
    ``neighbor_rows`` (k, F) int32: ROW of i's j-th neighbour; ``weights`` (k, F) float32;
    ``reverse_offsets`` (F + 1) / ``reverse_edges`` (F k) int32: CSR over the edges j * F + i that list
    each Gaussian, in ascending edge order (the backward's summation order)."""
    P: int
    F: int
    k: int
    foreground_rows: torch.Tensor
    row_to_foreground: torch.Tensor
    neighbor_rows: torch.Tensor
    weights: torch.Tensor
    reverse_offsets: torch.Tensor
    reverse_edges: torch.Tensor


@dataclass
class NeighborInfo:
    """train.py's NeighborInfo (``indices`` (F, k) int64 into the foreground Gaussians, ``weights``
    (F, k) float32) plus the packed form."""
    indices: torch.Tensor
    weights: torch.Tensor
    packed: Optional[PackedNeighbors] = None


@dataclass
class ForegroundInfo:
    """train.py's ForegroundInfo (``inverted_rotations`` (F, 4), ``offsets_to_neighbors`` (F, k, 3)) plus
    the offsets in the kernels' (k, 3, F) layout."""
    inverted_rotations: torch.Tensor
    offsets_to_neighbors: torch.Tensor
    packed_offsets: Optional[torch.Tensor] = None


def _foreground_rows(params):
    mask = params["segmentation_masks"][:, 0] > 0.5
    return mask.nonzero().squeeze(1)


def _check_indices(indices, F, what):
    """(F, k) integer indices into [0, F): one host read."""
    if indices.dim() != 2 or indices.shape[0] != F:
        raise ValueError(f"{what}: expected indices of shape ({F}, k) for {F} foreground Gaussians, got "
                         f"{tuple(indices.shape)}")
    if indices.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"{what}: indices must be int64 or int32, got {indices.dtype}")
    if indices.numel() == 0:
        raise ValueError(f"{what}: empty neighbour lists")
    lo, hi = torch.stack((indices.min(), indices.max())).tolist()
    if lo < 0 or hi >= F:
        raise ValueError(f"{what}: neighbour indices span [{lo}, {hi}], outside [0, {F})")


def pack_neighbors(params, indices, weights):
    """The packed form of neighbour lists over the foreground Gaussians of ``params`` (segmentation
    mask > 0.5).  Validates the shapes and the index range (one host synchronisation, here and not per
    step): a bad index is a ``ValueError``, not a GPU fault."""
    means = params["means"]
    _need_gpu(means, "params")
    _need_gpu(indices, "neighbour indices")
    _need_gpu(weights, "neighbour weights")
    rows = _foreground_rows(params)
    P, F = means.shape[0], rows.shape[0]
    _check_indices(indices, F, "pack_neighbors")
    k = indices.shape[1]
    if tuple(weights.shape) != (F, k):
        raise ValueError(f"pack_neighbors: weights {tuple(weights.shape)} do not match indices {(F, k)}")
    if F * k >= 2 ** 31:
        raise ValueError("pack_neighbors: more than 2^31 edges")
    dev = means.device
    idx = indices.long()
    row_to_fg = torch.full((P,), -1, dtype=torch.int32, device=dev)
    row_to_fg[rows] = torch.arange(F, dtype=torch.int32, device=dev)
    targets = idx.t().reshape(-1)  # target of edge e = j * F + i
    order = torch.sort(targets, stable=True).indices
    offsets = torch.zeros(F + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(torch.bincount(targets, minlength=F), 0)
    return PackedNeighbors(P=P, F=F, k=k, foreground_rows=rows.int().contiguous(), row_to_foreground=row_to_fg,
                           neighbor_rows=rows[idx].t().int().contiguous(),
                           weights=weights.detach().float().t().contiguous(),
                           reverse_offsets=offsets.int().contiguous(), reverse_edges=order.int().contiguous())


def create_neighbor_info(params, k=20):
    """train.py:166-182: the ``k`` nearest foreground neighbours of every foreground Gaussian and the
    weights ``exp(-2000 d^2)`` (evaluated in float64, stored float32), with the packed form."""
    means = params["means"]
    _need_gpu(means, "params")
    rows = _foreground_rows(params)
    indices, d2 = knn(means.detach()[rows].float(), k)
    weights = torch.exp(-2000 * d2).float().contiguous()
    indices = indices.contiguous()
    return NeighborInfo(indices=indices, weights=weights, packed=pack_neighbors(params, indices, weights))


def _pack_offsets(offsets):
    return offsets.detach().float().permute(1, 2, 0).contiguous()  # (F, k, 3) -> (k, 3, F)


def create_foreground_info(params, indices):
    """train.py:228-248: the normalised foreground rotations, conjugated, and the offsets from every
    foreground Gaussian to its neighbours -- the state the next timestep's rigidity term compares with."""
    means = params["means"].detach()
    _need_gpu(means, "params")
    rows = _foreground_rows(params)
    _check_indices(indices, rows.shape[0], "create_foreground_info")
    rot = torch.nn.functional.normalize(params["rotation_quaternions"].detach())[rows]
    rot[:, 1:] = -1 * rot[:, 1:]
    fg = means[rows]
    offsets = (fg[indices.long()] - fg[:, None]).contiguous()
    return ForegroundInfo(inverted_rotations=rot.contiguous(), offsets_to_neighbors=offsets,
                          packed_offsets=_pack_offsets(offsets))


def _cached(obj, name, key, make):
    """``make()`` remembered on ``obj`` under ``name`` while ``key`` (the source tensors' storage and
    version) stays the same; objects that take no attributes are packed on every call."""
    hit = getattr(obj, name, None)
    if hit is not None and hit[0] == key:
        return hit[1]
    value = make()
    try:
        setattr(obj, name, (key, value))
    except (AttributeError, TypeError):
        pass
    return value


def _key(*ts):
    return tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in ts)


def _packed_neighbors(params, info):
    packed = getattr(info, "packed", None)
    if packed is None:
        packed = _cached(info, "_gsr_packed", _key(info.indices, info.weights),
                         lambda: pack_neighbors(params, info.indices, info.weights))
    if packed.P != params["means"].shape[0]:
        raise ValueError(f"rigidity: the neighbour info was built for {packed.P} Gaussians, the parameters hold "
                         f"{params['means'].shape[0]}")
    return packed


def _packed_offsets(info, F, k):
    off = info.offsets_to_neighbors
    if tuple(off.shape) != (F, k, 3):
        raise ValueError(f"rigidity: offsets_to_neighbors {tuple(off.shape)} do not match the neighbour lists "
                         f"{(F, k, 3)}")
    if tuple(info.inverted_rotations.shape) != (F, 4):
        raise ValueError(f"rigidity: inverted_rotations {tuple(info.inverted_rotations.shape)}, expected {(F, 4)}")
    packed = getattr(info, "packed_offsets", None)
    if packed is None:
        packed = _cached(info, "_gsr_packed_offsets", _key(off), lambda: _pack_offsets(off))
    return packed


def _empty_state(nb, dev):
    """Uninitialised (inverted rotations (F, 4), offsets (k, 3, F)): the kernels write every element."""
    return (torch.empty((nb.F, 4), dtype=torch.float32, device=dev),
            torch.empty((nb.k, 3, nb.F), dtype=torch.float32, device=dev))


def _state_info(inv, packed):
    """ForegroundInfo over the kernels' two arrays: the reference-layout offsets are a view of ``packed``."""
    return ForegroundInfo(inverted_rotations=inv, offsets_to_neighbors=packed.permute(2, 0, 1), packed_offsets=packed)


class _Rigidity(torch.autograd.Function):
    """``state``: also return the evaluated cloud's own (inverted rotations, packed offsets), non-differentiable."""

    @staticmethod
    def forward(ctx, means, quats, nb, prev_off, prev_inv, state=False):
        L = _C.feature_library("foreground") if state else _C.load_library()
        m, q = means.contiguous(), quats.contiguous()
        for t in (m, q, prev_off, prev_inv):
            _C._ptr(t)  # GPU + float32 checks (no CPU path)
        dev = m.device
        save = bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        scratch = torch.empty(L.gsr_rigidity_scratch_bytes(nb.F, nb.k, int(save)), dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        args = (nb.P, nb.F, nb.k, m.data_ptr(), q.data_ptr(), nb.foreground_rows.data_ptr(),
                nb.neighbor_rows.data_ptr(), nb.weights.data_ptr(), prev_off.data_ptr(), prev_inv.data_ptr(),
                scratch.data_ptr(), int(save), loss.data_ptr())
        with _C._device_guard(dev):
            if state:
                inv, off = _empty_state(nb, dev)
                _C._check(L.gsr_rigidity_forward_state(*args, inv.data_ptr(), off.data_ptr(), _C._stream_ptr(dev)))
            else:
                _C._check(L.gsr_rigidity_forward(*args, _C._stream_ptr(dev)))
        if save:
            ctx.save_for_backward(scratch)
            ctx.nb = nb
        ctx.set_materialize_grads(False)
        if state:
            ctx.mark_non_differentiable(inv, off)
            return loss, inv, off
        return loss

    @staticmethod
    def backward(ctx, g, *_state_grads):
        nothing = (None,) * (len(ctx.needs_input_grad) - 2)  # nb, the previous state, the flag
        if g is None:
            return (None, None) + nothing
        L = _C.load_library()
        (scratch,) = ctx.saved_tensors
        nb = ctx.nb
        dev = scratch.device
        g = g.contiguous().float()
        dm = torch.empty((nb.P, 3), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dq = torch.empty((nb.P, 4), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        with _C._device_guard(dev):
            _C._check(L.gsr_rigidity_backward(nb.P, nb.F, nb.k, nb.row_to_foreground.data_ptr(),
                                              nb.reverse_offsets.data_ptr(), nb.reverse_edges.data_ptr(),
                                              scratch.data_ptr(), g.data_ptr(),
                                              dm.data_ptr() if dm is not None else None,
                                              dq.data_ptr() if dq is not None else None, _C._stream_ptr(dev)))
        return (dm, dq) + nothing


def calculate_rigidity_loss(params, neighbor_info, foreground_info):
    """train.py:325-351.  ``neighbor_info`` / ``foreground_info``: this module's objects or any with the
    reference's fields.  The foreground set is the one the neighbour info was built (or first used)
    with; the segmentation masks are not re-read per step."""
    means, quats = params["means"], params["rotation_quaternions"]
    _need_gpu(means, "params")
    _need_gpu(quats, "params")
    P = means.shape[0]
    if tuple(means.shape) != (P, 3) or tuple(quats.shape) != (P, 4):
        raise ValueError(f"rigidity: means {tuple(means.shape)} / rotation_quaternions {tuple(quats.shape)}, "
                         f"expected (P, 3) / (P, 4)")
    nb = _packed_neighbors(params, neighbor_info)
    prev_off = _packed_offsets(foreground_info, nb.F, nb.k)
    prev_inv = foreground_info.inverted_rotations.detach().float().contiguous()
    return _Rigidity.apply(means, quats, nb, prev_off, prev_inv)


def _checked_cloud(params):
    """(means (P, 3), rotation_quaternions (P, 4)) of ``params`` for the state calls: shapes and float32
    are a ``ValueError``, a CPU tensor raises (no CPU path)."""
    means, quats = params["means"], params["rotation_quaternions"]
    P = means.shape[0]
    if tuple(means.shape) != (P, 3) or tuple(quats.shape) != (P, 4):
        raise ValueError(f"rigidity: means {tuple(means.shape)} / rotation_quaternions {tuple(quats.shape)}, "
                         f"expected (P, 3) / (P, 4)")
    if means.dtype != torch.float32 or quats.dtype != torch.float32:
        raise ValueError(f"rigidity: means {means.dtype} / rotation_quaternions {quats.dtype}, expected float32")
    _need_gpu(means, "params")
    _need_gpu(quats, "params")
    return means, quats


def foreground_info(params, neighbor_info):
    """``create_foreground_info`` (train.py:228-248) of the cloud ``params`` in one kernel launch, from the
    packed neighbour lists: no torch op over (F, .) data and no host synchronisation (a bare object with
    only ``indices`` / ``weights`` is packed and validated once, as in ``calculate_rigidity_loss``).  The
    inputs are detached.  The offsets are written once, in the kernels' (k, 3, F) layout
    (``packed_offsets``); ``offsets_to_neighbors`` (F, k, 3) is a view of that buffer."""
    means, quats = _checked_cloud(params)
    nb = _packed_neighbors(params, neighbor_info)
    if nb.k > MAX_K:
        raise ValueError(f"foreground_info: k must be in [1, {MAX_K}], got {nb.k}")
    L = _C.feature_library("foreground")
    m, q = means.detach().contiguous(), quats.detach().contiguous()
    dev = m.device
    inv, off = _empty_state(nb, dev)
    with _C._device_guard(dev):
        _C._check(L.gsr_foreground_info(nb.P, nb.F, nb.k, m.data_ptr(), q.data_ptr(), nb.foreground_rows.data_ptr(),
                                        nb.neighbor_rows.data_ptr(), inv.data_ptr(), off.data_ptr(),
                                        _C._stream_ptr(dev)))
    return _state_info(inv, off)


def calculate_rigidity_loss_and_state(params, neighbor_info, foreground_info):
    """``(calculate_rigidity_loss(params, neighbor_info, foreground_info), foreground_info(params,
    neighbor_info))`` from one forward kernel: the state of the evaluated cloud is stored from the values
    the loss is computed with.  The loss carries the same gradients as ``calculate_rigidity_loss``'s; the
    state is not differentiable."""
    means, quats = _checked_cloud(params)
    nb = _packed_neighbors(params, neighbor_info)
    if nb.k > MAX_K:
        raise ValueError(f"calculate_rigidity_loss_and_state: k must be in [1, {MAX_K}], got {nb.k}")
    prev_off = _packed_offsets(foreground_info, nb.F, nb.k)
    prev_inv = foreground_info.inverted_rotations.detach().float().contiguous()
    loss, inv, off = _Rigidity.apply(means, quats, nb, prev_off, prev_inv, True)
    return loss, _state_info(inv, off)
