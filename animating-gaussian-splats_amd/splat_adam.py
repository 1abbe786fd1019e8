"""Fused Adam over the per-Gaussian parameters on the HIP kernel of ``libgsr.so``.

``FusedAdam`` is a drop-in for the ``torch.optim.Adam`` of densify.py:68-86 (one named param group
per parameter, ``lr=0.0`` default, ``eps=1e-15``): same constructor arguments, ``param_groups`` and
per-parameter ``state`` (``step`` CPU scalar tensor, ``exp_avg``, ``exp_avg_sq``), so the reference's
optimizer surgery (external.py:127-204) and ``splat_densify`` work on it unchanged.  ``step()``
updates every parameter with a gradient in ONE kernel launch, with torch's ``_multi_tensor_adam``
operation order: parameters, both moments and ``step`` are bitwise those of ``torch.optim.Adam`` on the
same device (tests/test_adam.py), also for gradients that are exactly zero, whose square underflows or is
subnormal (1e-30, 1e-22), or huge (1e18): no gradient class needs an ulp allowance.  Supported
configuration: the reference's -- no weight decay, no AMSGrad, not maximising.  There is no CPU path.

``gradient_norm`` is the drop-in for train.py:432-443 ``calculate_gradient_norm`` (one
``.norm(2).pow(2)`` and one blocking host read per parameter there): the L2 norm over every gradient as a
device scalar, from at most two launches per 16 tensors and without a host synchronisation.
``FusedAdam.step(grad_norm=True)`` takes the same norm from the update's own launches.  Both give
``sqrt(sum_t sum_i g_ti^2)`` accumulated in double and rounded once to float32 (include/gsr.h
gsr_grad_norm has the NaN, large-gradient and repeatability rules; tests/test_gradnorm_gpu.py).
"""
from __future__ import annotations

import ctypes

import torch

from diff_gaussian_rasterization import _C

__all__ = ["FusedAdam", "gradient_norm"]


class _AdamTensor(ctypes.Structure):
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("numel", ctypes.c_longlong), ("lr", ctypes.c_double),
                ("step", ctypes.c_double)]


class _GradTensor(ctypes.Structure):  # gsr_grad_tensor
    _fields_ = [("grad", ctypes.c_void_p), ("numel", ctypes.c_longlong)]


_bound = False


def _lib():
    global _bound
    L = _C.load_library()
    if not _bound:
        L.gsr_adam_step.restype = ctypes.c_int
        L.gsr_adam_step.argtypes = [ctypes.c_int, ctypes.POINTER(_AdamTensor), ctypes.c_double, ctypes.c_double,
                                    ctypes.c_double, ctypes.c_void_p]
        _bound = True
    return L


def _float32_contiguous(g):
    return g if g.is_contiguous() and g.dtype == torch.float32 else g.contiguous().float()


def _norm_buffers(L, numels, device):
    """(workspace, squared norms, norm) of a norm over tensors of ``numels`` elements: uninitialised
    device tensors (the kernels write every value that is read)."""
    arr = (ctypes.c_longlong * len(numels))(*numels)
    nbytes = L.gsr_grad_norm_workspace_bytes(len(numels), arr)
    return (torch.empty(nbytes // 8, dtype=torch.float64, device=device),
            torch.empty(len(numels), dtype=torch.float32, device=device),
            torch.empty((), dtype=torch.float32, device=device))


def gradient_norm(parameters, per_tensor=False):
    """``calculate_gradient_norm`` (train.py:432-443) of a module, or of an iterable of parameters (tensors
    with ``.grad``): the L2 norm over all their gradients as a 0-dim float32 device tensor; parameters
    whose ``grad`` is None are skipped, as there.  ``per_tensor=True``: ``(norm, squared_norms)``, the
    second a float32 vector with each gradient's squared norm, in parameter order.  Gradients that are not
    contiguous float32 are converted as ``FusedAdam.step`` converts them.  Without any gradient the norm
    is a device 0.0 (the reference's expression gives ``tensor(0.)``).  Nothing is synchronised."""
    if isinstance(parameters, torch.nn.Module):
        parameters = parameters.parameters()
    elif isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads, device, first = [], None, None
    for p in parameters:
        first = p.device if first is None else first
        g = p.grad
        if g is None:
            continue
        if g.is_sparse:
            raise RuntimeError("gradient_norm: sparse gradients are not supported")
        if not g.is_cuda:
            raise RuntimeError("gradient_norm: GPU gradients only (no CPU path)")
        if device is not None and g.device != device:
            raise RuntimeError(f"gradient_norm: gradients on more than one device ({device}, {g.device})")
        device = g.device
        grads.append(g)
    grads = [_float32_contiguous(g.detach()) for g in grads]  # after every refusal
    if not grads:
        device = first if first is not None and first.type == "cuda" else torch.device("cuda")
        norm = torch.zeros((), dtype=torch.float32, device=device)
        return (norm, torch.zeros(0, dtype=torch.float32, device=device)) if per_tensor else norm
    L = _C.feature_library("gradnorm")
    ws, sq, norm = _norm_buffers(L, [g.numel() for g in grads], device)
    arr = (_GradTensor * len(grads))(*[_GradTensor(g.data_ptr() if g.numel() else None, g.numel()) for g in grads])
    with _C._device_guard(device):
        _C._check(L.gsr_grad_norm(len(grads), ctypes.addressof(arr), ws.data_ptr(), sq.data_ptr(), norm.data_ptr(),
                                  _C._stream_ptr(device)))
    return (norm, sq) if per_tensor else norm


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False,
                 maximize=False):
        if weight_decay != 0 or amsgrad or maximize:
            raise NotImplementedError("FusedAdam: weight_decay / amsgrad / maximize are not supported "
                                      "(the reference uses plain Adam)")
        if not 0.0 <= lr or not 0.0 <= eps or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError("FusedAdam: invalid lr / eps / betas")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0.0, amsgrad=False,
                                      maximize=False))
        self.grad_norm = None     # step(grad_norm=True): 0-dim float32 device tensor
        self.grad_sqnorms = None  # ... and each consumed gradient's squared norm, in the order visited

    @torch.no_grad()
    def step(self, closure=None, *, grad_norm=False):
        """``grad_norm=True``: the update's launches also reduce the gradients they read; afterwards
        ``self.grad_norm`` is their L2 norm (0-dim float32 device tensor) and ``self.grad_sqnorms`` the
        float32 vector of each one's squared norm, in the order the parameters with gradients were visited
        (group by group) -- bitwise ``gradient_norm(..., per_tensor=True)`` on the same gradients, with no
        host synchronisation.  The update itself is the same bit for bit."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = _lib()
        by_cfg = {}
        visit = {}  # configuration -> its tensors' positions in the visit order (= in keep)
        keep = []
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32:
                    raise RuntimeError("FusedAdam: float32 GPU parameters only (no CPU path)")
                if p.grad.is_sparse:
                    raise RuntimeError("FusedAdam: sparse gradients are not supported")
                st = self.state[p]
                if len(st) == 0:  # torch.optim.Adam's lazy state (step on the CPU, moments like p)
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                if not (p.is_contiguous() and st["exp_avg"].is_contiguous() and st["exp_avg_sq"].is_contiguous()):
                    raise RuntimeError("FusedAdam: contiguous parameters and moments required")
                g = p.grad if p.grad.is_contiguous() and p.grad.dtype == torch.float32 else p.grad.contiguous().float()
                keep.append(g)
                visit.setdefault((b1, b2, group["eps"], p.device), []).append(len(keep) - 1)
                by_cfg.setdefault((b1, b2, group["eps"], p.device), []).append(
                    _AdamTensor(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                p.numel(), float(group["lr"]), float(st["step"].item())))
        if grad_norm:
            self._step_with_norm(by_cfg, visit, keep)
            return loss
        for (b1, b2, eps, dev), ts in by_cfg.items():
            arr = (_AdamTensor * len(ts))(*ts)
            _C._check(L.gsr_adam_step(len(ts), arr, float(b1), float(b2), float(eps), _C._stream_ptr(dev)))
        return loss

    def _step_with_norm(self, by_cfg, visit, grads):
        """One gsr_adam_step_norm per configuration over one workspace: the k-th gradient visited owns
        slot k, the last call sums the slots."""
        devices = {cfg[3] for cfg in by_cfg}
        if len(devices) > 1:
            raise RuntimeError(f"FusedAdam: grad_norm over gradients on more than one device ({sorted(map(str, devices))})")
        if not by_cfg:
            first = next((p.device for group in self.param_groups for p in group["params"]), None)
            dev = first if first is not None and first.type == "cuda" else torch.device("cuda")
            self.grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
            self.grad_sqnorms = torch.zeros(0, dtype=torch.float32, device=dev)
            return
        L = _C.feature_library("gradnorm")
        dev = devices.pop()
        ws, sq, norm = _norm_buffers(L, [g.numel() for g in grads], dev)
        calls = list(by_cfg.items())
        with _C._device_guard(dev):
            for c, (cfg, ts) in enumerate(calls):
                arr = (_AdamTensor * len(ts))(*ts)
                slots = (ctypes.c_int * len(ts))(*visit[cfg])
                _C._check(L.gsr_adam_step_norm(len(ts), ctypes.addressof(arr), float(cfg[0]), float(cfg[1]),
                                               float(cfg[2]), ws.data_ptr(), slots, len(grads),
                                               int(c == len(calls) - 1), sq.data_ptr(), norm.data_ptr(),
                                               _C._stream_ptr(dev)))
        self.grad_norm, self.grad_sqnorms = norm, sq
