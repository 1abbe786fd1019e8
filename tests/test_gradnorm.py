"""Gradient norm (splat_adam.gradient_norm, FusedAdam.step(grad_norm=True), splat_train.step_metrics), the part
that needs no GPU.  tests/gradnorm_ref.py holds the float64 restatement, the tolerance and the shared inputs;
tests/test_gradnorm_gpu.py runs the kernels on them.

Here: each size-driven case of the GPU file gets a restatement of the mistake it exists to catch, applied to
the float64 reference, and the norm must move by more than 100 tolerances; the reference's own float32
expression, evaluated on the CPU, is within the tolerance of the restatement on these inputs (the condition
that the inputs are fair); the workspace size follows the block-count formula; the C ABI and the Python
entry points refuse what they document, before anything is launched.
"""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gradnorm_ref as GR
from diff_gaussian_rasterization import _C

FAIR_CASES = ([("single", n) for n in GR.SINGLE_SIZES] + [("table", n) for n in (17, 33)] + [("two_config", 0)])


def _case(kind, n):
    return {"single": GR.single_case, "table": GR.table_case, "two_config": lambda _: GR.two_config_case()}[kind](n)


def _moves(case, mistake):
    """By how many tolerances (float32 ulps of the right norm) the float64 norm moves under ``mistake``."""
    right, _ = GR.gradient_norm(case)
    wrong, _ = GR.gradient_norm(mistake(case))
    return abs(right - wrong) / GR.ulp32(right)


# ---- sensitivity ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [n for n in GR.SINGLE_SIZES if n % GR.BLOCK])
def test_sensitive_to_a_dropped_partial_block(n):
    assert _moves(GR.single_case(n), GR.drop_last_partial_block) > 100


@pytest.mark.parametrize("n", [n for n in GR.SINGLE_SIZES if n % 4])
def test_sensitive_to_a_dropped_scalar_tail(n):
    assert _moves(GR.single_case(n), GR.drop_tail_past_last_float4) > 100


@pytest.mark.parametrize("n", [17, 33])
def test_sensitive_to_table_overflow_and_the_empty_tensor(n):
    case = GR.table_case(n)
    assert sum(1 for g in case if g is not None and g.size) == n
    assert sum(1 for g in case if g is None) == 1 and sum(1 for g in case if g is not None and not g.size) == 1
    assert _moves(case, GR.drop_after_table) > 100
    assert _moves(case, GR.stop_at_empty) > 100
    # the 17th / 33rd tensor alone, through the mark only it carries in its first element
    late = [g for g in case if g is not None and g.size][16 if n == 17 else 32]
    assert late[0] == GR.MARK

    def without_its_mark(c):
        return [np.concatenate([[np.float32(0)], g[1:]]) if g is late else g for g in c]

    assert _moves(case, without_its_mark) > 100


def test_sensitive_to_the_second_configuration():
    case = GR.two_config_case()
    assert sorted(i for grp in GR.TWO_CONFIG_GROUPS for i in grp) == list(range(len(case)))
    assert GR.TWO_CONFIG_SETTINGS[0] == GR.TWO_CONFIG_SETTINGS[2] != GR.TWO_CONFIG_SETTINGS[1]
    assert _moves(case, GR.drop_second_configuration) > 100


def test_one_marked_element_is_worth_a_million_tolerances():
    cases = [GR.single_case(n)[0] for n in (1, 3, 1023, 1024, 1025, 2049)]
    assert _moves(cases, lambda c: c[:-1] + [c[-1][:-1]]) > 1e6


# ---- the reference against the restatement ------------------------------------------------------------
def _reference_expression(case):
    """train.py:432-443 on CPU tensors."""
    grads = [torch.from_numpy(g) for g in case if g is not None]
    return torch.sqrt(torch.sum(torch.tensor([g.norm(2).pow(2) for g in grads])))


@pytest.mark.parametrize("kind,n", FAIR_CASES)
def test_reference_expression_is_within_the_tolerance(kind, n):
    case = _case(kind, n)
    want, _ = GR.gradient_norm(case)
    off = GR.ulps_off(_reference_expression(case), want)
    print(f"{kind} {n}: the reference's float32 expression is {off:.2f} ulp from float64")
    assert off <= 1


def test_reference_expression_overflows_where_the_restatement_does_not():
    """The documented difference: 1000 x 1e20 has a float32-representable norm, the reference gives inf."""
    big = [np.full(1000, 1e20, np.float32)]
    want, sq = GR.gradient_norm(big)
    assert math.isfinite(float(np.float32(want))) and want == pytest.approx(math.sqrt(1000) * 1e20, rel=1e-6)
    assert math.isinf(float(_reference_expression(big)))
    assert torch.isinf(torch.full((1000,), 1e20).norm(2).pow(2))
    assert GR.ulps_off(float("inf"), sq[0]) == 0 and GR.ulps_off(3e38, sq[0]) == math.inf  # the helper's non-finite rule


# ---- workspace, exports, C ABI refusals -----------------------------------------------------------------
def _lib():
    import splat_adam  # noqa: F401 - binds nothing on import; the structures below are its
    return _C.feature_library("gradnorm")


def test_workspace_bytes_follow_the_block_count():
    L = _lib()

    def size(numels):
        return L.gsr_grad_norm_workspace_bytes(len(numels), (ctypes.c_longlong * len(numels))(*numels))

    assert size([]) == 8  # the total alone
    for numels in ([0], [1], [1024], [1025], [0, 5, 2049, 1024 * 1024 + 1], list(GR.SINGLE_SIZES)):
        blocks = sum((m + GR.BLOCK - 1) // GR.BLOCK for m in numels)
        assert size(numels) == 8 * (1 + len(numels) + blocks), numels  # total, one per tensor, one per block
    assert size([3, -1]) == 0
    assert L.gsr_grad_norm_workspace_bytes(-1, None) == 0 and L.gsr_grad_norm_workspace_bytes(2, None) == 0


def test_symbols_are_exported_as_an_optional_group():
    names = ["gsr_grad_norm_workspace_bytes", "gsr_grad_norm", "gsr_adam_step_norm"]
    assert set(names) <= set(_C.EXPORTED_SYMBOLS)
    assert list(_C._OPTIONAL_EXPORT["gradnorm"][1]) == names
    L = _C.load_library()
    assert not _C._MISSING and all(hasattr(L, n) for n in names)
    assert L.gsr_abi_version() == 21


def test_c_abi_refusals():
    import splat_adam
    L = _lib()
    fake = ctypes.c_void_p(256)  # never dereferenced: every call below returns before a launch
    G, A = splat_adam._GradTensor, splat_adam._AdamTensor

    def grad_norm(tensors, ws=fake, sq=fake, out=fake, n=None):
        arr = (G * max(len(tensors), 1))(*tensors)
        return L.gsr_grad_norm(len(tensors) if n is None else n, ctypes.addressof(arr), ws, sq, out, None)

    for bad, msg in [(dict(ws=None), b"null workspace / out_norm"), (dict(out=None), b"null workspace / out_norm")]:
        assert grad_norm([G(256, 4)], **bad) == 1 and msg in L.gsr_last_error()
        assert grad_norm([], **bad) == 1 and msg in L.gsr_last_error()
    assert grad_norm([G(256, 4), G(256, -1)]) == 1 and b"tensor 1: negative numel" in L.gsr_last_error()
    assert grad_norm([G(256, 4), G(None, 3)]) == 1 and b"tensor 1: null gradient" in L.gsr_last_error()
    assert grad_norm([G(256, 4)], n=-1) == 1 and b"bad tensor list" in L.gsr_last_error()
    assert L.gsr_grad_norm(1, None, fake, fake, fake, None) == 1 and b"bad tensor list" in L.gsr_last_error()
    assert grad_norm([G(256, 1 << 42)]) != 0 and b"too large" in L.gsr_last_error()

    def step_norm(tensors, ws=fake, slots=None, nslots=None, out=fake):
        arr = (A * max(len(tensors), 1))(*tensors)
        sl = None if slots is None else (ctypes.c_int * len(slots))(*slots)
        return L.gsr_adam_step_norm(len(tensors), ctypes.addressof(arr), 0.9, 0.999, 1e-8, ws, sl,
                                    len(tensors) if nslots is None else nslots, 1, fake, out, None)

    good = A(256, 256, 256, 256, 4, 1e-3, 1.0)
    assert step_norm([good], ws=None) == 1 and b"null workspace / out_norm" in L.gsr_last_error()
    assert step_norm([good], out=None) == 1 and b"null workspace / out_norm" in L.gsr_last_error()
    assert step_norm([good, A(256, 256, 256, 256, -4, 1e-3, 1.0)]) == 1 and b"negative numel" in L.gsr_last_error()
    assert step_norm([good, A(256, None, 256, 256, 4, 1e-3, 1.0)]) == 1 and b"tensor 1: null pointer" in L.gsr_last_error()
    assert step_norm([good], slots=[1], nslots=1) == 1 and b"slot 1 outside [0, 1)" in L.gsr_last_error()
    assert step_norm([good], slots=[-1], nslots=1) == 1 and b"slot -1 outside" in L.gsr_last_error()
    assert step_norm([good, good], nslots=1) == 1 and b"2 tensors but 1 slots" in L.gsr_last_error()
    assert step_norm([good], nslots=-1) == 1
    # gsr_adam_step's own refusals are unchanged
    arr = (A * 1)(A(256, 256, 256, 256, 4, 1e-3, 0.0))
    assert splat_adam._lib().gsr_adam_step(1, arr, 0.9, 0.999, 1e-8, None) == 1
    assert b"step must be >= 1" in L.gsr_last_error()


# ---- Python refusals --------------------------------------------------------------------------------------
def test_python_refusals():
    import splat_adam
    p = torch.nn.Parameter(torch.zeros(5))
    p.grad = torch.ones(5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        splat_adam.gradient_norm([p])
    with pytest.raises(RuntimeError, match="no CPU path"):
        splat_adam.gradient_norm(_with_grads())  # a module
    sp = torch.nn.Parameter(torch.zeros(4, 3))
    sp.grad = torch.sparse_coo_tensor(torch.tensor([[1], [2]]), torch.tensor([1.0]), (4, 3))
    with pytest.raises(RuntimeError, match="sparse"):
        splat_adam.gradient_norm([sp])

    def on(device):  # stands for a parameter whose gradient lives on `device`: refused before it is touched
        d = torch.device(device)
        return SimpleNamespace(device=d, grad=SimpleNamespace(is_sparse=False, is_cuda=True, device=d))

    with pytest.raises(RuntimeError, match="more than one device"):
        splat_adam.gradient_norm([on("cuda:0"), on("cuda:1")])
    # the optimizer: CPU parameters are refused with or without the norm
    opt = splat_adam.FusedAdam([p])
    assert opt.grad_norm is None and opt.grad_sqnorms is None
    for flag in (False, True):
        with pytest.raises(RuntimeError, match="no CPU path"):
            opt.step(grad_norm=flag)
    with pytest.raises(TypeError):
        opt.step(None, True)  # keyword only


def _with_grads():
    m = torch.nn.Linear(3, 2)
    for q in m.parameters():
        q.grad = torch.ones_like(q)
    return m


# ---- step_metrics -----------------------------------------------------------------------------------------
def test_step_metrics_order_and_image_expression():
    import splat_train
    assert splat_train.STEP_METRIC_NAMES == ("train-loss/total", "train-loss/l1", "train-loss/ssim",
                                             "train-loss/image", "train-loss/rigidity", "gradient-norm")
    total, l1, ssim, rigid = (torch.tensor(v, dtype=torch.float32) for v in (7.25, 0.3337, 1.4142, 0.0625))
    state = object()  # train_step_loss(next_foreground_info=True)'s fifth element is ignored
    for losses in ((total, l1, ssim, rigid), (total.clone().requires_grad_(True), l1, ssim, rigid, state)):
        m = splat_train.step_metrics(losses, torch.tensor(2.5))
        assert m.shape == (6,) and m.dtype == torch.float32 and not m.requires_grad
        image = torch.tensor(0.8, dtype=torch.float32) * l1 + torch.tensor(0.2, dtype=torch.float32) * ssim
        assert torch.equal(m, torch.stack([total, l1, ssim, image, rigid, torch.tensor(2.5)]))
    log = splat_train.ScoreLog(depth=2)  # through the unchanged ScoreLog
    log.put(3, m)
    (step, values), = log.close()
    assert step == 3 and torch.equal(values, m)
    assert dict(zip(splat_train.STEP_METRIC_NAMES, values.tolist()))["gradient-norm"] == 2.5
