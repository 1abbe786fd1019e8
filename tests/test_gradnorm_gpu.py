"""Gradient norm on the GPU: splat_adam.gradient_norm (k_grad_sumsq + k_norm_final of csrc/gsr_adam.hip) and
FusedAdam.step(grad_norm=True) (k_adam<true> + k_norm_final) against the float64 restatement of
tests/gradnorm_ref.py, each case through both.

Tolerance (gradnorm_ref.py): |got - float32(ref64)| <= 1 float32 ulp of ref64, for the norm and for every
squared norm; tests/test_gradnorm.py shows that each size-driven case here moves the norm by more than 100
tolerances under the mistake it exists to catch.  Beyond the values: results are bitwise repeatable, the
fused step's norm and squared norms are bitwise gradient_norm's, the update under grad_norm=True is bitwise
torch.optim.Adam's (as tests/test_adam.py compares), nothing behind the workspace or the outputs is
written, and nothing synchronises with the host.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import gradnorm_ref as GR
import splat_adam
from diff_gaussian_rasterization import _C

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _parameters(case, dev, seed=0):
    """A parameter per entry of ``case`` with its gradient assigned (None: no gradient)."""
    g = torch.Generator().manual_seed(seed)
    params = []
    for entry in case:
        n = 11 if entry is None else entry.size
        p = torch.nn.Parameter(torch.randn(n, generator=g).to(dev))
        p.grad = None if entry is None else torch.from_numpy(entry).to(dev)
        params.append(p)
    return params


def _both(case, dev, groups=None):
    """(norm, squared norms) of ``case`` from gradient_norm and from FusedAdam.step(grad_norm=True)."""
    params = _parameters(case, dev)
    alone = splat_adam.gradient_norm(params, per_tensor=True)
    opt = splat_adam.FusedAdam(groups(params) if groups else params, lr=1e-3)
    opt.step(grad_norm=True)
    fused = (opt.grad_norm, opt.grad_sqnorms)
    torch.cuda.synchronize()
    for norm, sq in (alone, fused):
        assert norm.shape == () and norm.dtype == torch.float32 and norm.device == dev
        assert sq.dtype == torch.float32 and sq.shape == (sum(1 for e in case if e is not None),)
    return alone, fused


def _check(case, dev, what, groups=None):
    want_norm, want_sq = GR.gradient_norm(case)
    alone, fused = _both(case, dev, groups)
    for name, (norm, sq) in (("gradient_norm", alone), ("step(grad_norm=True)", fused)):
        off = GR.ulps_off(norm.item(), want_norm)
        offs = [GR.ulps_off(g, w) for g, w in zip(sq.tolist(), want_sq)]
        print(f"{what} {name}: norm {norm.item():.9e} float64 {want_norm:.9e} ({off:.2f} ulp), "
              f"squared norms worst {max(offs, default=0.0):.2f} ulp of {len(offs)}")
        assert off <= 1, (what, name)
        assert all(o <= 1 for o in offs), (what, name, offs)
    assert (_bits(fused[0]) == _bits(alone[0])).all(), what
    assert (_bits(fused[1]) == _bits(alone[1])).all(), what
    return alone


@pytest.mark.parametrize("n", GR.SINGLE_SIZES)
def test_single_tensors(cuda, n):
    _check(GR.single_case(n), cuda, f"{n} elements")


@pytest.mark.parametrize("n", [3, 4, 1027, 2049])
def test_unaligned_gradient(cuda, n):
    """A gradient 4 bytes off 16-byte alignment: the scalar branch of k_adam and of the reduction, with whole
    quads and a tail."""
    case = GR.single_case(n)
    want_norm, want_sq = GR.gradient_norm(case)
    buf = torch.zeros(n + 9, device=cuda)
    view = buf[1:1 + n]
    view.copy_(torch.from_numpy(case[0]))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    p = torch.nn.Parameter(torch.zeros(n, device=cuda))
    p.grad = view
    norm, sq = splat_adam.gradient_norm([p], per_tensor=True)
    opt = splat_adam.FusedAdam([p], lr=1e-3)
    opt.step(grad_norm=True)
    for got_norm, got_sq in ((norm, sq), (opt.grad_norm, opt.grad_sqnorms)):
        assert GR.ulps_off(got_norm.item(), want_norm) <= 1 and GR.ulps_off(got_sq.item(), want_sq[0]) <= 1
    aligned = _check(case, cuda, f"{n} elements, aligned")  # the branch taken does not change the bits
    assert (_bits(norm) == _bits(aligned[0])).all() and (_bits(opt.grad_norm) == _bits(aligned[0])).all()
    assert (_bits(sq) == _bits(aligned[1])).all() and (_bits(opt.grad_sqnorms) == _bits(aligned[1])).all()


@pytest.mark.parametrize("n", [17, 33])
def test_table_flush(cuda, n):
    """17 / 33 non-empty tensors: one / two flushes of the 16-entry table; an empty tensor (squared norm 0) and
    a parameter without a gradient (no entry) in the middle."""
    case = GR.table_case(n)
    _, sq = _check(case, cuda, f"{n} tensors")
    empty = [k for k, e in enumerate(e for e in case if e is not None) if e.size == 0]
    assert len(empty) == 1 and sq[empty[0]].item() == 0.0


def test_real_network(cuda):
    import splat_deform
    torch.manual_seed(11)
    net = splat_deform.DeformationNetwork(40, 3).to(cuda)
    rng = np.random.default_rng(40)
    case = [GR.marked(p.numel(), rng) for p in net.parameters()]
    assert len(case) == 22
    for p, g in zip(net.parameters(), case):
        p.grad = torch.from_numpy(g).to(cuda).view_as(p)
    want_norm, want_sq = GR.gradient_norm(case)
    norm, sq = splat_adam.gradient_norm(net, per_tensor=True)  # a module
    opt = splat_adam.FusedAdam(net.parameters(), lr=1e-3)
    opt.step(grad_norm=True)
    for got_norm, got_sq in ((norm, sq), (opt.grad_norm, opt.grad_sqnorms)):
        assert GR.ulps_off(got_norm.item(), want_norm) <= 1
        assert all(GR.ulps_off(g, w) <= 1 for g, w in zip(got_sq.tolist(), want_sq))
    assert (_bits(opt.grad_norm) == _bits(norm)).all() and (_bits(opt.grad_sqnorms) == _bits(sq)).all()
    assert (_bits(splat_adam.gradient_norm(net)) == _bits(norm)).all()  # without per_tensor: the scalar alone


def _two_config_groups(params):
    return [dict(params=[params[i] for i in idx], **kw) for idx, kw in zip(GR.TWO_CONFIG_GROUPS, GR.TWO_CONFIG_SETTINGS)]


def test_two_configurations_one_norm(cuda):
    """Two (betas, eps) configurations in one step(): two launches of the update, one norm over both, the
    squared norms in the order the parameters were visited (not the launches' order)."""
    case = GR.two_config_case()
    _, sq = _check(case, cuda, "two configurations", groups=_two_config_groups)
    _, want_sq = GR.gradient_norm(case)
    assert [GR.ulps_off(g, w) <= 1 for g, w in zip(sq.tolist(), want_sq)] == [True] * 4
    # tensors 2 and 3 change places between the visit order and the launches' order: exchanged, they would be seen
    assert abs(want_sq[2] - want_sq[3]) > 100 * GR.ulp32(want_sq[3])


def test_degenerate_inputs(cuda):
    zeros = [np.zeros(n, np.float32) for n in (5, 1025, 0)]
    for norm, sq in _both(zeros, cuda):
        assert (_bits(norm) == 0).all() and (_bits(sq) == 0).all()  # exactly +0.0
    # no gradients at all
    params = _parameters([None, None], cuda)
    norm, sq = splat_adam.gradient_norm(params, per_tensor=True)
    assert norm.shape == () and norm.device == cuda and norm.dtype == torch.float32 and norm.item() == 0.0
    assert sq.shape == (0,)
    assert splat_adam.gradient_norm([]).item() == 0.0 and splat_adam.gradient_norm([]).is_cuda
    opt = splat_adam.FusedAdam(params, lr=1e-3)
    before = [p.detach().clone() for p in params]
    opt.step(grad_norm=True)
    assert opt.grad_norm.device == cuda and opt.grad_norm.item() == 0.0 and opt.grad_sqnorms.shape == (0,)
    assert all(torch.equal(a, b) for a, b in zip(before, params)) and not opt.state


def test_non_finite_inputs(cuda):
    rng = np.random.default_rng(5)
    # one NaN element: its tensor's squared norm and the norm are NaN, the other tensors' entries are not
    case = [GR.marked(300, rng), GR.marked(1025, rng), GR.marked(7, rng)]
    case[1][1024] = np.nan
    _, want_sq = GR.gradient_norm(case)
    for norm, sq in _both(case, cuda):
        assert math.isnan(norm.item()) and math.isnan(sq[1].item())
        assert GR.ulps_off(sq[0].item(), want_sq[0]) <= 1 and GR.ulps_off(sq[2].item(), want_sq[2]) <= 1
    # 1000 x 1e20: the squared norm is beyond float32 (inf), the norm is not
    case = [GR.marked(300, rng), np.full(1000, 1e20, np.float32)]
    want_norm, want_sq = GR.gradient_norm(case)
    assert math.isfinite(np.float32(want_norm)) and want_sq[1] > float(np.finfo(np.float32).max)
    for norm, sq in _both(case, cuda):
        assert math.isfinite(norm.item()) and GR.ulps_off(norm.item(), want_norm) <= 1
        assert sq[1].item() == math.inf and GR.ulps_off(sq[0].item(), want_sq[0]) <= 1
    ref = torch.full((1000,), 1e20, device=cuda).norm(2).pow(2)  # the reference's float32 form overflows
    assert torch.isinf(ref)


def test_bitwise_repeatable(cuda):
    case = GR.table_case(33)
    a, fa = _both(case, cuda)
    b, fb = _both(case, cuda)
    for x, y in ((a, b), (fa, fb), (a, fb)):
        assert (_bits(x[0]) == _bits(y[0])).all() and (_bits(x[1]) == _bits(y[1])).all()


def _adam_run(cls, device, flag):
    """Three steps over the two-configuration case's groups, an lr change before the last; ``flag``: what
    step() is given (None: nothing)."""
    case = GR.two_config_case() + [np.zeros(0, np.float32), None]
    g = torch.Generator().manual_seed(3)
    params = _parameters(case, device, seed=2)
    groups = _two_config_groups(params) + [dict(params=params[4:])]
    opt = cls(groups, lr=3e-3)
    norms = []
    for it in range(3):
        if it == 2:
            for grp in opt.param_groups:
                grp["lr"] *= 0.5
        for p, entry in zip(params, case):
            if entry is not None:
                p.grad = (torch.from_numpy(entry) + 0.01 * torch.randn(entry.size, generator=g)).to(device)
        if flag is None:
            opt.step()
        else:
            opt.step(grad_norm=flag)
            norms.append((opt.grad_norm, opt.grad_sqnorms, splat_adam.gradient_norm(params, per_tensor=True)))
    return params, opt, norms


def test_update_is_bitwise_torch_adam_with_and_without_the_norm(cuda):
    from test_adam import _same_optimizer_state
    pa, oa, _ = _adam_run(torch.optim.Adam, cuda, None)
    pb, ob, norms = _adam_run(splat_adam.FusedAdam, cuda, True)
    _same_optimizer_state(oa, ob, pa, pb, "step(grad_norm=True)")
    assert len(norms) == 3
    for norm, sq, (want_norm, want_sq) in norms:  # each step's norm is that of the gradients it consumed
        assert (_bits(norm) == _bits(want_norm)).all() and (_bits(sq) == _bits(want_sq)).all()
        assert sq.shape == (5,) and norm.item() > 0
    pc, oc, _ = _adam_run(splat_adam.FusedAdam, cuda, None)  # step() without the flag: as it was
    _same_optimizer_state(oa, oc, pa, pc, "step()")
    assert oc.grad_norm is None and oc.grad_sqnorms is None
    pd, od, _ = _adam_run(splat_adam.FusedAdam, cuda, False)
    _same_optimizer_state(oa, od, pa, pd, "step(grad_norm=False)")
    assert od.grad_norm is None


# ---- C ABI ------------------------------------------------------------------------------------------------
POISON = 1234.5


@functools.lru_cache(maxsize=None)
def _abi_case():
    return tuple(GR.table_case(17))


def _abi_buffers(L, numels, dev):
    """(workspace, squared norms, norm), each with 8 poisoned values directly behind what the call may use."""
    nbytes = L.gsr_grad_norm_workspace_bytes(len(numels), (ctypes.c_longlong * len(numels))(*numels))
    assert nbytes == 8 * (1 + len(numels) + sum((m + GR.BLOCK - 1) // GR.BLOCK for m in numels))
    ws = torch.full((nbytes // 8 + 8,), POISON, dtype=torch.float64, device=dev)
    sq = torch.full((len(numels) + 8,), POISON, dtype=torch.float32, device=dev)
    return ws, sq, torch.full((1 + 8,), POISON, dtype=torch.float32, device=dev), nbytes // 8


@pytest.mark.parametrize("entry", ["gsr_grad_norm", "gsr_adam_step_norm"])
def test_c_abi_null_squared_norms_and_nothing_written_behind(cuda, entry):
    L = _C.feature_library("gradnorm")
    grads = [torch.from_numpy(g).to(cuda) for g in _abi_case() if g is not None]
    numels = [g.numel() for g in grads]
    want_norm, want_sq = GR.gradient_norm([g for g in _abi_case() if g is not None])
    state = [[torch.randn(n, device=cuda), torch.zeros(n, device=cuda), torch.zeros(n, device=cuda)] for n in numels]

    def call(want_sqnorms):
        ws, sq, norm, used = _abi_buffers(L, numels, cuda)
        sq_ptr = sq.data_ptr() if want_sqnorms else None
        with _C._device_guard(cuda):
            if entry == "gsr_grad_norm":
                arr = (splat_adam._GradTensor * len(grads))(*[splat_adam._GradTensor(g.data_ptr() if n else None, n)
                                                               for g, n in zip(grads, numels)])
                _C._check(L.gsr_grad_norm(len(grads), ctypes.addressof(arr), ws.data_ptr(), sq_ptr, norm.data_ptr(),
                                          _C._stream_ptr(cuda)))
            else:
                arr = (splat_adam._AdamTensor * len(grads))(*[
                    splat_adam._AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-3, 1.0)
                    for g, n, (p, m, v) in zip(grads, numels, state)])
                _C._check(L.gsr_adam_step_norm(len(grads), ctypes.addressof(arr), 0.9, 0.999, 1e-8, ws.data_ptr(), None,
                                               len(grads), 1, sq_ptr, norm.data_ptr(), _C._stream_ptr(cuda)))
        torch.cuda.synchronize()
        assert (ws[used:] == POISON).all() and (norm[1:] == POISON).all()
        assert (sq[len(numels):] == POISON).all()
        assert not (ws[:used] == POISON).any()  # every slot of the workspace is used
        return ws, sq, norm

    ws, sq, norm = call(True)
    assert GR.ulps_off(norm[0].item(), want_norm) <= 1
    assert all(GR.ulps_off(g, w) <= 1 for g, w in zip(sq[:len(numels)].tolist(), want_sq))
    assert ws[0].item() == pytest.approx(want_norm ** 2, rel=1e-12)  # the double total
    ws2, sq2, norm2 = call(False)  # out_sqnorms = NULL: the norm alone, nothing else touched
    assert (sq2 == POISON).all() and (_bits(norm2[:1]) == _bits(norm[:1])).all()
    assert torch.equal(ws2[:1 + len(numels)], ws[:1 + len(numels)])


def test_c_abi_nothing_to_do_writes_a_zero(cuda):
    L = _C.feature_library("gradnorm")
    ws = torch.full((4,), POISON, dtype=torch.float64, device=cuda)
    norm = torch.full((3,), POISON, dtype=torch.float32, device=cuda)
    with _C._device_guard(cuda):
        _C._check(L.gsr_grad_norm(0, None, ws.data_ptr(), None, norm.data_ptr(), _C._stream_ptr(cuda)))
        torch.cuda.synchronize()
        assert norm.tolist() == [0.0, POISON, POISON] and (ws == POISON).all()
        norm[0] = POISON
        _C._check(L.gsr_adam_step_norm(0, None, 0.9, 0.999, 1e-8, ws.data_ptr(), None, 0, 0, None, norm.data_ptr(),
                                       _C._stream_ptr(cuda)))  # not the last call of its chain: nothing at all
        torch.cuda.synchronize()
        assert (norm == POISON).all()
        _C._check(L.gsr_adam_step_norm(0, None, 0.9, 0.999, 1e-8, ws.data_ptr(), None, 0, 1, None, norm.data_ptr(),
                                       _C._stream_ptr(cuda)))
        torch.cuda.synchronize()
        assert norm.tolist() == [0.0, POISON, POISON] and (ws == POISON).all()


# ---- no host synchronisation ----------------------------------------------------------------------------
def test_no_host_synchronisation(cuda):
    import splat_train
    case = GR.table_case(17)
    params = _parameters(case, cuda)
    opt = splat_adam.FusedAdam(params, lr=1e-3)
    want_norm, _ = GR.gradient_norm(case)
    losses = tuple(torch.tensor(v, device=cuda) for v in (7.25, 0.3337, 1.4142, 0.0625))
    probe = torch.ones(1, device=cuda)
    log = splat_train.ScoreLog(depth=4)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    raises = False
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            probe.item()
        except RuntimeError:
            raises = True
        if raises:
            alone = splat_adam.gradient_norm(params)
            log.put(1, splat_train.step_metrics(losses, alone))
            opt.step(grad_norm=True)
            log.put(2, splat_train.step_metrics(losses, opt.grad_norm))
    finally:
        torch.cuda.set_sync_debug_mode(before)
    if not raises:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise for .item() in this torch build")
    done = log.close()
    assert [step for step, _ in done] == [1, 2]
    for _, values in done:
        assert values.shape == (6,) and not values.is_cuda
        got = dict(zip(splat_train.STEP_METRIC_NAMES, values.tolist()))
        assert got["train-loss/total"] == 7.25 and got["train-loss/rigidity"] == 0.0625
        assert got["train-loss/l1"] == np.float32(0.3337) and got["train-loss/ssim"] == np.float32(1.4142)
        assert got["train-loss/image"] == np.float32(0.8) * np.float32(0.3337) + np.float32(0.2) * np.float32(1.4142)
        assert GR.ulps_off(got["gradient-norm"], want_norm) <= 1
