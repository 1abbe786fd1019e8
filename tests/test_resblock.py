"""The deformation network's fused residual blocks (splat_deform.residual_block, csrc/gsr_resblock.hip).

CPU: ``ResidualBlock`` off the fused path is the seven torch lines of train.py:57-77 bit for bit and keeps
the reference's state_dict; a library without the entry points is a "rebuild" error.  GPU: the kernels
against the float64 torch block (tests/deform_ref.py) with the same parameters.

Bands (those of tests/test_deform.py): "project band" |got - ref| <= 1e-4 |ref| + 1e-6 max|ref|; "golden
band" 2e-4 |ref| + 2e-5 max|ref| for values the reference saved in fp32; "yardstick rule": per tensor the
larger of the project band and twice the float32 torch block's own worst error against float64 on the same
device and inputs.
"""
import copy
import functools
import os

import numpy as np
import pytest
import torch
from torch import nn

import deform_ref as DR
import splat_deform as D
from deform_ref import band, yardstick
from diff_gaussian_rasterization import _C

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "reference_deform.npz"))
PARAMS = ("fc1.weight", "bn1.weight", "bn1.bias", "fc2.weight", "bn2.weight", "bn2.bias")


def _torch_lines(block, x):
    """train.py:57-77 written out."""
    identity = x
    x = block.fc1(x)
    x = block.bn1(x)
    x = nn.functional.gelu(x)
    x = block.fc2(x)
    x = block.bn2(x)
    x = x + identity
    return nn.functional.gelu(x)


@functools.lru_cache(maxsize=None)
def _case(P, H, offset=False, seed=0):
    """Seeded CPU tensors of one block: its state (nn.Linear-range weights, random affine parameters, fresh
    running statistics), the input (N(0, 1), or 0.05 N(0, 1) + 30 with ``offset``) and the upstream gradient."""
    g = torch.Generator().manual_seed(31 * P + H + 7919 * seed)
    bound = 1 / H ** 0.5
    state = {"fc1.weight": (torch.rand(H, H, generator=g) * 2 - 1) * bound,
             "bn1.weight": torch.rand(H, generator=g) + 0.5, "bn1.bias": torch.randn(H, generator=g) * 0.5,
             "bn1.running_mean": torch.zeros(H), "bn1.running_var": torch.ones(H),
             "bn1.num_batches_tracked": torch.tensor(0),
             "fc2.weight": (torch.rand(H, H, generator=g) * 2 - 1) * bound,
             "bn2.weight": torch.rand(H, generator=g) + 0.5, "bn2.bias": torch.randn(H, generator=g) * 0.5,
             "bn2.running_mean": torch.zeros(H), "bn2.running_var": torch.ones(H),
             "bn2.num_batches_tracked": torch.tensor(0)}
    x = torch.randn(P, H, generator=g)
    if offset:
        x = 0.05 * x + 30.0
    return state, x, torch.randn(P, H, generator=g)


def _block(cls, H, state, device, dtype=torch.float32, momentum=None):
    block = cls(H).to(device).to(dtype).train()
    block.load_state_dict(state)  # values are cast
    if momentum is not None:
        block.bn1.momentum = block.bn2.momentum = momentum
    return block


def _grads(block, x):
    return {"x": x.grad, **{n: p.grad for n, p in block.named_parameters()}}


@functools.lru_cache(maxsize=None)
def _reference(device, P, H, offset=False, momentum=None, calls=1):
    """(out, gradients, block after ``calls`` forwards) of the torch block in float32 and in float64."""
    state, x, up = _case(P, H, offset)
    res = []
    for dtype in (torch.float32, torch.float64):
        block = _block(DR.ResidualBlock, H, state, device, dtype, momentum)
        xd = x.to(device).to(dtype).requires_grad_(True)
        for _ in range(calls - 1):
            block(xd.detach())
        out = block(xd)
        out.backward(up.to(device).to(dtype))
        res.append((out.detach(), _grads(block, xd), block))
    return res


def _fused(device, P, H, offset=False, momentum=None, max_blocks=0, calls=1, needs=None):
    """The fused block on the same case: (out, gradients, block)."""
    state, x, up = _case(P, H, offset)
    block = _block(D.ResidualBlock, H, state, device, momentum=momentum)
    xd = x.to(device)
    if needs is not None:
        for n, p in block.named_parameters():
            p.requires_grad_(n in needs)
    xd.requires_grad_(needs is None or "x" in needs)
    for _ in range(calls - 1):
        with torch.no_grad():
            D.residual_block(xd, block.fc1.weight, block.bn1, block.fc2.weight, block.bn2, max_blocks=max_blocks)
    out = D.residual_block(xd, block.fc1.weight, block.bn1, block.fc2.weight, block.bn2, max_blocks=max_blocks)
    out.backward(up.to(device))
    return out.detach(), _grads(block, xd), block


def _check_all(tag, got, r32, r64):
    yardstick(f"{tag} out", got[0], r32[0], r64[0])
    for name in ("x",) + PARAMS:
        yardstick(f"{tag} grad {name}", got[1][name], r32[1][name], r64[1][name])


# ---- CPU ------------------------------------------------------------------------------------------
def test_torch_path_bit_for_bit():
    H = 24
    state, x, _ = _case(37, H)
    ref = _block(DR.ResidualBlock, H, state, "cpu")
    assert list(D.ResidualBlock(H).state_dict().keys()) == list(ref.state_dict().keys())
    for k, v in D.ResidualBlock(H).state_dict().items():
        assert v.shape == ref.state_dict()[k].shape, k

    def same(train):
        a, b = _block(D.ResidualBlock, H, state, "cpu"), _block(D.ResidualBlock, H, state, "cpu")
        a.train(train), b.train(train)
        got, want = a(x), _torch_lines(b, x)
        assert torch.equal(got, want)
        for k, v in a.state_dict().items():
            assert torch.equal(v, b.state_dict()[k]), k

    same(True)   # CPU tensors
    same(False)  # eval mode
    previous = D.set_fused_residual_blocks(False)
    try:
        assert previous is True and D.set_fused_residual_blocks(False) is False
        same(True)
    finally:
        D.set_fused_residual_blocks(previous)
    with pytest.raises(RuntimeError, match="no CPU path"):
        b = _block(D.ResidualBlock, H, state, "cpu")
        D.residual_block(x, b.fc1.weight, b.bn1, b.fc2.weight, b.bn2)


# ---- GPU ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("max_blocks", [0, 2])
@pytest.mark.parametrize("P,H", [(2, 64), (63, 64), (65, 32), (257, 128), (1031, 40), (1031, 7), (4099, 64)])
def test_functional_against_float64(cuda, P, H, max_blocks):
    r32, r64 = _reference(cuda, P, H)
    got = _fused(cuda, P, H, max_blocks=max_blocks)
    assert got[0].shape == (P, H) and got[0].dtype == torch.float32
    _check_all(f"({P}, {H}, max_blocks={max_blocks})", got, r32, r64)


@pytest.mark.gpu
@pytest.mark.parametrize("P,H", [(257, 128), (1031, 40)])
def test_running_statistics(cuda, P, H):
    for calls in (1, 2):
        want = _reference(cuda, P, H, calls=calls)[1][2]
        block = _fused(cuda, P, H, calls=calls)[2]
        for bn, ref in ((block.bn1, want.bn1), (block.bn2, want.bn2)):
            assert int(bn.num_batches_tracked) == calls == int(ref.num_batches_tracked)
            band(f"running_mean after {calls}", bn.running_mean, ref.running_mean)
            band(f"running_var after {calls}", bn.running_var, ref.running_var)


@pytest.mark.gpu
@pytest.mark.parametrize("P,H", [(4099, 64), (1031, 40)])
def test_stable_variance(cuda, P, H):
    """x = 0.05 N(0, 1) + 30: the columns of y1 have a mean far above their spread, where an fp32
    sum-of-squares variance is off by tens of percent and a shifted one is within 1e-5."""
    r32, r64 = _reference(cuda, P, H, offset=True, momentum=1.0)
    got = _fused(cuda, P, H, offset=True, momentum=1.0)
    band("bn1.running_mean", got[2].bn1.running_mean, r64[2].bn1.running_mean)
    band("bn1.running_var", got[2].bn1.running_var, r64[2].bn1.running_var)
    _check_all(f"offset ({P}, {H})", got, r32, r64)


@pytest.mark.gpu
def test_golden_network(cuda):
    t = lambda name: torch.from_numpy(GOLD[name]).to(cuda)  # noqa: E731
    H = GOLD["state/fc_in.weight"].shape[0]
    net = D.DeformationNetwork(H, 1)
    net.load_state_dict({str(n): torch.from_numpy(GOLD[f"state/{n}"]) for n in GOLD["state_names"]})
    net = net.to(cuda).train()
    initial = {"means": t("initial_means"), "rotation_quaternions": t("initial_rotation_quaternions")}
    previous = {"means": t("previous_means"), "rotation_quaternions": t("previous_rotation_quaternions")}
    timestep, count = (int(v) for v in GOLD["timestep"])
    out = net(initial, previous, timestep, count)
    (out * t("upstream")).sum().backward()
    band("golden output", out, GOLD["output"], 2e-4, 2e-5)
    names = [n for n, _ in net.named_parameters()]
    assert any(n.startswith("residual_blocks.0.") for n in names)
    for n, p in net.named_parameters():
        band(f"golden grad {n}", p.grad, GOLD[f"grad/{n}"], 2e-4, 2e-5)


@pytest.mark.gpu
def test_saved_set(cuda):
    P, H = 257, 128
    state, x, _ = _case(P, H)
    block = _block(D.ResidualBlock, H, state, cuda)
    x = x.to(cuda).requires_grad_(True)
    call = lambda: D.residual_block(x, block.fc1.weight, block.bn1, block.fc2.weight, block.bn2)  # noqa: E731
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        with torch.no_grad():
            quiet = call()
        assert saved == [] and quiet.grad_fn is None and not quiet.requires_grad
        loud = call()
        assert loud.grad_fn is not None
    parameters = {p.data_ptr() for p in block.parameters()}
    kept = [t for t in saved if t.data_ptr() not in parameters]
    assert sorted(t.numel() for t in kept) == [4 * H, P * H, P * H, P * H]  # stats, x, y1, y2
    assert any(t.data_ptr() == x.data_ptr() for t in kept)
    assert torch.equal(quiet, loud.detach())


@pytest.mark.gpu
@pytest.mark.parametrize("P,H", [(4099, 64), (1031, 40)])
def test_bitwise_repeatable(cuda, P, H):
    a, b = _fused(cuda, P, H, max_blocks=2), _fused(cuda, P, H, max_blocks=2)
    assert torch.equal(a[0], b[0])
    for name in ("x",) + PARAMS:
        assert torch.equal(a[1][name], b[1][name]), name


@pytest.mark.gpu
@pytest.mark.parametrize("needs", [PARAMS, ("fc2.weight",)])
def test_gradient_subsets(cuda, needs):
    P, H = 257, 64
    full = _fused(cuda, P, H)
    part = _fused(cuda, P, H, needs=needs)
    assert torch.equal(part[0], full[0])
    for name in ("x",) + PARAMS:
        if name in needs:
            assert torch.equal(part[1][name], full[1][name]), name
        else:
            assert part[1][name] is None, name


@pytest.mark.gpu
def test_fallback_routing(cuda):
    P = 65
    count = lambda: _C.profile_read("resblock_fwd")[1]  # noqa: E731

    def run(H, train=True, fused=True):
        """The rise of the resblock_fwd count over one forward, and whether the output is the torch lines'."""
        state, x, _ = _case(P, H)
        block, twin = (_block(D.ResidualBlock, H, state, cuda).train(train) for _ in range(2))
        x = x.to(cuda)
        before = count()
        previous = D.set_fused_residual_blocks(fused)
        try:
            got = block(x)
        finally:
            D.set_fused_residual_blocks(previous)
        return count() - before, torch.equal(got, _torch_lines(twin, x))

    _C.profile_enable(True)
    _C.profile_select(["resblock_fwd"])
    _C.profile_reset()
    try:
        assert run(64)[0] == 1
        assert run(129) == (0, True)
        assert run(64, train=False) == (0, True)
        assert run(64, fused=False) == (0, True)
    finally:
        _C.profile_enable(False)
        _C.profile_select(None)
        _C.profile_reset()


@pytest.mark.gpu
def test_two_blocks_chained(cuda):
    P, H = 1031, 64
    states = [_case(P, H, seed=s)[0] for s in (1, 2)]
    _, x, up = _case(P, H)

    def run(cls, dtype):
        net = nn.Sequential(*(_block(cls, H, s, cuda, dtype) for s in states))
        xd = x.to(cuda).to(dtype).requires_grad_(True)
        out = net(xd)
        out.backward(up.to(cuda).to(dtype))
        return out.detach(), {"x": xd.grad, **{n: p.grad for n, p in net.named_parameters()}}

    r64, r32, got = run(DR.ResidualBlock, torch.float64), run(DR.ResidualBlock, torch.float32), run(D.ResidualBlock, torch.float32)
    yardstick("chained out", got[0], r32[0], r64[0])
    assert set(got[1]) == set(r64[1]) and len(got[1]) == 13
    for name in got[1]:
        yardstick(f"chained grad {name}", got[1][name], r32[1][name], r64[1][name])
