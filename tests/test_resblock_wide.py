"""The fused residual blocks at hidden dimensions 129 to 512 (csrc/gsr_resblock.hip, the k_res_*_wide kernels):
128-column blocks of the output, k panels of 128, dW in kernels of its own.

Same checkers and bands as tests/test_resblock.py, whose helpers are imported: "project band" |got - ref| <=
1e-4 |ref| + 1e-6 max|ref|; "yardstick rule": per tensor the larger of the project band and twice the float32
torch block's own worst error against float64 on the same device and inputs.

Grid constants the shapes are derived from (csrc/gsr_internal.h, gsr_resblock.hip): 64-row tiles; without a
bound the forward and the R = G W kernels run 256 / CB workgroups along the rows, CB = ceil(H / 128) column
blocks, and the dW kernels 256 / CB^2 row groups.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch
from torch import nn

import deform_ref as DR
import splat_deform as D
from deform_ref import band, yardstick
from diff_gaussian_rasterization import _C
from test_deform import _clouds, _to
from test_resblock import PARAMS, _block, _case, _check_all, _fused, _reference, _torch_lines

ROWS, PANEL, AUTO_WORKGROUPS = 64, 128, 256


def _column_blocks(H):
    return -(-H // PANEL)


def _auto_row_workgroups(H):
    """Workgroups along the rows of the forward / R = G W kernels when the caller sets no bound."""
    return AUTO_WORKGROUPS // _column_blocks(H)


# the smallest P at H = 160 at which a workgroup of the automatic grid takes a second tile, plus a full tile:
# 128 workgroups x 64 rows, then one whole tile and one row of the next (the dW kernels' 64 row groups are on
# their third trip there)
SECOND_TRIP_H = 160
SECOND_TRIP_P = _auto_row_workgroups(SECOND_TRIP_H) * ROWS + 65


def _align256(n):
    return (n + 255) // 256 * 256


# ---- CPU ------------------------------------------------------------------------------------------
def test_workspace_sizes():
    L = _C.feature_library("resblock")
    size = L.gsr_resblock_workspace_bytes
    for H in (129, 256, 512):
        assert size(1031, H, 0, 0) > 0 and size(1031, H, 0, 1) > 0, H
    assert size(1031, 513, 0, 0) == 0 and size(1031, 513, 0, 1) == 0
    for H in (64, 128):  # the narrow kernels' layout is what it was
        for P in (1031, 1_000_000):
            tiles = -(-P // ROWS)
            nb, no = min(tiles, 256 * (2 if H <= 64 else 1)), min(tiles, 1024)
            fwd = _align256(8 * 3 * H * max(nb, no))
            bwd = fwd + _align256(4 * nb * H * H) + _align256(16 * H) + 2 * _align256(4 * P * H)
            assert size(P, H, 0, 0) == fwd and size(P, H, 0, 1) == bwd, (P, H)
    P = 1_000_000
    for H in (129, 160, 192, 256, 257, 384, 385, 511, 512):
        extra = size(P, H, 0, 1) - 2 * _align256(4 * P * H)
        print(f"H = {H}: backward workspace beyond the two transient gradients {extra / 2 ** 20:.1f} MB")
        assert 0 < extra <= 64 * 2 ** 20, (H, extra)


def test_width_switch():
    assert D.set_fused_residual_block_width(128) == 128  # the default
    try:
        assert D.set_fused_residual_block_width(512) == 128
        assert D.set_fused_residual_block_width(256) == 512
        for bad in (127, 513):
            with pytest.raises(ValueError, match="outside"):
                D.set_fused_residual_block_width(bad)
        assert D.set_fused_residual_block_width(512) == 256  # a refused value changes nothing
        assert "set_fused_residual_block_width" in D.__all__
        H = 160
        state, x, _ = _case(37, H)
        a, b = _block(D.ResidualBlock, H, state, "cpu"), _block(D.ResidualBlock, H, state, "cpu")
        assert torch.equal(a(x), _torch_lines(b, x))  # CPU tensors: the torch lines, whatever the width
        for k, v in a.state_dict().items():
            assert torch.equal(v, b.state_dict()[k]), k
    finally:
        D.set_fused_residual_block_width(128)


def _restated(state, x, k_limit=None, stat_rows=None):
    """The block's forward written out in float64: fc1 over k < ``k_limit`` only, both BatchNorms' batch
    statistics over the first ``stat_rows`` rows only (None: all)."""
    x = x.double()
    w1, w2 = state["fc1.weight"].double(), state["fc2.weight"].double()

    def bn(y, name):
        s = y[:stat_rows]
        xh = (y - s.mean(0)) / torch.sqrt(s.var(0, unbiased=False) + 1e-5)
        return xh * state[f"{name}.weight"].double() + state[f"{name}.bias"].double()

    y1 = x[:, :k_limit] @ w1[:, :k_limit].T
    a1 = nn.functional.gelu(bn(y1, "bn1"))
    return nn.functional.gelu(bn(a1 @ w2.T, "bn2") + x)


def _tolerances_moved(got, ref):
    """The largest |got - ref| in units of the project band."""
    return float(((got - ref).abs() / (1e-4 * ref.abs() + 1e-6 * ref.abs().max())).max())


def test_seam_restatements():
    """What the sizes of the GPU cases are there to catch, shown on the float64 block without a GPU."""
    P, H = 65, 129
    state, x, _ = _case(P, H)
    ref = _block(DR.ResidualBlock, H, state, "cpu", torch.float64)(x.double()).detach()
    assert _tolerances_moved(_restated(state, x), ref) < 1e-3  # the restatement is the block
    moved = _tolerances_moved(_restated(state, x, k_limit=PANEL), ref)
    print(f"(a) fc1 without its k >= {PANEL} terms at ({P}, {H}): {moved:.3g} tolerances")
    assert moved > 100
    P = SECOND_TRIP_P
    state, x, _ = _case(P, H)
    ref = _restated(state, x)
    first_trip = _auto_row_workgroups(SECOND_TRIP_H) * ROWS
    moved = _tolerances_moved(_restated(state, x, stat_rows=first_trip), ref)
    print(f"(b) statistics without rows >= {first_trip} at ({P}, {H}): {moved:.3g} tolerances")
    assert moved > 100


# ---- GPU ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("max_blocks", [0, 2])
@pytest.mark.parametrize("P,H", [(2, 129), (63, 160), (65, 256), (257, 384), (257, 512), (1031, 192), (1031, 511)])
def test_functional_against_float64(cuda, P, H, max_blocks):
    r32, r64 = _reference(cuda, P, H)
    got = _fused(cuda, P, H, max_blocks=max_blocks)
    assert got[0].shape == (P, H) and got[0].dtype == torch.float32
    _check_all(f"({P}, {H}, max_blocks={max_blocks})", got, r32, r64)


@pytest.mark.gpu
def test_second_trip_of_the_automatic_grid(cuda):
    P, H = SECOND_TRIP_P, SECOND_TRIP_H
    assert P == 8257 and -(-P // ROWS) == _auto_row_workgroups(H) + 2
    r32, r64 = _reference(cuda, P, H)
    _check_all(f"({P}, {H})", _fused(cuda, P, H), r32, r64)


@pytest.mark.gpu
def test_running_statistics(cuda):
    P, H = 257, 256
    for calls in (1, 2):
        want = _reference(cuda, P, H, momentum=0.3, calls=calls)[1][2]
        block = _fused(cuda, P, H, momentum=0.3, calls=calls)[2]
        for bn, ref in ((block.bn1, want.bn1), (block.bn2, want.bn2)):
            assert int(bn.num_batches_tracked) == calls == int(ref.num_batches_tracked)
            band(f"running_mean after {calls}", bn.running_mean, ref.running_mean)
            band(f"running_var after {calls}", bn.running_var, ref.running_var)


@pytest.mark.gpu
def test_stable_variance(cuda):
    """x = 0.05 N(0, 1) + 30, as tests/test_resblock.py::test_stable_variance."""
    P, H = 1031, 160
    r32, r64 = _reference(cuda, P, H, offset=True, momentum=1.0)
    got = _fused(cuda, P, H, offset=True, momentum=1.0)
    band("bn1.running_mean", got[2].bn1.running_mean, r64[2].bn1.running_mean)
    band("bn1.running_var", got[2].bn1.running_var, r64[2].bn1.running_var)
    _check_all(f"offset ({P}, {H})", got, r32, r64)


@pytest.mark.gpu
@pytest.mark.parametrize("max_blocks", [0, 2])
@pytest.mark.parametrize("P,H", [(1031, 192), (257, 512)])
def test_bitwise_repeatable(cuda, P, H, max_blocks):
    a, b = _fused(cuda, P, H, max_blocks=max_blocks), _fused(cuda, P, H, max_blocks=max_blocks)
    assert torch.equal(a[0], b[0])
    for name in ("x",) + PARAMS:
        assert torch.equal(a[1][name], b[1][name]), name


@pytest.mark.gpu
@pytest.mark.parametrize("needs", [PARAMS, ("fc2.weight",)])
def test_gradient_subsets(cuda, needs):
    P, H = 257, 256
    full = _fused(cuda, P, H)
    part = _fused(cuda, P, H, needs=needs)
    assert torch.equal(part[0], full[0])
    for name in ("x",) + PARAMS:
        if name in needs:
            assert torch.equal(part[1][name], full[1][name]), name
        else:
            assert part[1][name] is None, name


def _abi_forward(cuda, x, state, max_blocks=0):
    """gsr_resblock_forward on ``x`` and the weights and affine vectors of ``state``: (y1, y2, out, stats)."""
    L = _C.feature_library("resblock")
    P, H = x.shape
    dev = lambda name: state[name].to(cuda).contiguous()  # noqa: E731
    w1, g1, b1, w2, g2, b2 = (dev(n) for n in PARAMS)
    y1, y2, out = (torch.empty(P, H, device=cuda) for _ in range(3))
    stats = torch.empty(4 * H, device=cuda)
    ws = torch.empty(L.gsr_resblock_workspace_bytes(P, H, max_blocks, 0), dtype=torch.uint8, device=cuda)
    _C._check(L.gsr_resblock_forward(P, H, x.data_ptr(), w1.data_ptr(), g1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                                     g2.data_ptr(), b2.data_ptr(), 1e-5, 1e-5, 0.1, 0.1, None, None, None, None,
                                     ws.data_ptr(), max_blocks, y1.data_ptr(), y2.data_ptr(), out.data_ptr(),
                                     stats.data_ptr(), _C._stream_ptr(cuda)))
    torch.cuda.synchronize()
    return y1, y2, out, stats


@pytest.mark.gpu
def test_null_dx_writes_nothing_of_that_size(cuda):
    """Through the C ABI: with dL_dx NULL a poisoned (P, H) buffer that directly follows the workspace the call is
    given keeps every bit, x is unchanged, and the six other gradients are those of the all-outputs call."""
    P, H = 257, 256
    L = _C.feature_library("resblock")
    state, x, up = _case(P, H)
    x, up = x.to(cuda), up.to(cuda)
    dev = lambda name: state[name].to(cuda).contiguous()  # noqa: E731
    w1, g1, b1, w2, g2, b2 = (dev(n) for n in PARAMS)
    y1, y2, _, stats = _abi_forward(cuda, x, state)
    size = L.gsr_resblock_workspace_bytes(P, H, 0, 1)
    assert size % 256 == 0
    ws = torch.empty(size + 4 * P * H, dtype=torch.uint8, device=cuda)
    sentinel = ws[size:].view(torch.int32)  # what a write past the workspace's end would hit first

    def backward(with_dx):
        dx = torch.empty(P, H, device=cuda) if with_dx else None
        grads = [torch.empty_like(t) for t in (w1, g1, b1, w2, g2, b2)]
        _C._check(L.gsr_resblock_backward(P, H, x.data_ptr(), y1.data_ptr(), y2.data_ptr(), stats.data_ptr(),
                                          w1.data_ptr(), g1.data_ptr(), b1.data_ptr(), w2.data_ptr(), g2.data_ptr(),
                                          b2.data_ptr(), up.data_ptr(), ws.data_ptr(), 0,
                                          dx.data_ptr() if with_dx else None, *(t.data_ptr() for t in grads),
                                          _C._stream_ptr(cuda)))
        torch.cuda.synchronize()
        return dx, grads

    full = backward(True)
    sentinel.fill_(0x7FC12345)
    before, x_before = sentinel.clone(), x.clone()
    part = backward(False)
    assert torch.equal(sentinel, before) and torch.equal(x, x_before)
    for name, a, b in zip(PARAMS, part[1], full[1]):
        assert torch.equal(a, b), name
    fused = _fused(cuda, P, H)
    assert torch.equal(full[0], fused[1]["x"])


@pytest.mark.gpu
def test_k_ordered_chain_across_panel_seams(cuda):
    """H = 160 holding an H = 96 block and zeros elsewhere: the wide kernels' y1 is the narrow kernels' bit for
    bit, so the panels accumulate into one chain over ascending k."""
    P, wide, narrow = 257, 160, 96
    state, x, _ = _case(P, narrow)
    padded = {}
    for name in PARAMS:
        v = state[name]
        padded[name] = torch.zeros((wide,) * v.dim())
        padded[name][tuple(slice(0, narrow) for _ in range(v.dim()))] = v
    xw = torch.zeros(P, wide)
    xw[:, :narrow] = x
    want = _abi_forward(cuda, x.to(cuda), state)
    got = _abi_forward(cuda, xw.to(cuda), padded)
    assert torch.equal(got[0][:, :narrow], want[0])
    assert not got[0][:, narrow:].any()
    band("y2", got[1][:, :narrow], want[1])
    band("out", got[2][:, :narrow], want[2])
    for q, name in enumerate(("mean1", "invstd1", "mean2", "invstd2")):
        band(name, got[3][q * wide:q * wide + narrow], want[3][q * narrow:(q + 1) * narrow])


def _fmaf(a, b, c):
    """float32 a * b + c rounded once (ties to even), from exact rationals."""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    near = np.float32(float(exact))  # within one float32 step of the answer; a double rounding may be one off
    cands = [np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf))]
    dist = [abs(Fraction(float(v)) - exact) for v in cands]
    best = [v for v, d in zip(cands, dist) if d == min(dist)]
    return best[0] if len(best) == 1 else next(v for v in best if not v.view(np.uint32) & 1)


def _chain(x_row, w_row, order):
    acc = np.float32(0)
    for k in order:
        acc = _fmaf(x_row[k], w_row[k], acc)
    return acc


@pytest.mark.gpu
def test_k_ordered_chain_with_both_panels_filled(cuda):
    """H = 160 with N(0, 1) data in every k: elements of y1 are, bit for bit, the float32 fmaf chain over
    k = 0, 1, ..., 159 computed on the host from exact rationals.  The same chain with the second panel's terms
    first gives other bits for these elements, so a panel taken out of order would show."""
    P, H = 65, 160
    state, x, _ = _case(P, H)
    y1 = _abi_forward(cuda, x.to(cuda), state)[0].cpu().numpy()
    xs, w = x.numpy(), state["fc1.weight"].numpy()
    ascending, swapped = list(range(H)), list(range(PANEL, H)) + list(range(PANEL))
    moved = 0
    for row, col in ((0, 0), (0, 159), (31, 127), (32, 128), (63, 131), (64, 5), (64, 159)):
        want = _chain(xs[row], w[col], ascending)
        assert y1[row, col].view(np.uint32) == want.view(np.uint32), (row, col, y1[row, col], want)
        moved += int(_chain(xs[row], w[col], swapped).view(np.uint32) != want.view(np.uint32))
    print(f"panels swapped: {moved} of 7 elements change bits")
    assert moved > 0


@pytest.mark.gpu
def test_routing(cuda):
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
        assert run(192) == (0, True)  # the default width
        previous = D.set_fused_residual_block_width(512)
        try:
            assert previous == 128
            assert run(192)[0] == 1
            assert run(512)[0] == 1
            assert run(192, fused=False) == (0, True)
            assert run(512, fused=False) == (0, True)
            assert run(192, train=False) == (0, True)
        finally:
            assert D.set_fused_residual_block_width(previous) == 512
        assert run(192) == (0, True)
    finally:
        _C.profile_enable(False)
        _C.profile_select(None)
        _C.profile_reset()


def _graph_nodes(fn):
    seen, todo, names = set(), [fn], []
    while todo:
        node = todo.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        names.append(type(node).__name__)
        todo.extend(n for n, _ in node.next_functions)
    return names


@pytest.mark.gpu
def test_whole_network(cuda):
    P, H, blocks = 257, 192, 2
    initial, previous = (_to(c, cuda) for c in _clouds(P))
    torch.manual_seed(11)
    net = D.DeformationNetwork(H, blocks).to(cuda).train()
    state = {k: v.clone() for k, v in net.state_dict().items()}
    up = torch.randn(P, 7, generator=torch.Generator().manual_seed(12)).to(cuda)

    def torch_only(dtype):
        ref = DR.TorchDeformationNetwork(H, blocks).to(cuda).to(dtype).train()
        ref.load_state_dict(state)
        return DR.network_output_and_grads(ref, initial, previous, 3 / 7, up, dtype)

    width = D.set_fused_residual_block_width(512)
    try:
        out = net(initial, previous, 3, 7)
    finally:
        D.set_fused_residual_block_width(width)
    nodes = _graph_nodes(out.grad_fn)
    print("autograd nodes:", sorted(set(nodes)))
    assert nodes.count("_ResBlockBackward") == blocks
    (out * up).sum().backward()
    o32, _, g32 = torch_only(torch.float32)
    o64, _, g64 = torch_only(torch.float64)
    yardstick("network out", out, o32, o64)
    assert {n for n, _ in net.named_parameters()} == set(g64)
    for n, p in net.named_parameters():
        yardstick(f"network grad {n}", p.grad, g32[n], g64[n])
