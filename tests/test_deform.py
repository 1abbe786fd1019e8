"""The deformation network's input side (splat_deform, csrc/gsr_deform.hip).

CPU: the restatements of tests/deform_ref.py reproduce what the reference itself computed
(tests/golden/reference_deform.npz, written by tests/golden/gen_golden_deform.py); the module has the
reference's state_dict and refuses CPU tensors and bad shapes.  GPU: the HIP kernels against the float64
restatement.  "Project band": |got - ref| <= 1e-4 |ref| + 1e-6 max|ref| with no value outside (the band of
tests/test_rigidity.py); "golden band": 2e-4 |ref| + 2e-5 max|ref| for values the reference saved in fp32.

k_posenc_ranges runs at most 256 workgroups of 256 rows and strides over the rest, so rows >= 65,536 are a
second trip of its loop: the P = 65,836 cases put every column's minimum and maximum (and, once, a NaN) there.
"""
import functools
import os

import numpy as np
import pytest
import torch

import deform_ref as DR
import splat_deform as D
from deform_ref import band
from diff_gaussian_rasterization import _C

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "reference_deform.npz"))
PROGRESS = 3 / 7
ULP2 = 2.4e-7  # 2 ulp of 1.0: every feature lies in [-1, 1]


def _t(name):
    return torch.from_numpy(GOLD[name])


def _gold_clouds(device="cpu"):
    return ({"means": _t("initial_means").to(device), "rotation_quaternions": _t("initial_rotation_quaternions").to(device)},
            {"means": _t("previous_means").to(device), "rotation_quaternions": _t("previous_rotation_quaternions").to(device)})


def _gold_progress():
    timestep, count = GOLD["timestep"]
    return int(timestep) / int(count)


def _gold_state():
    return {str(n): _t(f"state/{n}") for n in GOLD["state_names"]}


@functools.lru_cache(maxsize=None)
def _clouds(P, constant_column=False):
    """Seeded (initial, previous) clouds on the CPU; ``constant_column``: the initial y and the previous
    quaternion x are the same in every row (their normalisation is 0 / 0)."""
    g = torch.Generator().manual_seed(1000 + P)
    initial = {"means": (torch.rand(P, 3, generator=g) - 0.5) * 3.0, "rotation_quaternions": torch.randn(P, 4, generator=g)}
    previous = {"means": initial["means"] + 0.05 * torch.randn(P, 3, generator=g),
                "rotation_quaternions": initial["rotation_quaternions"] + 0.1 * torch.randn(P, 4, generator=g)}
    if constant_column:
        initial["means"][:, 1] = 0.25
        previous["rotation_quaternions"][:, 1] = -0.5
    return initial, previous


def _to(cloud, device):
    return {k: v.to(device) for k, v in cloud.items()}


@functools.lru_cache(maxsize=None)
def _layer(P, H):
    """Seeded fc_in weights, bias and upstream gradient for a (P, H) case, on the CPU."""
    g = torch.Generator().manual_seed(7 * P + H)
    bound = 1 / 192 ** 0.5  # nn.Linear's initialisation range
    return ((torch.rand(H, 192, generator=g) * 2 - 1) * bound, (torch.rand(H, generator=g) * 2 - 1) * bound,
            torch.randn(P, H, generator=g))


# ---- CPU ------------------------------------------------------------------------------------------
def test_encoding_restatement_reproduces_reference():
    initial, previous = _gold_clouds()
    for cloud, key in ((initial, "encoded_initial"), (previous, "encoded_previous")):
        e32 = DR.encode_means_and_rotations(cloud["means"], cloud["rotation_quaternions"], torch.float32)
        assert e32.dtype == torch.float32 and np.array_equal(e32.numpy(), GOLD[key]), key
        e64 = DR.encode_means_and_rotations(cloud["means"], cloud["rotation_quaternions"], torch.float64)
        err = np.abs(e64.numpy() - GOLD[key].astype(np.float64)).max()
        print(f"{key}: float64 restatement vs reference {err:.3e}")
        assert e64.dtype == torch.float64 and err <= ULP2
    p32 = DR.encode_progress(_gold_progress(), 5, "cpu", torch.float32)
    assert np.array_equal(p32.numpy(), np.broadcast_to(GOLD["encoded_progress"], (5, 8)))
    p64 = DR.encode_progress(_gold_progress(), 1, "cpu", torch.float64)
    assert np.abs(p64.numpy()[0] - GOLD["encoded_progress"]).max() <= ULP2


def test_network_restatement_reproduces_reference():
    initial, previous = _gold_clouds()
    H = GOLD["state/fc_in.weight"].shape[0]
    net = DR.TorchDeformationNetwork(H, 1)
    net.load_state_dict(_gold_state())
    net.train()
    out, fc_in_out, grads = DR.network_output_and_grads(net, initial, previous, _gold_progress(), _t("upstream"),
                                                        torch.float32)
    band("fc_in_output", fc_in_out, GOLD["fc_in_output"], 2e-4, 2e-5)
    band("output", out, GOLD["output"], 2e-4, 2e-5)
    for name, g in grads.items():
        band(f"grad {name}", g, GOLD[f"grad/{name}"], 2e-4, 2e-5)


FEATURES = ("deform", "resblock", "head")


@pytest.mark.parametrize("feature", FEATURES)
def test_stale_library_is_a_rebuild_error(monkeypatch, feature):
    """A libgsr.so without one feature's entry points still loads and serves everything else; that feature
    raises on first use, naming the remedy."""
    real = _C.load_library()
    assert not _C._MISSING and _C.feature_library(feature) is real
    absent = list(_C._OPTIONAL[feature][1])

    class Stale:
        def __getattr__(self, name):
            if name in absent:
                raise AttributeError(f"undefined symbol: {name}")
            return getattr(real, name)

    monkeypatch.setattr(_C, "_lib", None)
    monkeypatch.setattr(_C, "_MISSING", {})
    monkeypatch.setattr(_C, "_PREALLOC_FN", _C._PREALLOC_FN)
    monkeypatch.setattr(_C.ctypes, "CDLL", lambda path: Stale())
    stale = _C.load_library()
    assert isinstance(stale, Stale) and list(_C._MISSING) == [feature] and absent[0] in _C._MISSING[feature]
    assert all(_C.feature_library(other) is stale for other in FEATURES if other != feature)
    with pytest.raises(RuntimeError, match="rebuild"):
        _C.feature_library(feature)


def test_module_contract():
    net = D.DeformationNetwork(32, 1)
    state = net.state_dict()
    assert list(state.keys()) == [str(n) for n in GOLD["state_names"]]
    for name, shape in zip(GOLD["state_names"], GOLD["state_shapes"]):
        want = tuple(int(d) for d in str(shape).split(",") if d)
        assert tuple(state[str(name)].shape) == want, name
    net.load_state_dict(_gold_state())  # a reference checkpoint loads
    initial, previous = _gold_clouds()
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.encode_means_and_rotations(initial)
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.deform_input_layer(net.fc_in.weight, net.fc_in.bias, initial, previous, PROGRESS)
    with pytest.raises(RuntimeError, match="no CPU path"):
        net(initial, previous, 3, 7)
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.update_gaussian_cloud_parameters(net, initial, previous, 3, 7)
    with pytest.raises(ValueError):
        D.DeformationNetwork(513, 1)
    with pytest.raises(ValueError):
        D.deform_input_layer(torch.zeros(0, 192), torch.zeros(0), initial, previous, PROGRESS)
    with pytest.raises(ValueError):
        D.deform_input_layer(torch.zeros(513, 192), torch.zeros(513), initial, previous, PROGRESS)
    with pytest.raises(ValueError):
        D.deform_input_layer(torch.zeros(32, 191), torch.zeros(32), initial, previous, PROGRESS)
    with pytest.raises(ValueError):
        D.deform_input_layer(torch.zeros(32, 192), torch.zeros(31), initial, previous, PROGRESS)
    with pytest.raises(ValueError):
        D.deform_input_layer(torch.zeros(32, 192, dtype=torch.float64), torch.zeros(32), initial, previous, PROGRESS)
    with pytest.raises(ValueError):
        D.deform_input_layer(torch.zeros(32, 192), torch.zeros(32), initial, {"means": previous["means"][:5],
                             "rotation_quaternions": previous["rotation_quaternions"][:5]}, PROGRESS)
    with pytest.raises(ValueError):
        D.encode_means_and_rotations({"means": torch.zeros(4, 4), "rotation_quaternions": torch.zeros(4, 4)})
    with pytest.raises(ValueError):
        D.encode_means_and_rotations({"means": torch.zeros(4, 3, dtype=torch.float64),
                                      "rotation_quaternions": torch.zeros(4, 4)})


# ---- GPU: the encoding ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P,constant", [(1, False), (63, False), (63, True), (257, False), (4099, False)])
def test_encode_means_and_rotations(cuda, P, constant):
    """Against the float64 restatement; the yardstick is the float32 torch restatement's own worst error
    on this device on the same inputs, the kernel may have max(2 x that, 2.4e-7)."""
    cloud = _to(_clouds(P, constant)[0], cuda)
    got = D.encode_means_and_rotations(cloud)
    assert got.shape == (P, 92) and got.dtype == torch.float32
    r32 = DR.encode_means_and_rotations(cloud["means"], cloud["rotation_quaternions"], torch.float32)
    r64 = DR.encode_means_and_rotations(cloud["means"], cloud["rotation_quaternions"], torch.float64)
    nan = torch.isnan(r64)
    assert torch.equal(torch.isnan(got), nan) and torch.equal(torch.isnan(r32), nan)
    if P == 1:
        assert bool(nan.all())  # every column is constant: 0 / 0
        return
    assert bool(nan.any()) == constant
    if constant:  # exactly the sine and cosine slots of the constant column (mean y: column 1 of 3)
        cols = torch.zeros(92, dtype=torch.bool)
        cols[[j * 3 + 1 for j in range(20)]] = True
        assert torch.equal(nan.cpu(), cols.expand(P, 92))
    ok = ~nan
    yard = float((r32.double() - r64)[ok].abs().max())
    err = float((got.double() - r64)[ok].abs().max())
    print(f"P={P} constant={constant}: kernel {err:.3e}, float32 torch restatement {yard:.3e}")
    assert err <= max(2 * yard, ULP2)


# ---- the range kernel's second trip (P > 65,536) ----------------------------------------------------
RANGE_TRIP = 256 * 256  # GSR_POSENC_RANGE_BLOCKS workgroups x 256 rows
P_LATE = RANGE_TRIP + 300


@functools.lru_cache(maxsize=None)
def _late_clouds():
    """The seeded clouds at P_LATE rows with every column's minimum and maximum moved into rows >= 65,536
    (a different row for each of the 28 extremes)."""
    clouds = tuple({k: v.clone() for k, v in c.items()} for c in _clouds(P_LATE))
    row = RANGE_TRIP + 3
    for cloud in clouds:
        for t in cloud.values():
            for c in range(t.shape[1]):
                lo, hi = float(t[:, c].min()), float(t[:, c].max())
                t[row, c], t[row + 1, c] = lo - 0.37, hi + 0.61
                row += 7
    assert row < P_LATE
    return clouds


def _numpy_ranges(means, quats, rows=None):
    """lo = min, hi = fp32(max - lo) per column, numpy fp32; ``rows``: the mistake restated, later rows ignored."""
    x = np.concatenate((means.numpy(), quats.numpy()), axis=1)[:rows]
    lo = x.min(axis=0)
    return np.concatenate((lo, (x.max(axis=0) - lo).astype(np.float32)))


def _sample_rows():
    return torch.cat((torch.arange(0, 128), torch.arange(RANGE_TRIP - 128, P_LATE)))


def test_late_extremes_and_range_sensitivity():
    """Every extreme sits past the first trip; ranges from the first 65,536 rows alone differ in every one of the 14
    values' bits, and the encoding they give moves by more than 100 of the GPU test's tolerances."""
    for cloud in _late_clouds():
        means, quats = cloud["means"], cloud["rotation_quaternions"]
        x = torch.cat((means, quats), dim=1)
        assert int(x.argmin(dim=0).min()) >= RANGE_TRIP and int(x.argmax(dim=0).min()) >= RANGE_TRIP
        right, wrong = _numpy_ranges(means, quats), _numpy_ranges(means, quats, RANGE_TRIP)
        assert (right.view(np.int32) != wrong.view(np.int32)).all()
        rows = _sample_rows()
        r32 = DR.encode_means_and_rotations(means, quats, torch.float32)[rows]
        r64 = DR.encode_means_and_rotations(means, quats, torch.float64)[rows]
        lo, hi = torch.from_numpy(wrong[:7]), torch.from_numpy(wrong[7:])
        xn = (2.0 * (x - lo) / hi) - 1.0
        moved = torch.cat((DR.encode_arguments(DR.arguments(xn[:, :3], 10)), DR.encode_arguments(DR.arguments(xn[:, 3:], 4))),
                          dim=1)[rows]
        tol = max(2 * float((r32.double() - r64).abs().max()), ULP2)
        ratio = float((moved.double() - r64).abs().max()) / tol
        print(f"ranges of the first trip only: the encoding moves by {ratio:.0f} tolerances")
        assert ratio > 100


@pytest.mark.gpu
def test_encoding_ranges_second_trip(cuda):
    for cloud in _late_clouds():
        means, quats = cloud["means"], cloud["rotation_quaternions"]
        got = D.encoding_ranges(means.to(cuda), quats.to(cuda)).cpu().numpy()
        np.testing.assert_array_equal(got.view(np.int32), _numpy_ranges(means, quats).view(np.int32))


@pytest.mark.gpu
def test_encoding_ranges_keep_a_late_nan(cuda):
    """A NaN in row 65,736 of the quaternion y column: its minimum and its range are NaN, as torch's reductions
    (and numpy's) give; the other 12 values are untouched."""
    cloud = {k: v.clone() for k, v in _late_clouds()[0].items()}
    cloud["rotation_quaternions"][RANGE_TRIP + 200, 2] = float("nan")
    means, quats = cloud["means"], cloud["rotation_quaternions"]
    got = D.encoding_ranges(means.to(cuda), quats.to(cuda)).cpu().numpy()
    ref = _numpy_ranges(means, quats)
    col = 3 + 2
    assert np.isnan(ref[[col, 7 + col]]).all() and np.isnan(ref).sum() == 2
    assert torch.isnan(torch.cat((means, quats), dim=1).min(dim=0).values[col])
    assert np.isnan(got[[col, 7 + col]]).all()
    keep = ~np.isnan(ref)
    np.testing.assert_array_equal(got[keep].view(np.int32), ref[keep].view(np.int32))


@pytest.mark.gpu
def test_encode_second_trip(cuda):
    """test_encode_means_and_rotations' check on rows from both sides of row 65,536."""
    cloud = _to(_late_clouds()[0], cuda)
    got = D.encode_means_and_rotations(cloud)
    assert got.shape == (P_LATE, 92)
    rows = _sample_rows().to(cuda)
    r32 = DR.encode_means_and_rotations(cloud["means"], cloud["rotation_quaternions"], torch.float32)[rows]
    r64 = DR.encode_means_and_rotations(cloud["means"], cloud["rotation_quaternions"], torch.float64)[rows]
    assert not torch.isnan(r64).any() and torch.isfinite(got).all()
    yard = float((r32.double() - r64).abs().max())
    err = float((got[rows].double() - r64).abs().max())
    print(f"P={P_LATE}: kernel {err:.3e}, float32 torch restatement {yard:.3e}")
    assert err <= max(2 * yard, ULP2)


@pytest.mark.gpu
def test_fused_layer_second_trip(cuda):
    """deform_input_layer at H = 7 over P = 65,836 rows, with test_fused_forward's and test_fused_backward's checks."""
    P, H = P_LATE, 7
    initial, previous = (_to(c, cuda) for c in _late_clouds())
    w, b, up = (t.to(cuda) for t in _layer(P, H))
    x64 = DR.input_matrix(initial, previous, PROGRESS, torch.float64)
    w, b = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out = D.deform_input_layer(w, b, initial, previous, PROGRESS)
    assert out.shape == (P, H) and out.dtype == torch.float32
    band(f"fc_in output ({P}, {H})", out, x64 @ w.detach().double().t() + b.detach().double())
    out.backward(up)
    band(f"dW ({P}, {H})", w.grad, up.double().t() @ x64)
    band(f"db ({P}, {H})", b.grad, up.double().sum(0))
    pe64 = DR.encode_progress(PROGRESS, 1, cuda, torch.float64)[0]
    band("dW[:, 184:] = enc(progress) db", w.grad[:, 184:], b.grad.double()[:, None] * pe64[None, :])


# ---- GPU: the fused input layer -------------------------------------------------------------------
def _layer_case(cuda, P, H):
    initial, previous = (_to(c, cuda) for c in _clouds(P))
    w, b, up = (t.to(cuda) for t in _layer(P, H))
    x64 = DR.input_matrix(initial, previous, PROGRESS, torch.float64)
    return initial, previous, w, b, up, x64


@pytest.mark.gpu
@pytest.mark.parametrize("P,H", [(63, 64), (257, 128), (1031, 40), (4099, 64)])
def test_fused_forward(cuda, P, H):
    initial, previous, w, b, _, x64 = _layer_case(cuda, P, H)
    got = D.deform_input_layer(w, b, initial, previous, PROGRESS)
    assert got.shape == (P, H) and got.dtype == torch.float32
    band(f"fc_in output ({P}, {H})", got, x64 @ w.double().t() + b.double())


@pytest.mark.gpu
@pytest.mark.parametrize("max_blocks", [0, 2])
@pytest.mark.parametrize("P,H", [(63, 64), (257, 128), (1031, 40)])
def test_fused_backward(cuda, P, H, max_blocks):
    initial, previous, w, b, up, x64 = _layer_case(cuda, P, H)
    initial = {k: v.clone().requires_grad_(True) for k, v in initial.items()}
    previous = {k: v.clone().requires_grad_(True) for k, v in previous.items()}
    w, b = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out = D.deform_input_layer(w, b, initial, previous, PROGRESS, max_blocks=max_blocks)
    out.backward(up)
    band(f"dW ({P}, {H}, max_blocks={max_blocks})", w.grad, up.double().t() @ x64)
    band(f"db ({P}, {H}, max_blocks={max_blocks})", b.grad, up.double().sum(0))
    pe64 = DR.encode_progress(PROGRESS, 1, cuda, torch.float64)[0]
    band("dW[:, 184:] = enc(progress) db", w.grad[:, 184:], b.grad.double()[:, None] * pe64[None, :])
    for cloud in (initial, previous):
        assert all(v.grad is None for v in cloud.values())  # the encoded parameters are detached


@pytest.mark.gpu
def test_golden_fc_in(cuda):
    initial, previous = _gold_clouds(cuda)
    w = _t("state/fc_in.weight").to(cuda).requires_grad_(True)
    b = _t("state/fc_in.bias").to(cuda).requires_grad_(True)
    out = D.deform_input_layer(w, b, initial, previous, _gold_progress())
    band("golden fc_in output", out, GOLD["fc_in_output"], 2e-4, 2e-5)
    out.backward(_t("grad_fc_in_output").to(cuda))  # the gradient that reached fc_in's output in the reference
    band("golden grad fc_in.weight", w.grad, GOLD["grad/fc_in.weight"], 2e-4, 2e-5)
    band("golden grad fc_in.bias", b.grad, GOLD["grad/fc_in.bias"], 2e-4, 2e-5)


# ---- GPU: the whole network -----------------------------------------------------------------------
@pytest.mark.gpu
def test_whole_network(cuda):
    """P = 1031, H = 64, 2 blocks, train mode, against the float64 torch-only network with the same
    state_dict.  Per tensor the yardstick is the float32 torch-only network's worst error against float64
    on this device; the fused network may have twice that or the project band, whichever is larger."""
    P, H, blocks = 1031, 64, 2
    initial, previous = (_to(c, cuda) for c in _clouds(P))
    torch.manual_seed(5)
    fused = D.DeformationNetwork(H, blocks).to(cuda).train()
    state = {k: v.clone() for k, v in fused.state_dict().items()}
    up = torch.randn(P, 7, generator=torch.Generator().manual_seed(6)).to(cuda)
    base = torch.cat((initial["means"], initial["rotation_quaternions"]), dim=1)

    def torch_only(dtype):
        net = DR.TorchDeformationNetwork(H, blocks).to(cuda).to(dtype).train()
        net.load_state_dict(state)  # names and shapes match; values are cast
        out = net(DR.input_matrix(initial, previous, PROGRESS, dtype), base.to(dtype))
        y = base.to(dtype) + 0.01 * out  # train.py:295-307
        (y * up.to(dtype)).sum().backward()
        return net, y.detach(), {n: p.grad for n, p in net.named_parameters()}

    net64, y64, g64 = torch_only(torch.float64)
    _, y32, g32 = torch_only(torch.float32)

    extra = {"colors": torch.rand(P, 3, device=cuda), "segmentation_masks": torch.rand(P, 3, device=cuda)}
    deltas = []
    hook = fused.register_forward_hook(lambda m, i, o: deltas.append(o.detach()))
    updated = D.update_gaussian_cloud_parameters(fused, {**initial, **extra}, previous, 3, 7)
    hook.remove()
    assert set(updated) == {"means", "rotation_quaternions", "colors", "segmentation_masks"}
    assert updated["colors"] is extra["colors"] and updated["segmentation_masks"] is extra["segmentation_masks"]
    y = torch.cat((updated["means"], updated["rotation_quaternions"]), dim=1)
    (y * up).sum().backward()
    assert len(deltas) == 1 and torch.equal(y.detach(), base + deltas[0] * 0.01)

    def check(name, got, r32, r64):
        yard = float((r32.double() - r64).abs().max())
        band(name, got, r64, floor=2 * yard)

    check("updated means and quaternions", y, y32, y64)
    for name, p in fused.named_parameters():
        check(f"grad {name}", p.grad, g32[name], g64[name])

    # the state_dict round-trips into the torch-only network and back
    net32 = DR.TorchDeformationNetwork(H, blocks)
    net32.load_state_dict(fused.state_dict())
    back = D.DeformationNetwork(H, blocks)
    back.load_state_dict(net32.state_dict())
    for k, v in fused.state_dict().items():
        assert torch.equal(back.state_dict()[k], v.cpu()), k
    assert net64.fc_in.weight.dtype == torch.float64


# ---- GPU: repeatability, no_grad ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P,H", [(4099, 64), (1031, 40)])
def test_bitwise_repeatable(cuda, P, H):
    initial, previous, w, b, up, _ = _layer_case(cuda, P, H)

    def run():
        wp, bp = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        out = D.deform_input_layer(wp, bp, initial, previous, PROGRESS, max_blocks=2)
        out.backward(up)
        return out.detach(), wp.grad, bp.grad

    for a, c in zip(run(), run()):
        assert torch.equal(a, c)


@pytest.mark.gpu
def test_no_grad_saves_nothing(cuda):
    P, H = 257, 128
    initial, previous, w, b, _, _ = _layer_case(cuda, P, H)
    w, b = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        with torch.no_grad():
            quiet = D.deform_input_layer(w, b, initial, previous, PROGRESS)
        assert saved == [] and quiet.grad_fn is None and not quiet.requires_grad
        loud = D.deform_input_layer(w, b, initial, previous, PROGRESS)
        assert len(saved) == 6 and loud.grad_fn is not None
    assert sum(t.numel() for t in saved) == 2 * (7 * P + 14)  # the 14-float inputs and the ranges, nothing else
    assert torch.equal(quiet, loud.detach())
