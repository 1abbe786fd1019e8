"""Fused L1 + SSIM loss: oracle pinned to the reference, HIP kernels vs oracle.

CPU: the float64 oracle (oracle/ssim_oracle.py) reproduces the reference's own calc_ssim values and
autograd gradients (tests/golden, produced by importing external.py) and torch.autograd of a
float64 restatement.  GPU (-m gpu): splat_loss through the C ABI of libgsr.so against the oracle on
the golden inputs, ragged / tiny / batched shapes and a 1080p render-sized pair.  Tolerances: the
scalar means within 1e-5 relative (fp32 separable blur + double block sums vs float64), gradients
within 1e-4 relative + 1e-6 of the largest magnitude.

Those bands are known to hold on noise, where the window variances are large.  On the image families
training sees (identical, constant, smooth, binary targets) sigma = <x^2> - mu^2 cancels in fp32, in the
reference's own calc_ssim as in the kernels, so test_gpu_loss_image_families gives each bound a floor of
twice a yardstick: what a float32 torch restatement of calc_ssim (external.py:68-110) misses the float64
oracle by on the same pair, measured in the test on the CPU (the rule of tests/test_train_step.py).
test_gpu_loss_strip_edges puts a strip's input row count on 21 / 22 / 23 (the row loop is unrolled 2 x 11)
and the halo columns on the image edge (W = 64, 128).
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import ssim_oracle as SO

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_harness.npz"))


def _grad_close(got, ref, rtol=1e-4, atol_frac=1e-6):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    tol = rtol * np.abs(ref) + atol_frac * np.abs(ref).max()
    bad = np.abs(got - ref) > tol
    assert not bad.any(), f"{bad.sum()} of {bad.size} gradient values off, worst {np.abs(got - ref).max():.3e}"


def test_oracle_window_matches_reference_definition():
    w = SO.window_1d()
    assert w.dtype == np.float32 and w.shape == (11,)
    assert abs(float(w.sum()) - 1.0) < 1e-6 and np.all(w == w[::-1])


def test_oracle_matches_reference_ssim_value_and_grad():
    a, b = GOLD["ssim_in_img1"], GOLD["ssim_in_img2"]
    _, ssim, st = SO.l1_ssim(a, b)
    assert abs(ssim - float(GOLD["ssim_out"])) < 2e-6
    _grad_close(SO.l1_ssim_grad(st, 0.0, 1.0), GOLD["ssim_out_grad"], rtol=2e-4, atol_frac=2e-5)


def test_oracle_matches_reference_combined_loss():
    """0.8 l1 + 0.2 (1 - ssim) of densify.py:149-151 on a ragged binary-target pair."""
    a, b = GOLD["loss_in_img1"], GOLD["loss_in_img2"]
    l1, ssim, st = SO.l1_ssim(a, b)
    assert abs(l1 - float(GOLD["loss_out_l1"])) < 2e-6
    assert abs(ssim - float(GOLD["loss_out_ssim"])) < 2e-6
    _grad_close(SO.l1_ssim_grad(st, 0.8, -0.2), GOLD["loss_out_grad"], rtol=2e-4, atol_frac=2e-5)


def test_oracle_grad_matches_torch_autograd_float64():
    g = torch.Generator().manual_seed(3)
    a = torch.rand(2, 3, 19, 23, generator=g, dtype=torch.float64)
    b = torch.rand(2, 3, 19, 23, generator=g, dtype=torch.float64)
    x = a.clone().requires_grad_(True)
    w = torch.from_numpy(SO.window_1d().astype(np.float64))
    w2 = torch.outer(w, w)[None, None].expand(6, 1, 11, 11)

    def blur(t):
        return torch.nn.functional.conv2d(t.reshape(1, 6, 19, 23), w2, padding=5, groups=6).reshape(t.shape)

    mu1, mu2 = blur(x), blur(b)
    s = ((2 * mu1 * mu2 + SO.C1) * (2 * (blur(x * b) - mu1 * mu2) + SO.C2)) / (
        (mu1 ** 2 + mu2 ** 2 + SO.C1) * ((blur(x * x) - mu1 ** 2) + (blur(b * b) - mu2 ** 2) + SO.C2))
    loss = 0.3 * (x - b).abs().mean() + 0.7 * s.mean()
    loss.backward()
    l1, ssim, st = SO.l1_ssim(a.numpy(), b.numpy())
    assert abs(0.3 * l1 + 0.7 * ssim - loss.detach().item()) < 1e-12
    np.testing.assert_allclose(SO.l1_ssim_grad(st, 0.3, 0.7), x.grad.numpy(), rtol=1e-9, atol=1e-14)


# ------------------------------------------------------------------------------------------------
def _gpu_case(cuda, a, b, g_l1=0.8, g_ssim=-0.2):
    import splat_loss
    x = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(cuda).requires_grad_(True)
    y = torch.from_numpy(np.ascontiguousarray(b, np.float32)).to(cuda)
    l1, ssim = splat_loss.l1_and_ssim(x, y)
    (g_l1 * l1 + g_ssim * ssim).backward()
    torch.cuda.synchronize()
    rl1, rssim, st = SO.l1_ssim(a.astype(np.float32), b.astype(np.float32))
    assert abs(float(l1) - rl1) <= 1e-5 * abs(rl1) + 1e-7, (float(l1), rl1)
    assert abs(float(ssim) - rssim) <= 1e-5 * abs(rssim) + 1e-7, (float(ssim), rssim)
    ref = SO.l1_ssim_grad(st, g_l1, g_ssim)
    # |x - y| == 0 exactly is where sign() is 0 in both; elsewhere the sign terms agree bitwise
    _grad_close(x.grad.cpu().numpy(), ref)


@pytest.mark.gpu
def test_gpu_loss_matches_reference_goldens(cuda):
    import splat_loss
    x = torch.from_numpy(GOLD["ssim_in_img1"]).to(cuda).requires_grad_(True)
    y = torch.from_numpy(GOLD["ssim_in_img2"]).to(cuda)
    s = splat_loss.calc_ssim(x, y)
    s.backward()
    assert abs(s.detach().item() - float(GOLD["ssim_out"])) < 2e-6
    _grad_close(x.grad.cpu().numpy(), GOLD["ssim_out_grad"], rtol=2e-4, atol_frac=2e-5)
    x = torch.from_numpy(GOLD["loss_in_img1"]).to(cuda).requires_grad_(True)
    y = torch.from_numpy(GOLD["loss_in_img2"]).to(cuda)
    loss = splat_loss.image_loss(x, y)
    loss.backward()
    ref = 0.8 * float(GOLD["loss_out_l1"]) + 0.2 * (1 - float(GOLD["loss_out_ssim"]))
    assert abs(loss.detach().item() - ref) < 2e-6
    _grad_close(x.grad.cpu().numpy(), GOLD["loss_out_grad"], rtol=2e-4, atol_frac=2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 1, 1), (3, 5, 7), (1, 33, 65), (3, 64, 32), (3, 37, 130),
                                   (2, 3, 40, 70), (3, 100, 200)])
def test_gpu_loss_parity_shapes(cuda, shape):
    rng = np.random.default_rng(sum(shape))
    a = rng.random(shape, dtype=np.float32)
    b = np.clip(a + 0.2 * rng.standard_normal(shape).astype(np.float32), 0, 1)
    _gpu_case(cuda, a, b)


@pytest.mark.gpu
def test_gpu_loss_parity_1080p(cuda):
    rng = np.random.default_rng(7)
    a = rng.random((3, 1080, 1920), dtype=np.float32)
    b = (rng.random((3, 1080, 1920)) > 0.5).astype(np.float32)
    _gpu_case(cuda, a, b, 1.0, 1.0)


@pytest.mark.gpu
def test_gpu_loss_single_output_grads(cuda):
    """Only one of the two outputs used: the other upstream gradient is absent (NULL in the ABI)."""
    import splat_loss
    rng = np.random.default_rng(11)
    a, b = rng.random((3, 30, 40), dtype=np.float32), rng.random((3, 30, 40), dtype=np.float32)
    _, _, st = SO.l1_ssim(a, b)
    for which, (gl, gs) in (("ssim", (0.0, 1.0)), ("l1", (1.0, 0.0))):
        x = torch.from_numpy(a).to(cuda).requires_grad_(True)
        l1, ssim = splat_loss.l1_and_ssim(x, torch.from_numpy(b).to(cuda))
        (ssim if which == "ssim" else l1).backward()
        _grad_close(x.grad.cpu().numpy(), SO.l1_ssim_grad(st, gl, gs))


@pytest.mark.gpu
def test_gpu_loss_errors(cuda):
    import splat_loss
    x = torch.rand(3, 8, 8, device=cuda)
    with pytest.raises(NotImplementedError):
        splat_loss.l1_and_ssim(x, x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="shapes differ"):
        splat_loss.l1_and_ssim(x, torch.rand(3, 8, 9, device=cuda))
    with pytest.raises(NotImplementedError):
        splat_loss.calc_ssim(x, x, window_size=7)


def test_loss_refuses_cpu_tensors():
    import splat_loss
    with pytest.raises(RuntimeError, match="no CPU path"):
        splat_loss.l1_and_ssim(torch.rand(3, 8, 8), torch.rand(3, 8, 8))


# ---- strip edges ----------------------------------------------------------------------------------
STRIP_EDGES = [(1, 11, 64), (1, 12, 64), (1, 13, 69), (3, 44, 59), (3, 45, 128)]
STRIP_ROWS, UNROLL = 32, 22  # kSsRH output rows per strip; input rows per trip of the unrolled row loop


def _noise_pair(shape):
    rng = np.random.default_rng(sum(shape))
    a = rng.random(shape, dtype=np.float32)
    return a, np.clip(a + 0.2 * rng.standard_normal(shape).astype(np.float32), 0, 1)


def _second_trip_rows(H):
    """Output rows whose last input row is read in a later trip of the row loop (input row >= 22 of the strip)."""
    rows = np.arange(H)
    return (rows % STRIP_ROWS) + 10 >= UNROLL


@pytest.mark.parametrize("shape", STRIP_EDGES)
def test_strip_edge_shapes_and_row_trip_sensitivity(shape):
    """The shapes put a strip's input row count (output rows + 10) on 21, 22 and 23, 42 and 22, 42 and 23; leaving
    out the rows a second trip of the row loop produces moves the SSIM mean by more than 100 tolerances wherever
    there is such a row, and (11, 64) / (12, 64) have none: they end exactly at the trip's edge."""
    _, H, W = shape
    nin = [min(STRIP_ROWS, H - y0) + 10 for y0 in range(0, H, STRIP_ROWS)]
    assert nin == {11: [21], 12: [22], 13: [23], 44: [42, 22], 45: [42, 23]}[H]
    a, b = _noise_pair(shape)
    _, ssim, st = SO.l1_ssim(a, b)
    late = _second_trip_rows(H)
    assert late.any() == (H > 12)
    if late.any():
        moved = abs(st["S"][:, ~late, :].sum() / st["S"].size - ssim) / (1e-5 * abs(ssim))
        print(f"{shape}: second-trip rows left out move the SSIM mean by {moved:.0f} tolerances")
        assert moved > 100
        # and the gradient: the derivative maps' late rows never written (zero)
        keep = np.where(late[None, :, None], 0.0, 1.0)
        cut = dict(st, A=st["A"] * keep, S=st["S"] * keep, B=np.where(keep > 0, st["B"], st["A"] * keep),
                   D=np.where(keep > 0, st["D"], st["C"]))
        ref, wrong = SO.l1_ssim_grad(st, 0.8, -0.2), SO.l1_ssim_grad(cut, 0.8, -0.2)
        tol = 1e-4 * np.abs(ref) + 1e-6 * np.abs(ref).max()
        assert (np.abs(wrong - ref) / tol).max() > 100


@pytest.mark.gpu
@pytest.mark.parametrize("shape", STRIP_EDGES)
def test_gpu_loss_strip_edges(cuda, shape):
    _gpu_case(cuda, *_noise_pair(shape))


# ---- image families -------------------------------------------------------------------------------
FAMILY_SHAPE = (3, 45, 70)


def _smooth(phase, shape=FAMILY_SHAPE):
    c, y, x = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    return (0.5 + 0.3 * np.sin(2 * np.pi * (x / 61.0 + 0.11 * c) + phase) * np.cos(2 * np.pi * y / 47.0 + 0.5 * phase)
            + 0.1 * np.sin(2 * np.pi * (x + 2 * y) / 97.0)).astype(np.float32)


def _family(name):
    rng = np.random.default_rng(17)
    if name == "identical":
        a = _smooth(0.0)
        return a, a.copy()
    if name == "equal_constants":
        return np.full(FAMILY_SHAPE, 0.6, np.float32), np.full(FAMILY_SHAPE, 0.6, np.float32)
    if name == "different_constants":
        return np.full(FAMILY_SHAPE, 0.6, np.float32), np.full(FAMILY_SHAPE, 0.35, np.float32)
    if name == "smooth_pair":
        return _smooth(0.0), _smooth(0.05)
    if name == "smooth_vs_binary_mask":
        yy, xx = np.mgrid[:FAMILY_SHAPE[1], :FAMILY_SHAPE[2]]
        disc = ((yy - 20) ** 2 + (xx - 30) ** 2 < 15 ** 2).astype(np.float32)
        return _smooth(0.0), np.repeat(disc[None], 3, 0)
    if name == "outside_unit_range":
        return (3 * rng.random(FAMILY_SHAPE, dtype=np.float32) - 1), (3 * rng.random(FAMILY_SHAPE, dtype=np.float32) - 1)
    raise KeyError(name)


FAMILIES = ("identical", "equal_constants", "different_constants", "smooth_pair", "smooth_vs_binary_mask",
            "outside_unit_range")


def _torch_restatement(a, b, dtype, g_l1=0.8, g_ssim=-0.2):
    """calc_ssim (external.py:68-110: grouped conv2d with the 11 x 11 window, sigma = <x^2> - mu^2) and
    l1_loss in ``dtype`` on the CPU: (l1, ssim, d(g_l1 l1 + g_ssim ssim) / d img1)."""
    x = torch.from_numpy(a).to(dtype).requires_grad_(True)
    y = torch.from_numpy(b).to(dtype)
    C = a.shape[0]
    w1 = torch.from_numpy(SO.window_1d()).to(dtype)[:, None]  # create_window: the 1-D window's outer product
    w2 = w1.mm(w1.t())[None, None].expand(C, 1, 11, 11).contiguous()

    def blur(t):
        return torch.nn.functional.conv2d(t[None], w2, padding=5, groups=C)[0]

    mu1, mu2 = blur(x), blur(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq, sigma2_sq, sigma12 = blur(x * x) - mu1_sq, blur(y * y) - mu2_sq, blur(x * y) - mu1_mu2
    s = ((2 * mu1_mu2 + SO.C1) * (2 * sigma12 + SO.C2)) / ((mu1_sq + mu2_sq + SO.C1) * (sigma1_sq + sigma2_sq + SO.C2))
    l1, ssim = (x - y).abs().mean(), s.mean()
    (g_l1 * l1 + g_ssim * ssim).backward()
    return float(l1.detach()), float(ssim.detach()), x.grad.numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _family_reference(name, g_l1=0.8, g_ssim=-0.2):
    """Per family, computed once: the pair, the float64 oracle's (l1, ssim, gradient) and the yardsticks -- what the
    float32 restatement misses them by."""
    a, b = _family(name)
    l1, ssim, st = SO.l1_ssim(a, b)
    grad = SO.l1_ssim_grad(st, g_l1, g_ssim)
    l32, s32, g32 = _torch_restatement(a, b, torch.float32, g_l1, g_ssim)
    yard = {"l1": abs(l32 - l1), "ssim": abs(s32 - ssim), "grad": float(np.abs(g32 - grad).max())}
    return a, b, l1, ssim, grad, yard


@pytest.mark.parametrize("name", FAMILIES)
def test_family_yardsticks(name):
    """The restatement in float64 is the oracle (so its float32 run measures float32 arithmetic, not a different
    formula); the yardsticks are printed, and stay far below the quantities they bound."""
    a, b, l1, ssim, grad, yard = _family_reference(name)
    l64, s64, g64 = _torch_restatement(a, b, torch.float64)
    assert abs(l64 - l1) <= 1e-14 and abs(s64 - ssim) <= 1e-12
    np.testing.assert_allclose(g64, grad, rtol=1e-7, atol=max(1e-9 * np.abs(grad).max(), 1e-15))
    scale = np.abs(grad).max()
    band = 1e-4 * np.abs(grad) + 1e-6 * scale
    l32, s32, g32 = _torch_restatement(a, b, torch.float32)
    outside = int((np.abs(g32 - grad) > band).sum())
    print(f"{name}: ssim {ssim:.9f} yardstick {yard['ssim']:.3e} ({yard['ssim'] / abs(ssim):.3e} relative), "
          f"gradient max|ref| {scale:.3e} yardstick {yard['grad']:.3e}, float32 restatement outside the band "
          f"{outside}/{grad.size}")
    assert yard["ssim"] <= 1e-3 * abs(ssim) and yard["l1"] <= 1e-6 * max(l1, 1e-30) + 1e-12
    if name in ("identical", "equal_constants"):
        assert ssim == pytest.approx(1.0, abs=1e-12) and l1 == 0 and scale < 1e-12  # the gradient is rounding alone
    else:
        assert yard["grad"] <= 1e-2 * scale


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_gpu_loss_image_families(cuda, name):
    """Scalars within max(1e-5 relative, 2 yardsticks), gradients within max(1e-4 |ref| + 1e-6 max|ref|,
    2 yardsticks) of the float64 oracle."""
    import splat_loss
    a, b, rl1, rssim, ref, yard = _family_reference(name)
    x = torch.from_numpy(a).to(cuda).requires_grad_(True)
    l1, ssim = splat_loss.l1_and_ssim(x, torch.from_numpy(b).to(cuda))
    (0.8 * l1 - 0.2 * ssim).backward()
    torch.cuda.synchronize()
    got = x.grad.cpu().numpy().astype(np.float64)
    l1, ssim = float(l1.detach()), float(ssim.detach())
    err = np.abs(got - ref)
    scale = np.abs(ref).max()
    band = 1e-4 * np.abs(ref) + 1e-6 * scale
    tol = np.maximum(band, 2 * yard["grad"])
    print(f"{name}: l1 error {abs(l1 - rl1):.3e} (yardstick {yard['l1']:.3e}), ssim error {abs(ssim - rssim):.3e} = "
          f"{abs(ssim - rssim) / abs(rssim):.3e} relative (yardstick {yard['ssim']:.3e}), gradient error "
          f"{err.max():.3e} (yardstick {yard['grad']:.3e}, max|ref| {scale:.3e}), outside the plain band "
          f"{int((err > band).sum())}/{err.size}, outside the tolerance {int((err > tol).sum())}/{err.size}")
    assert abs(l1 - rl1) <= max(1e-5 * abs(rl1), 2 * yard["l1"]), (l1, rl1)
    assert abs(ssim - rssim) <= max(1e-5 * abs(rssim), 2 * yard["ssim"]), (ssim, rssim)
    assert not (err > tol).any(), f"{int((err > tol).sum())} of {err.size} gradient values off, worst {err.max():.3e}"
