"""Forward-only scores of a timestep's views (gsr_image_scores, splat_loss.image_scores): the host side.

No GPU here: the workspace size, the C ABI's argument checks, the Python entry point's refusals, ScoreLog's
ring on host tensors, and -- the rule README states for size-driven cases -- for each size-driven case of
tests/test_scores_gpu.py a float64 restatement of the mistake it exists to catch, which must move the compared
quantity by more than 100 of the tolerances the GPU test applies:

* (920, 190) x 3 planes has 3 x 29 x 3 = 261 partial sums per view, 5 more than the 256 threads of the per-view
  sum take in their first pass: a sum that stops there loses strips;
* 33 views are one more than the 32 pointer pairs of a launch: a call that stops there loses the last view;
* (33, 65) ends in a strip of 1 row and a strip of 1 column: a kernel that takes them for full sums SSIM values
  of pixels outside the image, or divides by the strips' pixel count.

The cases, their seeded images and their float64 references (oracle/ssim_oracle.py, a restatement of
external.py:49-110, plus the squared error) are defined here and shared with the GPU tests.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from oracle import ssim_oracle as SO

STRIP_W, STRIP_H, SUM_THREADS, LAUNCH_VIEWS = 64, 32, 256, 32  # csrc/gsr_loss.hip: strips, k_scores_sum, kSsEvalViews
REL, ABS = 1e-5, 1e-7                  # tests/test_loss.py _gpu_case: |got - ref| <= REL |ref| + ABS, for l1 and ssim
PSNR_ABS = 10.0 / math.log(10.0) * REL  # d psnr = -10 / ln 10 * d mse / mse
ULP32 = 2.0 ** -23

# (views, planes per view, H, W)
BASE = [(V, 3, H, W) for V in (1, 2, 5) for H, W in ((21, 64), (22, 64), (23, 128))]
PARTIAL = [(2, 3, 33, 65), (2, 3, 1, 1), (2, 1, 33, 65)]
SECOND_TRIP = (2, 3, 920, 190)
CHUNK = (33, 3, 21, 64)
CASES = BASE + PARTIAL + [SECOND_TRIP, CHUNK]


def partials_per_view(C, H, W):
    return C * -(-W // STRIP_W) * -(-H // STRIP_H)


def case_images(case):
    """The case's seeded pairs, (V, C, H, W) float32 each: noise renders against noisier targets, the noise level
    rising with the view so that no two views score alike; where there are at least three views, view 1 is an
    identical pair and view 2 a pair of two constants."""
    V, C, H, W = case
    rng = np.random.default_rng(1000 * V + 100 * C + H + W)
    a = rng.random((V, C, H, W), dtype=np.float32)
    level = (0.1 + 0.01 * np.arange(V, dtype=np.float32))[:, None, None, None]
    b = np.clip(a + level * rng.standard_normal((V, C, H, W)).astype(np.float32), 0, 1).astype(np.float32)
    if V >= 3:
        b[1] = a[1]
        a[2], b[2] = 0.6, 0.35
    return a, b


def reference_view(a, b):
    """float64 (l1, ssim, mse, psnr, image_loss) of one pair, and the oracle's state."""
    l1, ssim, st = SO.l1_ssim(a, b)
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    mse = float((d * d).mean())
    psnr = math.inf if mse == 0 else -10.0 * math.log10(mse)
    return (l1, ssim, mse, psnr, 0.8 * l1 + 0.2 * (1.0 - ssim)), st


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """Computed once per case and shared: the images, a (V, 5) float64 array of the references, and the mean."""
    a, b = case_images(case)
    rows = np.array([reference_view(a[v], b[v])[0] for v in range(case[0])])
    return a, b, rows, float(rows[:, 4].mean())


def tolerances(ref):
    """Per quantity (l1, ssim, mse): REL |ref| + ABS."""
    return REL * np.abs(ref) + ABS


# ---- the workspace and the C ABI's checks ---------------------------------------------------------
def _lib():
    from diff_gaussian_rasterization import _C
    return _C.feature_library("scores")


@pytest.mark.parametrize("case", CASES)
def test_workspace_bytes(case):
    L = _lib()
    V, C, H, W = case
    per_view = 12 * partials_per_view(C, H, W)  # (sum |x-y|, sum S, sum (x-y)^2) per wave strip, no header
    assert L.gsr_image_scores_workspace_bytes(V, C, H, W) == V * per_view
    sizes = [L.gsr_image_scores_workspace_bytes(v, C, H, W) for v in range(0, 70)]
    assert sizes[0] == 0 and all(y - x == per_view for x, y in zip(sizes, sizes[1:]))


def test_second_trip_and_chunk_cases_follow_the_shipped_constants():
    V, C, H, W = SECOND_TRIP
    assert SUM_THREADS < partials_per_view(C, H, W) == 261 and V == 2
    assert all(partials_per_view(*c[1:]) <= SUM_THREADS for c in CASES if c != SECOND_TRIP)
    assert CHUNK[0] == LAUNCH_VIEWS + 1


def test_argument_errors():
    L = _lib()
    fake = ctypes.c_void_p(256)  # never dereferenced: every call below returns before a launch
    one = (ctypes.c_void_p * 1)(256)
    for args in ((-1, 3, 4, 4), (1, -3, 4, 4), (1, 3, -4, 4), (1, 3, 4, -4)):
        assert L.gsr_image_scores_workspace_bytes(*args) == 0
        assert L.gsr_image_scores(*args, one, one, fake, fake, None, None) == 1
        assert b"image_scores: negative size" in L.gsr_last_error()
    for p1, p2 in ((None, one), (one, None), (None, None)):
        assert L.gsr_image_scores(1, 3, 4, 4, p1, p2, fake, fake, None, None) == 1
        assert b"image_scores: null image array" in L.gsr_last_error()
    hole = (ctypes.c_void_p * 2)(256, None)
    two = (ctypes.c_void_p * 2)(256, 512)
    assert L.gsr_image_scores(2, 3, 4, 4, two, hole, fake, fake, None, None) == 1
    assert b"image_scores: null image (view 1)" in L.gsr_last_error()
    for ws, out in ((None, fake), (fake, None)):
        assert L.gsr_image_scores(1, 3, 4, 4, one, one, ws, out, None, None) == 1
        assert b"image_scores: null workspace / output" in L.gsr_last_error()
    assert L.gsr_image_scores(1, 3, 0, 4, one, one, fake, fake, None, None) == 1
    assert b"empty image" in L.gsr_last_error()
    assert L.gsr_image_scores(1, 3, 1 << 15, 1 << 15, one, one, fake, fake, None, None) != 0
    assert b"too large" in L.gsr_last_error()
    # no views: valid, nothing to launch, and without a mean to write nothing at all
    assert L.gsr_image_scores(0, 3, 4, 4, None, None, None, None, None, None) == 0


def test_symbols_are_an_optional_group():
    from diff_gaussian_rasterization import _C
    assert {"gsr_image_scores", "gsr_image_scores_workspace_bytes"} <= set(_C.EXPORTED_SYMBOLS)
    assert list(_C._OPTIONAL_EXPORT["scores"][1]) == ["gsr_image_scores_workspace_bytes", "gsr_image_scores"]


# ---- the Python entry point's refusals --------------------------------------------------------------
def test_image_scores_refusals():
    import splat_loss
    x = torch.rand(2, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        splat_loss.image_scores(x, x.clone())
    with pytest.raises(RuntimeError, match="no CPU path"):
        splat_loss.image_scores([x[0], x[1]], [x[1], x[0]])
    with pytest.raises(RuntimeError, match="shapes differ"):
        splat_loss.image_scores([x[0], torch.rand(3, 8, 9)], [x[0], torch.rand(3, 8, 9)])
    with pytest.raises(RuntimeError, match="shapes differ"):
        splat_loss.image_scores(x, torch.rand(2, 3, 9, 8))
    with pytest.raises(RuntimeError, match="2 renders but 1 targets"):
        splat_loss.image_scores(x, x[:1])
    with pytest.raises(NotImplementedError, match="target requires grad"):
        splat_loss.image_scores(x, x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="expected float32"):
        splat_loss.image_scores(x.double(), x.double())
    with pytest.raises(RuntimeError, match=r"expected a \(V, C, H, W\) batch"):
        splat_loss.image_scores(x[0], x[0])
    with pytest.raises(ValueError, match="empty list"):
        splat_loss.image_scores([], [])


def test_evaluate_views_refuses_no_views():
    import splat_train
    with pytest.raises(ValueError, match="no views"):
        splat_train.evaluate_views({}, [])


# ---- ScoreLog's ring, on host tensors ---------------------------------------------------------------
def _host_scores(k, V=3):
    import splat_loss
    rows = [torch.arange(V, dtype=torch.float32) + 10 * q + 100 * k for q in range(5)]
    return splat_loss.ImageScores(*rows, torch.tensor(float(k)))


def test_score_log_ring_order_and_overflow():
    import splat_loss
    import splat_train
    log = splat_train.ScoreLog(depth=2)
    assert log.drain() == [] and len(log) == 0
    for k in range(5):  # three more than the ring holds: the oldest is kept, not dropped
        log.put(k, _host_scores(k))
    assert len(log) == 5
    got = log.drain()
    assert [s for s, _ in got] == [0, 1, 2, 3, 4] and log.drain() == []
    for k, (_, values) in enumerate(got):
        assert isinstance(values, splat_loss.ImageScores)
        for have, want in zip(values, _host_scores(k)):
            assert have.shape == want.shape and torch.equal(have, want)
    log.put(7, torch.tensor([1.5, 2.5]))
    rest = log.close()
    assert [s for s, _ in rest] == [7] and torch.equal(rest[0][1], torch.tensor([1.5, 2.5]))
    assert log.close() == []
    with pytest.raises(RuntimeError, match="after close"):
        log.put(8, torch.tensor(0.0))
    with pytest.raises(ValueError, match="depth=0"):
        splat_train.ScoreLog(depth=0)
    with pytest.raises(TypeError, match="got float"):
        splat_train.ScoreLog().put(0, 1.0)


# ---- the mistakes the size-driven cases exist to catch, restated in float64 ------------------------
def _strip_sums(a, b, st):
    """Per wave strip, in the kernel's partial order (plane, strip row, strip column): sums of |x-y|, S, (x-y)^2."""
    C, H, W = a.shape
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    out = []
    for c in range(C):
        for y0 in range(0, H, STRIP_H):
            for x0 in range(0, W, STRIP_W):
                sl = (c, slice(y0, y0 + STRIP_H), slice(x0, x0 + STRIP_W))
                out.append((np.abs(d[sl]).sum(), st["S"][sl].sum(), (d[sl] ** 2).sum()))
    return np.array(out)


def test_second_sum_trip_sensitivity():
    a, b, rows, _ = case_reference(SECOND_TRIP)
    for v in range(SECOND_TRIP[0]):
        _, st = reference_view(a[v], b[v])
        parts = _strip_sums(a[v], b[v], st)
        assert len(parts) == 261
        assert np.allclose(parts.sum(0) / a[v].size, rows[v, :3], rtol=1e-12, atol=0)
        moved = np.abs(parts[:SUM_THREADS].sum(0) / a[v].size - rows[v, :3]) / tolerances(rows[v, :3])
        print(f"view {v}: partials past the first pass left out move (l1, ssim, mse) by {moved} tolerances")
        assert (moved > 100).all()
        psnr_wrong = -10.0 * math.log10(parts[:SUM_THREADS, 2].sum() / a[v].size)
        assert abs(psnr_wrong - rows[v, 3]) > 100 * PSNR_ABS


def test_launch_chunk_sensitivity():
    _, _, rows, mean = case_reference(CHUNK)
    wrong = rows[:LAUNCH_VIEWS, 4].mean()
    moved = abs(wrong - mean) / (ULP32 * abs(mean))  # the GPU test's bound on the mean: 1 float32 ulp
    print(f"the 33rd view left out moves the mean image loss by {moved:.0f} ulp")
    assert moved > 100
    # and its own row, were it left at another view's values
    assert (np.abs(rows[LAUNCH_VIEWS, :3] - rows[LAUNCH_VIEWS - 1, :3]) > 100 * tolerances(rows[LAUNCH_VIEWS, :3])).all()


@pytest.mark.parametrize("case", [PARTIAL[0], PARTIAL[1], PARTIAL[2]])
def test_partial_strip_sensitivity(case):
    V, C, H, W = case
    a, b, rows, _ = case_reference(case)
    FH, FW = -(-H // STRIP_H) * STRIP_H, -(-W // STRIP_W) * STRIP_W  # the strips' full extent
    assert (FH, FW) != (H, W)
    for v in range(V):
        pa, pb = (np.pad(t[v], ((0, 0), (0, FH - H), (0, FW - W))) for t in (a, b))
        _, st = reference_view(pa, pb)  # zero outside the image, as the kernel stages it
        inside = st["S"][:, :H, :W].sum() / a[v].size
        assert abs(inside - rows[v, 1]) <= 1e-12
        # the last strips taken for full: SSIM of the pixels outside the image summed as well
        ssim_wrong = st["S"].sum() / a[v].size
        assert abs(ssim_wrong - rows[v, 1]) > 100 * tolerances(rows[v, 1])
        # or every mean taken over the strips' pixel count
        scaled = rows[v, :3] * (H * W) / (FH * FW)
        moved = np.abs(scaled - rows[v, :3]) / tolerances(rows[v, :3])
        print(f"{case} view {v}: full-strip pixel count moves (l1, ssim, mse) by {moved} tolerances")
        assert (moved > 100).all()
