"""Forward-only scores of a timestep's views on the GPU: splat_loss.image_scores (k_ssim_eval, k_scores_sum,
k_scores_mean), the no-grad path of splat_loss.l1_and_ssim, splat_train.evaluate_views and ScoreLog.

The cases, their seeded images and float64 references come from tests/test_scores.py, which also shows on the
CPU that each size-driven case moves by more than 100 tolerances under the mistake it exists to catch.  For
every case:

* per view, l1 and ssim are bitwise what the training path (l1_and_ssim on a render that requires grad: k_ssim_fwd
  with its derivative maps, k_ssim_sum) returns for that view alone; image_loss is bitwise torch's float32
  0.8 * l1 + 0.2 * (1.0 - ssim); the mean is within 1 float32 ulp of the float64 mean of the image_loss values;
* against the float64 restatement: l1, ssim and mse within 1e-5 |ref| + 1e-7, the band tests/test_loss.py puts on
  l1 and ssim of noise pairs; on the identical and the constant pair, where sigma = <x^2> - mu^2 cancels in fp32,
  within max(1e-5 |ref|, 2 yardsticks) as test_gpu_loss_image_families does (the yardstick: what a float32 torch
  restatement misses the oracle by, measured here on the CPU); psnr within 10 / ln 10 * 1e-5, absolute;
* a batch's slices give the separately allocated views' bits; a second run repeats them; permuting the views
  permutes the rows; a NaN in one view stays in its row and the mean.
"""
import functools
import math

import numpy as np
import pytest
import torch

import test_scores as TS
from test_loss import _torch_restatement

pytestmark = pytest.mark.gpu


def _separate(cuda, batch):
    """Every view a tensor of its own allocation, as rasterize_parameters returns them."""
    return [torch.from_numpy(np.ascontiguousarray(batch[v])).to(cuda) for v in range(batch.shape[0])]


def _rows(res):
    return torch.stack([res.l1, res.ssim, res.mse, res.psnr, res.image_loss], 1)


def _same_bits(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def _yardstick(case, v):
    """What float32 arithmetic misses the float64 oracle by on view v's pair: (l1, ssim)."""
    a, b, ref, _ = TS.case_reference(case)
    l32, s32, _ = _torch_restatement(a[v], b[v], torch.float32)
    return abs(l32 - ref[v, 0]), abs(s32 - ref[v, 1])


def _training_path(render, target):
    import splat_loss
    l1, ssim = splat_loss.l1_and_ssim(render.clone().requires_grad_(True), target)
    assert l1.requires_grad  # the kernels with the derivative maps
    return torch.stack([l1.detach(), ssim.detach()])


@pytest.mark.parametrize("case", TS.CASES, ids=lambda c: "V%d_C%d_%dx%d" % c)
def test_gpu_scores_case(cuda, case):
    import splat_loss
    V, C, H, W = case
    a, b, ref, _ = TS.case_reference(case)
    renders, targets = _separate(cuda, a), _separate(cuda, b)
    res = splat_loss.image_scores(renders, targets)
    got = _rows(res)
    assert got.shape == (V, 5) and res.mean_image_loss.shape == () and not got.requires_grad

    # bitwise against the training path, view by view
    alone = torch.stack([_training_path(r, t) for r, t in zip(renders, targets)])
    assert _same_bits(got[:, :2], alone), (got[:, :2] - alone).abs().max().item()
    assert _same_bits(res.image_loss, 0.8 * res.l1 + 0.2 * (1.0 - res.ssim))
    for v in range(V):  # and on the two float32 scalars
        assert _same_bits(res.image_loss[v], 0.8 * res.l1[v] + 0.2 * (1.0 - res.ssim[v]))
    mean64 = float(res.image_loss.double().cpu().mean())
    assert abs(float(res.mean_image_loss) - mean64) <= float(np.spacing(np.float32(abs(mean64))))

    # against the float64 restatement
    host = got.double().cpu().numpy()
    for v in range(V):
        special = V >= 3 and v in (1, 2)  # the identical and the constant pair
        tol = TS.tolerances(ref[v, :3])
        if special:
            yl, ys = _yardstick(case, v)
            tol = np.array([max(TS.REL * abs(ref[v, 0]), 2 * yl), max(TS.REL * abs(ref[v, 1]), 2 * ys), tol[2]])
        err = np.abs(host[v, :3] - ref[v, :3])
        print(f"{case} view {v}: (l1, ssim, mse) errors {err} tolerances {tol}, psnr {host[v, 3]} ref {ref[v, 3]}")
        assert (err <= tol).all(), (v, host[v], ref[v])
        if math.isinf(ref[v, 3]):
            assert host[v, 0] == 0 and host[v, 2] == 0 and host[v, 3] == math.inf
        else:
            assert abs(host[v, 3] - ref[v, 3]) <= TS.PSNR_ABS

    # pointer handling: slices of one batch; repeatability
    batch = splat_loss.image_scores(torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda))
    again = splat_loss.image_scores(renders, targets)
    for other in (batch, again):
        assert _same_bits(_rows(other), got) and _same_bits(other.mean_image_loss, res.mean_image_loss)

    # view independence: a permutation of the views permutes the rows
    perm = np.random.default_rng(V).permutation(V)
    moved = splat_loss.image_scores([renders[p] for p in perm], [targets[p] for p in perm])
    assert _same_bits(_rows(moved), got[torch.from_numpy(perm).to(cuda)])

    # NaN containment
    j = 3 if V > 3 else V - 1
    poisoned = list(renders)
    poisoned[j] = renders[j].clone()
    poisoned[j][C - 1, H // 2, W // 2] = float("nan")
    bad = splat_loss.image_scores(poisoned, targets)
    rows = _rows(bad)
    keep = torch.arange(V, device=cuda) != j
    assert torch.isnan(rows[j]).all() and torch.isnan(bad.mean_image_loss)
    assert _same_bits(rows[keep], got[keep])


def test_gpu_scores_unaligned_view(cuda):
    """One view's storage 4 bytes off a 16-byte boundary: the same bits as from aligned storage."""
    import splat_loss
    case = (2, 3, 23, 128)
    a, b, _, _ = TS.case_reference(case)
    renders, targets = _separate(cuda, a), _separate(cuda, b)
    want = _rows(splat_loss.image_scores(renders, targets))
    for side in (renders, targets):
        flat = torch.empty(side[1].numel() + 1, dtype=torch.float32, device=cuda)
        assert flat.data_ptr() % 16 == 0
        off = flat[1:].view(side[1].shape)
        off.copy_(side[1])
        assert off.data_ptr() % 16 == 4 and off.is_contiguous()
        side[1] = off
    assert _same_bits(_rows(splat_loss.image_scores(renders, targets)), want)


def test_gpu_scores_no_views(cuda):
    import splat_loss
    none = torch.empty(0, 3, 8, 8, device=cuda)
    res = splat_loss.image_scores(none, none)
    assert all(t.shape == (0,) for t in res[:5]) and torch.isnan(res.mean_image_loss)


@pytest.mark.parametrize("shape", [(3, 21, 64), (3, 33, 65), (1, 1, 1), (2, 3, 40, 70), (3, 920, 190)])
def test_gpu_l1_and_ssim_no_grad_values(cuda, shape):
    """Under no_grad, and for a render that does not require grad, l1_and_ssim takes the forward-only kernels: the
    same bits as the training kernels give."""
    import splat_loss
    rng = np.random.default_rng(sum(shape))
    x = torch.from_numpy(rng.random(shape, dtype=np.float32)).to(cuda)
    y = torch.from_numpy(rng.random(shape, dtype=np.float32)).to(cuda)
    want = _training_path(x, y)
    with torch.no_grad():
        got = torch.stack(splat_loss.l1_and_ssim(x.clone().requires_grad_(True), y))
    plain = splat_loss.l1_and_ssim(x, y)
    assert not plain[0].requires_grad and plain[0].shape == () and plain[1].shape == ()
    assert _same_bits(got, want) and _same_bits(torch.stack(plain), want)
    assert _same_bits(splat_loss.l1_and_ssim_loss(x, y)[1], 1.0 - want[1])


def test_gpu_l1_and_ssim_no_grad_memory(cuda):
    """At (3, 360, 640) the three derivative maps are planes * H * W * 12 bytes: the no-grad call allocates less
    than that in all, the grad-mode call at least that."""
    import splat_loss
    planes, H, W = 3, 360, 640
    maps = planes * H * W * 12
    x = torch.rand(planes, H, W, device=cuda)
    y = torch.rand(planes, H, W, device=cuda)
    xg = x.clone().requires_grad_(True)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(cuda)
        before = torch.cuda.memory_allocated(cuda)
        out = fn()
        torch.cuda.synchronize()
        delta = torch.cuda.max_memory_allocated(cuda) - before
        del out
        return delta

    def no_grad():
        with torch.no_grad():
            return splat_loss.l1_and_ssim(xg, y)

    quiet, training = peak(no_grad), peak(lambda: splat_loss.l1_and_ssim(xg, y))
    print(f"allocated over the call: no_grad {quiet} bytes, grad mode {training} bytes, the three maps {maps} bytes")
    assert quiet < maps <= training


def test_gpu_evaluate_views(cuda):
    """Three views of a small cloud: evaluate_views' rows are the bits of rendering each view under no_grad and
    scoring it alone."""
    import splat_loss
    import splat_scenes as S
    import splat_train
    from diff_gaussian_rasterization import rasterize_parameters
    W, H = 96, 72
    params = S.synthetic_cloud(2000, 0.03, seed=2, device=cuda)
    g = torch.Generator().manual_seed(5)
    views = [splat_train.View(k, S.render_settings(W, H, S.intrinsics(100.0, W, H), S.look_at(yaw, 0.2, 4.0),
                                                   device=cuda),
                              torch.rand(3, H, W, generator=g).to(cuda), None)
             for k, yaw in enumerate((0.0, 35.0, 200.0))]
    res = splat_train.evaluate_views(params, views)
    got = _rows(res)
    assert got.shape == (3, 5) and bool((res.l1 > 0).all())
    for k, view in enumerate(views):
        with torch.no_grad():
            image = rasterize_parameters(params, view.render_settings)[0]
        one = splat_loss.image_scores([image], [view.image])
        assert _same_bits(_rows(one)[0], got[k])
    mean64 = float(res.image_loss.double().cpu().mean())
    assert abs(float(res.mean_image_loss) - mean64) <= float(np.spacing(np.float32(abs(mean64))))


def test_gpu_score_log(cuda):
    """Every step put comes back once, in order, with the device values; an empty log drains to nothing; two puts
    more than the ring holds block on the oldest slots and lose none."""
    import splat_loss
    import splat_train
    a, b, _, _ = TS.case_reference((5, 3, 21, 64))
    renders, targets = _separate(cuda, a), _separate(cuda, b)
    log = splat_train.ScoreLog(depth=3)
    assert log.drain() == [] and len(log) == 0
    put = []
    for step in range(5):
        res = splat_loss.image_scores(renders[step:] + renders[:step], targets)
        log.put(10 + step, res)
        put.append(res)
    assert len(log) == 5
    torch.cuda.synchronize()
    got = log.drain()
    assert [s for s, _ in got] == [10, 11, 12, 13, 14] and log.drain() == []
    for (_, values), res in zip(got, put):
        assert isinstance(values, splat_loss.ImageScores)
        for have, want in zip(values, res):
            assert not have.is_cuda and _same_bits(have, want.cpu())
    log.put(15, put[0].mean_image_loss)
    rest = log.close()
    assert [s for s, _ in rest] == [15] and _same_bits(rest[0][1], put[0].mean_image_loss.cpu())
