"""The exact saturation re-walk with more flagged pixels than its list holds (-m gpu).

k_render_fwd flags every pixel whose final T lies within the drift window of 1e-4 and appends a record to
IMAGE tsat_list, which holds tsat_capacity(W H) = W H / 8 + 64 records.  Two opaque layers flag a pixel:
alpha is clamped to 0.99f, so T1 = 1 - 0.99f = 0.00999999046 and T2 = fl(T1 T1) = 9.999981e-05, below the
reference's 1e-4f (it stops with n_contrib = 1) and above the fast walk's widened stop 1e-4 (1 - t_window)
(it blends the second layer).  Opaque sheets across the whole image therefore flag every pixel, 8x the
capacity; k_render_tsat then finds the flagged pixels from the per-pixel state instead of the list
(DESIGN.md 3).  Every case is compared with the CPU oracle with no allowance, forward and backward, after
asserting from the oracle state and from the device-side count that it is on the intended side of the
capacity.
"""
import numpy as np
import pytest
import torch

import splat_scenes as S
from oracle import oracle as O
from test_gpu_parity import (STATS, _gpu_backward, _gpu_forward, _np, _ora_forward,  # noqa: F401 -- STATS: the stat dump
                             check_backward, check_forward)

pytestmark = pytest.mark.gpu

BG = (0.2, 0.5, 0.9)
# name: (W, H, sheet scale, faint sheets in front, expected n_contrib everywhere (None: not uniform), over capacity)
CASES = {
    "over": (32, 32, 40.0, 0, 1, True),
    "over_ragged": (40, 24, 40.0, 0, 1, True),  # partial tiles: the pixels outside the image are never flagged
    # 70 sheets of opacity 1/512 (alpha < 1/255: skipped, T stays 1) nearer the camera: the contributor is list
    # entry 71, past the first 64-entry segment boundary
    "over_late": (32, 32, 40.0, 70, 71, True),
    # control: sheets narrow enough that only the pixels around the centre have two clamped layers (r <= 0.14
    # sigma), fewer than the list holds
    "under": (64, 64, 7.5, 0, None, False),
}


def capacity(W, H):
    return W * H // 8 + 64  # gsr_common.h tsat_capacity


def sheets(W, H, scale, n_faint):
    """Three opaque isotropic Gaussians on the optical axis at depths 3, 3.5 and 4 (world z -1, -0.5, 0 seen
    from look_at(0, 0, 4), focal 32), behind n_faint faint ones at depths 0.5 .. 2.5."""
    z = np.concatenate([np.linspace(-3.5, -1.5, n_faint), [-1.0, -0.5, 0.0]]).astype(np.float32)
    P = z.size
    g = torch.Generator().manual_seed(21)
    m = torch.zeros(P, 3)
    m[:, 2] = torch.from_numpy(z)
    op = torch.full((P, 1), 1.0 / 512.0)
    op[n_faint:] = 1.0
    a = {"means3D": m, "colors_precomp": 0.1 + 0.8 * torch.rand(P, 3, generator=g), "opacities": op,
         "scales": torch.full((P, 3), float(scale)), "rotations": torch.tensor([[1.0, 0, 0, 0]]).repeat(P, 1)}
    rs = S.render_settings(W, H, S.intrinsics(32.0, W, H), S.look_at(0, 0, 4), device="cpu")
    return a, rs._replace(bg=torch.tensor(BG, dtype=torch.float32))


def both_clamped(st):
    """Pixels whose first two live contributors (power <= 0, alpha >= 1/255, in list order) both have
    o exp(power) above 0.99f: the pixels the forward flags (fp32 numpy on the oracle's conic_opacity / xy)."""
    H, W = st["H"], st["W"]
    gx = (W + 15) // 16
    f = np.float32
    co, xy, pl = st["conic_opacity"], st["xy"], st["point_list"]
    total = 0
    for tile, (r0, r1) in enumerate(st["ranges"].astype(np.int64)):
        tx0, ty0 = (tile % gx) * 16, (tile // gx) * 16
        ys, xs = np.mgrid[ty0:min(ty0 + 16, H), tx0:min(tx0 + 16, W)]
        live = np.zeros(xs.shape, np.int32)
        clamped = np.zeros(xs.shape, np.int32)
        for k in range(r0, r1):
            g = int(pl[k])
            dx, dy = xy[g, 0] - xs.astype(f), xy[g, 1] - ys.astype(f)
            power = f(-0.5) * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy
            raw = co[g, 3] * np.exp(power)
            ok = (power <= 0) & (np.minimum(f(0.99), raw) >= f(1.0 / 255.0)) & (live < 2)
            clamped += ok & (raw > f(0.99))
            live += ok
            if (live >= 2).all():
                break
        total += int((clamped == 2).sum())
    return total


@pytest.mark.parametrize("case", list(CASES))
def test_saturation_overflow(case, cuda):
    W, H, scale, n_faint, nc, over = CASES[case]
    a, rs = sheets(W, H, scale, n_faint)
    P = a["means3D"].shape[0]
    cap = capacity(W, H)
    st = _ora_forward(a, rs)
    # preconditions from the oracle: the reference's stop, and the flagged count's side of the capacity
    assert (st["radii"] > 0).all() and st["depths"].min() > 0.2
    if nc is not None:
        assert (st["n_contrib"] == nc).all(), np.unique(st["n_contrib"])
    flagged = both_clamped(st)
    if over:
        assert flagged > cap, (flagged, cap)
    else:
        assert 0 < flagged < cap, (flagged, cap)
    fw = _gpu_forward(a, rs, cuda)
    count = int(_np(fw["dec"]["tsat_count"])[0])
    print(f"{case}: both-clamped pixels {flagged}, tsat_count {count}, capacity {cap}")
    if over:
        assert count > cap, (count, cap)
    else:
        assert 0 < count <= cap, (count, cap)
    check_forward(fw, st, 0.0)
    dl = S.upstream_grad(H, W, device="cpu")
    gref = O.backward(st, dl.numpy())
    gb = _gpu_backward(a, rs, cuda, fw, dl)
    check_backward(gb, gref, P, st["M"], 0.0)
