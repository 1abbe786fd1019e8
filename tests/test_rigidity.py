"""The rigidity term and the neighbour search (splat_rigidity, csrc/gsr_rigidity.hip).

CPU: the checkers of tests/rigidity_ref.py (a float64 torch restatement of train.py:325-351 and a numpy
brute-force k-nearest-neighbour search) reproduce what the reference itself computed
(tests/golden/reference_rigidity.npz, written by tests/golden/gen_golden_rigidity.py); splat_rigidity
refuses CPU tensors.  GPU: the HIP kernels against those checkers and against the reference's saved
values.  Gradient band everywhere but the golden comparisons: |got - ref| <= 1e-4 |ref| + 1e-6 max|ref|
with no value outside (the reference's own fp32 run stays inside it, at most 8.4e-7 max|ref| off its
float64 run at these perturbations).

Shapes chosen for the paths they reach: k_rigid_sum strides 256 threads over the per-block partials, so a second
trip needs more than 256 partials, F > 65,536 (test_sum_second_trip: F = 65,836); k_knn<32> serves every
k != 20 and is run at k = 1, 21 and 32 = K, and at n = 256 / 257 (one full candidate tile, then a tile and a
query block with one live lane).  NOT covered: the query split of launch_knn -- its second launch (q0 > 0)
needs n^2 > 2^37 pairs, n > 370,727 points: a full-size run of minutes, not a test."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rigidity_ref as RR
import splat_rigidity as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "reference_rigidity.npz"))
PERTURBATIONS = [(0.003, 0.05), (0.03, 0.5)]


def _t(name):
    return torch.from_numpy(GOLD[name])


def _gold_mask():
    return _t("prev_segmentation_masks")[:, 0] > 0.5


def _band(name, got, ref, rtol, atol_frac):
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = np.abs(ref).max()
    err = np.abs(got - ref)
    bad = err > rtol * np.abs(ref) + atol_frac * scale
    print(f"{name}: worst {err.max():.3e} = {err.max() / max(scale, 1e-300):.3e} max|ref| ({scale:.3e}), outside {bad.sum()}/{bad.size}")
    assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} outside the band, worst {err.max():.3g} (scale {scale:.3g})"


def _rel(name, got, ref, tol):
    got, ref = float(got), float(ref)
    print(f"{name}: got {got:.9e} ref {ref:.9e} rel {abs(got - ref) / abs(ref):.3e}")
    assert abs(got - ref) <= tol * abs(ref), (name, got, ref)


# ---- CPU ------------------------------------------------------------------------------------------
def test_restatement_reproduces_reference_loss_and_gradients():
    mask = _gold_mask()
    loss, gm, gq = RR.rigidity_loss_and_grads(_t("cur_means"), _t("cur_rotation_quaternions"), mask,
                                              _t("knn_indices"), _t("weights"), _t("fi_inverted_rotations"),
                                              _t("fi_offsets_to_neighbors"))
    _rel("loss", loss, GOLD["loss"], 1e-6)
    _band("grad_means", gm.numpy(), GOLD["grad_means"], 2e-4, 2e-5)
    _band("grad_rotation_quaternions", gq.numpy(), GOLD["grad_rotation_quaternions"], 2e-4, 2e-5)
    assert (GOLD["grad_means"][~mask.numpy()] == 0).all() and (gm[~mask] == 0).all() and (gq[~mask] == 0).all()


def test_restatement_reproduces_reference_foreground_info():
    inv, off = RR.foreground_info(_t("prev_means"), _t("prev_rotation_quaternions"), _gold_mask(), _t("knn_indices"),
                                  dtype=torch.float32)
    assert np.abs(inv.numpy() - GOLD["fi_inverted_rotations"]).max() <= 1e-6
    assert np.abs(off.numpy() - GOLD["fi_offsets_to_neighbors"]).max() <= 1e-6


def test_brute_force_knn_reproduces_reference_neighbours():
    fg = GOLD["prev_means"][_gold_mask().numpy()]
    idx, d2 = RR.brute_force_knn(fg, GOLD["knn_indices"].shape[1])
    assert np.array_equal(idx, GOLD["knn_indices"])
    assert (np.abs(d2 - GOLD["knn_squared_distances"]) <= 1e-12 * GOLD["knn_squared_distances"]).all()
    w = np.exp(-2000 * d2).astype(np.float32)
    assert np.array_equal(w, GOLD["weights"])


def test_no_cpu_path():
    params = {"means": _t("cur_means"), "rotation_quaternions": _t("cur_rotation_quaternions"),
              "segmentation_masks": _t("prev_segmentation_masks")}
    ni = SimpleNamespace(indices=_t("knn_indices"), weights=_t("weights"))
    fi = SimpleNamespace(inverted_rotations=_t("fi_inverted_rotations"),
                         offsets_to_neighbors=_t("fi_offsets_to_neighbors"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.calculate_rigidity_loss(params, ni, fi)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.knn(_t("prev_means"), 20)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.create_neighbor_info(params)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.create_foreground_info(params, _t("knn_indices"))
    with pytest.raises(ValueError):
        R.knn(torch.zeros(20, 3), 20)  # n <= k is refused before anything else


# ---- GPU: neighbour search ------------------------------------------------------------------------
KNN_SHAPES = [(4, 3), (21, 20), (64, 20), (65, 20), (300, 20), (4099, 20),
              (2, 1), (22, 21), (33, 32), (256, 32), (257, 32), (257, 21)]


def _knn_points(n):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(100 + n))


def _knn_reference(pts, n, k):
    """Brute-force (indices, distances) with one distance more than k where it exists, and the positions whose
    distance is separated from both sorted neighbours by more than 1e-9 relative."""
    kk = min(k + 1, n - 1)  # the (k + 1)-th distance bounds the last position (absent when n = k + 1)
    ridx, rd2 = RR.brute_force_knn(pts.numpy(), kk)
    ext = np.concatenate([np.full((n, 1), -np.inf), rd2, np.full((n, k + 2 - rd2.shape[1] - 1), np.inf)], axis=1)
    lo, mid, hi = ext[:, :k], ext[:, 1:k + 1], ext[:, 2:k + 2]
    clear = (mid - lo > 1e-9 * mid) & (hi - mid > 1e-9 * mid)
    return ridx, rd2, clear


@pytest.mark.parametrize("n,k", KNN_SHAPES)
def test_knn_seeds_stay_under_the_near_tie_cap(n, k):
    """The brute-force reference alone: the seeded points leave at most 1e-3 of the positions to the near-tie
    exclusion, so the GPU test's index comparison covers the rest."""
    ridx, rd2, clear = _knn_reference(_knn_points(n), n, k)
    assert clear.shape == (n, k) and (~clear).mean() <= 1e-3
    assert (ridx != np.arange(n)[:, None]).all() and (np.diff(rd2, axis=1) >= 0).all()


@pytest.mark.parametrize("n,k", [(257, 32), (257, 21), (300, 20)])
def test_knn_reference_is_sensitive_to_the_second_candidate_tile(n, k):
    """The brute-force search with the candidates past the first tile of 256 left out: the point(s) of the
    second tile are among somebody's k nearest, so index lists change at positions the GPU test compares."""
    pts = _knn_points(n)
    ridx, _, clear = _knn_reference(pts, n, k)
    first_tile, _ = RR.brute_force_knn(pts.numpy()[:256], k)
    changed = first_tile != ridx[:256, :k]
    print(f"n={n} k={k}: {changed.sum()} compared positions change without the second candidate tile")
    assert (changed & clear[:256]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", KNN_SHAPES)
def test_knn_matches_brute_force(cuda, n, k):
    pts = _knn_points(n)
    idx, d2 = R.knn(pts.to(cuda), k)
    assert idx.dtype == torch.int64 and d2.dtype == torch.float64 and idx.shape == d2.shape == (n, k)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    ridx, rd2, clear = _knn_reference(pts, n, k)
    assert (np.diff(d2, axis=1) >= 0).all()
    assert (np.abs(d2 - rd2[:, :k]) <= 1e-12 * rd2[:, :k]).all()
    assert (idx != np.arange(n)[:, None]).all()
    print(f"n={n}: {(~clear).sum()}/{clear.size} positions excluded as near-ties")
    assert (~clear).mean() <= 1e-3
    assert np.array_equal(idx[clear], ridx[:, :k][clear])


@pytest.mark.gpu
def test_knn_exact_duplicates(cuda):
    g = torch.Generator().manual_seed(7)
    base = torch.rand(20, 3, generator=g)
    pts = torch.cat([base, base])  # point i and point i + 20 coincide
    idx, d2 = R.knn(pts.to(cuda), 3)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    twin = (np.arange(40) + 20) % 40
    assert np.array_equal(idx[:, 0], twin) and (d2[:, 0] == 0).all()
    assert (idx != np.arange(40)[:, None]).all()
    # positions 1 and 2 are the two copies of the nearest other point: equal distance, lower index first
    assert (d2[:, 1] == d2[:, 2]).all() and (d2[:, 1] > 0).all()
    assert np.array_equal(idx[:, 2], idx[:, 1] + 20)
    ridx, rd2 = RR.brute_force_knn(pts.numpy(), 3)
    assert np.array_equal(idx, ridx) and np.array_equal(d2, rd2)


# ---- GPU: loss and gradients ----------------------------------------------------------------------
def _cloud(P, mask, seed, spread=0.2):
    g = torch.Generator().manual_seed(seed)
    m = mask.float()
    return {"means": torch.rand(P, 3, generator=g) * spread, "rotation_quaternions": torch.randn(P, 4, generator=g),
            "segmentation_masks": torch.stack((m, torch.zeros(P), 1 - m), 1)}, g


def _masks(P):
    if P == 5:
        return torch.tensor([True, True, False, True, True])
    if P == 130:
        return torch.arange(P) % 2 == 0  # interleaved foreground / background rows
    return torch.rand(P, generator=torch.Generator().manual_seed(P)) < 0.6


def _perturbed(prev, g, dm, dq):
    P = prev["means"].shape[0]
    cur = dict(prev)
    cur["means"] = prev["means"] + dm * torch.randn(P, 3, generator=g)
    cur["rotation_quaternions"] = prev["rotation_quaternions"] + dq * torch.randn(P, 4, generator=g)
    return cur


def _gpu_run(cur, ni, fi, dev, grads=(True, True), scale=1.0):
    p = {k: v.detach().to(dev) for k, v in cur.items()}
    p["means"].requires_grad_(grads[0])
    p["rotation_quaternions"].requires_grad_(grads[1])
    loss = R.calculate_rigidity_loss(p, ni, fi)
    if any(grads):
        (scale * loss).backward()
    return loss.detach().cpu(), p["means"].grad, p["rotation_quaternions"].grad


def _ref_run(cur, ni, fi):
    mask = cur["segmentation_masks"][:, 0] > 0.5
    return RR.rigidity_loss_and_grads(cur["means"], cur["rotation_quaternions"], mask, ni.indices.cpu(),
                                      ni.weights.cpu(), fi.inverted_rotations.cpu(), fi.offsets_to_neighbors.cpu())


def _check_parity(cur, ni, fi, dev):
    loss, gm, gq = _gpu_run(cur, ni, fi, dev)
    rl, rm, rq = _ref_run(cur, ni, fi)
    _rel("loss", loss, rl, 1e-5)
    _band("grad_means", gm.cpu().numpy(), rm.numpy(), 1e-4, 1e-6)
    _band("grad_rotation_quaternions", gq.cpu().numpy(), rq.numpy(), 1e-4, 1e-6)
    bg = ~(cur["segmentation_masks"][:, 0] > 0.5)
    assert (gm.cpu()[bg] == 0).all() and (gq.cpu()[bg] == 0).all()
    return loss, gm, gq


@functools.lru_cache(maxsize=None)
def _state(P, k, dev):
    """The previous state of a seeded cloud with its neighbour and foreground info (built on the GPU)."""
    prev, g = _cloud(P, _masks(P), seed=P + k)
    pg = {n: v.to(dev) for n, v in prev.items()}
    ni = R.create_neighbor_info(pg, k)
    fi = R.create_foreground_info(pg, ni.indices)
    return prev, g.get_state(), ni, fi


def _case(P, k, pert, dev):
    prev, gstate, ni, fi = _state(P, k, dev)
    g = torch.Generator()
    g.set_state(gstate)
    return _perturbed(prev, g, *PERTURBATIONS[pert]), ni, fi


@pytest.mark.gpu
@pytest.mark.parametrize("pert", [0, 1])
@pytest.mark.parametrize("P,k", [(5, 3), (130, 20), (1000, 20)])
def test_loss_and_gradients_match_restatement(cuda, P, k, pert):
    cur, ni, fi = _case(P, k, pert, cuda)
    F = int(_masks(P).sum())
    assert ni.indices.shape == (F, k) and ni.indices.dtype == torch.int64 and ni.weights.dtype == torch.float32
    fg = cur["segmentation_masks"][:, 0] > 0.5
    prev = _state(P, k, cuda)[0]
    ridx, rd2 = RR.brute_force_knn(prev["means"][fg].numpy(), k)
    assert np.array_equal(ni.indices.cpu().numpy(), ridx)  # the same float64 operations, the same tie rule
    # exp(-2000 d^2) in float64, then float32: one float32 rounding, plus a float64 ulp of the two exp()
    assert np.allclose(ni.weights.cpu().numpy(), np.exp(-2000 * rd2).astype(np.float32), rtol=2e-7, atol=0)
    _check_parity(cur, ni, fi, cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("pert", [0, 1])
def test_zero_weights(cuda, pert):
    P, k = 1000, 20
    prev, g = _cloud(P, _masks(P), seed=31, spread=2.0)
    pg = {n: v.to(cuda) for n, v in prev.items()}
    ni = R.create_neighbor_info(pg, k)
    fi = R.create_foreground_info(pg, ni.indices)
    zero = (ni.weights == 0).float().mean().item()
    print(f"zero weights: {zero:.3f}")
    assert 0.5 < zero < 1.0
    cur = _perturbed(prev, g, *PERTURBATIONS[pert])
    _check_parity(cur, ni, fi, cuda)
    # every weight zero: each term is exactly sqrt(1e-20) and nothing has a gradient
    none = SimpleNamespace(indices=ni.indices, weights=torch.zeros_like(ni.weights))
    loss, gm, gq = _gpu_run(cur, none, fi, cuda)
    assert abs(float(loss) - 1e-10) <= 1e-16
    assert (gm == 0).all() and (gq == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("pert", [0, 1])
def test_uneven_reverse_adjacency(cuda, pert):
    """Every Gaussian lists row 0 (a reverse list of ~F edges) and nobody lists the last one (an empty one)."""
    F, k, B = 300, 20, 30
    mask = torch.arange(F + B) >= B  # background rows first: foreground index != row
    prev, g = _cloud(F + B, mask, seed=77)
    i, j = torch.arange(F)[:, None], torch.arange(k)[None]
    idx = 1 + (i + j) % (F - 2)  # targets in [1, F - 2]
    idx[:, 0] = 0
    idx[0, 0] = 1
    w = torch.rand(F, k, generator=g)
    ni = SimpleNamespace(indices=idx.to(cuda), weights=w.to(cuda))
    pg = {n: v.to(cuda) for n, v in prev.items()}
    fi = R.create_foreground_info(pg, ni.indices)
    packed = R.pack_neighbors(pg, ni.indices, ni.weights)
    counts = np.diff(packed.reverse_offsets.cpu().numpy())
    assert counts[0] == F - 1 and counts[F - 1] == 0 and counts.sum() == F * k
    _check_parity(_perturbed(prev, g, *PERTURBATIONS[pert]), ni, fi, cuda)


SUM_TRIP = 256 * 256  # k_rigid_sum: 256 threads over the partials of 256-row blocks


def _second_trip_cloud():
    """F = 65,536 + 300 foreground rows (258 block partials) after 30 background rows, k = 3, the neighbour lists
    of test_uneven_reverse_adjacency: every Gaussian lists row 0, nobody lists the last one."""
    F, k, B = SUM_TRIP + 300, 3, 30
    mask = torch.arange(F + B) >= B
    prev, g = _cloud(F + B, mask, seed=78)
    i, j = torch.arange(F)[:, None], torch.arange(k)[None]
    idx = 1 + (i + j) % (F - 2)
    idx[:, 0] = 0
    idx[0, 0] = 1
    return F, k, mask, prev, g, idx, torch.rand(F, k, generator=g)


@pytest.mark.parametrize("pert", [0, 1])
def test_reference_is_sensitive_to_the_sum_second_trip(pert):
    """The float64 restatement with the partials past the first 256 left out of the sum (the first 65,536 rows'
    terms over the same F k): the loss moves by more than 100 of the GPU test's 1e-5 tolerances."""
    F, k, mask, prev, g, idx, w = _second_trip_cloud()
    inv, off = RR.foreground_info(prev["means"], prev["rotation_quaternions"], mask, idx, dtype=torch.float32)
    cur = _perturbed(prev, g, *PERTURBATIONS[pert])
    fm, fq = cur["means"].double()[mask], RR.unit(cur["rotation_quaternions"].double())[mask]
    rot = RR.rotation_matrices(RR.hamilton(fq, inv.double()))
    v = torch.einsum("frc,fkr->fkc", rot, fm[idx] - fm[:, None])
    terms = ((v - off.double()).pow(2).sum(-1) * w.double() + 1e-20).sqrt()
    full = RR.rigidity_loss(cur["means"], cur["rotation_quaternions"], mask, idx, w, inv, off)
    assert abs(float(terms.mean()) - float(full)) <= 1e-12 * float(full)
    first_trip = float(terms[:SUM_TRIP].sum()) / (F * k)
    moved = abs(first_trip - float(full)) / (1e-5 * float(full))
    print(f"first trip only: the loss moves by {moved:.0f} tolerances")
    assert moved > 100


@pytest.mark.gpu
@pytest.mark.parametrize("pert", [0, 1])
def test_sum_second_trip(cuda, pert):
    F, k, mask, prev, g, idx, w = _second_trip_cloud()
    ni = SimpleNamespace(indices=idx.to(cuda), weights=w.to(cuda))
    pg = {n: v.to(cuda) for n, v in prev.items()}
    fi = R.create_foreground_info(pg, ni.indices)
    assert R.pack_neighbors(pg, ni.indices, ni.weights).F == F > SUM_TRIP
    _check_parity(_perturbed(prev, g, *PERTURBATIONS[pert]), ni, fi, cuda)


@pytest.mark.gpu
def test_golden(cuda):
    prev = {n: _t("prev_" + n).to(cuda) for n in ("means", "rotation_quaternions", "segmentation_masks")}
    ni = SimpleNamespace(indices=_t("knn_indices").to(cuda), weights=_t("weights").to(cuda))
    fi = R.create_foreground_info(prev, ni.indices)
    assert (fi.inverted_rotations.cpu() - _t("fi_inverted_rotations")).abs().max() <= 1e-6
    assert (fi.offsets_to_neighbors.cpu() - _t("fi_offsets_to_neighbors")).abs().max() <= 1e-6
    ref_fi = SimpleNamespace(inverted_rotations=_t("fi_inverted_rotations").to(cuda),
                             offsets_to_neighbors=_t("fi_offsets_to_neighbors").to(cuda))
    cur = {"means": _t("cur_means"), "rotation_quaternions": _t("cur_rotation_quaternions"),
           "segmentation_masks": _t("prev_segmentation_masks")}
    loss, gm, gq = _gpu_run(cur, ni, ref_fi, cuda)
    _rel("loss", loss, GOLD["loss"], 1e-5)
    _band("grad_means", gm.cpu().numpy(), GOLD["grad_means"], 2e-4, 2e-5)
    _band("grad_rotation_quaternions", gq.cpu().numpy(), GOLD["grad_rotation_quaternions"], 2e-4, 2e-5)
    own = R.create_neighbor_info(prev, 20)
    assert np.array_equal(own.indices.cpu().numpy(), GOLD["knn_indices"])
    assert np.allclose(own.weights.cpu().numpy(), GOLD["weights"], rtol=2e-7, atol=0)


@pytest.mark.gpu
def test_unperturbed_state(cuda):
    prev, _, ni, fi = _state(1000, 20, cuda)
    loss, gm, gq = _gpu_run(prev, ni, fi, cuda)
    print(f"unperturbed loss {float(loss):.4e} (reference, golden case: {float(GOLD['loss_unperturbed']):.4e})")
    assert 0.99e-10 <= float(loss) < 1e-7
    assert torch.isfinite(gm).all() and torch.isfinite(gq).all()


@pytest.mark.gpu
def test_repeatable_and_packing_on_the_fly(cuda):
    cur, ni, fi = _case(1000, 20, 1, cuda)
    a = _gpu_run(cur, ni, fi, cuda)
    b = _gpu_run(cur, ni, fi, cuda)
    # an object with only the reference's fields (int64 (F, k) indices, no packed form)
    bare_ni = SimpleNamespace(indices=ni.indices.clone(), weights=ni.weights.clone())
    bare_fi = SimpleNamespace(inverted_rotations=fi.inverted_rotations.clone(),
                              offsets_to_neighbors=fi.offsets_to_neighbors.clone())
    c = _gpu_run(cur, bare_ni, bare_fi, cuda)
    for other in (b, c):
        for x, y in zip(a, other):
            assert torch.equal(x, y)


@pytest.mark.gpu
def test_gradient_routing(cuda):
    cur, ni, fi = _case(130, 20, 0, cuda)
    loss, gm, gq = _gpu_run(cur, ni, fi, cuda)
    l1, m1, q1 = _gpu_run(cur, ni, fi, cuda, grads=(True, False))
    assert q1 is None and torch.equal(m1, gm) and torch.equal(l1, loss)
    l2, m2, q2 = _gpu_run(cur, ni, fi, cuda, grads=(False, True))
    assert m2 is None and torch.equal(q2, gq) and torch.equal(l2, loss)
    p = {k: v.to(cuda) for k, v in cur.items()}
    out = R.calculate_rigidity_loss(p, ni, fi)
    assert not out.requires_grad and out.grad_fn is None and torch.equal(out.cpu(), loss)
    _, m3, q3 = _gpu_run(cur, ni, fi, cuda, scale=3.0)
    torch.testing.assert_close(m3, 3 * gm, rtol=1e-6, atol=0)
    torch.testing.assert_close(q3, 3 * gq, rtol=1e-6, atol=0)


@pytest.mark.gpu
def test_errors(cuda):
    prev, _ = _cloud(30, torch.arange(30) < 20, seed=1)
    pg = {n: v.to(cuda) for n, v in prev.items()}
    with pytest.raises(ValueError):
        R.create_neighbor_info(pg, 20)  # F = 20 <= k
    ni = R.create_neighbor_info(pg, 5)
    fi = R.create_foreground_info(pg, ni.indices)
    bad = ni.indices.clone()
    bad[3, 2] = 20  # == F
    with pytest.raises(ValueError, match="outside"):
        R.calculate_rigidity_loss(pg, SimpleNamespace(indices=bad, weights=ni.weights), fi)
    with pytest.raises(ValueError, match="outside"):
        R.create_foreground_info(pg, bad)
    with pytest.raises(ValueError):
        R.calculate_rigidity_loss(pg, SimpleNamespace(indices=ni.indices, weights=ni.weights[:, :4]), fi)
    with pytest.raises(ValueError):
        R.calculate_rigidity_loss(pg, SimpleNamespace(indices=ni.indices[:19], weights=ni.weights[:19]), fi)
    short = SimpleNamespace(inverted_rotations=fi.inverted_rotations, offsets_to_neighbors=fi.offsets_to_neighbors[:, :4])
    with pytest.raises(ValueError):
        R.calculate_rigidity_loss(pg, ni, short)
    fewer = {n: v[:25] for n, v in pg.items()}
    with pytest.raises(ValueError):
        R.calculate_rigidity_loss(fewer, ni, fi)


# ---- GPU: the training step's loss ----------------------------------------------------------------
@pytest.mark.gpu
def test_train_step_loss(cuda):
    import splat_loss
    import splat_scenes as S
    import splat_train
    from diff_gaussian_rasterization import GaussianRasterizer

    P, W, H, k = 2000, 64, 48, 20
    base = S.synthetic_cloud(P, 0.05, seed=4, device="cpu")
    g = torch.Generator().manual_seed(5)
    m = (torch.rand(P, generator=g) < 0.6).float()
    base["segmentation_masks"] = torch.stack((m, torch.zeros(P), 1 - m), 1)
    base["rotation_quaternions"] = base["rotation_quaternions"] * (0.5 + torch.rand(P, 1, generator=g))
    prev = {n: v.to(cuda) for n, v in base.items()}
    rows = (m > 0.5).nonzero().squeeze(1).to(cuda)
    idx, d2 = R.knn(prev["means"][rows], k)
    ni = R.NeighborInfo(indices=idx, weights=torch.exp(-20 * d2).float())  # a cloud this sparse: softer weights
    fi = R.create_foreground_info(prev, ni.indices)
    cur = _perturbed(base, g, 0.03, 0.5)
    views = [splat_train.View(camera_index=c, render_settings=S.render_settings(
                 W, H, S.intrinsics(48.0, W, H), S.look_at(yaw, 0.1, 4.0), device=cuda),
                 image=torch.rand(3, H, W, generator=g).to(cuda), segmentation_mask=None)
             for c, yaw in enumerate((10.0, 200.0))]
    leaves = ("means", "rotation_quaternions", "opacity_logits", "log_scales", "colors")

    pa = {n: v.detach().to(cuda).requires_grad_(n in leaves) for n, v in cur.items()}
    total, l1, ss, rig = splat_train.train_step_loss(pa, views, ni, fi)
    total.backward()

    pb = {n: v.detach().to(cuda).requires_grad_(n in leaves) for n, v in cur.items()}
    l1b = ssb = 0
    for v in views:
        img, _, _ = GaussianRasterizer(raster_settings=v.render_settings)(**S.render_arguments(pb))
        a, b = splat_loss.l1_and_ssim_loss(img, v.image)
        l1b, ssb = l1b + a, ssb + b
    rigb = len(views) * RR.rigidity_loss(pb["means"], pb["rotation_quaternions"], m.to(cuda) > 0.5, ni.indices,
                                         ni.weights, fi.inverted_rotations, fi.offsets_to_neighbors).float()
    totalb = 0.8 * l1b + 0.2 * ssb + 3 * rigb
    totalb.backward()
    _rel("total", total.detach(), totalb.detach(), 1e-5)
    _rel("l1", l1.detach(), l1b.detach(), 1e-5)
    _rel("ssim", ss.detach(), ssb.detach(), 1e-5)
    _rel("rigidity", rig.detach(), rigb.detach(), 1e-5)
    assert float(rig) > 1e-3 * float(total)  # the rigidity term takes part
    for n in leaves:
        _band("grad " + n, pa[n].grad.cpu().numpy(), pb[n].grad.cpu().numpy(), 1e-4, 1e-6)
