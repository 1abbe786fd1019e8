"""Densification with Adam state surgery.

CPU: the numpy oracle (oracle/densify_oracle.py) reproduces the reference's densify_gaussians
(external.py:211-314, run by tests/golden/gen_golden.py on seeded data with a populated torch Adam)
at i = 500 / 3000 / 5000: every parameter row, Adam moment and statistic bit-exact, except the split
copies' means (R q * sample: matrix-product rounding, <= 1e-6 absolute) and log-scales (exp / log
rounding, <= 1e-6 absolute).  GPU (-m gpu): splat_densify through the C ABI against the same golden
outputs (fed the reference's recorded torch.normal draw), against the oracle on a 200k-Gaussian
random cloud, and the statistics kernels against the reference's densify statistics sequence.

Block edges and the scan's carry: k_dens_flags counts per 1024-row block, k_dens_scan turns the block counts
into offsets in sweeps of 1024 blocks with a carry between sweeps.  P in {1, 1023, 1024, 1025, 2049} puts rows
of every output category on both sides of each block boundary; an all-pruned and an all-split call reach
P_out = 0 and n_keep_orig = 0; P = 1024 * 1024 + 1025 puts blocks 1024 and 1025 in the second sweep, checked
against a closed form (row index in means[:, 0], fate from a hash of the index, every input a factor 5 from its
threshold).  CPU tests restate the two mistakes these exist to catch (block offsets ignored, the carry
dropped) on that closed form and assert the output bits change.
"""
import os

import numpy as np
import pytest
import torch

from oracle import densify_oracle as DO

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_harness.npz"))
SPLIT_TOL = 1e-6
LR = {"means": 0.00016, "colors": 0.0025, "segmentation_masks": 0.0, "rotation_quaternions": 0.001,
      "opacity_logits": 0.05, "log_scales": 0.001, "camera_matrices": 1e-4, "camera_center": 1e-4}


def _case(c):
    pre = f"dens{c}_pre_"
    keys = [k[len(pre):] for k in GOLD.files if k.startswith(pre) and not k.startswith(pre + "m_")
            and not k.startswith(pre + "v_")]
    g = {k: GOLD[pre + k] for k in keys}
    m = {k: GOLD[pre + "m_" + k] for k in keys if k not in DO.GAUSSIAN_EXCLUDED}
    v = {k: GOLD[pre + "v_" + k] for k in keys if k not in DO.GAUSSIAN_EXCLUDED}
    return keys, g, m, v


def _compare(keys, got_p, got_m, got_v, c, n_base):
    """n_base = rows before the split copies (originals + clones kept): the split rows follow."""
    for k in keys:
        ref = GOLD[f"dens{c}_out_{k}"]
        got = np.asarray(got_p[k])
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        if k in ("means", "log_scales"):
            np.testing.assert_array_equal(got[:n_base], ref[:n_base], err_msg=k)
            np.testing.assert_allclose(got[n_base:], ref[n_base:], rtol=0, atol=SPLIT_TOL, err_msg=k)
        else:
            np.testing.assert_array_equal(got, ref, err_msg=k)
        if k in got_m:
            np.testing.assert_array_equal(np.asarray(got_m[k]), GOLD[f"dens{c}_out_m_{k}"], err_msg=k)
            np.testing.assert_array_equal(np.asarray(got_v[k]), GOLD[f"dens{c}_out_v_{k}"], err_msg=k)


@pytest.mark.parametrize("c", range(3))
def test_oracle_matches_reference_densify(c):
    keys, g, m, v = _case(c)
    p2, m2, v2, acc, cnt, mr, info = DO.densify(
        g, m, v, GOLD[f"dens{c}_in_acc"], GOLD[f"dens{c}_in_count"], GOLD[f"dens{c}_in_max_radii"],
        GOLD[f"dens{c}_in_vis"], GOLD[f"dens{c}_in_m2grad"], float(GOLD[f"dens{c}_scene_radius"]),
        int(GOLD[f"dens{c}_iter"]), GOLD[f"dens{c}_samples"])
    assert info["n_clone"] > 0 and info["n_split"] > 0
    _compare(keys, p2, m2, v2, c, _first_split_row(g, c))
    for nm, a in {"acc": acc, "count": cnt, "max_radii": mr}.items():
        np.testing.assert_array_equal(a, GOLD[f"dens{c}_out_{nm}"])


def _first_split_row(g, c):
    """Row index where the split copies begin in the densified arrays (after kept originals and kept
    clones): recomputed from the oracle's own decisions."""
    acc = GOLD[f"dens{c}_in_acc"].copy()
    cnt = GOLD[f"dens{c}_in_count"].copy()
    acc, cnt = DO.accumulate_grads(GOLD[f"dens{c}_in_vis"], GOLD[f"dens{c}_in_m2grad"], acc, cnt)
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = acc / cnt
    avg[np.isnan(avg)] = 0
    i = int(GOLD[f"dens{c}_iter"])
    sr = float(GOLD[f"dens{c}_scene_radius"])
    ms = np.exp(g["log_scales"]).max(1)
    hot = avg >= np.float32(0.0002)
    clone = hot & (ms <= np.float32(0.01 * sr))
    split = hot & (ms > np.float32(0.01 * sr))
    pr = (1 / (1 + np.exp(-g["opacity_logits"][:, 0])) < np.float32(0.25 if i == 5000 else 0.005))
    if i >= 3000:
        pr = pr | (ms > np.float32(0.1 * sr))
    return int((~split & ~pr).sum() + (clone & ~pr).sum())


def test_oracle_statistics_match_reference():
    radii, grads = GOLD["dstat_in_radii"], GOLD["dstat_in_grad"]
    P = radii.shape[1]
    mr, acc, cnt = np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(P, np.float32)
    for r, g in zip(radii, grads):
        mr, vis = DO.update_max_radii(r, mr)
        acc, cnt = DO.accumulate_grads(vis, g, acc, cnt)
    np.testing.assert_array_equal(mr, GOLD["dstat_out_max_radii"])
    np.testing.assert_array_equal(cnt, GOLD["dstat_out_visibility_count"])
    np.testing.assert_allclose(acc, GOLD["dstat_out_grad_accum"], rtol=1e-6)


# ------------------------------------------------------------------------------------------------
def _gpu_setup(cuda, keys, g, m, v, step=2.0):
    params = {k: torch.nn.Parameter(torch.from_numpy(g[k]).to(cuda).contiguous()) for k in keys}
    opt = torch.optim.Adam([{"params": [p], "name": k, "lr": LR.get(k, 1e-3)} for k, p in params.items()],
                           lr=0.0, eps=1e-15)
    for k in m:
        opt.state[params[k]] = {"step": torch.tensor(step), "exp_avg": torch.from_numpy(m[k]).to(cuda),
                                "exp_avg_sq": torch.from_numpy(v[k]).to(cuda)}
    return params, opt


def _dv(cuda, acc, cnt, mr, vis, m2grad):
    from splat_densify import DensificationVariables
    m2 = torch.zeros(len(acc), 3, device=cuda, requires_grad=True)
    m2.grad = torch.from_numpy(m2grad).to(cuda)
    return DensificationVariables(
        visibility_count=torch.from_numpy(cnt).to(cuda).clone(),
        mean_2d_gradients_accumulated=torch.from_numpy(acc).to(cuda).clone(),
        max_2d_radii=torch.from_numpy(mr).to(cuda).clone(),
        gaussian_is_visible_mask=torch.from_numpy(vis).to(cuda), means_2d=m2)


@pytest.mark.gpu
@pytest.mark.parametrize("c", range(3))
def test_gpu_densify_matches_reference(cuda, c):
    import splat_densify
    keys, g, m, v = _case(c)
    params, opt = _gpu_setup(cuda, keys, g, m, v)
    dv = _dv(cuda, GOLD[f"dens{c}_in_acc"], GOLD[f"dens{c}_in_count"], GOLD[f"dens{c}_in_max_radii"],
             GOLD[f"dens{c}_in_vis"], GOLD[f"dens{c}_in_m2grad"])
    samples = torch.from_numpy(GOLD[f"dens{c}_samples"]).to(cuda)
    seen = {}

    def sample_fn(mean, std):
        seen["std"] = std.cpu().numpy()
        assert mean.shape == std.shape == samples.shape
        return samples.clone()

    splat_densify.densify_gaussians(params, dv, float(GOLD[f"dens{c}_scene_radius"]), opt,
                                    int(GOLD[f"dens{c}_iter"]), sample_fn=sample_fn)
    torch.cuda.synchronize()
    got_p = {k: params[k].detach().cpu().numpy() for k in keys}
    got_m = {k: opt.state[params[k]]["exp_avg"].cpu().numpy() for k in m}
    got_v = {k: opt.state[params[k]]["exp_avg_sq"].cpu().numpy() for k in m}
    _compare(keys, got_p, got_m, got_v, c, _first_split_row(g, c))
    for k in m:
        assert float(opt.state[params[k]]["step"]) == float(GOLD[f"dens{c}_out_step_{k}"])
        assert opt.param_groups[[gr["name"] for gr in opt.param_groups].index(k)]["params"][0] is params[k]
    np.testing.assert_array_equal(dv.visibility_count.cpu().numpy(), GOLD[f"dens{c}_out_count"])
    np.testing.assert_array_equal(dv.mean_2d_gradients_accumulated.cpu().numpy(), GOLD[f"dens{c}_out_acc"])
    np.testing.assert_array_equal(dv.max_2d_radii.cpu().numpy(), GOLD[f"dens{c}_out_max_radii"])
    # the std handed to torch.normal is exp(log_scales) of the split rows, twice (external.py:257-259)
    _, _, _, _, _, _, info = DO.densify(g, m, v, GOLD[f"dens{c}_in_acc"], GOLD[f"dens{c}_in_count"],
                                        GOLD[f"dens{c}_in_max_radii"], GOLD[f"dens{c}_in_vis"],
                                        GOLD[f"dens{c}_in_m2grad"], float(GOLD[f"dens{c}_scene_radius"]),
                                        int(GOLD[f"dens{c}_iter"]), GOLD[f"dens{c}_samples"])
    np.testing.assert_allclose(seen["std"], info["stds"], rtol=1e-6, atol=0)


@pytest.mark.gpu
def test_gpu_densify_large_random_vs_oracle(cuda):
    import splat_densify
    rng = np.random.default_rng(5)
    P, sr, it = 200_000, 3.0, 3000
    g = {"means": rng.standard_normal((P, 3), np.float32), "colors": rng.random((P, 3), np.float32),
         "segmentation_masks": rng.random((P, 3), np.float32),
         "rotation_quaternions": rng.standard_normal((P, 4), np.float32),
         "opacity_logits": (3 * rng.standard_normal((P, 1))).astype(np.float32),
         "log_scales": (np.log(0.03) + 0.8 * rng.standard_normal((P, 3))).astype(np.float32),
         "camera_matrices": np.zeros((50, 3), np.float32), "camera_center": np.zeros((50, 3), np.float32)}
    keys = list(g)
    m = {k: rng.standard_normal(g[k].shape).astype(np.float32) * 1e-3 for k in keys if k not in DO.GAUSSIAN_EXCLUDED}
    v = {k: rng.random(g[k].shape, np.float32) * 1e-6 for k in m}
    cnt = rng.integers(0, 6, P).astype(np.float32)
    acc = (cnt * 4e-4 * rng.random(P)).astype(np.float32)
    vis = rng.random(P) > 0.3
    m2g = (3e-4 * rng.standard_normal((P, 3))).astype(np.float32)
    mr = rng.integers(0, 9, P).astype(np.float32)
    params, opt = _gpu_setup(cuda, keys, g, m, v)
    dv = _dv(cuda, acc, cnt, mr, vis, m2g)
    drawn = {}

    def sample_fn(mean, std):
        drawn["s"] = torch.normal(mean=mean, std=std)
        return drawn["s"]

    info = splat_densify.densify_gaussians(params, dv, sr, opt, it, sample_fn=sample_fn)
    assert info["n_split"] > 1000 and info["n_keep_clone"] > 1000
    p2, m2, v2, *_ = DO.densify(g, m, v, acc, cnt, mr, vis, m2g, sr, it, drawn["s"].cpu().numpy())
    n_base = info["n_keep_orig"] + info["n_keep_clone"]
    for k in keys:
        got, ref = params[k].detach().cpu().numpy(), p2[k]
        assert got.shape == ref.shape, k
        if k in ("means", "log_scales"):
            np.testing.assert_array_equal(got[:n_base], ref[:n_base], err_msg=k)
            np.testing.assert_allclose(got[n_base:], ref[n_base:], rtol=0, atol=4e-6, err_msg=k)
        else:
            np.testing.assert_array_equal(got, ref, err_msg=k)
        if k in m2:
            np.testing.assert_array_equal(opt.state[params[k]]["exp_avg"].cpu().numpy(), m2[k])
            np.testing.assert_array_equal(opt.state[params[k]]["exp_avg_sq"].cpu().numpy(), v2[k])


@pytest.mark.gpu
def test_gpu_densify_c3_size_vs_oracle(cuda):
    """BASELINE configs[2]'s densify.py clone / split at its size: the bench's 1M-Gaussian densify
    event (bench.py densify_call_site: densify.py's parameter dict, statistics scaled so ~20 % of the
    seen Gaussians pass the 0.0002 threshold, scene radius at 100 x the median maximum scale, i = 600)
    through the native path against the golden-pinned numpy restatement of external.py:211-314
    (oracle/densify_oracle.py) with the split samples shared: row counts bit-exact, every row and
    Adam moment bit-exact except the split copies' means / log-scales (<= 4e-6 absolute)."""
    import splat_densify
    import splat_scenes as S
    P, it = 1_000_000, 600
    base = S.synthetic_cloud(P, 0.005, seed=0, device="cpu")
    rng = np.random.default_rng(7)
    g = {"means": base["means"].numpy(), "colors": base["colors"].numpy(),
         "segmentation_masks": np.repeat((rng.random((P, 1)) > 0.5).astype(np.float32), 3, 1),
         "rotation_quaternions": base["rotation_quaternions"].numpy(),
         "opacity_logits": base["opacity_logits"].numpy(), "log_scales": base["log_scales"].numpy(),
         "camera_matrices": np.zeros((50, 3), np.float32), "camera_center": np.zeros((50, 3), np.float32)}
    keys = list(g)
    m = {k: (rng.standard_normal(g[k].shape) * 1e-3).astype(np.float32) for k in keys if k not in DO.GAUSSIAN_EXCLUDED}
    v = {k: (rng.random(g[k].shape) * 1e-6).astype(np.float32) for k in m}
    cnt = rng.integers(0, 6, P).astype(np.float32)
    avg = rng.random(P).astype(np.float32) * np.float32(2.5e-4)  # ~20 % of the seen rows >= 0.0002
    acc = (avg * cnt).astype(np.float32)
    vis = rng.random(P) > 0.4
    m2g = (3e-4 * rng.standard_normal((P, 3))).astype(np.float32)
    mr = rng.integers(0, 9, P).astype(np.float32)
    sr = float(100.0 * np.median(np.exp(g["log_scales"]).max(axis=1)))
    params, opt = _gpu_setup(cuda, keys, g, m, v)
    dv = _dv(cuda, acc, cnt, mr, vis, m2g)
    drawn = {}

    def sample_fn(mean, std):
        drawn["s"] = torch.normal(mean=mean, std=std)
        return drawn["s"]

    info = splat_densify.densify_gaussians(params, dv, sr, opt, it, sample_fn=sample_fn)
    torch.cuda.synchronize()
    p2, m2, v2, acc2, cnt2, mr2, oinfo = DO.densify(g, m, v, acc, cnt, mr, vis, m2g, sr, it, drawn["s"].cpu().numpy())
    assert info["n_split"] > 10_000 and info["n_keep_clone"] > 10_000
    assert info["n_split"] == oinfo["n_split"] and oinfo["n_clone"] >= info["n_keep_clone"]
    assert info["P_out"] == p2["means"].shape[0] > P
    n_base = info["n_keep_orig"] + info["n_keep_clone"]
    for k in keys:
        got, ref = params[k].detach().cpu().numpy(), p2[k]
        assert got.shape == ref.shape, k
        if k in ("means", "log_scales"):
            np.testing.assert_array_equal(got[:n_base], ref[:n_base], err_msg=k)
            np.testing.assert_allclose(got[n_base:], ref[n_base:], rtol=0, atol=4e-6, err_msg=k)
        else:
            np.testing.assert_array_equal(got, ref, err_msg=k)
        if k in m2:
            np.testing.assert_array_equal(opt.state[params[k]]["exp_avg"].cpu().numpy(), m2[k])
            np.testing.assert_array_equal(opt.state[params[k]]["exp_avg_sq"].cpu().numpy(), v2[k])
    np.testing.assert_array_equal(dv.visibility_count.cpu().numpy(), cnt2)
    np.testing.assert_array_equal(dv.mean_2d_gradients_accumulated.cpu().numpy(), acc2)
    np.testing.assert_array_equal(dv.max_2d_radii.cpu().numpy(), mr2)


@pytest.mark.gpu
def test_gpu_statistics_match_reference(cuda):
    import splat_densify
    radii, grads = GOLD["dstat_in_radii"], GOLD["dstat_in_grad"]
    P = radii.shape[1]
    dv = splat_densify.DensificationVariables(visibility_count=torch.zeros(P, device=cuda),
                                             mean_2d_gradients_accumulated=torch.zeros(P, device=cuda),
                                             max_2d_radii=torch.zeros(P, device=cuda))
    for r, gr in zip(radii, grads):
        splat_densify.update_max_2d_radii_and_visibility_mask(torch.from_numpy(r).to(cuda), dv)
        m2 = torch.zeros(P, 3, device=cuda, requires_grad=True)
        m2.grad = torch.from_numpy(gr).to(cuda)
        dv.means_2d = m2
        splat_densify.accumulate_mean_2d_gradients(dv)
    np.testing.assert_array_equal(dv.max_2d_radii.cpu().numpy(), GOLD["dstat_out_max_radii"])
    np.testing.assert_array_equal(dv.visibility_count.cpu().numpy(), GOLD["dstat_out_visibility_count"])
    np.testing.assert_allclose(dv.mean_2d_gradients_accumulated.cpu().numpy(), GOLD["dstat_out_grad_accum"],
                               rtol=1e-6)


@pytest.mark.gpu
def test_gpu_densify_off_schedule_and_empty(cuda):
    """i = 550: statistics only; i = 600 with no hot Gaussians: unchanged rows, statistics reset."""
    import splat_densify
    keys, g, m, v = _case(0)
    params, opt = _gpu_setup(cuda, keys, g, m, v)
    P = g["means"].shape[0]
    dv = _dv(cuda, np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(P, np.float32),
             np.ones(P, bool), np.zeros((P, 3), np.float32))
    assert splat_densify.densify_gaussians(params, dv, 2.0, opt, 550) is None
    assert float(dv.visibility_count.sum()) == P
    info = splat_densify.densify_gaussians(params, dv, 2.0, opt, 600)
    assert info["n_split"] == 0 and info["n_keep_clone"] == 0
    pr = 1 / (1 + np.exp(-g["opacity_logits"][:, 0])) < np.float32(0.005)
    np.testing.assert_array_equal(params["colors"].detach().cpu().numpy(), g["colors"][~pr])
    assert float(dv.visibility_count.abs().sum()) == 0 and dv.visibility_count.numel() == int((~pr).sum())


def test_oracle_opacity_reset_only_at_3000():
    """external.py:306-314 sits inside `if i <= 5000:` (external.py:218): the opacity reset fires at
    i = 3000 and never again (i = 6000, 9000, ... leave opacity_logits and its moments alone)."""
    keys, g, m, v = _case(0)
    P = g["means"].shape[0]
    z = np.zeros(P, np.float32)
    for i, resets in ((3000, True), (6000, False), (9000, False), (27000, False)):
        p2, m2, v2, *_ = DO.densify(g, m, v, z, z, z, np.zeros(P, bool), np.zeros((P, 3), np.float32), 2.0, i,
                                    np.zeros((0, 3), np.float32))
        if resets:
            assert np.allclose(1 / (1 + np.exp(-p2["opacity_logits"])), 0.01, atol=1e-6)
            assert not m2["opacity_logits"].any()
        else:
            np.testing.assert_array_equal(p2["opacity_logits"], g["opacity_logits"])
            np.testing.assert_array_equal(m2["opacity_logits"], m["opacity_logits"])
            np.testing.assert_array_equal(v2["opacity_logits"], v["opacity_logits"])


@pytest.mark.gpu
def test_gpu_opacity_reset_only_at_3000(cuda):
    import splat_densify
    keys, g, m, v = _case(0)
    P = g["means"].shape[0]
    for i, resets in ((6000, False), (9000, False), (3000, True)):
        params, opt = _gpu_setup(cuda, keys, g, m, v)
        dv = _dv(cuda, np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(P, np.float32),
                 np.zeros(P, bool), np.zeros((P, 3), np.float32))
        splat_densify.densify_gaussians(params, dv, 2.0, opt, i)
        ol = params["opacity_logits"].detach().cpu().numpy()
        st = opt.state[params["opacity_logits"]]
        if resets:
            assert np.allclose(1 / (1 + np.exp(-ol)), 0.01, atol=1e-6) and not st["exp_avg"].any()
        else:
            np.testing.assert_array_equal(ol, g["opacity_logits"])
            np.testing.assert_array_equal(st["exp_avg"].cpu().numpy(), m["opacity_logits"])


# ---- block edges, empty / doubled outputs, the scan's carry -----------------------------------------
BLOCK = 1024  # kDensBlock of csrc/gsr_densify.hip: rows per block, and block sums per sweep of k_dens_scan
CATEGORIES = ("keep_orig", "keep_clone", "split", "keep_split")


def _decisions(g, acc, cnt, vis, m2g, sr, it):
    """The four output categories of every input row (float32, the oracle's expressions)."""
    acc, cnt = DO.accumulate_grads(vis, m2g, acc, cnt)
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = acc / cnt
    avg[np.isnan(avg)] = 0
    ms = np.exp(g["log_scales"]).max(1)
    hot = avg >= np.float32(0.0002)
    small = np.float32(0.01 * sr)
    clone, split = hot & (ms <= small), hot & (ms > small)
    op = DO._sigmoid(g["opacity_logits"])[:, 0] < np.float32(0.25 if it == 5000 else 0.005)
    ms2 = np.exp(np.log((np.exp(g["log_scales"]) / np.float32(1.6)).astype(np.float32))).max(1)
    big, big2 = (ms > np.float32(0.1 * sr), ms2 > np.float32(0.1 * sr)) if it >= 3000 else (False, False)
    return {"keep_orig": ~split & ~(op | big), "keep_clone": clone & ~(op | big), "split": split,
            "keep_split": split & ~(op | big2)}


def _edge_cloud(P, seed=5, sr=3.0):
    """The random cloud of test_gpu_densify_large_random_vs_oracle at P rows; the two rows on each side of
    every 1024-row boundary are set far from the thresholds: even rows clone and stay (surviving original +
    surviving clone), odd rows split and their copies stay (split + surviving split)."""
    rng = np.random.default_rng(seed + P)
    g = {"means": rng.standard_normal((P, 3), np.float32), "colors": rng.random((P, 3), np.float32),
         "segmentation_masks": rng.random((P, 3), np.float32),
         "rotation_quaternions": rng.standard_normal((P, 4), np.float32),
         "opacity_logits": (3 * rng.standard_normal((P, 1))).astype(np.float32),
         "log_scales": (np.log(0.03) + 0.8 * rng.standard_normal((P, 3))).astype(np.float32),
         "camera_matrices": np.zeros((50, 3), np.float32), "camera_center": np.zeros((50, 3), np.float32)}
    m = {k: rng.standard_normal(g[k].shape).astype(np.float32) * 1e-3 for k in g if k not in DO.GAUSSIAN_EXCLUDED}
    v = {k: rng.random(g[k].shape, np.float32) * 1e-6 for k in m}
    cnt = rng.integers(0, 6, P).astype(np.float32)
    acc = (cnt * 4e-4 * rng.random(P)).astype(np.float32)
    vis = rng.random(P) > 0.3
    m2g = (3e-4 * rng.standard_normal((P, 3))).astype(np.float32)
    mr = rng.integers(0, 9, P).astype(np.float32)
    for b in range(BLOCK, P, BLOCK):
        for r in range(b - 2, min(b + 2, P)):
            cnt[r], acc[r], vis[r] = 2.0, 2 * 8e-4, False
            g["opacity_logits"][r] = 2.0
            g["log_scales"][r] = np.log(0.005 if r % 2 == 0 else 0.1)
    return g, m, v, acc, cnt, mr, vis, m2g, sr


def _assert_categories_on_both_sides(dec, P):
    """All four categories within two rows before and (where the cloud has them) two rows after each boundary;
    a lone last row (P = 1025) is a clone that stays: the two categories one row can carry."""
    for b in range(BLOCK, P, BLOCK):
        for lo, hi in ((b - 2, b), (b, min(b + 2, P))):
            have = [c for c in CATEGORIES if dec[c][lo:hi].any()]
            assert have == (list(CATEGORIES) if hi - lo == 2 else ["keep_orig", "keep_clone"]), (P, b, lo, hi, have)


def _sources(dec, sweep=None):
    """Source row of every output row (surviving originals, surviving clones, first and second surviving
    split copies, each in index order) as the kernels compute it: slot = offset of the row's block + rank in
    the block.  ``sweep``: the mistake restated -- the running offset restarts every ``sweep`` blocks (1: block
    offsets ignored; 1024: k_dens_scan without its carry); rows then overwrite each other."""
    P = dec["split"].shape[0]
    idx = np.arange(P)
    n = {c: int(dec[c].sum()) for c in CATEGORIES}
    out = np.full(n["keep_orig"] + n["keep_clone"] + 2 * n["keep_split"], -1, np.int64)
    bases = {"keep_orig": (0,), "keep_clone": (n["keep_orig"],),
             "keep_split": (n["keep_orig"] + n["keep_clone"], n["keep_orig"] + n["keep_clone"] + n["keep_split"])}
    for c, where in bases.items():
        slot = np.cumsum(dec[c]) - dec[c]
        if sweep is not None:
            first = (idx // (BLOCK * sweep)) * (BLOCK * sweep)  # first row of the row's sweep
            slot = slot - slot[first]
        for base in where:
            out[base + slot[dec[c]]] = idx[dec[c]]
    return out, n


@pytest.mark.parametrize("P", [1, 1023, 1024, 1025, 2049])
def test_block_edge_clouds_and_block_offset_sensitivity(P):
    """The edge clouds hold every category on both sides of each boundary; the closed form of the output order
    reproduces the oracle's rows; ignoring the block offsets changes it wherever a second block exists."""
    g, m, v, acc, cnt, mr, vis, m2g, sr = _edge_cloud(P)
    dec = _decisions(g, acc, cnt, vis, m2g, sr, 3000)
    _assert_categories_on_both_sides(dec, P)
    src, n = _sources(dec)
    S = n["split"]
    p2, m2, *_, info = DO.densify(g, m, v, acc, cnt, mr, vis, m2g, sr, 3000, np.zeros((2 * S, 3), np.float32))
    assert info["n_split"] == S and p2["colors"].shape[0] == src.shape[0]
    np.testing.assert_array_equal(p2["colors"], g["colors"][src])
    np.testing.assert_array_equal(p2["means"], g["means"][src])  # zero samples: the split copies sit on the original
    wrong, _ = _sources(dec, sweep=1)
    assert (wrong != src).any() == (P > BLOCK)
    if P > BLOCK:
        assert (g["colors"][wrong].view(np.int32) != p2["colors"].view(np.int32)).any()


def _oracle_parity(params, opt, keys, info, p2, m2, v2):
    """The comparisons of test_gpu_densify_large_random_vs_oracle."""
    n_base = info["n_keep_orig"] + info["n_keep_clone"]
    for k in keys:
        got, ref = params[k].detach().cpu().numpy(), p2[k]
        assert got.shape == ref.shape, k
        if k in ("means", "log_scales"):
            np.testing.assert_array_equal(got[:n_base], ref[:n_base], err_msg=k)
            np.testing.assert_allclose(got[n_base:], ref[n_base:], rtol=0, atol=4e-6, err_msg=k)
        else:
            np.testing.assert_array_equal(got, ref, err_msg=k)
        if k in m2:
            np.testing.assert_array_equal(opt.state[params[k]]["exp_avg"].cpu().numpy(), m2[k])
            np.testing.assert_array_equal(opt.state[params[k]]["exp_avg_sq"].cpu().numpy(), v2[k])


def _gpu_vs_oracle(cuda, g, m, v, acc, cnt, mr, vis, m2g, sr, it):
    import splat_densify
    keys = list(g)
    params, opt = _gpu_setup(cuda, keys, g, m, v)
    dv = _dv(cuda, acc, cnt, mr, vis, m2g)
    drawn = {}

    def sample_fn(mean, std):
        drawn["s"] = torch.normal(mean=mean, std=std) if std.numel() else torch.zeros_like(std)
        return drawn["s"]

    info = splat_densify.densify_gaussians(params, dv, sr, opt, it, sample_fn=sample_fn)
    torch.cuda.synchronize()
    p2, m2, v2, acc2, cnt2, mr2, oinfo = DO.densify(g, m, v, acc, cnt, mr, vis, m2g, sr, it, drawn["s"].cpu().numpy())
    assert info["n_split"] == oinfo["n_split"] and info["P_out"] == p2["means"].shape[0]
    _oracle_parity(params, opt, keys, info, p2, m2, v2)
    for got, ref in ((dv.visibility_count, cnt2), (dv.mean_2d_gradients_accumulated, acc2), (dv.max_2d_radii, mr2)):
        np.testing.assert_array_equal(got.cpu().numpy(), ref)
    return params, opt, info


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 1023, 1024, 1025, 2049])
def test_gpu_densify_block_edges(cuda, P):
    cloud = _edge_cloud(P)
    g, m, v, acc, cnt, mr, vis, m2g, sr = cloud
    dec = _decisions(g, acc, cnt, vis, m2g, sr, 3000)
    _assert_categories_on_both_sides(dec, P)
    _, _, info = _gpu_vs_oracle(cuda, *cloud, 3000)
    n = {c: int(dec[c].sum()) for c in CATEGORIES}
    assert (info["n_keep_orig"], info["n_keep_clone"], info["n_split"], info["n_keep_split"]) == tuple(
        n[c] for c in CATEGORIES)


def _uniform_cloud(P, hot, large, opaque, seed=3):
    """P rows with per-row booleans: hot (gradient 8e-4 against 2e-4), large (scale 0.1 against 0.03, else
    0.005), opaque (logit 2, else -8: opacity 3e-4 against 0.005)."""
    rng = np.random.default_rng(seed)
    g = {"means": rng.standard_normal((P, 3), np.float32), "colors": rng.random((P, 3), np.float32),
         "rotation_quaternions": rng.standard_normal((P, 4), np.float32),
         "opacity_logits": np.where(opaque, 2.0, -8.0).astype(np.float32)[:, None],
         "log_scales": np.repeat(np.log(np.where(large, 0.1, 0.005)).astype(np.float32)[:, None], 3, 1),
         "camera_matrices": np.zeros((50, 3), np.float32)}
    m = {k: rng.standard_normal(g[k].shape).astype(np.float32) * 1e-3 for k in g if k not in DO.GAUSSIAN_EXCLUDED}
    v = {k: rng.random(g[k].shape, np.float32) * 1e-6 for k in m}
    cnt = np.full(P, 2.0, np.float32)
    acc = np.where(hot, 2 * 8e-4, 2 * 1e-5).astype(np.float32)
    return (g, m, v, acc, cnt, np.ones(P, np.float32), np.zeros(P, bool), np.zeros((P, 3), np.float32), 3.0)


def test_oracle_all_pruned_and_all_split():
    P = 1500
    rows = np.arange(P)
    g, m, v, *rest = _uniform_cloud(P, rows % 2 == 0, np.ones(P, bool), np.zeros(P, bool))
    p2, m2, v2, acc, cnt, mr, info = DO.densify(g, m, v, *rest, 600, np.ones((2 * (P // 2), 3), np.float32))
    assert info["n_split"] == P // 2 and p2["means"].shape == (0, 3) and m2["colors"].shape == (0, 3) and acc.shape == (0,)
    g, m, v, *rest = _uniform_cloud(P, np.ones(P, bool), np.ones(P, bool), np.ones(P, bool))
    p2, m2, v2, acc, cnt, mr, info = DO.densify(g, m, v, *rest, 600, np.zeros((2 * P, 3), np.float32))
    assert info["n_split"] == P and p2["means"].shape == (2 * P, 3) and not m2["means"].any()
    np.testing.assert_array_equal(p2["colors"], np.tile(g["colors"], (2, 1)))


@pytest.mark.gpu
def test_gpu_densify_all_pruned(cuda):
    """Every row transparent; every second one also splits, and its copies are as transparent: P_out = 0 with
    split samples drawn.  Parameters and moments are empty, the statistics have length 0, and the optimizer
    still steps."""
    P = 1500
    cloud = _uniform_cloud(P, np.arange(P) % 2 == 0, np.ones(P, bool), np.zeros(P, bool))
    params, opt, info = _gpu_vs_oracle(cuda, *cloud, 600)
    assert info == {"n_keep_orig": 0, "n_keep_clone": 0, "n_split": P // 2, "n_keep_split": 0, "P_out": 0}
    for grp in opt.param_groups:
        p = grp["params"][0]
        if grp["name"] in DO.GAUSSIAN_EXCLUDED:
            continue
        assert p is params[grp["name"]] and p.shape[0] == 0 and p.requires_grad
        st = opt.state[p]
        assert st["exp_avg"].shape == p.shape == st["exp_avg_sq"].shape and float(st["step"]) == 2.0
        p.grad = torch.zeros_like(p)
    opt.step()
    assert all(float(opt.state[params[k]]["step"]) == 3.0 for k in cloud[1])


@pytest.mark.gpu
def test_gpu_densify_all_split(cuda):
    """Every row splits and both copies stay: no surviving original, no clone, P_out = 2 P."""
    P = 1500
    params, opt, info = _gpu_vs_oracle(cuda, *_uniform_cloud(P, np.ones(P, bool), np.ones(P, bool), np.ones(P, bool)), 600)
    assert info == {"n_keep_orig": 0, "n_keep_clone": 0, "n_split": P, "n_keep_split": P, "P_out": 2 * P}


P_CARRY = BLOCK * BLOCK + 1025  # 1026 blocks: blocks 1024 and 1025 are k_dens_scan's second sweep


def _hashed_cloud(P):
    """Fate of row i from an integer hash of i: 0 stays, 1 clones and stays, 2 splits and its copies stay,
    3 is pruned.  means[:, 0] and the first column of its first moment hold the row index (+ 1)."""
    i = np.arange(P, dtype=np.uint64)
    fate = (((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(13)) % np.uint64(4)
    hot, large, opaque = (fate == 1) | (fate == 2), fate == 2, fate != 3
    means = np.zeros((P, 3), np.float32)
    means[:, 0] = np.arange(P)
    g = {"means": means, "rotation_quaternions": np.tile(np.float32([1, 0, 0, 0]), (P, 1)),
         "opacity_logits": np.where(opaque, 2.0, -8.0).astype(np.float32)[:, None],
         "log_scales": np.repeat(np.log(np.where(large, 0.2, 0.005)).astype(np.float32)[:, None], 3, 1)}
    m = {k: np.zeros_like(a) for k, a in g.items()}
    m["means"][:, 0] = np.arange(P) + 1
    v = {k: np.zeros_like(a) for k, a in g.items()}
    cnt = np.ones(P, np.float32)
    acc = np.where(hot, 1e-3, 4e-5).astype(np.float32)
    dec = {"keep_orig": (fate == 0) | (fate == 1), "keep_clone": fate == 1, "split": fate == 2, "keep_split": fate == 2}
    return g, m, v, acc, cnt, dec


def _assert_far_from_thresholds(g, acc, cnt, sr):
    """Every decision input a factor >= 5 from its threshold: no decision depends on an expf ulp.  At i = 600
    nothing is pruned for its size, so the split copies (same opacity, scale / 1.6) face the opacity test only."""
    def far(x, t):
        return bool(((x >= 5 * t) | (x <= t / 5)).all())
    scale = np.exp(g["log_scales"].astype(np.float64))
    opacity = 1 / (1 + np.exp(-g["opacity_logits"].astype(np.float64)))
    assert far(acc.astype(np.float64) / cnt, 0.0002) and far(scale, 0.01 * sr) and far(opacity, 0.005)


def test_closed_form_is_the_oracle_and_needs_the_carry():
    """On a cloud small enough for the oracle the closed form reproduces it bit for bit; at the full size,
    offsets without k_dens_scan's carry change the means column and the moment column."""
    P = 3 * BLOCK + 7
    g, m, v, acc, cnt, dec = _hashed_cloud(P)
    _assert_far_from_thresholds(g, acc, cnt, 3.0)
    z = np.zeros(P, np.float32)
    d = _decisions(g, acc, cnt, np.zeros(P, bool), np.zeros((P, 3), np.float32), 3.0, 600)
    assert all(np.array_equal(d[c], dec[c]) for c in CATEGORIES) and all(dec[c].sum() > P // 8 for c in CATEGORIES)
    src, n = _sources(dec)
    p2, m2, *_ = DO.densify(g, m, v, acc, cnt, z, np.zeros(P, bool), np.zeros((P, 3), np.float32), 3.0, 600,
                            np.zeros((2 * n["split"], 3), np.float32))
    np.testing.assert_array_equal(p2["means"][:, 0], src.astype(np.float32))
    expect_m = np.where(np.arange(src.shape[0]) < n["keep_orig"], src + 1, 0).astype(np.float32)
    np.testing.assert_array_equal(m2["means"][:, 0], expect_m)
    # the full size: only the index lists are needed
    g, m, v, acc, cnt, dec = _hashed_cloud(P_CARRY)
    src, n = _sources(dec)
    assert (src >= 0).all() and (np.diff(src[:n["keep_orig"]]) > 0).all()
    wrong, _ = _sources(dec, sweep=BLOCK)
    changed = wrong != src
    assert changed.any()
    assert (wrong.astype(np.float32).view(np.int32) != src.astype(np.float32).view(np.int32)).any()
    assert all((dec[c][BLOCK * BLOCK:]).any() for c in CATEGORIES)  # the second sweep's blocks hold every category


@pytest.mark.gpu
def test_gpu_densify_scan_carry(cuda):
    """P = 1024 * 1024 + 1025: counts, the means column and one Adam moment column against the closed form, bitwise."""
    import splat_densify
    P, sr = P_CARRY, 3.0
    g, m, v, acc, cnt, dec = _hashed_cloud(P)
    _assert_far_from_thresholds(g, acc, cnt, sr)
    src, n = _sources(dec)
    keys = list(g)
    params, opt = _gpu_setup(cuda, keys, g, m, v)
    dv = _dv(cuda, acc, cnt, np.zeros(P, np.float32), np.zeros(P, bool), np.zeros((P, 3), np.float32))
    info = splat_densify.densify_gaussians(params, dv, sr, opt, 600, sample_fn=lambda mean, std: torch.zeros_like(std))
    torch.cuda.synchronize()
    assert info == {"n_keep_orig": n["keep_orig"], "n_keep_clone": n["keep_clone"], "n_split": n["split"],
                    "n_keep_split": n["keep_split"], "P_out": src.shape[0]}
    got = params["means"].detach()[:, 0].cpu().numpy()
    np.testing.assert_array_equal(got.view(np.int32), src.astype(np.float32).view(np.int32))
    expect_m = np.where(np.arange(src.shape[0]) < n["keep_orig"], src + 1, 0).astype(np.float32)
    got_m = opt.state[params["means"]]["exp_avg"][:, 0].cpu().numpy()
    np.testing.assert_array_equal(got_m.view(np.int32), expect_m.view(np.int32))
    assert dv.visibility_count.shape == (src.shape[0],)
