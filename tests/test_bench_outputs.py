"""bench.py's plain run and ``--dump-outputs``.

CPU: ``bench.dump_outputs`` writes float32 arrays, keeps an array within its share of the byte budget
whole and samples a larger one at indices that depend only on its position, so two runs sample the
same elements.

GPU (-m gpu): one plain run of the small C2 workload (100k Gaussians, 4 cameras of 800x800) in a
fresh process with ``--dump-outputs``: the result line carries the headline keys and none of the
``--full`` legs, ``--steps`` is the number of timed steps, and the dumped images and gradients of the
last timed step equal the same 4 views rendered in this process through the same ``RenderStep`` --
within 1e-5 relative + 1e-6 x max per array, the bound tests/test_dp_gpu.py derives for two
evaluations of one step whose fp32 sums may group differently (here both group alike).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
import splat_scenes as S
import splat_step

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_samples_reproducibly(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 3 * 4 * 1000)  # 3 arrays -> 1000 elements each
    g = torch.Generator().manual_seed(0)
    arrays = {"small": torch.rand(10, 7, generator=g), "big": torch.rand(50, 999, generator=g),
              "wide": torch.rand(3001, generator=g).double()}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in arrays}
    for k in arrays:
        assert got[k].dtype == np.float32
        assert np.array_equal(got[k], np.load(tmp_path / "b" / f"{k}.npy"))
    assert np.array_equal(got["small"], arrays["small"].numpy())  # within its share: whole, shape kept
    assert got["big"].shape == (1000,) and got["wide"].shape == (1000,)
    flat = arrays["big"].reshape(-1).numpy()
    idx = np.sort(np.random.default_rng(1).integers(0, flat.size, size=1000))  # "big" is array 1
    assert np.array_equal(got["big"], flat[idx])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 3 * 4 * 1000 + 3 * 128


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(cuda, tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, "-u", os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", "C2", "--steps", "3",
           "--warmup", "1", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and len(line["step_ms_quartiles"]) == 3
    assert line["unit"] == "Msplats/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] > 0 and line["ms_per_step"] > 0 and "800x800" in line["metric"]
    assert line["full"] is False
    for k in ("roofline", "cpu_baseline", "phase_ms_per_launch", "c2", "call_site"):
        assert k not in line

    # the same step here: C2's leaves, its 4 cameras, one thread over 3 streams, a fresh means2D per render
    cfg = S.CONFIGS["C2"]
    p = S.synthetic_cloud(cfg.P, cfg.s0, sh_degree=cfg.sh_degree, seed=0, device=cuda)
    with torch.no_grad():
        act = S.activated_inputs(p, cfg.sh_degree)
    if cfg.sh_degree >= 0:
        act.pop("colors_precomp")
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in act.items()}
    cams = S.scene_cameras(cfg, device=cuda)
    cur = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in range(3)]
    for s in streams:
        s.wait_stream(cur)
    step = splat_step.RenderStep(cuda, cams, lambda ci: dict(leaves, means2D=torch.zeros_like(leaves["means3D"],
                                                                                          requires_grad=True)),
                                 S.upstream_grad(cfg.height, cfg.width, device=cuda), streams, threads=False)
    try:
        imgs = step(list(range(len(cams))))  # views_of(it) at C2, one rank: all 4 cameras, in order
    finally:
        step.close()
    torch.cuda.synchronize()
    arrays = {f"image_{k}": img for k, img in enumerate(imgs)}
    arrays.update({f"grad_{k}": v.grad for k, v in leaves.items() if v.grad is not None})
    ref_dir = tmp_path / "ref"
    bench.dump_outputs(str(ref_dir), arrays)

    names = sorted(os.listdir(out))
    assert names == sorted(f"{k}.npy" for k in arrays) and len(imgs) == 4
    assert sum(os.path.getsize(out / n) for n in names) <= 64 << 20
    for n in names:
        got, ref = np.load(out / n), np.load(ref_dir / n).astype(np.float64)
        assert got.dtype == np.float32 and got.shape == ref.shape and np.isfinite(got).all()
        assert np.abs(ref).max() > 0, n
        err = np.abs(got - ref)
        bad = err > 1e-5 * np.abs(ref) + 1e-6 * np.abs(ref).max()
        assert not bad.any(), f"{n}: {bad.sum()} of {ref.size} off, worst {err.max():.3g} (max |ref| {np.abs(ref).max():.3g})"
