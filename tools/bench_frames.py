"""A/B timing of the frame export of one inference timestep: the reference's per-camera host
composition against frames_to_uint8 + one 8-bit copy, each with and without PNG writing.
Writes one JSON file (default profiles/frames_ab.json).

    python tools/bench_frames.py                 # 5 cameras at 1280 x 720

The images are one synthetic render: splat_scenes.synthetic_cloud seen by the five inference cameras
(splat_scenes.inference_cameras), rendered once before the timing and kept on the GPU as five
separately allocated (3, 720, 1280) float tensors, which is what a timestep's renders leave behind.
One step is what train.py does with them per timestep (train.py:534-546, 587-596):

* reference: per camera ``image.cpu().numpy()``, clip, scale by 255, cast, transpose -- and, with
  PNGs, the file written on that same thread before the next camera (PIL here where the reference
  calls imageio.imwrite, which writes PNGs through PIL as well);
* native: one ``frames_to_uint8`` over the five images and one 8-bit copy to the host -- and, with
  PNGs, ``FrameWriter.submit``, which hands copy and encoding to its side stream and thread pool.

Both alternate in one process; a step without PNGs ends when its frames are on the host, a step
with PNGs when its files are written (reference) or when submit returns (native: the pipeline's
steady-state rate, the ring blocks it when the encoders fall behind), and the native run's total
includes draining the writer at the end.  Times are host perf_counter; the kernel's device time is
libgsr's own event timing of the ``frames_pack`` phase; host bytes copied are counted from shapes.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from pathlib import Path

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "animating-gaussian-splats_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import splat_export as E  # noqa: E402
import splat_scenes as S  # noqa: E402
from diff_gaussian_rasterization import GaussianRasterizer, _C  # noqa: E402


def _stats(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1],
            "p10_ms": s[len(s) // 10], "p90_ms": s[min(len(s) - 1, (9 * len(s)) // 10)], "reps": len(s)}


def _timed(fn, *a):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(*a)
    return (time.perf_counter() - t0) * 1e3


def _reference_frame(image):  # train.py:534-545
    return (255 * np.clip(image.cpu().numpy(), 0, 1)).astype(np.uint8).transpose(1, 2, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "frames_ab.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    W, H = S.INFERENCE_W, S.INFERENCE_H
    params = S.synthetic_cloud(a.P, 0.01, seed=0, device=dev)
    names = list(S.inference_rig())
    with torch.no_grad():
        images = [GaussianRasterizer(raster_settings=rs)(**S.render_arguments(params))[0].clone()
                  for rs in S.inference_cameras(device=dev)]
    F = len(images)
    root = Path(tempfile.mkdtemp(prefix="gsr_frames_"))
    step = [0]

    def paths(leg):
        step[0] += 1
        return [root / leg / n / f"{step[0]:06d}.png" for n in names]

    def reference(png):
        for image, path in zip(images, paths("reference") if png else [None] * F):
            frame = _reference_frame(image)
            if path is not None:
                path.parent.mkdir(parents=True, exist_ok=True)
                Image.fromarray(frame).save(path, format="PNG")

    def native():
        return E.frames_to_uint8(images).cpu().numpy()

    try:
        same = all(np.array_equal(_reference_frame(im), fr) for im, fr in zip(images, native()))
        writer = E.FrameWriter()
        for _ in range(a.warmup):
            reference(False), reference(True), native()
            writer.submit(E.frames_to_uint8(images), paths("native")).result()
        t = {"reference": [], "reference_png": [], "native": [], "native_png_submit": []}
        drain = 0.0
        for _ in range(a.reps):  # alternate, so drift of the clocks hits all alike
            t["reference"].append(_timed(reference, False))
            t["reference_png"].append(_timed(reference, True))
            t["native"].append(_timed(native))
        # the pipelined leg in a run of its own: its encoders would otherwise work through the others' steps
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            t1 = time.perf_counter()
            writer.submit(E.frames_to_uint8(images), paths("native"))
            t["native_png_submit"].append((time.perf_counter() - t1) * 1e3)
        writer.close()
        total = (time.perf_counter() - t0) * 1e3
        drain = total - sum(t["native_png_submit"])
        workers = min(F, 8)

        # the same pipeline fed by the reference's host composition (submit_host): what the writer
        # alone is worth without the kernel
        with E.FrameWriter() as w2:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                w2.submit_host(np.stack([_reference_frame(im) for im in images]), paths("reference_writer"))
        total_host = (time.perf_counter() - t0) * 1e3

        E.frames_to_uint8(images)
        _C.profile_reset(); _C.profile_select(["frames_pack"]); _C.profile_enable(True)
        for _ in range(a.reps):
            E.frames_to_uint8(images)
        _C.profile_enable(False)
        tot, n = _C.profile_read("frames_pack")
        _C.profile_select(None)
        files = sum(len(list((root / leg / nm).glob("*.png"))) for leg in ("reference", "native") for nm in names)
    finally:
        shutil.rmtree(root, ignore_errors=True)

    per_step_kernel = tot / max(n, 1) * F
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "workload": f"{F} cameras at {W}x{H}, one render of {a.P} synthetic Gaussians; one step = one timestep's frames",
           "timing": "host perf_counter, ms per timestep; steps without PNGs end with the frames on the host",
           "frames_bitwise_equal_to_reference_ops": bool(same),
           "reference": _stats(t["reference"]), "reference_png": _stats(t["reference_png"]),
           "native": _stats(t["native"]),
           "native_png": {"submit": _stats(t["native_png_submit"]), "drain_ms_at_close": drain,
                          "total_ms_per_timestep": total / a.reps, "writer_depth": 2, "writer_workers": workers},
           "reference_composition_through_writer": {"total_ms_per_timestep": total_host / a.reps},
           "frames_pack_kernel": {"launches_per_timestep": F, "device_ms_per_launch": tot / max(n, 1),
                                  "device_ms_per_timestep": per_step_kernel,
                                  "GBps": 15 * H * W * F / (per_step_kernel * 1e-3) / 1e9 if per_step_kernel else None},
           "host_bytes_copied_per_timestep": {"reference": 12 * H * W * F, "native": 3 * H * W * F},
           "png_files_written": files}
    res["speedup_no_png"] = res["reference"]["median_ms"] / res["native"]["median_ms"]
    res["speedup_png"] = res["reference_png"]["median_ms"] / res["native_png"]["total_ms_per_timestep"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
