"""A/B timing of the fused output head against the two torch lines it replaces.
Writes one JSON file (default profiles/head_ab.json).

    python tools/bench_head.py               # P = 1M, H = 64, 128 and 512

Per hidden dimension: the tail of one ``splat_deform.DeformationNetwork`` (its own ``_fused_head`` rule and
``fc_out`` parameters) on a (P, H) N(0, 1) activation that requires a gradient (inside the network it is the
last block's output), with an N(0, 1) upstream gradient and initial parameters that do not require one, as in
the reference.  The fused leg runs the kernels of csrc/gsr_head.hip; the torch leg is the SAME tail after
``set_fused_output_head(False)``: ``fc_out(x)`` and ``+ torch.cat((means, quaternions), dim=1)`` with
autograd's backward.  Both alternate in one process; every repetition ends in a device synchronise and is
timed on the host around it.  Forward + backward and the forward alone (under no_grad) are timed for both.
Peak allocated memory is torch's, over one forward + backward, above what is allocated before it.
``default_on`` applies the rule that decides the default: the fused median below the torch median and the two
legs' min-max ranges apart.  ``forward_hbm_floor_ms`` is the time of the forward's compulsory bytes,
P (4 H + 56) from the shapes (not measured traffic), at ``--hbm-tbs`` TB/s.  ``device_ms`` holds times
without the host's dispatch cost: the library's event pairs around the head's launches and a torch event
pair around each leg's forward.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "animating-gaussian-splats_amd")]
import torch  # noqa: E402

import splat_deform as D  # noqa: E402
from diff_gaussian_rasterization import _C  # noqa: E402


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def _peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _device_times(legs, reps):
    """Device-side times, free of the host's dispatch cost: the library's event pairs around the head's own
    launches (mean over ``reps`` calls), and a torch event pair around each leg's forward-only call (median)."""
    res = {}
    _C.profile_enable(True)
    try:
        for phase, leg_name in (("deform_out_fwd", "fused_forward_only"), ("deform_out_bwd", "fused_fwd_bwd")):
            _C.profile_select([phase])
            _C.profile_reset()
            for _ in range(reps):
                legs[leg_name]()
            torch.cuda.synchronize()
            total, count = _C.profile_read(phase)
            res[f"{phase}_kernels_mean"] = total / max(count, 1)
    finally:
        _C.profile_select(None)
        _C.profile_reset()
        _C.profile_enable(False)
    for name in ("fused_forward_only", "torch_ops_forward_only"):
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            legs[name]()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        res[f"{name}_events_median"] = statistics.median(ms)
    return res


def _tail(net, x, initial):
    """DeformationNetwork.forward from the last block's output on."""
    if net._fused_head(x):
        return D.deform_output_layer(x, net.fc_out.weight, net.fc_out.bias, initial)
    return net.fc_out(x) + torch.cat((initial["means"], initial["rotation_quaternions"]), dim=1)


def leg(P, H, reps, warmup, hbm_tbs):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(H)
    net = D.DeformationNetwork(H, 0).to(dev).train()
    x = torch.randn(P, H, generator=g).to(dev).requires_grad_(True)
    up = torch.randn(P, 7, generator=g).to(dev)
    initial = {"means": ((torch.rand(P, 3, generator=g) - 0.5) * 3.0).to(dev),
               "rotation_quaternions": torch.randn(P, 4, generator=g).to(dev)}
    params = [x, net.fc_out.weight, net.fc_out.bias]

    def switched(fused, fn):
        def run():
            previous = D.set_fused_output_head(fused)
            try:
                return fn()
            finally:
                D.set_fused_output_head(previous)
        return run

    def step():
        for p in params:
            p.grad = None
        out = _tail(net, x, initial)
        out.backward(up)
        return type(out.grad_fn).__name__

    def forward():
        with torch.no_grad():
            return _tail(net, x, initial)

    diffs, nodes = {}, {}
    outs = [switched(f, forward)() for f in (True, False)]
    diffs["output"] = _rel(*outs)
    del outs
    grads = []
    for f in (True, False):
        nodes["fused" if f else "torch_ops"] = switched(f, step)()
        grads.append([p.grad.clone() for p in params])
    for n, a, b in zip(("dx", "dW", "db"), *grads):
        diffs[n] = _rel(a, b)
    del grads
    if nodes["fused"] != "_DeformOutBackward" or not nodes["torch_ops"].startswith("AddBackward"):
        raise RuntimeError(f"the legs ran {nodes}: the switch did not select them")

    legs = {"fused_fwd_bwd": switched(True, step), "torch_ops_fwd_bwd": switched(False, step),
            "fused_forward_only": switched(True, forward), "torch_ops_forward_only": switched(False, forward)}
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    t = {k: [] for k in legs}
    for _ in range(reps):  # alternate, so drift of the clocks hits both alike
        for k, fn in legs.items():
            t[k].append(_timed(fn))
    out = {"P": P, "H": H, "autograd_nodes": nodes, **{k: _stats(v) for k, v in t.items()}}
    out["device_ms"] = _device_times(legs, reps)
    for name, fused in (("fused_peak_bytes", True), ("torch_ops_peak_bytes", False)):
        for p in params:
            p.grad = None
        out[name] = _peak_bytes(switched(fused, step))
    out["tensor_bytes"] = P * H * 4
    out["max_abs_diff_over_max"] = diffs
    f, o = out["fused_fwd_bwd"], out["torch_ops_fwd_bwd"]
    ff, fo = out["fused_forward_only"], out["torch_ops_forward_only"]
    out["speedup_fwd_bwd"] = o["median_ms"] / f["median_ms"]
    out["speedup_forward_only"] = fo["median_ms"] / ff["median_ms"]
    out["default_on"] = bool(f["median_ms"] < o["median_ms"] and f["max_ms"] < o["min_ms"])
    out["forward_only_wins"] = bool(ff["median_ms"] < fo["median_ms"] and ff["max_ms"] < fo["min_ms"])
    out["peak_lower"] = bool(out["fused_peak_bytes"] < out["torch_ops_peak_bytes"])
    out["forward_bytes_from_shapes"] = P * (4 * H + 56)
    out["backward_bytes_from_shapes"] = P * (8 * H + 28)
    out["forward_hbm_floor_ms"] = out["forward_bytes_from_shapes"] / (hbm_tbs * 1e12) * 1e3
    out["forward_over_hbm_floor"] = ff["median_ms"] / out["forward_hbm_floor_ms"]
    out["forward_kernel_over_hbm_floor"] = out["device_ms"]["deform_out_fwd_kernels_mean"] / out["forward_hbm_floor_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--H", type=int, nargs="+", default=[64, 128, 512])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=6.29, help="achievable HBM bandwidth the floor is taken at (TB/s)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "head_ab.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "timing": "host perf_counter around a call that ends in torch.cuda.synchronize(); ms",
           "hbm_tbs": a.hbm_tbs,
           "legs": [leg(a.P, H, a.reps, a.warmup, a.hbm_tbs) for H in a.H]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
