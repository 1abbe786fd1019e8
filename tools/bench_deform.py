"""A/B timing of the fused deformation input layer against the same layer written with torch ops.
Writes one JSON file (default profiles/deform_in_ab.json).

    python tools/bench_deform.py                 # P = 1M, H = 64 and 128

Per hidden dimension: P synthetic Gaussians (splat_scenes.synthetic_cloud), the previous cloud the
initial one plus 0.01 N(0, 1) on the means and 0.05 N(0, 1) on the raw quaternions.  One step of the
torch composition is what train.py does per timestep: encode the previous cloud
(normalize_and_encode_means_and_rotations with PositionalEncoding's own ops), repeat the progress
encoding over the rows, cat both with the initial encoding (kept from before the loop, as in train.py)
into the (P, 192) matrix, F.linear, and autograd's backward for weight and bias.  The fused step is
splat_deform.deform_input_layer forward + backward, its range reductions included.  Both alternate in
one process; every repetition ends in a device synchronise and is timed on the host around it.  Peak
allocated memory is torch's, over one step, above what is allocated before it.
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
import splat_scenes as S  # noqa: E402


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1],
            "p10_ms": s[len(s) // 10], "p90_ms": s[min(len(s) - 1, (9 * len(s)) // 10)], "reps": len(s)}


def _peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


# ---- train.py:113-127 / 185-204 with its own ops ----
def _positional_encoding(x, frequency_count):
    factors = ((torch.ones(frequency_count) * 2).pow(torch.arange(frequency_count)) * torch.pi).to(x.device)
    emb = (factors * x[:, :, None]).repeat_interleave(2, 2)
    emb[:, :, ::2] = torch.sin(emb[:, :, ::2])
    emb[:, :, 1::2] = torch.cos(emb[:, :, ::2])
    return emb.permute(0, 2, 1).flatten(start_dim=1)


def _normalize_and_encode(params):
    means, rotations = params["means"], params["rotation_quaternions"]
    nm = means - means.min(dim=0).values
    nm = (2.0 * nm / nm.max(dim=0).values) - 1.0
    nr = rotations - rotations.min(dim=0).values
    nr = (2.0 * nr / nr.max(dim=0).values) - 1.0
    return torch.cat((_positional_encoding(nm, 10), _positional_encoding(nr, 4)), dim=1)


def leg(P, H, reps, warmup):
    dev = torch.device("cuda:0")
    cloud = S.synthetic_cloud(P, 0.01, seed=0, device=dev)
    g = torch.Generator().manual_seed(1)
    initial = {"means": cloud["means"], "rotation_quaternions": cloud["rotation_quaternions"]}
    previous = {"means": initial["means"] + 0.01 * torch.randn(P, 3, generator=g).to(dev),
                "rotation_quaternions": initial["rotation_quaternions"] + 0.05 * torch.randn(P, 4, generator=g).to(dev)}
    fc_in = torch.nn.Linear(192, H).to(dev)
    w, b = fc_in.weight, fc_in.bias
    up = torch.randn(P, H, generator=g).to(dev)
    progress = 3 / 7
    enc_initial = _normalize_and_encode(initial)  # train.py keeps it from before the timestep loop

    def fused():
        w.grad = b.grad = None
        D.deform_input_layer(w, b, initial, previous, progress).backward(up)

    def fused_forward():
        with torch.no_grad():
            D.deform_input_layer(w, b, initial, previous, progress)

    def torch_ops():
        w.grad = b.grad = None
        enc_previous = _normalize_and_encode(previous)
        enc_progress = _positional_encoding(torch.tensor(progress).view(1, 1).repeat(P, 1).to(dev), 4)
        x = torch.cat((enc_initial, enc_previous, enc_progress), dim=1)
        torch.nn.functional.linear(x, w, b).backward(up)

    fused()
    a = (D.deform_input_layer(w, b, initial, previous, progress).detach(), w.grad.clone(), b.grad.clone())
    torch_ops()
    x = torch.cat((enc_initial, _normalize_and_encode(previous),
                   _positional_encoding(torch.tensor(progress).view(1, 1).repeat(P, 1).to(dev), 4)), dim=1)
    ref = (torch.nn.functional.linear(x, w, b).detach(), w.grad.clone(), b.grad.clone())
    del x
    diff = [float((p - q).abs().max() / q.abs().max()) for p, q in zip(a, ref)]
    del a, ref
    for _ in range(warmup):
        fused(), torch_ops(), fused_forward()
    t = {"fused": [], "torch_ops": [], "fused_forward": []}
    for _ in range(reps):  # alternate, so drift of the clocks hits both alike
        t["fused"].append(_timed(fused))
        t["torch_ops"].append(_timed(torch_ops))
        t["fused_forward"].append(_timed(fused_forward))
    out = {"P": P, "H": H, "fused_fwd_bwd": _stats(t["fused"]), "torch_ops_fwd_bwd": _stats(t["torch_ops"]),
           "fused_forward_only": _stats(t["fused_forward"]),
           "fused_peak_bytes": _peak_bytes(fused), "torch_ops_peak_bytes": _peak_bytes(torch_ops),
           "torch_ops_kept_initial_encoding_bytes": enc_initial.numel() * 4,
           "output_max_abs_diff_over_max": diff[0], "grad_weight_max_abs_diff_over_max": diff[1],
           "grad_bias_max_abs_diff_over_max": diff[2],
           "torch_ops_matrix_bytes": P * 192 * 4, "fused_input_bytes": P * 14 * 4,
           "output_bytes": P * H * 4}
    out["speedup_fwd_bwd"] = out["torch_ops_fwd_bwd"]["median_ms"] / out["fused_fwd_bwd"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--H", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "deform_in_ab.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "timing": "host perf_counter around a call that ends in torch.cuda.synchronize(); ms",
           "legs": [leg(a.P, H, a.reps, a.warmup) for H in a.H]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
