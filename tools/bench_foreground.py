"""A/B timing of the rigidity term's per-timestep state: ``create_foreground_info`` (torch ops, two host
synchronisations) against ``foreground_info`` (one kernel), and the loss forward without and with the
state as a side output.  Writes one JSON file (default profiles/foreground_ab.json).

    python tools/bench_foreground.py                    # P = 1M, ~60 % foreground, k = 20

The cloud and the neighbour lists are those of tools/bench_rigidity.py's rigidity leg; the current state is
the previous one plus 0.003 N(0, 1) on the means and 0.05 N(0, 1) on the raw quaternions.  The four legs
alternate in one process; every repetition ends in a device synchronise and is timed on the host around
it.  The measuring process is a child of this one and runs under ``--timeout`` seconds: a hung kernel ends
the measurement instead of holding the device.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def _peak(torch, fn):
    """Peak allocated bytes of ``fn`` above what was allocated before it (its result is released first)."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def measure(P, k, reps, warmup):
    sys.path[:0] = [os.path.join(REPO, "animating-gaussian-splats_amd")]
    import torch

    import splat_rigidity as R
    import splat_scenes as S

    dev = torch.device("cuda:0")
    prev = S.synthetic_cloud(P, 0.01, seed=0, device=dev)
    g = torch.Generator().manual_seed(1)
    m = (torch.rand(P, generator=g) < 0.6).float()
    prev["segmentation_masks"] = torch.stack((m, torch.zeros(P), 1 - m), 1).to(dev)
    ni = R.create_neighbor_info(prev, k)
    F = ni.indices.shape[0]
    fi = R.foreground_info(prev, ni)
    cur = dict(prev, means=prev["means"] + 0.003 * torch.randn(P, 3, generator=g).to(dev),
               rotation_quaternions=prev["rotation_quaternions"] + 0.05 * torch.randn(P, 4, generator=g).to(dev))

    legs = {
        "create_foreground_info": lambda: R.create_foreground_info(cur, ni.indices),
        "foreground_info": lambda: R.foreground_info(cur, ni),
        "rigidity_forward": lambda: R.calculate_rigidity_loss(cur, ni, fi),
        "rigidity_forward_and_state": lambda: R.calculate_rigidity_loss_and_state(cur, ni, fi),
    }
    # the same state from the three routes, at the size that is timed
    old, new = legs["create_foreground_info"](), legs["foreground_info"]()
    loss_s, side = legs["rigidity_forward_and_state"]()
    loss = legs["rigidity_forward"]()
    same = {"offsets_bit_equal_to_torch_ops": bool(torch.equal(old.offsets_to_neighbors, new.offsets_to_neighbors)),
            "inverted_rotations_max_abs_diff_to_torch_ops":
                float((old.inverted_rotations - new.inverted_rotations).abs().max()),
            "side_output_bit_equal_to_kernel": bool(torch.equal(side.packed_offsets, new.packed_offsets) and
                                                    torch.equal(side.inverted_rotations, new.inverted_rotations)),
            "loss_bit_equal": bool(torch.equal(loss, loss_s)), "loss": float(loss)}
    del old, new, side
    with torch.no_grad():
        for _ in range(warmup):
            for fn in legs.values():
                fn()
        t = {name: [] for name in legs}
        for _ in range(reps):  # alternate, so drift of the clocks hits all legs alike
            for name, fn in legs.items():
                t[name].append(_timed(torch, fn))
        peak = {name: _peak(torch, legs[name]) for name in ("create_foreground_info", "foreground_info")}
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "timing": "host perf_counter around a call that ends in torch.cuda.synchronize(); ms; the legs alternate",
           "P": P, "F": F, "k": k, **{name: _stats(ms) for name, ms in t.items()},
           "peak_allocated_bytes": peak, "outputs": same}
    out["forward_plus_foreground_info_median_ms"] = (out["rigidity_forward"]["median_ms"] +
                                                     out["foreground_info"]["median_ms"])
    out["bytes_from_shapes"] = {
        "note": "computed from shapes, each array counted once per op that reads or writes it; not measured traffic",
        "foreground_info": F * (4 + 12 + 16 + 16) + F * k * (4 + 12 + 12),
        "foreground_info_formula": "F*(4 row + 12 mean + 16 quaternion + 16 out) + F*k*(4 row + 12 gathered mean + 12 out)",
        "side_output_extra": F * 16 + F * k * 12,
        "side_output_extra_formula": "F*16 + F*k*12: the two stores; every input is already in registers",
        "create_foreground_info": P * (12 + 1 + 1 + 16 + 16) + F * (8 + 16 + 16 + 16 + 16 + 12 + 12) +
                                  F * k * (2 * 8 + 8 + 12 + 12 + 12 + 12 + 12 + 12 + 12),
        "create_foreground_info_formula": "P*(mask column read at its 12-byte stride, bool written and read by nonzero, "
                                          "normalize 16 in + 16 out) + F*(int64 rows, quaternion gather in + out, negation "
                                          "in + out, mean gather in + out) + F*k*(index min and max 2*8, int64 index 8, "
                                          "gather 12 in + 12 out, subtraction 12 in + 12 out, permuted copy 12 in + 12 out; "
                                          "the broadcast own mean not counted)",
    }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds the measuring child process may take")
    ap.add_argument("--child", action="store_true", help="(child process) measure and print the JSON line")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "foreground_ab.json"))
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.P, a.k, a.reps, a.warmup)))
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--P", str(a.P), "--k", str(a.k),
           "--reps", str(a.reps), "--warmup", str(a.warmup)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)  # kills the child at the limit
    if r.returncode != 0:
        sys.exit(f"bench_foreground: the measuring process ended with status {r.returncode}")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
