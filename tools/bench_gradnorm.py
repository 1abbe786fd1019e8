"""A/B timing of the end of a train.py step -- the gradient norm (train.py:432-443, logged at :769-772) and
optimizer.step() (:774) -- on the parameter shapes of DeformationNetwork(128, 6) and (512, 6) with random
gradients.  Writes one JSON file (default profiles/gradnorm_ab.json).

    python tools/bench_gradnorm.py

Three legs, one iteration each:

* reference: the reference's ``calculate_gradient_norm``, restated below (a Python list of
  ``parameter.grad.norm(2).pow(2)`` handed to ``torch.tensor``: one blocking device-to-host read per
  parameter), then ``FusedAdam.step()``;
* stand_alone: ``splat_adam.gradient_norm`` and ``step()``, the value sent to the host through ``ScoreLog``;
* fused: ``step(grad_norm=True)`` and ``ScoreLog``.

Per leg: the host wall time of one iteration (perf_counter around the calls, no synchronise inside: what the
host thread is held for), as the median of alternated repeats after warm-up; the time of ``batch``
iterations ending in a synchronise, per iteration (what the device is held for); and the kernel launches and
blocking host reads of one iteration, counted from the code.  Everything is timed twice: with the GPU
otherwise idle, and with about 2 ms of queued work ahead of the iteration (``torch.cuda._sleep``), the case
in which the reference's reads make the host wait for the queue to drain.
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

import splat_adam  # noqa: E402
import splat_deform  # noqa: E402
import splat_train  # noqa: E402


def calculate_gradient_norm(parameters):
    """train.py:432-443."""
    return torch.sqrt(torch.sum(torch.tensor([p.grad.norm(2).pow(2) for p in parameters if p.grad is not None])))


def _stats(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def _sleep_cycles_for(ms, dev):
    """Cycles of torch.cuda._sleep that take about ``ms`` on this device (calibrated with events)."""
    probe = 20_000_000
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(probe)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(probe)
    b.record()
    torch.cuda.synchronize()
    return max(int(probe * ms / a.elapsed_time(b)), 1)


def bench(hidden, a, dev):
    torch.manual_seed(hidden)
    net = splat_deform.DeformationNetwork(hidden, 6).to(dev)
    params = list(net.parameters())
    for p in params:
        p.grad = 1e-3 * torch.randn_like(p)
    opt = splat_adam.FusedAdam(params, lr=1e-4)
    log = splat_train.ScoreLog(depth=8)
    n, tables = len(params), -(-len(params) // 16)

    def reference():
        value = calculate_gradient_norm(params)
        opt.step()
        return value

    def stand_alone():
        log.put(0, splat_adam.gradient_norm(params))
        opt.step()
        log.drain()

    def fused():
        opt.step(grad_norm=True)
        log.put(0, opt.grad_norm)
        log.drain()

    legs = {"reference": reference, "stand_alone": stand_alone, "fused": fused}
    # from the code: norm + pow per parameter, sum + sqrt on the host tensor; k_adam per table;
    # k_grad_sumsq + k_norm_final per table; k_adam<true> + k_norm_final per table
    launches = {"reference": 2 * n + tables, "stand_alone": 3 * tables, "fused": 2 * tables}
    host_reads = {"reference": n, "stand_alone": 0, "fused": 0}
    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    cycles = _sleep_cycles_for(a.queued_ms, dev)
    out = {}
    for cond, ahead in (("idle", 0), ("queued", cycles)):
        host = {k: [] for k in legs}
        through = {k: [] for k in legs}
        for _ in range(a.reps):  # alternate, so drift hits all alike
            for k, fn in legs.items():
                torch.cuda.synchronize()
                if ahead:
                    torch.cuda._sleep(ahead)
                t0 = time.perf_counter()
                fn()
                host[k].append((time.perf_counter() - t0) * 1e3)
            for k, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.batch):
                    if ahead:
                        torch.cuda._sleep(ahead)
                    fn()
                torch.cuda.synchronize()
                through[k].append((time.perf_counter() - t0) * 1e3 / a.batch)
        out[cond] = {k: {"host": _stats(host[k]), "per_iteration_to_synchronise": _stats(through[k])} for k in legs}
    log.close()
    return {"parameters": n, "elements": sum(p.numel() for p in params), "launches": launches,
            "blocking_host_reads": host_reads, "queued_sleep_cycles": cycles,
            "timing": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--queued-ms", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gradnorm_ab.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "workload": "gradient norm + optimizer step over DeformationNetwork(H, 6)'s parameters, random gradients",
           "timing": "host perf_counter, ms; 'host': one iteration without a synchronise inside; "
                     "'per_iteration_to_synchronise': a batch of iterations ending in a synchronise; "
                     f"'queued': about {a.queued_ms} ms of torch.cuda._sleep ahead of every iteration (its time is "
                     "inside per_iteration_to_synchronise)",
           "networks": {f"DeformationNetwork({h}, 6)": bench(h, a, dev) for h in a.hidden}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
