"""Generate tests/golden/reference_rigidity.npz by running the REFERENCE's rigidity functions on the CPU.

Run in the build container only (needs the reference tree, like gen_golden.py, whose shims it uses):
    python tests/golden/gen_golden_rigidity.py
Only data is written: the seeded inputs and what the reference's ``create_foreground_info`` and
``calculate_rigidity_loss`` (with autograd) return for them.  The neighbour lists come from
scipy.spatial.cKDTree on the float64 coordinates (open3d, which the reference's own search needs, is a
stub here); the k + 1 nearest are queried and the query point itself dropped.
"""
import importlib
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import REF, _install_shims  # noqa: E402

P, K = 300, 20


def main():
    from scipy.spatial import cKDTree
    _install_shims()
    sys.path.insert(0, REF)
    train = importlib.import_module("train")
    g = torch.Generator().manual_seed(20)
    mask = (torch.rand(P, generator=g) < 0.6).float()
    seg = torch.stack((mask, torch.zeros(P), 1 - mask), 1)
    prev = {"means": torch.rand(P, 3, generator=g) * 0.2, "rotation_quaternions": torch.randn(P, 4, generator=g),
            "colors": torch.rand(P, 3, generator=g), "opacity_logits": torch.randn(P, 1, generator=g),
            "log_scales": torch.randn(P, 3, generator=g) - 4.0, "segmentation_masks": seg}
    fg = prev["means"][mask > 0.5].numpy().astype(np.float64)
    d, idx = cKDTree(fg).query(fg, K + 1)
    assert np.array_equal(idx[:, 0], np.arange(fg.shape[0]))  # no coincident points in the seeded cloud
    idx, d2 = idx[:, 1:], d[:, 1:] ** 2
    # squared distances as the sum of squared float64 coordinate differences (not the rounded root's square)
    diff = fg[idx] - fg[:, None]
    d2 = (diff * diff).sum(-1)
    info = train.NeighborInfo(indices=torch.tensor(idx).long().contiguous(),
                              weights=torch.tensor(np.exp(-2000 * d2)).float().contiguous())
    fi = train.create_foreground_info(prev, info.indices)

    def loss_of(params):
        p = dict(params)
        p["means"] = params["means"].clone().requires_grad_(True)
        p["rotation_quaternions"] = params["rotation_quaternions"].clone().requires_grad_(True)
        loss = train.calculate_rigidity_loss(p, info, fi)
        loss.backward()
        return loss.detach(), p["means"].grad, p["rotation_quaternions"].grad

    cur = dict(prev)
    cur["means"] = prev["means"] + 0.003 * torch.randn(P, 3, generator=g)
    cur["rotation_quaternions"] = prev["rotation_quaternions"] + 0.05 * torch.randn(P, 4, generator=g)
    loss, gm, gq = loss_of(cur)
    loss0, _, _ = loss_of(prev)
    out = {f"prev_{k}": v.numpy() for k, v in prev.items()}
    out.update({"cur_means": cur["means"].numpy(), "cur_rotation_quaternions": cur["rotation_quaternions"].numpy(),
                "knn_indices": idx.astype(np.int64), "knn_squared_distances": d2,
                "weights": info.weights.numpy(), "fi_inverted_rotations": fi.inverted_rotations.numpy(),
                "fi_offsets_to_neighbors": fi.offsets_to_neighbors.numpy(), "loss": loss.numpy(),
                "grad_means": gm.numpy(), "grad_rotation_quaternions": gq.numpy(),
                "loss_unperturbed": loss0.numpy()})
    path = os.path.join(HERE, "reference_rigidity.npz")
    np.savez_compressed(path, **out)
    F = int((mask > 0.5).sum())
    bg = mask < 0.5
    print(f"wrote {path}: {os.path.getsize(path)} bytes; F = {F}, loss {float(loss):.4e}, unperturbed "
          f"{float(loss0):.3e}, background grads zero: {bool((gm[bg] == 0).all() and (gq[bg] == 0).all())}")


if __name__ == "__main__":
    main()
