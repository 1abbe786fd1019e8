"""Checkers for the rigidity tests (not a test module): a float64 torch restatement of the rigidity
term of train.py:325-351, differentiated by autograd, and a numpy brute-force float64 k-nearest-
neighbour search.  The GPU tests compare the HIP kernels with these and with
tests/golden/reference_rigidity.npz (the reference's own outputs); nothing else is needed."""
import numpy as np
import torch


def rotation_matrices(q):
    """(N, 4) quaternions (w, x, y, z), normalised here, to (N, 3, 3) rotation matrices."""
    q = q / q.pow(2).sum(-1, keepdim=True).sqrt()
    w, x, y, z = q.unbind(-1)
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, -1).reshape(-1, 3, 3)


def hamilton(a, b):
    """Quaternion product a b of (N, 4) arrays, components (w, x, y, z)."""
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz,
                        aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw], -1)


def unit(q):
    """torch.nn.functional.normalize: q / max(|q|, 1e-12)."""
    return q / q.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)


def rigidity_loss(means, quats, mask, indices, weights, inverted_rotations, offsets, dtype=torch.float64):
    """The loss from full (P, 3) means / (P, 4) raw quaternions, a boolean foreground mask (P), (F, k)
    indices into the foreground rows, (F, k) weights, (F, 4) previous inverted rotations and (F, k, 3)
    previous offsets; evaluated in ``dtype`` on the inputs' device."""
    fm = means.to(dtype)[mask]
    fq = unit(quats.to(dtype))[mask]
    R = rotation_matrices(hamilton(fq, inverted_rotations.to(dtype)))
    d = fm[indices] - fm[:, None]                      # (F, k, 3) world-space offsets
    v = torch.einsum("frc,fkr->fkc", R, d)             # R^T d
    s = (v - offsets.to(dtype)).pow(2).sum(-1) * weights.to(dtype)
    return (s + 1e-20).sqrt().mean()


def rigidity_loss_and_grads(means, quats, mask, indices, weights, inverted_rotations, offsets, dtype=torch.float64):
    """(loss, d loss / d means (P, 3), d loss / d quats (P, 4)) in ``dtype``."""
    m = means.detach().to(dtype).requires_grad_(True)
    q = quats.detach().to(dtype).requires_grad_(True)
    loss = rigidity_loss(m, q, mask, indices, weights, inverted_rotations, offsets, dtype)
    gm, gq = torch.autograd.grad(loss, (m, q))
    return loss.detach(), gm, gq


def foreground_info(means, quats, mask, indices, dtype=torch.float64):
    """(inverted rotations (F, 4), offsets (F, k, 3)) of a state: the conjugated unit quaternions and
    the offsets to the neighbours of the foreground rows."""
    fq = unit(quats.to(dtype))[mask].clone()
    fq[:, 1:] = -fq[:, 1:]
    fm = means.to(dtype)[mask]
    return fq, fm[indices] - fm[:, None]


def brute_force_knn(points, k, chunk=512):
    """The k nearest OTHER points of each row of ``points`` (n, 3): float64 squared distances from the
    given coordinates, self excluded by index, ascending, ties by the lower index (stable argsort).
    Returns (indices (n, k) int64, squared distances (n, k) float64)."""
    p = np.ascontiguousarray(points, dtype=np.float64)
    n = p.shape[0]
    idx = np.empty((n, k), dtype=np.int64)
    d2 = np.empty((n, k), dtype=np.float64)
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        dx = p[None, :, 0] - p[a:b, None, 0]
        dy = p[None, :, 1] - p[a:b, None, 1]
        dz = p[None, :, 2] - p[a:b, None, 2]
        d = dx * dx + dy * dy + dz * dz
        d[np.arange(b - a), np.arange(a, b)] = np.inf
        order = np.argsort(d, axis=1, kind="stable")[:, :k]
        idx[a:b] = order
        d2[a:b] = np.take_along_axis(d, order, axis=1)
    return idx, d2
