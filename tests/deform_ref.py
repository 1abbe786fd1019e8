"""Checkers for the deformation network's input side (splat_deform, csrc/gsr_deform.hip): a closed-form
restatement of train.py:113-127 / 185-204 / 269-294 and a torch-only restatement of train.py:57-110.

The encoding is parameterised by dtype.  ``torch.float32`` uses the reference's own ops on the same
arguments (its result equals the reference's bit for bit on the same device); ``torch.float64`` starts
from the SAME fp32 arguments ``f_l * xn`` (the normalisation and the product stay fp32: they are part of
the definition) and evaluates the sine and the cosine of it in float64.

``band`` and ``yardstick`` are the comparisons the three test files of the network share.
"""
import numpy as np
import torch
from torch import nn


def band(name, got, ref, rtol=1e-4, atol_frac=1e-6, floor=0.0):
    """|got - ref| <= max(rtol |ref| + atol_frac max|ref|, floor) everywhere, both finite."""
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, np.float64)
    ref = np.asarray(ref.detach().cpu() if torch.is_tensor(ref) else ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(ref).all() and np.isfinite(got).all(), name
    scale = np.abs(ref).max()
    err = np.abs(got - ref)
    bad = err > np.maximum(rtol * np.abs(ref) + atol_frac * scale, floor)
    print(f"{name}: worst {err.max():.3e} = {err.max() / max(scale, 1e-300):.3e} max|ref| ({scale:.3e}), "
          f"floor {floor:.3e}, outside {bad.sum()}/{bad.size}")
    assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} outside the band, worst {err.max():.3g} (scale {scale:.3g})"


def yardstick(name, got, r32, r64):
    """``band`` against the float64 result, never tighter than twice what torch's own float32 composition misses
    it by."""
    yard = float((r32.double() - r64).abs().max()) if r64.numel() else 0.0
    print(f"{name}: float32 torch composition vs float64 {yard:.3e}")
    band(name, got, r64, floor=2 * yard)


def normalize(x):
    """train.py:190-197, fp32: per column (2 (x - min)) / max(x - min) - 1."""
    n = x - x.min(dim=0).values
    return (2.0 * n / n.max(dim=0).values) - 1.0


def frequencies(count, device):
    """train.py:116-119: fp32(2^l) * fp32(pi)."""
    return ((torch.ones(count) * 2).pow(torch.arange(count)) * torch.pi).to(device)


def arguments(x, frequency_count):
    """(P, C, L) fp32 products f_l * x_c, as train.py:123 forms them."""
    return frequencies(frequency_count, x.device) * x.float()[:, :, None]


def encode_arguments(args, dtype=torch.float32):
    """(P, C, L) arguments -> (P, 2 L C) features: index (2 l) C + c = sin, (2 l + 1) C + c = the cosine of
    that sine (train.py:124-125 read the slots they have just overwritten)."""
    s = torch.sin(args.to(dtype))
    c = torch.cos(s)
    emb = torch.stack((s, c), dim=3).flatten(2)  # (P, C, 2 L): [.., 2 l] = sin, [.., 2 l + 1] = cos
    return emb.permute(0, 2, 1).flatten(start_dim=1)


def encode_means_and_rotations(means, quats, dtype=torch.float32):
    """train.py:185-204: (P, 92)."""
    return torch.cat((encode_arguments(arguments(normalize(means), 10), dtype),
                      encode_arguments(arguments(normalize(quats), 4), dtype)), dim=1)


def encode_progress(progress, rows, device, dtype=torch.float32):
    """train.py:277-282: (rows, 8), every row the same."""
    p = torch.tensor(progress, dtype=torch.float32).view(1, 1).repeat(rows, 1).to(device)
    return encode_arguments(arguments(p, 4), dtype)


def input_matrix(initial, previous, progress, dtype=torch.float32):
    """The (P, 192) matrix fc_in multiplies (train.py:96-103); ``initial`` / ``previous``: dicts with
    ``means`` and ``rotation_quaternions``."""
    P, dev = initial["means"].shape[0], initial["means"].device
    return torch.cat((encode_means_and_rotations(initial["means"], initial["rotation_quaternions"], dtype),
                      encode_means_and_rotations(previous["means"], previous["rotation_quaternions"], dtype),
                      encode_progress(progress, P, dev, dtype)), dim=1)


class ResidualBlock(nn.Module):
    def __init__(self, dimension):
        super().__init__()
        self.fc1 = nn.Linear(dimension, dimension, bias=False)
        self.bn1 = nn.BatchNorm1d(dimension)
        self.fc2 = nn.Linear(dimension, dimension, bias=False)
        self.bn2 = nn.BatchNorm1d(dimension)

    def forward(self, x):
        identity = x
        x = nn.functional.gelu(self.bn1(self.fc1(x)))
        x = self.bn2(self.fc2(x))
        return nn.functional.gelu(x + identity)


class TorchDeformationNetwork(nn.Module):
    """train.py:80-110, torch only, in the dtype it is converted to; ``forward`` takes the (P, 192) input
    matrix and the (P, 7) initial means and quaternions."""

    def __init__(self, hidden_dimension, residual_block_count):
        super().__init__()
        self.fc_in = nn.Linear(192, hidden_dimension)
        self.residual_blocks = nn.Sequential(*(ResidualBlock(hidden_dimension) for _ in range(residual_block_count)))
        self.fc_out = nn.Linear(hidden_dimension, 7)

    def forward(self, x, initial_means_and_rotations):
        return self.fc_out(self.residual_blocks(self.fc_in(x))) + initial_means_and_rotations


def network_output_and_grads(net, initial, previous, progress, upstream, dtype):
    """Output, fc_in output and every parameter's gradient of ``net`` (a TorchDeformationNetwork already in
    ``dtype``) for the upstream gradient ``upstream``."""
    x = input_matrix(initial, previous, progress, dtype)
    net.zero_grad()
    fc_in_out = []
    hook = net.fc_in.register_forward_hook(lambda m, i, o: fc_in_out.append(o.detach()))
    out = net(x, torch.cat((initial["means"], initial["rotation_quaternions"]), dim=1).to(dtype))
    hook.remove()
    (out * upstream.to(dtype)).sum().backward()
    return out.detach(), fc_in_out[0], {n: p.grad.clone() for n, p in net.named_parameters()}
