"""Generate tests/golden/reference_deform.npz by running the REFERENCE's deformation network on the CPU.

Run in the build container only (needs the reference tree, like gen_golden.py, whose shims it uses):
    python tests/golden/gen_golden_deform.py
Only data is written: seeded inputs (P = 257 Gaussians, hidden dimension 32, one residual block, train
mode) and what the reference's ``normalize_and_encode_means_and_rotations``, ``PositionalEncoding``
(progress) and ``DeformationNetwork`` (with autograd, for a seeded upstream gradient) return for them --
``fc_in``'s output and the gradient that reaches it included -- plus the ``state_dict`` names and shapes.
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

P, H, BLOCKS = 257, 32, 1
TIMESTEP, TIMESTEP_COUNT = 3, 7


def main():
    _install_shims()
    sys.path.insert(0, REF)
    train = importlib.import_module("train")
    g = torch.Generator().manual_seed(31)
    cloud = lambda: {"means": (torch.rand(P, 3, generator=g) - 0.5) * 3.0,  # noqa: E731
                     "rotation_quaternions": torch.randn(P, 4, generator=g)}
    initial, previous = cloud(), cloud()
    previous["means"] = initial["means"] + 0.05 * torch.randn(P, 3, generator=g)
    enc_initial = train.normalize_and_encode_means_and_rotations(initial)
    enc_previous = train.normalize_and_encode_means_and_rotations(previous)
    enc_progress = train.PositionalEncoding(frequency_count=4)(
        torch.tensor(TIMESTEP / TIMESTEP_COUNT).view(1, 1).repeat(P, 1))

    torch.manual_seed(32)
    net = train.DeformationNetwork(H, BLOCKS)
    net.train()
    fc_in_out = []

    def keep(module, inputs, output):
        output.retain_grad()
        fc_in_out.append(output)

    hook = net.fc_in.register_forward_hook(keep)
    out = net(initial_means_and_rotations=torch.cat((initial["means"], initial["rotation_quaternions"]), dim=1),
              encoded_normalized_initial_means_and_rotations=enc_initial,
              encoded_normalized_previous_means_and_rotations=enc_previous, encoded_progress=enc_progress)
    hook.remove()
    upstream = torch.randn(P, 7, generator=g)
    # the state before the forward's BatchNorm update is not needed: train mode uses batch statistics
    (out * upstream).sum().backward()

    data = {"initial_means": initial["means"], "initial_rotation_quaternions": initial["rotation_quaternions"],
            "previous_means": previous["means"], "previous_rotation_quaternions": previous["rotation_quaternions"],
            "timestep": torch.tensor([TIMESTEP, TIMESTEP_COUNT]), "encoded_initial": enc_initial,
            "encoded_previous": enc_previous, "encoded_progress": enc_progress[0], "fc_in_output": fc_in_out[0].detach(),
            "grad_fc_in_output": fc_in_out[0].grad, "output": out.detach(), "upstream": upstream}
    names = []
    for name, value in net.state_dict().items():
        names.append(name)
        data[f"state/{name}"] = value
    for name, p in net.named_parameters():
        data[f"grad/{name}"] = p.grad
    arrays = {k: v.numpy() for k, v in data.items()}
    arrays["state_names"] = np.array(names)
    arrays["state_shapes"] = np.array([",".join(str(d) for d in net.state_dict()[n].shape) for n in names])
    path = os.path.join(HERE, "reference_deform.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; |fc_in out| max {float(fc_in_out[0].detach().abs().max()):.3f}, "
          f"|out| max {float(out.detach().abs().max()):.3f}")


if __name__ == "__main__":
    main()
