"""Checker for a whole train.py step (not a test module): the deformation network, the update of the cloud,
one render per view, L1 + SSIM, the rigidity term and the backward, restated on the CPU in a given dtype
from the pieces the suite already has -- ``deform_ref.TorchDeformationNetwork`` and its encodings
(train.py:57-127, 185-204), ``rigidity_ref.rigidity_loss`` (train.py:325-351), ``oracle/dense_torch.py``
(the float64 differentiable rasterizer) and ``oracle/oracle.py`` (the fp32 C oracle).

``step`` is train.py:269-308 (``update_gaussian_cloud_parameters``) followed by train.py:354-418
(``calculate_loss``) and ``backward()``.  Two renderers:

* ``torch.float64``: ``dense_torch.dense_forward`` on an oracle state per view.  The state (tile lists,
  depth order, cull) comes from ``oracle.forward`` on the fp32 cloud ``decisions`` -- by default the
  step's own updated cloud rounded to fp32, for the GPU tests the fused path's updated cloud -- which
  contributes decisions only, never values;
* ``torch.float32``: ``_OracleRender``, an ``autograd.Function`` around ``oracle.forward`` /
  ``oracle.backward`` that returns the ``means3D`` and ``rotations`` gradients (everything else is
  frozen in train.py).  With ``TorchDeformationNetwork`` in fp32 this is a whole step without one HIP
  kernel: the yardstick of what fp32 arithmetic alone misses float64 by.

Everything is rendered as train.py renders it (shared.py:29-42): normalised quaternions, sigmoid
opacities, exp scales, RGB ``colors_precomp``, scale modifier 1.

Nothing here touches ``libgsr.so`` or needs a GPU.
"""
from math import exp

import numpy as np
import torch

import deform_ref as DR
import rigidity_ref as RR
from oracle import dense_torch as DT
from oracle import oracle as O

FROZEN = ("means", "rotation_quaternions", "log_scales", "opacity_logits", "colors", "segmentation_masks")


def torch_ssim(img1, img2):
    """external.py:68-110: mean SSIM, 11 x 11 Gaussian window (sigma 1.5), zero padding, in ``img1``'s dtype."""
    g = torch.tensor([exp(-((x - 5) ** 2) / float(2 * 1.5 ** 2)) for x in range(11)], dtype=img1.dtype)
    g = (g / g.sum()).unsqueeze(1)
    C = img1.size(-3)
    w = g.mm(g.t())[None, None].expand(C, 1, 11, 11).contiguous().to(img1.device)
    conv = lambda t: torch.nn.functional.conv2d(t, w, padding=5, groups=C)  # noqa: E731
    mu1, mu2 = conv(img1), conv(img2)
    s1, s2, s12 = conv(img1 * img1) - mu1 ** 2, conv(img2 * img2) - mu2 ** 2, conv(img1 * img2) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 ** 2 + mu2 ** 2 + c1) * (s1 + s2 + c2))).mean()


def activations(cloud, dtype):
    """shared.py:29-42 on the raw parameters of ``cloud``, evaluated in ``dtype``: (rotations, opacities, scales)."""
    return (torch.nn.functional.normalize(cloud["rotation_quaternions"].to(dtype)),
            torch.sigmoid(cloud["opacity_logits"].to(dtype)), torch.exp(cloud["log_scales"].to(dtype)))


def _oracle_forward(rs, means, colors, opacities, scales, rotations):
    n = lambda t: t.detach().cpu().float().numpy()  # noqa: E731
    return O.forward(n(rs.bg), n(means), n(colors), n(opacities), n(scales), n(rotations), rs.scale_modifier, None,
                     rs.viewmatrix.cpu(), rs.projmatrix.cpu(), rs.tanfovx, rs.tanfovy, rs.image_height,
                     rs.image_width, None, 0, n(rs.campos))


def oracle_state(cloud, rs):
    """The fp32 oracle's forward state of ``cloud`` (raw fp32 parameters, activated in fp32) seen through ``rs``."""
    rotations, opacities, scales = activations(cloud, torch.float32)
    return _oracle_forward(rs, cloud["means"], cloud["colors"], opacities, scales, rotations)


class _OracleRender(torch.autograd.Function):
    """The fp32 C oracle as a differentiable render of (means3D, rotations): train.py:359-361 with every
    other input a constant."""

    @staticmethod
    def forward(ctx, means, rotations, colors, opacities, scales, rs, states):
        st = _oracle_forward(rs, means, colors, opacities, scales, rotations)
        ctx.st = st
        states.append(st)
        return torch.from_numpy(st["color"].copy())

    @staticmethod
    def backward(ctx, grad):
        g = O.backward(ctx.st, grad.contiguous().numpy())
        return torch.from_numpy(g["means3D"]), torch.from_numpy(g["rotations"]), None, None, None, None, None


def network(state, dtype):
    """A train-mode ``TorchDeformationNetwork`` in ``dtype`` holding ``state`` (a ``state_dict``, buffers included)."""
    hidden = state["fc_in.weight"].shape[0]
    blocks = len({k.split(".")[1] for k in state if k.startswith("residual_blocks.")})
    net = DR.TorchDeformationNetwork(hidden, blocks).to(dtype).train()
    net.load_state_dict({k: v.detach().cpu() for k, v in state.items()})
    return net


def step(state, initial, previous, timestep, timestep_count, views, neighbors, foreground, dtype,
         decisions=None, rigidity_count=None, backward=True):
    """One train.py step on the CPU in ``dtype``.

    ``state``: the network's ``state_dict``; ``initial``: the frozen cloud (``FROZEN``, fp32); ``previous``:
    the previous timestep's means and quaternions; ``views``: (render settings, (3, H, W) target) pairs;
    ``neighbors``: (indices (F, k), weights (F, k)); ``foreground``: (inverted rotations (F, 4), offsets
    (F, k, 3)).  ``decisions`` (float64 only): the fp32 cloud whose oracle states the dense renderer takes its
    discrete decisions from (None: this step's updated cloud rounded to fp32).  ``rigidity_count``: how many
    times the rigidity term is counted (None: once per view, as train.py:395-418 does).  ``backward=False``
    stops after the renders (train.py:578-596) and returns the images instead of losses and gradients.

    Returns a dict: ``losses`` (total, sum l1, sum (1 - ssim), V rigidity) as a float64 tensor, ``means``,
    ``rotation_quaternions`` (updated, detached), ``grads`` and ``buffers`` by ``state_dict`` name, ``states``
    (one oracle state per view), ``images`` and, for float64, ``margin`` (the smallest ``dense_forward``
    threshold margin over the views).
    """
    initial = {k: initial[k].detach().cpu() for k in FROZEN}
    previous = {k: previous[k].detach().cpu() for k in ("means", "rotation_quaternions")}
    net = network(state, dtype)
    x = DR.input_matrix(initial, previous, timestep / timestep_count, dtype)
    base = torch.cat((initial["means"], initial["rotation_quaternions"]), dim=1).to(dtype)
    updated = base.detach() + net(x, base) * 0.01  # train.py:283-307
    means, quats = updated[:, :3], updated[:, 3:]
    cloud = dict(initial, means=means, rotation_quaternions=quats)
    rotations, opacities, scales = activations(cloud, dtype)
    colors = initial["colors"].to(dtype)

    states, images, margin = [], [], np.inf
    for rs, _ in views:
        if dtype == torch.float64:
            src = cloud if decisions is None else dict(initial, **{k: decisions[k].detach().cpu() for k in
                                                                    ("means", "rotation_quaternions")})
            st = oracle_state({k: v.detach().float() for k, v in src.items()}, rs)
            states.append(st)
            image, extras = DT.dense_forward(st, means, opacities, colors=colors.clone().requires_grad_(True),
                                             scales=scales, rotations=rotations)
            margin = min(margin, extras["margin"])
        else:
            image = _OracleRender.apply(means, rotations, colors, opacities, scales, rs, states)
        images.append(image)
    out = {"means": means.detach(), "rotation_quaternions": quats.detach(), "states": states,
           "images": [i.detach() for i in images], "buffers": {k: v.clone() for k, v in net.named_buffers()}}
    if dtype == torch.float64:
        out["margin"] = margin
    if not backward:
        return out

    l1 = sum(torch.nn.functional.l1_loss(i, t.cpu().to(dtype)) for i, (_, t) in zip(images, views))
    ssim = sum(1.0 - torch_ssim(i, t.cpu().to(dtype)) for i, (_, t) in zip(images, views))
    mask = initial["segmentation_masks"][:, 0] > 0.5
    count = len(views) if rigidity_count is None else rigidity_count
    rigidity = count * RR.rigidity_loss(means, quats, mask, neighbors[0].cpu(), neighbors[1].cpu(),
                                        foreground[0].cpu(), foreground[1].cpu(), dtype)
    total = 0.8 * l1 + 0.2 * ssim + 3 * rigidity
    total.backward()
    out["losses"] = torch.stack((total, l1, ssim, rigidity)).detach().double()
    out["grads"] = {n: p.grad.clone() for n, p in net.named_parameters()}
    return out
