"""A whole train.py step (train.py:738-776), network to Adam, against the float64 restatement of
tests/train_ref.py, and train.py's inference chain (550-616).

The fused step is built as train.py builds it: every Gaussian parameter frozen,
``splat_deform.update_gaussian_cloud_parameters`` -> ``splat_train.train_step_loss`` -> ``backward()`` ->
optimizer, the next step's foreground info taken from the updated cloud before the backward.

CPU: the checker checks itself (its fp32 step, which runs no HIP kernel, lies within max(project band,
1e-5 max|ref|) of its float64 step), the scenes' preconditions hold, and the checker moves by more than
100 tolerances under the mistakes the GPU tests are there to catch.  GPU: one step at three network
shapes, three consecutive timesteps with ``torch.optim.Adam`` and ``splat_adam.FusedAdam`` (bitwise equal),
and the inference chain, each step teacher-forced: the reference gets the fused network's state, previous
cloud and foreground info and takes its discrete decisions (tile lists, order, cull) from the fused
path's own updated cloud.

Tolerances.  "Project band": |got - ref| <= 1e-4 |ref| + 1e-6 max|ref|, no value outside.  Gradients:
the band with a floor of twice the yardstick, the yardstick being what the checker's own fp32 step misses
its float64 step by on that tensor (the rule of test_deform.py::test_whole_network).  Losses: 1e-5
relative.  Images: rtol 1e-4, atol 2e-5 (test_oracle.py's for dense_forward against the oracle).

Scenes.  ``splat_scenes.synthetic_cloud(P, S0, seed)`` with raw quaternions of norm 0.5 .. 1.5, about 60 %
foreground, a 40 x 24 image (3 x 2 tiles, ragged on both axes), focal 30, three cameras, k = 20 brute-force
neighbours with weights exp(-WEIGHT_DECAY d^2) (the cloud is far sparser than a trained one: train.py's
2000 would zero every weight).  The single steps start from a perturbed previous cloud; the chains start, as
train.py does, from previous = initial.  The seeds are fixed: each was searched on the CPU for a float64
threshold margin >= 1e-4 in every view (DESIGN.md 3.1 lists them with their margins).
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import deform_ref as DR
import rigidity_ref as RR
import splat_scenes as S
import train_ref as TR
from deform_ref import band

W, H, FOCAL, K = 40, 24, 30.0, 20
YAWS = (10.0, 100.0, 200.0)
S0 = 0.08
WEIGHT_DECAY = 5.0
T = 7
MARGIN = 1e-4
# name -> (hidden dimension, residual blocks, P, scene seed, timestep)
CASES = {"h40": (40, 2, 257, 9, 3), "h128": (128, 1, 160, 29, 3), "h192": (192, 1, 160, 52, 3)}
CHAIN = (40, 2, 257, 37)      # hidden dimension, residual blocks, P, scene seed: timesteps 1..3 of T
CHAIN_GAIN = 3.0              # the chain starts from previous = initial: only the network moves the cloud
INFERENCE = (40, 2, 257, 12)  # the same for the inference chain: timesteps 1..2 of T
LR = 1e-3


def _cameras(device):
    return [S.render_settings(W, H, S.intrinsics(FOCAL, W, H), S.look_at(yaw, 0.1, 4.0), device=device)
            for yaw in YAWS]


@functools.lru_cache(maxsize=None)
def _scene(P, seed, targets=1):
    """Everything a step reads, on the CPU: the frozen cloud, a perturbed previous cloud, ``targets`` sets of
    three target images, the foreground mask and the neighbour lists of the initial foreground."""
    cloud = S.synthetic_cloud(P, S0, seed=seed, device="cpu")
    g = torch.Generator().manual_seed(1000 + seed)
    m = (torch.rand(P, generator=g) < 0.6).float()
    cloud["segmentation_masks"] = torch.stack((m, torch.zeros(P), 1 - m), 1)
    cloud["rotation_quaternions"] = cloud["rotation_quaternions"] * (0.5 + torch.rand(P, 1, generator=g))
    previous = {"means": cloud["means"] + 0.03 * torch.randn(P, 3, generator=g),
                "rotation_quaternions": cloud["rotation_quaternions"] + 0.3 * torch.randn(P, 4, generator=g)}
    images = [[torch.rand(3, H, W, generator=g) for _ in YAWS] for _ in range(targets)]
    mask = m > 0.5
    idx, d2 = RR.brute_force_knn(cloud["means"][mask].numpy(), K)
    neighbors = (torch.from_numpy(idx), torch.from_numpy(np.exp(-WEIGHT_DECAY * d2).astype(np.float32)))
    return SimpleNamespace(P=P, cloud=cloud, previous=previous, images=images, mask=mask, neighbors=neighbors)


def _foreground(scene, cloud):
    """train.py:228-248 of ``cloud`` (means and raw quaternions) in fp32 on the CPU."""
    return RR.foreground_info(cloud["means"], cloud["rotation_quaternions"], scene.mask, scene.neighbors[0],
                              dtype=torch.float32)


def _views(scene, which=0, device="cpu"):
    return list(zip(_cameras(device), scene.images[which]))


@functools.lru_cache(maxsize=None)
def _state(hidden, blocks, seed, gain=1.0):
    """A seeded ``state_dict`` of the network with BatchNorms that are not the identity: affine parameters
    and running statistics away from (1, 0) and (0, 1).  ``gain`` scales ``fc_out``: a network that moves the
    cloud ``gain`` times as far as a freshly initialised one."""
    torch.manual_seed(100 + seed)
    net = DR.TorchDeformationNetwork(hidden, blocks)
    g = torch.Generator().manual_seed(200 + seed)
    with torch.no_grad():
        for block in net.residual_blocks:
            for bn in (block.bn1, block.bn2):
                bn.weight.add_(0.2 * torch.randn(hidden, generator=g))
                bn.bias.add_(0.1 * torch.randn(hidden, generator=g))
                bn.running_mean.add_(0.1 * torch.randn(hidden, generator=g))
                bn.running_var.add_(0.2 * torch.rand(hidden, generator=g))
        net.fc_out.weight.mul_(gain)
        net.fc_out.bias.mul_(gain)
    return {k: v.clone() for k, v in net.state_dict().items()}


def _tolerance(ref, yard):
    ref = np.abs(np.asarray(ref, np.float64))
    return np.maximum(1e-4 * ref + 1e-6 * ref.max(), 2 * yard)


def _yard(r32, r64):
    return float((r32.double() - r64).abs().max())


def _rel(name, got, ref, tol=1e-5):
    got, ref = float(got), float(ref)
    print(f"{name}: got {got:.9e} ref {ref:.9e} rel {abs(got - ref) / abs(ref):.3e}")
    assert abs(got - ref) <= tol * abs(ref), (name, got, ref)


LOSSES = ("total", "l1", "ssim", "rigidity")


# ---- the CPU runs every CPU test shares -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _single(name):
    """(scene, step inputs, float64 step, fp32 step) of a single-step case."""
    hidden, blocks, P, seed, t = CASES[name]
    scene = _scene(P, seed)
    args = dict(state=_state(hidden, blocks, seed), initial=scene.cloud, previous=scene.previous, timestep=t,
                timestep_count=T, views=_views(scene), neighbors=scene.neighbors,
                foreground=_foreground(scene, scene.previous))
    return scene, args, TR.step(**args, dtype=torch.float64), TR.step(**args, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _cpu_chain():
    """Three timesteps in train.py's order with the checker's fp32 step and ``torch.optim.Adam`` on the CPU;
    per step (inputs, float64 step on the same inputs, fp32 step)."""
    hidden, blocks, P, seed = CHAIN
    scene = _scene(P, seed, targets=3)
    net = TR.network(_state(hidden, blocks, seed, CHAIN_GAIN), torch.float32)
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    previous = {k: scene.cloud[k] for k in ("means", "rotation_quaternions")}  # train.py:731-737
    foreground = _foreground(scene, previous)
    out = []
    for t in (1, 2, 3):
        args = dict(state={k: v.clone() for k, v in net.state_dict().items()}, initial=scene.cloud,
                    previous=previous, timestep=t, timestep_count=T, views=_views(scene, t - 1),
                    neighbors=scene.neighbors, foreground=foreground)
        r32 = TR.step(**args, dtype=torch.float32)
        out.append((args, TR.step(**args, dtype=torch.float64), r32))
        previous = {k: r32[k] for k in ("means", "rotation_quaternions")}
        foreground = _foreground(scene, previous)
        net.load_state_dict({**net.state_dict(), **r32["buffers"]})
        for n, p in net.named_parameters():
            p.grad = r32["grads"][n]
        opt.step()
        opt.zero_grad()
    return scene, out


@functools.lru_cache(maxsize=None)
def _cpu_inference():
    """Two timesteps of train.py:575-616 with the checker's fp32 forward; per step (inputs, float64, fp32)."""
    hidden, blocks, P, seed = INFERENCE
    scene = _scene(P, seed, targets=3)
    state = _state(hidden, blocks, seed)
    previous = {k: scene.cloud[k] for k in ("means", "rotation_quaternions")}
    out = []
    for t in (1, 2):
        args = dict(state=state, initial=scene.cloud, previous=previous, timestep=t, timestep_count=T,
                    views=_views(scene)[t - 1:t], neighbors=None, foreground=None, backward=False)
        r32 = TR.step(**args, dtype=torch.float32)
        out.append((args, TR.step(**args, dtype=torch.float64), r32))
        previous = {k: r32[k] for k in ("means", "rotation_quaternions")}
        state = {**state, **r32["buffers"]}
    return scene, out


def _every_training_step():
    for name in CASES:
        scene, _, r64, r32 = _single(name)
        yield name, scene, r64, r32
    scene, steps = _cpu_chain()
    for t, (_, r64, r32) in enumerate(steps, 1):
        yield f"chain t={t}", scene, r64, r32


# ---- CPU ------------------------------------------------------------------------------------------
def test_reference_checks_itself():
    """The fp32 step that runs no HIP kernel against the float64 step, on every scene the GPU tests use."""
    for name, _, r64, r32 in _every_training_step():
        for i, loss in enumerate(LOSSES):
            band(f"{name} loss {loss}", r32["losses"][i], r64["losses"][i], floor=1e-5 * abs(float(r64["losses"][i])))
        for n, g64 in r64["grads"].items():
            band(f"{name} grad {n}", r32["grads"][n], g64, floor=1e-5 * float(g64.abs().max()))
        band(f"{name} updated means", r32["means"], r64["means"])
        band(f"{name} updated quaternions", r32["rotation_quaternions"], r64["rotation_quaternions"])
    for t, (_, r64, r32) in enumerate(_cpu_inference()[1], 1):
        band(f"inference t={t} updated means", r32["means"], r64["means"])
        np.testing.assert_allclose(r32["images"][0].numpy(), r64["images"][0].numpy(), rtol=1e-4, atol=2e-5)


def test_scene_preconditions():
    for name, scene, r64, _ in _every_training_step():
        radii = np.stack([st["radii"] for st in r64["states"]])
        share = 3 * float(r64["losses"][3]) / float(r64["losses"][0])
        print(f"{name}: margin {r64['margin']:.3e}, visible per view {(radii > 0).sum(1)}, F {int(scene.mask.sum())}, "
              f"rigidity share {share:.3f}")
        assert r64["margin"] >= MARGIN
        assert (radii > 0).any(0).all()   # every Gaussian takes part in some view
        assert (radii == 0).any()         # and some view has one culled or off every tile
        assert int(scene.mask.sum()) >= K + 1
        assert 0.01 <= share <= 0.5
        for n, g in r64["grads"].items():
            assert float(g.abs().max()) > 0, n
    for t, (_, r64, _) in enumerate(_cpu_inference()[1], 1):
        print(f"inference t={t}: margin {r64['margin']:.3e}")
        assert r64["margin"] >= MARGIN


@pytest.mark.parametrize("mistake", ["previous_is_initial", "stale_foreground_info", "rigidity_counted_once",
                                     "one_view_dropped"])
@pytest.mark.parametrize("name", list(CASES))
def test_reference_is_sensitive(name, mistake):
    """Each mistake moves some gradient tensor of the checker by more than 100 of the tolerances the GPU tests
    apply to it."""
    scene, args, r64, r32 = _single(name)
    initial = {k: scene.cloud[k] for k in ("means", "rotation_quaternions")}
    wrong = dict(args, **{"previous_is_initial": dict(previous=initial),
                          "stale_foreground_info": dict(foreground=_foreground(scene, initial)),
                          "rigidity_counted_once": dict(rigidity_count=1),
                          "one_view_dropped": dict(views=args["views"][:-1], rigidity_count=len(YAWS))}[mistake])
    moved = TR.step(**wrong, dtype=torch.float32)
    ratios = {}
    for n, g64 in r64["grads"].items():
        tol = _tolerance(g64.numpy(), _yard(r32["grads"][n], g64))
        ratios[n] = float((np.abs((moved["grads"][n] - r32["grads"][n]).numpy()) / tol).max())
    worst = max(ratios, key=ratios.get)
    print(f"{name} {mistake}: {worst} moves by {ratios[worst]:.1f} tolerances")
    assert ratios[worst] > 100


# ---- GPU: the fused step --------------------------------------------------------------------------
def _to(d, device):
    return {k: v.to(device) for k, v in d.items()}


def _fused_network(state, hidden, blocks, device):
    import splat_deform as D
    net = D.DeformationNetwork(hidden, blocks)
    net.load_state_dict(state)
    return net.to(device).train()


def _gpu_views(scene, which, device, keep=slice(None)):
    import splat_train
    return [splat_train.View(camera_index=i, render_settings=rs, image=image.to(device), segmentation_mask=None)
            for i, (rs, image) in enumerate(_views(scene, which, device))][keep]


def _host(d):
    return {k: v.detach().cpu().clone() for k, v in d.items()}


def _radii(updated, views):
    from diff_gaussian_rasterization import rasterize_parameters
    with torch.no_grad():
        cloud = {k: v.detach() for k, v in updated.items()}
        return [rasterize_parameters(cloud, v.render_settings)[1].cpu().numpy() for v in views]


def _reference_pair(args, updated):
    """(float64 step deciding from the fused path's ``updated`` cloud, fp32 step) on ``args``."""
    r64 = TR.step(**args, dtype=torch.float64, decisions=updated)
    return r64, TR.step(**args, dtype=torch.float32)


def _check_decisions(name, radii, r64):
    for v, (got, st) in enumerate(zip(radii, r64["states"])):
        np.testing.assert_array_equal(got, st["radii"], err_msg=f"{name} view {v}: radii")
    print(f"{name}: margin {r64['margin']:.3e}")
    assert r64["margin"] >= MARGIN


def _check_step(name, got, r64, r32):
    """``got``: losses (4), means, rotation_quaternions, grads and buffers of a fused step."""
    for i, loss in enumerate(LOSSES):
        _rel(f"{name} loss {loss}", got["losses"][i], r64["losses"][i])
    band(f"{name} updated means", got["means"], r64["means"])
    band(f"{name} updated quaternions", got["rotation_quaternions"], r64["rotation_quaternions"])
    for n, g64 in r64["grads"].items():
        yard = _yard(r32["grads"][n], g64)
        print(f"{name} grad {n}: yardstick {yard:.3e} = {yard / float(g64.abs().max()):.3e} max|ref|")
        band(f"{name} grad {n}", got["grads"][n], g64, floor=2 * yard)
    for n, b64 in r64["buffers"].items():
        if n.endswith("num_batches_tracked"):
            assert int(got["buffers"][n]) == int(b64), n
        else:
            band(f"{name} {n}", got["buffers"][n], b64)


def _buffers(net):
    return {k: v.detach().cpu().clone() for k, v in net.named_buffers()}


def _fused_single(name, device):
    import splat_deform as D
    import splat_rigidity as R
    import splat_train
    from diff_gaussian_rasterization import pending_views
    hidden, blocks, P, seed, t = CASES[name]
    scene = _scene(P, seed)
    net = _fused_network(_state(hidden, blocks, seed), hidden, blocks, device)
    initial, previous = _to(scene.cloud, device), _to(scene.previous, device)
    assert not any(v.requires_grad for v in initial.values())
    views = _gpu_views(scene, 0, device)
    ni = R.NeighborInfo(indices=scene.neighbors[0].to(device), weights=scene.neighbors[1].to(device))  # packed on first use
    fi = R.create_foreground_info(dict(initial, **previous), ni.indices)
    updated = D.update_gaussian_cloud_parameters(net, initial, previous, t, T)
    assert updated["means"].grad_fn is not None and updated["rotation_quaternions"].grad_fn is not None
    losses = splat_train.train_step_loss(updated, views, ni, fi)
    losses[0].backward()
    torch.cuda.synchronize()
    assert pending_views() == 0
    assert all(v.grad is None for v in initial.values())
    got = {"losses": [float(x.detach()) for x in losses], "means": updated["means"].detach().cpu(),
           "rotation_quaternions": updated["rotation_quaternions"].detach().cpu(),
           "grads": {n: p.grad.detach().cpu() for n, p in net.named_parameters()}, "buffers": _buffers(net)}
    args = dict(state=_state(hidden, blocks, seed), initial=scene.cloud, previous=scene.previous, timestep=t,
                timestep_count=T, views=_views(scene), neighbors=scene.neighbors,
                foreground=(fi.inverted_rotations.cpu(), fi.offsets_to_neighbors.cpu()))
    r64, r32 = _reference_pair(args, _host({k: updated[k] for k in ("means", "rotation_quaternions")}))
    _check_decisions(name, _radii(updated, views), r64)
    _check_step(name, got, r64, r32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_one_step_against_float64(cuda, name):
    _fused_single(name, cuda)


@pytest.mark.gpu
def test_one_step_against_float64_torch_blocks_and_head(cuda):
    """The same step with the residual blocks and the output head on the torch ops."""
    import splat_deform as D
    blocks, head = D.set_fused_residual_blocks(False), D.set_fused_output_head(False)
    try:
        _fused_single("h40", cuda)
    finally:
        D.set_fused_residual_blocks(blocks)
        D.set_fused_output_head(head)


# ---- GPU: three consecutive timesteps -------------------------------------------------------------
_CHAIN_RUNS = {}


def _fused_chain(device, optimizer, run=0):
    """Three timesteps in train.py's order (train.py:738-776) with ``optimizer`` ("adam" / "fused"); per step
    what the reference needs to be teacher-forced, what the fused step produced and the optimizer's state after
    it.  Remembered per (optimizer, run)."""
    if (optimizer, run) in _CHAIN_RUNS:
        return _CHAIN_RUNS[(optimizer, run)]
    import splat_adam
    import splat_deform as D
    import splat_rigidity as R
    import splat_train
    from diff_gaussian_rasterization import pending_views
    hidden, blocks, P, seed = CHAIN
    scene = _scene(P, seed, targets=3)
    net = _fused_network(_state(hidden, blocks, seed, CHAIN_GAIN), hidden, blocks, device)
    cls = {"adam": torch.optim.Adam, "fused": splat_adam.FusedAdam}[optimizer]
    opt = cls(net.parameters(), lr=LR)
    initial = _to(scene.cloud, device)
    idx, w = (t.to(device) for t in scene.neighbors)
    ni = R.NeighborInfo(indices=idx, weights=w, packed=R.pack_neighbors(initial, idx, w))  # as create_neighbor_info
    previous = {k: initial[k] for k in ("means", "rotation_quaternions")}
    fi = R.create_foreground_info(initial, ni.indices)
    steps, stale = [], None
    for t in (1, 2, 3):
        rec = SimpleNamespace(state=_host(net.state_dict()), previous=_host(previous),
                              foreground=(fi.inverted_rotations.cpu().clone(), fi.offsets_to_neighbors.cpu().clone()))
        views = _gpu_views(scene, t - 1, device)
        updated = D.update_gaussian_cloud_parameters(net, initial, previous, t, T)
        losses = splat_train.train_step_loss(updated, views, ni, fi)
        if stale is not None:  # this step's loss with the foreground info of the step before
            with torch.no_grad():
                rec.stale_losses = [float(x) for x in splat_train.train_step_loss(
                    {k: v.detach() for k, v in updated.items()}, views, ni, stale)]
        stale = fi
        fi = R.create_foreground_info(updated, ni.indices)  # train.py:759-765: before the backward
        losses[0].backward()
        assert pending_views() == 0
        rec.radii = _radii(updated, views)
        rec.got = {"losses": [float(x.detach()) for x in losses], "means": updated["means"].detach().cpu(),
                   "rotation_quaternions": updated["rotation_quaternions"].detach().cpu(),
                   "grads": {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters()},
                   "buffers": _buffers(net)}
        opt.step()
        opt.zero_grad()
        rec.optimizer = {n: {k: v.detach().cpu().clone() for k, v in opt.state[p].items()}
                         for n, p in net.named_parameters()}
        rec.parameters = {n: p.detach().cpu().clone() for n, p in net.named_parameters()}
        steps.append(rec)
        previous = {k: updated[k].detach() for k in ("means", "rotation_quaternions")}
    torch.cuda.synchronize()
    assert all(v.grad is None for v in initial.values())
    _CHAIN_RUNS[(optimizer, run)] = (scene, steps)
    return scene, steps


@pytest.mark.gpu
@pytest.mark.parametrize("t", [1, 2, 3])
def test_three_steps_against_float64(cuda, t):
    """Step ``t`` of the chain run with torch.optim.Adam, the reference teacher-forced with the fused run's
    state, previous cloud and foreground info before that step."""
    scene, steps = _fused_chain(cuda, "adam")
    rec = steps[t - 1]
    args = dict(state=rec.state, initial=scene.cloud, previous=rec.previous, timestep=t, timestep_count=T,
                views=_views(scene, t - 1), neighbors=scene.neighbors, foreground=rec.foreground)
    r64, r32 = _reference_pair(args, {k: rec.got[k] for k in ("means", "rotation_quaternions")})
    _check_decisions(f"chain t={t}", rec.radii, r64)
    _check_step(f"chain t={t}", rec.got, r64, r32)
    if t > 1:  # a stale foreground info (a cache hit on the step before) would be seen: of the four losses compared
        # above at 1e-5 relative, it moves at least one by more than 100 times that
        moved = [abs(s - g) / abs(g) for s, g in zip(rec.stale_losses, rec.got["losses"])]
        print(f"chain t={t}: the previous step's foreground info moves the losses by "
              + ", ".join(f"{n} {m:.3e}" for n, m in zip(LOSSES, moved)) + " relative")
        assert max(moved) > 1e-3


def _same_bits(a, b, what):
    np.testing.assert_array_equal(a.numpy(), b.numpy(), err_msg=what)


@pytest.mark.gpu
def test_fused_adam_is_torch_adam_on_the_network(cuda):
    """``FusedAdam(net.parameters(), lr)`` with the default eps = 1e-8 on (H, 192), (H, H), (H,), (7, H) and
    (7,) tensors: parameters, both moments and the step count bitwise equal to torch.optim.Adam's after every
    one of the three steps."""
    _, a = _fused_chain(cuda, "adam")
    _, b = _fused_chain(cuda, "fused")
    for t, (ra, rb) in enumerate(zip(a, b), 1):
        shapes = set()
        for n in ra.parameters:
            shapes.add(tuple(ra.parameters[n].shape))
            _same_bits(rb.got["grads"][n], ra.got["grads"][n], f"t={t} grad {n}")
            _same_bits(rb.parameters[n], ra.parameters[n], f"t={t} {n}")
            for k in ("exp_avg", "exp_avg_sq"):
                _same_bits(rb.optimizer[n][k], ra.optimizer[n][k], f"t={t} {n}.{k}")
            assert float(rb.optimizer[n]["step"]) == float(ra.optimizer[n]["step"]) == float(t)
        assert shapes == {(40, 192), (40, 40), (40,), (7, 40), (7,)}


@pytest.mark.gpu
@pytest.mark.parametrize("optimizer", ["adam", "fused"])
def test_three_steps_bitwise_repeatable(cuda, optimizer):
    _, a = _fused_chain(cuda, optimizer)
    _, b = _fused_chain(cuda, optimizer, run=1)
    for t, (ra, rb) in enumerate(zip(a, b), 1):
        assert ra.got["losses"] == rb.got["losses"], t
        for n in ra.parameters:
            _same_bits(rb.got["grads"][n], ra.got["grads"][n], f"t={t} grad {n}")
            _same_bits(rb.parameters[n], ra.parameters[n], f"t={t} {n}")
        for n in ra.got["buffers"]:
            _same_bits(rb.got["buffers"][n], ra.got["buffers"][n], f"t={t} {n}")
        _same_bits(rb.got["means"], ra.got["means"], f"t={t} updated means")


# ---- GPU: the inference chain ---------------------------------------------------------------------
@pytest.mark.gpu
def test_inference_chain(cuda):
    """train.py:575-616: the network in train mode under ``no_grad``, ``previous = updated``, one render per step."""
    import splat_deform as D
    from diff_gaussian_rasterization import rasterize_parameters
    hidden, blocks, P, seed = INFERENCE
    scene = _scene(P, seed, targets=3)
    state = _state(hidden, blocks, seed)
    net = _fused_network(state, hidden, blocks, cuda)
    initial = _to(scene.cloud, cuda)
    cameras = _cameras(cuda)
    previous = {k: initial[k] for k in ("means", "rotation_quaternions")}
    saved = []
    for t in (1, 2):
        before, previous_host = _host(net.state_dict()), _host(previous)
        with torch.autograd.graph.saved_tensors_hooks(lambda x: saved.append(x) or x, lambda x: x):
            with torch.no_grad():
                updated = D.update_gaussian_cloud_parameters(net, initial, previous, t, T)
                image, radii, _ = rasterize_parameters(updated, cameras[t - 1])
        assert saved == []
        for x in (updated["means"], updated["rotation_quaternions"], image):
            assert x.grad_fn is None and not x.requires_grad
        args = dict(state=before, initial=scene.cloud, previous=previous_host, timestep=t, timestep_count=T,
                    views=_views(scene)[t - 1:t], neighbors=None, foreground=None, backward=False)
        r64 = TR.step(**args, dtype=torch.float64,
                      decisions=_host({k: updated[k] for k in ("means", "rotation_quaternions")}))
        _check_decisions(f"inference t={t}", [radii.cpu().numpy()], r64)
        band(f"inference t={t} updated means", updated["means"], r64["means"])
        band(f"inference t={t} updated quaternions", updated["rotation_quaternions"], r64["rotation_quaternions"])
        np.testing.assert_allclose(image.cpu().numpy(), r64["images"][0].numpy(), rtol=1e-4, atol=2e-5)
        after = _buffers(net)
        for n, b64 in r64["buffers"].items():
            if n.endswith("num_batches_tracked"):
                assert int(after[n]) == int(b64) == t, n
            else:
                band(f"inference t={t} {n}", after[n], b64)
                assert not torch.equal(after[n], before[n]), n  # blended, not left alone
        previous = {k: updated[k] for k in ("means", "rotation_quaternions")}
