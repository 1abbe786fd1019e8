"""Fused Adam against the reference's own optimizer, torch.optim.Adam.

The reference optimises the Gaussians with torch.optim.Adam (densify.py:68-86: one named group per
parameter, lr = 0.0 default, eps = 1e-15), which IS the parity target here: the GPU tests run both on
identical parameters / gradients for several steps, including a group with lr = 0 (segmentation
masks), groups without gradients (camera_*), sizes that are not multiples of 4, a learning-rate
change between steps, and densification surgery in between.  Parameters, both moments and step
counts must be BITWISE equal: the kernel reproduces _multi_tensor_adam's operation order and its
compiler's FMA contractions (lerp, addcmul, addcdiv), verified with tools/adam_probe.py.

The second half pins the paths only production shapes reach: more than 16 tensors in one call (the
AdamTable of csrc/gsr_api_aux.hip is flushed and refilled), a real DeformationNetwork(40, 3) under
train.py's scheduler, 16-byte-unaligned parameters or gradients (k_adam's scalar branch with four whole
elements), an empty tensor, two (betas, eps) configurations in one step(), step = 30 000, and the gradient
classes of a trained cloud (exact zeros, g^2 underflowing or subnormal, 1e18, mixed signs).  These compare
BITS (int32 views), so -0.0 and NaN payloads count.  Each size-driven case has a CPU test that restates, on
torch.optim.Adam itself, the mistake the case exists to catch, and asserts the bits change.
"""
import numpy as np
import pytest
import torch

LR = {"means": 0.00016 * 3.0, "colors": 0.0025, "segmentation_masks": 0.0, "rotation_quaternions": 0.001,
      "opacity_logits": 0.05, "log_scales": 0.001, "camera_matrices": 1e-4, "camera_center": 1e-4}
WIDTH = {"means": 3, "colors": 3, "segmentation_masks": 3, "rotation_quaternions": 4, "opacity_logits": 1,
         "log_scales": 3}


def _params(P, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    p = {k: torch.randn(P, w, generator=g) for k, w in WIDTH.items()}
    p["camera_matrices"] = torch.zeros(50, 3)
    p["camera_center"] = torch.zeros(50, 3)
    return {k: torch.nn.Parameter(v.to(dev)) for k, v in p.items()}


def _opt(cls, params):
    return cls([{"params": [v], "name": k, "lr": LR[k]} for k, v in params.items()], lr=0.0, eps=1e-15)


def _close(a, b, what):
    """Bitwise equal: the fused kernel follows torch's foreach operation order and contractions."""
    np.testing.assert_array_equal(a.detach().cpu().numpy(), b.detach().cpu().numpy(), err_msg=what)


def test_fused_adam_refuses_cpu_and_unsupported():
    import splat_adam
    with pytest.raises(NotImplementedError):
        splat_adam.FusedAdam([torch.nn.Parameter(torch.zeros(3))], weight_decay=0.1)
    p = torch.nn.Parameter(torch.zeros(3))
    opt = splat_adam.FusedAdam([p])
    p.grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        opt.step()


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 1001, 65536 + 3])
def test_gpu_fused_adam_matches_torch_adam(cuda, P):
    import splat_adam
    pa, pb = _params(P, cuda), _params(P, cuda)
    oa, ob = _opt(torch.optim.Adam, pa), _opt(splat_adam.FusedAdam, pb)
    g = torch.Generator().manual_seed(1)
    for it in range(6):
        if it == 3:  # a scheduler-style lr change
            for o in (oa, ob):
                for grp in o.param_groups:
                    grp["lr"] *= 0.5
        for k in WIDTH:
            gr = (0.01 * torch.randn(pa[k].shape, generator=g)).to(cuda)
            pa[k].grad, pb[k].grad = gr.clone(), gr.clone()
        oa.step()
        ob.step()
    torch.cuda.synchronize()
    for k in pa:
        _close(pb[k], pa[k], k)
        if k in WIDTH:
            sa, sb = oa.state[pa[k]], ob.state[pb[k]]
            assert float(sa["step"]) == float(sb["step"]) == 6.0
            _close(sb["exp_avg"], sa["exp_avg"], k + ".exp_avg")
            _close(sb["exp_avg_sq"], sa["exp_avg_sq"], k + ".exp_avg_sq")
        else:
            assert len(ob.state[pb[k]]) == 0  # never had a gradient: no state, like torch
    np.testing.assert_array_equal(pb["segmentation_masks"].detach().cpu().numpy(),
                                  _params(P, "cpu")["segmentation_masks"].detach().numpy())  # lr = 0


@pytest.mark.gpu
def test_gpu_fused_adam_through_densification(cuda):
    """Adam state surgery by splat_densify works on FusedAdam exactly as on torch.optim.Adam."""
    import splat_adam
    import splat_densify
    P = 5000
    runs = []
    for cls in (torch.optim.Adam, splat_adam.FusedAdam):
        params = _params(P, cuda, seed=3)
        with torch.no_grad():
            params["log_scales"].mul_(0.5).add_(float(np.log(0.03)))
        opt = _opt(cls, params)
        g = torch.Generator().manual_seed(4)
        for k in WIDTH:
            params[k].grad = (0.01 * torch.randn(params[k].shape, generator=g)).to(cuda)
        opt.step()
        dv = splat_densify.DensificationVariables(
            visibility_count=torch.full((P,), 2.0, device=cuda),
            mean_2d_gradients_accumulated=(8e-4 * torch.rand(P, generator=g)).to(cuda),
            max_2d_radii=torch.zeros(P, device=cuda),
            gaussian_is_visible_mask=torch.zeros(P, dtype=torch.bool, device=cuda),
            means_2d=torch.zeros(P, 3, device=cuda, requires_grad=True))
        dv.means_2d.grad = torch.zeros(P, 3, device=cuda)
        torch.manual_seed(9)
        info = splat_densify.densify_gaussians(params, dv, 3.0, opt, 1000)
        for k in WIDTH:
            params[k].grad = (0.01 * torch.randn(params[k].shape, generator=g)).to(cuda)
        opt.step()
        runs.append((params, opt, info))
    (pa, oa, ia), (pb, ob, ib) = runs
    assert ia == ib and ia["n_split"] > 0 and ia["n_keep_clone"] > 0
    for k in WIDTH:
        _close(pb[k], pa[k], k)
        _close(ob.state[pb[k]]["exp_avg"], oa.state[pa[k]]["exp_avg"], k)
        assert float(ob.state[pb[k]]["step"]) == float(oa.state[pa[k]]["step"]) == 2.0


# ---- paths only production shapes reach -----------------------------------------------------------
SIZES = (1, 3, 5, 1023, 1024, 1025, 4099)
TABLE = 16  # kAdamMaxTensors of csrc/gsr_internal.h: tensors per launch


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _same_bits(a, b, what):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


def _same_optimizer_state(oa, ob, pa, pb, what=""):
    """Parameters, both moments and step of two optimizers over twin parameter lists: bitwise equal."""
    if pa and pa[0].is_cuda:
        torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(pa, pb)):
        _same_bits(b, a, f"{what} parameter {i} ({a.numel()} elements)")
        sa, sb = oa.state.get(a, {}), ob.state.get(b, {})
        assert sorted(sa) == sorted(sb), (what, i, sorted(sa), sorted(sb))
        if sa:
            assert float(sa["step"]) == float(sb["step"]), (what, i)
            _same_bits(sb["exp_avg"], sa["exp_avg"], f"{what} exp_avg {i}")
            _same_bits(sb["exp_avg_sq"], sa["exp_avg_sq"], f"{what} exp_avg_sq {i}")


def _plan(n):
    """A list of (numel, has_gradient) with ``n`` non-empty tensors that get gradients, sizes cycling through
    SIZES, one empty tensor with a gradient in the middle and a tensor without a gradient after every third."""
    plan = []
    for i in range(n):
        plan.append((SIZES[(3 * i + i // 7) % len(SIZES)], True))
        if i == n // 2:
            plan.append((0, True))
        if i % 3 == 2:
            plan.append((SIZES[i % len(SIZES)], False))
    assert sum(1 for m, g in plan if g and m) == n and set(m for m, g in plan if g and m) == set(SIZES)
    return plan


def _plan_lr(i):
    return 1e-3 * (1 + i % 5) * (1.5 if i % 2 else 1.0)  # neighbours and entries 16 apart differ


def _run_plan(cls, device, plan, steps=4, mistake=None):
    """``steps`` steps of ``cls`` over the tensors of ``plan`` (one param group each, its own lr), seeded
    gradients; at step 1 every fifth tensor gets none, so the step counts (and bias corrections) differ
    between tensors.  ``mistake`` restates a table bug on the reference: "dropped" gives the non-empty tensors
    after the 16th no gradient, "stale" steps them with the lr of the entry 16 before (a slot not rewritten
    after reset())."""
    g = torch.Generator().manual_seed(len(plan))
    params = [torch.nn.Parameter(torch.randn(m, generator=g).to(device)) for m, _ in plan]
    slot, slots = 0, []
    for m, has in plan:
        slots.append(slot if has and m else None)
        slot += bool(has and m)
    groups = []
    for i, p in enumerate(params):
        lr = _plan_lr(i)
        if mistake == "stale" and slots[i] is not None and slots[i] >= TABLE:
            lr = _plan_lr(slots.index(slots[i] - TABLE))
        groups.append({"params": [p], "lr": lr})
    opt = cls(groups, lr=0.0, eps=1e-15)
    for s in range(steps):
        for i, (p, (m, has)) in enumerate(zip(params, plan)):
            gr = (0.01 * torch.randn(m, generator=g)).to(device)
            skipped = (s == 1 and i % 5 == 4) or (mistake == "dropped" and slots[i] is not None and slots[i] >= TABLE)
            p.grad = gr if has and not skipped else None
        opt.step()
    return params, opt, slots


@pytest.mark.parametrize("n", [17, 33])
@pytest.mark.parametrize("mistake", ["dropped", "stale"])
def test_reference_is_sensitive_to_table_overflow(n, mistake):
    """torch.optim.Adam on the CPU, run right and with the mistake restated: every tensor past the 16th
    changes bits, no earlier one does."""
    plan = _plan(n)
    (pa, oa, slots), (pb, ob, _) = _run_plan(torch.optim.Adam, "cpu", plan), _run_plan(torch.optim.Adam, "cpu", plan,
                                                                                   mistake=mistake)
    for i, (a, b) in enumerate(zip(pa, pb)):
        late = slots[i] is not None and slots[i] >= TABLE
        assert bool((_bits(a) != _bits(b)).any()) == late, (i, slots[i])
    assert sum(1 for s in slots if s is not None and s >= TABLE) == n - TABLE


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 33])
def test_gpu_table_overflow(cuda, n):
    """17 / 33 non-empty tensors with gradients in one step(): one / two flushes of the 16-entry table."""
    import splat_adam
    plan = _plan(n)
    pa, oa, _ = _run_plan(torch.optim.Adam, cuda, plan)
    pb, ob, _ = _run_plan(splat_adam.FusedAdam, cuda, plan)
    _same_optimizer_state(oa, ob, pa, pb, f"{n} tensors")
    steps = {float(oa.state[p]["step"]) for p in pa if p in oa.state}
    assert steps == {3.0, 4.0}  # the tensors' bias corrections differ
    empty = [p for p, (m, has) in zip(pb, plan) if has and not m]
    assert len(empty) == 1 and float(ob.state[empty[0]]["step"]) in (3.0, 4.0)  # stepped like torch's, no launch


def _scheduler(opt, warmup, total):
    """train.py:138-152 create_learning_rate_scheduler."""
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, SequentialLR
    return SequentialLR(opt, schedulers=[LinearLR(opt, start_factor=1 / 1000, total_iters=warmup),
                                         CosineAnnealingLR(opt, T_max=total - warmup)], milestones=[warmup])


def _network_run(cls, device, hidden=40, blocks=3, warmup=3, total=8, mistake=None):
    import splat_deform
    torch.manual_seed(11)
    net = splat_deform.DeformationNetwork(hidden, blocks)
    params = [torch.nn.Parameter(p.detach().clone().to(device)) for p in net.parameters()]
    opt = cls(params, lr=1e-2)
    sched = _scheduler(opt, warmup, total)
    g = torch.Generator().manual_seed(12)
    lrs = []
    for _ in range(total + 1):  # the last step runs at the cosine's last value (lr = eta_min = 0)
        lrs.append(opt.param_groups[0]["lr"])
        for i, p in enumerate(params):
            gr = (0.1 * torch.randn(p.shape, generator=g)).to(device)
            p.grad = None if mistake == "dropped" and i >= TABLE else gr
        opt.step()
        sched.step()
    return params, opt, lrs


def test_network_has_more_tensors_than_the_table():
    """DeformationNetwork(40, 3): 2 + 3 x 6 + 2 = 22 tensors; torch.optim.Adam without the last 6 changes them."""
    (pa, oa, lrs), (pb, ob, _) = _network_run(torch.optim.Adam, "cpu"), _network_run(torch.optim.Adam, "cpu",
                                                                                     mistake="dropped")
    assert len(pa) == 22
    assert lrs[0] == pytest.approx(1e-5) and lrs[3] == pytest.approx(1e-2) and max(lrs) == lrs[3] and lrs[-1] < 1e-18
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert bool((_bits(a) != _bits(b)).any()) == (i >= TABLE), i


@pytest.mark.gpu
def test_gpu_network_under_scheduler(cuda):
    import splat_adam
    pa, oa, la = _network_run(torch.optim.Adam, cuda)
    pb, ob, lb = _network_run(splat_adam.FusedAdam, cuda)
    assert la == lb and len(pb) == 22
    _same_optimizer_state(oa, ob, pa, pb, "DeformationNetwork(40, 3)")


def _unaligned(values, device):
    """A contiguous view one float into a larger buffer: data_ptr() % 16 == 4."""
    buf = torch.zeros(values.numel() + 9, device=device)
    view = buf[1:1 + values.numel()]
    view.copy_(values)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _unaligned_run(cls, device, which, n, mistake=None):
    g = torch.Generator().manual_seed(n)
    init = torch.randn(n, generator=g)
    p = torch.nn.Parameter(_unaligned(init, device) if which == "param" else init.to(device))
    opt = cls([p], lr=1e-2, eps=1e-15)
    for _ in range(3):
        gr = 0.1 * torch.randn(n, generator=g)
        if mistake == "whole_quads_skipped":  # only a thread's ragged tail is updated
            gr[:n // 4 * 4] = 0
        p.grad = _unaligned(gr, device) if which == "grad" else gr.to(device)
        opt.step()
    return [p], opt


@pytest.mark.parametrize("n", [4, 7, 4099])
def test_reference_accepts_unaligned_and_empty(n):
    """torch.optim.Adam takes a Parameter that is a view at a 4-byte offset, and an empty one; leaving out the
    threads that hold four whole elements (the branch only an unaligned tensor reaches) changes the result."""
    (pa, oa), (pb, ob) = _unaligned_run(torch.optim.Adam, "cpu", "param", n), _unaligned_run(
        torch.optim.Adam, "cpu", "param", n, mistake="whole_quads_skipped")
    assert pa[0].data_ptr() % 16 == 4
    changed = _bits(pa[0]) != _bits(pb[0])
    assert changed[:n // 4 * 4].all() and not changed[n // 4 * 4:].any()
    e = torch.nn.Parameter(torch.zeros(0))
    opt = torch.optim.Adam([e], lr=1e-2)
    e.grad = torch.zeros(0)
    opt.step()
    assert float(opt.state[e]["step"]) == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["param", "grad"])
@pytest.mark.parametrize("n", [4, 7, 4099])
def test_gpu_unaligned(cuda, which, n):
    import splat_adam
    pa, oa = _unaligned_run(torch.optim.Adam, cuda, which, n)
    pb, ob = _unaligned_run(splat_adam.FusedAdam, cuda, which, n)
    _same_optimizer_state(oa, ob, pa, pb, f"unaligned {which} {n}")


def _two_config_run(cls, device):
    g = torch.Generator().manual_seed(21)
    params = [torch.nn.Parameter(torch.randn(m, generator=g).to(device)) for m in (1025, 7, 300, 4099)]
    opt = cls([{"params": params[:2], "betas": (0.9, 0.999), "eps": 1e-15},
               {"params": params[2:3], "betas": (0.8, 0.99), "eps": 1e-15},
               {"params": params[3:], "betas": (0.9, 0.999), "eps": 1e-8}], lr=3e-3)
    for _ in range(3):
        for p in params:
            p.grad = (0.05 * torch.randn(p.shape, generator=g)).to(device)
        opt.step()
    return params, opt


def test_reference_separates_configurations():
    """The three groups' (betas, eps) matter: with the first group's everywhere, groups 2 and 3 change."""
    pa, _ = _two_config_run(torch.optim.Adam, "cpu")

    def merged(groups, **kw):
        for grp in groups[1:]:
            grp["betas"], grp["eps"] = (0.9, 0.999), 1e-15
        return torch.optim.Adam(groups, **kw)

    pb, _ = _two_config_run(merged, "cpu")
    assert [bool((_bits(a) != _bits(b)).any()) for a, b in zip(pa, pb)] == [False, False, True, True]


@pytest.mark.gpu
def test_gpu_configurations_in_one_step(cuda):
    """Param groups with different betas and with a different eps in one step(): one launch per configuration."""
    import splat_adam
    pa, oa = _two_config_run(torch.optim.Adam, cuda)
    pb, ob = _two_config_run(splat_adam.FusedAdam, cuda)
    _same_optimizer_state(oa, ob, pa, pb, "three configurations")


def _late_run(cls, device, start=29_999.0):
    g = torch.Generator().manual_seed(31)
    params = [torch.nn.Parameter(torch.randn(m, generator=g).to(device)) for m in (1025, 5)]
    opt = cls(params, lr=1.6e-4, eps=1e-15)
    for p in params:
        opt.state[p] = {"step": torch.tensor(start), "exp_avg": (1e-3 * torch.randn(p.shape, generator=g)).to(device),
                        "exp_avg_sq": (1e-6 * torch.rand(p.shape, generator=g)).to(device)}
    for _ in range(2):
        for p in params:
            p.grad = (0.01 * torch.randn(p.shape, generator=g)).to(device)
        opt.step()
    return params, opt


def test_reference_late_steps_differ_from_early_ones():
    """step = 29 999 is not step = 9: the bias corrections (here 1 - 0.999^t) still differ in fp32."""
    (pa, _), (pb, _) = _late_run(torch.optim.Adam, "cpu"), _late_run(torch.optim.Adam, "cpu", start=9.0)
    assert all((_bits(a) != _bits(b)).any() for a, b in zip(pa, pb))


@pytest.mark.gpu
def test_gpu_late_steps(cuda):
    import splat_adam
    pa, oa = _late_run(torch.optim.Adam, cuda)
    pb, ob = _late_run(splat_adam.FusedAdam, cuda)
    _same_optimizer_state(oa, ob, pa, pb, "steps 30 000 and 30 001")
    assert float(ob.state[pb[0]]["step"]) == 30_001.0


# name -> (gradient values, moments populated?)
GRADIENT_CLASSES = {
    "zeros_fresh": (lambda r: torch.zeros(1030), False),
    "zeros_with_moments": (lambda r: torch.zeros(1030), True),
    "g2_underflows_fresh": (lambda r: torch.full((1030,), 1e-30) * _signs(r), False),
    "g2_underflows_with_moments": (lambda r: torch.full((1030,), 1e-30) * _signs(r), True),
    "g2_subnormal_fresh": (lambda r: torch.full((1030,), 1e-22) * _signs(r), False),
    "g2_subnormal_with_moments": (lambda r: torch.full((1030,), 1e-22) * _signs(r), True),
    "huge_fresh": (lambda r: torch.full((1030,), 1e18) * _signs(r), False),
    "huge_with_moments": (lambda r: torch.full((1030,), 1e18) * _signs(r), True),
    "mixed": (lambda r: torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e-22, -1e-22, 1e18, -1e18, 1e-3, -1e-3]).repeat(103), True),
}


def _signs(g):
    return torch.where(torch.rand(1030, generator=g) < 0.5, -1.0, 1.0)


def _class_run(cls, device, name):
    make, populated = GRADIENT_CLASSES[name]
    g = torch.Generator().manual_seed(41)
    p = torch.nn.Parameter(torch.randn(1030, generator=g).to(device))
    opt = cls([p], lr=1e-3, eps=1e-15)
    if populated:
        m, v = 1e-3 * torch.randn(1030, generator=g), 1e-6 * torch.rand(1030, generator=g)
        m[::3], v[::3] = 0.0, 0.0  # rows never seen before, among rows that were
        opt.state[p] = {"step": torch.tensor(5.0), "exp_avg": m.to(device), "exp_avg_sq": v.to(device)}
    for _ in range(2):
        p.grad = make(g).to(device)
        opt.step()
    return [p], opt


def test_reference_handles_every_gradient_class():
    """torch.optim.Adam on the CPU stays finite on every class, and the classes are what they claim to be."""
    for name, (make, _) in GRADIENT_CLASSES.items():
        (p,), opt = _class_run(torch.optim.Adam, "cpu", name)
        assert torch.isfinite(p).all() and torch.isfinite(opt.state[p]["exp_avg_sq"]).all(), name
    f = torch.tensor([1e-30, 1e-22, 1e18])
    sq = f * f
    assert sq[0] == 0 and 0 < sq[1] < torch.finfo(torch.float32).tiny and torch.isfinite(sq[2])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRADIENT_CLASSES))
def test_gpu_gradient_classes(cuda, name):
    """Every class bitwise: none needed the 1-ulp allowance the fused kernel's contract would permit for a
    class one of the two sides flushes."""
    import splat_adam
    pa, oa = _class_run(torch.optim.Adam, cuda, name)
    pb, ob = _class_run(splat_adam.FusedAdam, cuda, name)
    _same_optimizer_state(oa, ob, pa, pb, name)
