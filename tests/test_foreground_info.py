"""The rigidity term's per-timestep state from the kernels (splat_rigidity.foreground_info,
calculate_rigidity_loss_and_state, splat_train.advance_timestep; csrc/gsr_rigidity.hip k_foreground_info and
the state instantiation of k_rigid_fwd).

CPU: the new calls refuse CPU tensors and malformed clouds, the C ABI refuses bad sizes before anything is
launched, and a libgsr.so without the two entry points serves everything else.  GPU: the offsets are ONE
IEEE subtraction per component, so they are compared bit for bit with ``fg[idx] - fg[:, None]`` evaluated
by torch in fp32 on the device (the golden ``fi_offsets_to_neighbors`` is bit-equal to that expression);
the inverted rotations within 1e-6 absolute of the float64 restatement (tests/rigidity_ref.py) and of the
golden ``fi_inverted_rotations`` -- the bound tests/test_rigidity.py uses for this quantity: the fp32
left-to-right restatement reproduces the golden bit for bit on the CPU, so the bound leaves room only for
the device's contraction.  The side output of the loss forward is bit-equal to the stand-alone kernel, and
its loss and gradients to ``calculate_rigidity_loss``.  A three-timestep chain carries the state through
``train_step_loss(next_foreground_info=True)`` / ``advance_timestep``: each rigidity loss within 1e-5
relative (test_rigidity's band for the GPU loss) of the float64 restatement fed the float64 state of the
previous cloud."""
import ctypes
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rigidity_ref as RR
import splat_rigidity as R
import splat_train
from diff_gaussian_rasterization import _C

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "reference_rigidity.npz"))
PERTURBATIONS = [(0.003, 0.05), (0.03, 0.5)]  # = test_rigidity.PERTURBATIONS (asserted below)
# (P, F, k): the golden cloud, a tiny one, the 256-lane block edge from both sides, k = 1, k = 32 (the
# largest), several blocks with ~60 % of the rows foreground
SHAPES = ["golden", (5, 4, 3), (400, 256, 20), (400, 257, 20), (70, 64, 1), (100, 40, 32), (4099, None, 20)]
PARITY_SHAPES = ["golden", (400, 257, 20)]


def _t(name):
    return torch.from_numpy(GOLD[name])


def _shape_id(s):
    return s if isinstance(s, str) else "-".join(str(v) for v in s)


def _cpu_cloud(shape):
    """(params on the CPU, k) of a case: seeded randoms, exactly F foreground rows scattered over the P."""
    if shape == "golden":
        return {"means": _t("prev_means"), "rotation_quaternions": _t("prev_rotation_quaternions"),
                "segmentation_masks": _t("prev_segmentation_masks")}, 20
    P, F, k = shape
    g = torch.Generator().manual_seed(1000 * P + k)
    if P == 5:
        mask = torch.tensor([True, True, False, True, True])
    elif F is None:
        mask = torch.rand(P, generator=g) < 0.6
    else:
        mask = torch.zeros(P, dtype=torch.bool)
        mask[torch.randperm(P, generator=g)[:F]] = True
    m = mask.float()
    return {"means": torch.rand(P, 3, generator=g) * 0.2, "rotation_quaternions": torch.randn(P, 4, generator=g),
            "segmentation_masks": torch.stack((m, torch.zeros(P), 1 - m), 1)}, k


@functools.lru_cache(maxsize=None)
def _case(shape, dev):
    """A case's cloud on the device with its neighbour lists, the kernel's state and the expectations:
    built once, shared by the tests, never modified."""
    cpu, k = _cpu_cloud(shape)
    pg = {n: v.to(dev) for n, v in cpu.items()}
    ni = R.create_neighbor_info(pg, k)
    fi = R.foreground_info(pg, ni)
    mask = cpu["segmentation_masks"][:, 0] > 0.5
    fg = pg["means"][mask.to(dev)]
    want_off = fg[ni.indices] - fg[:, None]  # fp32 on the device: one IEEE subtraction per component
    want_inv, _ = RR.foreground_info(cpu["means"], cpu["rotation_quaternions"], mask, ni.indices.cpu())
    return SimpleNamespace(cpu=cpu, params=pg, ni=ni, fi=fi, mask=mask, want_off=want_off, want_inv=want_inv,
                           P=mask.numel(), F=int(mask.sum()), k=k)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _gold_cpu_inputs():
    params = {"means": _t("cur_means"), "rotation_quaternions": _t("cur_rotation_quaternions"),
              "segmentation_masks": _t("prev_segmentation_masks")}
    ni = SimpleNamespace(indices=_t("knn_indices"), weights=_t("weights"))
    fi = SimpleNamespace(inverted_rotations=_t("fi_inverted_rotations"),
                         offsets_to_neighbors=_t("fi_offsets_to_neighbors"))
    return params, ni, fi


# ---- CPU ------------------------------------------------------------------------------------------
def test_no_cpu_path():
    params, ni, fi = _gold_cpu_inputs()
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.foreground_info(params, ni)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.calculate_rigidity_loss_and_state(params, ni, fi)
    with pytest.raises(RuntimeError, match="no CPU path"):
        splat_train.advance_timestep(params, ni)
    # a given state is carried, not recomputed: nothing touches the device
    prev, same = splat_train.advance_timestep({n: v.clone().requires_grad_(v.is_floating_point())
                                               for n, v in params.items()}, ni, fi)
    assert same is fi and set(prev) == set(params)
    assert all(not v.requires_grad and torch.equal(v, params[n]) for n, v in prev.items())


def test_malformed_clouds_are_value_errors():
    params, ni, fi = _gold_cpu_inputs()
    P = params["means"].shape[0]
    bad = [dict(params, means=torch.zeros(P, 4)), dict(params, means=params["means"].double()),
           dict(params, rotation_quaternions=params["rotation_quaternions"][:P - 1]),
           dict(params, rotation_quaternions=params["rotation_quaternions"].half()),
           dict(params, rotation_quaternions=torch.zeros(P, 3))]
    for p in bad:
        with pytest.raises(ValueError):
            R.foreground_info(p, ni)
        with pytest.raises(ValueError):
            R.calculate_rigidity_loss_and_state(p, ni, fi)
        with pytest.raises(ValueError):
            splat_train.advance_timestep(p, ni)


def test_c_abi_refuses_bad_sizes_before_launching():
    """F <= 0, k outside [1, 32], P < F and a missing state output are errors found on the host."""
    L = _C.feature_library("foreground")
    for P, F, k in [(10, 0, 3), (10, -1, 3), (10, 4, 0), (10, 4, 33), (3, 4, 3)]:
        assert L.gsr_foreground_info(P, F, k, None, None, None, None, None, None, None) != 0, (P, F, k)
        assert L.gsr_last_error()
        assert L.gsr_rigidity_forward_state(P, F, k, *[None] * 8, 0, *[None] * 4) != 0, (P, F, k)
    assert L.gsr_foreground_info(10, 4, 3, None, None, None, None, None, None, None) != 0  # null inputs
    buf = (ctypes.c_float * 64)()  # never dereferenced: the call is refused for its missing state outputs
    p = ctypes.cast(buf, ctypes.c_void_p)
    for nxt in [(None, None), (p, None), (None, p)]:
        assert L.gsr_rigidity_forward_state(10, 4, 3, *[p] * 8, 0, p, *nxt, None) != 0
        assert b"state" in L.gsr_last_error()


def test_stale_library_is_a_rebuild_error(monkeypatch):
    """As tests/test_deform.py::test_stale_library_is_a_rebuild_error, for the fourth optional group."""
    import test_deform
    assert test_deform.FEATURES == ("deform", "resblock", "head")  # its own list, not _OPTIONAL's keys
    assert list(_C._OPTIONAL) == list(test_deform.FEATURES) + ["foreground"]
    real = _C.load_library()
    assert not _C._MISSING and _C.feature_library("foreground") is real
    absent = list(_C._OPTIONAL["foreground"][1])
    assert absent == ["gsr_foreground_info", "gsr_rigidity_forward_state"]

    class Stale:
        def __getattr__(self, name):
            if name in absent:
                raise AttributeError(f"undefined symbol: {name}")
            return getattr(real, name)

    monkeypatch.setattr(_C, "_lib", None)
    monkeypatch.setattr(_C, "_MISSING", {})
    monkeypatch.setattr(_C, "_PREALLOC_FN", _C._PREALLOC_FN)
    monkeypatch.setattr(_C.ctypes, "CDLL", lambda path: Stale())
    stale = _C.load_library()
    assert isinstance(stale, Stale) and list(_C._MISSING) == ["foreground"]
    assert absent[0] in _C._MISSING["foreground"]
    assert all(_C.feature_library(other) is stale for other in test_deform.FEATURES)
    assert stale.gsr_rigidity_forward is real.gsr_rigidity_forward  # the loss itself is still served
    with pytest.raises(RuntimeError, match="rebuild"):
        _C.feature_library("foreground")


def test_perturbations_are_test_rigiditys():
    import test_rigidity
    assert PERTURBATIONS == test_rigidity.PERTURBATIONS


# ---- GPU: values ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_values(cuda, shape):
    c = _case(shape, cuda)
    fi, F, k = c.fi, c.F, c.k
    if shape != "golden" and shape[1] is not None:
        assert (c.P, F, k) == shape
    assert isinstance(fi, R.ForegroundInfo)
    assert fi.inverted_rotations.shape == (F, 4) and fi.inverted_rotations.is_contiguous()
    assert fi.offsets_to_neighbors.shape == (F, k, 3)
    assert fi.packed_offsets.shape == (k, 3, F) and fi.packed_offsets.is_contiguous()
    for t in (fi.inverted_rotations, fi.offsets_to_neighbors, fi.packed_offsets):
        assert t.dtype == torch.float32 and t.device == c.params["means"].device and not t.requires_grad
    # one buffer: the reference-layout field is a view of the packed one
    assert fi.offsets_to_neighbors.untyped_storage().data_ptr() == fi.packed_offsets.untyped_storage().data_ptr()
    assert fi.offsets_to_neighbors.data_ptr() == fi.packed_offsets.data_ptr()
    assert _same_bits(fi.offsets_to_neighbors, c.want_off)
    assert _same_bits(fi.packed_offsets, c.want_off.permute(1, 2, 0))
    err = (fi.inverted_rotations.cpu().double() - c.want_inv).abs().max().item()
    print(f"{_shape_id(shape)}: P={c.P} F={F} k={k} inverted rotations worst |err| vs float64 {err:.3e}")
    assert err <= 1e-6
    if shape == "golden":
        assert (c.P, F, k) == (300, 173, 20)
        assert np.array_equal(c.ni.indices.cpu().numpy(), GOLD["knn_indices"])
        gerr = (fi.inverted_rotations.cpu() - _t("fi_inverted_rotations")).abs().max().item()
        print(f"golden: inverted rotations worst |err| vs the reference's {gerr:.3e}")
        assert gerr <= 1e-6
        assert _same_bits(fi.offsets_to_neighbors.cpu(), _t("fi_offsets_to_neighbors"))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_repeatable_and_feeds_the_loss(cuda, shape):
    c = _case(shape, cuda)
    again = R.foreground_info(c.params, c.ni)
    assert _same_bits(again.inverted_rotations, c.fi.inverted_rotations)
    assert _same_bits(again.packed_offsets, c.fi.packed_offsets)
    # straight into the unchanged calculate_rigidity_loss, and equal to feeding it the torch-op state
    ref_fi = R.create_foreground_info(c.params, c.ni.indices)
    ref_fi.inverted_rotations = c.fi.inverted_rotations  # (the two normalisations may differ in the last bit)
    g = torch.Generator().manual_seed(9)
    cur = dict(c.params, means=c.params["means"] + 0.003 * torch.randn(c.P, 3, generator=g).to(cuda))
    a = R.calculate_rigidity_loss(cur, c.ni, c.fi)
    b = R.calculate_rigidity_loss(cur, c.ni, ref_fi)
    assert torch.isfinite(a) and _same_bits(a, b)


@pytest.mark.gpu
def test_zero_quaternion_gives_zeros(cuda):
    c = _case((400, 257, 20), cuda)
    rows = c.ni.packed.foreground_rows.long()
    q = c.params["rotation_quaternions"].clone()
    q[rows[3]] = 0
    q[rows[256]] = 0  # the first lane of the second block
    fi = R.foreground_info(dict(c.params, rotation_quaternions=q), c.ni)
    assert torch.isfinite(fi.inverted_rotations).all()
    assert (fi.inverted_rotations[3] == 0).all() and (fi.inverted_rotations[256] == 0).all()
    keep = torch.ones(c.F, dtype=torch.bool, device=cuda)
    keep[[3, 256]] = False
    assert _same_bits(fi.inverted_rotations[keep], c.fi.inverted_rotations[keep])
    assert _same_bits(fi.packed_offsets, c.fi.packed_offsets)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(5, 4, 3), (400, 257, 20), (4099, None, 20)], ids=_shape_id)
def test_background_rows_are_never_read(cuda, shape):
    c = _case(shape, cuda)
    bg = ~c.mask.to(cuda)
    assert bg.any()
    means, quats = c.params["means"].clone(), c.params["rotation_quaternions"].clone()
    means[bg] = float("nan")
    quats[bg] = float("nan")
    poisoned = dict(c.params, means=means, rotation_quaternions=quats)
    fi = R.foreground_info(poisoned, c.ni)
    assert torch.isfinite(fi.inverted_rotations).all() and torch.isfinite(fi.packed_offsets).all()
    assert _same_bits(fi.inverted_rotations, c.fi.inverted_rotations)
    assert _same_bits(fi.packed_offsets, c.fi.packed_offsets)
    loss, st = R.calculate_rigidity_loss_and_state(poisoned, c.ni, c.fi)
    assert torch.isfinite(loss)
    assert _same_bits(st.inverted_rotations, c.fi.inverted_rotations)
    assert _same_bits(st.packed_offsets, c.fi.packed_offsets)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(5, 4, 3), (400, 257, 20)], ids=_shape_id)
def test_c_abi_null_outputs(cuda, shape):
    c = _case(shape, cuda)
    L = _C.feature_library("foreground")
    nb = c.ni.packed
    m, q = c.params["means"].contiguous(), c.params["rotation_quaternions"].contiguous()

    def run(want_inv, want_off):
        inv = torch.full((c.F, 4), float("nan"), device=cuda)
        off = torch.full((c.k, 3, c.F), float("nan"), device=cuda)
        with _C._device_guard(cuda):
            _C._check(L.gsr_foreground_info(nb.P, nb.F, nb.k, m.data_ptr(), q.data_ptr(), nb.foreground_rows.data_ptr(),
                                            nb.neighbor_rows.data_ptr(), inv.data_ptr() if want_inv else None,
                                            off.data_ptr() if want_off else None, _C._stream_ptr(cuda)))
        torch.cuda.synchronize()
        return inv, off

    both = run(True, True)
    assert _same_bits(both[0], c.fi.inverted_rotations) and _same_bits(both[1], c.fi.packed_offsets)
    poison = run(False, False)  # nothing wanted: nothing launched, nothing written
    assert torch.isnan(poison[0]).all() and torch.isnan(poison[1]).all()
    inv, off = run(True, False)
    assert _same_bits(inv, both[0]) and _same_bits(off, poison[1])
    inv, off = run(False, True)
    assert _same_bits(off, both[1]) and _same_bits(inv, poison[0])


# ---- GPU: side output and entry points --------------------------------------------------------------
def _perturbed(c, pert, dev):
    dm, dq = PERTURBATIONS[pert]
    g = torch.Generator().manual_seed(50 + pert)
    return dict(c.params, means=c.params["means"] + (dm * torch.randn(c.P, 3, generator=g)).to(dev),
                rotation_quaternions=c.params["rotation_quaternions"] + (dq * torch.randn(c.P, 4, generator=g)).to(dev))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_side_output_equals_stand_alone_kernel(cuda, shape):
    c = _case(shape, cuda)
    cur = _perturbed(c, 0, cuda)
    alone = R.foreground_info(cur, c.ni)
    loss, st = R.calculate_rigidity_loss_and_state(cur, c.ni, c.fi)
    assert isinstance(st, R.ForegroundInfo) and st.offsets_to_neighbors.shape == (c.F, c.k, 3)
    assert st.offsets_to_neighbors.data_ptr() == st.packed_offsets.data_ptr()
    assert _same_bits(st.inverted_rotations, alone.inverted_rotations)
    assert _same_bits(st.packed_offsets, alone.packed_offsets)
    assert _same_bits(st.offsets_to_neighbors, alone.offsets_to_neighbors)
    assert _same_bits(loss, R.calculate_rigidity_loss(cur, c.ni, c.fi))
    assert not loss.requires_grad and loss.grad_fn is None  # nothing asked for a gradient


@pytest.mark.gpu
@pytest.mark.parametrize("pert", [0, 1])
@pytest.mark.parametrize("shape", PARITY_SHAPES, ids=_shape_id)
def test_loss_and_gradients_equal_calculate_rigidity_loss(cuda, shape, pert):
    c = _case(shape, cuda)
    cur = _perturbed(c, pert, cuda)

    def run(with_state, grads=(True, True)):
        p = dict(cur, means=cur["means"].detach().clone().requires_grad_(grads[0]),
                 rotation_quaternions=cur["rotation_quaternions"].detach().clone().requires_grad_(grads[1]))
        if with_state:
            loss, st = R.calculate_rigidity_loss_and_state(p, c.ni, c.fi)
        else:
            loss, st = R.calculate_rigidity_loss(p, c.ni, c.fi), None
        (2.5 * loss).backward()
        return loss.detach(), p["means"].grad, p["rotation_quaternions"].grad, st

    l0, m0, q0, _ = run(False)
    l1, m1, q1, st = run(True)
    assert float(l0) > 0 and m0.abs().max() > 0 and q0.abs().max() > 0
    assert _same_bits(l1, l0) and _same_bits(m1, m0) and _same_bits(q1, q0)
    # the state is not differentiable: it requires no gradient and receives none
    for t in (st.inverted_rotations, st.packed_offsets, st.offsets_to_neighbors):
        assert not t.requires_grad and t.grad_fn is None and t.grad is None
    alone = R.foreground_info(cur, c.ni)
    assert _same_bits(st.inverted_rotations, alone.inverted_rotations)
    assert _same_bits(st.packed_offsets, alone.packed_offsets)
    # gradient routing as in calculate_rigidity_loss
    l2, m2, q2, _ = run(True, grads=(True, False))
    assert q2 is None and _same_bits(m2, m0) and _same_bits(l2, l0)
    l3, m3, q3, _ = run(True, grads=(False, True))
    assert m3 is None and _same_bits(q3, q0) and _same_bits(l3, l0)


@pytest.mark.gpu
def test_errors(cuda):
    c = _case((400, 257, 20), cuda)
    fewer = {n: v[:300] for n, v in c.params.items()}
    with pytest.raises(ValueError):
        R.foreground_info(fewer, c.ni)
    with pytest.raises(ValueError):
        R.calculate_rigidity_loss_and_state(fewer, c.ni, c.fi)
    short = SimpleNamespace(inverted_rotations=c.fi.inverted_rotations,
                            offsets_to_neighbors=c.fi.offsets_to_neighbors[:, :4])
    with pytest.raises(ValueError):
        R.calculate_rigidity_loss_and_state(c.params, c.ni, short)
    bad = c.ni.indices.clone()
    bad[3, 2] = c.F
    with pytest.raises(ValueError, match="outside"):  # a bare object is validated when it is packed
        R.foreground_info(c.params, SimpleNamespace(indices=bad, weights=c.ni.weights))
    bare = SimpleNamespace(indices=c.ni.indices.clone(), weights=c.ni.weights.clone())
    fi = R.foreground_info(c.params, bare)
    assert _same_bits(fi.packed_offsets, c.fi.packed_offsets) and bare._gsr_packed is not None


@pytest.mark.gpu
def test_three_timestep_chain(cuda):
    import splat_scenes as S

    c = _case("golden", cuda)
    P, W, H = c.P, 64, 48
    g = torch.Generator().manual_seed(21)
    base = S.synthetic_cloud(P, 0.05, seed=4, device="cpu")
    cloud = dict(base, **c.cpu)  # the golden means, quaternions and masks; seeded appearance
    views = [splat_train.View(camera_index=v, render_settings=S.render_settings(
                 W, H, S.intrinsics(48.0, W, H), S.look_at(yaw, 0.1, 4.0), device=cuda),
                 image=torch.rand(3, H, W, generator=g).to(cuda), segmentation_mask=None)
             for v, yaw in enumerate((10.0, 200.0))]
    leaves = ("means", "rotation_quaternions")
    prev, fi = splat_train.advance_timestep({n: v.to(cuda) for n, v in cloud.items()}, c.ni)
    assert _same_bits(fi.packed_offsets, c.fi.packed_offsets)
    assert _same_bits(fi.inverted_rotations, c.fi.inverted_rotations)
    prev_cpu = cloud
    for t in range(1, 4):
        cur_cpu = dict(prev_cpu, means=prev_cpu["means"] + 0.003 * torch.randn(P, 3, generator=g),
                       rotation_quaternions=prev_cpu["rotation_quaternions"] + 0.05 * torch.randn(P, 4, generator=g))
        cur = {n: v.to(cuda).requires_grad_(n in leaves) for n, v in cur_cpu.items()}
        out = splat_train.train_step_loss(cur, views, c.ni, fi, next_foreground_info=True)
        assert len(out) == 5 and isinstance(out[4], R.ForegroundInfo)
        plain = splat_train.train_step_loss(cur, views, c.ni, fi)
        assert isinstance(plain, tuple) and len(plain) == 4
        assert all(_same_bits(a.detach(), b.detach()) for a, b in zip(plain, out[:4]))
        out[0].backward()
        assert all(torch.isfinite(cur[n].grad).all() for n in leaves)
        # float64 all the way: the previous cloud's state and this cloud's loss
        inv64, off64 = RR.foreground_info(prev_cpu["means"], prev_cpu["rotation_quaternions"], c.mask, c.ni.indices.cpu())
        want = RR.rigidity_loss(cur_cpu["means"], cur_cpu["rotation_quaternions"], c.mask, c.ni.indices.cpu(),
                                c.ni.weights.cpu(), inv64, off64)
        got = float(out[3].detach()) / len(views)
        rel = abs(got - float(want)) / abs(float(want))
        print(f"timestep {t}: rigidity {got:.9e} float64 {float(want):.9e} rel {rel:.3e}")
        assert rel <= 1e-5
        prev, fi = splat_train.advance_timestep(cur, c.ni, out[4])
        assert fi is out[4] and all(not v.requires_grad for v in prev.values())
        assert all(prev[n].data_ptr() == cur[n].data_ptr() for n in cur)  # detached, not copied
        alone = splat_train.advance_timestep(cur, c.ni)[1]  # the stand-alone route gives the same state
        assert _same_bits(alone.packed_offsets, fi.packed_offsets)
        assert _same_bits(alone.inverted_rotations, fi.inverted_rotations)
        prev_cpu = cur_cpu


@pytest.mark.gpu
def test_no_host_synchronisation(cuda):
    c = _case((400, 257, 20), cuda)
    assert c.ni.packed is not None  # create_neighbor_info packs (and validates) once
    cur = _perturbed(c, 0, cuda)
    cur = dict(cur, means=cur["means"].requires_grad_(True))
    probe = torch.ones(1, device=cuda)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    raises = False
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            probe.item()
        except RuntimeError:
            raises = True
        if raises:
            fi = R.foreground_info(cur, c.ni)
            loss, st = R.calculate_rigidity_loss_and_state(cur, c.ni, fi)
            loss.backward()
            prev, carried = splat_train.advance_timestep(cur, c.ni, st)
            prev, alone = splat_train.advance_timestep(cur, c.ni)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    if not raises:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise for .item() in this torch build")
    assert carried is st and _same_bits(alone.packed_offsets, st.packed_offsets)
    assert torch.isfinite(cur["means"].grad).all()
