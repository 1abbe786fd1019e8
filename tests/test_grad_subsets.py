"""The backward's NULL, accumulate and overwrite outputs against the CPU oracle.

Any of the eight gradient outputs of the backward (include/gsr.h gsr_grads) may be NULL, may be marked
``accumulate`` (old + new) and, through the multi-view entry point, may be a fresh uninitialised array
that the first launch overwrites.  The two per-Gaussian kernels (k_gauss_bwd and k_gauss_bwd_multi,
csrc/gsr_backward.hip) gate their loads and stores on those pointers and bits -- dL/dmeans2D and dL/dSH each
in its own code, the other six outputs in the tail both call (gauss_grads_store) -- and the
Python side keeps matching books (``_C._grad_outputs``, ``needed=``, ``_try_defer``'s targets,
``_run_group``).  Every other parity test requests all eight outputs; here every form is run with subsets
of them (``train_py``: the reference's own call site, train.py:155-163 freezes the Gaussians so only
means3D, rotations and means2D carry a gradient) and compared with the oracle and, bit for bit, with the
run that requests everything: the pointers gate memory traffic only, so no value may depend on which
other outputs exist.

Scene: synthetic_cloud(P = 2999, s0 = 0.03, seed 3) -- not a multiple of 64 or 128, so the tail lanes and
their clamped index are live -- at 96 x 80, focal 80, distance 4, views (yaw, height) = (0, 0), (90, 0.3),
(200, -0.3), the last 40 means moved to y = 40, upstream gradient upstream_grad(80, 96, seed = 1 + view).
The oracle gave, for every kind: pair counts 5567 / 5440 / 5423, 40 Gaussians with radius 0 in all three
views (the moved ones), 137 visible in some views but not all; Gaussians seen by both views of a pair with
different SH clamp masks: 108-148 at SH1, 205-231 at SH2, 238-279 at SH3 (and at the 25-coefficient
generic kind); at SH0 the colour does not depend on the direction, so the masks of two views are equal by
construction (asserted instead).  The nine views of the two-launch case (yaw 0, 40, ..., 320 at height
0.2): 40 never visible, 198 partly visible, 205-296 differing clamp masks per pair.  Each test asserts
its regime from the oracle state before it touches the GPU.

Tolerances are the project's band (test_gpu_parity._close: 1e-4 relative + 1e-5 max|ref|, nothing
outside); the multi-view sums are compared with the float64 sum of the oracle's per-view gradients as
test_c3_summed_step_vs_oracle does.  Accumulated results of the multi-view call are compared with
float64(old) + that sum: the kernel's one fp32 add contributes at most 2^-24 max(|old|, |sum|), two
orders below the band's floor of 1e-5 max|old + sum| (old is random, so that maximum is of the order
of max(|old|, |sum|)).  _close lets NaN through (a NaN
comparison is false), so every compared array is also asserted finite, and rows no view sees are asserted
exactly zero (the oracle's gradient there).
"""
import itertools

import numpy as np
import pytest
import torch

import splat_scenes as S
from diff_gaussian_rasterization import (GaussianRasterizer, _C, pending_views, rasterize_parameters,
                                         set_deferred_backward)
from oracle import oracle as O
from test_gpu_parity import STATS, _close, _gpu_forward, _inputs, _np, _ora_forward  # noqa: F401 -- STATS: the stat dump

gpu = pytest.mark.gpu

P, W, H, FOCAL, S0 = 2999, 96, 80, 80.0, 0.03
VIEWS = ((0.0, 0.0), (90.0, 0.3), (200.0, -0.3))
NINE = tuple((40.0 * k, 0.2) for k in range(9))  # more than kMultiViews = 8: two launches
# kind: (sh_degree, extra stored coefficients)
KINDS = {"rgb": (-1, 0), "sh0": (0, 0), "sh1": (1, 0), "sh2": (2, 0), "sh3": (3, 0), "sh_m25": (3, 9),
         "cov3d": (-1, 0)}
# output slots (the order of gsr_grads) and the oracle's names for them
M2D, COL, OPA, M3D, COV, SH, SCA, ROT = range(8)
REF = ("means2D", "colors", "opacities", "means3D", "cov3D", "sh", "scales", "rotations")
ALL = frozenset(range(8))
SUBSETS = {"all": ALL, "train_py": frozenset((M2D, M3D, ROT)), "means3D": frozenset((M3D,)),
           "colour": frozenset((COL, SH)), "opacity": frozenset((OPA,)), "scales": frozenset((SCA,)),
           "rotations": frozenset((ROT,)), "no_means2D": ALL - {M2D}, "no_colour": ALL - {COL, SH},
           "cov3D": frozenset((COV,)), "means3D+cov3D": frozenset((M3D, COV))}
COV_ONLY = ("cov3D", "means3D+cov3D")


def _present(kind):
    """The slots that exist for a kind (the others come back empty under skip_unused)."""
    if kind == "cov3d":
        return frozenset((M2D, COL, OPA, M3D, COV))
    if kind == "rgb":
        return frozenset((M2D, COL, OPA, M3D, SCA, ROT))
    return frozenset((M2D, OPA, M3D, SH, SCA, ROT))


def _shape(kind, k):
    M = (KINDS[kind][0] + 1) ** 2 + KINDS[kind][1] if KINDS[kind][0] >= 0 else 0
    return ((P, 3), (P, 3), (P, 1), (P, 3), (P, 6), (P, M, 3), (P, 3), (P, 4))[k]


def _same_bits(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


# ---- the scene, its oracle state (computed once per kind, never modified) and its GPU forwards --------
_ORACLE, _GPU = {}, {}


def _scene(kind, views):
    deg, extra = KINDS[kind]
    a, cams = None, []
    for yaw, h in views:
        ai, rs = _inputs(P, W, H, FOCAL, S0, seed=3, sh_degree=deg, yaw=yaw, height=h, distance=4.0,
                         extra_coeffs=extra)
        a = ai if a is None else a
        cams.append(rs)
    a["means3D"] = a["means3D"].clone()
    a["means3D"][-40:, 1] = 40.0  # far outside every frustum: radius 0 in every view
    cov = None
    if kind == "cov3d":
        from oracle import dense_torch as DT
        cov = DT.cov3d_from(a["scales"].double(), a["rotations"].double(), 1.0).float()
    return a, cams, cov


def _oracle(kind, views=VIEWS):
    key = (kind, views)
    if key not in _ORACLE:
        a, cams, cov = _scene(kind, views)
        sts = [_ora_forward(a, rs, cov3D=cov) for rs in cams]
        dls = [S.upstream_grad(H, W, seed=1 + v, device="cpu") for v in range(len(cams))]
        grefs = [O.backward(st, dl.numpy()) for st, dl in zip(sts, dls)]
        vis = np.stack([st["radii"] > 0 for st in sts])
        _ORACLE[key] = dict(a=a, cams=cams, cov=cov, sts=sts, dls=dls, grefs=grefs, vis=vis,
                            never=~vis.any(0))
    return _ORACLE[key]


def _sum_ref(ora, name, views=None):
    """float64 sum over the views of the oracle's per-view gradient."""
    vs = range(len(ora["grefs"])) if views is None else views
    return sum(ora["grefs"][v][name].astype(np.float64) for v in vs)


def _assert_regime(kind, ora):
    vis, sts = ora["vis"], ora["sts"]
    never = int(ora["never"].sum())
    some = int((vis.any(0) & ~vis.all(0)).sum())
    assert never >= 32 and not vis[:, -40:].any(), never
    assert some >= 50, some
    if KINDS[kind][0] == 0:  # SH0: no direction dependence, the masks cannot differ
        for u, v in itertools.combinations(range(len(sts)), 2):
            both = vis[u] & vis[v]
            assert np.array_equal(sts[u]["clamped"][both], sts[v]["clamped"][both])
    elif KINDS[kind][0] > 0:
        diff = max(int((vis[u] & vis[v] & (sts[u]["clamped"] != sts[v]["clamped"]).any(1)).sum())
                   for u, v in itertools.combinations(range(len(sts)), 2))
        assert diff >= 50, diff


def _gpu(kind, dev, views=VIEWS):
    """Device copies of a kind's inputs, cameras and upstream gradients and ONE forward per view, shared by
    every subset (the backward calls read the forward's buffers, they do not write them)."""
    key = (kind, views)
    if key not in _GPU:
        ora = _oracle(kind, views)
        _assert_regime(kind, ora)
        a, cov = ora["a"], ora["cov"]
        e = torch.empty(0, device=dev)
        d = lambda k: a[k].to(dev) if a.get(k) is not None else e  # noqa: E731
        t = dict(means3D=d("means3D"), colors=d("colors_precomp"), opacities=d("opacities"),
                 scales=e if cov is not None else d("scales"), rotations=e if cov is not None else d("rotations"),
                 cov=cov.to(dev) if cov is not None else e, shs=d("shs"))
        cams = [rs._replace(bg=rs.bg.to(dev), viewmatrix=rs.viewmatrix.to(dev), projmatrix=rs.projmatrix.to(dev),
                            campos=rs.campos.to(dev)) for rs in ora["cams"]]
        fws = [_gpu_forward(a, rs, dev, cov3D=cov) for rs in ora["cams"]]
        for f, st in zip(fws, ora["sts"]):
            np.testing.assert_array_equal(_np(f["radii"]), st["radii"])
            assert f["K"] == st["num_rendered"]
        _GPU[key] = dict(t=t, cams=cams, fws=fws, dls=[dl.to(dev) for dl in ora["dls"]], sums={}, single={})
    return _GPU[key]


def _poison(kind, dev):
    """Best effort: NaN-filled tensors of the eight output shapes, freed at once, so that the caching
    allocator hands the next torch.empty of those sizes NaN instead of the zeros fresh device memory
    usually holds (a skipped zero fill of an invisible row then shows).  Nothing guarantees the reuse;
    the multi-view tests below check the same contract deterministically (overwrite into NaN)."""
    ts = [torch.full(_shape(kind, k), float("nan"), device=dev) for k in range(8) if _shape(kind, k)[1]]
    del ts


def _backward1(kind, dev, v, want, accumulate_into=None):
    """gsr_backward of view `v` with the outputs `want` (slot indices) requested."""
    G = _gpu(kind, dev)
    t, c, f = G["t"], G["cams"][v], G["fws"][v]
    out = _C.rasterize_gaussians_backward(
        c.bg, t["means3D"], f["radii"], t["colors"], t["scales"], t["rotations"], c.scale_modifier, t["cov"],
        c.viewmatrix, c.projmatrix, c.tanfovx, c.tanfovy, G["dls"][v], t["shs"], c.sh_degree, c.campos,
        f["geom"], f["K"], f["binning"], f["img"], skip_unused=True, needed=[k in want for k in range(8)],
        accumulate_into=accumulate_into)
    torch.cuda.synchronize()
    return out


def _single(kind, dev, subset, route, v=0):
    """The single-view run of a subset under a marshalling route (cached: the `all` run is what every other
    subset, the accumulate cases and the multi-view means2D arrays are compared with)."""
    G = _gpu(kind, dev)
    key = (subset, route, v)
    if key not in G["single"]:
        if subset in ("all", "train_py"):
            _poison(kind, dev)
        G["single"][key] = _backward1(kind, dev, v, SUBSETS[subset])
    return G["single"][key]


@pytest.fixture(params=[0, 15], ids=["ctypes", "native"])
def route(request):
    """Both marshalling routes of the binding: _C.py's ctypes calls and gsr_bind."""
    prev = _C._NATIVE_PARTS
    if _C._native() is None and request.param:
        pytest.skip("gsr_bind.so not built")
    _C._NATIVE_PARTS = request.param
    yield request.param
    _C._NATIVE_PARTS = prev


def _check_slots(kind, tag, out, want, ref_of, never, same_as=None):
    """Unrequested slots None, absent ones empty, the others finite, exactly zero where no view sees the
    Gaussian, inside the band against ref_of(name) and (same_as) bitwise another run's."""
    present = _present(kind)
    for k in range(8):
        if k not in want:
            assert out[k] is None, (tag, REF[k])
        elif k not in present:
            assert out[k] is not None and out[k].numel() == 0, (tag, REF[k])
        else:
            assert out[k] is not None and tuple(out[k].shape) == _shape(kind, k), (tag, REF[k])
            assert torch.isfinite(out[k]).all(), (tag, REF[k])
            assert not out[k][torch.from_numpy(never).to(out[k].device)].any(), (tag, REF[k])
            _close(f"{tag} {REF[k]}", _np(out[k]), ref_of(REF[k]))
            if same_as is not None:
                assert _same_bits(out[k], same_as[k]), (tag, REF[k])


def _kind_subsets(kinds, subsets):
    return [(k, s) for k in kinds for s in subsets if (s not in COV_ONLY or k == "cov3d")]


# ---- 1. single view, C ABI level --------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,subset", _kind_subsets(KINDS, SUBSETS))
def test_single_view_subsets(kind, subset, route, cuda):
    """gsr_backward with NULL outputs (needed=) under both marshalling routes: every requested slot in band
    against the oracle's view 0 and bitwise the slot of the run that requests all eight."""
    ora = _oracle(kind)
    full = _single(kind, cuda, "all", route)
    out = _single(kind, cuda, subset, route)
    _check_slots(kind, f"{kind}/{subset}", out, SUBSETS[subset], lambda n: ora["grefs"][0][n], ora["never"], full)


# ---- 1b. accumulate targets, guard rows, one unaligned target ----------------------------------------
@gpu
@pytest.mark.parametrize("subset", ["all", "train_py"])
@pytest.mark.parametrize("kind", ["rgb", "sh1", "sh3", "cov3d"])
def test_single_view_accumulate_guards(kind, subset, route, cuda):
    """Each requested slot accumulates into rows [64 : 64 + P] of a (P + 128, ...) buffer of random old
    values (64 rows keep every slot's start 256-byte aligned): the guard rows stay bitwise unchanged, the
    interior is bitwise old + g (torch's add on the GPU, the equality test_accumulate.py relies on) with
    g the plain run's gradient, unrequested slots stay None."""
    want = SUBSETS[subset]
    g1 = _single(kind, cuda, subset, route)
    gen = torch.Generator().manual_seed(7)
    bufs, acc = {}, [None] * 8
    for k in sorted(want & _present(kind)):
        shp = _shape(kind, k)
        bufs[k] = (1e-2 * torch.randn((P + 128,) + shp[1:], generator=gen)).to(cuda)
        acc[k] = bufs[k][64:64 + P]
        assert acc[k].is_contiguous() and acc[k].data_ptr() % 256 == 0
    old = {k: b.clone() for k, b in bufs.items()}
    out = _backward1(kind, cuda, 0, want, accumulate_into=acc)
    for k in range(8):
        if k not in want:
            assert out[k] is None, REF[k]
        elif k not in bufs:
            assert out[k].numel() == 0, REF[k]
        else:
            assert out[k].data_ptr() == acc[k].data_ptr(), REF[k]
            assert _same_bits(bufs[k][:64], old[k][:64]) and _same_bits(bufs[k][64 + P:], old[k][64 + P:]), REF[k]
            assert _same_bits(bufs[k][64:64 + P], old[k][64:64 + P] + g1[k]), REF[k]


@gpu
@pytest.mark.parametrize("kind,slot", [("sh0", SH), ("sh1", SH), ("sh2", SH), ("sh3", SH), ("sh_m25", SH),
                                       ("rgb", M3D)])
def test_single_view_unaligned_target(kind, slot, cuda):
    """An accumulate target four bytes off 16-byte alignment (buf[1 : 1 + n] of a flat buffer, one guard
    float either side).  Every store to the eight outputs is a scalar store (gput, gput_old, sh_backward)
    or checks its destination's alignment (sh_rows_from_lds, whose block offsets are multiples of four
    floats, so every block of this target takes its scalar branch): the result is bitwise the aligned
    target's and the guards are untouched."""
    shp = _shape(kind, slot)
    n = int(np.prod(shp))
    old = 1e-2 * torch.randn(n + 2, generator=torch.Generator().manual_seed(11))
    buf = old.to(cuda)
    tgt = buf[1:1 + n].view(shp)
    ali = old[1:1 + n].to(cuda).view(shp)
    assert tgt.data_ptr() % 16 == 4 and ali.data_ptr() % 16 == 0 and tgt.is_contiguous()
    for t in (tgt, ali):
        acc = [None] * 8
        acc[slot] = t
        out = _backward1(kind, cuda, 0, frozenset((slot,)), accumulate_into=acc)
        assert out[slot].data_ptr() == t.data_ptr() and all(out[k] is None for k in range(8) if k != slot)
    assert _same_bits(tgt, ali)
    assert not _same_bits(ali, old[1:1 + n].to(cuda).view(shp))  # the gradient was added
    assert _same_bits(buf[:1], old[:1].to(cuda)) and _same_bits(buf[-1:], old[-1:].to(cuda))
    _close(f"{kind}/unaligned {REF[slot]}", _np(tgt), old[1:1 + n].view(shp).double().numpy() +
           _oracle(kind)["grefs"][0][REF[slot]].astype(np.float64))


# ---- 2. multi-view, C ABI level ----------------------------------------------------------------------
MULTI_KINDS = [k for k in KINDS if k != "sh_m25"]
MULTI_SUBSETS = ["all", "train_py", "colour", "opacity", "scales", "rotations", "no_colour"]


def _render_half(G, v):
    """The view's SUMS buffer (gsr_backward_render), computed once: the per-Gaussian call only reads it."""
    if v not in G["sums"]:
        t, c, f = G["t"], G["cams"][v], G["fws"][v]
        G["sums"][v] = _C.rasterize_gaussians_backward_render(
            c.bg, t["means3D"], f["radii"], t["colors"], t["scales"], t["rotations"], c.scale_modifier, t["cov"],
            c.viewmatrix, c.projmatrix, c.tanfovx, c.tanfovy, G["dls"][v], t["shs"], c.sh_degree, c.campos,
            f["geom"], f["K"], f["binning"], f["img"])
    return G["sums"][v]


def _views_call(kind, dev, want, m2=None, views=VIEWS, accumulate_into=None, overwrite=(), only=None):
    """gsr_backward_gaussians over the views (only: the indices of those passed, default all); m2: per view
    None or (array, accumulate_means2D)."""
    G = _gpu(kind, dev, views)
    t = G["t"]
    vs = []
    for v, (c, f) in enumerate(zip(G["cams"], G["fws"])):
        if only is not None and v not in only:
            continue
        d = {"viewmatrix": c.viewmatrix, "projmatrix": c.projmatrix, "tanfovx": c.tanfovx, "tanfovy": c.tanfovy,
             "image_height": H, "image_width": W, "campos": c.campos, "bg": c.bg, "radii": f["radii"],
             "geomBuffer": f["geom"], "scratch": _render_half(G, v), "num_rendered": f["K"]}
        if m2 is not None and m2[v] is not None:
            d["means2D_grad"], d["accumulate_means2D"] = m2[v]
        vs.append(d)
    out = _C.rasterize_gaussians_backward_views(
        vs, t["means3D"], t["colors"], t["scales"], t["rotations"], G["cams"][0].scale_modifier, t["cov"], t["shs"],
        G["cams"][0].sh_degree, skip_unused=True, accumulate_into=accumulate_into, overwrite=overwrite,
        needed=[k in want for k in range(8)])
    torch.cuda.synchronize()
    return out


def _nan(shape, dev):
    return torch.full(shape, float("nan"), device=dev)


@gpu
@pytest.mark.parametrize("kind,subset", _kind_subsets(MULTI_KINDS, MULTI_SUBSETS))
def test_multi_view_subsets(kind, subset, cuda):
    """gsr_backward_gaussians over three views with NULL outputs: plain, overwriting NaN-filled fresh
    targets (finite, in band, bitwise the plain run) and accumulating into old values; views 0 and 2
    write their own means2D arrays (bitwise the single-view call's), view 1 has none."""
    ora = _oracle(kind)
    want = SUBSETS[subset]
    slots = sorted((want - {M2D}) & _present(kind))
    sums = lambda n: _sum_ref(ora, n)  # noqa: E731
    never = ora["never"]

    def m2_arrays():
        return [(_nan((P, 3), cuda), False), None, (_nan((P, 3), cuda), False)] if M2D in want else None

    def check_m2(m2):
        if m2 is None:
            return
        for v in (0, 2):
            ref = _single(kind, cuda, "all", _C._NATIVE_PARTS, v)[M2D]
            assert _same_bits(m2[v][0], ref), (kind, subset, v)  # the record sums themselves: exact

    m2 = m2_arrays()
    plain = _views_call(kind, cuda, want, m2)
    _check_slots(kind, f"multi {kind}/{subset}", plain, want - {M2D}, sums, never)
    check_m2(m2)
    # overwrite: fresh gradients (NaN) written without being read
    tg = [None] * 8
    for k in slots:
        tg[k] = _nan(_shape(kind, k), cuda)
    m2 = m2_arrays()
    over = _views_call(kind, cuda, want, m2, accumulate_into=tg, overwrite=tuple(slots))
    for k in slots:
        assert over[k].data_ptr() == tg[k].data_ptr()
    _check_slots(kind, f"multi-overwrite {kind}/{subset}", over, want - {M2D}, sums, never, plain)
    check_m2(m2)
    # accumulate: old + sum
    gen = torch.Generator().manual_seed(13)
    old = {k: 1e-2 * torch.randn(_shape(kind, k), generator=gen) for k in slots}
    tg = [None] * 8
    for k in slots:
        tg[k] = old[k].to(cuda)
    accd = _views_call(kind, cuda, want, m2_arrays(), accumulate_into=tg)
    for k in range(1, 8):
        if k not in want:
            assert accd[k] is None, REF[k]
        elif k in old:
            assert accd[k].data_ptr() == tg[k].data_ptr() and torch.isfinite(accd[k]).all(), REF[k]
            nv = torch.from_numpy(never)
            assert _same_bits(accd[k].cpu()[nv], old[k][nv]), REF[k]  # no view sees them: content kept
            _close(f"multi-accumulate {kind}/{subset} {REF[k]}", _np(accd[k]),
                   old[k].double().numpy() + sums(REF[k]))


@gpu
@pytest.mark.parametrize("kind", MULTI_KINDS)
def test_one_view_launch_equals_single_view(kind, cuda):
    """gsr_backward_gaussians over view 0 alone against gsr_backward of view 0, all eight outputs on both
    routes.  Both kernels add the view's records in emission order, run the same chains on the sums and
    store through one tail (gauss_grads_store), and k_gauss_bwd_multi adds its single view's values to +0:
    every output is equal in value (torch.equal, not the bit patterns: a zero's sign may differ).  Plain,
    the launch writing means2D into a NaN-filled array, and accumulating into the same random old values."""
    ora = _oracle(kind)
    assert P % 128 and int((~ora["vis"][0]).sum()) >= 40  # live tail lanes, rows of radius 0
    one = _single(kind, cuda, "all", _C._NATIVE_PARTS)
    m2 = [(_nan((P, 3), cuda), False), None, None]
    out = _views_call(kind, cuda, ALL, m2, only=(0,))
    assert out[M2D] is None
    for k in range(8):
        got = m2[0][0] if k == M2D else out[k]
        assert got.shape == one[k].shape and torch.equal(got, one[k]), (kind, REF[k])
    gen = torch.Generator().manual_seed(17)
    old = {k: 1e-2 * torch.randn(_shape(kind, k), generator=gen) for k in sorted(_present(kind))}
    acc1 = [old[k].to(cuda) if k in old else None for k in range(8)]
    accv = [old[k].to(cuda) if k in old and k != M2D else None for k in range(8)]
    m2 = [(old[M2D].to(cuda), True), None, None]
    one = _backward1(kind, cuda, 0, ALL, accumulate_into=acc1)
    out = _views_call(kind, cuda, ALL, m2, accumulate_into=accv, only=(0,))
    for k in range(8):
        got = m2[0][0] if k == M2D else out[k]
        assert got.shape == one[k].shape and torch.equal(got, one[k]), (kind, "accumulate", REF[k])
        if k in old:
            assert one[k].data_ptr() == acc1[k].data_ptr() and not torch.equal(one[k].cpu(), old[k]), REF[k]


@gpu
@pytest.mark.parametrize("kind", MULTI_KINDS)
def test_multi_view_shared_means2D(kind, cuda):
    """Views 0 and 2 share one means2D array: the first is written with accumulate_means2D = False into NaN
    (whichever of the two the launch sums first overwrites), the second accumulates."""
    ora = _oracle(kind)
    shared = _nan((P, 3), cuda)
    out = _views_call(kind, cuda, SUBSETS["train_py"], [(shared, False), None, (shared, True)])
    _check_slots(kind, f"multi-shared {kind}", out, SUBSETS["train_py"] - {M2D}, lambda n: _sum_ref(ora, n), ora["never"])
    assert torch.isfinite(shared).all() and not shared[torch.from_numpy(ora["never"]).to(cuda)].any()
    _close(f"multi-shared {kind} means2D", _np(shared), _sum_ref(ora, "means2D", (0, 2)))


@gpu
def test_multi_view_generic_sh_count_unsupported(cuda):
    """25 stored coefficients: the multi-view pass has no generic-count instantiation and says so."""
    G = _gpu("sh_m25", cuda)
    t, c, f = G["t"], G["cams"][0], G["fws"][0]
    view = {"viewmatrix": c.viewmatrix, "projmatrix": c.projmatrix, "tanfovx": c.tanfovx, "tanfovy": c.tanfovy,
            "image_height": H, "image_width": W, "campos": c.campos, "bg": c.bg, "radii": f["radii"],
            "geomBuffer": f["geom"], "scratch": _render_half(G, 0), "num_rendered": f["K"]}
    with pytest.raises(RuntimeError, match="SH coefficients"):
        _C.rasterize_gaussians_backward_views([view], t["means3D"], t["colors"], t["scales"], t["rotations"], 1.0,
                                              t["cov"], t["shs"], 3)
    torch.cuda.synchronize()


@gpu
def test_multi_view_two_launches_overwrite_with_null_outputs(cuda):
    """Nine views (two launches of <= kMultiViews = 8), SH3, the train.py subset, every target a fresh
    NaN-filled array: the first launch overwrites, the second adds (its accumulate bits forced on) while
    the unrequested outputs stay NULL in both; every view's own means2D array is overwritten."""
    ora = _oracle("sh3", NINE)
    want = SUBSETS["train_py"]
    tg = [None] * 8
    tg[M3D], tg[ROT] = _nan((P, 3), cuda), _nan((P, 4), cuda)
    m2 = [(_nan((P, 3), cuda), False) for _ in NINE]
    out = _views_call("sh3", cuda, want, m2, views=NINE, accumulate_into=tg, overwrite=(M3D, ROT))
    assert out[M3D].data_ptr() == tg[M3D].data_ptr() and out[ROT].data_ptr() == tg[ROT].data_ptr()
    _check_slots("sh3", "multi-nine sh3/train_py", out, want - {M2D}, lambda n: _sum_ref(ora, n), ora["never"])
    nv = torch.from_numpy(ora["never"]).to(cuda)
    for v, (arr, _) in enumerate(m2):
        assert torch.isfinite(arr).all() and not arr[nv].any(), v
        _close(f"multi-nine view {v} means2D", _np(arr), ora["grefs"][v]["means2D"])


# ---- 3. autograd level -------------------------------------------------------------------------------
# input names of the module path per output slot, and of rasterize_parameters' raw parameters
MOD_NAMES = {M2D: "means2D", COL: "colors_precomp", OPA: "opacities", M3D: "means3D", COV: "cov3D_precomp",
             SH: "shs", SCA: "scales", ROT: "rotations"}
RAW_NAMES = {M2D: "means2D", COL: "colors", OPA: "opacity_logits", M3D: "means", SH: "shs", SCA: "log_scales",
             ROT: "rotation_quaternions"}
AUTO_SUBSETS = ["train_py", "means3D", "colour", "opacity", "no_means2D"]
WAYS = ["deferred", "immediate", "nonleaf"]
_AUTO = {}


def _auto_inputs(path, kind, dev):
    """name -> device tensor of the path's inputs (module: activated; params: raw parameters), and the
    slot of each name."""
    G = _gpu(kind, dev)
    if path == "module":
        t = G["t"]
        src = {COL: t["colors"], OPA: t["opacities"], M3D: t["means3D"], COV: t["cov"], SH: t["shs"],
               SCA: t["scales"], ROT: t["rotations"]}
        names = {k: MOD_NAMES[k] for k, v in src.items() if v.numel()}
        vals = {names[k]: src[k] for k in names}
    else:
        deg = KINDS[kind][0]
        p = S.synthetic_cloud(P, S0, sh_degree=deg, seed=3, device="cpu")
        p["means"][-40:, 1] = 40.0
        if deg >= 0:
            p.pop("colors")
        names = {k: n for k, n in RAW_NAMES.items() if n in p}
        vals = {n: p[n].to(dev) for n in names.values()}
    names[M2D] = "means2D"
    vals["means2D"] = torch.zeros(P, 3, device=dev)
    return names, vals


def _auto_run(path, kind, way, live, dev):
    """Three views, the losses summed before ONE backward; `live`: the names that require grad.  Returns
    name -> .grad (None for frozen leaves)."""
    G = _gpu(kind, dev)
    names, vals = _auto_inputs(path, kind, dev)
    leaves = {n: v.detach().clone().requires_grad_(n in live) for n, v in vals.items()}
    if way == "nonleaf":  # the reference's call shape: activated tensors computed from the parameters
        args = {n: (v * 1.0 if v.requires_grad else v) for n, v in leaves.items()}
    else:
        args = leaves
    prev = set_deferred_backward(way != "immediate")
    try:
        imgs = []
        for c in G["cams"]:
            if path == "module":
                imgs.append(GaussianRasterizer(raster_settings=c)(**args)[0])
            else:
                params = {n: v for n, v in args.items() if n not in ("means2D", "shs")}
                params.setdefault("colors", None)
                imgs.append(rasterize_parameters(params, c, means2D=args["means2D"] if "means2D" in live else None,
                                                 shs=args.get("shs"))[0])
        sum((img * dl).sum() for img, dl in zip(imgs, G["dls"])).backward()
    finally:
        set_deferred_backward(prev)
    torch.cuda.synchronize()
    assert pending_views() == 0
    return {n: v.grad for n, v in leaves.items()}


def _live_names(names, subset):
    want = SUBSETS[subset]
    return {n for k, n in names.items() if k in want}


@gpu
@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("subset", AUTO_SUBSETS)
@pytest.mark.parametrize("path,kind", [("module", "rgb"), ("module", "sh3"), ("module", "cov3d"),
                                       ("params", "rgb"), ("params", "sh3")])
def test_autograd_subsets(path, kind, subset, way, cuda):
    """GaussianRasterizer / rasterize_parameters with frozen inputs, as leaves with the deferred multi-view
    pass, as leaves without it, and as non-leaf inputs: frozen leaves get no .grad, no view stays queued,
    every live gradient is bitwise the all-live run's of the same path and way, and (module path) in band
    against the oracle's sum.  rasterize_parameters' all-live run is pinned by
    test_fused_parameters_parity; its subset runs are tied to it bitwise."""
    ora = _oracle(kind)
    key = (path, kind, way)
    names, _ = _auto_inputs(path, kind, cuda)
    if key not in _AUTO:
        _AUTO[key] = _auto_run(path, kind, way, set(names.values()), cuda)
        assert all(g is not None for g in _AUTO[key].values()), key
    full = _AUTO[key]
    live = _live_names(names, subset)
    assert live, (path, kind, subset)
    grads = _auto_run(path, kind, way, live, cuda)
    nv = torch.from_numpy(ora["never"]).to(cuda)
    for k, n in names.items():
        if n not in live:
            assert grads[n] is None, n
            continue
        assert grads[n] is not None and torch.isfinite(grads[n]).all(), n
        assert not grads[n][nv].any(), n
        assert _same_bits(grads[n], full[n]), (path, kind, subset, way, n)
        if path == "module":
            _close(f"autograd {kind}/{subset}/{way} {n}", _np(grads[n]), _sum_ref(ora, REF[k]))


@gpu
def test_autograd_generic_sh_count_falls_back_to_immediate(cuda):
    """25 stored SH coefficients as leaves with deferral on: _try_defer declines (no multi-view
    instantiation), the immediate per-view path runs and the gradients are in band."""
    ora = _oracle("sh_m25")
    names, _ = _auto_inputs("module", "sh_m25", cuda)
    grads = _auto_run("module", "sh_m25", "deferred", set(names.values()), cuda)
    for k, n in names.items():
        assert grads[n] is not None and torch.isfinite(grads[n]).all(), n
        _close(f"autograd sh_m25 {n}", _np(grads[n]), _sum_ref(ora, REF[k]))


# ---- 4. the binding's output bookkeeping (CPU) --------------------------------------------------------
@pytest.mark.parametrize("skip", [(), (0,), (1, 2, 4, 5, 6), tuple(range(8))])
def test_grad_outputs_bookkeeping(skip):
    """_C._grad_outputs on CPU tensors (no accumulate_into: recording its stream needs a GPU): `skip` gives
    None in exactly those slots, skip_unused gives (0,) shapes for absent colours, cov3D and
    scales / rotations, and nothing is marked accumulate."""
    n, M = 7, 4
    cpu = torch.device("cpu")
    col, cov, sc, rot = torch.zeros(n, 3), torch.zeros(n, 6), torch.zeros(n, 3), torch.zeros(n, 4)
    e = torch.empty(0)
    full = [(n, 3), (n, 3), (n, 1), (n, 3), (n, 6), (n, M, 3), (n, 3), (n, 4)]
    cases = [  # (colours, cov3D, scales, rotations, skip_unused) -> slots that shrink to (0,)
        ((col, cov, sc, rot, True), ()),
        ((e, e, sc, rot, True), (1, 4)),
        ((None, None, sc, rot, True), (1, 4)),
        ((col, cov, e, e, True), (6, 7)),
        ((col, cov, sc, e, True), (6, 7)),
        ((e, e, e, e, False), ()),
    ]
    for (c, v, s, r, unused), empty in cases:
        out, bits = _C._grad_outputs(n, M, cpu, c, v, s, r, unused, None, skip=skip)
        assert bits == 0 and len(out) == 8
        for k in range(8):
            if k in skip:
                assert out[k] is None, (k, skip)
            else:
                assert out[k] is not None and out[k].dtype == torch.float32, (k, skip)
                assert tuple(out[k].shape) == ((0,) if k in empty else full[k]), (k, empty)
