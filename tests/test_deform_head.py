"""The deformation network's output head (splat_deform.deform_output_layer, csrc/gsr_head.hip): fc_out and the
``+ [initial means | initial quaternions]`` update in one kernel, with its backward.

CPU: the exports, the argument validation, the untouched state_dict and torch lines.
GPU: the kernels against the float64 restatement.  The yardstick is the float32 torch composition's own worst
error against float64 on the same device and inputs; the kernel may have the project band
(1e-4 |ref| + 1e-6 max|ref|) or twice that yardstick, whichever is larger.  "Golden band": 2e-4 |ref| +
2e-5 max|ref| for values the reference saved in fp32.
"""
import ctypes
import functools
import itertools
import os

import pytest
import torch
import torch.nn.functional as F

import deform_ref as DR
import splat_deform as D
from deform_ref import band, yardstick
from diff_gaussian_rasterization import _C
from test_deform import GOLD, _clouds, _gold_clouds, _gold_progress, _gold_state, _t, _to

CASES = [(1, 64), (63, 64), (65, 1), (130, 129), (257, 128), (1031, 7), (1031, 40), (4099, 64), (257, 512)]


@functools.lru_cache(maxsize=None)
def _head(P, H):
    """Seeded x, fc_out weight and bias and upstream gradient of a (P, H) case, on the CPU."""
    g = torch.Generator().manual_seed(11 * P + H)
    bound = 1 / H ** 0.5  # nn.Linear's initialisation range
    return (torch.randn(P, H, generator=g), (torch.rand(7, H, generator=g) * 2 - 1) * bound,
            (torch.rand(7, generator=g) * 2 - 1) * bound, torch.randn(P, 7, generator=g))


@functools.lru_cache(maxsize=None)
def _case(P, H):
    """The case on the GPU with its float32 torch and float64 results: computed once, shared, never changed."""
    dev = torch.device("cuda:0")
    x, w, b, up = (t.to(dev) for t in _head(P, H))
    initial = _to(_clouds(P)[0], dev)
    base = torch.cat((initial["means"], initial["rotation_quaternions"]), dim=1)
    ref = {}
    for dtype in (torch.float32, torch.float64):
        xd, wd, bd, ud = (t.to(dtype) for t in (x, w, b, up))
        ref[dtype] = {"out": F.linear(xd, wd, bd) + base.to(dtype), "dx": ud @ wd, "dw": ud.t() @ xd, "db": ud.sum(0)}
    return x, w, b, up, initial, ref[torch.float32], ref[torch.float64]


def _run(x, w, b, up, initial, max_blocks, need=(True, True, True)):
    """One forward + backward; the output and the gradients of (x, weight, bias), None where not required."""
    leaves = [t.clone().requires_grad_(n) for t, n in zip((x, w, b), need)]
    out = D.deform_output_layer(*leaves, initial, max_blocks=max_blocks)
    out.backward(up)
    return (out.detach(),) + tuple(t.grad for t in leaves)


# ---- CPU ------------------------------------------------------------------------------------------
def test_contract():
    assert "deform_output_layer" in D.__all__ and "set_fused_output_head" in D.__all__
    P, H = 5, 32
    x, w, b = torch.zeros(P, H), torch.zeros(7, H), torch.zeros(7)
    init = {"means": torch.zeros(P, 3), "rotation_quaternions": torch.zeros(P, 4)}
    bad = [
        (x, torch.zeros(6, H), b, init, {}),
        (x, torch.zeros(7, H + 1), b, init, {}),
        (x, w, torch.zeros(6), init, {}),
        (x, w, torch.zeros(7, 1), init, {}),
        (torch.zeros(P, 0), torch.zeros(7, 0), b, init, {}),
        (torch.zeros(P, 513), torch.zeros(7, 513), b, init, {}),
        (torch.zeros(P, H, dtype=torch.float64), w, b, init, {}),
        (x, w.double(), b, init, {}),
        (x, w, b.double(), init, {}),
        (torch.zeros(H), w, b, init, {}),
        (x, w, b, {"means": torch.zeros(P + 1, 3), "rotation_quaternions": torch.zeros(P + 1, 4)}, {}),
        (x, w, b, {"means": torch.zeros(P, 3), "rotation_quaternions": torch.zeros(P, 3)}, {}),
        (x, w, b, {"means": torch.zeros(P, 3, dtype=torch.float64), "rotation_quaternions": torch.zeros(P, 4)}, {}),
        (x, w, b, init, {"max_blocks": -1}),
    ]
    for xa, wa, ba, ia, kw in bad:
        with pytest.raises(ValueError, match="deform_output_layer"):
            D.deform_output_layer(xa, wa, ba, ia, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.deform_output_layer(x, w, b, init)
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.deform_output_layer(torch.zeros(P, 512), torch.zeros(7, 512), b, init, max_blocks=2)

    first = D.set_fused_output_head(False)
    try:
        assert first is True  # the default
        assert D.set_fused_output_head(True) is False
        assert D.set_fused_output_head(True) is True
    finally:
        D.set_fused_output_head(first)
    assert D.set_fused_output_head(first) is first


def test_state_dict_and_torch_lines_untouched(monkeypatch):
    net = D.DeformationNetwork(32, 1)
    state = net.state_dict()
    assert list(state.keys()) == [str(n) for n in GOLD["state_names"]]
    for name, shape in zip(GOLD["state_names"], GOLD["state_shapes"]):
        assert tuple(state[str(name)].shape) == tuple(int(d) for d in str(shape).split(",") if d), name

    # the tail on CPU tensors: the input layer and the blocks replaced, fc_out and the addition as they are
    P, H = 37, 32
    g = torch.Generator().manual_seed(3)
    act = torch.randn(P, H, generator=g)
    initial = _clouds(P)[0]
    base = torch.cat((initial["means"], initial["rotation_quaternions"]), dim=1)
    ref = DR.TorchDeformationNetwork(H, 1)
    ref.load_state_dict(state)
    want = ref.fc_out(act) + base
    assert torch.equal(want, F.linear(act, state["fc_out.weight"], state["fc_out.bias"]) + base)
    monkeypatch.setattr(D, "deform_input_layer", lambda *a, **k: act)
    net.residual_blocks = torch.nn.Identity()
    for on in (False, True):  # CPU tensors are never eligible
        previous = D.set_fused_output_head(on)
        try:
            got = net(initial, initial, 3, 7)
        finally:
            D.set_fused_output_head(previous)
        assert torch.equal(got, want) and got.grad_fn.name().startswith("AddBackward")


# ---- GPU ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P,H", CASES)
def test_forward(cuda, P, H):
    x, w, b, _, initial, r32, r64 = _case(P, H)
    got = D.deform_output_layer(x, w, b, initial)
    assert got.shape == (P, 7) and got.dtype == torch.float32
    yardstick(f"output ({P}, {H})", got, r32["out"], r64["out"])


@pytest.mark.gpu
@pytest.mark.parametrize("P,H,max_blocks", [(P, H, mb) for P, H in CASES[:-1] for mb in (0, 2)] + [(257, 512, 2)])
def test_backward(cuda, P, H, max_blocks):
    x, w, b, up, initial, r32, r64 = _case(P, H)
    out, dx, dw, db = _run(x, w, b, up, initial, max_blocks)
    tag = f"({P}, {H}, max_blocks={max_blocks})"
    yardstick(f"output {tag}", out, r32["out"], r64["out"])
    yardstick(f"dx {tag}", dx, r32["dx"], r64["dx"])
    yardstick(f"dW {tag}", dw, r32["dw"], r64["dw"])
    yardstick(f"db {tag}", db, r32["db"], r64["db"])
    assert all(v.grad is None for v in initial.values())


@pytest.mark.gpu
def test_initial_parameters_gradient(cuda):
    P, H = 63, 64
    x, w, b, up, initial, _, _ = _case(P, H)
    live = {k: v.clone().requires_grad_(True) for k, v in initial.items()}
    plain = _run(x, w, b, up, initial, 0)
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
    out = D.deform_output_layer(*leaves, live)
    out.backward(up)
    assert torch.equal(live["means"].grad, up[:, :3]) and torch.equal(live["rotation_quaternions"].grad, up[:, 3:])
    for a, c in zip(plain, (out.detach(),) + tuple(t.grad for t in leaves)):
        assert torch.equal(a, c)
    # they alone require a gradient: nothing is saved, they still get theirs
    for v in live.values():
        v.grad = None
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        out = D.deform_output_layer(x, w, b, live)
    out.backward(up)
    assert saved == []
    assert torch.equal(live["means"].grad, up[:, :3]) and torch.equal(live["rotation_quaternions"].grad, up[:, 3:])


@pytest.mark.gpu
def test_gradient_subsets(cuda):
    P, H = 1031, 40
    x, w, b, up, initial, _, _ = _case(P, H)
    full = _run(x, w, b, up, initial, 2)
    for need in itertools.product((False, True), repeat=3):
        if not any(need):
            continue
        got = _run(x, w, b, up, initial, 2, need)
        assert torch.equal(got[0], full[0])
        for n, a, c in zip(need, got[1:], full[1:]):
            assert (a is None) if not n else torch.equal(a, c), need


@pytest.mark.gpu
def test_null_dx_writes_nothing_of_that_size(cuda):
    """Through the C ABI: with dL_dx NULL a poisoned (P, H) buffer of the caller's -- the only one of that size
    besides x -- keeps every bit, and x itself is unchanged; with only dL_dx wanted x may be NULL (it is not
    read) and the result is the same."""
    P, H = 1031, 40
    x, w, b, up, initial, _, _ = _case(P, H)
    L = _C.feature_library("head")
    full = _run(x, w, b, up, initial, 2)
    sentinel = torch.full((P, H), float("nan"), device=cuda)
    sentinel.view(torch.int32).fill_(0x7FC12345)
    before, x_before = sentinel.view(torch.int32).clone(), x.clone()
    ws = torch.empty(L.gsr_deform_out_workspace_bytes(P, H, 2), dtype=torch.uint8, device=cuda)
    dw, db = torch.empty(7, H, device=cuda), torch.empty(7, device=cuda)
    stream = _C._stream_ptr(cuda)
    _C._check(L.gsr_deform_out_backward(P, H, x.data_ptr(), w.data_ptr(), up.data_ptr(), ws.data_ptr(), 2, None,
                                        dw.data_ptr(), db.data_ptr(), stream))
    torch.cuda.synchronize()
    assert torch.equal(sentinel.view(torch.int32), before) and torch.equal(x, x_before)
    assert torch.equal(dw, full[2]) and torch.equal(db, full[3])
    dx = torch.empty(P, H, device=cuda)
    _C._check(L.gsr_deform_out_backward(P, H, None, w.data_ptr(), up.data_ptr(), None, 2, dx.data_ptr(), None, None,
                                        stream))
    torch.cuda.synchronize()
    assert torch.equal(dx, full[1])
    assert L.gsr_deform_out_backward(P, H, None, w.data_ptr(), up.data_ptr(), ws.data_ptr(), 2, None, dw.data_ptr(),
                                     None, stream) == 1  # dL_dweight needs x
    assert L.gsr_deform_out_workspace_bytes(P, H, 2) >= 2 * (7 * H + 7) * ctypes.sizeof(ctypes.c_float)


@pytest.mark.gpu
@pytest.mark.parametrize("P,H", [(4099, 64), (1031, 40)])
def test_bitwise_repeatable(cuda, P, H):
    x, w, b, up, initial, _, _ = _case(P, H)
    for a, c in zip(_run(x, w, b, up, initial, 2), _run(x, w, b, up, initial, 2)):
        assert torch.equal(a, c)


@pytest.mark.gpu
def test_no_grad_saves_nothing(cuda):
    P, H = 257, 128
    x, w, b, _, initial, _, _ = _case(P, H)
    x, w, b = (t.clone().requires_grad_(True) for t in (x, w, b))
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        with torch.no_grad():
            quiet = D.deform_output_layer(x, w, b, initial)
        assert saved == [] and quiet.grad_fn is None and not quiet.requires_grad
        loud = D.deform_output_layer(x, w, b, initial)
        assert len(saved) == 2 and loud.grad_fn is not None
    assert sum(t.numel() for t in saved) == P * H + 7 * H  # x and weight, nothing else
    assert torch.equal(quiet, loud.detach())


@pytest.mark.gpu
def test_empty_cloud(cuda):
    H = 64
    _, w, b, _ = (t.to(cuda) for t in _head(1, H))
    x = torch.zeros(0, H, device=cuda, requires_grad=True)
    w, b = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    initial = {"means": torch.zeros(0, 3, device=cuda), "rotation_quaternions": torch.zeros(0, 4, device=cuda)}
    out = D.deform_output_layer(x, w, b, initial)
    assert out.shape == (0, 7) and out.dtype == torch.float32
    out.backward(torch.zeros(0, 7, device=cuda))
    assert x.grad.shape == (0, H)
    assert w.grad.shape == (7, H) and b.grad.shape == (7,)
    assert not w.grad.any() and not b.grad.any()


@pytest.mark.gpu
def test_golden(cuda):
    initial, previous = _gold_clouds(cuda)
    timestep, count = (int(v) for v in GOLD["timestep"])
    assert timestep / count == _gold_progress()
    net = D.DeformationNetwork(32, 1).to(cuda).train()
    net.load_state_dict(_gold_state())
    out = net(initial, previous, timestep, count)
    assert type(out.grad_fn).__name__ == "_DeformOutBackward"
    out.backward(_t("upstream").to(cuda))
    band("golden output", out, GOLD["output"], 2e-4, 2e-5)
    for name in ("fc_out.weight", "fc_out.bias", "fc_in.weight"):
        band(f"golden grad {name}", net.get_parameter(name).grad, GOLD[f"grad/{name}"], 2e-4, 2e-5)


@pytest.mark.gpu
def test_routing(cuda):
    """P = 1031, H = 64, 2 blocks: the same state and inputs with the switch on and off."""
    P, H, blocks = 1031, 64, 2
    initial, previous = (_to(c, cuda) for c in _clouds(P))
    torch.manual_seed(5)
    net = D.DeformationNetwork(H, blocks).to(cuda).train()
    state = {k: v.clone() for k, v in net.state_dict().items()}
    up = torch.randn(P, 7, generator=torch.Generator().manual_seed(6)).to(cuda)
    names = ("fc_out.weight", "fc_out.bias", "residual_blocks.1.fc2.weight")

    def fused_network(on):
        net.load_state_dict(state)  # the same running statistics too
        net.zero_grad()
        calls = []
        hook = net.register_forward_hook(lambda m, i, o: calls.append(o))
        previous_switch = D.set_fused_output_head(on)
        try:
            out = net(initial, previous, 3, 7)
        finally:
            D.set_fused_output_head(previous_switch)
            hook.remove()
        assert len(calls) == 1 and calls[0] is out and out.shape == (P, 7)
        node = type(out.grad_fn).__name__
        out.backward(up)
        return node, out.detach(), {n: net.get_parameter(n).grad.clone() for n in names}

    def torch_only(dtype):
        ref = DR.TorchDeformationNetwork(H, blocks).to(cuda).to(dtype).train()
        ref.load_state_dict(state)
        base = torch.cat((initial["means"], initial["rotation_quaternions"]), dim=1).to(dtype)
        out = ref(DR.input_matrix(initial, previous, 3 / 7, dtype), base)
        out.backward(up.to(dtype))
        return out.detach(), {n: ref.get_parameter(n).grad for n in names}

    node_on, out_on, g_on = fused_network(True)
    node_off, out_off, g_off = fused_network(False)
    print(f"autograd nodes: on {node_on}, off {node_off}")
    assert node_on == "_DeformOutBackward" and node_off.startswith("AddBackward")
    o32, g32 = torch_only(torch.float32)
    o64, g64 = torch_only(torch.float64)

    def close(name, a, c, r32, r64):  # the two legs differ by no more than the band around either
        yard = float((r32.double() - r64).abs().max())
        band(name, a, c, floor=2 * yard)

    close("output on vs off", out_on, out_off, o32, o64)
    for n in names:
        close(f"grad {n} on vs off", g_on[n], g_off[n], g32[n], g64[n])

    # an activation the head does not take runs the torch lines, without raising
    class Strided(torch.nn.Module):
        def forward(self, x):
            return x.t().contiguous().t()

    class Double(torch.nn.Module):
        def forward(self, x):
            return x.double()

    net.load_state_dict(state)
    net.residual_blocks = Strided()
    out = net(initial, previous, 3, 7)
    assert out.shape == (P, 7) and out.grad_fn.name().startswith("AddBackward")
    net.residual_blocks = Double()
    net.fc_out.double()
    out = net(initial, previous, 3, 7)
    assert out.dtype == torch.float64 and out.grad_fn.name().startswith("AddBackward")
