"""Frame export on the GPU (SURVEY.md component 9): ``gsr_frames_pack`` through
``splat_export.frames_to_uint8``, the pipelined ``FrameWriter.submit``, and the two render-and-export
entry points.  Every comparison is bitwise against the numpy restatement of train.py:534-545 in
tests/export_ref.py; NaN positions are compared with 0.
"""
import numpy as np
import pytest
import torch
from PIL import Image

import export_ref as R
import splat_export
import splat_io
import splat_scenes as S
from diff_gaussian_rasterization import GaussianRasterizer

pytestmark = pytest.mark.gpu

# 1x1 .. 1x5: fewer pixels than one thread's four, with and without a partial group; 23x37 ragged and
# 24x40 vector (the loader's fixture sizes); 1023 / 1024 / 1025 pixels: either side of one block of
# 256 threads x 4 pixels; 32x33: vector path over two blocks with a partly filled second one.
SHAPES = [(1, 1), (1, 3), (2, 2), (1, 5), (23, 37), (24, 40), (1, 1023), (1, 1024), (1, 1025), (32, 33)]


def _check(got, images):
    """A GPU result against the restatement of the same host images."""
    ref = R.reference_frames(images)
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == ref.shape
    nan = np.isnan(images).transpose(0, 2, 3, 1)
    assert not got[nan].any()
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("F", [1, 2, 5])
@pytest.mark.parametrize("H,W", SHAPES)
def test_frames_to_uint8_bitwise(cuda, F, H, W):
    x = R.test_image(F, H, W, seed=H * W + F)
    got = splat_export.frames_to_uint8(torch.from_numpy(x).to(cuda))
    assert got.is_cuda and got.is_contiguous()
    _check(got, x)


def test_special_values(cuda):
    x = torch.from_numpy(np.broadcast_to(R.SPECIALS, (3, 1, 8)).copy()).to(cuda)  # vector path
    assert splat_export.frames_to_uint8(x).cpu().numpy()[0, :, 1].tolist() == R.SPECIAL_BYTES.tolist()
    y = torch.from_numpy(np.broadcast_to(R.SPECIALS[:7], (3, 1, 7)).copy()).to(cuda)  # scalar path
    assert splat_export.frames_to_uint8(y).cpu().numpy()[0, :, 2].tolist() == R.SPECIAL_BYTES[:7].tolist()
    nan = torch.full((3, 2, 4), float("nan"), device=cuda)
    assert not splat_export.frames_to_uint8(nan).any()
    assert not splat_export.frames_to_uint8(nan[:, :, :3]).any()


@pytest.mark.parametrize("H,W", [(23, 37), (24, 40)])
def test_input_forms(cuda, H, W):
    x = R.test_image(5, H, W, seed=7)
    ref = R.reference_frames(x)
    stacked = splat_export.frames_to_uint8(torch.from_numpy(x).to(cuda))
    separate = [torch.from_numpy(x[c].copy()).to(cuda) for c in range(5)]  # five allocations
    from_list = splat_export.frames_to_uint8(separate)
    assert from_list.shape == (5, H, W, 3) and torch.equal(from_list, stacked)
    assert np.array_equal(from_list.cpu().numpy(), ref)
    one = splat_export.frames_to_uint8(separate[2])
    assert one.shape == (H, W, 3) and np.array_equal(one.cpu().numpy(), ref[2])
    # the reference's own layout: HWC memory seen as CHW through permute
    hwc = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).to(cuda)
    view = hwc.permute(0, 3, 1, 2)
    assert not view.is_contiguous()
    _check(splat_export.frames_to_uint8(view), x)
    _check(splat_export.frames_to_uint8([v for v in view]), x)


def test_misaligned_storage_offset(cuda):
    """H * W % 4 == 0, but the storage starts 4 bytes into its buffer: no 16-byte loads there."""
    F, H, W = 2, 24, 40
    x = R.test_image(F, H, W, seed=11)
    buf = torch.empty(F * 3 * H * W + 1, dtype=torch.float32, device=cuda)
    shifted = buf[1:].view(F, 3, H, W)
    shifted.copy_(torch.from_numpy(x))
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    _check(splat_export.frames_to_uint8(shifted), x)
    _check(splat_export.frames_to_uint8([shifted[0], shifted[1]]), x)


def test_empty_batch(cuda):
    out = splat_export.frames_to_uint8(torch.zeros((0, 3, 4, 4), device=cuda))
    assert out.shape == (0, 4, 4, 3) and out.dtype == torch.uint8 and out.is_cuda
    out = splat_export.frames_to_uint8(torch.zeros((2, 3, 0, 4), device=cuda))
    assert out.shape == (2, 0, 4, 3)


@pytest.mark.parametrize("H,W", [(23, 37), (24, 40)])
def test_round_trip_through_both_kernels(cuda, H, W):
    rgb = np.random.default_rng(H).integers(0, 256, size=(3, H, W, 3), dtype=np.uint8)
    rgb[0].reshape(-1)[:256] = np.arange(256, dtype=np.uint8)  # every byte value
    d = torch.from_numpy(rgb).to(cuda)
    back = splat_export.frames_to_uint8(splat_io.pack_views(d)[0])
    assert torch.equal(back, d)


def test_errors(cuda):
    form = r"frames_to_uint8: (images\[\d\]: )?got .*expected "
    with pytest.raises(RuntimeError, match=form + "a GPU tensor"):
        splat_export.frames_to_uint8(torch.zeros((1, 3, 4, 4)))
    with pytest.raises(TypeError, match=form + "float32"):
        splat_export.frames_to_uint8(torch.zeros((1, 3, 4, 4), dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError, match=form + r"\(F, 3, H, W\)"):
        splat_export.frames_to_uint8(torch.zeros((1, 4, 4, 4), device=cuda))
    with pytest.raises(ValueError, match=form + r"\(3, 4, 4\)"):
        splat_export.frames_to_uint8([torch.zeros((3, 4, 4), device=cuda), torch.zeros((3, 4, 5), device=cuda)])
    with pytest.raises(TypeError, match="expected a GPU uint8 tensor"):
        with splat_export.FrameWriter() as writer:
            writer.submit(torch.zeros((1, 4, 4, 3), device=cuda), [None])


def test_frame_writer_from_the_gpu(cuda, tmp_path):
    """7 submissions through 2 staging buffers from a non-default stream, the producing tensor
    overwritten with the next content before each: the copy, its event and the reuse of the buffers
    are ordered when every PNG and every returned array is its own submission's."""
    F, H, W = 3, 37, 23
    x = R.test_image(7 * F, H, W, seed=3).reshape(7, F, 3, H, W)
    contents = torch.from_numpy(x).to(cuda)
    stream = torch.cuda.Stream(cuda)
    stream.wait_stream(torch.cuda.current_stream(cuda))
    futures = []
    with torch.cuda.stream(stream), splat_export.FrameWriter(depth=2, workers=3) as writer:
        producer = torch.empty((F, 3, H, W), device=cuda)
        for t in range(7):
            producer.copy_(contents[t])
            frames = splat_export.frames_to_uint8(producer)
            futures.append(writer.submit(frames, [tmp_path / f"cam{c}" / f"{t + 1:06d}.png" for c in range(F)]))
            del frames  # the allocator may hand its memory to the next one
    stream.synchronize()
    for t, fut in enumerate(futures):
        ref = R.reference_frames(x[t])
        got = fut.result()
        assert isinstance(got, np.ndarray) and np.array_equal(got, ref), t
        for c in range(F):
            with Image.open(tmp_path / f"cam{c}" / f"{t + 1:06d}.png") as im:
                assert np.array_equal(np.asarray(im), ref[c]), (t, c)


@pytest.fixture(scope="module")
def cloud(cuda):
    return S.synthetic_cloud(2000, 0.02, seed=2, device=cuda)


def _reference_render(params, w2c, aspect, device):
    rs = S.render_settings(S.INFERENCE_W, S.INFERENCE_H, S.inference_intrinsics(aspect), w2c, device=device)
    with torch.no_grad():
        image, _, _ = GaussianRasterizer(raster_settings=rs)(**S.render_arguments(params))
    return R.reference_frame(image.cpu().numpy())


def test_render_and_export_frame(cuda, cloud, tmp_path):
    w2c, aspect = S.inference_rig()["090"]
    frame = splat_export.render_and_export_frame(cloud, 12, aspect, w2c, tmp_path / "090")
    assert isinstance(frame, np.ndarray) and frame.dtype == np.uint8 and frame.shape == (720, 1280, 3)
    ref = _reference_render(cloud, w2c, aspect, cuda)
    assert ref.any()  # the camera sees the cloud
    assert np.array_equal(frame, ref)
    with Image.open(tmp_path / "090" / "000012.png") as im:
        assert np.array_equal(np.asarray(im), frame)


def test_export_timestep_frames(cuda, cloud, tmp_path):
    rig = S.inference_rig()
    with splat_export.FrameWriter() as writer:
        future = splat_export.export_timestep_frames(cloud, 3, tmp_path, writer)
        frames = future.result()
    assert frames.shape == (5, 720, 1280, 3) and frames.dtype == np.uint8
    for c, (name, (w2c, aspect)) in enumerate(rig.items()):
        assert np.array_equal(frames[c], _reference_render(cloud, w2c, aspect, cuda)), name
        with Image.open(tmp_path / name / "000003.png") as im:
            assert np.array_equal(np.asarray(im), frames[c]), name
