"""Frame export, host side (SURVEY.md component 9): the numpy restatement of the reference's frame
expression the GPU tests compare with, the shared test image and the mistakes it has to catch,
``splat_export.FrameWriter`` over numpy frames, and ``gsr_frames_pack``'s argument checks.

Every comparison is bitwise: a frame byte is a clamp, one float32 multiply and a truncation.
"""
import ctypes
import os

import numpy as np
import pytest
from PIL import Image

import export_ref as R
import splat_export
from diff_gaussian_rasterization import _C


# ---------------------------------------------------------------- the restatement
def test_restatement_on_special_values():
    image = np.broadcast_to(R.SPECIALS, (3, 1, len(R.SPECIALS))).copy()
    frame = R.reference_frame(image)
    assert frame.shape == (1, len(R.SPECIALS), 3) and frame.dtype == np.uint8
    for ch in range(3):
        assert frame[0, :, ch].tolist() == R.SPECIAL_BYTES.tolist() == [0, 0, 0, 0, 254, 255, 255, 255]


@pytest.mark.parametrize("decode", ["reciprocal", "division"])
def test_every_byte_survives_decode_then_export(decode):
    """What the loader makes of a byte (k * (1.0f / 255) on the GPU, k / 255 on the CPU) exports as k."""
    k = np.arange(256, dtype=np.float32)
    x = k * (np.float32(1.0) / np.float32(255.0)) if decode == "reciprocal" else k / np.float32(255.0)
    assert x.dtype == np.float32
    frame = R.reference_frame(np.broadcast_to(x, (3, 1, 256)).copy())
    assert np.array_equal(frame[0, :, 0], np.arange(256, dtype=np.uint8))


# ---------------------------------------------------------------- the shared image catches the mistakes
def test_image_moves_under_every_mistake():
    """The mistakes a frame kernel can make each change a large share of the test image's bytes, so a
    bitwise comparison on it cannot pass by accident."""
    x = R.test_image(5, 23, 37)
    finite = np.isfinite(x)
    assert finite.sum() >= x.size - 3 * x.shape[0]  # the spliced infinities and NaN, nothing else
    v = np.where(finite, x, np.float32(0.5))
    assert (v < 0).mean() >= 0.05 and (v > 1).mean() >= 0.05
    good = (255 * np.clip(v, 0, 1)).astype(np.uint8)
    inside = (v >= 0) & (v <= 1)
    rounded = np.rint(255 * np.clip(v, 0, 1)).astype(np.uint8)
    assert (rounded != good)[inside].mean() >= 0.25
    unclamped = (255 * v).astype(np.int64).astype(np.uint8)  # a cast that wraps what the clamp would hold
    assert (unclamped != good).mean() >= 0.05
    frames = R.reference_frames(v)
    mixed_up = good.reshape(frames.shape)  # planar bytes read as if they were interleaved
    assert (mixed_up != frames).mean() > 0.5


def test_image_is_seeded_and_carries_the_specials():
    a, b = R.test_image(2, 24, 40), R.test_image(2, 24, 40)
    assert np.array_equal(a, b, equal_nan=True) and a.dtype == np.float32
    assert not np.array_equal(a, R.test_image(2, 24, 40, seed=1), equal_nan=True)
    for f in range(2):
        assert np.isnan(a[f]).sum() == 1 and np.isinf(a[f]).sum() == 2
        assert np.signbit(a[f][a[f] == 0]).any()  # the -0.0
    assert np.isnan(R.test_image(1, 1, 1)).sum() == 0 and R.test_image(1, 1, 1).shape == (1, 3, 1, 1)
    assert np.isnan(R.test_image(1, 1, 3)).sum() == 1


# ---------------------------------------------------------------- FrameWriter over numpy frames
F, H, W = 3, 37, 23


def _content(t):
    return np.random.default_rng(100 + t).integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)


def test_frame_writer_ring_and_files(tmp_path):
    """7 submissions through 2 staging buffers and 3 workers: every PNG and every returned array is
    its own submission's, also after its buffer has been reused several times."""
    futures, early = [], None
    with splat_export.FrameWriter(depth=2, workers=3) as writer:
        for t in range(1, 8):
            paths = [tmp_path / f"cam{c}" / f"{t:06d}.png" for c in range(F)]
            if t == 4:
                paths[1] = None
            frames = _content(t)
            futures.append(writer.submit_host(frames, paths))
            frames[:] = 0  # the writer has taken its copy
            if t == 1:
                early = futures[0].result()
                kept = early.copy()
        assert np.array_equal(early, kept)  # its buffer has been refilled three times since
        assert writer.pool._max_workers == 3
    for t, fut in enumerate(futures, start=1):
        got = fut.result()
        assert got.dtype == np.uint8 and got.shape == (F, H, W, 3)
        assert np.array_equal(got, _content(t)), t
        for c in range(F):
            path = tmp_path / f"cam{c}" / f"{t:06d}.png"
            if t == 4 and c == 1:
                assert not path.exists()
                continue
            with Image.open(path) as im:
                assert im.mode == "RGB" and np.array_equal(np.asarray(im), _content(t)[c]), (t, c)
    assert sorted(os.listdir(tmp_path / "cam0")) == [f"{t:06d}.png" for t in range(1, 8)]
    assert sorted(os.listdir(tmp_path / "cam1")) == [f"{t:06d}.png" for t in range(1, 8) if t != 4]
    assert sorted(os.listdir(tmp_path)) == ["cam0", "cam1", "cam2"]


def test_frame_writer_default_pool_and_empty_batch(tmp_path):
    with splat_export.FrameWriter() as writer:
        assert writer.depth == 2 and writer.pool is None
        empty = writer.submit_host(np.zeros((0, 4, 4, 3), dtype=np.uint8), []).result()
        assert empty.shape == (0, 4, 4, 3)
        got = writer.submit_host(_content(1), [None] * F).result()
        assert writer.pool._max_workers == min(F, 8)
        assert np.array_equal(got, _content(1))
        with pytest.raises(ValueError, match="got 1 paths, expected 3"):
            writer.submit_host(_content(1), [None])
        with pytest.raises(TypeError, match="got float32 frames, expected uint8"):
            writer.submit_host(_content(1).astype(np.float32), [None] * F)
    assert os.listdir(tmp_path) == []


def test_frame_writer_errors_surface(tmp_path):
    blocker = tmp_path / "not_a_directory"
    blocker.write_bytes(b"x")
    writer = splat_export.FrameWriter(depth=2, workers=2)
    ok = writer.submit_host(_content(1), [tmp_path / "ok" / f"{c}.png" for c in range(F)])
    bad = writer.submit_host(_content(2), [tmp_path / "ok" / "a.png", blocker / "b.png", None])
    with pytest.raises(OSError):
        bad.result()
    assert np.array_equal(ok.result(), _content(1))
    with pytest.raises(OSError):
        writer.close()
    with pytest.raises(RuntimeError, match="after close"):
        writer.submit_host(_content(3), [None] * F)
    with pytest.raises(OSError):  # leaving the with block raises it too
        with splat_export.FrameWriter(depth=1, workers=1) as w2:
            w2.submit_host(_content(2), [blocker / "c.png", None, None])


# ---------------------------------------------------------------- the C boundary, host side only
def test_frames_pack_argument_checks():
    L = _C.feature_library("frames")
    assert "gsr_frames_pack" in _C.EXPORTED_SYMBOLS and L.gsr_abi_version() == 21
    fake = ctypes.c_void_p(256)  # never dereferenced: every call below returns before a launch
    for args in ((1, 4, 4, None, None), (1, 4, 4, fake, None), (1, 4, 4, None, fake)):
        assert L.gsr_frames_pack(*args, None) != 0
        assert b"frames_pack: null" in L.gsr_last_error()
    for args in ((-1, 4, 4), (1, -4, 4), (1, 4, -4)):
        assert L.gsr_frames_pack(*args, fake, fake, None) != 0
        assert b"frames_pack: negative size" in L.gsr_last_error()
    for args in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (0, 0, 0)):
        assert L.gsr_frames_pack(*args, None, None, None) == 0
    assert L.gsr_frames_pack(1, 1 << 15, 1 << 15, fake, fake, None) != 0
    assert b"too large" in L.gsr_last_error()


def test_stale_library_is_a_rebuild_error_on_first_use(monkeypatch):
    """A libgsr.so from before gsr_frames_pack still loads and serves everything else; the export
    feature alone raises, with the rebuild hint."""
    real = _C.load_library()
    assert not _C._MISSING and _C.feature_library("frames") is real

    class Stale:
        def __getattr__(self, name):
            if name == "gsr_frames_pack":
                raise AttributeError(f"undefined symbol: {name}")
            return getattr(real, name)

    monkeypatch.setattr(_C, "_lib", None)
    monkeypatch.setattr(_C, "_MISSING", {})
    monkeypatch.setattr(_C, "_PREALLOC_FN", _C._PREALLOC_FN)
    monkeypatch.setattr(_C.ctypes, "CDLL", lambda path: Stale())
    stale = _C.load_library()
    assert isinstance(stale, Stale) and list(_C._MISSING) == ["frames"]
    assert _C.feature_library("foreground") is stale
    with pytest.raises(RuntimeError, match="lacks the 8-bit frame export .*gsr_frames_pack.*rebuild it"):
        _C.feature_library("frames")


def test_frames_to_uint8_has_no_cpu_path():
    import torch
    with pytest.raises(RuntimeError, match=r"frames_to_uint8: got .*expected a GPU tensor"):
        splat_export.frames_to_uint8(torch.zeros((1, 3, 4, 4)))
