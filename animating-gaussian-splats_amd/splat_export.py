"""Frame export (SURVEY.md component 9): rendered images -> 8-bit frames -> PNG files.

Reference behaviour restated here (same names, arguments and results):

* ``render_and_export_frame(gaussian_cloud_parameters, timestep, aspect_ratio, extrinsic_matrix,
  directory)`` (train.py:506-547): one 1280 x 720 render of a fixed camera, the frame
  ``(255 * np.clip(image.cpu().numpy(), 0, 1)).astype(np.uint8).transpose(1, 2, 0)`` written as
  ``directory / f"{timestep:06d}.png"`` and returned.
* ``export_timestep_frames`` is the body of the inference loop over the rig (train.py:587-596).

How it is done on MI355X: the reference copies every float image to the host (11 MB at 1280 x 720,
a copy that synchronises the device), clips, scales, casts and transposes it on one host thread and
encodes the PNG on that thread before the next render is queued.  Here ``gsr_frames_pack``
(csrc/gsr_io.hip) writes the interleaved 8-bit frame on the GPU, so one device-to-host copy moves
3 bytes per pixel instead of 12 for the whole rig, and ``FrameWriter`` takes it through a ring of
pinned buffers on a side stream to a thread pool that encodes the PNGs while the next timestep
renders -- the mirror of ``splat_io.TimestepDecoder`` / ``gsr_views_pack`` on the input side.

Each byte is clamp to [0, 1], one float32 multiply by 255, truncation: bitwise the reference's for
every finite or infinite value.  NaN gives 0 (numpy's cast of NaN depends on the platform).  PNGs
are written with PIL; PNG is lossless, so the stored pixels are those ``imageio.imwrite`` stores.
MP4 assembly and the wandb upload are out of scope.
"""
from __future__ import annotations

import concurrent.futures as cf
import threading
from pathlib import Path

import numpy as np
import torch

import splat_scenes as S
from diff_gaussian_rasterization import GaussianRasterizer, _C

__all__ = ["frames_to_uint8", "FrameWriter", "render_and_export_frame", "export_timestep_frames"]


def _describe(x):
    if isinstance(x, torch.Tensor):
        return f"{tuple(x.shape)} {x.dtype} on {x.device}"
    return type(x).__name__


def _pack(L, frames, H, W, src, dst):
    _C._check(L.gsr_frames_pack(frames, H, W, src.data_ptr(), dst.data_ptr(), _C._stream_ptr(src.device)))


def frames_to_uint8(images):
    """``(255 * clip(images, 0, 1)).astype(uint8)`` in HWC order, on the GPU (``gsr_frames_pack``).

    ``images``: a float32 GPU tensor (F, 3, H, W) -> (F, H, W, 3) uint8, or (3, H, W) -> (H, W, 3), or
    a list of (3, H, W) tensors of one size and device -> (F, H, W, 3): every image of a list is
    written into its slice of the one output (a launch per image, no stacked float copy), so one
    copy takes the whole rig to the host.  Any strides and storage offset; current stream."""
    if isinstance(images, (list, tuple)):
        if not images:
            raise ValueError("frames_to_uint8: got an empty list, expected at least one (3, H, W) image")
        first = images[0]
        for k, im in enumerate(images):
            if not isinstance(im, torch.Tensor) or im.dim() != 3 or im.size(0) != 3:
                raise ValueError(f"frames_to_uint8: images[{k}]: got {_describe(im)}, expected a (3, H, W) tensor")
            if not im.is_cuda:
                raise RuntimeError(f"frames_to_uint8: images[{k}]: got {_describe(im)}, expected a GPU tensor "
                                   "(no CPU path)")
            if im.dtype != torch.float32:
                raise TypeError(f"frames_to_uint8: images[{k}]: got {_describe(im)}, expected float32")
            if im.shape != first.shape or im.device != first.device:
                raise ValueError(f"frames_to_uint8: images[{k}]: got {_describe(im)}, expected "
                                 f"{tuple(first.shape)} on {first.device} like images[0]")
        srcs, single = list(images), False
    else:
        if not isinstance(images, torch.Tensor):
            raise TypeError(f"frames_to_uint8: got {_describe(images)}, expected a tensor or a list of tensors")
        if not images.is_cuda:
            raise RuntimeError(f"frames_to_uint8: got {_describe(images)}, expected a GPU tensor (no CPU path)")
        if images.dtype != torch.float32:
            raise TypeError(f"frames_to_uint8: got {_describe(images)}, expected float32")
        if images.dim() not in (3, 4) or images.size(-3) != 3:
            raise ValueError(f"frames_to_uint8: got {_describe(images)}, expected (F, 3, H, W) or (3, H, W)")
        single = images.dim() == 3
        srcs = None
    L = _C.feature_library("frames")
    if srcs is None:
        src = images.detach().contiguous()
        src = src.unsqueeze(0) if single else src
        F, _, H, W = src.shape
        out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=src.device)
        if F * H * W:
            with _C._device_guard(src.device):
                _pack(L, F, H, W, src, out)
        return out[0] if single else out
    _, H, W = srcs[0].shape
    out = torch.empty((len(srcs), H, W, 3), dtype=torch.uint8, device=srcs[0].device)
    if H * W:
        with _C._device_guard(out.device):
            for k, im in enumerate(srcs):
                _pack(L, 1, H, W, im.detach().contiguous(), out[k])
    return out


def _write_png(path, frame):
    from PIL import Image  # imported lazily: only the writer needs it
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(frame).save(path, format="PNG")


class _Slot:
    __slots__ = ("staging", "busy")

    def __init__(self):
        self.staging = None  # flat uint8 host tensor (pinned when a GPU is present), grown on demand
        self.busy = None     # the future of the last encode that read it


class FrameWriter:
    """Pipelined PNG writer: a ring of ``depth`` pinned 8-bit staging buffers and a thread pool.

    ``submit(frames_u8, paths)``: a GPU (F, H, W, 3) uint8 tensor and F paths.  The tensor is copied
    on a side stream (ordered after the current stream's work so far) into the next staging buffer;
    the pool waits for the copy's event, takes each frame out of the buffer and writes its PNG
    (parent directories are created; a path of None skips the file).  Returns a future of the
    (F, H, W, 3) uint8 numpy array -- a copy, valid after the buffer is reused.  ``submit_host`` takes
    a numpy array through the same ring and pool.  A buffer is reused only after the encode that
    read it has finished: ``submit`` then blocks on that encode, and on nothing else.  An encoder
    error is raised by the future's ``result()`` and by ``close()`` / leaving the ``with`` block.
    ``workers``: pool size, by default min(F, 8) of the first submission."""

    def __init__(self, depth: int = 2, workers: int | None = None):
        if depth < 1:
            raise ValueError(f"FrameWriter: got depth={depth}, expected at least 1")
        self.depth, self.workers = depth, workers
        self.pool = None
        self._slots = [_Slot() for _ in range(depth)]
        self._next = 0
        self._streams = {}  # device -> the side stream of its copies
        self._lock = threading.Lock()
        self._pending, self._errors = set(), []
        self._closed = False

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        try:
            self.close()
        except Exception:
            if exc_type is None:  # an error already on its way out is not replaced by ours
                raise
        return False

    def close(self):
        """Wait for every encode, stop the pool, and raise the first encoder error there was."""
        self._closed = True
        with self._lock:
            pending = list(self._pending)
        cf.wait(pending)
        if self.pool is not None:
            self.pool.shutdown(wait=True)
            self.pool = None
        if self._errors:
            err, self._errors = self._errors[0], []
            raise err

    # ---- the host half: ring + pool ------------------------------------------------------------
    def _acquire(self, shape, paths):
        """The next slot, free and with a staging view of ``shape``."""
        if self._closed:
            raise RuntimeError("FrameWriter: submit after close()")
        if len(shape) != 4 or shape[3] != 3:
            raise ValueError(f"FrameWriter: got frames of shape {tuple(shape)}, expected (F, H, W, 3)")
        if len(paths) != shape[0]:
            raise ValueError(f"FrameWriter: got {len(paths)} paths, expected {shape[0]} (one per frame)")
        slot = self._slots[self._next]
        self._next = (self._next + 1) % self.depth
        if slot.busy is not None:
            cf.wait([slot.busy])  # its error, if any, belongs to its own future and to close()
            slot.busy = None
        n = int(np.prod(shape))
        if slot.staging is None or slot.staging.numel() < n:
            slot.staging = torch.empty(max(n, 1), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        return slot, slot.staging[:n].view(tuple(shape))

    def _encode(self, slot, staged, paths, event=None):
        """Queue the frames of a filled slot; the returned future is what frees the slot."""
        F = staged.shape[0]
        done = cf.Future()
        out = np.empty(tuple(staged.shape), dtype=np.uint8)
        if F == 0:
            done.set_result(out)
            return done
        if self.pool is None:
            self.pool = cf.ThreadPoolExecutor(self.workers or min(F, 8))
        src = staged.numpy()
        lock, left, errs = threading.Lock(), [F], []

        def one(c):
            if event is not None:
                event.synchronize()  # the device-to-host copy has landed
            out[c] = src[c]
            if paths[c] is not None:
                _write_png(paths[c], out[c])

        def finish(j):
            with lock:
                if j.exception() is not None:
                    errs.append(j.exception())
                left[0] -= 1
                last = left[0] == 0
            if last:  # exactly one callback gets here
                with self._lock:
                    self._pending.discard(done)
                    if errs:
                        self._errors.append(errs[0])
                if errs:
                    done.set_exception(errs[0])
                else:
                    done.set_result(out)

        slot.busy = done
        with self._lock:
            self._pending.add(done)
        for c in range(F):
            self.pool.submit(one, c).add_done_callback(finish)
        return done

    def submit_host(self, frames, paths) -> cf.Future:
        frames = np.asarray(frames)
        if frames.dtype != np.uint8:
            raise TypeError(f"FrameWriter.submit_host: got {frames.dtype} frames, expected uint8")
        paths = list(paths)
        slot, staged = self._acquire(frames.shape, paths)
        np.copyto(staged.numpy(), frames)
        return self._encode(slot, staged, paths)

    # ---- the GPU half ----------------------------------------------------------------------------
    def submit(self, frames_u8, paths) -> cf.Future:
        if not isinstance(frames_u8, torch.Tensor) or not frames_u8.is_cuda or frames_u8.dtype != torch.uint8:
            raise TypeError(f"FrameWriter.submit: got {_describe(frames_u8)}, expected a GPU uint8 tensor "
                            "(frames_to_uint8's result; numpy frames go to submit_host)")
        paths = list(paths)
        slot, staged = self._acquire(frames_u8.shape, paths)
        if frames_u8.numel() == 0:
            return self._encode(slot, staged, paths)
        dev = frames_u8.device
        side = self._streams.get(dev)
        if side is None:
            side = self._streams[dev] = torch.cuda.Stream(dev)
        src = frames_u8.contiguous()
        side.wait_stream(torch.cuda.current_stream(dev))  # after the kernel that produced the frames
        with torch.cuda.stream(side):
            staged.copy_(src, non_blocking=True)
            event = torch.cuda.Event()
            event.record(side)
        src.record_stream(side)  # the allocator must not hand its memory out before the copy has read it
        return self._encode(slot, staged, paths, event)


_SETTINGS = {}
_SETTINGS_MAX = 64


def _inference_settings(aspect_ratio, extrinsic_matrix, device):
    """The 1280 x 720 render settings of train.py:513-526, kept per camera: building them uploads
    small tensors, which waits for the device."""
    w2c = np.asarray(extrinsic_matrix, dtype=np.float64)
    key = (float(aspect_ratio), w2c.tobytes(), str(device))
    rs = _SETTINGS.get(key)
    if rs is None:
        if len(_SETTINGS) >= _SETTINGS_MAX:
            _SETTINGS.clear()
        rs = _SETTINGS[key] = S.render_settings(
            image_width=S.INFERENCE_W, image_height=S.INFERENCE_H,
            intrinsic_matrix=S.inference_intrinsics(aspect_ratio), extrinsic_matrix=w2c, device=device)
    return rs


def _render(gaussian_cloud_parameters, aspect_ratio, extrinsic_matrix):
    device = gaussian_cloud_parameters["means"].device
    rs = _inference_settings(aspect_ratio, extrinsic_matrix, device)
    with torch.no_grad():
        image, _, _ = GaussianRasterizer(raster_settings=rs)(**S.render_arguments(gaussian_cloud_parameters))
    return image


def render_and_export_frame(gaussian_cloud_parameters, timestep: int, aspect_ratio: float, extrinsic_matrix,
                            directory):
    """train.py:506-547 on the native path: returns the (720, 1280, 3) uint8 frame and writes it as
    ``directory / f"{timestep:06d}.png"``.  The 8-bit frame is made on the GPU; the copy that waits
    for the device moves a quarter of the reference's bytes."""
    image = _render(gaussian_cloud_parameters, aspect_ratio, extrinsic_matrix)
    frame = frames_to_uint8(image).cpu().numpy()
    _write_png(Path(directory) / f"{timestep:06d}.png", frame)
    return frame


def export_timestep_frames(params, timestep: int, frames_directory, writer: FrameWriter, rig=None) -> cf.Future:
    """The pipelined form of train.py:587-596: every camera of ``rig`` (name -> (w2c, aspect ratio),
    default ``splat_scenes.inference_rig()``) rendered under ``no_grad``, one 8-bit batch, one
    ``writer.submit`` to ``frames_directory / name / f"{timestep:06d}.png"``.  Returns the writer's
    future of the (cameras, 720, 1280, 3) frames in the rig's order; the PNGs are encoded while the
    caller goes on to the next timestep."""
    rig = S.inference_rig() if rig is None else rig
    images = [_render(params, aspect_ratio, w2c) for w2c, aspect_ratio in rig.values()]
    paths = [Path(frames_directory) / name / f"{timestep:06d}.png" for name in rig]
    return writer.submit(frames_to_uint8(images), paths)
