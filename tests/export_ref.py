"""What the frame-export tests compare with: a numpy restatement of the reference's frame expression
(train.py:534-545) and one seeded test image.  Nothing here touches the code under test."""
import numpy as np

SPECIALS = np.array([-np.inf, -1.0, -0.0, 0.0, 0.99999994, 1.0, 1.0000001, np.inf], dtype=np.float32)
SPECIAL_BYTES = np.array([0, 0, 0, 0, 254, 255, 255, 255], dtype=np.uint8)


def reference_frame(image):
    """train.py:534-545 for a (3, H, W) float32 image (already on the host) -> (H, W, 3) uint8."""
    return (255 * np.clip(image, 0, 1)).astype(np.uint8).transpose(1, 2, 0)


def reference_frames(images):
    """reference_frame per image of (F, 3, H, W), with the NaN positions defined as 0 (numpy's own
    cast of NaN depends on the platform, so NaN never reaches it)."""
    images = np.asarray(images, dtype=np.float32)
    clean = np.where(np.isnan(images), np.float32(0), images)
    out = np.stack([reference_frame(im) for im in clean]) if len(images) else \
        np.zeros((0,) + images.shape[2:] + (3,), dtype=np.uint8)
    assert not out[np.isnan(images).transpose(0, 2, 3, 1)].any()
    return out


def test_image(F, H, W, seed=0):
    """(F, 3, H, W) float32: seeded normal values x 0.6 + 0.5 (a fifth below 0, a fifth above 1), with
    the special values and a NaN spliced in at the start of every frame as far as they fit."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((F, 3, H, W)).astype(np.float32) * np.float32(0.6) + np.float32(0.5))
    flat = x.reshape(F, -1)
    sp = np.concatenate([SPECIALS, np.array([np.nan], dtype=np.float32)])
    n = min(len(sp), flat.shape[1])
    # spread over the three planes when the frame is large enough, else at the start
    pos = np.arange(n) * (flat.shape[1] // n) if flat.shape[1] >= 3 * n else np.arange(n)
    flat[:, pos] = sp[:n]
    return x


test_image.__test__ = False  # a generator, not a test
