"""Shapes, mask kinds and the literal host chain shared by test_present_cpu.py and test_hip_present.py."""
import numpy as np
from PIL import Image

# (mh, mw) -> (H, W)
SHAPES = [
    ((28, 28), (300, 400)),   # the usual up-scale
    ((56, 56), (333, 250)),   # odd sizes, W % 4 = 2
    ((28, 28), (17, 23)),     # down-scale, ks = 11, W % 4 = 3
    ((56, 56), (56, 56)),     # both passes skipped
    ((28, 28), (28, 90)),     # the vertical pass alone skipped
    ((56, 56), (1, 1)),       # ks = 337
    ((28, 28), (5, 300)),     # thin
    ((56, 56), (40, 500)),    # thin
    ((28, 28), (224, 224)),
]
KINDS = ["uniform", "hard", "clipped_normal"]


def make_mask(kind: str, mh: int, mw: int, rng) -> np.ndarray:
    if kind == "uniform":
        return rng.random((mh, mw), dtype=np.float32)
    if kind == "hard":       # Lanczos ringing under- and overshoots: both clips fire
        return (rng.random((mh, mw)) > 0.5).astype(np.float32)
    return np.clip(rng.normal(0.5, 0.6, (mh, mw)), 0, 1).astype(np.float32)   # many exact 0 and 1 values


def make_case(i: int, kind: str):
    """case i of SHAPES with a mask of ``kind`` -> (mask float32 (mh, mw), upload uint8 (H, W, 3)), seeded by (i, kind)"""
    (mh, mw), (H, W) = SHAPES[i]
    rng = np.random.Generator(np.random.PCG64([i, KINDS.index(kind), 20241]))
    return make_mask(kind, mh, mw, rng), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def pil_mask(mask_f32: np.ndarray, H: int, W: int) -> Image.Image:
    """app.py:296-298"""
    return Image.fromarray((mask_f32 * 255).astype(np.uint8)).resize((W, H), Image.Resampling.LANCZOS)


def pil_heat(mask_img: Image.Image, rgb: np.ndarray) -> Image.Image:
    """app.py:300-311, literally (needs matplotlib)"""
    import matplotlib.pyplot as plt
    from PIL import ImageEnhance
    original = Image.fromarray(rgb)
    rgba = (plt.get_cmap("jet")(np.array(mask_img) / 255.0) * 255).astype(np.uint8)
    heat_img = Image.fromarray(rgba).convert("RGBA").resize(original.size, Image.Resampling.LANCZOS)
    return ImageEnhance.Brightness(Image.blend(original.convert("RGBA"), heat_img, alpha=0.5)).enhance(1.1)
