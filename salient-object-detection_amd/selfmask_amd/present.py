"""The serving response's images (SelfMaskInference.predict, app.py:296-311) restated as integer arithmetic: the host half of
``csrc/present.hip``.

The reference turns the selected low-resolution mask into two pictures of the upload's size: the mask itself (8 bits, Pillow LANCZOS
resize) and a heat map (matplotlib's ``jet`` on the resized mask, ``Image.blend`` with the upload at 0.5, ``ImageEnhance.Brightness``
at 1.1).  Every step is determined to the bit:

* the resize is Pillow's two-pass 8-bit resampler (horizontal first, uint8 in between, 22-bit fixed-point taps, a pass whose input and
  output lengths agree skipped) with the Lanczos-3 filter: ``pil_lanczos_coeffs`` builds the taps as ``precompute_coeffs`` +
  ``normalize_coeffs_8bpc`` do;
* ``cmap(v / 255.0)`` of an 8-bit ``v`` is entry ``v`` of the colour map's 256-entry table: ``JET_RGBA`` pins that table as data, so
  nothing here needs matplotlib;
* the heat image's second LANCZOS resize (app.py:306) is to its own size, which Pillow answers with a copy;
* blend and brightness are Pillow's ``ImagingBlend``: fp32, multiply and add rounded separately, truncated (clipped when the factor
  lies outside [0, 1]).

``present_reference_numpy`` is the restatement the CPU tests pin against Pillow and matplotlib and the GPU tests hold the kernels to -
the role ``pipeline.resize_reference_numpy`` plays for the input pipeline.
"""
from typing import Tuple

import numpy as np

from .resample import pil_coeffs, resample_pass

BLEND_ALPHA = 0.5   # Image.blend(original, heat, alpha=0.5), app.py:309
BRIGHTNESS = 1.1    # ImageEnhance.Brightness(...).enhance(1.1), app.py:310-311

# (cmap(i) * 255).astype(uint8) for i in 0 .. 255 of matplotlib's "jet" (N = 256): 256 x RGBA, row-major
JET_RGBA_SHA256 = "878b65944cde43dd8015035710be8c53357a64fa2fbc6eae358ee5257a876b8e"
JET_RGBA = np.frombuffer(bytes.fromhex(
    "00007fff000084ff000088ff00008dff000091ff000096ff00009aff00009fff0000a3ff0000a8ff0000acff0000b1ff0000b6ff0000baff0000bfff0000c3ff"
    "0000c8ff0000ccff0000d1ff0000d5ff0000daff0000deff0000e3ff0000e8ff0000ecff0000f1ff0000f5ff0000faff0000feff0000ffff0000ffff0000ffff"
    "0000ffff0004ffff0008ffff000cffff0010ffff0014ffff0018ffff001cffff0020ffff0024ffff0028ffff002cffff0030ffff0034ffff0038ffff003cffff"
    "0040ffff0044ffff0048ffff004cffff0050ffff0054ffff0058ffff005cffff0060ffff0064ffff0068ffff006cffff0070ffff0074ffff0078ffff007cffff"
    "0080ffff0084ffff0088ffff008cffff0090ffff0094ffff0098ffff009cffff00a0ffff00a4ffff00a8ffff00acffff00b0ffff00b4ffff00b8ffff00bcffff"
    "00c0ffff00c4ffff00c8ffff00ccffff00d0ffff00d4ffff00d8ffff00dcfeff00e0faff00e4f7ff02e8f4ff05ecf1ff08f0edff0cf4eaff0ff8e7ff12fce4ff"
    "15ffe1ff18ffddff1cffdaff1fffd7ff22ffd4ff25ffd0ff29ffcdff2cffcaff2fffc7ff32ffc3ff36ffc0ff39ffbdff3cffbaff3fffb7ff42ffb3ff46ffb0ff"
    "49ffadff4cffaaff4fffa6ff53ffa3ff56ffa0ff59ff9dff5cff9aff5fff96ff63ff93ff66ff90ff69ff8dff6cff89ff70ff86ff73ff83ff76ff80ff79ff7dff"
    "7cff79ff80ff76ff83ff73ff86ff70ff89ff6cff8dff69ff90ff66ff93ff63ff96ff5fff9aff5cff9dff59ffa0ff56ffa3ff53ffa6ff4fffaaff4cffadff49ff"
    "b0ff46ffb3ff42ffb7ff3fffbaff3cffbdff39ffc0ff36ffc3ff32ffc7ff2fffcaff2cffcdff29ffd0ff25ffd4ff22ffd7ff1fffdaff1cffddff18ffe0ff15ff"
    "e4ff12ffe7ff0fffeaff0cffedff08fff1fc05fff4f802fff7f400fffaf000fffeed00ffffe900ffffe500ffffe200ffffde00ffffda00ffffd700ffffd300ff"
    "ffcf00ffffcb00ffffc800ffffc400ffffc000ffffbd00ffffb900ffffb500ffffb100ffffae00ffffaa00ffffa600ffffa300ffff9f00ffff9b00ffff9800ff"
    "ff9400ffff9000ffff8c00ffff8900ffff8500ffff8100ffff7e00ffff7a00ffff7600ffff7300ffff6f00ffff6b00ffff6700ffff6400ffff6000ffff5c00ff"
    "ff5900ffff5500ffff5100ffff4d00ffff4a00ffff4600ffff4200ffff3f00ffff3b00ffff3700ffff3400ffff3000ffff2c00ffff2800ffff2500ffff2100ff"
    "ff1d00ffff1a00ffff1600fffe1200fffa0f00fff50b00fff10700ffec0300ffe80000ffe30000ffde0000ffda0000ffd50000ffd10000ffcc0000ffc80000ff"
    "c30000ffbf0000ffba0000ffb60000ffb10000ffac0000ffa80000ffa30000ff9f0000ff9a0000ff960000ff910000ff8d0000ff880000ff840000ff7f0000ff"
), np.uint8).reshape(256, 4)


def pil_lanczos_coeffs(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray, int]:
    """``resample.pil_coeffs`` for the LANCZOS filter (support 3.0): (bounds, taps, ks), cached there.  ks = 7 when up-scaling,
    ceil(3 in / out) * 2 + 1 when the output is the smaller one."""
    return pil_coeffs(in_size, out_size, "lanczos")


def quantize_mask(mask_f32: np.ndarray) -> np.ndarray:
    """``(mask * 255).astype(np.uint8)`` (app.py:297) of a float32 mask in [0, 1]: an fp32 multiply, truncated; NaN gives 0."""
    t = np.asarray(mask_f32, np.float32) * np.float32(255.0)
    return np.where(np.isnan(t), np.float32(0.0), np.clip(t, 0, 255)).astype(np.uint8)


def resize_mask_reference_numpy(m8: np.ndarray, H: int, W: int) -> np.ndarray:
    """``Image.fromarray(m8).resize((W, H), LANCZOS)`` in numpy integers: horizontal pass, then vertical on the uint8 intermediate;
    a pass between equal lengths is skipped, as Pillow's need_horizontal / need_vertical skip it"""
    a = np.ascontiguousarray(m8, np.uint8)
    if a.shape[1] != W:
        a = resample_pass(a, W, "lanczos")
    if a.shape[0] != H:
        a = resample_pass(np.ascontiguousarray(a.T), H, "lanczos").T
    return np.ascontiguousarray(a)


def _blend(a: np.ndarray, b: np.ndarray, alpha: float) -> np.ndarray:
    """Blend.c on int32 planes: a + alpha * (b - a) in fp32, the product and the sum rounded separately -> float32"""
    return a.astype(np.float32) + np.float32(alpha) * (b - a).astype(np.float32)


def heatmap_reference_numpy(mask_u8: np.ndarray, rgb: np.ndarray, alpha: float = BLEND_ALPHA, brightness: float = BRIGHTNESS,
                            lut: np.ndarray = JET_RGBA) -> np.ndarray:
    """(H, W) uint8 resized mask + (H, W, 3) uint8 upload -> (H, W, 4) uint8: ``Brightness(blend(upload as RGBA, lut[mask], alpha))
    .enhance(brightness)``.  0 <= alpha <= 1 (Pillow's unclipped blend)."""
    H, W = mask_u8.shape
    o = np.concatenate([rgb, np.full((H, W, 1), 255, np.uint8)], 2).astype(np.int32)
    bl = _blend(o, lut[mask_u8].astype(np.int32), alpha).astype(np.uint8).astype(np.int32)
    deg = np.zeros_like(o)      # ImageEnhance.Brightness: a black image that keeps the enhanced image's alpha
    deg[..., 3] = bl[..., 3]
    t = _blend(deg, bl, brightness)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def present_reference_numpy(mask_f32: np.ndarray, rgb: np.ndarray, alpha: float = BLEND_ALPHA, brightness: float = BRIGHTNESS,
                            lut: np.ndarray = JET_RGBA):
    """(mh, mw) float32 mask in [0, 1] + (H, W, 3) uint8 upload -> ((H, W) uint8 mask, (H, W, 4) uint8 heat map), the two images
    of the reference's response."""
    H, W = rgb.shape[:2]
    m = resize_mask_reference_numpy(quantize_mask(mask_f32), H, W)
    return m, heatmap_reference_numpy(m, rgb, alpha, brightness, lut)
