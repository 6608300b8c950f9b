"""Plain-numpy restatement of the back half of a baseline JPEG decode as libjpeg-turbo does it at Pillow's defaults
(JDCT_ISLOW, fancy up-sampling): dequantise, islow IDCT, chroma up-sampling, YCbCr -> RGB.  Input: what
``sm_jpeg_entropy_decode`` wrote (coefficients, quantisation tables, the header's numbers).  The reference of
tests/test_jpeg_cpu.py (pinned against Pillow bit for bit) and of tests/test_hip_jpeg.py, plus the generated test files
both share.  Integer arithmetic in int64 with a check that int32 - the device's width - would have held every value."""
import ctypes as C
import io

import numpy as np
from PIL import Image

from selfmask_amd import _native as N

GRAY, S444, S422, S420 = range(4)
CONST_BITS, PASS1_BITS = 13, 2
(F_0_298631336, F_0_390180644, F_0_541196100, F_0_765366865, F_0_899976223, F_1_175875602, F_1_501321110, F_1_847759065,
 F_1_961570560, F_2_053119869, F_2_562915447, F_3_072711026) = (2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819,
                                                                20995, 25172)
I32 = 2 ** 31


def _fits(*arrays):
    for a in arrays:
        assert a.min() >= -I32 and a.max() < I32, "an IDCT intermediate leaves 32 bits"


def _idct8(x, shift):
    """one pass of jpeg_idct_islow along the LAST axis of x (..., 8) int64"""
    i0, i1, i2, i3, i4, i5, i6, i7 = (x[..., k] for k in range(8))
    z1 = (i2 + i6) * F_0_541196100
    tmp2 = z1 + i6 * (-F_1_847759065)
    tmp3 = z1 + i2 * F_0_765366865
    tmp0 = (i0 + i4) << CONST_BITS
    tmp1 = (i0 - i4) << CONST_BITS
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175875602
    t0, t1, t2, t3 = t0 * F_0_298631336, t1 * F_2_053119869, t2 * F_3_072711026, t3 * F_1_501321110
    z1, z2, z3, z4 = z1 * -F_0_899976223, z2 * -F_2_562915447, z3 * -F_1_961570560 + z5, z4 * -F_0_390180644 + z5
    _fits(z1, z2, z3, z4, z5, t0, t1, t2, t3)
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    r = 1 << (shift - 1)
    outs = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
    _fits(t0, t1, t2, t3, tmp10, tmp11, tmp12, tmp13, *[o + r for o in outs])
    return np.stack([(o + r) >> shift for o in outs], axis=-1)


def idct_blocks(coef, qt):
    """coef (n, 8, 8) int16 natural order, qt (64,) -> (n, 8, 8) uint8 samples"""
    x = coef.astype(np.int64) * qt.astype(np.int64).reshape(1, 8, 8)
    ws = _idct8(x.transpose(0, 2, 1), CONST_BITS - PASS1_BITS).transpose(0, 2, 1)  # columns
    out = _idct8(ws, CONST_BITS + PASS1_BITS + 3)                                   # rows
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def plane(samples, bh, bw):
    """(bh * bw, 8, 8) blocks in raster order -> (bh * 8, bw * 8) plane"""
    return samples.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample_h2v1(s, W):
    """s (h, cw) real down-sampled samples -> (h, W); libjpeg picks the triangle filter only when cw > 2"""
    s = s.astype(np.int64)
    cw = s.shape[1]
    if cw <= 2:
        return np.repeat(s, 2, axis=1)[:, :W]
    prev = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    nxt = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    even = (3 * s + prev + 1) >> 2
    odd = (3 * s + nxt + 2) >> 2
    even[:, 0], odd[:, -1] = s[:, 0], s[:, -1]
    out = np.empty((s.shape[0], 2 * cw), np.int64)
    out[:, 0::2], out[:, 1::2] = even, odd
    return out[:, :W]


def upsample_h2v2(s, H, W):
    """s (ch, cw) real down-sampled samples -> (H, W)"""
    s = s.astype(np.int64)
    ch, cw = s.shape
    if cw <= 2:
        return np.repeat(np.repeat(s, 2, axis=0), 2, axis=1)[:H, :W]
    up = np.concatenate([s[:1], s[:-1]], axis=0)    # the row above, the first row repeated
    down = np.concatenate([s[1:], s[-1:]], axis=0)  # the row below, the last row repeated
    rows = np.empty((2 * ch, cw), np.int64)
    rows[0::2], rows[1::2] = 3 * s + up, 3 * s + down
    prev = np.concatenate([rows[:, :1], rows[:, :-1]], axis=1)
    nxt = np.concatenate([rows[:, 1:], rows[:, -1:]], axis=1)
    even = (3 * rows + prev + 8) >> 4
    odd = (3 * rows + nxt + 7) >> 4
    even[:, 0] = (4 * rows[:, 0] + 8) >> 4
    odd[:, -1] = (4 * rows[:, -1] + 7) >> 4
    out = np.empty((2 * ch, 2 * cw), np.int64)
    out[:, 0::2], out[:, 1::2] = even, odd
    return out[:H, :W]


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def entropy_decode(data: bytes):
    """-> (rc, info, coef int16 array, qt uint16 (3, 64)) through the library's host half"""
    lib = N.load()
    info = N.JpegInfo()
    assert lib.sm_jpeg_probe(data, len(data), info) == 0
    n = max(int(info.coef_bytes), 16) if info.supported else 16
    coef = np.zeros(n // 2, np.int16)
    qt = np.zeros((3, 64), np.uint16)
    info2 = N.JpegInfo()
    rc = lib.sm_jpeg_entropy_decode(data, len(data), coef.ctypes.data, coef.nbytes, qt.ctypes.data, info2)
    if info.supported:
        assert bytes(info) == bytes(info2) or rc != 0
    return rc, info2, coef, qt


def back_half(info, coef, qt):
    """-> (H, W, 3) uint8, what Image.open(f).convert("RGB") gives"""
    H, W, nc = info.height, info.width, info.components
    planes, o = [], 0
    for c in range(nc):
        bh, bw = info.blocks_h[c], info.blocks_w[c]
        n = bh * bw
        planes.append(plane(idct_blocks(coef[o:o + n * 64].reshape(n, 8, 8), qt[c]), bh, bw))
        o += n * 64
    y = planes[0][:H, :W]
    if nc == 1:
        return np.stack([y, y, y], axis=-1)
    if info.sampling == S444:
        cb, cr = planes[1][:H, :W], planes[2][:H, :W]
    elif info.sampling == S422:
        cw = (W + 1) // 2
        cb, cr = (upsample_h2v1(p[:H, :cw], W) for p in planes[1:])
    else:
        ch, cw = (H + 1) // 2, (W + 1) // 2
        cb, cr = (upsample_h2v2(p[:ch, :cw], H, W) for p in planes[1:])
    return ycc_to_rgb(y, cb, cr)


# ---- generated files: the case matrix of the device test ---------------------------------------------------------------------
SIZES = [(1, 1), (8, 8), (16, 16), (17, 17), (16, 33), (37, 53), (64, 48)]  # (H, W)
QUALITIES = (30, 85, 100)


def content(kind, h, w, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == "noise":  # at quality 100 this drives coefficients and clamps to their extremes
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    img = np.stack([255 * xx / max(w - 1, 1), 255 * yy / max(h - 1, 1), 255 * (xx + yy) / max(h + w - 2, 1)], axis=-1)
    img[:, w // 2:] = 255 - img[:, w // 2:]  # a sharp vertical edge through a smooth colour gradient
    img[h // 3:h // 3 + 2] = (250, 10, 30)
    return img.astype(np.uint8)


def encode(rgb, mode="RGB", **save):
    im = Image.fromarray(rgb)
    if mode != "RGB":
        im = im.convert(mode)
    buf = io.BytesIO()
    im.save(buf, "JPEG", **save)
    return buf.getvalue()


def pillow_pixels(data: bytes):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), np.uint8)


def case_matrix():
    """-> list of (case id, file bytes): every size x (subsampling 0 / 1 / 2, mode L) x quality x content kind, plus optimize=True
    and restart_marker_blocks=2 once per sampling"""
    cases = []
    seed = 0
    for (h, w) in SIZES:
        for samp in (0, 1, 2, "L"):
            for q in QUALITIES:
                for kind in ("edge", "noise"):
                    seed += 1
                    rgb = content(kind, h, w, seed)
                    data = encode(rgb, "L", quality=q) if samp == "L" else encode(rgb, quality=q, subsampling=samp)
                    cases.append((f"{h}x{w}-s{samp}-q{q}-{kind}", data))
    for samp in (0, 1, 2, "L"):
        for extra, kw in (("optimize", dict(optimize=True)), ("restart", dict(restart_marker_blocks=2))):
            seed += 1
            rgb = content("edge" if extra == "optimize" else "noise", 37, 53, seed)
            data = encode(rgb, "L", quality=85, **kw) if samp == "L" else encode(rgb, quality=85, subsampling=samp, **kw)
            cases.append((f"37x53-s{samp}-q85-{extra}", data))
    return cases


def unsupported_files():
    """-> {name: bytes}: files the device path must leave to Pillow.  "truncated": a baseline file cut in the middle of its scan and
    closed by EOI, which Pillow still opens (libjpeg pads the missing MCUs)"""
    rgb = content("edge", 37, 53, 1001)
    base = encode(content("noise", 64, 48, 1002), quality=85, subsampling=2)
    png = io.BytesIO()
    Image.fromarray(rgb).save(png, "PNG")
    return {"progressive": encode(rgb, quality=85, progressive=True), "cmyk": encode(rgb, "CMYK", quality=85), "png": png.getvalue(),
            "empty": b"", "truncated": base[:len(base) * 2 // 3] + b"\xff\xd9"}
