"""Host half of the device JPEG decode, without a GPU: the library's entropy decoder feeds tests/_jpeg_ref.py (plain numpy:
dequantise, islow IDCT, fancy up-sampling, YCbCr -> RGB), whose output must be Pillow's bit for bit on the whole case matrix of
the device test - the specification the kernels restate is pinned against this environment's Pillow before any kernel runs."""
import numpy as np
import pytest

import _jpeg_ref as R
from selfmask_amd import _native as N
from selfmask_amd import jpeg as J
from selfmask_amd.pipeline import packed_pixel_offsets

CASES = R.case_matrix()


@pytest.mark.parametrize("cid,data", CASES, ids=[c[0] for c in CASES])
def test_back_half_restated_in_numpy_equals_pillow(cid, data):
    rc, info, coef, qt = R.entropy_decode(data)
    assert rc == 0 and info.supported == 1, "every file of the matrix is a single-scan baseline file"
    ref = R.pillow_pixels(data)
    assert (info.height, info.width) == ref.shape[:2]
    out = R.back_half(info, coef, qt)
    assert out.dtype == np.uint8 and np.array_equal(out, ref), f"{int((out != ref).sum())} bytes differ from Pillow"


def test_supported_kinds_are_reported_supported():
    rgb = R.content("edge", 37, 53, 5)
    files = {"default": R.encode(rgb), "optimize": R.encode(rgb, optimize=True), "restart": R.encode(rgb, restart_marker_blocks=2),
             "L": R.encode(rgb, "L")}
    files.update({f"subsampling={s}": R.encode(rgb, subsampling=s) for s in (0, 1, 2)})
    for name, data in files.items():
        h = J.probe_jpeg(data)
        assert h.supported and (h.height, h.width) == (37, 53), name
        assert h.components == (1 if name == "L" else 3), name
        assert h.coef_bytes > 0 and h.coef_bytes % 128 == 0, name
    assert J.probe_jpeg(files["subsampling=0"]).sampling == N.JPEG_444
    assert J.probe_jpeg(files["subsampling=1"]).sampling == N.JPEG_422
    assert J.probe_jpeg(files["subsampling=2"]).sampling == N.JPEG_420
    assert J.probe_jpeg(files["L"]).sampling == N.JPEG_GRAY
    assert N.JpegInfo.restart_interval.offset > 0 and R.entropy_decode(files["restart"])[1].restart_interval > 0


def test_unsupported_kinds_are_reported_unsupported_without_a_crash(tmp_path):
    lib = N.load()
    for name, data in R.unsupported_files().items():
        info = N.JpegInfo()
        assert lib.sm_jpeg_probe(data, len(data), info) == 0, name
        coef, qt = np.zeros(1 << 16, np.int16), np.zeros(192, np.uint16)
        out = N.JpegInfo()
        rc = lib.sm_jpeg_entropy_decode(data, len(data), coef.ctypes.data, coef.nbytes, qt.ctypes.data, out)
        assert rc == N.JPEG_UNSUPPORTED and out.supported == 0, name
        if name == "truncated":  # the header is fine: only the scan shows it
            assert info.supported == 1
        else:
            assert info.supported == 0, name
            assert not J.probe_jpeg(data).supported
    p = tmp_path / "p.jpg"
    p.write_bytes(R.unsupported_files()["progressive"])
    h = J.probe_jpeg(str(p))
    assert not h.supported and (h.height, h.width, h.components) == (37, 53, 3)
    # room for fewer coefficients than the file has: refused, nothing written past the buffer
    data = CASES[-1][1]
    small = np.zeros(8, np.int16)
    assert lib.sm_jpeg_entropy_decode(data, len(data), small.ctypes.data, small.nbytes, qt.ctypes.data, out) == -3
    assert lib.sm_jpeg_probe(None, 0, out) == -1 and b"null pointer" in lib.sm_last_error()


def test_every_truncation_of_a_small_file_is_success_or_unsupported():
    data = R.encode(R.content("noise", 17, 17, 9), quality=85, subsampling=2, restart_marker_blocks=1)
    lib = N.load()
    coef, qt, out = np.zeros(1 << 14, np.int16), np.zeros(192, np.uint16), N.JpegInfo()
    for n in range(len(data)):
        rc = lib.sm_jpeg_entropy_decode(data[:n], n, coef.ctypes.data, coef.nbytes, qt.ctypes.data, out)
        assert rc == N.JPEG_UNSUPPORTED, n  # a file cut anywhere lacks its EOI at least
    assert lib.sm_jpeg_entropy_decode(data, len(data), coef.ctypes.data, coef.nbytes, qt.ctypes.data, out) == 0


def test_packed_layout_is_the_pipelines():
    shapes = [(1, 1), (8, 8), (17, 17), (16, 33), (37, 53), (64, 48), (5, 7)]
    offs, total = J.packed_layout(shapes)
    assert offs == packed_pixel_offsets(shapes)
    assert all(o % 16 == 0 for o in offs) and total == offs[-1] + ((5 * 7 * 3 + 15) & ~15)
    assert J.packed_layout([(1, 1)]) == ([0], 16)


def test_idct_stays_inside_32_bits_at_full_range():
    """quality 100 (every divisor 1) with coefficients at the extremes a forward DCT of 8-bit samples reaches: the blocks of a
    +-128 checkerboard and of +-128 stripes, and uniform noise - _jpeg_ref asserts every intermediate fits int32"""
    yy, xx = np.mgrid[:8, :8]
    blocks = [np.where((yy + xx) % 2 == 0, 255, 0), np.where(xx % 2 == 0, 255, 0), np.where(yy < 4, 255, 0), np.full((8, 8), 255),
              np.random.Generator(np.random.PCG64(3)).integers(0, 256, (8, 8))]
    img = np.concatenate([np.stack([b, b, b], axis=-1).astype(np.uint8) for b in blocks], axis=1)
    data = R.encode(img, quality=100, subsampling=0)
    rc, info, coef, qt = R.entropy_decode(data)
    assert rc == 0 and int(qt.max()) == 1 and int(np.abs(coef).max()) >= 1000
    assert np.array_equal(R.back_half(info, coef, qt), R.pillow_pixels(data))


def test_predictor_decode_option_is_validated():
    from selfmask_amd.predictor import SaliencyPredictor, build_parser
    with pytest.raises(ValueError, match="decode="):
        SaliencyPredictor(object(), device="cuda:0", decode="gpu")
    args = build_parser().parse_args(["--config", "c", "--p_state_dict", "s", "--images", "i", "--out", "o", "--decode", "device"])
    assert args.decode == "device"
    assert build_parser().parse_args(["--config", "c", "--p_state_dict", "s", "--images", "i", "--out", "o"]).decode == "host"


def test_a_header_that_promises_more_than_the_file_holds_is_cheap_and_goes_to_pillow(tmp_path):
    """a few hundred bytes that claim 65500 x 65500: the entropy decoder stops at the first MCU past the data, and the Python
    surface sizes nothing from such a header"""
    import time
    data = bytearray(R.encode(R.content("edge", 16, 16, 3), quality=85, subsampling=2))
    at = data.index(b"\xff\xc0") + 5
    data[at:at + 4] = bytes([0xFF, 0xDC, 0xFF, 0xDC])  # height, width = 65500
    data = bytes(data)
    lib = N.load()
    info = N.JpegInfo()
    assert lib.sm_jpeg_probe(data, len(data), info) == 0 and info.supported == 1 and info.coef_bytes > 1 << 33
    h = J.probe_jpeg(data)
    assert (h.height, h.width) == (65500, 65500) and not h.supported
    small = R.encode(R.content("edge", 16, 16, 3), quality=85, subsampling=2)
    cut = bytearray(small[:len(small) - 30] + b"\xff\xd9")
    at = cut.index(b"\xff\xc0") + 5
    cut[at:at + 4] = bytes([0x10, 0x00, 0x10, 0x00])  # 4096 x 4096: 50 MB of coefficients promised, one MCU delivered
    coef, qt, out = np.zeros(4096 * 4096 * 3 // 2, np.int16), np.zeros(192, np.uint16), N.JpegInfo()
    t = time.perf_counter()
    rc = lib.sm_jpeg_entropy_decode(bytes(cut), len(cut), coef.ctypes.data, coef.nbytes, qt.ctypes.data, out)
    dt = time.perf_counter() - t
    assert rc == N.JPEG_UNSUPPORTED
    assert dt < 0.5, f"{dt:.2f} s: the decoder went on past the end of the data"  # clearing the buffer is ~10 ms, 65 536 MCUs of zeros far more
    p = tmp_path / "long_header.jpg"
    p.write_bytes(small[:20] + b"\xff\xfe\xff\xff" + bytes(65533) + b"\xff\xfe\xff\xff" + bytes(65533) + small[20:])
    assert J.probe_jpeg(str(p)) == J.probe_jpeg(small)  # the scan header lies beyond the 64 KiB prefix
