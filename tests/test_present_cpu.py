"""CPU-only checks of the response's images (selfmask_amd/present.py, csrc/present.hip): the integer restatement equals Pillow and
matplotlib bit for bit, the colour table is pinned, and the C ABI's arguments are validated on the host before any launch (its
layout and exports: tests/test_abi_cpu.py)."""
import hashlib

import numpy as np
import pytest

from selfmask_amd import _native as N
from selfmask_amd import present as P
from _present_cases import KINDS, SHAPES, make_case, pil_heat, pil_mask

CASES = [(i, k) for i in range(len(SHAPES)) for k in KINDS]


@pytest.mark.parametrize("i,kind", CASES)
def test_mask_resize_equals_pillow_lanczos(i, kind):
    mask, rgb = make_case(i, kind)
    H, W = rgb.shape[:2]
    got, _ = P.present_reference_numpy(mask, rgb)
    want = np.array(pil_mask(mask, H, W))
    assert got.dtype == np.uint8 and got.shape == (H, W)
    assert np.array_equal(got, want)
    if kind == "hard" and min(H, W) > 56:
        assert got.min() == 0 and got.max() == 255


def test_lanczos_tap_counts():
    assert P.pil_lanczos_coeffs(28, 300)[2] == 7 and P.pil_lanczos_coeffs(28, 17)[2] == 11
    assert P.pil_lanczos_coeffs(56, 1)[2] == 337 and P.pil_lanczos_coeffs(448, 1)[2] == 2689
    bounds, taps, ks = P.pil_lanczos_coeffs(28, 17)
    assert bounds.shape == (17, 2) and taps.shape == (17, ks) and bounds.dtype == np.int32 and taps.dtype == np.int32
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= 28).all() and (bounds[:, 1] <= ks).all()


@pytest.mark.parametrize("n_in,n_out,want", [(28, 300, ("abdbff08a826d165", 7)), (28, 17, ("34a24bd360e154c7", 11)),
                                             (56, 1, ("3d1e8acc2b064e1c", 337)), (1, 9, ("6595c8f17eb42ba3", 7)),
                                             (28, 29, ("6ef37bf9d90c95c0", 7)), (448, 1, ("82f64c4a315f7bc4", 2689))])
def test_lanczos_tables_are_the_recorded_ones(n_in, n_out, want):
    """digests of the tables as they stood before resample.pil_coeffs became the one builder"""
    from selfmask_amd.resample import pil_coeffs
    bounds, taps, ks = pil_coeffs(n_in, n_out, "lanczos")
    assert (hashlib.sha256(bounds.tobytes() + taps.tobytes() + str(ks).encode()).hexdigest()[:16], ks) == want
    assert all(a is b for a, b in zip(P.pil_lanczos_coeffs(n_in, n_out), (bounds, taps, ks)))  # the old name: a binding, one cache


EDGE_MASKS = [(mh, mw, H, W) for mh, mw in [(1, 1), (2, 3), (28, 28)]
              for H, W in [(1, 1), (1, 9), (9, 1), (mh, mw), (mh, 5), (3, mw), (57, 64)]]


@pytest.mark.parametrize("mh,mw,H,W", EDGE_MASKS)
def test_mask_resize_equals_pillow_lanczos_at_the_edges(mh, mw, H, W):
    """one-pixel masks and outputs, and each pass skipped alone or with the other (equal lengths, as Pillow skips it)"""
    from PIL import Image
    m8 = np.random.Generator(np.random.PCG64([mh, mw, H, W])).integers(0, 256, (mh, mw), dtype=np.uint8)
    got = P.resize_mask_reference_numpy(m8, H, W)
    assert got.dtype == np.uint8 and got.flags.c_contiguous
    assert np.array_equal(got, np.array(Image.fromarray(m8).resize((W, H), Image.Resampling.LANCZOS)))


@pytest.mark.parametrize("i,kind", CASES)
def test_heatmap_equals_the_reference_chain(i, kind):
    pytest.importorskip("matplotlib")
    mask, rgb = make_case(i, kind)
    H, W = rgb.shape[:2]
    got_mask, got_heat = P.present_reference_numpy(mask, rgb)
    want = pil_heat(pil_mask(mask, H, W), rgb)
    assert want.mode == "RGBA"
    assert np.array_equal(got_heat, np.array(want))


def test_pinned_table_equals_matplotlib_jet():
    plt = pytest.importorskip("matplotlib.pyplot")
    cm = plt.get_cmap("jet")
    assert cm.N == 256
    assert np.array_equal(P.JET_RGBA, (cm(np.arange(256)) * 255).astype(np.uint8))
    assert np.array_equal(P.JET_RGBA, (cm(np.arange(256) / 255.0) * 255).astype(np.uint8))  # cmap(v / 255.0) is entry v


def test_pinned_table_digest():
    assert P.JET_RGBA.shape == (256, 4) and P.JET_RGBA.dtype == np.uint8
    assert hashlib.sha256(P.JET_RGBA.tobytes()).hexdigest() == P.JET_RGBA_SHA256 == \
        "878b65944cde43dd8015035710be8c53357a64fa2fbc6eae358ee5257a876b8e"


def test_library_exports_the_present_symbols():
    lib = N.load()
    assert lib.sm_present_workspace_bytes(1, 28, 400) >= 28 * 400
    assert lib.sm_present_workspace_bytes(3, 56, 1920) >= 3 * 56 * 1920
    for bad in ((0, 28, 400), (1, 0, 400), (1, 513, 400), (1, 28, 0), (65536, 28, 400)):
        assert lib.sm_present_workspace_bytes(*bad) == 0


def _valid_call():
    """arguments that pass every check (the pointers are never followed: each test breaks one argument, and validation returns
    before any launch)"""
    mh = mw = 28
    H, W = 30, 40
    table = (N.PresentImage * 1)()
    d = table[0]
    d.img_off, d.px_off, d.H, d.W, d.coef_x, d.coef_y, d.ksx, d.ksy = 0, 0, H, W, 0, 1000, 7, 7
    ws = N.load().sm_present_workspace_bytes(1, mh, W)
    fake = 0x10000  # non-null, 16-byte aligned
    return dict(masks=fake, stride=mh * mw, mh=mh, mw=mw, rgb=fake, host=table, dev=fake, coef=fake, lut=fake, alpha=0.5, brightness=1.1,
                mask_out=fake, heat_out=fake, ws=fake, ws_bytes=ws, B=1)


def _call(a):
    return N.load().sm_present_masks_u8(a["masks"], a["stride"], a["mh"], a["mw"], a["rgb"], a["host"], a["dev"], a["coef"], a["lut"],
                                        a["alpha"], a["brightness"], a["mask_out"], a["heat_out"], a["ws"], a["ws_bytes"], a["B"], None)


@pytest.mark.parametrize("change,message", [
    (dict(masks=None), b"null pointer"),
    (dict(B=0), b"B=0"),
    (dict(mh=513), b"mask 513 x 28"),
    (dict(ws_short=1), b"workspace"),
    (dict(mask_out=None, heat_out=None), b"null pointer"),
    (dict(heat_out=0x10004), b"misaligned"),
])
def test_argument_validation_without_gpu(change, message):
    a = _valid_call()
    if "ws_short" in change:
        a["ws_bytes"] -= change["ws_short"]  # one byte short
    else:
        a.update(change)
    assert _call(a) == -1
    assert message in N.load().sm_last_error(), N.load().sm_last_error()


def test_image_table_validation_without_gpu():
    lib = N.load()
    for field, value, message in (("H", 0, b"image 0 is 0 x 40"), ("W", 1 << 24, b"at most"), ("ksx", 0, b"skipped pass"), ("px_off", -4, b"negative")):
        a = _valid_call()
        setattr(a["host"][0], field, value)
        assert _call(a) == -1 and message in lib.sm_last_error(), (field, lib.sm_last_error())
