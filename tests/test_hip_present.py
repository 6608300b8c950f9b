"""The response's images on the device (csrc/present.hip, ops.present_masks, SelfMaskInference.predict_images) against the integer
restatement that test_present_cpu.py pins to Pillow and matplotlib: zero tolerance, the reference is integer arithmetic."""
import threading
from argparse import Namespace

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from selfmask_amd import _native as N  # noqa: E402
from selfmask_amd import MaskFormer, SelfMaskInference, ops, synthetic_state_dict  # noqa: E402
from selfmask_amd import present as P  # noqa: E402
from _present_cases import KINDS, SHAPES, make_case, pil_heat, pil_mask  # noqa: E402

DEV = torch.device("cuda:0")
GUARD, FILL = 64, 0xA5
CFG = dict(n_queries=20, n_decoder_layers=6, learnable_pixel_decoder=False, lateral_connection=False,
           loss_every_decoder_layer=True, scale_factor=2, abs_2d_pe_init=False, use_binary_classifier=True,
           arch="vit_small", training_method="dino", patch_size=16)

_REF = {}


def _reference(i, kind):
    """the case and its expected images, computed once and handed out read-only"""
    if (i, kind) not in _REF:
        mask, rgb = make_case(i, kind)
        want = P.present_reference_numpy(mask, rgb)
        for a in (mask, rgb) + tuple(want):
            a.setflags(write=False)
        _REF[(i, kind)] = (mask, rgb, want[0], want[1])
    return _REF[(i, kind)]


def _run_abi(masks, rgbs, want_mask=True, want_heat=True, out=None):
    """One sm_present_masks_u8 call on buffers of the test's own: outputs packed back to back (px_off = the running pixel count, so
    most images start off a 4-pixel boundary), each followed by GUARD bytes, everything prefilled with FILL.  masks: list of
    (mh, mw) float32 of one shape.  -> (mask buffer, heat buffer, px_off list) on the host."""
    B = len(masks)
    mh, mw = masks[0].shape
    table = (N.PresentImage * B)()
    parts, ci, io, po = [], 0, 0, 0
    for b, rgb in enumerate(rgbs):
        H, W = rgb.shape[:2]
        d = table[b]
        d.img_off, d.px_off, d.H, d.W = io, po, H, W
        for n_in, n_out, key in ((mw, W, "x"), (mh, H, "y")):
            o = ks = 0
            if n_in != n_out:
                bounds, taps, ks = P.pil_lanczos_coeffs(n_in, n_out)
                o = ci
                parts += [bounds.reshape(-1), taps.reshape(-1)]
                ci += bounds.size + taps.size
            setattr(d, "coef_" + key, o)
            setattr(d, "ks" + key, ks)
        io += H * W * 3
        po += H * W + GUARD
    coef = torch.from_numpy(np.concatenate(parts + [np.zeros(1, np.int32)])).to(DEV)
    dev_table = torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).to(DEV)
    pixels = torch.from_numpy(np.concatenate([r.reshape(-1) for r in rgbs])).to(DEV)
    m = torch.from_numpy(np.stack(masks)).to(DEV)
    lut = torch.from_numpy(P.JET_RGBA.copy()).to(DEV)
    if out is None:
        out = (torch.full((po,), FILL, dtype=torch.uint8, device=DEV), torch.full((4 * po,), FILL, dtype=torch.uint8, device=DEV))
    lib = N.load()
    max_w = max(r.shape[1] for r in rgbs)
    ws_bytes = lib.sm_present_workspace_bytes(B, mh, max_w)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    N.check(lib.sm_present_masks_u8(m.data_ptr(), m.stride(0), mh, mw, pixels.data_ptr(), table, dev_table.data_ptr(), coef.data_ptr(),
                                    lut.data_ptr(), 0.5, 1.1, out[0].data_ptr() if want_mask else None,
                                    out[1].data_ptr() if want_heat else None, ws.data_ptr(), ws_bytes, B,
                                    torch.cuda.current_stream().cuda_stream), "sm_present_masks_u8")
    torch.cuda.synchronize()
    return out[0].cpu().numpy(), out[1].cpu().numpy(), [table[b].px_off for b in range(B)], out


def _check_packed(mask_buf, heat_buf, px_off, rgbs, wants, mask_written=True, heat_written=True):
    for po, rgb, (wm, wh) in zip(px_off, rgbs, wants):
        n = rgb.shape[0] * rgb.shape[1]
        if mask_written:
            assert np.array_equal(mask_buf[po:po + n], wm.reshape(-1))
        else:
            assert (mask_buf[po:po + n] == FILL).all()
        if heat_written:
            assert np.array_equal(heat_buf[4 * po:4 * (po + n)], wh.reshape(-1))
        else:
            assert (heat_buf[4 * po:4 * (po + n)] == FILL).all()
        assert (mask_buf[po + n:po + n + GUARD] == FILL).all() and (heat_buf[4 * (po + n):4 * (po + n + GUARD)] == FILL).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_mask_and_heatmap_equal_the_reference(i, kind):
    mask, rgb, wm, wh = _reference(i, kind)
    mask_buf, heat_buf, px_off, _ = _run_abi([mask], [rgb])
    _check_packed(mask_buf, heat_buf, px_off, [rgb], [(wm, wh)])
    if kind == "hard" and min(rgb.shape[:2]) > 56:
        assert wm.min() == 0 and wm.max() == 255  # both clips fired


@pytest.mark.parametrize("i", [1, 2])
def test_a_null_output_is_left_alone(i):
    mask, rgb, wm, wh = _reference(i, "uniform")
    mask_buf, heat_buf, px_off, _ = _run_abi([mask], [rgb], want_heat=False)
    _check_packed(mask_buf, heat_buf, px_off, [rgb], [(wm, wh)], heat_written=False)
    mask_buf, heat_buf, px_off, _ = _run_abi([mask], [rgb], want_mask=False)
    _check_packed(mask_buf, heat_buf, px_off, [rgb], [(wm, wh)], mask_written=False)


def test_images_of_one_call_are_independent():
    """three sizes in one call, in either table order: per image the bytes of its own single call"""
    cases = [_reference(i, "clipped_normal") for i in (0, 2, 6)]  # (28, 28) -> 300 x 400, 17 x 23, 5 x 300
    single = []
    for mask, rgb, wm, wh in cases:
        mb, hb, _, _ = _run_abi([mask], [rgb])
        n = rgb.shape[0] * rgb.shape[1]
        single.append((mb[:n].copy(), hb[:4 * n].copy()))
        assert np.array_equal(single[-1][0], wm.reshape(-1)) and np.array_equal(single[-1][1], wh.reshape(-1))
    for order in ((0, 1, 2), (2, 1, 0)):
        sel = [cases[k] for k in order]
        mb, hb, px_off, _ = _run_abi([c[0] for c in sel], [c[1] for c in sel])
        assert any(po % 4 for po in px_off)  # a group cut that is not the image's own
        for k, po in zip(order, px_off):
            n = single[k][0].size
            assert np.array_equal(mb[po:po + n], single[k][0]) and np.array_equal(hb[4 * po:4 * (po + n)], single[k][1])
        _check_packed(mb, hb, px_off, [c[1] for c in sel], [(c[2], c[3]) for c in sel])


def test_nan_quantises_to_zero():
    mask, rgb, _, _ = _reference(4, "uniform")
    mask = mask.copy()
    mask[3, 5] = np.nan
    wm, wh = P.present_reference_numpy(mask, rgb)
    mask_buf, heat_buf, px_off, _ = _run_abi([mask], [rgb])
    _check_packed(mask_buf, heat_buf, px_off, [rgb], [(wm, wh)])


def test_ops_present_masks_host_and_device():
    cases = [_reference(i, "uniform") for i in (0, 2, 8)]
    masks = torch.from_numpy(np.stack([c[0] for c in cases])).to(DEV)
    rgbs = [c[1] for c in cases]
    for _ in range(2):  # the second call finds its tables cached on the device
        got = ops.present_masks(masks, rgbs)
        for (gm, gh), (_, _, wm, wh) in zip(got, cases):
            assert isinstance(gm, np.ndarray) and np.array_equal(gm, wm) and np.array_equal(gh, wh)
    got = ops.present_masks(masks, rgbs, host=False)
    for (gm, gh), (_, _, wm, wh) in zip(got, cases):
        assert gm.is_cuda and np.array_equal(gm.cpu().numpy(), wm) and np.array_equal(gh.cpu().numpy(), wh)
    (gm, gh), = ops.present_masks(masks[:1], rgbs[:1], want_heat=False)
    assert gh is None and np.array_equal(gm, cases[0][2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.present_masks(masks.cpu(), rgbs)


def test_skipped_passes_share_a_batch_with_resampled_ones():
    """one call, a 4 x 6 mask onto sizes that skip both passes, either one and neither (ks = 0 markers beside shared tables)"""
    rng = np.random.Generator(np.random.PCG64(46))
    mask = rng.random((4, 6), dtype=np.float32)
    rgbs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(4, 6), (4, 9), (7, 6), (1, 1), (9, 13)]]
    got = ops.present_masks(torch.from_numpy(np.stack([mask] * len(rgbs))).to(DEV), rgbs)
    for (gm, gh), rgb in zip(got, rgbs):
        wm, wh = P.present_reference_numpy(mask, rgb)
        assert np.array_equal(gm, wm) and np.array_equal(gh, wh), rgb.shape
    assert np.array_equal(got[0][0], P.quantize_mask(mask))  # both passes skipped: the quantised mask itself


# ---- the serving class --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inference():
    m = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    m.load_state_dict(synthetic_state_dict(2, "soft", patch_size=16), strict=True)
    return SelfMaskInference(None, Namespace(**CFG), device=DEV, model=m)


def _uploads():
    rng = np.random.Generator(np.random.PCG64(77))
    return [rng.integers(0, 256, size=(37, 53, 3), dtype=np.uint8), rng.integers(0, 256, size=(300, 400, 3), dtype=np.uint8)]


def _url(img):
    import base64
    from io import BytesIO
    buf = BytesIO()
    img.save(buf, format="PNG")
    return "data:image/png;base64," + base64.b64encode(buf.getvalue()).decode()


def test_predict_images_mask_equals_the_host_chain(inference):
    for rgb in _uploads():
        t = inference.predict_tensors(rgb)
        want = pil_mask(t["mask"], rgb.shape[0], rgb.shape[1])
        got = inference.predict_images(rgb)
        assert got["mask"].dtype == np.uint8 and np.array_equal(got["mask"], np.array(want))
        assert got["best_idx"] == t["best_idx"] and np.array_equal(got["objectness_scores"], t["objectness_scores"])
        assert np.array_equal(got["heatmap"], P.heatmap_reference_numpy(np.array(want), rgb))
        r = inference.predict(rgb)
        assert r["mask"] == _url(want) and r["original"] == _url(Image.fromarray(rgb))
        assert r["heatmap"].startswith("data:image/png;base64,") and r["best_idx"] == t["best_idx"]
    g = inference.base_structure._graphed
    assert g.failed is None and g.captures == 1 and g.replays >= 5  # one capture, every later call a replay


def test_predict_heatmap_equals_the_host_chain(inference):
    pytest.importorskip("matplotlib")
    for rgb in _uploads():
        t = inference.predict_tensors(rgb)
        want = pil_heat(pil_mask(t["mask"], rgb.shape[0], rgb.shape[1]), rgb)
        got = inference.predict_images(rgb)
        assert got["heatmap"].shape == rgb.shape[:2] + (4,) and np.array_equal(got["heatmap"], np.array(want))
        assert inference.predict(rgb)["heatmap"] == _url(want)


def test_concurrent_requests_get_their_own_images(inference):
    """the pattern of test_hip_inference.py: eight threads x four requests, every thread over images of its own"""
    rng = np.random.Generator(np.random.PCG64(13))
    imgs = [[rng.integers(0, 256, size=(40 + 7 * t + 3 * k, 90 - 5 * t + k, 3), dtype=np.uint8) for k in range(2)] for t in range(8)]
    want = [[inference.predict_images(im) for im in per] for per in imgs]
    errors = []

    def worker(t):
        try:
            for k in range(4):
                got, w = inference.predict_images(imgs[t][k % 2]), want[t][k % 2]
                if got["best_idx"] != w["best_idx"] or not np.array_equal(got["mask"], w["mask"]) \
                        or not np.array_equal(got["heatmap"], w["heatmap"]):
                    errors.append((t, k))
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
