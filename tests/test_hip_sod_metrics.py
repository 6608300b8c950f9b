"""E-measure and weighted F-measure on the device (csrc/sod_metrics.hip behind ``ops.sod_metrics``, ``ops.upsample_selected_u8``,
``ops.evaluate_masks(extra=True)`` and ``Evaluator(extra_metrics=True)``) against the numpy definition, selfmask_amd/sod_metrics.py.

Bounds.  The histograms are integers: equal.  E is a dozen fp64 operations on exact integer counts: 1e-12 is four orders above its
rounding.  The weighted sums add up to 1.3e5 terms per image in an order that differs from numpy's pairwise sum (worst-case relative
error n 2^-53 = 1.4e-11) and the device's fp64 exp adds an ulp or two: 1e-10.  The largest differences seen are printed."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _sod_metrics_ref as R  # noqa: E402
from selfmask_amd import ops  # noqa: E402
from selfmask_amd import sod_metrics as S  # noqa: E402

DEV = "cuda:0"
E_TOL, W_TOL = 1e-12, 1e-10


def _big_cases():
    out = []
    for name, kind, H, W, seed in (("speckle_64x61", "speckle", 64, 61, 3),
                                   ("strip_130x2049", "speckle", 130, 2049, 4),   # a row longer than a chunk: chunk ends inside rows
                                   ("rect_300x400", "rect", 300, 400, 5),
                                   ("blob_300x400", "blob", 300, 400, 6),
                                   ("wide_9x2600", "speckle", 9, 2600, 7)):      # rows too long for the LDS window: global taps
        gt = R.make_gt(kind, H, W, seed=seed)
        out.append((name, R.make_pred(gt, seed=seed), gt))
    return out


CASES = R.small_cases() + _big_cases()
BY_NAME = {c[0]: c for c in CASES}
MIXED = ("speckle_37x53", "strip_130x2049", "empty_5x3", "rect_300x400", "checker_9x1")


@functools.lru_cache(maxsize=None)
def _ref(name):
    """the definition's row and histograms of a case, computed once"""
    _, p8, gt = BY_NAME[name]
    return S.sod_metrics(p8, gt), S.histograms(p8, gt)


def _run(names, return_hist=True):
    preds = [torch.from_numpy(BY_NAME[n][1]).to(DEV) for n in names]
    gts = [torch.from_numpy(BY_NAME[n][2]).to(DEV) for n in names]
    return ops.sod_metrics(preds, gts, return_hist=return_hist)


def _check(names, out, hist):
    out, hist = out.cpu().numpy(), hist.cpu().numpy()
    assert out.shape == (len(names), 4) and out.dtype == np.float64 and hist.shape == (len(names), 2, 256) and hist.dtype == np.int32
    for b, n in enumerate(names):
        want, want_hist = _ref(n)
        assert np.array_equal(hist[b], want_hist), n
        d = np.abs(out[b] - want)
        print(f"\n{n}: e_adp {d[0]:.2e} e_mean {d[1]:.2e} e_max {d[2]:.2e} wfm {d[3]:.2e}  (wfm = {want[3]:.6f})")
        assert d[:3].max() <= E_TOL, (n, out[b], want)
        assert d[3] <= W_TOL, (n, out[b], want)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_one_image_equals_the_definition(name):
    _check([name], *_run([name]))


def test_mixed_size_batch_equals_the_definition():
    _check(list(MIXED), *_run(list(MIXED)))


def test_values_do_not_depend_on_the_batch():
    """alone, first in a batch and last in a batch of other sizes: the same bits; and again on a second call"""
    for name in ("strip_130x2049", "speckle_37x53", "rect_300x400", "empty_5x3", "full_1x1"):
        alone = _run([name], return_hist=False).view(torch.int64)
        first = _run([name, "blob_300x400", "corner_9x1"], return_hist=False).view(torch.int64)
        last = _run(["checker_37x53", "wide_9x2600", name], return_hist=False).view(torch.int64)
        again = _run([name], return_hist=False).view(torch.int64)
        assert torch.equal(alone[0], first[0]) and torch.equal(alone[0], last[2]) and torch.equal(alone, again), name


def test_packed_buffer_with_offsets_and_argument_checks():
    """a flat prediction buffer beside a GtBatch whose planes do not lie end to end (GtBatch.from_device)"""
    names = ["rect_37x53", "speckle_5x3", "speckle_64x61"]
    offs, flat_p, flat_g, o = [], [], [], 0
    for n in names:
        o += 100  # a gap in front of every plane
        offs.append(o)
        o += BY_NAME[n][1].size
    buf_p, buf_g = np.full(o, 77, np.uint8), np.full(o, 1, np.uint8)
    for n, at in zip(names, offs):
        buf_p[at:at + BY_NAME[n][1].size] = BY_NAME[n][1].reshape(-1)
        buf_g[at:at + BY_NAME[n][2].size] = BY_NAME[n][2].reshape(-1)
    gb = ops.GtBatch.from_device(torch.from_numpy(buf_g).to(DEV), [BY_NAME[n][2].shape for n in names], offs)
    _check(names, *ops.sod_metrics(torch.from_numpy(buf_p).to(DEV), gb, return_hist=True))
    _check(names, *ops.sod_metrics([torch.from_numpy(BY_NAME[n][1]).to(DEV) for n in names], gb, return_hist=True))
    with pytest.raises(RuntimeError):
        ops.sod_metrics([torch.from_numpy(BY_NAME[names[0]][1])], [torch.from_numpy(BY_NAME[names[0]][2]).to(DEV)])  # a CPU tensor
    with pytest.raises(ValueError):
        ops.sod_metrics([torch.from_numpy(BY_NAME[names[0]][1]).to(DEV)], [torch.from_numpy(BY_NAME[names[1]][2]).to(DEV)])
    with pytest.raises(ValueError):
        ops.sod_metrics(torch.from_numpy(buf_p[:-1]).to(DEV), gb)


# ---- the 8-bit plane of the selected query ------------------------------------------------------------------------------------
from _mask_planes import _compare_planes, _masks  # noqa: E402  (shared with test_hip_selected_planes.py)


@pytest.mark.parametrize("k,mh,mw,sizes", [(4, 50, 75, [(200, 300), (187, 300), (200, 291), (1, 1)]),
                                           (8, 28, 42, [(224, 336), (199, 300), (217, 333)])])
def test_upsample_selected_u8_scale_mode(k, mh, mw, sizes):
    from selfmask_amd.bilateral_solver import MixedBatch
    B = len(sizes)
    masks, obj, rows = _masks(60 + k, B, 6, mh, mw)
    mp, ob, rw = (torch.from_numpy(a).to(DEV) for a in (masks, obj, rows))
    gb = ops.GtBatch([torch.zeros(s, dtype=torch.uint8) for s in sizes], torch.device(DEV))
    mb = MixedBatch(sizes, DEV)
    assert gb.offsets == list(mb.px_off)
    for which in ("pick", "ub"):
        u8 = ops.upsample_selected_u8(mp, rw, gb, float(k), which).cpu().numpy()
        f64 = ops.upsample_selected_native(mp, rw, mb, float(k), which).cpu().numpy()
        assert u8.dtype == np.uint8 and u8.shape == f64.shape
        _compare_planes(u8, f64, f"x{k} {which}")
    masks, obj, rows = _masks(90 + k, B, 6, mh, mw, spread=1.3)  # the clip at both ends
    mp, ob, rw = (torch.from_numpy(a).to(DEV) for a in (masks, obj, rows))
    soft = ops.predict_masks(mp, ob, ops.PackedImages(sizes, DEV), float(k), rle=False, binary=False, soft=True).result()["soft"]
    u8 = ops.upsample_selected_u8(mp, rw, gb, float(k), "pick").cpu().numpy()
    assert (u8 == 0).any() and (u8 == 255).any()
    for b, (h, w) in enumerate(sizes):
        assert np.array_equal(u8[gb.offsets[b]:gb.offsets[b] + h * w].reshape(h, w), soft[b]), b  # the predictor's bytes


def test_upsample_selected_u8_resize_mode():
    B, nq, mh, mw, size = 3, 5, 14, 14, (97, 61)
    masks, obj, rows = _masks(71, B, nq, mh, mw)
    mp, ob, rw = (torch.from_numpy(a).to(DEV) for a in (masks, obj, rows))
    gb = ops.GtBatch([torch.zeros(size, dtype=torch.uint8)] * B, torch.device(DEV))
    for which in ("pick", "ub"):
        u8 = ops.upsample_selected_u8(mp, rw, gb, 0.0, which).cpu().numpy().reshape(B, *size)
        _compare_planes(u8, ops.upsample_selected(mp, rw, size, which).cpu().numpy(), f"resize {which}")
    # sizes that differ within the batch, against the predictor's soft planes; the clip at both ends
    sizes = [(97, 61), (40, 200), (1, 9)]
    masks, obj, rows = _masks(72, B, nq, mh, mw, spread=1.3)
    mp, ob, rw = (torch.from_numpy(a).to(DEV) for a in (masks, obj, rows))
    gb = ops.GtBatch([torch.zeros(s, dtype=torch.uint8) for s in sizes], torch.device(DEV))
    soft = ops.predict_masks(mp, ob, ops.PackedImages(sizes, DEV), 0.0, rle=False, binary=False, soft=True).result()["soft"]
    u8 = ops.upsample_selected_u8(mp, rw, gb, 0.0, "pick").cpu().numpy()
    for b, (h, w) in enumerate(sizes):
        assert np.array_equal(u8[gb.offsets[b]:gb.offsets[b] + h * w].reshape(h, w), soft[b]), b


@pytest.mark.parametrize("scale", [0.0, 4.0])
def test_evaluate_masks_extra(scale):
    """rows are what they are without ``extra``; extra = the definition on the planes of upsample_selected_u8"""
    sizes = [(120, 160), (97, 131), (120, 160)]
    B, nq, mh, mw = 3, 6, 30, 40
    masks, obj, _ = _masks(81, B, nq, mh, mw, spread=1.2)
    gts = [R.make_gt("blob", h, w, seed=b) // np.uint8(255 if b % 2 else 1) for b, (h, w) in enumerate(sizes)]
    mp, ob = torch.from_numpy(masks).to(DEV), torch.from_numpy(obj).to(DEV)
    gb = ops.GtBatch([torch.from_numpy(g) for g in gts], torch.device(DEV))
    plain = ops.evaluate_masks(mp, ob, gb, scale=scale)
    rows, extra = ops.evaluate_masks(mp, ob, gb, scale=scale, extra=True)
    rows2, ious, extra2 = ops.evaluate_masks(mp, ob, gb, scale=scale, return_ious=True, extra=True)
    assert torch.equal(plain, rows) and torch.equal(plain, rows2) and torch.equal(extra, extra2) and ious.shape == (B, nq)
    assert extra.shape == (B, 2, 4) and extra.dtype == torch.float64
    extra = extra.cpu().numpy()
    for j, which in enumerate(("pick", "ub")):
        planes = ops.upsample_selected_u8(mp, rows, gb, scale, which).cpu().numpy()
        for b, (h, w) in enumerate(sizes):
            want = S.sod_metrics(planes[gb.offsets[b]:gb.offsets[b] + h * w].reshape(h, w), gts[b])
            d = np.abs(extra[b, j] - want)
            assert d[:3].max() <= E_TOL and d[3] <= W_TOL, (which, b, extra[b, j], want)


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _write_dataset(root, name, sizes, seed):
    """write_synthetic_dataset with chosen sizes"""
    from PIL import Image
    from selfmask_amd import datasets as DS
    sub, di, gi, dg, gg = DS.LAYOUTS[name]
    os.makedirs(os.path.join(root, sub, di), exist_ok=True)
    os.makedirs(os.path.join(root, sub, dg), exist_ok=True)
    rng = np.random.Generator(np.random.PCG64(seed))
    for i, (h, w) in enumerate(sizes):
        img, gt = DS.synthetic_scene(rng, h, w)
        Image.fromarray(img).save(os.path.join(root, sub, di, f"{i:05d}.jpg"), quality=92)
        Image.fromarray((gt * 255).astype(np.uint8)).save(os.path.join(root, sub, dg, f"{i:05d}.png"))


def test_evaluator_extra_metrics_end_to_end(tmp_path):
    from selfmask_amd import MaskFormer, synthetic_state_dict
    from selfmask_amd import datasets as DS
    from selfmask_amd.bilateral_solver import MixedBatch
    from selfmask_amd.distributed import KEYS
    from selfmask_amd.evaluator import Evaluator
    sizes = [(120, 160), (131, 177), (120, 160), (150, 200), (131, 177), (150, 200)]
    _write_dataset(str(tmp_path), "ecssd", sizes, seed=23)
    model = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    model.load_state_dict(synthetic_state_dict(24, "calib", patch_size=16), strict=True)
    model = model.to(DEV)
    ev = Evaluator(network=model, dir_dataset=str(tmp_path))
    ev.device = torch.device(DEV)
    plain = ev("ecssd", dir_ckpt=str(tmp_path / "plain"), batch_size=4, device=torch.device(DEV))
    rows_plain = ev.last_rows.copy()
    res = ev("ecssd", dir_ckpt=str(tmp_path / "extra"), batch_size=4, device=torch.device(DEV), extra_metrics=True)
    names = [k + sfx for sfx in ("", "_ub") for k in S.NAMES]
    assert set(plain) == {k + s for k in KEYS for s in ("", "_ub")} and set(res) == set(plain) | set(names)
    assert all(res[k] == plain[k] for k in plain) and np.array_equal(ev.last_rows, rows_plain)
    txt = "metrics_ecssd.txt"
    assert open(tmp_path / "plain" / txt, "rb").read() == open(tmp_path / "extra" / txt, "rb").read()
    assert not os.path.exists(tmp_path / "plain" / "metrics_ecssd_extra.txt")
    head, vals = open(tmp_path / "extra" / "metrics_ecssd_extra.txt").read().split("\n")
    assert head.split(",") == names and [float(v) for v in vals.split(",")] == [res[k] for k in names]
    assert ev.last_extra.shape == (6, 2, 4)

    # the definition over the maps the rows were scored on, image by image
    ds = DS.get_dataset(str(tmp_path), "ecssd")
    want = np.zeros((6, 2, 4))
    if getattr(model, "attention_path", None) == "auto":
        model.attention_path = "unfused"  # the path the evaluator pins for a native-resolution run
    for i in range(6):
        it = ds[i]
        out = model(it["x"][None].to(DEV))
        mp, ob = out["mask_pred"][:, -1], out["objectness"][:, -1].squeeze(-1)
        gt = it["m"].squeeze().to(torch.uint8)
        rows = ops.evaluate_masks(mp, ob, [gt.to(DEV)], scale=8.0)
        assert np.array_equal(rows.cpu().numpy()[0], rows_plain[i]), i
        mb = MixedBatch([tuple(gt.shape)], DEV)
        for j, which in enumerate(("pick", "ub")):
            x = ops.upsample_selected_native(mp, rows, mb, 8.0, which).cpu().numpy().reshape(gt.shape)
            want[i, j] = S.sod_metrics((np.clip(x, 0.0, 1.0) * 255.0).astype(np.uint8), gt.numpy())
    d = np.abs(ev.last_extra - want)
    print("\nper-image max |device - definition|: E", d[..., :3].max(), "wfm", d[..., 3].max())
    for j, sfx in enumerate(("", "_ub")):
        for c, k in enumerate(S.NAMES):
            assert abs(res[k + sfx] - want[:, j, c].mean()) <= 1e-10, (k + sfx, res[k + sfx], want[:, j, c].mean())

    # two virtual ranks give the single-rank values (the gather of the extra values follows the rows')
    class TwoRanks:
        def __init__(self, rank, store):
            self.rank, self.world_size, self.store = rank, 2, store

        def all_gather(self, t):
            mine = self.store.setdefault(self.rank, [])
            mine.append(t.clone())
            peer = self.store.get(1 - self.rank, [])
            if len(peer) >= len(mine):
                other = peer[len(mine) - 1]
            else:  # the rank that runs first: a stand-in for its peer's images
                own = {int(v) for v in t[:, 0].tolist() if v >= 0}
                other = torch.full_like(t, -1.0)
                missing = [i for i in range(6) if i not in own]
                other[:len(missing), 0] = torch.tensor(missing, dtype=t.dtype, device=t.device)
                other[:len(missing), 1:] = 0.0
            parts = {self.rank: t, 1 - self.rank: other}
            return torch.stack([parts[0], parts[1]])

    store = {}
    ev("ecssd", dir_ckpt=str(tmp_path / "r0"), batch_size=4, device=torch.device(DEV), extra_metrics=True, comm=TwoRanks(0, store))
    res2 = ev("ecssd", dir_ckpt=str(tmp_path / "r1"), batch_size=4, device=torch.device(DEV), extra_metrics=True, comm=TwoRanks(1, store))
    assert res2 == res


@pytest.mark.parametrize("img_size,bs", [(None, 4), (224, 3)])
def test_evaluator_extra_metrics_with_refinement(tmp_path, img_size, bs):
    """refine="bilateral" on both of its branches: four more values for the refined mask, and nothing else moves"""
    from selfmask_amd import MaskFormer, synthetic_state_dict
    from selfmask_amd.distributed import KEYS
    from selfmask_amd.evaluator import Evaluator
    sizes = [(120, 160), (131, 177), (120, 160), (150, 200), (131, 177), (150, 200)]
    _write_dataset(str(tmp_path), "ecssd", sizes, seed=29)
    model = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    model.load_state_dict(synthetic_state_dict(24, "calib", patch_size=16), strict=True)
    ev = Evaluator(network=model.to(DEV), dir_dataset=str(tmp_path))
    ev.device = torch.device(DEV)
    kw = dict(img_size=img_size, batch_size=bs, device=torch.device(DEV), refine="bilateral")
    plain = ev("ecssd", dir_ckpt=str(tmp_path / "plain"), **kw)
    refined_plain = ev.last_rows_refined.copy()
    res = ev("ecssd", dir_ckpt=str(tmp_path / "extra"), extra_metrics=True, **kw)
    names = [k + sfx for sfx in ("", "_ub", "_refined") for k in S.NAMES]
    assert len(plain) == 21 and set(res) == set(plain) | set(names) and all(res[k] == plain[k] for k in plain)
    assert np.array_equal(ev.last_rows_refined, refined_plain) and ev.last_extra.shape == (6, 3, 4)
    for txt in ("metrics_ecssd.txt", "metrics_ecssd_refined.txt"):
        assert open(tmp_path / "plain" / txt, "rb").read() == open(tmp_path / "extra" / txt, "rb").read()
    head, vals = open(tmp_path / "extra" / "metrics_ecssd_extra.txt").read().split("\n")
    assert head.split(",") == names and [float(v) for v in vals.split(",")] == [res[k] for k in names]
    ex = ev.last_extra
    assert np.isfinite(ex).all() and (ex[..., 3] >= 0).all() and (ex[..., 3] <= 1).all() and (ex[..., 1] <= ex[..., 2]).all()
    # a refined mask is binary, its 8-bit plane 0 / 255: the adaptive map is one of the 256 threshold maps, so e_adp is on the curve
    assert (ex[:, 2, 0] <= ex[:, 2, 2] + 1e-12).all() and len(KEYS) == 7
