"""The bilateral solver on batches whose images differ in size (sm_bilateral_solver_mixed_f64), the native-resolution target
(sm_upsample_selected_native_f64) and the evaluator's ``refine="bilateral"`` at ``img_size=None``.  The contract throughout:
every image of a mixed batch gives the bits of its own single solve, whatever its neighbours and their order."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import bilateral_oracle as BO  # noqa: E402  (checkers only)
from oracle import evaluator_oracle as E  # noqa: E402
from oracle import selfmask_oracle as O  # noqa: E402
from selfmask_amd import MaskFormer, ops, synthetic_state_dict  # noqa: E402
from selfmask_amd import datasets as DS, distributed as D  # noqa: E402
from selfmask_amd.bilateral_solver import (MixedBatch, bilateral_solver_batch_device, bilateral_solver_mixed_device,  # noqa: E402
                                           bilateral_solver_output_device)
from selfmask_amd.evaluator import Evaluator  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden", "bilateral.npz")
DEV = torch.device("cuda:0")
SIZES = [(97, 131), (224, 224), (300, 400), (120, 152), (17, 301), (301, 17), (64, 64), (250, 333), (384, 384), (64, 64), (64, 64)]


def _scenes(seed=5):
    """One scene per entry of SIZES: synthetic_scene images with noisy-blob targets; the last three are the degenerate cases
    of test_hip_bilateral.test_degenerate_targets (an exactly-grey image with an all-zero and an all-one target) and a grey
    image with a blob."""
    rng = np.random.Generator(np.random.PCG64(seed))
    imgs, tgts = [], []
    for k, (h, w) in enumerate(SIZES):
        img, gt = DS.synthetic_scene(rng, h, w)
        tgt = np.clip(0.15 + 0.7 * gt + rng.standard_normal((h, w)) * 0.1, 0, 1)
        if k >= len(SIZES) - 3:
            img = np.full((h, w, 3), 90, np.uint8)
        if k == len(SIZES) - 3:
            tgt = np.zeros((h, w))
        if k == len(SIZES) - 2:
            tgt = np.ones((h, w))
        imgs.append(img)
        tgts.append(tgt)
    return imgs, tgts


def _dev(imgs, tgts):
    return [torch.from_numpy(i).to(DEV) for i in imgs], [torch.from_numpy(t).to(DEV) for t in tgts]


_SINGLE = {}


def _single(k, I, T):
    """The single solve of scene k (cached: several tests compare against it)."""
    if k not in _SINGLE:
        _SINGLE[k] = bilateral_solver_output_device(I, T, return_info=True)
    return _SINGLE[k]


def test_every_image_of_a_mixed_batch_equals_its_single_solve():
    imgs, tgts = _scenes()
    I, T = _dev(imgs, tgts)
    soft, binary, info = bilateral_solver_mixed_device(I, T, return_info=True)
    assert len(soft) == len(binary) == len(SIZES) and info.shape == (len(SIZES), 4)
    for k in range(len(SIZES)):
        s1, b1, i1 = _single(k, I[k], T[k])
        assert soft[k].shape == s1.shape and binary[k].dtype == torch.uint8
        assert torch.equal(soft[k], s1), (k, SIZES[k], float((soft[k] - s1).abs().max()))
        assert torch.equal(binary[k], b1), (k, SIZES[k])
        assert torch.equal(info[k], i1), (k, SIZES[k], info[k], i1)
    # a second call reproduces the first
    soft2, binary2, info2 = bilateral_solver_mixed_device(I, T, return_info=True)
    assert all(torch.equal(a, b) for a, b in zip(soft, soft2)) and all(torch.equal(a, b) for a, b in zip(binary, binary2))
    assert torch.equal(info, info2)


@pytest.mark.parametrize("ks", [(0, 2, 4, 7, 9, 10)])
def test_mixed_batch_matches_the_oracle(ks):
    imgs, tgts = _scenes()
    I, T = _dev(imgs, tgts)
    soft, binary, info = bilateral_solver_mixed_device(I, T, return_info=True)
    for k in ks:
        rs, rb, grid = BO.bilateral_solver_output(imgs[k], tgts[k])
        d = np.abs(soft[k].cpu().numpy() - rs).max()
        print(f"\n{SIZES[k]}: V={int(info[k, 0])} cg_iters={int(info[k, 1])} max|soft-oracle|={d:.2e}")
        assert d <= 1e-9
        assert np.array_equal(binary[k].cpu().numpy().astype(bool), rb)
        assert int(info[k, 0]) == grid.nvertices


def test_order_and_company_do_not_matter():
    imgs, tgts = _scenes()
    I, T = _dev(imgs, tgts)
    n = len(SIZES)
    soft, binary, info = bilateral_solver_mixed_device(I[::-1], T[::-1], return_info=True)
    for k in range(n):
        s1, b1, i1 = _single(k, I[k], T[k])
        assert torch.equal(soft[n - 1 - k], s1) and torch.equal(binary[n - 1 - k], b1) and torch.equal(info[n - 1 - k], i1), k
    # scene 7 (250 x 333) in the middle of 32 neighbours of other sizes, larger and smaller
    rng = np.random.Generator(np.random.PCG64(99))
    oi, ot = [], []
    for j in range(32):
        h, w = int(rng.integers(20, 400)), int(rng.integers(20, 400))
        img, gt = DS.synthetic_scene(rng, h, w)
        oi.append(img)
        ot.append(np.clip(0.15 + 0.7 * gt + rng.standard_normal((h, w)) * 0.1, 0, 1))
    OI, OT = _dev(oi, ot)
    soft, binary, info = bilateral_solver_mixed_device(OI[:13] + [I[7]] + OI[13:], OT[:13] + [T[7]] + OT[13:], return_info=True)
    s1, b1, i1 = _single(7, I[7], T[7])
    assert torch.equal(soft[13], s1) and torch.equal(binary[13], b1) and torch.equal(info[13], i1)
    for j in (0, 12, 14, 32):  # and the neighbours are their own single solves too
        src = j if j < 13 else j - 1
        s1, b1, i1 = bilateral_solver_output_device(OI[src], OT[src], return_info=True)
        assert torch.equal(soft[j], s1) and torch.equal(binary[j], b1) and torch.equal(info[j], i1), j


def test_uniform_sizes_through_the_mixed_entry_point():
    h, w, n = 120, 152, 8
    rng = np.random.Generator(np.random.PCG64(11))
    scenes = [DS.synthetic_scene(rng, h, w) for _ in range(n)]
    imgs = np.stack([im for im, _ in scenes])
    tgts = np.stack([np.clip(0.15 + 0.7 * g + rng.standard_normal((h, w)) * 0.1, 0, 1) for _, g in scenes])
    I, T = torch.from_numpy(imgs).to(DEV), torch.from_numpy(tgts).to(DEV)
    sb, bb, ib = bilateral_solver_batch_device(I, T, return_info=True)
    sm, bm, im = bilateral_solver_mixed_device(list(I), list(T), return_info=True)
    assert torch.equal(torch.stack(sm), sb) and torch.equal(torch.stack(bm), bb) and torch.equal(im, ib)
    # the packed form of the same call
    sp, bp = bilateral_solver_mixed_device(I.reshape(-1), T.reshape(-1), shapes=[(h, w)] * n)
    assert torch.equal(torch.stack(sp), sb) and torch.equal(torch.stack(bp), bb)


def test_golden_cases_as_one_mixed_batch():
    """The three outputs of the real reference (64^2, 224^2, 256 x 384) in ONE batch: the gate of
    test_hip_bilateral.test_matches_reference_outputs."""
    g = np.load(GOLD)
    n = int(g["n_cases"])
    I, T = _dev([g[f"img_{i}"] for i in range(n)], [g[f"target_{i}"] for i in range(n)])
    assert len({tuple(t.shape) for t in T}) == n
    soft, binary, info = bilateral_solver_mixed_device(I, T, return_info=True)
    for i in range(n):
        assert int(info[i, 0]) == int(g[f"nvert_{i}"])
        d = np.abs(soft[i].cpu().numpy() - g[f"soft_{i}"]).max()
        print(f"\ncase {i}: V={int(info[i, 0])} cg_iters={int(info[i, 1])} max|soft-ref|={d:.2e}")
        assert d <= 1e-9
        assert np.array_equal(binary[i].cpu().numpy().astype(bool), g[f"binary_{i}"])


@pytest.mark.parametrize("k,mh,mw,sizes", [(4, 30, 41, [(120, 164), (117, 161), (97, 131)]),
                                           (8, 28, 42, [(224, 336), (199, 300), (217, 333)])])
@pytest.mark.parametrize("which", ["pick", "ub"])
def test_upsample_selected_native(k, mh, mw, sizes, which):
    rng = np.random.Generator(np.random.PCG64(40 + k))
    nq, B = 6, len(sizes)
    masks = rng.random((B, nq, mh, mw)).astype(np.float32)
    rows = np.zeros((B, 16), np.float32)
    rows[:, 14], rows[:, 15] = rng.integers(0, nq, B), rng.integers(0, nq, B)
    mp, rw = torch.from_numpy(masks).to(DEV), torch.from_numpy(rows).to(DEV)
    mb = MixedBatch(sizes, DEV)
    out = mb.views(ops.upsample_selected_native(mp, rw, mb, float(k), which))
    full = ops.upsample_selected(mp, rw, (k * mh, k * mw), which)  # size mode at the whole grid: the same source ratio 1 / k
    assert sizes[0] == (k * mh, k * mw)
    for b, (h, w) in enumerate(sizes):
        assert out[b].dtype == torch.float64 and out[b].shape == (h, w)
        assert torch.equal(out[b], full[b, :h, :w]), (b, float((out[b] - full[b, :h, :w]).abs().max()))  # a crop moves no source index
        q = int(rows[b, 14 if which == "pick" else 15])
        ref = F.interpolate(torch.from_numpy(masks[b, q])[None, None], scale_factor=k, mode="bilinear", align_corners=False)[0, 0, :h, :w]
        got = out[b].cpu().numpy()
        d = np.abs(got - ref.double().numpy()).max()
        print(f"\nx{k} {which} image {b} {h}x{w}: max|native - F.interpolate| = {d:.2e}")
        assert np.allclose(got, ref.double().numpy(), rtol=1e-6, atol=1e-7)


# ---- the evaluator at native resolution ------------------------------------------------------------------------------------
def _model(patch, seed, style="calib"):
    m = MaskFormer(n_queries=20, patch_size=patch, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    sd = synthetic_state_dict(seed, style, patch_size=patch)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV), sd


class FakeComm:
    """Two ranks evaluated in turn in one process (the pattern of test_hip_evaluator.py).  A refined run gathers twice - the plain
    rows, then the refined ones - so the rank that runs first cannot park at its first gather: it records what it contributes and
    is handed a stand-in for its peer (the missing image indices with zero rows) to run to its end; the rank that runs second
    receives the first rank's real contributions, and its gathered rows are the ones compared."""

    def __init__(self, rank, world, store, n_total):
        self.rank, self.world_size, self.store, self.n_total = rank, world, store, n_total

    def all_gather(self, t):
        mine = self.store.setdefault(self.rank, [])
        mine.append(t.clone())
        k, peer = len(mine) - 1, self.store.get(1 - self.rank, [])
        if len(peer) > k:
            parts = {self.rank: t, 1 - self.rank: peer[k]}
            return torch.stack([parts[r] for r in range(self.world_size)])
        own = {int(v) for v in t[:, 0].tolist() if v >= 0}
        missing = [i for i in range(self.n_total) if i not in own]
        stand_in = torch.full_like(t, -1.0)
        stand_in[:len(missing), 0] = torch.tensor(missing, dtype=t.dtype, device=t.device)
        stand_in[:len(missing), 1:] = 0.0
        parts = {self.rank: t, 1 - self.rank: stand_in}
        return torch.stack([parts[r] for r in range(self.world_size)])


def test_evaluator_native_refinement_end_to_end(tmp_path):
    """ViT-S/16 at native resolution: refine="bilateral" with img_size=None, batch 1 and token-grid buckets, against the oracle
    chained the same way.  Per-image refined metrics within 2e-3 (a 1e-5 logit difference moves a handful of pixels across 0.5:
    the gate and the reason of test_configs2_384_bilateral_refinement_end_to_end); the picked query must match exactly."""
    from PIL import Image
    n_img = 16
    DS.write_synthetic_dataset(str(tmp_path), "ecssd", n_img, seed=17, size_range=(120, 200))
    model, sd = _model(16, 24)
    ev = Evaluator(network=model, dir_dataset=str(tmp_path))
    ev.device = DEV
    ev("ecssd", dir_ckpt=str(tmp_path / "plain"), batch_size=8, device=DEV)
    rows_plain = ev.last_rows.copy()
    res = ev("ecssd", dir_ckpt=str(tmp_path / "ckpt8"), batch_size=8, device=DEV, refine="bilateral")
    assert set(res) == {k + s for k in D.KEYS for s in ("", "_ub", "_refined")} and len(res) == 21
    assert os.path.exists(tmp_path / "ckpt8" / "metrics_ecssd_refined.txt")
    assert np.array_equal(ev.last_rows, rows_plain)
    refined8 = ev.last_rows_refined.copy()
    res1 = ev("ecssd", dir_ckpt=str(tmp_path / "ckpt1"), batch_size=1, device=DEV, refine="bilateral")
    assert np.array_equal(ev.last_rows, rows_plain)
    assert np.array_equal(ev.last_rows_refined, refined8)
    assert res1 == res

    # two virtual ranks give the single-rank rows
    store = {}
    ev("ecssd", dir_ckpt=str(tmp_path / "c0"), batch_size=8, device=DEV, refine="bilateral", comm=FakeComm(0, 2, store, n_img))
    res2 = ev("ecssd", dir_ckpt=str(tmp_path / "c1"), batch_size=8, device=DEV, refine="bilateral", comm=FakeComm(1, 2, store, n_img))
    assert len(store[0]) == len(store[1]) == 2
    assert np.array_equal(ev.last_rows, rows_plain)
    assert np.array_equal(ev.last_rows_refined, refined8)
    assert res2 == res

    # the oracle chained the same way
    ds = DS.get_dataset(str(tmp_path), "ecssd")
    ref = []
    for i in range(n_img):
        it = ds[i]
        out = O.forward(it["x"][None], sd, 16)
        gt = it["m"].to(torch.int64)
        pm, q, ub, _ = E.postprocess(out["mask_pred"][0, -1], out["objectness"][0, -1, :, 0], gt, scale_factor=8)
        assert q == int(rows_plain[i, 14]), (i, q, rows_plain[i, 14])
        rgb = np.asarray(Image.open(ds.p_imgs[i]).convert("RGB"))
        assert tuple(pm[q].shape) == rgb.shape[:2] == tuple(gt.shape)
        binary = BO.bilateral_solver_output(rgb, pm[q].double().numpy())[1]
        ref.append(E.all_metrics(torch.from_numpy(binary.astype(np.float32)), gt))
    ref, got = np.array(ref), refined8[:, :7]
    print("\nnative refined metrics, max |hip - oracle| per image:\n", np.round(np.abs(got - ref).max(1), 6))
    assert np.abs(got - ref).max() <= 2e-3
