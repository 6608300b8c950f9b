"""SaliencyPredictor end to end on the device: files in, masks out.  The forward is the model's own (fetched from the device); only
the finish is re-derived, on the host (tests/_predict_ref.py).  Seven JPEG / PNG files of seven sizes spanning three token grids at
P = 16, synthetic weights of kind WEIGHTS."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _predict_ref as R  # noqa: E402
from selfmask_amd import MaskFormer, ops, synthetic_state_dict  # noqa: E402
from selfmask_amd.datasets import synthetic_scene  # noqa: E402
from selfmask_amd.mask_generator import rle_decode, rle_encode  # noqa: E402
from selfmask_amd.pipeline import decode_item, preprocess_on_device  # noqa: E402
from selfmask_amd.predictor import SaliencyPredictor, main  # noqa: E402

DEV = "cuda:0"
PATCH, SCALE = 16, 8.0
# the weight kind whose CPU-oracle forward (oracle.selfmask_oracle.forward on these seven files) gives at least five non-empty
# masks - the condition of test_agreement_with_the_evaluator.  Checked on the host when the test was written: "calib" 7 of 7 non-empty
# (36-70 % of the pixels set), "soft" 7 of 7 (24-37 %), "peaky" 7 of 7 but nearly full (98-100 %); "calib" has the most varied shapes
WEIGHTS = "calib"
SIZES = [(250, 333), (180, 200), (241, 330), (150, 230), (256, 336), (190, 205), (160, 240)]  # grids 16x21, 12x13, 10x15
CONFIG = dict(n_queries=20, n_decoder_layers=6, learnable_pixel_decoder=False, lateral_connection=False, loss_every_decoder_layer=True,
              scale_factor=2, abs_2d_pe_init=False, use_binary_classifier=True, arch="vit_small", training_method="dino", patch_size=PATCH)


def write_files(root):
    from PIL import Image
    rng = np.random.Generator(np.random.PCG64(21))
    files = []
    for i, (h, w) in enumerate(SIZES):
        rgb, _ = synthetic_scene(rng, h, w)
        p = os.path.join(str(root), f"img{i}.{'png' if i % 3 == 0 else 'jpg'}")
        Image.fromarray(rgb).save(p, **({} if p.endswith("png") else {"quality": 92}))
        files.append(p)
    return files


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """files, model, and per file the model's own last-layer masks / objectness at native resolution (batch 1, the attention path the
    predictor pins for a native run), computed once and left unchanged"""
    root = tmp_path_factory.mktemp("predict")
    files = write_files(root)
    sd = synthetic_state_dict(4, WEIGHTS, patch_size=PATCH)
    model = MaskFormer(n_queries=20, patch_size=PATCH, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    fwd = {}
    model.attention_path = "unfused"
    try:
        for p in files:
            rgb, _ = decode_item(p, None)
            h, w = rgb.shape[:2]
            x = preprocess_on_device([rgb], None, DEV, pad_to=(-(-h // PATCH) * PATCH, -(-w // PATCH) * PATCH))
            out = model(x)
            fwd[os.path.basename(p)] = (rgb, out["mask_pred"][0, -1].clone(), out["objectness"][0, -1, :, 0].clone())
    finally:
        model.attention_path = "auto"
    torch.cuda.synchronize()
    ref = {n: R.finish_one(m.cpu(), o.cpu().numpy(), rgb.shape[:2], SCALE) for n, (rgb, m, o) in fwd.items()}
    return {"root": root, "files": files, "sd": sd, "model": model, "fwd": fwd, "ref": ref, "names": [os.path.basename(p) for p in files]}


def test_batch_and_stream_invariance(world):
    a = SaliencyPredictor(world["model"], device=DEV, batch_size=4, streams=3, workers=2)
    ra = a(world["files"])
    b = SaliencyPredictor(world["model"], device=DEV, batch_size=1, streams=1, workers=2, hip_graph=False)
    rb = b(world["files"])
    assert list(ra) == world["names"] and ra == rb and a.last_best == b.last_best
    for n in world["names"]:
        assert ra[n] == world["ref"][n]["rle"], n
        assert a.last_best[n] == world["ref"][n]["best"], n


def test_agreement_with_the_evaluator(world):
    """the predicted binary mask handed to evaluate_masks as ground truth: the same query is picked and its IoU is exactly 1"""
    p = SaliencyPredictor(world["model"], device=DEV, batch_size=4, workers=2)
    binary = p(world["files"], output="binary")
    nonempty = 0
    for n in world["names"]:
        _, m, o = world["fwd"][n]
        assert np.array_equal(binary[n], world["ref"][n]["binary"]), n
        rows = ops.evaluate_masks(m[None], o[None], [torch.from_numpy(binary[n])], scale=SCALE).cpu().numpy()
        assert int(rows[0, 14]) == p.last_best[n], n
        if binary[n].any():
            nonempty += 1
            assert rows[0, 0] == 1.0, (n, rows[0, 0])
    assert nonempty >= 5, f"only {nonempty} of 7 masks are non-empty with the {WEIGHTS!r} weights"


def test_bilateral_refinement_native(world):
    from selfmask_amd.bilateral_solver import bilateral_solver_mixed_device
    p = SaliencyPredictor(world["model"], device=DEV, batch_size=4, workers=2)
    got = p(world["files"], refine="bilateral")
    imgs = [torch.from_numpy(world["fwd"][n][0]).to(DEV) for n in world["names"]]
    targets = [torch.from_numpy(world["ref"][n]["value"]).double().to(DEV) for n in world["names"]]
    _, binary = bilateral_solver_mixed_device(imgs, targets)
    for n, b in zip(world["names"], binary):
        assert got[n] == rle_encode(b.cpu().numpy()), n
    gb = p(world["files"], output="binary", refine="bilateral")
    for n, b in zip(world["names"], binary):
        assert np.array_equal(gb[n], b.cpu().numpy()), n


def test_bilateral_refinement_resized(world):
    """img_size = 224: the S x S solve of ``bilateral_solver_batch_device`` on the resized images; its binary mask then takes the way of
    every mask of the resized mode - bilinear to the file's own size, > 0.5 (what the evaluator scores as ``*_refined``)"""
    from selfmask_amd.bilateral_solver import bilateral_solver_batch_device
    S = 224
    p = SaliencyPredictor(world["model"], device=DEV, batch_size=4, workers=2)
    got = p(world["files"], img_size=S, refine="bilateral")
    model = world["model"]
    rgbs = [world["fwd"][n][0] for n in world["names"]]
    model.attention_path = "unfused"  # what the predictor pins for batches under 16
    try:
        x, u8 = preprocess_on_device(rgbs, S, DEV, return_u8=True)
        out = model(x)
    finally:
        model.attention_path = "auto"
    masks, obj = out["mask_pred"][:, -1].cpu(), out["objectness"][:, -1, :, 0].cpu()
    targets = torch.stack([R.upsampled(masks[b, R.first_argmax(obj[b].numpy())], (S, S), 0.0) for b in range(len(rgbs))]).double()
    _, binary = bilateral_solver_batch_device(u8, targets.to(DEV))
    for b, n in enumerate(world["names"]):
        v = R.upsampled(binary[b].float().cpu(), rgbs[b].shape[:2], 0.0).numpy()
        assert got[n] == rle_encode((v > np.float32(0.5)).astype(np.uint8)), n


def test_soft_output_and_png(world, tmp_path):
    from PIL import Image
    import yaml
    p = SaliencyPredictor(world["model"], device=DEV, batch_size=4, workers=2)
    soft = p(world["files"], output="soft")
    for n in world["names"]:
        assert soft[n].dtype == np.uint8 and np.array_equal(soft[n], world["ref"][n]["soft"]), n
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump(CONFIG, f)
    torch.save(world["sd"], tmp_path / "weights.pt")
    main(["--config", str(tmp_path / "config.yaml"), "--p_state_dict", str(tmp_path / "weights.pt"), "--images", str(world["root"]),
          "--out", str(tmp_path / "masks.json"), "--batch_size", "4", "--png_dir", str(tmp_path / "png")])
    codes = json.load(open(tmp_path / "masks.json"))
    assert sorted(codes) == sorted(world["names"])
    for n in world["names"]:
        assert codes[n] == world["ref"][n]["rle"], n
        assert np.array_equal(rle_decode(codes[n]), world["ref"][n]["binary"]), n
        png = np.asarray(Image.open(tmp_path / "png" / (os.path.splitext(n)[0] + ".png")))
        assert png.dtype == np.uint8 and np.array_equal(png, world["ref"][n]["soft"]), n


def test_replayed_graphs_and_retry_read_that_batchs_outputs(world):
    """resized mode at batch 1 on one and on three streams: seven equal batches, so from the third sighting per stream the forward is
    a replayed graph whose static outputs the finish reads - also when the runs are found a second time (cap = 4 overflows on every
    non-trivial mask) streams batches later.  Same results as eager launches."""
    S = 224
    eager = SaliencyPredictor(world["model"], device=DEV, batch_size=1, streams=1, workers=2, hip_graph=False)
    want = eager(world["files"], img_size=S)
    assert eager.graph_stats["replays"] == 0
    for streams, cap, min_replays in ((1, 8192, 4), (1, 4, 4), (3, 4, 1)):
        p = SaliencyPredictor(world["model"], device=DEV, batch_size=1, streams=streams, workers=2, cap=cap)
        got = p(world["files"] * 1, img_size=S)
        assert p.graph_stats["failed"] is None and p.graph_stats["replays"] >= min_replays, p.graph_stats
        assert got == want and p.last_best == eager.last_best, (streams, cap)
    assert max(len(r["counts"]) for r in want.values()) > 5  # cap = 4 did overflow
