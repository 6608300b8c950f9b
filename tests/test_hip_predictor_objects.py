"""``SaliencyPredictor(...)(files, output="objects")`` end to end on the device: the objects of every file's mask equal the host
restatement (tests/_objects_ref.py) applied to the binary (and soft) planes the same run returns, in native and resized mode and
behind the bilateral solver; the run-length codes do not change when objects are computed beside them.  Synthetic weights as
tests/test_hip_predictor.py."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _objects_ref as R  # noqa: E402
from selfmask_amd import MaskFormer, synthetic_state_dict  # noqa: E402
from selfmask_amd.datasets import synthetic_scene  # noqa: E402
from selfmask_amd.predictor import SaliencyPredictor, main  # noqa: E402

DEV = "cuda:0"
PATCH = 16
SIZES = [(150, 230), (180, 200), (160, 240), (190, 205), (155, 236)]  # token grids 10 x 15 and 12 x 13
OPTS = dict(connectivity=8, min_area=4, max_objects=8)
CONFIG = dict(n_queries=20, n_decoder_layers=6, learnable_pixel_decoder=False, lateral_connection=False, loss_every_decoder_layer=True,
              scale_factor=2, abs_2d_pe_init=False, use_binary_classifier=True, arch="vit_small", training_method="dino", patch_size=PATCH)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("objects")
    rng = np.random.Generator(np.random.PCG64(23))
    files = []
    for i, (h, w) in enumerate(SIZES):
        rgb, _ = synthetic_scene(rng, h, w)
        files.append(os.path.join(str(root), f"img{i}.png"))
        Image.fromarray(rgb).save(files[-1])
    sd = synthetic_state_dict(4, "calib", patch_size=PATCH)
    model = MaskFormer(n_queries=20, patch_size=PATCH, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    model.load_state_dict(sd, strict=True)
    return {"root": root, "files": files, "names": [os.path.basename(p) for p in files], "model": model.to(DEV).eval(), "sd": sd}


def _reference(res, names, best, scored):
    return {n: {**R.objects(res["binary"][n], res["soft"][n] if scored else None, **OPTS), "best": best[n]} for n in names}


@pytest.mark.parametrize("img_size", [None, 224])
def test_objects_equal_the_reference_on_the_runs_own_planes(world, img_size):
    p = SaliencyPredictor(world["model"], device=DEV, batch_size=4, workers=2)
    res = p._run(world["files"], img_size, 2, ("rle", "binary", "soft", "objects"), None, objects=OPTS)
    want = _reference(res, world["names"], p.last_best, True)
    assert res["objects"] == want
    assert sum(len(o["objects"]) for o in want.values()) >= len(world["names"]) - 2  # masks with something in them
    # the public call gives the same, and the codes are those of a run without objects
    assert p(world["files"], img_size=img_size, output="objects", objects=OPTS) == want
    assert p(world["files"], img_size=img_size) == res["rle"]
    assert json.loads(json.dumps(want))  # plain data all the way down


def test_objects_of_the_refined_mask(world):
    p = SaliencyPredictor(world["model"], device=DEV, batch_size=4, workers=2)
    res = p._run(world["files"], None, 2, ("rle", "binary", "objects"), "bilateral", objects=OPTS)
    assert res["objects"] == _reference(res, world["names"], p.last_best, False)
    assert p(world["files"], refine="bilateral") == res["rle"]


def test_cli_writes_the_objects_beside_the_codes(world, tmp_path):
    import yaml
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump(CONFIG, f)
    torch.save(world["sd"], tmp_path / "weights.pt")
    res = main(["--config", str(tmp_path / "config.yaml"), "--p_state_dict", str(tmp_path / "weights.pt"), "--images", str(world["root"]),
                "--out", str(tmp_path / "masks.json"), "--batch_size", "4", "--objects_out", str(tmp_path / "objects.json"),
                "--min_area", "4", "--max_objects", "8"])
    assert json.load(open(tmp_path / "masks.json")) == res["rle"]
    want = json.loads(json.dumps(res["objects"]))
    assert json.load(open(tmp_path / "objects.json")) == want and sorted(want) == sorted(world["names"])
    assert all(len(v["objects"]) <= 8 and all(o["area"] >= 4 for o in v["objects"]) for v in want.values())


def test_a_file_wider_than_the_limit_is_refused_at_planning(world, tmp_path):
    from PIL import Image
    wide = str(tmp_path / "wide.png")
    Image.fromarray(np.zeros((1, 16385), np.uint8)).save(wide)
    p = SaliencyPredictor(world["model"], device=DEV, batch_size=4, workers=2)
    with pytest.raises(ValueError, match="wide.png.*16384.*nothing was run"):
        p(world["files"] + [wide], output="objects")
    assert p._ring is None and p.last_best == {}  # nothing was queued
