"""The serving class and the predictor with the device PNG encoder (predict(encoder="device"), predict_png, --png_encoder device): the
files decode - by Pillow, which knows nothing of the encoder - to the pixels of the host path, which itself keeps its bytes."""
import base64
import json
import os
import threading
from argparse import Namespace
from io import BytesIO

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from selfmask_amd import MaskFormer, SelfMaskInference, png, synthetic_state_dict  # noqa: E402
from selfmask_amd.datasets import synthetic_scene  # noqa: E402
from selfmask_amd.predictor import SaliencyPredictor, main  # noqa: E402

DEV = torch.device("cuda:0")
PREFIX = "data:image/png;base64,"
CFG = dict(n_queries=20, n_decoder_layers=6, learnable_pixel_decoder=False, lateral_connection=False,
           loss_every_decoder_layer=True, scale_factor=2, abs_2d_pe_init=False, use_binary_classifier=True,
           arch="vit_small", training_method="dino", patch_size=16)
KEYS = ("original", "mask", "heatmap")


@pytest.fixture(scope="module")
def inference():
    m = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    m.load_state_dict(synthetic_state_dict(2, "soft", patch_size=16), strict=True)
    return SelfMaskInference(None, Namespace(**CFG), device=DEV, model=m)


def _uploads():
    rng = np.random.Generator(np.random.PCG64(78))
    return [rng.integers(0, 256, size=(37, 53, 3), dtype=np.uint8), synthetic_scene(rng, 300, 400)[0]]


def _file(url: str) -> bytes:
    assert url.startswith(PREFIX)
    return base64.b64decode(url[len(PREFIX):])


def _pixels(data: bytes) -> np.ndarray:
    img = Image.open(BytesIO(data))
    img.load()
    return np.asarray(img)


def _url(img):
    buf = BytesIO()
    img.save(buf, format="PNG")
    return PREFIX + base64.b64encode(buf.getvalue()).decode()


def test_device_urls_decode_to_the_host_paths_pixels(inference):
    for rgb in _uploads():
        host = inference.predict(rgb)
        dev = inference.predict(rgb, encoder="device")
        assert list(dev) == list(host)
        for k, mode in zip(KEYS, ("RGB", "L", "RGBA")):
            got = Image.open(BytesIO(_file(dev[k])))
            assert got.mode == mode
            assert np.array_equal(np.asarray(got), _pixels(_file(host[k]))), k
        assert np.array_equal(_pixels(_file(dev["original"])), rgb)
        assert dev["best_idx"] == host["best_idx"] and np.array_equal(dev["objectness_scores"], host["objectness_scores"])
        # the files are the restatement's, byte for byte
        imgs = inference.predict_images(rgb)
        assert _file(dev["mask"]) == png.encode_reference(imgs["mask"]) and _file(dev["heatmap"]) == png.encode_reference(imgs["heatmap"])
        assert _file(dev["original"]) == png.encode_reference(rgb)


def test_the_default_is_still_the_host_chain_byte_for_byte(inference):
    for rgb in _uploads():
        imgs = inference.predict_images(rgb)
        r = inference.predict(rgb)
        assert all(r[k] == inference.predict(rgb, encoder="host")[k] for k in KEYS)
        assert r["original"] == _url(Image.fromarray(rgb)) and r["mask"] == _url(Image.fromarray(imgs["mask"]))
        assert r["heatmap"] == _url(Image.fromarray(imgs["heatmap"]))
    with pytest.raises(ValueError):
        inference.predict(_uploads()[0], encoder="gpu")


def test_predict_png_matches_the_decoded_urls(inference):
    for rgb in _uploads():
        t = inference.predict_png(rgb)
        dev = inference.predict(rgb, encoder="device")
        imgs = inference.predict_images(rgb)
        for k in KEYS:
            assert isinstance(t[k], bytes) and t[k] == _file(dev[k])
        assert np.array_equal(_pixels(t["mask"]), imgs["mask"]) and np.array_equal(_pixels(t["heatmap"]), imgs["heatmap"])
        assert t["best_idx"] == imgs["best_idx"] and np.array_equal(t["objectness_scores"], imgs["objectness_scores"])


def test_concurrent_device_requests_get_their_own_images(inference):
    rng = np.random.Generator(np.random.PCG64(14))
    imgs = [rng.integers(0, 256, size=(40 + 9 * t, 90 - 7 * t, 3), dtype=np.uint8) for t in range(2)]
    want = [inference.predict(im, encoder="device") for im in imgs]
    errors = []

    def worker(t):
        try:
            for _ in range(4):
                got = inference.predict(imgs[t], encoder="device")
                if any(got[k] != want[t][k] for k in KEYS) or got["best_idx"] != want[t]["best_idx"]:
                    errors.append(t)
                if not np.array_equal(_pixels(_file(got["original"])), imgs[t]):
                    errors.append((t, "original"))
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_predictor_png_encoder_device(tmp_path):
    import yaml
    rng = np.random.Generator(np.random.PCG64(22))
    root = tmp_path / "images"
    root.mkdir()
    names = []
    for i, (h, w) in enumerate([(96, 130), (80, 81), (100, 128), (33, 47)]):
        Image.fromarray(synthetic_scene(rng, h, w)[0]).save(root / f"img{i}.png")
        names.append(f"img{i}.png")
    sd = synthetic_state_dict(4, "calib", patch_size=16)
    model = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    files = [str(root / n) for n in names]
    soft = SaliencyPredictor(model, device=DEV, batch_size=4, workers=2)(files, output="soft")
    pred = SaliencyPredictor(model, device=DEV, batch_size=4, workers=2, png_encoder="device")
    encoded = pred(files, output="soft_png")
    assert list(encoded) == names
    for n in names:
        assert isinstance(encoded[n], bytes) and encoded[n] == png.encode_reference(soft[n])
        assert np.array_equal(_pixels(encoded[n]), soft[n])
    with pytest.raises(ValueError):
        SaliencyPredictor(model, device=DEV, png_encoder="gpu")
    # the command line: the same files on disk, the host path's pixels
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump(CFG, f)
    torch.save(sd, tmp_path / "weights.pt")
    common = ["--config", str(tmp_path / "config.yaml"), "--p_state_dict", str(tmp_path / "weights.pt"), "--images", str(root),
              "--batch_size", "4"]
    main(common + ["--out", str(tmp_path / "dev.json"), "--png_dir", str(tmp_path / "dev"), "--png_encoder", "device"])
    main(common + ["--out", str(tmp_path / "host.json"), "--png_dir", str(tmp_path / "host")])
    assert json.load(open(tmp_path / "dev.json")) == json.load(open(tmp_path / "host.json"))
    for n in names:
        stem = os.path.splitext(n)[0] + ".png"
        data = open(tmp_path / "dev" / stem, "rb").read()
        assert data == encoded[n]
        assert np.array_equal(_pixels(data), np.asarray(Image.open(tmp_path / "host" / stem))) and Image.open(BytesIO(data)).mode == "L"
