#!/usr/bin/env python3
"""Generate tests/golden/resnet50_<case>.npz and tests/golden/resnet50_keys.json: the four feature maps of the REAL reference
backbone on the CPU.

Usage (from the repository root, on the build machine that has the reference checkout):
    python scripts/gen_resnet_golden.py

The reference is imported as it is (``networks.resnet_backbone.ResNetBackbone``: "resnet50_dilated8", or "resnet50" for the
non-dilated case; ``ResNet50.__init__`` itself cannot be used - its weight types import torchvision or read hard-coded paths);
this script holds none of its text.  Weights and inputs are the synthetic ones of tests/_resnet_cases.py, re-generated from their
seeds by the tests.  Stored per case, evaluated in fp32 and fp64:
  map4_f64              (B, 2048, h, w)   layer 4 whole
  map1_f64 ... map3_f64 (B, C / 8, h, w)  layers 1-3 on every 8th channel
  shapes                (4, 4)            the full shapes of the four maps
  e32                   (4,)              max |ref32 - ref64| per map over what is stored
The key list holds names, shapes and dtypes of the 318 state_dict entries under ``network.`` (what ``ResNet50`` adds).
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from oracle import gen_golden as G  # noqa: E402
import _resnet_cases as RC  # noqa: E402


def build(dilated: bool, sd, dtype):
    from networks.resnet_backbone import ResNetBackbone
    net = ResNetBackbone(backbone="resnet50_dilated8" if dilated else "resnet50", pretrained=None, width_multiplier=1.0)
    net.load_state_dict({k[len("network."):]: v for k, v in sd.items()}, strict=True)
    return net.to(dtype).eval()


@torch.no_grad()
def main():
    sys.path.insert(0, G.REF)
    torch.set_num_threads(G.N_THREADS)
    keys = None
    for name, (dilated, shape, wseed, xseed) in RC.CASES.items():
        sd = RC.synthetic_resnet_state_dict(wseed, dilated)
        x = RC.synthetic_input(xseed, shape)
        net32 = build(dilated, sd, torch.float32)
        if keys is None:
            keys = [["network." + k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in net32.state_dict().items()]
            assert len(keys) == 318 and [k[0] for k in keys] == list(sd.keys())
        m32 = [m.double() for m in net32(x)]
        m64 = build(dilated, sd, torch.float64)(x.double())
        save = dict(meta=np.array([int(dilated), *shape, wseed, xseed, G.N_THREADS]), shapes=np.array([list(m.shape) for m in m64]))
        e32 = []
        for i, (a, b) in enumerate(zip(m32, m64)):
            sl = slice(None) if i == 3 else slice(None, None, RC.STORE_EVERY)
            a, b = a[:, sl], b[:, sl]
            e = (a - b).abs().max().item()
            mx, pos = b.abs().max().item(), (b > 0).double().mean().item()
            print(f"{name} map{i + 1} {tuple(m64[i].shape)}: max|x| {mx:.2f}, {100 * pos:.0f} % positive, fp32 - fp64 {e:.2e}")
            assert 1.0 <= mx <= 8.0 and pos >= 0.5 and e <= 1e-5, (name, i, mx, pos, e)
            e32.append(e)
            save[f"map{i + 1}_f64"] = b.numpy()
        save["e32"] = np.array(e32)
        fp = os.path.join(G.GOLD, f"resnet50_{name}.npz")
        np.savez_compressed(fp, **save)
        print(f"  -> {os.path.basename(fp)}: {os.path.getsize(fp) / 1e6:.2f} MB")
        assert os.path.getsize(fp) < (1 << 20)
    with open(os.path.join(G.GOLD, "resnet50_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
