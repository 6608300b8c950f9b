#!/usr/bin/env python3
"""The neighbour lists at 2048 dimensions and the pseudo-mask generator with one, two and three feature types, on the MI355X.

Part 1 (``sm_knn_f32`` through ``voting.knn``, device events around each call, F16X2 split and squared norms included):
  - D = 2048, n = 8192, B = 1: the streaming kernel against the Gram-matrix path, the two alternating call by call;
  - D = 2048, n = 19 200 (a 480 x 640 photo's ResNet grid), B = 1 and B = 8: streaming against the Gram matrix in slabs of 2048 rows;
  - D = 384, n = 32 400, B = 1: the same pair at the width DESIGN.md quotes for the kernel with the query fragments in registers.
  TFLOP/s counts 2 B n^2 D per call (fp32-grade products: the three f16 MFMA products of a multiply-add count once).
Part 2 (``MaskGenerator.__call__``, host clock around whole passes over the files, run-length codes out): images / s with
  ["dino"], ["mocov2", "dino"] and ["mocov2", "swav", "dino"] on synthetic 224 x 224 and 300 x 400 PNG files (synthetic weights: the
  arithmetic does not depend on them; the eigen-solver's iteration count does depend on the features).
Every line is the median of the timed repeats with min - max.  usage: knn_dim_bench.py [--out FILE] [--reps 30] [--passes 5] [--files 32]"""
import argparse
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "salient-object-detection_amd"), REPO, os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "knn_dim_bench.log"))
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--files", type=int, default=32)
ap.add_argument("--skip-generator", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("knn_dim_bench.py measures on the GPU; there is none here")
from selfmask_amd import voting as VT  # noqa: E402

DEV = torch.device("cuda:0")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
log = open(args.out, "w")


def say(line=""):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def stats(v):
    v = np.asarray(v)
    return float(np.median(v)), float(v.min()), float(v.max())


def time_knn(x, methods, reps):
    """ms per call of voting.knn(x, 10, method), the methods alternating call by call; one warm-up call each"""
    out = {m: [] for m in methods}
    for m in methods:
        VT.knn(x, 10, m)
    torch.cuda.synchronize()
    for _ in range(reps):
        for m in methods:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            VT.knn(x, 10, m)
            b.record()
            b.synchronize()
            out[m].append(a.elapsed_time(b))
    return out


say(f"# knn_dim_bench.py on {torch.cuda.get_device_name(0)}; knn: median of {args.reps} calls (min - max), 10 neighbours")
gen = torch.Generator(device=DEV).manual_seed(5)
for D, n, B, methods in ((2048, 8192, 1, ("stream", "gram")), (2048, 19200, 1, ("stream", "gram")), (2048, 19200, 8, ("stream", "gram")),
                         (384, 32400, 1, ("stream", "gram"))):
    x = torch.randn((B, n, D), generator=gen, device=DEV, dtype=torch.float32)
    t = time_knn(x, methods, args.reps)
    lists = {m: VT.knn(x, 10, m) for m in methods}
    for m in methods:
        med, lo, hi = stats(t[m])
        tf = 2.0 * B * n * n * D / 1e12
        name = "gram slabs" if m == "gram" and n > VT.SPECTRAL_GRAM_POINTS else m
        say(f"knn D={D} n={n} B={B} {name:10s}: {med:9.3f} ms ({lo:.3f} - {hi:.3f}), {med / B:9.3f} ms / image, "
            f"{tf / (med * 1e-3):7.1f} TFLOP/s fp32-grade ({3 * tf / (med * 1e-3):7.1f} of f16 MFMA issue)")
    if len(methods) == 2:
        same = (lists[methods[0]] == lists[methods[1]]).all(dim=2).float().mean().item()
        say(f"    rows with identical lists, {methods[0]} against {methods[1]}: {100 * same:.3f} %")
    del x, lists
    VT.release_scratch()
    torch.cuda.empty_cache()

if not args.skip_generator:
    import _resnet_cases as RC
    from PIL import Image
    from selfmask_amd import MaskFormer, ResNet50, synthetic_state_dict
    from selfmask_amd.datasets import synthetic_scene
    from selfmask_amd.mask_generator import MaskGenerator
    model = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    model.load_state_dict(synthetic_state_dict(31, "soft", patch_size=16), strict=True)
    model = model.to(DEV)
    backbones = {}
    for name, seed in (("mocov2", 11), ("swav", 12)):
        r = ResNet50(use_dilated_resnet=True)
        r.load_state_dict(RC.synthetic_resnet_state_dict(seed, True), strict=True)
        backbones[name] = r.to(DEV).eval()
    say(f"# MaskGenerator(...)(files): {args.files} PNG files of one size, batch_size 16, 3 streams; median of {args.passes} passes "
        f"(min - max) after one warm-up pass")
    with tempfile.TemporaryDirectory() as d:
        for h, w in ((224, 224), (300, 400)):
            rng = np.random.Generator(np.random.PCG64(h))
            paths = []
            for i in range(args.files):
                p = os.path.join(d, f"s{h}x{w}_{i}.png")
                Image.fromarray(synthetic_scene(rng, h, w)[0]).save(p)
                paths.append(p)
            for types_ in (["dino"], ["mocov2", "dino"], ["mocov2", "swav", "dino"]):
                g = MaskGenerator(feature_types=types_, network=model, backbones=backbones, device=DEV, batch_size=16)
                g(paths)
                torch.cuda.synchronize()
                rates = []
                for _ in range(args.passes):
                    t0 = time.perf_counter()
                    out = g(paths)
                    torch.cuda.synchronize()
                    rates.append(len(out) / (time.perf_counter() - t0))
                med, lo, hi = stats(rates)
                say(f"generator {h}x{w} {'+'.join(types_):18s}: {med:8.2f} images / s ({lo:.2f} - {hi:.2f}), "
                    f"{sum(g.cluster_sizes) * len(types_)} candidates per image")
                del g
                VT.release_scratch()
                torch.cuda.empty_cache()
log.close()
