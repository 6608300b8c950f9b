"""Bilateral refinement at native resolution: what the mixed-size solver batch buys.

One synthetic dataset of native sizes (300-400 px, ViT-S/16: a few dozen token grids), then, the two sides of every comparison
alternating inside this one run, each side until it has run for more than a second:
  (a) native bucketed evaluation without refinement      | (b) the same with refine="bilateral"        [wall clock, whole pipeline]
  (c) the solver alone on one bucket as ONE mixed batch  | (d) the same images, one single solve each  [device events]
  (e) 32 x 384^2 through the mixed entry point (and with its table built beforehand) | the uniform batch entry point [device events]
Every figure is mean +- standard deviation over the repetitions (min .. max)."""
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "salient-object-detection_amd"))
from selfmask_amd import MaskFormer, synthetic_state_dict  # noqa: E402
from selfmask_amd import datasets as DS  # noqa: E402
from selfmask_amd.bilateral_solver import (MixedBatch, bilateral_solver_batch_device, bilateral_solver_mixed_device,  # noqa: E402
                                           bilateral_solver_mixed_packed, bilateral_solver_output_device)
from selfmask_amd.evaluator import Evaluator  # noqa: E402
from selfmask_amd.pipeline import native_buckets  # noqa: E402

DEV = torch.device("cuda:0")
N_IMAGES, BATCH, MIN_SECONDS, MIN_REPS = 512, 32, 1.2, 5


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(sides, clock, warmup=2):
    """sides: {name: callable}; one repetition = every side once, in turn."""
    for _ in range(warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    while min(sum(v) for v in ms.values()) < MIN_SECONDS * 1e3 or len(next(iter(ms.values()))) < MIN_REPS:
        for k, fn in sides.items():
            ms[k].append(clock(fn))
    return {k: np.array(v) for k, v in ms.items()}


def report(label, ms, n_images):
    print(f"  {label:58s} {ms.mean():9.3f} ms +- {ms.std():6.3f} ({ms.min():.3f} .. {ms.max():.3f}, {len(ms)} reps)"
          f"   {n_images / ms.mean() * 1e3:8.0f} images/s", flush=True)


def main():
    model = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    model.load_state_dict(synthetic_state_dict(24, "calib", patch_size=16), strict=True)
    model = model.to(DEV).eval()
    root = tempfile.mkdtemp(prefix="sm_refine_native_")
    try:
        DS.write_synthetic_dataset(root, "duts", N_IMAGES, seed=7, size_range=(300, 400))
        ds = DS.get_dataset(root, "duts")
        sizes = [ds.image_size(i) for i in range(N_IMAGES)]
        plan = native_buckets(sizes, 16, BATCH)
        print(f"{N_IMAGES} images of {min(h for h, _ in sizes)}-{max(h for h, _ in sizes)} x {min(w for _, w in sizes)}-"
              f"{max(w for _, w in sizes)} px, {len({(-(-h // 16), -(-w // 16)) for h, w in sizes})} token grids, {len(plan)} buckets of <= {BATCH}")
        ev = Evaluator(network=model, dir_dataset=root)
        ev.device = DEV
        run = lambda **kw: ev("duts", dir_ckpt=os.path.join(root, "ck"), batch_size=BATCH, device=DEV, streams=3, **kw)  # noqa: E731
        ms = alternate({"a": lambda: run(), "b": lambda: run(refine="bilateral")}, wall_ms, warmup=1)
        print("native bucketed evaluation (decode + forward + metrics [+ refinement]), wall clock:")
        report("(a) without refinement", ms["a"], N_IMAGES)
        report("(b) refine='bilateral' (one mixed solve per bucket)", ms["b"], N_IMAGES)

        bucket = max(plan, key=len)
        from PIL import Image
        rng = np.random.Generator(np.random.PCG64(3))
        imgs, tgts = [], []
        for i in bucket:
            gt = np.asarray(Image.open(ds.p_gts[i]).convert("L")) > 127
            imgs.append(torch.from_numpy(np.asarray(Image.open(ds.p_imgs[i]).convert("RGB")).copy()).to(DEV))
            tgts.append(torch.from_numpy(np.clip(0.15 + 0.7 * gt + rng.standard_normal(gt.shape) * 0.1, 0, 1)).to(DEV))
        shapes = [tuple(t.shape) for t in tgts]
        pix, tg = torch.cat([i.reshape(-1) for i in imgs]), torch.cat([t.reshape(-1) for t in tgts])
        mixed = lambda: bilateral_solver_mixed_device(pix, tg, shapes=shapes)  # noqa: E731
        loop = lambda: [bilateral_solver_output_device(i, t) for i, t in zip(imgs, tgts)]  # noqa: E731
        same = all(torch.equal(a, b[1]) for a, b in zip(mixed()[1], loop()))
        ms = alternate({"c": mixed, "d": loop}, device_ms)
        print(f"the solver alone on one bucket: {len(bucket)} images of {min(shapes)} .. {max(shapes)}, device events (binary identical: {same}):")
        report("(c) one mixed batch", ms["c"], len(bucket))
        report("(d) a loop of single solves", ms["d"], len(bucket))
        print(f"  (d) / (c) = {ms['d'].mean() / ms['c'].mean():.2f}x")

        S, n = 384, 32
        scenes = [DS.synthetic_scene(rng, S, S) for _ in range(n)]
        I = torch.from_numpy(np.stack([im for im, _ in scenes])).to(DEV)
        T = torch.from_numpy(np.stack([np.clip(0.15 + 0.7 * g + rng.standard_normal((S, S)) * 0.1, 0, 1) for _, g in scenes])).to(DEV)
        If, Tf = I.reshape(-1), T.reshape(-1)
        mb = MixedBatch([(S, S)] * n, DEV)  # the table built and uploaded once: the launch sequence alone
        ms = alternate({"mixed": lambda: bilateral_solver_mixed_device(If, Tf, shapes=[(S, S)] * n),
                        "prebuilt": lambda: bilateral_solver_mixed_packed(If, Tf, mb),
                        "uniform": lambda: bilateral_solver_batch_device(I, T)}, device_ms)
        print(f"(e) {n} x {S}^2, device events:")
        report("mixed entry point (sm_bilateral_solver_mixed_f64)", ms["mixed"], n)
        report("mixed entry point, descriptor table already on the device", ms["prebuilt"], n)
        report("uniform entry point (sm_bilateral_solver_batch_f64)", ms["uniform"], n)
        print(f"  mixed / uniform = {ms['mixed'].mean() / ms['uniform'].mean():.4f}, table prebuilt / uniform = "
              f"{ms['prebuilt'].mean() / ms['uniform'].mean():.4f}   (uniform's own spread: +- {ms['uniform'].std() / ms['uniform'].mean():.4f})")
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
