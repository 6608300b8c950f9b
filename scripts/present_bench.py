"""The response's images on the device against the host chain -> profiles/present_bench.log.

Uploads of 300 x 400 and 1080 x 1920 (a smooth synthetic picture with noise), masks of 28 x 28 (patch 16) and 56 x 56 (patch 8).
Steps, each a child process of its own under its own time limit (a step that fails or runs out of time ends the run):
  kernel   sm_present_masks_u8 alone (both launches, mask + heat map): device events around 10 calls queued back to back, per call in
           microseconds, and the GB/s that is of the bytes the call must move (3 B read + 5 B written per pixel, the mask, the
           intermediate written and read once).
  images   SelfMaskInference.predict_images() against the host chain (Pillow LANCZOS, matplotlib jet, Image.blend, Brightness) fed
           from predict_tensors(): the same process, alternating, wall clock from the call to the arrays on the host.
  predict  whole predict() (three PNG data URLs) against the parent commit's predict(), restated here from predict_tensors() and the
           host chain; the three PNG encodes alone alongside, to show the share of a request that is left to the encoder.
Every figure: the median of REPS timed repetitions after WARMUP, with the min - max range.

    python scripts/present_bench.py            # all steps, tee'd into profiles/present_bench.log
"""
import argparse
import base64
import os
import subprocess
import sys
import time
from io import BytesIO

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "salient-object-detection_amd"))
STEPS = {"kernel": 200, "images": 300, "predict": 400}  # seconds
WARMUP, REPS = 3, 30
UPLOADS = ((300, 400), (1080, 1920))
PATCHES = ((16, 28), (8, 56))  # patch size -> side of the mask
CFG = dict(n_queries=20, n_decoder_layers=6, learnable_pixel_decoder=False, lateral_connection=False, loss_every_decoder_layer=True,
           scale_factor=2, abs_2d_pe_init=False, use_binary_classifier=True, arch="vit_small", training_method="dino")


def _stats(v, unit="ms"):
    import numpy as np
    v = np.asarray(v)
    return f"median {np.median(v):9.3f}  min {v.min():9.3f}  max {v.max():9.3f} {unit} ({len(v)} reps)"


def _upload(h, w):
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(h))
    yy, xx = np.mgrid[:h, :w]
    rgb = np.stack([120 + 80 * np.sin(xx / 23.0), 90 + 60 * np.cos(yy / 31.0), 60 + 0.1 * xx], -1)
    return np.clip(rgb + rng.standard_normal(rgb.shape) * 6, 0, 255).astype(np.uint8)


def _inference(patch):
    import torch
    from argparse import Namespace
    from selfmask_amd import MaskFormer, SelfMaskInference, synthetic_state_dict
    m = MaskFormer(n_queries=20, patch_size=patch, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    m.load_state_dict(synthetic_state_dict(2, "soft", patch_size=patch), strict=True)
    return SelfMaskInference(None, Namespace(patch_size=patch, **CFG), device=torch.device("cuda:0"), model=m)


def _host_images(t, rgb):
    """the reference's chain (app.py:296-311) on the host, as the parent commit's predict() ran it -> (mask image, heat image)"""
    import matplotlib.pyplot as plt
    import numpy as np
    from PIL import Image, ImageEnhance
    original = Image.fromarray(rgb)
    mask_img = Image.fromarray((t["mask"] * 255).astype(np.uint8)).resize(original.size, Image.Resampling.LANCZOS)
    rgba = (plt.get_cmap("jet")(np.array(mask_img) / 255.0) * 255).astype(np.uint8)
    heat_img = Image.fromarray(rgba).convert("RGBA").resize(original.size, Image.Resampling.LANCZOS)
    return mask_img, ImageEnhance.Brightness(Image.blend(original.convert("RGBA"), heat_img, alpha=0.5)).enhance(1.1)


def _url(img):
    buf = BytesIO()
    img.save(buf, format="PNG")
    return "data:image/png;base64," + base64.b64encode(buf.getvalue()).decode()


def _alternate(sides):
    import torch
    ms = {k: [] for k in sides}
    last = {}
    for rep in range(WARMUP + REPS):
        for name, fn in sides.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            last[name] = fn()
            if rep >= WARMUP:
                ms[name].append((time.perf_counter() - t) * 1e3)
    return ms, last


def step_kernel():
    import numpy as np
    import torch
    from selfmask_amd import _native as N, ops
    from selfmask_amd.present import present_reference_numpy
    dev = torch.device("cuda:0")
    lib = N.load()
    calls = 10
    for (H, W) in UPLOADS:
        for _, side in PATCHES:
            rng = np.random.Generator(np.random.PCG64(side))
            masks = torch.from_numpy(rng.random((1, side, side), dtype=np.float32)).to(dev)
            rgb = _upload(H, W)
            pixels = torch.from_numpy(rgb.reshape(-1)).to(dev)
            t = ops._present_tables(side, side, ((H, W, 0),), dev)
            lut = ops._present_lut(dev)
            wsb = lib.sm_present_workspace_bytes(1, side, W)
            ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
            mask_out = torch.zeros(H * W, dtype=torch.uint8, device=dev)
            heat_out = torch.zeros(4 * H * W, dtype=torch.uint8, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            nbytes = 8 * H * W + 4 * side * side + 2 * side * W
            us = []
            for rep in range(WARMUP + REPS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    N.check(lib.sm_present_masks_u8(masks.data_ptr(), side * side, side, side, pixels.data_ptr(), t.host, t.dev.data_ptr(),
                                                    t.coef.data_ptr(), lut.data_ptr(), 0.5, 1.1, mask_out.data_ptr(), heat_out.data_ptr(),
                                                    ws.data_ptr(), wsb, 1, st), "sm_present_masks_u8")
                e1.record()
                e1.synchronize()
                if rep >= WARMUP:
                    us.append(e0.elapsed_time(e1) * 1e3 / calls)
            wm, wh = present_reference_numpy(masks[0].cpu().numpy(), rgb)
            same = np.array_equal(mask_out.cpu().numpy(), wm.reshape(-1)) and np.array_equal(heat_out.cpu().numpy(), wh.reshape(-1))
            med = float(np.median(us))
            print(f"kernel  {H:4d} x {W:4d}, mask {side} x {side}: {_stats(us, 'us')}  {nbytes / 1e6:6.2f} MB -> "
                  f"{nbytes / med / 1e3:7.1f} GB/s at the median (range {nbytes / max(us) / 1e3:.1f} - {nbytes / min(us) / 1e3:.1f}); "
                  f"bits equal the reference: {same}", flush=True)


def step_images():
    import numpy as np
    for patch, side in PATCHES:
        inf = _inference(patch)
        for (H, W) in UPLOADS:
            rgb = _upload(H, W)
            sides = {"predict_images()": lambda: inf.predict_images(rgb),
                     "host chain": lambda: _host_images(inf.predict_tensors(rgb), rgb),
                     "predict_tensors()": lambda: inf.predict_tensors(rgb)}
            ms, last = _alternate(sides)
            same = np.array_equal(last["predict_images()"]["mask"], np.array(last["host chain"][0])) and \
                np.array_equal(last["predict_images()"]["heatmap"], np.array(last["host chain"][1]))
            print(f"images  {H:4d} x {W:4d}, mask {side} x {side} (patch {patch}); arrays equal: {same}")
            for k in sides:
                print(f"  {k:18s} {_stats(ms[k])}")
            a, b = np.median(ms["host chain"]), np.median(ms["predict_images()"])
            print(f"  host chain / predict_images() (medians) = {a / b:.2f}x; the images add {b - np.median(ms['predict_tensors()']):.3f} ms "
                  f"to predict_tensors() on the device, {a - np.median(ms['predict_tensors()']):.3f} ms on the host", flush=True)


def step_predict():
    import numpy as np
    from PIL import Image
    for patch, side in PATCHES:
        inf = _inference(patch)
        for (H, W) in UPLOADS:
            rgb = _upload(H, W)

            def parent():
                t = inf.predict_tensors(rgb)
                mask_img, heat = _host_images(t, rgb)
                return {"original": _url(Image.fromarray(rgb)), "mask": _url(mask_img), "heatmap": _url(heat)}

            got = inf.predict_images(rgb)
            imgs = (Image.fromarray(rgb), Image.fromarray(got["mask"]), Image.fromarray(got["heatmap"]))
            sides = {"predict()": lambda: inf.predict(rgb), "parent's predict()": parent,
                     "three PNG encodes": lambda: [_url(im) for im in imgs]}
            ms, last = _alternate(sides)
            same = all(last["predict()"][k] == last["parent's predict()"][k] for k in ("original", "mask", "heatmap"))
            print(f"predict {H:4d} x {W:4d}, mask {side} x {side} (patch {patch}); data URLs equal: {same}")
            for k in sides:
                print(f"  {k:18s} {_stats(ms[k])}")
            a, b, e = (np.median(ms[k]) for k in ("parent's predict()", "predict()", "three PNG encodes"))
            print(f"  parent / predict() (medians) = {a / b:.2f}x; the encoder is {100 * e / b:.0f} % of predict() "
                  f"({100 * e / a:.0f} % of the parent's)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS), default=None)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "present_bench.log"))
    args = ap.parse_args()
    if args.step:
        {"kernel": step_kernel, "images": step_images, "predict": step_predict}[args.step]()
        return 0
    with open(args.log, "w") as log:
        for step, limit in STEPS.items():
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], timeout=limit, capture_output=True, text=True)
            except subprocess.TimeoutExpired:
                log.write(f"[{step}] ran out of its {limit} s\n")
                print(f"[{step}] ran out of its {limit} s")
                return 124
            log.write(p.stdout)
            log.flush()
            print(p.stdout, end="", flush=True)
            if p.returncode != 0:
                log.write(f"[{step}] failed with status {p.returncode}\n{p.stderr[-2000:]}\n")
                print(p.stderr[-2000:])
                return p.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
