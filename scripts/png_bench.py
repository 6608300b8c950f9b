"""The device PNG encoder against Pillow on the host -> profiles/png_bench.log.

Uploads of 300 x 400 and 1080 x 1920 (scripts/present_bench.py's smooth synthetic picture with noise), masks of 28 x 28 (patch 16).
Steps, each a child process of its own under its own time limit (a step that fails or runs out of time ends the run):
  kernel   sm_png_encode_batch_u8 of the response's three pictures (RGB upload, L mask, RGBA heat map) in one call: per launch, the
           device-event pairs of the library's own taps (sm_forward_timing) around each of the four launches.
  encode   ops.png_encode of the three pictures (launches, sizes, the used bytes into page-locked memory, bytes objects) against Pillow
           encoding the same three arrays on the host: the same process, alternating, wall clock.
  predict  predict(encoder="device") against predict() of the same commit (the parent's figures: profiles/present_bench.log), with
           predict_png() and the base64 of its three files alone alongside.
  sizes    the files' sizes against Pillow's, for the three pictures and for tests/_present_cases.make_case(0, kind) at 300 x 400.
Every time: the median of REPS timed repetitions after WARMUP, with the min - max range.

    python scripts/png_bench.py            # all steps, tee'd into profiles/png_bench.log
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
STEPS = {"kernel": 200, "encode": 400, "predict": 500, "sizes": 200}  # seconds
WARMUP, REPS = 3, 30
UPLOADS = ((300, 400), (1080, 1920))
PATCH, SIDE = 16, 28


def _three(H, W):
    """the response's three pictures for the bench's upload and a seeded mask, on the host: (rgb, mask, heat map)"""
    import numpy as np
    from present_bench import _upload
    from selfmask_amd.present import present_reference_numpy
    rgb = _upload(H, W)
    mask = np.random.Generator(np.random.PCG64(SIDE)).random((SIDE, SIDE), dtype=np.float32)
    m, h = present_reference_numpy(mask, rgb)
    return rgb, m, h


def _pillow(a):
    from PIL import Image
    buf = BytesIO()
    Image.fromarray(a).save(buf, format="PNG")
    return buf.getvalue()


def step_kernel():
    import numpy as np
    import torch
    from present_bench import _stats
    from selfmask_amd import _native as N, ops
    dev = torch.device("cuda:0")
    lib = N.load()
    for (H, W) in UPLOADS:
        arrays = _three(H, W)
        tensors = [torch.from_numpy(a).to(dev) for a in arrays]
        flat = torch.cat([t.reshape(-1) for t in tensors])
        offs = np.cumsum([0] + [a.size for a in arrays[:-1]]).tolist()
        shapes = [(H, W, 3), (H, W, 1), (H, W, 4)]
        us = {}
        for rep in range(WARMUP + REPS):
            N.check(lib.sm_forward_timing(1), "sm_forward_timing")
            pending = ops.png_encode_async(packed=(flat, offs, shapes))
            buf = (N.KernelTime * 16)()
            n = lib.sm_forward_timing_read(buf, 16)
            lib.sm_forward_timing(0)
            files = pending.result()
            if rep >= WARMUP:
                for k in range(n):
                    us.setdefault(buf[k].name.decode(), []).append(buf[k].total_us)
        chunks = sum(-(-(H * (W * c + 1)) // 16384) for _, _, c in shapes)
        print(f"kernel  {H:4d} x {W:4d}: three pictures, {flat.numel() / 1e6:.2f} MB of pixels, {chunks} chunks -> {sum(map(len, files)) / 1e6:.2f} MB of files")
        for name, v in us.items():
            print(f"  {name:12s} {_stats(v, 'us')}")
        tot = np.sum([v for v in us.values()], axis=0)
        print(f"  {'all four':12s} {_stats(tot, 'us')}  {flat.numel() / np.median(tot) / 1e3:.1f} GB/s of pixels at the median", flush=True)


def step_encode():
    import numpy as np
    import torch
    from present_bench import _alternate, _stats
    from selfmask_amd import ops, png
    dev = torch.device("cuda:0")
    for (H, W) in UPLOADS:
        arrays = _three(H, W)
        tensors = [torch.from_numpy(a).to(dev) for a in arrays]
        sides = {"ops.png_encode": lambda: ops.png_encode(tensors), "Pillow, host": lambda: [_pillow(a) for a in arrays]}
        ms, last = _alternate(sides)
        ok = H * W > 200000 or last["ops.png_encode"] == [png.encode_reference(a) for a in arrays]
        from PIL import Image
        decoded = all(np.array_equal(np.asarray(Image.open(BytesIO(f))), a) for f, a in zip(last["ops.png_encode"], arrays))
        print(f"encode  {H:4d} x {W:4d}: three pictures; Pillow decodes the device's files to the inputs: {decoded}"
              + ("" if H * W > 200000 else f"; bytes equal the restatement: {ok}"))
        for k in sides:
            print(f"  {k:18s} {_stats(ms[k])}")
        print(f"  Pillow / ops.png_encode (medians) = {np.median(ms['Pillow, host']) / np.median(ms['ops.png_encode']):.1f}x", flush=True)


def step_predict():
    import numpy as np
    from PIL import Image
    from present_bench import _alternate, _inference, _stats, _upload
    inf = _inference(PATCH)
    for (H, W) in UPLOADS:
        rgb = _upload(H, W)
        files = inf.predict_png(rgb)
        three = [files[k] for k in ("original", "mask", "heatmap")]
        sides = {'predict(encoder="device")': lambda: inf.predict(rgb, encoder="device"), "predict()": lambda: inf.predict(rgb),
                 "predict_png()": lambda: inf.predict_png(rgb), "predict_images()": lambda: inf.predict_images(rgb),
                 "base64 of the files": lambda: [base64.b64encode(f).decode() for f in three]}
        ms, last = _alternate(sides)
        dev_r, host_r = last['predict(encoder="device")'], last["predict()"]

        def px(url):
            return np.asarray(Image.open(BytesIO(base64.b64decode(url.split(",", 1)[1]))))
        same = all(np.array_equal(px(dev_r[k]), px(host_r[k])) for k in ("original", "mask", "heatmap"))
        print(f"predict {H:4d} x {W:4d}, mask {SIDE} x {SIDE} (patch {PATCH}); the two responses decode to the same pixels: {same}")
        for k in sides:
            print(f"  {k:26s} {_stats(ms[k])}")
        d, h, b = (ms[k] for k in ('predict(encoder="device")', "predict()", "base64 of the files"))
        apart = max(d) < min(h)
        print(f"  predict() / predict(encoder=\"device\") (medians) = {np.median(h) / np.median(d):.1f}x; ranges apart: {apart}; base64 is "
              f"{100 * np.median(b) / np.median(d):.0f} % of the device path", flush=True)


def step_sizes():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from _present_cases import KINDS, make_case
    from selfmask_amd import ops
    from selfmask_amd.present import present_reference_numpy
    dev = torch.device("cuda:0")
    rows = []
    for (H, W) in UPLOADS:
        for name, a in zip(("upload RGB", "mask L", "heat map RGBA"), _three(H, W)):
            rows.append((f"{H} x {W} {name}", a))
    for kind in KINDS:
        mask, rgb = make_case(0, kind)
        m, h = present_reference_numpy(mask, rgb)
        rows += [(f"make_case(0, {kind}) mask", m), (f"make_case(0, {kind}) heat map", h)]
    for name, a in rows:
        dev_file, = ops.png_encode([torch.from_numpy(a).to(dev)])
        pil = _pillow(a)
        print(f"sizes   {name:38s} raw {a.size:9d}  Pillow {len(pil):9d}  device {len(dev_file):9d}  device / Pillow = {len(dev_file) / len(pil):.3f}",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS), default=None)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "png_bench.log"))
    args = ap.parse_args()
    if args.step:
        {"kernel": step_kernel, "encode": step_encode, "predict": step_predict, "sizes": step_sizes}[args.step]()
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
