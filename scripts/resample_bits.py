"""Digests of everything the Pillow resampler kernels and the aligned bilinear up-sample produce, for A/B runs of two builds of the
library that must agree bit for bit (a change of csrc/resample.h, preprocess.hip, present.hip or upsample.h that moves no arithmetic).

Runs a fixed, seeded case list on the library that SM_HIP_LIB names (default: lib/libselfmask_hip.so) and prints ONE JSON object
{case: sha256 of the output's bytes}: ``preprocess_on_device`` at S = 224 and 384 over the sizes of tests/test_hip_pipeline.py (fp32
and the resized uint8 images) and its two native-resolution paths, ``present_masks`` (mask and heat map) over tests/_present_cases.py,
and the aligned up-sample through both entry points.  ``--time`` prints timings instead (device events around ten calls queued back
to back, min / median / max per call over 30 repetitions): sm_preprocess_resize_u8 alone and the two up-samples.  Run it once per
library, each in a fresh process, and compare:

    SM_HIP_LIB=$PWD/salient-object-detection_amd/lib/libselfmask_hip_prev.so python scripts/resample_bits.py --out prev.json
    python scripts/resample_bits.py --out new.json
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [os.path.join(ROOT, "salient-object-detection_amd"), ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = torch.device("cuda:0")


def sha(t):
    a = t.contiguous().cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return hashlib.sha256(a.tobytes()).hexdigest()


def _images(S, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    sizes = [(300, 400), (371, 262), (224, 224), (97, 61), (400, 400), (S, S + 1), (1000, 333)]
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]


def bits():
    from _present_cases import KINDS, SHAPES, make_case
    from selfmask_amd import ops, pipeline as P, resnet as R, voting as VT
    res = {}
    for S in (224, 384):
        x, u8 = P.preprocess_on_device(_images(S, S), S, DEV, return_u8=True)
        res[f"preprocess|S{S}|f32"], res[f"preprocess|S{S}|u8"] = sha(x), sha(u8)
    imgs = _images(64, 5)[:4]
    res["preprocess|native"] = [sha(v) for v in P.preprocess_on_device(imgs, None, DEV)]
    res["preprocess|native|padded"] = sha(P.preprocess_on_device(imgs, None, DEV, pad_to=(384, 400)))
    for i in range(len(SHAPES)):
        for kind in KINDS:
            mask, rgb = make_case(i, kind)
            (m, h), = ops.present_masks(torch.from_numpy(mask[None]).to(DEV), [rgb])
            res[f"present|{i}|{kind}|mask"], res[f"present|{i}|{kind}|heat"] = sha(m), sha(h)
    for gh, gw, scale in ((14, 14, 2), (13, 21, 2), (5, 1, 3)):
        tok = torch.randn(2, gh * gw, 384, generator=torch.Generator().manual_seed(gh * 100 + gw)).to(DEV)
        res[f"upsample|tokens|{gh}x{gw}x{scale}"] = sha(VT.upsample_tokens_aligned(tok, gh, gw, scale))
    for h, w in ((3, 3), (5, 7)):
        for C in (2048, 384):
            f = torch.randn(2, h, w, C, generator=torch.Generator().manual_seed(h * w + C)).to(DEV)
            res[f"upsample|nhwc|{h}x{w}|C{C}"] = sha(R.upsample_nhwc_aligned(f, 2))
    return res


def _time(fn, calls=10, warmup=3, reps=30):
    us = []
    for rep in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        if rep >= warmup:
            us.append(e0.elapsed_time(e1) * 1e3 / calls)
    return f"min {min(us):9.2f}  median {float(np.median(us)):9.2f}  max {max(us):9.2f} us per call ({reps} x {calls} calls)"


def timings():
    from selfmask_amd import _native as N, pipeline as P, resnet as R, voting as VT
    lib, st = N.load(), torch.cuda.current_stream(DEV).cuda_stream
    B, S, side = 64, 224, 350
    rng = np.random.Generator(np.random.PCG64(1))
    pixels, coef, descr, max_h, _, _ = P.pack_images([rng.integers(0, 256, (side, side, 3), dtype=np.uint8) for _ in range(B)], S)
    pd, cd, dd, lut = pixels.to(DEV), coef.to(DEV), descr.to(DEV), P._lut(DEV)
    tmp = torch.empty((B, max_h * S * 3), dtype=torch.uint8, device=DEV)
    out = torch.empty((B, 3, S, S), dtype=torch.float32, device=DEV)
    u8 = torch.empty((B, S, S, 3), dtype=torch.uint8, device=DEV)
    for name, u in (("fp32 only", None), ("fp32 + u8", u8.data_ptr())):
        t = _time(lambda: N.check(lib.sm_preprocess_resize_u8(pd.data_ptr(), dd.data_ptr(), cd.data_ptr(), lut.data_ptr(), tmp.data_ptr(),
                                                              tmp.stride(0), out.data_ptr(), u, B, S, max_h, st), "sm_preprocess_resize_u8"))
        print(f"sm_preprocess_resize_u8  B = {B}, {side} x {side} -> {S}, {name}: {t}", flush=True)
    tok = torch.randn(64, 14 * 14, 384, device=DEV)
    print(f"upsample_tokens_aligned  B = 64, 14 x 14 x 384, x 2:         {_time(lambda: VT.upsample_tokens_aligned(tok, 14, 14, 2))}", flush=True)
    f, up = torch.randn(1, 28, 28, 2048, device=DEV), torch.empty(1, 56, 56, 2048, device=DEV)
    print(f"upsample_nhwc_aligned    B = 1, 28 x 28 x 2048, x 2:         {_time(lambda: R.upsample_nhwc_aligned(f, 2, up))}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the JSON object to this file")
    ap.add_argument("--time", action="store_true", help="print timings of the resize launch and the up-samples instead of digests")
    a = ap.parse_args()
    if a.time:
        timings()
        sys.exit(0)
    res = bits()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1, sort_keys=True) + "\n")
    print(json.dumps(res, sort_keys=True))
