"""Digests of everything sm_evaluate_masks_f32 returns, for A/B runs of two builds of the library that must agree bit for bit (a change
of csrc/eval.hip that moves no arithmetic and keeps the order of every fp64 sum).

Runs a fixed, seeded case list on the library that SM_HIP_LIB names (default: lib/libselfmask_hip.so) and prints ONE JSON object
{case: sha256 of the bytes of ``rows`` and ``ious``}: every case of tests/_eval_cases.py, the plateau constants, the three workloads
of scripts/eval_bench.py (B = 64, nq = 20, mask sides 28 / 56 / 48, its seed) and one nq = 100 batch of four 300-400 px images.
``--time`` prints what scripts/eval_bench.py prints instead.  Run it once per library, each in a fresh process, and compare; with a
tuning library SM_EVAL_BAND_MIN=0 (raster walk for every image) and SM_EVAL_UPW=1 (one unit per wave) reach the other paths:

    SM_HIP_LIB=$PWD/salient-object-detection_amd/lib/libselfmask_hip_prev.so python scripts/eval_bits.py --out prev.json
    python scripts/eval_bits.py --out new.json
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [os.path.join(ROOT, "salient-object-detection_amd"), ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"


def _digest(masks, objs, gts, scale):
    from selfmask_amd import ops
    as_dev = lambda v: (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v).to(DEV)  # noqa: E731
    rows, ious = ops.evaluate_masks(as_dev(masks), as_dev(objs), gts if isinstance(gts, ops.GtBatch) else [as_dev(g) for g in gts],
                                    scale=scale, return_ious=True)
    return hashlib.sha256(rows.contiguous().cpu().numpy().tobytes() + ious.contiguous().cpu().numpy().tobytes()).hexdigest()


def _bench_gts(B, seed=99):
    """the ground truths of scripts/eval_bench.py: ellipses of 300-400 px a side"""
    rng = np.random.Generator(np.random.PCG64(seed))
    gts = []
    for _ in range(B):
        h, w = (int(v) for v in rng.integers(300, 401, size=2))
        yy, xx = np.mgrid[:h, :w]
        gts.append(torch.from_numpy(((((yy - h * rng.uniform(.3, .7)) / (h * rng.uniform(.1, .3))) ** 2 +
                                      ((xx - w * rng.uniform(.3, .7)) / (w * rng.uniform(.1, .3))) ** 2) <= 1).astype(np.uint8)))
    return gts


def bits():
    import _eval_cases as C
    from selfmask_amd import ops
    res = {}
    for i, case in enumerate(C.CASES):
        res[f"case|{case[0]}"] = _digest(*C.build_case(i), case[1])
    for c in (0.7,) + C.PLATEAU_OTHERS:
        res[f"plateau|{c}"] = _digest(*C.plateau_case(c), 0)
    gb = ops.GtBatch(_bench_gts(64), DEV)
    for side in (28, 56, 48):  # the inputs of eval_bench.py, drawn as it draws them
        torch.manual_seed(side)
        mp = torch.sigmoid(torch.randn(64, 20, side, side, device=DEV) * 3)
        res[f"bench|{side}"] = _digest(mp, torch.rand(64, 20, device=DEV), gb, 0.0)
    g = torch.Generator().manual_seed(100)
    mp = torch.sigmoid(torch.randn(4, 100, 28, 28, generator=g) * 3)
    res["nq100"] = _digest(mp, torch.rand(4, 100, generator=g), _bench_gts(4, seed=100), 0.0)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the JSON object to this file")
    ap.add_argument("--time", action="store_true", help="print the timings of scripts/eval_bench.py instead of digests")
    ap.add_argument("sides", nargs="*", type=int, help="with --time: the mask sides (default 28 56 48)")
    a = ap.parse_args()
    if a.time:
        import eval_bench
        sys.argv[1:] = [str(s) for s in a.sides]
        eval_bench.main()
        sys.exit(0)
    res = bits()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1, sort_keys=True) + "\n")
    print(json.dumps(res, sort_keys=True))
