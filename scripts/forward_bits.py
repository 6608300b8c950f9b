"""Digests of whole forwards, for A/B runs of two builds of the library whose results must be bit-identical (a change of host
code only: the launch sequence of csrc/forward.hip).

Runs a fixed, seeded case list on the library that SM_HIP_LIB names (default: lib/libselfmask_hip.so) and prints ONE JSON object
{case: {output name: sha256 of the tensor's bytes}} over every tensor of forward(..., return_logits=True) and of the attention
calls.  Run it once per library, each in a fresh process, and compare the two objects.

    SM_HIP_LIB=$PWD/salient-object-detection_amd/lib/libselfmask_hip_prev.so python scripts/forward_bits.py --out prev.json
    python scripts/forward_bits.py --out new.json
    python scripts/forward_bits.py --time     # instead: ms per forward of 200 eager, un-graphed B = 1 forwards, one synchronise at
                                              # the end (where the host code of the forward is the bottleneck), 3 repeats
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "salient-object-detection_amd"))

import torch  # noqa: E402
from selfmask_amd import MaskFormer, synthetic_state_dict, synthetic_images  # noqa: E402

DEV = "cuda:0"
MODES = ["w16", "f16x2", "fp32", "f16"]
# name: (patch, B, H, W, nq, L, attention_path, MaskFormer keywords)
FIVE_D = dict(return_intermediate=True, use_binary_classifier=True)
FFN = dict(return_intermediate=True, use_binary_classifier=False)
THREE_D = dict(return_intermediate=False, use_binary_classifier=False)
CASES = {
    "s16_224_b1_auto": (16, 1, 224, 224, 20, 6, "auto", FIVE_D),
    "s16_224_b2_fused": (16, 2, 224, 224, 20, 6, "fused", FIVE_D),
    "s16_224_b2_unfused": (16, 2, 224, 224, 20, 6, "unfused", FIVE_D),
    "s16_224_b16_auto": (16, 16, 224, 224, 20, 6, "auto", FIVE_D),
    "s16_224_b2_prenorm": (16, 2, 224, 224, 20, 6, "auto", dict(FIVE_D, normalize_before=True)),
    "s16_224_b2_ffn": (16, 2, 224, 224, 20, 6, "auto", FFN),
    "s16_224_b2_3d": (16, 2, 224, 224, 20, 6, "auto", THREE_D),
    "s8_72x88_b3": (8, 3, 72, 88, 20, 6, "auto", FIVE_D),
    "s8_72x88_b3_ffn": (8, 3, 72, 88, 20, 6, "auto", FFN),
    "s8_250x130_b1_nq33_L4": (8, 1, 250, 130, 33, 4, "auto", FIVE_D),
    "s16_224x192_b2_sf1": (16, 2, 224, 192, 20, 6, "auto", dict(FIVE_D, scale_factor=1)),
    "s16_224x192_b2_sf4": (16, 2, 224, 192, 20, 6, "auto", dict(FIVE_D, scale_factor=4)),
}
ATTENTION_CASE = "s16_224_b2_fused"  # also run with return_attention / get_last_selfattention / encoder_only ("f16" has no maps)


def _model(patch, nq, L, path, kw, mode, seed=1):
    m = MaskFormer(n_queries=nq, patch_size=patch, n_decoder_layers=L, gemm_mode=mode, **kw)
    m.load_state_dict(synthetic_state_dict(seed, "calib", n_queries=nq, patch_size=patch, n_decoder_layers=L,
                                           use_binary_classifier=kw["use_binary_classifier"]), strict=True)
    m = m.to(DEV)
    m.attention_path = path
    return m


def _digests(out):
    torch.cuda.synchronize()
    return {k: hashlib.sha256(v.contiguous().cpu().numpy().tobytes()).hexdigest() for k, v in sorted(out.items())}


def bits():
    res = {}
    for mode in MODES:
        for name, (patch, B, H, W, nq, L, path, kw) in CASES.items():
            m = _model(patch, nq, L, path, kw, mode)
            x = torch.from_numpy(synthetic_images(40, (B, 3, H, W))).to(DEV)
            res[f"{name}|{mode}"] = _digests(m(x, return_logits=True))
            if name == ATTENTION_CASE:
                res[f"{name}|{mode}|encoder_only"] = _digests(m(x, encoder_only=True))
                if mode != "f16":
                    res[f"{name}|{mode}|return_attention"] = _digests(m(x, return_logits=True, return_attention=True))
                    res[f"{name}|{mode}|return_attention_cls"] = _digests(m(x, return_logits=True, return_attention="cls"))
                    res[f"{name}|{mode}|get_last_selfattention"] = _digests({"attn": m.get_last_selfattention(x),
                                                                             "cls": m.get_last_selfattention(x, cls_only=True)})
    return res


def eager_b1_ms(forwards=200, repeats=3):
    patch, B, H, W, nq, L, path, kw = CASES["s16_224_b1_auto"]
    m = _model(patch, nq, L, path, kw, "w16")
    x = torch.from_numpy(synthetic_images(40, (B, 3, H, W))).to(DEV)
    for _ in range(20):
        m(x)
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(forwards):
            m(x)
        torch.cuda.synchronize()
        out.append(round((time.perf_counter() - t0) * 1e3 / forwards, 4))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the JSON object to this file")
    ap.add_argument("--time", action="store_true", help="time eager B = 1 forwards instead of hashing outputs")
    a = ap.parse_args()
    res = {"eager_b1_ms_per_forward": eager_b1_ms()} if a.time else bits()
    text = json.dumps(res, indent=1, sort_keys=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(res, sort_keys=True))
