"""ms per forward under "auto" and under the "fused" pin at batches of 16 images or more with at most 512 token rows.  Written when
the two differed in fc2 there (auto: four K-slices summed by the next LayerNorm launch; pin: one launch) - the log it made is the
price of making them equal; on the forward as it is both columns time the same launches.  Eager forwards on one stream,
300 per window between device events after 10 warm-up calls, the two paths alternating, medians (min-max) of 7 windows each.
    python scripts/auto_vs_pin_time.py  ->  profiles/auto_vs_fused_pin_small_grids.log"""
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "salient-object-detection_amd"), REPO]
import torch  # noqa: E402
from selfmask_amd import MaskFormer, synthetic_images, synthetic_state_dict  # noqa: E402

DEV = "cuda:0"
m = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True, gemm_mode="w16")
m.load_state_dict(synthetic_state_dict(4, "calib", patch_size=16), strict=True)
m = m.to(DEV)


def ms(x, path, reps):
    m.attention_path = path
    for _ in range(10):
        m(x)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        m(x)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


for B, S in [(16, 32), (16, 64), (16, 80), (32, 48), (64, 32), (100, 32)]:
    x = torch.from_numpy(synthetic_images(1, (B, 3, S, S))).to(DEV)
    rows = B * ((S // 16) ** 2 + 1)
    t = {"auto": [], "fused": []}
    for rnd in range(7):
        for path in ("auto", "fused"):
            t[path].append(ms(x, path, 300))
    med = {k: statistics.median(v) for k, v in t.items()}
    print(f"B={B} {S}x{S} rows={rows}: auto {med['auto']:.4f} ms ({min(t['auto']):.4f}-{max(t['auto']):.4f})  "
          f"fused pin {med['fused']:.4f} ms ({min(t['fused']):.4f}-{max(t['fused']):.4f})  pin/auto {med['fused'] / med['auto']:.3f}", flush=True)
