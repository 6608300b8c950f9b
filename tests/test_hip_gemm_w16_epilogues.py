"""Bit-exact pin of every epilogue of the W16 GEMM (gemm_w16.hip): each tile variant x epilogue x output format, launched
through the C ABI (sm_gemm_w16_tile: sm_gemm_w16 is the same call after sm_gemm_w16_pick, and the pick would send every
shape this small to the 64 x 64 tile), compared with torch.equal against the output the library gave BEFORE the epilogues
became compile-time specialisations (tests/golden/gemm_w16_epilogues/*.npy).  The specialised kernels (the host picks them
for launches without LayerNorm fold, second A operand and split-K), their unguarded interior-tile copy and the generic
kernel of each tile must reproduce those bits: same products, same accumulation order, same expression per element.

Shapes: M = 2 BM + 5 (two interior row tiles - the specialisations' unguarded path - and a ragged third), N = BN + 4 for
fp32 outputs (a ragged column tile) and N = BN for F16X2 outputs (N % 8 == 0), K = 64 (two K-tiles: the ring wraps).
Extras: the 64 x 64 tile with split-K = 2 at K = 128, the consumer and the producer side of the LayerNorm fold, the second A
operand - all on generic kernels - and an out-of-place residual next to the in-place ones (C aliases R, as in the forward).

The expected outputs were written by this file run against a library built from the parent commit's sources:

    SM_HIP_LIB=<parent build>/libselfmask_hip.so python tests/test_hip_gemm_w16_epilogues.py --write-golden [DIR]

(inputs come from seeded CPU generators; only outputs are stored)."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gemm_w16_epilogues")
DEV = "cuda:0"
TILES = {40: (256, 256), 42: (128, 128), 43: (256, 192), 44: (64, 64), 45: (128, 64), 47: (256, 128)}
EPI = {"bias": 0, "gelu": 1, "relu": 2, "residual": 3, "patch": 5}  # SM_EPI_*
PATCH_N = 49


def _cases():
    out = []
    for v in TILES:
        for epi in ("bias", "gelu", "relu"):
            for f16 in (False, True):
                out.append((f"v{v}_{epi}_{'f16x2' if f16 else 'f32'}", dict(variant=v, epi=epi, f16=f16)))
        out.append((f"v{v}_residual_inplace", dict(variant=v, epi="residual", inplace=True)))
        out.append((f"v{v}_patch", dict(variant=v, epi="patch")))
    out.append(("v47_residual_outofplace", dict(variant=47, epi="residual")))
    out.append(("v44_splitk2_k128", dict(variant=44, epi="bias", K=128, split_k=2, bias=False)))
    out.append(("v47_fold_consumer_gelu_f16x2", dict(variant=47, epi="gelu", f16=True, K=384, fold=True)))
    out.append(("v44_fold_producer_residual", dict(variant=44, epi="residual", inplace=True, N=384, producer=True)))
    out.append(("v44_second_operand", dict(variant=44, epi="bias", N=256 + 68, alt_from_n=256)))
    return out


CASES = _cases()


def _rand(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


def _run(name, variant, epi, f16=False, K=64, N=None, inplace=False, split_k=1, bias=True, fold=False, producer=False,
         alt_from_n=0):
    """One launch on seeded inputs; returns {suffix: CPU tensor} of everything the launch wrote."""
    from selfmask_amd import ops
    bm, bn = TILES[variant]
    M = 2 * bm + 5
    N = N or (bn if f16 else bn + 4)
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    a, w = _rand(gen, M, K), _rand(gen, N, K, scale=0.05)
    b = _rand(gen, N).to(DEV) if bias else None
    a_s = ops.split_f16x2(a.to(DEV))
    kw = {}
    w16, ws = ops.split_w16(w.to(DEV))
    if fold:  # consumer side: row statistics (mean, M2) of the twelve 32-column segments and the weight's row sums c (any values do:
        # the bits are what is compared, and ops.fold_layernorm would put torch GPU reductions into the inputs)
        stats = torch.stack([_rand(gen, M, 12, scale=0.3), torch.rand(M, 12, generator=gen) * 40 + 8], 2).contiguous().to(DEV)
        kw.update(ln_stats=stats, ln_c=_rand(gen, N, scale=0.5).to(DEV), ln_eps=1e-6)
    res = {}
    if epi == "residual":
        r = _rand(gen, M, N).to(DEV)
        kw.update(residual=r, out=r if inplace else None)
    if epi == "patch":
        rows = -(-M // PATCH_N) * (PATCH_N + 1)
        kw.update(residual=_rand(gen, PATCH_N + 1, N).to(DEV), patch_n=PATCH_N, out=torch.zeros(rows, N, device=DEV))
    if producer:
        kw.update(xs_out=torch.zeros(M, N, device=DEV), stats_out=torch.zeros(M, 12, 2, device=DEV))
    if alt_from_n:
        kw.update(a_alt=ops.split_f16x2(_rand(gen, M, K).to(DEV)), alt_from_n=alt_from_n)
    c = ops.gemm_w16(a_s, w16, ws, b, epilogue=EPI[epi], variant=variant, out_f16x2=f16, split_k=split_k, **kw)
    torch.cuda.synchronize()
    res["c"] = c.cpu()
    if producer:
        res["xs"], res["stats"] = kw["xs_out"].cpu(), kw["stats_out"].cpu()
    return res


@pytest.mark.parametrize("name,case", CASES, ids=[n for n, _ in CASES])
def test_epilogue_bits(name, case):
    got = _run(name, **case)
    for key, t in got.items():
        want = torch.from_numpy(np.load(os.path.join(GOLDEN, f"{name}.{key}.npy")))
        assert t.shape == want.shape and t.dtype == want.dtype
        # compared as bit patterns: F16X2 outputs are f16 pairs viewed as fp32, where a NaN pattern would defeat a float compare
        assert torch.equal(t.contiguous().view(torch.int32), want.view(torch.int32)), \
            f"{name}.{key}: {(t.contiguous().view(torch.int32) != want.view(torch.int32)).sum().item()} of {t.numel()} words differ"


if __name__ == "__main__":
    sys.path[:0] = [os.path.join(HERE, "..", "salient-object-detection_amd"), os.path.join(HERE, "..")]
    assert "--write-golden" in sys.argv, __doc__
    dst = sys.argv[sys.argv.index("--write-golden") + 1] if sys.argv[-1] != "--write-golden" else GOLDEN
    os.makedirs(dst, exist_ok=True)
    for name, case in CASES:
        for key, t in _run(name, **case).items():
            np.save(os.path.join(dst, f"{name}.{key}.npy"), t.contiguous().numpy())
    print(f"wrote {len(CASES)} cases to {dst} with {os.environ.get('SM_HIP_LIB', 'the default library')}")
