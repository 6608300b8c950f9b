"""The references of _kernel_refs.py (what the GPU tests of the forward's glue kernels expect) witnessed on the CPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _kernel_refs as R


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


GRIDS = [(14, 14), (16, 21), (25, 21), (1, 1), (1, 7), (3, 1), (9, 11)]


@pytest.mark.parametrize("gh,gw", GRIDS)
@pytest.mark.parametrize("sf", [1, 2, 4])
def test_bilinear_ref_matches_torch_fp64_at_exact_scales(sf, gh, gw):
    """1 / sf is a power of two: the fp32 coordinates are exact, so the reference and torch's fp64 interpolation use the same
    weights and differ by the rounding of the fp64 blend alone."""
    x = _rand(3, 5, gh, gw, seed=1, scale=4.0)
    want = F.interpolate(x.double(), scale_factor=sf, mode="bilinear")
    got = R.bilinear_ref(x, sf)
    assert got.shape == want.shape and got.dtype == torch.float64
    assert (got - want).abs().max().item() <= 1e-12
    if sf == 1:
        assert torch.equal(got, x.double())


@pytest.mark.parametrize("gh,gw", GRIDS)
@pytest.mark.parametrize("sf", [3, 8, 16])
def test_bilinear_ref_matches_torch_fp32_weights(sf, gh, gw):
    """sf = 3: fl32(1/3) is not 1/3, and the fp32 coordinate arithmetic rounds.  The reference must carry torch's fp32 weights,
    so it differs from torch's fp32 result by the rounding of the fp32 blend alone (two weights 1 - w, four products, three
    sums: under 8 roundings of values <= max|x|); an exact-1/3 reference would be ~1e-6 max|x| away at the far edge."""
    ramp = torch.arange(gw, dtype=torch.float32).reshape(1, 1, 1, gw)
    i0, i1, w = R.bilinear_taps(gw, sf)
    assert torch.equal(F.interpolate(ramp, scale_factor=(1, sf), mode="bilinear")[0, 0, 0].double(),
                       i0.double() * (1 - w) + i1.double() * w)  # torch's own coordinates, read off a ramp: the same bits
    x = _rand(2, 4, gh, gw, seed=2, scale=4.0)
    want = F.interpolate(x, scale_factor=sf, mode="bilinear")
    got = R.bilinear_ref(x, sf)
    assert got.shape == want.shape
    assert (got - want.double()).abs().max().item() <= 8 * 2.0 ** -24 * x.abs().max().item()


def test_bilinear_taps_unfused_form_is_not_torch():
    """Why the coordinate is one fused multiply-add: with the product rounded first, column 48 of 63 (gw = 21, sf = 3) sits an
    ulp of 16 (9.5e-7) away from where torch puts it; for power-of-two scales the two forms agree exactly."""
    ramp = torch.arange(21, dtype=torch.float32).reshape(1, 1, 1, 21)
    want = F.interpolate(ramp, scale_factor=(1, 3), mode="bilinear")[0, 0, 0].double()
    i0, i1, w = R.bilinear_taps(21, 3, fused=False)
    d = (i0.double() * (1 - w) + i1.double() * w - want).abs()
    assert 0 < d.max().item() <= 2.0 ** -20
    for sf in (1, 2, 4, 8, 16):
        for a, b in zip(R.bilinear_taps(21, sf), R.bilinear_taps(21, sf, fused=False)):
            assert torch.equal(a, b)


def test_bilinear_taps_edges():
    for size, sf in [(1, 3), (7, 2), (5, 16), (14, 3)]:
        i0, i1, w1 = R.bilinear_taps(size, sf)
        assert len(i0) == sf * size and int(i0.min()) == 0 and int(i1.max()) == size - 1
        assert bool(((i1 == i0 + 1) | (i0 == size - 1)).all()) and bool(((w1 >= 0) & (w1 < 1)).all())
        assert float(w1[0]) == 0.0  # the clamp at 0: the first output sits on the first sample
    # sf = 2: the classic 0.25 / 0.75 weights
    _, _, w = R.bilinear_taps(4, 2)
    assert w.tolist() == [0.0, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0.25]


def test_partial_sum_order_against_a_plain_loop():
    S, rows = 4, 7
    parts, bias, res = _rand(S, rows, 24, seed=3, scale=30.0), _rand(24, seed=4), _rand(rows, 24, seed=5, scale=1e-3)
    got = R.partial_sum_f32(parts, bias, res)
    pn, bn, rn = parts.numpy(), bias.numpy(), res.numpy()
    for r in range(rows):
        for c in range(24):
            v = np.float32(pn[0, r, c])
            for s in range(1, S):
                v = np.float32(v + pn[s, r, c])
            v = np.float32(np.float32(v + bn[c]) + rn[r, c])
            assert got[r, c].item() == float(v)
    assert got.dtype == torch.float32
    # the order matters at this spread of magnitudes: summing the other way round gives other bits somewhere
    other = (res + bias[None, :]) + (parts[3] + parts[2] + parts[1] + parts[0])
    assert not torch.equal(other, got)


def test_split_bits_follow_the_definition():
    """Element by element, with Python scalars, on the values test_split_bits_match_the_definition feeds the kernel."""
    x = torch.cat([_rand(2, 16, seed=6, scale=s) for s in (1e-6, 1e-3, 1.0, 30.0, 3000.0)])
    x[0, :8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 65504.0 / 2, 2.0 ** -14, 2.0 ** -24, 1.0 + 2.0 ** -11])
    bits = R.split_bits(x)
    assert bits.shape == (10, 2, 2, 8) and bits.dtype == np.uint16
    xn = x.numpy()
    for r in range(xn.shape[0]):
        for k in range(xn.shape[1]):
            hi = np.float16(xn[r, k])
            lo = np.float16(np.float32(np.float32(xn[r, k] - np.float32(hi)) * np.float32(2048.0)))
            assert bits[r, k // 8, 0, k % 8] == hi.view(np.uint16) and bits[r, k // 8, 1, k % 8] == lo.view(np.uint16)
    # layout: a container built from those bits reads back as the values, to the format's precision
    cont = torch.from_numpy(bits.reshape(10, -1).view(np.float32).copy())
    assert cont.shape == x.shape
    assert np.array_equal(R.container_bits(cont), bits)
    back = R.unsplit(cont)
    assert bool(((back - x.double()).abs() <= R.F16X2_REL * x.double().abs() + 2.0 ** -35).all())  # 2^-35: lo's f16 subnormal step / 2^11
    assert bits[0, 0, 0, 1] == 0x8000  # -0.0 keeps its sign in hi


def test_map_rows():
    assert R.map_rows(5, (0, 0, 0)).tolist() == [0, 1, 2, 3, 4]
    assert R.map_rows(6, (3, 4, 1)).tolist() == [1, 2, 3, 5, 6, 7]          # drop row 0 of groups of 4
    assert R.map_rows(4, (2, 6, 2)).tolist() == [2, 3, 8, 9]                # layer 1 of 3, nq = 2
    t = _rand(2, 5, 8, seed=7)
    assert torch.equal(R.planes_to_tokens(R.tokens_to_planes(t.reshape(2, 5, 8), 5, 1)), t)
