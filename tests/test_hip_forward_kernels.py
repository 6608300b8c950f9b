"""Direct parity of the kernels BETWEEN the forward's GEMMs and attention: every option of the LayerNorm launch, the F16X2
outputs of the attention kernels, the up-samplers of the mask head and the small producers (im2col, cls rows, query mean,
broadcast), each through the C ABI against a plain fp64 reference (_kernel_refs.py, witnessed by test_kernel_refs_cpu.py).

Two contracts run through the file:
  * an F16X2 output IS split(fp32 value), bit for bit - compared as integers against sm_split_f16x2 of the fp32 output;
  * an output buffer is pre-filled with NaN: what a kernel must not write keeps the fill, what it must write is finite.
Bounds are those of the existing test of the same arithmetic (test_hip_ops.py), derived from the number formats, or
"3 x torch-fp32's own error against fp64 + a floor"; none is fitted to what the kernels return.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import _kernel_refs as R  # noqa: E402
import _ledger  # noqa: E402
from selfmask_amd import _native as N  # noqa: E402
from selfmask_amd import ops  # noqa: E402

DEV = "cuda:0"
D = 384
NAN_BITS = 0x7FC00000  # torch.full(..., nan) in fp32


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def _maxerr(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().max().item()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def _untouched(t) -> bool:
    """every element still holds the NaN fill, bit for bit"""
    return t.numel() == 0 or bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


def _same_bits(a, b) -> bool:
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _is_split_of(container, value) -> bool:
    """container (F16X2) == sm_split_f16x2(value) as integers, and == the numpy definition of the format when small"""
    ok = _same_bits(container, ops.split_f16x2(value.contiguous()))
    if ok and value.numel() <= 1 << 18:
        ok = np.array_equal(R.container_bits(container), R.split_bits(value))
    return ok


def _p(t):
    return None if t is None else t.data_ptr()


# ===== 1. LayerNorm launch ===================================================================================================
def _ln(x, gamma, beta, eps, rows, *, ldx=D, in_map=(0, 0, 0), y=None, ys=None, ldy=D, out_map=(0, 0, 0), y2=None, ldy2=D,
        add=None, add_rows=None, y2_f16x2=False, parts=0, partial_stride=0, pre_bias=None, residual=None, raw=None,
        chain=None, x_ptr=None):
    """One sm_layernorm_rows_f32 launch, every field of sm_ln_args reachable; tensors are device tensors (or None)."""
    a = N.LnArgs()
    a.x, a.ldx, a.in_map = (x.data_ptr() if x_ptr is None else x_ptr), ldx, N.RowMap(*in_map)
    a.gamma, a.beta = _p(gamma), _p(beta)
    a.y, a.ys, a.ldy, a.out_map = _p(y), _p(ys), ldy, N.RowMap(*out_map)
    a.y2, a.ldy2, a.add, a.y2_f16x2 = _p(y2), ldy2, _p(add), 1 if y2_f16x2 else 0
    a.add_rows = (add.shape[0] if add is not None else 0) if add_rows is None else add_rows
    a.rows, a.eps = rows, eps
    a.n_partials, a.partial_stride, a.pre_bias, a.residual, a.raw = parts, partial_stride, _p(pre_bias), _p(residual), _p(raw)
    if chain is not None:
        a.chain_gamma, a.chain_beta, a.chain_eps = _p(chain["gamma"]), _p(chain.get("beta")), chain["eps"]
        a.chain_y, a.chain_ys, a.chain_ldy = _p(chain.get("y")), _p(chain.get("ys")), chain.get("ldy", D)
        a.chain_map = N.RowMap(*chain.get("map", (0, 0, 0)))
    N.check(N.load().sm_layernorm_rows_f32(a, _stream()), "sm_layernorm_rows_f32")


def _affine(seed):
    return 1 + 0.1 * _rand(D, seed=seed), 0.1 * _rand(D, seed=seed + 1)


def _ln_tol(y, ref, x32_for_torch, g, b, eps, scale=1.0, fmt=0.0):
    """The rule of test_layernorm: 2e-6 absolute AND 3 x torch-fp32's own error + 5e-7, at the input's scale (`scale` = 1 for
    normalised values of order one); `fmt` adds the F16X2 format's relative term.  Returns (err, err_torch, bound)."""
    err = _maxerr(y, ref)
    err_t = _maxerr(F.layer_norm(x32_for_torch, (D,), g, b, eps), ref)
    bound = min(2e-6 * scale, 3 * err_t + 5e-7 * scale) + fmt * ref.abs().max().item()
    return err, err_t, bound


@pytest.mark.parametrize("rows", [1, 3, 4, 5, 15, 16, 17, 394, 1283])
def test_layernorm_f16x2_output(rows):
    """ys alone (y == NULL: every LayerNorm of the default W16 mode), and y + ys in one launch.  The row counts give every fill
    of the last 4-row wave and of the last 16-row block."""
    eps = 1e-6 if rows % 2 else 1e-5
    x, (g, b) = _rand(rows, D, seed=100 + rows, scale=3.0) + 0.7, _affine(21)
    xd, gd, bd = x.to(DEV), g.to(DEV), b.to(DEV)
    pad = 3
    ys_only, y, ys = _nan(rows + pad, D), _nan(rows + pad, D), _nan(rows + pad, D)
    _ln(xd, gd, bd, eps, rows, ys=ys_only)
    _ln(xd, gd, bd, eps, rows, y=y, ys=ys)
    assert _untouched(ys_only[rows:]) and _untouched(y[rows:]) and _untouched(ys[rows:])
    assert bool(torch.isfinite(y[:rows]).all())
    assert _is_split_of(ys[:rows], y[:rows])
    assert _same_bits(ys_only[:rows], ys[:rows])
    ref = R.layernorm_ref(x, g, b, eps)
    err, err_t, bound = _ln_tol(R.unsplit(ys_only[:rows]), ref, x, g, b, eps, fmt=R.F16X2_REL)
    _ledger.record("forward_kernels", f"layernorm_ys_only[{rows}]", {"err_vs_fp64": err, "torch_fp32_err": err_t, "bound": bound})
    assert err <= bound
    err, err_t, bound = _ln_tol(y[:rows], ref, x, g, b, eps)
    assert err <= bound


def test_layernorm_f16x2_edge_rows():
    """Rows whose normalised values reach the corners of the split: one 3000x outlier (values near sqrt(383) next to values
    near -0.05), a row at the 1e-6 scale (variance far under eps: outputs of 1e-3, lo halves in the f16 subnormals), and
    constant rows.  The constants are 1.0 and -2.5 on purpose: every partial sum of the kernel's reduction is then an exact
    fp32 number and 384 c * fl(1/384) = c (1 + 2^-25) rounds back to c, so the mean is exact, every deviation is exactly 0
    and the output must be beta itself, whatever the order of the reduction."""
    eps = 1e-6
    x, (g, b) = _rand(6, D, seed=130, scale=3.0) + 0.7, _affine(23)
    x[0, 77] = 3000.0 * 3.0
    x[1] = _rand(D, seed=131, scale=1e-6)
    x[2] = 1.0
    x[3] = -2.5
    x[4, :] = 0.0
    xd, gd, bd = x.to(DEV), g.to(DEV), b.to(DEV)
    y, ys, ys_only = _nan(6, D), _nan(6, D), _nan(6, D)
    _ln(xd, gd, bd, eps, 6, y=y, ys=ys)
    _ln(xd, gd, bd, eps, 6, ys=ys_only)
    assert bool(torch.isfinite(y).all())
    assert _is_split_of(ys, y) and _same_bits(ys_only, ys)
    for r in (2, 3, 4):
        assert torch.equal(y[r].cpu(), b), r
    ref = R.layernorm_ref(x, g, b, eps)
    for r in range(6):  # per row, at the row's own output scale (the outlier row reaches ~20)
        scale = max(1.0, ref[r].abs().max().item())
        err, err_t, bound = _ln_tol(y[r:r + 1], ref[r:r + 1], x[r:r + 1], g, b, eps, scale=scale)
        _ledger.record("forward_kernels", f"layernorm_edge_row[{r}]", {"err_vs_fp64": err, "torch_fp32_err": err_t, "bound": bound})
        assert err <= bound, (r, err, bound)
        assert _maxerr(R.unsplit(ys[r:r + 1]), ref[r:r + 1]) <= bound + R.F16X2_REL * scale


@pytest.mark.parametrize("add_rows", [1, 20, 47])
def test_layernorm_y2_is_indexed_by_the_logical_row(add_rows):
    """y2[r] = y[r] + add[r % add_rows] with a NON-identity out_map: y / ys land on the mapped row, y2 and the add row follow the
    logical row (47 rows: not a multiple of 20).  One fp32 add of the stored y, so y2 is checked bit for bit."""
    rows, omap = 47, (5, 9, 2)
    orows = int(R.map_rows(rows, omap).max()) + 4
    x, (g, b), add = _rand(rows, D, seed=140), _affine(25), _rand(add_rows, D, seed=141)
    xd, gd, bd, addd = x.to(DEV), g.to(DEV), b.to(DEV), add.to(DEV)
    y, ys, y2, y2s = _nan(orows, D), _nan(orows, D), _nan(rows + 2, D), _nan(rows + 2, D)
    _ln(xd, gd, bd, 1e-5, rows, y=y, ys=ys, out_map=omap, y2=y2, add=addd)
    _ln(xd, gd, bd, 1e-5, rows, ys=_nan(orows, D), out_map=omap, y2=y2s, add=addd, y2_f16x2=True)
    idx = R.map_rows(rows, omap)
    hole = torch.ones(orows, dtype=torch.bool)
    hole[idx] = False
    assert _untouched(y[hole.to(DEV)]) and _untouched(ys[hole.to(DEV)]) and _untouched(y2[rows:]) and _untouched(y2s[rows:])
    ym = y[idx.to(DEV)]
    ref = R.layernorm_ref(x, g, b, 1e-5)
    assert _maxerr(ym, ref) <= 2e-6
    assert _is_split_of(ys[idx.to(DEV)], ym)
    want_y2 = ym.cpu() + add[torch.arange(rows) % add_rows]  # fp32, one rounding
    assert torch.equal(y2[:rows].cpu(), want_y2)
    assert _maxerr(y2[:rows], ref + add[torch.arange(rows) % add_rows].double()) <= 2e-6
    assert _is_split_of(y2s[:rows], y2[:rows])


@pytest.mark.parametrize("B,n", [(3, 4), (2, 196), (3, 99)])
def test_layernorm_in_map_with_f16x2_output(B, n):
    """The encoder's final norm: drop the cls row of every image (groups of n out of n + 1) and write TOK and TOKs."""
    rows = B * n
    x, (g, b) = _rand(B * (n + 1), D, seed=150 + n, scale=2.0), _affine(27)
    xd, gd, bd = x.to(DEV), g.to(DEV), b.to(DEV)
    y, ys, ys_only = _nan(rows + 1, D), _nan(rows + 1, D), _nan(rows + 1, D)
    _ln(xd, gd, bd, 1e-6, rows, in_map=(n, n + 1, 1), y=y, ys=ys)
    _ln(xd, gd, bd, 1e-6, rows, in_map=(n, n + 1, 1), ys=ys_only)
    assert _untouched(y[rows:]) and _untouched(ys[rows:]) and _untouched(ys_only[rows:])
    xin = x.view(B, n + 1, D)[:, 1:].reshape(rows, D)
    ref = R.layernorm_ref(xin, g, b, 1e-6)
    err, err_t, bound = _ln_tol(y[:rows], ref, xin, g, b, 1e-6)
    _ledger.record("forward_kernels", f"layernorm_in_map[{B}x{n}]", {"err_vs_fp64": err, "torch_fp32_err": err_t, "bound": bound})
    assert err <= bound
    assert _is_split_of(ys[:rows], y[:rows]) and _same_bits(ys_only, ys)


def _chain_bound(ref1, g2):
    """LN(LN(x)) against fp64: the first norm's 2e-6 reaches the second norm's output times its gain |gamma2| / std(y) (y is the
    first norm's output, std taken per row), and the second norm adds its own 2e-6."""
    gain = g2.abs().max().item() / ref1.std(dim=1, unbiased=False).min().item()
    return 2e-6 * (1.0 + gain)


@pytest.mark.parametrize("variant", ["all", "chain_ys_only", "no_y"])
def test_layernorm_chained_norm_is_a_launch_of_its_own(variant):
    """chain_y / chain_ys against a SEPARATE launch on the stored y with (chain_gamma, chain_beta, chain_eps): same bits, as the
    header promises.  eps differs from chain_eps, the affine pairs differ, the chain scatters layer l of L."""
    Bq, nq, L, l = 3, 7, 4, 2
    rows, cmap = Bq * nq, (nq, L * nq, l * nq)
    x, (g, b), (g2, b2) = _rand(rows, D, seed=160, scale=2.0) + 0.3, _affine(29), _affine(31)
    g2 = g2 * 1.3
    eps, ceps = 1e-5, 1e-6
    xd, gd, bd, g2d, b2d = (t.to(DEV) for t in (x, g, b, g2, b2))
    y, ys, cy, cys = _nan(rows, D), _nan(rows, D), _nan(Bq * L * nq, D), _nan(Bq * L * nq, D)
    if variant == "all":
        _ln(xd, gd, bd, eps, rows, y=y, ys=ys, chain=dict(gamma=g2d, beta=b2d, eps=ceps, y=cy, ys=cys, map=cmap))
    elif variant == "chain_ys_only":
        _ln(xd, gd, bd, eps, rows, y=y, chain=dict(gamma=g2d, beta=b2d, eps=ceps, ys=cys, map=cmap))
    else:
        _ln(xd, gd, bd, eps, rows, ys=ys, chain=dict(gamma=g2d, beta=b2d, eps=ceps, y=cy, ys=cys, map=cmap))
    # the first norm, from a launch without a chain: the stored y the chain must have normalised
    y1, ys1 = _nan(rows, D), _nan(rows, D)
    _ln(xd, gd, bd, eps, rows, y=y1, ys=ys1)
    if variant != "no_y":
        assert _same_bits(y, y1)
    if variant != "chain_ys_only":
        assert _same_bits(ys, ys1)
    sy, sys_ = _nan(Bq * L * nq, D), _nan(Bq * L * nq, D)
    _ln(y1, g2d, b2d, ceps, rows, y=sy, ys=sys_, out_map=cmap)
    layer = cy.view(Bq, L, nq, D) if variant != "chain_ys_only" else None
    if layer is not None:
        assert _same_bits(cy, sy)  # NaN fill included: the other layers' rows are untouched in both
        assert _untouched(layer[:, :l]) and _untouched(layer[:, l + 1:]) and bool(torch.isfinite(layer[:, l]).all())
    else:
        assert _untouched(cy)
    assert _same_bits(cys, sys_)
    lys = cys.view(Bq, L, nq, D)
    assert _untouched(lys[:, :l]) and _untouched(lys[:, l + 1:])
    assert _is_split_of(lys[:, l].reshape(rows, D), sy.view(Bq, L, nq, D)[:, l].reshape(rows, D))
    ref1 = R.layernorm_ref(x, g, b, eps)
    ref2 = R.layernorm_ref(ref1, g2, b2, ceps)
    got = R.unsplit(lys[:, l].reshape(rows, D))
    err, bound = _maxerr(got, ref2), _chain_bound(ref1, g2) + R.F16X2_REL * ref2.abs().max().item()
    err_t = _maxerr(F.layer_norm(F.layer_norm(x, (D,), g, b, eps), (D,), g2, b2, ceps), ref2)
    _ledger.record("forward_kernels", f"layernorm_chain[{variant}]", {"err_vs_fp64": err, "torch_fp32_err": err_t, "bound": bound})
    assert err <= bound
    # chain_eps, not eps: with eps in its place the result moves by ~ (eps - chain_eps) / 2 * |y|, far above the bound
    wrong = R.layernorm_ref(ref1, g2, b2, eps)
    assert (wrong - ref2).abs().max().item() > bound


@pytest.mark.parametrize("B,nq", [(1, 20), (3, 20), (7, 5), (100, 3)])
def test_layernorm_decoder_norm3_everything_at_once(B, nq):
    """What the decoder's norm3 launch sets, together: four split-K slices + pre_bias + residual, y, ys, y2 in F16X2 with
    add_rows = nq, the chained shared norm scattered into (B, L, nq, 384) - plus `raw`, to see the reduced sum itself."""
    rows, L, l = B * nq, 3, 1
    cmap = (nq, L * nq, l * nq)
    parts, bias, res = _rand(4, rows, D, seed=170 + B, scale=1.0), _rand(D, seed=171, scale=0.3), _rand(rows, D, seed=172)
    (g, b), (g2, b2), qpos = _affine(33), _affine(35), _rand(nq, D, seed=173)
    pd, biasd, resd, gd, bd, g2d, b2d, qd = (t.to(DEV) for t in (parts, bias, res, g, b, g2, b2, qpos))
    res_before = resd.clone()
    y, ys, y2s, raw = _nan(rows + 1, D), _nan(rows + 1, D), _nan(rows + 1, D), _nan(rows + 1, D)
    cy, cys = _nan(B * L * nq, D), _nan(B * L * nq, D)
    _ln(pd, gd, bd, 1e-5, rows, y=y, ys=ys, y2=y2s, add=qd, y2_f16x2=True, parts=4, partial_stride=rows * D, pre_bias=biasd,
        residual=resd, raw=raw, chain=dict(gamma=g2d, beta=b2d, eps=1e-6, y=cy, ys=cys, map=cmap))
    for t in (y, ys, y2s, raw):
        assert _untouched(t[rows:])
    assert _same_bits(resd, res_before)
    want_raw = R.partial_sum_f32(parts, bias, res)
    assert torch.equal(raw[:rows].cpu(), want_raw)  # slices in order, then the bias, then the residual: bit for bit
    x64 = parts.double().sum(0) + bias.double() + res.double()
    assert _maxerr(raw[:rows], x64) <= 5 * 2.0 ** -24 * (parts.abs().sum(0) + bias.abs() + res.abs()).max().item()  # 5 roundings
    ref = R.layernorm_ref(x64, g, b, 1e-5)
    err, err_t, bound = _ln_tol(y[:rows], ref, want_raw, g, b, 1e-5)
    _ledger.record("forward_kernels", f"layernorm_norm3[{B}x{nq}]", {"err_vs_fp64": err, "torch_fp32_err": err_t, "bound": bound})
    assert err <= bound
    assert _is_split_of(ys[:rows], y[:rows])
    assert _is_split_of(y2s[:rows], (y[:rows].cpu() + qpos.repeat(B, 1)).to(DEV))
    # the chain: a launch of its own on the stored y
    sy, sys_ = _nan(B * L * nq, D), _nan(B * L * nq, D)
    _ln(y, g2d, b2d, 1e-6, rows, y=sy, ys=sys_, out_map=cmap)
    assert _same_bits(cy, sy) and _same_bits(cys, sys_)
    layer = cy.view(B, L, nq, D)
    assert _untouched(layer[:, :l]) and _untouched(layer[:, l + 1:]) and bool(torch.isfinite(layer[:, l]).all())
    ref2 = R.layernorm_ref(ref, g2, b2, 1e-6)
    assert _maxerr(layer[:, l].reshape(rows, D), ref2) <= _chain_bound(ref, g2)


def test_layernorm_encoder_split_fc2_form():
    """The encoder's split-fc2 launch: raw ALIASES residual (the stream is updated in place), ys only."""
    rows = 394
    parts, bias, res = _rand(4, rows, D, seed=180, scale=1.5), _rand(D, seed=181, scale=0.3), _rand(rows, D, seed=182, scale=2.0)
    g, b = _affine(37)
    pd, biasd, stream, gd, bd = (t.to(DEV) for t in (parts, bias, res, g, b))
    ys = _nan(rows + 1, D)
    _ln(pd, gd, bd, 1e-6, rows, ys=ys, parts=4, partial_stride=rows * D, pre_bias=biasd, residual=stream, raw=stream)
    want_raw = R.partial_sum_f32(parts, bias, res)
    assert torch.equal(stream.cpu(), want_raw)
    assert _untouched(ys[rows:])
    x64 = parts.double().sum(0) + bias.double() + res.double()
    ref = R.layernorm_ref(x64, g, b, 1e-6)
    err, err_t, bound = _ln_tol(R.unsplit(ys[:rows]), ref, want_raw, g, b, 1e-6, fmt=R.F16X2_REL)
    _ledger.record("forward_kernels", "layernorm_split_fc2", {"err_vs_fp64": err, "torch_fp32_err": err_t, "bound": bound})
    assert err <= bound
    # and the same bits as a plain launch on the reduced stream
    ys2 = _nan(rows, D)
    _ln(stream, gd, bd, 1e-6, rows, ys=ys2)
    assert _same_bits(ys[:rows], ys2)


def test_layernorm_argument_checks():
    x, (g, b) = _rand(8, 2 * D, seed=190).to(DEV), _affine(39)
    gd, bd = g.to(DEV), b.to(DEV)
    y, ys = _nan(8, 2 * D), _nan(8, 2 * D)
    with pytest.raises(RuntimeError, match="F16X2 outputs need ld"):
        _ln(x, gd, bd, 1e-6, 8, ldx=2 * D, ys=ys, ldy=D + 4)
    with pytest.raises(RuntimeError, match="bad y2/add"):
        _ln(x, gd, bd, 1e-6, 8, ldx=2 * D, y=y, ldy=2 * D, y2=ys)
    with pytest.raises(RuntimeError, match="bad chained norm"):
        _ln(x, gd, bd, 1e-6, 8, ldx=2 * D, y=y, ldy=2 * D, chain=dict(gamma=gd, beta=bd, eps=1e-6))
    with pytest.raises(RuntimeError, match="16-B aligned"):
        _ln(x, gd, bd, 1e-6, 8, ldx=2 * D, y=y, ldy=2 * D, x_ptr=x.data_ptr() + 4)
    with pytest.raises(RuntimeError, match="bad partials"):
        _ln(x, gd, bd, 1e-6, 8, ldx=2 * D, y=y, ldy=2 * D, parts=2, partial_stride=4 * D, pre_bias=bd)
    with pytest.raises(RuntimeError, match="null pointer"):
        _ln(x, gd, bd, 1e-6, 8, ldx=2 * D)
    torch.cuda.synchronize()
    assert _untouched(y) and _untouched(ys)  # a refused launch writes nothing
    _ln(x, gd, bd, 1e-6, 0, ldx=2 * D, y=y, ys=ys, ldy=2 * D)  # rows = 0: OK, nothing written
    torch.cuda.synchronize()
    assert _untouched(y) and _untouched(ys)


# ===== 2. attention: F16X2 output, the cross-attention K/V layout ================================================================
def _attn(split, q, k, v, o, B, nq, nk, sQb, sQr, sKb, sKr, sOb, sOr, out_f16x2):
    a = N.AttnArgs()
    a.Q, a.K, a.V, a.O = q, k, v, o.data_ptr()
    a.sQb, a.sQr, a.sKb, a.sKr, a.sVb, a.sVr, a.sOb, a.sOr = sQb, sQr, sKb, sKr, sKb, sKr, sOb, sOr
    a.batch, a.heads, a.n_q, a.n_k, a.scale, a.out_f16x2 = B, 6, nq, nk, 0.125, 1 if out_f16x2 else 0
    fn = N.load().sm_attention_f16x2 if split else N.load().sm_attention_f32
    N.check(fn(a, _stream()), "sm_attention")


def _attn_ref(q, k, v, scale):
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * scale
    return torch.einsum("bhqk,bkhd->bqhd", s.softmax(-1), v.double()).reshape(q.shape[0], q.shape[1], -1)


@pytest.mark.parametrize("B,nq,nk,ldo", [(2, 197, 197, 384), (1, 577, 577, 384), (3, 20, 20, 384), (3, 20, 196, 384),
                                          (2, 33, 225, 384), (1, 1, 1, 384), (3, 20, 196, 512), (2, 197, 197, 512)])
@pytest.mark.parametrize("split", [False, True], ids=["f32", "f16x2"])
def test_attention_f16x2_output(split, B, nq, nk, ldo):
    """out_f16x2 = 1 of both attention kernels, K / V read as strided views of a (B, n, L * 768) buffer at layer l (the
    forward's all-layer K/V tensor).  Both kernels scale one register value and either store it or split it (attention.hip:
    `w` -> store_f16x2_4; attention_f16x2.hip: `x`, `y` -> store_f16x2_8 after a lane swap that moves whole values), so the
    F16X2 output must be split(fp32 output of the same kernel), bit for bit.  ldo = 512: the output lands in a wider buffer
    and the gap keeps its fill."""
    L, l = 2, 1
    KVW = L * 768
    q, kv = _rand(B, nq, D, seed=200, scale=1.5), _rand(B, nk, KVW, seed=201, scale=1.5)
    qd, kvd = q.to(DEV), kv.to(DEV)
    if split:  # F16X2 images of the rows: 768 l and 384 are multiples of 8, so a slice of the split row is the split of the slice
        qd, kvd = ops.split_f16x2(qd), ops.split_f16x2(kvd)
    kp, vp = kvd.data_ptr() + 4 * (l * 768), kvd.data_ptr() + 4 * (l * 768 + D)
    o32, o16 = _nan(B, nq + 1, ldo), _nan(B, nq + 1, ldo)
    for o, f in ((o32, False), (o16, True)):
        _attn(split, qd.data_ptr(), kp, vp, o, B, nq, nk, nq * D, D, nk * KVW, KVW, (nq + 1) * ldo, ldo, f)
    for o in (o32, o16):
        assert _untouched(o[:, nq:]) and _untouched(o[:, :, D:])
    got32 = o32[:, :nq, :D].contiguous()
    assert bool(torch.isfinite(got32).all())
    assert _is_split_of(o16[:, :nq, :D].contiguous(), got32)
    k4, v4 = kv[:, :, l * 768:l * 768 + D].reshape(B, nk, 6, 64), kv[:, :, l * 768 + D:(l + 1) * 768].reshape(B, nk, 6, 64)
    q4 = q.reshape(B, nq, 6, 64)
    ref = _attn_ref(q4, k4, v4, 0.125)
    ref32 = F.scaled_dot_product_attention(q4.transpose(1, 2), k4.transpose(1, 2), v4.transpose(1, 2),
                                           scale=0.125).transpose(1, 2).reshape(B, nq, -1)
    err, err_t = _maxerr(R.unsplit(o16[:, :nq, :D]), ref), _maxerr(ref32, ref)
    bound = max(1e-5, 3 * err_t) + R.F16X2_REL * ref.abs().max().item()  # the rule of test_attention_shapes + the format
    _ledger.record("forward_kernels", f"attention_out_f16x2[{'f16x2' if split else 'f32'}-{B}x{nq}x{nk}-ld{ldo}]",
                   {"err_vs_fp64": err, "torch_fp32_err": err_t, "bound": bound})
    assert err <= bound
    assert _maxerr(got32, ref) <= max(1e-5, 3 * err_t)


# ===== 3. up-samplers ========================================================================================================
def _up_logits(low, planes, gh, gw, sf, want_logits=True, alias2x=False):
    """-> (logits or None, prob), each with one extra plane that must keep the fill"""
    opix = sf * sf * gh * gw
    logits = _nan(planes + 1, opix) if want_logits else None
    prob = _nan(planes + 1, opix)
    if alias2x:
        assert sf == 2
        rc = N.load().sm_upsample2x_logits_sigmoid_f32(low.data_ptr(), _p(logits), prob.data_ptr(), planes, gh, gw, _stream())
    else:
        rc = N.load().sm_upsample_logits_sigmoid_f32(low.data_ptr(), _p(logits), prob.data_ptr(), planes, gh, gw, sf, _stream())
    N.check(rc, "sm_upsample_logits_sigmoid_f32")
    assert _untouched(prob[planes:]) and (logits is None or _untouched(logits[planes:]))
    return (None if logits is None else logits[:planes]), prob[:planes]


def _logits_input(planes, gh, gw, seed):
    g = torch.Generator().manual_seed(seed)
    low = (torch.rand(planes, gh, gw, generator=g) * 120.0 - 60.0).float()  # both saturating tails of the sigmoid
    flat = low.view(-1)
    flat[0] = 60.0
    if flat.numel() > 1:
        flat[-1] = -60.0
    return low


def _check_logits_case(planes, gh, gw, sf, seed):
    low = _logits_input(planes, gh, gw, seed)
    lowd = low.to(DEV)
    logits, prob = _up_logits(lowd, planes, gh, gw, sf)
    _, prob_only = _up_logits(lowd, planes, gh, gw, sf, want_logits=False)
    assert _same_bits(prob_only, prob)  # the logits == NULL branch
    if sf == 2:
        l2, p2 = _up_logits(lowd, planes, gh, gw, 2, alias2x=True)
        assert _same_bits(l2, logits) and _same_bits(p2, prob)
    lg = logits.cpu().view(planes, sf * gh, sf * gw)
    if sf == 1:
        assert torch.equal(lg, low)
    ref = R.bilinear_ref(low, sf)
    ref32 = F.interpolate(low[None], scale_factor=sf, mode="bilinear")[0]
    err, err_t = _maxerr(lg, ref), _maxerr(ref32, ref)
    bound = 3 * err_t + 1e-6 * low.abs().max().item()
    _ledger.record("forward_kernels", f"upsample_logits[{planes}x{gh}x{gw}-sf{sf}]", {"err_vs_fp64": err, "torch_fp32_err": err_t, "bound": bound})
    assert err <= bound, (err, bound)
    pr = prob.cpu().view(-1)
    assert bool(torch.isfinite(pr).all()) and pr.min().item() >= 0.0 and pr.max().item() <= 1.0
    assert _maxerr(pr, torch.sigmoid(lg.double().view(-1))) <= 2e-6  # the bound of test_gemm_epilogues for the same expf form
    order = torch.argsort(lg.reshape(-1))
    assert bool((pr[order][1:] >= pr[order][:-1]).all())  # monotone with the kernel's own logit
    assert pr.max().item() > 1 - 1e-6 and (low.numel() == 1 or pr.min().item() < 1e-6)  # both tails were reached


SFS = [1, 2, 3, 4, 8, 16]
LOGIT_GRIDS = [(14, 14), (16, 21), (25, 21), (1, 1), (1, 7), (3, 1), (48, 48)]


@pytest.mark.parametrize("gh,gw", LOGIT_GRIDS)
@pytest.mark.parametrize("sf", SFS)
def test_upsample_logits_sigmoid(sf, gh, gw):
    """Every scale on every grid with 17 planes (one full group of 16 and a group of one); a single plane where 17 planes of
    the output would pass 3M elements (the 48 x 48 grid at x16)."""
    planes = 17 if 17 * sf * sf * gh * gw <= 3_000_000 else 1
    _check_logits_case(planes, gh, gw, sf, seed=300 + sf)


@pytest.mark.parametrize("planes", [1, 15, 16, 120])
@pytest.mark.parametrize("gh,gw,sf", [(14, 14, 2), (3, 1, 3), (1, 1, 16)])
def test_upsample_logits_plane_groups(gh, gw, sf, planes):
    _check_logits_case(planes, gh, gw, sf, seed=310 + planes)


@pytest.mark.parametrize("gh,gw,sf", [(14, 14, 2), (1, 7, 3)])
def test_upsample_logits_forward_plane_count(gh, gw, sf):
    """64 images x 6 layers x 20 queries = 7680 planes: 480 plane groups in blockIdx.y."""
    _check_logits_case(7680, gh, gw, sf, seed=320)


def _up_tokens(tokbuf, B, n, gh, gw, sf, split, alias2x=False):
    """tokens = the first n rows of each image of tokbuf (B, n + extra, 384): strideb is larger than n * 384"""
    up = _nan(B * sf * sf * n + 1, D)
    lib = N.load()
    if alias2x:
        fn = lib.sm_upsample2x_tokens_f16x2 if split else lib.sm_upsample2x_tokens_f32
        rc = fn(tokbuf.data_ptr(), tokbuf.stride(0), up.data_ptr(), B, gh, gw, _stream())
    else:
        fn = lib.sm_upsample_tokens_f16x2 if split else lib.sm_upsample_tokens_f32
        rc = fn(tokbuf.data_ptr(), tokbuf.stride(0), up.data_ptr(), B, gh, gw, sf, _stream())
    N.check(rc, "sm_upsample_tokens")
    assert _untouched(up[-1:])
    return up[:-1].view(B, sf * sf * n, D)


@pytest.mark.parametrize("gh,gw", [(14, 14), (9, 11), (1, 1), (3, 1)])
@pytest.mark.parametrize("sf", SFS)
def test_upsample_tokens(sf, gh, gw):
    """fp32 and F16X2 tokens at every scale, taken from a buffer with a larger image stride.  The bit equality of the two
    outputs is a regression test: with the blend left to the compiler's contraction, the two template instantiations of the
    kernel were fused differently and the F16X2 tokens differed from split(fp32 tokens) in the last bit at every scale > 1."""
    n = gh * gw
    B = 2 if sf * sf * n <= 4096 else 1  # one image where the output passes 4096 pixels (1.5M floats)
    buf = _rand(B, n + 3, D, seed=400 + sf, scale=2.0)
    bufd = buf.to(DEV)
    up = _up_tokens(bufd, B, n, gh, gw, sf, False)
    ups = _up_tokens(bufd, B, n, gh, gw, sf, True)
    assert bool(torch.isfinite(up).all())
    assert _is_split_of(ups, up)
    if sf == 2:
        assert _same_bits(_up_tokens(bufd, B, n, gh, gw, 2, True, alias2x=True), ups)
        assert _same_bits(_up_tokens(bufd, B, n, gh, gw, 2, False, alias2x=True), up)
    tok = buf[:, :n]
    if sf == 1:
        assert torch.equal(up.cpu(), tok)
    planes = R.tokens_to_planes(tok, gh, gw)
    ref = R.planes_to_tokens(R.bilinear_ref(planes, sf))
    ref32 = R.planes_to_tokens(F.interpolate(planes, scale_factor=sf, mode="bilinear"))
    err, err_t = _maxerr(up, ref), _maxerr(ref32, ref)
    bound = 3 * err_t + 1e-6 * tok.abs().max().item()
    _ledger.record("forward_kernels", f"upsample_tokens[{gh}x{gw}-sf{sf}]", {"err_vs_fp64": err, "torch_fp32_err": err_t, "bound": bound})
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("sf", [1, 2, 4])
def test_mask_head_orders_agree(sf):
    """For n % 4 == 0 the forward evaluates up(Q tok^T) in place of the literal Q up(tok)^T (maskformer.py:144-162, 223).  Both
    orders through the library, each against the fp64 evaluation of the literal order; the yardstick is torch CPU fp32 doing
    the literal order on the same data."""
    gh = gw = 14
    n, R_ = gh * gw, 120
    q, tok = _rand(R_, D, seed=500), _rand(1, n, D, seed=501, scale=0.25)  # logits of magnitude up to ~16
    qd, tokd = q.to(DEV), tok.to(DEV)
    low = ops.gemm(qd, tokd[0])  # (120, n)
    la, pa = _up_logits(low.contiguous(), R_, gh, gw, sf)
    up = _up_tokens(tokd, 1, n, gh, gw, sf, False)
    lb, pb = ops.gemm(qd, up[0].contiguous(), None, epilogue=N.EPI_SIGMOID2)
    planes = R.tokens_to_planes(tok, gh, gw)
    ref = q.double() @ R.planes_to_tokens(R.bilinear_ref(planes, sf))[0].T
    lit32 = q @ R.planes_to_tokens(F.interpolate(planes, scale_factor=sf, mode="bilinear"))[0].T
    err_a, err_b, err_t = _maxerr(la, ref), _maxerr(lb, ref), _maxerr(lit32, ref)
    bound = 3 * err_t + 1e-6
    _ledger.record("forward_kernels", f"mask_head_orders[sf{sf}]",
                   {"err_up_of_gemm": err_a, "err_gemm_of_up": err_b, "torch_fp32_err": err_t, "bound": bound,
                    "max_logit": ref.abs().max().item()})
    assert err_a <= bound and err_b <= bound, (err_a, err_b, bound)
    assert _maxerr(pa, torch.sigmoid(la.double())) <= 2e-6 and _maxerr(pb, torch.sigmoid(lb.double())) <= 2e-6


def test_upsample_refusals():
    lib = N.load()
    t, o = _rand(1, 4, D, seed=600).to(DEV), _nan(64, D)
    for sf in (0, 17):
        with pytest.raises(RuntimeError, match="sm_upsample_tokens: bad arguments"):
            N.check(lib.sm_upsample_tokens_f32(t.data_ptr(), 4 * D, o.data_ptr(), 1, 2, 2, sf, _stream()))
        with pytest.raises(RuntimeError, match="sm_upsample_tokens: bad arguments"):
            N.check(lib.sm_upsample_tokens_f16x2(t.data_ptr(), 4 * D, o.data_ptr(), 1, 2, 2, sf, _stream()))
        with pytest.raises(RuntimeError, match="sm_upsample_logits_sigmoid_f32: bad arguments"):
            N.check(lib.sm_upsample_logits_sigmoid_f32(t.data_ptr(), None, o.data_ptr(), 1, 2, 2, sf, _stream()))
    with pytest.raises(RuntimeError, match="sm_upsample_tokens: bad arguments"):
        N.check(lib.sm_upsample_tokens_f32(t.data_ptr(), 4 * D + 2, o.data_ptr(), 1, 2, 2, 2, _stream()))
    # 65536 plane groups do not fit blockIdx.y; the check comes before the launch (misc.hip), so small buffers are safe
    with pytest.raises(RuntimeError, match="beyond the launch grid"):
        N.check(lib.sm_upsample_logits_sigmoid_f32(t.data_ptr(), None, o.data_ptr(), 65536 * 16, 1, 1, 1, _stream()))
    torch.cuda.synchronize()
    assert _untouched(o)


# ===== 4. small producers ====================================================================================================
@pytest.mark.parametrize("P,H,W", [(16, 224, 224), (8, 64, 72), (16, 250, 333), (8, 30, 21), (16, 97, 211)])
def test_im2col_f16x2(P, H, W):
    x = _rand(2, 3, H, W, seed=40)
    xd = x.to(DEV)
    gh, gw = -(-H // P), -(-W // P)
    rows, K = 2 * gh * gw, 3 * P * P
    cols, colss = _nan(rows + 1, K), _nan(rows + 1, K)
    N.check(N.load().sm_im2col_patches_f32(xd.data_ptr(), cols.data_ptr(), 2, H, W, P, _stream()), "sm_im2col_patches_f32")
    N.check(N.load().sm_im2col_patches_f16x2(xd.data_ptr(), colss.data_ptr(), 2, H, W, P, _stream()), "sm_im2col_patches_f16x2")
    assert _untouched(cols[rows:]) and _untouched(colss[rows:])
    xp = F.pad(x, (0, (P - W % P) % P, 0, (P - H % P) % P))
    ref = F.unfold(xp, kernel_size=P, stride=P).transpose(1, 2).reshape(-1, K)
    assert torch.equal(cols[:rows].cpu(), ref)
    assert _is_split_of(colss[:rows], cols[:rows])


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("Nt", [2, 197, 785])
def test_cls_rows(Nt, B):
    cls, pos = _rand(D, seed=700), _rand(Nt, D, seed=701)
    clsd, posd, tokens = cls.to(DEV), pos.to(DEV), _nan(B, Nt, D)
    N.check(N.load().sm_cls_rows_f32(clsd.data_ptr(), posd.data_ptr(), tokens.data_ptr(), B, Nt, _stream()), "sm_cls_rows_f32")
    assert torch.equal(tokens[:, 0].cpu(), (cls + pos[0]).expand(B, D))
    assert _untouched(tokens[:, 1:])


@pytest.mark.parametrize("nq", [1, 7, 8, 9, 20, 33, 100])
def test_query_mean(nq):
    """features = mean over the queries of the LAST layer.  Layer l is offset by 10 l, so another layer's mean is 10 away.
    Bound: a sequential fp32 sum of nq terms, then one division: (nq + 1) 2^-24 max|q| against the fp64 mean."""
    for L in (1, 3, 6):
        for B in (1, 5):
            q = _rand(B, L, nq, D, seed=800 + 10 * L + B) + 10.0 * torch.arange(L, dtype=torch.float32).view(1, L, 1, 1)
            qd, f = q.to(DEV), _nan(B + 1, D)
            N.check(N.load().sm_query_mean_f32(qd.data_ptr(), f.data_ptr(), B, L, nq, _stream()), "sm_query_mean_f32")
            assert _untouched(f[B:])
            ref = q[:, L - 1].double().mean(1)
            bound = (nq + 1) * 2.0 ** -24 * q[:, L - 1].abs().max().item()
            assert _maxerr(f[:B], ref) <= bound, (L, B, _maxerr(f[:B], ref), bound)


@pytest.mark.parametrize("rows_per", [1, 20, 100])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_broadcast_rows(B, rows_per):
    src = _rand(rows_per, D, seed=900 + rows_per)
    srcd, dst = src.to(DEV), _nan(B * rows_per + 2, D)
    N.check(N.load().sm_broadcast_rows_f32(srcd.data_ptr(), dst.data_ptr(), rows_per, B, _stream()), "sm_broadcast_rows_f32")
    assert torch.equal(dst[:B * rows_per].cpu().view(B, rows_per, D), src.expand(B, rows_per, D))
    assert _untouched(dst[B * rows_per:])
