"""The ResNet-50 backbone on the device (csrc/conv.hip, selfmask_amd/resnet.py): each streaming kernel through the C ABI against its
numpy form (tests/_resnet_ref.py) - the gathers and the F16X2 outputs bit for bit - and the whole forward against the fp64 maps of the
REAL reference (tests/golden/resnet50_*.npz, scripts/gen_resnet_golden.py).

The forward's gate is the project's 1e-4 (BASELINE.json): the fixtures keep every map at max |x| <= 8 and the reference's own fp32
evaluation within e32 <= 1e-5 of fp64; F16X2 operands keep 22 of fp32's 24 significant bits, so the expected distance is a small
multiple of e32 - a wrong tap, a wrong fold or a dropped lo term is orders outside the gate.  With SM_RESNET_PARITY_OUT=<file> in
the environment the measured distances are written there as JSON (profiles/resnet_parity.json is such a run).
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import _resnet_cases as RC  # noqa: E402
import _resnet_ref as RR  # noqa: E402
from selfmask_amd import ResNet50, resnet_features  # noqa: E402
from selfmask_amd import _native as N  # noqa: E402
from selfmask_amd import ops  # noqa: E402
from selfmask_amd import resnet as R  # noqa: E402

DEV = "cuda:0"
GATE = 1e-4
_PARITY = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().contiguous().cpu().view(torch.int32).numpy()


def _rand(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


# ---- tap gather ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(5, 7), (3, 3)])
@pytest.mark.parametrize("cin", [64, 512])
@pytest.mark.parametrize("k,stride,dil", [(1, 2, 1), (3, 1, 1), (3, 2, 1), (3, 1, 2), (3, 1, 4)])
def test_conv_gather_bit_identical(k, stride, dil, cin, hw):
    H, W = hw
    pad = dil if k == 3 else 0
    x = _rand(k * 100 + stride * 10 + dil, 2, H, W, cin)
    x[1] = 1000.123  # image 1: a constant no tap of image 0 may show (and the reverse); not an f16 value, so lo != 0
    xs = ops.split_f16x2(x.to(DEV))
    host = _bits(xs)
    assert (host.view(np.int16).reshape(-1, 2, 8)[:, 1] != 0).any(), "the input needs a non-trivial lo half"
    exp = RR.gather_taps(host, k, stride, dil, pad)
    out = _nan(*exp.shape)
    N.check(N.load().sm_conv_gather_f16x2(xs.data_ptr(), out.data_ptr(), 2, H, W, cin, k, stride, dil, pad, _stream()), "gather")
    got = _bits(out)
    assert np.array_equal(got, exp)
    const = _bits(ops.split_f16x2(torch.full((1, 8), 1000.123, device=DEV)))[0]
    g0 = got[0].reshape(-1, 8)
    assert not (g0 == const).all(axis=1).any(), "a tap of image 0 read image 1"
    g1 = got[1].reshape(-1, 8)
    assert ((g1 == const).all(axis=1) | (g1 == 0).all(axis=1)).all(), "a tap of image 1 is neither its constant nor padding"


@pytest.mark.parametrize("shape", [(2, 3, 17, 23), (1, 3, 40, 56)])
def test_stem_gather(shape):
    x = _rand(shape[2], *shape)
    exp_f32 = RR.gather_stem(x.numpy())
    assert exp_f32.shape[-1] == 160 and (exp_f32[..., 147:] == 0).all()
    exp = _bits(ops.split_f16x2(torch.from_numpy(exp_f32).to(DEV)))
    out = _nan(*exp.shape)
    N.check(N.load().sm_resnet_stem_gather_f16x2(x.to(DEV).data_ptr(), out.data_ptr(), shape[0], shape[2], shape[3], _stream()), "stem")
    got = _bits(out)
    assert np.array_equal(got, exp)
    assert (got[..., 152:] == 0).all() and (got.view(np.int16).reshape(*got.shape[:-1], 20, 2, 8)[..., 18, :, 3:] == 0).all()  # columns 147..159


@pytest.mark.parametrize("hw,negative", [((9, 12), False), ((20, 28), False), ((9, 12), True)])
def test_maxpool(hw, negative):
    H, W = hw
    x = _rand(H + int(negative), 2, H, W, 64)
    if negative:
        x = -x.abs() - 0.25
    exp = RR.maxpool3x3s2(x.numpy())
    out, outs = _nan(*exp.shape), _nan(*exp.shape)
    xd = x.to(DEV)
    N.check(N.load().sm_maxpool3x3s2_nhwc_f32(xd.data_ptr(), out.data_ptr(), outs.data_ptr(), 2, H, W, 64, _stream()), "maxpool")
    assert np.array_equal(out.cpu().numpy(), exp)
    if negative:
        assert out.max().item() < 0
    assert np.array_equal(_bits(outs), _bits(ops.split_f16x2(out)))
    only = _nan(*exp.shape)  # the forward's call: no fp32 output
    N.check(N.load().sm_maxpool3x3s2_nhwc_f32(xd.data_ptr(), None, only.data_ptr(), 2, H, W, 64, _stream()), "maxpool")
    assert np.array_equal(_bits(only), _bits(outs))


def test_relu_split():
    x = _rand(9, 37, 256).to(DEV)
    exp = torch.relu(x)
    dst, dsts = _nan(37, 256), _nan(37, 256)
    N.check(N.load().sm_relu_split_f16x2(x.data_ptr(), dst.data_ptr(), dsts.data_ptr(), 37, 256, _stream()), "relu_split")
    assert torch.equal(dst, exp) and np.array_equal(_bits(dsts), _bits(ops.split_f16x2(exp)))
    xin = x.clone()  # in place, as the forward runs it
    dsts2 = _nan(37, 256)
    N.check(N.load().sm_relu_split_f16x2(xin.data_ptr(), xin.data_ptr(), dsts2.data_ptr(), 37, 256, _stream()), "relu_split")
    assert torch.equal(xin, exp) and np.array_equal(_bits(dsts2), _bits(dsts))


@pytest.mark.parametrize("hw", [(3, 3), (5, 7)])
def test_upsample_2048_channels(hw):
    h, w = hw
    f = _rand(h * w, 2, h, w, 2048)
    ref = F.interpolate(f.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    got = R.upsample_nhwc_aligned(f.to(DEV), 2).cpu()
    assert got.shape == ref.shape == (2, 2 * h, 2 * w, 2048)
    d = (got - ref).abs().max().item()
    print(f"upsample {hw}: max |hip - F.interpolate| = {d:.2e}")
    assert d <= 1e-6


# ---- the whole forward --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    out = {}
    for dilated in (True, False):
        m = ResNet50(use_dilated_resnet=dilated)
        m.load_state_dict(RC.synthetic_resnet_state_dict(11, dilated), strict=True)
        out[dilated] = m.to(DEV)
    return out


def _check_maps(name, maps, fx):
    assert [list(m.shape) for m in maps] == fx["shapes"].tolist()
    dist = []
    for i, m in enumerate(maps):
        ref = fx[f"map{i + 1}_f64"]
        got = (m if i == 3 else m[:, ::RC.STORE_EVERY]).double().cpu().numpy()
        dist.append(float(np.abs(got - ref).max()))
        print(f"{name} map{i + 1}: max |hip - ref64| = {dist[-1]:.3e} (e32 {fx['e32'][i]:.2e}, max |ref| {np.abs(ref).max():.2f})")
    return dist


@pytest.mark.parametrize("name", list(RC.CASES))
def test_forward_matches_reference(name, models, golden_dir):
    dilated, shape, wseed, xseed = RC.CASES[name]
    assert wseed == 11
    fx = np.load(os.path.join(golden_dir, f"resnet50_{name}.npz"))
    maps = models[dilated](RC.synthetic_input(xseed, shape).to(DEV))
    dist = _check_maps(name, maps, fx)
    _PARITY[name] = {"max_abs_hip_minus_ref64": dist, "e32": [float(e) for e in fx["e32"]], "gate": GATE}
    path = os.environ.get("SM_RESNET_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(_PARITY, f, indent=1)
    assert max(dist) <= GATE, dist


def test_second_call_other_batch_size(models, golden_dir):
    """workspace and packed weights are reused: B = 2, then B = 1 on the same module, then B = 2 again gives the first result"""
    dilated, shape, _wseed, xseed = RC.CASES["d8_17x23_b2"]
    fx = np.load(os.path.join(golden_dir, "resnet50_d8_17x23_b2.npz"))
    m = models[dilated]
    x = RC.synthetic_input(xseed, shape).to(DEV)
    first = [t.clone() for t in m(x)]
    gen = m.weights_generation
    one = m(x[:1])
    for i, t in enumerate(one):
        ref = fx[f"map{i + 1}_f64"][:1]
        got = (t if i == 3 else t[:, ::RC.STORE_EVERY]).double().cpu().numpy()
        assert np.abs(got - ref).max() <= GATE
    again = m(x)
    assert m.weights_generation == gen and len(m._workspace) == 1
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert max(_check_maps("d8_17x23_b2 (again)", again, fx)) <= GATE


def test_resnet_features(models):
    dilated, shape, wseed, xseed = RC.CASES["d8_17x23_b2"]
    x = RC.synthetic_input(xseed, shape)
    ref, hw_ref = RR.features(RC.synthetic_resnet_state_dict(wseed, dilated), x, dilated)
    feats, hw = resnet_features(models[dilated], x.to(DEV))
    assert hw == hw_ref == (3, 3) and tuple(feats.shape) == tuple(ref.shape) == (2, 36, 2048)
    d = (feats.double().cpu() - ref).abs().max().item()
    print(f"resnet_features: max |hip - restatement fp64| = {d:.3e}")
    assert d <= GATE
