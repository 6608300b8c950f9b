"""The device PNG encoder (csrc/png.hip, ops.png_encode) against selfmask_amd/png.py's encode_reference, which test_png_cpu.py has Pillow
decode: byte equality, zero tolerance - the format is integer arithmetic on the input alone."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from selfmask_amd import _native as N  # noqa: E402
from selfmask_amd import ops, png  # noqa: E402
from _png_cases import CASES  # noqa: E402

DEV = torch.device("cuda:0")
GUARD, FILL = 64, 0xA5

_REF = {}


def _reference(name):
    """the case and its expected file, computed once and handed out read-only"""
    if name not in _REF:
        a, mode = CASES[name]()
        a.setflags(write=False)
        _REF[name] = (a, mode, png.encode_reference(a, mode))
    return _REF[name]


def _channels(a):
    return 1 if a.ndim == 2 else a.shape[2]


def _table(images, modes, cap_delta=0):
    B = len(images)
    table = (N.PngImage * B)()
    lib = N.load()
    po = oo = 0
    for b, (a, mode) in enumerate(zip(images, modes)):
        d = table[b]
        d.pix_off, d.out_off, d.H, d.W, d.channels, d.filter_mode = po, oo, a.shape[0], a.shape[1], _channels(a), mode
        d.out_cap = lib.sm_png_bound(d.H, d.W, d.channels) + cap_delta
        po += a.size
        oo += d.out_cap + GUARD
    return table, oo


def _run_abi(images, modes):
    """One sm_png_encode_batch_u8 call on buffers of the test's own: pixels and files packed back to back (so most start off any
    alignment), GUARD bytes behind each out_cap, the output prefilled with FILL -> per image (file bytes, everything behind them up to
    the next image's out_off)."""
    table, total = _table(images, modes)
    B = len(images)
    lib = N.load()
    pixels = torch.from_numpy(np.concatenate([a.reshape(-1) for a in images])).to(DEV)
    dev_table = torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).to(DEV)
    out = torch.full((total,), FILL, dtype=torch.uint8, device=DEV)
    sizes = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    ws_bytes = lib.sm_png_workspace_bytes(table, B)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    N.check(lib.sm_png_encode_batch_u8(pixels.data_ptr(), table, dev_table.data_ptr(), B, out.data_ptr(), sizes.data_ptr(), ws.data_ptr(),
                                       ws_bytes, torch.cuda.current_stream().cuda_stream), "sm_png_encode_batch_u8")
    torch.cuda.synchronize()
    out_h, sizes_h = out.cpu().numpy(), sizes.cpu().numpy()
    res = []
    for b in range(B):
        o, n = table[b].out_off, int(sizes_h[b])
        assert 0 < n <= table[b].out_cap, (b, n)
        res.append((out_h[o:o + n].tobytes(), out_h[o + n:o + table[b].out_cap + GUARD]))
    return res


@pytest.mark.parametrize("name", sorted(CASES))
def test_file_equals_the_reference(name):
    a, mode, want = _reference(name)
    (got, rest), = _run_abi([a], [mode])
    assert len(got) == len(want), (len(got), len(want))
    assert got == want
    assert (rest == FILL).all()                      # nothing behind the file is touched, the guard least of all


def test_the_cases_reach_every_block_type():
    """stored, fixed and dynamic blocks, a one-byte last chunk, runs across a cut: what the byte comparisons above have walked through"""
    kinds = {}
    for name in ("noise-x3", "mixed-1x7x1", "chunk+1-x1", "fibonacci-shifted-filter0", "const255-filter0-x4", "zeros-x1"):
        a, mode, _ = _reference(name)
        s = png.filtered_stream(a, mode)
        kinds[name] = [png.deflate_chunk(s[o:o + png.PNG_CHUNK], o + png.PNG_CHUNK >= len(s))[1] for o in range(0, len(s), png.PNG_CHUNK)]
    assert kinds["noise-x3"] == [0, 0] and kinds["mixed-1x7x1"] == [1] and kinds["chunk+1-x1"] == [2, 1]
    assert kinds["fibonacci-shifted-filter0"] == [2] and len(kinds["const255-filter0-x4"]) >= 2 and len(kinds["zeros-x1"]) == 2


def test_images_of_one_call_are_independent():
    """L, RGB and RGBA images of different sizes in one call, in either table order: per image the bytes of its own single call"""
    names = ["photo300x400-x1", "mixed-17x23x3", "3chunks+5-x4", "zeros-x3", "mixed-1x1x4"]
    cases = [_reference(n) for n in names]
    single = [_run_abi([a], [m])[0][0] for a, m, _ in cases]
    for s, (_, _, want) in zip(single, cases):
        assert s == want
    for order in (list(range(len(names))), list(range(len(names)))[::-1]):
        res = _run_abi([cases[k][0] for k in order], [cases[k][1] for k in order])
        for k, (got, rest) in zip(order, res):
            assert got == single[k] and (rest == FILL).all()


def test_range_checks_return_errors_before_any_launch():
    lib = N.load()
    a = np.zeros((5, 6, 3), np.uint8)
    pixels = torch.zeros(a.size, dtype=torch.uint8, device=DEV)
    out = torch.full((4096,), FILL, dtype=torch.uint8, device=DEV)
    sizes = torch.full((1,), -1, dtype=torch.int64, device=DEV)

    def call(table, ws_short=0):
        ws_bytes = max(lib.sm_png_workspace_bytes(table, 1), 256 * 1024)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        dev_table = torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).to(DEV)
        need = lib.sm_png_workspace_bytes(table, 1)
        rc = lib.sm_png_encode_batch_u8(pixels.data_ptr(), table, dev_table.data_ptr(), 1, out.data_ptr(), sizes.data_ptr(), ws.data_ptr(),
                                        need - ws_short if need else ws_bytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, lib.sm_last_error()

    table, _ = _table([a], [-1])
    table[0].channels = 2
    assert lib.sm_png_bound(5, 6, 2) == 0 and lib.sm_png_workspace_bytes(table, 1) == 0
    rc, msg = call(table)
    assert rc == -1 and b"channels" in msg
    table, _ = _table([a], [-1], cap_delta=-1)
    rc, msg = call(table)
    assert rc == -3 and b"out_cap" in msg
    table, _ = _table([a], [-1])
    rc, msg = call(table, ws_short=1)
    assert rc == -3 and b"workspace" in msg
    table, _ = _table([a], [5])
    assert call(table)[0] == -1
    assert (out.cpu().numpy() == FILL).all() and int(sizes.cpu()[0]) == -1   # nothing ran
    table, _ = _table([a], [-1])
    assert call(table)[0] == 0 and int(sizes.cpu()[0]) == len(png.encode_reference(a))
    assert lib.sm_png_bound(5, 6, 3) == png.bound(5, 6, 3) and lib.sm_png_bound(4096, 4096, 4) == png.bound(4096, 4096, 4)


def test_ops_png_encode_tensors_and_packed():
    names = ["mixed-17x23x3", "hard-mask", "mixed-5x300x4"]
    cases = [_reference(n) for n in names]
    tensors = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a, _, _ in cases]
    for _ in range(2):                               # the second call finds its table cached on the device
        files = ops.png_encode(tensors)
        assert [type(f) for f in files] == [bytes] * 3 and files == [w for _, _, w in cases]
    flat = torch.cat([torch.zeros(5, dtype=torch.uint8, device=DEV)] + [t.reshape(-1) for t in tensors])
    offs, o = [], 5
    for a, _, _ in cases:
        offs.append(o)
        o += a.size
    shapes = [(a.shape[0], a.shape[1], _channels(a)) for a, _, _ in cases]
    assert ops.png_encode(packed=(flat, offs, shapes)) == [w for _, _, w in cases]
    a = cases[0][0]
    assert ops.png_encode([tensors[0]], filter_mode=3) == [png.encode_reference(a, 3)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.png_encode([tensors[0].cpu()])
    with pytest.raises(ValueError):
        ops.png_encode(packed=(flat, [flat.numel() - 3], [(2, 2, 1)]))
