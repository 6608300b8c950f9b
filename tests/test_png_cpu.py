"""The PNG restatement (selfmask_amd/png.py: the definition of what csrc/png.hip writes) against witnesses of its own: Pillow decodes
every file (and with it checks every CRC-32; zlib checks the Adler-32), the filters are pinned to the standard's formulas, the tokens to
hand-written lists, and the size to a zlib model of the same scheme."""
import zlib
from io import BytesIO

import numpy as np
import pytest
from PIL import Image

from selfmask_amd import png
from selfmask_amd import present as P
from _present_cases import KINDS, make_case
from _png_cases import CASES, photo

MODES = {1: "L", 3: "RGB", 4: "RGBA"}


def _channels(a):
    return 1 if a.ndim == 2 else a.shape[2]


@pytest.mark.parametrize("name", sorted(CASES))
def test_pillow_decodes_every_case_to_its_input(name):
    a, filter_mode = CASES[name]()
    data = png.encode_reference(a, filter_mode)
    img = Image.open(BytesIO(data))
    img.load()                                    # every chunk's CRC, the zlib stream's Adler-32
    assert img.mode == MODES[_channels(a)] and img.size == (a.shape[1], a.shape[0])
    assert np.array_equal(np.asarray(img), a)
    assert len(data) <= png.bound(a.shape[0], a.shape[1], _channels(a))
    assert data[:8] == png.SIGNATURE and data[12:16] == b"IHDR" and data[-12:] == bytes.fromhex("0000000049454e44ae426082")
    # signature, IHDR, IDATs, IEND and nothing else
    at, kinds = 8, []
    while at < len(data):
        n = int.from_bytes(data[at:at + 4], "big")
        kinds.append(data[at + 4:at + 8])
        at += 12 + n
    assert at == len(data) and kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and set(kinds[1:-1]) == {b"IDAT"}
    assert len(kinds) - 2 == png.n_chunks(a.shape[0], a.shape[1], _channels(a))


def test_the_fibonacci_cases_count_what_they_say():
    from _png_cases import _fibonacci
    for shifted, depth in ((False, 9), (True, 17)):
        a = _fibonacci(shifted)
        stream = png.filtered_stream(a, 0)
        counts = np.bincount(stream, minlength=286)
        counts[256] = 1
        assert all(t[0] == "lit" for t in png.chunk_tokens(stream.tobytes()))
        assert max(png.code_lengths(counts.tolist(), 32)) == depth
        assert max(png.code_lengths(counts.tolist(), 15)) == min(depth, 15)
    assert sorted(np.bincount(_fibonacci().reshape(-1)).tolist())[1:] == [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987]


def test_bound_and_shape_limits():
    assert png.bound(1, 1, 1) == 2 + 22 + 51
    assert png.bound(0, 4, 3) == 0 and png.bound(4, 4, 2) == 0 and png.bound(4097, 4096, 1) == 0 and png.bound(4096, 4096, 4) > 0
    with pytest.raises(ValueError):
        png.encode_reference(np.zeros((2, 2, 2), np.uint8))
    with pytest.raises(ValueError):
        png.encode_reference(np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError):
        png.filtered_stream(np.zeros((2, 2), np.uint8), 5)


# ---- filters ----------------------------------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


@pytest.mark.parametrize("bpp", [1, 3, 4])
def test_each_filter_against_the_standards_formula(bpp):
    rng = np.random.Generator(np.random.PCG64([bpp, 5]))
    cur, up = rng.integers(0, 256, 16 * bpp, dtype=np.uint8), rng.integers(0, 256, 16 * bpp, dtype=np.uint8)
    up[bpp:2 * bpp] = cur[:bpp]                      # a == b: Paeth's first tie
    for first_row in (False, True):
        b_row = np.zeros_like(up) if first_row else up
        got = png.filter_candidates(cur, b_row, bpp)
        x, b = cur.astype(int), b_row.astype(int)
        a = np.concatenate([np.zeros(bpp, int), x[:-bpp]])
        c = np.concatenate([np.zeros(bpp, int), b[:-bpp]])
        assert np.array_equal(got[0], cur)
        assert np.array_equal(got[1], ((x - a) % 256).astype(np.uint8))
        assert np.array_equal(got[2], ((x - b) % 256).astype(np.uint8))
        assert np.array_equal(got[3], ((x - (a + b) // 2) % 256).astype(np.uint8))
        assert np.array_equal(got[4], np.array([(x[i] - _paeth(a[i], b[i], c[i])) % 256 for i in range(len(x))], np.uint8))


def test_paeth_ties_follow_the_order_a_b_c():
    # (a, b, c) -> predictor, by hand: all distances equal -> a; pa == pc < pb -> a over c; pb == pc < pa -> b over c; a == b -> a
    for a, b, c, want in ((7, 7, 7, 7), (16, 10, 12, 16), (10, 16, 12, 16), (5, 5, 0, 5)):
        assert _paeth(a, b, c) == want
        cur, up = np.array([a, 200], np.uint8), np.array([c, b], np.uint8)
        assert png.filter_candidates(cur, up, 1)[4][1] == (200 - want) % 256


def test_adaptive_pick_is_the_smallest_sum_ties_to_the_lowest_id():
    a = np.zeros((3, 8), np.uint8)                  # every filter gives zeros: filter 0 wins every row
    assert png.filtered_stream(a).reshape(3, 9)[:, 0].tolist() == [0, 0, 0]
    a = np.tile(np.arange(8, dtype=np.uint8) * 3, (3, 1))
    s = png.filtered_stream(a).reshape(3, 9)
    assert s[0, 0] == 1 and s[1, 0] == 2 and s[2, 0] == 2   # a ramp: Sub on the first row; Up gives zeros below (Paeth ties, id 4 loses)
    rng = np.random.Generator(np.random.PCG64(3))
    a = rng.integers(0, 256, (6, 11, 3), dtype=np.uint8)
    s = png.filtered_stream(a).reshape(6, 34)
    rows = a.reshape(6, 33)
    for y in range(6):
        cand = png.filter_candidates(rows[y], rows[y - 1] if y else np.zeros(33, np.uint8), 3)
        cost = [int(np.abs(c.view(np.int8).astype(int)).sum()) for c in cand]
        assert s[y, 0] == cost.index(min(cost)) and np.array_equal(s[y, 1:], cand[s[y, 0]])
    for mode in range(5):
        assert (png.filtered_stream(a, mode).reshape(6, 34)[:, 0] == mode).all()


# ---- tokens -----------------------------------------------------------------------------------------------------------------------------
L, M = (lambda v=9: ("lit", v)), (lambda n: ("match", n))
RUNS = {1: [L()], 2: [L(), L()], 3: [L(), L(), L()], 4: [L(), M(3)], 258: [L(), M(257)], 259: [L(), M(258)], 260: [L(), M(258), L()],
        261: [L(), M(258), L(), L()], 262: [L(), M(258), M(3)], 517: [L(), M(258), M(258)]}


@pytest.mark.parametrize("n", sorted(RUNS))
def test_tokens_of_a_run(n):
    assert png.chunk_tokens(bytes([9]) * n) == RUNS[n]
    # the same run between two other bytes
    assert png.chunk_tokens(bytes([1]) + bytes([9]) * n + bytes([2])) == [("lit", 1)] + RUNS[n] + [("lit", 2)]


def test_length_symbols_are_rfc_1951s():
    base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    extra = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    sym, eb, ev = png.length_symbol(np.arange(3, 259))
    for length in range(3, 259):
        i = 28 if length == 258 else max(j for j in range(28) if base[j] <= length)
        assert (sym[length - 3], eb[length - 3], ev[length - 3]) == (257 + i, extra[i], length - base[i])


def test_code_lengths_are_complete_limited_and_deterministic():
    fib = [1, 1]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    assert max(png.code_lengths(fib, 32)) == 16     # a strict Fibonacci row: one chain
    lens = png.code_lengths(fib, 15)
    assert max(lens) == 15 and sum(2 ** (15 - v) for v in lens) == 2 ** 15 and lens == sorted(lens, reverse=True)
    assert png.code_lengths([0, 5, 0], 15) == [0, 1, 0] and png.code_lengths([0, 0], 7) == [0, 0]
    assert png.code_lengths([3, 3, 3, 3], 15) == [2, 2, 2, 2]
    lens = png.code_lengths([1, 2, 4, 8, 16, 32, 64, 128, 256], 7)
    assert max(lens) == 7 and sum(2 ** (7 - v) for v in lens) == 2 ** 7 and lens == sorted(lens, reverse=True)
    rng = np.random.Generator(np.random.PCG64(11))
    counts = rng.integers(0, 50, 286).tolist()
    lens = png.code_lengths(counts, 15)
    assert all((v > 0) == (c > 0) for v, c in zip(lens, counts)) and sum(2 ** (15 - v) for v in lens if v) == 2 ** 15
    codes = png.canonical_codes(lens)               # prefix-free: no code is the start of another (bit-reversed: compare from bit 0)
    words = sorted(format(c, "0%db" % v)[::-1] for c, v in zip(codes, lens) if v)
    assert all(not words[i + 1].startswith(words[i]) for i in range(len(words) - 1))


# ---- size ---------------------------------------------------------------------------------------------------------------------------------
def _model_bytes(stream: bytes) -> int:
    """raw deflate, Z_RLE, level 6, a full flush every PNG_CHUNK bytes"""
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
    n = 0
    for o in range(0, len(stream), png.PNG_CHUNK):
        n += len(c.compress(stream[o:o + png.PNG_CHUNK])) + len(c.flush(zlib.Z_FULL_FLUSH))
    return n + len(c.flush())


def _size_cases():
    for kind in KINDS:
        mask, rgb = make_case(0, kind)
        m, h = P.present_reference_numpy(mask, rgb)
        yield kind + "-mask", m
        yield kind + "-heat", h
    yield "photo", photo(300, 400)


@pytest.mark.parametrize("name,a", list(_size_cases()), ids=[n for n, _ in _size_cases()])
def test_size_against_a_zlib_model_of_the_scheme(name, a):
    payload = sum(len(p) for p in png.idat_payloads(a)) - 6          # without the zlib header and the Adler-32
    model = _model_bytes(png.filtered_stream(a).tobytes())
    chunks = png.n_chunks(a.shape[0], a.shape[1], _channels(a))
    buf = BytesIO()
    Image.fromarray(a).save(buf, format="PNG")
    print(f"{name}: payload {payload}, zlib model {model} (x{payload / model:.4f}), Pillow's file {len(buf.getvalue())}, "
          f"this file {len(png.encode_reference(a))}")
    assert payload <= model * 1.02 + 16 * chunks
    assert len(png.encode_reference(a)) <= png.bound(a.shape[0], a.shape[1], _channels(a))


# ---- the C ABI's host half (no GPU: every check below returns before a launch) -------------------------------------------------------------
def test_abi_bound_workspace_and_range_checks():
    from selfmask_amd import _native as N
    lib = N.load()
    for H, W, C in ((1, 1, 1), (17, 23, 3), (300, 400, 4), (4096, 4096, 4), (1, 1 << 24, 1)):
        assert lib.sm_png_bound(H, W, C) == png.bound(H, W, C) > 0
    assert lib.sm_png_bound(5, 6, 2) == 0 and lib.sm_png_bound(0, 6, 3) == 0 and lib.sm_png_bound(4097, 4096, 1) == 0
    t = (N.PngImage * 1)()
    t[0].H, t[0].W, t[0].channels, t[0].filter_mode, t[0].out_cap = 5, 6, 3, -1, png.bound(5, 6, 3)
    need = lib.sm_png_workspace_bytes(t, 1)
    assert need >= 5 * 19 + 16384 and lib.sm_png_workspace_bytes(t, 0) == 0
    fake = 1 << 20                                  # never dereferenced: the checks come first

    def call(ws_bytes):
        return lib.sm_png_encode_batch_u8(fake, t, fake, 1, fake, fake, fake, ws_bytes, None)
    assert call(need - 1) == -3 and b"workspace" in lib.sm_last_error()
    t[0].out_cap -= 1
    assert call(need) == -3 and b"out_cap" in lib.sm_last_error()
    t[0].out_cap += 1
    t[0].channels = 2
    assert lib.sm_png_workspace_bytes(t, 1) == 0 and call(need) == -1 and b"channels" in lib.sm_last_error()
    t[0].channels, t[0].filter_mode = 3, 5
    assert call(need) == -1 and b"filter_mode" in lib.sm_last_error()
    t[0].filter_mode = -1
    assert lib.sm_png_encode_batch_u8(None, t, fake, 1, fake, fake, fake, need, None) == -1
