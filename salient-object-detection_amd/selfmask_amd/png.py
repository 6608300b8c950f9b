"""The PNG encoder of the serving response restated in numpy and Python integers: the host half of ``csrc/png.hip`` and THE DEFINITION
of its output.  Every step is a function of the input alone (integer histograms, no floats, nothing that depends on an order of
execution), so the device gives these bytes exactly; the GPU tests hold it to that with zero tolerance, and the CPU tests have Pillow
decode what this file writes (Pillow checks every CRC-32, zlib the Adler-32).

The format, choice by choice:

* **Container.**  (H, W) / (H, W, 3) / (H, W, 4) uint8 -> colour type 0 / 2 / 6, 8 bits, not interlaced: signature, IHDR, one IDAT per
  deflate chunk, IEND; no ancillary chunks.  The first IDAT begins with the zlib header ``78 01``, the last ends with the Adler-32 of the
  filtered stream.
* **Filter.**  Per row all five PNG filters; the one with the smallest sum of |signed byte| wins, ties to the lowest id; the row above
  the first is zeros; Paeth with the standard's tie order (a, b, c).  ``filter_mode`` 0 .. 4 forces one filter for every row.
* **Chunks.**  The filtered stream (H (W C + 1) bytes) is cut every ``PNG_CHUNK`` bytes; no match reaches back across a cut.
* **Tokens** (``position_tokens``).  Inside a chunk a maximal run of n equal bytes is: its first byte as a literal; of the other n - 1,
  matches of length 258 at distance 1 while 258 or more remain; one match of the remainder if it is >= 3, else 1 or 2 literals.
* **Block.**  One deflate block per chunk, the smallest in bits of stored / fixed Huffman / dynamic Huffman, ties to the earlier.
* **Dynamic code** (``code_lengths``).  Symbols with a count are sorted by (count, symbol) ascending; Huffman by two queues, a leaf taken
  before an internal node of equal weight; the number of leaves per depth, with depths beyond the limit counted at the limit, is
  repaired until the Kraft sum is exact (drop one code of the limit's length, move one code of the longest shorter length one level
  down next to it: the repair miniz made known); lengths are then dealt out by rank, the rarest symbols the longest codes.  Limit 15 for
  literal/length, 7 for the code-length code.  The distance code has the one symbol 0: length 1 if the chunk has a match, else one
  code of zero bits (RFC 1951, 3.2.7); HDIST is always 0.
* **Code-length sequence.**  Literal/length lengths 0 .. HLIT - 1, then the one distance length.  Zero runs of the literal/length part
  are coded in closed form: 18(138) while 138 or more remain, then 18 (11 ..), 17 (3 .. 10) or 1 - 2 plain zeros.  Symbol 16 (repeat
  the previous length) is never used: on a photo-like chunk neighbouring lengths seldom agree three times, and it costs under 0.3 % of
  a 16 KiB chunk there; zero runs are what matters on masks, where most of the alphabet is unused.
* **Alignment.**  Every chunk but the last ends with an empty stored block (zlib's sync flush), so every chunk begins on a byte; the last
  chunk's block carries BFINAL and is padded with zero bits.

``bound`` is the size no output exceeds: the stored block caps a chunk at its raw size + 10 bytes.
"""
import struct
import zlib
from typing import List, Tuple

import numpy as np

PNG_CHUNK = 16384                # bytes of filtered stream per deflate block; csrc/png.hip: PNG_CHUNK
MAX_PIXELS = 1 << 24
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
COLOUR_TYPE = {1: 0, 3: 2, 4: 6}
FIXED_LENGTHS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


def _shape(a) -> Tuple[int, int, int]:
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (3, 4)) or a.size == 0:
        raise ValueError("png: (H, W), (H, W, 3) or (H, W, 4) uint8, not empty")
    return a.shape[0], a.shape[1], (1 if a.ndim == 2 else a.shape[2])


def n_chunks(H: int, W: int, C: int) -> int:
    return (H * (W * C + 1) + PNG_CHUNK - 1) // PNG_CHUNK


def bound(H: int, W: int, C: int) -> int:
    """upper bound of ``len(encode_reference(a))``: signature 8 + IHDR 25 + IEND 12 + zlib header 2 + Adler-32 4 = 51 bytes per file;
    per chunk the IDAT framing 12 + a stored block 5 + the sync block 5 = 22 bytes on top of its raw bytes.  0: out of range."""
    if H < 1 or W < 1 or H * W > MAX_PIXELS or C not in COLOUR_TYPE:
        return 0
    return H * (W * C + 1) + 22 * n_chunks(H, W, C) + 51


# ---- filters ----------------------------------------------------------------------------------------------------------------------------
def filter_candidates(cur: np.ndarray, up: np.ndarray, bpp: int) -> np.ndarray:
    """rows ``cur`` and ``up`` (the row above; zeros for the first), each (..., W C) uint8 -> (5, ..., W C) uint8: filters 0 .. 4"""
    x = cur.astype(np.int32)
    b = up.astype(np.int32)
    a = np.zeros_like(x)
    a[..., bpp:] = x[..., :-bpp]
    c = np.zeros_like(x)
    c[..., bpp:] = b[..., :-bpp]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]).astype(np.uint8)


def filtered_stream(a: np.ndarray, filter_mode: int = -1) -> np.ndarray:
    """the H (W C + 1) bytes deflate sees: per row the filter id, then the filtered row"""
    H, W, C = _shape(a)
    if not -1 <= filter_mode <= 4:
        raise ValueError("filter_mode: -1 (adaptive) or 0 .. 4")
    rows = np.ascontiguousarray(a).reshape(H, W * C)
    up = np.zeros_like(rows)
    up[1:] = rows[:-1]
    cand = filter_candidates(rows, up, C)                                         # (5, H, WC)
    if filter_mode < 0:
        cost = np.where(cand < 128, cand.astype(np.int64), 256 - cand.astype(np.int64)).sum(2)   # |signed byte|
        pick = np.argmin(cost, axis=0)                                            # the first minimum: ties to the lowest id
    else:
        pick = np.full(H, filter_mode, np.int64)
    out = np.empty((H, W * C + 1), np.uint8)
    out[:, 0] = pick
    out[:, 1:] = cand[pick, np.arange(H)]
    return out.reshape(-1)


# ---- tokens -----------------------------------------------------------------------------------------------------------------------------
def position_tokens(d: np.ndarray):
    """one chunk's bytes -> per position (is_literal, match length or 0): what position p emits, from the start s and end e of its
    run alone - the form the kernel evaluates, one position per step"""
    n = len(d)
    p = np.arange(n)
    start = np.ones(n, bool)
    start[1:] = d[1:] != d[:-1]
    s = np.maximum.accumulate(np.where(start, p, 0))
    nxt = np.minimum.accumulate(np.where(start, p, n)[::-1])[::-1]                # the first run start at or after p
    e = np.concatenate([nxt[1:], [n]])
    k, r = p - s, e - s - 1
    j, q = k - 1, r // 258
    rem = r - q * 258
    full = (k > 0) & (j < q * 258)
    tail = (k > 0) & ~full
    lit = (k == 0) | (tail & (rem < 3))
    length = np.where(full & (j % 258 == 0), 258, np.where(tail & (rem >= 3) & (j == q * 258), rem, 0))
    return lit, length


def chunk_tokens(data) -> List[tuple]:
    """the token list of one chunk: ("lit", byte) / ("match", length), every match at distance 1"""
    d = np.frombuffer(bytes(data), np.uint8)
    lit, length = position_tokens(d)
    return [("lit", int(d[i])) if lit[i] else ("match", int(length[i])) for i in range(len(d)) if lit[i] or length[i]]


def length_symbol(length: np.ndarray):
    """match length 3 .. 258 -> (literal/length symbol, number of extra bits, their value), RFC 1951 3.2.5 in closed form"""
    m = np.asarray(length, np.int64) - 3
    lg = np.zeros_like(m)
    for b in range(1, 8):
        lg[m >= (1 << b)] = b
    eb = np.where(m < 8, 0, lg - 2)
    sym = np.where(m < 8, 257 + m, 261 + 4 * eb + ((m >> eb) & 3))
    ev = m & ((1 << eb) - 1)
    is258 = m == 255
    return np.where(is258, 285, sym), np.where(is258, 0, eb), np.where(is258, 0, ev)


# ---- Huffman ----------------------------------------------------------------------------------------------------------------------------
def code_lengths(counts, limit: int) -> List[int]:
    """length-limited code lengths of the symbols with a count (0 for the others): see the module docstring"""
    order = sorted((int(c), s) for s, c in enumerate(counts) if c > 0)
    n = len(order)
    out = [0] * len(counts)
    if n == 0:
        return out
    if n == 1:
        out[order[0][1]] = 1
        return out
    w = [c for c, _ in order]
    leaf_parent, node_w, node_parent = [0] * n, [0] * (n - 1), [0] * (n - 1)
    i = h = 0
    for k in range(n - 1):
        tot = 0
        for _ in range(2):
            if i < n and (h >= k or w[i] <= node_w[h]):       # a leaf before an internal node of equal weight
                tot += w[i]
                leaf_parent[i] = k
                i += 1
            else:
                tot += node_w[h]
                node_parent[h] = k
                h += 1
        node_w[k] = tot
    depth = [0] * (n - 1)
    for k in range(n - 3, -1, -1):
        depth[k] = depth[node_parent[k]] + 1
    per_len = [0] * (limit + 1)
    for j in range(n):
        per_len[min(depth[leaf_parent[j]] + 1, limit)] += 1
    total = sum(per_len[length] << (limit - length) for length in range(1, limit + 1))
    while total > (1 << limit):
        per_len[limit] -= 1
        for length in range(limit - 1, 0, -1):
            if per_len[length]:
                per_len[length] -= 1
                per_len[length + 1] += 2
                break
        total -= 1
    j = 0
    for length in range(limit, 0, -1):                        # the rarest symbols the longest codes
        for _ in range(per_len[length]):
            out[order[j][1]] = length
            j += 1
    return out


def canonical_codes(lengths) -> List[int]:
    """RFC 1951 3.2.2 codes, BIT-REVERSED: deflate packs a Huffman code from its most significant bit, everything else from the least"""
    limit = max(lengths) if len(lengths) else 0
    per_len = [0] * (limit + 2)
    for length in lengths:
        per_len[length] += 1
    per_len[0] = 0
    nxt, code = [0] * (limit + 2), 0
    for length in range(1, limit + 1):
        code = (code + per_len[length - 1]) << 1
        nxt[length] = code
    out = []
    for length in lengths:
        c = 0
        if length:
            v = nxt[length]
            nxt[length] += 1
            for b in range(length):
                c |= ((v >> b) & 1) << (length - 1 - b)
        out.append(c)
    return out


def code_length_sequence(ll: List[int], hlit: int, dist_len: int) -> List[tuple]:
    """(code-length symbol, extra bits, their value) for literal/length lengths 0 .. hlit - 1, zero runs in closed form, and the one
    distance length"""
    seq, i = [], 0
    while i < hlit:
        if ll[i]:
            seq.append((ll[i], 0, 0))
            i += 1
            continue
        z = i
        while z < hlit and ll[z] == 0:
            z += 1
        z -= i
        i += z
        while z >= 138:
            seq.append((18, 7, 127))
            z -= 138
        if z >= 11:
            seq.append((18, 7, z - 11))
        elif z >= 3:
            seq.append((17, 3, z - 3))
        else:
            seq += [(0, 0, 0)] * z
    seq.append((dist_len, 0, 0))
    return seq


def _pack(vals: np.ndarray, nbits: np.ndarray) -> Tuple[bytes, int]:
    """fields, least significant bit first, back to back from bit 0 -> (bytes, zero-padded; number of bits)"""
    width = 32
    bits = ((vals.astype(np.uint64)[:, None] >> np.arange(width, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
    stream = bits[np.arange(width)[None] < nbits[:, None]]
    return np.packbits(stream, bitorder="little").tobytes(), int(nbits.sum())


def deflate_chunk(d: np.ndarray, last: bool) -> Tuple[bytes, int]:
    """one chunk of the filtered stream -> (its deflate bytes, whole bytes: the block and, unless ``last``, the sync block; the block
    type chosen: 0 stored, 1 fixed, 2 dynamic)"""
    n = len(d)
    lit, length = position_tokens(d)
    is_match = length > 0
    emit = lit | is_match
    lsym, leb, lev = length_symbol(np.where(is_match, length, 3))
    sym = np.where(lit, d.astype(np.int64), lsym)[emit]
    eb = np.where(lit, 0, leb)[emit]
    ev = np.where(lit, 0, lev)[emit]
    mt = is_match[emit]
    n_match = int(mt.sum())
    counts = np.bincount(sym, minlength=286)
    counts[256] += 1
    extra_bits = int(eb.sum())

    # dynamic
    ll = code_lengths(counts.tolist(), 15)
    dist_len = 1 if n_match else 0
    hlit = max(s for s in range(286) if ll[s]) + 1                              # >= 257: the end-of-block symbol is used
    seq = code_length_sequence(ll, hlit, dist_len)
    cl_counts = [0] * 19
    for s, _, _ in seq:
        cl_counts[s] += 1
    cl = code_lengths(cl_counts, 7)
    hclen = max(4, max(i for i in range(19) if cl[CL_ORDER[i]]) + 1)
    cost_dyn = 3 + 14 + 3 * hclen + sum(cl[s] + e for s, e, _ in seq) + sum(int(counts[s]) * ll[s] for s in range(286)) + extra_bits + n_match * dist_len
    cost_fix = 3 + sum(int(counts[s]) * FIXED_LENGTHS[s] for s in range(286)) + extra_bits + 5 * n_match
    cost_sto = 8 * (5 + n)
    kind = min((cost_sto, 0), (cost_fix, 1), (cost_dyn, 2))[1]

    bfinal = 1 if last else 0
    if kind == 0:
        body, nb = bytes([bfinal]) + struct.pack("<HH", n, n ^ 0xFFFF) + d.tobytes(), cost_sto
    else:
        lens = FIXED_LENGTHS if kind == 1 else ll
        codes = canonical_codes(lens)
        dl = 5 if kind == 1 else dist_len
        head = [(bfinal, 1), (kind, 2)]
        if kind == 2:
            cl_codes = canonical_codes(cl)
            head += [(hlit - 257, 5), (0, 5), (hclen - 4, 4)] + [(cl[CL_ORDER[i]], 3) for i in range(hclen)]
            head += [(cl_codes[s] | (v << cl[s]), cl[s] + e) for s, e, v in seq]
        la, ca = np.asarray(lens, np.int64), np.asarray(codes, np.int64)
        tv = ca[sym] | (ev << la[sym])                                           # code, extra bits, then the distance code 0
        tn = la[sym] + eb + np.where(mt, dl, 0)
        vals = np.concatenate([np.array([v for v, _ in head], np.int64), tv, [codes[256]]])
        nbs = np.concatenate([np.array([b for _, b in head], np.int64), tn, [lens[256]]])
        body, nb = _pack(vals, nbs)
        assert nb == (cost_fix if kind == 1 else cost_dyn), (nb, cost_fix, cost_dyn)
    if not last:                                                                 # sync flush: an empty stored block on a byte boundary
        if nb % 8 == 0 or nb % 8 > 5:                                            # its 3 header bits open another byte
            body += b"\x00"
        body += b"\x00\x00\xff\xff"
    return body, kind


def _png_chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def idat_payloads(a: np.ndarray, filter_mode: int = -1) -> List[bytes]:
    """the data of every IDAT: chunk k's deflate bytes, the zlib header in front of the first, the Adler-32 behind the last"""
    stream = filtered_stream(a, filter_mode)
    cuts = range(0, len(stream), PNG_CHUNK)
    out = [deflate_chunk(stream[o:o + PNG_CHUNK], o + PNG_CHUNK >= len(stream))[0] for o in cuts]
    out[0] = b"\x78\x01" + out[0]
    out[-1] += struct.pack(">I", zlib.adler32(stream.tobytes()))
    return out


def encode_reference(a: np.ndarray, filter_mode: int = -1) -> bytes:
    """the PNG file of ``a``: the definition of what ``sm_png_encode_batch_u8`` writes"""
    H, W, C = _shape(a)
    if H * W > MAX_PIXELS:
        raise ValueError(f"png: {H} x {W} (at most {MAX_PIXELS} pixels)")
    ihdr = struct.pack(">IIBBBBB", W, H, 8, COLOUR_TYPE[C], 0, 0, 0)
    return SIGNATURE + _png_chunk(b"IHDR", ihdr) + b"".join(_png_chunk(b"IDAT", p) for p in idat_payloads(a, filter_mode)) + \
        _png_chunk(b"IEND", b"")
