"""Plain-Python restatement of the device's entropy decoder (csrc/jpeg_entropy.hip) on top of what ``sm_jpeg_scan_prepare`` writes:
sub-sequence decodes from guessed states, synchronisation rounds, prefix sum, write pass, DC scan, block checks - the same states,
the same stopping rules, the same verdict, so tests/test_jpeg_entropy_cpu.py can pin the ALGORITHM against the host decoder
(``sm_jpeg_entropy_decode``) before any kernel runs, and tests/test_hip_jpeg_entropy.py shares its inputs.  Also a byte-wise
restatement of the prepare step itself (``unstuff``)."""
import numpy as np

from selfmask_amd import _native as N

import _jpeg_ref as R

ERR = 0xFFFFFFFF
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
COL_SUM_MAX, BLOCK_SUM_MAX = 5800, 11000  # csrc/jpeg_host.h


def prepare(data: bytes, cap=None):
    """-> (rc, info, scan, record uint8 array, qt uint16 (3, 64)) through the library"""
    lib = N.load()
    info = N.JpegInfo()
    assert lib.sm_jpeg_probe(data, len(data), info) == 0
    if cap is None:
        cap = int(lib.sm_jpeg_scan_bound(info, len(data)))
    raw = np.zeros(cap + 16, np.uint8)
    o = (-raw.ctypes.data) % 16
    rec = raw[o:o + cap]
    qt = np.zeros((3, 64), np.uint16)
    scan, out = N.JpegScan(), N.JpegInfo()
    rc = lib.sm_jpeg_scan_prepare(data, len(data), rec.ctypes.data, cap, scan, qt.ctypes.data, out)
    return rc, out, scan, rec, qt


def scan_start(data: bytes) -> int:
    """first byte behind the SOS header of a well-formed file"""
    pos = 2
    while True:
        assert data[pos] == 0xFF
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        length = (data[pos + 1] << 8) | data[pos + 2]
        pos += 1 + length
        if m == 0xDA:
            return pos


def unstuff(data: bytes, pos: int, n_seg: int):
    """byte by byte: -> (unstuffed bytes, [(offset, length)] per interval), or None where the marker structure is not the expected one"""
    out, segs, start, k = bytearray(), [], 0, 0
    n = len(data)
    while True:
        if pos >= n:
            return None
        b = data[pos]
        if b != 0xFF:
            out.append(b)
            pos += 1
            continue
        if pos + 1 < n and data[pos + 1] == 0x00:
            out.append(0xFF)
            pos += 2
            continue
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos >= n:
            return None
        segs.append((start, len(out) - start))
        if k == n_seg - 1:
            return (bytes(out), segs) if data[pos] == 0xD9 else None
        if data[pos] != 0xD0 + (k & 7):
            return None
        k, start, pos = k + 1, len(out), pos + 1


class _Huff:
    def __init__(self, raw: np.ndarray):
        self.fast = raw[:1024].view(np.uint16).tolist()
        self.maxcode = raw[1024:1092].view(np.int32).tolist()
        self.valoff = raw[1092:1160].view(np.int32).tolist()
        self.vals = raw[1160:1416].tolist()

    def symbol(self, bits):
        e = self.fast[bits >> 23]
        if e:
            return e >> 8, e & 255
        for l in range(10, 17):
            code = bits >> (32 - l)
            if code <= self.maxcode[l]:
                i = code + self.valoff[l]
                if i < 0 or i > 255:
                    break
                return l, self.vals[i]
        return 0, 0


class Model:
    """one image's record, decoded as the kernel's workgroup decodes it"""

    def __init__(self, scan: N.JpegScan, rec: np.ndarray):
        self.sc = sc = scan
        nc = sc.components
        self.huff = [_Huff(rec[sc.huff_off + N.JPEG_HUFF_BYTES * i:sc.huff_off + N.JPEG_HUFF_BYTES * (i + 1)]) for i in range(sc.n_huff)]
        self.qt = rec[sc.qt_off:sc.qt_off + 384].view(np.uint16).reshape(3, 64).astype(np.int64)
        nw = (sc.scan_len + 3) // 4 + 2
        self.bits = int.from_bytes(bytes(rec[sc.scan_off:sc.scan_off + 4 * nw]), "big")  # the padded scan as one number
        self.nbits = 32 * nw
        self.segs = [(s.byte_off, s.byte_len, s.mcu0, s.mcus)
                     for s in (N.JpegSegment * sc.n_seg).from_buffer_copy(bytes(rec[sc.seg_off:sc.seg_off + 16 * sc.n_seg]))]
        self.blk, self.base, o = [], [], 0
        for c in range(nc):
            self.base.append(o)
            o += sc.blocks_w[c] * sc.blocks_h[c] * 64
            for vv in range(sc.v[c]):
                for hh in range(sc.h[c]):
                    self.blk.append((c, vv, hh))
        self.nb = len(self.blk)
        self.coef = np.zeros(o, np.int16)
        self.rounds = self.chunks = 0
        self.flag = False

    def peek32(self, bit):
        """bits behind the padded scan read as zero"""
        sh = self.nbits - bit - 32
        return (self.bits >> sh if sh >= 0 else self.bits << -sh) & 0xFFFFFFFF

    def run(self, st, limit, seg_end, write=False, blk0=0, seg_blocks=0, mcu0=0):
        """je_run: st = [p, bi, z] is updated in place -> (blocks completed, bits behind the interval's last block or -1)"""
        sc, done, tail = self.sc, 0, -1
        if st[0] == ERR:
            return 0, tail
        while st[0] < limit:
            if write and blk0 + done >= seg_blocks:
                break
            p, bi, z = st
            c, vv, hh = self.blk[bi]
            bits = self.peek32(p)
            length, sym = self.huff[sc.dc[c] if z == 0 else sc.ac[c]].symbol(bits)
            bad, store, eob, r = length == 0, False, False, 0
            if z == 0:
                s = sym
                bad = bad or s > 11
                store = True
            else:
                r, s = sym >> 4, sym & 15
                if s == 0:
                    if r == 15:
                        bad = bad or z + 16 > 64
                    elif r != 0:
                        bad = True
                    else:
                        eob = True
                else:
                    bad = bad or z + r > 63 or s > 10
                    store = True
            total = length + s
            if bad or total > seg_end - p:
                st[0] = ERR
                break
            if store:
                z += r
                if write:
                    val = 0
                    if s:
                        raw = ((bits << length) & 0xFFFFFFFF) >> (32 - s)
                        val = raw - (1 << s) + 1 if raw < (1 << (s - 1)) else raw
                    bn = blk0 + done
                    mcu = mcu0 + bn // self.nb
                    my, mx = divmod(mcu, sc.mcus_x)
                    at = self.base[c] + ((my * sc.v[c] + vv) * sc.blocks_w[c] + mx * sc.h[c] + hh) * 64
                    self.coef[at + ZIGZAG[z]] = val
                z += 1
            elif eob:
                z = 64
            else:
                z += 16
            st[0] = p + total
            if z >= 64:
                z = 0
                st[1] = 0 if bi + 1 == self.nb else bi + 1
                done += 1
                if write and blk0 + done == seg_blocks:
                    tail = seg_end - st[0]
            st[2] = z
        return done, tail

    def decode(self, subseq_bits=0, chunk_subseqs=0):
        """-> status (0 / 1); self.coef holds the coefficients (all zero when flagged)"""
        sb = subseq_bits or N.JPEG_SUBSEQ_BITS_DEFAULT
        cs = chunk_subseqs or N.JPEG_CHUNK_SUBSEQS_MAX
        assert sb % 32 == 0 and N.JPEG_SUBSEQ_BITS_MIN <= sb <= 65536 and 1 <= cs <= N.JPEG_CHUNK_SUBSEQS_MAX
        sc = self.sc
        for (boff, blen, mcu0, mcus) in self.segs:
            bit0, seg_end = boff * 8, (boff + blen) * 8
            seg_blocks, nsub = mcus * self.nb, (blen * 8 + sb - 1) // sb
            carry, carry_blocks, seg_tail = [bit0, 0, 0], 0, -1
            for c0 in range(0, nsub, cs):
                n = min(cs, nsub - c0)
                self.chunks += 1
                hi = [min(bit0 + (c0 + t + 1) * sb, seg_end) for t in range(n)]
                # 1: own sub-sequences
                st = [list(carry) if t == 0 else [bit0 + (c0 + t) * sb, 0, 0] for t in range(n)]
                cnt = [self.run(st[t], hi[t], seg_end)[0] for t in range(n)]
                stored = [tuple(s) for s in st]
                active = [t + 1 < n and st[t][0] != ERR for t in range(n)]
                cur = list(range(n))
                # 2: rounds; lane t alone touches sub-sequence cur[t] + 1 in a round, so the order inside a round does not matter
                for _ in range(1, n):
                    for t in range(n):
                        if active[t]:
                            nxt = cur[t] + 1
                            cnt[nxt] = self.run(st[t], hi[nxt], seg_end)[0]
                            if stored[nxt] == tuple(st[t]):
                                active[t] = False
                            else:
                                stored[nxt] = tuple(st[t])
                            cur[t] = nxt
                            if nxt + 1 >= n or st[t][0] == ERR:
                                active[t] = False
                    self.rounds += 1
                    if not any(active):
                        break
                # 3 + 4: prefix sum, write pass from the true entry states
                first = carry_blocks
                for t in range(n):
                    en = list(carry) if t == 0 else list(stored[t - 1])
                    if en[0] != ERR and 0 <= first < seg_blocks:
                        _, tail = self.run(en, hi[t], seg_end, True, first, seg_blocks, mcu0)
                        if en[0] == ERR:
                            self.flag = True
                        if tail >= 0:
                            seg_tail = tail
                    first += cnt[t]
                carry, carry_blocks = list(stored[n - 1]), first
                if carry[0] == ERR or carry_blocks >= seg_blocks:
                    break
            if seg_tail < 0 or seg_tail >= 8:
                self.flag = True
        # DC prediction per component and interval, in the order of the stream
        n_mcu = sc.mcus_x * sc.mcus_y
        ri = sc.restart_interval if 0 < sc.restart_interval < n_mcu else n_mcu
        for c in range(sc.components):
            pred = 0
            for mcu in range(n_mcu):
                if mcu % ri == 0:
                    pred = 0
                my, mx = divmod(mcu, sc.mcus_x)
                for vv in range(sc.v[c]):
                    for hh in range(sc.h[c]):
                        at = self.base[c] + ((my * sc.v[c] + vv) * sc.blocks_w[c] + mx * sc.h[c] + hh) * 64
                        pred += int(self.coef[at])
                        if not -32768 <= pred <= 32767:
                            self.flag = True
                        self.coef[at] = np.int16(((pred + 32768) & 0xFFFF) - 32768)
        # block checks
        for c in range(sc.components):
            n = sc.blocks_w[c] * sc.blocks_h[c]
            v = self.coef[self.base[c]:self.base[c] + n * 64].astype(np.int64).reshape(n, 8, 8) * self.qt[c].reshape(1, 8, 8)
            col = np.abs(v).sum(axis=1)
            if n and (v.min() < -32768 or v.max() > 32767 or col.max() > COL_SUM_MAX or col.sum(axis=1).max() > BLOCK_SUM_MAX):
                self.flag = True
        if self.flag:
            self.coef[:] = 0
        return int(self.flag)


def model_decode(data: bytes, subseq_bits=0, chunk_subseqs=0):
    """-> (status or the prepare step's code, coef, qt, Model or None)"""
    rc, info, scan, rec, qt = prepare(data)
    if rc != 0:
        return rc, None, qt, None
    m = Model(scan, rec)
    return m.decode(subseq_bits, chunk_subseqs), m.coef, qt, m


# ---- inputs chosen to be hard for the scheme (tests/test_hip_jpeg_entropy.py, and the CPU model first) ---------------------------
def hard_files():
    flat = lambda h, w: np.full((h, w, 3), (90, 140, 200), np.uint8)
    return {
        "flat-256x256-420": R.encode(flat(256, 256), quality=85, subsampling=2),  # ~5 bits per block: guesses do not synchronise
        "flat-64x48-444": R.encode(flat(48, 64), quality=85, subsampling=0),
        "flat-64x48-420": R.encode(flat(48, 64), quality=85, subsampling=2),
        "noise-64x48-q100-444": R.encode(R.content("noise", 48, 64, 2001), quality=100, subsampling=0),
        "noise-17x17-420-rst1": R.encode(R.content("noise", 17, 17, 2002), quality=85, subsampling=2, restart_marker_blocks=1),
        "noise-256x192-q95-420": R.encode(R.content("noise", 192, 256, 2003), quality=95, subsampling=2),
    }


def multi_chunk_file():
    """more than one chunk at the default parameters (1024 x 1024 bits = 128 KiB of scan)"""
    return R.encode(R.content("noise", 384, 512, 2004), quality=100, subsampling=0)


def restart_file():
    """the 17 x 17 restart-interval file of tests/test_jpeg_cpu.py"""
    return R.encode(R.content("noise", 17, 17, 9), quality=85, subsampling=2, restart_marker_blocks=1)


def damaged(data: bytes):
    """-> [bytes]: every byte of the scan set to 0x00, to 0xFF, and XORed with 0x10, one file each"""
    a, out = scan_start(data), []
    for i in range(a, len(data) - 2):
        for v in (0x00, 0xFF, data[i] ^ 0x10):
            if v != data[i]:
                d = bytearray(data)
                d[i] = v
                out.append(bytes(d))
    return out
