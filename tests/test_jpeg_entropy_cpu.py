"""The device's JPEG entropy decoder, without a GPU: the prepare step (markers + byte stuffing, the only new host code that reads
untrusted bytes) against a byte-wise restatement, and the device ALGORITHM - restated in plain Python in tests/_jpeg_entropy_ref.py -
against the host decoder ``sm_jpeg_entropy_decode``, coefficient for coefficient and verdict for verdict, before any kernel runs."""
import ctypes
import os
import re

import numpy as np
import pytest

import _jpeg_entropy_ref as E
import _jpeg_ref as R
from selfmask_amd import _native as N
from selfmask_amd import jpeg as J

CASES = R.case_matrix()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALLEST = (N.JPEG_SUBSEQ_BITS_MIN, 4)  # 64-bit sub-sequences, four at a time: many chunks and rounds on 64 x 48 images


def _same_as_host(data, subseq_bits, chunk_subseqs):
    rc, info, coef, qt = R.entropy_decode(data)
    st, c2, qt2, m = E.model_decode(data, subseq_bits, chunk_subseqs)
    assert st == rc, f"verdict {st}, the host decoder's {rc}"
    if m is not None:
        assert c2.dtype == np.int16 and c2.nbytes == info.coef_bytes
        if rc == 0:
            assert np.array_equal(c2, coef[:c2.size]), f"{int((c2 != coef[:c2.size]).sum())} coefficients differ"
            assert np.array_equal(qt2, qt)
        else:
            assert not c2.any(), "a flagged image's coefficients are zero"
    return rc, m


@pytest.mark.parametrize("params", [(0, 0), SMALLEST], ids=["default", "smallest"])
def test_the_device_algorithm_restated_in_python_equals_the_host_decoder(params):
    rounds = 0
    for cid, data in CASES:
        rc, m = _same_as_host(data, *params)
        assert rc == 0 and m is not None, cid
        rounds += m.rounds
    if params == SMALLEST:
        assert rounds > 10 * len(CASES), "the smallest parameters must force synchronisation rounds"


@pytest.mark.parametrize("name", sorted(E.hard_files()))
def test_hard_inputs_in_python(name):
    data = E.hard_files()[name]
    for params in ((0, 0), SMALLEST) if len(data) < 20000 else ((0, 0), (256, 8)):
        rc, m = _same_as_host(data, *params)
        assert rc == 0, name


def test_verdict_on_damaged_streams_in_python():
    """what tests/test_hip_jpeg_entropy.py gives the kernel, through the model first: every scan byte set to 00, to FF and XORed
    with 0x10, and a file cut mid-scan and closed with EOI"""
    small = R.encode(R.content("edge", 16, 16, 3), quality=85, subsampling=2)
    files = E.damaged(E.restart_file()) + E.damaged(small) + [R.unsupported_files()["truncated"]]
    ok = flagged = 0
    for data in files:
        rc, m = _same_as_host(data, *SMALLEST)
        ok += rc == 0
        flagged += rc != 0 and m is not None
    assert ok > 50 and flagged > 50, "both verdicts must occur, and the decoder itself (not only the prepare step) must flag files"


def test_prepare_against_a_bytewise_restatement():
    lib = N.load()
    for cid, data in CASES + sorted(E.hard_files().items()):
        rc, info, scan, rec, qt = E.prepare(data)
        assert rc == 0 and info.supported == 1, cid
        rc0, info0, _, qt0 = R.entropy_decode(data)
        assert bytes(info) == bytes(info0) and np.array_equal(qt, qt0), cid
        assert np.array_equal(rec[scan.qt_off:scan.qt_off + 384].view(np.uint16).reshape(3, 64), qt0), cid
        want = E.unstuff(data, E.scan_start(data), scan.n_seg)
        assert want is not None, cid
        assert bytes(rec[scan.scan_off:scan.scan_off + scan.scan_len]) == want[0], cid
        assert not rec[scan.scan_off + scan.scan_len:scan.rec_bytes].any() and scan.rec_bytes >= scan.scan_off + scan.scan_len + 8, cid
        segs = (N.JpegSegment * scan.n_seg).from_buffer_copy(bytes(rec[scan.seg_off:scan.seg_off + 16 * scan.n_seg]))
        assert [(s.byte_off, s.byte_len) for s in segs] == want[1], cid
        n_mcu, ri = info.mcus_x * info.mcus_y, info.restart_interval or info.mcus_x * info.mcus_y
        assert [(s.mcu0, s.mcus) for s in segs] == [(k, min(ri, n_mcu - k)) for k in range(0, n_mcu, ri)], cid
        assert scan.rec_bytes <= lib.sm_jpeg_scan_bound(info, len(data)) and scan.rec_bytes % 16 == 0, cid
        assert (scan.components, scan.mcus_x, scan.mcus_y, scan.restart_interval) == (info.components, info.mcus_x, info.mcus_y, info.restart_interval)
        for c in range(info.components):
            assert (scan.h[c], scan.v[c], scan.blocks_w[c], scan.blocks_h[c]) == (info.h_samp[c], info.v_samp[c], info.blocks_w[c], info.blocks_h[c])
            assert 0 <= scan.dc[c] < scan.n_huff and 0 <= scan.ac[c] < scan.n_huff and scan.dc[c] != scan.ac[c]
    assert any(b"\xff\x00" in d[E.scan_start(d):] for _, d in CASES), "the matrix must hold stuffed bytes"


def test_prepare_fill_bytes_wrong_markers_and_trailing_bytes():
    """0xFF fill bytes in front of RSTn / EOI are tolerated, a wrong or missing marker is not; bytes behind EOI are not looked at -
    each exactly as the host decoder decides"""
    data = E.restart_file()
    a = E.scan_start(data)
    at = data.index(b"\xff\xd0", a)
    variants = {
        "fill before RST0": data[:at] + b"\xff\xff" + data[at:],
        "fill before EOI": data[:-2] + b"\xff\xff\xff" + data[-2:],
        "RST1 in place of RST0": data[:at + 1] + b"\xd1" + data[at + 2:],
        "RST0 removed": data[:at] + data[at + 2:],
        "no EOI": data[:-2],
        "EOI twice": data + b"\xff\xd9",
        "bytes behind EOI": data + b"garbage",
        "a COM marker inside the scan": data[:at] + b"\xff\xfe\x00\x02" + data[at:],
        "lone FF at the end": data[:-1],
    }
    seen = set()
    for name, d in variants.items():
        rc0 = R.entropy_decode(d)[0]
        rc, info, scan, rec, _ = E.prepare(d)
        assert rc == rc0, f"{name}: prepare says {rc}, the host decoder {rc0}"
        assert info.supported == (rc == 0), name
        if rc == 0:
            assert E.model_decode(d, *SMALLEST)[0] == 0, name
        seen.add(rc)
    assert seen == {0, N.JPEG_UNSUPPORTED}


def test_prepare_refuses_what_the_header_stage_refuses_and_reports_errors():
    lib = N.load()
    for name, data in R.unsupported_files().items():
        probe = N.JpegInfo()
        assert lib.sm_jpeg_probe(data, len(data), probe) == 0
        rc, info, scan, rec, _ = E.prepare(data, cap=1 << 16)
        if name == "truncated":  # a sound header and sound markers: passed on, the decode itself finds the scan short
            assert probe.supported == 1 and rc == 0 and info.supported == 1
            assert E.model_decode(data)[0] == N.JPEG_UNSUPPORTED == R.entropy_decode(data)[0]
        else:
            assert probe.supported == 0 and rc == N.JPEG_UNSUPPORTED and info.supported == 0, name
            assert (info.width, info.height, info.components) == (probe.width, probe.height, probe.components), name
    data = CASES[-1][1]
    rc, info, scan, rec, _ = E.prepare(data)
    assert rc == 0
    for cap in (0, 16, scan.scan_off, scan.rec_bytes - 16):
        rc2, _, _, rec2, _ = E.prepare(data, cap=cap)
        assert rc2 == -3 and b"sm_jpeg_scan_prepare" in lib.sm_last_error(), cap
    out, sc, buf = N.JpegInfo(), N.JpegScan(), np.zeros(4096, np.uint8)
    assert lib.sm_jpeg_scan_prepare(None, 0, buf.ctypes.data, 4096, sc, None, out) == -1 and b"null pointer" in lib.sm_last_error()
    assert lib.sm_jpeg_scan_prepare(data, len(data), None, 4096, sc, None, out) == -1 and b"null pointer" in lib.sm_last_error()
    assert lib.sm_jpeg_scan_prepare(data, len(data), buf.ctypes.data, 4096, None, None, out) == -1
    assert lib.sm_jpeg_scan_bound(None, 10) == 0 and b"null pointer" in lib.sm_last_error()
    # the decode call validates before it launches: no GPU is touched by a refused call
    assert lib.sm_jpeg_entropy_decode_batch(None, None, 1, None, None, None, None, 0, 0, 0, None) == -1 and b"null pointer" in lib.sm_last_error()
    table = (N.JpegScan * 1)(scan)
    for sb, cs in ((32, 0), (65, 0), (1 << 17, 0), (0, 1025), (0, -1)):
        assert lib.sm_jpeg_entropy_workspace_bytes(ctypes.addressof(table), 1, sb, cs) == 0, (sb, cs)
        assert lib.sm_jpeg_entropy_decode_batch(ctypes.addressof(table), 16, 1, 16, 16, 16, 16, 64, sb, cs, None) == -1, (sb, cs)
        assert b"subseq_bits" in lib.sm_last_error()
    assert lib.sm_jpeg_entropy_workspace_bytes(ctypes.addressof(table), 1, 0, 0) >= 8
    assert lib.sm_jpeg_entropy_decode_batch(ctypes.addressof(table), 16, 1, 16, 16, 16, 16, 0, 0, 0, None) == -3
    table[0].n_seg += 1
    assert lib.sm_jpeg_entropy_decode_batch(ctypes.addressof(table), 16, 1, 16, 16, 16, 16, 64, 0, 0, None) == -1 and b"n_seg" in lib.sm_last_error()


def test_every_truncation_of_the_restart_file_is_unsupported_or_the_host_decoders_verdict():
    data = E.restart_file()
    assert R.entropy_decode(data)[0] == 0 and R.entropy_decode(data)[1].restart_interval == 1
    for n in range(len(data)):
        rc, info, scan, rec, _ = E.prepare(data[:n])
        assert rc == N.JPEG_UNSUPPORTED or (rc == 0 and E.model_decode(data[:n], *SMALLEST)[0] == R.entropy_decode(data[:n])[0]), n
    assert E.prepare(data)[0] == 0


def test_symbols_are_declared_bound_and_exported_and_structs_have_the_c_sizes():
    header = open(os.path.join(ROOT, "include", "selfmask_hip.h")).read()
    assert N.JpegScan.scan_off.offset == 16 and N.JpegScan.components.offset == 48 and N.JpegScan.ta.offset == 148
    for macro, value in (("SM_JPEG_HUFF_BYTES", N.JPEG_HUFF_BYTES), ("SM_JPEG_SUBSEQ_BITS_MIN", N.JPEG_SUBSEQ_BITS_MIN),
                         ("SM_JPEG_SUBSEQ_BITS_DEFAULT", N.JPEG_SUBSEQ_BITS_DEFAULT), ("SM_JPEG_CHUNK_SUBSEQS_MAX", N.JPEG_CHUNK_SUBSEQS_MAX)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro
    assert N.JPEG_SUBSEQ_BITS_MIN >= 16 + 11, "a sub-sequence holds at least the longest symbol"
    # the struct as C lays it out: the prepare step's own numbers land in the mirrored fields
    rc, info, scan, rec, _ = E.prepare(CASES[0][1])
    assert rc == 0 and scan.seg_off == 0 and scan.n_seg == 1 and scan.huff_off == 16 and scan.qt_off % 16 == 0 and scan.scan_off == scan.qt_off + 384
    assert '"jpeg_entropy.hip"' in open(os.path.join(ROOT, "salient-object-detection_amd", "build.py")).read()


def test_entropy_option_is_validated():
    from selfmask_amd.predictor import SaliencyPredictor, build_parser
    with pytest.raises(ValueError, match="entropy="):
        J.HostBatch([CASES[0][1]], 1, entropy="gpu")
    with pytest.raises(ValueError, match="entropy="):
        J.decode_jpeg_batch([CASES[0][1]], "cpu", entropy="auto")
    with pytest.raises(ValueError, match=r"entropy='device'.*decode='host'"):
        SaliencyPredictor(object(), device="cuda:0", decode="host", entropy="device")
    with pytest.raises(ValueError, match="entropy="):
        SaliencyPredictor(object(), device="cuda:0", decode="device", entropy="gpu")
    with pytest.raises(ValueError, match="decode="):
        SaliencyPredictor(object(), device="cuda:0", decode="gpu", entropy="device")
    base = ["--config", "c", "--p_state_dict", "s", "--images", "i", "--out", "o"]
    assert build_parser().parse_args(base).entropy == "host"
    assert build_parser().parse_args(base + ["--decode", "device", "--entropy", "device"]).entropy == "device"
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--entropy", "gpu"])


def _dht_tables(data):
    """{(class, id): (counts[16], symbols)} from the file's DHT segments, read here byte by byte"""
    tables, pos = {}, 2
    while data[pos + 1] != 0xDA:
        length = (data[pos + 2] << 8) | data[pos + 3]
        if data[pos + 1] == 0xC4:
            o, end = pos + 4, pos + 2 + length
            while o < end:
                counts = list(data[o + 1:o + 17])
                tables[(data[o] >> 4, data[o] & 15)] = (counts, list(data[o + 17:o + 17 + sum(counts)]))
                o += 17 + sum(counts)
        pos += 2 + length
    return tables


def test_the_one_symbol_lookup_equals_a_canonical_code_decode_on_every_16_bit_prefix():
    """The table walk that the host decoder and the kernel share (jpeg_host.h's huff_lookup, restated as ``_Huff.symbol`` on the very
    table bytes the library builds and sends) against a decode that knows no tables: the canonical code of T.81 Annex C laid out over
    all 65 536 sixteen-bit prefixes, straight from the file's DHT segments.  Every table of a grey, a 4:2:0 and a restart-interval file."""
    cases = dict(CASES)
    long_codes = no_code = tables = 0
    for cid in ("37x53-sL-q85-optimize", "37x53-s2-q85-optimize", "37x53-s0-q85-restart"):
        data = cases[cid]
        rc, info, scan, rec, _ = E.prepare(data)
        assert rc == 0 and (info.components, info.sampling, info.restart_interval > 0) == {"L": (1, N.JPEG_GRAY, False), "2": (3, N.JPEG_420, False),
                                                                                         "0": (3, N.JPEG_444, True)}[cid[7]], cid
        dht = _dht_tables(data)
        slots = {}
        for c in range(info.components):
            slots[scan.dc[c]], slots[scan.ac[c]] = (0, scan.td[c]), (1, scan.ta[c])
        assert sorted(slots) == list(range(scan.n_huff)), cid
        for slot, key in slots.items():
            counts, symbols = dht[key]
            want_len, want_sym = np.zeros(1 << 16, np.int64), np.zeros(1 << 16, np.int64)
            code = k = 0
            for length in range(1, 17):  # C.2: codes of a length are consecutive, the first one follows the last shorter one, doubled
                for _ in range(counts[length - 1]):
                    a = code << (16 - length)
                    assert not want_len[a:a + (1 << (16 - length))].any(), "a prefix code"
                    want_len[a:a + (1 << (16 - length))], want_sym[a:a + (1 << (16 - length))] = length, symbols[k]
                    code, k = code + 1, k + 1
                code <<= 1
            huff = E._Huff(rec[scan.huff_off + N.JPEG_HUFF_BYTES * slot:scan.huff_off + N.JPEG_HUFF_BYTES * (slot + 1)])
            got = np.array([huff.symbol(p << 16) for p in range(1 << 16)], np.int64)
            assert np.array_equal(got[:, 0], want_len) and np.array_equal(got[:, 1], want_sym), (cid, key)
            # the 16 bits behind the prefix never matter
            assert all(huff.symbol((p << 16) | 0xFFFF) == tuple(got[p]) for p in range(0, 1 << 16, 257)), (cid, key)
            long_codes += int((want_len > 9).any())
            no_code += int((want_len == 0).any())
            tables += 1
    assert tables >= 2 + 2 + 2 and long_codes and no_code, "codes behind the fast table and prefixes without a code must both occur"
