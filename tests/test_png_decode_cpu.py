"""CPU checks of the device PNG decode: the Python restatement of the algorithm (tests/_png_decode_ref.py) against Pillow and zlib on
the generated case matrix, what every case exercises, the verdicts on refused and damaged files, the new ABI's host-side validation
(its layout and exports: tests/test_abi_cpu.py), the prepare step against its byte-wise restatement, and the shared bit-level decoder
(csrc/png_inflate.h) compiled for the host against zlib on the corpus."""
import ctypes
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

import _png_decode_cases as C
import _png_decode_ref as R
from selfmask_amd import _native as N

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def decoded():
    """the model's result on every matrix file, computed once"""
    return {name: R.decode(data, "rgb") for name, data in C.case_matrix().items()}


def test_model_equals_pillow_and_zlib_on_the_matrix(decoded):
    for name, data in C.case_matrix().items():
        r = decoded[name]
        assert r.verdict == "ok", (name, r.stats.get("why"))
        assert r.inflated == zlib.decompress(C.idat_stream(data)), name
        for mode in ("rgb", "l", "gt"):
            assert np.array_equal(R.emit(r.unfiltered, mode), C.pillow_pixels(data, mode)), (name, mode)


def test_every_case_exercises_what_its_name_claims(decoded):
    seen_filters, seen_blocks = set(), set()
    for name, want in C.EXPECT.items():
        s = decoded[name].stats
        blocks = {k for k in range(3) if s["blocks"][k]}
        seen_filters |= s["filters"]
        seen_blocks |= blocks
        if "filters" in want:
            assert s["filters"] == want["filters"], (name, s["filters"])
        if "blocks" in want:
            assert want["blocks"] <= blocks and (len(want["blocks"]) > 1 or blocks == want["blocks"]), (name, s["blocks"])
        if "min_blocks" in want:
            assert sum(s["blocks"]) >= want["min_blocks"], (name, s["blocks"])
        if "min_code_len" in want:
            assert s["max_code_len"] >= want["min_code_len"], (name, s["max_code_len"])
        if "max_dist" in want:
            assert s["max_dist"] == want["max_dist"], (name, s["max_dist"])
        if "max_len" in want:
            assert s["max_len"] == want["max_len"], (name, s["max_len"])
        if want.get("overlaps"):
            assert s["overlaps"] > 0, name
        if want.get("cross_block_match"):
            assert s["cross_block_matches"] > 0, name
        if "dist_codes" in want:
            assert s["dist_codes"] == want["dist_codes"], (name, s["dist_codes"])
        if "matches" in want:
            assert s["matches"] == want["matches"], (name, s["matches"])
        data = C.case_matrix()[name]
        if "idats" in want:
            assert data.count(b"IDAT") == want["idats"], (name, data.count(b"IDAT"))
        if "cuts_in_first_header" in want:  # IDAT borders (offsets in the zlib stream, 2 header bytes in front of the data) inside block 1's header
            assert all(0 < 8 * (c - 2) < s["header_end_bits"][0] for c in want["cuts_in_first_header"]), (name, s["header_end_bits"][:1])
        if "chunks" in want:
            at = [data.index(k) for k in want["chunks"]]
            assert at[0] < data.index(b"IDAT") < at[-1] < data.index(b"IEND") and data.endswith(want["tail"]), name
    assert seen_filters == {0, 1, 2, 3, 4} and seen_blocks == {0, 1, 2}
    # stored blocks of the > 64 KiB case, empty stored blocks of the sync flushes, 1-byte IDATs
    assert decoded["150x150-c3-noise-level0"].stats["blocks"][0] >= 2
    assert len(decoded["150x150-c3-noise-level0"].inflated) > 65536
    assert C.case_matrix()["37x53-c3-idat-1byte"].count(b"IDAT") > 100


def test_ground_truth_rule_cases():
    m = C.case_matrix()
    assert set(np.unique(C.pillow_pixels(m["64x40-c1-gt-255"], "gt"))) == {0, 1}
    assert set(np.unique(C.pillow_pixels(m["64x40-c1-gt-255"], "l"))) == {0, 255}
    assert np.array_equal(C.pillow_pixels(m["64x40-c1-gt-01"], "gt"), C.pillow_pixels(m["64x40-c1-gt-01"], "l"))
    assert C.pillow_pixels(m["64x40-c1-gt-zero"], "gt").max() == 0
    soft = C.pillow_pixels(m["64x40-c1-gt-soft"], "l")
    assert len(np.unique(soft)) > 4 and np.array_equal(C.pillow_pixels(m["64x40-c1-gt-soft"], "gt"), (soft > 0).astype(np.uint8))
    assert C.pillow_pixels(m["9x9-c3-gt-blue1"], "rgb").max() == 1 and C.pillow_pixels(m["9x9-c3-gt-blue1"], "gt").max() == 0


def _native_prepare(data, cap=None):
    lib = N.load()
    info = N.PngInfo()
    N.check(lib.sm_png_probe(data, len(data), info), "sm_png_probe")
    bound = int(lib.sm_png_stream_bound(info, len(data)))
    if not info.supported:
        assert bound == 0
        bound = 16
    cap = bound if cap is None else cap
    guard = 32
    rec = (ctypes.c_uint8 * (cap + guard))(*([0xA5] * (cap + guard)))
    st, out = N.PngStream(), N.PngInfo()
    rc = lib.sm_png_stream_prepare(data, len(data), ctypes.addressof(rec), cap, st, out)
    return rc, bytes(rec), st, out, info


def test_prepare_step_equals_its_restatement():
    files = dict(C.case_matrix())
    files.update(C.refused_files())
    files.update(C.flagged_files())
    n_ok = 0
    for name, data in files.items():
        want = R.prepare(data)
        rc, rec, st, out, info = _native_prepare(data)
        assert bool(info.supported) == want.info.supported, name
        assert (info.height, info.width, info.colour_type, info.bit_depth, info.interlace) == want.info[:5], name
        if want.verdict != "ok":
            assert rc == N.PNG_UNSUPPORTED and not out.supported, (name, rc)
            continue
        n_ok += 1
        assert rc == 0 and out.supported, (name, rc)
        assert (st.data_len, st.rec_bytes, st.adler, st.magic) == (want.data_len, len(want.record), want.adler, N.PNG_STREAM_MAGIC), name
        assert (st.H, st.W, st.colour_type, st.bpp, st.inflated_bytes) == (want.info.height, want.info.width, want.info.colour_type, want.info.bpp,
                                                                           want.info.inflated_bytes), name
        assert rec[:st.rec_bytes] == want.record and st.rec_bytes >= st.data_len + 8, name
        assert set(rec[st.rec_bytes:]) == {0xA5}, name  # nothing behind the record
        # a short record: refused, and nothing is written
        rc2, rec2, _, _, _ = _native_prepare(data, cap=st.rec_bytes - 16)
        assert rc2 == -3 and set(rec2) == {0xA5}, name
    assert n_ok >= len(C.case_matrix())


def test_refused_files_are_refused_by_probe_or_prepare():
    for name, data in C.refused_files().items():
        assert R.decode(data).verdict == "unsupported", name
        assert _native_prepare(data)[0] == N.PNG_UNSUPPORTED, name
    from selfmask_amd.png_decode import probe_png
    for name in ("palette", "1bit", "16bit", "interlaced", "jpeg"):
        assert not probe_png(C.refused_files()[name]).supported, name
    h = probe_png(C.case_matrix()["37x53-c4-photo-cycle"])
    assert h == (37, 53, 6, 8, True, 37 * (53 * 4 + 1))


def test_flagged_files_get_the_verdict_flag():
    """every damaged data stream ends in "flag" (a mutant of the zlib header: in "unsupported"); the model is never more lenient
    than zlib"""
    n_flag = 0
    for name, data in C.flagged_files().items():
        r = R.decode(data)
        if name.startswith("mutant-"):
            assert r.verdict in ("flag", "unsupported"), name
        else:
            assert r.verdict == "flag", (name, r.verdict)
        n_flag += r.verdict == "flag"
        try:
            zlib.decompress(C.idat_stream(data))
        except zlib.error:
            assert r.verdict != "ok", name
    assert n_flag >= 40
    mutants = [n for n in C.flagged_files() if n.startswith("mutant-")]
    assert len({n[:9] for n in mutants}) >= 15  # every data byte of the small file


def test_argument_validation_without_gpu():
    lib = N.load()
    assert lib.sm_png_probe(None, 0, None) == -1 and b"null pointer" in lib.sm_last_error()
    assert lib.sm_png_decode_workspace_bytes(None, 1) == 0
    st = (N.PngStream * 1)()
    assert lib.sm_png_decode_batch_u8(ctypes.addressof(st), 16, 1, 16, 16, 64, 16, 16, 0, None) == -1  # not a prepared descriptor
    _, _, good, _, _ = _native_prepare(C.case_matrix()["1x7-c1-noise"])
    st[0] = good
    assert lib.sm_png_decode_workspace_bytes(ctypes.addressof(st), 1) == 16
    assert lib.sm_png_decode_batch_u8(ctypes.addressof(st), 16, 1, 16, 16, 4, 16, 16, 0, None) == -3  # workspace too small
    assert lib.sm_png_decode_batch_u8(ctypes.addressof(st), 16, 1, 16, 16, 64, 16, 16, 3, None) == -1  # mode


def test_shared_decoder_on_the_host_equals_zlib_on_the_corpus(tmp_path):
    """csrc/png_inflate.h is what lane 0 of the kernel runs; scripts/png_host_check.cpp runs it on the host (here without the
    sanitizers: profiles/png_host_check.txt records the sanitized run) and compares verdicts and bytes with zlib's"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "png_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(REPO, "scripts", "png_host_check.cpp"), "-o", str(exe)], check=True)
    subprocess.run([sys.executable, os.path.join(REPO, "scripts", "png_corpus.py"), str(tmp_path / "corpus")], check=True, capture_output=True)
    run = subprocess.run([str(exe), str(tmp_path / "corpus")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1].startswith("ok:"), run.stdout[-2000:]
