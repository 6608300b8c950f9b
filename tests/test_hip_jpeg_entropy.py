"""The device's JPEG entropy decoder (csrc/jpeg_entropy.hip) against the host decoder ``sm_jpeg_entropy_decode``, bit for bit in
coefficients and verdict, and against Pillow in pixels: the case matrix in one mixed batch and case by case, at the default and at
the smallest sub-sequence / chunk sizes (many chunks, many synchronisation rounds), inputs chosen to be hard for the scheme, damaged
streams (every one an ordinary flagged image: the kernel's bounds hold, and tests/test_jpeg_entropy_cpu.py has run the same inputs
through the Python model first), mixed batches through ``decode_jpeg_batch(entropy="device")`` and the predictor.  No tolerance."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _jpeg_entropy_ref as E  # noqa: E402
import _jpeg_ref as R  # noqa: E402
from selfmask_amd import MaskFormer, synthetic_state_dict  # noqa: E402
from selfmask_amd import _native as N  # noqa: E402
from selfmask_amd import jpeg as J  # noqa: E402
from selfmask_amd.datasets import synthetic_scene  # noqa: E402
from selfmask_amd.jpeg import decode_jpeg_batch  # noqa: E402
from selfmask_amd.pipeline import packed_pixel_offsets  # noqa: E402
from selfmask_amd.predictor import SaliencyPredictor  # noqa: E402

DEV = "cuda:0"
SMALLEST = N.JPEG_SUBSEQ_BITS_MIN


def device_decode(files, subseq_bits=0, chunk_subseqs=0):
    """files the prepare step takes -> ([status], [int16 coefficients], [(rounds, chunks)]) through sm_jpeg_entropy_decode_batch"""
    lib = N.load()
    B = len(files)
    table = (N.JpegScan * B)()
    recs, r, o = [], 0, 0
    for b, data in enumerate(files):
        rc, info, scan, rec, _ = E.prepare(data)
        assert rc == 0, f"file {b}: the prepare step refuses it ({rc})"
        scan.rec_off, scan.coef_off = r, o
        table[b] = scan
        recs.append(rec[:scan.rec_bytes])
        r += scan.rec_bytes
        o += int(info.coef_bytes)
    scans = torch.from_numpy(np.concatenate(recs)).to(DEV)
    descr = torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).to(DEV)
    coef = torch.full((o // 2,), 0x5A5A, dtype=torch.int16, device=DEV)  # the kernel must leave nothing of this
    status = torch.full((B,), -77, dtype=torch.int32, device=DEV)
    ws = int(lib.sm_jpeg_entropy_workspace_bytes(ctypes.addressof(table), B, subseq_bits, chunk_subseqs))
    assert ws >= 8 * B
    stats = torch.zeros(ws // 4, dtype=torch.int32, device=DEV)
    N.check(lib.sm_jpeg_entropy_decode_batch(ctypes.addressof(table), descr.data_ptr(), B, scans.data_ptr(), coef.data_ptr(), status.data_ptr(),
                                             stats.data_ptr(), ws, subseq_bits, chunk_subseqs, torch.cuda.current_stream().cuda_stream),
            "sm_jpeg_entropy_decode_batch")
    torch.cuda.synchronize()
    coef, stats = coef.cpu().numpy(), stats.cpu().numpy()
    offs = [table[b].coef_off // 2 for b in range(B)] + [o // 2]
    return status.cpu().tolist(), [coef[offs[b]:offs[b + 1]] for b in range(B)], [(int(stats[2 * b]), int(stats[2 * b + 1])) for b in range(B)]


def host_decode(files):
    """-> [(rc, coefficients)] of the host decoder, the reference of every comparison here"""
    out = []
    for d in files:
        rc, info, coef, _ = R.entropy_decode(d)
        out.append((rc, coef))
    return out


def _compare(files, got, ref, names=None):
    status, coefs, _ = got
    bad = []
    for b in range(len(files)):
        rc, want = ref[b]
        ok = status[b] == rc and (np.array_equal(coefs[b], want[:coefs[b].size]) if rc == 0 else not coefs[b].any())
        if not ok:
            bad.append((names[b] if names else b, status[b], rc))
    assert not bad, f"{len(bad)} of {len(files)} files differ from the host decoder (name, status, host code): {bad[:10]}"


@pytest.fixture(scope="module")
def matrix():
    """the cases, the host decoder's coefficients and Pillow's pixels of each (computed once, left unchanged), and the mixed batch of
    all of them at the default parameters, through the C entry point and through decode_jpeg_batch"""
    cases = R.case_matrix()
    files = [d for _, d in cases]
    host = host_decode(files)
    pil = [torch.from_numpy(R.pillow_pixels(d)) for d in files]
    raw = device_decode(files)
    px = decode_jpeg_batch(files, DEV, return_info=True, entropy="device")
    px_host = decode_jpeg_batch(files, DEV, return_info=True)
    torch.cuda.synchronize()
    return {"cases": cases, "files": files, "host": host, "pil": pil, "raw": raw, "px": (px[0].cpu(),) + tuple(px[1:]),
            "px_host": (px_host[0].cpu(),) + tuple(px_host[1:])}


def _slot(pixels, shapes, offs, b):
    h, w = shapes[b]
    return pixels[offs[b]:offs[b] + h * w * 3].view(h, w, 3)


def test_mixed_batch_at_the_defaults_equals_the_host_decoder_and_pillow(matrix):
    names = [c for c, _ in matrix["cases"]]
    assert all(rc == 0 for rc, _ in matrix["host"])
    assert matrix["raw"][0] == [0] * len(names)
    _compare(matrix["files"], matrix["raw"], matrix["host"], names)
    pixels, shapes, offs, flags = matrix["px"]
    assert flags == ["device"] * len(names), "a fallback must not hide a failure"
    assert offs == packed_pixel_offsets(shapes) and shapes == [tuple(r.shape[:2]) for r in matrix["pil"]]
    assert matrix["px_host"][1:] == (shapes, offs, flags)
    bad = [names[b] for b in range(len(names)) if not torch.equal(_slot(pixels, shapes, offs, b), matrix["pil"][b])]
    assert not bad, f"{len(bad)} cases differ from Pillow: {bad[:12]}"
    bad = [names[b] for b in range(len(names)) if not torch.equal(_slot(pixels, shapes, offs, b), _slot(matrix["px_host"][0], shapes, offs, b))]
    assert not bad, f"{len(bad)} cases differ from entropy='host': {bad[:12]}"


def test_every_case_alone_equals_its_batch_result(matrix):
    bad = []
    for b, (cid, data) in enumerate(matrix["cases"]):
        status, coefs, _ = device_decode([data])
        if status != [0] or not np.array_equal(coefs[0], matrix["raw"][1][b]):
            bad.append(cid)
    assert not bad, f"{len(bad)} cases differ alone: {bad[:12]}"
    px, shp, off, flag = decode_jpeg_batch([matrix["files"][-1]], DEV, threads=1, return_info=True, entropy="device")
    pixels, shapes, offs, _ = matrix["px"]
    assert flag == ["device"] and torch.equal(_slot(px.cpu(), shp, off, 0), _slot(pixels, shapes, offs, len(shapes) - 1))


@pytest.mark.parametrize("chunk", [4, 8])
def test_smallest_parameters_on_the_matrix(matrix, chunk):
    got = device_decode(matrix["files"], SMALLEST, chunk)
    _compare(matrix["files"], got, matrix["host"], [c for c, _ in matrix["cases"]])
    big = max(range(len(matrix["files"])), key=lambda b: len(matrix["files"][b]))
    rounds, chunks = got[2][big]
    assert chunks > 100 and rounds >= chunks, "64-bit sub-sequences, a few at a time, must give many chunks and rounds"


def test_hard_inputs_at_the_smallest_and_the_default_parameters():
    hard = E.hard_files()
    names, files = list(hard), list(hard.values())
    host = host_decode(files)
    assert all(rc == 0 for rc, _ in host)
    for params in ((0, 0), (SMALLEST, 4), (SMALLEST, 8), (SMALLEST, 0), (96, 5)):
        got = device_decode(files, *params)
        _compare(files, got, host, names)
        if params == (SMALLEST, 4):  # the kernel took the rounds and chunks the Python model of it takes
            for name in ("flat-64x48-444", "flat-64x48-420", "noise-17x17-420-rst1", "flat-256x256-420"):
                m = E.model_decode(hard[name], *params)[3]
                assert got[2][names.index(name)] == (m.rounds, m.chunks), name
        if params == (SMALLEST, 0):  # long codes in 64-bit sub-sequences: hundreds of rounds inside one chunk, the model's number
            m = E.model_decode(hard["noise-64x48-q100-444"], *params)[3]
            assert got[2][names.index("noise-64x48-q100-444")] == (m.rounds, m.chunks) and m.rounds > 100 * m.chunks
    pixels, shapes, offs, flags = decode_jpeg_batch(files, DEV, return_info=True, entropy="device")
    assert flags == ["device"] * len(files)
    pixels = pixels.cpu()
    for b, d in enumerate(files):
        assert torch.equal(_slot(pixels, shapes, offs, b), torch.from_numpy(R.pillow_pixels(d))), names[b]


def test_a_scan_of_several_chunks_at_the_defaults():
    data = E.multi_chunk_file()
    host = host_decode([data])
    assert host[0][0] == 0
    got = device_decode([data])
    assert got[2][0][1] > 1, "more than 128 KiB of scan: more than one chunk"
    _compare([data], got, host)


def test_verdict_on_damaged_streams():
    small = R.encode(R.content("edge", 16, 16, 3), quality=85, subsampling=2)
    files = E.damaged(E.restart_file()) + E.damaged(small) + [R.unsupported_files()["truncated"]]
    taken = [d for d in files if E.prepare(d)[0] == 0]  # the rest never reaches the device: the prepare step's verdict, see the CPU tests
    assert len(taken) > 400
    host = host_decode(taken)
    assert 50 < sum(rc == 0 for rc, _ in host) < len(taken) - 50, "both verdicts must occur"
    for a in range(0, len(taken), 400):
        part = taken[a:a + 400]
        _compare(part, device_decode(part), host[a:a + 400])
        _compare(part, device_decode(part, SMALLEST, 4), host[a:a + 400])


def test_flagged_and_refused_files_fall_back_and_leave_their_neighbours_alone(matrix, tmp_path):
    un = R.unsupported_files()
    # a stream the device flags and Pillow still decodes: a damaged scan byte that the host decoder refuses too
    small = R.encode(R.content("edge", 16, 16, 3), quality=85, subsampling=2)
    flagged = None
    for d in E.damaged(small):
        if E.prepare(d)[0] == 0 and R.entropy_decode(d)[0] != 0:
            try:
                R.pillow_pixels(d)
            except Exception:
                continue
            flagged = d
            break
    assert flagged is not None
    keep = [d for cid, d in matrix["cases"] if cid.startswith(("37x53", "17x17"))][::5]
    path = tmp_path / "from_a_path.jpg"
    path.write_bytes(keep[0])
    cut = tmp_path / "cut.jpg"
    cut.write_bytes(un["truncated"])
    sources = [str(path), un["progressive"], keep[1], str(cut), flagged, un["cmyk"], keep[2]]
    expect = ["device", "fallback", "device", "fallback", "fallback", "fallback", "device"]
    ref = [torch.from_numpy(R.pillow_pixels(d)) for d in (keep[0], un["progressive"], keep[1], un["truncated"], flagged, un["cmyk"], keep[2])]
    hb = J.HostBatch(sources, 2, entropy="device")
    assert hb.flags == ["device", "fallback", "device", "device", "device", "fallback", "device"], "the scans' verdicts come from the device"
    pixels = hb.to_device(DEV)
    shapes, offs, flags = hb.shapes, hb.offsets, hb.flags
    assert flags == expect and offs == packed_pixel_offsets(shapes)
    again = decode_jpeg_batch(sources, DEV, return_info=True)
    assert again[1:] == (shapes, offs, expect)
    pixels, again = pixels.cpu(), again[0].cpu()
    for b in range(len(sources)):
        assert torch.equal(_slot(pixels, shapes, offs, b), ref[b]) and torch.equal(_slot(again, shapes, offs, b), ref[b]), (b, flags[b])
    with pytest.raises(OSError):  # a file Pillow refuses (cut, no EOI) is refused by the batch as well: Pillow decides
        decode_jpeg_batch([keep[0], keep[1][:-40]], DEV, entropy="device")


def test_host_batch_with_device_entropy_stages_records_not_coefficients():
    """the host half of entropy="device" (its page-locked staging buffer needs the device's runtime): records, tables and both
    descriptor tables in one buffer; header-refused files are Pillow's on the thread as before"""
    files = [d for _, d in R.case_matrix()[-8:]] + [R.unsupported_files()["progressive"]]
    hb = J.HostBatch(files, 2, entropy="device")
    ref = J.HostBatch(files, 2)
    try:
        assert hb.flags == ref.flags == ["device"] * 8 + ["fallback"] and hb.shapes == ref.shapes and hb.offsets == ref.offsets
        assert hb.n_device == 8 and hb.device_slots == list(range(8)) and hb.coef_bytes == ref.coef_bytes
        st = hb.staging.numpy()
        assert bytes(hb.table) == bytes(ref.table), "the back half's descriptors do not depend on who decodes the scans"
        assert bytes(st[hb.descr_at:hb.descr_at + 8 * 64]) == bytes(hb.table)[:8 * 64] and ctypes.sizeof(N.JpegImage) == 64
        scans = (N.JpegScan * 8).from_buffer_copy(bytes(st[hb.scan_at:hb.scan_at + 8 * 160]))
        for k, sc in enumerate(scans):
            rc, _, want, rec, _ = E.prepare(files[k])
            assert rc == 0 and sc.rec_off % 16 == 0 and sc.coef_off == ref.table[k].coef_off
            assert bytes(st[sc.rec_off:sc.rec_off + sc.rec_bytes]) == bytes(rec[:want.rec_bytes])
            m = E.Model(sc, st[sc.rec_off:sc.rec_off + sc.rec_bytes])
            assert m.decode() == 0
            host = ref.staging.numpy()[sc.coef_off:sc.coef_off + m.coef.nbytes].view(np.int16)
            assert np.array_equal(m.coef, host)
            nq = 128 * sc.components  # the tables of the back half, where the host decoder puts them
            assert bytes(st[hb.qt_at + 384 * k:hb.qt_at + 384 * k + nq]) == bytes(ref.staging.numpy()[ref.qt_at + 384 * k:ref.qt_at + 384 * k + nq])
        with pytest.raises(RuntimeError, match="HIP device"):
            hb.to_device("cpu")
    finally:
        hb.discard()
        ref.discard()


def test_predictor_with_device_entropy_returns_the_host_decode_results(tmp_path):
    from PIL import Image
    rng = np.random.Generator(np.random.PCG64(33))
    files = []
    for i in range(12):
        h, w = [(150, 230), (180, 200), (161, 239)][i % 3]
        rgb, _ = synthetic_scene(rng, h, w)
        p = os.path.join(str(tmp_path), f"img{i:02d}.jpg")
        Image.fromarray(rgb).save(p, quality=90, subsampling=i % 3)
        files.append(p)
    model = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    model.load_state_dict(synthetic_state_dict(4, "calib", patch_size=16), strict=True)
    model = model.to(DEV).eval()
    host = SaliencyPredictor(model, device=DEV, batch_size=4, workers=2, decode="host")
    dev = SaliencyPredictor(model, device=DEV, batch_size=4, workers=2, decode="device", entropy="device")
    for output in ("rle", "binary"):
        a, b = host(files, output=output), dev(files, output=output)
        assert list(a) == list(b) == [os.path.basename(p) for p in files]
        assert host.last_best == dev.last_best
        for n in a:
            if output == "rle":
                assert a[n] == b[n], n
            else:
                assert a[n].dtype == b[n].dtype and a[n].shape == b[n].shape and a[n].tobytes() == b[n].tobytes(), n
