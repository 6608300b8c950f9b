"""CPU-only checks of the mixed-size bilateral batch: the host-side workspace sizing and the argument validation of
sm_bilateral_solver_mixed_f64 (all of it runs before any launch).  Exports and the table's layout: tests/test_abi_cpu.py."""
import ctypes

from selfmask_amd import _native as N

SIZES = [(97, 131), (120, 152), (17, 301), (300, 400)]
SIGMAS = (16.0, 16.0, 8.0)


def _table(sizes):
    t = (N.BilateralImage * len(sizes))()
    for e, (h, w) in zip(t, sizes):
        e.H, e.W = h, w
    return t


def test_new_entry_points_are_declared_and_exported():
    import selfmask_amd
    assert callable(selfmask_amd.bilateral_solver_mixed_device)


def test_mixed_workspace_layout():
    lib = N.load()
    t = _table(SIZES)
    total = lib.sm_bilateral_mixed_workspace_bytes(ctypes.addressof(t), len(SIZES), *SIGMAS)
    single = [lib.sm_bilateral_workspace_bytes(h, w, *SIGMAS) for h, w in SIZES]
    assert all(s > 0 for s in single)
    offs = [e.ws_off for e in t]
    assert offs[0] >= 0 and all(o % 256 == 0 for o in offs)
    assert all(b > a for a, b in zip(offs, offs[1:])), offs
    ends = offs[1:] + [total]
    for o, e, s in zip(offs, ends, single):
        assert e - o >= s, (o, e, s)
    assert total >= sum(single)
    # H, W and the caller's other offsets are left alone
    assert [(e.H, e.W) for e in t] == SIZES and all(e.img_off == 0 and e.px_off == 0 for e in t)


def test_mixed_workspace_rejects_what_the_lattice_cannot_take():
    lib = N.load()
    for bad in ((0, 131), (97, -3)):
        t = _table([SIZES[0], bad, SIZES[1]])
        assert lib.sm_bilateral_mixed_workspace_bytes(ctypes.addressof(t), 3, *SIGMAS) == 0
    t = _table(SIZES)
    assert lib.sm_bilateral_mixed_workspace_bytes(ctypes.addressof(t), len(SIZES), 40.0, 16.0, 8.0) == 0  # 40 x 40 pixels > one workgroup
    assert lib.sm_bilateral_mixed_workspace_bytes(None, 4, *SIGMAS) == 0
    assert lib.sm_bilateral_mixed_workspace_bytes(ctypes.addressof(t), 0, *SIGMAS) == 0


def _args(ws_bytes):
    a = N.BilateralArgs()
    # never dereferenced: every case below is refused on the host, before the first launch
    a.img = a.target = a.soft = a.binary = a.workspace = 256
    a.workspace_bytes = ws_bytes
    a.sigma_spatial, a.sigma_luma, a.sigma_chroma = SIGMAS
    a.lam, a.a_diag_min, a.cg_tol, a.confidence, a.cg_maxiter = 256.0, 1e-5, 1e-5, 0.999, 25
    return a


def test_mixed_solver_validates_on_the_host():
    lib = N.load()
    t = _table(SIZES)
    total = lib.sm_bilateral_mixed_workspace_bytes(ctypes.addressof(t), len(SIZES), *SIGMAS)
    tp, n = ctypes.addressof(t), len(SIZES)

    assert lib.sm_bilateral_solver_mixed_f64(None, tp, tp, n, None) == -1 and b"null pointer" in lib.sm_last_error()
    assert lib.sm_bilateral_solver_mixed_f64(N.BilateralArgs(), tp, tp, n, None) == -1 and b"null pointer" in lib.sm_last_error()
    a = _args(total)
    assert lib.sm_bilateral_solver_mixed_f64(a, None, tp, n, None) == -1 and b"null pointer" in lib.sm_last_error()
    assert lib.sm_bilateral_solver_mixed_f64(a, tp, None, n, None) == -1 and b"null pointer" in lib.sm_last_error()
    assert lib.sm_bilateral_solver_mixed_f64(a, tp, tp, 0, None) == -1 and b"n_images=0" in lib.sm_last_error()
    # a workspace one byte short of the last image's end
    assert lib.sm_bilateral_solver_mixed_f64(_args(total - 1), tp, tp, n, None) == -3 and b"workspace" in lib.sm_last_error()
    # offsets that are misaligned or run into the image before
    t2 = _table(SIZES)
    lib.sm_bilateral_mixed_workspace_bytes(ctypes.addressof(t2), n, *SIGMAS)
    t2[2].ws_off += 8
    assert lib.sm_bilateral_solver_mixed_f64(a, ctypes.addressof(t2), tp, n, None) == -1 and b"ws_off" in lib.sm_last_error()
    t2[2].ws_off = t2[1].ws_off
    assert lib.sm_bilateral_solver_mixed_f64(a, ctypes.addressof(t2), tp, n, None) == -1 and b"ws_off" in lib.sm_last_error()
    # an empty image, a fractional sigma_spatial
    t3 = _table(SIZES)
    lib.sm_bilateral_mixed_workspace_bytes(ctypes.addressof(t3), n, *SIGMAS)
    t3[1].H = 0
    assert lib.sm_bilateral_solver_mixed_f64(a, ctypes.addressof(t3), tp, n, None) == -1 and b"image 1" in lib.sm_last_error()
    a.sigma_spatial = 16.5
    assert lib.sm_bilateral_solver_mixed_f64(a, tp, tp, n, None) == -1 and b"sigma" in lib.sm_last_error()


def test_native_glue_validates_on_the_host():
    lib = N.load()
    assert lib.sm_upsample_selected_native_f64(None, 0, None, 14, None, None, 1, 4, 4, 4.0, 16, None) == -1
    assert lib.sm_upsample_selected_native_f64(256, 0, 256, 13, 256, 256, 1, 4, 4, 4.0, 16, None) == -1  # not a selection column
    assert lib.sm_upsample_selected_native_f64(256, 0, 256, 14, 256, 256, 1, 4, 4, 0.0, 16, None) == -1  # scale-factor mode only
    assert lib.sm_mask_planes_u8_to_f32(None, None, None, 1, 8, 8, 64, None) == -1
