"""Images shared by test_png_cpu.py and test_hip_png.py: name -> a function giving (uint8 array, filter_mode), seeded by the name."""
import zlib

import numpy as np

from selfmask_amd import png
from selfmask_amd import present as P
from _present_cases import make_case

CH = png.PNG_CHUNK


def _rng(name: str):
    return np.random.Generator(np.random.PCG64(zlib.crc32(name.encode())))


def _shaped(flat: np.ndarray, H: int, W: int, C: int) -> np.ndarray:
    return flat.reshape((H, W) if C == 1 else (H, W, C))


def photo(H: int, W: int) -> np.ndarray:
    """smooth plus noise, RGB"""
    rng = _rng(f"photo{H}x{W}")
    y, x = np.mgrid[0:H, 0:W]
    planes = [128 + 100 * np.sin(x / 37.0) * np.cos(y / 51.0), 128 + 90 * np.cos((x + y) / 23.0), (x + 2 * y) / 4.0]
    return np.clip(np.stack([p + rng.normal(0, 4, (H, W)) for p in planes], 2), 0, 255).astype(np.uint8)


def _mixed(H: int, W: int, C: int, name: str) -> np.ndarray:
    """smooth rows, flat stretches and noise side by side: runs of every length, every filter wins somewhere"""
    rng = _rng(name)
    n = H * W * C
    a = (np.arange(n) // 7 % 256).astype(np.uint8)
    cut = sorted(rng.integers(0, n + 1, 8).tolist())
    a[cut[0]:cut[1]] = 17
    a[cut[2]:cut[3]] = rng.integers(0, 256, cut[3] - cut[2], dtype=np.uint8)
    a[cut[4]:cut[5]] = 255
    a[cut[6]:cut[7]] = rng.integers(0, 4, cut[7] - cut[6], dtype=np.uint8) * 60
    return _shaped(a, H, W, C)


def _stream_shape(nbytes: int, C: int):
    """(H, W) whose filtered stream H (W C + 1) has exactly nbytes bytes, the widest such image; None if there is none"""
    for H in range(1, nbytes // 2 + 1):
        if nbytes % H == 0 and (nbytes // H - 1) % C == 0 and nbytes // H > 1:
            return H, (nbytes // H - 1) // C
    return None


def _fibonacci(shifted: bool = False) -> np.ndarray:
    """one chunk, filter 0, byte frequencies 1, 1, 2, 3, ..., 987 (2 583 bytes with the row's filter byte, which is value 0's one byte;
    no three neighbours agree).  With the end-of-block symbol the counts are 1, 1, 1, 2, 3, ...: under png.py's tie rule (a leaf before
    an internal node of equal weight) Huffman pairs them into two interleaved chains, 9 deep, so the limit does not bite on this one.
    ``shifted``: 1, 2, 3, 5, ..., 2584 - with the end-of-block symbol a strict Fibonacci row of 18, one chain 17 deep whatever the tie
    rule, which the 15-bit limit has to repair."""
    fib = [1, 1]
    while len(fib) < (18 if shifted else 16):
        fib.append(fib[-1] + fib[-2])
    if shifted:
        fib = fib[2:]                               # 2, 3, 5, ..., 2584 for values 1 .. 16
        counts = [0] + fib
    else:
        counts = [0] + fib[1:]                      # value 0's one byte is the filter byte in front of the row
    vals = np.repeat(np.arange(len(counts), dtype=np.uint8), counts)
    rng = _rng("fibonacci" + str(shifted))
    rng.shuffle(vals)
    top = len(counts) - 1                           # the most frequent value: spread the others between its bytes, so no run reaches 3
    rest = vals[vals != top]
    out, n_top, k = [], int(counts[top]), 0
    for i in range(len(rest)):
        out.append(rest[i])
        want = (i + 1) * n_top // len(rest)
        while k < want:
            out.append(top)
            k += 1
        # two bytes of the top value in a row at the most: n_top <= 2 len(rest) does not hold for the tail, checked below
    vals = np.array(out, np.uint8)
    for i in range(2, len(vals)):
        if vals[i] == vals[i - 1] == vals[i - 2]:   # what is left: swap with a byte further on that fits in here
            for j in range(len(vals) - 2, 2, -1):
                if abs(i - j) > 2 and vals[j] != vals[i] and vals[i] not in (vals[j - 1], vals[j + 1]) and vals[j] not in (vals[i - 1], vals[min(i + 1, len(vals) - 1)]):
                    vals[i], vals[j] = vals[j], vals[i]
                    break
    assert not ((vals[2:] == vals[1:-1]) & (vals[1:-1] == vals[:-2])).any() and vals[0] != 0
    assert np.bincount(vals, minlength=len(counts)).tolist() == counts
    return vals.reshape(1, -1)


def _all_literals(C: int) -> np.ndarray:
    rng = _rng(f"all_literals{C}")
    n = 40 * 50 * C
    a = np.resize(np.arange(256, dtype=np.uint8), n)
    for o, ln, v in ((300, 2, 5), (700, 3, 6), (1500, 4, 7), (2000 * C // 2, 258, 8), (3000 * C // 2, 600, 9)):
        a[o:o + ln] = v
    a[-260:] = 200
    a[10:200] = rng.integers(0, 256, 190, dtype=np.uint8)
    return _shaped(a, 40, 50, C)


def _present(which: int):
    mask, rgb = make_case(0, "hard")
    return P.present_reference_numpy(mask, rgb)[which]


CASES = {}
for _C in (1, 3, 4):
    for _H, _W in ((1, 1), (1, 7), (17, 23), (5, 300)):
        CASES[f"mixed-{_H}x{_W}x{_C}"] = (lambda H=_H, W=_W, C=_C: (_mixed(H, W, C, f"m{H}x{W}x{C}"), -1))
    for _name, _n in (("chunk", CH), ("chunk-1", CH - 1), ("chunk+1", CH + 1), ("3chunks+5", 3 * CH + 5)):
        _hw = _stream_shape(_n, _C)
        while _hw is None and _name == "3chunks+5":  # no image has that many bytes with this channel count: the next size that one has
            _n += 1
            _hw = _stream_shape(_n, _C)
        if _hw is not None:                         # (H (4 W + 1) is never 2^14: no RGBA image fills one chunk exactly)
            CASES[f"{_name}-x{_C}"] = (lambda hw=_hw, C=_C, name=_name: (_mixed(hw[0], hw[1], C, f"{name}x{C}"), -1))
    CASES[f"zeros-x{_C}"] = (lambda C=_C: (_shaped(np.zeros(130 * 131 * C, np.uint8), 130, 131, C), -1))
    CASES[f"const255-filter0-x{_C}"] = (lambda C=_C: (_shaped(np.full(90 * 200 * C, 255, np.uint8), 90, 200, C), 0))
    CASES[f"noise-x{_C}"] = (lambda C=_C: (_shaped(_rng(f"noise{C}").integers(0, 256, 77 * 91 * C, dtype=np.uint8), 77, 91, C), -1))
    CASES[f"all-literals-x{_C}"] = (lambda C=_C: (_all_literals(C), 0))
    CASES[f"pattern012-filter0-x{_C}"] = (lambda C=_C: (_shaped(np.resize(np.array([0, 1, 2], np.uint8), 30 * 40 * C), 30, 40, C), 0))
    for _m in range(-1, 5):
        CASES[f"gradient-filter{_m}-x{_C}"] = (lambda C=_C, m=_m: (_shaped(((np.arange(64 * 75 * C) // C % 75 * 3 + np.arange(64 * 75 * C) // (75 * C) * 2) % 256)
                                                                           .astype(np.uint8), 64, 75, C), m))
    CASES[f"photo300x400-x{_C}"] = (lambda C=_C: ({1: photo(300, 400)[..., 0].copy(), 3: photo(300, 400),
                                                   4: np.concatenate([photo(300, 400), photo(300, 400)[..., :1]], 2)}[C], -1))
CASES["fibonacci-filter0"] = lambda: (_fibonacci(), 0)
CASES["fibonacci-shifted-filter0"] = lambda: (_fibonacci(True), 0)
CASES["hard-mask"] = lambda: (_present(0), -1)
CASES["hard-heat"] = lambda: (_present(1), -1)
