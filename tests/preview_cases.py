"""Shared by the preview tests (tests/test_preview_host.py, tests/test_preview_gpu.py): the
geometry, the random frames and the byte-budget rule of include/at_api.h, restated."""
import numpy as np


def size_ref(w, h, s):
    pw, ph = (w // s) & ~7, (h // s) & ~7
    return pw, ph, (w - pw * s) // 2, (h - ph * s) // 2


def make_frame(fmt, w, h, seed=1):
    r = np.random.RandomState(seed)
    shape = {"bgr8": (h, w, 3), "gray8": (h, w), "yuyv": (h, w, 2)}[fmt]   # yuyv: Y, U and V independent
    return r.randint(0, 256, shape).astype(np.uint8)


def search_ref(encode, quality, max_bytes):
    """The rule of include/at_api.h over encode(q) -> bytes: (bytes or None, quality used,
    encodes run)."""
    runs = []

    def enc(q):
        runs.append(q)
        return encode(q)

    first = enc(quality)
    if max_bytes == 0 or len(first) <= max_bytes:
        return first, quality, len(runs)
    if quality == 1:
        return None, 1, len(runs)
    lo, hi, best = 1, quality - 1, None
    while lo < hi:
        mid = (lo + hi + 1) // 2
        b = enc(mid)
        if len(b) <= max_bytes:
            lo, best = mid, b
        else:
            hi = mid - 1
    if best is None:
        best = enc(1)
        if len(best) > max_bytes:
            return None, 1, len(runs)
    assert len(set(runs)) == len(runs)       # no quality encoded twice
    return best, lo, len(runs)
