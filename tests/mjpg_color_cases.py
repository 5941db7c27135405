"""Streams of the MJPG colour tests (host and GPU): `mjpg_cases`' encoder on inputs that
carry real chroma, and the expected image -- Pillow's RGB decode of the same bytes,
channel-reversed to BGR."""
import io
import os

import numpy as np
from PIL import Image

import mjpg_cases as mc

SIZES = [(328, 248), (24, 40)]   # chroma 164 x 124 / 12 x 20 at 4:2:0: no multiples of 8
QUALITIES = [30, 95]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def pil_bgr(jpg):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(jpg)).convert("RGB"))[:, :, ::-1])


def board(w, h):
    return mc.board(w, h, ntags=2 if w > 100 else 1, side_range=(40, 72) if w > 100 else (16, 20))


def tinted_board(w, h):
    return mc.tinted(board(w, h))


def three_tables(img, sampling):
    """A stream whose Y, Cb and Cr each use a quantisation table of their own.  Pillow
    writes it from qtables=[q0, q1, q2] (three DQT tables, Tq = 0, 1, 2 in the SOF0), so
    nothing is patched by hand; the assertion checks that it did."""
    q0 = [3 + (k % 7) for k in range(64)]
    q1 = [5 + (k % 5) for k in range(64)]
    q2 = [9 + 2 * (k % 4) for k in range(64)]
    jpg = mc.encode(img, 75, sampling, qtables=[q0, q1, q2])
    sof = next(a for m, a, _ in mc.segments(jpg) if m == 0xC0)
    assert (jpg[sof + 12], jpg[sof + 15], jpg[sof + 18]) == (0, 1, 2)
    return jpg


def host_cases():
    """name -> (JPEG bytes, the bytes Pillow decodes for the expected image): every
    stream the host colour decode is checked on."""
    c = {}
    for w, h in SIZES:
        img = tinted_board(w, h)
        for s in mc.SAMPLINGS:
            for q in QUALITIES:
                c["%dx%d-%s-q%d" % (w, h, s, q)] = mc.encode(img, q, s)
    w, h = SIZES[0]
    img = tinted_board(w, h)
    for s in ("444", "420"):
        c["noise-%s-q100" % s] = mc.encode(mc.noise(w, h), 100, s)
    c["flat-422-q5"] = mc.encode(np.full((h, w, 3), (93, 140, 31), np.uint8), 5, "422")
    for s in ("422", "420"):
        c["rst-blocks-%s" % s] = mc.encode(img, 75, s, restart_marker_blocks=1)
        c["rst-rows-%s" % s] = mc.encode(img, 75, s, restart_marker_rows=1)
    for s in ("422", "420"):
        c["three-tables-%s" % s] = three_tables(img, s)
    for name in ("colorimage.jpg", "grayimage.jpg"):
        c[name] = open(os.path.join(GOLDEN, name), "rb").read()
    c = {k: (v, v) for k, v in c.items()}
    # a DHT-less stream with the AVI1 APP0 of UVC cameras: the expected image is that of
    # the stream it was made from (as tests/test_mjpg_host.py does for luma)
    full = mc.encode(img, 75, "422")
    c["avi1-nodht-422"] = (mc.with_avi1_app0(mc.strip_dht(full)), full)
    return c
