"""JPEG streams for the MJPG tests: encoded here with Pillow from synthetic boards
or noise; the expected luma is always Pillow's luma-only decode of the same bytes."""
import io

import numpy as np
from PIL import Image

# name -> Pillow's `subsampling` (None: a single-component stream)
SAMPLINGS = {"444": 0, "422": 1, "420": 2, "gray": None}


def encode(gray, quality, sampling, **extra):
    """`gray` (H, W) uint8, or (H, W, 3) for real chroma, as a JPEG of the named sampling."""
    gray = np.asarray(gray, np.uint8)
    ss = SAMPLINGS[sampling]
    b = io.BytesIO()
    if ss is None:
        Image.fromarray(gray if gray.ndim == 2 else gray[:, :, 1]).save(b, "JPEG", quality=quality, **extra)
    else:
        rgb = gray if gray.ndim == 3 else tinted(gray)
        Image.fromarray(rgb).save(b, "JPEG", quality=quality, subsampling=ss, **extra)
    return b.getvalue()


def tinted(gray):
    """An RGB image with real chroma from a gray one (so the chroma blocks of the
    interleaved scan carry coefficients the decoder has to step over)."""
    g = gray.astype(np.int32)
    h, w = gray.shape
    yy, xx = np.mgrid[0:h, 0:w]
    r = np.clip(g + 40 * np.sin(xx / 9.0), 0, 255)
    b = np.clip(g - 35 * np.cos(yy / 7.0), 0, 255)
    return np.stack([r, g, b], -1).astype(np.uint8)


def pil_luma(jpg):
    im = Image.open(io.BytesIO(jpg))
    im.draft("L", im.size)
    return np.asarray(im.convert("L"))


def board(w, h, seed=766, ntags=2, ids=None, side_range=(40, 72)):
    from ros_vision_amd import synth
    return synth.render_board(w, h, seed=seed, ntags=ntags, ids=ids, side_range=side_range)[0]


def noise(w, h, seed=5):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def segments(jpg):
    """[(marker, start, end)] of the segments in front of the scan data."""
    out, i = [], 2
    while i + 4 <= len(jpg):
        assert jpg[i] == 0xFF
        m, n = jpg[i + 1], jpg[i + 2] * 256 + jpg[i + 3]
        out.append((m, i, i + 2 + n))
        if m == 0xDA:
            break
        i += 2 + n
    return out


def strip_dht(jpg):
    """The same stream without its DHT segments (what many UVC cameras send)."""
    keep, last = [jpg[:2]], 2
    for m, a, b in segments(jpg):
        if m == 0xC4:
            keep.append(jpg[last:a])
            last = b
    keep.append(jpg[last:])
    out = b"".join(keep)
    assert len(out) < len(jpg)
    return out


def dht_tables(jpg):
    """{(class, slot): (bits[16], values)} of the stream's DHT segments."""
    t = {}
    for m, a, b in segments(jpg):
        if m != 0xC4:
            continue
        p = a + 4
        while p < b:
            n = sum(jpg[p + 1:p + 17])
            t[(jpg[p] >> 4, jpg[p] & 15)] = (bytes(jpg[p + 1:p + 17]), bytes(jpg[p + 17:p + 17 + n]))
            p += 17 + n
    return t


def with_avi1_app0(jpg):
    """The stream with the JFIF APP0 replaced by the `AVI1` APP0 and a COM segment, as
    UVC cameras write them."""
    segs = segments(jpg)
    assert segs[0][0] == 0xE0
    app0 = b"\xff\xe0\x00\x10AVI1\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00"
    com = b"\xff\xfe\x00\x07hello"
    return jpg[:2] + app0 + com + jpg[segs[0][2]:]


def truncations(jpg, n=50):
    return [jpg[:int(round(k * len(jpg) / (n + 1.0)))] for k in range(1, n + 1)]


def corruptions(jpg, n=200, seed=11):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        b = bytearray(jpg)
        b[int(rs.randint(2, len(b)))] = int(rs.randint(0, 256))
        out.append(bytes(b))
    return out
