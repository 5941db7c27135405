"""Images and helpers of the JPEG output tests.  The reference everywhere is Pillow
(libjpeg-turbo) saving the same RGB image with one restart interval per MCU row."""
import io

import numpy as np
from PIL import Image

# name -> (the ABI's sampling code, Pillow's `subsampling`)
SAMPLINGS = {"4:2:0": (0, 2), "4:2:2": (1, 1), "4:4:4": (2, 0)}


def pillow(bgr, quality, sampling):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(
        b, "JPEG", quality=quality, subsampling=SAMPLINGS[sampling][1], restart_marker_rows=1)
    return b.getvalue()


def decode(jpg):
    """Pillow's decode as BGR8 (raises if the stream is no JPEG)."""
    im = Image.open(io.BytesIO(jpg))
    im.load()
    return np.asarray(im.convert("RGB"))[:, :, ::-1]


def noise(w, h, seed=5):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def board(w, h, seed=766):
    """A tinted synthetic tag board: flat areas, sharp edges and real chroma."""
    from ros_vision_amd import synth
    small = w < 100
    g = synth.render_board(w, h, seed=seed, ntags=1 if small else 2,
                           side_range=(16, 20) if small else (40, 72))[0].astype(np.int32)
    yy, xx = np.mgrid[0:h, 0:w]
    r = np.clip(g + 40 * np.sin(xx / 9.0), 0, 255)
    b = np.clip(g - 35 * np.cos(yy / 7.0), 0, 255)
    return np.stack([b, g, r], -1).astype(np.uint8)


def primaries(w, h):
    """Vertical bars of the saturated primaries, their complements, black and white (Cb and
    Cr reach 0 and 255), 5 px wide so that the bars cut through blocks, under a ramp."""
    cols = np.array([[0, 0, 255], [0, 255, 0], [255, 0, 0], [255, 255, 0], [255, 0, 255], [0, 255, 255],
                     [0, 0, 0], [255, 255, 255]], np.uint8)
    img = cols[(np.arange(w) // 5) % 8][None, :, :].repeat(h, 0)
    img[h // 2:] = (img[h // 2:].astype(np.int32) * (np.arange(h - h // 2)[:, None, None] % 7) // 6).astype(np.uint8)
    return np.ascontiguousarray(img)


def flat(w, h, value):
    return np.full((h, w, 3), value, np.uint8)


def split(jpg):
    """(segments, scan): segments is the list of (marker, bytes of the whole segment) in front
    of the entropy-coded data, SOS included; scan is everything behind SOS up to and with EOI."""
    assert jpg[:2] == b"\xff\xd8"
    segs, i = [], 2
    while True:
        assert jpg[i] == 0xFF, "marker expected at %d" % i
        m, n = jpg[i + 1], jpg[i + 2] * 256 + jpg[i + 3]
        segs.append((m, bytes(jpg[i:i + 2 + n])))
        i += 2 + n
        if m == 0xDA:
            break
    assert jpg[-2:] == b"\xff\xd9"
    return segs, bytes(jpg[i:])


def assert_same_stream(got, want):
    """Every segment that is no APPn, in order, and the entropy-coded data: byte for byte."""
    gs, gscan = split(got)
    ws, wscan = split(want)
    ga = [(m, s) for m, s in gs if not 0xE0 <= m <= 0xEF]
    wa = [(m, s) for m, s in ws if not 0xE0 <= m <= 0xEF]
    assert [m for m, _ in ga] == [m for m, _ in wa], ([hex(m) for m, _ in ga], [hex(m) for m, _ in wa])
    for (m, a), (_, b) in zip(ga, wa):
        assert a == b, "segment %02x differs" % m
    assert [m for m, _ in ga] == [0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    if gscan != wscan:
        n = min(len(gscan), len(wscan))
        at = next((i for i in range(n) if gscan[i] != wscan[i]), n)
        raise AssertionError("entropy-coded data differs at byte %d of %d / %d" % (at, len(gscan), len(wscan)))
