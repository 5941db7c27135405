"""MJPG colour, host side (no GPU): csrc/at_mjpg.cpp's full decode to BGR8
(at_mjpg_decode_bgr_host: chroma IDCT, libjpeg's fancy upsampling and colour conversion,
the arithmetic k_mjpg_idct_chroma / k_mjpg_bgr share) against Pillow's RGB decode of the
same bytes, channel-reversed.  The target is equality: every step is integer arithmetic
libjpeg specifies exactly.

Also: with colour off the coefficient stream is byte for byte as long as before the
colour path existed (literals recorded from the parent commit), and the colour-on host
path over truncated / corrupted streams in a stand-alone program built with the address
and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import mjpg_cases as mc
import mjpg_color_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mjpg_stream_mode(jpg) of every case on the parent commit (luma only; colour did not
# exist): the colour-off stream must not have changed
PARENT_STREAM = {
    "328x248-444-q30": ("sparse", 24544),
    "328x248-444-q95": ("sparse", 122096),
    "328x248-422-q30": ("sparse", 24544),
    "328x248-422-q95": ("sparse", 122096),
    "328x248-420-q30": ("sparse", 24544),
    "328x248-420-q95": ("sparse", 122096),
    "328x248-gray-q30": ("sparse", 16724),
    "328x248-gray-q95": ("sparse", 118228),
    "24x40-444-q30": ("sparse", 1520),
    "24x40-444-q95": ("dense", 2176),
    "24x40-422-q30": ("sparse", 1520),
    "24x40-422-q95": ("dense", 2176),
    "24x40-420-q30": ("sparse", 1520),
    "24x40-420-q95": ("dense", 2176),
    "24x40-gray-q30": ("sparse", 1520),
    "24x40-gray-q95": ("dense", 2176),
    "noise-444-q100": ("dense", 162944),
    "noise-420-q100": ("dense", 162944),
    "flat-422-q5": ("sparse", 10428),
    "rst-blocks-422": ("sparse", 40056),
    "rst-rows-422": ("sparse", 40056),
    "rst-blocks-420": ("sparse", 40056),
    "rst-rows-420": ("sparse", 40056),
    "three-tables-422": ("dense", 162944),
    "three-tables-420": ("dense", 162944),
    "colorimage.jpg": ("sparse", 1807516),
    "grayimage.jpg": ("sparse", 849792),
    "avi1-nodht-422": ("sparse", 40056),
}


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


@pytest.fixture(scope="module")
def cases():
    return cc.host_cases()


def test_case_list_is_the_recorded_one(cases):
    assert sorted(cases) == sorted(PARENT_STREAM)


@pytest.mark.parametrize("name", sorted(PARENT_STREAM))
def test_bgr_equals_pillow(rva, cases, name):
    """{444, 422, 420, gray} x quality {30, 95} x both sizes, noise at q100, a flat frame at
    q5, restart markers both ways, a DHT-less AVI1 stream, three quantisation tables, and
    the reference's two fixtures (1920x1080 4:2:0: chroma 960 x 540, 540 rows are no
    multiple of 8; 1280x800 single-component)."""
    jpg, ref = cases[name]
    want = cc.pil_bgr(ref)
    got = rva.mjpg_decode_bgr(jpg)
    assert got.shape == want.shape and got.dtype == np.uint8
    nd = int(np.count_nonzero(got != want))
    assert nd == 0, "%d samples differ from Pillow's RGB" % nd
    if "gray" in name:
        assert np.array_equal(got[:, :, 0], got[:, :, 1]) and np.array_equal(got[:, :, 0], got[:, :, 2])
        assert np.array_equal(got[:, :, 0], rva.mjpg_decode_gray(jpg))
    else:
        assert not np.array_equal(got[:, :, 0], got[:, :, 2])   # (the inputs carry real chroma)


@pytest.mark.parametrize("sampling", ["422", "420"])
def test_cr_uses_its_own_quantisation_table(rva, cases, sampling):
    """Pillow writes the three-table stream itself (qtables=[q0, q1, q2]: Tq 0, 1, 2; see
    mjpg_color_cases.three_tables -- nothing patched by hand).  With Cr pointed at Cb's
    table instead, Pillow's image changes: the tables do differ where it matters."""
    jpg, _ = cases["three-tables-" + sampling]
    sof = next(a for m, a, _ in mc.segments(jpg) if m == 0xC0)
    same = bytearray(jpg)
    same[sof + 18] = 1
    assert not np.array_equal(cc.pil_bgr(bytes(same)), cc.pil_bgr(jpg))
    assert np.array_equal(rva.mjpg_decode_bgr(bytes(same)), cc.pil_bgr(bytes(same)))


def test_missing_chroma_table_is_refused_only_with_colour(rva, cases):
    """A stream whose Cr names a table no DQT defines: the luma decode never needed it
    (and still does not), the colour decode refuses it."""
    jpg, _ = cases["328x248-420-q30"]
    sof = next(a for m, a, _ in mc.segments(jpg) if m == 0xC0)
    b = bytearray(jpg)
    b[sof + 18] = 3
    assert np.array_equal(rva.mjpg_decode_gray(bytes(b)), mc.pil_luma(jpg))
    with pytest.raises(rva.MjpgError) as e:
        rva.mjpg_decode_bgr(bytes(b))
    assert e.value.code == -1


def test_rejections_carry_the_same_codes(rva, cases):
    jpg, _ = cases["328x248-422-q30"]
    with pytest.raises(rva.MjpgError) as e:
        rva.mjpg_decode_bgr(mc.encode(cc.tinted_board(*cc.SIZES[0]), 75, "422", progressive=True))
    assert e.value.code == -6
    for junk in (b"", b"\xff\xd8", jpg[2:], jpg[:len(jpg) // 2]):
        with pytest.raises(rva.MjpgError) as e:
            rva.mjpg_decode_bgr(junk)
        assert e.value.code == -1


@pytest.mark.parametrize("name", sorted(PARENT_STREAM))
def test_colour_off_stream_is_the_parents(rva, cases, name):
    assert rva.mjpg_stream_mode(cases[name][0]) == PARENT_STREAM[name]


def test_sanitized_standalone_program(tmp_path):
    """tests/mjpg_color_host_check.cpp + csrc/at_mjpg.cpp built with the host compiler and
    -fsanitize=address,undefined, run as a child process: decode(keep_chroma) + pack +
    to_bgr over the truncations and corruptions of one 4:2:0 and one 4:4:4 stream (and
    the good streams of every sampling)."""
    exe = tmp_path / "mjpg_color_host_check"
    # (the sanitizer runtimes linked statically, as tests/test_mjpg_host.py builds its program)
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-o", str(exe), os.path.join(ROOT, "tests", "mjpg_color_host_check.cpp"),
                    os.path.join(ROOT, "ros_vision_amd", "csrc", "at_mjpg.cpp")], check=True, timeout=300)
    w, h = cc.SIZES[1]
    img = cc.tinted_board(w, h)
    good = [mc.encode(img, q, s) for s in mc.SAMPLINGS for q in (5, 100)] + [mc.encode(mc.noise(w, h), 100, "444")]
    damaged = []
    for base in (mc.encode(img, 75, "420", restart_marker_blocks=2), mc.encode(img, 75, "444")):
        good.append(base)
        damaged += mc.truncations(base, 50) + mc.corruptions(base, 200)
    files = []
    for i, jpg in enumerate(good + damaged):
        p = tmp_path / ("case%03d.jpg" % i)
        p.write_bytes(jpg)
        files.append(str(p))
    r = subprocess.run([str(exe), str(w), str(h)] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    decoded, refused = int(r.stdout.split()[1]), int(r.stdout.split()[3])
    assert decoded >= len(good) and refused >= 20 and decoded + refused == len(files)
