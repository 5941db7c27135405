"""The parallel entropy decode of the MJPG path, host form (no GPU): at_mjpg_entropy_host
runs the subsequence algorithm of k_mjpg_entropy (csrc/at_mjpg_entropy.h) sequentially over
the threads' pieces.  Its dense coefficient streams must equal, byte for byte, what the
serial MjpgDecoder decodes (at_mjpg_dense_host), at every piece size; it must accept exactly
the streams MjpgDecoder accepts; and the synchronisation must end within `pieces` rounds
after round 0, the bound derived in at_mjpg_entropy.h.

Typical rounds at 328x248, S = 64 (recorded, not asserted): boards q5..q75 2..7, q95 16..18,
q100 18..31, 4:4:4 noise at q100 137 of 5229 pieces, one restart interval per MCU row
10..20 (a piece learns the interval's MCU count only from the marker in front of it)."""
import os
import subprocess

import numpy as np
import pytest

import mjpg_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(328, 248), (24, 40)]
SUBSEQ = [4, 16, 64, 256, 1 << 24]   # the last: larger than any scan, the serial decode


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


@pytest.fixture(scope="module")
def boards():
    return {(w, h): mc.board(w, h, ntags=2 if w > 100 else 1, side_range=(40, 72) if w > 100 else (16, 20))
            for w, h in SIZES}


def scan_of(jpg):
    """(offset, bytes) of the scan data: everything behind the SOS segment."""
    a = mc.segments(jpg)[-1][2]
    return a, jpg[a:]


ROUNDS = []   # (pieces, rounds) of every stream that went through _equal


def _equal(rva, jpg, size=(0, 0), subseq=SUBSEQ):
    for chroma in (False, True):
        want = rva.mjpg_dense_host(jpg, *size, keep_chroma=chroma)
        for S in subseq:
            got, rounds = rva.mjpg_entropy_host(jpg, S, *size, keep_chroma=chroma, nbytes=want.size)
            nd = int(np.count_nonzero(got != want))
            assert nd == 0, "S = %d, chroma %d: %d bytes differ from the serial decode" % (S, chroma, nd)
            pieces = max(1, -(-len(scan_of(jpg)[1]) // S))
            assert 1 <= rounds <= pieces + 1, (S, rounds, pieces)
            ROUNDS.append((S, pieces, rounds))


@pytest.mark.parametrize("quality", [5, 50, 75, 95, 100])
@pytest.mark.parametrize("sampling", list(mc.SAMPLINGS))
@pytest.mark.parametrize("size", SIZES)
def test_boards_equal_the_serial_decode(rva, boards, size, sampling, quality):
    _equal(rva, mc.encode(boards[size], quality, sampling), size)


@pytest.mark.parametrize("size", SIZES)
def test_noise_q100(rva, size):
    _equal(rva, mc.encode(mc.noise(*size), 100, "444"), size)


@pytest.mark.parametrize("sampling,quality", [("422", 5), ("420", 75), ("gray", 95)])
def test_flat_frames_whole_pieces_inside_runs_of_eobs(rva, sampling, quality):
    w, h = SIZES[0]
    jpg = mc.encode(np.full((h, w, 3), 93, np.uint8), quality, sampling)
    # DC only: a block takes a few bits, so a 16-byte piece holds nothing but whole blocks
    assert len(scan_of(jpg)[1]) * 8 < 12 * 3 * (w // 8 + 1) * (h // 8 + 1)
    _equal(rva, jpg, (w, h))


@pytest.mark.parametrize("extra", [{"restart_marker_rows": 1}, {"restart_marker_blocks": 1}])
@pytest.mark.parametrize("sampling", list(mc.SAMPLINGS))
def test_restart_markers(rva, boards, sampling, extra):
    jpg = mc.encode(boards[SIZES[0]], 75, sampling, **extra)
    assert jpg.count(b"\xff\xd7") >= 1 and b"\xff\xdd" in jpg
    _equal(rva, jpg, SIZES[0])


def test_uvc_stream_without_dht_and_optimised_tables(rva, boards):
    jpg = mc.encode(boards[SIZES[0]], 75, "422")
    _equal(rva, mc.with_avi1_app0(mc.strip_dht(jpg)), SIZES[0])
    _equal(rva, mc.encode(boards[SIZES[0]], 75, "420", optimize=True), SIZES[0])


@pytest.mark.parametrize("name", ["colorimage.jpg", "grayimage.jpg"])
def test_reference_fixtures(rva, golden_dir, name):
    _equal(rva, open(os.path.join(golden_dir, name), "rb").read())


def test_rounds_recorded():
    """Not a performance claim: prints what the streams above needed (pytest -s)."""
    for S in SUBSEQ[:-1]:
        r = sorted(x[2] for x in ROUNDS if x[0] == S)
        if r:
            print("S = %d: rounds median %d, most %d over %d streams" % (S, r[len(r) // 2], r[-1], len(r)))


# ---- piece boundaries, built by hand ---------------------------------------------
def _symbols(jpg):
    """A plain serial walk of a stream with DHT segments and no restart markers:
    [(kind, first bit, code bits, magnitude bits, first bit without stuffing)] with kind
    'dc' / 'ac', the first bit counted in the scan's raw bytes (stuffed zeros included)."""
    segs = {m: (a, b) for m, a, b in mc.segments(jpg)}
    sof = jpg[segs[0xC0][0] + 4:segs[0xC0][1]]
    h, w, nf = sof[1] * 256 + sof[2], sof[3] * 256 + sof[4], sof[5]
    hs, vs = (sof[7] >> 4, sof[7] & 15) if nf == 3 else (1, 1)
    sos = jpg[segs[0xDA][0] + 4:segs[0xDA][1]]
    sel = [(sos[2 + 2 * i] >> 4, sos[2 + 2 * i] & 15) for i in range(nf)]
    codes = {}
    for key, (bits, vals) in mc.dht_tables(jpg).items():
        t, code, k = {}, 0, 0
        for l in range(1, 17):
            for _ in range(bits[l - 1]):
                t[(l, code)] = vals[k]
                code, k = code + 1, k + 1
            code <<= 1
        codes[key] = t
    _, scan = scan_of(jpg)
    raw_of, data, i = [], bytearray(), 0     # destuffed bytes and where each lies in the scan
    while i < len(scan) and not (scan[i] == 0xFF and scan[i + 1] != 0):
        raw_of.append(i)
        data.append(scan[i])
        i += 2 if scan[i] == 0xFF else 1
    bits = "".join(format(b, "08b") for b in data)
    rawbit = lambda p: raw_of[p // 8] * 8 + p % 8
    pos, out = 0, []

    def symbol(tab):
        nonlocal pos
        for l in range(1, 17):
            s = tab.get((l, int(bits[pos:pos + l], 2)))
            if s is not None:
                pos += l
                return s, l
        raise AssertionError("no code")

    bw, bh = (w + 7) // 8, (h + 7) // 8
    nmcu = -(-bw // hs) * -(-bh // vs)
    order = [0] * (hs * vs) + ([1, 2] if nf == 3 else [])
    for _ in range(nmcu):
        for c in order:
            p0 = pos
            t, l = symbol(codes[(0, sel[c][0])])
            out.append(("dc", rawbit(p0), l, t, p0))
            pos += t
            k = 1
            while k < 64:
                p0 = pos
                rs, l = symbol(codes[(1, sel[c][1])])
                out.append(("ac", rawbit(p0), l, rs & 15, p0))
                pos += rs & 15
                if rs & 15 == 0 and rs >> 4 != 15:
                    break
                k += (rs >> 4) + 1 if rs & 15 else 16
    return out, scan, rawbit


def test_ff00_pair_straddles_a_piece_boundary(rva):
    w, h = SIZES[0]
    jpg = mc.encode(mc.noise(w, h), 100, "444")
    _, scan = scan_of(jpg)
    for S in (4, 16, 64):
        assert any(scan[p - 1] == 0xFF and scan[p] == 0 for p in range(S, len(scan), S)), S
    _equal(rva, jpg, (w, h), subseq=[4, 16, 64])


def test_restart_marker_straddles_a_piece_boundary(rva, boards):
    w, h = SIZES[0]
    jpg = mc.encode(boards[(w, h)], 75, "420", restart_marker_blocks=1)
    a, scan = scan_of(jpg)
    for S in (4, 16, 64):
        assert any(scan[p - 1] == 0xFF and 0xD0 <= scan[p] <= 0xD7 for p in range(S, len(scan), S)), S
    _equal(rva, jpg, (w, h), subseq=[4, 16, 64])


def test_piece_in_which_no_block_begins_and_piece_inside_magnitude_bits(rva):
    w, h = SIZES[1]
    jpg = mc.encode(mc.noise(w, h), 100, "444")
    syms, scan, _ = _symbols(jpg)
    S = 16
    starts = {s[1] // (8 * S) for s in syms if s[0] == "dc"}
    last = max(s[1] for s in syms) // (8 * S)
    assert any(p not in starts for p in range(last)), "every piece has a block beginning in it"
    # S = 1: some magnitude field covers a whole byte of the scan
    inside = [s for s in syms if (-(s[4] + s[2]) % 8) + 8 <= s[3]]
    assert inside, "no magnitude field covers a whole byte"
    _equal(rva, jpg, (w, h), subseq=[1, 2, S])


def test_last_piece_one_byte_long(rva, boards):
    w, h = SIZES[1]
    jpg = mc.encode(boards[(w, h)], 75, "422")
    for S in (4, 16, 64):
        n = len(scan_of(jpg)[1])
        padded = jpg + b"\x00" * ((1 - n) % S)     # bytes behind EOI belong to the last piece
        assert len(scan_of(padded)[1]) % S == 1
        _equal(rva, padded, (w, h), subseq=[S])
        _equal(rva, jpg[:len(jpg) - 2], (w, h), subseq=[S])   # no EOI: the data simply ends


# ---- accept / refuse parity ------------------------------------------------------
def _damaged(boards):
    b = boards[SIZES[1]]
    out = []
    for extra in ({"restart_marker_blocks": 2}, {}):
        good = mc.encode(b, 75, "420", **extra)
        out += [good] + mc.truncations(good, 50) + mc.corruptions(good, 200)
    return out


def test_accepts_exactly_what_the_serial_decoder_accepts(rva, boards):
    w, h = SIZES[1]
    accepted = refused = 0
    for jpg in _damaged(boards):
        try:
            want = rva.mjpg_dense_host(jpg, w, h, keep_chroma=True)
        except rva.MjpgError as e:
            for S in (4, 64):
                with pytest.raises(rva.MjpgError) as e2:
                    rva.mjpg_entropy_host(jpg, S, w, h, keep_chroma=True, nbytes=4224)
                assert e2.value.code == e.code
            refused += 1
            continue
        for S in (4, 16, 64, 256):
            got, _ = rva.mjpg_entropy_host(jpg, S, w, h, keep_chroma=True, nbytes=want.size)
            assert np.array_equal(got, want), S
        accepted += 1
    assert accepted > 50 and refused > 50


def test_sanitized_standalone_program(boards, tmp_path):
    """tests/mjpg_entropy_host_check.cpp + csrc/at_mjpg.cpp built with the host compiler and
    -fsanitize=address,undefined, run as a child process over the same truncations and
    corruptions (and good streams of every sampling) at piece sizes 4 .. 256 and one piece."""
    exe = tmp_path / "mjpg_entropy_host_check"
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-o", str(exe), os.path.join(ROOT, "tests", "mjpg_entropy_host_check.cpp"),
                    os.path.join(ROOT, "ros_vision_amd", "csrc", "at_mjpg.cpp")], check=True, timeout=300)
    w, h = SIZES[1]
    cases = [mc.encode(boards[SIZES[1]], q, s) for s in mc.SAMPLINGS for q in (5, 100)] + \
            [mc.encode(mc.noise(w, h), 100, "444"),
             mc.encode(boards[SIZES[1]], 75, "422", restart_marker_blocks=1)] + _damaged(boards)
    files = []
    for i, jpg in enumerate(cases):
        p = tmp_path / ("case%03d.jpg" % i)
        p.write_bytes(jpg)
        files.append(str(p))
    r = subprocess.run([str(exe), str(w), str(h), "4,16,64,256,16777216"] + files, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    decoded, refused = int(r.stdout.split()[1]), int(r.stdout.split()[3])
    assert decoded >= 100 and refused >= 100
