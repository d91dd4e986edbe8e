"""The baseline JPEG decoding rule on the host (no GPU): the numpy restatement tests/jpeg_decode_restate.py against the pixels Pillow
(libjpeg-turbo) decodes - recorded in tests/golden/jpeg_decode_pillow.npz and, where Pillow imports, live -, the parser's refusals in
the restatement and in the library, the synchronisation rule against the serial decoder, the library's argument checks.  Seven
mutants of the restatement each fail a named check.

Extreme coefficients.  The files around the encoder tests' 128 extreme blocks decode to Pillow's pixels at its default settings under
the tables of quality 100 and 99 (at 99 both clamps of the range limit occur).  From quality 98 down, samples leave [-512, 511] before
the range limit, where jidctint.c wraps (`& 1023`): there the rule is held to Pillow with libjpeg-turbo's SIMD off (JSIMD_FORCENONE=1
in a child process), which runs jidctint.c itself.  libjpeg-turbo's 16-bit SIMD IDCT, the default on x86, saturates instead: measured
on the quality-98 file, Pillow's default pixels equal the saturating variant and differ from jidctint.c's in 1144 of 8192 pixels.  No
8-bit encoder writes such coefficients (quality 100 reaches [-128, 127] exactly)."""
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import jpeg_decode_restate as JD
import jpeg_restate as JR
from helpers import ROOT

SIZES = [(1, 1), (2, 3), (3, 2), (5, 4), (4, 5), (1, 6), (6, 1), (9, 5), (16, 16), (17, 33), (37, 53), (130, 70)]
MUTANTS = {          # mutant -> the check below that it fails
    "replicate_all": "check_fixture",
    "plus8_both": "check_fixture",
    "no_colour_half": "check_fixture",
    "truncating_pass1": "check_fixture",
    "one_dc_predictor": "check_fixture",
    "keep_stuffing": "check_fixture",
    "same_round_buffer": "check_recorded_rounds",
}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "jpeg_decode_pillow.npz"))


@pytest.fixture(scope="module")
def fixture(golden):
    cases = []
    for line in golden["meta"]:
        k = str(line).split()[0]
        cases.append((golden[f"jpg_{k}"].tobytes(), golden[f"px_{k}"], str(line)))
    return cases


def pillow_pixels(data):
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(io.BytesIO(data)))


def pillow_pixels_scalar(data):
    """Pillow's pixels with libjpeg-turbo's SIMD off: the variable is read once per process, so a child decodes"""
    pytest.importorskip("PIL.Image")
    code = ("import sys, io, numpy as np; from PIL import Image; b = io.BytesIO(); "
            "np.save(b, np.asarray(Image.open(io.BytesIO(sys.stdin.buffer.read())))); sys.stdout.buffer.write(b.getvalue())")
    r = subprocess.run([sys.executable, "-c", code], input=data, stdout=subprocess.PIPE, check=True, env={**os.environ, "JSIMD_FORCENONE": "1"})
    return np.load(io.BytesIO(r.stdout))


def pillow_file(img, sub, **kw):
    Image = pytest.importorskip("PIL.Image")
    b = io.BytesIO()
    if sub != "gray":
        kw["subsampling"] = {"444": 0, "420": 2}[sub]
    Image.fromarray(img).save(b, "JPEG", **kw)
    return b.getvalue()


def decode_rgb(data, px_ndim, mutant=None, B=None):
    return JD.decode(data, "rgb", gray=px_ndim == 2, subseq_bits=B, mutant=mutant)


# ---- the checks (each takes the mutant to apply; None: the rule) --------------------------------------------------------------------------
def check_fixture(cases, mutant=None):
    for data, px, line in cases:
        got, status, _ = decode_rgb(data, px.ndim, mutant)
        assert status == 0 and np.array_equal(got, px), line


def check_recorded_rounds(cases, golden, mutant=None):
    """the rounds each file takes at B = 128, 160 and 1024 are the recorded ones, and the fixed point is the serial decode"""
    for B in (128, 160, 1024):
        rec = golden[f"rounds_{B}"]
        for (data, px, line), want in zip(cases, rec):
            serial = JD.coefficients(data)
            coef, status, rounds = JD.coefficients(data, B, mutant=mutant)
            assert np.array_equal(coef, serial[0]) and status == serial[1] == 0, (line, B)
            assert rounds == int(want), (line, B, rounds, int(want))


# ---- restatement against Pillow -------------------------------------------------------------------------------------------------------------
def test_restatement_is_the_fixture(fixture):
    assert len(fixture) == 157
    kinds = {line.split()[5] for _, _, line in fixture}
    assert kinds == {"noise", "smooth", "optimize", "qtables", "segments"}
    assert {tuple(int(v) for v in line.split()[1:3]) for _, _, line in fixture} == set(SIZES)
    check_fixture(fixture)


def test_restatement_is_live_pillow():
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:130, 0:70]
    for H, W in SIZES:
        for sub in ("420", "444", "gray"):
            for q in (1, 50, 95, 100):
                img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
                if q == 50:
                    img = (img // 16 + np.stack([128 + 100 * np.sin(x / 9.0 + k) * np.cos(y / 7.0) for k in range(3)], -1)[:H, :W]).clip(0, 255).astype(np.uint8)
                img = img[..., 0] if sub == "gray" else img
                for kw in (dict(quality=q), dict(quality=q, optimize=True)):
                    data = pillow_file(img, sub, **kw)
                    got, status, _ = decode_rgb(data, img.ndim)
                    assert status == 0 and np.array_equal(got, pillow_pixels(data)), (H, W, sub, kw)
            qt = [[int(v) for v in rng.integers(1, 256, 64)] for _ in range(2)]
            img = rng.integers(0, 256, (H, W) if sub == "gray" else (H, W, 3), dtype=np.uint8)
            data = pillow_file(img, sub, qtables=qt[:1] if sub == "gray" else qt)
            assert np.array_equal(decode_rgb(data, img.ndim)[0], pillow_pixels(data)), (H, W, sub, "qtables")
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    data = pillow_file(img, "420", quality=80, comment=b"hello", exif=b"Exif\0\0MM\0*\0\0\0\x08\0\0\0\0\0\0")
    assert b"\xff\xfe" in data and b"\xff\xe1" in data
    assert np.array_equal(decode_rgb(data, 3)[0], pillow_pixels(data))


def test_optimised_files_are_pillows():
    """jpeg_decode_restate.optimised_file (what the GPU tests decode) writes the bytes Pillow writes with optimize=True"""
    rng = np.random.default_rng(1)
    for H, W, sub, q in [(37, 53, "420", 75), (16, 16, "444", 95), (9, 5, "gray", 50), (17, 33, "420", 100), (5, 4, "444", 1)]:
        img = rng.integers(0, 256, (H, W) if sub == "gray" else (H, W, 3), dtype=np.uint8)
        coef, _ = JR.coefficients(img, q, sub, "rgb")
        mine = JD.optimised_file(coef, H, W, JR.mode_of(sub, 1 if sub == "gray" else 3), q)
        assert mine == pillow_file(img, sub, quality=q, optimize=True), (H, W, sub, q)


# ---- extreme coefficients -------------------------------------------------------------------------------------------------------------------
def raw_samples(data):
    """the IDCT's results before the range limit, [blocks, 8, 8]"""
    info = JD.parse(data)
    coef, status, _ = JD.coefficients(data, info=info)
    assert status == 0
    nat = np.zeros((len(coef), 64), np.int32)
    nat[:, JD.ZIGZAG] = coef.astype(np.int32) * np.array(info["quant"][0], np.int32)[None]
    cols = JD._idct_pass(nat.reshape(-1, 8, 8).transpose(0, 2, 1), 11).transpose(0, 2, 1)
    return JD._idct_pass(cols, 18)


def test_extreme_coefficients(golden):
    seen = {}
    for q in (100, 99, 98, 95, 75):
        data, want = golden[f"ext_jpg_{q}"].tobytes(), golden[f"ext_px_{q}"]
        assert want.shape == (8, 8 * 128)
        got, status, _ = JD.decode(data, gray=True)
        assert status == 0 and np.array_equal(got, want), q
        raw = raw_samples(data)
        seen[q] = (int(raw.min()), int(raw.max()))
    assert seen[100] == (-128, 127)                                        # what an 8-bit encoder's coefficients reach
    assert seen[99][0] + 128 < 0 and seen[99][1] + 128 > 255 and -512 <= seen[99][0] and seen[99][1] <= 511          # both clamps, no wrap
    for q in (98, 95, 75):
        assert seen[q][0] < -512 and seen[q][1] > 511                      # the & 1023 wrap, both ways
    print("IDCT results before the range limit, per quality:", seen)


def test_extreme_coefficients_live_pillow(golden):
    for q in (100, 99):
        data = golden[f"ext_jpg_{q}"].tobytes()
        assert np.array_equal(JD.decode(data, gray=True)[0], pillow_pixels(data)), q
    for q in (98, 95, 75):
        data = golden[f"ext_jpg_{q}"].tobytes()
        assert np.array_equal(JD.decode(data, gray=True)[0], pillow_pixels_scalar(data)), q
    data = golden["ext_jpg_98"].tobytes()
    simd, rule = pillow_pixels(data), JD.decode(data, gray=True)[0]
    print("quality 98: pixels where Pillow's default (SIMD) decode differs from jidctint.c's:", int((simd != rule).sum()), "of", rule.size)


# ---- the parser -------------------------------------------------------------------------------------------------------------------------------
def test_parser_refuses_by_name(golden):
    import dsnerf_amd
    L = dsnerf_amd._lib
    assert L.JPEGD_REASONS == JD.REASONS
    want = {"progressive": "progressive", "s422": "sampling", "restart": "restart", "table16": "table16", "two_scans": "multiscan",
            "truncated_header": "truncated", "twelve_bits": "precision", "arithmetic": "arithmetic", "no_eoi": "no_eoi", "not_jpeg": "not_jpeg"}
    assert {str(r).split()[0]: str(r).split()[1] for r in golden["refused"]} == want
    for name, reason in want.items():
        data = golden[f"refused_{name}"].tobytes()
        with pytest.raises(JD.Refused) as e:
            JD.parse(data)
        assert e.value.reason == reason, name
        assert L.JPEGD_REASONS[L.jpeg_parse(data)[1]] == reason, name
    good = golden["jpg_c40"].tobytes()
    for cut in range(0, JD.parse(good)["scan_offset"], 7):          # every header cut short is refused, by both parsers alike
        with pytest.raises(JD.Refused) as e:
            JD.parse(good[:cut])
        assert L.JPEGD_REASONS[L.jpeg_parse(good[:cut])[1]] == e.value.reason in ("not_jpeg", "truncated"), cut


def test_library_parser_fills_the_descriptor(fixture):
    import dsnerf_amd
    L = dsnerf_amd._lib
    assert C.sizeof(L.JpegdDesc) == 3504 and C.sizeof(L.JpegdHuff) == 400
    for data, px, line in fixture:
        d, st = L.jpeg_parse(data)
        i = JD.parse(data)
        assert st == 0, line
        assert (d.H, d.W, d.mode, d.ncomp, d.scan_offset, d.scan_length, d.file_length) == \
            (i["H"], i["W"], i["mode"], i["ncomp"], i["scan_offset"], i["scan_length"], len(data)), line
        for c in range(i["ncomp"]):
            assert (d.qsel[c], d.dcsel[c], d.acsel[c]) == (i["qsel"][c], i["dcsel"][c], i["acsel"][c])
            assert list(d.quant[d.qsel[c]]) == i["quant"][i["qsel"][c]]
            for mine, theirs in ((d.dc[d.dcsel[c]], i["dc"][i["dcsel"][c]]), (d.ac[d.acsel[c]], i["ac"][i["acsel"][c]])):
                n = len(theirs["vals"])
                assert list(mine.bits) == theirs["bits"] and list(mine.vals)[:n] == theirs["vals"] and not any(list(mine.vals)[n:])
                assert list(mine.lim) == theirs["lim"] and list(mine.base) == theirs["base"]


# ---- the synchronisation rule ---------------------------------------------------------------------------------------------------------------------
def test_fixed_point_is_the_serial_decode(fixture, golden):
    check_recorded_rounds(fixture, golden)
    for B in (128, 160, 1024):
        rec = golden[f"rounds_{B}"]
        print(f"rounds at B = {B}: max {int(rec.max())}, median {int(np.median(rec))}, files with more than 3: {int((rec > 3).sum())} of {len(rec)}")
    assert int(golden["rounds_128"].max()) > 100          # noise at quality 100 has no end-of-block codes to re-synchronise on


def grey_scan_of(bits_wanted=None, ff_at=None):
    """a one-row grey file found by search: its unstuffed scan is exactly `bits_wanted` bits long, or its unstuffed byte `ff_at` is 0xFF"""
    rng = np.random.default_rng(17)
    for _ in range(20000):
        n = int(rng.integers(1, 4))
        coef = (rng.integers(-300, 301, (n, 64)) * (rng.random((n, 64)) < 0.2)).astype(np.int16)
        raw = JR.raw_scan(coef, JR.MGRAY)
        if bits_wanted is not None and JR.scan_bits(coef, JR.MGRAY) == bits_wanted:
            return JR.scan_file(coef, 8, 8 * n, JR.MGRAY, 90), raw
        if ff_at is not None and len(raw) > ff_at + 4 and raw[ff_at] == 0xFF:
            return JR.scan_file(coef, 8, 8 * n, JR.MGRAY, 90), raw
    raise AssertionError("no such scan found")


def test_synchronisation_corner_files(fixture):
    """a file shorter than one subsequence, one of exactly B bits, and a scan whose stuffed byte straddles a subsequence edge"""
    short = next(d for d, px, line in fixture if line.split()[1:3] == ["1", "1"])
    for B in (128, 160, 1024):
        assert 8 * len(JD.unstuff(JR.split_file(short)[1])[0]) < B
        assert JD.coefficients(short, B)[2] == 1 and np.array_equal(JD.coefficients(short, B)[0], JD.coefficients(short)[0])
    for B in (128, 160):
        data, raw = grey_scan_of(bits_wanted=B)
        assert 8 * len(raw) == B
        coef, status, rounds = JD.coefficients(data, B)
        assert rounds == 1 and status == 0 and np.array_equal(coef, JD.coefficients(data)[0])
        assert JD.coefficients(data, 128)[1] == 0 and np.array_equal(JD.coefficients(data, 128)[0], coef)
    data, raw = grey_scan_of(ff_at=15)          # unstuffed byte 15 = bits 120 ... 127: the 0x00 behind it would be the next subsequence's first byte
    scan = JR.split_file(data)[1]
    assert scan[15:17] == b"\xff\x00" or b"\xff\x00" in scan[:17]
    for B in (128, 160, 1024):
        coef, status, rounds = JD.coefficients(data, B)
        assert status == 0 and np.array_equal(coef, JD.coefficients(data)[0])


def test_status_bits():
    """a marker, a scan cut short, a scan with bytes to spare, and padding that is not all ones"""
    img = np.random.default_rng(3).integers(0, 256, (24, 24), dtype=np.uint8)
    data = JR.encode(img, 90, "gray")[0]
    i = JD.parse(data)
    a, n = i["scan_offset"], i["scan_length"]
    for B in (None, 128):
        assert JD.coefficients(data, B)[1] == 0
        st = JD.coefficients(data[:a + n // 2] + b"\xff\xd0" + data[a + n // 2 + 2:], B)[1]
        assert st & JD.MARKER and st & JD.CORRUPT
        st = JD.coefficients(data[:a + n // 2] + data[-2:], B)[1]
        assert st & JD.COUNT and st & JD.CORRUPT and not st & JD.MARKER
        st = JD.coefficients(data[:a + n] + b"\xff\x00\xff\x00" + data[-2:], B)[1]
        assert st == JD.PADDING
    pixels, st, _ = JD.decode(data[:a + n // 2] + data[-2:])
    assert st & JD.CORRUPT and pixels.shape == (24, 24, 3) and not pixels.any()          # an error frame is all zeros


# ---- the library's argument checks --------------------------------------------------------------------------------------------------------------
def test_argument_checks_go_through_the_library():
    import dsnerf_amd
    lib = dsnerf_amd._lib.lib()
    z, one, sz = None, C.c_void_p(256), C.c_size_t
    ws = 1 << 24
    calls = {
        "dsn_jpeg_parse_host": lambda: lib.dsn_jpeg_parse_host(z, 10, z, z),
        "dsn_jpegd_sync": lambda: lib.dsn_jpegd_sync(z, 0, z, z, 1, 8, 8, 0, 100, 1024, 1, 1, z, z, z, 0, z),
        "dsn_jpegd_coefficients": lambda: lib.dsn_jpegd_coefficients(z, 1, 8, 8, 0, 100, 1024, z, z, z, 0, z),
        "dsn_jpegd_pixels": lambda: lib.dsn_jpegd_pixels(z, z, z, 1, 8, 8, 0, 100, 0, 0, z, z, 0, z),
        "dsn_jpeg_decode": lambda: lib.dsn_jpeg_decode(z, 0, z, z, 1, 8, 8, 0, 100, 1024, 8, 0, 0, z, z, z, z, 0, z),
        "dsn_jpegd_workspace_coef": lambda: lib.dsn_jpegd_workspace_coef(z, 1, 8, 8, 0, 100, z),
    }
    for name, call in calls.items():
        assert call() != 0, name
        assert name.encode() in lib.dsn_last_error() and b"null" in lib.dsn_last_error(), (name, lib.dsn_last_error())
    dec = lambda **k: lib.dsn_jpeg_decode(k.get("files", one), k.get("nbytes", 4096), one, one, k.get("F", 1), k.get("H", 8), 8, k.get("mode", 0),  # noqa: E731
                                          k.get("scan", 100), k.get("B", 1024), k.get("rounds", 8), 0, k.get("gray", 0), one, one, one,
                                          k.get("ws", one), k.get("wsb", ws), z)
    bad = [
        (lambda: dec(mode=3), b"mode"), (lambda: dec(H=0), b"H and W"), (lambda: dec(F=16385), b"F must be"),
        (lambda: dec(B=100), b"subseq_bits"), (lambda: dec(B=4128), b"subseq_bits"), (lambda: dec(B=1000), b"subseq_bits"),
        (lambda: dec(rounds=0), b"rounds"), (lambda: dec(gray=1), b"gray_out"), (lambda: dec(scan=(1 << 27) + 1), b"max_scan_bytes"),
        (lambda: dec(files=C.c_void_p(264)), b"16-byte aligned"), (lambda: dec(nbytes=4100), b"multiple of 16"),
        (lambda: dec(wsb=16), b"workspace_bytes"), (lambda: dec(ws=C.c_void_p(8)), b"256-byte"),
        (lambda: lib.dsn_jpegd_sync(one, 4096, one, one, 1, 8, 8, 0, 100, 1024, 1, -1, z, z, one, ws, z), b"rounds"),
        (lambda: lib.dsn_jpegd_pixels(one, z, one, 1, 8, 8, 0, 100, 0, 1, one, one, ws, z), b"gray_out"),
        (lambda: lib.dsn_jpegd_coefficients(one, 1, 8, 8, 0, 100, 1024, C.c_void_p(258), one, one, ws, z), b"16-byte aligned"),
    ]
    for call, msg in bad:
        assert call() != 0 and msg in lib.dsn_last_error(), (msg, lib.dsn_last_error())
    assert lib.dsn_jpeg_decode(z, 0, z, z, 0, 8, 8, 0, 100, 1024, 8, 0, 0, z, z, z, z, 0, z) == 0          # no frames: nothing to do
    n1, n2 = lib.dsn_jpegd_workspace_bytes(1, 64, 64, 0, 10000), lib.dsn_jpegd_workspace_bytes(2, 64, 64, 0, 10000)
    assert 0 < n1 < n2 and n1 > 10000 + 24 * 64 * 3
    assert lib.dsn_jpegd_workspace_bytes(1, 64, 64, 3, 10000) == 0 and lib.dsn_jpegd_workspace_bytes(0, 64, 64, 0, 10000) == 0
    assert lib.dsn_jpegd_workspace_bytes(1, 64, 64, 0, sz((1 << 27) + 1)) == 0
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dsnerf_amd.jpeg.decode(JR.encode(np.zeros((8, 8, 3), np.uint8))[0])
    with pytest.raises(ValueError, match="progressive"):
        dsnerf_amd.jpeg.decode(np.load(os.path.join(ROOT, "tests", "golden", "jpeg_decode_pillow.npz"))["refused_progressive"].tobytes())


def test_documents_state_the_claim():
    text = open(os.path.join(ROOT, "README.md")).read()
    assert "jpeg.decode" in text and "cv2.imread" in text
    head = open(os.path.join(ROOT, "include", "dsnerf.h")).read()
    for word in ("dsn_jpeg_parse_host", "jpeg_idct_islow", "& 1023", "downsampled_width > 2", "91881", "PREVIOUS round's buffer"):
        assert word in head, word
    assert "#define DSN_ABI_VERSION 8" in head


# ---- mutants ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutant_fails_its_named_check(fixture, golden, mutant):
    small = [c for c in fixture if int(c[2].split()[1]) * int(c[2].split()[2]) <= 37 * 53]
    with pytest.raises(AssertionError):
        if MUTANTS[mutant] == "check_fixture":
            check_fixture(small, mutant)
        else:
            check_recorded_rounds(small, golden, mutant)
