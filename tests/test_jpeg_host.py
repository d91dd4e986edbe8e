"""The baseline JPEG rule on the host (no GPU): the numpy restatement tests/jpeg_restate.py against the bytes Pillow (libjpeg-turbo)
writes - recorded in tests/golden/jpeg_pillow.npz and, where Pillow imports, live -, against closed forms, its own decoder and its
float64 twins; the Motion-JPEG container; the library's argument checks.  Six mutants of the restatement each fail a named test."""
import ctypes as C
import io
import os
import struct

import numpy as np
import pytest

import jpeg_restate as JR
from helpers import ROOT

MUTANTS = {          # mutant -> the check below that it fails
    "no_stuffing": "check_fixture",
    "zero_padding": "check_fixture",
    "half_up_levels": "check_level_rule",
    "swap_rb": "check_fixture",
    "dc_reset_per_row": "check_two_mcu_rows",
    "flat_bias": "check_downsampling_bias",
}


@pytest.fixture(scope="module")
def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_pillow.npz"))
    cases = []
    for line in g["meta"]:
        k, H, W, sub, q, kind = str(line).split()
        cases.append((g[f"img_{k}"], int(q), sub, g[f"jpg_{k}"].tobytes(), str(line)))
    return cases


def pillow_bytes(img, q, sub):
    Image = pytest.importorskip("PIL.Image")
    b = io.BytesIO()
    if img.ndim == 2:
        Image.fromarray(img).save(b, "JPEG", quality=q, optimize=False)
    else:
        Image.fromarray(img).save(b, "JPEG", quality=q, subsampling={"444": 0, "420": 2}[sub], optimize=False)
    return b.getvalue()


# ---- the checks (each takes the mutant to apply; None: the rule) --------------------------------------------------------------------------
def check_fixture(cases, mutant=None):
    for img, q, sub, data, line in cases:
        assert JR.encode(img, q, sub, "rgb", mutant=mutant)[0] == data, line


def check_level_rule(mutant=None):
    f = np.float32
    v = np.array([0.5, 1.5, 2.5, 3.5, 254.5, 255.5, -0.5, -3.0, 300.0, 1e30, np.inf, -np.inf, np.nan, 127.49999, 0.0], f)
    want = [0, 2, 2, 4, 254, 255, 0, 0, 255, 255, 255, 0, 0, 127, 0]
    got, bad = JR.levels(v.reshape(1, -1, 1), scale=1.0, mutant=mutant)
    assert got.reshape(-1).tolist() == want and bad
    # the scripts' form: [0, 1] times 255 in float32; every level comes back, halves go to the even neighbour
    k = np.arange(256)
    got, bad = JR.levels((k / 255.0).astype(f).reshape(1, -1, 1), mutant=mutant)
    assert got.reshape(-1).tolist() == k.tolist() and not bad
    half = ((k[:-1] + 0.5) / 255.0).astype(f)
    exact = (half * f(255.0)) == (k[:-1] + f(0.5))          # where the float32 product lands on the tie exactly
    assert exact.sum() > 50
    got, _ = JR.levels(half.reshape(1, -1, 1), mutant=mutant)
    assert (got.reshape(-1)[exact] == (k[:-1] + (k[:-1] & 1))[exact]).all()
    assert JR.levels(np.array([[7, 200]], np.uint8))[0].tolist() == [[7, 200]]


def check_two_mcu_rows(mutant=None):
    """the DC predictors run on across MCU rows: a 40 x 48 frame (three MCU rows at 4:2:0) decodes to its own coefficients"""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (40, 48, 3), dtype=np.uint8)
    coef, _ = JR.coefficients(img, 90, "420")
    scan = JR.entropy_encode(coef, JR.M420, W=48, mutant=mutant)
    back, used = JR.decode_scan(scan, len(coef), JR.M420)
    assert np.array_equal(back, coef)


def check_downsampling_bias(mutant=None):
    """the bias 1 / 2 alternates over the output columns: 2 x 2 sums that leave a remainder round differently on even and odd columns"""
    u8 = np.random.default_rng(8).integers(0, 256, (16, 16, 3), dtype=np.uint8)
    cb = JR.ycc(u8)[..., 1]
    s = cb[0::2, 0::2] + cb[0::2, 1::2] + cb[1::2, 0::2] + cb[1::2, 1::2]
    want = (s + 1 + (np.arange(8) & 1)[None, :]) >> 2
    assert (((s + 1) >> 2) != ((s + 2) >> 2))[:, 0::2].any() and (((s + 1) >> 2) != ((s + 2) >> 2))[:, 1::2].any()
    blocks, dummy = JR.sample_blocks(u8, JR.M420, "rgb", mutant)
    assert np.array_equal(blocks[4], want) and not dummy.any()


# ---- restatement against Pillow -------------------------------------------------------------------------------------------------------------
def test_restatement_is_the_fixture(fixture):
    assert len(fixture) == 24
    check_fixture(fixture)


def test_restatement_is_live_pillow():
    rng = np.random.default_rng(11)
    for H, W in [(17, 33), (18, 33), (33, 17), (34, 50), (1, 16), (16, 1), (15, 15), (49, 2)]:          # H odd and even just above 16, 32
        for sub in ("420", "444", "gray"):
            for q in (10, 75, 100):
                img = rng.integers(0, 256, (H, W) if sub == "gray" else (H, W, 3), dtype=np.uint8)
                assert JR.encode(img, q, sub, "rgb")[0] == pillow_bytes(img, q, sub), (H, W, sub, q)
    for H, W in [(1, 1), (8, 8), (19, 23), (64, 64)]:
        for sub in ("420", "444", "gray"):
            img = np.full((H, W) if sub == "gray" else (H, W, 3), 201, np.uint8)
            assert JR.encode(img, 95, sub, "rgb")[0] == pillow_bytes(img, 95, sub), (H, W, sub)


def test_header_and_tables_are_pillows():
    img = np.zeros((9, 21, 3), np.uint8)
    for q in (1, 10, 50, 75, 95, 100):
        for sub, mode in (("420", JR.M420), ("444", JR.M444), ("gray", JR.MGRAY)):
            data = pillow_bytes(img[..., 0] if sub == "gray" else img, q, sub)
            assert JR.split_file(data)[0] == JR.header(9, 21, mode, q), (q, sub)
    assert len(JR.header(9, 21, JR.M420, 50)) == 623 and len(JR.header(9, 21, JR.MGRAY, 50)) == 328


def test_library_header_and_sizes():
    import dsnerf_amd
    L = dsnerf_amd._lib
    for H, W, mode, q in [(1, 1, 0, 1), (37, 53, 0, 50), (130, 70, 1, 95), (63, 65, 2, 100), (512, 512, 0, 10), (65535, 16, 2, 75)]:
        assert L.jpeg_header(H, W, mode, q) == JR.header(H, W, mode, q)
        assert L.jpeg_max_bytes(H, W, mode) == JR.max_bytes(H, W, mode)
        assert L.jpeg_blocks(H, W, mode) == JR.n_blocks(H, W, mode)
        assert L.lib().dsn_jpeg_workspace_bytes(2, H, W, mode) > 2 * JR.n_blocks(H, W, mode) * (128 + 208)
    assert L.lib().dsn_jpeg_max_bytes(4096, 4096, 1) > 0                      # 2^24 pixels fit in every mode
    assert L.lib().dsn_jpeg_max_bytes(65535, 65535, 2) == 0                   # 67 M blocks x 1664 bits leave int32
    assert L.lib().dsn_jpeg_workspace_bytes(1, 65535, 65535, 0) == 0
    assert L.lib().dsn_jpeg_max_bytes(0, 8, 0) == 0 and L.lib().dsn_jpeg_max_bytes(8, 8, 3) == 0
    with pytest.raises(ValueError):
        L.jpeg_max_bytes(65535, 65535, 1)


def test_argument_checks_go_through_the_library():
    import dsnerf_amd
    lib = dsnerf_amd._lib.lib()
    z, one = None, C.c_void_p(256)
    f = C.c_float(255.0)
    calls = {
        "dsn_jpeg_coefficients": lambda: lib.dsn_jpeg_coefficients(z, 0, 1, 8, 8, 0, 95, 0, f, z, z, z),
        "dsn_jpeg_scan": lambda: lib.dsn_jpeg_scan(z, z, 1, 8, 8, 0, 95, z, 1000, z, z, z, 0, z),
        "dsn_jpeg_encode": lambda: lib.dsn_jpeg_encode(z, 0, 1, 8, 8, 0, 95, 0, f, z, 1000, z, z, z, 0, z),
        "dsn_jpeg_header_host": lambda: lib.dsn_jpeg_header_host(8, 8, 0, 95, z, 640, z),
    }
    for name, call in calls.items():
        assert call() != 0, name
        assert name.encode() in lib.dsn_last_error() and b"null" in lib.dsn_last_error(), (name, lib.dsn_last_error())
    bad = [
        (lambda: lib.dsn_jpeg_encode(one, 0, 1, 8, 8, 3, 95, 0, f, one, 1000, one, one, one, 1 << 20, z), b"mode"),
        (lambda: lib.dsn_jpeg_encode(one, 0, 1, 8, 8, 0, 0, 0, f, one, 1000, one, one, one, 1 << 20, z), b"quality"),
        (lambda: lib.dsn_jpeg_encode(one, 0, 1, 8, 8, 0, 101, 0, f, one, 1000, one, one, one, 1 << 20, z), b"quality"),
        (lambda: lib.dsn_jpeg_encode(one, 2, 1, 8, 8, 0, 95, 0, f, one, 1000, one, one, one, 1 << 20, z), b"dtype"),
        (lambda: lib.dsn_jpeg_encode(one, 0, 1, 0, 8, 0, 95, 0, f, one, 1000, one, one, one, 1 << 20, z), b"H and W"),
        (lambda: lib.dsn_jpeg_encode(one, 0, 1, 65535, 65535, 1, 95, 0, f, one, 1000, one, one, one, 1 << 20, z), b"too many blocks"),
        (lambda: lib.dsn_jpeg_encode(one, 0, 65536, 8, 8, 0, 95, 0, f, one, 1000, one, one, one, 1 << 20, z), b"F must be"),
        (lambda: lib.dsn_jpeg_encode(one, 0, 1, 8, 8, 0, 95, 0, f, one, 1000, one, one, one, 16, z), b"workspace_bytes"),
        (lambda: lib.dsn_jpeg_encode(one, 0, 1, 8, 8, 0, 95, 0, f, one, 1000, one, one, C.c_void_p(8), 1 << 20, z), b"256-byte"),
        (lambda: lib.dsn_jpeg_scan(one, one, 1, 8, 8, 0, 95, one, 1000, one, one, one, 1 << 20, z), b"must differ"),
        (lambda: lib.dsn_jpeg_header_host(8, 8, 0, 95, one, 100, one), b"capacity"),
    ]
    for call, msg in bad:
        assert call() != 0 and msg in lib.dsn_last_error(), (msg, lib.dsn_last_error())
    assert lib.dsn_jpeg_encode(z, 0, 0, 8, 8, 0, 95, 0, f, z, 0, z, z, z, 0, z) == 0          # no frames: nothing to do
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dsnerf_amd.jpeg.encode(np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(ValueError):
        dsnerf_amd.jpeg.imwrite("frame.png", np.zeros((8, 8, 3), np.uint8))


# ---- decoder and coefficients ---------------------------------------------------------------------------------------------------------------
def test_decoder_returns_the_coefficients(fixture):
    for img, q, sub, data, line in fixture:
        coef, _ = JR.coefficients(img, q, sub, "rgb")
        mode = JR.mode_of(sub, 1 if img.ndim == 2 else 3)
        head, scan, tail = JR.split_file(data)          # Pillow's own scan
        back, used = JR.decode_scan(scan, len(coef), mode)
        assert np.array_equal(back, coef), line
        assert used == JR.scan_bits(coef, mode)


def extreme_blocks():
    """+-128 along the signs of every basis function: the blocks that drive one coefficient as far as it goes"""
    k = np.arange(8)
    A = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k == 0, np.sqrt(1 / 8), 0.5)[:, None]
    ext = np.stack([np.where(np.outer(A[u], A[v]) >= 0, 127, -128) for u in range(8) for v in range(8)])
    return np.concatenate([ext, -ext - 1])


def test_integer_dct_is_within_its_bar_of_float64():
    bar = 0.5          # DSN_JPEG_DCT_BAR: derived from the rounding steps in include/dsnerf.h
    assert "#define DSN_JPEG_DCT_BAR 0.5" in open(os.path.join(ROOT, "include", "dsnerf.h")).read()
    rng = np.random.default_rng(0)
    blocks = np.concatenate([rng.integers(-128, 128, (4000, 8, 8)), extreme_blocks(), np.full((1, 8, 8), -128), np.full((1, 8, 8), 127)])
    err = np.abs(JR.fdct(blocks) / 8.0 - JR.fdct_float64(blocks)).max()
    print("integer DCT / 8 against float64:", err)
    assert err <= bar
    assert np.abs(JR.fdct(blocks)).max() < 2 ** 15
    one = np.zeros((1, 8, 8), np.int64)
    one[0, 0, 0] = 64
    assert JR.fdct(np.full((1, 8, 8), 5))[0, 0, 0] == 5 * 64 and not JR.fdct(np.full((1, 8, 8), 5))[0].reshape(-1)[1:].any()


def test_extreme_blocks_stay_inside_the_code_sizes():
    tabs = JR.quant_tables(100)
    assert (tabs[0] == 1).all() and (tabs[1] == 1).all()
    z = JR.quantise(JR.fdct(extreme_blocks()), tabs[0]).reshape(-1, 64)
    assert int(JR._size(z[:, 1:]).max()) <= 10
    assert int(JR._size(np.array([z[:, 0].max() - z[:, 0].min()])).max()) <= 11
    coef = JR.hand_made_scans()["all_ff_block"][0]
    assert JR.scan_bits(coef[:1], JR.MGRAY) == 1658 == 20 + 63 * 26          # the longest block: what DSN_JPEG_BLOCK_BYTES covers
    assert 8 * 208 >= 1658


def test_quantisation_rule():
    t = JR.quant_tables(50)
    assert np.array_equal(t[0], JR.Q_LUMA) and np.array_equal(t[1], JR.Q_CHROMA)
    assert JR.quant_tables(1)[0].max() == 255 and JR.quant_tables(1)[0].min() == 255
    assert JR.quant_tables(75)[0][:4].tolist() == [8, 6, 5, 8]
    c = np.zeros((1, 8, 8), np.int64)
    c[0, 0, :6] = [63, 64, -63, -64, 191, -192]          # d = 8 x 16, 8 x 11, ...: below half a step -> 0, at half a step -> away from zero
    tab = np.full(64, 16)
    assert JR.quantise(c, tab)[0, 0, :6].tolist() == [0, 1, 0, -1, 1, -2]


# ---- scans of hand-made coefficients --------------------------------------------------------------------------------------------------------
def test_hand_made_scans():
    cases = JR.hand_made_scans()
    for name, (coef, mode, H, W) in cases.items():
        assert JR.n_blocks(H, W, mode) == len(coef), name
        scan = JR.entropy_encode(coef, mode)
        back, used = JR.decode_scan(scan, len(coef), mode)
        assert np.array_equal(back, coef) and used == JR.scan_bits(coef, mode), name
        assert b"\xff" not in scan.replace(b"\xff\x00", b""), name          # every 0xFF is followed by 0x00
    zrl, eob = 11, 4          # lengths of the luminance ZRL and EOB codes
    base = JR.scan_bits(cases["run15"][0], JR.MGRAY)          # DC + (15/2) code of 16 bits + 2 + EOB
    assert base == 3 + 3 + 16 + 2 + eob
    assert JR.scan_bits(cases["run16"][0], JR.MGRAY) == 3 + 3 + zrl + 2 + 2 + eob          # one ZRL, then (0/2): 01 + 2 bits
    assert JR.scan_bits(cases["run17"][0], JR.MGRAY) == 3 + 3 + zrl + 5 + 2 + eob          # (1/2): 11011
    assert JR.scan_bits(cases["run32"][0], JR.MGRAY) == 3 + 3 + 2 * zrl + 2 + 2 + eob
    assert JR.scan_bits(cases["run62"][0], JR.MGRAY) == 3 + 3 + 3 * zrl + 16 + 2               # (14/2); coefficient 63 set: no EOB
    val, cnt = JR.block_symbols(cases["c63_set_and_clear"][0], JR.MGRAY)
    assert cnt[0, 63] == 3 * zrl + 16 + 1 and (int(val[1, 63]), int(cnt[1, 63])) == (0b1010, eob)          # (14/1) + amplitude; EOB
    assert JR.scan_bits(cases["ends_on_byte_boundary"][0], JR.MGRAY) % 8 == 0
    coef = cases["ends_on_byte_boundary"][0]
    assert JR.entropy_encode(coef, JR.MGRAY) == JR.entropy_encode(coef, JR.MGRAY, mutant="zero_padding")          # nothing to pad
    coef = cases["padded_last_byte_is_ff"][0]
    assert JR.scan_bits(coef, JR.MGRAY) % 8 and JR.entropy_encode(coef, JR.MGRAY)[-2:] == b"\xff\x00"
    assert JR.entropy_encode(coef, JR.MGRAY, mutant="zero_padding")[-1] != 0
    coef = cases["all_ff_block"][0]
    raw = JR.raw_scan(coef, JR.MGRAY)
    assert raw.count(b"\xff") > len(raw) // 3 and len(JR.entropy_encode(coef, JR.MGRAY)) == len(raw) + raw.count(b"\xff")
    sizes = JR._size(np.diff(np.concatenate([[0], cases["dc_sizes"][0][:, 0].astype(np.int64)])))
    assert sorted(set(sizes.tolist())) == list(range(12))


def test_hand_made_scans_open_in_pillow():
    Image = pytest.importorskip("PIL.Image")
    for name, (coef, mode, H, W) in JR.hand_made_scans().items():
        im = Image.open(io.BytesIO(JR.scan_file(coef, H, W, mode, 50)))
        im.load()
        assert im.size == (W, H), name


# ---- colour and levels -----------------------------------------------------------------------------------------------------------------------
def test_colour_conversion_is_within_one_level_of_jfif():
    v = np.arange(0, 256, 5)
    v[-1] = 255
    rgb = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    got = JR.ycc(rgb)
    r, g, b = (rgb[:, i].astype(np.float64) for i in range(3))
    want = np.stack([0.299 * r + 0.587 * g + 0.114 * b,
                     -0.168735892 * r - 0.331264108 * g + 0.5 * b + 128,
                     0.5 * r - 0.418687589 * g - 0.081312411 * b + 128], -1)
    assert np.abs(got - want).max() <= 1.0
    assert got.min() >= 0 and got.max() <= 255
    assert JR.ycc(np.array([[0, 0, 0], [255, 255, 255], [128, 128, 128]])).tolist() == [[0, 128, 128], [255, 128, 128], [128, 128, 128]]


def test_level_rule():
    check_level_rule()


def test_dc_predictors_run_across_mcu_rows():
    check_two_mcu_rows()


def test_downsampling_bias_alternates():
    check_downsampling_bias()


def test_channel_order():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)
    assert JR.encode(img, 90, "444", "bgr")[0] == JR.encode(img[..., ::-1], 90, "444", "rgb")[0] != JR.encode(img, 90, "444", "rgb")[0]


# ---- container --------------------------------------------------------------------------------------------------------------------------------
def riff_chunks(data, start, end):
    out = []
    p = start
    while p < end:
        tag, n = data[p:p + 4], struct.unpack("<I", data[p + 4:p + 8])[0]
        out.append((tag, p + 8, n))
        p += 8 + n + (n & 1)
    assert p == end
    return out


def test_write_avi(tmp_path):
    import dsnerf_amd
    rng = np.random.default_rng(4)
    files = [JR.encode(rng.integers(0, 256, (24, 40, 3), dtype=np.uint8), q, "420")[0] for q in (95, 20, 60)]
    assert len({len(f) & 1 for f in files}) >= 1
    paths = []
    for k, f in enumerate(files[:2]):
        paths.append(str(tmp_path / f"{k}.jpg"))
        open(paths[-1], "wb").write(f)
    path = str(tmp_path / "clip.avi")
    assert dsnerf_amd.jpeg.write_avi(path, paths + [files[2]], fps=25) == 3
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and struct.unpack("<I", data[4:8])[0] == len(data) - 8 and data[8:12] == b"AVI "
    top = riff_chunks(data, 12, len(data))
    assert [t for t, _, _ in top] == [b"LIST", b"LIST", b"idx1"]
    (_, h0, hn), (_, m0, mn), (_, i0, i_n) = top
    assert data[h0:h0 + 4] == b"hdrl" and data[m0:m0 + 4] == b"movi"
    hdrl = riff_chunks(data, h0 + 4, h0 + hn)
    assert [t for t, _, _ in hdrl] == [b"avih", b"LIST"] and hdrl[0][2] == 56
    avih = struct.unpack("<14I", data[hdrl[0][1]:hdrl[0][1] + 56])
    assert avih[0] == 40000 and avih[3] & 0x10 and avih[4] == 3 and avih[6] == 1 and avih[8:10] == (40, 24)
    assert avih[7] == max(len(f) for f in files)
    s0, sn = hdrl[1][1], hdrl[1][2]
    assert data[s0:s0 + 4] == b"strl"
    strl = riff_chunks(data, s0 + 4, s0 + sn)
    assert [t for t, _, _ in strl] == [b"strh", b"strf"] and strl[0][2] == 56 and strl[1][2] == 40
    strh = data[strl[0][1]:strl[0][1] + 56]
    assert strh[:8] == b"vidsMJPG"
    scale, rate, start, length = struct.unpack("<4I", strh[20:36])
    assert (scale, rate, start, length) == (1, 25, 0, 3) and struct.unpack("<4h", strh[48:56]) == (0, 0, 40, 24)
    strf = struct.unpack("<IiiHH4sIiiII", data[strl[1][1]:strl[1][1] + 40])
    assert strf[:6] == (40, 40, 24, 1, 24, b"MJPG")
    movi = riff_chunks(data, m0 + 4, m0 + mn)
    assert [t for t, _, _ in movi] == [b"00dc"] * 3
    idx = [struct.unpack("<4sIII", data[i0 + 16 * k:i0 + 16 * k + 16]) for k in range(3)]
    assert i_n == 48
    for k, ((tag, p, n), (itag, flags, off, size)) in enumerate(zip(movi, idx)):
        assert data[p:p + n] == files[k] and (itag, flags, size) == (b"00dc", 0x10, n)
        assert m0 + off == p - 8                             # offsets count from the 'movi' tag to the chunk's header
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        for tag, p, n in movi:
            im = Image.open(io.BytesIO(data[p:p + n]))
            im.load()
            assert im.size == (40, 24)
    assert dsnerf_amd.jpeg.write_avi(path, files, fps=29.97) == 3
    data = open(path, "rb").read()
    assert struct.unpack("<2I", data[data.index(b"strh") + 8 + 20:][:8]) == (1000, 29970)
    with pytest.raises(ValueError):
        dsnerf_amd.jpeg.write_avi(path, [])
    with pytest.raises(ValueError):
        dsnerf_amd.jpeg.write_avi(path, files + [JR.encode(np.zeros((8, 8, 3), np.uint8), 90, "420")[0]])


def test_readme_states_what_is_unverified():
    text = open(os.path.join(ROOT, "README.md")).read()
    assert "no player has opened" in text.lower() and "convertTo(CV_8U)" in text and "unverified" in text


# ---- the mutants ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutant_fails_its_named_test(fixture, mutant):
    check = globals()[MUTANTS[mutant]]
    args = (fixture,) if MUTANTS[mutant] == "check_fixture" else ()
    check(*args)                                             # the rule passes
    with pytest.raises(AssertionError):
        check(*args, mutant=mutant)
