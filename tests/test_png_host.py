"""PNG decoding, the part that needs no GPU: the numpy restatement (tests/png_decode_restate.py: its own CRC-32, bit reader, inflate,
Adler-32, unfilter and pixel rule) against zlib.decompress and against the pixels Pillow decoded (tests/golden/png_pillow.npz, written
by tests/golden/make_golden_png.py; fresh files where Pillow imports), its status words against the recorded ones, and
dsn_png_parse_host through the library: descriptor fields, segment tables, every refusal, null and short arguments."""
import ctypes as C
import io
import os
import zlib

import numpy as np
import pytest

import dsnerf_amd.png  # noqa: F401  (every test here is about this module)
import png_decode_restate as PR
from helpers import ROOT


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(ROOT, "tests", "golden", "png_pillow.npz"))


@pytest.fixture(scope="module")
def L():
    import dsnerf_amd
    import dsnerf_amd.png  # noqa: F401
    return dsnerf_amd._lib


def keys(G):
    return [str(line).split()[0] for line in G["meta"]]


_stages = {}


def stages_of(G, k):
    if k not in _stages:
        _stages[k] = PR.stages(G[f"png_{k}"].tobytes())
    return _stages[k]


def test_fixture_covers_the_grid(G):
    meta = [str(m).split() for m in G["meta"]]
    assert len(meta) > 400
    kinds = {(int(m[4]), int(m[5])) for m in meta}
    assert kinds == {(1, 0), (2, 0), (4, 0), (8, 0), (8, 2), (1, 3), (2, 3), (4, 3), (8, 3), (8, 4), (8, 6)}
    for W in (1, 2, 3, 7, 8, 9, 63, 64, 65, 257):
        for H in (1, 2, 5):
            assert any(int(m[2]) == W and int(m[3]) == H for m in meta), (W, H)
    assert sum(int(m[2]) == 1024 and int(m[3]) == 1024 for m in meta) == 3
    assert {str(c).split()[1] for c in G["corrupt"]} == set(PR.STATUS_BITS) | {"ok"}
    assert {str(c).split()[1] for c in G["refused"]} == set(PR.REASONS) - {"ok"}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "png_pillow.npz")) < (1 << 20)


def test_checksums_are_zlibs():
    rng = np.random.default_rng(1)
    for n in (0, 1, 2, 15, 16, 17, 5551, 5552, 5553, 70000):
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert PR.crc32(d) == zlib.crc32(d) and PR.adler32(d) == zlib.adler32(d), n
    assert PR.adler32(b"\xff" * 300000) == zlib.adler32(b"\xff" * 300000)


def test_restated_inflate_is_zlib_decompress(G):
    seen = set()
    for k in keys(G):
        s = stages_of(G, k)
        z = s["stream"]
        d = zlib.decompressobj()
        assert s["raw"] == d.decompress(z) and s["status"] == 0, k
        assert s["adler"] == zlib.adler32(s["raw"]) == s["stored"], k
        assert (s["endbit"] + 7) // 8 + 4 == len(z) - len(d.unused_data), k
        seen.add(z[2] >> 1 & 3)          # the first block's type
    assert seen == {0, 1, 2}


def test_restated_pixels_are_pillows(G):
    for k in keys(G):
        s = stages_of(G, k)
        info, rows = s["info"], s["rows"]
        want = G[f"px_{k}"]
        nat = PR.pixels(rows, info, "native")
        assert np.array_equal(nat, want[..., None] if want.ndim == 2 else want), k
        rgb = G[f"rgb_{k}"] if f"rgb_{k}" in G.files else np.repeat(want[..., None], 3, 2) if want.ndim == 2 else \
            np.repeat(want[..., :1], 3, 2) if want.shape[2] == 2 else want[..., :3]
        assert np.array_equal(PR.pixels(rows, info, "rgb"), rgb), k
        assert np.array_equal(PR.pixels(rows, info, "bgr"), rgb[..., ::-1]), k
        assert np.array_equal(PR.pixels(rows, info, "bgr", True), rgb[..., 2]) and np.array_equal(PR.pixels(rows, info, "native", True), nat[..., 0]), k


def test_restatement_on_fresh_pillow_files():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    n = 0
    for mode, C in (("L", 1), ("RGB", 3), ("RGBA", 4), ("LA", 2), ("P", 1), ("1", 1)):
        for W, H in ((1, 1), (5, 3), (31, 17), (100, 41)):
            for level in (0, 3, 9):
                a = rng.integers(0, 256, (H, W, C), dtype=np.uint8) >> int(rng.integers(0, 7))
                im = Image.fromarray(a[..., 0] if C == 1 else a, "L" if mode in ("P", "1") else mode)
                if mode == "P":
                    im = im.convert("P")
                    im.putpalette(rng.integers(0, 256, 768, dtype=np.uint8).tobytes())
                elif mode == "1":
                    im = im.point(lambda v: 255 * (v & 1)).convert("1")
                b = io.BytesIO()
                im.save(b, "PNG", compress_level=level)
                back = Image.open(io.BytesIO(b.getvalue()))
                px, st = PR.decode(b.getvalue(), "rgb")
                assert st == 0 and np.array_equal(px, np.asarray(back.convert("RGB"))), (mode, W, H, level)
                nat = np.asarray(back.convert("L") if mode == "1" else back)
                assert np.array_equal(PR.decode(b.getvalue(), "native")[0], nat[..., None] if nat.ndim == 2 else nat), (mode, W, H, level)
                n += 1
    assert n == 72


def test_restated_status_is_the_recorded_one(G):
    for line in G["corrupt"]:
        k, expect, pillow = str(line).split()
        data = G[f"bad_{k}"].tobytes()
        px, st = PR.decode(data)
        assert st == (PR.STATUS_BITS[expect] if expect != "ok" else 0), (k, expect, st)
        if expect == "ok":
            assert pillow == "decoded" and np.array_equal(px, G[f"px_{k}"][..., ::-1])
        else:
            assert not px.any(), k
        if k in ("adler", "early_end"):
            assert pillow == "raised", k          # Pillow raises OSError for a flipped Adler byte and for a stream cut in half
    # (recorded too: Pillow decodes a stream that lacks only its last Adler bytes, having all the rows by then)


def test_overlapping_matches_repeat_their_bytes():
    """distance < length, distance 1 included: byte i of the copy is out[start - dist + (i mod dist)]"""
    for period in (1, 2, 3, 7, 64, 257):
        raw = bytes((7 * k + period) & 255 for k in range(period)) * (2000 // period + 2)
        for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_RLE, zlib.Z_FIXED):
            co = zlib.compressobj(9, zlib.DEFLATED, 15, 9, strategy)
            z = co.compress(raw) + co.flush()
            out, st, stored, _ = PR.inflate(z, len(raw))
            assert out == raw and st == 0 and stored == zlib.adler32(raw), (period, strategy)


# ---- the library's host part -------------------------------------------------------------------------------------------------------------
def test_parse_host_is_the_restatement(G, L):
    for k in keys(G):
        data = G[f"png_{k}"].tobytes()
        info = PR.parse(data)
        d, segs, st = L.png_parse(data, seg_capacity=3)          # (files with more IDATs are parsed a second time with room for all)
        assert st == 0 and L.PNG_REASONS[st] == info["reason"], k
        for f in ("W", "H", "bits", "ctype", "channels", "row_bytes", "raw_bytes", "npal", "zlen"):
            assert int(getattr(d, f)) == info[f], (k, f)
        assert int(d.nseg) == len(info["segs"]) and segs == info["segs"] and int(d.file_length) == len(data), k
        assert np.array_equal(np.frombuffer(bytes(d.palette), np.uint8).reshape(256, 3), info["palette"]), k
    many = [k for k in keys(G) if len(PR.parse(G[f"png_{k}"].tobytes())["segs"]) > 500]
    assert many          # one-byte IDATs


def test_parse_host_refusals(G, L):
    for line in G["refused"]:
        k, reason = str(line).split()
        data = G[f"ref_{k}"].tobytes()
        assert PR.parse(data)["reason"] == reason, k
        assert L.PNG_REASONS[L.png_parse(data)[2]] == reason, k


def test_parse_host_on_every_prefix_and_on_flipped_bytes(G, L):
    """every read is bounded by the file's length: each prefix of a file, and the file with any one byte changed, gets the
    restatement's verdict"""
    for k in ("hand_ancillary", "pil_P_9x5"):
        data = G[f"png_{k}"].tobytes()
        for cut in range(len(data) + 1):
            piece = data[:cut]
            assert L.PNG_REASONS[L.png_parse(piece)[2]] == PR.parse(piece)["reason"], (k, cut)
        for at in range(len(data)):
            bad = bytearray(data)
            bad[at] ^= 0x41
            assert L.PNG_REASONS[L.png_parse(bytes(bad))[2]] == PR.parse(bytes(bad))["reason"], (k, at)


def test_null_and_short_arguments(L):
    lib = L.lib()
    d, st = L.PngDesc(), C.c_int(0)
    segs = (C.c_uint32 * 8)()
    assert lib.dsn_png_parse_host(None, 0, C.byref(d), segs, 4, C.byref(st)) != 0 and b"dsn_png_parse_host" in lib.dsn_last_error()
    assert lib.dsn_png_parse_host(b"x", 1, None, segs, 4, C.byref(st)) != 0
    assert lib.dsn_png_parse_host(b"x", 1, C.byref(d), segs, 4, None) != 0
    assert lib.dsn_png_parse_host(b"x", 1, C.byref(d), None, 4, C.byref(st)) != 0 and b"seg_capacity" in lib.dsn_last_error()
    assert lib.dsn_png_parse_host(b"", 0, C.byref(d), None, 0, C.byref(st)) == 0 and st.value == L.PNG_REASONS.index("not_png")
    assert C.sizeof(L.PngDesc) == 64 + 768
    # sizes: zero for what the decoder does not take
    ws = lib.dsn_png_workspace_bytes
    assert ws(1, 64, 64, 8, 2, 1000) > 64 * (1 + 192) + 64 * 192 + 1000
    for bad in ((0, 64, 64, 8, 2), (1, 0, 64, 8, 2), (1, 64, 0, 8, 2), (1, 16385, 1, 8, 0), (1, 64, 64, 16, 0), (1, 64, 64, 4, 2), (1, 64, 64, 8, 5),
                (1, 16384, 16384, 8, 6), (16385, 1, 1, 8, 0)):
        assert ws(*bad, 1000) == 0, bad
    assert ws(1, 64, 64, 8, 2, (1 << 28) + 1) == 0
    lay = (C.c_size_t * 8)()
    assert lib.dsn_png_workspace_layout(2, 64, 64, 8, 2, 1000, lay) == 0 and lay[7] == ws(2, 64, 64, 8, 2, 1000)
    assert all(int(lay[i]) % 256 == 0 for i in (0, 1, 3, 5)) and lay[0] < lay[1] < lay[3] < lay[5] < lay[7]
    assert lay[2] >= 1000 and lay[4] >= 64 * 193 and lay[6] >= 64 * 192
    assert lib.dsn_png_workspace_layout(2, 64, 64, 8, 2, 1000, None) != 0
    assert lib.dsn_png_workspace_layout(2, 64, 64, 8, 5, 1000, lay) != 0 and b"dsn_png_workspace_layout" in lib.dsn_last_error()
    # the decode entry point checks its arguments before touching the device
    one = C.c_void_p(256)
    z = None
    dec = lib.dsn_png_decode
    assert dec(z, 0, z, 0, z, z, 1, 64, 64, 8, 2, 1000, 0, 0, 31, z, z, z, 0, z) != 0 and b"dsn_png_decode" in lib.dsn_last_error()
    assert dec(one, 16, one, 1, one, one, 1, 64, 64, 8, 5, 1000, 0, 0, 31, one, one, one, 1 << 30, z) != 0 and b"bits / ctype" in lib.dsn_last_error()
    assert dec(one, 16, one, 1, one, one, 1, 64, 64, 8, 2, 1000, 3, 0, 31, one, one, one, 1 << 30, z) != 0 and b"channels" in lib.dsn_last_error()
    assert dec(one, 16, one, 1, one, one, 1, 64, 64, 8, 2, 1000, 0, 0, 0, one, one, one, 1 << 30, z) != 0 and b"stages" in lib.dsn_last_error()
    assert dec(one, 16, one, 1, one, one, 1, 64, 64, 8, 2, 1000, 0, 0, 31, one, one, one, 100, z) != 0 and b"workspace_bytes" in lib.dsn_last_error()
    assert dec(one, 16, one, 1, one, one, 1, 64, 64, 8, 2, 1000, 0, 0, 31, one, one, C.c_void_p(264), 1 << 30, z) != 0 and b"aligned" in lib.dsn_last_error()
    assert dec(one, 16, one, 1, one, one, 1, 64, 64, 8, 2, 1000, 0, 0, 31, z, one, one, 1 << 30, z) != 0 and b"out is null" in lib.dsn_last_error()
    assert dec(one, 16, one, 1, one, one, 16385, 64, 64, 8, 2, 1000, 0, 0, 31, one, one, one, 1 << 30, z) != 0
    assert dec(z, 0, z, 0, z, z, 0, 64, 64, 8, 2, 1000, 0, 0, 31, z, z, z, 0, z) == 0          # no files: nothing to do


def test_modules_name_each_other(tmp_path, G):
    import dsnerf_amd
    p = tmp_path / "mask.png"
    p.write_bytes(G["png_pil_L_9x5"].tobytes())
    with pytest.raises(ValueError, match="dsnerf_amd.png"):
        dsnerf_amd.jpeg.imread(str(p))
    q = tmp_path / "frame.jpg"
    q.write_bytes(b"\xff\xd8\xff\xe0" + bytes(32))
    with pytest.raises(ValueError, match="dsnerf_amd.jpeg"):
        dsnerf_amd.png.imread(str(q))
    with pytest.raises(ValueError, match="not_png.*dsnerf_amd.jpeg"):
        dsnerf_amd.png.decode(b"\xff\xd8\xff\xe0" + bytes(32), names=["frame"])
    with pytest.raises(ValueError, match="interlace"):
        dsnerf_amd.png.decode(G["ref_interlace"].tobytes())
    with pytest.raises(ValueError, match="channels"):
        dsnerf_amd.png.decode(G["png_pil_L_9x5"].tobytes(), channels="gbr")
