"""Writes tests/golden/png_pillow.npz: PNG files and the pixels Pillow decodes from them, so that the tests need neither Pillow nor
anything else at run time.  Only PNG bytes and pixels are stored:
    meta            lines "<key> <origin> <W> <H> <bits> <ctype>"; png_<key> the file, px_<key> np.asarray(Image.open(...)) ("1" -> 0 / 255),
                    rgb_<key> Pillow's convert("RGB") for palette files (the others follow from px_)
    corrupt         lines "<key> <status bit's name or ok> <pillow: raised | decoded>"; bad_<key> the file
    refused         lines "<key> <reason>"; ref_<key> the file
Pillow-written files come in modes 1, L, P, RGB, RGBA, LA at compress_level 0, 1, 6, 9; hand-assembled ones (IHDR + filtered rows +
zlib.compressobj) force what encoders rarely produce.  Run from the repository root: python tests/golden/make_golden_png.py"""
import io
import os
import struct
import sys
import zlib

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import png_decode_restate as PR  # noqa: E402

SIG = b"\x89PNG\r\n\x1a\n"
CH = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
WIDTHS, HEIGHTS = [1, 2, 3, 7, 8, 9, 63, 64, 65, 257], [1, 2, 5]


class SBits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, n):          # least significant bit first
        self.v |= value << self.n
        self.n += n

    def code(self, value, n):         # a Huffman code: most significant bit first
        for k in range(n - 1, -1, -1):
            self.put(value >> k & 1, 1)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def chunk(typ, body, crc=None):
    c = zlib.crc32(typ + body) if crc is None else crc
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", c & 0xFFFFFFFF)


def ihdr(W, H, bits, ctype, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, bits, ctype, 0, 0, interlace))


def pack_rows(s, bits):
    """samples uint8 [H, W, C] -> the rows' bytes [H, row_bytes] (1 / 2 / 4 bits: most significant first, padded with zeros)"""
    H, W, C = s.shape
    if bits == 8:
        return s.reshape(H, W * C).copy()
    per = 8 // bits
    pad = (-W) % per
    v = np.concatenate([s[..., 0], np.zeros((H, pad), np.uint8)], 1).reshape(H, -1, per).astype(np.uint32)
    sh = (8 - bits - bits * np.arange(per)).astype(np.uint32)
    return (v << sh).sum(2).astype(np.uint8)


def filter_rows(rows, bpp, filters):
    """forward PNG filters: rows uint8 [H, rb] -> the bytes inflate must give (a filter byte before every row)"""
    H, rb = rows.shape
    out = bytearray()
    prev = np.zeros(rb, np.int64)
    for r in range(H):
        cur = rows[r].astype(np.int64)
        a = np.concatenate([np.zeros(bpp, np.int64), cur[:-bpp]]) if rb > bpp else np.zeros(rb, np.int64)
        if rb <= bpp:
            a = np.zeros(rb, np.int64)
        c = np.concatenate([np.zeros(bpp, np.int64), prev[:-bpp]]) if rb > bpp else np.zeros(rb, np.int64)
        b = prev
        ft = filters[r % len(filters)]
        if ft == 0:
            f = cur
        elif ft == 1:
            f = cur - a
        elif ft == 2:
            f = cur - b
        elif ft == 3:
            f = cur - ((a + b) >> 1)
        else:
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            f = cur - np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        out.append(ft)
        out += (f & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, sync_at=None):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    if sync_at is None:
        return co.compress(raw) + co.flush()
    return co.compress(raw[:sync_at]) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(raw[sync_at:]) + co.flush()


def assemble(W, H, bits, ctype, z, cut=None, palette=None, before=(), between=(), empty_idat=False):
    """a file around the zlib stream z: IDATs of `cut` bytes (None: one), ancillary chunks before and between them"""
    parts = [SIG, ihdr(W, H, bits, ctype)]
    parts += [chunk(t, b) for t, b in before]
    if palette is not None:
        parts.append(chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes()))
    pieces = [z] if cut is None else [z[k:k + cut] for k in range(0, len(z), cut)]
    for k, piece in enumerate(pieces):
        if empty_idat and k == 1:
            parts.append(chunk(b"IDAT", b""))
        parts.append(chunk(b"IDAT", piece))
        if k == 0:
            parts += [chunk(t, b) for t, b in between]
    if empty_idat and len(pieces) < 2:
        parts.append(chunk(b"IDAT", b""))
    parts.append(chunk(b"IEND", b""))
    return b"".join(parts)


def content(rng, H, W, C, maxval, kind):
    y, x = np.mgrid[0:H, 0:W]
    if kind == "noise":          # (four levels across the range above 3 bits: the fixture stays small, the streams keep their literals)
        if maxval < 8:
            return rng.integers(0, maxval + 1, (H, W, C), dtype=np.uint8)
        return (rng.integers(0, 4, (H, W, C), dtype=np.uint8) * (maxval // 3)).astype(np.uint8)
    if kind == "const":
        return np.full((H, W, C), maxval // 2 + 1 if maxval > 1 else 1, np.uint8)
    return np.stack([((x // 3 + y // 2 + k) % (maxval + 1)).astype(np.uint8) for k in range(C)], -1)


def blobs(n=1024, labels=20, seed=5):
    """a label map like the data sets' masks: discs of small integer labels on zero"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:n, 0:n]
    m = np.zeros((n, n), np.uint8)
    for k in range(40):
        cy, cx, r = rng.integers(0, n), rng.integers(0, n), rng.integers(20, 160)
        m[(y - cy) ** 2 + (x - cx) ** 2 < r * r] = 1 + k % labels
    return m


def palette_of(n, seed=9):
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)


def pillow_px(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    px = np.asarray(im.convert("L")) if im.mode == "1" else np.asarray(im)
    rgb = np.asarray(im.convert("RGB")) if im.mode == "P" else None
    return np.ascontiguousarray(px, np.uint8), rgb, im.mode


def main():
    rng = np.random.default_rng(2024)
    out, meta = {}, []

    def add(key, origin, data, for_pillow=None):
        info = PR.parse(data)
        assert info["reason"] == "ok", (key, info["reason"])
        px, rgb, mode = pillow_px(data if for_pillow is None else for_pillow)
        mine, st = PR.decode(data, "native")
        assert st == 0, (key, st)
        want = px[..., None] if px.ndim == 2 else px
        assert np.array_equal(mine, want), (key, mode)
        if rgb is not None:
            assert np.array_equal(PR.decode(data, "rgb")[0], rgb), key
            out[f"rgb_{key}"] = rgb
        out[f"png_{key}"] = np.frombuffer(data, np.uint8)
        out[f"px_{key}"] = px
        meta.append(f"{key} {origin} {info['W']} {info['H']} {info['bits']} {info['ctype']}")

    # ---- Pillow-written files
    def pillow_file(mode, W, H, level, kind):
        if mode == "1":
            im = Image.fromarray(content(rng, H, W, 1, 1, kind)[..., 0] * 255).convert("1")
        elif mode == "L":
            im = Image.fromarray(content(rng, H, W, 1, 255, kind)[..., 0], "L")
        elif mode == "P":
            im = Image.fromarray(content(rng, H, W, 1, 199, kind)[..., 0], "P")
            im.putpalette(palette_of(200).tobytes())
        else:
            im = Image.fromarray(content(rng, H, W, len(mode), 255, kind), mode)
        b = io.BytesIO()
        im.save(b, "PNG", compress_level=level)
        return b.getvalue()

    levels, kinds = [0, 1, 6, 9], ["noise", "ramp", "const"]
    n = 0
    for mode in ("1", "L", "P", "RGB", "RGBA", "LA"):
        for W in WIDTHS:
            for H in HEIGHTS:
                add(f"pil_{mode}_{W}x{H}", "pillow", pillow_file(mode, W, H, levels[n % 4], kinds[n % 3]))
                n += 1
        for level in levels:
            add(f"pil_{mode}_130x70_l{level}", "pillow", pillow_file(mode, 130, 70, level, kinds[level % 3]))
    for bits in (1, 2, 4):          # palette files below 8 bits
        for W in (1, 3, 5, 9, 65):
            im = Image.fromarray(content(rng, 5, W, 1, (1 << bits) - 1, "noise")[..., 0], "P")
            im.putpalette(palette_of(1 << bits).tobytes())
            b = io.BytesIO()
            im.save(b, "PNG", bits=bits)
            add(f"pil_P{bits}_{W}x5", "pillow", b.getvalue())

    # ---- hand-assembled files
    def hand(key, W, H, bits, ctype, kind="ramp", filters=(0, 1, 2, 3, 4), level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, sync_at=None,
             rows=None, **kw):
        C = CH[ctype]
        if rows is None:
            rows = pack_rows(content(rng, H, W, C, (1 << bits) - 1, kind), bits)
        raw = filter_rows(rows, max(1, bits * C // 8), filters)
        z = deflate(raw, level, strategy, wbits, None if sync_at is None else len(raw) // 2)
        assert zlib.decompress(z) == raw
        if ctype == 3 and "palette" not in kw:
            kw["palette"] = palette_of(1 << bits)
        # (Pillow takes the first chunk that is not IDAT as the stream's end: it is shown the same file without the chunks between)
        plain = assemble(W, H, bits, ctype, z, **{k: v for k, v in kw.items() if k != "between"}) if "between" in kw else None
        add(key, "hand", assemble(W, H, bits, ctype, z, **kw), plain)
        return z

    strategies = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE}
    kinds_c = {0: "L", 2: "RGB", 3: "P", 4: "LA", 6: "RGBA"}
    # every filter on every row position (a rotation per file: Up, Average and Paeth on row 0 too), every strategy, 5-byte IDATs
    n = 0
    for ctype in (0, 2, 3, 4, 6):
        for W in (1, 3, 65):
            for rot in range(5):
                sname = list(strategies)[n % 4]
                hand(f"hand_{kinds_c[ctype]}_{W}x7_f{rot}_{sname}", W, 7, 8, ctype, kind=kinds[n % 2], filters=[(rot + k) % 5 for k in range(5)],
                     strategy=strategies[sname], level=[6, 0, 9, 1][n % 4], cut=5)
                n += 1
    # grey and palette below 8 bits at widths that do not fill the last byte
    for ctype in (0, 3):
        for bits in (1, 2, 4):
            for W in (1, 2, 3, 7, 8, 9, 63, 64, 65, 257):
                for H in ((1, 2, 5) if W in (1, 9, 257) else (5,)):
                    hand(f"hand_{kinds_c[ctype]}{bits}_{W}x{H}", W, H, bits, ctype, kind="noise", filters=[(W + k) % 5 for k in range(5)])
            hand(f"hand_{kinds_c[ctype]}{bits}_130x70", 130, 70, bits, ctype, kind="noise")
    for ctype in (0, 2, 3, 4, 6):
        hand(f"hand_{kinds_c[ctype]}_130x70", 130, 70, 8, ctype, kind="noise", filters=(4, 3, 1, 2, 0))
        hand(f"hand_{kinds_c[ctype]}_257x5", 257, 5, 8, ctype, kind="ramp", filters=(3, 4))
    # the zlib corners
    hand("hand_stored_1byte", 65, 5, 8, 2, kind="noise", level=0, cut=1)
    hand("hand_dynamic_1byte", 64, 9, 8, 0, kind="ramp", cut=1)
    hand("hand_cut8192", 170, 170, 8, 2, kind="noise", level=1, cut=8192)
    hand("hand_empty_idat", 63, 5, 8, 0, cut=40, empty_idat=True)
    hand("hand_sync_flush", 130, 20, 8, 0, sync_at=True, cut=5)
    hand("hand_sync_flush_fixed", 9, 5, 8, 6, sync_at=True, strategy=zlib.Z_FIXED)
    hand("hand_wbits9", 257, 40, 8, 0, kind="ramp", wbits=9)
    hand("hand_wbits9_noise", 130, 70, 8, 2, kind="noise", wbits=9, strategy=zlib.Z_FIXED)
    hand("hand_const_rows", 1000, 9, 8, 0, kind="const", filters=(0,))          # matches of length 258 at distance 1
    hand("hand_const_rows_rle", 600, 7, 8, 6, kind="const", filters=(0, 2), strategy=zlib.Z_RLE)
    per = rng.integers(0, 4, (2, 16383), dtype=np.uint8) * 85          # two rows and their filter bytes: 32768 bytes, then the same again
    hand("hand_period_32768", 16383, 6, 8, 0, rows=np.tile(per, (3, 1)), filters=(0,), level=9)
    hand("hand_period_8192", 8191, 6, 8, 0, rows=np.repeat(per[:1, :8191], 6, 0), filters=(0,), level=9)
    hand("hand_one_period", 64, 40, 8, 0, rows=np.repeat(rng.integers(0, 4, (1, 64), dtype=np.uint8), 40, 0), filters=(0,), level=9)
    # zlib always sends two distance codes: a dynamic block with ONE distance code (length 1: an incomplete set zlib accepts) by hand -
    # literal/length lengths {0: 2, 256: 2, 257: 1}, a zero byte and 21 matches of length 3 at distance 1: 4 rows of 15 zero pixels
    sb = SBits(); sb.put(1, 1); sb.put(2, 2); sb.put(1, 5); sb.put(0, 5); sb.put(14, 4)
    for sym in PR.ORDER[:18]:
        sb.put({18: 1, 1: 2, 2: 2}.get(sym, 0), 3)
    sb.code(0b11, 2)                                            # symbol 0: length 2
    sb.code(0, 1); sb.put(127, 7); sb.code(0, 1); sb.put(106, 7)          # 138 + 117 zeros: symbols 1 ... 255
    sb.code(0b11, 2); sb.code(0b10, 2); sb.code(0b10, 2)        # 256: 2, 257: 1, the distance code: 1
    sb.code(0b10, 2)
    for _ in range(21):
        sb.code(0, 1); sb.code(0, 1)
    sb.code(0b11, 2)
    zs = b"\x78\x9c" + sb.bytes() + struct.pack(">I", zlib.adler32(bytes(64)))
    assert zlib.decompress(zs) == bytes(64)
    add("hand_single_distance_code", "hand", assemble(15, 4, 8, 0, zs))
    hand("hand_ancillary", 33, 9, 8, 3, cut=16, before=[(b"gAMA", struct.pack(">I", 45455)), (b"tEXt", b"Comment\0made by hand")],
         between=[(b"tIME", bytes(7)), (b"zzTp", b"private")])
    hand("hand_huffman_130x70", 130, 70, 8, 6, kind="noise", strategy=zlib.Z_HUFFMAN_ONLY, filters=(1, 4))
    # the masks' own shape: a 1024 x 1024 label map of blobs as grey, palette and three-channel
    m = blobs()
    for name, im in (("L", Image.fromarray(m, "L")), ("P", Image.fromarray(m, "P")), ("RGB", Image.fromarray(np.repeat(m[..., None], 3, 2), "RGB"))):
        if name == "P":
            im.putpalette(palette_of(256).tobytes())
        b = io.BytesIO()
        im.save(b, "PNG")
        add(f"mask_{name}_1024", "pillow", b.getvalue())

    # ---- corrupt files: accepted by the parser, flagged by the decoder
    corrupt = []

    def pillow_verdict(data):
        try:
            Image.open(io.BytesIO(data)).load()
            return "decoded"
        except Exception:
            return "raised"

    def add_bad(key, expect, data):
        info = PR.parse(data)
        assert info["reason"] == "ok", (key, info["reason"])
        st = PR.stages(data)["status"]
        assert st == (PR.STATUS_BITS[expect] if expect != "ok" else 0), (key, expect, st)
        out[f"bad_{key}"] = np.frombuffer(data, np.uint8)
        corrupt.append(f"{key} {expect} {pillow_verdict(data)}")

    W, H = 37, 11
    rows = pack_rows(content(rng, H, W, 3, 255, "ramp"), 8)
    raw = filter_rows(rows, 3, (0, 1, 2, 3, 4))
    z = deflate(raw)

    hdr = b"\x78\x9c"
    tail = struct.pack(">I", zlib.adler32(raw))
    add_bad("early_end", "early_end", assemble(W, H, 8, 2, z[:len(z) // 2]))
    add_bad("early_end_stored", "early_end", assemble(W, H, 8, 2, deflate(raw, 0)[:200]))
    add_bad("early_end_no_adler", "early_end", assemble(W, H, 8, 2, z[:-2]))
    b = SBits(); b.put(1, 1); b.put(3, 2)
    add_bad("block_type", "block_type", assemble(W, H, 8, 2, hdr + b.bytes() + bytes(8)))
    z0 = bytearray(deflate(raw, 0))
    z0[5] ^= 0x10                                                # NLEN of the first stored block
    add_bad("stored_len", "stored_len", assemble(W, H, 8, 2, bytes(z0)))
    b = SBits(); b.put(1, 1); b.put(2, 2); b.put(0, 5); b.put(0, 5); b.put(15, 4)
    for _ in range(19):
        b.put(1, 3)                                              # nineteen code-length codes of length 1
    add_bad("bad_codes_oversubscribed", "bad_codes", assemble(W, H, 8, 2, hdr + b.bytes() + bytes(8)))
    b = SBits(); b.put(1, 1); b.put(2, 2); b.put(0, 5); b.put(0, 5); b.put(0, 4)
    b.put(1, 3); b.put(0, 3); b.put(0, 3); b.put(0, 3)           # one single code-length code: incomplete
    add_bad("bad_codes_incomplete", "bad_codes", assemble(W, H, 8, 2, hdr + b.bytes() + bytes(8)))
    b = SBits(); b.put(1, 1); b.put(1, 2); b.code(0b00110000 + 65, 8); b.code(0b11000110, 8)          # 'A', then symbol 286
    add_bad("no_code", "no_code", assemble(W, H, 8, 2, hdr + b.bytes() + bytes(8)))
    b = SBits(); b.put(1, 1); b.put(1, 2); b.code(0b00110000 + 65, 8); b.code(0b0000001, 7); b.code(30, 5)          # distance symbol 30
    add_bad("no_code_distance", "no_code", assemble(W, H, 8, 2, hdr + b.bytes() + bytes(8)))
    b = SBits(); b.put(1, 1); b.put(1, 2); b.code(0b00110000 + 65, 8); b.code(0b0000001, 7); b.code(1, 5); b.code(0, 7)   # length 3 at distance 2
    add_bad("far_distance", "far_distance", assemble(W, H, 8, 2, hdr + b.bytes() + bytes(8)))
    b = SBits(); b.put(1, 1); b.put(1, 2); b.code(0b0000001, 7); b.code(0, 5); b.code(0, 7)
    add_bad("far_distance_at_start", "far_distance", assemble(W, H, 8, 2, hdr + b.bytes() + bytes(8)))
    more = raw + raw[:1 + 3 * W]
    add_bad("too_much", "too_much", assemble(W, H, 8, 2, deflate(more)))
    add_bad("too_much_stored", "too_much", assemble(W, H, 8, 2, deflate(more, 0)))
    add_bad("too_much_match", "too_much", assemble(64, 4, 8, 0, deflate(bytes(65 * 4 + 200))))
    add_bad("too_little", "too_little", assemble(W, H, 8, 2, deflate(raw[:-(1 + 3 * W)])))
    add_bad("too_little_empty", "too_little", assemble(W, H, 8, 2, deflate(b"")))
    bad = bytearray(raw)
    bad[4 * (1 + 3 * W)] = 5
    add_bad("filter", "filter", assemble(W, H, 8, 2, deflate(bytes(bad))))
    bad[4 * (1 + 3 * W)] = 255
    add_bad("filter_255", "filter", assemble(W, H, 8, 2, deflate(bytes(bad))))
    add_bad("adler", "adler", assemble(W, H, 8, 2, z[:-1] + bytes([z[-1] ^ 1])))
    add_bad("adler_high", "adler", assemble(W, H, 8, 2, z[:-4] + bytes([z[-4] ^ 0x80]) + z[-3:]))
    add_bad("trailing_garbage", "ok", assemble(W, H, 8, 2, z + b"garbage behind the stream", cut=7))
    out[f"px_trailing_garbage"] = pillow_px(assemble(W, H, 8, 2, z))[0]

    # ---- refused by the parser
    refused = []

    def add_ref(key, reason, data):
        assert PR.parse(data)["reason"] == reason, (key, reason, PR.parse(data)["reason"])
        out[f"ref_{key}"] = np.frombuffer(data, np.uint8)
        refused.append(f"{key} {reason}")

    good = assemble(W, H, 8, 2, z)
    pal_file = assemble(9, 5, 8, 3, deflate(filter_rows(pack_rows(content(rng, 5, 9, 1, 7, "noise"), 8), 1, (0,))), palette=palette_of(8))
    at = {t: pal_file.index(t) for t in (b"IHDR", b"PLTE", b"IDAT", b"IEND")}
    add_ref("not_png", "not_png", b"\xff\xd8\xff\xe0" + bytes(40))
    add_ref("short", "not_png", SIG[:5])
    for t in (b"IHDR", b"PLTE", b"IDAT"):
        d = bytearray(pal_file)
        d[at[t] + 5] ^= 1
        add_ref(f"crc_{t.decode()}", "crc", bytes(d))
    d = bytearray(pal_file)
    d[-1] ^= 1
    add_ref("crc_IEND", "crc", bytes(d))
    add_ref("interlace", "interlace", SIG + ihdr(W, H, 8, 2, 1) + chunk(b"IDAT", z) + chunk(b"IEND", b""))
    b16 = io.BytesIO()
    Image.fromarray((np.arange(35, dtype=np.uint16) * 1000).reshape(5, 7)).save(b16, "PNG")
    add_ref("depth16", "depth16", b16.getvalue())
    add_ref("depth16_rgb", "depth16", SIG + ihdr(W, H, 16, 2) + chunk(b"IDAT", z) + chunk(b"IEND", b""))
    add_ref("no_ihdr", "no_ihdr", SIG + chunk(b"IDAT", z) + chunk(b"IEND", b""))
    add_ref("no_idat", "no_idat", SIG + ihdr(W, H, 8, 2) + chunk(b"IEND", b""))
    add_ref("no_idat_empty", "no_idat", SIG + ihdr(W, H, 8, 2) + chunk(b"IDAT", b"") + chunk(b"IDAT", b"\x78") + chunk(b"IEND", b""))
    add_ref("no_plte", "no_plte", SIG + ihdr(9, 5, 8, 3) + pal_file[at[b"IDAT"] - 4:])
    add_ref("zero_width", "zero_dim", SIG + ihdr(0, H, 8, 2) + chunk(b"IDAT", z) + chunk(b"IEND", b""))
    add_ref("zero_height", "zero_dim", SIG + ihdr(W, 0, 8, 2) + chunk(b"IDAT", z) + chunk(b"IEND", b""))
    add_ref("too_wide", "too_large", SIG + ihdr(16385, 1, 8, 0) + chunk(b"IDAT", z) + chunk(b"IEND", b""))
    add_ref("too_many_bytes", "too_large", SIG + ihdr(16384, 16384, 8, 6) + chunk(b"IDAT", z) + chunk(b"IEND", b""))
    add_ref("zlib_method", "zlib_method", assemble(W, H, 8, 2, bytes([0x77, 31 - (0x7700 % 31)]) + z[2:]))
    add_ref("zlib_window", "zlib_method", assemble(W, H, 8, 2, bytes([0x88, 31 - (0x8800 % 31)]) + z[2:]))
    flg = 0x20
    flg += 31 - ((0x7800 + flg) % 31)
    add_ref("zlib_dict", "zlib_dict", assemble(W, H, 8, 2, bytes([0x78, flg]) + z[2:]))
    add_ref("zlib_check", "zlib_check", assemble(W, H, 8, 2, bytes([0x78, 0x9d]) + z[2:]))
    add_ref("truncated_chunk", "truncated", good[:len(good) - 30])
    add_ref("truncated_no_iend", "truncated", good[:-12])
    add_ref("bad_ihdr_depth", "bad_ihdr", SIG + ihdr(W, H, 4, 2) + chunk(b"IDAT", z) + chunk(b"IEND", b""))

    out["meta"] = np.array(meta)
    out["corrupt"] = np.array(corrupt)
    out["refused"] = np.array(refused)
    path = os.path.join(HERE, "png_pillow.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(meta), "files,", len(corrupt), "corrupt,", len(refused), "refused")


if __name__ == "__main__":
    main()
