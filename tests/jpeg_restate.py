"""numpy restatement of the baseline JPEG rule written out in include/dsnerf.h (dsn_jpeg_*): levels, JFIF colour, libjpeg's edge
and downsampling rules, the IJG slow-integer DCT, Annex K quantisation and Huffman tables, byte stuffing and the header Pillow
writes.  Vectorised over blocks; a 256 x 256 frame takes about a second.

    encode(img, quality, subsampling, channels, scale, mutant=None) -> (bytes, status)
    coefficients(img, ...) -> (int16 [blocks, 64] in zigzag and scan order, status)
    entropy_encode(coef, mode) -> the scan's bytes (stuffed, padded), no header, no EOI
    scan_file(coef, H, W, mode, quality) -> the complete file around hand-made coefficients
    decode_scan(scan_bytes, n_blocks, mode) -> the coefficient array back (a small Huffman decoder)
    fdct_float64(blocks) -> the float64 twin of fdct(blocks) / 8

`mutant` names one deliberate mistake (tests show that each fails a named test):
    "no_stuffing", "zero_padding", "half_up_levels", "swap_rb", "dc_reset_per_row", "flat_bias"
"""
import numpy as np

M420, M444, MGRAY = 0, 1, 2
MODES = {"420": M420, "444": M444, "gray": MGRAY, "grey": MGRAY}
NONFINITE, OVERFLOW = 1, 2

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])          # zigzag position -> natural (row * 8 + column) index

Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                   80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                   95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
                     99, 99, 99] + [99] * 32)

DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
AC_VALS = (
    [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51,
     98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84,
     85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136,
     137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183,
     184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229,
     230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250],
    [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98,
     114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74,
     83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133,
     134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180,
     181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227,
     228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250])


def huff_table(bits, vals):
    """(code [256], length [256]) of a table given as Annex C does: codes of each length count upwards, lengths ascending"""
    code = np.zeros(256, np.int64)
    length = np.zeros(256, np.int64)
    c, k = 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            code[vals[k]], length[vals[k]] = c, ln
            c += 1
            k += 1
        c <<= 1
    return code, length


DC_TAB = [huff_table(DC_BITS[t], DC_VALS[t]) for t in (0, 1)]
AC_TAB = [huff_table(AC_BITS[t], AC_VALS[t]) for t in (0, 1)]


def mode_of(subsampling, C):
    return MGRAY if C == 1 else MODES[str(subsampling)]


def geometry(H, W, mode):
    """(MCU columns, MCU rows, blocks per MCU, component of each block of an MCU)"""
    if mode == M420:
        return (W + 15) // 16, (H + 15) // 16, 6, np.array([0, 0, 0, 0, 1, 2])
    if mode == M444:
        return (W + 7) // 8, (H + 7) // 8, 3, np.array([0, 1, 2])
    return (W + 7) // 8, (H + 7) // 8, 1, np.array([0])


def n_blocks(H, W, mode):
    mw, mh, bpm, _ = geometry(H, W, mode)
    return mw * mh * bpm


def quant_tables(quality):
    """the two tables in natural order for quality 1 ... 100"""
    q = int(quality)
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return [np.clip((base * s + 50) // 100, 1, 255).astype(np.int64) for base in (Q_LUMA, Q_CHROMA)]


def levels(img, scale=255.0, mutant=None):
    """uint8 passes; float32: v * scale in float32, nearest with ties to even, saturated, NaN -> 0.  -> (uint8, non-finite seen)"""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img, False
    assert img.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        t = img * np.float32(scale)
        bad = not bool(np.isfinite(img).all())
        r = np.floor(t + np.float32(0.5)) if mutant == "half_up_levels" else np.rint(t)
        r = np.where(np.isnan(t), np.float32(0), np.clip(r, 0, 255))
    return r.astype(np.uint8), bad


def ycc(rgb):
    """JFIF YCbCr in 16-bit fixed point: int64 [..., 3] from levels [..., 3] (R, G, B)"""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return np.stack([y, cb, cr], -1)


def _pad_to(p, h, w):
    """replicate right and down"""
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")


def _blocks(p):
    """[h, w] -> [h / 8, w / 8, 8, 8]"""
    h, w = p.shape
    return p.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def sample_blocks(u8, mode, channels="bgr", mutant=None):
    """the MCUs' sample blocks in scan order, int64 [blocks, 8, 8] (levels, before the shift by 128), and which of them are dummy"""
    H, W = u8.shape[:2]
    mw, mh, bpm, _ = geometry(H, W, mode)
    if mode == MGRAY:
        b = _blocks(_pad_to(u8.reshape(H, W).astype(np.int64), mh * 8, mw * 8))
        return b.reshape(-1, 8, 8), np.zeros(mw * mh, bool)
    rgb = u8 if (channels == "rgb") != (mutant == "swap_rb") else u8[..., ::-1]
    c = ycc(rgb)
    if mode == M444:
        b = np.stack([_blocks(_pad_to(c[..., k], mh * 8, mw * 8)) for k in range(3)], 2)          # [mh, mw, 3, 8, 8]
        return b.reshape(-1, 8, 8), np.zeros(mw * mh * 3, bool)
    bw, bh = (W + 7) // 8, (H + 7) // 8
    yb = _blocks(_pad_to(_pad_to(c[..., 0], bh * 8, bw * 8), mh * 16, mw * 16))                   # [2 mh, 2 mw, 8, 8]; beyond bh / bw: dummy
    yb = yb.reshape(mh, 2, mw, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(mh, mw, 4, 8, 8)
    by = (np.arange(mh)[:, None, None] * 2 + np.array([0, 0, 1, 1])[None, None, :]) + np.zeros((1, mw, 1), int)
    bx = (np.arange(mw)[None, :, None] * 2 + np.array([0, 1, 0, 1])[None, None, :]) + np.zeros((mh, 1, 1), int)
    dummy_y = (by >= bh) | (bx >= bw)
    chroma = []
    for k in (1, 2):
        p = _pad_to(c[..., k], H + (H & 1), mw * 16)                     # right to the MCU grid, down by one row if H is odd
        s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
        bias = 2 if mutant == "flat_bias" else 1 + (np.arange(s.shape[1]) & 1)[None, :]
        chroma.append(_blocks(_pad_to((s + bias) >> 2, mh * 8, mw * 8)))  # the last downsampled row replicated
    b = np.concatenate([yb, chroma[0][:, :, None], chroma[1][:, :, None]], 2)                     # [mh, mw, 6, 8, 8]
    dummy = np.concatenate([dummy_y, np.zeros((mh, mw, 2), bool)], 2)
    return b.reshape(-1, 8, 8), dummy.reshape(-1)


C = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069, f2053=16819,
         f2562=20995, f3072=25172)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """one pass of the IJG slow-integer DCT along the last axis (int64 [..., 8])"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o0 = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o4 = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * C["f0541"]
    o2 = _descale(z1 + t13 * C["f0765"], n)
    o6 = _descale(z1 - t12 * C["f1847"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * C["f1175"]
    t4, t5, t6, t7 = t4 * C["f0298"], t5 * C["f2053"], t6 * C["f3072"], t7 * C["f1501"]
    z1, z2, z3, z4 = -z1 * C["f0899"], -z2 * C["f2562"], -z3 * C["f1961"], -z4 * C["f0390"]
    z3, z4 = z3 + z5, z4 + z5
    o7, o5, o3, o1 = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack([o0, o1, o2, o3, o4, o5, o6, o7], -1)


def fdct(blocks):
    """int64 [N, 8, 8] samples minus 128 -> 8 x the DCT, rows first, then columns"""
    rows = _fdct_pass(np.asarray(blocks, np.int64), True)
    return _fdct_pass(rows.transpose(0, 2, 1), False).transpose(0, 2, 1)


def fdct_float64(blocks):
    """the orthonormal 8 x 8 DCT-II in float64"""
    k = np.arange(8)
    A = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k == 0, np.sqrt(1 / 8), 0.5)[:, None]
    return A @ np.asarray(blocks, np.float64) @ A.T


def quantise(coef, table):
    """[N, 8, 8] DCT x 8 by a natural-order table [64]"""
    d = 8 * table.reshape(1, 8, 8)
    a = np.abs(coef) + (d >> 1)
    return np.sign(coef) * (a // d)


def coefficients(img, quality=95, subsampling="420", channels="bgr", scale=255.0, mutant=None):
    """-> (int16 [blocks, 64] quantised coefficients in zigzag order, blocks in scan order, dummy blocks resolved; status)"""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[..., None]
    H, W, Cn = img.shape
    mode = mode_of(subsampling, Cn)
    u8, bad = levels(img, scale, mutant)
    samples, dummy = sample_blocks(u8, mode, channels, mutant)
    _, _, bpm, comp = geometry(H, W, mode)
    tabs = quant_tables(quality)
    comp_of = np.tile(comp, samples.shape[0] // bpm)
    dct = fdct(samples - 128)
    q = np.where((comp_of == 0)[:, None, None], quantise(dct, tabs[0]), quantise(dct, tabs[1]))
    z = q.reshape(-1, 64)[:, ZIGZAG]
    for i in np.nonzero(dummy)[0]:          # the MCU's own order: the block before is resolved by then
        z[i] = 0
        z[i, 0] = z[i - 1, 0]
    return z.astype(np.int16), (NONFINITE if bad else 0)


def _size(v):
    """number of bits of |v|"""
    a = np.abs(v).astype(np.int64)
    s = np.zeros_like(a)
    for k in range(16):
        s += (a >> k) > 0
    return s


def block_symbols(coef, mode, W=None, mutant=None):
    """per coefficient slot the bits it contributes: (value uint64 [blocks, 64], bit count [blocks, 64]).  Slot 0 carries the DC
    code, a non-zero AC slot its ZRLs, run/size code and amplitude, slot 63 the EOB when coefficient 63 is zero."""
    coef = np.asarray(coef, np.int64).reshape(-1, 64)
    nb = coef.shape[0]
    bpm = {M420: 6, M444: 3, MGRAY: 1}[mode]
    comp = {M420: np.array([0, 0, 0, 0, 1, 2]), M444: np.array([0, 1, 2]), MGRAY: np.array([0])}[mode]
    comp_of = np.tile(comp, nb // bpm)
    tab = (comp_of > 0).astype(np.int64)
    # DC differences per component
    diff = np.zeros(nb, np.int64)
    for c in range(comp.max() + 1):
        idx = np.nonzero(comp_of == c)[0]
        dc = coef[idx, 0]
        prev = np.concatenate([[0], dc[:-1]])
        if mutant == "dc_reset_per_row" and W is not None:
            per_row = ((W + 15) // 16 if mode == M420 else (W + 7) // 8) * (4 if (mode == M420 and c == 0) else 1)
            prev[np.arange(len(idx)) % per_row == 0] = 0
        diff[idx] = dc - prev
    val = np.zeros((nb, 64), np.uint64)
    cnt = np.zeros((nb, 64), np.int64)
    s = _size(diff)
    amp = np.where(diff < 0, diff + (1 << s) - 1, diff)
    dcc = np.where(tab == 0, DC_TAB[0][0][s], DC_TAB[1][0][s])
    dcl = np.where(tab == 0, DC_TAB[0][1][s], DC_TAB[1][1][s])
    val[:, 0] = ((dcc << s) | amp).astype(np.uint64)
    cnt[:, 0] = dcl + s
    # AC
    ac = coef.copy()
    ac[:, 0] = 0
    pos = np.arange(64)[None, :]
    last = np.maximum.accumulate(np.where(ac != 0, pos, 0), axis=1)
    prev = np.concatenate([np.zeros((nb, 1), np.int64), last[:, :-1]], 1)
    run = pos - prev - 1
    s = _size(ac)
    amp = np.where(ac < 0, ac + (1 << s) - 1, ac)
    sym = ((run & 15) << 4) | s
    t2 = tab[:, None] + np.zeros((1, 64), np.int64)
    code = np.where(t2 == 0, AC_TAB[0][0][sym], AC_TAB[1][0][sym])
    clen = np.where(t2 == 0, AC_TAB[0][1][sym], AC_TAB[1][1][sym])
    zc = np.where(t2 == 0, AC_TAB[0][0][0xF0], AC_TAB[1][0][0xF0])
    zl = np.where(t2 == 0, AC_TAB[0][1][0xF0], AC_TAB[1][1][0xF0])
    nz = run >> 4
    v = np.zeros((nb, 64), np.int64)
    for k in range(3):
        v = np.where(nz > k, (v << zl) | zc, v)
    v = (((v << clen) | code) << s) | amp
    n = nz * zl + clen + s
    on = ac != 0
    val = np.where(on, v.astype(np.uint64), val)
    cnt = np.where(on, n, cnt)
    eob = coef[:, 63] == 0
    val[:, 63] = np.where(eob, np.where(tab == 0, AC_TAB[0][0][0], AC_TAB[1][0][0]).astype(np.uint64), val[:, 63])
    cnt[:, 63] = np.where(eob, np.where(tab == 0, AC_TAB[0][1][0], AC_TAB[1][1][0]), cnt[:, 63])
    return val, cnt


def pack_bits(val, cnt):
    """the bit string: every slot's `cnt` low bits of `val`, most significant first, slots in order -> (uint8 bits, total)"""
    val, cnt = val.reshape(-1), cnt.reshape(-1)
    keep = cnt > 0
    val, cnt = val[keep], cnt[keep]
    total = int(cnt.sum())
    start = np.cumsum(cnt) - cnt
    owner = np.repeat(np.arange(len(cnt)), cnt)
    j = np.arange(total) - start[owner]
    return ((val[owner] >> (cnt[owner] - 1 - j).astype(np.uint64)) & np.uint64(1)).astype(np.uint8), total


def entropy_encode(coef, mode, W=None, mutant=None):
    """the scan of a coefficient array [blocks, 64]: padded with 1-bits, every 0xFF followed by 0x00"""
    bits, total = pack_bits(*block_symbols(coef, mode, W, mutant))
    pad = (-total) % 8
    bits = np.concatenate([bits, np.full(pad, 0 if mutant == "zero_padding" else 1, np.uint8)])
    raw = np.packbits(bits)
    if mutant == "no_stuffing":
        return raw.tobytes()
    ff = raw == 0xFF
    out = np.zeros(len(raw) + int(ff.sum()), np.uint8)
    out[np.arange(len(raw)) + np.cumsum(ff) - ff] = raw
    return out.tobytes()


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(H, W, mode, quality):
    """SOI, APP0, DQT per table, SOF0, DHT per table, SOS: what Pillow writes with optimize=False"""
    tabs = quant_tables(quality)
    nc = 1 if mode == MGRAY else 3
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in range(1 if nc == 1 else 2):
        out += _seg(0xDB, bytes([t]) + bytes(int(v) for v in tabs[t][ZIGZAG]))
    samp = [0x22 if mode == M420 else 0x11, 0x11, 0x11]
    sof = bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([nc])
    for c in range(nc):
        sof += bytes([c + 1, samp[c], 0 if c == 0 else 1])
    out += _seg(0xC0, sof)
    for t in range(1 if nc == 1 else 2):
        out += _seg(0xC4, bytes([t]) + bytes(DC_BITS[t]) + bytes(DC_VALS[t]))
        out += _seg(0xC4, bytes([0x10 | t]) + bytes(AC_BITS[t]) + bytes(AC_VALS[t]))
    sos = bytes([nc])
    for c in range(nc):
        sos += bytes([c + 1, 0x00 if c == 0 else 0x11])
    out += _seg(0xDA, sos + bytes([0, 63, 0]))
    return out


def scan_file(coef, H, W, mode, quality, mutant=None):
    return header(H, W, mode, quality) + entropy_encode(coef, mode, W, mutant) + b"\xff\xd9"


def encode(img, quality=95, subsampling="420", channels="bgr", scale=255.0, mutant=None):
    """-> (the file's bytes, status)"""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[..., None]
    H, W, Cn = img.shape
    coef, status = coefficients(img, quality, subsampling, channels, scale, mutant)
    return scan_file(coef, H, W, mode_of(subsampling, Cn), quality, mutant), status


def max_bytes(H, W, mode):
    return len(header(H, W, mode, 50)) + 416 * n_blocks(H, W, mode) + 2


def split_file(data):
    """(header up to and including SOS, scan, trailer) of a baseline file without restart markers"""
    i = 2
    while True:
        assert data[i] == 0xFF
        L = int.from_bytes(data[i + 2:i + 4], "big")
        if data[i + 1] == 0xDA:
            i += 2 + L
            break
        i += 2 + L
    assert data[-2:] == b"\xff\xd9"
    return data[:i], data[i:-2], data[-2:]


def decode_scan(scan, blocks, mode):
    """a small Huffman decoder: the quantised coefficients [blocks, 64] (zigzag order) of a stuffed scan.  Returns (coef, bits read)."""
    raw = bytes(scan).replace(b"\xff\x00", b"\xff")
    bits = np.unpackbits(np.frombuffer(raw, np.uint8))
    comp = {M420: [0, 0, 0, 0, 1, 2], M444: [0, 1, 2], MGRAY: [0]}[mode]
    lut = []
    for tabs in (DC_TAB, AC_TAB):
        lut.append([{(int(t[1][s]), int(t[0][s])): s for s in range(256) if t[1][s]} for t in tabs])
    p = 0

    def symbol(d):
        nonlocal p
        c, n = 0, 0
        while True:
            c, n, p = (c << 1) | int(bits[p]), n + 1, p + 1
            if (n, c) in d:
                return d[(n, c)]
            assert n < 16, "no code"

    def receive(s):
        nonlocal p
        v = 0
        for _ in range(s):
            v, p = (v << 1) | int(bits[p]), p + 1
        return v if (s == 0 or v >> (s - 1)) else v - (1 << s) + 1

    out = np.zeros((blocks, 64), np.int64)
    pred = [0, 0, 0]
    for b in range(blocks):
        c = comp[b % len(comp)]
        t = 1 if c else 0
        pred[c] += receive(symbol(lut[0][t]))
        out[b, 0] = pred[c]
        k = 1
        while k < 64:
            rs = symbol(lut[1][t])
            r, s = rs >> 4, rs & 15
            if s == 0:
                if r == 15:
                    k += 16
                    continue
                break
            k += r
            out[b, k] = receive(s)
            k += 1
    return out, p


def scan_bits(coef, mode):
    """number of bits of the unstuffed, unpadded scan"""
    return int(block_symbols(coef, mode)[1].sum())


def raw_scan(coef, mode):
    """the padded scan before stuffing"""
    return entropy_encode(coef, mode, mutant="no_stuffing")


def hand_made_scans():
    """coefficient arrays that aim at the entropy coder's corners: {name: (coef int16 [blocks, 64], mode, H, W)}; the blocks of a GRAY
    case lie in one row of 8 x 8 MCUs, those of a 444 case in one row of three-block MCUs"""
    out = {}

    def gray(name, blocks):
        c = np.asarray(blocks, np.int16).reshape(-1, 64)
        out[name] = (c, MGRAY, 8, 8 * len(c))

    for run in (15, 16, 17, 32, 62):          # zeros in front of one coefficient; 62: coefficient 63 is set, no EOB
        b = np.zeros(64, np.int16)
        b[0], b[1 + run] = 5, -3
        gray(f"run{run}", [b])
    b = np.zeros((2, 64), np.int16)
    b[0, 63], b[1, 62] = 1, 1                 # coefficient 63 set (no EOB) and clear (EOB)
    gray("c63_set_and_clear", b)
    diffs = [0]
    for s in range(1, 12):                    # every DC size, both signs, smallest and largest magnitude of the size
        diffs += [(1 << s) - 1, -((1 << s) - 1), 1 << (s - 1), -(1 << (s - 1))]
    b = np.zeros((len(diffs), 64), np.int16)
    b[:, 0] = np.cumsum(diffs)
    gray("dc_sizes", b)
    b3 = np.zeros((len(diffs) // 3 * 3, 64), np.int16)          # the same through the chrominance DC table (444: Y, Cb, Cr)
    for c in range(3):
        b3[c::3, 0] = np.cumsum(diffs[:len(b3) // 3])
    out["dc_sizes_444"] = (b3, M444, 8, 8 * (len(b3) // 3))
    # a scan that ends on a byte boundary, and one whose padded last byte is 0xFF: found by search, checked by the tests
    aligned = padded_ff = None
    for v in range(1, 1024):
        for pos in (1, 2, 5, 63):
            b = np.zeros((1, 64), np.int16)
            b[0, 0], b[0, pos] = 3, v
            n = scan_bits(b, MGRAY)
            if aligned is None and n % 8 == 0:
                aligned = b
            if padded_ff is None and n % 8 and raw_scan(b, MGRAY)[-1] == 0xFF:
                padded_ff = b
    gray("ends_on_byte_boundary", aligned)
    gray("padded_last_byte_is_ff", padded_ff)
    # the longest block there is: DC difference of size 11, 63 coefficients of size 10 whose 16-bit codes begin with eight 1-bits and
    # whose amplitudes are ten 1-bits: 1658 bits, nearly all of them 0xFF bytes
    b = np.full((2, 64), 1023, np.int16)
    b[0, 0], b[1, 0] = 2047, 0
    gray("all_ff_block", b)
    rng = np.random.default_rng(7)            # sparse random blocks in 4:2:0 order over two MCU rows
    b = (rng.integers(-40, 41, (6 * 6, 64)) * (rng.random((36, 64)) < 0.15)).astype(np.int16)
    out["sparse_420"] = (b, M420, 32, 48)
    return out
