"""The PNG encoder's rule (include/dsnerf.h, "PNG ENCODING on the device") restated in numpy, stage by stage: levels, filter, tokens,
code lengths, header, bits, container.  The device is held to this file byte for byte; this file is held to zlib.decompress, Pillow and
tests/png_decode_restate.py (tests/test_png_encode_host.py).  Keyword arguments named `mutant_*` switch one rule off each: the host tests
show that a named check fails for every one of them."""
import numpy as np

ADAPTIVE = 5
GRAY, COLOUR, REPLICATE = 0, 1, 2
CHUNK_DEFAULT = 32768
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


# ---- levels ------------------------------------------------------------------------------------------------------------------------------------
def levels(img, scale=255.0):
    """uint8 passes through; float32: v * scale in float32, nearest-even, saturated, NaN -> 0.  -> (uint8 array, any non-finite input)"""
    a = np.asarray(img)
    if a.dtype == np.uint8:
        return a.copy(), False
    v = a.astype(np.float32)
    bad = bool((~np.isfinite(v)).any())
    with np.errstate(invalid="ignore", over="ignore"):
        t = v * np.float32(scale)
        r = np.rint(t)
    r = np.where(np.isnan(t), np.float32(0), np.clip(r, 0, 255))
    return r.astype(np.uint8), bad


def file_pixels(lv, channels="bgr", replicate=False):
    """levels [H, W] or [H, W, 3] -> the file's unfiltered rows uint8 [H, row_bytes] and its channel count"""
    if lv.ndim == 2:
        if replicate:
            return np.repeat(lv[:, :, None], 3, axis=2).reshape(lv.shape[0], -1), 3
        return lv.copy(), 1
    px = lv[:, :, ::-1] if channels == "bgr" else lv
    return np.ascontiguousarray(px).reshape(lv.shape[0], -1), 3


# ---- filter ------------------------------------------------------------------------------------------------------------------------------------
def _paeth(a, b, c, order="abc"):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    if order == "abc":
        return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.where((pc <= pa) & (pc <= pb), c, np.where(pb <= pa, b, a))          # the mutant: ties go to c, then b


def filtered_rows(rows, bpp, mutant_paeth=False):
    """rows uint8 [H, rb] -> int [5, H, rb]: every row under every filter"""
    x = rows.astype(np.int32)
    H, rb = x.shape
    a = np.zeros_like(x); a[:, bpp:] = x[:, :-bpp] if rb > bpp else a[:, bpp:]
    b = np.zeros_like(x); b[1:] = x[:-1]
    c = np.zeros_like(x); c[1:, bpp:] = x[:-1, :-bpp] if rb > bpp else c[1:, bpp:]
    subs = [np.zeros_like(x), a, b, (a + b) >> 1, _paeth(a, b, c, "cba" if mutant_paeth else "abc")]
    return np.stack([(x - s) & 255 for s in subs])


def filter_image(rows, bpp, filt=ADAPTIVE, mutant_unsigned=False, mutant_paeth=False):
    """-> (raw stream uint8 [H (1 + rb)], the filter of every row)"""
    f5 = filtered_rows(rows, bpp, mutant_paeth)
    H, rb = rows.shape
    if filt == ADAPTIVE:
        mag = f5 if mutant_unsigned else np.where(f5 < 128, f5, 256 - f5)
        choice = np.argmin(mag.sum(axis=2), axis=0)          # argmin: the first of equal sums = the lower filter number
    else:
        choice = np.full(H, int(filt))
    raw = np.empty((H, 1 + rb), np.uint8)
    raw[:, 0] = choice
    raw[:, 1:] = f5[choice, np.arange(H)]
    return raw.reshape(-1), choice


# ---- checksums ---------------------------------------------------------------------------------------------------------------------------------
def adler32(data):
    d = np.frombuffer(bytes(data), np.uint8).astype(np.int64)
    n = len(d)
    a = (1 + int(d.sum())) % 65521
    b = (n + int(((n - np.arange(n)) % 65521 * d).sum() % 65521)) % 65521 if n else 0
    return (b << 16 | a) if n else 1


_CRC = []
for _n in range(256):
    _v = _n
    for _k in range(8):
        _v = 0xEDB88320 ^ (_v >> 1) if _v & 1 else _v >> 1
    _CRC.append(_v)


def crc32(data):
    c = 0xFFFFFFFF
    for b in bytes(data):
        c = _CRC[(c ^ b) & 255] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


# ---- tokens ------------------------------------------------------------------------------------------------------------------------------------
def candidate_distances(bpp, row_stride):
    return [d for d in sorted({1, int(bpp), int(row_stride)}) if 1 <= d <= 32768]


def _run_lengths(eq):
    """eq bool [L] -> for every i the number of consecutive True from i on"""
    L = len(eq)
    stop = np.where(~eq, np.arange(L), L)
    nxt = np.minimum.accumulate(stop[::-1])[::-1]
    return nxt - np.arange(L)


def matches(raw, cs, ce, dists, mutant_cross=False):
    """best (length, distance) per position of the chunk raw[cs:ce]; length 0 for a literal"""
    L = ce - cs
    best_len, best_d = np.zeros(L, np.int64), np.zeros(L, np.int64)
    for d in dists:
        lo = 0 if mutant_cross else cs
        eq = np.zeros(L, bool)
        first = max(cs, lo + d)                                  # positions whose source lies at or behind `lo`
        if first < ce:
            eq[first - cs:] = raw[first:ce] == raw[first - d:ce - d]
        ln = np.minimum(_run_lengths(eq), 258)
        better = ln > best_len                                   # ascending distances: ties keep the smaller one
        best_len[better], best_d[better] = ln[better], d
    lit = (best_len < 3) | ((best_len == 3) & (best_d > 4096))
    best_len[lit] = 0
    return best_len, best_d


def parse(raw, cs, ce, dists, mutant_cross=False):
    """the serial greedy parse -> tokens: (byte,) for a literal, (length, distance) for a match"""
    ln, dd = matches(raw, cs, ce, dists, mutant_cross)
    out, p, L = [], 0, ce - cs
    while p < L:
        if ln[p]:
            out.append((int(ln[p]), int(dd[p])))
            p += int(ln[p])
        else:
            out.append((int(raw[cs + p]),))
            p += 1
    return out


def length_code(n):
    for k in range(28, -1, -1):
        if n >= LEN_BASE[k]:
            return k, LEN_EXTRA[k], n - LEN_BASE[k]


def dist_code(d):
    for k in range(29, -1, -1):
        if d >= DIST_BASE[k]:
            return k, DIST_EXTRA[k], d - DIST_BASE[k]


def histograms(tokens):
    ll, dd = [0] * 286, [0] * 30
    for t in tokens:
        if len(t) == 1:
            ll[t[0]] += 1
        else:
            ll[257 + length_code(t[0])[0]] += 1
            dd[dist_code(t[1])[0]] += 1
    ll[256] = 1
    return ll, dd


# ---- code lengths ------------------------------------------------------------------------------------------------------------------------------
def huff_lengths(counts, limit, mutant_no_limit=False):
    counts = [int(c) for c in counts]
    n = len(counts)
    used = sum(1 for c in counts if c)
    for i in range(n):
        if used >= 2:
            break
        if counts[i] == 0:
            counts[i], used = 1, used + 1
    order = sorted((i for i in range(n) if counts[i]), key=lambda i: (counts[i], i))
    m = len(order)
    w = [counts[i] for i in order] + [0] * (m - 1)
    parent = [0] * (2 * m - 1)
    li, ii, nxt = 0, m, m
    while nxt < 2 * m - 1:
        pick = []
        for _ in range(2):
            if li < m and (ii >= nxt or w[li] <= w[ii]):
                pick.append(li); li += 1
            else:
                pick.append(ii); ii += 1
        w[nxt] = w[pick[0]] + w[pick[1]]
        parent[pick[0]] = parent[pick[1]] = nxt
        nxt += 1
    depth = [0] * (2 * m - 1)
    for k in range(2 * m - 3, -1, -1):
        depth[k] = depth[parent[k]] + 1
    top = max(depth[:m]) if mutant_no_limit else limit
    bl = [0] * (top + 1)
    for k in range(m):
        bl[min(depth[k], top)] += 1
    total = sum(bl[l] << (top - l) for l in range(1, top + 1))
    while total > (1 << top):
        bl[top] -= 1
        l = top - 1
        while bl[l] == 0:
            l -= 1
        bl[l] -= 1
        bl[l + 1] += 2
        total -= 1
    lens, k = [0] * n, 0
    for l in range(top, 0, -1):
        for _ in range(bl[l]):
            lens[order[k]] = l
            k += 1
    return lens


def canonical(lens):
    """-> codes (most significant bit first, as RFC 1951 3.2.2 numbers them)"""
    top = max(max(lens), 1)
    cnt = [0] * (top + 1)
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    nxt, code = [0] * (top + 1), 0
    for l in range(1, top + 1):
        code = (code + cnt[l - 1]) << 1
        nxt[l] = code
    codes = []
    for l in lens:
        codes.append(nxt[l] if l else 0)
        if l:
            nxt[l] += 1
    return codes


def kraft(lens):
    from fractions import Fraction
    return sum(Fraction(1, 1 << l) for l in lens if l)


# ---- the block -----------------------------------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.out, self.acc, self.n, self.total = bytearray(), 0, 0, 0

    def put(self, v, nb):                                        # least significant bit first
        self.acc |= (v & ((1 << nb) - 1)) << self.n
        self.n += nb
        self.total += nb
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, nb):                                       # a Huffman code: most significant bit first
        self.put(int(format(c, "0%db" % nb)[::-1], 2) if nb else 0, nb)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def rle(lens):
    """the header's symbols of one alphabet's lengths: (symbol, extra value)"""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, r = lens[i], 1
        while i + r < n and lens[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                t = min(r, 138); out.append((18, t - 11)); r -= t
            if r >= 3:
                out.append((17, r - 3)); r = 0
        else:
            out.append((v, 0)); r -= 1
            while r >= 3:
                t = min(r, 6); out.append((16, t - 3)); r -= t
        out += [(v, 0)] * r
    return out


def dynamic_header(ll_lens, d_lens):
    """-> dict(hlit, hdist, hclen, seq, cl_lens, bits)"""
    hlit, hdist = 286, 30
    while hlit > 257 and ll_lens[hlit - 1] == 0:
        hlit -= 1
    while hdist > 1 and d_lens[hdist - 1] == 0:
        hdist -= 1
    seq = rle(ll_lens[:hlit]) + rle(d_lens[:hdist])
    hist = [0] * 19
    for s, _ in seq:
        hist[s] += 1
    cl = huff_lengths(hist, 7)
    hclen = 19
    while hclen > 4 and cl[ORDER[hclen - 1]] == 0:
        hclen -= 1
    bits = 14 + 3 * hclen + sum(cl[s] + {16: 2, 17: 3, 18: 7}.get(s, 0) for s, _ in seq)
    return dict(hlit=hlit, hdist=hdist, hclen=hclen, seq=seq, cl_lens=cl, bits=bits)


def token_bits(ll_hist, d_hist, ll_lens, d_lens):
    return (sum(n * (ll_lens[i] + (LEN_EXTRA[i - 257] if i > 256 else 0)) for i, n in enumerate(ll_hist))
            + sum(n * (d_lens[i] + DIST_EXTRA[i]) for i, n in enumerate(d_hist)))


def chunk_plan(raw, cs, ce, dists, stored_only=False, mutant_cross=False, mutant_no_limit=False):
    """everything the block of chunk raw[cs:ce] is made from"""
    plan = dict(stored=8 + 32 + 8 * (ce - cs))
    if stored_only:
        plan["btype"] = 0
        return plan
    tokens = parse(raw, cs, ce, dists, mutant_cross)
    ll_hist, d_hist = histograms(tokens)
    ll_lens, d_lens = huff_lengths(ll_hist, 15, mutant_no_limit), huff_lengths(d_hist, 15, mutant_no_limit)
    hdr = dynamic_header(ll_lens, d_lens)
    plan.update(tokens=tokens, ll_hist=ll_hist, d_hist=d_hist, ll_lens=ll_lens, d_lens=d_lens, header=hdr,
                fixed=3 + token_bits(ll_hist, d_hist, FIXED_LL, FIXED_D),
                dynamic=3 + hdr["bits"] + token_bits(ll_hist, d_hist, ll_lens, d_lens))
    costs = [plan["stored"], plan["fixed"], plan["dynamic"]]
    plan["btype"] = costs.index(min(costs))                      # ties: stored, fixed, dynamic
    return plan


def chunk_bytes(raw, cs, ce, plan, last, mutant_no_separator=False):
    w = Bits()
    bt = plan["btype"]
    w.put(1 if last else 0, 1)
    w.put(bt, 2)
    if bt == 0:
        w.align()
        n = ce - cs
        w.put(n, 16); w.put(n ^ 0xFFFF, 16)
        w.out += bytes(raw[cs:ce])
    else:
        if bt == 2:
            ll_lens, d_lens, h = plan["ll_lens"], plan["d_lens"], plan["header"]
            w.put(h["hlit"] - 257, 5); w.put(h["hdist"] - 1, 5); w.put(h["hclen"] - 4, 4)
            for k in range(h["hclen"]):
                w.put(h["cl_lens"][ORDER[k]], 3)
            cl_codes = canonical(h["cl_lens"])
            for s, e in h["seq"]:
                w.code(cl_codes[s], h["cl_lens"][s])
                if s >= 16:
                    w.put(e, {16: 2, 17: 3, 18: 7}[s])
        else:
            ll_lens, d_lens = FIXED_LL, FIXED_D
        ll_codes, d_codes = canonical(list(ll_lens)), canonical(list(d_lens))
        for t in plan["tokens"]:
            if len(t) == 1:
                w.code(ll_codes[t[0]], ll_lens[t[0]])
            else:
                k, nb, e = length_code(t[0])
                w.code(ll_codes[257 + k], ll_lens[257 + k]); w.put(e, nb)
                k, nb, e = dist_code(t[1])
                w.code(d_codes[k], d_lens[k]); w.put(e, nb)
        w.code(ll_codes[256], ll_lens[256])
        assert w.total == plan["fixed" if bt == 1 else "dynamic"], (w.total, plan)
    if last:
        w.align()
    elif not mutant_no_separator:
        w.put(0, 3); w.align()
        w.out += b"\x00\x00\xff\xff"
    else:
        w.align()
    return bytes(w.out)


def deflate(raw, bpp, row_stride, chunk=CHUNK_DEFAULT, stored_only=False, plans=None, pieces=None, **mutants):
    """raw bytes -> the deflate stream (no zlib header, no Adler-32); plans / pieces (lists) receive every chunk's plan / bytes"""
    raw = np.frombuffer(bytes(raw), np.uint8)
    dists = candidate_distances(bpp, row_stride)
    out, n = b"", len(raw)
    for cs in range(0, n, chunk):
        ce = min(cs + chunk, n)
        plan = chunk_plan(raw, cs, ce, dists, stored_only, mutants.get("mutant_cross", False), mutants.get("mutant_no_limit", False))
        if plans is not None:
            plans.append(plan)
        piece = chunk_bytes(raw, cs, ce, plan, ce == n, mutants.get("mutant_no_separator", False))
        if pieces is not None:
            pieces.append(piece)
        out += piece
    return out


def deflate_max_bytes(n, chunk):
    nch = (n + chunk - 1) // chunk
    return n + 10 * nch - 5


def encode_max_bytes(W, H, channels, chunk=CHUNK_DEFAULT):
    return 63 + deflate_max_bytes(H * (1 + W * channels), chunk)


# ---- container ---------------------------------------------------------------------------------------------------------------------------------
def png_chunk(kind, data, mutant_crc_no_type=False):
    crc = crc32(data) if mutant_crc_no_type else crc32(kind + data)
    return len(data).to_bytes(4, "big") + kind + data + crc.to_bytes(4, "big")


def container(W, H, channels, stream, adler, mutant_crc_no_type=False):
    ihdr = W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes([8, 2 if channels == 3 else 0, 0, 0, 0])
    idat = b"\x78\x01" + stream + int(adler).to_bytes(4, "big")
    return (b"\x89PNG\r\n\x1a\n" + png_chunk(b"IHDR", ihdr, mutant_crc_no_type) + png_chunk(b"IDAT", idat, mutant_crc_no_type)
            + png_chunk(b"IEND", b"", mutant_crc_no_type))


def encode_one(img, channels="bgr", scale=255.0, replicate=False, filt=ADAPTIVE, chunk=CHUNK_DEFAULT, stored_only=False, stages=None,
               **mutants):
    """one image [H, W] / [H, W, 3] -> (file bytes, status: 1 = a non-finite input).  stages (a dict) receives every stage's output."""
    lv, bad = levels(img, scale)
    rows, ch = file_pixels(lv, channels, replicate)
    H, W = lv.shape[:2]
    raw, choice = filter_image(rows, ch, filt, mutants.get("mutant_unsigned", False), mutants.get("mutant_paeth", False))
    plans, pieces = [], []
    stream = deflate(raw, ch, 1 + W * ch, chunk, stored_only, plans, pieces, **mutants)
    adler = adler32(rows.reshape(-1)) if mutants.get("mutant_adler_pixels") else adler32(raw)
    data = container(W, H, ch, stream, adler, mutants.get("mutant_crc_no_type", False))
    if stages is not None:
        stages.update(levels=lv, rows=rows, raw=raw, filters=choice, plans=plans, pieces=pieces, stream=stream, adler=adler)
    return data, (1 if bad else 0)


def encode(images, **kw):
    out = [encode_one(x, **kw) for x in images]
    return [d for d, _ in out], [s for _, s in out]


def idat_payload(data):
    """the concatenated IDAT payloads of a file, every chunk's CRC checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    i, out = 8, b""
    while i < len(data):
        n = int.from_bytes(data[i:i + 4], "big")
        kind, body = data[i + 4:i + 8], data[i + 8:i + 8 + n]
        assert crc32(kind + body) == int.from_bytes(data[i + 8 + n:i + 12 + n], "big"), kind
        if kind == b"IDAT":
            out += body
        i += 12 + n
    return out
