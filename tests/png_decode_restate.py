"""PNG decoding restated in plain Python / numpy: the rule of include/dsnerf.h ("PNG DECODING on the device"), stage for stage as
csrc/dsn_png.hip runs it - container and CRC-32, gather, inflate (its own bit reader and Huffman tables; zlib is NOT called here),
Adler-32, unfilter, pixels - with the same status words.  test_png_host.py holds it to zlib.decompress and to Pillow's pixels;
test_gpu_png.py holds the kernels to it bit for bit."""
import numpy as np

EARLY_END, BLOCK_TYPE, STORED_LEN, BAD_CODES, NO_CODE, FAR_DISTANCE, TOO_MUCH, TOO_LITTLE, FILTER, ADLER = (1 << k for k in range(10))
STATUS_BITS = {"early_end": EARLY_END, "block_type": BLOCK_TYPE, "stored_len": STORED_LEN, "bad_codes": BAD_CODES, "no_code": NO_CODE,
               "far_distance": FAR_DISTANCE, "too_much": TOO_MUCH, "too_little": TOO_LITTLE, "filter": FILTER, "adler": ADLER}
REASONS = ["ok", "not_png", "truncated", "crc", "bad_ihdr", "interlace", "depth16", "no_ihdr", "no_idat", "no_plte", "zero_dim", "too_large",
           "zlib_method", "zlib_dict", "zlib_check"]
MAX_DIM, MAX_RAW, MAX_STREAM = 16384, 1 << 30, 1 << 28
SIGNATURE = b"\x89PNG\r\n\x1a\n"

_CRC = []
for _n in range(256):
    _v = _n
    for _ in range(8):
        _v = 0xEDB88320 ^ (_v >> 1) if _v & 1 else _v >> 1
    _CRC.append(_v)


def crc32(data):
    c = 0xFFFFFFFF
    for b in data:
        c = _CRC[(c ^ b) & 255] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def channels_of(bits, ctype):
    low = bits in (1, 2, 4)
    return {0: 1 if low or bits == 8 else 0, 2: 3 if bits == 8 else 0, 3: 1 if low or bits == 8 else 0, 4: 2 if bits == 8 else 0,
            6: 4 if bits == 8 else 0}.get(ctype, 0)


def _be32(d, i):
    return int.from_bytes(d[i:i + 4], "big")


def parse(data):
    """the container: {"reason": one of REASONS, W, H, bits, ctype, channels, row_bytes, raw_bytes, palette uint8 [256, 3], npal,
    segs [(offset, length)], zlen}; everything behind "reason" is complete only for "ok\""""
    d = bytes(data)
    n = len(d)
    info = {"reason": "ok", "W": 0, "H": 0, "bits": 0, "ctype": 0, "channels": 0, "row_bytes": 0, "raw_bytes": 0,
            "palette": np.zeros((256, 3), np.uint8), "npal": 0, "segs": [], "zlen": 0}

    def refuse(why):
        info["reason"] = why
        return info

    if n < 8 or d[:8] != SIGNATURE:
        return refuse("not_png")
    first, have_plte, have_iend, zlen, z = True, False, False, 0, []
    i = 8
    while i < n:
        if n - i < 12:
            return refuse("truncated")
        L = _be32(d, i)
        if L > n - i - 12:
            return refuse("truncated")
        typ, body = d[i + 4:i + 8], d[i + 8:i + 8 + L]
        if first and typ != b"IHDR":
            return refuse("no_ihdr")
        if typ in (b"IHDR", b"PLTE", b"IDAT", b"IEND") and crc32(typ + body) != _be32(d, i + 8 + L):
            return refuse("crc")
        if typ == b"IHDR":
            if not first or L != 13:
                return refuse("bad_ihdr")
            W, H, bits, ctype = _be32(body, 0), _be32(body, 4), body[8], body[9]
            if W == 0 or H == 0:
                return refuse("zero_dim")
            if bits == 16 and ctype in (0, 2, 4, 6):
                return refuse("depth16")
            ch = channels_of(bits, ctype)
            if not ch or body[10] or body[11] or body[12] > 1:
                return refuse("bad_ihdr")
            if body[12] == 1:
                return refuse("interlace")
            if W > MAX_DIM or H > MAX_DIM:
                return refuse("too_large")
            rb = (W * bits * ch + 7) // 8
            if H * (1 + rb) > MAX_RAW:
                return refuse("too_large")
            info.update(W=W, H=H, bits=bits, ctype=ctype, channels=ch, row_bytes=rb, raw_bytes=H * (1 + rb))
        elif typ == b"PLTE":
            if L == 0 or L > 768 or L % 3:
                return refuse("no_plte")
            if not info["segs"]:
                pal = np.zeros((256, 3), np.uint8)
                pal[:L // 3] = np.frombuffer(body, np.uint8).reshape(-1, 3)
                info.update(palette=pal, npal=L // 3)
                have_plte = True
        elif typ == b"IDAT":
            if info["ctype"] == 3 and not have_plte:
                return refuse("no_plte")
            z.extend(body[:max(0, 2 - len(z))])
            info["segs"].append((i + 8, L))
            zlen += L
            if zlen > MAX_STREAM:
                return refuse("too_large")
        elif typ == b"IEND":
            have_iend = True
            break
        first = False
        i += 12 + L
    if first:
        return refuse("no_ihdr")
    if not have_iend:
        return refuse("truncated")
    if not info["segs"] or zlen < 2:
        return refuse("no_idat")
    info["zlen"] = zlen
    if (z[0] & 15) != 8 or (z[0] >> 4) > 7:
        return refuse("zlib_method")
    if z[1] & 0x20:
        return refuse("zlib_dict")
    if (z[0] * 256 + z[1]) % 31:
        return refuse("zlib_check")
    return info


def gather(data, info):
    """the file's zlib stream: its IDAT payloads one behind the other"""
    return b"".join(bytes(data[o:o + n]) for o, n in info["segs"])


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class Code:
    """a canonical prefix code from code lengths: `usable` by the header's rule; lut[window of maxlen bits, first bit lowest] = (symbol
    << 4 | length) or -1"""

    def __init__(self, lens, incomplete_ok):
        count = [0] * 16
        for l in lens:
            count[l] += 1
        count[0] = 0
        left = 1
        for l in range(1, 16):
            left = -1 if left < 0 else (left << 1) - count[l]
        n = sum(count)
        self.usable = left == 0 or (incomplete_ok and left > 0 and (n == 0 or (n == 1 and count[1] == 1)))
        self.maxlen = max([l for l in lens if l] or [0])
        self.lut = [-1] * (1 << self.maxlen)
        if not self.usable:
            return
        nxt, code = [0] * 16, 0
        for l in range(1, 16):
            code = (code + count[l - 1]) << 1
            nxt[l] = code
        for sym, l in enumerate(lens):
            if l:
                c = nxt[l]
                nxt[l] += 1
                r = int(format(c, f"0{l}b")[::-1], 2)          # the code's bits arrive most significant first
                for k in range(r, 1 << self.maxlen, 1 << l):
                    self.lut[k] = sym << 4 | l


FIXED_L = Code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, False)
FIXED_D = Code([5] * 32, False)


class _Stop(Exception):
    def __init__(self, status):
        self.status = status


def inflate(z, cap):
    """the zlib stream z (header checked by parse) -> (bytes output, status, stored Adler-32, p at the end).  cap = raw_bytes."""
    zlen = len(z)
    total = zlen * 8
    zp = bytes(z) + bytes(16)          # bits at and past 8 zlen read 0

    def window():
        at = p >> 3
        return int.from_bytes(zp[at:at + 8], "little") >> (p & 7) if at < zlen + 8 else 0
    out = bytearray()
    p = 16

    def take(n):
        nonlocal p
        v = window() & ((1 << n) - 1)
        p += n
        return v

    def symbol(code):
        nonlocal p
        e = code.lut[window() & ((1 << code.maxlen) - 1)]
        if e < 0:
            raise _Stop(NO_CODE)
        p += e & 15
        return e >> 4

    def early():
        if p > total:
            raise _Stop(EARLY_END)

    status, stored = 0, 0
    try:
        while True:
            bfinal, btype = take(1), take(2)
            early()
            if btype == 3:
                raise _Stop(BLOCK_TYPE)
            if btype == 0:
                p += -p & 7
                ln, nln = take(16), take(16)
                early()
                if ln ^ 0xFFFF != nln:
                    raise _Stop(STORED_LEN)
                at = p >> 3
                if at + ln > zlen:
                    raise _Stop(EARLY_END)
                if len(out) + ln > cap:
                    raise _Stop(TOO_MUCH)
                out += z[at:at + ln]
                p = (at + ln) * 8
            else:
                if btype == 1:
                    L, D = FIXED_L, FIXED_D
                else:
                    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
                    early()
                    if hlit > 286 or hdist > 30:
                        raise _Stop(BAD_CODES)
                    cl = [0] * 19
                    for k in range(hclen):
                        cl[ORDER[k]] = take(3)
                    early()
                    C = Code(cl, False)
                    if not C.usable:
                        raise _Stop(BAD_CODES)
                    lens, prev = [], 0
                    while len(lens) < hlit + hdist:
                        s = symbol(C)
                        rep, val = 1, s
                        if s == 16:
                            rep, val = 3 + take(2), prev
                        elif s == 17:
                            rep, val = 3 + take(3), 0
                        elif s == 18:
                            rep, val = 11 + take(7), 0
                        early()
                        if (s == 16 and not lens) or len(lens) + rep > hlit + hdist:
                            raise _Stop(BAD_CODES)
                        lens += [val] * rep
                        prev = val
                    if lens[256] == 0:
                        raise _Stop(BAD_CODES)
                    L, D = Code(lens[:hlit], True), Code(lens[hlit:], True)
                    if not L.usable or not D.usable:
                        raise _Stop(BAD_CODES)
                while True:
                    s = symbol(L)
                    if s < 256:
                        early()
                        if len(out) >= cap:
                            raise _Stop(TOO_MUCH)
                        out.append(s)
                        continue
                    ln = 0 if s == 256 or s > 285 else LBASE[s - 257] + take(LEXT[s - 257])
                    early()
                    if s == 256:
                        break
                    if s > 285:
                        raise _Stop(NO_CODE)
                    ds = symbol(D)
                    dist = DBASE[ds] + take(DEXT[ds]) if ds < 30 else 0
                    early()
                    if ds > 29:
                        raise _Stop(NO_CODE)
                    if dist > len(out):
                        raise _Stop(FAR_DISTANCE)
                    if len(out) + ln > cap:
                        raise _Stop(TOO_MUCH)
                    start = len(out)
                    if dist >= ln:
                        out += out[start - dist:start - dist + ln]
                    else:
                        out += bytes(out[start - dist + (i % dist)] for i in range(ln))          # an overlapping match repeats its d bytes
            if bfinal:
                break
        at = (p + 7) >> 3
        if at + 4 > zlen:
            raise _Stop(EARLY_END)
        stored = int.from_bytes(z[at:at + 4], "big")
        if len(out) < cap:
            status = TOO_LITTLE
    except _Stop as e:
        status = e.status
    return bytes(out), status, stored, p


def adler32(data):
    """blockwise, as the kernel has it: a = 1 + sum d_i, b = n + sum (n - i) d_i, both mod 65521 (blocks of 2^20 keep the sums in 64 bits)"""
    d = np.frombuffer(bytes(data), np.uint8).astype(np.uint64)
    n = len(d)
    a, b = 1, n % 65521
    for k in range(0, n, 1 << 20):
        blk = d[k:k + (1 << 20)]
        w = (np.uint64(n) - np.arange(k, k + len(blk), dtype=np.uint64)) % np.uint64(65521)
        a = (a + int(blk.sum())) % 65521
        b = (b + int((w * blk).sum() % np.uint64(65521))) % 65521
    return b << 16 | a


def unfilter(raw, info):
    """raw_bytes inflated bytes -> (rows uint8 [H, row_bytes], whether a filter byte above 4 was met)"""
    H, rb, bits, ch = info["H"], info["row_bytes"], info["bits"], info["channels"]
    bpp = max(1, bits * ch // 8)
    src = np.frombuffer(bytes(raw), np.uint8).reshape(H, 1 + rb)
    rows = np.zeros((H, rb), np.uint8)
    bad = False
    above = np.zeros(rb, np.int64)
    for r in range(H):
        ft, x = int(src[r, 0]), src[r, 1:].astype(np.int64)
        if ft > 4:
            bad, ft = True, 0
        if ft == 0:
            cur = x
        elif ft == 2:
            cur = (x + above) & 255
        elif ft == 1:
            cur = x.copy()
            for k in range(bpp):
                cur[k::bpp] = np.cumsum(x[k::bpp]) & 255          # a bytewise prefix sum mod 256 per channel lane
        else:
            cur = np.zeros(rb, np.int64)
            xs, ab = x.tolist(), above.tolist()
            c = [0] * rb
            for i in range(rb):
                a = c[i - bpp] if i >= bpp else 0
                b = ab[i]
                if ft == 3:
                    add = (a + b) >> 1
                else:
                    cc = ab[i - bpp] if i >= bpp else 0
                    pp = a + b - cc
                    pa, pb, pc = abs(pp - a), abs(pp - b), abs(pp - cc)
                    add = a if pa <= pb and pa <= pc else b if pb <= pc else cc
                c[i] = (xs[i] + add) & 255
            cur = np.asarray(c, np.int64)
        rows[r] = cur
        above = cur
    return rows, bad


def samples(rows, info):
    """[H, W, channels] samples as the file has them (1 / 2 / 4 bits unpacked, most significant first, row padding dropped)"""
    H, W, bits, ch = info["H"], info["W"], info["bits"], info["channels"]
    if bits == 8:
        return rows.reshape(H, W, ch)
    per = 8 // bits
    sh = (8 - bits - bits * np.arange(per)).astype(np.uint8)
    u = (rows[:, :, None] >> sh[None, None, :]) & ((1 << bits) - 1)
    return u.reshape(H, -1)[:, :W, None].astype(np.uint8)


def pixels(rows, info, channels="bgr", first_channel=False, status=0):
    """the output of dsn_png_decode for one file: uint8 [H, W, C], or [H, W] with first_channel; zeros for a frame with a status"""
    H, W, bits, ctype = info["H"], info["W"], info["bits"], info["ctype"]
    s = samples(rows, info)
    if ctype in (0, 4):
        nat = s.copy()
        nat[..., 0] = s[..., 0] * {1: 255, 2: 85, 4: 17, 8: 1}[bits]
        rgb = np.repeat(nat[..., :1], 3, 2)
    elif ctype == 3:
        nat = s
        rgb = info["palette"][s[..., 0]]
    else:
        nat = s
        rgb = s[..., :3]
    if channels == "native":
        out = nat
    elif channels == "rgb":
        out = rgb
    elif channels == "bgr":
        out = rgb[..., ::-1]
    else:
        raise ValueError(channels)
    out = np.ascontiguousarray(out, np.uint8)
    if status:
        out = np.zeros_like(out)
    return np.ascontiguousarray(out[..., 0]) if first_channel else out


def stages(data, info=None):
    """every stage of one accepted file: {"info", "stream", "raw", "status", "stored", "adler", "rows"} (rows None with a status)"""
    info = parse(data) if info is None else info
    if info["reason"] != "ok":
        raise ValueError(f"png restatement: refused ({info['reason']})")
    z = gather(data, info)
    raw, status, stored, endbit = inflate(z, info["raw_bytes"])
    res = {"info": info, "stream": z, "raw": raw, "stored": stored, "adler": None, "rows": None, "endbit": endbit}
    if not status & ~TOO_LITTLE:
        res["adler"] = adler32(raw)
        if res["adler"] != stored:
            status |= ADLER
    if status == 0:
        rows, bad = unfilter(raw, info)
        res["rows"] = rows
        if bad:
            status |= FILTER
    res["status"] = status
    return res


def decode(data, channels="bgr", first_channel=False):
    """-> (pixels, status)"""
    s = stages(data)
    rows = s["rows"] if s["rows"] is not None else np.zeros((s["info"]["H"], s["info"]["row_bytes"]), np.uint8)
    return pixels(rows, s["info"], channels, first_channel, s["status"]), s["status"]
