"""numpy restatement of the baseline JPEG DECODING rule written out in include/dsnerf.h (dsn_jpegd_*): the header parser with its
refusals, unstuffing, the entropy decoder as one serial pass AND as the subsequence synchronisation the device runs (the same
symbol step serves both), DC prediction, dequantisation, the IJG slow-integer IDCT in int32, libjpeg's "fancy" 4:2:0 upsampling with
its narrow-image exception, the 16-bit fixed-point colour conversion.  tests/test_jpeg_decode_host.py pins it to Pillow's pixels.

    parse(data) -> dict (H, W, mode, qsel / dcsel / acsel, quant, dc / ac tables, scan_offset, scan_length) or raises Refused(reason)
    coefficients(data, subseq_bits=None, mutant=None) -> (int16 [blocks, 64] zigzag, DC summed, status, rounds)
    pixels(coef, info, channels="bgr", gray=False, status=0, mutant=None) -> uint8 [H, W, 3] or [H, W]
    decode(data, ...) -> (pixels, status, rounds);  synchronise(...) -> the subsequence table at its fixed point

`mutant` names one deliberate mistake:
    "replicate_all", "plus8_both", "no_colour_half", "truncating_pass1", "one_dc_predictor", "keep_stuffing", "same_round_buffer"
"""
import numpy as np

import jpeg_restate as JR

M420, M444, MGRAY = JR.M420, JR.M444, JR.MGRAY
CORRUPT, PADDING, UNMATCHED, OVERRUN, MARKER, COUNT = 1, 2, 16, 32, 64, 128          # DSN_JPEGD_*: a frame's status bits
REASONS = ["ok", "not_jpeg", "truncated", "progressive", "extended", "arithmetic", "precision", "sampling", "components", "table16",
           "multiscan", "restart", "missing_table", "bad_table", "no_eoi", "bad_segment", "too_large"]          # dsn_jpeg_parse_host's status
ZIGZAG = JR.ZIGZAG


class Refused(ValueError):
    def __init__(self, reason):
        super().__init__(reason)
        self.reason = reason


# ---- the header ------------------------------------------------------------------------------------------------------------------------------
def derive(bits, vals, is_dc):
    """Annex C in the form the decoders use: lim[l-1] = (first code NOT of length <= l) left-justified in 16 bits; a 16-bit window v
    holds a code of length l = the smallest l with v < lim[l-1], and the symbol is vals[base[l-1] + (v >> (16 - l))]"""
    lim, base, code, k = [0] * 16, [0] * 16, 0, 0
    for ln in range(1, 17):
        base[ln - 1] = k - code
        code += bits[ln - 1]
        k += bits[ln - 1]
        if code > (1 << ln):
            raise Refused("bad_table")
        lim[ln - 1] = code << (16 - ln)
        code <<= 1
    if k > 256 or k != len(vals) or (is_dc and any(v > 15 for v in vals)):
        raise Refused("bad_table")
    return dict(bits=list(bits), vals=list(vals), lim=lim, base=base)


def parse(data):
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b"\xff\xd8":
        raise Refused("not_jpeg")
    quant, dc, ac, sof, i = {}, {}, {}, None, 2
    while True:
        if i + 4 > n:
            raise Refused("truncated")
        if data[i] != 0xFF:
            raise Refused("bad_segment")
        m = data[i + 1]
        if m == 0xFF:          # a fill byte
            i += 1
            continue
        L = int.from_bytes(data[i + 2:i + 4], "big")
        if L < 2 or i + 2 + L > n:
            raise Refused("truncated")
        seg = data[i + 4:i + 2 + L]
        i += 2 + L
        if 0xE0 <= m <= 0xEF or m == 0xFE:
            continue
        if m == 0xDB:
            j = 0
            while j < len(seg):
                if seg[j] >> 4:
                    raise Refused("table16")
                if (seg[j] & 15) > 3 or j + 65 > len(seg):
                    raise Refused("bad_segment")
                quant[seg[j] & 15] = list(seg[j + 1:j + 65])          # zigzag order, as the file has it
                j += 65
        elif m == 0xC4:
            j = 0
            while j < len(seg):
                if j + 17 > len(seg) or (seg[j] >> 4) > 1 or (seg[j] & 15) > 3:
                    raise Refused("bad_segment")
                bits = list(seg[j + 1:j + 17])
                cnt = sum(bits)
                if cnt > 256 or j + 17 + cnt > len(seg):
                    raise Refused("bad_table" if cnt > 256 else "bad_segment")
                (ac if seg[j] >> 4 else dc)[seg[j] & 15] = derive(bits, list(seg[j + 17:j + 17 + cnt]), not (seg[j] >> 4))
                j += 17 + cnt
        elif m == 0xC2:
            raise Refused("progressive")
        elif m in (0xC1, 0xC3, 0xC5, 0xC6, 0xC7):
            raise Refused("extended")
        elif m in (0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF):
            raise Refused("arithmetic")
        elif m == 0xDD:
            if len(seg) != 2:
                raise Refused("bad_segment")
            if seg[0] or seg[1]:
                raise Refused("restart")
        elif m == 0xC0:
            if sof is not None or len(seg) < 6:
                raise Refused("bad_segment")
            if seg[0] != 8:
                raise Refused("precision")
            H, W, nc = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big"), seg[5]
            if nc not in (1, 3):
                raise Refused("components")
            if len(seg) != 6 + 3 * nc or H == 0 or W == 0:
                raise Refused("bad_segment")
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c], seg[8 + 3 * c]) for c in range(nc)]
            samp = [c[1] for c in comps]
            if samp == [0x11] * nc:
                mode = MGRAY if nc == 1 else M444
            elif samp == [0x22, 0x11, 0x11]:
                mode = M420
            else:
                raise Refused("sampling")
            if any(c[2] > 3 for c in comps):
                raise Refused("bad_segment")
            sof = (H, W, nc, mode, comps)
        elif m == 0xDA:
            if sof is None or len(seg) < 1:
                raise Refused("bad_segment")
            H, W, nc, mode, comps = sof
            if seg[0] != nc:
                raise Refused("multiscan")
            if len(seg) != 4 + 2 * nc:
                raise Refused("bad_segment")
            dcsel, acsel = [], []
            for c in range(nc):
                if seg[1 + 2 * c] != comps[c][0] or (seg[2 + 2 * c] >> 4) > 3 or (seg[2 + 2 * c] & 15) > 3:
                    raise Refused("bad_segment")
                dcsel.append(seg[2 + 2 * c] >> 4)
                acsel.append(seg[2 + 2 * c] & 15)
            if tuple(seg[1 + 2 * nc:]) != (0, 63, 0):
                raise Refused("bad_segment")
            qsel = [c[2] for c in comps]
            if any(q not in quant for q in qsel) or any(t not in dc for t in dcsel) or any(t not in ac for t in acsel):
                raise Refused("missing_table")
            if data[-2:] != b"\xff\xd9" or n - 2 < i:
                raise Refused("no_eoi")
            if JR.n_blocks(H, W, mode) * 1664 >= 2 ** 31 or n >= 2 ** 27:
                raise Refused("too_large")
            return dict(H=H, W=W, mode=mode, ncomp=nc, qsel=qsel, dcsel=dcsel, acsel=acsel, quant=quant, dc=dc, ac=ac, scan_offset=i,
                        scan_length=n - 2 - i, file_length=n)
        else:
            raise Refused("bad_segment")


# ---- the scan ------------------------------------------------------------------------------------------------------------------------------------
def unstuff(scan, mutant=None):
    """a 0x00 behind a 0xFF is dropped; any other byte behind a 0xFF, or a 0xFF as the last byte, is a marker -> (bytes, marker seen)"""
    b = np.frombuffer(bytes(scan), np.uint8)
    prev_ff = np.concatenate([[False], b[:-1] == 0xFF])
    marker = bool((prev_ff & (b != 0)).any() or (len(b) and b[-1] == 0xFF))
    if mutant == "keep_stuffing":
        return b.tobytes(), marker
    return b[~(prev_ff & (b == 0))].tobytes(), marker


class Reader:
    """the unstuffed scan with the frame's resolved tables: the symbol step that the serial decoder and every subsequence share"""

    def __init__(self, info, raw):
        self.raw = bytes(raw) + b"\0" * 8          # bits past the end read as 0
        self.p_end = None
        self.total = 8 * len(raw)
        self.mode = info["mode"]
        self.comp = {M420: [0, 0, 0, 0, 1, 2], M444: [0, 1, 2], MGRAY: [0]}[self.mode]
        self.bpm = len(self.comp)
        self.tabs = []          # [component][0 DC, 1 AC] -> (length [65536], symbol [65536]) by the derived table's own search
        for c in range(info["ncomp"]):
            pair = []
            for t in (info["dc"][info["dcsel"][c]], info["ac"][info["acsel"][c]]):
                ln, sym, lo = np.zeros(65536, np.uint8), np.zeros(65536, np.uint8), 0
                vals = np.array(t["vals"] + [0], np.int64)
                for l in range(1, 17):
                    hi = min(t["lim"][l - 1], 65536)
                    if hi > lo:
                        ln[lo:hi] = l
                        sym[lo:hi] = vals[np.minimum((t["base"][l - 1] + (np.arange(lo, hi) >> (16 - l))) & 255, len(vals) - 1)]
                        lo = hi
                pair.append((ln.tolist(), sym.tolist()))
            self.tabs.append(pair)

    def run(self, p, k, z, end, coef=None, blk=0):
        """symbols from state (p, k, z) until p >= end or a symbol needs bits past the scan's end.  `blk`: the index the next block
        to START gets (the one in progress is blk - 1).  With `coef` (emitting) decoding stops behind block len(coef) - 1, whose end
        goes to self.p_end, and nothing past it is looked at.  -> (p, k, z, blocks started, flags)"""
        raw, total, started, flags = self.raw, self.total, 0, 0
        nb = len(coef) if coef is not None else 0
        while p < end:
            if coef is not None and (blk > nb or (z == 0 and blk == nb)):
                break
            v32 = (int.from_bytes(raw[p >> 3:(p >> 3) + 5], "big") >> (8 - (p & 7))) & 0xFFFFFFFF
            ln_t, sym_t = self.tabs[self.comp[k]][1 if z else 0]
            v = v32 >> 16
            ln = ln_t[v]
            if ln == 0:                      # no code: one bit on, unless the window hangs over the end
                if total - p < 16:
                    break
                p += 1
                flags |= UNMATCHED
                continue
            sym = sym_t[v]
            s = sym & 15
            if p + ln + s > total:
                break
            val = (v32 >> (32 - ln - s)) & ((1 << s) - 1) if s else 0
            if s and not val >> (s - 1):
                val -= (1 << s) - 1
            p += ln + s
            if z == 0:
                if coef is not None and blk < nb:
                    coef[blk, 0] = val
                blk += 1
                started += 1
                z = 1
            else:
                r = sym >> 4
                if s == 0:
                    z = z + 16 if r == 15 else 64
                    if z > 64:
                        flags |= OVERRUN
                else:
                    z += r
                    if z > 63:
                        flags |= OVERRUN
                        z = 64
                    else:
                        if coef is not None and 0 < blk <= nb:
                            coef[blk - 1, z] = val
                        z += 1
            if z >= 64:
                k, z = (k + 1) % self.bpm, 0
                if coef is not None and blk == nb:
                    self.p_end = p
                    break
        return p, k, z, started, flags


def synchronise(rd, B, mutant=None, max_rounds=None):
    """the device's rounds: -> (entry [S, 3], exit [S, 3], started [S], flags [S], rounds).  Round 0: every subsequence from
    (s B, 0, 0).  Round r: s takes the exit of s - 1 from the PREVIOUS round's buffer; equal to the entry it used: nothing; else it
    decodes again.  A round in which nothing changed is the last one, and it counts."""
    S = max(1, -(-rd.total // B))
    entry = [(s * B, 0, 0) for s in range(S)]
    ex, started, flags = [None] * S, [0] * S, [0] * S
    for s in range(S):
        *ex[s], started[s], flags[s] = rd.run(*entry[s], min((s + 1) * B, rd.total))
        ex[s] = tuple(ex[s])
    rounds, changed = 1, S > 1
    look = list(range(1, S))          # the subsequences whose predecessor's exit may differ from the entry they used
    while changed and (max_rounds is None or rounds < max_rounds):
        changed = False
        if mutant == "same_round_buffer":
            prev, look = ex, list(range(1, S))
        else:
            prev = {s - 1: ex[s - 1] for s in look}
        moved = []
        for s in look:
            if prev[s - 1] != entry[s]:
                entry[s] = prev[s - 1]
                *e, started[s], flags[s] = rd.run(*entry[s], min((s + 1) * B, rd.total))
                if tuple(e) != ex[s] and s + 1 < S:
                    moved.append(s + 1)
                ex[s] = tuple(e)
                changed = True
        look = moved
        rounds += 1
    return entry, ex, started, flags, rounds


def coefficients(data, subseq_bits=None, mutant=None, info=None):
    """-> (coef int16 [blocks, 64] in zigzag and scan order with DC values, status, rounds).  subseq_bits None: one serial pass
    (rounds 0); else the fixed point of the subsequence rounds, emitted subsequence by subsequence as the device does."""
    info = info or parse(data)
    raw, marker = unstuff(bytes(data)[info["scan_offset"]:info["scan_offset"] + info["scan_length"]], mutant)
    rd = Reader(info, raw)
    nb = JR.n_blocks(info["H"], info["W"], info["mode"])
    coef = np.zeros((nb, 64), np.int64)
    if subseq_bits is None:
        flags = rd.run(0, 0, 0, rd.total, coef, 0)[4]
        rounds = 0
    else:
        entry, ex, cnt, fl, rounds = synchronise(rd, subseq_bits, mutant)
        base, flags = 0, 0
        for s in range(len(entry)):
            flags |= rd.run(*entry[s], min((s + 1) * subseq_bits, rd.total), coef, base)[4]
            base += cnt[s]
    status = flags | (MARKER if marker else 0)
    if rd.p_end is None:          # the frame's last block was never completed
        status |= COUNT
    if status & (UNMATCHED | OVERRUN | MARKER | COUNT):
        status |= CORRUPT
    p = rd.total if rd.p_end is None else rd.p_end
    rest = rd.total - p
    tail = (int.from_bytes(rd.raw[p >> 3:(p >> 3) + 5], "big") >> (8 - (p & 7))) & 0xFFFFFFFF
    if rest > 7 or (rest and (tail >> (32 - rest)) != (1 << rest) - 1):
        status |= PADDING
    comp_of = np.tile(np.array(rd.comp), nb // rd.bpm)
    for c in range(info["ncomp"]):
        idx = np.nonzero((comp_of == c) if mutant != "one_dc_predictor" else np.ones(nb, bool))[0]
        coef[idx, 0] = np.cumsum(coef[idx, 0])
        if mutant == "one_dc_predictor":
            break
    return coef.astype(np.int32).astype(np.int16), status, rounds


# ---- pixels ---------------------------------------------------------------------------------------------------------------------------------
def _i32(x):
    return np.asarray(x).astype(np.int32)


def _idct_pass(d, shift, mutant=None):
    """one pass of jpeg_idct_islow along the last axis, int32 (wrapping as the device's registers do)"""
    i0, i1, i2, i3, i4, i5, i6, i7 = (d[..., i] for i in range(8))
    c = lambda v: np.int32(v)          # noqa: E731
    z1 = (i2 + i6) * c(4433)
    t2 = z1 + i6 * c(-15137)
    t3 = z1 + i2 * c(6270)
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * c(9633)
    t0, t1, t2, t3 = t0 * c(2446), t1 * c(16819), t2 * c(25172), t3 * c(12299)
    z1, z2, z3, z4 = z1 * c(-7373), z2 * c(-20995), z3 * c(-16069) + z5, z4 * c(-3196) + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    half = c(0) if mutant == "truncating_pass1" and shift == 11 else c(1 << (shift - 1))
    out = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([(o + half) >> shift for o in out], -1)


def idct(coef, table, mutant=None):
    """int16 [N, 64] zigzag coefficients x a zigzag-order table [64] -> samples uint8 [N, 8, 8]: columns, then rows; the result
    taken & 1023 as a signed 10-bit number, + 128, clamped"""
    nat = np.zeros((len(coef), 64), np.int32)
    with np.errstate(over="ignore"):
        nat[:, ZIGZAG] = _i32(coef) * _i32(table)[None, :]
        d = nat.reshape(-1, 8, 8)
        cols = _idct_pass(d.transpose(0, 2, 1), 11, mutant).transpose(0, 2, 1)
        rows = _idct_pass(cols, 18, mutant)
    x = rows & 1023
    x = np.where(x >= 512, x - 1024, x) + 128
    return np.clip(x, 0, 255).astype(np.uint8)


def planes(coef, info, mutant=None):
    """the component planes at the MCU grid's size, uint8"""
    H, W, mode = info["H"], info["W"], info["mode"]
    mw, mh, bpm, comp = JR.geometry(H, W, mode)
    c4 = np.asarray(coef).reshape(mh, mw, bpm, 64)
    out = []
    for c in range(info["ncomp"]):
        q = info["quant"][info["qsel"][c]]
        if mode == M420 and c == 0:
            b = idct(c4[:, :, :4].reshape(-1, 64), q, mutant).reshape(mh, mw, 2, 2, 8, 8)
            out.append(b.transpose(0, 2, 4, 1, 3, 5).reshape(mh * 16, mw * 16))
        else:
            k = (c + 3 if c else 0) if mode == M420 else c
            b = idct(c4[:, :, k].reshape(-1, 64), q, mutant).reshape(mh, mw, 8, 8)
            out.append(b.transpose(0, 2, 1, 3).reshape(mh * 8, mw * 8))
    return out


def upsample_420(p, H, W, mutant=None):
    """libjpeg's h2v2 fancy upsampling of the chroma plane's real part [ceil(H/2), ceil(W/2)] -> int64 [H, W]"""
    ch, cw = (H + 1) // 2, (W + 1) // 2
    p = p[:ch, :cw].astype(np.int64)
    if cw <= 2 or mutant == "replicate_all":
        return np.repeat(np.repeat(p, 2, 0), 2, 1)[:H, :W]
    up, down = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
    v = np.empty((2 * ch, cw), np.int64)
    v[0::2], v[1::2] = 3 * p + up, 3 * p + down
    left, right = np.concatenate([v[:, :1], v[:, :-1]], 1), np.concatenate([v[:, 1:], v[:, -1:]], 1)
    o = np.empty((2 * ch, 2 * cw), np.int64)
    o[:, 0::2] = (3 * v + left + 8) >> 4
    o[:, 1::2] = (3 * v + right + (8 if mutant == "plus8_both" else 7)) >> 4          # (the edges: 3 v + v = 4 v)
    return o[:H, :W]


def pixels(coef, info, channels="bgr", gray=False, status=0, mutant=None):
    H, W, mode = info["H"], info["W"], info["mode"]
    shape = (H, W) if gray else (H, W, 3)
    if status & CORRUPT:
        return np.zeros(shape, np.uint8)
    pl = planes(coef, info, mutant)
    y = pl[0][:H, :W].astype(np.int64)
    if mode == MGRAY:
        return y.astype(np.uint8) if gray else np.repeat(y[..., None], 3, 2).astype(np.uint8)
    assert not gray, "a grey output needs a one-component file"
    if mode == M420:
        cb, cr = upsample_420(pl[1], H, W, mutant) - 128, upsample_420(pl[2], H, W, mutant) - 128
    else:
        cb, cr = pl[1][:H, :W].astype(np.int64) - 128, pl[2][:H, :W].astype(np.int64) - 128
    half = 0 if mutant == "no_colour_half" else 32768
    r = y + ((91881 * cr + half) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + half) >> 16)
    b = y + ((116130 * cb + half) >> 16)
    return np.clip(np.stack([b, g, r] if channels == "bgr" else [r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data, channels="bgr", gray=False, subseq_bits=None, mutant=None):
    """-> (pixels, status, rounds)"""
    info = parse(data)
    coef, status, rounds = coefficients(data, subseq_bits, mutant, info)
    return pixels(coef, info, channels, gray, status, mutant), status, rounds


# ---- files with other Huffman tables (what the tests decode besides the encoder's own files) ----------------------------------------------
def optimal_table(freq):
    """libjpeg's jpeg_gen_optimal_table: (bits [16], vals) of the length-limited Huffman code for symbol counts freq [256]; the
    pseudo-symbol 256 keeps the all-ones code free"""
    freq = [int(v) for v in freq] + [1]
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, 1 << 62
        for i in range(257):
            if freq[i] and freq[i] <= v:
                v, c1 = freq[i], i
        c2, v = -1, 1 << 62
        for i in range(257):
            if freq[i] and freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 33
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    return bits[1:17], [j for n in range(1, 33) for j in range(256) if codesize[j] == n]


def symbol_counts(coef, mode):
    """how often each DC size and each AC run/size symbol occurs per table (0: Y, 1: Cb and Cr) in the scan of `coef`"""
    coef = np.asarray(coef, np.int64).reshape(-1, 64)
    comp = {M420: [0, 0, 0, 0, 1, 2], M444: [0, 1, 2], MGRAY: [0]}[mode]
    dc, ac, pred = np.zeros((2, 256), np.int64), np.zeros((2, 256), np.int64), [0, 0, 0]
    for b, blk in enumerate(coef):
        c = comp[b % len(comp)]
        t = 1 if c else 0
        dc[t, int(abs(int(blk[0]) - pred[c])).bit_length()] += 1
        pred[c] = int(blk[0])
        last = 0
        for z in np.nonzero(blk[1:])[0] + 1:
            run = int(z) - last - 1
            ac[t, 0xF0] += run >> 4
            ac[t, ((run & 15) << 4) | int(abs(int(blk[z]))).bit_length()] += 1
            last = int(z)
        if last != 63:
            ac[t, 0] += 1
    return dc, ac


class tables:
    """with tables(dc, ac): jpeg_restate writes its headers and scans with these (bits, vals) pairs instead of Annex K's"""

    NAMES = ("DC_BITS", "DC_VALS", "AC_BITS", "AC_VALS", "DC_TAB", "AC_TAB")

    def __init__(self, dc, ac):
        self.new = ([t[0] for t in dc], [t[1] for t in dc], [t[0] for t in ac], [t[1] for t in ac],
                    [JR.huff_table(*t) for t in dc], [JR.huff_table(*t) for t in ac])

    def __enter__(self):
        self.old = [getattr(JR, n) for n in self.NAMES]
        for n, v in zip(self.NAMES, self.new):
            setattr(JR, n, v)

    def __exit__(self, *exc):
        for n, v in zip(self.NAMES, self.old):
            setattr(JR, n, v)


def optimised_file(coef, H, W, mode, quality):
    """the file around `coef` with Huffman tables made for it (what libjpeg's optimize_coding writes)"""
    dc, ac = symbol_counts(coef, mode)
    nt = 1 if mode == MGRAY else 2
    dct = [optimal_table(dc[t]) for t in range(nt)] + [(JR.DC_BITS[1], JR.DC_VALS[1])] * (2 - nt)
    act = [optimal_table(ac[t]) for t in range(nt)] + [(JR.AC_BITS[1], JR.AC_VALS[1])] * (2 - nt)
    with tables(dct, act):
        return JR.scan_file(coef, H, W, mode, quality)
