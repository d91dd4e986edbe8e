"""The PNG encoder's rule on the host (no GPU): the numpy restatement tests/png_encode_restate.py writes valid files (zlib, Pillow and
the decoder's restatement give the levels back), its parts hold on their own (complete codes within their limits, the block type of
least cost, the filter heuristic), files stay inside the derived bounds, the library checks its arguments, and seven mutants of the
restatement each fail a named check."""
import ctypes as C
import io
import zlib

import numpy as np
import pytest

import png_decode_restate as DR
import png_encode_restate as R

SIZES = [(1, 1), (1, 2), (3, 1), (21, 1), (22, 1), (5, 9), (64, 64)]          # (W, H): 21 and 22 wide are row bytes 63 and 66
MODES = ["grey", "rgb", "replicated"]
FIB = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765, 10946, 17711, 28657, 46368, 75025, 121393,
       196418, 317811, 514229, 832040]
MUTANTS = {          # mutant -> the check below that it fails
    "mutant_no_limit": "check_lengths_within_limit",
    "mutant_cross": "check_file_is_valid",
    "mutant_no_separator": "check_file_is_valid",
    "mutant_crc_no_type": "check_file_is_valid",
    "mutant_adler_pixels": "check_file_is_valid",
    "mutant_paeth": "check_file_is_valid",
    "mutant_unsigned": "check_filter_choice",
}


def contents(H, W, seed=0):
    """noise (stored blocks must win), constant (runs of 258) and smooth uint8 frames [H, W, 3], by name"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    smooth = np.stack([(128 + 100 * np.sin(x / 9.0 + k) * np.cos(y / 7.0 + 0.3 * k)).astype(np.uint8) for k in range(3)], -1)
    const = np.empty((H, W, 3), np.uint8)
    const[...] = np.array([77, 130, 200])
    return {"noise": rng.integers(0, 256, (H, W, 3), dtype=np.uint8), "constant": const, "smooth": smooth}


def in_mode(img, mode):
    """-> (the encoder's input, its keyword arguments, the levels [H, W] / [H, W, 3 in R, G, B] every decoder must return)"""
    if mode == "rgb":
        return img, {}, img[:, :, ::-1]
    g = np.ascontiguousarray(img[:, :, 0])
    return (g, {}, g) if mode == "grey" else (g, {"replicate": True}, np.repeat(g[:, :, None], 3, axis=2))


# ---- the named checks ----------------------------------------------------------------------------------------------------------------------------
def check_file_is_valid(img, kw, want, chunk=256, **mutants):
    """zlib inflates the IDAT to the raw stream and every chunk's bytes ON THEIR OWN to the chunk; Pillow and the decoder's restatement
    return the levels"""
    Image = pytest.importorskip("PIL.Image")
    stages = {}
    data, status = R.encode_one(img, chunk=chunk, stages=stages, **kw, **mutants)
    assert status == 0
    assert zlib.decompress(R.idat_payload(data)) == stages["raw"].tobytes()
    for k, piece in enumerate(stages["pieces"]):
        assert zlib.decompressobj(-15).decompress(piece) == stages["raw"][chunk * k:chunk * (k + 1)].tobytes(), k
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), want)
    got, st = DR.decode(data, channels="native")
    assert st == 0 and np.array_equal(got.reshape(want.shape), want)
    W, H = want.shape[1], want.shape[0]
    assert len(data) <= R.encode_max_bytes(W, H, 1 if want.ndim == 2 else 3, chunk)
    return data, stages


def check_lengths_within_limit(counts, limit, **mutants):
    lens = R.huff_lengths(counts, limit, **mutants)
    assert max(lens) <= limit, (max(lens), limit)
    assert R.kraft(lens) == 1, R.kraft(lens)
    assert all((l > 0) == (c > 0) for l, c in zip(lens, counts)) or sum(1 for c in counts if c) < 2
    return lens


FILTER_ROWS = {          # two rows [2, 8] of one channel on which filter k is the one of least signed magnitude, for the second row
    0: ([[100, 20, 230, 60, 150, 5, 90, 200], [1, 255, 2, 254, 1, 255, 2, 254]]),
    1: ([[9, 200, 31, 120, 77, 250, 3, 66], [50, 52, 54, 56, 58, 60, 62, 64]]),
    2: ([[10, 200, 30, 120, 70, 250, 0, 66], [11, 201, 31, 121, 71, 251, 1, 67]]),
    3: ([[0, 100, 0, 100, 0, 100, 0, 100], [40, 70, 35, 68, 34, 67, 33, 67]]),
    4: ([[10, 20, 40, 80, 120, 160, 200, 240], [30, 40, 60, 100, 140, 180, 220, 4]]),
}


def check_filter_choice(**mutants):
    for k, rows in FILTER_ROWS.items():
        rows = np.array(rows, np.uint8)
        f5 = R.filtered_rows(rows, 1)
        mag = np.where(f5 < 128, f5, 256 - f5).sum(axis=2)[:, 1]
        assert int(np.argmin(mag)) == k, (k, mag)               # the case is what it claims to be
        raw, choice = R.filter_image(rows, 1, **mutants)
        assert choice[1] == k, (k, choice, mag)
        assert raw.reshape(2, 9)[1, 0] == k
    # ties go to the lower filter number: a first row has Up == None and Paeth == Sub; zeros tie all five
    _, choice = R.filter_image(np.array([[5, 5, 5, 5]], np.uint8), 1, **mutants)
    assert choice[0] == 1          # None costs 20, Sub / Paeth 5, Up 20, Average 5 + 3 + 3 + 3: Sub before Paeth
    _, choice = R.filter_image(np.zeros((3, 4), np.uint8), 1, **mutants)
    assert choice.tolist() == [0, 0, 0]


# ---- the file is a valid PNG -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_file_is_valid(size, mode):
    W, H = size
    for kind, img in contents(H, W).items():
        x, kw, want = in_mode(img, mode)
        data, stages = check_file_is_valid(x, kw, want, chunk=256)
        if kind == "noise" and W * H >= 64 * 64 and mode != "replicated":          # (three equal channels do compress)
            assert all(p["btype"] == 0 for p in stages["plans"][:-1]), "noise: stored blocks must win"
        if kind == "constant" and W * H >= 64 * 64:             # (a chunk of 256 bytes has no room for a match of 258)
            data, stages = check_file_is_valid(x, kw, want, chunk=1024)
            assert any(t[0] == 258 for p in stages["plans"] for t in p.get("tokens", ())), "constant: runs of 258 must appear"


def test_float_levels_and_status():
    v = np.array([[0.0, 0.5 / 255, 1.5 / 255, 2.5 / 255, 1.0, 1.7, -0.3, np.nan, np.inf, -np.inf]], np.float32)
    lv, bad = R.levels(v)
    assert lv.tolist() == [[0, 0, 2, 2, 255, 255, 0, 0, 255, 0]] and bad
    assert R.levels(v[:, :7])[1] is False
    data, status = R.encode_one(v)
    assert status == 1 and np.array_equal(DR.decode(data, channels="native")[0].reshape(1, 10), lv)


def test_forced_filters_and_chunk_edges():
    img = contents(9, 5)["smooth"]
    for f in range(5):
        st = {}
        data, _ = R.encode_one(img, filt=f, chunk=256, stages=st)
        assert set(st["filters"].tolist()) == {f}
        assert np.array_equal(DR.decode(data, channels="native")[0], img[:, :, ::-1])
    for C_ in (256, 1024):
        for n in (C_ - 1, C_, C_ + 1, 2 * C_ + 1):          # raw sizes around the chunk edges: one grey row of n - 1 pixels
            g = (np.arange(n - 1) * 7 % 251).astype(np.uint8)[None, :]
            plans = []
            z = R.deflate(R.filter_image(g, 1)[0], 1, n, C_, plans=plans)
            assert len(plans) == (n + C_ - 1) // C_
            assert zlib.decompress(z, -15) == R.filter_image(g, 1)[0].tobytes()


# ---- the parts hold on their own ---------------------------------------------------------------------------------------------------------------------
def huff_cases():
    cases = [(FIB[:n], 15) for n in (17, 18, 20, 25, 30)] + [(FIB[:n], 7) for n in (9, 10, 12, 19)]
    cases += [([0] * 40 + [9] + [0] * 245, 15), ([0] * 19, 7)]                                  # one used symbol, none at all
    cases += [([0, 3, 0, 0, 0, 0, 0, 5] + [0] * 278, 15), ([1] * 286, 15), ([1] * 19, 7)]       # two used symbols, every symbol once
    rng = np.random.default_rng(5)
    cases += [((rng.integers(0, 50, 286) * (rng.random(286) < 0.6)).tolist(), 15) for _ in range(4)]
    return cases


def test_code_lengths():
    for counts, limit in huff_cases():
        lens = check_lengths_within_limit(counts, limit)
        codes = R.canonical(lens)
        used = sorted((l, c) for l, c in zip(lens, codes) if l)
        words = [format(c, "0%db" % l) for l, c in used]
        assert len(set(words)) == len(words)
        assert not any(b.startswith(a) for i, a in enumerate(words) for b in words[i + 1:]), "prefix-free"
    assert max(R.huff_lengths(FIB[:17], 15, mutant_no_limit=True)) == 16          # the 15-bit limit IS needed from 17 symbols on
    assert max(R.huff_lengths(FIB[:9], 7, mutant_no_limit=True)) == 8
    one = R.huff_lengths([0] * 40 + [9] + [0] * 245, 15)
    assert one[0] == 1 and one[40] == 1 and sum(one) == 2                          # the lowest unused symbol completes the code
    assert R.huff_lengths([0, 3, 0, 0, 0, 0, 0, 5], 15) == [0, 1, 0, 0, 0, 0, 0, 1]
    assert sorted(set(R.huff_lengths([1] * 286, 15))) == [8, 9]
    # optimal where no limit binds: the cost equals the textbook Huffman cost
    import heapq
    rng = np.random.default_rng(6)
    for _ in range(5):
        counts = rng.integers(1, 1000, 40).tolist()
        h = list(counts)
        heapq.heapify(h)
        cost = 0
        while len(h) > 1:
            a, b = heapq.heappop(h), heapq.heappop(h)
            cost += a + b
            heapq.heappush(h, a + b)
        assert sum(c * l for c, l in zip(counts, R.huff_lengths(counts, 15))) == cost


def independent_costs(raw, cs, ce, plan):
    """the three block costs from the tokens alone, by RFC 1951's tables rather than the restatement's sums"""
    stored = 8 * (1 + 4 + (ce - cs))
    fixed = dynamic = 3
    for t in plan["tokens"] + [(256,)]:
        if len(t) == 1:
            fixed += R.FIXED_LL[t[0]]
            dynamic += plan["ll_lens"][t[0]]
        else:
            k, nb, _ = R.length_code(t[0])
            kd, nbd, _ = R.dist_code(t[1])
            assert R.LEN_BASE[k] <= t[0] < R.LEN_BASE[k] + (1 << nb) or t[0] == 258
            assert R.DIST_BASE[kd] <= t[1] < R.DIST_BASE[kd] + (1 << nbd)
            fixed += R.FIXED_LL[257 + k] + nb + 5 + nbd
            dynamic += plan["ll_lens"][257 + k] + nb + plan["d_lens"][kd] + nbd
    h = plan["header"]
    cl = h["cl_lens"]
    assert R.kraft(cl) == 1 and max(cl) <= 7
    dynamic += 14 + 3 * h["hclen"] + sum(cl[s] + (2 if s == 16 else 3 if s == 17 else 7 if s == 18 else 0) for s, _ in h["seq"])
    return [stored, fixed, dynamic]


def test_block_type_is_the_cheapest():
    seen = set()
    for (W, H) in [(5, 9), (22, 1), (64, 64)]:
        for kind, img in contents(H, W).items():
            st = {}
            R.encode_one(img, chunk=256, stages=st)
            raw = st["raw"]
            for k, plan in enumerate(st["plans"]):
                cs, ce = 256 * k, min(256 * k + 256, len(raw))
                costs = independent_costs(raw, cs, ce, plan)
                assert costs == [plan["stored"], plan["fixed"], plan["dynamic"]]
                assert plan["btype"] == costs.index(min(costs))
                assert R.kraft(plan["ll_lens"]) == 1 and R.kraft(plan["d_lens"]) == 1
                seen.add(plan["btype"])
    assert seen == {0, 1, 2}


def test_parse_is_greedy_and_inside_its_chunk():
    img = contents(64, 64)["smooth"]
    st = {}
    R.encode_one(img, chunk=1024, stages=st)
    raw = st["raw"]
    for k, plan in enumerate(st["plans"]):
        p = 1024 * k
        for t in plan.get("tokens", ()):
            if len(t) == 2:
                n, d = t
                assert d in (1, 3, 1 + 64 * 3) and p - d >= 1024 * k and 3 <= n <= 258 and p + n <= min(1024 * (k + 1), len(raw))
                assert all(raw[p + i] == raw[p + i - d] for i in range(n))
                p += n
            else:
                assert raw[p] == t[0]
                p += 1
        assert p == min(1024 * (k + 1), len(raw))


def test_filter_choice():
    check_filter_choice()


# ---- derived bars --------------------------------------------------------------------------------------------------------------------------------
def test_constant_image_is_small():
    """a 258-byte match costs at most 15 + 5 + 15 + 13 = 48 bits and here 2 (one code each); the chunks' headers add the rest"""
    img = np.empty((256, 256, 3), np.uint8)
    img[...] = np.array([77, 130, 200])
    data, _ = R.encode_one(img)
    assert len(data) < 0.03 * img.size, len(data)
    assert np.array_equal(DR.decode(data, channels="native")[0], img[:, :, ::-1])


def test_bounds():
    for (W, H, ch, chunk) in [(1, 1, 1, 256), (64, 64, 3, 256), (64, 64, 3, 32768), (511, 3, 1, 1024)]:
        n = H * (1 + W * ch)
        nch = (n + chunk - 1) // chunk
        assert R.encode_max_bytes(W, H, ch, chunk) == 8 + 25 + 12 + 2 + 4 + 12 + n + 5 * nch + 5 * (nch - 1)
        img = np.random.default_rng(7).integers(0, 256, (H, W, ch), dtype=np.uint8)
        data, _ = R.encode_one(img[:, :, 0] if ch == 1 else img, chunk=chunk, stored_only=True, filt=0)
        assert len(data) == R.encode_max_bytes(W, H, ch, chunk)          # every chunk stored: the bound is reached, never passed
        assert zlib.decompress(R.idat_payload(data))[1:1 + W * ch] == (img[0, :, 0] if ch == 1 else img[0, :, ::-1]).tobytes()


# ---- the library's argument checks (it loads without a GPU) ------------------------------------------------------------------------------------------
def test_argument_checks():
    import dsnerf_amd
    lib = dsnerf_amd._lib.lib()
    z, one, f = None, C.c_void_p(256), C.c_float(255.0)
    assert lib.dsn_png_encode_max_bytes(64, 64, 3, 256) == R.encode_max_bytes(64, 64, 3, 256)
    assert lib.dsn_png_encode_max_bytes(1, 1, 1, 32768) == 63 + 2 + 5
    assert lib.dsn_png_encode_max_bytes(64, 64, 2, 256) == 0 and lib.dsn_png_encode_max_bytes(0, 64, 3, 256) == 0
    assert lib.dsn_png_encode_max_bytes(64, 64, 3, 300) == 0 and lib.dsn_png_encode_max_bytes(16385, 64, 3, 256) == 0
    assert lib.dsn_png_deflate_max_bytes(1000, 256) == R.deflate_max_bytes(1000, 256)
    assert lib.dsn_png_encode_workspace_bytes(2, 64, 64, 1, 256) > 2 * 64 * (1 + 64 * 3) * 4
    assert lib.dsn_png_encode_workspace_bytes(0, 64, 64, 1, 256) == 0 and lib.dsn_png_encode_workspace_bytes(1, 64, 64, 3, 256) == 0
    big = 1 << 40
    bad = [
        (lambda: lib.dsn_png_encode(one, 0, 1, 8, 8, 1, 0, f, 5, 100, 0, one, 1000, one, one, one, big, z), b"chunk must be a power of two"),
        (lambda: lib.dsn_png_encode(one, 0, 1, 8, 8, 1, 0, f, 5, 65536, 0, one, 1000, one, one, one, big, z), b"chunk must be a power of two"),
        (lambda: lib.dsn_png_encode(one, 0, 1, 8, 8, 3, 0, f, 5, 256, 0, one, 1000, one, one, one, big, z), b"mode DSN_PNGE_GRAY"),
        (lambda: lib.dsn_png_encode(one, 0, 1, 0, 8, 1, 0, f, 5, 256, 0, one, 1000, one, one, one, big, z), b"W and H must be"),
        (lambda: lib.dsn_png_encode(one, 2, 1, 8, 8, 1, 0, f, 5, 256, 0, one, 1000, one, one, one, big, z), b"dtype"),
        (lambda: lib.dsn_png_encode(one, 0, 1, 8, 8, 1, 0, f, 6, 256, 0, one, 1000, one, one, one, big, z), b"filter must be"),
        (lambda: lib.dsn_png_encode(one, 0, 16385, 8, 8, 1, 0, f, 5, 256, 0, one, 1000, one, one, one, big, z), b"F must be"),
        (lambda: lib.dsn_png_encode(z, 0, 1, 8, 8, 1, 0, f, 5, 256, 0, one, 1000, one, one, one, big, z), b"null argument"),
        (lambda: lib.dsn_png_encode(one, 0, 1, 8, 8, 1, 0, f, 5, 256, 0, one, 1000, one, one, C.c_void_p(260), big, z), b"256-byte aligned"),
        (lambda: lib.dsn_png_encode(one, 0, 1, 8, 8, 1, 0, f, 5, 256, 0, one, 1000, one, one, one, 16, z), b"workspace_bytes is too small"),
        (lambda: lib.dsn_png_encode(C.c_void_p(258), 1, 1, 8, 8, 1, 0, f, 5, 256, 0, one, 1000, one, one, one, big, z), b"4-byte aligned"),
        (lambda: lib.dsn_png_filter(z, 0, 1, 8, 8, 1, 0, f, 5, z, z, z), b"dsn_png_filter: null argument"),
        (lambda: lib.dsn_png_filter(one, 0, 1, 8, 8, 1, 0, f, -1, one, one, z), b"filter must be"),
        (lambda: lib.dsn_png_deflate(z, 1, 100, 1, 9, 256, 0, z, 0, z, z, z, 0, z), b"dsn_png_deflate: null argument"),
        (lambda: lib.dsn_png_deflate(one, 1, 0, 1, 9, 256, 0, one, 0, one, one, one, big, z), b"n must be"),
        (lambda: lib.dsn_png_deflate(one, 1, 100, 0, 9, 256, 0, one, 0, one, one, one, big, z), b"bpp must be"),
        (lambda: lib.dsn_png_deflate(one, 1, 100, 1, 9, 128, 0, one, 0, one, one, one, big, z), b"chunk must be"),
        (lambda: lib.dsn_png_deflate(one, 1, 100, 1, 9, 256, 0, one, 0, one, one, one, 8, z), b"workspace_bytes is too small"),
        (lambda: lib.dsn_huff_lengths(z, 1, 19, 7, z, z), b"dsn_huff_lengths: null argument"),
        (lambda: lib.dsn_huff_lengths(one, 1, 19, 4, one, z), b"at most 2^limit"),
        (lambda: lib.dsn_huff_lengths(one, 1, 289, 15, one, z), b"n must be 2 ... 288"),
        (lambda: lib.dsn_huff_lengths(one, 1, 19, 16, one, z), b"limit must be"),
        (lambda: lib.dsn_png_adler(z, 1, 10, z, z, 0, z), b"dsn_png_adler: null argument"),
        (lambda: lib.dsn_png_adler(one, 1, 10, one, one, 4, z), b"below 8 F"),
        (lambda: lib.dsn_png_container(z, 10, z, z, z, 1, 8, 8, 3, z, 0, z, z, z, 0, z), b"dsn_png_container: null argument"),
        (lambda: lib.dsn_png_container(one, 10, one, one, z, 1, 8, 8, 2, one, 0, one, one, one, 4, z), b"channels must be 1 or 3"),
        (lambda: lib.dsn_png_container(one, 10, one, one, one, 1, 8, 8, 3, one, 0, one, one, one, 4, z), b"must differ"),
        (lambda: lib.dsn_png_container(one, 10, one, one, z, 1, 8, 8, 3, one, 0, one, one, one, 2, z), b"below 4 F"),
    ]
    for call, msg in bad:
        assert call() != 0 and msg in lib.dsn_last_error(), (msg, lib.dsn_last_error())
    assert lib.dsn_png_encode(z, 0, 0, 8, 8, 1, 0, f, 5, 256, 0, z, 0, z, z, z, 0, z) == 0          # no frames: nothing to do
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dsnerf_amd.png.encode(np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="jpeg.imwrite"):
        dsnerf_amd.png.imwrite("frame.jpg", np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(ValueError):
        dsnerf_amd.png.encode_device(np.zeros((8, 8, 3), np.uint8), chunk=300)
    with pytest.raises(ValueError):
        dsnerf_amd.png.encode_device(np.zeros((8, 8, 3), np.uint8), filter="best")
    with pytest.raises(ValueError):
        dsnerf_amd.png.encode_device(np.zeros((8, 8, 3), np.uint8), channels="gbr")


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------------------
def mutant_case(name):
    """the inputs on which the mutant's named check must fail"""
    H, W = 12, 40
    y, x = np.mgrid[0:H, 0:W]
    smooth = np.stack([(x * 5 + y * 3) % 256, (x * 2 + y * 7) % 256, (x * y) % 256], -1).astype(np.uint8)
    if name == "mutant_no_limit":
        return lambda **m: check_lengths_within_limit(FIB[:20], 15, **m)
    if name == "mutant_unsigned":
        return lambda **m: check_filter_choice(**m)
    if name == "mutant_cross":          # rows repeat: a match at the row distance reaches before a chunk's start unless it is cut there
        rep = np.tile(np.random.default_rng(8).integers(0, 256, (1, W, 3), dtype=np.uint8), (H, 1, 1))
        return lambda **m: check_file_is_valid(rep, {"filt": 0}, rep[:, :, ::-1], chunk=256, **m)
    if name == "mutant_paeth":
        px = np.random.default_rng(9).integers(0, 4, (H, W, 3), dtype=np.uint8) * 3          # many ties among pa, pb, pc
        return lambda **m: check_file_is_valid(px, {"filt": 4}, px[:, :, ::-1], chunk=256, **m)
    return lambda **m: check_file_is_valid(smooth, {}, smooth[:, :, ::-1], chunk=256, **m)


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutant_fails_its_check(name):
    run = mutant_case(name)
    run()                                                        # the rule itself passes the check on these inputs
    with pytest.raises((AssertionError, zlib.error, ValueError, OSError, SyntaxError)):
        run(**{name: True})
