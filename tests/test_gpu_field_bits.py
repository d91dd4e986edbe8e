"""The split-fp16 field, lighting and screen kernels against RECORDED bits (tests/golden/field16_bits.npz).

test_gpu_tiles.py judges these kernels against float64 with a tolerance; a change of instruction scheduling, register allocation or
compiler options must not move one output bit, and a tolerance cannot see that.  The fixture holds, for the parameter sets `w4` and
`default` and every point of test_gpu_tiles' 4096-point pool (near / shell / far bands; the pool is imported, not copied), the raw
bits of
  field.*    sigma, essence, d sigma/dx of the single launch (_lib.field: k_field16<full>) AND of _lib.field_forward +
             _lib.field_reverse (k_field16<forward>, k_field16<reverse>): one table for both forms - the recorder refuses to write
             a fixture unless the recording library gives the two forms the same bits (the gradient of the split form where
             sigma > 0, the binding's zeros elsewhere),
  light.*    the colour of _lib.light (k_light16, dense) on the pool's lighting inputs,
  shade.*    colour and light factor of _lib.shade(want_factor=True) on the pool's shading inputs (the normal search, then
             k_light16<true>; without the factor output k_light16<false> gives the same colour bits and is held to the same table),
  screen.*   the density screen's estimate and term magnitude (_lib.screen_debug: k_screen16<8>; its 4-wave and x2 variants are held
             to the same table),
and, once (w4),
  multi.*    the colours of a 64 x 64 x 64 frame under three lights in one pass (_lib.render_rays_lights: k_light16_multi),
  density.*  sigma of the density-only kernel (k_field16<density only>) on a 16 x 16 x 16 grid over the posed body's box, per set:
             that kernel is reached through dsn_density_grid only, which makes its own points from grid axes and warps them, so it
             cannot be handed the pool; the grid is a function of the committed golden case alone.  The test repeats the block
             along x (the x axis holds the 16 values k times) until more points survive the warp than G T: some workgroup then
             walks a second tile, and every copy of the block must hold the recorded bits.

The fixture was recorded with scripts/record_field_bits.py from the library of the commit BEFORE the one that added this module
(the recorder takes the library's path) and is never re-recorded from the build under test: a kernel change that moves a bit on
purpose re-records it from its own parent's point of view, i.e. says so in its diff.

Every launch on the pool is compared bit for bit at 1, 31, 129 and G T + 1 points (G persistent workgroups, T = 128: at G T + 1 one
workgroup walks a second tile; the screen's tiles are 256 points: G 2T + 1 as well), dense and - where the binding takes a list -
through a shuffled list; the sigma > 0 list is compared as a set.  Outputs being position independent bit for bit (test_gpu_tiles
assertion 4), one table per pool point serves every count and form.  A fixture with one bit of one gradient and of one grid density
flipped fails test_field_bits[w4] and test_density_only_bits[default] (run once on the MI355X when this module was written)."""
import os

import numpy as np
import pytest
import torch

import test_gpu_tiles as TT
from test_gpu_relight import five_lights
from test_gpu_round2 import full_frame, renderer_with

pytestmark = pytest.mark.gpu

TAGS = ("w4", "default")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "field16_bits.npz")
GRID = 16                      # density-only kernel: GRID^3 points


def counts(G):
    return [1, 31, 129, G * TT.T + 1]


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.int32)


def grid_axes(g):
    """GRID points per axis over the posed vertices' box + 5 cm"""
    lo, hi = g["xyz"].reshape(-1, 3).min(0) - 0.05, g["xyz"].reshape(-1, 3).max(0) + 0.05
    return [np.linspace(lo[k], hi[k], GRID).astype(np.float32) for k in range(3)]


def run_field(ctx, s, x, act):
    """bits of (single sigma, essence, grad), (split sigma, essence, grad), the sigma > 0 list of the split form"""
    lib = ctx.lib
    single = [bits(t) for t in lib.field(s["scene"], s["packed"], x, active=act)]
    sig, ess, rec, pos = lib.field_forward(s["scene"], s["packed"], x, active=act)
    gr = lib.field_reverse(s["scene"], s["packed"], x, rec, pos, sig, ess)
    torch.cuda.synchronize()
    n_pos = int(pos[1][0])
    return single, [bits(sig), bits(ess), bits(gr)], pos[0].cpu().numpy()[:n_pos]


def run_light(ctx, s, src):
    L = s["L"]
    return bits(ctx.lib.light(s["packed"], *(TT.Tn(L[k][src], ctx.dev) for k in ("n", "x_w", "view", "ess"))))


def run_shade(ctx, s, src, act, factor):
    """bits of the colour [N,3] and (factor) of the light factor [N, 1] of every row"""
    L = s["L"]
    a = [TT.Tn(L[k][src], ctx.dev) for k in ("x_c", "grad", "x_w", "view", "ess")]
    out = ctx.lib.shade(s["scene"], s["packed"], *a, 1, active=act, want_factor=factor)
    torch.cuda.synchronize()
    return bits(out[2]), (bits(out[3]).reshape(-1, 1) if factor else None)


MULTI_HW, MULTI_S = 64, 64


def run_multi(ctx):
    """bits of the colours [3, R, 3] of a small w4 frame under three lights in one pass (k_light16_multi)"""
    canon, faces, batch = full_frame(hw=MULTI_HW)
    r = renderer_with(TT.state(TT.SETS["w4"]), canon, faces, density_screen=False)
    r.eval()
    r._set_frame(batch)
    o, d = r._dev(batch["ray_o"][0]), r._dev(batch["ray_d"][0])
    n, f = r._dev(batch["near"][0]).clone(), r._dev(batch["far"][0]).clone()
    lights = five_lights()[1:4]          # a shifted light, a rotated one, both
    out = ctx.lib.render_rays_lights(r.scene, r.net.packed(r.device), ctx.lib.RenderWorkspace(r.device), o, d, n, f, MULTI_S,
                                     r._t_vals(MULTI_S), ctx.lib.light_records(lights, batch["Th"], r.device))
    torch.cuda.synchronize()
    return bits(out["color"])


def run_screen(ctx, s, src):
    sg, s1 = ctx.lib.screen_debug(s["scene"], s["packed"], TT.Tn(ctx.x[src], ctx.dev))
    torch.cuda.synchronize()
    return np.stack([bits(sg), bits(s1)], 1)


def run_density(ctx, s, repeat=1):
    """[repeat, GRID, GRID, GRID]: the grid's block `repeat` times along x"""
    ax = grid_axes(s["g"])
    ax[0] = np.tile(ax[0], repeat)
    return bits(ctx.lib.density_grid(s["scene"], s["packed"], ax)).reshape(repeat, GRID, GRID, GRID)


def record(ctx):
    """the fixture's arrays from the loaded library: the pool once, dense, in pool order"""
    out = {}
    ident = np.arange(TT.M)
    for tag in TAGS:
        s = ctx.set(tag)
        single, split, plist = run_field(ctx, s, TT.Tn(ctx.x, ctx.dev), None)
        positive = single[0].view(np.float32) > 0
        assert np.array_equal(np.sort(plist), np.nonzero(positive)[0])
        for k, a, b in zip(("sigma", "essence", "grad"), single, split):
            assert np.array_equal(b, a if k != "grad" else np.where(positive[:, None], a, 0)), (tag, k, "the two forms differ in the recording library")
            out["%s.field.%s" % (tag, k)] = a
        out["%s.light.colour" % tag] = run_light(ctx, s, ident)
        col, fac = run_shade(ctx, s, ident, None, True)
        assert np.array_equal(col, run_shade(ctx, s, ident, None, False)[0]), (tag, "k_light16<true> and <false> differ in the recording library")
        out["%s.shade.colour" % tag], out["%s.shade.factor" % tag] = col, fac
        out["%s.screen.sg_s1" % tag] = run_screen(ctx, s, ident)
        out["%s.density.sigma" % tag] = run_density(ctx, s)[0]
    out["w4.multi.colour"] = run_multi(ctx)
    return out


@pytest.fixture(scope="module")
def ctx():
    return TT.Ctx()


@pytest.fixture(scope="module")
def want():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def differ(a, b):
    return np.nonzero((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(1))[0]


@pytest.mark.parametrize("tag", TAGS)
def test_field_bits(ctx, want, tag):
    """k_field16 single launch, forward + reverse: sigma, essence, d sigma/dx bit for bit; the sigma > 0 list as a set"""
    s, G = ctx.set(tag), ctx.G
    problems = []
    for count in counts(G):
        for form, N, rows, src in TT.forms(count, 9000 + count % 997):
            at = "%s count %d" % (form, count)
            act = TT.active(ctx, N, rows) if form == "listed" else None
            single, split, plist = run_field(ctx, s, TT.Tn(ctx.x[src], ctx.dev), act)
            p = src[rows]
            pos = want["%s.field.sigma" % tag][p].view(np.float32) > 0
            for kind, got in (("single", single), ("split", split)):
                for k, a in zip(("sigma", "essence", "grad"), got):
                    rec = want["%s.field.%s" % (tag, k)][p]
                    if kind == "split" and k == "grad":
                        rec = np.where(pos[:, None], rec, 0)
                    bad = differ(a[rows], rec)
                    if len(bad):
                        problems.append((at, kind, k, "%d of %d rows differ from the recorded bits: %r" % (len(bad), count, TT.where(bad, src, rows, G))))
            positive = rows[pos]
            if not np.array_equal(np.sort(plist), np.sort(positive)):
                problems.append((at, "split", "pos", "the sigma > 0 list holds %d entries, the recorded sigma is positive on %d listed rows (or other rows)"
                                 % (len(plist), len(positive))))
    assert not problems, "\n".join(map(str, problems[:20]))


@pytest.mark.parametrize("tag", TAGS)
def test_light_bits(ctx, want, tag):
    """k_light16, dense: the colour bit for bit"""
    s, G = ctx.set(tag), ctx.G
    problems = []
    for count in counts(G):
        src = TT.src_for(count, 9500 + count % 997)
        bad = differ(run_light(ctx, s, src), want["%s.light.colour" % tag][src])
        if len(bad):
            problems.append(("dense count %d" % count, "%d slots differ from the recorded bits: %r" % (len(bad), TT.where(bad, src, np.arange(count), G))))
    assert not problems, "\n".join(map(str, problems[:20]))


@pytest.mark.parametrize("tag", TAGS)
def test_shade_bits(ctx, want, tag):
    """_lib.shade dense and through a shuffled list, with the factor output (k_light16<true>) and without (k_light16<false>): colour
    and factor bit for bit"""
    s, G = ctx.set(tag), ctx.G
    problems = []
    for count in counts(G):
        for form, N, rows, src in TT.forms(count, 9300 + count % 997):
            act = TT.active(ctx, N, rows) if form == "listed" else None
            for factor in (True, False):
                col, fac = run_shade(ctx, s, src, act, factor)
                for k, a in (("colour", col), ("factor", fac)):
                    if a is None:
                        continue
                    bad = differ(a[rows], want["%s.shade.%s" % (tag, k)][src[rows]])
                    if len(bad):
                        problems.append(("%s count %d" % (form, count), "factor output %s" % factor, k,
                                         "%d of %d rows differ from the recorded bits: %r" % (len(bad), count, TT.where(bad, src, rows, G))))
    assert not problems, "\n".join(map(str, problems[:20]))


def test_multi_light_bits(ctx, want):
    """k_light16_multi through _lib.render_rays_lights: every light's colours of the small frame bit for bit"""
    got, rec = run_multi(ctx), want["w4.multi.colour"]
    assert got.shape == rec.shape == (3, MULTI_HW * MULTI_HW, 3)
    assert all(np.count_nonzero(rec[k].any(1)) > 500 for k in range(3)) and not np.array_equal(rec[0], rec[1]), "the frame hits the body, the lights differ"
    bad = np.nonzero((got != rec).any(2))
    assert len(bad[0]) == 0, "%d (light, ray) pairs differ from the recorded bits, first %r" % (len(bad[0]), list(zip(*bad))[:6])


@pytest.mark.parametrize("tag", TAGS)
def test_screen_bits(ctx, want, tag, monkeypatch):
    """k_screen16<8> (DSN_SCREEN_WAVES unset), k_screen16<4> (4), k_screen16x2 (2), dense: estimate and term magnitude bit for bit"""
    s, G = ctx.set(tag), ctx.G
    problems = []
    for count in counts(G) + [2 * G * TT.T + 1]:
        src = TT.src_for(count, 9700 + count % 997)
        for waves in (None, "4", "2"):
            if waves is None:
                monkeypatch.delenv("DSN_SCREEN_WAVES", raising=False)
            else:
                monkeypatch.setenv("DSN_SCREEN_WAVES", waves)
            bad = differ(run_screen(ctx, s, src), want["%s.screen.sg_s1" % tag][src])
            if len(bad):
                problems.append(("dense count %d" % count, "DSN_SCREEN_WAVES=%s" % waves, "%d slots differ from the recorded bits: %r" % (len(bad), bad[:6].tolist())))
    monkeypatch.delenv("DSN_SCREEN_WAVES", raising=False)
    assert not problems, "\n".join(map(str, problems[:20]))


@pytest.mark.parametrize("tag", TAGS)
def test_density_only_bits(ctx, want, tag):
    """k_field16<density only> through dsn_density_grid: the volume bit for bit, the block repeated until a workgroup walks a second tile"""
    rec = want["%s.density.sigma" % tag]
    evaluated = int(np.count_nonzero(rec))          # (at least: a surviving point whose density is exactly 0 is not counted)
    assert evaluated > GRID, "the grid crosses the body"
    repeat = ctx.G * TT.T // evaluated + 2
    assert repeat * evaluated > ctx.G * TT.T
    got = run_density(ctx, ctx.set(tag), repeat)
    bad = [k for k in range(repeat) if not np.array_equal(got[k], rec)]
    assert not bad, "%d of %d copies of the block differ from the recorded bits (first copy %d: %d grid points)" % (
        len(bad), repeat, bad[0], int((got[bad[0]] != rec).sum()))
