"""Generate tests/golden/maps_light.npz from the REAL reference: the light factor of every sample of every eval case.

Run in the build container only (needs the reference, see oracle/ref_harness.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_maps.py

The golden cases hold the reference's essence, n_w, colour, weights, sigma and transparent per sample; what the decomposition maps
(dsn_render_rays_maps) need beside them is the reference's own light factor L = ELU(lights_encoding) + 1 (model/spacenet.py:174-188),
which the reference only ever multiplies into the essence.  For every eval case the case is rebuilt from the inputs stored in its
.npz (the same Renderer, parameters, light tweak and batch as make_golden.py), run through oracle/ref_harness.run_stages - whose
regenerated colour and n_w must be bit-identical to the committed case - with a forward pre-hook on net.lighting_mlp that captures the
module's inputs during net(...); the module is then called again on those inputs with essence = 1, which returns L itself.

    maps_light.npz:  "light:<case>"  [N] float32  (N = R S samples, the case's sample order)

Data only: no reference source is stored.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import ref_harness as rh  # noqa: E402
from helpers import ALL_CASES, load, state  # noqa: E402

EVAL_CASES = [c for c in ALL_CASES if "train" not in c]


def light_of(name):
    import torch

    g = load(name)
    S = int(g["S"])
    render = rh.build_reference(g["canonical_vertex"], g["faces"], state(name), S)
    if name == "small_novel":                  # make_golden.py: novel()
        render.net.set_light_center(torch.from_numpy(g["light_center"]))
        render.net.nerf.w = 0
    if name == "small_rot":                    # make_golden.py: rotl()
        render.net.set_rot_center(torch.from_numpy(g["rot_center"]))
        render.net.set_rot(torch.from_numpy(g["rot"]))
    rays = {k: g[k] for k in ("ray_o", "ray_d", "near", "far")}
    batch = rh.make_batch(rays, g["xyz"], g["poses"], g["Th"], int(g["frame"]))
    seen = []
    hook = render.net.lighting_mlp.register_forward_pre_hook(lambda mod, args: seen.append([a.detach().clone() for a in args]))
    out = rh.run_stages(render, batch, train=False)
    hook.remove()
    assert len(seen) == 1, (name, len(seen))
    for k in ("colour", "n_w", "essence", "weights", "sigma"):
        assert np.array_equal(out[k], g[k], equal_nan=True), f"{name}: regenerated {k} differs from the committed case"
    normal, xyz_world, view_dir, essence = seen[0]
    with torch.no_grad():
        L = render.net.lighting_mlp(normal, xyz_world, view_dir, torch.ones_like(essence))
    L = L.numpy().astype(np.float32)
    assert L.shape == essence.shape and np.array_equal(L[:, 0], L[:, 1]) and np.array_equal(L[:, 0], L[:, 2])
    L = np.ascontiguousarray(L[:, 0])
    # the factor times the case's essence is the case's colour (to float32 rounding: the module computed w * essence in one product)
    err = np.abs(L[:, None].astype(np.float64) * g["essence"] - g["colour"]).max()
    bar = 2.0 ** -22 * max(1.0, float(np.abs(g["colour"]).max()))
    assert err <= bar, (name, err, bar)
    print(f"{name}: N = {L.size}, L in [{L.min():.4g}, {L.max():.4g}], max |L e - colour| = {err:.2e}")
    return L


def main():
    import torch

    torch.set_num_threads(8)
    arrs = {"light:" + c: light_of(c) for c in EVAL_CASES}
    path = os.path.join(HERE, "maps_light.npz")
    np.savez_compressed(path, **arrs)
    print(f"maps_light: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrs)} arrays, {sum(a.size for a in arrs.values())} floats")


if __name__ == "__main__":
    main()
