"""utils/visualizer.py Visualizer3D with its device-bound methods on gfx950 kernels: the density grid of get_grid_pred_batch
(Renderer.density_grid, dsn_density_grid) and the marching cubes of get_mesh_from_grid (dsn_mc_count / dsn_mc_emit, the rule of
include/dsnerf.h), and the preview image of render_mesh (dsn_raster_mesh: a deterministic rasteriser with the reference's camera and
spotlight, not a pixel copy of pyrender's GL output).  No skimage, trimesh or pyrender: meshes are numpy (verts, faces) pairs or the
dicts of Renderer.extract_mesh, which may carry vertex normals (dsn_mc_normals, skimage's third output) and the field's albedo, normal
and lit colour at the vertices (Renderer.mesh_attributes); render_mesh shades them smooth and in colour (dsn_raster_mesh_attr) and
save_ply writes them to a file.  The largest connected component of a mesh (the reference's connected=True, by trimesh there) comes from
dsn_mesh_cc_label / dsn_mesh_cc_emit: get_mesh_from_grid(..., largest_component=True), Renderer.extract_mesh(..., largest_component=True)
or largest_component(mesh) below.  Components join through shared vertex INDICES (trimesh: shared edges - the same partition on a
marching-cubes mesh, not at the pinch vertices of an arbitrary one), the largest summed float32 area wins, ties go to the smaller
vertex index (include/dsnerf.h).  The constructor switch connected=True itself still raises NotImplementedError and names the keyword:
wiring it to the keyword is one line, held back while a pinned test expects the raise.
A mesh follows the body into other poses without a second extraction: Renderer.bind_mesh once, Renderer.pose_mesh per frame
(dsn_mesh_pose, the rule of include/dsnerf.h); render_mesh_sequence previews such a sequence and cull_stretched drops the triangles
a pose tore.  simplify_mesh (or simplify_cell= / target_vertices= of extract_mesh and get_mesh_from_grid) thins a mesh by vertex
clustering (dsn_mesh_simplify_count / dsn_mesh_simplify_emit, the rule of include/dsnerf.h): the vertices that stay are input vertices, so
every per-vertex array and a binding follow by one gather.  smooth_mesh (or smooth= of extract_mesh and get_mesh_from_grid) takes the
stair steps of the thresholded grid out with Taubin or Laplacian umbrella steps (dsn_mesh_smooth), and vertex_normals gives a mesh whose
vertices moved - smoothed, posed, loaded from a file - normals from its faces (dsn_mesh_vertex_normals); both by the rules of
include/dsnerf.h, in integer sums: the same bits every call.  mesh_distance says how far any of these tools moved the surface: the
exact nearest point on the other mesh for every vertex or surface sample (closest_point: dsn_mesh_dist_build / dsn_mesh_dist_query),
reduced on the device to mean, rms and maximum per direction, a Chamfer and a Hausdorff distance (dsn_mesh_dist_reduce); sample_surface
draws the area-weighted samples (dsn_mesh_sample_surface)."""
import numpy as np
import torch

from . import _lib


class Visualizer3D(object):
    """Visualizer3D of 3D implicit representations (same constructor as the reference)."""

    def __init__(self, resolution_mc, resolution_render, mc_value, gradient_direction, uniform_grid=False, connected=False,
                 verbose=False):
        super().__init__()
        self.resolution_mc = resolution_mc
        self.resolution_render = resolution_render
        self.mc_value = mc_value
        self.gradient_direction = gradient_direction
        self.uniform_grid = uniform_grid
        self.connected = connected
        self.verbose = verbose
        self.grid_info = None          # get_grid_pred_batch(coarse=...): that call's certificate; None after a dense call

    @staticmethod
    def _grid(axes, length, shortest):
        x, y, z = axes
        xx, yy, zz = torch.meshgrid(torch.tensor(x), torch.tensor(y), torch.tensor(z), indexing="ij")
        grid_points = torch.vstack([xx.flatten(), yy.flatten(), zz.flatten()]).T.float()
        return {"grid_pts": grid_points, "shortest_axis_length": length, "xyz": [x, y, z], "shortest_axis_index": shortest}

    def get_grid(self, points):
        from .can_render import Renderer
        axes = Renderer.grid_axes(points, self.resolution_mc)
        p = points.detach().reshape(-1, 3).float().cpu().numpy()
        s = int(np.argmin(p.max(axis=0) - p.min(axis=0)))          # (grid_axes' shortest axis)
        return self._grid(axes, np.max(axes[s]) - np.min(axes[s]), s)

    def get_grid_uniform(self):
        from .can_render import Renderer
        return self._grid(Renderer.grid_axes_uniform(self.resolution_mc), 2.4, 0)

    @torch.no_grad()
    def get_grid_pred_batch(self, render, points=None, batch=None, chunk=100000, coarse=None, dilate=1):
        """numpy grid_pts [1, X, Y, Z, 3] and grid_pred [1, X, Y, Z, 1] as the reference returns them: the density volume of the grid
        over `points` (or the uniform grid) for `batch`'s posed body, with a frame code drawn as the reference draws it
        (torch.randperm(300)[:B]).  `chunk` is accepted and unused: the grid runs in device slabs.
        coarse (2, 4, 8 or 16; default None: every point evaluated): the volume of Renderer.density_grid_hier at this visualizer's
        mc_value - densities only near that level's surface, elsewhere a coarse value of the same side, which get_mesh_from_grid
        turns into the same mesh wherever self.grid_info["leaks"] == 0 (no retry here: check it, or use Renderer.extract_mesh;
        self.grid_info is None after a dense call)."""
        if batch is None:
            raise ValueError("get_grid_pred_batch: needs the batch (the reference warps the grid with it)")
        if self.uniform_grid:
            grid = self.get_grid_uniform()
            B = 1
        else:
            grid = self.get_grid(points.reshape(-1, points.shape[-1]))
            B = points.shape[0]
        if B != 1:
            raise NotImplementedError("get_grid_pred_batch: one body per call (B = 1)")
        code_idx = torch.randperm(300)[:B]
        if self.verbose:
            print("Code_idx:", code_idx)
        if coarse is None:
            self.grid_info = None
            _, vol = render.density_grid(batch, axes=tuple(grid["xyz"]), frame=int(code_idx[0]))
        else:
            _, vol, self.grid_info = render.density_grid_hier(batch, level=self.mc_value, coarse=coarse, dilate=dilate,
                                                              axes=tuple(grid["xyz"]), frame=int(code_idx[0]))
        X, Y, Z = (len(a) for a in grid["xyz"])
        grid_pred = vol.cpu().numpy().reshape(B, X, Y, Z, 1)
        grid_pts = grid["grid_pts"].reshape(B, X, Y, Z, 3).numpy()
        return grid_pts, grid_pred

    def get_mesh_from_grid(self, grid_pts, grid_pred, return_normals=False, largest_component=False, simplify_cell=None,
                           target_vertices=None, smooth=None, report_distance=False):
        """(verts [V,3] float32, faces [T,3] int32) numpy arrays of the iso-surface at mc_value in the grid's coordinates, or None
        where the level is not crossed.  grid_pts / grid_pred: [X,Y,Z,3] / [X,Y,Z,1] (or with the leading B = 1).
        return_normals=True: a third array, the unit vertex normals [V,3] float32 (skimage's vertex_normals, by dsn_mc_normals).
        largest_component=True: only the connected component with the largest area (the reference's connected=True; the rule of
        include/dsnerf.h, on the device), the normals gathered with it.
        simplify_cell / target_vertices (one of them): the mesh thinned by simplify_mesh, after the component filter.
        smooth: an int (Taubin pairs) or a dict of smooth_mesh's keywords - the mesh smoothed by smooth_mesh after the component filter
        and before the thinning; the normals returned are then those of the smoothed faces.
        report_distance=True (with simplify_cell or target_vertices): one more element at the end of the tuple, the dict of
        mesh_distance(thinned mesh, the mesh before thinning) - how far the thinning moved the surface."""
        if self.connected:
            raise NotImplementedError("Visualizer3D(connected=True) is not wired up: pass largest_component=True to get_mesh_from_grid "
                                      "(or use dsnerf_amd.visualizer.largest_component) for the largest connected component")
        grid_pts = np.asarray(grid_pts)
        grid_pred = np.asarray(grid_pred)
        if grid_pts.ndim == 5:
            grid_pts, grid_pred = grid_pts[0], grid_pred[0]
        axes = (grid_pts[:, 0, 0, 0], grid_pts[0, :, 0, 1], grid_pts[0, 0, :, 2])
        vol = torch.from_numpy(np.ascontiguousarray(grid_pred.reshape(grid_pts.shape[:3]), dtype=np.float32)).cuda()
        out = _lib.marching_cubes(vol, axes, self.mc_value, self.gradient_direction, want_normals=bool(return_normals))
        if out[1].shape[0] == 0:
            return None
        if largest_component:
            v, f, src = _lib.largest_component(out[0], out[1], want_source=bool(return_normals))
            out = (v, f) + ((out[2][src.long()],) if return_normals else ())
        if smooth is not None:
            out = smooth_mesh(tuple(out), **smooth_keywords(smooth))
        report = None
        if report_distance and simplify_cell is None and target_vertices is None:
            raise ValueError("get_mesh_from_grid: report_distance needs simplify_cell or target_vertices")
        if simplify_cell is not None or target_vertices is not None:
            dense = tuple(out)
            out = simplify_mesh(dense, cell=simplify_cell, target_vertices=target_vertices)
            if report_distance:
                report = mesh_distance(out, dense)
        return tuple(a.cpu().numpy() for a in out) + ((report,) if report_distance else ())

    @torch.no_grad()
    def render_mesh(self, mesh, camera_pose=None, smooth=None, colors=None, lit=True):
        """numpy uint8 [resolution_render, resolution_render, 3], as pyrender's `color` (utils/visualizer.py:144-168): the mesh under
        the reference's camera (yfov pi/3, aspect 1) and spotlight (intensity 30, cones pi/16 and pi/6) on a white background, by
        dsn_raster_mesh.  mesh: the (verts, faces) pair of get_mesh_from_grid or the {"verts", "faces"} dict of
        Renderer.extract_mesh, numpy or device.  camera_pose: a 4 x 4 camera-to-world matrix (default the reference's: 2.5 in front
        of the origin, looking down -z) - a real body is not at the origin; the light rides with the camera, as the reference adds
        both with one pose.
        A (verts, faces, normals) triple or a dict with "normals" is shaded smooth (smooth=None: when normals are there; False: flat).
        colors: per-vertex colours [V,3] in [0, 1], or the key of the mesh dict that holds them ("albedo", "colour"); they take the
        grey's place under the spotlight, or with lit=False are painted as they are (dsn_raster_mesh_attr).  A plain (verts, faces)
        pair renders as it always did."""
        if mesh is None:
            raise ValueError("render_mesh: no mesh (get_mesh_from_grid returns None where the level is not crossed)")
        if isinstance(mesh, dict):
            verts, faces, normals = mesh["verts"], mesh["faces"], mesh.get("normals")
        else:
            verts, faces, normals = (tuple(mesh) + (None,))[:3]
        if isinstance(colors, str):
            if not isinstance(mesh, dict) or colors not in mesh:
                raise ValueError(f"render_mesh: the mesh has no {colors!r}")
            colors = mesh[colors]
        if smooth and normals is None:
            raise ValueError("render_mesh: smooth=True needs a mesh with normals")
        smooth = normals is not None if smooth is None else bool(smooth)

        def dev(a, dtype):
            a = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
            return a.to(device="cuda", dtype=dtype)
        kw = {}
        if smooth or colors is not None or not lit:
            kw = dict(vertex_normals=dev(normals, torch.float32) if smooth else None,
                      vertex_colors=None if colors is None else dev(colors, torch.float32), smooth=smooth, lit=bool(lit))
        out = _lib.raster_mesh(dev(verts, torch.float32), dev(faces, torch.int32), camera_pose=camera_pose,
                               height=self.resolution_render, width=self.resolution_render, **kw)
        return out["color"].cpu().numpy()

    @torch.no_grad()
    def render_mesh_sequence(self, render, binding, targets, camera_pose=None, chunk=8, max_stretch=None, **render_mesh_kw):
        """The preview of a bound mesh (Renderer.bind_mesh) under a sequence of poses - novel_pose_vis.py's animation, for the mesh:
        numpy uint8 [P, resolution_render, resolution_render, 3].  `targets` as Renderer.pose_mesh takes them (a [Vb,3] body or
        "canonical": P = 1); `chunk` poses are carried at a time (dsn_mesh_pose) and each is rasterised by render_mesh with
        `camera_pose` and render_mesh's keywords (colors may name a per-vertex entry of the binding: "albedo", "colour"), so device
        memory is bounded by the chunk, not by P.  max_stretch: triangles stretched beyond that ratio are dropped per frame
        (cull_stretched)."""
        if isinstance(targets, str):
            if targets != "canonical":
                raise ValueError(f"render_mesh_sequence: unknown target {targets!r} (\"canonical\")")
            targets = torch.as_tensor(render.canonical_vertex).reshape(1, -1, 3)
        elif not isinstance(targets, (list, tuple)) and np.ndim(targets) == 2:
            targets = targets[None]
        P = len(targets)
        chunk = max(int(chunk), 1)
        frames = np.empty((P, self.resolution_render, self.resolution_render, 3), np.uint8)
        for p0 in range(0, P, chunk):
            posed = render.pose_mesh(binding, targets[p0:p0 + chunk], stretch=max_stretch is not None)
            for k in range(posed["verts"].shape[0]):
                mesh = dict(binding, verts=posed["verts"][k])
                if posed["normals"] is not None:
                    mesh["normals"] = posed["normals"][k]
                if max_stretch is not None:
                    mesh = cull_stretched(mesh, posed["stretch"][k], max_stretch)
                frames[p0 + k] = self.render_mesh(mesh, camera_pose=camera_pose, **render_mesh_kw)
        return frames


PER_VERTEX_KEYS = ("normals", "albedo", "normal", "colour", "sigma", "valid")


@torch.no_grad()
def largest_component(mesh):
    """The connected component of a mesh with the largest area (dsn_mesh_cc_label / dsn_mesh_cc_emit, the rule of include/dsnerf.h).
    mesh: a (verts, faces[, normals]) tuple or the dict of Renderer.extract_mesh, numpy or device; the result has the same form and
    lives where verts lived.  Every per-vertex array the dict carries (normals, albedo, normal, colour - also in its [K,V,3] form -,
    sigma, valid) is gathered through the kept vertices; the dict gains "source_vertex" [V'] int32 (each kept vertex's index in the
    mesh given) and "n_components".  Other keys are carried over as they are."""
    is_dict = isinstance(mesh, dict)
    if is_dict:
        verts, faces = mesh["verts"], mesh["faces"]
    else:
        verts, faces = mesh[0], mesh[1]
    on_host = not torch.is_tensor(verts)

    def dev(a, dtype=None):
        a = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        return a.to(device="cuda", dtype=dtype)

    def back(a):
        return a.cpu().numpy() if on_host else a
    info = {}
    v, f, src = _lib.largest_component(dev(verts, torch.float32), dev(faces, torch.int32), info=info)
    idx = src.long()

    def gather(a):
        a = dev(a)
        return a[:, idx] if a.dim() == 3 else a[idx]
    if not is_dict:
        return (back(v), back(f)) + tuple(back(gather(a)) for a in tuple(mesh)[2:3])
    out = dict(mesh)
    out.update(verts=back(v), faces=back(f), source_vertex=back(src), n_components=info["n_components"])
    for k in PER_VERTEX_KEYS:
        if out.get(k) is not None:
            out[k] = back(gather(out[k]))
    return out


BINDING_KEYS = ("face_idx", "uv", "h", "cov", "x_c")          # Renderer.bind_mesh's per-vertex entries ("valid" is in PER_VERTEX_KEYS)


@torch.no_grad()
def simplify_mesh(mesh, cell=None, target_vertices=None):
    """A mesh thinned by vertex clustering (dsn_mesh_simplify_count / dsn_mesh_simplify_emit, the rule of include/dsnerf.h): the
    vertices of every grid cell of edge `cell` (the grid starts at the minimum of the finite vertices) collapse to the one of them
    nearest to their mean, faces that lose an edge and duplicates go.  The vertices that stay are input vertices, bit for bit.
    mesh: a (verts, faces[, normals]) tuple or the dict of Renderer.extract_mesh / Renderer.bind_mesh, numpy or device; the result
    has the same form and lives where verts lived.  Every per-vertex array the dict carries - largest_component's (normals, albedo,
    normal, colour - also in its [K,V,3] form -, sigma, valid), the entries of a binding (face_idx, uv, h, cov, x_c) and
    source_vertex - is gathered through "cluster_source" [V'] int32 (each output vertex's index in the mesh given), so a simplified
    binding poses with Renderer.pose_mesh as it is; the dict also gains "vertex_cluster" [V] int32 (the output vertex every input
    vertex went to; -1: not finite) and "simplify_info" (the counts of _lib.MESH_SIMPLIFY_COUNTS, cell, origin, g, and for a target
    n and the probes).  Other keys are carried over as they are.
    target_vertices=N instead of cell: the cell is float32(extent / n) (1 + 2^-20) for n cells along the longest finite extent, with
    the largest n in [1, 4096] whose vertex count K(n) <= N found by bisection on the counting-only call (at most 12 probes, one
    8-byte host read each).  K(n) is treated as monotone, which it is not strictly: the result has at most N vertices, not
    necessarily as many as some other n would give.  Giving both or neither raises ValueError.  Clustering can pinch the surface;
    no manifold repair is attempted."""
    if (cell is None) == (target_vertices is None):
        raise ValueError("simplify_mesh: give one of cell and target_vertices")
    is_dict = isinstance(mesh, dict)
    if is_dict:
        verts, faces = mesh["verts"], mesh["faces"]
    else:
        verts, faces = mesh[0], mesh[1]
    on_host = not torch.is_tensor(verts)

    def dev(a, dtype=None):
        a = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        return a.to(device="cuda", dtype=dtype)

    def back(a):
        return a.cpu().numpy() if on_host else a
    dv, df = dev(verts, torch.float32).reshape(-1, 3), dev(faces, torch.int32)
    info = {}
    if target_vertices is not None:
        cell = _lib.mesh_target_search(dv, target_vertices, info=info)
    v, f, src, vc = _lib.mesh_simplify(dv, df, cell, info=info)
    idx = src.long()
    V = dv.shape[0]

    def gather(a):
        a = dev(a)
        return a[:, idx] if (a.dim() == 3 and a.shape[1] == V) else a[idx]
    if not is_dict:
        return (back(v), back(f)) + tuple(back(gather(a)) for a in tuple(mesh)[2:3])
    out = dict(mesh)
    for k in PER_VERTEX_KEYS + BINDING_KEYS + ("source_vertex",):
        if out.get(k) is not None:
            out[k] = back(gather(out[k]))
    out.update(verts=back(v), faces=back(f), cluster_source=back(src), vertex_cluster=back(vc), simplify_info=info)
    return out


def smooth_keywords(smooth):
    """smooth= of Renderer.extract_mesh / get_mesh_from_grid as smooth_mesh's keywords: an int is the number of Taubin pairs"""
    if isinstance(smooth, dict):
        return dict(smooth)
    if isinstance(smooth, bool) or not isinstance(smooth, (int, np.integer)):
        raise ValueError(f"smooth: an int (Taubin pairs) or a dict of smooth_mesh's keywords, got {smooth!r}")
    return {"iterations": int(smooth)}


def _mesh_parts(mesh):
    if isinstance(mesh, dict):
        return mesh["verts"], mesh["faces"], mesh.get("normals")
    return (tuple(mesh) + (None,))[:3]


def _to_device(a, dtype=None):
    a = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return a.to(device="cuda", dtype=dtype)


@torch.no_grad()
def vertex_normals(mesh):
    """Unit vertex normals [V,3] float32 from the faces of a mesh (dsn_mesh_vertex_normals, the rule of include/dsnerf.h): area-weighted,
    oriented by the winding, (0, 0, 0) at a vertex no face with finite corners uses.  For a mesh whose vertices moved since marching
    cubes gave it normals - smoothed, posed - or that never had any: mesh["normals"] = vertex_normals(mesh) and render_mesh shades it
    smooth.  mesh: a (verts, faces[, ...]) tuple or a dict with "verts" and "faces", numpy or device; the result lives where verts
    lived."""
    verts, faces, _ = _mesh_parts(mesh)
    n = _lib.mesh_vertex_normals(_to_device(verts, torch.float32).reshape(-1, 3), _to_device(faces, torch.int32))
    return n if torch.is_tensor(verts) else n.cpu().numpy()


@torch.no_grad()
def smooth_mesh(mesh, iterations=10, lamb=0.5, mu=-0.53, normals=None):
    """A mesh smoothed by umbrella steps on the device (dsn_mesh_smooth, the rule of include/dsnerf.h): every vertex moves by a factor
    times the mean offset of its neighbours, every face giving each corner its two others (on a closed surface trimesh's uniform
    filter_laplacian weights; a boundary edge counts once).  `iterations` Taubin pairs of a lambda step and a mu step (mu < -lambda < 0:
    the second step undoes the shrinkage of the first), or with mu=None `iterations` plain lambda steps, which shrink.  Faces, vertex
    count and order do not change; vertices no face with finite, distinct corners uses stay bit for bit.
    mesh: a (verts, faces[, normals]) tuple or the dict of Renderer.extract_mesh, numpy or device; the result has the same form and
    lives where verts lived.  normals=None: a mesh that carries normals gets them recomputed from the smoothed faces (vertex_normals:
    marching cubes' normals describe the surface before); True: computed in any case; False: none, stale ones are dropped.
    The entries of a binding (face_idx, uv, h, cov, x_c) are DROPPED - they describe the old positions: bind after smoothing.  Other
    per-vertex arrays (albedo, colour, source_vertex, ...) and keys are carried over as they are; the field's attributes are not
    evaluated again at the moved vertices (Renderer.extract_mesh(smooth=...) evaluates them after smoothing).  The dict gains
    "smooth_info": the counts of _lib.MESH_SMOOTH_COUNTS, origin, scale_exp and the factors."""
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError("smooth_mesh: iterations must be >= 0")
    factors = [float(lamb)] * iterations if mu is None else [float(lamb), float(mu)] * iterations
    if len(factors) > _lib.MESH_SMOOTH_MAX_STEPS:
        raise ValueError(f"smooth_mesh: {len(factors)} steps, more than {_lib.MESH_SMOOTH_MAX_STEPS}")
    is_dict = isinstance(mesh, dict)
    verts, faces, had = _mesh_parts(mesh)
    on_host = not torch.is_tensor(verts)

    def back(a):
        return a.cpu().numpy() if on_host else a
    dv, df = _to_device(verts, torch.float32).reshape(-1, 3), _to_device(faces, torch.int32)
    info = {}
    v = _lib.mesh_smooth(dv, df, factors, info=info)
    want = had is not None if normals is None else bool(normals)
    n = _lib.mesh_vertex_normals(v, df) if want else None
    if not is_dict:
        return (back(v), faces) + ((back(n),) if want else ())
    out = {k: a for k, a in mesh.items() if k not in BINDING_KEYS and k != "normals"}
    out.update(verts=back(v), smooth_info=info)
    if want:
        out["normals"] = back(n)
    return out


@torch.no_grad()
def closest_point(mesh, points):
    """The nearest point of a mesh for every row of `points` [n,3], exactly (dsn_mesh_dist_build / dsn_mesh_dist_query, the rule of
    include/dsnerf.h: the minimum over all faces of the float32 point-to-triangle distance, ties to the lowest face index) - what
    trimesh.proximity.closest_point answers on the host.  mesh: a (verts, faces[, ...]) tuple or a dict with "verts" and "faces", numpy
    or device.  Returns device tensors {"distance" [n] float32, "face" [n] int32, "point" [n,3] float32}; a point that is not finite
    gives NaN, -1, NaN.  A mesh without a valid face raises ValueError."""
    verts, faces, _ = _mesh_parts(mesh)
    index = _lib.mesh_dist_build(_to_device(verts, torch.float32).reshape(-1, 3), _to_device(faces, torch.int32))
    out = _lib.mesh_dist_query(index, _to_device(points, torch.float32).reshape(-1, 3))
    return {"distance": torch.sqrt(out["dist2"]), "face": out["face"], "point": out["point"]}


@torch.no_grad()
def sample_surface(mesh, n, seed=0):
    """`n` points on the surface of a mesh, area-weighted (dsn_mesh_sample_surface, the rule of include/dsnerf.h): sample i depends on
    (seed, i) and the mesh only, so the first k of a larger draw are the smaller draw.  mesh as closest_point takes it.  Returns device
    tensors {"points" [n,3] float32, "face" [n] int32}."""
    verts, faces, _ = _mesh_parts(mesh)
    pts, face = _lib.mesh_sample_surface(_to_device(verts, torch.float32).reshape(-1, 3), _to_device(faces, torch.int32), n, seed)
    return {"points": pts, "face": face}


def _direction_stats(words):
    count, _, sum_d, sum_d2, max_d, arg = (float(x) for x in words)
    nan = float("nan")
    return {"mean": sum_d / count if count else nan, "rms": (sum_d2 / count) ** 0.5 if count else nan, "max": max_d if count else nan,
            "argmax": arg, "count": count}


@torch.no_grad()
def mesh_distance(a, b, samples="vertices", seed=0, symmetric=True, return_distances=False):
    """How far is mesh `a` from mesh `b`?  Points of a (samples="vertices": its vertices; an int: that many area-weighted surface
    samples, sample_surface(a, samples, seed) - the right choice after simplification, where vertices are sparse on flat parts) are
    measured against the surface of b by closest_point's exact search, and with symmetric=True points of b against a.  Returns a dict
    of Python floats, all from one small device->host copy: per direction ("a_to_b", and "b_to_a" when symmetric) "mean", "rms", "max",
    "argmax" (the index of the farthest query point, the lowest on ties) and "count" (points measured; points that are not finite are
    left out), and over the directions measured "chamfer" (the mean of the directional means) and "hausdorff" (the largest maximum).
    The sums are float64 in a fixed order (dsn_mesh_dist_reduce): the same call returns the same bits.
    return_distances=True adds per direction "distance" [n] float32 and "points" [n,3] (the query points) as device tensors.
    a, b: (verts, faces[, ...]) tuples or dicts with "verts" and "faces", numpy or device."""
    if not (isinstance(samples, str) and samples == "vertices") and (isinstance(samples, bool) or not isinstance(samples, (int, np.integer))):
        raise ValueError(f"mesh_distance: samples must be \"vertices\" or an int, got {samples!r}")
    if not isinstance(samples, str) and int(samples) < 0:
        raise ValueError("mesh_distance: samples must be >= 0")
    meshes = []
    for m in (a, b):
        verts, faces, _ = _mesh_parts(m)
        meshes.append((_to_device(verts, torch.float32).reshape(-1, 3).contiguous(), _to_device(faces, torch.int32).reshape(-1, 3).contiguous()))
    directions = [("a_to_b", 0, 1)] + ([("b_to_a", 1, 0)] if symmetric else [])
    words, extra = [], {}
    for name, src, dst in directions:
        if isinstance(samples, str):
            pts = meshes[src][0]
        else:
            pts = _lib.mesh_sample_surface(meshes[src][0], meshes[src][1], int(samples), seed, want_face=False)[0]
        index = _lib.mesh_dist_build(meshes[dst][0], meshes[dst][1], check=False)
        d2 = _lib.mesh_dist_query(index, pts, want_face=False, want_point=False)["dist2"]
        words.append(torch.cat([_lib.mesh_dist_reduce(d2), index["counts"].double()]))
        if return_distances:
            extra[name] = {"distance": torch.sqrt(d2), "points": pts}
    host = torch.stack(words).cpu().numpy()              # the one device->host copy: 10 float64 per direction
    out = {}
    for k, (name, _, dst) in enumerate(directions):
        if host[k, 6] == 0:
            raise ValueError(f"mesh_distance: mesh {'ab'[dst]} has no valid face (indices in range, finite vertices)")
        out[name] = _direction_stats(host[k, :6])
        if return_distances:
            out[name].update(extra[name])
    out["chamfer"] = float(np.mean([out[name]["mean"] for name, _, _ in directions]))
    out["hausdorff"] = float(np.max([out[name]["max"] for name, _, _ in directions]))
    return out


def cull_stretched(mesh, stretch, max_ratio=2.0):
    """The mesh without the triangles a pose tore: faces[stretch <= max_ratio], with `stretch` [T] of Renderer.pose_mesh(...,
    stretch=True) for that pose (NaN and +inf are dropped too).  mesh: a dict with "faces" (the other entries are carried over; the
    vertices are kept, so per-vertex arrays stay valid) or a (verts, faces[, normals]) tuple; numpy or device.  2.0 is a default,
    not a claim: the ratio that separates a fold from a tear depends on the motion."""
    faces = mesh["faces"] if isinstance(mesh, dict) else mesh[1]
    keep = torch.as_tensor(stretch).reshape(-1) <= max_ratio
    if keep.shape[0] != faces.shape[0]:
        raise ValueError(f"cull_stretched: {keep.shape[0]} stretch values for {faces.shape[0]} faces")
    kept = faces[keep.to(faces.device)] if torch.is_tensor(faces) else np.asarray(faces)[keep.cpu().numpy()]
    if isinstance(mesh, dict):
        return dict(mesh, faces=kept)
    return (mesh[0], kept) + tuple(mesh[2:])


def save_ply(path, mesh, colors=None):
    """Write a mesh as binary little-endian PLY (numpy only): float x y z per vertex, float nx ny nz where the mesh has normals, uchar
    red green blue where colours are given, and the faces as `uchar 3` + three int32.  mesh: a (verts, faces[, normals]) tuple or the
    dict of Renderer.extract_mesh, numpy or device; colors: [V,3] floats (clamped to [0, 1], NaN as 0, level floor(c 255 + 0.5)) or the
    key of the mesh dict that holds them ("albedo", "colour")."""
    def host(a, dtype):
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        return np.ascontiguousarray(a, dtype=dtype)
    if isinstance(mesh, dict):
        verts, faces, normals = mesh["verts"], mesh["faces"], mesh.get("normals")
    else:
        verts, faces, normals = (tuple(mesh) + (None,))[:3]
    if isinstance(colors, str):
        if not isinstance(mesh, dict) or colors not in mesh:
            raise ValueError(f"save_ply: the mesh has no {colors!r}")
        colors = mesh[colors]
    verts, faces = host(verts, "<f4").reshape(-1, 3), host(faces, "<i4").reshape(-1, 3)
    V, T = verts.shape[0], faces.shape[0]
    fields, cols = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")], [verts]
    if normals is not None:
        normals = host(normals, "<f4").reshape(-1, 3)
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        cols.append(normals)
    if colors is not None:
        c = host(colors, np.float64).reshape(-1, 3)
        c = np.where(c > 0, c, 0.0)                    # (NaN: 0)
        colors = np.floor(np.where(c < 1, c, 1.0) * 255.0 + 0.5).astype(np.uint8)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        cols.append(colors)
    if any(a.shape != (V, 3) for a in cols):
        raise ValueError("save_ply: normals and colours need one row per vertex")
    vrec = np.empty(V, dtype=fields)
    for k, (name, _) in enumerate(fields):
        vrec[name] = cols[k // 3][:, k % 3]
    frec = np.empty(T, dtype=[("n", "u1"), ("v", "<i4", (3,))])
    frec["n"], frec["v"] = 3, faces
    ply_type = {"<f4": "float", "u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {V}"]
    header += [f"property {ply_type[t]} {name}" for name, t in fields]
    header += [f"element face {T}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())
