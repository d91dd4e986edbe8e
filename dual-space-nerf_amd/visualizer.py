"""utils/visualizer.py Visualizer3D with its device-bound methods on gfx950 kernels: the density grid of get_grid_pred_batch
(Renderer.density_grid, dsn_density_grid) and the marching cubes of get_mesh_from_grid (dsn_mc_count / dsn_mc_emit, the rule of
include/dsnerf.h), and the preview image of render_mesh (dsn_raster_mesh: a deterministic rasteriser with the reference's camera and
spotlight, not a pixel copy of pyrender's GL output).  No skimage, trimesh or pyrender: meshes are returned as numpy (verts, faces);
connected=True (trimesh's component split) is not provided."""
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
    def get_grid_pred_batch(self, render, points=None, batch=None, chunk=100000):
        """numpy grid_pts [1, X, Y, Z, 3] and grid_pred [1, X, Y, Z, 1] as the reference returns them: the density volume of the grid
        over `points` (or the uniform grid) for `batch`'s posed body, with a frame code drawn as the reference draws it
        (torch.randperm(300)[:B]).  `chunk` is accepted and unused: the grid runs in device slabs."""
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
        _, vol = render.density_grid(batch, axes=tuple(grid["xyz"]), frame=int(code_idx[0]))
        X, Y, Z = (len(a) for a in grid["xyz"])
        grid_pred = vol.cpu().numpy().reshape(B, X, Y, Z, 1)
        grid_pts = grid["grid_pts"].reshape(B, X, Y, Z, 3).numpy()
        return grid_pts, grid_pred

    def get_mesh_from_grid(self, grid_pts, grid_pred):
        """(verts [V,3] float32, faces [T,3] int32) numpy arrays of the iso-surface at mc_value in the grid's coordinates, or None
        where the level is not crossed.  grid_pts / grid_pred: [X,Y,Z,3] / [X,Y,Z,1] (or with the leading B = 1)."""
        if self.connected:
            raise NotImplementedError("Visualizer3D(connected=True): the largest-component split (trimesh) is not provided")
        grid_pts = np.asarray(grid_pts)
        grid_pred = np.asarray(grid_pred)
        if grid_pts.ndim == 5:
            grid_pts, grid_pred = grid_pts[0], grid_pred[0]
        axes = (grid_pts[:, 0, 0, 0], grid_pts[0, :, 0, 1], grid_pts[0, 0, :, 2])
        vol = torch.from_numpy(np.ascontiguousarray(grid_pred.reshape(grid_pts.shape[:3]), dtype=np.float32)).cuda()
        verts, faces = _lib.marching_cubes(vol, axes, self.mc_value, self.gradient_direction)
        if faces.shape[0] == 0:
            return None
        return verts.cpu().numpy(), faces.cpu().numpy()

    @torch.no_grad()
    def render_mesh(self, mesh, camera_pose=None):
        """numpy uint8 [resolution_render, resolution_render, 3], as pyrender's `color` (utils/visualizer.py:144-168): the mesh under
        the reference's camera (yfov pi/3, aspect 1) and spotlight (intensity 30, cones pi/16 and pi/6) on a white background, by
        dsn_raster_mesh.  mesh: the (verts, faces) pair of get_mesh_from_grid or the {"verts", "faces"} dict of
        Renderer.extract_mesh, numpy or device.  camera_pose: a 4 x 4 camera-to-world matrix (default the reference's: 2.5 in front
        of the origin, looking down -z) - a real body is not at the origin; the light rides with the camera, as the reference adds
        both with one pose."""
        if mesh is None:
            raise ValueError("render_mesh: no mesh (get_mesh_from_grid returns None where the level is not crossed)")
        verts, faces = (mesh["verts"], mesh["faces"]) if isinstance(mesh, dict) else mesh

        def dev(a, dtype):
            a = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
            return a.to(device="cuda", dtype=dtype)
        out = _lib.raster_mesh(dev(verts, torch.float32), dev(faces, torch.int32), camera_pose=camera_pose,
                               height=self.resolution_render, width=self.resolution_render)
        return out["color"].cpu().numpy()
