"""TileTree (src/terrain_data/tile_tree.rs:103-387) + GpuTileTree (gpu_tile_tree.rs:22-95) behind the reference's
names: `TileTree.new(tile_atlas, view_config)`, `compute_requests` / `update`, `adjust_to_tile_atlas`,
`approximate_height`, and the free functions `sample_attachment` / `sample_height` (terrain_data/mod.rs:265-307).
The node tables live on the GPU; this module is a thin ctypes mirror used by the tests."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _ffi
from .terrain import TerrainModel, TerrainViewConfig, TileCoordinate
from .tile_atlas import TileAtlas, device_open


def model_c(model: TerrainModel) -> _ffi.TerrainModelC:
    m = _ffi.TerrainModelC()
    m.kind = {"planar": 0, "spherical": 1, "ellipsoidal": 2}[model.kind]
    for i in range(3):
        m.position[i] = model.translation[i]
    if model.kind == "planar":
        m.a = model.side_length
    elif model.kind == "spherical":
        m.a = model.radius
    else:
        m.a, m.b = model.major_axis, model.minor_axis
    m.min_height, m.max_height = model.min_height, model.max_height
    return m


def view_config_c(vc: TerrainViewConfig) -> _ffi.TerrainViewConfigC:
    c = _ffi.TerrainViewConfigC()
    for name in ("tree_size", "geometry_tile_count", "refinement_count", "grid_size", "subdivision_tolerance",
                 "precision_threshold_distance", "load_distance", "morph_distance", "blend_distance", "morph_range",
                 "blend_range", "origin_lod"):
        setattr(c, name, getattr(vc, name))
    return c


def view_state_from_config(model: TerrainModel, view_config: TerrainViewConfig, view_world_position: Sequence[float],
                           approximate_height: float) -> _ffi.ViewStateC:
    """bt_view_state_from_config: the prepass' per-frame inputs derived in the library (f64, `as f32` casts)."""
    v = _ffi.ViewStateC()
    pos = (C.c_double * 3)(*view_world_position)
    _ffi.check(_ffi.lib().bt_view_state_from_config(C.byref(model_c(model)), C.byref(view_config_c(view_config)), pos,
                                                    C.c_float(approximate_height), C.byref(v)))
    return v


def model_approximation_from_config(model: TerrainModel, view_config: TerrainViewConfig, view_world_position: Sequence[float]) -> _ffi.ModelApproximationC:
    """bt_model_approximation_from_config: the Taylor coefficients of the high-precision geometry (TerrainModelApproximation::compute) for a
    view position, f64 in the library, `as f32` at the end; derive the view (view_state_from_config) from the same position."""
    a = _ffi.ModelApproximationC()
    pos = (C.c_double * 3)(*view_world_position)
    _ffi.check(_ffi.lib().bt_model_approximation_from_config(C.byref(model_c(model)), C.byref(view_config_c(view_config)), pos, C.byref(a)))
    return a


# numpy mirrors of bt_ray / bt_ray_hit (include/bevy_terrain_amd.h)
RAY_DTYPE = np.dtype([("origin", np.float64, 3), ("direction", np.float64, 3), ("t_min", np.float64), ("t_max", np.float64)])
RAY_HIT_DTYPE = np.dtype([("status", np.uint32), ("step", np.uint32), ("t", np.float64), ("t_above", np.float64), ("position", np.float64, 3),
                          ("height", np.float32), ("_padding", np.uint32)])

# numpy mirrors of bt_sphere / bt_sphere_contact / bt_sphere_sweep / bt_sweep_hit
SPHERE_DTYPE = np.dtype([("center", np.float64, 3), ("radius", np.float64)])
SPHERE_CONTACT_DTYPE = np.dtype([("status", np.uint32), ("candidate", np.uint32), ("distance", np.float64), ("depth", np.float64), ("point", np.float64, 3),
                                 ("normal", np.float64, 3), ("height", np.float32), ("_padding", np.uint32)])
SPHERE_SWEEP_DTYPE = np.dtype([("origin", np.float64, 3), ("direction", np.float64, 3), ("radius", np.float64), ("t_min", np.float64), ("t_max", np.float64)])
SWEEP_HIT_DTYPE = np.dtype([("status", np.uint32), ("step", np.uint32), ("t", np.float64), ("t_above", np.float64), ("contact", SPHERE_CONTACT_DTYPE)])


class RenderCamera:
    """bt_render_camera (include/bevy_terrain_amd.h): the camera of TileTree.render.  origin, forward, right and up are used as given (f64):
    pixel (x, y) looks along forward + sx * right + sy * up (perspective) or starts at origin + sx * right + sy * up and looks along
    forward (orthographic), sx, sy in (-1, 1) at the pixel centres, y down.  Build one with perspective() or orthographic()."""

    def __init__(self, origin, forward, right, up, width: int, height: int, t_min: float, t_max: float, *, orthographic: bool = False,
                 lighting: bool = False, albedo_attachment: Optional[int] = None, sun=(0.0, 1.0, 0.0), ambient: float = 0.25, background=(0, 0, 0, 0)):
        self.origin, self.forward, self.right, self.up = (np.array(v, dtype=np.float64).reshape(3) for v in (origin, forward, right, up))
        self.width, self.height, self.t_min, self.t_max = int(width), int(height), float(t_min), float(t_max)
        self.orthographic, self.lighting, self.albedo_attachment = bool(orthographic), bool(lighting), albedo_attachment
        self.sun, self.ambient, self.background = tuple(float(v) for v in sun), float(ambient), tuple(int(v) for v in background)

    @staticmethod
    def _frame(forward, up):
        f = np.asarray(forward, dtype=np.float64)
        f = f / np.linalg.norm(f)
        r = np.cross(f, np.asarray(up, dtype=np.float64))
        r = r / np.linalg.norm(r)
        return f, r, np.cross(r, f)

    @staticmethod
    def perspective(position, forward, up, fov_y: float, width: int, height: int, t_min: float, t_max: float, **kw) -> "RenderCamera":
        """a pinhole camera at `position` looking along `forward` (normalised here) with `up` roughly up and a vertical field of view of
        fov_y radians; t is then linear view depth"""
        f, r, u = RenderCamera._frame(forward, up)
        tan = np.tan(0.5 * float(fov_y))
        return RenderCamera(position, f, r * (tan * (float(width) / float(height))), u * tan, width, height, t_min, t_max, **kw)

    @staticmethod
    def orthographic(position, forward, up, half_width: float, half_height: float, width: int, height: int, t_min: float, t_max: float, **kw) -> "RenderCamera":
        """parallel rays along `forward` (normalised here) from a window of 2 half_width x 2 half_height world units centred on `position`"""
        f, r, u = RenderCamera._frame(forward, up)
        return RenderCamera(position, f, r * float(half_width), u * float(half_height), width, height, t_min, t_max, orthographic=True, **kw)

    def c(self) -> _ffi.RenderCameraC:
        cam = _ffi.RenderCameraC()
        for i in range(3):
            cam.origin[i], cam.forward[i], cam.right[i], cam.up[i], cam.sun[i] = self.origin[i], self.forward[i], self.right[i], self.up[i], self.sun[i]
        cam.t_min, cam.t_max, cam.width, cam.height = self.t_min, self.t_max, self.width, self.height
        cam.flags = (_ffi.RENDER_ORTHOGRAPHIC if self.orthographic else 0) | (_ffi.RENDER_LIGHTING if self.lighting else 0)
        cam.albedo_attachment = _ffi.RENDER_NO_ALBEDO if self.albedo_attachment is None else self.albedo_attachment
        cam.ambient = self.ambient
        for i in range(4):
            cam.background[i] = self.background[i]
        return cam


def render_rays(camera: RenderCamera) -> Tuple[np.ndarray, np.ndarray]:
    """PIXEL RAY of include/bevy_terrain_amd.h for every pixel of a camera, row-major, y down: (origins, directions), each
    (height * width, 3) float64, operation by operation as the kernel computes them; march them from camera.t_min to camera.t_max"""
    w, h = camera.width, camera.height
    x, y = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
    sx = np.tile((2.0 * (x + 0.5)) / np.float64(w) - 1.0, h)
    sy = np.repeat(1.0 - (2.0 * (y + 0.5)) / np.float64(h), w)
    with np.errstate(all="ignore"):
        base, other = (camera.origin, camera.forward) if camera.orthographic else (camera.forward, camera.origin)
        moved = (base[None, :] + sx[:, None] * camera.right[None, :]) + sy[:, None] * camera.up[None, :]
    fixed = np.tile(other, (w * h, 1))
    return (moved, fixed) if camera.orthographic else (fixed, moved)


def write_ppm(path: str, rgba: np.ndarray):
    """an (height, width, 3 or 4) uint8 image (TileTree.render's "rgba" plane) as a binary PPM (P6; alpha is dropped): no library needed"""
    rgba = np.asarray(rgba)
    if rgba.dtype != np.uint8 or rgba.ndim != 3 or rgba.shape[2] not in (3, 4):
        raise ValueError("write_ppm wants an (height, width, 3 or 4) uint8 array")
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgba.shape[1], rgba.shape[0]))
        f.write(np.ascontiguousarray(rgba[:, :, :3]).tobytes())


# numpy mirror of bt_terrain_vertex
TERRAIN_VERTEX_DTYPE = np.dtype([("position", np.float32, 3), ("height", np.float32), ("normal", np.float32, 3), ("tile_index", np.uint32),
                                 ("coordinate_uv", np.float32, 2), ("view_distance", np.float32), ("blend_ratio", np.float32)])


def _geometry_flags(grid: bool, morph: bool, blend: bool, approximation=None, view_relative: bool = False) -> int:
    if view_relative and approximation is None:
        raise ValueError("view_relative=True needs approximation= (BT_GEOMETRY_VIEW_RELATIVE is the high-precision calls')")
    return (_ffi.GEOMETRY_GRID if grid else 0) | (0 if morph else _ffi.GEOMETRY_NO_MORPH) | (0 if blend else _ffi.GEOMETRY_NO_BLEND) | \
        (_ffi.GEOMETRY_VIEW_RELATIVE if view_relative else 0)


class TileTree:
    def __init__(self, tile_atlas: TileAtlas, model: TerrainModel, lod_count: int, view_config: TerrainViewConfig):
        self.atlas = tile_atlas
        self.model = model
        self.lod_count = lod_count
        self.view_config = view_config
        self.sides = model.side_count()
        self.nodes = self.sides * lod_count * view_config.tree_size ** 2
        h = C.c_void_p()
        _ffi.check(_ffi.lib().bt_tile_tree_create(tile_atlas.device._h, C.byref(model_c(model)), lod_count,
                                                  C.byref(view_config_c(view_config)), C.byref(h)))
        self._h = h

    @staticmethod
    def new(tile_atlas: TileAtlas, view_config: TerrainViewConfig) -> "TileTree":
        return TileTree(tile_atlas, tile_atlas.config.model, tile_atlas.config.lod_count, view_config)

    def update(self, view_position: Sequence[float]) -> Tuple[List[tuple], List[tuple]]:
        """TileTree::update: returns (released_tiles, requested_tiles) in the reference's push order."""
        pos = (C.c_double * 3)(*view_position)
        _ffi.check(_ffi.lib().bt_tile_tree_update(self._h, pos))
        rel, req = C.POINTER(_ffi.TileCoordinateC)(), C.POINTER(_ffi.TileCoordinateC)()
        nrel, nreq = C.c_uint32(), C.c_uint32()
        _ffi.check(_ffi.lib().bt_tile_tree_requests(self._h, C.byref(rel), C.byref(nrel), C.byref(req), C.byref(nreq)))
        t = lambda c: (c.side, c.lod, c.x, c.y)
        return [t(rel[i]) for i in range(nrel.value)], [t(req[i]) for i in range(nreq.value)]

    def apply_requests(self):
        _ffi.check(_ffi.lib().bt_tile_tree_apply_requests(self._h, self.atlas._h))

    def adjust_to_tile_atlas(self):
        _ffi.check(_ffi.lib().bt_tile_tree_adjust_to_tile_atlas(self._h, self.atlas._h))

    def read(self):
        """(entries (n, 2) u32, origins (sides, lods, 2) u32, node coordinates (n, 4) u32, requested (n,) u32)."""
        entries = np.zeros((self.nodes, 2), np.uint32)
        origins = np.zeros((self.sides, self.lod_count, 2), np.uint32)
        coords = np.zeros((self.nodes, 4), np.uint32)
        requested = np.zeros(self.nodes, np.uint32)
        _ffi.check(_ffi.lib().bt_tile_tree_read(
            self._h, entries.ctypes.data_as(C.POINTER(_ffi.TileTreeEntryC)), self.nodes,
            origins.ctypes.data_as(C.POINTER(C.c_uint32)), origins.size,
            coords.ctypes.data_as(C.POINTER(_ffi.TileCoordinateC)), requested.ctypes.data_as(C.POINTER(C.c_uint32))))
        return entries, origins, coords, requested

    def buffers(self) -> Tuple[int, int]:
        e, o = C.c_void_p(), C.c_void_p()
        _ffi.check(_ffi.lib().bt_tile_tree_buffers(self._h, C.byref(e), C.byref(o)))
        return e.value, o.value

    def sample_attachment(self, attachment_index: int, positions: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        positions = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        n = len(positions)
        out = np.zeros((n, 4), np.float32)
        heights = np.zeros(n, np.float32)
        _ffi.check(_ffi.lib().bt_tile_tree_sample_attachment(
            self._h, self.atlas._h, attachment_index, positions.ctypes.data_as(C.POINTER(C.c_double)), n,
            out.ctypes.data_as(C.POINTER(C.c_float)), heights.ctypes.data_as(C.POINTER(C.c_float))))
        return out, heights

    def sample_normal(self, attachment_index: int, positions: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """bt_tile_tree_sample_normal: the world normals of the ground under a batch of world positions, the reference shader's (LOD blend
        and best-loaded-tile fallback included), in one launch -> ((n, 3) float32 unit normals, (n,) float32 cosines of the slope against
        the mesh normal); zeros for a position with a non-finite component."""
        positions = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        n = len(positions)
        normals = np.zeros((n, 3), np.float32)
        up_dot = np.zeros(n, np.float32)
        _ffi.check(_ffi.lib().bt_tile_tree_sample_normal(
            self._h, self.atlas._h, attachment_index, positions.ctypes.data_as(C.POINTER(C.c_double)), n,
            normals.ctypes.data_as(C.POINTER(C.c_float)), up_dot.ctypes.data_as(C.POINTER(C.c_float))))
        return normals, up_dot

    def raycast(self, attachment_index: int, origins, directions, t_min, t_max, steps: int = 256, refine_rounds: int = 2, normals: bool = False):
        """bt_tile_tree_raycast: one launch for the whole batch.  origins / directions (n, 3), t_min / t_max scalars or (n,); returns a
        structured array (RAY_HIT_DTYPE): status (_ffi.RAY_*), step, t, t_above, position, height.  normals=True: returns (hits, normals),
        the second being sample_normal(attachment_index, hits["position"])[0] (one more launch; the position of a MISS or INVALID ray is
        the zero vector and its row is whatever the ground under that point gives)."""
        origins = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
        n = len(origins)
        rays = np.zeros(n, RAY_DTYPE)
        rays["origin"] = origins
        rays["direction"] = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
        rays["t_min"] = t_min
        rays["t_max"] = t_max
        hits = np.zeros(n, RAY_HIT_DTYPE)
        _ffi.check(_ffi.lib().bt_tile_tree_raycast(self._h, self.atlas._h, attachment_index, rays.ctypes.data_as(C.POINTER(_ffi.RayC)), n, steps,
                                                   refine_rounds, hits.ctypes.data_as(C.POINTER(_ffi.RayHitC))))
        if normals:
            return hits, self.sample_normal(attachment_index, hits["position"])[0]
        return hits

    def collide_spheres(self, attachment_index: int, centers, radii, refine_rounds: int = 2):
        """bt_tile_tree_collide_spheres: "does this sphere touch the ground: where, how deep, along which normal" for a batch, one launch.
        centers (n, 3), radii a scalar or (n,); returns a structured array (SPHERE_CONTACT_DTYPE): status (_ffi.CONTACT_*), candidate,
        distance (to the closest ground point found; the altitude over the foot when BELOW), depth = radius - distance, point, normal
        (from the point towards the centre), height.  CONTACT_NONE reports the clearance; CONTACT_FAR and CONTACT_INVALID nothing."""
        centers = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
        n = len(centers)
        spheres = np.zeros(n, SPHERE_DTYPE)
        spheres["center"] = centers
        spheres["radius"] = radii
        contacts = np.zeros(n, SPHERE_CONTACT_DTYPE)
        _ffi.check(_ffi.lib().bt_tile_tree_collide_spheres(self._h, self.atlas._h, attachment_index, spheres.ctypes.data_as(C.POINTER(_ffi.SphereC)), n,
                                                           refine_rounds, contacts.ctypes.data_as(C.POINTER(_ffi.SphereContactC))))
        return contacts

    def sweep_spheres(self, attachment_index: int, origins, directions, radii, t_min, t_max, steps: int = 64, bisections: int = 16, refine_rounds: int = 2):
        """bt_tile_tree_sweep_spheres: continuous collision of spheres moving as origin + t * direction for t in [t_min, t_max], one launch.
        The march stops at the first of steps + 1 positions where the sphere touches the ground (or its centre is under it) and bisects
        the bracket.  Returns a structured array (SWEEP_HIT_DTYPE): status (_ffi.RAY_*), step, t (blocked), t_above (free) and the
        contact at t (collide_spheres' record)."""
        origins = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
        n = len(origins)
        sweeps = np.zeros(n, SPHERE_SWEEP_DTYPE)
        sweeps["origin"] = origins
        sweeps["direction"] = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
        sweeps["radius"], sweeps["t_min"], sweeps["t_max"] = radii, t_min, t_max
        hits = np.zeros(n, SWEEP_HIT_DTYPE)
        _ffi.check(_ffi.lib().bt_tile_tree_sweep_spheres(self._h, self.atlas._h, attachment_index, sweeps.ctypes.data_as(C.POINTER(_ffi.SphereSweepC)), n, steps,
                                                         bisections, refine_rounds, hits.ctypes.data_as(C.POINTER(_ffi.SweepHitC))))
        return hits

    def render(self, camera: RenderCamera, steps: int = 256, refine_rounds: int = 2, planes=("t", "status", "normal", "rgba"), attachment_index: int = 0):
        """bt_tile_tree_render: the camera's view of the terrain, one ray per pixel marched on the device as raycast() marches it, shaded
        at the hit.  Returns a dict with the planes asked for — "t" (height, width) float64 (0 where nothing was met), "status"
        (height, width) uint8 (_ffi.RAY_*), "normal" (height, width, 3) float32, "rgba" (height, width, 4) uint8 — and "stats"
        (launches, hit_pixels, inside_pixels, miss_pixels).  attachment_index: the R16 height attachment."""
        unknown = set(planes) - {"t", "status", "normal", "rgba"}
        if unknown:
            raise ValueError(f"unknown planes {sorted(unknown)}")
        w, h = camera.width, camera.height
        shapes = {"t": ((h, w), np.float64, C.c_double), "status": ((h, w), np.uint8, C.c_uint8), "normal": ((h, w, 3), np.float32, C.c_float),
                  "rgba": ((h, w, 4), np.uint8, C.c_uint8)}
        out = {name: np.zeros(shapes[name][0], shapes[name][1]) for name in shapes if name in planes}
        ptr = lambda name: out[name].ctypes.data_as(C.POINTER(shapes[name][2])) if name in out else None
        stats = _ffi.RenderStatsC()
        _ffi.check(_ffi.lib().bt_tile_tree_render(self._h, self.atlas._h, attachment_index, C.byref(camera.c()), steps, refine_rounds, ptr("t"), ptr("status"),
                                                  ptr("normal"), ptr("rgba"), C.byref(stats)))
        out["stats"] = {name: getattr(stats, name) for name, _ in _ffi.RenderStatsC._fields_}
        return out

    def sun_occlusion(self, attachment_index: int, positions, directions, lift: float, distance: float, steps: int = 64):
        """bt_tile_tree_sun_occlusion: "is this point in the sun, for this direction towards it?" for every pair of positions (n, 3) and
        directions (k, 3) or (3,), the directions used as given (distance is in units of their length).  A point's shadow ray starts
        `lift` above it along the terrain's up direction there and is marched like raycast()'s at `steps` steps, no refinement.  Returns
        ((n, k) uint8 statuses, stats): _ffi.RAY_MISS is lit, RAY_HIT and RAY_INSIDE are occluded, RAY_INVALID a point or direction that
        cannot be marched; stats holds launches, lit, occluded, invalid.  A point raycast() or render() reported lies at or under the
        ground: give it a lift larger than that march's residual."""
        positions = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        directions = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
        n, k = len(positions), len(directions)
        status = np.zeros((n, k), np.uint8)
        stats = _ffi.OcclusionStatsC()
        as_doubles = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        _ffi.check(_ffi.lib().bt_tile_tree_sun_occlusion(self._h, self.atlas._h, attachment_index, as_doubles(positions), n, as_doubles(directions), k, lift,
                                                         distance, steps, status.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(stats)))
        return status, {name: getattr(stats, name) for name, _ in _ffi.OcclusionStatsC._fields_}

    def render_shadowed(self, camera: RenderCamera, lift: float, distance: float, shadow_steps: int = 64, steps: int = 256, refine_rounds: int = 2,
                        planes=("t", "status", "normal", "rgba", "shadow"), attachment_index: int = 0):
        """bt_tile_tree_render_shadowed: render() with cast shadows.  A pixel that met the ground casts a shadow ray towards camera.sun
        (sun_occlusion's, with this lift, distance and shadow_steps); with camera.lighting an occluded pixel keeps only the ambient
        light.  The extra plane "shadow" (height, width) uint8 holds the shadow ray's status (_ffi.RAY_*), _ffi.SHADOW_NONE where the
        pixel met nothing; the other planes and "stats" are render()'s."""
        unknown = set(planes) - {"t", "status", "normal", "rgba", "shadow"}
        if unknown:
            raise ValueError(f"unknown planes {sorted(unknown)}")
        w, h = camera.width, camera.height
        shapes = {"t": ((h, w), np.float64, C.c_double), "status": ((h, w), np.uint8, C.c_uint8), "normal": ((h, w, 3), np.float32, C.c_float),
                  "rgba": ((h, w, 4), np.uint8, C.c_uint8), "shadow": ((h, w), np.uint8, C.c_uint8)}
        out = {name: np.zeros(shapes[name][0], shapes[name][1]) for name in shapes if name in planes}
        ptr = lambda name: out[name].ctypes.data_as(C.POINTER(shapes[name][2])) if name in out else None
        stats = _ffi.RenderStatsC()
        shadow = _ffi.SunShadowC(lift, distance, shadow_steps, 0)
        _ffi.check(_ffi.lib().bt_tile_tree_render_shadowed(self._h, self.atlas._h, attachment_index, C.byref(camera.c()), steps, refine_rounds, C.byref(shadow),
                                                           ptr("t"), ptr("status"), ptr("normal"), ptr("rgba"), ptr("shadow"), C.byref(stats)))
        out["stats"] = {name: getattr(stats, name) for name, _ in _ffi.RenderStatsC._fields_}
        return out

    def vertices_per_tile(self, grid: bool = False) -> int:
        """slots a tile takes in either geometry layout: the strip's 2 g (g + 2) (bt_view_state.vertices_per_tile) or the grid's (g + 1)^2"""
        g = self.view_config.grid_size
        return (g + 1) ** 2 if grid else 2 * g * (g + 2)

    def tile_geometry(self, attachment_index: int, tiles, view=None, *, grid: bool = False, morph: bool = True, blend: bool = True, approximation=None,
                      view_relative: bool = False) -> np.ndarray:
        """bt_tile_tree_tile_geometry: the reference's vertex stage for the listed tiles ((n, 4) [side, lod, x, y] or TileCoordinates)
        -> an (n, vertices_per_tile(grid)) structured array (TERRAIN_VERTEX_DTYPE): position, height, the mesh normal, tile_index (the
        row), the morphed uv, view_distance, blend_ratio.  view: a bt_view_state (default: view_state()).  Synchronous; a read.
        approximation (a bt_model_approximation of the same position as the view: model_approximation() / model_approximation_from_config):
        bt_tile_tree_tile_geometry_hp, the reference's HIGH_PRECISION branch — vertices nearer than its precision_threshold_distance come
        from the Taylor series around the view; view_relative=True: positions relative to the view (BT_GEOMETRY_VIEW_RELATIVE)."""
        tiles = np.ascontiguousarray([(t.side, t.lod, t.x, t.y) if isinstance(t, TileCoordinate) else tuple(t) for t in tiles], dtype=np.uint32).reshape(-1, 4)
        out = np.zeros((len(tiles), self.vertices_per_tile(grid)), TERRAIN_VERTEX_DTYPE)
        flags = _geometry_flags(grid, morph, blend, approximation, view_relative)
        head = (self._h, self.atlas._h, attachment_index, C.byref(view) if view is not None else None)
        tail = (tiles.ctypes.data_as(C.POINTER(_ffi.TileCoordinateC)), len(tiles), flags, out.ctypes.data_as(C.POINTER(_ffi.TerrainVertexC)), out.nbytes)
        if approximation is None:
            _ffi.check(_ffi.lib().bt_tile_tree_tile_geometry(*head, *tail))
        else:
            _ffi.check(_ffi.lib().bt_tile_tree_tile_geometry_hp(*head, C.byref(approximation), *tail))
        return out

    def build_geometry(self, prepass, attachment_index: int = 0, view=None, *, vertices: Optional[int] = None, vertex_capacity: int = 0,
                       grid: bool = False, morph: bool = True, blend: bool = True, approximation=None, view_relative: bool = False):
        """bt_tile_tree_build_geometry: the vertices of the final tiles `prepass` last produced, in list order.  Pass the view the prepass
        ran with (default: view_state()).
        With vertices (a 16-byte aligned device pointer, e.g. Device.malloc's) and vertex_capacity (in vertices): one asynchronous
        launch behind that run, no host synchronisation; a tile that does not fit whole is skipped; returns None.
        Without: the convenience form — reads the list's length (one synchronisation), builds into a buffer of its own and returns the
        (tiles, vertices_per_tile(grid)) structured array (TERRAIN_VERTEX_DTYPE).
        approximation / view_relative: bt_tile_tree_build_geometry_hp, as in tile_geometry."""
        flags = _geometry_flags(grid, morph, blend, approximation, view_relative)
        head = (self._h, self.atlas._h, attachment_index, C.byref(view) if view is not None else None)
        if approximation is None:
            call = lambda ptr, capacity: _ffi.check(_ffi.lib().bt_tile_tree_build_geometry(*head, prepass._h, flags, C.c_void_p(ptr), capacity))
        else:
            call = lambda ptr, capacity: _ffi.check(_ffi.lib().bt_tile_tree_build_geometry_hp(*head, C.byref(approximation), prepass._h, flags, C.c_void_p(ptr), capacity))
        if vertices is not None:
            call(vertices, vertex_capacity)
            return None
        shape = (len(prepass.read()[0]), self.vertices_per_tile(grid))
        if shape[0] == 0:
            return np.zeros(shape, TERRAIN_VERTEX_DTYPE)
        device = self.atlas.device
        ptr = device.malloc(shape[0] * shape[1] * TERRAIN_VERTEX_DTYPE.itemsize)
        try:
            call(ptr, shape[0] * shape[1])
            return device.download(ptr, shape, TERRAIN_VERTEX_DTYPE)
        finally:
            device.free(ptr)

    def approximate_height(self) -> float:
        h = C.c_float()
        _ffi.check(_ffi.lib().bt_tile_tree_approximate_height(self._h, self.atlas._h, C.byref(h)))
        return h.value

    def frame_update(self, view_position: Sequence[float], prepass=None, *, unordered=False, plain=False, keep_requests=False, keep_height=False):
        """One frame of this view as ONE library call with one host synchronisation (bt_frame_update): update -> the lists
        applied to the atlas -> adjust_to_tile_atlas -> approximate_height (left on the device) -> the tiling prepass.
        Returns bt_frame_info (list lengths, the status of the apply step, the height this frame's update used)."""
        pos = (C.c_double * 3)(*view_position)
        info = _ffi.FrameInfoC()
        flags = (_ffi.FRAME_PREPASS_UNORDERED if unordered else 0) | (_ffi.FRAME_PREPASS_PLAIN if plain else 0) | \
            (_ffi.FRAME_KEEP_REQUESTS if keep_requests else 0) | (_ffi.FRAME_KEEP_HEIGHT if keep_height else 0)
        # the lists are consumed by the call (apply_requests drains them): read them through KEEP_REQUESTS when wanted
        _ffi.check(_ffi.lib().bt_frame_update(self._h, self.atlas._h, prepass._h if prepass is not None else None, pos, flags, C.byref(info)))
        return info

    def view_state(self) -> _ffi.ViewStateC:
        v = _ffi.ViewStateC()
        _ffi.check(_ffi.lib().bt_tile_tree_view_state(self._h, C.byref(v)))
        return v

    def model_approximation(self) -> _ffi.ModelApproximationC:
        """bt_tile_tree_model_approximation: the Taylor coefficients of the tree's last view position (the companion of view_state())"""
        a = _ffi.ModelApproximationC()
        _ffi.check(_ffi.lib().bt_tile_tree_model_approximation(self._h, C.byref(a)))
        return a

    def close(self):
        if getattr(self, "_h", None):
            if device_open(getattr(getattr(self, "atlas", None), "device", None)):
                _ffi.lib().bt_tile_tree_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sample_attachment(tile_tree: TileTree, tile_atlas: TileAtlas, attachment_index: int, sample_world_position):
    return tile_tree.sample_attachment(attachment_index, np.asarray([sample_world_position]))[0][0]


def sample_height(tile_tree: TileTree, tile_atlas: TileAtlas, sample_world_position) -> float:
    return float(tile_tree.sample_attachment(0, np.asarray([sample_world_position]))[1][0])


def sample_normal(tile_tree: TileTree, tile_atlas: TileAtlas, sample_world_position):
    """the world normal of the ground (height attachment) under one world position, as a tuple"""
    return tuple(float(v) for v in tile_tree.sample_normal(0, np.asarray([sample_world_position]))[0][0])


def raycast_terrain(tile_tree: TileTree, tile_atlas: TileAtlas, origin, direction, max_distance: float, steps: int = 256, refine_rounds: int = 2):
    """One ray from `origin` along `direction` (normalised here) up to `max_distance` against the height attachment: the world position where
    it meets the ground and the distance to it, or None when it does not (an origin under the ground meets it at distance 0)."""
    d = np.asarray(direction, dtype=np.float64)
    hit = tile_tree.raycast(0, [origin], [d / np.linalg.norm(d)], 0.0, max_distance, steps, refine_rounds)[0]
    if hit["status"] not in (_ffi.RAY_HIT, _ffi.RAY_INSIDE):
        return None
    return tuple(float(v) for v in hit["position"]), float(hit["t"])
