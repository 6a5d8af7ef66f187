"""Device context and TileAtlas (src/terrain_data/tile_atlas.rs:519-624 + gpu_tile_atlas.rs)."""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import List, Optional, Tuple, Union

import numpy as np

from . import _ffi
from .terrain import AttachmentFormat, TerrainConfig, TileCoordinate


def device_open(device) -> bool:
    """False once the Device (bt_ctx) behind a dependent object has been closed.  Python's cyclic garbage collector finalises the objects of a
    cycle in any order (an exception traceback that holds an atlas, its preprocessor and the device is such a cycle): a dependent object whose
    context was destroyed first must not call into the library with it — its native half is then left to the process's exit."""
    return device is not None and bool(getattr(device, "_h", None))


class Device:
    """One GPU + one HIP stream (bt_ctx).  With PyTorch present the context runs on torch's current
    stream of that device, so torch.cuda.Event timing and torch.distributed collectives order with it."""

    def __init__(self, index: int = 0, stream: Optional[int] = None):
        L = _ffi.lib()
        self.torch_stream = None
        if stream is None:
            try:
                import torch

                if torch.cuda.is_available():
                    # a dedicated torch stream: kernels, torch.cuda.Event timing and torch.distributed
                    # collectives issued under `with torch.cuda.stream(device.torch_stream)` share one queue
                    torch.cuda.set_device(index)
                    self.torch_stream = torch.cuda.Stream(device=index)
                    stream = self.torch_stream.cuda_stream
            except ImportError:
                stream = None
        h = C.c_void_p()
        _ffi.check(L.bt_ctx_create(index, C.c_void_p(stream) if stream else None, C.byref(h)))
        self._h = h
        self.index = index

    def synchronize(self):
        _ffi.check(_ffi.lib().bt_ctx_synchronize(self._h))

    def set_io_threads(self, threads: int = 0) -> int:
        """bt_ctx_set_io_threads: writer / reader threads of this context's save and load paths (0 = automatic: min(16, CPUs the
        process may use)); returns the count the next save / load uses"""
        _ffi.check(_ffi.lib().bt_ctx_set_io_threads(self._h, threads))
        return int(_ffi.lib().bt_ctx_io_threads(self._h))

    def io_threads(self) -> int:
        return int(_ffi.lib().bt_ctx_io_threads(self._h))

    def trim(self) -> int:
        """bt_ctx_trim: give back the raster buffer kept for the next queue and the pinned staging buffers; bytes released"""
        freed = C.c_uint64()
        _ffi.check(_ffi.lib().bt_ctx_trim(self._h, C.byref(freed)))
        return freed.value

    def timer_begin(self):
        _ffi.check(_ffi.lib().bt_ctx_timer_begin(self._h))

    def timer_end(self) -> float:
        ms = C.c_float()
        _ffi.check(_ffi.lib().bt_ctx_timer_end(self._h, C.byref(ms)))
        return ms.value

    def malloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        _ffi.check(_ffi.lib().bt_device_malloc(self._h, nbytes, C.byref(p)))
        return p.value

    def free(self, ptr: int):
        _ffi.check(_ffi.lib().bt_device_free(self._h, C.c_void_p(ptr)))

    def upload(self, array: np.ndarray) -> int:
        array = np.ascontiguousarray(array)
        ptr = self.malloc(array.nbytes)
        _ffi.check(_ffi.lib().bt_memcpy_h2d(self._h, C.c_void_p(ptr), array.ctypes.data_as(C.c_void_p), array.nbytes))
        return ptr

    def download(self, ptr: int, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        _ffi.check(_ffi.lib().bt_memcpy_d2h(self._h, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes))
        return out

    def synth_fbm_r16(self, width, height, seed, *, x0=0, y0=0, base_cell=None, octaves=6, dst: Optional[int] = None, pitch: Optional[int] = None) -> int:
        """Deterministic integer fBm heightmap in HBM; returns the device pointer (u16, tightly packed).  With dst / pitch / x0 / y0
        / base_cell it fills a WINDOW of a larger raster: texel (i, j) of the call is texel (x0 + i, y0 + j) of the pattern."""
        base_cell = base_cell or max(max(width, height) // 4, 1)
        ptr = dst if dst is not None else self.malloc(width * height * 2)
        _ffi.check(_ffi.lib().bt_synth_fbm_r16(self._h, C.c_void_p(ptr), width, height, pitch or width * 2, x0, y0, base_cell,
                                               octaves, seed & 0xFFFFFFFF))
        return ptr

    def close(self):
        if getattr(self, "_h", None):
            _ffi.lib().bt_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class EditStamp:
    """bt_edit_stamp: one brush stamp of TileAtlas.edit_height.  center / radius are in mosaic texels of the edited LOD on `side`
    (mosaic_position); amount is a normalised height (1 = max_height - min_height): the signed delta of "add", the target of "flatten"."""
    center: Tuple[float, float]
    radius: float
    amount: float
    mode: str = "add"        # "add" | "flatten"
    falloff: str = "smooth"  # "smooth": w = (1 - d^2 / r^2)^2 | "hard": w = 1
    side: int = 0

    def _c(self):
        return _ffi.EditStampC(self.side, {"add": _ffi.EDIT_ADD, "flatten": _ffi.EDIT_FLATTEN}[self.mode],
                               {"smooth": _ffi.EDIT_FALLOFF_SMOOTH, "hard": _ffi.EDIT_FALLOFF_HARD}[self.falloff], 0,
                               (C.c_float * 2)(float(self.center[0]), float(self.center[1])), float(self.radius), float(self.amount))


@dataclass
class SmoothStamp:
    """bt_smooth_stamp: one stamp of TileAtlas.smooth_height.  center / radius as EditStamp's; strength in (0, 1] is how far a texel under
    the stamp's full weight moves towards the box mean of its neighbourhood (1: onto it)."""
    center: Tuple[float, float]
    radius: float
    strength: float = 1.0
    falloff: str = "smooth"  # "smooth": w = (1 - d^2 / r^2)^2 | "hard": w = 1
    side: int = 0

    def _c(self):
        return _ffi.SmoothStampC(self.side, {"smooth": _ffi.EDIT_FALLOFF_SMOOTH, "hard": _ffi.EDIT_FALLOFF_HARD}[self.falloff],
                                 (C.c_float * 2)(float(self.center[0]), float(self.center[1])), float(self.radius), float(self.strength))


@dataclass
class PaintStamp:
    """bt_paint_stamp: one stamp of TileAtlas.paint (Rgba8).  center / radius as EditStamp's; color is normalised (1 = 255): the target of
    "blend", the signed delta of "add"; opacity in (0, 1] scales the falloff weight; channels selects what is painted: an iterable of
    channel indices or letters out of "rgba" (channel k is byte k of the texel)."""
    center: Tuple[float, float]
    radius: float
    color: Tuple[float, float, float, float]
    opacity: float = 1.0
    mode: str = "blend"      # "blend" | "add"
    falloff: str = "smooth"  # "smooth": w = (1 - d^2 / r^2)^2 | "hard": w = 1
    channels: object = "rgba"
    side: int = 0

    def channel_mask(self) -> int:
        if isinstance(self.channels, int):
            return self.channels
        mask = 0
        for ch in self.channels:
            mask |= 1 << ("rgba".index(ch) if isinstance(ch, str) else int(ch))
        return mask

    def _c(self):
        return _ffi.PaintStampC(self.side, {"blend": _ffi.PAINT_BLEND, "add": _ffi.PAINT_ADD}[self.mode],
                                {"smooth": _ffi.EDIT_FALLOFF_SMOOTH, "hard": _ffi.EDIT_FALLOFF_HARD}[self.falloff], self.channel_mask(),
                                (C.c_float * 2)(float(self.center[0]), float(self.center[1])), float(self.radius), float(self.opacity),
                                (C.c_float * 4)(*[float(v) for v in self.color]))


@dataclass
class SplatRule:
    """bt_splat_rule: one rule of TileAtlas.splat_from_height.  A texel's weight under the rule is weight * band(height) * band(steep), each band 1
    between its limits and falling to 0 (smoothstep) over `fade` outside them; fade 0 is a hard edge.  height: (lo, hi) in world height units
    (the model's min_height .. max_height), -inf / +inf allowed.  slope: (lo, hi) in DEGREES from flat, converted here to the library's
    steep = 1 - cos(slope); a lower limit <= 0 degrees becomes -inf and an upper limit >= 90 degrees +inf (no limit).  slope_fade is in units
    of steep (1 - cos), not in degrees.  colour (r, g, b), normalised, is what "colour" mode blends; "weights" mode ignores it."""
    height: Tuple[float, float] = (-math.inf, math.inf)
    slope: Tuple[float, float] = (0.0, 90.0)
    height_fade: float = 0.0
    slope_fade: float = 0.0
    weight: float = 1.0
    colour: Tuple[float, float, float] = (0.0, 0.0, 0.0)

    def steep(self) -> Tuple[float, float]:
        """the slope limits as the C struct carries them: 1 - cos, in binary32"""
        lo, hi = float(self.slope[0]), float(self.slope[1])
        lo = -math.inf if lo <= 0.0 else 1.0 - math.cos(math.radians(lo))
        hi = math.inf if hi >= 90.0 else 1.0 - math.cos(math.radians(hi))
        return float(np.float32(lo)), float(np.float32(hi))

    def _c(self):
        lo, hi = self.steep()
        return _ffi.SplatRuleC(float(self.height[0]), float(self.height[1]), float(self.height_fade), lo, hi, float(self.slope_fade), float(self.weight),
                               (C.c_float * 3)(*[float(v) for v in self.colour]), (C.c_uint32 * 2)(0, 0))


@dataclass
class ScatterRule:
    """bt_scatter_rule: one rule of TileAtlas.scatter_instances.  A cell places an instance of the rule with the probability density *
    band(height) * band(steep) * mask, the bands being SplatRule's (height in world height units, slope in DEGREES from flat, slope_fade in
    units of steep = 1 - cos).  mask_channel: None, or the channel (0 .. 3 or "r", "g", "b", "a") of the mask attachment whose byte / 255
    multiplies the probability.  scale: (lo, hi), the range an instance's scale is drawn from.  Rules exclude each other: a cell places at
    most one instance, of the first rule (in list order) its random number falls to."""
    height: Tuple[float, float] = (-math.inf, math.inf)
    slope: Tuple[float, float] = (0.0, 90.0)
    height_fade: float = 0.0
    slope_fade: float = 0.0
    density: float = 1.0
    scale: Tuple[float, float] = (1.0, 1.0)
    mask_channel: Optional[Union[int, str]] = None

    def steep(self) -> Tuple[float, float]:
        """the slope limits as the C struct carries them: 1 - cos, in binary32"""
        return SplatRule.steep(self)

    def channel(self) -> int:
        if self.mask_channel is None:
            return _ffi.SCATTER_NO_MASK
        return "rgba".index(self.mask_channel) if isinstance(self.mask_channel, str) else int(self.mask_channel)

    def _c(self):
        lo, hi = self.steep()
        return _ffi.ScatterRuleC(float(self.height[0]), float(self.height[1]), float(self.height_fade), lo, hi, float(self.slope_fade), float(self.density),
                                 float(self.scale[0]), float(self.scale[1]), self.channel(), (C.c_uint32 * 2)(0, 0))


# bt_scatter_instance as a numpy record: 56 bytes, no padding
SCATTER_INSTANCE_DTYPE = np.dtype([("position", "<f8", 3), ("normal", "<f4", 3), ("scale", "<f4"), ("yaw", "<f4"), ("rule", "<u4"), ("cell", "<u4", 2)])


@dataclass
class PathCost:
    """bt_path_cost: how TileAtlas.path_field turns heights into edge weights.  A raw texel becomes the height min_height + (max_height -
    min_height) * raw / 65535; cell_size is the world length of one texel (on a cube face, where texels are not uniform, the caller's
    approximation).  A step of length run (cell_size, or cell_size * sqrt 2) that rises by `rise` has the grade g = |rise| / run, exists only
    if g <= max_grade, and costs run * (1 + grade_weight * g) + climb_weight * max(rise, 0) + descend_weight * max(-rise, 0)."""
    min_height: float = 0.0
    max_height: float = 1.0
    cell_size: float = 1.0
    max_grade: float = math.inf
    grade_weight: float = 0.0
    climb_weight: float = 0.0
    descend_weight: float = 0.0

    def _c(self):
        return _ffi.PathCostC(float(self.min_height), float(self.max_height), float(self.cell_size), float(self.max_grade), float(self.grade_weight),
                              float(self.climb_weight), float(self.descend_weight), 0)


@dataclass
class ErosionParams:
    """bt_erosion_params: the constants of TileAtlas.erode_height.  A raw texel is the height min_height + (max_height - min_height) * raw /
    65535; cell_size is the world length of one texel.  Per step of length dt: `rain` * dt of water falls on every cell, water flows to the
    4-neighbours by the height differences of the water surface (gravity), a cell's carrying capacity is capacity * max(sin(slope), min_tilt) *
    speed (the speed taken over a depth of at least min_depth); it takes `erode` of what it lacks from the ground or leaves `deposit` of what
    it has too much, the sediment travels with the water, and evaporation * dt of the water goes.  Stability is the caller's: dt * gravity *
    depth / cell_size^2 well below 1."""
    min_height: float = 0.0
    max_height: float = 1.0
    cell_size: float = 1.0
    dt: float = 0.05
    rain: float = 0.5
    evaporation: float = 0.3
    gravity: float = 9.81
    capacity: float = 0.05
    erode: float = 0.3
    deposit: float = 0.3
    min_tilt: float = 0.05
    min_depth: float = 0.01
    steps: int = 1

    def _c(self):
        return _ffi.ErosionParamsC(float(self.min_height), float(self.max_height), float(self.cell_size), float(self.dt), float(self.rain), float(self.evaporation),
                                   float(self.gravity), float(self.capacity), float(self.erode), float(self.deposit), float(self.min_tilt), float(self.min_depth),
                                   int(self.steps), (C.c_uint32 * 3)(0, 0, 0))


PATH_TRACE_STATUS = {_ffi.PATH_TRACE_OK: "ok", _ffi.PATH_TRACE_BLOCKED: "blocked", _ffi.PATH_TRACE_UNREACHABLE: "unreachable", _ffi.PATH_TRACE_LOOP: "loop"}


def trace_path(next_plane: np.ndarray, start: Tuple[int, int]) -> Tuple[np.ndarray, str]:
    """bt_path_trace: follows the (h, w) uint8 next plane of TileAtlas.path_field from start = (x, y) to a goal -> ((n, 2) uint32 array of
    the cells (x, y) on the way, start and goal included; "ok", "blocked", "unreachable" or "loop").  Host code: no device."""
    next_plane = np.ascontiguousarray(next_plane, dtype=np.uint8)
    h, w = next_plane.shape
    count, status = C.c_uint32(), C.c_uint32()
    ptr = next_plane.ctypes.data_as(C.POINTER(C.c_uint8))
    _ffi.check(_ffi.lib().bt_path_trace(ptr, w, h, int(start[0]), int(start[1]), None, 0, C.byref(count), C.byref(status)))
    cells = np.zeros((count.value, 2), dtype=np.uint32)
    _ffi.check(_ffi.lib().bt_path_trace(ptr, w, h, int(start[0]), int(start[1]), cells.ctypes.data_as(C.POINTER(C.c_uint32)), count.value, C.byref(count), C.byref(status)))
    return cells, PATH_TRACE_STATUS[status.value]


def mosaic_position(uv, lod: int, center_size: int) -> Tuple[float, float]:
    """The mosaic position (EditStamp.center units) of face coordinate uv in [0, 1]^2 at `lod`: the face is 2^lod * center_size texels
    wide and texel g covers [g / n, (g + 1) / n) with its position at the integer g, so the middle of texel g maps to g."""
    n = (1 << lod) * center_size
    return (float(uv[0]) * n - 0.5, float(uv[1]) * n - 0.5)


def texel_dtype(fmt: AttachmentFormat):
    return np.uint16 if fmt == AttachmentFormat.R16 else np.uint8


class TileAtlas:
    """TileAtlas::new(&TerrainConfig) — owns the attachment atlases in HBM and the tile index allocator."""

    def __init__(self, config: TerrainConfig, device: Optional[Device] = None):
        self.config = config
        self.device = device or Device(0)
        self.model = config.model
        self.lod_count = config.lod_count
        self.atlas_size = config.atlas_size
        self.path = config.path
        cfg = _ffi.TerrainConfigC()
        cfg.lod_count = config.lod_count
        cfg.atlas_size = config.atlas_size
        cfg.spherical = int(config.model.is_spherical())
        cfg.attachment_count = len(config.attachments)
        for i, a in enumerate(config.attachments):
            cfg.attachments[i].name = a.name.encode()[:63]
            cfg.attachments[i].texture_size = a.texture_size
            cfg.attachments[i].border_size = a.border_size
            cfg.attachments[i].mip_level_count = a.mip_level_count
            cfg.attachments[i].format = a.format.id()
        cfg.path = config.path.encode()[:255]
        h = C.c_void_p()
        _ffi.check(_ffi.lib().bt_atlas_create(self.device._h, C.byref(cfg), C.byref(h)))
        self._h = h

    @staticmethod
    def new(config: TerrainConfig, device: Optional[Device] = None) -> "TileAtlas":
        return TileAtlas(config, device)

    # --- tile_atlas.rs:553-559
    def get_tile(self, c: TileCoordinate) -> Tuple[TileCoordinate, int]:
        t = _ffi.AtlasTileC()
        _ffi.check(_ffi.lib().bt_atlas_get_tile(self._h, c._c(), C.byref(t)))
        return TileCoordinate._from_c(t.coordinate), t.atlas_index

    def get_or_allocate_tile(self, c: TileCoordinate) -> Tuple[TileCoordinate, int]:
        t = _ffi.AtlasTileC()
        _ffi.check(_ffi.lib().bt_atlas_get_or_allocate_tile(self._h, c._c(), C.byref(t)))
        return TileCoordinate._from_c(t.coordinate), t.atlas_index

    def tiles(self) -> List[Tuple[TileCoordinate, int]]:
        """existing tiles with their atlas indices, in allocation order."""
        n = _ffi.lib().bt_atlas_tiles(self._h, None, None, 0)
        coords = (_ffi.TileCoordinateC * max(n, 1))()
        idx = (C.c_uint32 * max(n, 1))()
        _ffi.lib().bt_atlas_tiles(self._h, coords, idx, n)
        return [(TileCoordinate._from_c(coords[i]), idx[i]) for i in range(n)]

    # --- the streaming half of TileAtlasState (tile_atlas.rs:418-503)
    def request_tile(self, c: TileCoordinate):
        _ffi.check(_ffi.lib().bt_atlas_request_tile(self._h, c._c()))

    def release_tile(self, c: TileCoordinate):
        _ffi.check(_ffi.lib().bt_atlas_release_tile(self._h, c._c()))

    def get_best_tile(self, c: TileCoordinate) -> Tuple[int, int]:
        e = _ffi.TileTreeEntryC()
        _ffi.check(_ffi.lib().bt_atlas_get_best_tile(self._h, c._c(), C.byref(e)))
        return e.atlas_index, e.atlas_lod

    def pending_loads(self) -> int:
        return _ffi.lib().bt_atlas_pending_loads(self._h)

    def update(self, assets_root: str = "assets", max_loads: int = 0) -> Tuple[int, int]:
        """TileAtlasState::update + AtlasAttachment::update: run the queued tile loads; (loaded, failed)."""
        loaded, failed = C.c_uint32(), C.c_uint32()
        _ffi.check(_ffi.lib().bt_atlas_update(self._h, assets_root.encode(), max_loads, C.byref(loaded), C.byref(failed)))
        return loaded.value, failed.value

    def attachment_storage(self, attachment_index: int) -> Tuple[int, int, int]:
        """(device pointer, bytes per tile, layers) of the attachment's level-0 atlas."""
        p, tb, layers = C.c_void_p(), C.c_uint64(), C.c_uint32()
        _ffi.check(_ffi.lib().bt_atlas_attachment_storage(self._h, attachment_index, C.byref(p), C.byref(tb), C.byref(layers)))
        return p.value, tb.value, layers.value

    def _tile_shape(self, attachment_index, mip=0):
        a = self.config.attachments[attachment_index]
        T = a.texture_size >> mip
        return (T, T) if a.format == AttachmentFormat.R16 else (T, T, 4)

    def download_tiles(self, attachment_index: int, first_layer: int, count: int) -> np.ndarray:
        a = self.config.attachments[attachment_index]
        out = np.empty((count,) + self._tile_shape(attachment_index), dtype=texel_dtype(a.format))
        _ffi.check(_ffi.lib().bt_atlas_download_tiles(self._h, attachment_index, first_layer, count,
                                                      out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def download_tile(self, attachment_index: int, atlas_index: int) -> np.ndarray:
        return self.download_tiles(attachment_index, atlas_index, 1)[0]

    def upload_tile(self, attachment_index: int, atlas_index: int, data: np.ndarray):
        data = np.ascontiguousarray(data)
        _ffi.check(_ffi.lib().bt_atlas_upload_tile(self._h, attachment_index, atlas_index, data.ctypes.data_as(C.c_void_p), data.nbytes))

    def generate_mipmaps(self, attachment_index: int, first_layer: int = 0, count: Optional[int] = None):
        count = self.atlas_size - first_layer if count is None else count
        _ffi.check(_ffi.lib().bt_atlas_generate_mipmaps(self._h, attachment_index, first_layer, count))

    def download_mip(self, attachment_index: int, mip: int, atlas_index: int) -> np.ndarray:
        if mip == 0:  # a read stays a read: bt_atlas_mip_storage(level 0) counts as a write to every layer
            return self.download_tile(attachment_index, atlas_index)
        p, tb = C.c_void_p(), C.c_uint64()
        _ffi.check(_ffi.lib().bt_atlas_mip_storage(self._h, attachment_index, mip, C.byref(p), C.byref(tb)))
        if not p.value:
            raise ValueError(f"mip level {mip} of attachment {attachment_index} has no storage yet (generate_mipmaps or load_tiles allocates it)")
        a = self.config.attachments[attachment_index]
        return self.device.download(p.value + tb.value * atlas_index, self._tile_shape(attachment_index, mip), texel_dtype(a.format))

    def attachment_directory(self, assets_root: str, attachment_index: int) -> str:
        """AtlasAttachment::new: "assets/{path}/data/{name}" (tile_atlas.rs:175)."""
        return os.path.join(assets_root, self.path, "data", self.config.attachments[attachment_index].name)

    def save_attachment(self, attachment_index: int, directory: str):
        _ffi.check(_ffi.lib().bt_atlas_save_attachment(self._h, attachment_index, directory.encode()))

    def save_tile_config(self, assets_root: str = "assets"):
        os.makedirs(os.path.join(assets_root, self.path), exist_ok=True)
        _ffi.check(_ffi.lib().bt_atlas_save_tile_config(self._h, os.path.join(assets_root, self.path, "config.tc").encode()))

    def load_tile_config(self, assets_root: str = "assets"):
        _ffi.check(_ffi.lib().bt_atlas_load_tile_config(self._h, os.path.join(assets_root, self.path, "config.tc").encode()))

    def load_tiles(self, attachment_index: int, assets_root: str = "assets", coords: Optional[list] = None):
        """The tile load path (start_loading + upload_tiles, tile_atlas.rs:118-149, gpu_tile_atlas.rs:309-336) for a
        batch: `.bin` files -> atlas layers, then the mip chain of those layers on the GPU.  coords=None: every tile
        of the loaded tile config."""
        directory = self.attachment_directory(assets_root, attachment_index).encode()
        if coords is None:
            _ffi.check(_ffi.lib().bt_atlas_load_tiles(self._h, attachment_index, directory, None, 0))
        else:
            arr = (_ffi.TileCoordinateC * max(len(coords), 1))(*[c._c() for c in coords])
            _ffi.check(_ffi.lib().bt_atlas_load_tiles(self._h, attachment_index, directory, arr, len(coords)))
        return self

    def sample(self, attachment_index: int, atlas_indices, atlas_uvs, atlas_lods=None) -> np.ndarray:
        """TileAtlas::sample_attachment for a batch of TileLookups (tile_atlas.rs:249-258, 569-571): bilinear sample
        of level 0 of tile `atlas_indices[i]` at `atlas_uvs[i]` (uv over the tile's centre) -> (n, 4) float32."""
        idx = np.ascontiguousarray(atlas_indices, dtype=np.uint32).ravel()
        uv = np.ascontiguousarray(atlas_uvs, dtype=np.float32).reshape(-1, 2)
        n = len(idx)
        lookups = np.zeros(n, dtype=np.dtype([("atlas_index", "<u4"), ("atlas_lod", "<u4"), ("atlas_uv", "<f4", (2,))]))
        lookups["atlas_index"] = idx
        lookups["atlas_lod"] = 0 if atlas_lods is None else np.asarray(atlas_lods, dtype=np.uint32)
        lookups["atlas_uv"] = uv
        out = np.empty((n, 4), dtype=np.float32)
        _ffi.check(_ffi.lib().bt_atlas_sample(self._h, attachment_index, lookups.ctypes.data_as(C.c_void_p), n,
                                              out.ctypes.data_as(C.c_void_p)))
        return out

    def tile_bounds(self, attachment_index: int, layers=None, grid: int = 1, skip_zero: bool = False) -> List[np.ndarray]:
        """bt_atlas_tile_bounds: the min/max pyramid of R16 layers (layers=None: the layers of tiles(), in that order) -> one uint16 array
        per level, finest first, shaped (len(layers), n_k, n_k, 2) with n_k = grid >> k and [..., 0] = min, [..., 1] = max (raw unorm16).
        A cell covers its block plus the first column to its right and the first row below it; with skip_zero texels equal to 0 are left
        out and a cell without texels is (0xFFFF, 0)."""
        if layers is None:
            layers = [i for _, i in self.tiles()]
        idx = np.ascontiguousarray(layers, dtype=np.uint32).ravel()
        levels = [grid >> k for k in range(max(grid, 1).bit_length())]
        out = np.empty((len(idx), sum(n * n for n in levels), 2), dtype=np.uint16)
        _ffi.check(_ffi.lib().bt_atlas_tile_bounds(self._h, attachment_index, idx.ctypes.data_as(C.POINTER(C.c_uint32)), len(idx), grid,
                                                   _ffi.BOUNDS_SKIP_ZERO if skip_zero else 0, out.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                   out.nbytes))
        result, base = [], 0
        for n in levels:
            result.append(out[:, base:base + n * n].reshape(len(idx), n, n, 2))
            base += n * n
        return result

    def tile_normals(self, attachment_index: int, coords) -> np.ndarray:
        """bt_atlas_tile_normals: the tangent-space normal map of the centre texels of the listed tiles of an R16 attachment, for the
        config's terrain model -> (n, c, c, 4) uint8: r, g, b = the normal's x, y, z as round(255 * (0.5 + 0.5 * v)), a = 255 where the
        texel has data, (128, 128, 255, 0) where it has none.  Ordered behind the queued work; synchronous; a read."""
        from .tile_tree import model_c
        coords = list(coords)
        a = self.config.attachments[attachment_index]
        c = a.texture_size - 2 * a.border_size
        arr = (_ffi.TileCoordinateC * max(len(coords), 1))(*[t._c() if hasattr(t, "_c") else _ffi.TileCoordinateC(*t) for t in coords])
        out = np.zeros((len(coords), c, c, 4), dtype=np.uint8)
        _ffi.check(_ffi.lib().bt_atlas_tile_normals(self._h, attachment_index, C.byref(model_c(self.config.model)), arr, len(coords),
                                                    out.ctypes.data_as(C.POINTER(C.c_uint8)), out.nbytes))
        return out

    def _edit_result(self, call) -> Tuple[List[TileCoordinate], dict]:
        """runs call(changed, cap, stats) and, if the list did not fit, is NOT run again: the first call sizes the list for any edit"""
        cap = max(self.atlas_size, 1)  # a call cannot write more tiles than the atlas has layers
        changed = (_ffi.TileCoordinateC * cap)()
        stats = _ffi.EditStatsC()
        _ffi.check(call(changed, cap, C.byref(stats)))
        out = {name: getattr(stats, name) for name, _ in _ffi.EditStatsC._fields_}
        return [TileCoordinate._from_c(changed[i]) for i in range(min(stats.changed_count, cap))], out

    def edit_height(self, attachment_index: int, stamps, lod: Optional[int] = None) -> Tuple[List[TileCoordinate], dict]:
        """bt_atlas_edit_height: apply the EditStamps, in list order, to the centre texels of the existing tiles of `lod` (default: the
        finest, lod_count - 1) of an R16 attachment, then restore the ancestors, the aprons and the mips that depend on them, on the
        device and without synchronising.  Returns (changed tiles: LOD descending then atlas index, bt_edit_stats as a dict).  Tiles finer
        than `lod` are not touched (stats["tiles_with_children"]); a HeightBounds table follows with update(atlas, changed), tile-tree state is the caller's to refresh."""
        lod = self.lod_count - 1 if lod is None else lod
        stamps = list(stamps)
        arr = (_ffi.EditStampC * max(len(stamps), 1))(*[s._c() for s in stamps])
        return self._edit_result(lambda changed, cap, stats: _ffi.lib().bt_atlas_edit_height(self._h, attachment_index, lod, arr, len(stamps), changed, cap, stats))

    def smooth_height(self, attachment_index: int, stamps, kernel_radius: int = 1, lod: Optional[int] = None) -> Tuple[List[TileCoordinate], dict]:
        """bt_atlas_smooth_height: move the centre texels under the SmoothStamps towards the mean of their (2 * kernel_radius + 1)^2 box
        (no-data texels excluded and left alone; kernel_radius 1 .. 4 and <= border_size), every mean taken from the state BEFORE the call:
        one call is one Jacobi pass under all its stamps.  Then everything is restored as by edit_height.  Returns (changed, stats);
        stats["launches"] counts two launches for the brush."""
        lod = self.lod_count - 1 if lod is None else lod
        stamps = list(stamps)
        arr = (_ffi.SmoothStampC * max(len(stamps), 1))(*[s._c() for s in stamps])
        return self._edit_result(lambda changed, cap, stats: _ffi.lib().bt_atlas_smooth_height(self._h, attachment_index, lod, kernel_radius, arr, len(stamps), changed, cap, stats))

    def paint(self, attachment_index: int, stamps, lod: Optional[int] = None) -> Tuple[List[TileCoordinate], dict]:
        """bt_atlas_paint: apply the PaintStamps, in list order, to the centre texels of the existing tiles of `lod` (default: the finest) of
        an Rgba8 attachment, then restore the ancestors, the aprons and the mips as edit_height does, without synchronising.  Texels without
        data (rgb == 0) are left alone and none is made.  Returns (changed, stats)."""
        lod = self.lod_count - 1 if lod is None else lod
        stamps = list(stamps)
        arr = (_ffi.PaintStampC * max(len(stamps), 1))(*[s._c() for s in stamps])
        return self._edit_result(lambda changed, cap, stats: _ffi.lib().bt_atlas_paint(self._h, attachment_index, lod, arr, len(stamps), changed, cap, stats))

    def splat_from_height(self, height_attachment: int, target_attachment: int, rules, mode: str = "colour", fallback=(0, 0, 0, 255), rect=None,
                          lod: Optional[int] = None, side: int = 0) -> Tuple[List[TileCoordinate], dict]:
        """bt_atlas_splat_from_height: procedural texturing.  Evaluates the SplatRules (at most 8; 4 in "weights" mode) on the height and the
        slope of every centre texel of the R16 attachment `height_attachment` inside rect = (x0, y0, w, h) (mosaic texels of `lod` on `side`;
        default: the whole face) and writes the same texels of the Rgba8 attachment `target_attachment` (same texture and border size):
        "colour": the rules' colours blended by their weights, alpha 255; "weights": byte k = rule k's share of the weight (a splat map).
        A texel no rule reaches gets the four `fallback` bytes, a texel without height data becomes (0, 0, 0, 0).  Then the target's
        ancestors, aprons and mips are restored as by write_region; on the device, without synchronising.  The terrain model is the
        config's.  Returns (changed, stats) of the target."""
        from .tile_tree import model_c
        lod = self.lod_count - 1 if lod is None else lod
        if rect is None:
            a = self.config.attachments[target_attachment]
            n = (a.texture_size - 2 * a.border_size) << lod
            rect = (0, 0, n, n)
        x0, y0, w, h = rect
        rules = list(rules)
        arr = (_ffi.SplatRuleC * max(len(rules), 1))(*[r._c() for r in rules])
        bytes4 = (C.c_uint8 * 4)(*[int(v) for v in fallback])
        mode_c = {"weights": _ffi.SPLAT_WEIGHTS, "colour": _ffi.SPLAT_COLOUR}[mode]
        model = model_c(self.config.model)
        return self._edit_result(lambda changed, cap, stats: _ffi.lib().bt_atlas_splat_from_height(
            self._h, height_attachment, target_attachment, C.byref(model), side, lod, x0, y0, w, h, mode_c, arr, len(rules), bytes4, changed, cap, stats))

    def scatter_instances(self, height_attachment: int, rules, coords, mask_attachment: Optional[int] = None, seed: int = 0, jitter: float = 1.0,
                          cap: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, dict]:
        """bt_atlas_scatter_instances: vegetation placement.  Every centre texel (cell) of the listed tiles of the R16 attachment
        `height_attachment` places at most one instance: of the first ScatterRule (at most 8) its random number falls to, a rule's
        probability being density * band(height) * band(slope) * the byte of its mask_channel of the Rgba8 attachment `mask_attachment`
        (same texture and border size; e.g. a weights splat map or a painted density) / 255.  The random numbers are a hash of `seed` and
        the cell's mosaic position, so a tile's instances do not depend on what else is listed; `jitter` in [0, 1] moves an instance off its
        texel's centre.  Returns (instances, first, stats): instances, a structured array (SCATTER_INSTANCE_DTYPE: position f64 x 3 and normal
        f32 x 3 in world space, scale, yaw in [0, 2 pi), rule, cell = mosaic texel) in list order, j major then i within a tile; first
        (len(coords) + 1) uint64: first[t] is the index of tile t's first instance, first[-1] the total; stats: bt_scatter_stats as a dict.
        cap=None sizes the list with a first call that writes nothing; with a cap only the first min(total, cap) instances come back while
        first and stats describe the whole list.  The terrain model is the config's.  Ordered behind the queued work; synchronous; a read."""
        from .tile_tree import model_c
        coords, rules = list(coords), list(rules)
        arr = (_ffi.TileCoordinateC * max(len(coords), 1))(*[t._c() if hasattr(t, "_c") else _ffi.TileCoordinateC(*t) for t in coords])
        rules_c = (_ffi.ScatterRuleC * max(len(rules), 1))(*[r._c() for r in rules])
        model = model_c(self.config.model)
        mask = _ffi.SCATTER_NO_MASK if mask_attachment is None else mask_attachment
        first = np.zeros(len(coords) + 1, dtype=np.uint64)
        stats = _ffi.ScatterStatsC()

        def call(out, n):
            _ffi.check(_ffi.lib().bt_atlas_scatter_instances(self._h, height_attachment, mask, C.byref(model), arr, len(coords), rules_c, len(rules), seed, float(jitter),
                                                             out.ctypes.data_as(C.POINTER(_ffi.ScatterInstanceC)) if n else None, n,
                                                             first.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(stats)))

        if cap is None:
            call(None, 0)
            cap = stats.total
        out = np.zeros(cap, dtype=SCATTER_INSTANCE_DTYPE)
        call(out, cap)
        result = {name: getattr(stats, name) for name, _ in _ffi.ScatterStatsC._fields_ if name != "_padding"}
        result["per_rule"] = list(stats.per_rule)
        return out[:stats.written], first, result

    def read_region(self, attachment_index: int, x0: int, y0: int, w: int, h: int, lod: Optional[int] = None, side: int = 0) -> Tuple[np.ndarray, int]:
        """bt_atlas_read_region: the w x h rectangle of centre texels at mosaic position (x0, y0) of `lod` on `side`, the inverse of
        write_region: ((h, w) uint16 for R16, (h, w, 4) uint8 for Rgba8; zeros where the atlas holds no tile, number of such tiles).
        Ordered behind the queued work; synchronous."""
        lod = self.lod_count - 1 if lod is None else lod
        a = self.config.attachments[attachment_index]
        out = np.zeros((h, w) if a.format == AttachmentFormat.R16 else (h, w, 4), dtype=texel_dtype(a.format))
        missing = C.c_uint32()
        _ffi.check(_ffi.lib().bt_atlas_read_region(self._h, attachment_index, side, lod, x0, y0, w, h, out.ctypes.data_as(C.c_void_p), 0, C.byref(missing)))
        return out, missing.value

    def path_field(self, attachment_index: int, x0: int, y0: int, w: int, h: int, cost: "PathCost", goals, blocked: Optional[np.ndarray] = None,
                   lod: Optional[int] = None, side: int = 0, want_cost: bool = True, want_next: bool = True):
        """bt_atlas_path_field: the shortest-path field of the w x h window of centre texels at mosaic position (x0, y0) of `lod` on `side`
        of an R16 attachment towards `goals` (up to 4096 of (x, y) or (x, y, cost0), in cells of the window), over the 8-connected grid
        without corner cutting, with the edge weights of `cost` (PathCost).  Texels without data, tiles the atlas does not hold and cells
        where the optional (h, w) mask `blocked` is non-zero are blocked.  Returns (cost, next, stats): cost (h, w) float32, the cost of
        travelling from each cell to its best goal (+inf: none, or blocked); next (h, w) uint8: 0..7 the neighbour to step to ((1,0),
        (1,1), (0,1), (-1,1), (-1,0), (-1,-1), (0,-1), (1,-1)), 8 a goal, 254 unreachable, 255 blocked (trace_path follows it); stats:
        bt_path_stats as a dict.  want_cost / want_next False: that plane is not copied out and None comes back in its place.  Both planes
        are exact: bit for bit what Dijkstra's algorithm gives in binary32.  Ordered behind the queued work; synchronous; a read."""
        lod = self.lod_count - 1 if lod is None else lod
        goals = [tuple(g) for g in goals]
        arr = (_ffi.PathGoalC * max(len(goals), 1))(*[_ffi.PathGoalC(int(g[0]), int(g[1]), float(g[2]) if len(g) > 2 else 0.0) for g in goals])
        mask = None
        if blocked is not None:
            mask = np.ascontiguousarray(blocked, dtype=np.uint8)
            if mask.shape != (h, w):
                raise ValueError(f"path_field: a mask of shape {mask.shape} for a window of {(h, w)}")
        cost_out = np.zeros((h, w), dtype=np.float32) if want_cost else None
        next_out = np.zeros((h, w), dtype=np.uint8) if want_next else None
        stats = _ffi.PathStatsC()
        cost_c = cost._c()
        _ffi.check(_ffi.lib().bt_atlas_path_field(
            self._h, attachment_index, side, lod, x0, y0, w, h, C.byref(cost_c), arr, len(goals),
            mask.ctypes.data_as(C.POINTER(C.c_uint8)) if mask is not None else None,
            cost_out.ctypes.data_as(C.POINTER(C.c_float)) if want_cost else None,
            next_out.ctypes.data_as(C.POINTER(C.c_uint8)) if want_next else None, C.byref(stats)))
        return cost_out, next_out, {name: getattr(stats, name) for name, _ in _ffi.PathStatsC._fields_}

    def drainage(self, attachment_index: int, x0: int, y0: int, w: int, h: int, void: Optional[np.ndarray] = None, weight: Optional[np.ndarray] = None,
                 lod: Optional[int] = None, side: int = 0, want_filled: bool = True, want_flat: bool = True, want_direction: bool = True,
                 want_accumulation: bool = True):
        """bt_atlas_drainage: where water collects and where it runs in the w x h window of centre texels at mosaic position (x0, y0) of `lod`
        on `side` of an R16 attachment, by the header's DRAINAGE section, in integers.  Texels without data, tiles the atlas does not hold
        and cells where the optional (h, w) mask `void` is non-zero are void; an active cell beside a void one or on the window's edge is an
        outlet.  Returns (filled, flat, direction, accumulation, stats): filled (h, w) uint16, the level the depressions fill to (filled -
        height = the lake's depth; 0 on void cells); flat (h, w) uint32, the distance inside a level area to the nearest cell that drains
        lower; direction (h, w) uint8: 0..7 the neighbour the water goes to ((1,0), (1,1), (0,1), (-1,1), (-1,0), (-1,-1), (0,-1), (1,-1)),
        8 an outlet, 255 void (trace_path follows it downstream); accumulation (h, w) uint32: the sum of `weight` ((h, w) uint8, 1 where
        None) over the cell and everything that drains through it; stats: bt_drainage_stats as a dict.  want_* False: that plane is not
        copied out and None comes back in its place.  All planes are exact: byte for byte what priority-flood, a breadth-first search and a
        topological sum give.  Ordered behind the queued work; synchronous; a read."""
        lod = self.lod_count - 1 if lod is None else lod

        def plane(array, name):
            if array is None:
                return None
            array = np.ascontiguousarray(array, dtype=np.uint8)
            if array.shape != (h, w):
                raise ValueError(f"drainage: a {name} plane of shape {array.shape} for a window of {(h, w)}")
            return array

        void_c, weight_c = plane(void, "void"), plane(weight, "weight")
        outs = [np.zeros((h, w), dtype=t) if want else None
                for t, want in ((np.uint16, want_filled), (np.uint32, want_flat), (np.uint8, want_direction), (np.uint32, want_accumulation))]
        types = (C.c_uint16, C.c_uint32, C.c_uint8, C.c_uint32)
        stats = _ffi.DrainageStatsC()
        _ffi.check(_ffi.lib().bt_atlas_drainage(
            self._h, attachment_index, side, lod, x0, y0, w, h,
            void_c.ctypes.data_as(C.POINTER(C.c_uint8)) if void_c is not None else None,
            weight_c.ctypes.data_as(C.POINTER(C.c_uint8)) if weight_c is not None else None,
            *[o.ctypes.data_as(C.POINTER(t)) if o is not None else None for o, t in zip(outs, types)], C.byref(stats)))
        return (*outs, {name: getattr(stats, name) for name, _ in _ffi.DrainageStatsC._fields_ if name != "_padding"})

    def viewshed(self, attachment_index: int, x0: int, y0: int, w: int, h: int, observers, target_height: int = 0, lod: Optional[int] = None, side: int = 0,
                 clearance: bool = True, count: bool = True, mask: bool = False):
        """bt_atlas_viewshed: what `observers` see of the w x h window of centre texels at mosaic position (x0, y0) of `lod` on `side` of an
        R16 attachment, by the header's VIEWSHED section, in integers.  observers: an (N, 4) integer array or a list of (x, y, eye_height,
        radius) (shorter tuples: eye_height 0, radius 0 = unlimited), in cells of the window, 64 at most; one on a cell without data is
        skipped.  Returns (clearance, count, mask, stats): clearance (h, w) uint32, the smallest whole height above the ground of the cell
        that any observer covering it sees (VIEWSHED_NONE: no data, or no observer covers it); count (h, w) uint8, the observers that see a
        target of `target_height` on the cell; mask (h, w) uint64, bit o set for exactly those observers; stats: bt_viewshed_stats as a
        dict.  clearance / count / mask False: that plane is not copied out and None comes back in its place.  All planes are exact.
        Ordered behind the queued work; synchronous; a read."""
        lod = self.lod_count - 1 if lod is None else lod
        rows = [tuple(int(v) for v in o) for o in (observers.tolist() if isinstance(observers, np.ndarray) else observers)]
        arr = (_ffi.ViewshedObserverC * max(len(rows), 1))(*[_ffi.ViewshedObserverC(*(o + (0, 0))[:4]) for o in rows])
        outs = [np.zeros((h, w), dtype=t) if want else None for t, want in ((np.uint32, clearance), (np.uint8, count), (np.uint64, mask))]
        types = (C.c_uint32, C.c_uint8, C.c_uint64)
        stats = _ffi.ViewshedStatsC()
        _ffi.check(_ffi.lib().bt_atlas_viewshed(self._h, attachment_index, side, lod, x0, y0, w, h, arr, len(rows), target_height,
                                                *[o.ctypes.data_as(C.POINTER(t)) if o is not None else None for o, t in zip(outs, types)], C.byref(stats)))
        return (*outs, {name: getattr(stats, name) for name, _ in _ffi.ViewshedStatsC._fields_ if name != "_padding"})

    def distance_field(self, attachment_index: int, x0: int, y0: int, w: int, h: int, *, lo: Optional[int] = None, hi: Optional[int] = None, channel: int = 0,
                       seeds: Optional[np.ndarray] = None, invert: bool = False, bake=None, lod: Optional[int] = None, side: int = 0,
                       dist2: bool = True, nearest: bool = True):
        """bt_atlas_distance_field: the exact Euclidean distance transform of the w x h window of centre texels at mosaic position (x0, y0)
        of `lod` on `side` of an R16 or Rgba8 attachment, by the header's DISTANCE section, in integers.  A cell is a seed when its texel
        value (the raw u16; byte `channel` of an Rgba8 texel) lies in [lo, hi] (either given: BT_DISTANCE_FROM_TEXELS; lo alone reaches up to
        the format's largest value, hi alone down to 0), or when the optional (h, w) uint8 plane `seeds` is non-zero there; `invert`
        exchanges seeds and the rest.  Returns (dist2,
        nearest, stats): dist2 (h, w) uint32, the squared distance in cells to the nearest seed; nearest (h, w) uint32, the index
        y * w + x of that seed, the smallest on a tie; both DISTANCE_NONE without a seed; stats: bt_distance_stats as a dict.  dist2 /
        nearest False: that plane is not copied out and None comes back in its place.  bake: (attachment, channel, reach) or
        (attachment, channel, reach, near) or a dict of those names: byte `channel` of that Rgba8 attachment becomes
        min(255, floor(255 * distance / reach)) over the window, 255 minus that with `near`, and the atlas is updated as by write_region;
        stats["edit"] is then its bt_edit_stats and stats["changed"] the changed tiles.  Ordered behind the queued work; synchronous; a
        read without `bake`."""
        lod = self.lod_count - 1 if lod is None else lod
        flags = (_ffi.DISTANCE_INVERT if invert else 0) | (_ffi.DISTANCE_FROM_TEXELS if lo is not None or hi is not None else 0)
        formats = self.config.attachments
        top = 255 if attachment_index < len(formats) and formats[attachment_index].format == AttachmentFormat.Rgba8 else 65535
        seeds_c = _ffi.DistanceSeedsC(channel, 0 if lo is None else lo, (top if flags & _ffi.DISTANCE_FROM_TEXELS else 0) if hi is None else hi, flags)
        plane = None
        if seeds is not None:
            plane = np.ascontiguousarray(seeds, dtype=np.uint8)
            if plane.shape != (h, w):
                raise ValueError(f"distance_field: a seeds plane of shape {plane.shape} for a window of {(h, w)}")
        bake_c = None
        if bake is not None:
            if isinstance(bake, dict):
                bake = (bake["attachment"], bake["channel"], bake["reach"], bake.get("near", False))
            bake = tuple(bake) + (False,) * (4 - len(bake))
            bake_c = _ffi.DistanceBakeC(bake[0], bake[1], bake[2], _ffi.DISTANCE_BAKE_NEAR if bake[3] else 0)
        outs = [np.zeros((h, w), dtype=np.uint32) if want else None for want in (dist2, nearest)]
        cap = max(self.atlas_size, 1)
        changed = (_ffi.TileCoordinateC * cap)()
        stats = _ffi.DistanceStatsC()
        _ffi.check(_ffi.lib().bt_atlas_distance_field(
            self._h, attachment_index, side, lod, x0, y0, w, h, C.byref(seeds_c), plane.ctypes.data_as(C.POINTER(C.c_uint8)) if plane is not None else None,
            *[o.ctypes.data_as(C.POINTER(C.c_uint32)) if o is not None else None for o in outs], C.byref(bake_c) if bake_c is not None else None, changed, cap,
            C.byref(stats)))
        out = {name: getattr(stats, name) for name, _ in _ffi.DistanceStatsC._fields_ if name not in ("edit", "_padding")}
        out["edit"] = {name: getattr(stats.edit, name) for name, _ in _ffi.EditStatsC._fields_}
        out["changed"] = [TileCoordinate._from_c(changed[i]) for i in range(min(stats.edit.changed_count, cap))]
        return (*outs, out)

    REGION_DTYPE = np.dtype([("label", "<u4"), ("area", "<u4"), ("x_min", "<u2"), ("y_min", "<u2"), ("x_max", "<u2"), ("y_max", "<u2"), ("v_min", "<u2"),
                             ("v_max", "<u2"), ("edges", "<u4"), ("v_sum", "<u8")])  # bt_region, 32 bytes

    def label_regions(self, attachment_index: int, x0: int, y0: int, w: int, h: int, *, lo: Optional[int] = None, hi: Optional[int] = None, channel: int = 0,
                      members: Optional[np.ndarray] = None, invert: bool = False, eight: bool = False, max_step: int = 65535, bake=None,
                      lod: Optional[int] = None, side: int = 0, label: bool = True, id: bool = True, region_cap: Optional[int] = None):
        """bt_atlas_label_regions: the connected regions of a mask over the w x h window of centre texels at mosaic position (x0, y0) of
        `lod` on `side` of an R16 or Rgba8 attachment, by the header's REGIONS section, in integers.  A cell is a member when its texel value
        (the raw u16; byte `channel` of an Rgba8 texel) lies in [lo, hi] (either given: BT_REGIONS_FROM_TEXELS; lo alone reaches up to the
        format's largest value, hi alone down to 0), or when the optional (h, w) uint8 plane `members` is non-zero there; `invert`
        exchanges members and the rest.  Two adjacent members (with `eight` also across a corner) whose values differ by at most max_step
        are linked.  Returns (label, id, regions, stats): label (h, w) uint32, the smallest cell index y * w + x of the cell's region; id
        (h, w) uint32, the rank of that label, 0 .. regions - 1; both REGIONS_NONE where the cell is no member; regions: a structured
        array (REGION_DTYPE) of the first min(regions, region_cap) records in id order (region_cap None: every region, w * h records of
        room); stats: bt_regions_stats as a dict.  label / id False: that plane is not copied out and None comes back in its place.
        bake: (attachment, channel, min_area, max_area, value) or a dict of those names: byte `channel` of that Rgba8 attachment becomes
        `value` on the members whose region's area lies in [min_area, max_area], and the atlas is updated as by write_region; a fifth
        element, the changed tiles, is then returned as well, and stats["edit"] is its bt_edit_stats.  Ordered behind the queued work;
        synchronous; a read without `bake`."""
        lod = self.lod_count - 1 if lod is None else lod
        flags = (_ffi.REGIONS_INVERT if invert else 0) | (_ffi.REGIONS_EIGHT if eight else 0) | (_ffi.REGIONS_FROM_TEXELS if lo is not None or hi is not None else 0)
        formats = self.config.attachments
        top = 255 if attachment_index < len(formats) and formats[attachment_index].format == AttachmentFormat.Rgba8 else 65535
        rule_c = _ffi.RegionsRuleC(channel, 0 if lo is None else lo, (top if flags & _ffi.REGIONS_FROM_TEXELS else 0) if hi is None else hi, max_step, flags)
        plane = None
        if members is not None:
            plane = np.ascontiguousarray(members, dtype=np.uint8)
            if plane.shape != (h, w):
                raise ValueError(f"label_regions: a members plane of shape {plane.shape} for a window of {(h, w)}")
        bake_c = None
        if bake is not None:
            if isinstance(bake, dict):
                bake = (bake["attachment"], bake["channel"], bake.get("min_area", 0), bake.get("max_area", 0xFFFFFFFF), bake["value"])
            bake_c = _ffi.RegionsBakeC(*bake, 0)
        outs = [np.zeros((h, w), dtype=np.uint32) if want else None for want in (label, id)]
        region_cap = w * h if region_cap is None else region_cap
        table = np.zeros(region_cap, dtype=self.REGION_DTYPE)
        cap = max(self.atlas_size, 1)
        changed = (_ffi.TileCoordinateC * cap)()
        stats = _ffi.RegionsStatsC()
        _ffi.check(_ffi.lib().bt_atlas_label_regions(
            self._h, attachment_index, side, lod, x0, y0, w, h, C.byref(rule_c), plane.ctypes.data_as(C.POINTER(C.c_uint8)) if plane is not None else None,
            *[o.ctypes.data_as(C.POINTER(C.c_uint32)) if o is not None else None for o in outs], table.ctypes.data_as(C.POINTER(_ffi.RegionC)) if region_cap else None,
            region_cap, C.byref(bake_c) if bake_c is not None else None, changed, cap, C.byref(stats)))
        out = {name: getattr(stats, name) for name, _ in _ffi.RegionsStatsC._fields_ if name not in ("edit", "_padding")}
        out["edit"] = {name: getattr(stats.edit, name) for name, _ in _ffi.EditStatsC._fields_}
        result = (*outs, table[:stats.regions_written].copy() if region_cap > stats.regions_written else table, out)
        if bake_c is None:
            return result
        return (*result, [TileCoordinate._from_c(changed[i]) for i in range(min(stats.edit.changed_count, cap))])

    @staticmethod
    def sun_directions(azimuth_deg, elevation_deg, cell_size: float, raw_unit: float, resolution: int = 64):
        """Real sun angles -> the (dx, dy, sun_num, sun_den) rows of `skyline`, an (N, 4) int64 array.  azimuth_deg and elevation_deg:
        scalars or equally long sequences.  Azimuth 0 is +x and turns towards +y.  cell_size: the width of a cell and raw_unit: the height of
        one raw unit, in the same world unit.  The rounding: (dx, dy) = floor(resolution * (cos, sin) + 0.5), so the azimuth is met within
        about 0.5 / resolution radians (resolution <= 1024); the sun's rise per step of the major axis,
        tan(elevation) * cell_size * hypot(dx, dy) / max(|dx|, |dy|) / raw_unit, is taken as a floor over sun_den = 4096 (a product within
        2^-40 of a whole number counts as that number), so the sun stands at most 1/4096 of a raw unit per step lower than asked and no
        cell is lit that the real sun leaves in shadow on these lines; it is capped at 2^31 - 1 (an elevation of 90 and near it).
        Elevations below 0 are refused: suns below the horizontal are out of scope."""
        az, el = np.atleast_1d(np.asarray(azimuth_deg, dtype=np.float64)), np.atleast_1d(np.asarray(elevation_deg, dtype=np.float64))
        az, el = np.broadcast_arrays(az, el)
        if not 1 <= resolution <= _ffi.SKYLINE_MAX_COMPONENT:
            raise ValueError(f"sun_directions: resolution {resolution}, 1 to {_ffi.SKYLINE_MAX_COMPONENT}")
        if (el < 0).any() or (el > 90).any() or not (cell_size > 0 and raw_unit > 0):
            raise ValueError("sun_directions: elevations in [0, 90], cell_size and raw_unit above 0")
        rows = np.zeros((len(az), 4), dtype=np.int64)
        for i, (a, e) in enumerate(zip(az.tolist(), el.tolist())):
            dx, dy = math.floor(resolution * math.cos(math.radians(a)) + 0.5), math.floor(resolution * math.sin(math.radians(a)) + 0.5)
            per_step = cell_size * math.hypot(dx, dy) / max(abs(dx), abs(dy)) / raw_unit
            num = (1 << 31) - 1 if e >= 90.0 else min((1 << 31) - 1, math.floor(math.tan(math.radians(e)) * per_step * 4096.0 * (1.0 + 2.0 ** -40)))
            rows[i] = (dx, dy, num, 4096)
        return rows

    def skyline(self, attachment_index: int, x0: int, y0: int, w: int, h: int, directions, *, lod: Optional[int] = None, side: int = 0,
                steps: bool = True, rise: bool = True, mask: bool = True, count: bool = True, bake=None):
        """bt_atlas_skyline: the horizon of every cell of the w x h window of centre texels at mosaic position (x0, y0) of `lod` on `side`
        of an R16 attachment in each of `directions`, by the header's SKYLINE section, in integers.  directions: an (N, 4) integer array or
        a list of (dx, dy, sun_num, sun_den) (see sun_directions; shorter tuples: sun_num 0, sun_den 1, a sun on the horizontal), 64 at
        most.  Returns (steps, rise, mask, count, stats): steps (N, h, w) uint16 and rise (N, h, w) int32, the distance in steps of the
        major axis and the height difference of each cell's horizon cell towards (dx, dy) (0 and 0 at the window's edge); mask (h, w)
        uint64, bit k set where the cell is lit by direction k (rise * sun_den <= steps * sun_num); count (h, w) uint8, the set bits;
        stats: bt_skyline_stats as a dict.  steps / rise / mask / count False: that plane is not copied out and None comes back in its
        place.  bake: (attachment, channel) or (attachment, channel, shade) or a dict of those names: byte `channel` of that Rgba8
        attachment becomes floor(255 * count / N) over the window, 255 minus that with `shade`, and the atlas is updated as by
        write_region; stats["edit"] is then its bt_edit_stats and stats["changed"] the changed tiles.  All planes are exact.  Ordered behind
        the queued work; synchronous; a read without `bake`."""
        lod = self.lod_count - 1 if lod is None else lod
        rows = [tuple(int(v) for v in d) for d in (directions.tolist() if isinstance(directions, np.ndarray) else directions)]
        arr = (_ffi.SkylineDirectionC * max(len(rows), 1))(*[_ffi.SkylineDirectionC(*(d + (0, 1)[len(d) - 2:])[:4]) for d in rows])
        n = len(rows)
        shapes = (((n, h, w), np.uint16, steps), ((n, h, w), np.int32, rise), ((h, w), np.uint64, mask), ((h, w), np.uint8, count))
        outs = [np.zeros(shape, dtype=t) if want else None for shape, t, want in shapes]
        types = (C.c_uint16, C.c_int32, C.c_uint64, C.c_uint8)
        bake_c = None
        if bake is not None:
            if isinstance(bake, dict):
                bake = (bake["attachment"], bake["channel"], bake.get("shade", False))
            bake = tuple(bake) + (False,) * (3 - len(bake))
            bake_c = _ffi.SkylineBakeC(bake[0], bake[1], _ffi.SKYLINE_BAKE_SHADE if bake[2] else 0, 0)
        cap = max(self.atlas_size, 1)
        changed = (_ffi.TileCoordinateC * cap)()
        stats = _ffi.SkylineStatsC()
        _ffi.check(_ffi.lib().bt_atlas_skyline(
            self._h, attachment_index, side, lod, x0, y0, w, h, arr, n, *[o.ctypes.data_as(C.POINTER(t)) if o is not None else None for o, t in zip(outs, types)],
            C.byref(bake_c) if bake_c is not None else None, changed, cap, C.byref(stats)))
        out = {name: getattr(stats, name) for name, _ in _ffi.SkylineStatsC._fields_ if name != "edit"}
        out["edit"] = {name: getattr(stats.edit, name) for name, _ in _ffi.EditStatsC._fields_}
        out["changed"] = [TileCoordinate._from_c(changed[i]) for i in range(min(stats.edit.changed_count, cap))]
        return (*outs, out)

    _SHAPE_OPS = {"set": _ffi.SHAPE_SET, "max": _ffi.SHAPE_MAX, "min": _ffi.SHAPE_MIN, "add": _ffi.SHAPE_ADD, "sub": _ffi.SHAPE_SUB}

    @staticmethod
    def pack_shapes(shapes, fixed: bool = False):
        """Python shapes -> (vertices, entries) as bt_atlas_rasterize_shapes takes them: an (N, 2) int32 array and an (E, 8) uint32 array
        in the field order of bt_shape.  A shape is a dict.  {"polygon": ring or [outer, hole, ...], "nonzero": False, "op": "set",
        "value": 1}: a ring is a list of (x, y); every ring becomes one contour, linked by BT_SHAPE_MORE.  {"stroke": [(x, y), ...],
        "half_width": r, "closed": False, "op": "set", "value": 1}.  op: "set", "max", "min", "add", "sub" or the BT_SHAPE_* number.
        Coordinates and half_width are floats in cells relative to the window's origin, a texel's centre being the integer itself.  THE
        ROUNDING, made once, here: v -> floor(256 v + 0.5), to the nearest 1/256 cell, a half upwards; from then on everything is exact.
        fixed=True: the numbers are already integers in 1/256 cell and are taken as they are."""
        q = (lambda v: int(v)) if fixed else (lambda v: int(math.floor(float(v) * 256.0 + 0.5)))
        vertices, entries = [], []
        for s in shapes:
            op = s.get("op", "set")
            op = TileAtlas._SHAPE_OPS[op] if isinstance(op, str) else int(op)
            value = int(s.get("value", 1))
            if "polygon" in s:
                rings = s["polygon"]
                if len(rings) and not isinstance(rings[0][0], (tuple, list, np.ndarray)):
                    rings = [rings]
                for i, ring in enumerate(rings):
                    flags = (_ffi.SHAPE_NONZERO if s.get("nonzero") else 0) | (_ffi.SHAPE_MORE if i + 1 < len(rings) else 0)
                    entries.append((_ffi.SHAPE_POLYGON, flags, len(vertices), len(ring), 0, op, value, 0))
                    vertices += [(q(x), q(y)) for x, y in ring]
            else:
                points = s["stroke"]
                entries.append((_ffi.SHAPE_STROKE, _ffi.SHAPE_CLOSED if s.get("closed") else 0, len(vertices), len(points), q(s.get("half_width", 0)), op, value, 0))
                vertices += [(q(x), q(y)) for x, y in points]
        return np.array(vertices, dtype=np.int32).reshape(-1, 2), np.array(entries, dtype=np.uint32).reshape(-1, 8)

    @staticmethod
    def check_shapes(vertices: np.ndarray, entries: np.ndarray, w: int, h: int):
        """bt_shapes_check, without a device: (boxes, shapes) of a packed list for a w x h window, boxes an (shapes, 4) uint16 array of
        (x_lo, y_lo, x_hi, y_hi) in cells, (1, 1, 0, 0) for an empty one.  A list that breaks a rule raises BtError naming the entry."""
        vertices, entries = np.ascontiguousarray(vertices, dtype=np.int32), np.ascontiguousarray(entries, dtype=np.uint32)
        boxes = np.zeros((max(len(entries), 1), 4), dtype=np.uint16)
        count = C.c_uint32()
        _ffi.check(_ffi.lib().bt_shapes_check(vertices.ctypes.data_as(C.POINTER(_ffi.ShapeVertexC)), len(vertices), entries.ctypes.data_as(C.POINTER(_ffi.ShapeC)),
                                              len(entries), w, h, boxes.ctypes.data_as(C.POINTER(_ffi.ShapeBoxC)), C.byref(count), None))
        return boxes[:count.value].copy(), count.value

    def rasterize_shapes(self, attachment_index: int, x0: int, y0: int, w: int, h: int, shapes, *, channel: int = 0, lod: Optional[int] = None, side: int = 0,
                         dry_run: bool = False, fixed: bool = False, count: bool = True, last: bool = True):
        """bt_atlas_rasterize_shapes: polygons (with holes) and strokes rasterised into the w x h window of centre texels at mosaic position
        (x0, y0) of `lod` on `side` of an R16 or Rgba8 attachment (byte `channel` of an Rgba8 texel), by the header's SHAPES section, in
        integers.  shapes: a list of dicts as pack_shapes takes them (floats in cells, rounded once to 1/256 cell; fixed=True: integers in
        1/256 cell), or a (vertices, entries) pair packed already.  Every shape that covers a cell folds its op and value into the texel in
        list order; the written rectangle is the union of the shapes' boxes, and the atlas is updated as by write_region of it.  Returns
        (count, last, stats): count (h, w) uint8, the shapes that cover each cell, capped at 255; last (h, w) uint16, the last of them,
        SHAPES_NONE where none does; stats: bt_shapes_stats as a dict, "box" as (x_lo, y_lo, x_hi, y_hi), "edit" the bt_edit_stats of the
        write-back and "changed" the changed tiles.  count / last False: that plane is not copied out and None comes back.  dry_run: the
        planes and the counts only; nothing is written.  Ordered behind the queued work; synchronous."""
        lod = self.lod_count - 1 if lod is None else lod
        vertices, entries = shapes if isinstance(shapes, tuple) else self.pack_shapes(shapes, fixed)
        vertices, entries = np.ascontiguousarray(vertices, dtype=np.int32), np.ascontiguousarray(entries, dtype=np.uint32)
        outs = [np.zeros((h, w), dtype=t) if want else None for t, want in ((np.uint8, count), (np.uint16, last))]
        cap = max(self.atlas_size, 1)
        changed = (_ffi.TileCoordinateC * cap)()
        stats = _ffi.ShapesStatsC()
        _ffi.check(_ffi.lib().bt_atlas_rasterize_shapes(
            self._h, attachment_index, side, lod, x0, y0, w, h, channel, vertices.ctypes.data_as(C.POINTER(_ffi.ShapeVertexC)), len(vertices),
            entries.ctypes.data_as(C.POINTER(_ffi.ShapeC)), len(entries), _ffi.SHAPES_DRY_RUN if dry_run else 0,
            *[o.ctypes.data_as(C.POINTER(t)) if o is not None else None for o, t in zip(outs, (C.c_uint8, C.c_uint16))], changed, cap, C.byref(stats)))
        out = {name: getattr(stats, name) for name, _ in _ffi.ShapesStatsC._fields_ if name not in ("edit", "_padding", "box")}
        out["box"] = (stats.box.x_lo, stats.box.y_lo, stats.box.x_hi, stats.box.y_hi)
        out["edit"] = {name: getattr(stats.edit, name) for name, _ in _ffi.EditStatsC._fields_}
        out["changed"] = [TileCoordinate._from_c(changed[i]) for i in range(min(stats.edit.changed_count, cap))]
        return (*outs, out)

    def erode_height(self, attachment_index: int, x0: int, y0: int, w: int, h: int, params: "ErosionParams", weight: Optional[np.ndarray] = None,
                     water: Optional[np.ndarray] = None, sediment: Optional[np.ndarray] = None, lod: Optional[int] = None, side: int = 0):
        """bt_atlas_erode_height: hydraulic erosion.  Runs params.steps steps of the simulation the header's EROSION section defines over the
        w x h window of centre texels at mosaic position (x0, y0) of `lod` on `side` of an R16 attachment (texels without data, tiles the
        atlas does not hold and the window's edge are walls), blends the new heights over the old ones by the optional (h, w) uint8 `weight`
        plane (255: all of the change, 0: the texel is kept), writes them back and restores the ancestors, the aprons and the mips as
        write_region does.  `water` / `sediment`: optional (h, w) float32 planes (finite, >= 0) the simulation starts from; where given, the
        plane after the last step comes back and the call is synchronous, otherwise it starts from 0 and the call only enqueues.  Fluxes
        start at 0 in every call.  Returns (changed, stats, water, sediment): changed tiles as write_region lists them, bt_erosion_stats as a
        dict (its "edit" entry: the bt_edit_stats of the write-back), and the two planes (None where none was given)."""
        lod = self.lod_count - 1 if lod is None else lod

        def plane(array, dtype, name):
            if array is None:
                return None
            array = np.array(array, dtype=dtype, order="C")  # a copy: the call writes into it
            if array.shape != (h, w):
                raise ValueError(f"erode_height: a {name} plane of shape {array.shape} for a window of {(h, w)}")
            return array

        weight_c, water_c, sediment_c = plane(weight, np.uint8, "weight"), plane(water, np.float32, "water"), plane(sediment, np.float32, "sediment")
        cap = max(self.atlas_size, 1)
        changed = (_ffi.TileCoordinateC * cap)()
        stats = _ffi.ErosionStatsC()
        params_c = params._c()
        _ffi.check(_ffi.lib().bt_atlas_erode_height(
            self._h, attachment_index, side, lod, x0, y0, w, h, C.byref(params_c),
            weight_c.ctypes.data_as(C.POINTER(C.c_uint8)) if weight_c is not None else None,
            water_c.ctypes.data_as(C.POINTER(C.c_float)) if water_c is not None else None,
            sediment_c.ctypes.data_as(C.POINTER(C.c_float)) if sediment_c is not None else None, changed, cap, C.byref(stats)))
        out = {name: getattr(stats, name) for name, _ in _ffi.ErosionStatsC._fields_ if name != "edit"}
        out["edit"] = {name: getattr(stats.edit, name) for name, _ in _ffi.EditStatsC._fields_}
        return [TileCoordinate._from_c(changed[i]) for i in range(min(stats.edit.changed_count, cap))], out, water_c, sediment_c

    def write_region(self, attachment_index: int, texels: np.ndarray, x0: int, y0: int, lod: Optional[int] = None, side: int = 0):
        """bt_atlas_write_region: copy `texels` ((h, w) uint16 for R16, (h, w, 4) uint8 for Rgba8; zeros allowed) verbatim over the centre
        texels at mosaic position (x0, y0) of `lod` on `side`, then propagate like edit_height.  Returns (changed, stats)."""
        lod = self.lod_count - 1 if lod is None else lod
        a = self.config.attachments[attachment_index]
        texels = np.ascontiguousarray(texels, dtype=texel_dtype(a.format))
        if texels.ndim != (2 if a.format == AttachmentFormat.R16 else 3):
            raise ValueError(f"write_region: texels of shape {texels.shape} for a {a.format.name} attachment")
        h, w = texels.shape[:2]
        return self._edit_result(lambda changed, cap, stats: _ffi.lib().bt_atlas_write_region(
            self._h, attachment_index, side, lod, x0, y0, w, h, texels.ctypes.data_as(C.c_void_p), 0, changed, cap, stats))

    def save_tiles(self, attachment_index: int, directory: str, coords):
        """bt_atlas_save_tiles: "{directory}/{coord}.bin" of the listed tiles only (the `changed` list of an edit)."""
        coords = list(coords)
        arr = (_ffi.TileCoordinateC * max(len(coords), 1))(*[c._c() for c in coords])
        _ffi.check(_ffi.lib().bt_atlas_save_tiles(self._h, attachment_index, directory.encode(), arr, len(coords)))

    # --- packed tiles (the header's PACKED TILES section)
    def pack_tiles(self, attachment_index: int, layers, sizes_only: bool = False, capacity: Optional[int] = None) -> Tuple[bytes, np.ndarray]:
        """bt_atlas_pack_tiles: the listed layers (any order, repeats allowed) encoded on the device.  Returns (bytes, offsets): stream i is
        bytes[offsets[i]:offsets[i + 1]].  sizes_only: dst_host = NULL, bytes is empty.  capacity: the size of the buffer handed over (a
        sizing call sets it otherwise); one that is too small raises BtError (BT_ERR_OVERFLOW) whose `offsets` attribute is filled."""
        layers = np.ascontiguousarray(layers, dtype=np.uint32)
        n = len(layers)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        lp, op = layers.ctypes.data_as(C.POINTER(C.c_uint32)), offsets.ctypes.data_as(C.POINTER(C.c_uint64))
        if sizes_only or capacity is None:
            _ffi.check(_ffi.lib().bt_atlas_pack_tiles(self._h, attachment_index, lp, n, None, 0, op))
            if sizes_only:
                return b"", offsets
            capacity = int(offsets[n])
        out = np.zeros(max(capacity, 1), dtype=np.uint8)
        try:
            _ffi.check(_ffi.lib().bt_atlas_pack_tiles(self._h, attachment_index, lp, n, out.ctypes.data_as(C.c_void_p), capacity, op))
        except _ffi.BtError as e:
            e.offsets = offsets
            raise
        return out[:int(offsets[n])].tobytes(), offsets

    def unpack_tiles(self, attachment_index: int, layers, data, offsets):
        """bt_atlas_unpack_tiles: stream i = data[offsets[i]:offsets[i + 1]] decoded on the device into layers[i], then the mip levels."""
        layers = np.ascontiguousarray(layers, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if len(offsets) != len(layers) + 1:
            raise ValueError(f"unpack_tiles: {len(layers)} layers need {len(layers) + 1} offsets, not {len(offsets)}")
        buf = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)  # (never an empty buffer)
        if len(layers) and int(offsets.max()) > len(buf) - 1:
            raise ValueError("unpack_tiles: offsets past the end of data")
        _ffi.check(_ffi.lib().bt_atlas_unpack_tiles(self._h, attachment_index, layers.ctypes.data_as(C.POINTER(C.c_uint32)), len(layers),
                                                    buf.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.POINTER(C.c_uint64))))
        return self

    def _packed_files(self, fn, attachment_index, directory, coords):
        if coords is None:
            _ffi.check(fn(self._h, attachment_index, directory.encode(), None, 0))
        else:
            coords = list(coords)
            arr = (_ffi.TileCoordinateC * max(len(coords), 1))(*[c._c() for c in coords])
            _ffi.check(fn(self._h, attachment_index, directory.encode(), arr, len(coords)))
        return self

    def save_tiles_packed(self, attachment_index: int, directory: str, coords=None):
        """bt_atlas_save_tiles_packed: "{directory}/{coord}.btp" of the listed tiles; coords=None: every existing tile."""
        return self._packed_files(_ffi.lib().bt_atlas_save_tiles_packed, attachment_index, directory, coords)

    def load_tiles_packed(self, attachment_index: int, directory: str, coords=None):
        """bt_atlas_load_tiles_packed: load_tiles for "{directory}/{coord}.btp", decoded on the device; coords=None: every tile of the
        loaded tile config."""
        return self._packed_files(_ffi.lib().bt_atlas_load_tiles_packed, attachment_index, directory, coords)

    def set_tile_files(self, packed: bool):
        """bt_atlas_set_tile_files: update() reads "{coord}.btp" (packed=True) or "{coord}.bin" (the default)."""
        _ffi.check(_ffi.lib().bt_atlas_set_tile_files(self._h, _ffi.TILE_FILES_PACKED if packed else _ffi.TILE_FILES_BIN))
        return self

    def close(self):
        if getattr(self, "_h", None):
            if device_open(getattr(self, "device", None)):
                _ffi.lib().bt_atlas_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HeightBounds:
    """bt_height_bounds: the min/max height table of the culling test — one raw unorm16 {min, max} pair per quadtree tile of LODs
    0 .. levels-1, on the device.  Level l follows level l-1; inside a level entry ((side * n + y) * n + x), n = 1 << l."""

    def __init__(self, device: Device, sides: int, levels: int):
        self.device, self.sides, self.levels = device, sides, levels
        self._h = None
        h = C.c_void_p()
        _ffi.check(_ffi.lib().bt_height_bounds_create(device._h, sides, levels, C.byref(h)))
        self._h = h
        self.entries = sides * (4 ** levels - 1) // 3

    def level_offset(self, level: int) -> int:
        return self.sides * (4 ** level - 1) // 3

    def build(self, atlas: "TileAtlas", attachment_index: int = 0) -> "HeightBounds":
        """from every tile `atlas` holds with lod < levels: the min / max of its whole layer; a missing tile takes its parent's, a
        missing root the whole range; every entry is then united with its children's"""
        _ffi.check(_ffi.lib().bt_height_bounds_build(self._h, atlas._h, attachment_index))
        return self

    def update(self, atlas: "TileAtlas", tiles, attachment_index: int = 0) -> dict:
        """bt_height_bounds_update: bring the table, last built or updated against `atlas`, up to date after `tiles` changed (in content
        or in being held) — the `changed` list of TileAtlas.edit_height / write_region as it is, or tiles just loaded or dropped.  The
        result is what build() would give; queued on the device's stream behind the edit, without synchronising.  Returns
        bt_bounds_update_stats as a dict."""
        tiles = list(tiles)
        arr = (_ffi.TileCoordinateC * max(len(tiles), 1))(*[c._c() for c in tiles])
        stats = _ffi.BoundsUpdateStatsC()
        _ffi.check(_ffi.lib().bt_height_bounds_update(self._h, atlas._h, attachment_index, arr, len(tiles), C.byref(stats)))
        return {name: getattr(stats, name) for name, _ in _ffi.BoundsUpdateStatsC._fields_ if name != "_pad"}

    def read(self) -> np.ndarray:
        """(entries, 2) uint16: [:, 0] = min, [:, 1] = max"""
        out = np.empty((self.entries, 2), dtype=np.uint16)
        _ffi.check(_ffi.lib().bt_height_bounds_read(self._h, out.ctypes.data_as(C.POINTER(C.c_uint16)), out.nbytes))
        return out

    def write(self, table: np.ndarray):
        table = np.ascontiguousarray(table, dtype=np.uint16)
        _ffi.check(_ffi.lib().bt_height_bounds_write(self._h, table.ctypes.data_as(C.POINTER(C.c_uint16)), table.nbytes))

    def close(self):
        if getattr(self, "_h", None):
            if device_open(getattr(self, "device", None)):
                _ffi.lib().bt_height_bounds_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def generate_mipmaps(device: Device, fmt: AttachmentFormat, level0: np.ndarray, mip_level_count: int) -> np.ndarray:
    """AttachmentData::generate_mipmaps (terrain_data/mod.rs:143-219) on the GPU: all levels concatenated."""
    T = level0.shape[0]
    ch = 1 if fmt == AttachmentFormat.R16 else 4
    total = sum((T >> k) ** 2 for k in range(mip_level_count)) * ch
    level0 = np.ascontiguousarray(level0)
    out = np.empty(total, dtype=texel_dtype(fmt))
    _ffi.check(_ffi.lib().bt_generate_mipmaps(device._h, fmt.id(), T, mip_level_count, level0.ctypes.data_as(C.c_void_p),
                                              out.ctypes.data_as(C.c_void_p), out.nbytes))
    return out


def packed_tile_bound(fmt: AttachmentFormat, texture_size: int) -> int:
    """bt_packed_tile_bound: the largest packed stream of a texture_size^2 tile of `fmt` (needs no device)."""
    out = C.c_uint64()
    _ffi.check(_ffi.lib().bt_packed_tile_bound(fmt.id(), texture_size, C.byref(out)))
    return out.value


def packed_tile_check(data) -> Tuple[AttachmentFormat, int]:
    """bt_packed_tile_check: (format, texture_size) of a valid packed stream; raises BtError naming the first violated rule (needs no device)."""
    data = bytes(data)
    fmt, size = C.c_uint32(), C.c_uint32()
    _ffi.check(_ffi.lib().bt_packed_tile_check(C.c_char_p(data), len(data), C.byref(fmt), C.byref(size)))
    return next(f for f in AttachmentFormat if f.id() == fmt.value), size.value


def tc_encode(coords: List[TileCoordinate]) -> bytes:
    arr = (_ffi.TileCoordinateC * max(len(coords), 1))(*[c._c() for c in coords])
    n = _ffi.lib().bt_tc_encode(arr, len(coords), None, 0)
    buf = (C.c_uint8 * n)()
    _ffi.lib().bt_tc_encode(arr, len(coords), buf, n)
    return bytes(buf)


def tc_decode(data: bytes) -> List[TileCoordinate]:
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    n = _ffi.lib().bt_tc_decode(buf, len(data), None, 0)
    if n < 0:
        raise ValueError("malformed tile config")
    out = (_ffi.TileCoordinateC * max(n, 1))()
    _ffi.lib().bt_tc_decode(buf, len(data), out, n)
    return [TileCoordinate._from_c(out[i]) for i in range(n)]
