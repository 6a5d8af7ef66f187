"""ctypes binding of libbevy_terrain_amd.so (the C ABI in include/bevy_terrain_amd.h).

The product path has no CPU fallback: if the HIP library is missing or fails to load this module
raises, loudly.  PyTorch (when installed) is imported first so that the library binds to the same
HIP runtime instance torch uses — device pointers and streams are then interchangeable.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbevy_terrain_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "bevy_terrain_amd.h")


def header_abi_version() -> int:
    """BT_ABI_VERSION as include/bevy_terrain_amd.h declares it: the one place the number is written."""
    import re
    try:
        with open(HEADER_PATH) as f:
            text = f.read()
    except OSError as e:  # a deployment without the sibling include/ directory: a load failure like any other
        raise ImportError(f"bevy_terrain_amd: {HEADER_PATH} (the C ABI's header, which names the ABI version this binding checks the "
                          f"library against) cannot be read: {e}") from e
    m = re.search(r"^#define\s+BT_ABI_VERSION\s+(\d+)u?\s*$", text, flags=re.M)
    if not m:
        raise ImportError(f"{HEADER_PATH}: BT_ABI_VERSION not found")
    return int(m.group(1))


def header_symbols() -> set:
    """Every bt_* function include/bevy_terrain_amd.h declares."""
    import re
    with open(HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(bt_[a-z0-9_]+)\s*\(", text))

INVALID_ATLAS_INDEX = 0xFFFFFFFF
MAX_ATTACHMENTS = 8

BT_OK = 0
RUN_AUTO, RUN_GENERIC, RUN_KEEP_QUEUE, RUN_PROFILE, RUN_SHARD_LOCAL, RUN_SHARD_FINISH, RUN_SHARD_DISTRIBUTED, RUN_SHARD_EXCHANGE, RUN_SHARD_OVERLAP, RUN_REFERENCE_DISPATCH = 0, 1, 2, 4, 8, 16, 32, 64, 128, 256


class BtError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"bevy_terrain_amd: status {status}: {message}")
        self.status = status


class TileCoordinateC(C.Structure):
    _fields_ = [("side", C.c_uint32), ("lod", C.c_uint32), ("x", C.c_uint32), ("y", C.c_uint32)]


class AtlasTileC(C.Structure):
    _fields_ = [("coordinate", TileCoordinateC), ("atlas_index", C.c_uint32), ("_padding", C.c_uint32 * 3)]


class AttachmentConfigC(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("texture_size", C.c_uint32), ("border_size", C.c_uint32),
                ("mip_level_count", C.c_uint32), ("format", C.c_uint32)]


class TerrainConfigC(C.Structure):
    _fields_ = [("lod_count", C.c_uint32), ("atlas_size", C.c_uint32), ("spherical", C.c_uint32),
                ("attachment_count", C.c_uint32), ("attachments", AttachmentConfigC * MAX_ATTACHMENTS),
                ("path", C.c_char * 256)]


class RasterC(C.Structure):
    _fields_ = [("data", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("row_pitch", C.c_uint64),
                ("format", C.c_uint32), ("on_device", C.c_uint32)]


class ImageC(C.Structure):
    _fields_ = [("data", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_uint32),
                ("row_pitch", C.c_uint64)]


class PreprocessDatasetC(C.Structure):
    _fields_ = [("attachment_index", C.c_uint32), ("side", C.c_uint32), ("top_left", C.c_float * 2),
                ("bottom_right", C.c_float * 2), ("lod_begin", C.c_uint32), ("lod_end", C.c_uint32)]


class SphericalDatasetC(C.Structure):
    _fields_ = [("attachment_index", C.c_uint32), ("lod_begin", C.c_uint32), ("lod_end", C.c_uint32)]


class RunStatsC(C.Structure):
    _fields_ = [("kernel_launches", C.c_uint32), ("tiles", C.c_uint32), ("algorithmic_bytes", C.c_uint64),
                ("fused_jobs", C.c_uint32), ("generic_jobs", C.c_uint32), ("prev_zero_launches", C.c_uint32), ("variants", C.c_uint32)]


class ShardRangeC(C.Structure):
    _fields_ = [("attachment_index", C.c_uint32), ("side", C.c_uint32), ("lod", C.c_uint32), ("first_layer", C.c_uint32),
                ("layers_per_rank", C.c_uint32)]


class ShardPieceC(C.Structure):
    _fields_ = [("attachment_index", C.c_uint32), ("side", C.c_uint32), ("lod", C.c_uint32), ("first_layer", C.c_uint32),
                ("layers", C.c_uint32), ("owner_rank", C.c_uint32)]


class LaunchProfileC(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("tasks", C.c_uint32), ("algorithmic_bytes", C.c_uint64), ("avg_ms", C.c_float),
                ("samples", C.c_uint32)]


class SideParameterC(C.Structure):
    _fields_ = [("view_xy", C.c_int32 * 2), ("view_uv", C.c_float * 2)]


class ViewStateC(C.Structure):
    _fields_ = [("spherical", C.c_uint32), ("geometry_tile_count", C.c_uint32), ("refinement_count", C.c_uint32),
                ("vertices_per_tile", C.c_uint32), ("subdivision_distance", C.c_float), ("origin_lod", C.c_uint32),
                ("approximate_height", C.c_float), ("sides", SideParameterC * 6), ("world_position", C.c_float * 3),
                ("world_from_local", C.c_float * 12), ("local_from_world_transpose", C.c_float * 9)]


class IndirectC(C.Structure):
    _fields_ = [("vertex_count", C.c_uint32), ("instance_count", C.c_uint32), ("base_vertex", C.c_uint32),
                ("base_instance", C.c_uint32)]


class FrameInfoC(C.Structure):
    _fields_ = [("released_count", C.c_uint32), ("requested_count", C.c_uint32), ("apply_status", C.c_int32), ("approximate_height", C.c_float)]


FRAME_PREPASS_UNORDERED, FRAME_PREPASS_PLAIN, FRAME_KEEP_REQUESTS, FRAME_KEEP_HEIGHT = 1, 2, 4, 8
BOUNDS_SKIP_ZERO, BOUNDS_MAX_GRID = 1, 64


RAY_MISS, RAY_HIT, RAY_INSIDE, RAY_INVALID = 0, 1, 2, 3
RAYCAST_MAX_STEPS, RAYCAST_MAX_REFINE_ROUNDS, RAYCAST_MAX_SAMPLES = 65536, 4, 1 << 24


class RayC(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("direction", C.c_double * 3), ("t_min", C.c_double), ("t_max", C.c_double)]


class RayHitC(C.Structure):
    _fields_ = [("status", C.c_uint32), ("step", C.c_uint32), ("t", C.c_double), ("t_above", C.c_double), ("position", C.c_double * 3),
                ("height", C.c_float), ("_padding", C.c_uint32)]


CONTACT_NONE, CONTACT_TOUCHING, CONTACT_BELOW, CONTACT_INVALID, CONTACT_FAR = 0, 1, 2, 3, 4
COLLIDE_MAX_REFINE_ROUNDS, COLLIDE_MAX_SAMPLES, SWEEP_MAX_STEPS, SWEEP_MAX_BISECTIONS = 6, 1 << 24, 4096, 32


class SphereC(C.Structure):
    _fields_ = [("center", C.c_double * 3), ("radius", C.c_double)]


class SphereContactC(C.Structure):
    _fields_ = [("status", C.c_uint32), ("candidate", C.c_uint32), ("distance", C.c_double), ("depth", C.c_double), ("point", C.c_double * 3),
                ("normal", C.c_double * 3), ("height", C.c_float), ("_padding", C.c_uint32)]


class SphereSweepC(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("direction", C.c_double * 3), ("radius", C.c_double), ("t_min", C.c_double), ("t_max", C.c_double)]


class SweepHitC(C.Structure):
    _fields_ = [("status", C.c_uint32), ("step", C.c_uint32), ("t", C.c_double), ("t_above", C.c_double), ("contact", SphereContactC)]


RENDER_ORTHOGRAPHIC, RENDER_LIGHTING = 1, 2
RENDER_MAX_STEPS, RENDER_MAX_PIXELS, RENDER_NO_ALBEDO = 4096, 1 << 24, 0xFFFFFFFF


class RenderCameraC(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("forward", C.c_double * 3), ("right", C.c_double * 3), ("up", C.c_double * 3), ("t_min", C.c_double),
                ("t_max", C.c_double), ("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32), ("albedo_attachment", C.c_uint32),
                ("sun", C.c_float * 3), ("ambient", C.c_float), ("background", C.c_uint8 * 4), ("_padding", C.c_uint32)]


class RenderStatsC(C.Structure):
    _fields_ = [("launches", C.c_uint32), ("hit_pixels", C.c_uint32), ("inside_pixels", C.c_uint32), ("miss_pixels", C.c_uint32)]


OCCLUSION_MAX_RAYS, SHADOW_NONE = 1 << 24, 255


class OcclusionStatsC(C.Structure):
    _fields_ = [("launches", C.c_uint32), ("lit", C.c_uint32), ("occluded", C.c_uint32), ("invalid", C.c_uint32)]


class SunShadowC(C.Structure):
    _fields_ = [("lift", C.c_double), ("distance", C.c_double), ("steps", C.c_uint32), ("_padding", C.c_uint32)]


GEOMETRY_GRID, GEOMETRY_NO_MORPH, GEOMETRY_NO_BLEND = 1, 2, 4
GEOMETRY_MAX_GRID = 32
GEOMETRY_VIEW_RELATIVE = 8  # the _hp calls only


class TerrainVertexC(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("height", C.c_float), ("normal", C.c_float * 3), ("tile_index", C.c_uint32),
                ("coordinate_uv", C.c_float * 2), ("view_distance", C.c_float), ("blend_ratio", C.c_float)]


class SideCoefficientsC(C.Structure):
    _fields_ = [("c", C.c_float * 3), ("c_s", C.c_float * 3), ("c_t", C.c_float * 3), ("c_ss", C.c_float * 3), ("c_st", C.c_float * 3),
                ("c_tt", C.c_float * 3)]


class ModelApproximationC(C.Structure):
    _fields_ = [("sides", SideCoefficientsC * 6), ("precision_threshold_distance", C.c_float), ("origin_lod", C.c_uint32), ("_padding", C.c_uint32 * 2)]


class CullViewC(C.Structure):
    _fields_ = [("planes", (C.c_float * 4) * 5), ("plane_count", C.c_uint32), ("margin", C.c_float), ("min_height", C.c_float),
                ("max_height", C.c_float)]


class HorizonViewC(C.Structure):
    _fields_ = [("eye", C.c_float * 3), ("vh", C.c_float), ("occluder_radius", C.c_float), ("margin", C.c_float)]


HEIGHT_BOUNDS_MAX_LEVELS = 11

EDIT_ADD, EDIT_FLATTEN = 0, 1
EDIT_FALLOFF_SMOOTH, EDIT_FALLOFF_HARD = 0, 1
EDIT_MAX_STAMPS = 256
SMOOTH_MAX_KERNEL = 4
PAINT_BLEND, PAINT_ADD = 0, 1


class EditStampC(C.Structure):
    _fields_ = [("side", C.c_uint32), ("mode", C.c_uint32), ("falloff", C.c_uint32), ("_pad", C.c_uint32), ("center", C.c_float * 2),
                ("radius", C.c_float), ("amount", C.c_float)]


class SmoothStampC(C.Structure):
    _fields_ = [("side", C.c_uint32), ("falloff", C.c_uint32), ("center", C.c_float * 2), ("radius", C.c_float), ("strength", C.c_float)]


class PaintStampC(C.Structure):
    _fields_ = [("side", C.c_uint32), ("mode", C.c_uint32), ("falloff", C.c_uint32), ("channel_mask", C.c_uint32), ("center", C.c_float * 2),
                ("radius", C.c_float), ("opacity", C.c_float), ("color", C.c_float * 4)]


SPLAT_WEIGHTS, SPLAT_COLOUR = 0, 1
SPLAT_MAX_RULES, SPLAT_MAX_WEIGHT_RULES = 8, 4


class SplatRuleC(C.Structure):
    _fields_ = [("height_lo", C.c_float), ("height_hi", C.c_float), ("height_fade", C.c_float), ("steep_lo", C.c_float), ("steep_hi", C.c_float),
                ("steep_fade", C.c_float), ("weight", C.c_float), ("colour", C.c_float * 3), ("_padding", C.c_uint32 * 2)]


SCATTER_MAX_RULES, SCATTER_NO_MASK = 8, 0xFFFFFFFF


class ScatterRuleC(C.Structure):
    _fields_ = [("height_lo", C.c_float), ("height_hi", C.c_float), ("height_fade", C.c_float), ("steep_lo", C.c_float), ("steep_hi", C.c_float),
                ("steep_fade", C.c_float), ("density", C.c_float), ("scale_lo", C.c_float), ("scale_hi", C.c_float), ("mask_channel", C.c_uint32),
                ("_padding", C.c_uint32 * 2)]


class ScatterInstanceC(C.Structure):
    _fields_ = [("position", C.c_double * 3), ("normal", C.c_float * 3), ("scale", C.c_float), ("yaw", C.c_float), ("rule", C.c_uint32),
                ("cell", C.c_uint32 * 2)]


class ScatterStatsC(C.Structure):
    _fields_ = [("total", C.c_uint64), ("written", C.c_uint64), ("cells", C.c_uint64), ("cells_no_data", C.c_uint64),
                ("per_rule", C.c_uint64 * SCATTER_MAX_RULES), ("launches", C.c_uint32), ("_padding", C.c_uint32)]


PATH_MAX_CELLS, PATH_MAX_GOALS = 1 << 22, 4096
PATH_GOAL, PATH_UNREACHABLE, PATH_BLOCKED = 8, 254, 255
PATH_TRACE_OK, PATH_TRACE_BLOCKED, PATH_TRACE_UNREACHABLE, PATH_TRACE_LOOP = 0, 1, 2, 3


class PathCostC(C.Structure):
    _fields_ = [("min_height", C.c_float), ("max_height", C.c_float), ("cell_size", C.c_float), ("max_grade", C.c_float),
                ("grade_weight", C.c_float), ("climb_weight", C.c_float), ("descend_weight", C.c_float), ("_padding", C.c_uint32)]


class PathGoalC(C.Structure):
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("cost0", C.c_float)]


class PathStatsC(C.Structure):
    _fields_ = [("cells", C.c_uint32), ("blocked", C.c_uint32), ("reachable", C.c_uint32), ("goals_used", C.c_uint32),
                ("goals_blocked", C.c_uint32), ("tiles_missing", C.c_uint32), ("sweeps", C.c_uint32), ("launches", C.c_uint32)]


class EditStatsC(C.Structure):
    _fields_ = [("tiles_edited", C.c_uint32), ("tiles_missing", C.c_uint32), ("tiles_with_children", C.c_uint32),
                ("tiles_downsampled", C.c_uint32), ("tiles_stitched", C.c_uint32), ("layers_mipped", C.c_uint32), ("launches", C.c_uint32),
                ("changed_count", C.c_uint32)]


ERODE_MAX_CELLS, ERODE_MAX_STEPS, ERODE_BLOCK = 1 << 22, 4096, 32


class ErosionParamsC(C.Structure):
    _fields_ = [("min_height", C.c_float), ("max_height", C.c_float), ("cell_size", C.c_float), ("dt", C.c_float), ("rain", C.c_float),
                ("evaporation", C.c_float), ("gravity", C.c_float), ("capacity", C.c_float), ("erode", C.c_float), ("deposit", C.c_float),
                ("min_tilt", C.c_float), ("min_depth", C.c_float), ("steps", C.c_uint32), ("_padding", C.c_uint32 * 3)]


DRAIN_MAX_CELLS, DRAIN_BLOCK = 1 << 22, 32
DRAIN_OUTLET, DRAIN_VOID = 8, 255


class DrainageStatsC(C.Structure):
    _fields_ = [("cells", C.c_uint32), ("voids", C.c_uint32), ("outlets", C.c_uint32), ("tiles_missing", C.c_uint32), ("filled", C.c_uint32), ("flats", C.c_uint32),
                ("max_flat_distance", C.c_uint32), ("max_accumulation", C.c_uint32), ("outflow", C.c_uint32), ("sweeps_fill", C.c_uint32),
                ("sweeps_flat", C.c_uint32), ("sweeps_accumulate", C.c_uint32), ("launches", C.c_uint32), ("_padding", C.c_uint32 * 3)]


VIEWSHED_NONE, VIEWSHED_MAX_OBSERVERS, VIEWSHED_MAX_SIDE, VIEWSHED_MAX_CELLS = 0xFFFFFFFF, 64, 32768, 1 << 22


class ViewshedObserverC(C.Structure):
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("eye_height", C.c_uint32), ("radius", C.c_uint32)]


class ViewshedStatsC(C.Structure):
    _fields_ = [("cells", C.c_uint32), ("voids", C.c_uint32), ("tiles_missing", C.c_uint32), ("observers_used", C.c_uint32), ("observers_skipped", C.c_uint32),
                ("covered", C.c_uint32), ("visible", C.c_uint32), ("max_clearance", C.c_uint32), ("samples", C.c_uint64), ("launches", C.c_uint32),
                ("_padding", C.c_uint32 * 5)]


DISTANCE_NONE, DISTANCE_MAX_SIDE, DISTANCE_MAX_CELLS, DISTANCE_BAND = 0xFFFFFFFF, 8192, 1 << 22, 32
DISTANCE_FROM_TEXELS, DISTANCE_INVERT, DISTANCE_BAKE_NEAR = 1, 2, 1
# bt_distance.hip: the threads of a workgroup (columns of a group of the column phase, the stride of a row's cells in the row phase) and the
# cells of a workgroup of the finish launch (kDistanceThreads, kDistanceThreads * kFinishCells); tests place windows around them
DISTANCE_THREADS, DISTANCE_FINISH_CELLS = 256, 1024


class DistanceSeedsC(C.Structure):
    _fields_ = [("channel", C.c_uint32), ("lo", C.c_uint32), ("hi", C.c_uint32), ("flags", C.c_uint32)]


class DistanceBakeC(C.Structure):
    _fields_ = [("attachment", C.c_uint32), ("channel", C.c_uint32), ("reach", C.c_uint32), ("flags", C.c_uint32)]


class DistanceStatsC(C.Structure):
    _fields_ = [("cells", C.c_uint32), ("seeds", C.c_uint32), ("tiles_missing", C.c_uint32), ("max_dist2", C.c_uint32), ("sum_dist2", C.c_uint64),
                ("launches", C.c_uint32), ("_padding", C.c_uint32), ("edit", EditStatsC)]


REGIONS_NONE, REGIONS_MAX_SIDE, REGIONS_MAX_CELLS = 0xFFFFFFFF, 8192, 1 << 22
REGIONS_FROM_TEXELS, REGIONS_INVERT, REGIONS_EIGHT = 1, 2, 4
# bt_regions.hip: the cells across a block of the local launch and the consecutive cells of a workgroup of the linear launches; tests place
# windows and scenes around them
REGIONS_BLOCK, REGIONS_CHUNK = 32, 1024


class RegionsRuleC(C.Structure):
    _fields_ = [("channel", C.c_uint32), ("lo", C.c_uint32), ("hi", C.c_uint32), ("max_step", C.c_uint32), ("flags", C.c_uint32)]


class RegionsBakeC(C.Structure):
    _fields_ = [("attachment", C.c_uint32), ("channel", C.c_uint32), ("min_area", C.c_uint32), ("max_area", C.c_uint32), ("value", C.c_uint32),
                ("flags", C.c_uint32)]


class RegionC(C.Structure):
    _fields_ = [("label", C.c_uint32), ("area", C.c_uint32), ("x_min", C.c_uint16), ("y_min", C.c_uint16), ("x_max", C.c_uint16), ("y_max", C.c_uint16),
                ("v_min", C.c_uint16), ("v_max", C.c_uint16), ("edges", C.c_uint32), ("v_sum", C.c_uint64)]


class RegionsStatsC(C.Structure):
    _fields_ = [("cells", C.c_uint32), ("members", C.c_uint32), ("regions", C.c_uint32), ("regions_written", C.c_uint32), ("largest_area", C.c_uint32),
                ("largest_label", C.c_uint32), ("tiles_missing", C.c_uint32), ("baked", C.c_uint32), ("launches", C.c_uint32), ("_padding", C.c_uint32 * 3),
                ("edit", EditStatsC)]


SKYLINE_MAX_DIRECTIONS, SKYLINE_MAX_COMPONENT, SKYLINE_MAX_SIDE, SKYLINE_MAX_CELLS = 64, 1024, 32768, 1 << 22
SKYLINE_STACK_BUDGET, SKYLINE_BAKE_SHADE = 256 << 20, 1


PACK_STRIP_ROWS, TILE_FILES_BIN, TILE_FILES_PACKED = 32, 0, 1


class SkylineDirectionC(C.Structure):
    _fields_ = [("dx", C.c_int32), ("dy", C.c_int32), ("sun_num", C.c_uint32), ("sun_den", C.c_uint32)]


class SkylineBakeC(C.Structure):
    _fields_ = [("attachment", C.c_uint32), ("channel", C.c_uint32), ("flags", C.c_uint32), ("_padding", C.c_uint32)]


class SkylineStatsC(C.Structure):
    _fields_ = [("cells", C.c_uint32), ("voids", C.c_uint32), ("tiles_missing", C.c_uint32), ("directions", C.c_uint32), ("lines", C.c_uint32),
                ("longest_line", C.c_uint32), ("max_steps", C.c_uint32), ("launches", C.c_uint32), ("lit", C.c_uint64), ("sum_steps", C.c_uint64),
                ("edit", EditStatsC)]


SHAPES_NONE, SHAPES_NO_ENTRY, SHAPES_MAX_SHAPES, SHAPES_MAX_ENTRIES, SHAPES_MAX_VERTICES = 0xFFFF, 0xFFFFFFFF, 4096, 65536, 1 << 20
SHAPES_MAX_COORD, SHAPES_MAX_HALF_WIDTH, SHAPES_MAX_SIDE, SHAPES_MAX_CELLS = 1 << 23, 1 << 20, 8192, 1 << 22
# bt_shapes.hip: the edges of a chunk of vertices in LDS and the cells of a workgroup's block; tests place contours and windows around them
SHAPES_CHUNK, SHAPES_BLOCK_W, SHAPES_BLOCK_H = 256, 64, 16
SHAPE_POLYGON, SHAPE_STROKE = 0, 1
SHAPE_NONZERO, SHAPE_CLOSED, SHAPE_MORE = 1, 2, 4
SHAPE_SET, SHAPE_MAX, SHAPE_MIN, SHAPE_ADD, SHAPE_SUB = 0, 1, 2, 3, 4
SHAPES_DRY_RUN = 1


class ShapeVertexC(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32)]


class ShapeC(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("flags", C.c_uint32), ("first_vertex", C.c_uint32), ("vertex_count", C.c_uint32), ("half_width", C.c_uint32),
                ("op", C.c_uint32), ("value", C.c_uint32), ("_pad", C.c_uint32)]


class ShapeBoxC(C.Structure):
    _fields_ = [("x_lo", C.c_uint16), ("y_lo", C.c_uint16), ("x_hi", C.c_uint16), ("y_hi", C.c_uint16)]


class ShapesStatsC(C.Structure):
    _fields_ = [("cells", C.c_uint32), ("shapes", C.c_uint32), ("shapes_culled", C.c_uint32), ("tiles_missing", C.c_uint32), ("covered", C.c_uint64),
                ("written", C.c_uint64), ("box", ShapeBoxC), ("launches", C.c_uint32), ("_padding", C.c_uint32), ("edit", EditStatsC)]


class ErosionStatsC(C.Structure):
    _fields_ = [("cells", C.c_uint32), ("tiles_missing", C.c_uint32), ("steps", C.c_uint32), ("sim_launches", C.c_uint32), ("edit", EditStatsC)]


class BoundsUpdateStatsC(C.Structure):
    _fields_ = [("tiles_listed", C.c_uint32), ("layers_reduced", C.c_uint32), ("launches", C.c_uint32), ("_pad", C.c_uint32),
                ("entries_written", C.c_uint64)]


class TileTreeEntryC(C.Structure):
    _fields_ = [("atlas_index", C.c_uint32), ("atlas_lod", C.c_uint32)]


class TerrainModelC(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("_padding", C.c_uint32), ("position", C.c_double * 3), ("a", C.c_double),
                ("b", C.c_double), ("min_height", C.c_float), ("max_height", C.c_float)]


class TerrainViewConfigC(C.Structure):
    _fields_ = [("tree_size", C.c_uint32), ("geometry_tile_count", C.c_uint32), ("refinement_count", C.c_uint32),
                ("grid_size", C.c_uint32), ("subdivision_tolerance", C.c_double),
                ("precision_threshold_distance", C.c_double), ("load_distance", C.c_double),
                ("morph_distance", C.c_double), ("blend_distance", C.c_double), ("morph_range", C.c_float),
                ("blend_range", C.c_float), ("origin_lod", C.c_uint32), ("_padding", C.c_uint32)]


_vp, _u32, _u64, _i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32
_P = C.POINTER

# name -> (restype, argtypes); every function include/bevy_terrain_amd.h declares
PROTOTYPES = {
    "bt_abi_version": (_u32, []),
    "bt_last_error": (C.c_char_p, []),
    "bt_ctx_create": (_i32, [_i32, _vp, _P(_vp)]),
    "bt_ctx_destroy": (None, [_vp]),
    "bt_ctx_set_stream": (_i32, [_vp, _vp]),
    "bt_ctx_stream": (_vp, [_vp]),
    "bt_ctx_synchronize": (_i32, [_vp]),
    "bt_ctx_trim": (_i32, [_vp, C.POINTER(C.c_uint64)]),
    "bt_ctx_set_io_threads": (_i32, [_vp, C.c_uint32]),
    "bt_ctx_io_threads": (C.c_uint32, [_vp]),
    "bt_ctx_timer_begin": (_i32, [_vp]),
    "bt_ctx_timer_end": (_i32, [_vp, _P(C.c_float)]),
    "bt_device_malloc": (_i32, [_vp, C.c_size_t, _P(_vp)]),
    "bt_device_free": (_i32, [_vp, _vp]),
    "bt_memcpy_h2d": (_i32, [_vp, _vp, _vp, C.c_size_t]),
    "bt_memcpy_d2h": (_i32, [_vp, _vp, _vp, C.c_size_t]),
    "bt_tile_children": (None, [TileCoordinateC, _P(TileCoordinateC)]),
    "bt_tile_neighbours": (None, [TileCoordinateC, _u32, _P(TileCoordinateC)]),
    "bt_tile_parent": (TileCoordinateC, [TileCoordinateC]),
    "bt_tile_name": (_i32, [TileCoordinateC, C.c_char_p, C.c_size_t]),
    "bt_atlas_create": (_i32, [_vp, _P(TerrainConfigC), _P(_vp)]),
    "bt_atlas_destroy": (None, [_vp]),
    "bt_atlas_get_tile": (_i32, [_vp, TileCoordinateC, _P(AtlasTileC)]),
    "bt_atlas_get_or_allocate_tile": (_i32, [_vp, TileCoordinateC, _P(AtlasTileC)]),
    "bt_atlas_request_tile": (_i32, [_vp, TileCoordinateC]),
    "bt_atlas_release_tile": (_i32, [_vp, TileCoordinateC]),
    "bt_atlas_get_best_tile": (_i32, [_vp, TileCoordinateC, _P(TileTreeEntryC)]),
    "bt_atlas_update": (_i32, [_vp, C.c_char_p, _u32, _P(_u32), _P(_u32)]),
    "bt_atlas_pending_loads": (_u32, [_vp]),
    "bt_atlas_tiles": (_u32, [_vp, _P(TileCoordinateC), _P(_u32), _u32]),
    "bt_atlas_attachment_storage": (_i32, [_vp, _u32, _P(_vp), _P(_u64), _P(_u32)]),
    "bt_atlas_download_tiles": (_i32, [_vp, _u32, _u32, _u32, _vp, _u64]),
    "bt_atlas_upload_tile": (_i32, [_vp, _u32, _u32, _vp, _u64]),
    "bt_atlas_save_attachment": (_i32, [_vp, _u32, C.c_char_p]),
    "bt_atlas_save_tile_config": (_i32, [_vp, C.c_char_p]),
    "bt_atlas_load_tile_config": (_i32, [_vp, C.c_char_p]),
    "bt_atlas_load_tiles": (_i32, [_vp, _u32, C.c_char_p, _vp, _u32]),
    "bt_atlas_sample": (_i32, [_vp, _u32, _vp, _u32, _vp]),
    "bt_atlas_tile_bounds": (_i32, [_vp, _u32, _P(_u32), _u32, _u32, _u32, _P(C.c_uint16), _u64]),
    "bt_atlas_edit_height": (_i32, [_vp, _u32, _u32, _P(EditStampC), _u32, _P(TileCoordinateC), _u32, _P(EditStatsC)]),
    "bt_atlas_smooth_height": (_i32, [_vp, _u32, _u32, _u32, _P(SmoothStampC), _u32, _P(TileCoordinateC), _u32, _P(EditStatsC)]),
    "bt_atlas_paint": (_i32, [_vp, _u32, _u32, _P(PaintStampC), _u32, _P(TileCoordinateC), _u32, _P(EditStatsC)]),
    "bt_atlas_splat_from_height": (_i32, [_vp, _u32, _u32, _P(TerrainModelC), _u32, _u32, _u32, _u32, _u32, _u32, _u32, _P(SplatRuleC), _u32, _P(C.c_uint8),
                                          _P(TileCoordinateC), _u32, _P(EditStatsC)]),
    "bt_atlas_scatter_instances": (_i32, [_vp, _u32, _u32, _P(TerrainModelC), _P(TileCoordinateC), _u32, _P(ScatterRuleC), _u32, _u32, C.c_float,
                                          _P(ScatterInstanceC), _u64, _P(_u64), _P(ScatterStatsC)]),
    "bt_atlas_read_region": (_i32, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _u64, _P(_u32)]),
    "bt_atlas_write_region": (_i32, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _u64, _P(TileCoordinateC), _u32, _P(EditStatsC)]),
    "bt_atlas_save_tiles": (_i32, [_vp, _u32, C.c_char_p, _P(TileCoordinateC), _u32]),
    "bt_atlas_path_field": (_i32, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _P(PathCostC), _P(PathGoalC), _u32, _P(C.c_uint8), _P(C.c_float),
                                   _P(C.c_uint8), _P(PathStatsC)]),
    "bt_atlas_erode_height": (_i32, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _P(ErosionParamsC), _P(C.c_uint8), _P(C.c_float), _P(C.c_float),
                                     _P(TileCoordinateC), _u32, _P(ErosionStatsC)]),
    "bt_atlas_drainage": (_i32, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _P(C.c_uint8), _P(C.c_uint8), _P(C.c_uint16), _P(_u32), _P(C.c_uint8), _P(_u32),
                                 _P(DrainageStatsC)]),
    "bt_atlas_viewshed": (_i32, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _P(ViewshedObserverC), _u32, _u32, _P(_u32), _P(C.c_uint8), _P(C.c_uint64),
                                 _P(ViewshedStatsC)]),
    "bt_atlas_distance_field": (_i32, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _P(DistanceSeedsC), _P(C.c_uint8), _P(_u32), _P(_u32), _P(DistanceBakeC),
                                       _P(TileCoordinateC), _u32, _P(DistanceStatsC)]),
    "bt_skyline_line_count": (_i32, [_u32, _u32, C.c_int32, C.c_int32, _P(_u32), _P(_u32)]),
    "bt_atlas_skyline": (_i32, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _P(SkylineDirectionC), _u32, _P(C.c_uint16), _P(C.c_int32), _P(C.c_uint64),
                                _P(C.c_uint8), _P(SkylineBakeC), _P(TileCoordinateC), _u32, _P(SkylineStatsC)]),
    "bt_shapes_check": (_i32, [_P(ShapeVertexC), _u32, _P(ShapeC), _u32, _u32, _u32, _P(ShapeBoxC), _P(_u32), _P(_u32)]),
    "bt_atlas_rasterize_shapes": (_i32, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _P(ShapeVertexC), _u32, _P(ShapeC), _u32, _u32, _P(C.c_uint8),
                                         _P(C.c_uint16), _P(TileCoordinateC), _u32, _P(ShapesStatsC)]),
    "bt_atlas_label_regions": (_i32, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _P(RegionsRuleC), _P(C.c_uint8), _P(_u32), _P(_u32), _P(RegionC), _u32,
                                      _P(RegionsBakeC), _P(TileCoordinateC), _u32, _P(RegionsStatsC)]),
    "bt_packed_tile_bound": (_i32, [_u32, _u32, _P(_u64)]),
    "bt_packed_tile_check": (_i32, [_vp, _u64, _P(_u32), _P(_u32)]),
    "bt_atlas_pack_tiles": (_i32, [_vp, _u32, _P(_u32), _u32, _vp, _u64, _P(_u64)]),
    "bt_atlas_unpack_tiles": (_i32, [_vp, _u32, _P(_u32), _u32, _vp, _P(_u64)]),
    "bt_atlas_save_tiles_packed": (_i32, [_vp, _u32, C.c_char_p, _P(TileCoordinateC), _u32]),
    "bt_atlas_load_tiles_packed": (_i32, [_vp, _u32, C.c_char_p, _P(TileCoordinateC), _u32]),
    "bt_atlas_set_tile_files": (_i32, [_vp, _u32]),
    "bt_path_trace": (_i32, [_P(C.c_uint8), _u32, _u32, _u32, _u32, _P(_u32), _u32, _P(_u32), _P(_u32)]),
    "bt_tc_encode": (_u64, [_P(TileCoordinateC), _u32, _vp, _u64]),
    "bt_tc_decode": (C.c_int64, [_vp, _u64, _P(TileCoordinateC), _u32]),
    "bt_generate_mipmaps": (_i32, [_vp, _u32, _u32, _u32, _vp, _vp, _u64]),
    "bt_atlas_generate_mipmaps": (_i32, [_vp, _u32, _u32, _u32]),
    "bt_atlas_mip_storage": (_i32, [_vp, _u32, _u32, _P(_vp), _P(_u64)]),
    "bt_image_load": (_i32, [C.c_char_p, _u32, _P(ImageC)]),
    "bt_image_decode": (_i32, [_vp, C.c_size_t, _u32, _P(ImageC)]),
    "bt_image_free": (None, [_P(ImageC)]),
    "bt_preprocessor_create": (_i32, [_vp, _P(_vp)]),
    "bt_preprocessor_destroy": (None, [_vp]),
    "bt_preprocessor_clear_attachment": (_i32, [_vp, _vp, _u32, C.c_char_p]),
    "bt_preprocessor_preprocess_tile": (_i32, [_vp, _vp, _P(PreprocessDatasetC), _P(RasterC)]),
    "bt_preprocessor_preprocess_spherical": (_i32, [_vp, _vp, _P(SphericalDatasetC), _P(RasterC)]),
    "bt_preprocessor_task_counts": (_u32, [_vp, _P(_u32)]),
    "bt_preprocessor_run": (_i32, [_vp, _vp, _u32]),
    "bt_preprocessor_save": (_i32, [_vp, _vp, C.c_char_p]),
    "bt_preprocessor_last_run_stats": (_i32, [_vp, _P(RunStatsC)]),
    "bt_preprocessor_set_shard": (_i32, [_vp, _u32, _u32]),
    "bt_preprocessor_shard_ranges": (_i32, [_vp, _P(ShardRangeC), _u32, _P(_u32)]),
    "bt_preprocessor_shard_pieces": (_i32, [_vp, _P(ShardPieceC), _u32, _P(_u32)]),
    "bt_comm_unique_id": (_i32, [_P(C.c_uint8)]),
    "bt_comm_create": (_i32, [_vp, _u32, _u32, _P(C.c_uint8), _P(_vp)]),
    "bt_comm_adopt": (_i32, [_vp, _vp, _u32, _u32, _P(_vp)]),
    "bt_comm_destroy": (None, [_vp]),
    "bt_comm_check": (_i32, [_vp]),
    "bt_comm_preflight": (_i32, [_vp, C.c_uint64, C.POINTER(C.c_float)]),
    "bt_preprocessor_run_sharded": (_i32, [_vp, _vp, _vp, _u32]),
    "bt_preprocessor_finish_sharded": (_i32, [_vp, _vp, _vp, _u32]),
    "bt_preprocessor_source_window": (_i32, [_vp, _vp, _u32, _u32, _P(C.c_uint32), _P(C.c_uint64)]),
    "bt_preprocessor_profile": (_i32, [_vp, _P(LaunchProfileC), _u32, _P(_u32)]),
    "bt_tiling_prepass_create": (_i32, [_vp, _u32, _P(_vp)]),
    "bt_tiling_prepass_destroy": (None, [_vp]),
    "bt_tiling_prepass_run": (_i32, [_vp, _P(ViewStateC)]),
    "bt_tiling_prepass_run_plain": (_i32, [_vp, _P(ViewStateC)]),
    "bt_tiling_prepass_run_unordered": (_i32, [_vp, _P(ViewStateC)]),
    "bt_tiling_prepass_set_window": (_i32, [_vp, _u32]),
    "bt_tiling_prepass_buffers": (_i32, [_vp, _P(_vp), _P(_vp)]),
    "bt_tiling_prepass_read": (_i32, [_vp, _P(TileCoordinateC), _u32, _P(_u32), _P(IndirectC)]),
    "bt_height_bounds_create": (_i32, [_vp, _u32, _u32, _P(_vp)]),
    "bt_height_bounds_destroy": (None, [_vp]),
    "bt_height_bounds_build": (_i32, [_vp, _vp, _u32]),
    "bt_height_bounds_update": (_i32, [_vp, _vp, _u32, _P(TileCoordinateC), _u32, _P(BoundsUpdateStatsC)]),
    "bt_height_bounds_read": (_i32, [_vp, _P(C.c_uint16), _u64]),
    "bt_height_bounds_write": (_i32, [_vp, _P(C.c_uint16), _u64]),
    "bt_cull_planes": (None, [_P(C.c_float), _P(C.c_float)]),
    "bt_tiling_prepass_set_culling": (_i32, [_vp, _P(CullViewC), _vp]),
    "bt_tiling_prepass_cull_stats": (_i32, [_vp, _P(_u32), _P(_u32)]),
    "bt_tiling_prepass_set_horizon": (_i32, [_vp, _P(HorizonViewC)]),
    "bt_cull_horizon": (_i32, [_P(TerrainModelC), _P(C.c_double), C.c_float, _P(HorizonViewC)]),
    "bt_terrain_view_config_default": (None, [_P(TerrainViewConfigC)]),
    "bt_view_state_from_config": (_i32, [_P(TerrainModelC), _P(TerrainViewConfigC), _P(C.c_double), C.c_float, _P(ViewStateC)]),
    "bt_tile_tree_create": (_i32, [_vp, _P(TerrainModelC), _u32, _P(TerrainViewConfigC), _P(_vp)]),
    "bt_tile_tree_destroy": (None, [_vp]),
    "bt_tile_tree_update": (_i32, [_vp, _P(C.c_double)]),
    "bt_tile_tree_requests": (_i32, [_vp, _P(_P(TileCoordinateC)), _P(_u32), _P(_P(TileCoordinateC)), _P(_u32)]),
    "bt_tile_tree_apply_requests": (_i32, [_vp, _vp]),
    "bt_tile_tree_adjust_to_tile_atlas": (_i32, [_vp, _vp]),
    "bt_tile_tree_buffers": (_i32, [_vp, _P(_vp), _P(_vp)]),
    "bt_tile_tree_read": (_i32, [_vp, _P(TileTreeEntryC), _u32, _P(_u32), _u32, _P(TileCoordinateC), _P(_u32)]),
    "bt_tile_tree_sample_attachment": (_i32, [_vp, _vp, _u32, _P(C.c_double), _u32, _P(C.c_float), _P(C.c_float)]),
    "bt_tile_tree_approximate_height": (_i32, [_vp, _vp, _P(C.c_float)]),
    "bt_tile_tree_view_state": (_i32, [_vp, _P(ViewStateC)]),
    "bt_tile_tree_raycast": (_i32, [_vp, _vp, _u32, _P(RayC), _u32, _u32, _u32, _P(RayHitC)]),
    "bt_tile_tree_render": (_i32, [_vp, _vp, _u32, _P(RenderCameraC), _u32, _u32, _P(C.c_double), _P(C.c_uint8), _P(C.c_float), _P(C.c_uint8), _P(RenderStatsC)]),
    "bt_tile_tree_collide_spheres": (_i32, [_vp, _vp, _u32, _P(SphereC), _u32, _u32, _P(SphereContactC)]),
    "bt_tile_tree_sweep_spheres": (_i32, [_vp, _vp, _u32, _P(SphereSweepC), _u32, _u32, _u32, _u32, _P(SweepHitC)]),
    "bt_tile_tree_sun_occlusion": (_i32, [_vp, _vp, _u32, _P(C.c_double), _u32, _P(C.c_double), _u32, C.c_double, C.c_double, _u32, _P(C.c_uint8),
                                          _P(OcclusionStatsC)]),
    "bt_tile_tree_render_shadowed": (_i32, [_vp, _vp, _u32, _P(RenderCameraC), _u32, _u32, _P(SunShadowC), _P(C.c_double), _P(C.c_uint8), _P(C.c_float),
                                            _P(C.c_uint8), _P(C.c_uint8), _P(RenderStatsC)]),
    "bt_tile_tree_sample_normal": (_i32, [_vp, _vp, _u32, _P(C.c_double), _u32, _P(C.c_float), _P(C.c_float)]),
    "bt_atlas_tile_normals": (_i32, [_vp, _u32, _P(TerrainModelC), _P(TileCoordinateC), _u32, _P(C.c_uint8), _u64]),
    "bt_tile_tree_build_geometry": (_i32, [_vp, _vp, _u32, _P(ViewStateC), _vp, _u32, _vp, _u64]),
    "bt_tile_tree_tile_geometry": (_i32, [_vp, _vp, _u32, _P(ViewStateC), _P(TileCoordinateC), _u32, _u32, _P(TerrainVertexC), _u64]),
    "bt_model_approximation_from_config": (_i32, [_P(TerrainModelC), _P(TerrainViewConfigC), _P(C.c_double), _P(ModelApproximationC)]),
    "bt_tile_tree_model_approximation": (_i32, [_vp, _P(ModelApproximationC)]),
    "bt_tile_tree_build_geometry_hp": (_i32, [_vp, _vp, _u32, _P(ViewStateC), _P(ModelApproximationC), _vp, _u32, _vp, _u64]),
    "bt_tile_tree_tile_geometry_hp": (_i32, [_vp, _vp, _u32, _P(ViewStateC), _P(ModelApproximationC), _P(TileCoordinateC), _u32, _u32, _P(TerrainVertexC), _u64]),
    "bt_frame_update": (_i32, [_vp, _vp, _vp, _P(C.c_double), C.c_uint32, _P(FrameInfoC)]),
    "bt_selftest": (_i32, [_vp, _P(_u32)]),
    "bt_synth_fbm_r16": (_i32, [_vp, _vp, _u32, _u32, _u64, _u32, _u32, _u32, _u32, _u32]),
    "bt_preprocessor_run_streamed": (_i32, [_vp, _vp, C.c_char_p, _u32, _vp]),
    "bt_preprocessor_run_streamed_sharded": (_i32, [_vp, _vp, _vp, C.c_char_p, _u32, _vp]),
}


class StreamStatsC(C.Structure):
    _fields_ = [("streamed", C.c_uint32), ("bands", C.c_uint32), ("banded_launches", C.c_uint32), ("early_tiles", C.c_uint32),
                ("uploaded_bytes", C.c_uint64), ("saved_bytes", C.c_uint64)]


RASTER_HOST_DEFERRED = 2

_lib = None


def lib():
    """Load the HIP library (once).  Raises if it is missing: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C bevy_terrain_amd/csrc`). bevy_terrain_amd has no CPU fallback.")
    try:  # bind to torch's HIP runtime when torch is present (see module docstring)
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)  # AttributeError = ABI mismatch, also loud
        fn.restype = restype
        fn.argtypes = argtypes
    if L.bt_abi_version() != header_abi_version():
        raise ImportError(f"libbevy_terrain_amd.so is ABI {L.bt_abi_version()}, include/bevy_terrain_amd.h is "
                          f"{header_abi_version()}: rebuild (make -C bevy_terrain_amd/csrc)")
    _lib = L
    return L


def check(status):
    if status != BT_OK:
        raise BtError(status, lib().bt_last_error().decode(errors="replace"))
