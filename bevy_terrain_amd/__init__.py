"""bevy_terrain_amd — MI355X-native terrain-tile preprocessing and tile refinement.

The host-side mirror of the hot path of kurtkuehnert/bevy_terrain (its `prelude`, src/lib.rs:60-86,
restricted to that path): the same type names, fields, defaults and builder calls, driving
hand-written HIP kernels for gfx950 through the C ABI of include/bevy_terrain_amd.h.
Importing this package never falls back to a CPU implementation: any call that needs the
library raises if libbevy_terrain_amd.so is missing.
"""
from .terrain import (AttachmentConfig, AttachmentFormat, TerrainConfig, TerrainModel, TerrainViewConfig,
                      TileCoordinate)
from .tile_atlas import Device, EditStamp, ErosionParams, HeightBounds, PaintStamp, PathCost, ScatterRule, SmoothStamp, SplatRule, TileAtlas, generate_mipmaps, mosaic_position, packed_tile_bound, packed_tile_check, tc_decode, tc_encode, trace_path
from .preprocess import AssetServer, PreprocessDataset, Preprocessor, SphericalDataset
from .tiling_prepass import TilingPrepass, cull_horizon, cull_planes, make_view_state
from .tile_tree import TERRAIN_VERTEX_DTYPE, RenderCamera, TileTree, model_approximation_from_config, raycast_terrain, render_rays, sample_attachment, sample_height, sample_normal, view_state_from_config, write_ppm

__all__ = [
    "AttachmentConfig", "AttachmentFormat", "TerrainConfig", "TerrainModel", "TerrainViewConfig", "TileCoordinate",
    "Device", "EditStamp", "ErosionParams", "HeightBounds", "PaintStamp", "PathCost", "ScatterRule", "SmoothStamp", "SplatRule", "TileAtlas", "generate_mipmaps", "mosaic_position", "packed_tile_bound", "packed_tile_check", "tc_decode", "tc_encode", "trace_path",
    "AssetServer", "PreprocessDataset", "Preprocessor", "SphericalDataset",
    "TilingPrepass", "cull_horizon", "cull_planes", "make_view_state",
    "TERRAIN_VERTEX_DTYPE", "RenderCamera", "TileTree", "model_approximation_from_config", "raycast_terrain", "render_rays", "sample_attachment", "sample_height", "sample_normal", "view_state_from_config", "write_ppm",
]

from ._ffi import BtError  # noqa: E402,F401  (status + text of a failed C call)
