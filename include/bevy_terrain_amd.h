/*
 * bevy_terrain_amd.h — C ABI of the MI355X-native terrain preprocessing + tiling-prepass backend.
 *
 * This is the drop-in boundary.  The reference (kurtkuehnert/bevy_terrain @ 2025-03-14) has no
 * FFI: its preprocessing and tile refinement run as wgpu compute passes inside a Bevy render
 * graph.  A Rust host keeps the public API (TerrainPlugin / TerrainPreprocessPlugin /
 * Preprocessor / TileAtlas / TileTree) and replaces the internal seam
 *     GpuPreprocessor::prepare + TerrainPreprocessNode::run + GpuAtlasAttachment::{copy_*,
 *     download_tiles, start_downloading_tiles}           (src/preprocess/mod.rs:143-218,
 *                                                         src/preprocess/gpu_preprocessor.rs:120-223,
 *                                                         src/terrain_data/gpu_tile_atlas.rs:276-412)
 *     TilingPrepassNode::run + TerrainViewData buffers   (src/render/tiling_prepass.rs:204-272,
 *                                                         src/render/terrain_view_bind_group.rs:118-247)
 * with calls into this library (see INTEGRATION.md for the `extern "C"` block).
 *
 * Conventions: opaque handles; POD structs with explicit layout; every function returns a
 * bt_status (0 = ok, < 0 = error) and never throws or aborts; bt_last_error() returns the text of
 * the last error of the calling thread; no callbacks; no global state besides that error string
 * (per-queue device buffers live in the bt_preprocessor that built them);
 * one bt_ctx per GPU and per host thread that drives it.  All file:line citations are relative to the reference checkout.
 */
#ifndef BEVY_TERRAIN_AMD_H
#define BEVY_TERRAIN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 6 (round 6): bt_preprocessor_run_streamed pipelines every fused job of a queue (several attachments, the six rasters of a cube job) and
 * bt_preprocessor_run_streamed_sharded does the same for a BT_RUN_SHARD_DISTRIBUTED rank; bt_stream_stats and bt_run_stats GREW (new
 * trailing fields: callers must be rebuilt against this header); a split onto layers nothing has written since bt_atlas_create takes
 * the "previous value" of a no-data pixel as 0 without fetching it (bt_run_stats.prev_zero_launches) — same bytes;
 * bt_atlas_attachment_storage now counts as a write to every layer of the attachment.  bt_run_stats.reserved is now
 * bt_run_stats.variants (BT_VARIANT_* bits of the last run; same layout, a field that read 0 before).  Two BEHAVIOUR CHANGES (not additions): a borrowed
 * unaligned device raster (on_device = 1) is copied into the library's padded buffer by EVERY run of a kept queue, not only the first
 * (round 5 froze it at the first run); and the rows of a BT_RASTER_HOST_DEFERRED raster must stay alive until the queue is RELEASED,
 * not merely until its first run (a kept queue that is re-planned for another rank / mode reads what the device does not hold yet).
 * 5 (round 5): + bt_ctx_set_io_threads / bt_ctx_io_threads (writer / reader threads of the save and load paths follow the CPUs the
 * process may use), bt_comm_preflight (tile-sized health check of the communicator before the first sharded step) — additions only.
 * 4 (round 4): + bt_frame_update / bt_frame_info, BT_RUN_SHARD_OVERLAP + bt_preprocessor_finish_sharded, bt_preprocessor_source_window, BT_RUN_REFERENCE_DISPATCH, bt_ctx_trim; the fused plan no longer has a fused_todo launch (kind 6 of bt_launch_profile
 * does not occur any more) — additions only.
 * 3 (round 3): + bt_preprocessor_run_streamed, BT_RASTER_HOST_DEFERRED, BT_RUN_SHARD_EXCHANGE, bt_tiling_prepass_run_plain /
 * _run_unordered / _set_window, launch kind 6 (fused todo) in bt_launch_profile — additions only, every version-2 call keeps its
 * meaning. */
#define BT_ABI_VERSION 6u

typedef int32_t bt_status;
enum {
    BT_OK = 0,
    BT_ERR_INVALID_ARGUMENT = -1,
    BT_ERR_ATLAS_OUT_OF_INDICES = -2, /* the reference panics "Atlas out of indices", tile_atlas.rs:384 */
    BT_ERR_DEVICE = -3,               /* a HIP call failed; text in bt_last_error() */
    BT_ERR_IO = -4,
    BT_ERR_UNSUPPORTED = -5, /* e.g. AttachmentFormat::Rgb8 / Rg16: silently unprocessed upstream */
    BT_ERR_OUT_OF_MEMORY = -6,
    BT_ERR_OVERFLOW = -7, /* tile buffer of the tiling prepass too small */
    BT_ERR_INTERNAL = -8, /* a bound the library proves was passed (bt_atlas_path_field: more sweeps than cells): a defect, text in bt_last_error() */
};

#define BT_INVALID_ATLAS_INDEX 0xFFFFFFFFu /* terrain_data/mod.rs:34 */
#define BT_INVALID_LOD 0xFFFFFFFFu         /* terrain_data/mod.rs:35 */
#define BT_MAX_ATTACHMENTS 8u              /* shaders/bindings.wgsl:16-31 */

/* AttachmentFormat (terrain_data/mod.rs:37-57); values are AttachmentFormat::id(). */
enum {
    BT_FORMAT_RGBA8 = 0,
    BT_FORMAT_R16 = 1,
    BT_FORMAT_RG16 = 3, /* accepted in configs, not processed (like the reference) -> BT_ERR_UNSUPPORTED */
    BT_FORMAT_RGB8 = 5, /* dito */
};

/* TileCoordinate (math/coordinate.rs:155-167) — 16 bytes, also the GPU layout (types.wgsl:25-29). */
typedef struct bt_tile_coordinate {
    uint32_t side, lod, x, y;
} bt_tile_coordinate;

/* AtlasTile (terrain_data/tile_atlas.rs:30-35) — 32 bytes, GPU layout preprocessing.wgsl:16-22. */
typedef struct bt_atlas_tile {
    bt_tile_coordinate coordinate;
    uint32_t atlas_index;
    uint32_t _padding[3];
} bt_atlas_tile;

/* AttachmentConfig (terrain_data/mod.rs:87-109). */
typedef struct bt_attachment_config {
    char name[64];
    uint32_t texture_size;    /* default 512 */
    uint32_t border_size;     /* default 1 */
    uint32_t mip_level_count; /* default 1 */
    uint32_t format;          /* BT_FORMAT_* ; default R16 */
} bt_attachment_config;

/* TerrainConfig (terrain.rs:26-49); only the fields the path reads. */
typedef struct bt_terrain_config {
    uint32_t lod_count;    /* default 1 */
    uint32_t atlas_size;   /* default 1024 */
    uint32_t spherical;    /* TerrainModel::is_spherical(), math/terrain_model.rs:54-60 */
    uint32_t attachment_count;
    bt_attachment_config attachments[BT_MAX_ATTACHMENTS];
    char path[256];        /* terrain folder below the assets root */
} bt_terrain_config;

/* A source raster handed to Preprocessor::preprocess_tile in place of asset_server.load(path)
 * (preprocessor.rs:240).  Texels: u16 (R16) or RGBA8, row-major, `row_pitch` bytes per row. */
typedef struct bt_raster {
    const void* data;
    uint32_t width, height;
    uint64_t row_pitch;  /* bytes; 0 = tightly packed */
    uint32_t format;     /* BT_FORMAT_R16 or BT_FORMAT_RGBA8; must equal the attachment's */
    uint32_t on_device;  /* 0: host memory (copied to the GPU by the call), 1: device pointer (borrowed
                            until the preprocessor has run and read at run time, on EVERY run of a kept queue; an R16
                            raster whose base or pitch is not a multiple of 16 bytes is copied device-to-device into a
                            padded buffer of the library's at the start of each run — up to width x height x 2 bytes of
                            device memory, 0.15 ms for 0.5 GB), BT_RASTER_HOST_DEFERRED: host memory that stays the
                            caller's until the queue is RELEASED — copied by bt_preprocessor_run (all at once) or by
                            bt_preprocessor_run_streamed (band by band, beside the kernels and the downloads).  A queue kept
                            with BT_RUN_KEEP_QUEUE may read the rows again (only the window a sharded rank needs travels;
                            a later bt_preprocessor_set_shard / other run flags fetch what the device does not hold yet) */
} bt_raster;
#define BT_RASTER_HOST_DEFERRED 2u

/* A decoded source image in host memory, ready to be handed over as a bt_raster (on_device = 0).  Replaces
 * `asset_server.load(path)` + preprocessor_load_tile (preprocessor.rs:240, 401-422; formats/tiff.rs:14-62): a 16-bit
 * grayscale PNG / TIFF decodes to R16 texels (host byte order), an 8-bit gray / gray + alpha / RGB / RGBA PNG or TIFF to Rgba8 (gray
 * replicated, alpha 255 where the file has none, like Bevy's Image::from_dynamic).  PNG: non-interlaced, 8 / 16 bit.  TIFF: classic
 * (II / MM), strips or tiles, uncompressed / LZW / deflate / PackBits, horizontal predictor.  Anything else:
 * BT_ERR_UNSUPPORTED.  `data` is owned by the library until bt_image_free. */
typedef struct bt_image {
    void* data;
    uint32_t width, height;
    uint32_t format;    /* BT_FORMAT_R16 or BT_FORMAT_RGBA8 */
    uint64_t row_pitch; /* bytes, tightly packed */
} bt_image;
bt_status bt_image_load(const char* path, uint32_t format, bt_image* out);
bt_status bt_image_decode(const void* bytes, size_t size, uint32_t format, bt_image* out);
void bt_image_free(bt_image* image);

/* PreprocessDataset (preprocessor.rs:35-55). */
typedef struct bt_preprocess_dataset {
    uint32_t attachment_index;
    uint32_t side;
    float top_left[2];     /* default (0,0) */
    float bottom_right[2]; /* default (1,1) */
    uint32_t lod_begin, lod_end; /* lod_range = lod_begin..lod_end, default 0..1 */
} bt_preprocess_dataset;

/* SphericalDataset (preprocessor.rs:29-33); rasters are passed next to it, one per cube side. */
typedef struct bt_spherical_dataset {
    uint32_t attachment_index;
    uint32_t lod_begin, lod_end;
} bt_spherical_dataset;

typedef struct bt_ctx bt_ctx;                   /* one GPU + one stream */
typedef struct bt_atlas bt_atlas;               /* TileAtlas + GpuTileAtlas */
typedef struct bt_preprocessor bt_preprocessor; /* Preprocessor + GpuPreprocessor */
typedef struct bt_tiling_prepass bt_tiling_prepass; /* TerrainViewData buffers + TilingPrepassNode */

/* ------------------------------------------------------------------ context */
uint32_t bt_abi_version(void);
const char* bt_last_error(void);
/* `stream` is a hipStream_t owned by the caller (NULL = the library creates its own). */
bt_status bt_ctx_create(int32_t device, void* stream, bt_ctx** out);
void bt_ctx_destroy(bt_ctx* ctx);
/* Waits for the work queued on the current stream (a fresh atlas's zeroing among it) before later work goes to `stream`. */
bt_status bt_ctx_set_stream(bt_ctx* ctx, void* stream);
void* bt_ctx_stream(const bt_ctx* ctx);
bt_status bt_ctx_synchronize(bt_ctx* ctx);
/* Gives back what the context keeps between queues: the device rasters finished queues released (kept so that the next queue's
 * sources need not be allocated again: 0.5 GB for a 16k R16 raster, six of 128 MB for a cube job; at most 8 buffers and 4 GiB) and
 * the pinned staging buffers of the save / load paths and the device and pinned scratch of bt_atlas_tile_bounds,
 * the device scratch of bt_tile_tree_raycast, the device scratch of bt_tile_tree_sample_normal and bt_atlas_tile_normals (their pinned
 * half is the staging buffers above), the device planes of bt_tile_tree_render, the device scratch and list of bt_atlas_scatter_instances.
 * Synchronises the context's stream first.  `freed_bytes` (may be NULL): device + pinned bytes released. */
bt_status bt_ctx_trim(bt_ctx* ctx, uint64_t* freed_bytes);
/* Host threads that write (bt_preprocessor_save / _run_streamed) and read (bt_atlas_load_tiles) tile files for this context.
 * 0 = automatic: min(16, CPUs this process may use) — the affinity mask capped by the cgroup's CPU quota, not the machine's
 * hardware threads (the reference spawns one AsyncComputeTaskPool task per tile, tile_atlas.rs:77-116).  bt_ctx_io_threads returns
 * the number the next save / load will use. */
bt_status bt_ctx_set_io_threads(bt_ctx* ctx, uint32_t threads);
uint32_t bt_ctx_io_threads(const bt_ctx* ctx);
/* hipEvent pair on the context's stream: begin .. end -> elapsed milliseconds (end synchronises) */
bt_status bt_ctx_timer_begin(bt_ctx* ctx);
bt_status bt_ctx_timer_end(bt_ctx* ctx, float* elapsed_ms);
bt_status bt_device_malloc(bt_ctx* ctx, size_t bytes, void** out);
bt_status bt_device_free(bt_ctx* ctx, void* ptr);
bt_status bt_memcpy_h2d(bt_ctx* ctx, void* dst_device, const void* src_host, size_t bytes);
bt_status bt_memcpy_d2h(bt_ctx* ctx, void* dst_host, const void* src_device, size_t bytes);

/* --------------------------------------------- TileCoordinate (coordinate.rs) */
void bt_tile_children(bt_tile_coordinate c, bt_tile_coordinate out[4]);                     /* :196-206 */
void bt_tile_neighbours(bt_tile_coordinate c, uint32_t spherical, bt_tile_coordinate out[8]); /* :208-279 */
bt_tile_coordinate bt_tile_parent(bt_tile_coordinate c);                                    /* :187-194 */
/* "{side}_{lod}_{x}_{y}" (:282-286); returns the length written (without NUL) */
int32_t bt_tile_name(bt_tile_coordinate c, char* buf, size_t cap);

/* ------------------------------------- TileAtlas (terrain_data/tile_atlas.rs) */
/* TileAtlas::new (:531-551): allocates atlas_size x T x T texels per attachment in HBM (zeroed,
 * like a fresh wgpu texture), the index allocator and the existing-tile set. */
bt_status bt_atlas_create(bt_ctx* ctx, const bt_terrain_config* config, bt_atlas** out);
void bt_atlas_destroy(bt_atlas* atlas);
/* TileAtlas::get_tile / get_or_allocate_tile (:553-559, 369-416). */
bt_status bt_atlas_get_tile(bt_atlas* atlas, bt_tile_coordinate c, bt_atlas_tile* out);
bt_status bt_atlas_get_or_allocate_tile(bt_atlas* atlas, bt_tile_coordinate c, bt_atlas_tile* out);
/* TileTreeEntry (terrain_data/tile_tree.rs:49-66) — 8 bytes, also the GPU layout (types.wgsl: TileTreeEntry). */
typedef struct bt_tile_tree_entry {
    uint32_t atlas_index; /* BT_INVALID_ATLAS_INDEX: nothing loaded */
    uint32_t atlas_lod;   /* BT_INVALID_LOD */
} bt_tile_tree_entry;
/* The streaming side of TileAtlasState (tile_atlas.rs:418-503): request_tile (a tile not present gets the oldest
 * unused slot and is queued for loading, one entry per attachment), release_tile (the last release puts the slot at
 * the back of the LRU; its data stays cached until the slot is reused), get_best_tile (the tile itself or its closest
 * loaded ancestor).  Releasing a tile that is not present is BT_ERR_INVALID_ARGUMENT (the reference panics). */
bt_status bt_atlas_request_tile(bt_atlas* atlas, bt_tile_coordinate c);
bt_status bt_atlas_release_tile(bt_atlas* atlas, bt_tile_coordinate c);
bt_status bt_atlas_get_best_tile(const bt_atlas* atlas, bt_tile_coordinate c, bt_tile_tree_entry* out);
/* TileAtlasState::update + AtlasAttachment::update (:327-345, 195-224), synchronously: starts and finishes up to
 * `max_loads` queued tile loads (0 = all): "{assets_root}/{config.path}/data/{name}/{coord}.bin" -> the tile's atlas
 * layer (+ its mip levels); a tile is Loaded once all its attachments are.  A missing / short file leaves the tile
 * Loading forever, like the reference (:202-204); *loaded / *failed (optional) count this call's outcomes. */
bt_status bt_atlas_update(bt_atlas* atlas, const char* assets_root, uint32_t max_loads, uint32_t* loaded, uint32_t* failed);
/* number of queued loads (to_load.len()) */
uint32_t bt_atlas_pending_loads(const bt_atlas* atlas);

/* existing_tiles in atlas-index (= allocation) order. Returns the tile count; fills up to `cap`. */
uint32_t bt_atlas_tiles(const bt_atlas* atlas, bt_tile_coordinate* coords, uint32_t* atlas_indices, uint32_t cap);
/* Device storage of one attachment: layer `i` starts at ptr + i*tile_bytes; rows are T*pixel_size
 * bytes, tightly packed, texel layout = the `.bin` tile file layout.  The caller may write through the pointer (a host-side
 * collective does): asking for it (device_ptr != NULL) counts as a write to every layer (bt_run_stats.prev_zero_launches). */
bt_status bt_atlas_attachment_storage(const bt_atlas* atlas, uint32_t attachment_index, void** device_ptr,
                                      uint64_t* tile_bytes, uint32_t* layers);
/* download + de-pad (gpu_tile_atlas.rs:338-412): `count` consecutive layers into host memory. */
bt_status bt_atlas_download_tiles(bt_atlas* atlas, uint32_t attachment_index, uint32_t first_layer,
                                  uint32_t count, void* dst_host, uint64_t dst_bytes);
/* upload_tiles level 0 (gpu_tile_atlas.rs:309-336). */
bt_status bt_atlas_upload_tile(bt_atlas* atlas, uint32_t attachment_index, uint32_t layer, const void* src_host,
                               uint64_t src_bytes);
/* AtlasTileAttachmentWithData::start_saving (:77-116): writes "{directory}/{coord}.bin" for every
 * existing tile.  TileAtlas::save_tile_config (:605-612): bincode-2 TC file (tiles sorted). */
bt_status bt_atlas_save_attachment(bt_atlas* atlas, uint32_t attachment_index, const char* directory);
bt_status bt_atlas_save_tile_config(const bt_atlas* atlas, const char* file_path);
/* load_tile_config (:616-623): marks the listed tiles as existing. */
bt_status bt_atlas_load_tile_config(bt_atlas* atlas, const char* file_path);
/* formats/mod.rs:8-35 — bincode 2 `config::standard()` of Vec<TileCoordinate>. */
uint64_t bt_tc_encode(const bt_tile_coordinate* tiles, uint32_t count, uint8_t* out, uint64_t cap);
int64_t bt_tc_decode(const uint8_t* data, uint64_t bytes, bt_tile_coordinate* tiles, uint32_t cap);

/* AttachmentData::generate_mipmaps (terrain_data/mod.rs:143-219) on the GPU.
 * Single tile, host in/out: `out` receives all levels concatenated (level 0 first). */
bt_status bt_generate_mipmaps(bt_ctx* ctx, uint32_t format, uint32_t texture_size, uint32_t mip_level_count,
                              const void* level0_host, void* out_host, uint64_t out_bytes);
/* Whole atlas: builds mip levels 1.. of `count` layers starting at `first_layer` into the atlas's mip
 * storage (GpuAtlasAttachment::new allocates mip_level_count levels, gpu_tile_atlas.rs:195-237). */
bt_status bt_atlas_generate_mipmaps(bt_atlas* atlas, uint32_t attachment_index, uint32_t first_layer, uint32_t count);
/* The tile load path — AtlasTileAttachmentWithData::start_loading (tile_atlas.rs:118-149) + upload_tiles
 * (gpu_tile_atlas.rs:309-336) for a batch: reads "{directory}/{coord}.bin" of each tile into its atlas layer
 * (allocated on demand) and builds the mip levels of those layers on the GPU.  coords == NULL: every tile
 * that load_tile_config marked as existing.  A missing or wrongly sized file is BT_ERR_IO. */
bt_status bt_atlas_load_tiles(bt_atlas* atlas, uint32_t attachment_index, const char* directory,
                              const bt_tile_coordinate* coords, uint32_t count);
/* Device pointer + bytes per tile of mip level `mip_level` of the attachment (layers tightly packed).  Level 0 is the pointer
 * bt_atlas_attachment_storage returns, and asking for it (device_ptr != NULL) counts as a write to every layer in the same way
 * (bt_run_stats.prev_zero_launches); read level 0 with bt_atlas_download_tiles to keep the fresh layers' flag. */
bt_status bt_atlas_mip_storage(const bt_atlas* atlas, uint32_t attachment_index, uint32_t mip_level,
                               void** device_ptr, uint64_t* tile_bytes);

/* TileLookup (terrain_data/tile_tree.rs:67-81): the best loaded tile for a position and the uv inside its centre. */
typedef struct bt_tile_lookup {
    uint32_t atlas_index; /* BT_INVALID_ATLAS_INDEX: nothing loaded -> the sample is vec4(0) (tile_atlas.rs:250-252) */
    uint32_t atlas_lod;
    float atlas_uv[2];
} bt_tile_lookup;
/* TileAtlas::sample_attachment -> AtlasAttachment::sample + AttachmentData::sample (tile_atlas.rs:249-258, 569-571;
 * terrain_data/mod.rs:220-263) for a batch of lookups: bilinear sample of the tile's level 0, vec4 per lookup
 * (R16: x = height in [0, 1]).  The reference keeps a CPU copy of every loaded tile for this; here the tiles live in
 * HBM, so the query runs there: `lookups_host` in, `out_vec4_host` (4 floats per lookup) out, synchronous. */
bt_status bt_atlas_sample(bt_atlas* atlas, uint32_t attachment_index, const bt_tile_lookup* lookups_host, uint32_t count,
                          float* out_vec4_host);
/* Min/max height pyramid of R16 layers (culling, collision broad phase, picking).  `grid` g (a power of two, 1..BT_BOUNDS_MAX_GRID,
 * dividing T) cuts a T x T layer into cells of s = T / g texels; level k (0 .. log2 g) has n_k = g >> k cells per side of s << k texels.
 * Cell (cx, cy) of level k covers x in [cx*s_k, min((cx+1)*s_k, T-1)], y likewise: its own block plus the first column to its right and
 * the first row below it, so every bilinear sample inside the cell lies within its bounds and a level-(k+1) cell is the min / max of its
 * four level-k children.  Values are raw unorm16: world height = lerp(min_height, max_height, v / 65535).
 * BT_BOUNDS_SKIP_ZERO leaves texels equal to 0 (no data) out; a cell left without texels reports min 0xFFFF, max 0 (min > max: empty).
 * `layers` (NULL: 0 .. count-1; any order, repeats allowed) are read as they are, tile set or not.  Output per entry of `layers`, in list
 * order: the levels finest first, each n_k x n_k cells row-major (cy major), each cell a {min, max} pair of uint16, so
 *     out_bytes >= count * (4*g*g - 1) / 3 * 4.
 * Ordered behind the work queued on the context's stream; synchronous; a read (not a write for bt_run_stats.prev_zero_launches).
 * Non-R16 attachments: BT_ERR_UNSUPPORTED.  count == 0: BT_OK, nothing touched.  Scratch stays in the context until bt_ctx_trim. */
enum { BT_BOUNDS_SKIP_ZERO = 1, BT_BOUNDS_MAX_GRID = 64 };
bt_status bt_atlas_tile_bounds(bt_atlas* atlas, uint32_t attachment_index, const uint32_t* layers /* NULL: 0 .. count-1 */,
                               uint32_t count, uint32_t grid, uint32_t flags, uint16_t* out_host, uint64_t out_bytes);

/* ---------------- in-place editing: change centre texels of tiles in HBM and restore everything that depends on them
 * (docs/development.md "Real-Time Editing" of the reference names it as missing; it has no such operation).
 *
 * THE INVARIANT.  After any job of this library an attachment's atlas state is a function F of its "primary" centre texels:
 *   1. a tile none of whose four children exists is primary: its centre texels are data;
 *   2. any other existing tile is derived: its centre is downsample (downsample.wgsl:12-40) of its children's centres, an absent child
 *      reads as 0, a texel without data (count 0) is 0, taps in the order (0,0), (0,1), (1,0), (1,1);
 *   3. every existing tile's apron is stitch (stitch.wgsl:53-118) of its neighbours' centres: a missing neighbour clamps into the tile's
 *      own centre, cube faces go through project_to_side;
 *   4. mip levels 1.. of a layer are generate_mipmaps of its level 0 (attachments with mip_level_count > 1).
 * "Exists" = the atlas holds a layer for the tile (bt_atlas_tiles with an atlas index).  An edit at LOD `lod` changes centre texels of
 * existing tiles of that LOD and then restores 2 - 4 for what depends on them: the ancestors up to LOD 0 (stopping where a parent does
 * not exist), the aprons of the written tiles and of their existing neighbours at every written LOD, the mips of every written layer.
 * Tiles finer than `lod` are NOT touched (bt_edit_stats.tiles_with_children counts the edited tiles that have one): edit at the finest
 * LOD the atlas holds there.  The result is byte-identical to F of the edited texels.
 *
 * MOSAIC COORDINATES.  With c = texture_size - 2 * border_size, centre texel (i, j) of tile (side, lod, X, Y) is texel
 * (gx, gy) = (X * c + i, Y * c + j) of the face's mosaic of 2^lod * c texels per side; its position is the integer pair itself.
 *
 * THE BRUSH (bt_atlas_edit_height; R16 only).  IEEE binary32, one rounding per written operation, no contraction; f32(n) is exact for the
 * mosaic sizes that occur.  A centre texel (gx, gy) with raw value t takes the stamps IN LIST ORDER, those whose `side` is the tile's:
 *     dx = f32(gx) - center[0];  dy = f32(gy) - center[1];  d2 = (dx * dx) + (dy * dy);  r2 = radius * radius
 *     the stamp is skipped unless d2 < r2
 *     w = 1 (BT_EDIT_FALLOFF_HARD);  q = d2 / r2, s = 1 - q, w = s * s (BT_EDIT_FALLOFF_SMOOTH)
 *     h = f32(t) / 65535
 *     h' = h + amount * w (BT_EDIT_ADD);  h' = h + (amount - h) * w (BT_EDIT_FLATTEN)
 *     t' = max(1, floor(0.5 + 65535 * clamp(h', 0, 1)))          and t' is the t of the next stamp
 * A texel equal to 0 (no data) is never changed and a stamp never produces 0: the hole mask of a terrain is not the brush's to alter.  A
 * stamp is clipped to its face (it does not continue across a cube edge).  The tiles a stamp can reach are those that meet its box
 * [floor(center - radius), ceil(center + radius)] on both axes (no texel outside it passes d2 < r2); tiles_edited / tiles_missing count
 * the tiles of `lod` that meet a stamp's box and exist / do not exist, and every existing one is written, changed or not.
 *
 * bt_atlas_write_region (R16 and Rgba8) copies a width x height rectangle of centre texels, mosaic coordinates of `lod` on `side`, texels
 * in the attachment's format, zeros allowed, verbatim from host memory (row_pitch bytes per row, 0 = tightly packed), then propagates
 * in the same way.  The rectangle must lie inside [0, 2^lod * c)^2.  The texels travel through the context's pinned staging buffers;
 * the call waits for that copy and for nothing else.
 *
 * BOTH.  Texels that fall into tiles the atlas does not hold are skipped (tiles_missing); nothing outside the existing tiles' layers is
 * written.  `changed` (may be NULL with changed_cap 0) receives every tile, of all LODs, whose layer the call wrote — edited tiles, their
 * ancestors, and the existing neighbours of those (their aprons) — LOD descending, then atlas index, up to changed_cap entries;
 * stats->changed_count is the full number.  The list is host index arithmetic: the calls enqueue on the context's stream behind earlier
 * work and return without synchronising (apart from the staging copy above); every written layer counts as written for
 * bt_run_stats.prev_zero_launches.  Launches: one brush / region launch, one downsample launch per LOD above (the levels depend on each
 * other), one stitch launch, and the mip launches of the written layers (mip_level_count - 1 per run of consecutive layers).
 * A bt_height_bounds table follows an edit by bt_height_bounds_update(table, atlas, attachment_index, changed, changed_count), queued behind
 * the edit on the same stream; bt_atlas_tile_bounds results and a tile tree's approximate height are the caller's to refresh from
 * `changed`.  Plan scratch (device + pinned) stays in the context until bt_ctx_trim.
 * BT_OK with nothing touched: count == 0, width == 0 or height == 0.  BT_ERR_INVALID_ARGUMENT: NULL atlas or a NULL required pointer
 * (stamps, texels_host, changed with changed_cap > 0), attachment_index or lod >= lod_count out of range, side out of range (planar: 0;
 * cube: 0..5), a non-finite center or amount, a radius that is not finite or <= 0, an unknown mode or falloff, count > BT_EDIT_MAX_STAMPS,
 * a rectangle outside the mosaic, a row_pitch smaller than a row.  BT_ERR_UNSUPPORTED: an odd centre size c, Rg16 / Rgb8 attachments, this
 * brush on an Rgba8 attachment (Rgba8 has its own: bt_atlas_paint below).  Neither call aborts. */
enum { BT_EDIT_ADD = 0, BT_EDIT_FLATTEN = 1 };          /* bt_edit_stamp.mode */
enum { BT_EDIT_FALLOFF_SMOOTH = 0, BT_EDIT_FALLOFF_HARD = 1 };
#define BT_EDIT_MAX_STAMPS 256u
typedef struct bt_edit_stamp {
    uint32_t side, mode, falloff, _pad;
    float center[2];   /* mosaic texel units of `lod` on `side`: texel gx of tile X column i is X*c + i, position = the integer itself */
    float radius;      /* texels, finite, > 0 */
    float amount;      /* normalised height (1 = max_height - min_height): ADD delta (signed), FLATTEN target */
} bt_edit_stamp;
typedef struct bt_edit_stats {
    uint32_t tiles_edited, tiles_missing, tiles_with_children, tiles_downsampled, tiles_stitched, layers_mipped, launches, changed_count;
} bt_edit_stats;
bt_status bt_atlas_edit_height(bt_atlas* atlas, uint32_t attachment_index, uint32_t lod, const bt_edit_stamp* stamps, uint32_t count,
                               bt_tile_coordinate* changed, uint32_t changed_cap, bt_edit_stats* stats);
bt_status bt_atlas_write_region(bt_atlas* atlas, uint32_t attachment_index, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0,
                                uint32_t width, uint32_t height, const void* texels_host, uint64_t row_pitch,
                                bt_tile_coordinate* changed, uint32_t changed_cap, bt_edit_stats* stats);
/* SMOOTHING (bt_atlas_smooth_height; R16 only): the third brush.  Let S be a tile's level-0 layer, centre AND apron, AS IT STOOD BEFORE THE
 * CALL, k = kernel_radius (1 .. BT_SMOOTH_MAX_KERNEL, and k <= border_size: the box of a centre texel then lies inside the tile's own
 * layer, whose apron holds the neighbours' centre texels by item 3 of F), b = border_size.  Centre texel (i, j) of an existing tile of
 * `lod`, at layer pixel (px, py) = (b + i, b + j) and mosaic position (gx, gy):
 *   1. t0 = S[py][px].  A texel equal to 0 (no data) is never changed.
 *   2. the box mean, in integers and therefore independent of the order of summation:
 *        sum = the sum of S[py + dy][px + dx] over dx, dy in [-k, k];  n = the number of those texels that are != 0  (n >= 1: the texel itself)
 *        m = f32(sum) / (65535 * f32(n))       binary32; both operands are exact (sum <= 81 * 65535 < 2^24), one correctly rounded division
 *   3. the stamps IN LIST ORDER, those whose `side` is the tile's, with the running value t starting at t0:
 *        dx, dy, d2, r2, the test d2 < r2 and w exactly as in THE BRUSH
 *        a = strength * w;  h = f32(t) / 65535;  h' = h + (m - h) * a;  t' = max(1, floor(0.5 + 65535 * clamp(h', 0, 1)))
 *      one rounding per written operation, no contraction.
 * Then F is restored exactly as by bt_atlas_edit_height: the same plan, the same `changed` order, the same stats fields; the stamp's box,
 * the clipping to the face, tiles_edited / tiles_missing / tiles_with_children, "tiles finer than `lod` are not touched" and "enqueues and
 * returns without synchronising" carry over unchanged.  Consequences:
 *   - m comes from the state before the call for EVERY stamp of the call: one call is one Jacobi pass under all its stamps.  N calls of one
 *     stamp are NOT one call of N stamps (unlike ADD / FLATTEN, whose stamps only see their own texel).
 *   - Edges.  Where a neighbour tile does not exist the box sees the tile's own centre clamped (that is what the apron holds); across a
 *     cube edge it sees the re-projected neighbour; at a cube corner the diagonal is clamped.
 *   - Precondition.  The call assumes F holds beforehand; every operation of this library leaves it so (an overlay dataset whose
 *     neighbours' aprons are stale, DESIGN.md 3.13, is the caller's concern).
 *   - Fixed points.  A constant field and a linear ramp are fixed points (for a ramp sum = n * t, so m == h bit for bit and t' == t), and
 *     so is an isolated data texel (n = 1).  Holes are neither filled nor created.
 * Launches: TWO for the brush (no lane may read a texel the call has already written, and other workgroups write the rows next to a
 * workgroup's own: the first launch reads the layers and writes the new texels to scratch of the context, the second copies them in),
 * then as above: stats->launches = 2 + downsample levels + stitch + mips.  The scratch is the staged-rectangle buffer of
 * bt_atlas_write_region (stream-ordered with it; kept until bt_ctx_trim).
 * BT_ERR_INVALID_ARGUMENT (all checked before any device work): NULL atlas, NULL stamps with count > 0, NULL changed with changed_cap > 0,
 * count > BT_EDIT_MAX_STAMPS, kernel_radius 0 or > BT_SMOOTH_MAX_KERNEL, a bad side or falloff, a non-finite center, a radius that is not
 * finite or <= 0, a strength that is not finite or outside (0, 1], attachment_index or lod out of range.  BT_ERR_UNSUPPORTED:
 * kernel_radius > border_size, an odd centre size, a non-R16 attachment.  count == 0: BT_OK with nothing touched. */
#define BT_SMOOTH_MAX_KERNEL 4u
typedef struct bt_smooth_stamp {
    uint32_t side, falloff;      /* BT_EDIT_FALLOFF_* */
    float center[2];             /* mosaic texels of `lod` on `side`, as bt_edit_stamp */
    float radius;                /* texels, finite, > 0 */
    float strength;              /* finite, 0 < strength <= 1 */
} bt_smooth_stamp;
bt_status bt_atlas_smooth_height(bt_atlas* atlas, uint32_t attachment_index, uint32_t lod, uint32_t kernel_radius,
                                 const bt_smooth_stamp* stamps, uint32_t count,
                                 bt_tile_coordinate* changed, uint32_t changed_cap, bt_edit_stats* stats);
/* PAINT (bt_atlas_paint; Rgba8 only): the brush of the colour format.  IEEE binary32, one rounding per written operation, no contraction.
 * A centre texel (gx, gy) with bytes u[0..3] (u[k] = byte k of the texel: 0 r, 1 g, 2 b, 3 a) takes the stamps IN LIST ORDER, those whose
 * `side` is the tile's:
 *     the texel is skipped by every stamp when u[0] | u[1] | u[2] == 0: no data by the rule of downsample (rgb == 0, alpha ignored)
 *     dx, dy, d2, r2, the test d2 < r2 and w exactly as in THE BRUSH
 *     a = opacity * w
 *     for every k whose bit is set in channel_mask:
 *         c = f32(u[k]) / 255                                          the correctly rounded division
 *         c' = c + (color[k] - c) * a (BT_PAINT_BLEND);  c' = c + color[k] * a (BT_PAINT_ADD)
 *         u'[k] = floor(0.5 + 255 * clamp(c', 0, 1))
 *     channels outside the mask keep their byte
 *     if u'[0] | u'[1] | u'[2] == 0: u'[k] = 1 for every k < 3 of the mask           and u' is the u of the next stamp
 * A stamp never produces a hole and never fills one: the hole mask is not the brush's to alter.  (The last line always finds a k: the texel
 * had data before the stamp and the channels outside the mask did not move, so a channel of the mask went to 0.)
 * Everything else is bt_atlas_edit_height's, word for word: a stamp is clipped to its face; the tiles a stamp can reach are those that meet
 * its box [floor(center - radius), ceil(center + radius)]; tiles_edited / tiles_missing / tiles_with_children count as there and every
 * existing tile of the box is written, changed or not; tiles finer than `lod` are not touched; `changed` has the same content and order;
 * the call enqueues on the context's stream and returns without synchronising; every written layer counts as written for
 * bt_run_stats.prev_zero_launches; the plan scratch stays in the context until bt_ctx_trim.  Launches: one paint launch, one downsample
 * launch per LOD above, one stitch launch, then the mip launches.
 * BT_ERR_INVALID_ARGUMENT (all checked before any device work): NULL atlas, NULL stamps with count > 0, NULL changed with changed_cap > 0,
 * count > BT_EDIT_MAX_STAMPS, a bad side, mode or falloff, channel_mask 0 or above 15, a non-finite center or color, a radius that is not
 * finite or <= 0, an opacity that is not finite or outside (0, 1], attachment_index or lod out of range.  BT_ERR_UNSUPPORTED: a non-Rgba8
 * attachment, an odd centre size.  count == 0: BT_OK with nothing touched. */
enum { BT_PAINT_BLEND = 0, BT_PAINT_ADD = 1 };            /* bt_paint_stamp.mode */
typedef struct bt_paint_stamp {
    uint32_t side, mode, falloff, channel_mask;  /* BT_EDIT_FALLOFF_*; bit k selects channel k (0 r, 1 g, 2 b, 3 a = byte k of the texel) */
    float center[2];   /* mosaic texels of `lod` on `side`, as bt_edit_stamp */
    float radius;      /* texels, finite, > 0 */
    float opacity;     /* finite, 0 < opacity <= 1 */
    float color[4];    /* normalised (1 = 255), finite: BLEND target, ADD signed delta */
} bt_paint_stamp;      /* 48 bytes */
bt_status bt_atlas_paint(bt_atlas* atlas, uint32_t attachment_index, uint32_t lod, const bt_paint_stamp* stamps, uint32_t count,
                         bt_tile_coordinate* changed, uint32_t changed_cap, bt_edit_stats* stats);
/* bt_atlas_read_region (R16 and Rgba8): the inverse of bt_atlas_write_region.  Reads the width x height rectangle of centre texels at
 * mosaic (x0, y0) of `lod` on `side` into host memory, texels in the attachment's format, row_pitch bytes per row (0 = tightly packed;
 * bytes of a row past its texels are not touched).  Texels of tiles the atlas holds no layer for read as 0 in every byte; *tiles_missing
 * (may be NULL) counts those tiles of the rectangle.  Ordered behind the work queued on the context's stream (a read after an
 * un-synchronised edit sees the edit); synchronous; a read: no layer is marked written.  A gather launch copies the layers' texels into the
 * staged-rectangle buffer of bt_atlas_write_region on the device (absent tiles: a memset queued before it), from where the rows travel
 * through the context's pinned staging buffers in chunks of whole rows.
 * BT_ERR_INVALID_ARGUMENT: NULL atlas or texels_host, attachment_index, side or lod out of range, a rectangle outside [0, 2^lod * c)^2, a
 * row_pitch smaller than a row.  BT_ERR_UNSUPPORTED: Rg16 / Rgb8, an odd centre size: the refusals of bt_atlas_write_region, so whatever
 * can be read can be written back.  width == 0 or height == 0 (with valid arguments otherwise): BT_OK, nothing touched.
 * UNDO of any of the four edit calls: read the edit's clipped box (a stamp's [floor(center - radius), ceil(center + radius)] cut to the
 * face, or the written rectangle) before the edit, and write that rectangle back afterwards.  Zeros are legal there, so holes come back,
 * and the write restores ancestors, aprons and mips from the same primary texels: provided F held before the edit, the atlas is then
 * byte-identical to what it was. */
bt_status bt_atlas_read_region(bt_atlas* atlas, uint32_t attachment_index, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0,
                               uint32_t width, uint32_t height, void* texels_host, uint64_t row_pitch, uint32_t* tiles_missing /* may be NULL */);
/* bt_atlas_save_attachment for a list of tiles (the `changed` list of an edit): writes "{directory}/{coord}.bin" of the listed tiles only.
 * A coordinate the atlas holds no layer for: BT_ERR_INVALID_ARGUMENT before anything is written.  count == 0: the directory is created. */
bt_status bt_atlas_save_tiles(bt_atlas* atlas, uint32_t attachment_index, const char* directory, const bt_tile_coordinate* coords, uint32_t count);

/* ------------------------------- Preprocessor (preprocess/preprocessor.rs) */
bt_status bt_preprocessor_create(bt_ctx* ctx, bt_preprocessor** out); /* Preprocessor::new :224-232 */
void bt_preprocessor_destroy(bt_preprocessor* p);
/* clear_attachment (:290-296): existing_tiles.clear(); if `directory` is non-NULL also reset_directory
 * (:18-22): remove "{directory}/../../config.tc", rm -r + mkdir -p the directory. */
bt_status bt_preprocessor_clear_attachment(bt_preprocessor* p, bt_atlas* atlas, uint32_t attachment_index,
                                           const char* directory);
/* preprocess_tile (:298-312) / preprocess_spherical (:314-343): build the task queue and assign atlas
 * indices in the reference's order. Nothing runs on the GPU yet. */
bt_status bt_preprocessor_preprocess_tile(bt_preprocessor* p, bt_atlas* atlas, const bt_preprocess_dataset* dataset,
                                          const bt_raster* source);
bt_status bt_preprocessor_preprocess_spherical(bt_preprocessor* p, bt_atlas* atlas, const bt_spherical_dataset* dataset,
                                               const bt_raster sources[6]);
/* queued task counts in the order split, stitch, downsample, save, barrier (PreprocessTaskType :68-82) */
uint32_t bt_preprocessor_task_counts(const bt_preprocessor* p, uint32_t counts[5]);

enum {
    BT_RUN_AUTO = 0,    /* fused split+pyramid kernels where the job qualifies, else reference-shaped */
    BT_RUN_GENERIC = 1, /* one batched launch per queue phase: split / downsample / stitch */
    BT_RUN_KEEP_QUEUE = 2, /* do not clear the queue (benchmarks re-run the same queue) */
    BT_RUN_PROFILE = 4,    /* record a hipEvent after every launch; read with bt_preprocessor_profile() */
    BT_RUN_SHARD_LOCAL = 8,   /* sharded run, part 1: this rank's column strip of the finest LODs (no collective) */
    BT_RUN_SHARD_FINISH = 16, /* sharded run, part 2 (after the all-gathers): cross-strip aprons + the top LODs */
    BT_RUN_SHARD_DISTRIBUTED = 32, /* sharded planar job: the finest LOD is NOT exchanged — its tiles stay on the rank that
                                    * computed them (they are complete there: finest aprons come from the source), only the
                                    * two parent LODs travel (a quarter of the bytes), every rank still ends with every
                                    * lower LOD.  bt_preprocessor_save then writes this rank's share only.  Jobs with more
                                    * than one side (cube seams read neighbour tiles of the finest LOD): BT_ERR_UNSUPPORTED. */
    BT_RUN_SHARD_EXCHANGE = 64,    /* bt_preprocessor_run_sharded only: issue just the grouped collective of the compiled plan
                                    * (no kernels) — lets a benchmark time the exchange alone */
    BT_RUN_SHARD_OVERLAP = 128,    /* bt_preprocessor_run_sharded only (with BT_RUN_KEEP_QUEUE): the local phase on the context's
                                    * stream, the grouped collective behind it on the communicator's OWN stream, and return — the
                                    * finishing kernels come with bt_preprocessor_finish_sharded.  In between the caller runs the
                                    * local phase of another job (its own preprocessor + atlas): the collective of step k hides
                                    * behind the kernels of step k + 1 */
    BT_RUN_REFERENCE_DISPATCH = 256, /* bt_preprocessor_run / _run_streamed: reproduce the reference's dispatch for texture sizes
                                    * that are not multiples of 8 — it launches texture_size / 8 workgroup rows of 8 x 8
                                    * (src/terrain_data/gpu_tile_atlas.rs:105), so split, downsample and stitch never write the
                                    * last texture_size % 8 rows of a tile (they keep what the atlas held).  Default: every row is
                                    * processed.  No effect on attachments whose texture size is a multiple of 8 */
};
/* Replaces select_ready_tasks + GpuPreprocessor::prepare + TerrainPreprocessNode::run for the whole
 * queue: enqueues every kernel on the context's stream and returns (asynchronous).  Save tasks are
 * remembered; bt_preprocessor_save() writes their files. */
bt_status bt_preprocessor_run(bt_preprocessor* p, bt_atlas* atlas, uint32_t flags);
/* Executes the pending Save tasks: "{assets_root}/{config.path}/data/{name}/{coord}.bin" and, like
 * select_ready_tasks on completion (:358-371), "{assets_root}/{config.path}/config.tc". */
bt_status bt_preprocessor_save(bt_preprocessor* p, bt_atlas* atlas, const char* assets_root);
/* The reference's whole span (preprocessor.rs:363,419: all sources loaded -> all saves done) as one overlapped pipeline:
 * = bt_preprocessor_run + bt_preprocessor_save, but every fused main / direct launch of the plan whose sources are
 * BT_RASTER_HOST_DEFERRED rasters runs in bands of tile rows: a band's source rows travel to the GPU, its kernels start when they
 * have landed, and its finished tiles are downloaded and written while later bands (of the same raster, of the next cube face, of the
 * next attachment) upload and run — three HIP queues, one extra host thread.  Since ABI 6 that covers both of the reference's examples:
 * several attachments in one queue (examples/preprocess_planar.rs:16-60: height R16 + albedo Rgba8, one dataset each) and the six face
 * rasters of a cube job (examples/preprocess_spherical.rs:20-48; the finest tiles on a face edge wait for the seam stitch at the end,
 * all others leave with their band).  Launches that cannot be banded (generic plan, device rasters) run whole, in plan order; a queue
 * without any bandable launch runs the legs one after the other.  Files are byte-identical either way.
 * Synchronous: returns when every file is written.  flags: BT_RUN_GENERIC / BT_RUN_KEEP_QUEUE / BT_RUN_REFERENCE_DISPATCH. */
typedef struct bt_stream_stats {
    uint32_t streamed; /* 1: the overlapped pipeline ran; 0: upload, kernels and save ran one after the other */
    uint32_t bands;    /* bands of all banded launches together */
    uint32_t banded_launches; /* fused main / direct launches that ran band by band (ABI 6) */
    uint32_t early_tiles;     /* tiles downloaded and written before the last launch was issued (ABI 6) */
    uint64_t uploaded_bytes;  /* source bytes that travelled in this call (a sharded rank: its windows only) (ABI 6) */
    uint64_t saved_bytes;     /* tile bytes this call downloaded and wrote (a sharded rank: its share) (ABI 6) */
} bt_stream_stats;
bt_status bt_preprocessor_run_streamed(bt_preprocessor* p, bt_atlas* atlas, const char* assets_root, uint32_t flags, bt_stream_stats* out);
/* Launch statistics of the last bt_preprocessor_run: kernels launched, algorithmic bytes
 * (source texels read once + tile texels written once), tiles produced. */
typedef struct bt_run_stats {
    uint32_t kernel_launches;
    uint32_t tiles;
    uint64_t algorithmic_bytes;
    uint32_t fused_jobs, generic_jobs;
    uint32_t prev_zero_launches; /* (ABI 6) fused main / direct launches of the LAST run whose finest tiles nothing had written since
                                  * bt_atlas_create: "the previous value" of a no-data pixel (split.wgsl:34-42) was taken as the
                                  * atlas's initial 0 instead of fetched — same bytes, no atlas reads.  0 for re-runs of a kept queue */
    uint32_t variants; /* (ABI 6) BT_VARIANT_* bits: which plans and kernel variants the LAST bt_preprocessor_run /
                        * bt_preprocessor_run_sharded launched (cleared at the start of each; streamed runs set them too) */
} bt_run_stats;
/* bt_run_stats.variants: one bit per plan and per kernel variant of the preprocessing launches.  The three modes of the run-time-pitch
 * DMA instance (MAIN_DMA_PITCH, MAIN_APRON_GLOBAL, MAIN_SINGLE_BUFFER) exclude each other: a launch sets exactly one of them. */
enum {
    BT_VARIANT_GENERIC = 0x1u,            /* the batched kernels for the whole queue (BT_RUN_GENERIC, or a job that does not qualify) */
    BT_VARIANT_HYBRID = 0x2u,             /* batched split + stitch of the finest LOD, fused_tail below it (R16 with T > 512 or b > 8) */
    BT_VARIANT_STITCH_LAUNCH = 0x4u,      /* a batched stitch launch inside a fused plan (apron rows, cube seams) */
    BT_VARIANT_MAIN_DMA_528 = 0x8u,       /* fused_main, T = 512, LDS pitch 528, LDS-DMA staging */
    BT_VARIANT_MAIN_DMA_PITCH = 0x10u,    /* fused_main, run-time pitch, LDS-DMA staging, two buffers that hold the apron rows too */
    BT_VARIANT_MAIN_APRON_GLOBAL = 0x20u, /* the same instance, two buffers, apron rows read from global memory */
    BT_VARIANT_MAIN_SINGLE_BUFFER = 0x40u, /* the same instance, one buffer, apron rows read from global memory */
    BT_VARIANT_MAIN_REG_528 = 0x80u,      /* no longer reported: every R16 raster is 16-byte aligned, so T = 512 at LDS pitch 528 takes MAIN_DMA_528 */
    BT_VARIANT_MAIN_REG_PITCH = 0x100u,   /* fused_main, run-time pitch, register staging */
    BT_VARIANT_MAIN_UNSTAGED = 0x200u,    /* fused_corner + fused_main reading the source directly (no LDS window) */
    BT_VARIANT_DIRECT = 0x400u,           /* fused_direct (Rgba8), source rows step one by one */
    BT_VARIANT_DIRECT_REP = 0x800u,       /* fused_direct, a source coarser than the tile grid (rows repeat) */
    BT_VARIANT_DIRECT_SKIPS = 0x1000u,    /* fused_direct, a source finer than the tile grid (rows pass over source rows) */
    BT_VARIANT_TAIL_REGULAR = 0x2000u,    /* fused_tail, atlas indices in the closed form of the fresh layout */
    BT_VARIANT_TAIL_IRREGULAR = 0x4000u,  /* fused_tail, atlas indices looked up in the per-LOD grids */
};
bt_status bt_preprocessor_last_run_stats(const bt_preprocessor* p, bt_run_stats* out);
/* Multi-GPU: tiles shard by column strips of the finest LODs (new design, the reference is single-GPU;
 * SURVEY.md §8e).  Every rank builds the SAME queue (same atlas indices), calls set_shard(rank, world),
 * runs BT_RUN_SHARD_LOCAL, all-gathers each returned range IN PLACE over its atlas storage
 * (ncclAllGather with sendbuff = recvbuff + rank * count: layers [first_layer + r * layers_per_rank, ...) hold
 * rank r's tiles because atlas indices are x-major), then runs BT_RUN_SHARD_FINISH.  Every rank ends with the
 * full atlas, bit-identical to a single-GPU run (with BT_RUN_SHARD_DISTRIBUTED: with its own finest tiles and every
 * lower LOD — the ranges / pieces of the finest LOD are then skipped).  world == 1 restores the normal behaviour. */
typedef struct bt_shard_range {
    uint32_t attachment_index, side, lod;
    uint32_t first_layer;     /* atlas index of tile (x = 0, y = 0) of this (side, lod) */
    uint32_t layers_per_rank; /* contiguous layers owned by each rank */
} bt_shard_range;
bt_status bt_preprocessor_set_shard(bt_preprocessor* p, uint32_t rank, uint32_t world);
/* valid after the first run of the current queue; *count = 0 means "not sharded: every rank computed everything"
 * (or: sharded, but not the regular one-side layout — see bt_preprocessor_shard_pieces) */
/* The window [x0, x1) x [y0, y1) (window = {x0, y0, x1, y1}) of source raster `raster_index` (rasters in the order of the
 * preprocess_* calls; preprocess_spherical adds six) that this preprocessor's launches read; compiles the plan if necessary
 * (flags: BT_RUN_GENERIC).  For a sharded preprocessor with a fused plan that is this rank's column strips + halo — a rank needs
 * no other texel of the source: a BT_RASTER_HOST_DEFERRED raster is uploaded window-only by bt_preprocessor_run, and a caller
 * that fills a device raster itself fills only this (bench.py --gpus N generates only the window).  Otherwise the whole raster.
 * uploaded_bytes (may be NULL): the bytes of the last deferred raster that actually travelled. */
bt_status bt_preprocessor_source_window(bt_preprocessor* p, bt_atlas* atlas, uint32_t raster_index, uint32_t flags, uint32_t window[4],
                                        uint64_t* uploaded_bytes);
bt_status bt_preprocessor_shard_ranges(const bt_preprocessor* p, bt_shard_range* out, uint32_t cap, uint32_t* count);
/* The general form of the exchange (planar AND cube jobs): ownership goes by UNITS — one column strip of one cube side
 * at the granularity of the coarsest LOD the main kernel produces, numbered side-major, `units / world` consecutive
 * units per rank (a job shards iff world divides the unit count: 16k planar 8 units, the 6-face cube job 24).  Every
 * piece is a run of consecutive atlas layers computed by `owner_rank` alone; after BT_RUN_SHARD_LOCAL each piece is
 * broadcast in place from its owner (all pieces inside ONE ncclGroupStart / ncclGroupEnd), then BT_RUN_SHARD_FINISH. */
typedef struct bt_shard_piece {
    uint32_t attachment_index, side, lod;
    uint32_t first_layer, layers;
    uint32_t owner_rank;
} bt_shard_piece;
bt_status bt_preprocessor_shard_pieces(const bt_preprocessor* p, bt_shard_piece* out, uint32_t cap, uint32_t* count);

/* RCCL communicator of the sharded path (new design; `backend "nccl"` IS RCCL on ROCm).  The library resolves the RCCL
 * entry points at run time (the librccl already in the process, else librccl.so.1) — no link-time dependency, and a
 * host that owns an ncclComm_t can hand it over with bt_comm_adopt. */
#define BT_COMM_UNIQUE_ID_BYTES 128
typedef struct bt_comm bt_comm;
bt_status bt_comm_unique_id(uint8_t out[BT_COMM_UNIQUE_ID_BYTES]); /* ncclGetUniqueId: call on rank 0, ship to the others */
bt_status bt_comm_create(bt_ctx* ctx, uint32_t world, uint32_t rank, const uint8_t unique_id[BT_COMM_UNIQUE_ID_BYTES], bt_comm** out);
bt_status bt_comm_adopt(bt_ctx* ctx, void* nccl_comm, uint32_t world, uint32_t rank, bt_comm** out); /* borrowed ncclComm_t */
void bt_comm_destroy(bt_comm* comm);
/* health check: a small grouped in-place all-gather + broadcast through the communicator, verified on the host */
bt_status bt_comm_check(bt_comm* comm);
/* The same with slots of `slot_bytes` each (one atlas tile, say): ONE grouped collective — an in-place all-gather of one slot per rank
 * and an in-place broadcast from the last rank — on the context's stream, every byte verified on the host.  Meant to run once before the
 * first sharded step: a communicator that cannot move a tile fails HERE with RCCL's error string (or, if the collective hangs, under
 * the caller's watchdog) instead of inside a timed step.  `elapsed_ms` (may be NULL): device time of the collective.
 * slot_bytes: 1 .. 64 MiB (world + 1 slots are allocated on the device and on the host).  A HANG IS NOT DETECTED: when the collective
 * fails on some ranks only, the others block in the stream synchronisation — run it under a watchdog (bench.py --preflight-timeout). */
bt_status bt_comm_preflight(bt_comm* comm, uint64_t slot_bytes, float* elapsed_ms);
/* One step of a sharded job, entirely on the context's stream and without host synchronisation: this rank's strip
 * (BT_RUN_SHARD_LOCAL), ONE grouped collective (in-place ncclAllGather per LOD for the regular planar layout, in-place
 * ncclBroadcast per piece otherwise, between ncclGroupStart and ncclGroupEnd), the finishing kernels
 * (BT_RUN_SHARD_FINISH).  `flags`: BT_RUN_GENERIC / BT_RUN_KEEP_QUEUE / BT_RUN_PROFILE, and BT_RUN_SHARD_LOCAL alone to
 * skip the collective and the finish (kernel-only timing).  set_shard(rank, world) must match the communicator. */
bt_status bt_preprocessor_run_sharded(bt_preprocessor* p, bt_atlas* atlas, bt_comm* comm, uint32_t flags);
/* Second half of a BT_RUN_SHARD_OVERLAP step: the context's stream waits for that step's collective, then the finishing kernels
 * run.  flags: BT_RUN_GENERIC / BT_RUN_SHARD_DISTRIBUTED as in the first half, BT_RUN_PROFILE, BT_RUN_KEEP_QUEUE. */
bt_status bt_preprocessor_finish_sharded(bt_preprocessor* p, bt_atlas* atlas, bt_comm* comm, uint32_t flags);
/* The end-to-end span of a SHARDED job with a distributed result (BT_RUN_SHARD_DISTRIBUTED is implied; planar jobs): every rank is one
 * PCIe link.  Rank r uploads only its source window band by band (bt_preprocessor_source_window), runs its units, writes its finest
 * tiles band by band while later bands upload and run, exchanges the two parent LODs (the grouped collective of
 * bt_preprocessor_run_sharded, on the context's stream), runs the finishing kernels and writes its share of the lower LODs (every
 * world-th tile; config.tc from rank 0): the ranks together produce the reference's directory, one writer per file.
 * `comm` may be NULL for hosts that bring their own collective: call once with BT_RUN_SHARD_LOCAL (upload + local kernels + this rank's
 * finest files), exchange bt_preprocessor_shard_ranges / _pieces below the finest LOD yourself, call again with BT_RUN_SHARD_FINISH
 * (finishing kernels + the rest of this rank's files).  With `comm`: pass both flags (or neither) — one call does everything.
 * Other flags: BT_RUN_KEEP_QUEUE.  A preprocessor that is not sharded (world 1) behaves like bt_preprocessor_run_streamed. */
bt_status bt_preprocessor_run_streamed_sharded(bt_preprocessor* p, bt_atlas* atlas, bt_comm* comm, const char* assets_root, uint32_t flags,
                                               bt_stream_stats* out);

/* Per-launch device time of the runs made with BT_RUN_PROFILE since the last call (hipEvents on the
 * context's stream, averaged over those runs).  `kind`: 0 split, 1 downsample, 2 stitch, 3 fused main,
 * 4 fused tail, 5 fused direct (Rgba8), 6 fused todo (re-queued no-data chunks + apron corners, follows 3).  `algorithmic_bytes`: that launch's inputs read once + outputs written once.
 * Synchronises the stream.  Returns the number of launches per run through *count. */
typedef struct bt_launch_profile {
    uint32_t kind;
    uint32_t tasks;
    uint64_t algorithmic_bytes;
    float avg_ms;
    uint32_t samples;
} bt_launch_profile;
bt_status bt_preprocessor_profile(bt_preprocessor* p, bt_launch_profile* out, uint32_t cap, uint32_t* count);

/* ---------------- tiling prepass (render/tiling_prepass.rs, shaders/tiling_prepass) */
/* SideParameter fields the prepass reads (math/terrain_model.rs:228-233; named view_xy/view_uv in
 * types.wgsl:78-80). */
typedef struct bt_side_parameter {
    int32_t view_xy[2];
    float view_uv[2];
} bt_side_parameter;

/* Everything `refine_tiles` reads each frame. */
typedef struct bt_view_state {
    uint32_t spherical;                  /* SPHERICAL shader def (tiling_prepass.rs:61-78) */
    uint32_t geometry_tile_count;        /* TerrainViewConfigUniform (terrain_view_bind_group.rs:81-116) */
    uint32_t refinement_count;
    uint32_t vertices_per_tile;
    float subdivision_distance;
    uint32_t origin_lod;                 /* TerrainModelApproximation (terrain_model.rs:252-259) */
    float approximate_height;
    bt_side_parameter sides[6];
    float world_position[3];             /* CullingUniform.world_position (culling_bind_group.rs:41-55) */
    float world_from_local[12];          /* mesh[0].world_from_local: 3x3 columns then translation */
    float local_from_world_transpose[9]; /* mesh[0].local_from_world_transpose_{a,b}: 3x3 columns */
} bt_view_state;

/* Indirect (terrain_view_bind_group.rs:65-71) as prepare_render leaves it. */
typedef struct bt_indirect {
    uint32_t vertex_count, instance_count, base_vertex, base_instance;
} bt_indirect;

/* TerrainViewData::new (:130-142): final_tiles + temporary_tiles of `geometry_tile_count` entries. */
bt_status bt_tiling_prepass_create(bt_ctx* ctx, uint32_t geometry_tile_count, bt_tiling_prepass** out);
void bt_tiling_prepass_destroy(bt_tiling_prepass* t);
/* TilingPrepassNode::run (:204-272): prepare_root, refinement_count x (refine_tiles, prepare_next),
 * refine_tiles, prepare_render — as one persistent launch behind one chip-wide launch that precomputes the divide tests
 * (see bt_tiling_prepass_run_plain).  Asynchronous on the context's stream. */
bt_status bt_tiling_prepass_run(bt_tiling_prepass* t, const bt_view_state* view);
/* bt_tiling_prepass_run is two launches: every divide test that can matter is evaluated up front, chip-wide (a window of
 * tiles around the view at every LOD and side; the test depends on tile and view only), then the ordered schedule runs over
 * those bits out of LDS.  This is the single-launch form that evaluates each test inside its pass: the same list in the
 * same order, ~3x the worst-case latency; the checker of the two-launch form. */
bt_status bt_tiling_prepass_run_plain(bt_tiling_prepass* t, const bt_view_state* view);
/* The reference's contract is the SET of final tiles: refine_tiles appends them in the arrival order of a global atomic
 * (shaders/tiling_prepass/refine_tiles.wgsl:13-15, 41).  This form produces that set (and the same indirect arguments and
 * overflow verdict) in arrival order too, without the chain of passes: after the chip-wide divide tests a second chip-wide
 * launch decides every tile from its ancestors' bits.  Flat ~10 us per frame whatever the view; temporary_tiles is not
 * written.  The two entries above additionally reproduce the order of a run with invocations taken in id order. */
bt_status bt_tiling_prepass_run_unordered(bt_tiling_prepass* t, const bt_view_state* view);
/* Window radius (tiles around the view's tile at every LOD that get their divide test up front) of the unordered form:
 * 1..28, 0 = default (28).  A tuning / test knob: results do not depend on it (tiles outside the windows are evaluated
 * in place). */
bt_status bt_tiling_prepass_set_window(bt_tiling_prepass* t, uint32_t radius);
/* Device buffers a renderer binds: final_tiles (bt_tile_coordinate[]), indirect args, counters. */
bt_status bt_tiling_prepass_buffers(const bt_tiling_prepass* t, void** final_tiles_device, void** indirect_device);
/* Synchronises and copies the final tile list (bt_tiling_prepass_run / _run_plain: in the reference's sequential append
 * order; _run_unordered: arrival order). */
bt_status bt_tiling_prepass_read(bt_tiling_prepass* t, bt_tile_coordinate* final_tiles_host, uint32_t cap,
                                 uint32_t* count, bt_indirect* indirect);

/* ---------------- frustum and height-bounds culling in the tiling prepass
 * The reference declares it and never fills it in: CullingData carries `planes: array<vec4<f32>, 5>` (shaders/types.wgsl:99-103) and
 * culling_bind_group.rs:25-38 derives them, but CullingUniform::from leaves `planes: default()` and refine_tiles.wgsl reads only
 * culling_view.world_position; docs/implementation.md:59-71, 76, 82 describes the intent (bounding-box frustum culling of tiles from
 * min/max height data "stored at a way lower resolution").  The definition, operation by operation (IEEE binary32, one rounding per
 * written operation, no contraction):
 *
 * POINT of a tile.  point(tile, uv, h) is the arithmetic should_be_divided performs (functions.wgsl:73-96, 117-121 with
 * position_local_to_world / normal_local_to_world): u = (float(x) + uv.x) * 2^-lod, w = (float(y) + uv.y) * 2^-lod, the local position
 * (cube-sphere warp and normalisation when spherical), world = world_from_local * local + translation, normal = normalize(
 * local_from_world_transpose * (local, or (0, 1, 0) when planar)), point = world + h * normal.  The divide test is
 * length3(point(tile, view uv, approximate_height) - world_position) < subdivision_distance * 2^-lod; both run the same device function.
 *
 * HEIGHT RANGE of a tile (side, lod, x, y).  With a bt_height_bounds table of L levels: lb = min(lod, L - 1), the entry of cell
 * (x >> (lod - lb), y >> (lod - lb)) of level lb gives raw (vmin, vmax); without a table (0, 65535).  Then
 * h = min_height + (max_height - min_height) * (float(v) / 65535.0f): h_lo from vmin, h_hi from vmax.
 *
 * VOLUME.  Eight corners P_k = point(tile, uv, h), h in {h_lo, h_hi} (outer loop), uv in (0,0), (1,0), (0,1), (1,1).  A spherical tile
 * bulges beyond the hull of its corners: bulge = length3(point(tile, (0.5, 0.5), h_hi) - ((T0 + T1) + (T2 + T3)) * 0.25f), T the four
 * h_hi corners, componentwise, length3(x, y, z) = sqrt((x*x + y*y) + z*z); planar: bulge = 0.  slack = bulge + margin.
 *
 * TEST.  For each plane i < plane_count, (a, b, c, d): len_i = sqrt((a*a + b*b) + c*c), s_ik = ((a*P_k.x + b*P_k.y) + c*P_k.z) + d.
 * The tile is CULLED when for some plane s_ik < -(slack * len_i) holds for all eight k.  Inside is dot(n, p) + d >= 0; planes need not
 * be normalised; a comparison with a NaN is false, so a NaN plane culls nothing.
 *
 * THE CULLED PREPASS.  A tile is visited when all its ancestors divide and none of them is culled.  A visited, culled tile produces
 * neither children nor a final tile; a visited tile that is not culled behaves as without culling (refine_tiles drops a culled tile
 * before the divide test).  bt_tiling_prepass_run_plain produces the id-order list with the culled tiles left out,
 * bt_tiling_prepass_run_unordered the same set, bt_tiling_prepass_run takes the plain kernel while culling is set (same list, same
 * order; its windows' bits fill the LDS already).  The indirect arguments count the final tiles that remain.  For the overflow verdict
 * a culled tile counts as visited (it occupied a slot of temporary_tiles) and contributes no children.  With a horizon view set
 * (bt_tiling_prepass_set_horizon, below) a tile is culled when the frustum test OR the horizon test culls it, and everything in this
 * paragraph holds for either: the far side of a planet, behind the horizon of a sphere that lies inside the terrain, is dropped.
 * Occlusion by terrain in front of that horizon (a ridge hiding a valley) is not tested: such tiles stay in the list.
 *
 * HORIZON CULLING (spherical and ellipsoidal views).  The test works in SCALED SPACE, the local frame of bt_view_state, in which the
 * ellipsoid is the unit sphere; there the horizon of an ellipsoid is the horizon of a sphere, exactly.  Same arithmetic contract, with
 * dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, and max(x, 0) = x when x > 0, else 0.
 *
 * SCALED POINT of a tile, q(tile, uv, h).  l is the unit local position POINT computes (the cube-sphere warp and normalisation, before
 * world_from_local), n its world normal, t = local_from_world_transpose: g_r = (t[3r]*n.x + t[3r+1]*n.y) + t[3r+2]*n.z for r = 0, 1, 2
 * (local_from_world * n), q = l + h * g componentwise, one multiply and one add each.  q is computed from l, never from the world
 * point: a planet far from the world origin does not lose the test to cancellation.
 *
 * PER TILE.  h_lo, h_hi as in HEIGHT RANGE (the culling state's table and min_height / max_height).  Eight points Q_k = q(tile, uv, h),
 * h in {h_lo, h_hi} (outer loop), uv in (0,0), (1,0), (0,1), (1,1).  d = q(tile, (0.5, 0.5), h_hi) - ((Q_4 + Q_5) + (Q_6 + Q_7)) * 0.25f,
 * bulge = sqrt(dot3(d, d)), m = (bulge + margin) + BT_HORIZON_GUARD.  E = sqrt(dot3(eye, eye)), sv = sqrt(vh), lim = m * E.
 *
 * PER POINT k.  vt = Q_k - eye, ap = -dot3(vt, eye), along = ap / E, perp = sqrt(max(dot3(vt, vt) - along * along, 0)).  The point is
 * HIDDEN when both (ap - vh) > lim and ((along * occluder_radius) - (perp * sv)) > lim.
 *
 * The tile is HORIZON-CULLED when vh > 0 and all eight points are hidden.  A comparison with a NaN is false, so NaNs cull nothing.
 * Why it is conservative: what a sphere hides from the eye is its tangent cone intersected with the half-space beyond the tangent
 * circle, a convex set; the two inequalities say that the ball of radius m around the point lies inside it (along - vh / E is the
 * distance beyond the plane, (along * r - perp * sv) / E the distance inside the cone); so the hull of the eight points widened by m is
 * hidden — the volume argument of the frustum test.  BT_HORIZON_GUARD covers the binary32 rounding of the test itself when the eye is
 * close to the occluder (vh tiny, sv short of digits). */
#define BT_HORIZON_GUARD 9.5367431640625e-07f /* 2^-20, scaled units */

/* The min/max height store of the culling test: one {min, max} pair of raw unorm16 per quadtree tile of LODs 0 .. levels-1, dense, view
 * independent, on the device.  Level l follows level l-1; inside a level entry ((side * n + y) * n + x), n = 1 << l:
 * sides * (4^levels - 1) / 3 entries of 4 bytes, 1 <= levels <= BT_HEIGHT_BOUNDS_MAX_LEVELS (33.6 MB for a cube at 11).  Beside the
 * table the library keeps a private shadow of the same shape for bt_height_bounds_update (own(tile) of every held tile): the object
 * behind a bt_height_bounds* is larger than the struct below, and its device footprint is twice the table's (67 MB for a cube at 11). */
enum { BT_HEIGHT_BOUNDS_MAX_LEVELS = 11 };
/* Created and destroyed by the library only; the fields are there to be read (a renderer may bind `table` itself). */
typedef struct bt_height_bounds {
    bt_ctx* ctx;
    uint32_t sides, levels;
    uint64_t entries; /* sides * (4^levels - 1) / 3 */
    uint32_t* table;  /* device memory: entries words, min | max << 16 */
} bt_height_bounds;
/* sides: 1 (planar) or 6 (cube).  Every entry starts as (0, 65535). */
bt_status bt_height_bounds_create(bt_ctx* ctx, uint32_t sides, uint32_t levels, bt_height_bounds** out);
void bt_height_bounds_destroy(bt_height_bounds* b);
/* Fills the table from every tile the atlas currently holds (bt_atlas_tiles with an atlas index, loaded) with lod < levels, typically
 * the atlas a preprocessing job has just filled:
 *   1. own(tile) = the grid-1 result of bt_atlas_tile_bounds for its layer, flags 0: min and max over the whole T x T layer, border
 *      included, so bilinear samples and stitched texels are inside it;
 *   2. top down, a tile the atlas does not hold takes own of its parent (what the best-loaded-tile fallback would sample there); a root
 *      that is not held is (0, 65535);
 *   3. bottom up, entry(tile) = own(tile) united with entry(child 0..3) for lod + 1 < levels: a parent averages its children, so its own
 *      range is narrower than theirs, and the union makes an entry hold for every LOD a renderer may blend in.
 * After it no entry has min > max.  Synchronous; a read of the atlas (not a write for bt_run_stats.prev_zero_launches).  The atlas's side
 * count must be the table's.  Non-R16 attachment: BT_ERR_UNSUPPORTED. */
bt_status bt_height_bounds_build(bt_height_bounds* b, bt_atlas* atlas, uint32_t attachment_index);
/* Brings the table up to date after some tiles have changed, without reducing the others again and without synchronising.
 * PRECONDITIONS.  `b` was last brought up to date against this `atlas` and `attachment_index`, by bt_height_bounds_build or by earlier
 * updates; `tiles` lists every tile that has changed since then, in layer content or in whether the atlas holds it ("held" is what
 * bt_height_bounds_build tests: listed by bt_atlas_tiles with an atlas index, not loading).  Typically the `changed` list of
 * bt_atlas_edit_height / bt_atlas_write_region, or the tiles just loaded or dropped.  Listing more tiles than changed is harmless.
 * RESULT.  The table is byte-identical to what bt_height_bounds_build(b, atlas, attachment_index) would produce at that point: a
 * recomputation, not a union with the old entries, so ranges shrink as well as grow.
 * INPUT.  Duplicates are allowed.  Tiles with lod >= levels are ignored (they have no entry; deeper tiles read their ancestor at
 * levels - 1).  A listed tile the atlas does not hold is legal: that is how a dropped tile is reported.
 * HOW.  With U the distinct listed tiles of lod < levels: own(tile) of U's held tiles is reduced again (one grid-1 workgroup per layer, as
 * in step 1 of the build, into device scratch); then a table kernel rewrites U, the ancestors of U up to LOD 0, and the whole subtree,
 * down to levels - 1, below every child of a tile of U that the atlas does not hold (those tiles take own of their nearest held
 * ancestor, which may be the changed one).  Up to 4096 rewritten entries that is one launch of one workgroup (two launches per call);
 * above, one launch per step and level, at most 2 + levels per call.  Cost follows the list and those subtrees, not the terrain.
 * ASYNCHRONOUS.  The call enqueues on the context's stream behind earlier work (the edit whose `changed` list it is given) and returns
 * without synchronising; a prepass queued behind it reads the new table.  The plan travels through the pinned ring of the edit calls;
 * scratch stays in the context until bt_ctx_trim.  A read of the atlas (not a write for bt_run_stats.prev_zero_launches).
 * STATUS.  BT_OK with nothing touched: count == 0.  BT_ERR_INVALID_ARGUMENT, before anything is queued: NULL b or atlas, NULL tiles with
 * count > 0, attachment index out of range, table and atlas of different contexts or side counts, a coordinate with side >= sides or
 * x >> lod or y >> lod non-zero, and a table that is not current — never built, overwritten by bt_height_bounds_write since its last
 * build, or last built against another atlas or attachment: build first.  BT_ERR_UNSUPPORTED: a non-R16 attachment.  Never aborts.
 * NOT COVERED.  Evictions are not reported: bt_atlas_request_tile reuses an LRU slot without saying which tile left, and a caller who
 * tracks that lists the tile itself.  A tile tree's approximate height and bt_atlas_tile_bounds pyramids are not refreshed.  The edit's
 * `changed` list is conservative (every neighbour of a written tile): each listed layer is reduced whether its range moved or not. */
typedef struct bt_bounds_update_stats {
    uint32_t tiles_listed;    /* distinct listed tiles with lod < levels */
    uint32_t layers_reduced;  /* those of them the atlas holds: one grid-1 reduction each */
    uint32_t launches;
    uint32_t _pad;
    uint64_t entries_written; /* table entries the call recomputed */
} bt_bounds_update_stats;
bt_status bt_height_bounds_update(bt_height_bounds* b, bt_atlas* atlas, uint32_t attachment_index, const bt_tile_coordinate* tiles,
                                  uint32_t count, bt_bounds_update_stats* stats /* may be NULL */);
/* The whole table, {min, max} pairs in table order: out_bytes / bytes == entries * 4 (bt_height_bounds_write: a table saved earlier; the
 * library does not know own(tile) of a written table, so bt_height_bounds_update refuses it until the next build). */
bt_status bt_height_bounds_read(const bt_height_bounds* b, uint16_t* out_host, uint64_t out_bytes);
bt_status bt_height_bounds_write(bt_height_bounds* b, const uint16_t* src_host, uint64_t bytes);

typedef struct bt_cull_view {
    float planes[5][4];     /* CullingData.planes; inside: dot(xyz, p) + w >= 0 */
    uint32_t plane_count;   /* 0..5; 0 culls nothing */
    float margin;           /* world units added to every tile's slack, finite, >= 0 */
    float min_height, max_height; /* TerrainConfig's, for the unorm16 -> height map */
} bt_cull_view;
/* culling_bind_group.rs:25-38 on a column-major clip_from_world (glam Mat4): left, right, bottom, top, w - z.  Host only. */
void bt_cull_planes(const float clip_from_world[16], float planes[5][4]);
/* cull == NULL: culling off (the state after create).  bounds may be NULL (every tile spans min_height .. max_height); it is borrowed
 * and must outlive its use.  The view's side count is checked against the table's by every run (BT_ERR_INVALID_ARGUMENT before anything
 * is queued); plane_count > 5 and a negative or non-finite margin are refused here. */
bt_status bt_tiling_prepass_set_culling(bt_tiling_prepass* t, const bt_cull_view* cull, const bt_height_bounds* bounds);
/* tiles visited and tiles culled by the last run; synchronises.  After a run without culling: the tiles it visited, 0. */
bt_status bt_tiling_prepass_cull_stats(bt_tiling_prepass* t, uint32_t* visited, uint32_t* culled);

/* The horizon test's view (HORIZON CULLING above); bt_cull_horizon fills it per frame, like bt_cull_planes the planes. */
typedef struct bt_horizon_view {
    float eye[3];           /* the eye in scaled space */
    float vh;               /* |eye|^2 - occluder_radius^2; <= 0 (eye inside the occluder): culls nothing */
    float occluder_radius;  /* (0, 1]: scaled radius of a sphere that lies inside the terrain everywhere */
    float margin;           /* scaled units, finite, >= 0 */
} bt_horizon_view;
/* horizon == NULL: off (the state after create).  Refused here: a non-finite field, occluder_radius outside (0, 1], a negative margin.
 * The state holds for every later run of all three forms and for bt_frame_update until it is set again; callers set it per frame,
 * like the planes.  The test reads the culling state's heights and table: a run with a horizon view set but culling not set
 * (bt_tiling_prepass_set_culling(NULL)), or with a planar view, is BT_ERR_INVALID_ARGUMENT before anything is queued.  A cull view with
 * plane_count == 0 is legal and gives horizon culling alone.  bt_tiling_prepass_cull_stats counts the tiles culled by either test. */
bt_status bt_tiling_prepass_set_horizon(bt_tiling_prepass* t, const bt_horizon_view* horizon /* NULL: off */);

/* -------------------------- TerrainModel / TerrainViewConfig / TileTree (the per-frame CPU side of the prepass) */
enum { BT_MODEL_PLANAR = 0, BT_MODEL_SPHERICAL = 1, BT_MODEL_ELLIPSOIDAL = 2 };
/* TerrainModel (math/terrain_model.rs:41-115): rotation is the identity, as in all three reference constructors.
 * planar: a = side_length; sphere: a = radius; ellipsoid: a = major_axis, b = minor_axis (scale = (a, b, a)). */
typedef struct bt_terrain_model {
    uint32_t kind; /* BT_MODEL_* */
    uint32_t _padding;
    double position[3];
    double a, b;
    float min_height, max_height;
} bt_terrain_model;
/* TerrainViewConfig (terrain_view.rs:18-63), same fields and defaults. */
typedef struct bt_terrain_view_config {
    uint32_t tree_size;           /* 8 */
    uint32_t geometry_tile_count; /* 1000000 */
    uint32_t refinement_count;    /* 30 */
    uint32_t grid_size;           /* 16 */
    double subdivision_tolerance; /* 0.1 */
    double precision_threshold_distance; /* 0.001 */
    double load_distance;         /* 2.5 */
    double morph_distance;        /* 16.0 */
    double blend_distance;        /* 2.0 */
    float morph_range;            /* 0.2 */
    float blend_range;            /* 0.2 */
    uint32_t origin_lod;          /* 10 */
    uint32_t _padding;
} bt_terrain_view_config;
void bt_terrain_view_config_default(bt_terrain_view_config* out);

/* Everything the tiling prepass reads for one view and frame, derived the way the reference derives it:
 * TileTree::new (tile_tree.rs:135-173), TerrainViewConfigUniform::from_tile_tree (terrain_view_bind_group.rs:98-116),
 * TerrainModelApproximation::compute (terrain_model.rs:262-290: only origin_xy / origin_uv per side are read by
 * refine_tiles, HIGH_PRECISION is never defined for it), CullingUniform.world_position, and the mesh uniform of
 * TerrainModel::transform() (terrain_model.rs:195-201).  f64 on the host, `as f32` where the reference casts. */
bt_status bt_view_state_from_config(const bt_terrain_model* model, const bt_terrain_view_config* view_config,
                                    const double view_world_position[3], float approximate_height, bt_view_state* out);
/* The horizon view of a frame (HORIZON CULLING, bt_tiling_prepass_set_horizon).  Host only, float64 throughout.
 * eye = f32(local_from_world * (view - model.position)); occluder_radius = 1 + min(min_height, 0) / min(axes) rounded toward zero to
 * binary32 (a height h displaces a scaled point by at most |h| / the shortest axis, so that sphere lies inside the terrain);
 * vh = f32(dot64(eye32, eye32) - radius32^2), from the ROUNDED eye and radius, so the three fields agree with each other;
 * margin = margin_world / min(axes), rounded up.  BT_ERR_UNSUPPORTED: a planar model.  BT_ERR_INVALID_ARGUMENT: NULL pointers, a
 * non-finite position, a negative or non-finite margin, a min_height that reaches the centre (radius <= 0). */
bt_status bt_cull_horizon(const bt_terrain_model* model, const double view_world_position[3], float margin_world, bt_horizon_view* out);

typedef struct bt_tile_tree bt_tile_tree; /* TileTree + GpuTileTree of one (terrain, view) pair */
/* TileTree::new (tile_tree.rs:135-173).  The node tables (tile states, TileTreeEntry data, origins) live in HBM. */
bt_status bt_tile_tree_create(bt_ctx* ctx, const bt_terrain_model* model, uint32_t lod_count,
                              const bt_terrain_view_config* view_config, bt_tile_tree** out);
void bt_tile_tree_destroy(bt_tile_tree* tree);
/* TileTree::compute_requests -> update (tile_tree.rs:268-359) as ONE launch over sides x lods x tree_size^2 nodes
 * (f64, like the reference): origins, per-node tile coordinate / distance / request state, and the released and
 * requested tile lists in the reference's push order (stable ballot / prefix-sum compaction).  Synchronises; the lists
 * stay readable until the next update. */
bt_status bt_tile_tree_update(bt_tile_tree* tree, const double view_world_position[3]);
bt_status bt_tile_tree_requests(const bt_tile_tree* tree, const bt_tile_coordinate** released, uint32_t* released_count,
                                const bt_tile_coordinate** requested, uint32_t* requested_count);
/* TileAtlas::update's second half (tile_atlas.rs:590-600): drains the lists into release_tile / request_tile. */
bt_status bt_tile_tree_apply_requests(bt_tile_tree* tree, bt_atlas* atlas);
/* TileTree::adjust_to_tile_atlas (:363-374): every node's TileTreeEntry = get_best_tile(node coordinate), looked up on
 * the GPU in a device copy of the atlas's tile states (refreshed when they changed).  Asynchronous. */
bt_status bt_tile_tree_adjust_to_tile_atlas(bt_tile_tree* tree, const bt_atlas* atlas);
/* GpuTileTree buffers (gpu_tile_tree.rs:22-95), kept current on the device — no per-frame upload:
 * entries = bt_tile_tree_entry[side][lod][x][y], origins = uint32[side][lod][2]. */
bt_status bt_tile_tree_buffers(const bt_tile_tree* tree, void** entries_device, void** origins_device);
/* host copies for inspection / tests (synchronise) */
bt_status bt_tile_tree_read(bt_tile_tree* tree, bt_tile_tree_entry* entries, uint32_t entry_cap, uint32_t* origins_xy,
                            uint32_t origin_cap, bt_tile_coordinate* node_coordinates, uint32_t* node_requested);
/* sample_height / sample_attachment (terrain_data/mod.rs:265-307) for a batch of world positions: surface projection,
 * TileTree::compute_blend (:223-239), lookup_tile (:241-266) at lod and lod - 1, bilinear tile samples
 * (AtlasAttachment::sample) and their blend, on the GPU against the tree's entries and the atlas in HBM.
 * out_vec4: 4 floats per position (the attachment value: R16 -> (unorm16, 0, 0, 0), Rgba8 -> the four unorm8 channels, all through the
 * same lerps); heights (optional, may be NULL): lerp(min_height, max_height, value.x).  Heights of an Rgba8 attachment equal
 * lerp(min_height, max_height, red). */
bt_status bt_tile_tree_sample_attachment(bt_tile_tree* tree, bt_atlas* atlas, uint32_t attachment_index,
                                         const double* world_positions_xyz, uint32_t count, float* out_vec4, float* heights);
/* TileTree::approximate_height (:376-386): sample_height at the view position of the last update; also kept by the tree
 * for the next update's tile distances.  */
bt_status bt_tile_tree_approximate_height(bt_tile_tree* tree, bt_atlas* atlas, float* height);
/* the tree's current state as a prepass input (bt_view_state_from_config with the tree's view position / height) */
bt_status bt_tile_tree_view_state(const bt_tile_tree* tree, bt_view_state* out);

/* Batched ray queries against the terrain ("where does this ray meet the ground": picking, line of sight, collision).  The reference has
 * no ray query; the ground is wherever its sample_height says it is, LOD blending and best-loaded-tile fallback included, so a hit agrees
 * with bt_tile_tree_sample_attachment at the hit point bit for bit.
 *
 * For a world point p, the tree's current state (view position, approximate height, entries) and the terrain model m, in this order
 * (IEEE binary64, one rounding per written operation; dot3 / normalize3 = (x*x + y*y) + z*z, v * (1.0 / length)):
 *     local    = position_world_to_local(m, p)
 *     n        = normalize3(transform_vector(m, spherical ? local : (0, 1, 0)))
 *     ground0  = position_local_to_world(m, local, 0.0)
 *     altitude = dot3(p - ground0, n)
 *     h        = the `heights` value bt_tile_tree_sample_attachment returns for p (f32; an unloaded tile samples as 0: h = min_height)
 *     f(p)     = altitude - double(h)
 * n is the direction along which position_local_to_world displaces the surface by a height, so altitude and h are measured along one
 * line (on an ellipsoid that is not exactly the geometric normal, by the reference's choice).  A NaN f compares false: not hit.
 *
 * A ray is p(t) = origin + t * direction (one multiply, one add per component) for t in [t_min, t_max]; the direction need not be
 * normalised.  With N = steps and R = refine_rounds:
 *   coarse march: dt = (t_max - t_min) / double(N), t_i = t_min + double(i) * dt for i = 0 .. N; the hit step is the smallest i with
 *     f(p(t_i)) <= 0.  None: BT_RAY_MISS.  i == 0: BT_RAY_INSIDE, t = t_above = t_min.  Otherwise BT_RAY_HIT, lo = t_(i-1), hi = t_i;
 *   R refinement rounds: u_k = lo + (hi - lo) * (double(k) / 64.0) for k = 1 .. 63; k* = the smallest k with f(p(u_k)) <= 0, or 64;
 *     then hi = (k* == 64 ? hi : u_k*), lo = (k* == 1 ? lo : u_(k*-1)), both from the values before the round;
 *   t = hi, t_above = lo: f(p(t)) <= 0 and, for a hit, f(p(t_above)) > 0, with t - t_above about dt / 64^R.
 * A ray with a non-finite component, a zero direction, a non-finite bound or t_max < t_min is BT_RAY_INVALID and is not marched.
 * BT_RAY_MISS and BT_RAY_INVALID leave every other field of the hit 0.
 *
 * Limits, checked before anything is queued (BT_ERR_INVALID_ARGUMENT): 1 <= steps <= BT_RAYCAST_MAX_STEPS, refine_rounds <=
 * BT_RAYCAST_MAX_REFINE_ROUNDS, and count * 64 * ceil((steps + 1) / 64) <= BT_RAYCAST_MAX_SAMPLES: a ray's samples are counted in whole
 * rounds of 64, which is what the kernel spends (one wave per ray, 64 samples per round, a round with two active lanes costs what a
 * full one does); it implies count * (steps + 1) <= BT_RAYCAST_MAX_SAMPLES.  So at most 262144 rays per call (steps <= 63), 255 at
 * steps 65536; split larger batches.  The longest launch the limits allow is measured in DESIGN.md 3.11.
 * Non-R16 attachments: BT_ERR_UNSUPPORTED.  count == 0: BT_OK, nothing touched.  One launch, ordered behind the work queued on the context's
 * stream; synchronous (host arrays in and out); a read (not a write for bt_run_stats.prev_zero_launches).  Scratch (120 bytes of device
 * memory per ray of the largest batch so far, at most 30 MiB) stays in the context until bt_ctx_trim. */
enum { BT_RAY_MISS = 0, BT_RAY_HIT = 1, BT_RAY_INSIDE = 2, BT_RAY_INVALID = 3 };
enum { BT_RAYCAST_MAX_STEPS = 65536, BT_RAYCAST_MAX_REFINE_ROUNDS = 4, BT_RAYCAST_MAX_SAMPLES = 16777216 };
typedef struct bt_ray {
    double origin[3];
    double direction[3];
    double t_min, t_max;
} bt_ray;
typedef struct bt_ray_hit {
    uint32_t status; /* BT_RAY_* */
    uint32_t step;   /* the hit step i of the coarse march */
    double t, t_above;
    double position[3]; /* p(t) */
    float height;       /* h sampled at p(t) */
    uint32_t _padding;
} bt_ray_hit;
bt_status bt_tile_tree_raycast(bt_tile_tree* tree, bt_atlas* atlas, uint32_t attachment_index, const bt_ray* rays, uint32_t count,
                               uint32_t steps, uint32_t refine_rounds, bt_ray_hit* hits_out);

/* Surface normals ("which way does the ground face": collision response, slope limits and alignment of placed objects, slope-driven
 * texturing).  The reference derives the normal only in its fragment shader (sample_normal, src/shaders/attachments.wgsl:51-107, blended
 * over two LODs in render/fragment.wgsl:99-107); these two calls return that normal: bt_tile_tree_sample_normal for a batch of world
 * positions, with the LOD blend and best-loaded-tile fallback of bt_tile_tree_sample_attachment, and bt_atlas_tile_normals as the
 * tangent-space normal map of listed tiles.  Both evaluate ONE definition, in this order (IEEE binary32 unless marked f64, one rounding
 * per written operation, no contraction):
 *     dot3f(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z
 *     norm3f(v)   : r = 1.0f / sqrtf(dot3f(v, v)); (v.x*r, v.y*r, v.z*r)
 *     cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x)
 *
 * TILE NORMAL s(layer L, lod, uv[2]) of an R16 attachment (T = texture_size, b = border_size, c = T - 2b) and a terrain model:
 *     scale = f32(c) / f32(T); offset = f32(b) / f32(T); o = 0.5f / f32(c)   (the reference's 0.5 / attachments[0].size, size =
 *             center_size, terrain_bind_group.rs:64, applied in texture uv: T / (2c) texels, the reference's choice)
 *     u_a = uv_a * scale + offset
 *     taps, in texture uv: left (u_x - o, u_y), up (u_x, u_y - o), right (u_x + o, u_y), down (u_x, u_y + o)
 *     a tap (p, q): t_a = p_a * f32(T) - 0.5f; rem_a = fmodf(t_a, 1.0f); i_a = int(t_a) (truncating); texels
 *             (clamp(i_x + x, 0, T-1), clamp(i_y + y, 0, T-1)) for x, y in {0, 1} of layer L, each converted by the exact unorm16 -> f32;
 *             A = v00 + (v01 - v00) * rem_y; B = v10 + (v11 - v10) * rem_y; v = A + (B - A) * rem_x   (v[x][y]; the operations of
 *             bt_tile_tree_sample_attachment's tile sample from uv * T - 0.5 on: one code)
 *             (the kernels take rem_a as t_a - truncf(t_a), which is fmodf(t_a, 1.0f) for every finite t_a up to the sign of a zero, and
 *             that sign does not reach v: a unorm value plus either zero is itself)
 *     h = min_height + (max_height - min_height) * v
 *     side_length = f32(model scale) for a planar model, (3.14159265359f / 4.0f) * f32(model scale) otherwise; the model scale is
 *             TerrainModel::scale() in f64 (terrain_model.rs:183-193): side_length / 2 of a planar model, the radius of a sphere,
 *             (major + minor) / 2 of an ellipsoid.  So a planar terrain's "side_length" is HALF its side: the reference's quirk, kept.
 *     dist = side_length / (f32(c) * f32(1u << lod))
 *     s = norm3f((h_left - h_right, h_down - h_up, dist))
 *   L >= atlas_size (nothing loaded): s = (0, 0, 1).  Texels equal to 0 (no data) are read as heights, as the renderer reads them.
 *
 * WORLD NORMAL at world position p, with the tree's current state (view position, approximate height, entries):
 *     1. f64, as bt_tile_tree_sample_attachment: local = position_world_to_local(model, p); surface = position_local_to_world(model,
 *        local, approximate_height)
 *     2. mesh normal: planar VN = (0, 1, 0); otherwise VN = f32(normalize3((local.x / scale.x, local.y / scale.y, local.z / scale.z)))
 *        (f64, then cast): the reference's normal_local_to_world, local_from_world_transpose * local with identity rotation.  On an
 *        ellipsoid this is NOT the direction along which heights displace the surface and bt_tile_tree_raycast measures altitude.
 *     3. N = norm3f(VN)
 *     4. planar: W(s) = (s.x, s.z, s.y).  Otherwise, side = the cube face of `surface` as lookup_tile sees it, face_up = (0, 1, 0) for
 *        sides 0 and 1, (0, 0, -1) for 2 and 3, (-1, 0, 0) for 4 and 5 (attachments.wgsl:55-62): tan = cross(face_up, N); bit =
 *        cross(N, tan); W(s)_k = (tan_k * s.x + bit_k * s.y) + N_k * s.z
 *     5. (lod, ratio) = compute_blend(surface), as bt_tile_tree_sample_attachment
 *     6. l1 = lookup_tile(surface, lod); n1 = norm3f(W(s(l1.atlas_index, l1.atlas_lod, l1.uv)))
 *     7. ratio > 0: l2 = lookup_tile(surface, lod - 1), n2 likewise, n = n1 + (n2 - n1) * ratio per component; otherwise n = n1
 *     8. out = norm3f(n) when dot3f(n, n) > 0, otherwise N
 *     9. up_dot = dot3f(out, N): the cosine of the slope against the mesh normal
 *    10. a position with a non-finite component: out = (0, 0, 0), up_dot = 0, decided before any lookup
 *
 * NORMAL MAP of a tile (side, lod, X, Y) held in layer L (raw texels S[row][column]), for its centre texel (i, j):
 *     uv = ((f32(i) + 0.5f) / f32(c), (f32(j) + 0.5f) / f32(c)); s = s(L, lod, uv)
 *     enc(v) = u8(floor(0.5f + 255.0f * clamp(0.5f + 0.5f * v, 0, 1))); bytes r, g, b = enc(s.x), enc(s.y), enc(s.z); a = 255 when
 *     S[b + j][b + i] != 0, otherwise the texel is (128, 128, 255, 0).  Per entry of `coords`, in list order: c x c texels, j major, 4 bytes.
 *
 * Both calls: ordered behind the work queued on the context's stream; synchronous (host arrays in and out); a read (no layer is marked
 * written for bt_run_stats.prev_zero_launches); scratch stays in the context until bt_ctx_trim.  count == 0: BT_OK, nothing touched.
 * Non-R16 attachments: BT_ERR_UNSUPPORTED.  BT_ERR_INVALID_ARGUMENT, before anything is queued: NULL handles, NULL required arrays with
 * count > 0, attachment_index out of range.  bt_tile_tree_sample_normal is one launch; out_up_dot may be NULL.
 * bt_atlas_tile_normals also refuses, before any device work: a NULL or malformed model, out_bytes < count * c * c * 4, a coordinate with a
 * bad side, lod or x / y or one the atlas holds no layer for (all BT_ERR_INVALID_ARGUMENT; out_host is left untouched), and an attachment
 * with border_size 0 (BT_ERR_UNSUPPORTED: the taps of an edge texel need the neighbour's texels).  It runs one launch per 32 MiB of output. */
bt_status bt_tile_tree_sample_normal(bt_tile_tree* tree, bt_atlas* atlas, uint32_t attachment_index, const double* world_positions_xyz,
                                     uint32_t count, float* out_normals_xyz /* 3 per position */, float* out_up_dot /* may be NULL */);
bt_status bt_atlas_tile_normals(bt_atlas* atlas, uint32_t attachment_index, const bt_terrain_model* model, const bt_tile_coordinate* coords,
                                uint32_t count, uint8_t* out_host, uint64_t out_bytes);

/* SPLAT (bt_atlas_splat_from_height): procedural texturing, the "splat maps or something similar" the reference's roadmap
 * (docs/development.md) names as missing.  For a width x height rectangle of centre texels, mosaic coordinates of `lod` on `side`, the call
 * evaluates up to BT_SPLAT_MAX_RULES height-and-slope rules per texel of the R16 attachment H = height_attachment and writes the result
 * into the same texels of the Rgba8 attachment G = target_attachment of the same atlas (same texture_size and border_size), on the device;
 * then it restores F for G exactly as bt_atlas_write_region does: the same plan, the same `changed` order, the same stats fields.  After the
 * call G is byte-identical to F of the derived centre texels.  IEEE binary32, one rounding per written operation, no contraction.
 * T, b, c are those of H; S_H is the level-0 layer L of H that holds the existing tile (side, lod, X, Y) (a tile has one layer index in all
 * attachments of its atlas).  Centre texel (i, j) of that tile, whose mosaic texel (X * c + i, Y * c + j) lies in the rectangle:
 *   1. raw = S_H[b + j][b + i].  raw == 0 (no data): the target texel becomes (0, 0, 0, 0) and nothing else is evaluated: the derived
 *      map's hole mask is the heights'.
 *   2. v = f32(raw) / 65535.0f (the exact unorm conversion);  h = min_height + (max_height - min_height) * v
 *   3. uv = ((f32(i) + 0.5f) / f32(c), (f32(j) + 0.5f) / f32(c));  s = TILE NORMAL s(L, lod, uv) of H for `model` (the definition of the
 *      surface-normal section above, the value bt_atlas_tile_normals encodes for this texel);  steep = 1.0f - s.z   (0 flat, 1 vertical)
 *   4. clamp01(t) = t > 0 ? (t > 1 ? 1 : t) : 0   (a NaN gives 0);  sm(t) = (t * t) * (3.0f - 2.0f * t)
 *      band(x; lo, hi, fade):  fade > 0:  r = clamp01((x - (lo - fade)) / fade);  q = clamp01(((hi + fade) - x) / fade)
 *                              fade == 0: r = x >= lo ? 1 : 0;  q = x <= hi ? 1 : 0
 *                              band = sm(r) * sm(q)
 *   5. w_k = (weight_k * band(h; height_lo_k, height_hi_k, height_fade_k)) * band(steep; steep_lo_k, steep_hi_k, steep_fade_k) for k < count;
 *      sum = ((w_0 + w_1) + ...) in index order
 *   6. sum > 0:  BT_SPLAT_WEIGHTS (count <= BT_SPLAT_MAX_WEIGHT_RULES): byte k = enc8(w_k / sum) for k < count, 0 above
 *                BT_SPLAT_COLOUR: byte ch (0 r, 1 g, 2 b) = enc8((((w_0 * colour_0[ch]) + w_1 * colour_1[ch]) + ...) / sum), byte 3 = 255
 *                enc8 is the render section's: enc8(v) = u8(floorf(0.5f + 255.0f * clamp01(v)))
 *                (the kernel starts both sums at 0.0f: 0 + x is x up to the sign of a zero, which the comparison sum > 0 and enc8 do not see)
 *      otherwise (no rule reaches the texel): the four `fallback` bytes, verbatim
 *   7. the zero rule, as in PAINT (in-place editing): a data texel never becomes a no-data texel: if bytes 0, 1, 2 are all 0, byte 0 is set to 1
 * Tiles finer than `lod` are not touched (tiles_with_children), and the parents of G are downsample of its children, NOT the rules applied
 * to coarser heights: that is what F says of any attachment.
 * PRECONDITION: F holds for H (its aprons are its neighbours' centres; the taps of an edge texel read them), as for SMOOTHING.
 * REACH: the height texels a target texel reads lie at most R = T / (2c) + 2 (integer division) texels from it on either axis: the tap
 * offset of T / (2c) texels, the bilinear pair, one for the rounding of a tap position.  The call is a read of H (no layer of H is marked
 * written) and a write of G, ordered behind everything queued on the context's stream and not synchronising, so called straight after
 * bt_atlas_edit_height on H with the stamp's box widened by R on every side (and cut to the face) it re-derives what the edit invalidated.
 * `changed` and `stats` describe G; texels of tiles the atlas does not hold are skipped (tiles_missing).  Launches: one splat launch, then
 * as bt_atlas_write_region.  The rules travel in the plan scratch of the context (kept until bt_ctx_trim).
 * All refusals come before anything is queued, with G untouched and *stats zeroed.  BT_ERR_INVALID_ARGUMENT: NULL atlas, model, rules or
 * fallback, NULL changed with changed_cap > 0; an unknown mode; count == 0 or above the mode's limit; in any rule a NaN, lo > hi, a fade
 * that is negative or not finite, a weight that is negative or not finite, a non-finite colour in BT_SPLAT_COLOUR; height_attachment ==
 * target_attachment or either out of range; a malformed model; side, lod or the rectangle as refused by bt_atlas_write_region.
 * BT_ERR_UNSUPPORTED: H not R16 or G not Rgba8; texture_size or border_size differing between the two; border_size 0 (the taps of an edge
 * texel need the neighbour's texels); an odd centre size; a mosaic beyond 2^32 texels.  width == 0 or height == 0 (with valid arguments
 * otherwise): BT_OK, nothing touched, as bt_atlas_write_region. */
enum { BT_SPLAT_WEIGHTS = 0, BT_SPLAT_COLOUR = 1 };                      /* mode */
enum { BT_SPLAT_MAX_RULES = 8, BT_SPLAT_MAX_WEIGHT_RULES = 4 };
typedef struct bt_splat_rule {
    float height_lo, height_hi, height_fade;  /* world height units (the model's min_height .. max_height); lo / hi may be -inf / +inf */
    float steep_lo, steep_hi, steep_fade;     /* steep = 1 - cos(slope): 0 flat, 1 vertical */
    float weight;                             /* finite, >= 0 */
    float colour[3];                          /* BT_SPLAT_COLOUR only: normalised (1 = 255), finite */
    uint32_t _padding[2];
} bt_splat_rule;                              /* 48 bytes */
bt_status bt_atlas_splat_from_height(bt_atlas* atlas, uint32_t height_attachment, uint32_t target_attachment, const bt_terrain_model* model,
                                     uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, uint32_t mode,
                                     const bt_splat_rule* rules, uint32_t count, const uint8_t fallback[4],
                                     bt_tile_coordinate* changed, uint32_t changed_cap, bt_edit_stats* stats);

/* SCATTER (bt_atlas_scatter_instances): vegetation placement, the use of terrain data the reference's documents name and leave to the
 * application ("texturing, vegetation placement, etc.", docs/development.md; "a vegetation map (for placing trees and bushes)",
 * docs/implementation.md).  For every centre texel (a cell) of the listed tiles the call decides, from a hash of the cell's mosaic position
 * and up to BT_SCATTER_MAX_RULES height-and-slope rules, whether the cell places an instance, and returns the instances as one ordered
 * list on the host.  It works per tile, so a streaming view scatters a tile when it loads and again after an edit.
 * IEEE binary32, one rounding per written operation, no contraction; f64 where stated.  H is the R16 attachment height_attachment
 * (T = texture_size, b = border_size, c = T - 2b); L is the layer that holds the listed tile (side, lod, X, Y), S_H its texels
 * [row][column]; M is the optional Rgba8 attachment mask_attachment of the same atlas, with the same T and b (a tile has one layer index
 * in all attachments of its atlas).  Cell (i, j), 0 <= i, j < c, of a listed tile has the mosaic texel (gx, gy) = (X * c + i, Y * c + j):
 *   1. mix(x): x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16   (uint32, wrapping)
 *      k = mix(mix(mix(seed ^ (side << 8 | lod)) ^ gx) ^ gy);  r_n = mix(k + n * 0x9E3779B9u) for n = 0 .. 4
 *      f(r) = f32(r >> 8) * 2^-24   (exact, in [0, 1)).  The key holds only the mosaic position: an instance does not depend on which
 *      other tiles are listed, on their order, or on the atlas layer.
 *   2. a_x = 0.5f + (f(r_1) - 0.5f) * jitter;  a_y = 0.5f + (f(r_2) - 0.5f) * jitter
 *      uv = ((f32(i) + a_x) / f32(c), (f32(j) + a_y) / f32(c))
 *   3. no data: the cell places nothing if S_H[b + j][b + i] == 0, or if any of the four texels of the centre tap is 0: the tap (u_x, u_y)
 *      of TILE NORMAL at this uv (its t_a, rem_a, i_a and clamped texels).  Both count in cells_no_data; nothing else is evaluated.
 *   4. v = the centre tap's bilinear value (TILE NORMAL's A, B, v);  h = min_height + (max_height - min_height) * v
 *      s = TILE NORMAL s(L, lod, uv) of H for `model`;  steep = 1.0f - s.z
 *   5. p_k = ((density_k * band(h; height_lo_k, height_hi_k, height_fade_k)) * band(steep; steep_lo_k, steep_hi_k, steep_fade_k)) * m_k for
 *      k < rule_count, band() of SPLAT step 4;  m_k = 1.0f when mask_channel_k is BT_SCATTER_NO_MASK, otherwise
 *      f32(byte mask_channel_k of M's texel [b + j][b + i] of layer L) / 255.0f
 *   6. u = f(r_0);  A_0 = 0.0f;  A_(k+1) = A_k + p_k in index order.  The cell places ONE instance, of the first k with u < A_(k+1);
 *      without such a k it places nothing.  So rules exclude each other, and a rule behind a sum that has reached 1 places nothing.
 *   7. the instance: rule = k;  cell = (gx, gy);  scale = scale_lo_k + (scale_hi_k - scale_lo_k) * f(r_3);  yaw = 6.2831855f * f(r_4)
 *      position (f64) = coordinate_world_position({side, ((f64(X) + f64(uv.x)) / 2^lod, (f64(Y) + f64(uv.y)) / 2^lod)}, model, h)
 *      (coordinate.rs:115-135: the local position of the coordinate, unit on a spherical model, displaced by h along the model's normal)
 *      normal = norm3f(W(s)) with W of WORLD NORMAL steps 2 - 4, VN taken from that local position ((0, 1, 0) on a plane) and the
 *      tile's side as the face
 *   8. order: tiles in list order, within a tile j major, then i.  out_first[t] is the index of the first instance of coords[t] and
 *      out_first[count] = total.  A coordinate may be listed more than once: each entry gives its own, identical, segment.
 *   9. capacity: the first min(total, cap) instances are written to out_host; what lies beyond them is untouched.  total, per_rule,
 *      cells_no_data and out_first describe the whole list whatever cap is: cap == 0 with a NULL out_host asks for the size.
 * The list's bytes are the same from run to run.  PRECONDITION: F holds for H (the taps of an edge cell read its aprons), as for SPLAT.
 * Ordered behind the work queued on the context's stream; synchronous (host arrays in and out); a read (no layer of H or M is marked
 * written); scratch stays in the context until bt_ctx_trim.  Three launches per chunk of at most 1024 listed tiles (two with cap == 0).
 * count == 0 (with valid arguments otherwise): BT_OK, *stats zeroed, out_first untouched.
 * All refusals come before anything is queued, with *stats zeroed and the outputs untouched.  BT_ERR_INVALID_ARGUMENT: NULL atlas, model,
 * stats or rules; NULL coords with count > 0; NULL out_host with cap > 0; rule_count == 0 or above BT_SCATTER_MAX_RULES; in any rule a NaN,
 * lo > hi, a fade that is negative or not finite, a density outside [0, 1], a scale that is not finite or scale_lo > scale_hi, a
 * mask_channel that is neither 0 .. 3 nor BT_SCATTER_NO_MASK, a mask_channel while mask_attachment is BT_SCATTER_NO_MASK; jitter not in
 * [0, 1]; height_attachment == mask_attachment or either out of range; a malformed model; a coordinate with a bad side, lod or x / y, or
 * one the atlas holds no layer for.  BT_ERR_UNSUPPORTED: H not R16 or M not Rgba8; texture_size or border_size differing between the
 * two; border_size 0 (the taps of an edge cell need the neighbour's texels); an odd centre size; a mosaic beyond 2^32 texels (as SPLAT). */
enum { BT_SCATTER_MAX_RULES = 8 };
#define BT_SCATTER_NO_MASK 0xFFFFFFFFu
typedef struct bt_scatter_rule {
    float height_lo, height_hi, height_fade;  /* as bt_splat_rule */
    float steep_lo, steep_hi, steep_fade;     /* as bt_splat_rule */
    float density;                            /* probability per cell, finite, in [0, 1] */
    float scale_lo, scale_hi;                 /* finite, scale_lo <= scale_hi */
    uint32_t mask_channel;                    /* 0 .. 3: byte of the mask attachment's texel; BT_SCATTER_NO_MASK: none */
    uint32_t _padding[2];
} bt_scatter_rule;                            /* 48 bytes */
typedef struct bt_scatter_instance {
    double position[3];                       /* world, f64 */
    float normal[3];                          /* world, unit */
    float scale, yaw;                         /* yaw in [0, 2 pi) */
    uint32_t rule;                            /* index of the rule that placed it */
    uint32_t cell[2];                         /* mosaic texel (gx, gy) of its LOD and side */
} bt_scatter_instance;                        /* 56 bytes */
typedef struct bt_scatter_stats {
    uint64_t total, written;                  /* instances the list has; instances copied out (min(total, cap)) */
    uint64_t cells, cells_no_data;            /* cells of the listed tiles (count * c * c); those of step 3 */
    uint64_t per_rule[BT_SCATTER_MAX_RULES];  /* instances per rule, of the whole list */
    uint32_t launches, _padding;
} bt_scatter_stats;
bt_status bt_atlas_scatter_instances(bt_atlas* atlas, uint32_t height_attachment, uint32_t mask_attachment /* or BT_SCATTER_NO_MASK */,
                                     const bt_terrain_model* model, const bt_tile_coordinate* coords, uint32_t count,
                                     const bt_scatter_rule* rules, uint32_t rule_count, uint32_t seed, float jitter,
                                     bt_scatter_instance* out_host, uint64_t cap, uint64_t* out_first /* count + 1 entries, may be NULL */,
                                     bt_scatter_stats* stats);

/* Rendering ("what does the terrain look like from here": preview thumbnails of a preprocessed dataset, headless visual checks of an
 * edit, a depth or normal image for a tool that is not wgpu, top-down maps).  The reference's renderer is Bevy / wgpu and stays out of
 * scope; this call casts one ray per pixel on the device and evaluates the fragment stage at the hit, so every plane is defined by the
 * definitions above: the march of bt_tile_tree_raycast, WORLD NORMAL, bt_tile_tree_sample_attachment.
 *
 * Arithmetic: IEEE binary64 unless marked f32, one rounding per written operation, no contraction.
 *
 * PIXEL RAY of pixel (x, y), x = 0 .. width - 1 from the left, y = 0 .. height - 1 from the top:
 *     sx = (2.0 * (double(x) + 0.5)) / double(width) - 1.0
 *     sy = 1.0 - (2.0 * (double(y) + 0.5)) / double(height)
 *     perspective:  o = origin;  d_a = (forward_a + sx * right_a) + sy * up_a
 *     orthographic (BT_RENDER_ORTHOGRAPHIC):  o_a = (origin_a + sx * right_a) + sy * up_a;  d = forward
 *   forward, right and up are used as given and d is not normalised: a perspective caller scales right by tan(fov_y / 2) * aspect and up
 *   by tan(fov_y / 2); with a unit forward and right, up orthogonal to it, t is linear view depth.
 *
 * MARCH: status, step, t, t_above, position p(t) and height are exactly what bt_tile_tree_raycast returns for the ray {o, d, t_min, t_max}
 *   with the same steps and refine_rounds against height_attachment (the definition is that one, not restated).  A camera with non-finite
 *   vectors or bounds, or t_max < t_min, is no error: its pixels are BT_RAY_INVALID, as the ray definition says.
 *     out_t[y * width + x]      = t (0 for BT_RAY_MISS and BT_RAY_INVALID)
 *     out_status[y * width + x] = BT_RAY_*
 *
 * NORMAL PLANE, 3 floats per pixel: BT_RAY_HIT and BT_RAY_INSIDE: `out` of WORLD NORMAL (steps 1 - 10 above) at p(t); otherwise (0, 0, 0).
 *
 * COLOUR PLANE, 4 bytes per pixel, all f32:
 *     base: albedo_attachment == BT_RENDER_NO_ALBEDO: (g, g, g, 1.0f), g = 0.5f * v, v the first component bt_tile_tree_sample_attachment(
 *           height_attachment) returns at p(t) (the reference's sample_color, attachments.wgsl:109-113, under its two-LOD blend: x 0.5 is
 *           exact, so blending first gives the same value); otherwise the four components bt_tile_tree_sample_attachment(albedo_attachment)
 *           returns at p(t)
 *     BT_RENDER_LIGHTING: n = the NORMAL PLANE's value; d = dot3f(n, sun); l = d > 0.0f ? d : 0.0f; k = ambient + (1.0f - ambient) * l;
 *           rgb_c = base_c * k for c = 0, 1, 2; alpha unchanged.  sun is the direction TOWARDS the light, used as given (not normalised).
 *           This is a plain Lambert term.  It is NOT the reference's apply_pbr_lighting, which lives in bevy_pbr and not in the reference.
 *     bytes: enc8(v) = u8(floorf(0.5f + 255.0f * c)), c = v > 0.0f ? (v > 1.0f ? 1.0f : v) : 0.0f (a NaN encodes as 0)
 *     BT_RAY_MISS and BT_RAY_INVALID pixels get `background`.
 *
 * All four planes are host arrays, row-major, y down; each may be NULL (it then costs no store and no device memory), but not all.
 * stats (may be NULL): launches, and the number of BT_RAY_HIT, BT_RAY_INSIDE and BT_RAY_MISS pixels (the rest are BT_RAY_INVALID).
 *
 * The kernel gives a pixel to a lane and an 8 x 8 block of pixels to a wave; a lane marches its ray sample by sample and stops at its
 * hit.  One launch is a run of whole 8 x 8 blocks, in row-major block order, whose worst case, 64 * (steps + 1 + 63 * refine_rounds)
 * samples per block, stays within BT_RAYCAST_MAX_SAMPLES, the bound bt_tile_tree_raycast works under (the longest such launch is measured
 * in DESIGN.md 3.11); a run that holds a whole 8-row band of the image is cut to whole bands.  A larger image is several launches
 * (stats->launches); nothing is copied back before the last one has been queued.
 *
 * Refused before anything is queued, the planes untouched.  BT_ERR_INVALID_ARGUMENT: NULL handles or camera; handles of different
 * contexts; all planes NULL; width or height 0, or width * height > BT_RENDER_MAX_PIXELS; steps outside 1 .. BT_RENDER_MAX_STEPS;
 * refine_rounds > BT_RAYCAST_MAX_REFINE_ROUNDS; height_attachment or albedo_attachment (unless BT_RENDER_NO_ALBEDO) out of range;
 * a non-finite ambient or sun component; unknown flag bits.  BT_ERR_UNSUPPORTED: a height attachment that is not R16, an albedo attachment
 * that is not Rgba8.
 * Ordered behind the work queued on the context's stream; synchronous (host arrays out); a read (no layer is marked written for
 * bt_run_stats.prev_zero_launches).  Scratch (up to 25 bytes of device memory per pixel of the largest image so far, less without some
 * planes) stays in the context until bt_ctx_trim. */
enum { BT_RENDER_ORTHOGRAPHIC = 1, BT_RENDER_LIGHTING = 2 };
enum { BT_RENDER_MAX_STEPS = 4096, BT_RENDER_MAX_PIXELS = 16777216 };
#define BT_RENDER_NO_ALBEDO 0xFFFFFFFFu
typedef struct bt_render_camera {
    double origin[3];
    double forward[3], right[3], up[3]; /* used as given; perspective callers scale right / up by tan(fov/2) (x aspect) */
    double t_min, t_max;
    uint32_t width, height;
    uint32_t flags;             /* BT_RENDER_ORTHOGRAPHIC | BT_RENDER_LIGHTING */
    uint32_t albedo_attachment; /* an Rgba8 attachment index, or BT_RENDER_NO_ALBEDO */
    float sun[3];               /* direction TOWARDS the light, used as given */
    float ambient;
    uint8_t background[4];
    uint32_t _padding;
} bt_render_camera;
typedef struct bt_render_stats {
    uint32_t launches, hit_pixels, inside_pixels, miss_pixels;
} bt_render_stats;
bt_status bt_tile_tree_render(bt_tile_tree* tree, bt_atlas* atlas, uint32_t height_attachment, const bt_render_camera* camera,
                              uint32_t steps, uint32_t refine_rounds, double* out_t, uint8_t* out_status,
                              float* out_normal_xyz /* 3 per pixel */, uint8_t* out_rgba /* 4 per pixel */, bt_render_stats* stats);

/* Sun shadows ("is this point in the sun, for this sun direction": cast shadows in the pictures of bt_tile_tree_render, and the same
 * question for placement and analysis: where vegetation goes, where snow stays, solar exposure over a day's arc of directions, a
 * sky-view factor from a fan of them).  The reference's roadmap lists shadow rendering as missing; it has nothing to compare with, so
 * the answer is defined by the ray query above.
 *
 * SUN OCCLUSION.  For a world point q, a direction s TOWARDS the light (f64, used as given, not normalised), a lift (f64, world units), a
 * distance (f64, in units of |s|) and N = steps, against the tree's current state and one R16 attachment:
 *     n(q)  = the altitude direction of the ray section at q: local = position_world_to_local(m, q),
 *             n = normalize3(transform_vector(m, spherical ? local : (0, 1, 0)))
 *     ray   = {origin_a = q_a + lift * n_a (one multiply, one add per component), direction = s, t_min = 0.0, t_max = distance}
 *     result = the status bt_tile_tree_raycast returns for that ray with steps = N and refine_rounds = 0 (the definition is that one, not
 *             restated; the ceiling skip applies unchanged).
 *   BT_RAY_MISS: lit.  BT_RAY_HIT and BT_RAY_INSIDE: occluded.  BT_RAY_INVALID: a non-finite q (or a lifted origin that is not finite), a
 *   zero or non-finite s, a non-finite or negative distance; none of these is an error.
 *   What the lift is for: a point a ray query reported (bt_ray_hit.position, a pixel's p(t)) lies at or under the ground, f(q) <= 0, so
 *   with lift = 0 its shadow ray is BT_RAY_INSIDE whatever the sun: the ground shadows itself.  The lift must exceed the residual of the
 *   march that found the point (about |d| * (t_max - t_min) / (steps * 64^refine_rounds) along the ray, less in altitude for a grazing
 *   ray), and on slopes also the height the ground gains over one shadow step.  The lift is along n, not along the surface normal.
 *   The march is dt = distance / N long per step: an occluder thinner than |s| * dt along the ray can be stepped over, as by any ray here.
 *   Out of scope: soft shadows and penumbrae (the sun is a direction, the answer is binary), and baking the result into an atlas
 *   attachment.
 *
 * bt_tile_tree_sun_occlusion: SUN OCCLUSION of `count` points for each of `direction_count` directions shared by all points, one status
 * byte per pair: out_status[point * direction_count + d].  The kernel gives a ray to a lane, which marches it sample by sample and stops
 * at the first sample at or under the ground (bt_tile_tree_raycast spends a wave and whole rounds of 64 samples per ray).  A launch is a run of
 * whole waves (64 rays each; ray g of the batch is point g % count, direction g / count) whose worst case, 64 * (steps + 1)
 * samples per wave, stays within BT_RAYCAST_MAX_SAMPLES; a larger batch is several launches (stats->launches), and nothing is copied back
 * before the last one has been queued.  stats (may be NULL): launches and the number of lit (MISS), occluded (HIT or INSIDE) and invalid rays.
 * Refused before anything is queued, out_status untouched.  BT_ERR_INVALID_ARGUMENT: NULL handles, handles of different contexts, an
 * attachment index out of range, steps outside 1 .. BT_RENDER_MAX_STEPS, a non-finite lift, count * direction_count >
 * BT_OCCLUSION_MAX_RAYS, a NULL array when count * direction_count > 0.  BT_ERR_UNSUPPORTED: an attachment that is not R16.
 * count == 0 or direction_count == 0: BT_OK, nothing touched but a non-NULL stats, which is zeroed.  Ordered behind the work queued on the
 * context's stream; synchronous (host arrays in and out); a read (no layer is marked written).  Scratch (the ray queries': 24 bytes
 * per point and per direction and one per ray of the largest batch so far) stays in the context until bt_ctx_trim. */
enum { BT_OCCLUSION_MAX_RAYS = 16777216 };
typedef struct bt_occlusion_stats {
    uint32_t launches, lit, occluded, invalid;
} bt_occlusion_stats;
bt_status bt_tile_tree_sun_occlusion(bt_tile_tree* tree, bt_atlas* atlas, uint32_t attachment_index, const double* world_positions_xyz, uint32_t count,
                                     const double* directions_xyz, uint32_t direction_count, double lift, double distance, uint32_t steps,
                                     uint8_t* out_status /* count * direction_count, point-major */, bt_occlusion_stats* stats);

/* bt_tile_tree_render_shadowed: bt_tile_tree_render with cast shadows.  Every plane of bt_tile_tree_render is defined as it is there, and:
 *
 * SHADOW PLANE, 1 byte per pixel: for a BT_RAY_HIT or BT_RAY_INSIDE pixel, SUN OCCLUSION at q = p(t) with s_a = double(camera.sun[a]) (the
 *   exact widening) and shadow->lift, shadow->distance, shadow->steps; for any other pixel BT_SHADOW_NONE.
 * COLOUR PLANE with BT_RENDER_LIGHTING: sh = (the shadow plane's value is BT_RAY_HIT or BT_RAY_INSIDE) ? 0.0f : 1.0f and
 *   k = ambient + (1.0f - ambient) * (l * sh).  l * 1.0f is l, and for a finite l, l * 0.0f is 0: a lit pixel has the bytes
 *   bt_tile_tree_render gives it, an occluded pixel the bytes bt_tile_tree_render gives with sun = (0, 0, 0).  Without BT_RENDER_LIGHTING the
 *   colour is bt_tile_tree_render's and the shadow plane is defined all the same.
 * When out_shadow is NULL and the colour cannot show the result (no out_rgba, no BT_RENDER_LIGHTING, or l == 0) the kernel leaves the
 * shadow march out; that cannot be observed.
 *
 * A launch is a run of whole 8 x 8 blocks whose worst case, 64 * ((steps + 1 + 63 * refine_rounds) + (shadow->steps + 1)) samples per
 * block, stays within BT_RAYCAST_MAX_SAMPLES, cut to whole bands as in bt_tile_tree_render.  Refusals: those of bt_tile_tree_render, and
 * BT_ERR_INVALID_ARGUMENT for a NULL shadow, shadow->steps outside 1 .. BT_RENDER_MAX_STEPS, a non-finite shadow->lift, and all FIVE planes
 * NULL.  A non-finite or negative shadow->distance is no error (BT_RAY_INVALID in the shadow plane, lit in the colour).  Synchronous, a
 * read; the scratch is bt_tile_tree_render's, one byte per pixel more with a shadow plane. */
typedef struct bt_sun_shadow {
    double lift, distance; /* SUN OCCLUSION's, world units / units of |sun| */
    uint32_t steps;        /* 1 .. BT_RENDER_MAX_STEPS */
    uint32_t _padding;
} bt_sun_shadow;
#define BT_SHADOW_NONE 255u
bt_status bt_tile_tree_render_shadowed(bt_tile_tree* tree, bt_atlas* atlas, uint32_t height_attachment, const bt_render_camera* camera,
                                       uint32_t steps, uint32_t refine_rounds, const bt_sun_shadow* shadow, double* out_t, uint8_t* out_status,
                                       float* out_normal_xyz /* 3 per pixel */, uint8_t* out_rgba /* 4 per pixel */,
                                       uint8_t* out_shadow /* 1 per pixel */, bt_render_stats* stats);

/* Terrain collision ("does this body touch the ground: where, how deep, along which normal": a physics step, a character controller).
 * The reference's roadmap lists collision as missing.  A ray has no radius; these two calls answer for a sphere, against the ground every
 * other query here uses (sample_height with LOD blend and best-loaded-tile fallback), so a contact agrees with
 * bt_tile_tree_sample_attachment and bt_tile_tree_raycast bit for bit.  IEEE binary64 unless a value is marked f32, one rounding per
 * written operation, no contraction; dot3, normalize3, position_world_to_local, position_local_to_world, transform_vector as in the ray
 * section; cross as in the normals' section, in f64.  ray_frame(m, p) = (local, n, ground0) of the ray section at p.
 *
 * SPHERE CONTACT of a centre c, a radius r and R = refine_rounds, against the tree's current state and the model m:
 *   1. A non-finite component of c, a non-finite r or r < 0: BT_CONTACT_INVALID, every other field 0, nothing is sampled.
 *   2. local, n, ground0 = ray_frame(m, c); a = dot3(c - ground0, n).
 *   3. When border_size >= 1 and max_height >= min_height (the ray section's ceiling skip) and a - r > double(lerp(min_height, max_height,
 *      1.0f)): BT_CONTACT_FAR, every other field 0, nothing is fetched.  This broad phase is part of the definition.  On a plane and on a
 *      sphere the altitude line is the geometric normal and no ground is above the ceiling, so FAR implies no contact.  On an ellipsoid
 *      the altitude line is not the geometric normal (the reference's choice): the ellipsoid's FAR is that of the altitude line.
 *   4. The ground point G(q) of a world point q: local_q = position_world_to_local(m, q); h_q = the `heights` value (f32)
 *      bt_tile_tree_sample_attachment returns for q (its surface point is position_local_to_world(m, local_q, approximate_height); an
 *      unloaded tile samples as 0); G(q) = position_local_to_world(m, local_q, double(h_q)).
 *   5. g0 = G(c), f = a - double(h0).  f <= 0: BT_CONTACT_BELOW with point = g0, normal = n, distance = f, depth = r - f, candidate = 0,
 *      height = h0.  A NaN f compares false and the definition goes on.
 *   6. Tangent basis.  Planar: e1 = (1, 0, 0), e2 = (0, 0, 1).  Otherwise k = the index of the smallest |n_k| (ties: the lowest index), u =
 *      the unit vector of axis k, e1 = normalize3(cross(u, n)), e2 = cross(n, e1).
 *   7. best = {D2 = dot3(g0 - c, g0 - c), candidate 0, point g0, height h0}, (ox, oy) = (0, 0), w = r.  For round k = 0 .. R, lane
 *      l = 0 .. 63, i = l & 7, j = l >> 3:
 *          x = ox + w * ((2.0 * double(i) - 7.0) / 7.0);  y = oy + w * ((2.0 * double(j) - 7.0) / 7.0)
 *          q_a = c_a + (x * e1_a + y * e2_a);  g = G(q);  d2 = dot3(g - c, g - c)
 *      the round's winner is the smallest d2 (ties: the lowest l; a NaN d2 never wins).  If its d2 < best.D2 (strictly) best becomes the
 *      winner with candidate = 64 k + l + 1 and (ox, oy) its (x, y); otherwise both stay.  After each round w = w * (2.0 / 7.0).
 *   8. distance = sqrt(best.D2); status = distance < r ? BT_CONTACT_TOUCHING : BT_CONTACT_NONE (NONE reports every field: the clearance);
 *      depth = r - distance; point and height are best's; normal_a = (c_a - point_a) * (1.0 / distance) when distance > 0, otherwise n.
 *   The foot is a candidate, so flat ground gives the exact distance.  On a plane of gradient g (g * g <= 2) whose nearest point lies
 *   within the first window, the reported distance exceeds the true one, d, by at most (2 + g * g) * s * s / (8 d), s = r * (2/7)^(R+1)
 *   the last round's stencil spacing.  The distance never grows with R.
 *
 * SPHERE SWEEP (continuous collision, the "move" of move-and-slide): the centre moves as c(t) = origin + t * direction (the ray
 * section's p(t)).  blocked(t) = SPHERE CONTACT of (c(t), r, R) is TOUCHING or BELOW.  Coarse march: dt and t_i exactly as in the ray
 * section for i = 0 .. steps; the hit step is the smallest i with blocked(t_i).  None: BT_RAY_MISS.  i == 0: BT_RAY_INSIDE, t = t_above =
 * t_min.  Otherwise BT_RAY_HIT, lo = t_(i-1), hi = t_i, and for each of `bisections` rounds mid = lo + (hi - lo) * 0.5; blocked(mid) ? hi
 * = mid : lo = mid.  t = hi, t_above = lo, contact = SPHERE CONTACT at c(t).  BT_RAY_MISS and BT_RAY_INVALID leave every other field 0.
 * BT_RAY_INVALID: the ray section's rules, and r not finite or < 0.  Ground thinner than a step is passed through, as by any ray here.
 *
 * Limits, checked before anything is queued (BT_ERR_INVALID_ARGUMENT): NULL handles or two contexts (before the count == 0 shortcut),
 * refine_rounds <= BT_COLLIDE_MAX_REFINE_ROUNDS, 1 <= steps <= BT_SWEEP_MAX_STEPS, bisections <= BT_SWEEP_MAX_BISECTIONS, count * 64 *
 * (R + 1) <= BT_COLLIDE_MAX_SAMPLES for contacts and count * 64 * (R + 1) * (steps + bisections + 2) <= BT_COLLIDE_MAX_SAMPLES for sweeps
 * (64-bit products), a NULL array with count > 0.  Non-R16 attachments: BT_ERR_UNSUPPORTED.  count == 0: BT_OK, nothing touched.  Each call
 * is one launch (one wave per sphere or sweep, a round is one G(q) per lane), ordered behind the work queued on the context's stream;
 * synchronous (host arrays in and out); a read (no layer is marked written).  Scratch (the ray queries': 112 bytes per sphere, 176 per
 * sweep of the largest batch so far) stays in the context until bt_ctx_trim.
 * Out of scope: capsules and boxes, a contact manifold of more than one point, restitution and friction, bodies against bodies. */
enum { BT_CONTACT_NONE = 0, BT_CONTACT_TOUCHING = 1, BT_CONTACT_BELOW = 2, BT_CONTACT_INVALID = 3, BT_CONTACT_FAR = 4 };
enum { BT_COLLIDE_MAX_REFINE_ROUNDS = 6, BT_COLLIDE_MAX_SAMPLES = 16777216, BT_SWEEP_MAX_STEPS = 4096, BT_SWEEP_MAX_BISECTIONS = 32 };
typedef struct bt_sphere {
    double center[3];
    double radius;
} bt_sphere;
typedef struct bt_sphere_contact {
    uint32_t status;    /* BT_CONTACT_* */
    uint32_t candidate; /* 0: the foot; 64 k + l + 1: lane l of round k */
    double distance, depth;
    double point[3], normal[3];
    float height; /* h sampled for `point` */
    uint32_t _padding;
} bt_sphere_contact;
bt_status bt_tile_tree_collide_spheres(bt_tile_tree* tree, bt_atlas* atlas, uint32_t attachment_index, const bt_sphere* spheres, uint32_t count,
                                       uint32_t refine_rounds, bt_sphere_contact* contacts_out);
typedef struct bt_sphere_sweep {
    double origin[3], direction[3];
    double radius, t_min, t_max;
} bt_sphere_sweep;
typedef struct bt_sweep_hit {
    uint32_t status; /* BT_RAY_* */
    uint32_t step;   /* the hit step i of the coarse march */
    double t, t_above;
    bt_sphere_contact contact; /* SPHERE CONTACT at c(t) */
} bt_sweep_hit;
bt_status bt_tile_tree_sweep_spheres(bt_tile_tree* tree, bt_atlas* atlas, uint32_t attachment_index, const bt_sphere_sweep* sweeps, uint32_t count,
                                     uint32_t steps, uint32_t bisections, uint32_t refine_rounds, bt_sweep_hit* hits_out);

/* Terrain geometry ("where are the vertices of the tiles the prepass selected": colliders for the visible tiles, mesh export, a renderer
 * that is not wgpu).  bt_frame_update ends with final_tiles and indirect arguments whose vertex_count counts vertices of the reference's
 * vertex stage (src/shaders/render/vertex.wgsl: compute_tile_uv, compute_local_position, compute_morph, compute_blend, lookup_tile through
 * the tree's entries, sample_height with the two-LOD blend, the displacement along the mesh normal).  These two calls run that stage as
 * a compute pass: bt_tile_tree_build_geometry expands the prepass's final tiles on the device, bt_tile_tree_tile_geometry a listed set of
 * tiles into host memory.  The clip-space transform is left to the caller; the surface normal of a vertex is bt_tile_tree_sample_normal's.
 * These two run the stage with HIGH_PRECISION off; bt_tile_tree_build_geometry_hp / bt_tile_tree_tile_geometry_hp below run it with the
 * branch on (the reference's default: the Taylor series of TerrainModelApproximation).  The TILE_TREE_LOD branch is not built.
 *
 * Parameters.  From the tree (bt_tile_tree_create): grid_size g, tree_size, lod_count, morph_range, blend_range, min_height, max_height,
 * and morph_distance / blend_distance = f32(view_config value * TerrainModel::scale()) (tile_tree.rs:145-146, `as f32` as in
 * terrain_view_bind_group.rs:107-108).  From `view` (NULL: bt_tile_tree_view_state(tree)): what refine_tiles reads, i.e. spherical,
 * approximate_height, world_position and the two mesh matrices.
 *
 * TERRAIN GEOMETRY, the definition.  IEEE binary32 unless marked f64, one rounding per written operation, no contraction:
 *     mix(a, b, t) = a*(1 - t) + b*t        (the form oracle/wgsl_ref/wgsl_rt.hpp uses for the reference's WGSL)
 *     sat(x)       = x < 0 ? 0 : (x > 1 ? 1 : x)
 *     min(a, b)    = a < b ? a : b
 *     length3 and POINT: as in "frustum and height-bounds culling" above; POINT's pair (world, n) at (u, w) is its world position and
 *     normal before the displacement
 * With G = f32(g) and the tile (side, lod, x, y), the k-th of its list:
 *   1. grid vertex (cx, cy), 0 <= cx, cy <= g: tile_uv = (f32(cx) / G, f32(cy) / G).  In the strip layout slot gi of the tile holds the
 *      grid vertex of compute_tile_uv: vpr = 2*(g + 2); r = clamp(gi % vpr, 1, vpr - 2) - 1; col = gi / vpr; (cx, cy) = (col + (r & 1), r >> 1)
 *   2. (world0, n0) = POINT's pair at ((f32(x) + tile_uv.x) / 2^lod, (f32(y) + tile_uv.y) / 2^lod);
 *      d = length3((world0 + approximate_height * n0) - view.world_position), componentwise
 *   3. morph (BT_GEOMETRY_NO_MORPH: uv = tile_uv): per axis a, even_a = f32(u32(tile_uv_a * G) & ~1u) / G — the product is rounded,
 *      then truncated, so for a G that is not a power of two it can land below cx: the reference's behaviour, kept;
 *      target = f32(log2(f64((2.0f * morph_distance) / d)));
 *      ratio = lod == 0 ? 0 : sat((target - (f32(lod) + morph_range)) / (f32(lod) - (f32(lod) + morph_range)));
 *      uv_a = mix(tile_uv_a, even_a, ratio)
 *      (world, n) = POINT's pair at ((f32(x) + uv.x) / 2^lod, (f32(y) + uv.y) / 2^lod)
 *   4. blend, from the unmorphed d as the shader does: t = min(f32(log2(f64(blend_distance / d))), f32(lod_count) - 0.00001f);
 *      bl = u32(t), saturating (0 for a t that is not > 0);
 *      ratio_b = (bl == 0 || BT_GEOMETRY_NO_BLEND) ? 0 : sat((t - (f32(bl) + blend_range)) / (f32(bl) - (f32(bl) + blend_range)))
 *   5. lookup(o), for o = 0 and, when ratio_b > 0, o = 1: the coordinate (side, lod, x, y, uv) through coordinate_change_lod
 *      (functions.wgsl:164-188, the prepass's) to L = bl - o, giving (X, Y, uv'); entry = entries[((side * lod_count + L) * tree_size +
 *      X % tree_size) * tree_size + Y % tree_size].  entry.atlas_lod == BT_INVALID_LOD: value = 0, decided before any further step (the
 *      reference leaves this case undefined).  Otherwise coordinate_change_lod to entry.atlas_lod, u_a = uv''_a * scale + offset (the
 *      attachment uv of bt_tile_tree_sample_attachment's tile sample), and value = channel x of that sample's bilinear tail from
 *      u * f32(T) - 0.5f on: one code with it (an atlas_index >= atlas_size samples as 0 there).  h_o = mix(min_height, max_height, value)
 *   6. height = ratio_b > 0 ? mix(h_0, h_1, ratio_b) : h_0;  position = world + height * n, componentwise;  normal = n;
 *      tile_index = k; coordinate_uv = uv; view_distance = d; blend_ratio = ratio_b
 * The two log2 are the platform's f64 log2 (OCML on the device), the convention bt_tile_tree_sample_attachment's compute_blend already
 * has; OCML and libm may differ in the last place of a double, which can move the f32 result only when the double sits at an f32
 * rounding boundary.
 *
 * Layouts.  Default (strip): slot k * vertices_per_tile + gi, vertices_per_tile = 2 g (g + 2), holds the vertex the reference's shader
 * computes for vertex_index = k * vertices_per_tile + gi — the first and the last vertex of each strip row twice, for the degenerate
 * triangles — so bt_indirect.vertex_count vertices drawn as one triangle strip are the reference's draw.  BT_GEOMETRY_GRID: (g + 1)^2
 * vertices per tile, slot k * (g + 1)^2 + cy * (g + 1) + cx: the same vertices without the doubles, for consumers that index them.
 *
 * bt_tile_tree_build_geometry (device form): one launch of a fixed size on the context's stream, asynchronous, no host synchronisation;
 * the kernel reads the number of final tiles on the device from what the prepass's last run left (at most the prepass's capacity) and
 * takes the tiles in list order; a tile whose last slot would fall beyond vertex_capacity (in vertices) is skipped whole.
 * vertices_device is 16-byte aligned.  vertex_capacity == 0: BT_OK, nothing touched.  Pass the view the prepass ran with: after
 * bt_frame_update the height the prepass used stays on the device, one frame ahead of what bt_tile_tree_view_state reports.
 * bt_tile_tree_tile_geometry (host form): synchronous, host arrays in and out, one launch per 32 MiB of vertices; count == 0: BT_OK,
 * nothing touched.  Both are reads (no layer is marked written for bt_run_stats.prev_zero_launches); the host form's scratch stays in
 * the context until bt_ctx_trim.
 * Refusals, all before any device work.  BT_ERR_INVALID_ARGUMENT: NULL handles (the prepass of the device form included, or one of
 * another context), NULL required arrays with a count / capacity > 0, attachment_index out of range, unknown flags, a view whose
 * `spherical` does not match the tree's model, a tile of the host list with a bad side, lod >= lod_count or x / y >= 2^lod, out_bytes
 * too small, a morph_range / blend_range that is not finite and > 0 while its stage is on.  BT_ERR_UNSUPPORTED: a non-R16 attachment;
 * grid_size 0 or above BT_GEOMETRY_MAX_GRID (a tile's (g + 1)^2 vertices are staged in LDS; the reference's default is 16). */
typedef struct bt_terrain_vertex { /* 48 bytes: three 16-byte stores per vertex */
    float position[3];      /* world + height * n (vertex_output's world_position) */
    float height;           /* the blended height */
    float normal[3];        /* n: the mesh normal (info.world_normal), not the surface normal */
    uint32_t tile_index;    /* index into the tile list */
    float coordinate_uv[2]; /* the morphed uv */
    float view_distance;    /* d (approximate_view_distance) */
    float blend_ratio;      /* ratio_b */
} bt_terrain_vertex;
enum { BT_GEOMETRY_GRID = 1, BT_GEOMETRY_NO_MORPH = 2, BT_GEOMETRY_NO_BLEND = 4 };
enum { BT_GEOMETRY_MAX_GRID = 32 };
bt_status bt_tile_tree_build_geometry(bt_tile_tree* tree, bt_atlas* atlas, uint32_t attachment_index, const bt_view_state* view /* NULL: bt_tile_tree_view_state */,
                                      const bt_tiling_prepass* prepass, uint32_t flags, void* vertices_device, uint64_t vertex_capacity);
bt_status bt_tile_tree_tile_geometry(bt_tile_tree* tree, bt_atlas* atlas, uint32_t attachment_index, const bt_view_state* view /* NULL: bt_tile_tree_view_state */,
                                     const bt_tile_coordinate* tiles, uint32_t count, uint32_t flags, bt_terrain_vertex* out_host, uint64_t out_bytes);

/* HIGH PRECISION terrain geometry: the HIGH_PRECISION branch of the vertex stage (vertex.wgsl:40-61), which the reference turns on by
 * default (DebugTerrain::high_precision).  The plain stage computes world = scale * local + translation in binary32: on a planet (one ulp
 * of 6.4e6 m is 0.5 m) every vertex near the camera sits on a half-metre lattice.  TerrainModelApproximation (terrain_model.rs:222-361) is
 * the reference's answer: per cube side a second-order Taylor series of the surface around the point under the view, computed in f64 on
 * the host and evaluated in f32 RELATIVE TO THE VIEW for every vertex nearer than precision_threshold_distance.
 *
 * THE COEFFICIENTS, bt_model_approximation_from_config.  IEEE binary64, one rounding per written operation, the expressions as written
 * (left to right, the usual precedence), C = 0.87 * 0.87.  OUR DEFINITION of the reference's powi, whose multiplication order it leaves
 * to the compiler: cube(x) = x*x*x and pow5(x) = (x*x)*(x*x)*x, both left to right; powi(2) = x*x.
 *   view = Coordinate::from_world_position(view_world_position, model); per side: (s, t) = view.project_to_side(side).uv (the functions
 *   bt_view_state_from_config uses for view_xy / view_uv), then
 *     ud = sqrt(1.0 - 4.0*C*s*(s - 1.0));  u = (2.0*s - 1.0)/ud;  u_s = 2.0*(C + 1.0)/cube(ud);  u_ss = 12.0*C*(C + 1.0)*(2.0*s - 1.0)/pow5(ud)
 *     vd, v, v_t, v_tt: the same of t
 *     l = sqrt(1.0 + u*u + v*v);  l_s = u*u_s/l;  l_t = v*v_t/l;
 *     l_ss = (u*u_ss*l*l + (v*v + 1.0)*u_s*u_s)/cube(l);  l_st = -(u*v*u_s*v_t)/cube(l);  l_tt = (v*v_tt*l*l + (u*u + 1.0)*v_t*v_t)/cube(l)
 *     a = 1.0;  a_s = -l_s;  a_t = -l_t;  a_ss = 2.0*l_s*l_s - l*l_ss;  a_st = 2.0*l_s*l_t - l*l_st;  a_tt = 2.0*l_t*l_t - l*l_tt
 *     b = u;  b_s = -u*l_s + l*u_s;  b_t = -u*l_t;  b_ss = 2.0*u*l_s*l_s - l*(2.0*u_s*l_s + u*l_ss) + u_ss*l*l;
 *     b_st = 2.0*u*l_s*l_t - l*(u_s*l_t + u*l_st);  b_tt = 2.0*u*l_t*l_t - l*u*l_tt
 *     c = v;  c_s = -v*l_s;  c_t = -v*l_t + l*v_t;  c_ss = 2.0*v*l_s*l_s - l*v*l_ss;  c_st = 2.0*v*l_s*l_t - l*(v_t*l_s + v*l_st);
 *     c_tt = 2.0*v*l_t*l_t - l*(2.0*v_t*l_t + v*l_tt) + v_tt*l*l
 *   SM(a, b, c) = SIDE_MATRICES[side] * (a, b, c) (terrain_model.rs:14-21), each component (m_x*a + m_y*b) + m_z*c with the matrix's
 *   entries 0.0, 1.0, -1.0; W = world_from_local = scale * x (+ model.position for a point), componentwise;
 *     p = W_point(SM(a, b, c)/l);  p_s = W(SM(a_s, b_s, c_s)/(l*l));  p_t = W(SM(a_t, b_t, c_t)/(l*l));
 *     p_ss = W(SM(a_ss, b_ss, c_ss)/cube(l));  p_st, p_tt likewise over cube(l)
 *   sides[side]: c = f32(p - view_world_position), c_s = f32(p_s), c_t = f32(p_t), c_ss = f32(p_ss/2.0), c_st = f32(p_st),
 *   c_tt = f32(p_tt/2.0), componentwise.  precision_threshold_distance = f32(view_config.precision_threshold_distance *
 *   TerrainModel::scale()) (tile_tree.rs:153, terrain_view_bind_group.rs:111); origin_lod = view_config.origin_lod.
 * BT_ERR_INVALID_ARGUMENT: NULL arguments, a malformed model, a non-finite position, origin_lod > 31.  BT_ERR_UNSUPPORTED: a planar
 * model — the reference fills the structure with the cube sphere's derivatives there, which describe no plane (and its planar terrains
 * are small enough for binary32).  bt_tile_tree_model_approximation: the same of the tree's model, view configuration and last view
 * position (bt_tile_tree_update / bt_frame_update), like bt_tile_tree_view_state.
 *
 * REL(coordinate) = compute_relative_position (functions.wgsl:98-115), IEEE binary32, one rounding per written operation:
 *   (side, X, Y, uv') = coordinate_change_lod(coordinate, origin_lod); per axis a with view_xy / view_uv of view.sides[side]:
 *     st_a = ((f32(i32(XY_a) - view_xy_a) + uv'_a) - view_uv_a) / 2^origin_lod;  (s, t) = st
 *   REL = ((((c + c_s*s) + c_t*t) + (c_ss*s)*s) + (c_st*s)*t) + (c_tt*t)*t, componentwise, with the coefficients of sides[side]
 *
 * THE VERTEX.  Steps 1, 2 of TERRAIN GEOMETRY as they are (d0 = step 2's d), then
 *   2h. hp = d0 < precision_threshold_distance.  Not hp: steps 3 - 6 as they are (d = d0).  hp: rel0 = REL(tile, tile_uv);
 *       d = length3(rel0 + approximate_height * n0), componentwise
 *   3h. (hp) morph as step 3 with this d; rel = REL(tile, uv); world = view.world_position + rel, componentwise; n = n0, the normal at the
 *       UNMORPHED tile_uv, as vertex.wgsl:55 has it
 *   4 - 6 with this d (blend ratio, view_distance) and this (world, n).
 * The reference's view.world_position + rel throws the series' precision away again in binary32: it relies on big_space keeping the
 * camera near the origin.  BT_GEOMETRY_VIEW_RELATIVE is the form a consumer without big_space needs: position is relative to the view,
 *   hp vertex: position = rel + height * n;   any other vertex: position = (world - view.world_position) + height * n, componentwise
 * and the consumer adds its own f64 view position.  Every other field is the same in both forms.
 * precision_threshold_distance == 0: no vertex is hp, and without VIEW_RELATIVE the output is the plain calls' byte for byte.
 *
 * The two calls take the plain calls' arguments plus the approximation, and behave as they do (layouts, capacity, launch per 32 MiB,
 * reads).  Pass an approximation and a view derived from the SAME position (bt_model_approximation_from_config and
 * bt_view_state_from_config, or bt_tile_tree_model_approximation and bt_tile_tree_view_state): REL offsets the view's view_xy / view_uv.
 * Refusals: the plain calls', plus BT_ERR_INVALID_ARGUMENT for a NULL approximation, an origin_lod that differs from the view's, a
 * precision_threshold_distance that is not finite or is negative; BT_ERR_UNSUPPORTED for the tree of a planar model.  The plain calls
 * keep refusing BT_GEOMETRY_VIEW_RELATIVE. */
typedef struct bt_side_coefficients {
    float c[3], c_s[3], c_t[3], c_ss[3], c_st[3], c_tt[3];
} bt_side_coefficients;
typedef struct bt_model_approximation { /* 448 bytes: a kernel argument of its own */
    bt_side_coefficients sides[6];
    float precision_threshold_distance; /* f32(view_config.precision_threshold_distance * TerrainModel::scale()) */
    uint32_t origin_lod;                /* the origin_lod the coefficients (and the view's view_xy / view_uv) belong to */
    uint32_t _padding[2];
} bt_model_approximation;
enum { BT_GEOMETRY_VIEW_RELATIVE = 8 }; /* the _hp calls only */
bt_status bt_model_approximation_from_config(const bt_terrain_model* model, const bt_terrain_view_config* view_config,
                                             const double view_world_position[3], bt_model_approximation* out);
bt_status bt_tile_tree_model_approximation(bt_tile_tree* tree, bt_model_approximation* out);
bt_status bt_tile_tree_build_geometry_hp(bt_tile_tree* tree, bt_atlas* atlas, uint32_t attachment_index, const bt_view_state* view /* NULL: bt_tile_tree_view_state */,
                                         const bt_model_approximation* approximation, const bt_tiling_prepass* prepass, uint32_t flags, void* vertices_device,
                                         uint64_t vertex_capacity);
bt_status bt_tile_tree_tile_geometry_hp(bt_tile_tree* tree, bt_atlas* atlas, uint32_t attachment_index, const bt_view_state* view /* NULL: bt_tile_tree_view_state */,
                                        const bt_model_approximation* approximation, const bt_tile_coordinate* tiles, uint32_t count, uint32_t flags,
                                        bt_terrain_vertex* out_host, uint64_t out_bytes);

/* One frame of one view (src/plugin.rs:46-56: TileTree::compute_requests -> TileAtlas::update's release / request half ->
 * TileTree::adjust_to_tile_atlas -> TileTree::approximate_height -> TilingPrepassNode::run) as ONE call with ONE host
 * synchronisation — the one the structure forces: the atlas's streaming state machine is host code and needs the two lists,
 * which the update kernel writes straight into pinned memory.  Everything behind it is enqueued and left running on the
 * context's stream: tile states from pinned staging, the sampled height stays on the device (the prepass kernels and the
 * next frame's update read it there; bt_tile_tree_view_state / the next bt_frame_info report it one frame late), the final
 * tile list and indirect arguments land in bt_tiling_prepass_buffers().  File loads stay with bt_atlas_update().
 * Identical lists, entries and final tiles to the separate calls (tests/test_gpu_tile_tree.py). */
enum {
    BT_FRAME_PREPASS_UNORDERED = 1, /* bt_tiling_prepass_run_unordered instead of bt_tiling_prepass_run */
    BT_FRAME_PREPASS_PLAIN = 2,     /* bt_tiling_prepass_run_plain */
    BT_FRAME_KEEP_REQUESTS = 4,     /* do not apply the lists to the atlas: the caller does (bt_tile_tree_requests / _apply_requests) */
    BT_FRAME_KEEP_HEIGHT = 8,       /* skip approximate_height */
};
typedef struct bt_frame_info {
    uint32_t released_count, requested_count; /* this frame's lists (bt_tile_tree_requests) */
    bt_status apply_status;                   /* of bt_tile_tree_apply_requests (BT_OK when skipped) */
    float approximate_height;                 /* the height this frame's update used, i.e. the previous frame's sample */
} bt_frame_info;
bt_status bt_frame_update(bt_tile_tree* tree, bt_atlas* atlas, bt_tiling_prepass* prepass /* may be NULL */,
                          const double view_world_position[3], uint32_t flags, bt_frame_info* out /* may be NULL */);

/* ---------------- path-finding: a shortest-path field over a rectangle of heights, and the route it holds
 * PATH FIELD (bt_atlas_path_field; R16 only).  IEEE binary32, one rounding per written operation, no contraction.
 * Input: the width x height rectangle of centre texels at mosaic (x0, y0) of `lod` on `side` of an R16 attachment (the rectangle of
 * bt_atlas_read_region).  It lies inside one face: a path does not cross a cube edge.  Cell (x, y), 0 <= x < width, 0 <= y < height, is
 * mosaic texel (x0 + x, y0 + y); planes are row-major, cell (x, y) at index y * width + x.
 * Cells.  raw = the centre texel.  The cell is BLOCKED when raw == 0 (no data), when its tile is one the atlas does not hold (such texels
 * read as 0), or when blocked_host[y * width + x] != 0 (the optional host mask).  Otherwise
 *     h = min_height + (max_height - min_height) * (f32(raw) / 65535.0f)                       the correctly rounded division
 * Neighbours.  k = 0..7 with (dx, dy) = (1,0), (1,1), (0,1), (-1,1), (-1,0), (-1,-1), (0,-1), (1,-1).  The edge a -> b_k exists only if
 *     both cells are inside the window and not blocked,
 *     for odd k (a diagonal) both (a.x + dx, a.y) and (a.x, a.y + dy) are inside and not blocked (no corner cutting),
 *     and the grade test below passes.
 * Edge weight w(a -> b), with cell_diag = cell_size * 1.41421356f formed once on the host:
 *     run  = k odd ? cell_diag : cell_size
 *     rise = h_b - h_a
 *     g    = fabsf(rise) / run                      the edge exists only if g <= max_grade (a NaN fails)
 *     up   = rise > 0 ? rise : 0
 *     down = rise < 0 ? -rise : 0
 *     w    = ((run * (1.0f + grade_weight * g)) + climb_weight * up) + descend_weight * down
 * All weights are >= 0, so w >= run > 0.
 * Goals: up to BT_PATH_MAX_GOALS entries {x, y, cost0}, cost0 finite and >= 0.  A goal on a blocked cell is skipped and counted.
 * Field.  D(c) = the minimum over all paths c = c_n, ..., c_0 with c_0 a goal of the left fold v_0 = cost0, v_(i+1) = v_i + w(c_(i+1) -> c_i);
 * D(c) = +inf when no path exists or c is blocked.  D is the cost of travelling FROM the cell TO a goal: climb_weight and descend_weight
 * make it direction-dependent.  fl(v + w) is monotone in v and never below v, so Dijkstra with these rounded adds computes D, every fixed
 * point of X(c) = min(goal cost0 at c, min_k (X(b_k) + w(c -> b_k))) whose values are costs of real paths equals D, and relaxation from
 * +inf reaches D in any order: both planes are functions of the input alone, bit for bit.
 * Next plane (u8): BT_PATH_BLOCKED for a blocked cell; BT_PATH_UNREACHABLE for D = +inf; BT_PATH_GOAL where a usable goal at the cell has
 * cost0 == D(c) (checked first); otherwise the smallest k with D(b_k) + w(c -> b_k) == D(c).
 * cell_size is the caller's world length of one texel.  On a cube face the texels are not uniform: one cell_size is the caller's
 * approximation of them.
 * The call: synchronous, host arrays in and out, ordered behind the work queued on the context's stream; a read: no layer is marked
 * written.  cost_out (width * height floats), next_out (width * height bytes) and stats may each be NULL.  Launches: the gather of
 * bt_atlas_read_region, one prepare launch, sweeps of the relaxation kernel in batches of 4, 8, 16, then 32 (after each batch the last
 * sweep's count of blocks that still had work is read back; 0 ends the loop; more than width * height sweeps: BT_ERR_INTERNAL), one launch
 * for the next plane.  The scratch stays in the context until bt_ctx_trim.  stats->sweeps and stats->launches describe that schedule and may differ
 * from run to run; everything else in bt_path_stats, and both planes, are functions of the input.
 * Refusals, all before anything is queued, with the outputs untouched and *stats zeroed.  BT_ERR_INVALID_ARGUMENT: what
 * bt_atlas_read_region refuses of atlas, attachment, side, lod and rectangle; NULL cost or goals; goal_count 0 or above BT_PATH_MAX_GOALS;
 * width * height above BT_PATH_MAX_CELLS; a goal outside the window or with a cost0 that is not finite or negative; a cell_size that is
 * not finite or <= 0; a weight that is negative or not finite; a max_grade that is NaN or negative (+inf is allowed); a min_height,
 * max_height or max_height - min_height that is not finite.  BT_ERR_UNSUPPORTED: a non-R16 attachment, an odd centre size.  width == 0 or
 * height == 0 (with valid arguments otherwise; the goals, which cannot lie inside, are not looked at): BT_OK, nothing touched. */
#define BT_PATH_MAX_CELLS (1u << 22)
#define BT_PATH_MAX_GOALS 4096u
enum { BT_PATH_GOAL = 8, BT_PATH_UNREACHABLE = 254, BT_PATH_BLOCKED = 255 }; /* values of the next plane besides k = 0..7 */
typedef struct bt_path_cost {
    float min_height, max_height; /* finite, with a finite difference */
    float cell_size;              /* finite, > 0 */
    float max_grade;              /* >= 0, +inf allowed */
    float grade_weight, climb_weight, descend_weight; /* finite, >= 0 */
    uint32_t _padding;
} bt_path_cost; /* 32 bytes */
typedef struct bt_path_goal {
    uint32_t x, y; /* cell of the window */
    float cost0;   /* finite, >= 0 */
} bt_path_goal;    /* 12 bytes */
typedef struct bt_path_stats {
    uint32_t cells, blocked, reachable;  /* width * height; blocked cells; cells with a finite D */
    uint32_t goals_used, goals_blocked;  /* goal entries on free / on blocked cells */
    uint32_t tiles_missing;              /* tiles of the rectangle the atlas does not hold */
    uint32_t sweeps, launches;           /* relaxation launches; all kernel launches of the call, the gather counted as one */
} bt_path_stats;
bt_status bt_atlas_path_field(bt_atlas* atlas, uint32_t attachment_index, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0,
                              uint32_t width, uint32_t height, const bt_path_cost* cost, const bt_path_goal* goals, uint32_t goal_count,
                              const uint8_t* blocked_host /* may be NULL */, float* cost_out /* may be NULL */,
                              uint8_t* next_out /* may be NULL */, bt_path_stats* stats /* may be NULL */);
/* bt_path_trace: follows a next plane from (start_x, start_y) to a goal.  Host code, no device.  Writes up to `cap` cells as (x, y)
 * pairs into out_xy (may be NULL with cap 0), start and goal included, and *count_out (may be NULL) gets the full count of cells visited.
 * *status_out: BT_PATH_TRACE_OK (ended on BT_PATH_GOAL), _BLOCKED / _UNREACHABLE (the start is such a cell; count 1), _LOOP: no goal within
 * width * height steps, a step that leaves the window, or a byte on the way that is none of k = 0..7 and BT_PATH_GOAL.  On the planes of
 * bt_atlas_path_field a _LOOP can only arise where an add was absorbed: D >= 2^24 * w makes two cells tie and point at each other.
 * Never reads outside the plane.  BT_ERR_INVALID_ARGUMENT: NULL next or status_out, NULL out_xy with cap > 0, width or height 0, a start
 * outside the window. */
enum { BT_PATH_TRACE_OK = 0, BT_PATH_TRACE_BLOCKED = 1, BT_PATH_TRACE_UNREACHABLE = 2, BT_PATH_TRACE_LOOP = 3 };
bt_status bt_path_trace(const uint8_t* next, uint32_t width, uint32_t height, uint32_t start_x, uint32_t start_y, uint32_t* out_xy,
                        uint32_t cap, uint32_t* count_out, uint32_t* status_out);

/* ---------------- hydraulic erosion: a simulation over a rectangle of heights, written back as an edit
 * EROSION (bt_atlas_erode_height; R16 only).  The shallow-water "pipe" model on a grid: rain, outflow fluxes between 4-neighbours, a
 * velocity from the fluxes, erosion or deposition towards a carrying capacity, sediment carried WITH the fluxes (a share of a cell's
 * sediment leaves with every share of its water: a fixed stencil, conservative, no data-dependent reach), evaporation.
 * Arithmetic: IEEE binary32 with subnormals kept, one rounding per written operation, no contraction; / and sqrt are correctly rounded;
 * pos(x) = x > 0 ? x : 0 (a NaN goes to 0); ((a + b) + c) + d is summed in that order.  Which NaN an invalid operation gives (its sign and
 * payload) is left open; everything else is a function of the input, bit for bit.
 * Cells and state.  The window is the width x height rectangle of centre texels at mosaic (x0, y0) of `lod` on `side` (the rectangle of
 * bt_atlas_read_region; inside one face).  Cell (x, y) is mosaic texel (x0 + x, y0 + y); planes are row-major, cell (x, y) at index
 * y * width + x.  raw = the centre texel.  A cell is ACTIVE when raw != 0 and the atlas holds its tile; every other cell is a WALL, and so
 * is everything outside the window (the simulation is closed).  A wall holds no water and no sediment, has no flux in or out, and is never
 * written.  An active cell has b (height), d (water), s (sediment) and f[0..3], the outflow towards neighbour k = 0..3 =
 * (1,0), (0,1), (-1,0), (0,-1); opp(k) = (k + 2) & 3.
 * Initial state.  range = max_height - min_height;  b = min_height + range * (f32(raw) / 65535);  d and s from water_host / sediment_host
 * (width * height floats each; 0 where the pointer is NULL; forced to 0 on walls);  f = 0: fluxes do not survive the call, so two calls of
 * n steps differ from one of 2n by the restart of the fluxes.
 * Host constants, each formed once:  rain_dt = dt * rain;  cf = (dt * gravity) * cell_size;  l2 = cell_size * cell_size;
 * two_l = 2 * cell_size;  e = evaporation * dt;  keep = 1 - (e < 1 ? e : 1).
 * One step = phase A over all cells, then B over all cells, then C over all cells.  For an active cell, n_k its neighbour k:
 *   A.  d1 = d + rain_dt;  H = b + d1
 *       f'[k] = n_k active ? pos(f[k] + cf * (H - H_(n_k))) : 0
 *       out = ((f'[0] + f'[1]) + f'[2]) + f'[3]
 *       if out * dt > d1 * l2:  K = (d1 * l2) / (out * dt);  f'[k] = f'[k] * K for every k;  out is summed again
 *   B.  in_k = n_k active ? f'_(n_k)[opp(k)] : 0;  in = ((in_0 + in_1) + in_2) + in_3
 *       d2 = pos(d1 + (dt * (in - out)) / l2)
 *       dm = 0.5 * (d1 + d2);  dm = dm > min_depth ? dm : min_depth
 *       wx = 0.5 * ((in_2 - f'[2]) + (f'[0] - in_0));  wy = 0.5 * ((in_3 - f'[3]) + (f'[1] - in_1))
 *       vx = wx / (cell_size * dm);  vy = wy / (cell_size * dm);  speed = sqrt(vx * vx + vy * vy)
 *       b_k = n_k active ? b_(n_k) : b;  gx = (b_0 - b_2) / two_l;  gy = (b_1 - b_3) / two_l;  g2 = gx * gx + gy * gy
 *       sin_a = sqrt(g2 / (1 + g2));  sin_a = sin_a > min_tilt ? sin_a : min_tilt
 *       C = (capacity * sin_a) * speed
 *       C > s:      x = erode * (C - s);    b1 = b - x;  s1 = s + x
 *       otherwise:  x = deposit * (s - C);  b1 = b + x;  s1 = s - x
 *   C.  vol = d1 * l2;  m[k] = vol > 0 ? s1 * ((f'[k] * dt) / vol) : 0
 *       mo = ((m[0] + m[1]) + m[2]) + m[3];  mi = the same sum of mi_k = n_k active ? m_(n_k)[opp(k)] : 0
 *       s2 = pos((s1 - mo) + mi);  d3 = d2 * keep
 *       the next state: b1, d3, s2, f'.
 * After `steps` steps, with b0 the initial and bT the final height of an active cell:  w = weight_host ? f32(weight) / 255 : 1
 * (weight_host: width * height bytes);  h = b0 + (bT - b0) * w.  The texel keeps its value byte for byte when the cell is a wall, when
 * w == 0, when bT == b0 bit for bit, or when h is not finite.  Otherwise, with q = (h - min_height) / range and
 * clamp(q) = q < 0 ? 0 : q > 1 ? 1 : q,
 *       t' = max(1, floor(0.5 + 65535 * clamp(q)))
 * Holes are neither made nor filled.  Sediment still in suspension is not deposited: it comes back in sediment_host or is lost.  Stability
 * (dt against cell_size, gravity and the depths) is the caller's concern; a height that is not finite cannot reach the atlas.
 * The call.  water_host / sediment_host, where given, are read before and written after the steps (d and s of the last step; 0 on walls),
 * and the call is then synchronous.  With both NULL it enqueues on the context's stream and returns as bt_atlas_write_region does.  The new
 * texels are written and the invariant F restored exactly as by bt_atlas_write_region of them over the same rectangle, from the device: the same
 * plan, the same `changed` order, the same bt_edit_stats (stats->edit).  Launches: the gather of bt_atlas_read_region, one init launch, one
 * launch per step (a workgroup owns BT_ERODE_BLOCK x BT_ERODE_BLOCK cells and recomputes a halo of three around them: the result does not depend on
 * the block size), one finish launch (stats->sim_launches = steps + 2), then those of the edit.  No atomics, no host round trip between the
 * steps.  The planes stay in the context until bt_ctx_trim: 60 bytes per cell and the staged rectangle.
 * Refusals, all before anything is queued, with the outputs untouched and *stats zeroed.  BT_ERR_INVALID_ARGUMENT: what
 * bt_atlas_read_region refuses of atlas, attachment, side, lod and rectangle; NULL changed with changed_cap > 0; NULL params; a parameter
 * outside the range its field names below; steps 0 or above BT_ERODE_MAX_STEPS; width * height above BT_ERODE_MAX_CELLS; an entry of
 * water_host or sediment_host that is negative or not finite.  BT_ERR_UNSUPPORTED: a non-R16 attachment, an odd centre size.  width == 0 or
 * height == 0 (with valid arguments otherwise; the host planes are not looked at): BT_OK, nothing touched. */
#define BT_ERODE_MAX_CELLS (1u << 22)
#define BT_ERODE_MAX_STEPS 4096u
#define BT_ERODE_BLOCK 32u
typedef struct bt_erosion_params {
    float min_height, max_height;   /* world heights of raw 0 and 65535; finite, with a finite positive difference */
    float cell_size;                /* l: world length of a texel; finite, > 0 */
    float dt;                       /* finite, > 0 */
    float rain;                     /* water height added per unit time; finite, >= 0 */
    float evaporation;              /* per unit time; finite, >= 0 */
    float gravity;                  /* finite, > 0 */
    float capacity;                 /* Kc; finite, >= 0 */
    float erode, deposit;           /* Ks, Kd; finite, in [0, 1] */
    float min_tilt;                 /* lower bound of sin(alpha); in [0, 1] */
    float min_depth;                /* lower bound of the depth a velocity is divided by; finite, > 0 */
    uint32_t steps;                 /* 1 .. BT_ERODE_MAX_STEPS */
    uint32_t _padding[3];
} bt_erosion_params;                /* 64 bytes */
typedef struct bt_erosion_stats {
    uint32_t cells, tiles_missing, steps, sim_launches; /* width * height; tiles of the rectangle the atlas does not hold; params->steps; steps + 2 */
    bt_edit_stats edit;                                 /* of the write-back */
} bt_erosion_stats;
bt_status bt_atlas_erode_height(bt_atlas* atlas, uint32_t attachment_index, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0,
                                uint32_t width, uint32_t height, const bt_erosion_params* params,
                                const uint8_t* weight_host /* may be NULL */, float* water_host /* may be NULL: in and out */,
                                float* sediment_host /* may be NULL: in and out */, bt_tile_coordinate* changed, uint32_t changed_cap,
                                bt_erosion_stats* stats /* may be NULL */);

/* ---------------- drainage: filled lakes, flow directions and drained area over a rectangle of heights
 * DRAINAGE (bt_atlas_drainage; R16 only).  Integers throughout: no float appears, so every plane is a function of the input byte for byte.
 * Window: the width x height rectangle of centre texels at mosaic (x0, y0) of `lod` on `side` of an R16 attachment (the rectangle of
 * bt_atlas_read_region; inside one face: water does not cross a cube edge).  Cell (x, y), 0 <= x < width, 0 <= y < height, is mosaic
 * texel (x0 + x, y0 + y); planes are row-major, cell (x, y) at index i = y * width + x.
 * Cells.  raw = the centre texel.  The cell is VOID when raw == 0 (no data), when its tile is one the atlas does not hold (such texels read
 * as 0), or when void_host[i] != 0 (the optional host mask).  Every other cell is ACTIVE with the height z = raw, the integer.
 * Neighbours.  k = 0..7 with (dx, dy) = (1,0), (1,1), (0,1), (-1,1), (-1,0), (-1,-1), (0,-1), (1,-1), as in the path field.  All eight
 * count; there is no corner rule.
 * Outlets.  An active cell is an OUTLET when any of its eight neighbours lies outside the window or is void: water leaves the window at its
 * edge and into no-data.  Every 8-connected set of active cells therefore holds an outlet, and everything below is finite.
 * Filled level W(c) (u16): the minimum over all 8-connected paths of active cells from c to an outlet of the largest z on the path, c and
 * the outlet included.  This is what priority-flood computes.  Equally: start from X = z on outlets and +inf on every other cell and relax
 *     X(c) = max(z(c), min_k X(n_k))
 * FROM ABOVE, in any order: every value held is the bottleneck of a real path (or +inf), so the relaxation stops at W.  "From above" is part
 * of the definition: the fixed point of that equation is not unique (two adjacent pit cells hold each other at any level below their rim),
 * and W is the largest one.  65535 serves as +inf: it bounds every W.  W - z is the depth of the lake over the cell.
 * Flat distance F(c) (u32).  c is a DRAIN cell when it is an outlet or has a neighbour with W(n_k) < W(c).  F = 0 on drain cells; otherwise
 *     F(c) = 1 + min F(n_k) over the neighbours with W(n_k) == W(c).
 * F is finite on every active cell: a cell that is neither kind of drain cell has min_k W(n_k) == W(c), and its optimal path runs through
 * cells of that W until the first one with a lower neighbour, or the outlet.
 * Direction (u8).  BT_DRAIN_VOID on a void cell.  BT_DRAIN_OUTLET on an outlet.  On any other drain cell: among the k with
 * d_k = W(c) - W(n_k) > 0 the k with the largest score_k = d_k * d_k * (k odd ? 1 : 2), formed in 64 bits (it reaches 2 * 65534^2), the
 * smallest k on a tie: steepest descent with a diagonal run of sqrt(2), without a rounding.  On any other cell: the smallest k with
 * W(n_k) == W(c) and F(n_k) == F(c) - 1.  The receiver of a cell is strictly smaller in (W, F), so the directions form a forest rooted at
 * the outlets.  BT_DRAIN_OUTLET == BT_PATH_GOAL and BT_DRAIN_VOID == BT_PATH_BLOCKED on purpose: bt_path_trace follows a direction plane
 * downstream from any active cell to its outlet as it stands, and ends BT_PATH_TRACE_OK.
 * Accumulation A(c) (u32).  w(c) = weight_host ? weight_host[i] : 1 (the optional u8 plane: rainfall, say).
 *     A(c) = w(c) + the sum of A(d) over the cells d whose receiver is c;  A = 0 on void cells.
 * With at most BT_DRAIN_MAX_CELLS cells of weight <= 255 no A reaches 2^32.
 * Outputs: filled_out (u16; 0 on void), flat_out (u32; 0 on void), direction_out (u8), accumulation_out (u32), each width * height,
 * row-major, and stats; each may be NULL.  bt_drainage_stats: every field but sweeps_fill, sweeps_flat, sweeps_accumulate and launches is
 * a function of the input; those four describe the schedule and may differ from run to run.
 * The call: synchronous, host arrays in and out, ordered behind the work queued on the context's stream; a read: no layer is marked
 * written.  Launches: the gather of bt_atlas_read_region (counted as one); one prepare launch (void and outlet classes, the initial X);
 * the fill relaxation; one launch that seeds F; the flat relaxation; one launch for the direction plane, which also seeds A = w; the
 * accumulation (X = w + the sum over the neighbours that point at the cell, ascending from w: over a forest that has one fixed point);
 * one finish launch for the counts: launches = 5 + sweeps_fill + sweeps_flat + sweeps_accumulate.  Each relaxation is enqueued in batches
 * of 4, 8, 16, then 32 sweeps; in a sweep a workgroup owns BT_DRAIN_BLOCK x BT_DRAIN_BLOCK cells and works only when a neighbour or itself
 * flagged it; after each batch the last sweep's count of blocks that still had work is read back, and 0 ends the loop (more than
 * width * height sweeps: BT_ERR_INTERNAL).  No result depends on the block size or the schedule.  The scratch, 17 bytes per cell, stays in
 * the context until bt_ctx_trim.
 * Refusals, all before anything is queued, with the outputs untouched and *stats zeroed.  BT_ERR_INVALID_ARGUMENT: what
 * bt_atlas_read_region refuses of atlas, attachment, side, lod and rectangle; width * height above BT_DRAIN_MAX_CELLS.
 * BT_ERR_UNSUPPORTED: a non-R16 attachment, an odd centre size.  width == 0 or height == 0 (with valid arguments otherwise): BT_OK,
 * nothing touched. */
#define BT_DRAIN_MAX_CELLS (1u << 22)
#define BT_DRAIN_BLOCK 32u
enum { BT_DRAIN_OUTLET = 8, BT_DRAIN_VOID = 255 }; /* values of the direction plane besides k = 0..7 */
typedef struct bt_drainage_stats {
    uint32_t cells, voids, outlets;                           /* width * height; void cells; outlets */
    uint32_t tiles_missing;                                   /* tiles of the rectangle the atlas does not hold */
    uint32_t filled, flats;                                   /* cells with W > z; cells with F > 0 */
    uint32_t max_flat_distance, max_accumulation;             /* the largest F; the largest A */
    uint32_t outflow;                                         /* the sum of A over the outlets = the sum of w over the active cells */
    uint32_t sweeps_fill, sweeps_flat, sweeps_accumulate;     /* relaxation launches of the three fixed points */
    uint32_t launches;                                        /* all kernel launches of the call, the gather counted as one */
    uint32_t _padding[3];
} bt_drainage_stats; /* 64 bytes */
bt_status bt_atlas_drainage(bt_atlas* atlas, uint32_t attachment_index, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0,
                            uint32_t width, uint32_t height, const uint8_t* void_host /* may be NULL */,
                            const uint8_t* weight_host /* may be NULL */, uint16_t* filled_out /* may be NULL */,
                            uint32_t* flat_out /* may be NULL */, uint8_t* direction_out /* may be NULL */,
                            uint32_t* accumulation_out /* may be NULL */, bt_drainage_stats* stats /* may be NULL */);

/* ---------------- viewshed: what a set of observers can see of a rectangle of heights
 * VIEWSHED (bt_atlas_viewshed; R16 only).  Integers throughout: no float appears, so every plane is a function of the input byte for byte.
 * The ground is flat: the curvature of the earth and refraction are out of scope.
 * Window: the width x height rectangle of centre texels at mosaic (x0, y0) of `lod` on `side` of an R16 attachment (the rectangle of
 * bt_atlas_read_region).  Cell (x, y) is mosaic texel (x0 + x, y0 + y); planes are row-major, cell (x, y) at index i = y * width + x.
 * Cells.  raw = the centre texel.  The cell is VOID when raw == 0 (no data) or when its tile is one the atlas does not hold (such texels
 * read as 0; the tiles are counted in tiles_missing).  Every other cell is ACTIVE with the height z = raw, the integer.  On a sight line a
 * void cell is ground of height 0.
 * Observers: up to BT_VIEWSHED_MAX_OBSERVERS of bt_viewshed_observer {x, y, eye_height, radius}, in cells of the window.  The eye is at
 * E = z(O) + eye_height.  radius == 0: unlimited; otherwise the observer COVERS the cells with dx^2 + dy^2 <= radius^2 (in 64 bits).  An
 * observer on a void cell is SKIPPED and counted (the path field's rule for goals on blocked cells); every other one is USED.  Two
 * observers on one cell are two observers.
 * The line from O to a target T: dx = tx - ox, dy = ty - oy, n = max(|dx|, |dy|).  Its n - 1 interior points are P_j = O + (dx, dy) j / n,
 * j = 1..n-1.  On the major axis (x when |dx| >= |dy|; on an exact diagonal either, with the same result) the coordinate of P_j is an
 * integer.  On the minor axis it is o + m j / n with m the signed minor difference: q = floor(m j / n), the true floor, towards minus
 * infinity, and r = m j - q n in [0, n).  The ground at P_j is the linear interpolation of the cells at minor positions o + q and
 * o + q + 1, kept as a numerator over n:  G_j = z_a (n - r) + z_b r  (z_b is not read when r == 0).  With this floor the line from T to
 * O meets the same points with the same weights, so two cells see each other or neither does when eye and target heights are equal.
 * Clearance.  S_j = G_j - E n.  The line of sight to a target top at height Z passes P_j iff (Z - E) j >= S_j: grazing counts as seen.  So
 * Z - E >= M = max_j ceil(S_j / j), the ceiling of the signed rational towards plus infinity (found as the largest rational by
 * cross-multiplication, with one division at the end: the ceiling is monotone).  C_o(T) = max(0, E + M - z(T)), and 0 when n <= 1: the
 * smallest whole height above the ground at T that observer o sees.  It does not depend on target_height.
 * Bounds: width, height <= BT_VIEWSHED_MAX_SIDE; width * height <= BT_VIEWSHED_MAX_CELLS; eye_height, target_height <= 65535.  Hence
 * G_j < 2^31, E n < 2^32, |S_j| < 2^32, every cross product < 2^48, and C < 2^31 + 2^17: nothing saturates.
 * Outputs, each may be NULL, row-major.  clearance_out (u32): the minimum of C_o over the used observers that cover the cell;
 * BT_VIEWSHED_NONE on a void cell and on a cell no used observer covers.  count_out (u8): the number of used, covering observers with
 * C_o <= target_height; 0 on void cells.  mask_out (u64): bit o set for exactly those observers, o the index in the caller's array.
 * bt_viewshed_stats: every field but launches is a function of the input.
 * The call: synchronous, host arrays in and out, ordered behind the work queued on the context's stream; a read: no layer is marked
 * written.  Launches: the gather of bt_atlas_read_region (counted as one); one that transposes the texels; the line walk in two, the
 * x-major lines on the transposed texels and then the y-major ones, a wave to 64 consecutive targets along the minor axis, the observers
 * looped inside it (no atomic: no result depends on a schedule); one finish launch for the counts: launches = 5.  The scratch, 9 bytes
 * per cell and 8 more when the mask is asked for, stays in the context until bt_ctx_trim.
 * Refusals, all before anything is queued, with the outputs untouched and *stats zeroed.  BT_ERR_INVALID_ARGUMENT: what
 * bt_atlas_read_region refuses of atlas, attachment, side, lod and rectangle; NULL observers; observer_count 0 or above
 * BT_VIEWSHED_MAX_OBSERVERS; an eye_height or target_height above 65535; a side above BT_VIEWSHED_MAX_SIDE; width * height above
 * BT_VIEWSHED_MAX_CELLS; an observer outside the window.  BT_ERR_UNSUPPORTED: a non-R16 attachment, an odd centre size.  width == 0 or
 * height == 0 (with valid arguments otherwise; no observer can lie in such a window, and none is looked at): BT_OK, nothing touched. */
#define BT_VIEWSHED_NONE 0xFFFFFFFFu
#define BT_VIEWSHED_MAX_OBSERVERS 64u
#define BT_VIEWSHED_MAX_SIDE 32768u
#define BT_VIEWSHED_MAX_CELLS (1u << 22)
typedef struct bt_viewshed_observer {
    uint32_t x, y;        /* the cell, in the window */
    uint32_t eye_height;  /* above the ground at the cell, <= 65535 */
    uint32_t radius;      /* in cells; 0 = unlimited */
} bt_viewshed_observer; /* 16 bytes */
typedef struct bt_viewshed_stats {
    uint32_t cells, voids;                           /* width * height; void cells */
    uint32_t tiles_missing;                          /* tiles of the rectangle the atlas does not hold */
    uint32_t observers_used, observers_skipped;      /* on active cells; on void ones */
    uint32_t covered, visible;                       /* active cells at least one used observer covers; cells with count > 0 */
    uint32_t max_clearance;                          /* the largest clearance that is not BT_VIEWSHED_NONE (0: there is none) */
    uint64_t samples;                                /* the sum of max(n - 1, 0) over the (used observer, covered active cell) pairs */
    uint32_t launches;                               /* all kernel launches of the call, the gather counted as one */
    uint32_t _padding[5];
} bt_viewshed_stats; /* 64 bytes */
bt_status bt_atlas_viewshed(bt_atlas* atlas, uint32_t attachment_index, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0,
                            uint32_t width, uint32_t height, const bt_viewshed_observer* observers, uint32_t observer_count,
                            uint32_t target_height, uint32_t* clearance_out /* may be NULL */, uint8_t* count_out /* may be NULL */,
                            uint64_t* mask_out /* may be NULL */, bt_viewshed_stats* stats /* may be NULL */);

/* ---------------- distance field: the exact squared distance to the nearest seed cell of a rectangle, and which seed it is
 * DISTANCE (bt_atlas_distance_field; R16 and Rgba8).  Integers throughout: no float appears, so every plane is a function of the input byte
 * for byte.  The field is purely geometric: there is no void class.
 * Window: the width x height rectangle of centre texels at mosaic (x0, y0) of `lod` on `side` of attachment attachment_index (the rectangle
 * of bt_atlas_read_region; inside one face).  Cell (x, y) is mosaic texel (x0 + x, y0 + y); planes are row-major, cell (x, y) at index
 * i = y * width + x.  Texels of tiles the atlas does not hold read as 0; the tiles are counted in tiles_missing.
 * Seeds: bt_distance_seeds {channel, lo, hi, flags}.  v(c) = the raw u16 of an R16 texel (channel must be 0), byte `channel` (0..3) of an
 * Rgba8 one.
 *     from_texels(c) = (flags & BT_DISTANCE_FROM_TEXELS) && lo <= v(c) && v(c) <= hi
 *     from_host(c)   = seed_host && seed_host[i] != 0                     (seed_host: an optional plane of width * height bytes)
 *     seed(c)        = (from_texels(c) || from_host(c)) XOR ((flags & BT_DISTANCE_INVERT) != 0)
 * So: a sea level is FROM_TEXELS with lo = 0, hi = the level; no-data and missing tiles are lo = hi = 0; rivers are a host plane made from
 * bt_atlas_drainage's accumulation_out; INVERT gives the distance to the outside from within.
 * Field.  S = the set of seed cells.  For every cell c = (x, y):
 *     dist2(c)   = the minimum over s = (sx, sy) in S of (x - sx)^2 + (y - sy)^2                                    (u32)
 *     nearest(c) = the smallest index sy * width + sx among the seeds that attain that minimum                      (u32)
 * Both are BT_DISTANCE_NONE when S is empty.  A seed has dist2 = 0 and nearest = its own index.
 * Bounds: width, height <= BT_DISTANCE_MAX_SIDE; width * height <= BT_DISTANCE_MAX_CELLS.  Hence dist2 < 2^27: nothing saturates.
 * The separable reading, which an implementation may rely on.  Per column x, r(x, y) is the row of the seed of column x nearest to row y,
 * the upper one (the smaller row) on a tie; none when the column holds no seed.  Then (dist2, nearest)(x, y) is the lexicographic minimum
 * over the columns i that hold a seed of ((x - i)^2 + (y - r(i, y))^2, r(i, y), i): a seed of column i that attains the minimum is a
 * nearest one of its column, and of two such seeds r is the one with the smaller index.
 * Bake (optional): bt_distance_bake {attachment, channel, reach, flags} writes a proximity byte into channel `channel` of the Rgba8
 * attachment `attachment` of the same atlas, over the same rectangle.
 *     b(c) = min(255, isqrt64((uint64(dist2) * 65025) / (uint64(reach) * reach))),   isqrt64 = the floor square root;  255 when dist2 is NONE
 * which is floor(255 * sqrt(dist2) / reach) capped at 255, exactly: the floor of the square root of a floor is the floor of the square
 * root.  reach is 1..65535.  With BT_DISTANCE_BAKE_NEAR the byte is 255 - b: 255 on the seeds, 0 from `reach` on.  The other three bytes of
 * every texel keep their values.  The write is an edit like any other: the destination rectangle is gathered, the byte merged on the
 * device, and the texels written and the invariant F restored exactly as by bt_atlas_write_region of them over the rectangle: the same
 * plan, the same `changed` order, the same bt_edit_stats (stats->edit).  The destination may be the source attachment (seed on one
 * channel, bake another).  Without `bake` the call is a read: no layer is marked written, and `changed` is not written.
 * Outputs: dist2_out, nearest_out (u32, width * height, row-major) and stats; each may be NULL.  bt_distance_stats: every field but
 * launches is a function of the input.
 * The call: synchronous, host arrays in and out through the context's staging ring, ordered behind the work queued on the context's
 * stream.  Launches: the gather of bt_atlas_read_region (counted as one); the column phase in three: a lane to a column of a band of
 * BT_DISTANCE_BAND rows notes the band's first and last seed row, a lane to a column carries them across the bands, and a lane to a column
 * of a band writes r for its rows; the row phase: a workgroup to a row, that row of r in LDS, a lane to a cell searching outwards from its
 * own column until dx^2 exceeds the best distance; one finish launch for the counts, which also merges the baked byte: launches = 6.  With
 * a bake the gather of the destination is one more, launches = 7, and the launches of the edit follow in stats->edit.launches.  The count
 * depends on the arguments only.  No result depends on a schedule.  The scratch stays in the context until bt_ctx_trim: 10 bytes per cell
 * and the texel (2 or 4), 1 more with seed_host, 4 bytes per column and band, and with a bake the staged rectangle (4 per cell).
 * Refusals, all before anything is queued, with the outputs untouched and *stats zeroed.  BT_ERR_INVALID_ARGUMENT: what
 * bt_atlas_read_region refuses of atlas, attachment, side, lod and rectangle; NULL seeds; neither FROM_TEXELS nor seed_host; unknown flag
 * bits; lo > hi with FROM_TEXELS; a channel above 3, or non-zero on R16; hi above 65535 on R16, above 255 on Rgba8; a side above
 * BT_DISTANCE_MAX_SIDE; width * height above BT_DISTANCE_MAX_CELLS; NULL changed with changed_cap > 0; in a bake: an attachment out of
 * range, a channel above 3, reach 0 or above 65535, unknown flag bits.  BT_ERR_UNSUPPORTED: an odd centre size; a bake destination that is
 * not Rgba8, or whose texture_size or border_size differs from the source's.  width == 0 or height == 0 (with valid arguments otherwise;
 * seed_host is not looked at): BT_OK, nothing touched. */
#define BT_DISTANCE_NONE 0xFFFFFFFFu
#define BT_DISTANCE_MAX_SIDE 8192u
#define BT_DISTANCE_MAX_CELLS (1u << 22)
#define BT_DISTANCE_BAND 32u
enum { BT_DISTANCE_FROM_TEXELS = 1, BT_DISTANCE_INVERT = 2 }; /* bt_distance_seeds.flags */
enum { BT_DISTANCE_BAKE_NEAR = 1 };                           /* bt_distance_bake.flags */
typedef struct bt_distance_seeds {
    uint32_t channel;  /* of an Rgba8 texel, 0..3; 0 on R16 */
    uint32_t lo, hi;   /* the band of texel values that are seeds, both ends included (FROM_TEXELS) */
    uint32_t flags;    /* BT_DISTANCE_FROM_TEXELS | BT_DISTANCE_INVERT */
} bt_distance_seeds; /* 16 bytes */
typedef struct bt_distance_bake {
    uint32_t attachment;  /* the Rgba8 attachment that takes the byte */
    uint32_t channel;     /* 0..3 */
    uint32_t reach;       /* in cells, 1..65535: the distance at which b reaches 255 */
    uint32_t flags;       /* BT_DISTANCE_BAKE_NEAR */
} bt_distance_bake; /* 16 bytes */
typedef struct bt_distance_stats {
    uint32_t cells, seeds;      /* width * height; seed cells */
    uint32_t tiles_missing;     /* tiles of the rectangle the source attachment does not hold */
    uint32_t max_dist2;         /* the largest dist2 (0 when S is empty) */
    uint64_t sum_dist2;         /* the sum of dist2 over the cells (0 when S is empty) */
    uint32_t launches;          /* the kernel launches of the call before the edit's, the gathers counted as one each */
    uint32_t _padding;
    bt_edit_stats edit;         /* of the bake's write-back; zero without a bake */
} bt_distance_stats; /* 64 bytes */
bt_status bt_atlas_distance_field(bt_atlas* atlas, uint32_t attachment_index, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0,
                                  uint32_t width, uint32_t height, const bt_distance_seeds* seeds,
                                  const uint8_t* seed_host /* may be NULL */, uint32_t* dist2_out /* may be NULL */,
                                  uint32_t* nearest_out /* may be NULL */, const bt_distance_bake* bake /* may be NULL */,
                                  bt_tile_coordinate* changed, uint32_t changed_cap, bt_distance_stats* stats /* may be NULL */);

/* ---------------- skyline: the horizon of every cell of a rectangle of heights in a set of directions, sun hours, a shadow bake
 * SKYLINE (bt_atlas_skyline; R16 only).  Integers throughout: no float appears, so every plane is a function of the input byte for byte.
 * Out of scope: a distance cap on the line (it breaks the hull below); a receiver height above the ground (it needs a tangent search
 * into the hull); the curvature of the earth; suns below the horizontal.
 * Window: the width x height rectangle of centre texels at mosaic (x0, y0) of `lod` on `side` of an R16 attachment (the rectangle of
 * bt_atlas_read_region).  Cell (x, y) is mosaic texel (x0 + x, y0 + y); planes are row-major, cell (x, y) at index i = y * width + x.
 * z(c) = the raw u16.  Texels without data, and texels of tiles the atlas does not hold, read as 0 and are ground of height 0; the tiles
 * are counted in tiles_missing and the cells with z == 0 in voids.  There is no void class for results: every plane is a function of
 * the z plane alone.
 * Directions: up to BT_SKYLINE_MAX_DIRECTIONS of bt_skyline_direction {dx, dy, sun_num, sun_den}.  (dx, dy) points towards the sun, in
 * cells, not both 0, |dx|, |dy| <= BT_SKYLINE_MAX_COMPONENT.  The sun rises sun_num / sun_den raw height units per step of the major
 * axis; sun_den is 1..65535 and sun_num <= 2^31 - 1.
 * Digital lines.  The major axis is x when |dx| >= |dy|, otherwise y; the wording is for x-major, y-major exchanges the axes.
 * n = |dx|, s = sign(dx), m = dy * s.  off(x) = floor((2 x m + n) / (2 n)), the true floor, towards minus infinity, x counted in the
 * window.  Cell (x, y) lies on line j = y - off(x).  Every cell lies on exactly one line; the cells of a line inside the window occupy a
 * contiguous range of x; since off(0) = 0 and off moves by at most one per step, the lines are the j from -max(off) to
 * height - 1 - min(off), height + |off(width - 1)| of them.  Scaling (dx, dy) by a positive integer gives the same lines, (-dx, -dy) the
 * same lines walked the other way, and an exact diagonal the same lines on either axis.  The cells AHEAD of a are the cells b of its
 * line with (x_b - x_a) s > 0, at t = |x_b - x_a| steps.
 * Skyline.  For direction k and cell a, the HORIZON CELL is, among the cells ahead, the one that maximises the rational (z_b - z_a) / t,
 * negatives included; on a tie the nearest one.  steps[k][a] = its t (u16), rise[k][a] = z_b - z_a (i32); both 0 when no cell is ahead.
 * Bounds: width, height <= BT_SKYLINE_MAX_SIDE; width * height <= BT_SKYLINE_MAX_CELLS.  Hence t <= 32767, |rise| <= 65535 and every
 * cross product rise * t' is at most 65535 * 32767 < 2^31; they are formed in 64 bits anyway.
 * Sun.  Cell a is LIT by direction k iff rise * sun_den <= steps * sun_num, in 64 bits (< 2^32 against < 2^46): grazing counts as lit,
 * as in VIEWSHED, and a cell with nothing ahead is lit.  mask (u64): bit k set iff lit by direction k.  count (u8): the number of set
 * bits.
 * The hull reading, which an implementation may rely on.  Walk a line against its direction, keeping the upper convex hull of the cells
 * walked so far as a stack, the nearest on top.  For the new cell a, pop the top p while there is a q beneath it with
 * (z_q - z_a) t_p > (z_p - z_a) t_q.  The test is strict, so a collinear p stays: that is the nearest-on-a-tie rule.  The top is then a's
 * horizon cell; push a.  Each cell is pushed once and popped at most once, so a direction costs a number of steps linear in the cells.
 * Bake (optional): bt_skyline_bake {attachment, channel, flags, _padding} writes b = floor(255 * count / direction_count) into channel
 * `channel` of the Rgba8 attachment `attachment` of the same atlas, over the same rectangle; with BT_SKYLINE_BAKE_SHADE the byte is
 * 255 - b.  With one direction it is a shadow map of 0 and 255.  The other three bytes of every texel keep their values.  The write is
 * an edit like any other: the destination rectangle is gathered, the byte merged on the device, and the texels written and the atlas
 * invariant restored exactly as by bt_atlas_write_region of them over the rectangle: the same plan, the same `changed` order, the same
 * bt_edit_stats (stats->edit).  Without `bake` the call is a read: no layer is marked written, and `changed` is not written.
 * Outputs, each may be NULL.  steps_out (u16) and rise_out (i32): direction_count planes of width * height, direction-major.  mask_out
 * (u64) and count_out (u8): one plane.  bt_skyline_stats: every field but launches is a function of the input.
 * bt_skyline_line_count(width, height, dx, dy, &lines, &longest): the number of lines of one direction and the cells of the longest,
 * without a device; 0 and 0 for an empty window.  It refuses a zero vector and a component above BT_SKYLINE_MAX_COMPONENT.
 * The call: synchronous, host arrays in and out through the context's staging ring, ordered behind the work queued on the context's
 * stream.  Launches: the gather of bt_atlas_read_region (counted as one); one that transposes the texels; then per batch of directions
 * the walk and a finish.  The walk runs the batch's directions as a grid dimension.  The lines j and j + (length of the minor axis) are
 * never in the window at the same major coordinate, so they share a lane, one after the other: a lane to each of the minor axis'
 * residues, a wave to 64 consecutive lines.  x-major directions walk the transposed texels and y-major ones the texels as they lie, so
 * consecutive lanes read consecutive addresses at each step.  The top two hull entries stay in registers and the rest lies in scratch,
 * 4 bytes a cell and direction in flight; a batch is B = min(direction_count, max(1, floor(BT_SKYLINE_STACK_BUDGET / (4 * width *
 * height)))) directions, 16 at 2^22 cells.  The finish, a lane to a cell, ORs the batch's bits into the mask (one writer per cell, no
 * atomic); the last one also forms count and the baked byte.  launches = 2 + 2 * ceil(direction_count / B), one more with a bake for
 * the gather of the destination, whose edit's launches follow in stats->edit.launches.  The count depends on the arguments only.  No
 * result depends on a schedule.  The scratch stays in the context until bt_ctx_trim: 13 bytes per cell, 10 more per direction of a
 * batch, and with a bake the staged rectangle (4 per cell).
 * Refusals, all before anything is queued, with the outputs untouched and *stats zeroed.  BT_ERR_INVALID_ARGUMENT: what
 * bt_atlas_read_region refuses of atlas, attachment, side, lod and rectangle; NULL directions; direction_count 0 or above
 * BT_SKYLINE_MAX_DIRECTIONS; a zero vector; a component above BT_SKYLINE_MAX_COMPONENT; sun_den 0 or above 65535; sun_num above
 * 2^31 - 1; a side above BT_SKYLINE_MAX_SIDE; width * height above BT_SKYLINE_MAX_CELLS; NULL changed with changed_cap > 0; in a bake:
 * an attachment out of range, a channel above 3, unknown flag bits.  BT_ERR_UNSUPPORTED: a non-R16 attachment; an odd centre size; a
 * bake destination that is not Rgba8, or whose texture_size or border_size differs from the source's.  width == 0 or height == 0 (with
 * valid arguments otherwise): BT_OK, nothing touched. */
#define BT_SKYLINE_MAX_DIRECTIONS 64u
#define BT_SKYLINE_MAX_COMPONENT 1024
#define BT_SKYLINE_MAX_SIDE 32768u
#define BT_SKYLINE_MAX_CELLS (1u << 22)
#define BT_SKYLINE_STACK_BUDGET (256ull << 20) /* bytes of hull-stack scratch in flight */
enum { BT_SKYLINE_BAKE_SHADE = 1 }; /* bt_skyline_bake.flags */
typedef struct bt_skyline_direction {
    int32_t  dx, dy;            /* towards the sun, in cells; not both 0; |dx|, |dy| <= BT_SKYLINE_MAX_COMPONENT */
    uint32_t sun_num, sun_den;  /* the sun's rise in raw height units per step of the major axis: num / den; den 1..65535, num <= 2^31 - 1 */
} bt_skyline_direction; /* 16 bytes */
typedef struct bt_skyline_bake {
    uint32_t attachment;  /* the Rgba8 attachment that takes the byte */
    uint32_t channel;     /* 0..3 */
    uint32_t flags;       /* BT_SKYLINE_BAKE_SHADE */
    uint32_t _padding;
} bt_skyline_bake; /* 16 bytes */
typedef struct bt_skyline_stats {
    uint32_t cells, voids;      /* width * height; cells with z == 0 */
    uint32_t tiles_missing;     /* tiles of the rectangle the source attachment does not hold */
    uint32_t directions;        /* direction_count */
    uint32_t lines;             /* the lines, summed over the directions */
    uint32_t longest_line;      /* the cells of the longest line of any direction */
    uint32_t max_steps;         /* the largest entry of the steps planes */
    uint32_t launches;          /* the kernel launches of the call before the edit's, the gathers counted as one each */
    uint64_t lit;               /* the sum of count over the cells */
    uint64_t sum_steps;         /* the sum of the steps planes */
    bt_edit_stats edit;         /* of the bake's write-back; zero without a bake */
} bt_skyline_stats; /* 80 bytes */
bt_status bt_skyline_line_count(uint32_t width, uint32_t height, int32_t dx, int32_t dy, uint32_t* lines /* may be NULL */,
                                uint32_t* longest /* may be NULL */);
bt_status bt_atlas_skyline(bt_atlas* atlas, uint32_t attachment_index, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0,
                           uint32_t width, uint32_t height, const bt_skyline_direction* directions, uint32_t direction_count,
                           uint16_t* steps_out /* may be NULL */, int32_t* rise_out /* may be NULL */, uint64_t* mask_out /* may be NULL */,
                           uint8_t* count_out /* may be NULL */, const bt_skyline_bake* bake /* may be NULL */, bt_tile_coordinate* changed,
                           uint32_t changed_cap, bt_skyline_stats* stats /* may be NULL */);

/* ---------------- shapes: polygons and strokes rasterised into a rectangle of a layer, exactly
 * SHAPES (bt_atlas_rasterize_shapes, bt_shapes_check; R16 and Rgba8).  Integers throughout: no float appears and there is no tolerance
 * anywhere, so every plane and every texel is a function of the input byte for byte.
 * Window: the width x height rectangle of centre texels at mosaic (x0, y0) of `lod` on `side` of attachment attachment_index (the rectangle
 * of bt_atlas_read_region; inside one face).  Cell (cx, cy) is mosaic texel (x0 + cx, y0 + cy); planes are row-major, cell (cx, cy) at
 * index cy * width + cx.  Bounds: width, height <= BT_SHAPES_MAX_SIDE; width * height <= BT_SHAPES_MAX_CELLS.
 * Coordinates: bt_shape_vertex {x, y}, int32, in units of 1/256 cell relative to the window's origin.  The sample point of cell (cx, cy)
 * is P = (256 cx, 256 cy): as for the brushes, a texel's position is the integer itself.  |x|, |y| <= BT_SHAPES_MAX_COORD = 2^23, so a
 * shape may lie partly or wholly outside the window.  Widths: a difference of two points is below 2^25 and fits int32; a dot or cross
 * product of two differences is below 2^51 and fits int64; the square of a cross product needs 128 bits.
 * Entries and shapes.  The list is an array of bt_shape {kind, flags, first_vertex, vertex_count, half_width, op, value, _pad}, 32 bytes
 * each; an entry's vertices are vertices[first_vertex .. first_vertex + vertex_count).  kind: BT_SHAPE_POLYGON (one contour) or
 * BT_SHAPE_STROKE (a polyline with a width).  flags: BT_SHAPE_NONZERO (polygon: the non-zero fill rule; otherwise even-odd),
 * BT_SHAPE_MORE (polygon: the next entry is a further contour of the same polygon), BT_SHAPE_CLOSED (stroke).  A SHAPE is a stroke entry
 * or a maximal run of polygon entries linked by MORE; the entries of a run agree in kind, op, value and NONZERO, and the last entry of
 * the list does not carry MORE.  Shapes are numbered k = 0, 1, ... in list order.  Limits: at most BT_SHAPES_MAX_SHAPES shapes,
 * BT_SHAPES_MAX_ENTRIES entries and BT_SHAPES_MAX_VERTICES vertices; a contour has >= 3 vertices and a stroke >= 1; half_width <=
 * BT_SHAPES_MAX_HALF_WIDTH (1/256 cell) and is 0 on a polygon; value <= 65535; _pad is 0; vertex ranges lie inside the array.
 * Coverage of P by a polygon.  The winding number w is a sum over every contour of the shape and every edge a -> b of it (consecutive
 * vertices, the last back to the first).  With c = (b - a) x (P - a) = (b.x - a.x)(P.y - a.y) - (b.y - a.y)(P.x - a.x) in int64:
 *     +1 when a.y <= P.y < b.y and c > 0;        -1 when b.y <= P.y < a.y and c < 0.
 * P is covered when w != 0 (NONZERO) or w is odd (even-odd).  Hence a horizontal edge never counts; a sample point exactly on an edge or
 * a vertex is decided by the rule alone (the axis-aligned square with corners on the sample points (2, 2) and (6, 6) covers the cells
 * 2..5 on both axes, whichever way round it is listed); reversing a contour negates w.
 * Coverage of P by a stroke, r = half_width.  Its segments are (v_i, v_i+1); with CLOSED and n >= 2 also (v_n-1, v_0); with n == 1 the
 * degenerate (v_0, v_0).  P is covered when some segment a, b passes: with d = b - a, e = P - a, L = d.d, t = e.d,
 *     L == 0 or t <= 0:  e.e <= r^2;       t >= L:  (P - b).(P - b) <= r^2;       otherwise:  (d x e)^2 <= r^2 L, compared in 128 bits.
 * Round caps and round joins follow from the union; r = 0 covers exactly the sample points that lie on a segment.
 * Planes.  count(c) = min(255, the number of shapes that cover c) (u8).  last(c) = the largest k that covers c, BT_SHAPES_NONE when none
 * does (u16).
 * Fold.  The running value starts at the texel's value, and the shapes that cover the cell apply in list order: op BT_SHAPE_SET (value),
 * _MAX, _MIN, _ADD (running + value), _SUB (running - value).  R16: a texel equal to 0 (no data) is never changed and every result is
 * clamped to [1, 65535]: holes are neither filled nor made, as with the brushes.  Rgba8: `channel` 0..3 selects the byte, value <= 255,
 * the result is clamped to [0, 255], the other three bytes keep their values; there is no hole rule, as with the distance field's bake.
 * Boxes.  The box of shape k, per axis, over all its vertices, with r = half_width (0 for a polygon) and n = width or height:
 *     lo = max(0, ceil((min - r) / 256)),   hi = min(n - 1, floor((max + r) / 256)),   the division mathematical;
 * empty when lo > hi on either axis, written {1, 1, 0, 0}.  No cell outside its box is covered.  Stroke: a covered P lies within r of a
 * point of a segment, hence within r of [min, max] on each axis.  Polygon: an edge counts only with P.y in its y-range, and only when it
 * meets the row of P strictly to the right of P (c = (b.y - a.y)(x_edge - P.x)), so beyond max x nothing counts, and before min x every
 * edge in range counts, which sums to 0 on a closed contour.
 * bt_shapes_check validates a list by the rules above and writes the boxes (boxes_out, one per shape, may be NULL), the number of shapes
 * (shape_count_out, may be NULL) and, on a refusal, the index of the offending entry (bad_entry_out, may be NULL; BT_SHAPES_NO_ENTRY
 * when the defect is not one entry's, and on success), without a device; the device call uses the same function.
 * The write.  U = the union box of all shapes.  Without BT_SHAPES_DRY_RUN the texels of U are gathered, folded on the device and
 * written, and the invariant F restored exactly as by bt_atlas_write_region of those texels over U: the same plan, the same `changed`
 * order, the same bt_edit_stats (stats->edit).  Time is proportional to U, not to the window.  With U empty: BT_OK, nothing written.
 * With DRY_RUN the call is a read: no layer is marked written, `changed` is not written, stats->edit is zero; both planes are produced.
 * Outputs: count_out (u8) and last_out (u16), width * height, row-major, each may be NULL; outside U they are 0 and BT_SHAPES_NONE.
 * bt_shapes_stats: cells = width * height; shapes; shapes_culled = shapes with an empty box; covered = cells with count > 0; written =
 * texels of U whose folded value differs from the gathered one; tiles_missing = tiles of U the atlas does not hold (their texels are
 * gathered as 0, folded and counted like any other, and not stored); box = U.  Every field but launches is a function of the input.
 * The call: synchronous, host arrays in and out through the context's staging ring, ordered behind the work queued on the context's
 * stream.  Launches: the gather of U (counted as one) and ONE raster launch: launches = 2, or 0 when U is empty; the launches of the
 * edit follow in stats->edit.launches.  The count depends on the arguments only.  The raster: a workgroup of 256 lanes owns a block of
 * BT_SHAPES_BLOCK_W x BT_SHAPES_BLOCK_H cells of U, a lane BT_SHAPES_BLOCK_H / 4 cells of one column, whose running value, count, last
 * and winding number stay in registers across the whole list.  The shapes are walked in list order; one whose box misses the block is
 * skipped.  Vertices are staged through LDS BT_SHAPES_CHUNK edges at a time (the chunk also holds the end of its last edge, so an edge
 * that spans two chunks and the closing edge need nothing special).  A wave tests 64 edges of the chunk at a time, a lane to an edge,
 * and walks only those that can touch its cells: an edge whose y-range misses the wave's rows is skipped, and one that lies wholly to
 * one side of the block is resolved without the cross product; neither changes a result.  No atomics but one add
 * per workgroup to each of `covered` and `written`.  No result depends on a schedule.  The scratch stays in the context until
 * bt_ctx_trim: the vertices, the entries, 32 bytes per shape, and 3 bytes and a texel per cell of U.
 * Refusals, all before anything is queued, with the outputs untouched and *stats zeroed.  BT_ERR_INVALID_ARGUMENT: what
 * bt_atlas_read_region refuses of atlas, attachment, side, lod and rectangle; NULL vertices or shapes with a non-zero count; everything
 * bt_shapes_check refuses (the message names the entry); a channel above 3, or non-zero on R16; a value above 255 on Rgba8; unknown
 * bits in `flags`; a side above BT_SHAPES_MAX_SIDE; width * height above BT_SHAPES_MAX_CELLS; NULL changed with changed_cap > 0.
 * BT_ERR_UNSUPPORTED: an odd centre size; Rg16 or Rgb8.  entry_count == 0, width == 0 or height == 0 (with valid arguments otherwise;
 * the list is not looked at): BT_OK, nothing touched. */
#define BT_SHAPES_NONE 0xFFFFu
#define BT_SHAPES_NO_ENTRY 0xFFFFFFFFu
#define BT_SHAPES_MAX_SHAPES 4096u
#define BT_SHAPES_MAX_ENTRIES 65536u
#define BT_SHAPES_MAX_VERTICES (1u << 20)
#define BT_SHAPES_MAX_COORD (1 << 23)
#define BT_SHAPES_MAX_HALF_WIDTH (1u << 20)
#define BT_SHAPES_MAX_SIDE 8192u
#define BT_SHAPES_MAX_CELLS (1u << 22)
#define BT_SHAPES_CHUNK 256u
#define BT_SHAPES_BLOCK_W 64u
#define BT_SHAPES_BLOCK_H 16u
enum { BT_SHAPE_POLYGON = 0, BT_SHAPE_STROKE = 1 };                         /* bt_shape.kind */
enum { BT_SHAPE_NONZERO = 1, BT_SHAPE_CLOSED = 2, BT_SHAPE_MORE = 4 };      /* bt_shape.flags */
enum { BT_SHAPE_SET = 0, BT_SHAPE_MAX = 1, BT_SHAPE_MIN = 2, BT_SHAPE_ADD = 3, BT_SHAPE_SUB = 4 }; /* bt_shape.op */
enum { BT_SHAPES_DRY_RUN = 1 };                                             /* bt_atlas_rasterize_shapes flags */
typedef struct bt_shape_vertex {
    int32_t x, y;  /* 1/256 cell, relative to the window's origin; |x|, |y| <= BT_SHAPES_MAX_COORD */
} bt_shape_vertex; /* 8 bytes */
typedef struct bt_shape {
    uint32_t kind, flags;                 /* BT_SHAPE_POLYGON / _STROKE; BT_SHAPE_NONZERO | _MORE (polygon), BT_SHAPE_CLOSED (stroke) */
    uint32_t first_vertex, vertex_count;  /* of `vertices` */
    uint32_t half_width;                  /* a stroke's r in 1/256 cell; 0 on a polygon */
    uint32_t op, value;                   /* BT_SHAPE_SET .. _SUB and its operand */
    uint32_t _pad;                        /* 0 */
} bt_shape; /* 32 bytes */
typedef struct bt_shape_box {
    uint16_t x_lo, y_lo, x_hi, y_hi;  /* cells of the window, both ends included; empty: {1, 1, 0, 0} */
} bt_shape_box; /* 8 bytes */
typedef struct bt_shapes_stats {
    uint32_t cells, shapes;       /* width * height; shapes of the list */
    uint32_t shapes_culled;       /* shapes with an empty box */
    uint32_t tiles_missing;       /* tiles of U the attachment does not hold */
    uint64_t covered;             /* cells with count > 0 */
    uint64_t written;             /* texels whose value changed */
    bt_shape_box box;             /* U */
    uint32_t launches;            /* the kernel launches of the call before the edit's, the gather counted as one */
    uint32_t _padding;
    bt_edit_stats edit;           /* of the write-back; zero with BT_SHAPES_DRY_RUN */
} bt_shapes_stats; /* 80 bytes */
bt_status bt_shapes_check(const bt_shape_vertex* vertices, uint32_t vertex_count, const bt_shape* shapes, uint32_t entry_count, uint32_t width,
                          uint32_t height, bt_shape_box* boxes_out /* may be NULL */, uint32_t* shape_count_out /* may be NULL */,
                          uint32_t* bad_entry_out /* may be NULL */);
bt_status bt_atlas_rasterize_shapes(bt_atlas* atlas, uint32_t attachment_index, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0,
                                    uint32_t width, uint32_t height, uint32_t channel, const bt_shape_vertex* vertices, uint32_t vertex_count,
                                    const bt_shape* shapes, uint32_t entry_count, uint32_t flags, uint8_t* count_out /* may be NULL */,
                                    uint16_t* last_out /* may be NULL */, bt_tile_coordinate* changed, uint32_t changed_cap,
                                    bt_shapes_stats* stats /* may be NULL */);

/* ---------------- regions: the connected regions of a mask over a rectangle of a layer, their table, a bake by area
 * REGIONS (bt_atlas_label_regions; R16 and Rgba8).  Integers throughout: no float appears, so every plane and every record is a function
 * of the input byte for byte.
 * Window: DISTANCE's.  The width x height rectangle of centre texels at mosaic (x0, y0) of `lod` on `side` of attachment attachment_index
 * (the rectangle of bt_atlas_read_region; inside one face).  Cell (x, y) is mosaic texel (x0 + x, y0 + y); planes are row-major, cell
 * (x, y) at index i = y * width + x.  Texels of tiles the atlas does not hold read as 0; the tiles are counted in tiles_missing.
 * Bounds: width, height <= BT_REGIONS_MAX_SIDE; width * height <= BT_REGIONS_MAX_CELLS.
 * Rule: bt_regions_rule {channel, lo, hi, max_step, flags}.  v(c) = the raw u16 of an R16 texel (channel must be 0), byte `channel` (0..3)
 * of an Rgba8 one.
 *     from_texels(c) = (flags & BT_REGIONS_FROM_TEXELS) && lo <= v(c) && v(c) <= hi
 *     from_host(c)   = member_host && member_host[i] != 0                 (member_host: an optional plane of width * height bytes)
 *     member(c)      = (from_texels(c) || from_host(c)) XOR ((flags & BT_REGIONS_INVERT) != 0)
 * Two members a and b are linked when they are adjacent (they share an edge; with BT_REGIONS_EIGHT an edge or a corner) and
 * |v(a) - v(b)| <= max_step (0..65535, on both formats).  A region is a class of the transitive closure of "linked".  So: max_step 65535
 * gives the plain components of the mask; max_step 0 cuts a classification map into areas of one value; a small max_step on heights gives
 * the areas one can walk without a step higher than that.  v is the texel's whatever made the cell a member (a host plane included).
 * Planes (u32, width * height):
 *     label(c) = the smallest cell index of c's region                      BT_REGIONS_NONE where c is no member
 *     id(c)    = the rank of label(c) among all labels in ascending order   BT_REGIONS_NONE where c is no member
 * so ids are dense, 0 .. regions - 1, in the row-major order of the regions' first cells.
 * Table: regions_out[region_cap] of bt_region, the first min(regions, region_cap) records written in id order, the rest of the array
 * untouched.  Of region r: label; area, its cells; x_min .. y_max, its bounding box in cells of the window; v_min, v_max and v_sum, the
 * smallest, the largest and the sum of v over its cells; edges, the number of pairs (a cell c of r, one of the four edge neighbours n of c)
 * with n outside the window or label(n) != label(c): the perimeter in cell edges, whatever the connectivity.
 * bt_regions_stats: cells = width * height; members; regions; regions_written = min(regions, region_cap); largest_area, the area of the
 * largest region (0 without one) and largest_label, the smallest label among the regions of that area (BT_REGIONS_NONE without one);
 * tiles_missing; baked, the cells the bake wrote; launches.  Every field but launches is a function of the input; launches is a function
 * of the arguments alone, never of the texels.
 * Bake (optional): bt_regions_bake {attachment, channel, min_area, max_area, value, flags}.  For every member whose region's area lies in
 * [min_area, max_area], byte `channel` of the texel of the Rgba8 attachment `attachment` of the same atlas becomes `value` (0..255), over
 * the same rectangle; every other byte of the rectangle keeps its value.  No flag is defined: flags must be 0.  The write is an edit like
 * any other: the destination rectangle is gathered, the byte merged on the device, and the texels written and the invariant F restored
 * exactly as by bt_atlas_write_region of them over the rectangle: the same plan, the same `changed` order, the same bt_edit_stats
 * (stats->edit).  The destination may be the source attachment: a despeckle is one call (members byte == 255, max_area 15, value 0).
 * Without `bake` the call is a read: no layer is marked written, and `changed` is not written.
 * Outputs: label_out, id_out, regions_out, stats; each may be NULL (regions_out only with region_cap == 0).
 * The call: synchronous, host arrays in and out through the context's staging ring, ordered behind the work queued on the context's
 * stream.  A union-find over a parent plane P with P[c] <= c, links made only from a root to a smaller index, so the root of a region is
 * its smallest cell.  Launches: the gather of bt_atlas_read_region (counted as one); local: a workgroup to a block of BT_REGIONS_BLOCK x
 * BT_REGIONS_BLOCK cells resolves the block's own components in LDS; seams: a lane to each cell of a block's last column and last row
 * unites it with its linked neighbours in the blocks beside, below and diagonally below; flatten: in chunks of BT_REGIONS_CHUNK
 * consecutive cells, label = the root, the chunk's labels counted and ranked, the areas added; scan: the prefix sums of the chunks'
 * counts; emit: id, and the members folded into their regions' records by integer atomics, what shares a label reduced in the wave and
 * the workgroup first; finish: the largest region, the baked byte, the records: launches = 7.  With a bake the gather of the destination is one more,
 * launches = 8, and the launches of the edit follow in stats->edit.launches.  The count depends on the arguments only, not on how the
 * regions wind: that is the point of the form.  No result depends on a schedule.  The scratch stays in the context until bt_ctx_trim: 16
 * bytes per cell and the texel (2 or 4), 1 more with member_host, 80 per record of min(region_cap, cells), and with a bake the staged
 * rectangle (4 per cell).
 * Refusals, all before anything is queued, with the outputs untouched and *stats zeroed.  BT_ERR_INVALID_ARGUMENT: what
 * bt_atlas_read_region refuses of atlas, attachment, side, lod and rectangle; NULL rule; neither FROM_TEXELS nor member_host; unknown flag
 * bits; lo > hi with FROM_TEXELS; a channel above 3, or non-zero on R16; hi above 65535 on R16, above 255 on Rgba8; max_step above 65535;
 * a side above BT_REGIONS_MAX_SIDE; width * height above BT_REGIONS_MAX_CELLS; NULL regions_out with region_cap > 0; NULL changed with
 * changed_cap > 0; in a bake: an attachment out of range, a channel above 3, min_area > max_area, value above 255, flag bits.
 * BT_ERR_UNSUPPORTED: an odd centre size; a bake destination that is not Rgba8, or whose texture_size or border_size differs from the
 * source's.  width == 0 or height == 0 (with valid arguments otherwise; member_host is not looked at): BT_OK, nothing touched. */
#define BT_REGIONS_NONE 0xFFFFFFFFu
#define BT_REGIONS_MAX_SIDE 8192u
#define BT_REGIONS_MAX_CELLS (1u << 22)
#define BT_REGIONS_BLOCK 32u
#define BT_REGIONS_CHUNK 1024u
enum { BT_REGIONS_FROM_TEXELS = 1, BT_REGIONS_INVERT = 2, BT_REGIONS_EIGHT = 4 }; /* bt_regions_rule.flags */
typedef struct bt_regions_rule {
    uint32_t channel;   /* of an Rgba8 texel, 0..3; 0 on R16 */
    uint32_t lo, hi;    /* the band of texel values that are members, both ends included (FROM_TEXELS) */
    uint32_t max_step;  /* 0..65535: the largest |v(a) - v(b)| across a link */
    uint32_t flags;     /* BT_REGIONS_FROM_TEXELS | BT_REGIONS_INVERT | BT_REGIONS_EIGHT */
} bt_regions_rule; /* 20 bytes */
typedef struct bt_regions_bake {
    uint32_t attachment;          /* the Rgba8 attachment that takes the byte */
    uint32_t channel;             /* 0..3 */
    uint32_t min_area, max_area;  /* the areas whose regions are written, both ends included */
    uint32_t value;               /* 0..255 */
    uint32_t flags;               /* 0 */
} bt_regions_bake; /* 24 bytes */
typedef struct bt_region {
    uint32_t label;                        /* offset 0: the smallest cell index of the region */
    uint32_t area;                         /* 4: its cells */
    uint16_t x_min, y_min, x_max, y_max;   /* 8, 10, 12, 14: its bounding box in cells of the window */
    uint16_t v_min, v_max;                 /* 16, 18: the smallest and the largest v of its cells */
    uint32_t edges;                        /* 20: its perimeter in cell edges */
    uint64_t v_sum;                        /* 24: the sum of v over its cells */
} bt_region; /* 32 bytes */
typedef struct bt_regions_stats {
    uint32_t cells, members;        /* width * height; member cells */
    uint32_t regions;               /* regions of the window */
    uint32_t regions_written;       /* min(regions, region_cap) */
    uint32_t largest_area;          /* 0 without a region */
    uint32_t largest_label;         /* the smallest label among the regions of that area; BT_REGIONS_NONE without a region */
    uint32_t tiles_missing;         /* tiles of the rectangle the source attachment does not hold */
    uint32_t baked;                 /* cells the bake wrote */
    uint32_t launches;              /* the kernel launches of the call before the edit's, the gathers counted as one each */
    uint32_t _padding[3];
    bt_edit_stats edit;             /* of the bake's write-back; zero without a bake */
} bt_regions_stats; /* 80 bytes */
bt_status bt_atlas_label_regions(bt_atlas* atlas, uint32_t attachment_index, uint32_t side, uint32_t lod, uint32_t x0, uint32_t y0,
                                 uint32_t width, uint32_t height, const bt_regions_rule* rule,
                                 const uint8_t* member_host /* may be NULL */, uint32_t* label_out /* may be NULL */,
                                 uint32_t* id_out /* may be NULL */, bt_region* regions_out /* may be NULL with region_cap 0 */,
                                 uint32_t region_cap, const bt_regions_bake* bake /* may be NULL */, bt_tile_coordinate* changed,
                                 uint32_t changed_cap, bt_regions_stats* stats /* may be NULL */);

/* ---------------------------------------------------------------- PACKED TILES
 * A lossless tile codec that the device encodes and decodes itself: only packed bytes cross the file system and PCIe, and the atlas ends
 * up byte-identical to one loaded from `.bin`.  `.bin` stays the default everywhere; everything here is opt-in.
 *
 * One packed tile holds one layer of one attachment: T x T texels, R16 or Rgba8, self-contained.
 * PLANES.  R16: one plane of b = 16-bit values.  Rgba8: four planes of b = 8-bit values, plane c being byte c of the texel.
 * STRIPS.  The rows are cut into strips of S = BT_PACK_STRIP_ROWS rows (the last one shorter when T % S != 0), coded independently.
 * RESIDUAL.  r = v(x, y) - v(x-1, y) - v(x, y-1) + v(x-1, y-1) (mod 2^b); a term with x-1 < 0, or whose row lies above the strip's first
 * row, is 0.  Decoding is a 2-D inclusive prefix sum mod 2^b: along the row over the whole tile width, then down the columns of the strip.
 * ZIGZAG.  r read as signed s in [-2^(b-1), 2^(b-1)): z = 2s for s >= 0, z = -2s - 1 otherwise; b bits again.
 * GROUPS.  64 consecutive values of one row of one plane; gpr = ceil(T / 64) groups per row.  Lanes of the last group with x >= T have
 * z = 0 when encoding; their bits are ignored when decoding.  The group's width w is the bit length of the largest z among its real
 * lanes, 0 <= w <= b.  Its payload is w little-endian 64-bit words, bit i of word k being bit k of lane i's z (bit planes): 8 w bytes,
 * always 8-byte aligned.  w = 0 costs nothing; w = b is the raw escape.
 * ORDER.  Groups are ordered by (y, plane c, group g): index (y * planes + c) * gpr + g, for the widths and for the payload.
 * STREAM (= the file "{coord}.btp").  Bytes 0-3 'B' 'T' 'P' '1'; 4 the format (BT_FORMAT_R16 / BT_FORMAT_RGBA8); 5 the strip rows (32);
 * 6-7 T, u16 LE; 8-11 the payload bytes, u32 LE; 12-15 zero; then W = planes * T * gpr width bytes, one per group; zero bytes up to a
 * multiple of 8; then the 8 * sum(w) payload bytes.  There is no offset table: offsets are prefix sums of the widths.
 * CANONICAL AND ACCEPTED.  The encoder emits the minimal w, so a tile has exactly one encoding, byte-identical from run to run; the
 * decoder accepts any w <= b.
 * VALIDITY, all checked on the host before anything is launched (after that no device read can leave the stream): size >= 16; the magic;
 * the format one of the two; strip rows == 32; T >= 1; bytes 12-15 and the padding zero; every width <= b; the payload field == 8 sum(w);
 * the size == 16 + pad8(W) + payload.
 * BOUND.  bound(format, T) = 16 + pad8(W) + 8 b W: the raw size plus one byte per 64 values plus at most 23.
 *
 * bt_packed_tile_bound / bt_packed_tile_check need no device.  check: BT_ERR_IO with a text naming the first violated rule;
 * BT_ERR_UNSUPPORTED for a header whose format (Rg16 / Rgb8) or strip height this version does not read; format / texture_size (each may
 * be NULL) are filled once the header's fields are readable.
 *
 * bt_atlas_pack_tiles: the listed layers (any order, repeats allowed) -> streams, stream i at dst_host + offsets[i], offsets[count] the
 * total.  dst_host == NULL fills `offsets` only; a dst_bytes that is too small is BT_ERR_OVERFLOW with `offsets` still filled.  A read
 * (not a write for bt_run_stats.prev_zero_launches).  Three launches per chunk (measure, scan, emit), no atomics.
 * bt_atlas_unpack_tiles: the inverse, stream i (offsets[i] .. offsets[i+1]) into layers[i], followed by the mip levels of those layers;
 * the layers count as written exactly as after bt_atlas_load_tiles.  A repeated layer, a layer out of range, a stream whose format or T
 * is not the attachment's: BT_ERR_INVALID_ARGUMENT; an invalid stream: what bt_packed_tile_check says; in each case no layer is touched.
 * bt_atlas_save_tiles_packed / bt_atlas_load_tiles_packed: bt_atlas_save_tiles / bt_atlas_load_tiles for "{directory}/{coord}.btp";
 * coords == NULL: every existing tile.  A missing or invalid file is BT_ERR_IO.
 * bt_atlas_set_tile_files: what bt_atlas_update reads, "{coord}.bin" (BT_TILE_FILES_BIN, the default) or "{coord}.btp"
 * (BT_TILE_FILES_PACKED, decoded on the device batch by batch); a missing or invalid file leaves the tile Loading and counts as failed.
 * All of them work in chunks of at most 64 tiles or 32 MiB of raw texels through the context's staging ring; the scratch stays in the
 * context until bt_ctx_trim.  NULL handles or required pointers: BT_ERR_INVALID_ARGUMENT.  Attachments that are not R16 / Rgba8, a
 * texture_size above 65535 or a tile whose bound does not fit the payload field: BT_ERR_UNSUPPORTED.  count == 0: BT_OK (offsets[0] = 0). */
#define BT_PACK_STRIP_ROWS 32u
#define BT_TILE_FILES_BIN 0u
#define BT_TILE_FILES_PACKED 1u
bt_status bt_packed_tile_bound(uint32_t format, uint32_t texture_size, uint64_t* bytes);
bt_status bt_packed_tile_check(const void* bytes, uint64_t size, uint32_t* format /* may be NULL */, uint32_t* texture_size /* may be NULL */);
bt_status bt_atlas_pack_tiles(bt_atlas* atlas, uint32_t attachment_index, const uint32_t* layers, uint32_t count, void* dst_host /* may be NULL */,
                              uint64_t dst_bytes, uint64_t* offsets /* count + 1 */);
bt_status bt_atlas_unpack_tiles(bt_atlas* atlas, uint32_t attachment_index, const uint32_t* layers, uint32_t count, const void* src_host,
                                const uint64_t* offsets /* count + 1 */);
bt_status bt_atlas_save_tiles_packed(bt_atlas* atlas, uint32_t attachment_index, const char* directory, const bt_tile_coordinate* coords /* may be NULL */,
                                     uint32_t count);
bt_status bt_atlas_load_tiles_packed(bt_atlas* atlas, uint32_t attachment_index, const char* directory, const bt_tile_coordinate* coords /* may be NULL */,
                                     uint32_t count);
bt_status bt_atlas_set_tile_files(bt_atlas* atlas, uint32_t tile_files);

/* ---------------------------------------------------------------- diagnostics */
/* Exhaustive device check that the kernels' 3-operation unorm16 -> f32 conversion equals the correctly
 * rounded division t / 65535.0f for all 65536 texel values; *failures must come back 0. */
bt_status bt_selftest(bt_ctx* ctx, uint32_t* failures);

/* ---------------------------------------------------------------- synthetic inputs */
/* Deterministic integer fBm heightmap in [1, 65535] written straight into HBM (bench / tests: the
 * reference's Gaia and GEBCO source rasters are not in its checkout).  The window
 * (x0, y0, width, height) of the infinite field is produced, so shards can generate only their part. */
bt_status bt_synth_fbm_r16(bt_ctx* ctx, void* dst_device, uint32_t width, uint32_t height, uint64_t row_pitch,
                           uint32_t x0, uint32_t y0, uint32_t base_cell, uint32_t octaves, uint32_t seed);

#ifdef __cplusplus
}
#endif
#endif /* BEVY_TERRAIN_AMD_H */
