// The tile tree on the host: the handle's state and what its entry points share.  bt_tile_tree.hip holds the tree itself (its kernels,
// create / update / adjust / read, the per-frame chain), bt_tile_tree_query.cpp the queries that read the terrain through it (ray casting,
// rendering, normals, geometry).
#pragma once

#include "bt_internal.hpp"
#include "bt_model.hpp"
#include "bt_tile_tree_device.hpp"

namespace bt {

struct NodeState {  // TileState of the tree (tile_tree.rs:28-43)
    bt_tile_coordinate coordinate;
    uint32_t requested;  // RequestState::Requested
};

// One device copy of TileAtlasState::tile_states: open addressing, linear probing; key = coordinate
struct StateSlot {
    bt_tile_coordinate coordinate;  // side == kInvalid: empty
    uint32_t atlas_index;
    uint32_t loaded;
};

}  // namespace bt

struct bt_tile_tree {
    bt_ctx* ctx = nullptr;
    bt_terrain_model model_c{};
    bt_terrain_view_config view_config{};
    bt::model::Model model{};
    uint32_t lod_count = 0, sides = 0, nodes = 0;
    // TileTree::new (tile_tree.rs:135-173)
    double morph_distance = 0, blend_distance = 0, load_distance = 0, subdivision_distance = 0, precision_threshold_distance = 0;
    double view_world_position[3] = {0, 0, 0};
    float approximate_height = 0;
    // device tables
    bt::NodeState* d_nodes = nullptr;
    bt_tile_tree_entry* d_entries = nullptr;
    uint32_t* d_origins = nullptr;
    float* d_height = nullptr;  // [0] approximate_height (what the kernels read), [4..8) the vec4 sample behind it
    bt::StateSlot* d_table = nullptr;
    uint32_t table_capacity = 0;
    uint64_t table_version = 0;
    const bt_atlas* table_atlas = nullptr;
    // the last update's lists: pinned host memory the update kernel writes directly (one synchronisation, no copies)
    bt_tile_coordinate *h_released = nullptr, *h_requested = nullptr;
    uint32_t* h_counts = nullptr;
    uint32_t released_count = 0, requested_count = 0;
    // bt_frame_update: pinned staging of the view position, of the height read back one frame late, and of the atlas's tile states
    double* h_view_position = nullptr;
    float* h_height = nullptr;
    bool height_in_flight = false;  // an asynchronous copy d_height -> h_height was enqueued after the last synchronisation
    bt::StateSlot* h_table = nullptr;
    uint32_t h_table_capacity = 0;
    bool table_copy_pending = false;  // h_table -> d_table enqueued since the last synchronisation
};

namespace bt {

TreeParams make_params(const bt_tile_tree* t);  // what the kernels read of the tree, the host's copy of the height included
TerrainRef make_ground(const bt_tile_tree* t, const Attachment& at);  // what a query's launcher takes: the tree and one attachment's level 0
// after every synchronisation of the context's stream on the tree's behalf: the height a frame left in pinned memory becomes the host's
// copy, and the staging table may be rewritten
void synchronised(bt_tile_tree* t);
// what every query of the tree refuses first: a NULL tree or atlas, two contexts (BT_ERR_INVALID_ARGUMENT); then the height attachment
// (height_attachment, bt_internal.hpp).  query_handles is the first half alone, for a call with checks of its own between the two
bt_status query_handles(const char* who, const bt_tile_tree* t, const bt_atlas* a);
bt_status query_check(const char* who, const bt_tile_tree* t, const bt_atlas* a, uint32_t ai, const Attachment** height);

}  // namespace bt
