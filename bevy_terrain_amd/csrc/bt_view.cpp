// The view on the host, device-free f64 math: the default view configuration, the view state and the model approximation a frame's
// kernels read, the horizon of a spherical model, the frustum planes of a view-projection matrix, and the check of a caller's terrain
// model that every entry point taking one makes first.
#include <algorithm>
#include <cmath>

#include "bt_internal.hpp"
#include "bt_model.hpp"

using namespace bt;
using namespace bt::model;

bt_status bt::check_model(const bt_terrain_model* m, const char* who) {
    if (!m || m->kind > BT_MODEL_ELLIPSOIDAL || !(m->a > 0.0) || (m->kind == BT_MODEL_ELLIPSOIDAL && !(m->b > 0.0))) {
        set_error("%s: %s", who, m ? "terrain model: kind / axes" : "NULL model");
        return BT_ERR_INVALID_ARGUMENT;
    }
    return BT_OK;
}

extern "C" {

void bt_terrain_view_config_default(bt_terrain_view_config* out) {
    if (!out) return;
    *out = {8, 1000000, 30, 16, 0.1, 0.001, 2.5, 16.0, 2.0, 0.2f, 0.2f, 10, 0};  // terrain_view.rs:47-63
}

bt_status bt_view_state_from_config(const bt_terrain_model* model, const bt_terrain_view_config* vc, const double view_world_position[3],
                                    float approximate_height, bt_view_state* out) {
    if (!vc || !view_world_position || !out) return BT_ERR_INVALID_ARGUMENT;
    if (bt_status s = check_model(model, "bt_view_state_from_config")) return s;
    const Model m = make_model(*model);
    bt_view_state v{};
    v.spherical = is_spherical(m) ? 1u : 0u;
    v.geometry_tile_count = vc->geometry_tile_count;
    v.refinement_count = vc->refinement_count;
    v.vertices_per_tile = 2u * vc->grid_size * (vc->grid_size + 2u);  // terrain_view_bind_group.rs:106
    // tile_tree.rs:148-150 (f64), `as f32` at terrain_view_bind_group.rs:111
    v.subdivision_distance = float(vc->morph_distance * model_scale(m) * (1.0 + vc->subdivision_tolerance));
    v.origin_lod = vc->origin_lod;
    v.approximate_height = approximate_height;
    // TerrainModelApproximation::compute (terrain_model.rs:262-290): origin_xy / origin_uv per side
    const V3 view = {view_world_position[0], view_world_position[1], view_world_position[2]};
    const Coordinate c = coordinate_from_world_position(view, m);
    const double origin_count = double(1u << vc->origin_lod);
    for (uint32_t side = 0; side < 6; side++) {
        // (the planar model fills all six entries with the same coordinate: project_to_side returns self)
        const Coordinate p = coordinate_project_to_side(c, side, m);
        const double sx = p.uv.x * origin_count, sy = p.uv.y * origin_count;
        v.sides[side].view_xy[0] = saturating_i32(sx);  // as_ivec2
        v.sides[side].view_xy[1] = saturating_i32(sy);
        v.sides[side].view_uv[0] = float(sx - trunc(sx));  // DVec2::fract() = self - self.trunc() (glam 0.27), as_vec2
        v.sides[side].view_uv[1] = float(sy - trunc(sy));
    }
    for (int i = 0; i < 3; i++) v.world_position[i] = float(view_world_position[i]);  // culling_bind_group.rs:50
    // mesh uniform of TerrainModel::transform() (terrain_model.rs:195-201): scale / translation `as_vec3`, identity
    // rotation; local_from_world_transpose = transpose(inverse(mat3)) = diag(1 / scale) in f32
    const float sc[3] = {float(m.scale.x), float(m.scale.y), float(m.scale.z)};
    const float tr[3] = {float(m.position.x), float(m.position.y), float(m.position.z)};
    for (int col = 0; col < 3; col++) v.world_from_local[3 * col + col] = sc[col];
    for (int i = 0; i < 3; i++) v.world_from_local[9 + i] = tr[i];
    for (int col = 0; col < 3; col++) v.local_from_world_transpose[3 * col + col] = 1.0f / sc[col];
    *out = v;
    return BT_OK;
}

// TerrainModelApproximation::compute (terrain_model.rs:263-360) in f64, `as f32` at the end: the definition is the header's (HIGH PRECISION)
bt_status bt_model_approximation_from_config(const bt_terrain_model* model, const bt_terrain_view_config* vc, const double view_world_position[3],
                                             bt_model_approximation* out) {
    if (!model || !vc || !view_world_position || !out) {
        set_error("bt_model_approximation_from_config: NULL %s", !model ? "model" : (!vc ? "view_config" : (!out ? "out" : "view_world_position")));
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bt_status s = check_model(model, "bt_model_approximation_from_config")) return s;
    if (model->kind == BT_MODEL_PLANAR) {
        set_error("bt_model_approximation_from_config: a planar model has no series (the reference's coefficients are the cube sphere's there)");
        return BT_ERR_UNSUPPORTED;
    }
    if (!std::isfinite(view_world_position[0]) || !std::isfinite(view_world_position[1]) || !std::isfinite(view_world_position[2]) || vc->origin_lod > 31u) {
        set_error("bt_model_approximation_from_config: a non-finite position, or origin_lod %u (<= 31)", vc->origin_lod);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const Model m = make_model(*model);
    const V3 view = {view_world_position[0], view_world_position[1], view_world_position[2]};
    const Coordinate c = coordinate_from_world_position(view, m);
    bt_model_approximation a{};
    for (uint32_t side = 0; side < 6; side++) {
        const SideSeries q = side_series(side, coordinate_project_to_side(c, side, m).uv, m);
        bt_side_coefficients& k = a.sides[side];
        const V3 rel = {q.p.x - view.x, q.p.y - view.y, q.p.z - view.z};
        const V3 half_ss = div3(q.p_ss, 2.0), half_tt = div3(q.p_tt, 2.0);
        const V3* src[6] = {&rel, &q.p_s, &q.p_t, &half_ss, &q.p_st, &half_tt};
        float* dst[6] = {k.c, k.c_s, k.c_t, k.c_ss, k.c_st, k.c_tt};
        for (int i = 0; i < 6; i++) {
            dst[i][0] = float(src[i]->x);
            dst[i][1] = float(src[i]->y);
            dst[i][2] = float(src[i]->z);
        }
    }
    a.precision_threshold_distance = float(vc->precision_threshold_distance * model_scale(m));  // tile_tree.rs:153, terrain_view_bind_group.rs:111
    a.origin_lod = vc->origin_lod;
    *out = a;
    return BT_OK;
}

// f64 -> f32 with a directed rounding (the nearest value, stepped back when it lies on the wrong side)
static float f32_toward_zero(double d) {
    const float f = float(d);
    return fabs(double(f)) > fabs(d) ? nextafterf(f, 0.0f) : f;
}
static float f32_up(double d) {
    const float f = float(d);
    return double(f) < d ? nextafterf(f, INFINITY) : f;
}

bt_status bt_cull_horizon(const bt_terrain_model* model, const double view_world_position[3], float margin_world, bt_horizon_view* out) {
    if (!view_world_position || !out) {
        set_error("bt_cull_horizon: NULL %s", !out ? "out" : "view_world_position");
        return BT_ERR_INVALID_ARGUMENT;
    }
    if (bt_status s = check_model(model, "bt_cull_horizon")) return s;
    if (model->kind == BT_MODEL_PLANAR) {
        set_error("bt_cull_horizon: a planar model has no horizon");
        return BT_ERR_UNSUPPORTED;
    }
    if (!std::isfinite(view_world_position[0]) || !std::isfinite(view_world_position[1]) || !std::isfinite(view_world_position[2]) ||
        !(margin_world >= 0.0f) || !std::isfinite(margin_world)) {
        set_error("bt_cull_horizon: a non-finite position, or margin %g (finite, >= 0)", double(margin_world));
        return BT_ERR_INVALID_ARGUMENT;
    }
    const Model m = make_model(*model);
    const double shortest = std::min(m.scale.x, std::min(m.scale.y, m.scale.z));
    const V3 local = inverse_transform_point(m, {view_world_position[0], view_world_position[1], view_world_position[2]});
    bt_horizon_view h;
    h.eye[0] = float(local.x);
    h.eye[1] = float(local.y);
    h.eye[2] = float(local.z);
    h.occluder_radius = f32_toward_zero(1.0 + std::min(double(m.min_height), 0.0) / shortest);
    if (!(h.occluder_radius > 0.0f)) {
        set_error("bt_cull_horizon: min_height %g reaches the centre of a model whose shortest axis is %g", double(m.min_height), shortest);
        return BT_ERR_INVALID_ARGUMENT;
    }
    const V3 e = {double(h.eye[0]), double(h.eye[1]), double(h.eye[2])};
    h.vh = float(dot3(e, e) - double(h.occluder_radius) * double(h.occluder_radius));
    h.margin = f32_up(double(margin_world) / shortest);
    *out = h;
    return BT_OK;
}

// culling_bind_group.rs:25-38: row(i) of a column-major matrix is (m[i], m[4 + i], m[8 + i], m[12 + i])
void bt_cull_planes(const float m[16], float planes[5][4]) {
    if (!m || !planes) return;
    for (int i = 0; i < 5; i++)
        for (int k = 0; k < 4; k++) {
            const float row3 = m[4 * k + 3], row = m[4 * k + i / 2];
            planes[i][k] = ((i & 1) == 0 && i != 4) ? row3 + row : row3 - row;
        }
}

}  // extern "C"
