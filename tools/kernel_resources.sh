#!/bin/bash
# Register / scratch / LDS use of every kernel of a source file (default bt_fused.hip, the translation unit of every fused kernel: bt_fused_common.hpp
# and bt_fused_tail.hpp are its text and cannot be compiled on their own) as compiled for gfx950 (the metadata the assembler emits):
#   tools/kernel_resources.sh [pattern] [source.hip]          e.g. tools/kernel_resources.sh raycast bt_raycast.hip
#                                                               tools/kernel_resources.sh normal bt_normal.hip   (tile_tree_normal_kernel, tile_normals_kernel)
#                                                               tools/kernel_resources.sh edit bt_edit.hip   (edit_brush / edit_paint / edit_region / edit_gather / edit_smooth / edit_downsample)
#                                                               tools/kernel_resources.sh splat bt_splat.hip   (edit_splat_kernel)
#                                                               tools/kernel_resources.sh scatter bt_scatter.hip   (scatter_decide_kernel, scatter_scan_kernel, scatter_emit_kernel)
#                                                               tools/kernel_resources.sh collide bt_collide.hip   (collide_kernel; `sweep` for sweep_kernel)
#                                                               tools/kernel_resources.sh path bt_path.hip   (path_prepare_kernel, path_next_kernel; `relax` for relax_kernel<PathRule> of bt_relax.hpp)
#                                                               tools/kernel_resources.sh erode bt_erode.hip   (erode_init_kernel, erode_step_kernel, erode_finish_kernel)
#                                                               tools/kernel_resources.sh drain bt_drain.hip   (drain_prepare_kernel, drain_flat_seed_kernel, drain_direction_kernel, drain_finish_kernel; `relax` for relax_kernel<FillRule / FlatRule / AccumulateRule>)
#                                                               tools/kernel_resources.sh viewshed bt_viewshed.hip   (viewshed_transpose_kernel, viewshed_walk_kernel<true / false>, viewshed_finish_kernel)
#                                                               tools/kernel_resources.sh distance bt_distance.hip   (distance_summary_kernel, distance_carry_kernel, distance_fill_kernel, distance_rows_kernel, distance_finish_kernel)
#                                                               tools/kernel_resources.sh skyline bt_skyline.hip   (skyline_walk_kernel, skyline_finish_kernel; the transpose is the viewshed's)
#                                                               tools/kernel_resources.sh pack bt_pack.hip   (pack_measure_kernel, pack_emit_kernel, pack_decode_kernel, each <false / true> = R16 / Rgba8; pack_scan_kernel)
#                                                               tools/kernel_resources.sh shapes bt_shapes.hip   (shapes_raster_kernel)
#                                                               tools/kernel_resources.sh regions bt_regions.hip   (regions_local_kernel, regions_seam_kernel, regions_flatten_kernel, regions_scan_kernel, regions_emit_kernel, regions_finish_kernel)
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R/bevy_terrain_amd/csrc
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math --offload-arch=gfx950 -I../../include -I. -S --cuda-device-only -o /tmp/bt_fused_gfx950.s "${2:-bt_fused.hip}" 2>/dev/null
python3 - "$1" <<'PY'
import re, sys
text = open("/tmp/bt_fused_gfx950.s").read()
pat = sys.argv[1] if len(sys.argv) > 1 else ""
for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S):
    name, body = m.group(1), m.group(2)
    if pat and pat not in name:
        continue
    def g(k):
        r = re.search(r"\." + k + r"\s+(\S+)", body)
        return r.group(1) if r else "?"
    print(name[:110])
    print("   vgpr", g("amdhsa_next_free_vgpr"), "sgpr", g("amdhsa_next_free_sgpr"), "scratch", g("amdhsa_private_segment_fixed_size"), "lds", g("amdhsa_group_segment_fixed_size"))
for m in re.finditer(r"; (ScratchSize|codeLenInByte|NumVgprs|Occupancy|VGPR spill|SGPR spill|sgpr_spill_count|vgpr_spill_count)[^\n]*", text):
    pass
# the per-function remarks
for m in re.finditer(r"^(_Z\S+|\S+):.*?; NumVgprs: (\d+).*?; ScratchSize: (\d+).*?; Occupancy: (\d+)", text, flags=re.S | re.M):
    pass
PY
grep -E "^; (Kernel|NumVgprs|ScratchSize|Occupancy|SGPRBlocks)|vgpr_spill_count|sgpr_spill_count|\.name:" /tmp/bt_fused_gfx950.s | grep -A3 "${1:-fused_main}" | head -60
