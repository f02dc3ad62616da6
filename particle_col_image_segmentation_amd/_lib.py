"""ctypes binding of libpcseg.so (include/pcseg.h).

There is no CPU fallback: if the HIP library is missing or no GPU is visible
every compute call raises -- loudly, by design.
"""
import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpcseg.so")
_lib = None


class PcsegError(RuntimeError):
    pass


_P = c_void_p
_I = c_int
# name -> (restype, argtypes); mirrors include/pcseg.h one to one
SIGNATURES = {
    "pcseg_version": (c_int, []),
    "pcseg_last_error": (c_char_p, []),
    "pcseg_device_count": (c_int, []),
    "pcseg_timing_enable": (None, [c_int]),
    "pcseg_timing_report": (c_int, [c_char_p, c_size_t]),
    "pcseg_argmax_planes_f32": (c_int, [_P, _P, _I, _I, _I, _I, _P]),
    "pcseg_median5_u8": (c_int, [_P, _P, _I, _I, _I, _P]),
    "pcseg_classmap_label_workspace_bytes": (c_size_t, [_I, _I, _I]),
    "pcseg_classmap_label_f32": (c_int, [_P, _I, _P, _P, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_ccl_workspace_bytes": (c_size_t, [_I, _I, _I]),
    "pcseg_ccl8_equal_u8": (c_int, [_P, _P, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_ccl8_bool": (c_int, [_P, _P, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_ccl4_bool": (c_int, [_P, _P, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_compact_labels": (c_int, [_P, _P, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_region_reduce": (c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "pcseg_region_reduce_n": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "pcseg_region_reduce_sel": (c_int, [_P, _P, _P, ctypes.c_uint64, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "pcseg_region_init": (c_int, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "pcseg_region_sums2": (c_int, [_P, _P, ctypes.c_uint64, _I, _P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "pcseg_threshold_lt_f32": (c_int, [_P, c_float, _P, _I, _I, _I, _P]),
    "pcseg_edt_workspace_bytes": (c_size_t, [_I, _I, _I]),
    "pcseg_edt_sq_u8": (c_int, [_P, _P, _I, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_edt_sq_lt_f32": (c_int, [_P, c_int64, c_float, _P, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_dilate_disk_u8": (c_int, [_P, c_uint64, _I, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_fill_particle": (c_int, [_P, _P, _I, _I, _I, _I, _I, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_fill_holes_workspace_bytes": (c_size_t, [_I, _I, _I]),
    "pcseg_fill_holes": (c_int, [_P, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_local_maxima_workspace_bytes": (c_size_t, [_I, _I, _I]),
    "pcseg_local_maxima_i32": (c_int, [_P, _P, _P, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_watershed_workspace_bytes": (c_size_t, [_I, _I, _I]),
    "pcseg_watershed_counters": (None, [_P, _I]),
    "pcseg_watershed4_f32": (c_int, [_P, c_int64, _P, _P, _P, _P, _I, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_merge_groups_workspace_bytes": (c_size_t, [_I, _I]),
    "pcseg_merge_groups": (c_int, [_P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_dilate_ccl_workspace_bytes": (c_size_t, [_I, _I, _I]),
    "pcseg_dilate_ccl_roots_u8": (c_int, [_P, c_uint64, _I, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_dilate_ccl_runs_workspace_bytes": (c_size_t, [_I, _I, _I]),
    "pcseg_dilate_ccl_runs_u8": (c_int, [_P, c_uint64, _I, _P, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_merge_groups_runs": (c_int, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_dilate_ccl_runs_multi_u8": (c_int, [_P, _P, _I, _I, _P, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_merge_groups_fused_multi": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _I, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_merge_groups_fused": (c_int, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _I, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_group_reduce": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "pcseg_classify_regions": (c_int, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "pcseg_nearest_dist_f64": (c_int, [_P, _I, _P, _I, _P, _P]),
    "pcseg_overlap_workspace_bytes": (c_size_t, [_I, _I, _I]),
    "pcseg_remove_overlapping": (c_int, [_P, _P, c_double, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_table_workspace_bytes": (c_size_t, [_I, _I]),
    "pcseg_table_layout": (c_int, [_P, _P, _P, c_size_t, _P]),
    "pcseg_table_write": (c_int, [_P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "pcseg_cell_distances": (c_int, [_P, c_int64, _I, _P, c_double, c_double, _P, _I, _P, c_size_t, _P]),
    "pcseg_neighbours_workspace_bytes": (c_size_t, [c_int64, _I, _I, _I]),
    "pcseg_point_neighbours": (c_int, [_P, _P, _P, _P, c_int64, _I, _I, c_double, _P, _I, _P, _P, _P, _P, c_size_t, _P]),
    "pcseg_neighbours_pack_cells": (c_int, [_P, _I, _P, _I, _P, c_size_t, _P, _P, _P, _P, _P]),
    "pcseg_mixing_workspace_bytes": (c_size_t, [c_int64, _I, _I, _I, _I, _I]),
    "pcseg_pair_label_mixing": (c_int, [_P, _P, _P, _P, c_int64, _I, _I, c_double, _P, _I, _I, c_uint64, _P, _P, _P, c_size_t, _P]),
    "pcseg_mixing_tile": (c_int, []),
    "pcseg_label_parent_workspace_bytes": (c_size_t, [_I, _I, _I, _I]),
    "pcseg_label_parent": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_refined_workspace_bytes": (c_size_t, [_I, _I]),
    "pcseg_refined_layout": (c_int, [_P, _P, _P, c_size_t, _P]),
    "pcseg_refined_table_write": (c_int, [_P, _P, c_size_t, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "pcseg_surface_workspace_bytes": (c_size_t, [_I, _I, _I]),
    "pcseg_surface_points": (c_int, [_P, c_uint64, _P, _P, _P, _P, _P, c_int64, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_surface_distances": (c_int, [_P, _P, _P, c_int64, _P, _P, _P, _I, _I, _I, c_double, _P, _I, _I, _P, _P, _P, _P, _P, _P,
                                        c_size_t, _P]),
    "pcseg_surface_thresholds": (c_int, [_P, _I, c_double, _P]),
    "pcseg_surface_shells_workspace_bytes": (c_size_t, [_I, _I, _I]),
    "pcseg_surface_shells": (c_int, [_P, _P, _P, _I, _I, _I, c_double, _P, _I, _P, _P, c_size_t, _P]),
    "pcseg_surface_pack_cells": (c_int, [_P, _I, _P, _I, _P, c_size_t, _P, _P, _P, _P, _P]),
    "pcseg_surface_pack_refined": (c_int, [_P, _I, _P, _P, c_int64, _I, _P, _P]),
    "pcseg_region_shape_workspace_bytes": (c_size_t, [_I, _I, _I]),
    "pcseg_region_shape": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_shape_properties": (c_int, [_P, _P, _P, _P, _I, _I, _P]),
    "pcseg_region_hull_workspace_bytes": (c_size_t, [_I, _I, _I, _I]),
    "pcseg_region_hull": (c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_hull_properties": (c_int, [_P, _P, _P, _P, _I, _I, _P]),
    "pcseg_nearest_label_workspace_bytes": (c_size_t, [_I, _I, _I]),
    "pcseg_nearest_label_i32": (c_int, [_P, _P, _I, _P, _P, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_territory_labels": (c_int, [_P, _P, c_int64, _P, c_int64, _P]),
    "pcseg_territory_reduce": (c_int, [_P, _P, _P, c_int64, _I, _P, _I, _I, _I, _P]),
    "pcseg_territory_pairs_workspace_bytes": (c_size_t, [_I, _I]),
    "pcseg_territory_pairs": (c_int, [_P, _P, c_int64, _I, _P, _P, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_territory_pairs_write": (c_int, [_I, _P, _P, _I, _I, _P, _P, _P, _P, _I, _P, c_size_t, _P]),
    "pcseg_contingency_workspace_bytes": (c_size_t, [_I, _I]),
    "pcseg_label_contingency": (c_int, [_P, _P, _I, _I, _I, _P, _P, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_contingency_write": (c_int, [_I, _P, _P, _P, _P, _I, _P, c_size_t, _P]),
    "pcseg_agreement_match": (c_int, [_P, _P, _P, c_int64, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "pcseg_border_block": (c_int, [_P]),
    "pcseg_label_borders_workspace_bytes": (c_size_t, [_I, _I, _I]),
    "pcseg_label_borders": (c_int, [_P, _P, c_int64, _I, _I, _I, _P, _P, _P, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_label_borders_write": (c_int, [_I, _I, _P, _P, _P, _P, _P, _P, _I, _P, c_size_t, _P]),
    "pcseg_border_merge": (c_int, [_I, _I, _P, c_double, _I, _P, _P, _P, _I, _P, c_size_t, _P]),
    "pcseg_relabel_map": (c_int, [_P, _P, _I, _P, _I, _I, _I, _P]),
    "pcseg_thin_labels_workspace_bytes": (c_size_t, [_I, _I, _I]),
    "pcseg_thin_labels": (c_int, [_P, _P, _P, _I, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_region_skeleton_workspace_bytes": (c_size_t, [_I, _I, _I, _I]),
    "pcseg_region_skeleton": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_skeleton_properties": (c_int, [_P, _P, _P, _P, _I, _I, _P]),
    "pcseg_reconstruct_workspace_bytes": (c_size_t, [_I, _I, _I]),
    "pcseg_reconstruct_i32": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_reconstruct_f64": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, c_size_t, _P]),
    "pcseg_hmax_range_i32": (c_int, [_P, _P, _I, _I, _I, _P]),
    "pcseg_hmax_range_f64": (c_int, [_P, _P, _I, _I, _I, _P]),
    "pcseg_hmax_shift_i32": (c_int, [_P, c_int64, _I, _P, _I, _I, _I, _P]),
    "pcseg_hmax_shift_f64": (c_int, [_P, c_double, _I, _P, _I, _I, _I, _P]),
    "pcseg_hmax_shift_edt": (c_int, [_P, c_double, _P, _P, _I, _I, _I, _P]),
    "pcseg_hmax_mark_i32": (c_int, [_P, _P, c_int64, _I, _P, _P, _I, _I, _I, _P]),
    "pcseg_hmax_mark_f64": (c_int, [_P, _P, c_double, _I, _P, _I, _P, _I, _I, _I, _P]),
    "pcseg_otsu_hist_f32":(c_int, [_P, _P, _P, _I, _I, _I, _P]),
    "pcseg_otsu_f32": (c_int, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "pcseg_morph3x3": (c_int, [_P, _P, _I, _I, _I, _I, _P]),
}

# entry point -> the size query (pcseg_<value>_workspace_bytes) that sizes the (workspace, workspace_bytes) it is given; a
# _multi entry takes its single form's query with B * M frames
WORKSPACE = {
    "pcseg_classmap_label_f32": "classmap_label",
    "pcseg_ccl8_equal_u8": "ccl", "pcseg_ccl8_bool": "ccl", "pcseg_ccl4_bool": "ccl", "pcseg_compact_labels": "ccl",
    "pcseg_edt_sq_u8": "edt", "pcseg_edt_sq_lt_f32": "edt", "pcseg_dilate_disk_u8": "edt", "pcseg_fill_particle": "edt",
    "pcseg_fill_holes": "fill_holes",
    "pcseg_local_maxima_i32": "local_maxima",
    "pcseg_watershed4_f32": "watershed",
    "pcseg_dilate_ccl_roots_u8": "dilate_ccl",
    "pcseg_dilate_ccl_runs_u8": "dilate_ccl_runs", "pcseg_dilate_ccl_runs_multi_u8": "dilate_ccl_runs",
    "pcseg_merge_groups": "merge_groups", "pcseg_merge_groups_runs": "merge_groups", "pcseg_merge_groups_fused": "merge_groups",
    "pcseg_merge_groups_fused_multi": "merge_groups",
    "pcseg_remove_overlapping": "overlap",
    "pcseg_table_layout": "table", "pcseg_table_write": "table",
    "pcseg_refined_layout": "refined", "pcseg_refined_table_write": "refined",
    "pcseg_point_neighbours": "neighbours",
    "pcseg_pair_label_mixing": "mixing",
    "pcseg_label_parent": "label_parent",
    "pcseg_surface_points": "surface", "pcseg_surface_distances": "surface",
    "pcseg_surface_shells": "surface_shells",
    "pcseg_region_shape": "region_shape",
    "pcseg_region_hull": "region_hull",
    "pcseg_nearest_label_i32": "nearest_label",
    "pcseg_territory_pairs": "territory_pairs", "pcseg_territory_pairs_write": "territory_pairs",
    "pcseg_label_contingency": "contingency", "pcseg_contingency_write": "contingency",
    "pcseg_label_borders": "label_borders", "pcseg_label_borders_write": "label_borders", "pcseg_border_merge": "label_borders",
    "pcseg_thin_labels": "thin_labels",
    "pcseg_region_skeleton": "region_skeleton",
    "pcseg_reconstruct_i32": "reconstruct", "pcseg_reconstruct_f64": "reconstruct",
}
# ... and the (workspace, workspace_bytes) pairs that no query sizes: they read the head of the table workspace that
# pcseg_table_layout wrote (of pcseg_refined_table_write: its first pair; its second is its own, above)
WORKSPACE_HANDED_ON = ("pcseg_cell_distances", "pcseg_neighbours_pack_cells", "pcseg_surface_pack_cells", "pcseg_refined_table_write")


class TableInputs(ctypes.Structure):
    """struct pcseg_table_inputs of include/pcseg.h, field for field."""
    _fields_ = [("B", ctypes.c_int32), ("cap", ctypes.c_int32), ("C", ctypes.c_int32), ("n_ratios", ctypes.c_int32),
                ("frame_ids", _P),
                ("counts", _P), ("stats", _P), ("cls_out", _P), ("cc_sums", _P),
                ("kind", _P), ("slot_of", _P), ("cells", _P),
                ("particle_area", _P), ("overlap_area", _P), ("type_stats", _P), ("tie_flags", _P),
                ("region_list", _P), ("n_list", _P),
                ("group_of", _P * 5), ("n_groups", _P * 5), ("group_stats", _P * 5),
                ("n_markers", _P), ("ws_stats", _P), ("ws_sums", _P),
                ("ratio_num", ctypes.c_int32 * 8), ("ratio_den", (ctypes.c_int32 * 4) * 8),
                ("overflow", _P), ("ws_overflow", _P), ("nan_flag", _P)]


class RefinedInputs(ctypes.Structure):
    """struct pcseg_refined_inputs of include/pcseg.h, field for field."""
    _fields_ = [("B", ctypes.c_int32), ("cap", ctypes.c_int32), ("n_slots", ctypes.c_int32),
                ("frame_ids", _P),
                ("counts", _P), ("kind", _P), ("slot_of", _P), ("cells", _P),
                ("n_markers", _P), ("ws_stats", _P),
                ("parent", _P), ("parent_px", _P), ("n_overlap", _P), ("cls_r", _P),
                ("kind_r", _P), ("slot_r", _P), ("cells_r", _P), ("type_stats_r", _P),
                ("nan_flag_r", _P),
                ("parent_overflow", _P)]


def load():
    """Load libpcseg.so and declare every prototype of include/pcseg.h."""
    global _lib
    if _lib is not None:
        return _lib
    # PCSEG_LIB: an A/B build of the SAME library (particle_col_image_segmentation_amd.build.build(out_dir=...)), for
    # same-box kernel comparisons; never a different implementation -- the prototypes below must all resolve
    path = os.environ.get("PCSEG_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise PcsegError(
            "libpcseg.so is not built (%s). Run `python -m particle_col_image_segmentation_amd.build` "
            "or __graft_entry__.build(); there is no CPU fallback." % path)
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().pcseg_last_error()
        raise PcsegError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))
