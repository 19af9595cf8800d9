"""ctypes binding of the C-ABI in include/avr.h (libavr_hip.so, built in-tree).

This is the same binding a pbrt-side Python tool (or the ctypes stub in
INTEGRATION.md) would use. There is no fallback: if the HIP library is missing or
fails to load, importing the product raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# AVR_LIB overrides the library path (A/B experiments with variant builds); default in-tree.
LIB_PATH = os.environ.get("AVR_LIB", os.path.join(_HERE, "libavr_hip.so"))

c_float_p = ctypes.POINTER(ctypes.c_float)
c_double_p = ctypes.POINTER(ctypes.c_double)
c_int_p = ctypes.POINTER(ctypes.c_int)
c_u64_p = ctypes.POINTER(ctypes.c_ulonglong)
# pbrt's Inv4Pi as a float: the uniform graph render's default light_scale
INV_4PI = float(np.float32(0.07957747154594766788))


class AvrStats(ctypes.Structure):
    _fields_ = [
        ("medium_lookups", ctypes.c_ulonglong),
        ("medium_items_in", ctypes.c_ulonglong),
        ("medium_items_out", ctypes.c_ulonglong),
        ("shadow_lookups", ctypes.c_ulonglong),
        ("shadow_items", ctypes.c_ulonglong),
        ("medium_dda_steps", ctypes.c_ulonglong),
        ("shadow_dda_steps", ctypes.c_ulonglong),
        ("medium_launches", ctypes.c_ulonglong),
        ("loop_iterations", ctypes.c_ulonglong),
        ("active_lane_iterations", ctypes.c_ulonglong),
        ("ms_camera", ctypes.c_double),
        ("ms_medium", ctypes.c_double),
        ("ms_shadow", ctypes.c_double),
        ("ms_film", ctypes.c_double),
        ("ms_total", ctypes.c_double),
        ("ms_setup", ctypes.c_double),
        ("ms_binning", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AvrGraphSampling(ctypes.Structure):
    """avr_graph_sampling (include/avr.h): the graph tools' sampler setup."""
    _fields_ = [("sampler", ctypes.c_int), ("seed", ctypes.c_int), ("samples_per_pixel", ctypes.c_int),
                ("film_width", ctypes.c_int), ("film_height", ctypes.c_int), ("resolution_x", ctypes.c_int)]


class AvrGraphMergeStats(ctypes.Structure):
    """avr_graph_merge_stats (include/avr.h): one avr_graph_add_walks_device call."""
    _fields_ = [("rounds", ctypes.c_int), ("points", ctypes.c_longlong), ("new_vertices", ctypes.c_longlong),
                ("ms_sort", ctypes.c_double), ("ms_rounds", ctypes.c_double), ("ms_replay", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# avr_graph_set_geometry's values by the names graph.MediumData(primitive=...) uses
GRAPH_GEOMETRY = {"box": 0, "interface": 1}


class AvrVdbGrid(ctypes.Structure):
    """avr_vdb_grid (include/avr.h): one NanoVDB FloatGrid's tree."""
    _fields_ = [
        ("n_leaves", ctypes.c_int),
        ("leaf_origin", c_int_p),
        ("leaf_values", c_float_p),
        ("n_tiles", ctypes.c_int),
        ("tile_origin", c_int_p),
        ("tile_size", c_int_p),
        ("tile_value", c_float_p),
        ("background", ctypes.c_float),
        ("index_bbox", ctypes.c_int * 6),
        ("index_to_world", ctypes.c_double * 12),
        ("world_to_index", ctypes.c_double * 9),
    ]

    @classmethod
    def of(cls, grid):
        """Struct view of a vdb.NanoVDBGrid (the grid's arrays must outlive the call)."""
        g = cls()
        ip = lambda a: a.ctypes.data_as(c_int_p) if a.size else None
        g.n_leaves = len(grid.leaf_origins)
        g.leaf_origin = ip(grid.leaf_origins)
        g.leaf_values = grid.leaf_values.ctypes.data_as(c_float_p) if grid.leaf_values.size else None
        g.n_tiles = len(grid.tile_values)
        g.tile_origin = ip(grid.tile_origins)
        g.tile_size = ip(grid.tile_sizes)
        g.tile_value = grid.tile_values.ctypes.data_as(c_float_p) if grid.tile_values.size else None
        g.background = float(grid.background)
        g.index_bbox[:] = [int(v) for v in grid.index_bbox]
        g.index_to_world[:] = [float(v) for v in grid.index_to_world.reshape(-1)]
        g.world_to_index[:] = [float(v) for v in grid.world_to_index.reshape(-1)]
        return g


# name -> (restype, argtypes); every symbol include/avr.h declares
SIGNATURES = {
    "avr_last_error": (ctypes.c_char_p, []),
    "avr_context_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_void_p)]),
    "avr_context_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "avr_set_stream": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "avr_set_kernel_mode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "avr_set_render_mode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "avr_record_lookups": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]),
    "avr_density_fetch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, c_float_p, c_float_p]),
    "avr_vdb_fetch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, c_float_p,
                                     c_float_p]),
    "avr_rgbgrid_probe": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, c_float_p, c_float_p, c_float_p, c_float_p,
                                         c_float_p]),
    "avr_set_ray_binning": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "avr_set_majorant_occupancy": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "avr_set_pass_table_ahead": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "avr_set_pass_overlap": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "avr_pass_overlap_active": (ctypes.c_int, [ctypes.c_void_p]),
    "avr_set_majorant_res": (ctypes.c_int, [ctypes.c_void_p, c_int_p]),
    "avr_medium_boundary_sphere": (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_float]),
    "avr_medium_boundary_convex": (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_int]),
    "avr_tune_majorant": (ctypes.c_int, [ctypes.c_void_p, c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, c_int_p, c_float_p]),
    "avr_tune_walk": (ctypes.c_int, [ctypes.c_void_p, c_int_p, ctypes.c_int, c_int_p, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_int, c_int_p, c_float_p]),
    "avr_set_refill_min": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "avr_set_refill_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "avr_light_sampler": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "avr_light_probe": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [c_float_p] * 8),
    "avr_light_pick": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_float_p, c_int_p, c_float_p]),
    "avr_light_sampler_table": (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_int_p]),
    "avr_light_local": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_float_p, c_float_p, ctypes.c_float,
                                       ctypes.c_float]),
    "avr_light_probe_at": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [c_float_p] * 7),
    "avr_light_pick_at": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_float_p, c_float_p, c_int_p, c_float_p]),
    "avr_light_bvh": (ctypes.c_int, [ctypes.c_void_p, c_int_p, c_float_p, c_float_p, c_int_p, c_int_p, c_int_p, c_int_p,
                                     c_float_p, c_int_p]),
    "avr_set_dda_budget": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "avr_set_grid_layout": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "avr_grid_layout_active": (ctypes.c_int, [ctypes.c_void_p]),
    "avr_medium_grid": (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, ctypes.c_float,
                                       c_float_p, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_int_p]),
    "avr_medium_grid_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p,
                                              ctypes.c_float, c_float_p, c_float_p, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, c_int_p]),
    "avr_generate_cloud": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong,
                                          ctypes.c_longlong, ctypes.c_float, ctypes.c_float, ctypes.c_float]),
    "avr_generate_rgb_explosion": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong]),
    "avr_medium_rgbgrid_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                 c_float_p, c_float_p, c_float_p, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_float, ctypes.c_float, ctypes.c_void_p, c_float_p,
                                                 ctypes.c_float]),
    "avr_read_majorant": (ctypes.c_int, [ctypes.c_void_p, c_float_p]),
    "avr_lights": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_int_p, c_float_p, c_float_p, c_float_p,
                                  ctypes.c_float]),
    "avr_camera": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_float_p, c_float_p]),
    "avr_camera_lens": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_float, ctypes.c_float]),
    "avr_camera_spherical": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_float_p]),
    "avr_light_image": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_float_p, c_float_p, c_float_p,
                                       c_float_p, c_float_p]),
    "avr_flip": (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                c_float_p]),
    "avr_film_image_device": (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_int, ctypes.c_void_p]),
    "avr_film_set_reference": (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, ctypes.c_int]),
    "avr_film_metric": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_float_p]),
    "avr_last_pass_weights": (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_longlong]),
    "avr_last_pass_rays": (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, ctypes.c_longlong]),
    "avr_last_kernel": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]),
    "avr_transmittance": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, c_float_p, c_float_p, c_float_p,
                                         c_float_p]),
    "avr_transmittance_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "avr_medium_temperature": (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_float, ctypes.c_float]),
    "avr_medium_homogeneous": (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p,
                                              c_float_p, ctypes.c_float, c_float_p]),
    "avr_medium_cloud": (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p,
                                        ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float]),
    "avr_medium_nanovdb": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(AvrVdbGrid), ctypes.POINTER(AvrVdbGrid),
                                          c_float_p, c_float_p, c_float_p, c_float_p, ctypes.c_float, ctypes.c_float,
                                          ctypes.c_float, ctypes.c_float]),
    "avr_medium_bounds": (ctypes.c_int, [ctypes.c_void_p, c_float_p]),
    "avr_medium_rgbgrid": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_float_p,
                                          c_float_p, c_float_p, c_float_p, c_float_p, ctypes.c_float, ctypes.c_float,
                                          c_float_p, c_float_p, ctypes.c_float]),
    "avr_set_filter": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_float_p, ctypes.c_float]),
    "avr_set_sampler": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "avr_set_sampler_table": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "avr_set_sampler_pass_table": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "avr_set_pixel_order": (ctypes.c_int, [ctypes.c_void_p, c_int_p, ctypes.c_longlong]),
    "avr_film": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_float_p, c_float_p, ctypes.c_float,
                                ctypes.c_float]),
    "avr_film_clear": (ctypes.c_int, [ctypes.c_void_p]),
    "avr_render": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "avr_sync": (ctypes.c_int, [ctypes.c_void_p]),
    "avr_get_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(AvrStats)]),
    "avr_reset_stats": (ctypes.c_int, [ctypes.c_void_p]),
    "avr_film_read": (ctypes.c_int, [ctypes.c_void_p, c_double_p, c_double_p]),
    "avr_film_pixel_bounds": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "avr_film_get_bounds": (ctypes.c_int, [ctypes.c_void_p, c_int_p, c_int_p, c_int_p, c_int_p]),
    "avr_film_spectral": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float]),
    "avr_film_read_spectral": (ctypes.c_int, [ctypes.c_void_p, c_double_p, c_double_p]),
    "avr_film_spectral_device_ptrs": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
                                                     ctypes.POINTER(ctypes.c_void_p)]),
    "avr_film_device_ptrs": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
                                            ctypes.POINTER(ctypes.c_void_p)]),
    "avr_film_export_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "avr_film_reduce_rccl": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int]),
    "avr_last_pass_samples": (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, ctypes.c_longlong,
                                             c_int_p, c_int_p]),
    "avr_graph_set_geometry": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "avr_graph_start_rays": (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_float, c_float_p, ctypes.c_int,
                                            c_int_p, c_float_p, c_float_p]),
    "avr_graph_walks": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(AvrGraphSampling), ctypes.c_longlong, c_float_p,
                                       c_float_p, c_float_p, ctypes.POINTER(ctypes.c_longlong), ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, c_float_p, c_int_p]),
    "avr_graph_walks_from": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(AvrGraphSampling), ctypes.c_longlong,
                                            c_float_p, c_float_p, c_float_p, ctypes.POINTER(ctypes.c_longlong),
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_float_p, c_int_p]),
    "avr_graph_reinforce_rays": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(AvrGraphSampling), ctypes.c_int,
                                                c_int_p, c_float_p, ctypes.c_float, ctypes.c_int, ctypes.c_int,
                                                c_float_p, c_float_p, c_float_p, c_int_p]),
    "avr_graph_add_walks_from": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, c_float_p, c_int_p,
                                                c_int_p]),
    "avr_graph_merge_assign": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, c_float_p, c_int_p,
                                              c_int_p, c_int_p, c_int_p]),
    "avr_graph_merge_assign_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                                     c_float_p, c_int_p, c_int_p, c_int_p, c_int_p]),
    "avr_graph_add_walks_assigned": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, c_float_p,
                                                    c_int_p, c_int_p, c_int_p]),
    "avr_graph_add_walks_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                                  c_float_p, c_int_p, c_int_p, ctypes.c_void_p]),
    "avr_graph_out_degrees": (ctypes.c_int, [ctypes.c_void_p, c_int_p]),
    "avr_graph_count_in_radius": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_int_p, ctypes.c_float, c_int_p]),
    "avr_graph_light": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(AvrGraphSampling), ctypes.c_int, c_float_p,
                                       c_float_p, ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                       c_float_p]),
    "avr_graph_propagate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_int_p, c_int_p, c_float_p, c_float_p,
                                           ctypes.c_int, c_float_p, c_int_p]),
    "avr_graph_propagate_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                  ctypes.c_void_p, c_int_p]),
    "avr_graph_create": (ctypes.c_int, [ctypes.c_float, ctypes.POINTER(ctypes.c_void_p)]),
    "avr_graph_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "avr_graph_add_walks": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, c_float_p, c_int_p]),
    "avr_graph_size": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong),
                                      ctypes.POINTER(ctypes.c_longlong)]),
    "avr_graph_vertices": (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_int_p]),
    "avr_graph_edges": (ctypes.c_int, [ctypes.c_void_p, c_int_p, c_int_p, c_int_p]),
    "avr_graph_transport": (ctypes.c_int, [ctypes.c_void_p, c_int_p, c_int_p, c_float_p]),
    "avr_graph_in_node_path_length": (ctypes.c_int, [ctypes.c_void_p, c_float_p,
                                                     ctypes.POINTER(ctypes.c_longlong)]),
    "avr_graph_index_create": (ctypes.c_int, [ctypes.c_longlong, c_float_p, c_float_p, c_float_p, ctypes.c_float,
                                              ctypes.POINTER(ctypes.c_void_p)]),
    "avr_graph_index_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "avr_graph_index_connect": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, c_float_p, c_float_p, c_int_p]),
    "avr_graph_connect": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, c_float_p, c_float_p,
                                         c_int_p]),
    "avr_graph_index_knn": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_int_p, c_float_p]),
    "avr_graph_index_search_ranges": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_float_p]),
    "avr_graph_knn": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, c_int_p, c_float_p]),
    "avr_graph_search_ranges": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, c_float_p]),
    "avr_graph_render": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_float_p, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int]),
    "avr_graph_last_pass": (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_int_p,
                                           ctypes.c_longlong]),
    "avr_graph_uniform_create": (ctypes.c_int, [ctypes.c_longlong, c_int_p, c_float_p, ctypes.c_float,
                                                ctypes.POINTER(ctypes.c_void_p)]),
    "avr_graph_uniform_from_points": (ctypes.c_int, [ctypes.c_longlong, c_float_p, c_float_p, ctypes.c_float,
                                                     ctypes.c_int, c_int_p, ctypes.POINTER(ctypes.c_void_p)]),
    "avr_graph_uniform_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "avr_graph_uniform_size": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong), c_float_p]),
    "avr_graph_uniform_get": (ctypes.c_int, [ctypes.c_void_p, c_int_p, c_float_p]),
    "avr_graph_uniform_lookup": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, c_float_p, c_int_p, c_float_p]),
    "avr_graph_uniform_trace": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, c_float_p, c_float_p, c_int_p,
                                               c_float_p, c_float_p]),
    "avr_graph_uniform_lookup_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, c_float_p,
                                                       c_int_p, c_float_p]),
    "avr_graph_uniform_trace_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, c_float_p,
                                                      c_float_p, c_int_p, c_float_p, c_float_p]),
    "avr_graph_render_uniform": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_float_p, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_int, ctypes.c_float]),
    "avr_graph_index_coverage": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, c_float_p, c_int_p, c_int_p,
                                                c_float_p]),
    "avr_graph_coverage": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, c_float_p, c_int_p,
                                          c_int_p, c_float_p]),
    "avr_graph_analyze": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_float_p, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "avr_graph_analysis_read": (ctypes.c_int, [ctypes.c_void_p, c_u64_p, c_u64_p, c_u64_p, c_u64_p, c_double_p]),
    "avr_graph_analysis_clear": (ctypes.c_int, [ctypes.c_void_p]),
    "avr_graph_analyze_last_pass": (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_int_p, c_float_p, c_int_p,
                                                   c_int_p, c_float_p, ctypes.c_longlong, ctypes.c_int]),
    "avr_graph_capture": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_float_p, c_float_p, c_float_p, c_float_p,
                                         ctypes.c_int, c_float_p, ctypes.POINTER(ctypes.c_longlong)]),
    "avr_graph_uniform_count_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, c_float_p, ctypes.c_float,
                                                      ctypes.POINTER(ctypes.c_longlong)]),
    "avr_graph_uniform_from_points_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, c_float_p, ctypes.c_float,
                                                            ctypes.POINTER(ctypes.c_void_p), c_int_p]),
    "avr_graph_voxels_create": (ctypes.c_int, [c_float_p, c_float_p, ctypes.c_float, ctypes.c_longlong, c_int_p,
                                               ctypes.POINTER(ctypes.c_void_p)]),
    "avr_graph_voxels_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "avr_graph_voxels_single_layer": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_int_p]),
    "avr_graph_voxels_fill": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, c_int_p]),
    "avr_graph_voxels_state": (ctypes.c_int, [ctypes.c_void_p, c_int_p, c_int_p, ctypes.c_void_p, ctypes.c_longlong]),
    "avr_graph_voxels_visited": (ctypes.c_int, [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_longlong)] * 4),
}

_lib = None


def load():
    """Load libavr_hip.so (no GPU is touched). Raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
    lib = ctypes.CDLL(LIB_PATH)
    # a variant library named by AVR_LIB (A/B runs against older builds) may lack the newest
    # entry points (calling one then raises AttributeError); the in-tree library must export
    # every one, so a stale build fails here, at load, naming what is missing
    variant = os.path.abspath(LIB_PATH) != os.path.join(_HERE, "libavr_hip.so")
    missing = []
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            missing.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    if missing and not variant:
        raise RuntimeError(f"{LIB_PATH} is stale: it lacks {', '.join(missing)} — rebuild it (__graft_entry__.build())")
    _lib = lib
    return lib


def _fp(a):
    return a.ctypes.data_as(c_float_p) if a is not None else None


def _check(rc):
    if rc != 0:
        raise RuntimeError(f"avr error {rc}: {_lib.avr_last_error().decode()}")


class Context:
    """One HIP device context of the integrator (avr_context_create)."""

    def __init__(self, device=0, max_paths=0):
        self.lib = load()
        h = ctypes.c_void_p()
        _check(self.lib.avr_context_create(int(device), int(max_paths), ctypes.byref(h)))
        self.h = h
        self.device = int(device)
        self._keep = []

    def close(self):
        if self.h:
            self.lib.avr_context_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_render_mode(self, mode):
        """0 / "replay": canonical math, per-sample parity with the CPU oracle; 1 / "fast":
        hardware transcendentals, statistical parity (avr_set_render_mode)."""
        m = {"replay": 0, "fast": 1}.get(mode, mode)
        _check(self.lib.avr_set_render_mode(self.h, int(m)))

    def set_majorant_res(self, res):
        r = np.asarray(res, np.int32).reshape(3)
        _check(self.lib.avr_set_majorant_res(self.h, r.ctypes.data_as(c_int_p)))

    def tune_majorant(self, candidates, spp_begin, spp_end, seed, max_depth):
        """avr_tune_majorant: returns (chosen (x, y, z), per-candidate probe ms)."""
        cand = np.ascontiguousarray(np.asarray(candidates, np.int32).reshape(-1, 3))
        chosen = np.zeros(3, np.int32)
        ms = np.zeros(len(cand), np.float32)
        _check(self.lib.avr_tune_majorant(self.h, cand.ctypes.data_as(c_int_p), len(cand), int(spp_begin),
                                          int(spp_end), int(seed), int(max_depth), chosen.ctypes.data_as(c_int_p),
                                          ms.ctypes.data_as(c_float_p)))
        return tuple(int(v) for v in chosen), ms

    def tune_walk(self, refill, dda, spp_begin, spp_end, seed, max_depth):
        """avr_tune_walk: returns ((refill, dda) chosen, probe ms as a len(refill) x len(dda) array)."""
        r = np.ascontiguousarray(np.asarray(refill, np.int32).ravel())
        d = np.ascontiguousarray(np.asarray(dda, np.int32).ravel())
        chosen = np.zeros(2, np.int32)
        ms = np.zeros(len(r) * len(d), np.float32)
        _check(self.lib.avr_tune_walk(self.h, r.ctypes.data_as(c_int_p), len(r), d.ctypes.data_as(c_int_p), len(d),
                                      int(spp_begin), int(spp_end), int(seed), int(max_depth),
                                      chosen.ctypes.data_as(c_int_p), ms.ctypes.data_as(c_float_p)))
        return (int(chosen[0]), int(chosen[1])), ms.reshape(len(r), len(d))

    def set_ray_binning(self, on):
        _check(self.lib.avr_set_ray_binning(self.h, 1 if on else 0))

    def set_majorant_occupancy(self, on):
        _check(self.lib.avr_set_majorant_occupancy(self.h, 1 if on else 0))

    def set_pass_table_ahead(self, on):
        _check(self.lib.avr_set_pass_table_ahead(self.h, 1 if on else 0))

    def set_pass_overlap(self, on):
        """Run the next pass's camera stage on the side stream while k_paths runs (default on)."""
        _check(self.lib.avr_set_pass_overlap(self.h, 1 if on else 0))

    def pass_overlap_active(self):
        """Whether the last pass took camera records made ahead."""
        return bool(self.lib.avr_pass_overlap_active(self.h))

    def record_lookups(self, d_points, cap, d_count):
        """Trace the wavefront kernels' density fetches into device buffers (0 / None stops)."""
        _check(self.lib.avr_record_lookups(self.h, ctypes.c_void_p(d_points or None), int(cap),
                                           ctypes.c_void_p(d_count or None)))

    def density_fetch(self, d_points, n, d_out):
        """avr_density_fetch on device buffers; returns the kernel time in ms."""
        ms = ctypes.c_float(0.0)
        _check(self.lib.avr_density_fetch(self.h, ctypes.c_void_p(d_points), int(n),
                                          ctypes.cast(ctypes.c_void_p(d_out), c_float_p), ctypes.byref(ms)))
        return float(ms.value)

    def vdb_fetch(self, grid, d_points, n, d_out):
        """avr_vdb_fetch (grid 0 density, 1 temperature) on device buffers of medium-space float4
        points; returns the kernel time in ms."""
        ms = ctypes.c_float(0.0)
        _check(self.lib.avr_vdb_fetch(self.h, int(grid), ctypes.c_void_p(d_points or None), int(n),
                                      ctypes.cast(ctypes.c_void_p(d_out or None), c_float_p), ctypes.byref(ms)))
        return float(ms.value)

    def rgbgrid_probe(self, points, lam, outputs=("sigma_a", "sigma_s", "Le")):
        """avr_rgbgrid_probe: RGBGridMedium::SamplePoint at n render-space points (n, 3) and
        wavelength sets (n, 4) in nm; returns (sigma_a, sigma_s, Le), each (n, 4) float32, or
        None for an output not named in `outputs` (passed as NULL)."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        lam = np.ascontiguousarray(lam, np.float32).reshape(-1, 4)
        if len(p) != len(lam):
            raise ValueError("rgbgrid_probe: one wavelength set per point")
        out = [np.zeros((len(p), 4), np.float32) if k in outputs else None for k in ("sigma_a", "sigma_s", "Le")]
        _check(self.lib.avr_rgbgrid_probe(self.h, len(p), _fp(p), _fp(lam), *[_fp(o) for o in out]))
        return tuple(out)

    def set_kernel_mode(self, mode):
        """0 = persistent megakernel (default), 1 = wavefront queues."""
        _check(self.lib.avr_set_kernel_mode(self.h, int(mode)))

    def set_grid_layout(self, layout):
        """1 = fat footprint copy (default), 0 = pbrt's linear layout only; applies to the next set_scene."""
        _check(self.lib.avr_set_grid_layout(self.h, int(layout)))

    def grid_layout_active(self):
        return int(self.lib.avr_grid_layout_active(self.h))

    def set_dda_budget(self, cells):
        _check(self.lib.avr_set_dda_budget(self.h, int(cells)))

    def set_light_sampler(self, kind):
        """0: "bvh" (pbrt's BVHLightSampler); 1: "power"; 2: "uniform" — 0 and 2 are the same pick for
        lists of infinite lights (avr_light_sampler)."""
        _check(self.lib.avr_light_sampler(self.h, int(kind)))

    def light_probe(self, index, u2, w3, lambda4):
        """avr_light_probe of light `index`: (wi (n, 3), pdf of the sample (n), Ls (n, 4), PDF_Li (n),
        Le (n, 4)) for n (u0, u1), escaping directions and wavelength sets."""
        u2 = np.ascontiguousarray(u2, np.float32).reshape(-1, 2)
        w3 = np.ascontiguousarray(w3, np.float32).reshape(-1, 3)
        lam = np.ascontiguousarray(lambda4, np.float32).reshape(-1, 4)
        n = len(u2)
        if len(w3) != n or len(lam) != n:
            raise ValueError("light_probe: u2, w3 and lambda4 need one row per probe")
        wi, ps, Ls = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros((n, 4), np.float32)
        pl, Le = np.zeros(n, np.float32), np.zeros((n, 4), np.float32)
        _check(self.lib.avr_light_probe(self.h, int(index), n, _fp(u2), _fp(w3), _fp(lam), _fp(wi), _fp(ps), _fp(Ls),
                                        _fp(pl), _fp(Le)))
        return wi, ps, Ls, pl, Le

    def light_pick(self, u):
        """avr_light_pick: (index (-1: none), pmf) of the light sampler's pick per draw."""
        u = np.ascontiguousarray(u, np.float32).reshape(-1)
        idx, pmf = np.zeros(len(u), np.int32), np.zeros(len(u), np.float32)
        _check(self.lib.avr_light_pick(self.h, len(u), _fp(u), idx.ctypes.data_as(c_int_p), _fp(pmf)))
        return idx, pmf

    def light_probe_at(self, index, u2, p3, lambda4):
        """avr_light_probe_at of light `index`: (wi (n, 3), pdf of the sample (n), Ls (n, 4), distance (n))
        of SampleLi at n render-space reference points."""
        u2 = np.ascontiguousarray(u2, np.float32).reshape(-1, 2)
        p3 = np.ascontiguousarray(p3, np.float32).reshape(-1, 3)
        lam = np.ascontiguousarray(lambda4, np.float32).reshape(-1, 4)
        n = len(p3)
        if len(u2) != n or len(lam) != n:
            raise ValueError("light_probe_at: u2, p3 and lambda4 need one row per probe")
        wi, ps, Ls, r = (np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros((n, 4), np.float32),
                         np.zeros(n, np.float32))
        _check(self.lib.avr_light_probe_at(self.h, int(index), n, _fp(u2), _fp(p3), _fp(lam), _fp(wi), _fp(ps), _fp(Ls),
                                           _fp(r)))
        return wi, ps, Ls, r

    def light_pick_at(self, u, p3):
        """avr_light_pick_at: (index (-1: none), pmf) of the light sampler's pick per draw u at point p."""
        u = np.ascontiguousarray(u, np.float32).reshape(-1)
        p3 = np.ascontiguousarray(p3, np.float32).reshape(-1, 3)
        if len(p3) != len(u):
            raise ValueError("light_pick_at: one point per draw")
        idx, pmf = np.zeros(len(u), np.int32), np.zeros(len(u), np.float32)
        _check(self.lib.avr_light_pick_at(self.h, len(u), _fp(u), _fp(p3), idx.ctypes.data_as(c_int_p), _fp(pmf)))
        return idx, pmf

    def light_bvh(self):
        """avr_light_bvh: dict(phi, w, qcos, qb, link, leaf) per node, all_bounds (pMin, pMax) and n_infinite."""
        ip = lambda a: a.ctypes.data_as(c_int_p)   # noqa: E731
        nn, ninf = np.zeros(1, np.int32), np.zeros(1, np.int32)
        phi, w, qcos, qb = np.zeros(15, np.float32), np.zeros((15, 3), np.float32), np.zeros((15, 2), np.int32), np.zeros(
            (15, 2, 3), np.int32)
        link, leaf, allb = np.zeros(15, np.int32), np.zeros(15, np.int32), np.zeros(6, np.float32)
        _check(self.lib.avr_light_bvh(self.h, ip(nn), _fp(phi), _fp(w), ip(qcos), ip(qb), ip(link), ip(leaf), _fp(allb),
                                      ip(ninf)))
        k = int(nn[0])
        return dict(phi=phi[:k], w=w[:k], qcos=qcos[:k], qb=qb[:k], link=link[:k], leaf=leaf[:k].astype(bool),
                    all_bounds=allb, n_infinite=int(ninf[0]))

    def light_sampler_table(self, n):
        """avr_light_sampler_table of the n lights: (q, p, alias)."""
        q, p, alias = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
        _check(self.lib.avr_light_sampler_table(self.h, _fp(q), _fp(p), alias.ctypes.data_as(c_int_p)))
        return q, p, alias

    def set_refill_min(self, lanes):
        _check(self.lib.avr_set_refill_min(self.h, int(lanes)))

    def set_refill_batch(self, lanes):
        """Fewest waiting lanes for which a k_paths service round refills (0 = default)."""
        _check(self.lib.avr_set_refill_batch(self.h, int(lanes)))

    def set_sampler_table(self, dims):
        """ZSobol pixel-table dimensions (0 = compute every digit per call)."""
        _check(self.lib.avr_set_sampler_table(self.h, int(dims)))

    def set_sampler_pass_table(self, dims):
        """ZSobol per-pass table dimensions (avr_set_sampler_pass_table; 0 = off, default 96)."""
        _check(self.lib.avr_set_sampler_pass_table(self.h, int(dims)))

    def set_pixel_order(self, order):
        """avr_set_pixel_order: the persistent kernel's pixel order (a permutation of the film's
        row-major pixel ids), or None for scanline order."""
        if order is None:
            _check(self.lib.avr_set_pixel_order(self.h, None, 0))
            return
        o = np.ascontiguousarray(np.asarray(order, np.int32).reshape(-1))
        _check(self.lib.avr_set_pixel_order(self.h, o.ctypes.data_as(c_int_p), len(o)))

    def set_stream(self, stream_ptr):
        _check(self.lib.avr_set_stream(self.h, ctypes.c_void_p(stream_ptr)))

    def _check_device(self, tensors):
        """Device grids must live on this context's GPU (the kernels dereference them there)."""
        for t in tensors:
            if t is not None and hasattr(t, "data_ptr") and t.device.index != self.device:
                raise ValueError(f"grid tensor on {t.device}, but the context runs on cuda:{self.device}")

    def set_camera(self, scene):
        """Upload the scene's camera alone: avr_camera and its lens (a radius of 0 is the pinhole), or
        avr_camera_spherical. A Scene's render space is world space moved to the camera's position,
        and medium, lights and interface of the scene set last were uploaded in it: `scene` must have
        the same render_from_world (a camera at the same position; pose, kind and lens may differ),
        else ValueError — use set_scene for a camera that moved."""
        rfw = getattr(self, "_render_from_world", None)
        if rfw is not None and not np.array_equal(rfw, np.asarray(scene.render_from_world, np.float64)):
            raise ValueError("set_camera: the camera's position differs from the scene's set last (its render space "
                             "would disagree with the uploaded medium and lights): use set_scene")
        cam = scene.camera
        f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))
        if int(cam.type_id) == 2:
            _check(self.lib.avr_camera_spherical(self.h, int(cam.mapping_id), _fp(f32(scene.render_from_camera))))
            return
        _check(self.lib.avr_camera(self.h, int(cam.type_id), _fp(f32(scene.camera_from_raster)),
                                   _fp(f32(scene.render_from_camera))))
        if float(getattr(cam, "lensradius", 0.0)) > 0:
            self.set_camera_lens(cam.lensradius, cam.focaldistance)

    def set_camera_lens(self, lensradius, focaldistance=1e6):
        """avr_camera_lens: the thin lens of the camera set last (radius 0: the pinhole)."""
        _check(self.lib.avr_camera_lens(self.h, float(lensradius), float(focaldistance)))

    def set_scene(self, scene):
        med = scene.medium
        self._render_from_world = np.array(scene.render_from_world, np.float64)
        self._check_device([getattr(med, "device_density", None)] +
                           ([med.rgb_sigma_a, med.rgb_sigma_s, med.rgb_Le] if getattr(med, "type_id", 0) == 4 else []))
        mres = np.asarray(med.majorant_res, np.int32)
        f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))
        args = [f32(med.bounds), f32(scene.render_from_medium), f32(scene.medium_from_render), f32(med.sigma_a),
                f32(med.sigma_s)]
        Le = f32(med.Le) if med.Le is not None else None
        ls = f32(med.Lescale)
        self._keep = args + [Le, ls, mres]
        if getattr(med, "type_id", 0) == 1:
            _check(self.lib.avr_medium_homogeneous(self.h, _fp(args[0]), _fp(args[1]), _fp(args[2]), _fp(args[3]),
                                                   _fp(args[4]), float(med.g), _fp(Le)))
        elif getattr(med, "type_id", 0) == 4 and getattr(med, "on_device", False):
            ill = f32(med.illuminant)
            self._keep += [ill]
            ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
            _check(self.lib.avr_medium_rgbgrid_device(
                self.h, med.nx, med.ny, med.nz, _fp(args[0]), _fp(args[1]), _fp(args[2]), ptr(med.rgb_sigma_a),
                ptr(med.rgb_sigma_s), float(med.sigma_scale), float(med.g), ptr(med.rgb_Le), _fp(ill),
                float(med.Le_scale)))
        elif getattr(med, "type_id", 0) == 4:
            grids = [f32(g) if g is not None else None for g in (med.rgb_sigma_a, med.rgb_sigma_s, med.rgb_Le)]
            ill = f32(med.illuminant)
            self._keep += grids + [ill]
            _check(self.lib.avr_medium_rgbgrid(self.h, med.nx, med.ny, med.nz, _fp(args[0]), _fp(args[1]),
                                               _fp(args[2]), _fp(grids[0]), _fp(grids[1]), float(med.sigma_scale),
                                               float(med.g), _fp(grids[2]), _fp(ill), float(med.Le_scale)))
        elif getattr(med, "type_id", 0) == 3:
            dg = AvrVdbGrid.of(med.grid)
            tg = AvrVdbGrid.of(med.temperature_grid) if med.temperature_grid is not None else None
            _check(self.lib.avr_medium_nanovdb(self.h, ctypes.byref(dg), ctypes.byref(tg) if tg is not None else None,
                                               _fp(args[1]), _fp(args[2]), _fp(args[3]), _fp(args[4]), float(med.g),
                                               float(med.Lescale_value), float(med.temperature_offset),
                                               float(med.temperature_scale)))
        elif getattr(med, "type_id", 0) == 2:
            _check(self.lib.avr_medium_cloud(self.h, _fp(args[0]), _fp(args[1]), _fp(args[2]), _fp(args[3]),
                                             _fp(args[4]), float(med.g), *[float(v) for v in med.cloud]))
        elif med.device_density is not None:
            _check(self.lib.avr_medium_grid_device(
                self.h, ctypes.c_void_p(med.device_density.data_ptr()), med.nx, med.ny, med.nz, _fp(args[0]),
                _fp(args[1]), _fp(args[2]), _fp(args[3]), _fp(args[4]), float(med.g), _fp(Le), _fp(ls),
                ls.shape[2], ls.shape[1], ls.shape[0], mres.ctypes.data_as(c_int_p)))
        else:
            _check(self.lib.avr_medium_grid(
                self.h, _fp(med.density), med.nx, med.ny, med.nz, _fp(args[0]), _fp(args[1]), _fp(args[2]),
                _fp(args[3]), _fp(args[4]), float(med.g), _fp(Le), _fp(ls), ls.shape[2], ls.shape[1], ls.shape[0],
                mres.ctypes.data_as(c_int_p)))
        sph = getattr(scene, "interface_sphere_render", None)
        if sph is not None:
            c3 = f32(sph[:3])
            self._keep.append(c3)
            _check(self.lib.avr_medium_boundary_sphere(self.h, _fp(c3), float(sph[3])))
        planes = getattr(scene, "interface_planes_render", None)
        if planes is not None:
            pl = f32(planes.reshape(-1))
            self._keep.append(pl)
            _check(self.lib.avr_medium_boundary_convex(self.h, _fp(pl), len(planes)))
        temp = getattr(med, "temperature", None)
        if temp is not None:
            self._keep.append(temp)
            _check(self.lib.avr_medium_temperature(self.h, _fp(temp), float(med.temperature_scale),
                                                   float(med.temperature_offset)))
        types = np.ascontiguousarray(scene.light_types, np.int32)
        w = f32(scene.light_w.reshape(-1))
        L = f32(scene.light_L.reshape(-1))
        sc = f32(scene.light_scale)
        _check(self.lib.avr_lights(self.h, len(scene.lights), types.ctypes.data_as(c_int_p), _fp(w), _fp(L), _fp(sc),
                                   float(scene.scene_radius)))
        for i, light in enumerate(scene.lights):
            if light.type_id == 2:
                arrs = [f32(light.coeffs), f32(light.distribution), f32(light.illuminant), f32(scene.light_rfl[i]),
                        f32(scene.light_lfr[i])]
                self._keep += arrs
                _check(self.lib.avr_light_image(self.h, i, int(light.res), *[_fp(a) for a in arrs]))
            elif light.type_id in (3, 4):
                arrs = [f32(scene.light_rfl[i]), f32(scene.light_lfr[i])]
                self._keep += arrs
                _check(self.lib.avr_light_local(self.h, i, _fp(arrs[0]), _fp(arrs[1]), float(light.cos_falloff_start),
                                                float(light.cos_falloff_end)))
        self.set_camera(scene)
        film = scene.film
        _check(self.lib.avr_film(self.h, film.width, film.height, _fp(f32(film.filter_radius)), _fp(f32(film.sensor)),
                                 float(film.imaging_ratio), float(film.max_component_value)))
        if getattr(film, "nbuckets", 0):
            _check(self.lib.avr_film_spectral(self.h, int(film.nbuckets), float(film.lambdamin),
                                              float(film.lambdamax)))
        pb = tuple(getattr(film, "pixel_bounds", (0, 0, film.width, film.height)))
        if pb != (0, 0, film.width, film.height):
            self.film_pixel_bounds(*pb)
        flt = film.filter
        _check(self.lib.avr_set_filter(self.h, int(flt.type_id), _fp(f32(flt.radius)), float(flt.sigma)))
        _check(self.lib.avr_set_sampler(self.h, int(scene.sampler.type_id), int(scene.sampler.pixelsamples)))

    def generate_cloud(self, d_out_ptr, n, first, count, density=1.0, wispiness=1.0, frequency=5.0):
        _check(self.lib.avr_generate_cloud(self.h, ctypes.c_void_p(d_out_ptr), int(n), int(first), int(count),
                                           float(density), float(wispiness), float(frequency)))

    def generate_rgb_explosion(self, d_sa_ptr, d_ss_ptr, d_le_ptr, n, first, count):
        """k_rgb_explosion into three float4 device arrays (pointers at element `first`)."""
        _check(self.lib.avr_generate_rgb_explosion(self.h, ctypes.c_void_p(d_sa_ptr), ctypes.c_void_p(d_ss_ptr),
                                                   ctypes.c_void_p(d_le_ptr), int(n), int(first), int(count)))

    def medium_bounds(self):
        out = np.zeros(6, np.float32)
        _check(self.lib.avr_medium_bounds(self.h, _fp(out)))
        return out

    def majorant(self, n):
        out = np.empty(n, np.float32)
        _check(self.lib.avr_read_majorant(self.h, _fp(out)))
        return out

    def film_clear(self):
        _check(self.lib.avr_film_clear(self.h))

    def film_pixel_bounds(self, x0, y0, x1, y1):
        """avr_film_pixel_bounds: render and store the pixels [x0, x1) x [y0, y1) of the film only
        (the sums are reallocated and zeroed; every npix below is then the bounds' pixel count)."""
        _check(self.lib.avr_film_pixel_bounds(self.h, int(x0), int(y0), int(x1), int(y1)))

    def film_bounds(self):
        """(x0, y0, x1, y1) of the film's pixel bounds (avr_film_get_bounds)."""
        v = [ctypes.c_int() for _ in range(4)]
        _check(self.lib.avr_film_get_bounds(self.h, *[ctypes.byref(a) for a in v]))
        return tuple(a.value for a in v)

    def render(self, spp_begin, spp_end, seed, max_depth):
        _check(self.lib.avr_render(self.h, int(spp_begin), int(spp_end), int(seed), int(max_depth)))

    def sync(self):
        _check(self.lib.avr_sync(self.h))

    def reset_stats(self):
        _check(self.lib.avr_reset_stats(self.h))

    def stats(self):
        """Counters and kernel times accumulated since creation or reset_stats()."""
        s = AvrStats()
        _check(self.lib.avr_get_stats(self.h, ctypes.byref(s)))
        return s.as_dict()

    def film_read_spectral(self, npix, nbuckets):
        """SpectralFilm bucket sums: (bucket_sums, weight_sums), each (npix, nbuckets) fp64."""
        bs = np.zeros(npix * nbuckets, np.float64)
        bw = np.zeros(npix * nbuckets, np.float64)
        _check(self.lib.avr_film_read_spectral(self.h, bs.ctypes.data_as(c_double_p), bw.ctypes.data_as(c_double_p)))
        return bs.reshape(npix, nbuckets), bw.reshape(npix, nbuckets)

    def film_read(self, npix):
        rgb = np.zeros(3 * npix, np.float64)
        w = np.zeros(npix, np.float64)
        _check(self.lib.avr_film_read(self.h, rgb.ctypes.data_as(c_double_p), w.ctypes.data_as(c_double_p)))
        return rgb, w

    def last_pass_samples(self, npix, max_samples):
        n = npix * max_samples
        L = np.zeros((n, 4), np.float32)
        lam = np.zeros((n, 4), np.float32)
        pdf = np.zeros((n, 4), np.float32)
        first, ns = ctypes.c_int(), ctypes.c_int()
        _check(self.lib.avr_last_pass_samples(self.h, _fp(L), _fp(lam), _fp(pdf), n, ctypes.byref(first),
                                              ctypes.byref(ns)))
        m = npix * ns.value
        return first.value, ns.value, L[:m], lam[:m], pdf[:m]

    def last_kernel(self):
        """Template arguments of the last k_paths instantiation rendered ("k_paths<...>")."""
        buf = ctypes.create_string_buffer(64)
        _check(self.lib.avr_last_kernel(self.h, buf, 64))
        return buf.value.decode()

    def last_pass_weights(self, npix, max_samples):
        w = np.zeros(npix * max_samples, np.float32)
        _check(self.lib.avr_last_pass_weights(self.h, _fp(w), len(w)))
        return w

    def last_pass_rays(self, npix, max_samples):
        """The camera stage's rays of the last persistent pass, indexed as last_pass_samples: the
        origin after the medium-interface entry (n, 3), the direction (n, 3) and the first segment's
        free-flight draw (n), n = npix * max_samples (the pass's samples first)."""
        n = npix * max_samples
        o = np.zeros((n, 3), np.float32)
        d = np.zeros((n, 3), np.float32)
        u = np.zeros(n, np.float32)
        _check(self.lib.avr_last_pass_rays(self.h, _fp(o), _fp(d), _fp(u), n))
        return o, d, u

    def transmittance(self, p0, p1, lam):
        """Integrator::Tr for n queries: p0, p1 (n, 3) render-space points, lam (n, 4) nm."""
        p0 = np.ascontiguousarray(p0, np.float32)
        p1 = np.ascontiguousarray(p1, np.float32)
        lam = np.ascontiguousarray(lam, np.float32)
        out = np.zeros((len(p0), 4), np.float32)
        _check(self.lib.avr_transmittance(self.h, len(p0), _fp(p0), _fp(p1), _fp(lam), _fp(out)))
        return out

    # ---- lighting graph (src/graph) ----
    def set_graph_geometry(self, geometry):
        """The graph tools' primitive for this context: 0 the medium's bounds box (the default),
        1 the medium's interface sphere or mesh (the box when the scene has neither); also
        "box" / "interface". Every graph_* call of the context follows it."""
        geometry = GRAPH_GEOMETRY.get(geometry, geometry)
        if isinstance(geometry, bool) or not isinstance(geometry, (int, np.integer)):
            raise ValueError('graph geometry must be 0 / "box" or 1 / "interface"')
        _check(self.lib.avr_graph_set_geometry(self.h, int(geometry)))

    def graph_start_rays(self, bounds_center, max_dist_to_center, in_dir, steps):
        """BuildGraph's steps x steps ray grid on the device: per grid ray (x outer) the hit
        type (0 OutsideTwoHits, 2 no hit, 3 InsideOneHit), the origin after SkipIntersection
        (n, 3) and the first segment's tMax."""
        ctr = np.ascontiguousarray(bounds_center, np.float32).reshape(3)
        dr = np.ascontiguousarray(in_dir, np.float32).reshape(3)
        n = int(steps) * int(steps)
        ty = np.zeros(n, np.int32)
        o = np.zeros((n, 3), np.float32)
        t = np.zeros(n, np.float32)
        _check(self.lib.avr_graph_start_rays(self.h, _fp(ctr), float(max_dist_to_center), _fp(dr), int(steps),
                                             ty.ctypes.data_as(c_int_p), _fp(o), _fp(t)))
        return ty, o, t

    def graph_walks(self, sampling, o, d, t_first, index0, iterations, sample_index, max_depth, skip_dims=0):
        """FreeGraphBuilder::TracePath walks: (points (n_rays*iterations, max_depth, 3), counts)."""
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        t_first = np.ascontiguousarray(t_first, np.float32)
        index0 = np.ascontiguousarray(index0, np.int64)
        n = len(o) * int(iterations)
        pts = np.zeros((n, max(1, int(max_depth)), 3), np.float32)
        counts = np.zeros(n, np.int32)
        _check(self.lib.avr_graph_walks_from(self.h, ctypes.byref(sampling), len(o), _fp(o), _fp(d), _fp(t_first),
                                             index0.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
                                             int(iterations), int(sample_index), int(skip_dims), int(max_depth),
                                             _fp(pts), counts.ctypes.data_as(c_int_p)))
        return pts, counts

    def graph_reinforce_rays(self, sampling, ids, points, radius, n_rays, cycle):
        """ReinforceSparseVertices' rays: (o, d (n, n_rays, 3), t_first, valid (n, n_rays))."""
        ids = np.ascontiguousarray(ids, np.int32)
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n, k = len(ids), int(n_rays)
        o = np.zeros((n, k, 3), np.float32)
        d = np.zeros((n, k, 3), np.float32)
        t = np.zeros((n, k), np.float32)
        valid = np.zeros((n, k), np.int32)
        _check(self.lib.avr_graph_reinforce_rays(self.h, ctypes.byref(sampling), n, ids.ctypes.data_as(c_int_p),
                                                 _fp(pts), float(radius), k, int(cycle), _fp(o), _fp(d), _fp(t),
                                                 valid.ctypes.data_as(c_int_p)))
        return o, d, t, valid

    def graph_light(self, sampling, vertices, in_dir, radius, points_on_radius, iterations, max_dist_to_center):
        """LightingCalculator::GetLightVector: per-vertex light (Inv4Pi applied)."""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        dr = np.ascontiguousarray(in_dir, np.float32)
        out = np.zeros(len(v), np.float32)
        _check(self.lib.avr_graph_light(self.h, ctypes.byref(sampling), len(v), _fp(v), _fp(dr), float(radius),
                                        int(points_on_radius), int(iterations), float(max_dist_to_center),
                                        _fp(out)))
        return out

    def graph_propagate(self, row_ptr, col, val, light, bounces):
        """LightingCalculator::ComputeFinalLight: (total light, bounces completed)."""
        row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        col = np.ascontiguousarray(col, np.int32)
        val = np.ascontiguousarray(val, np.float32)
        light = np.ascontiguousarray(light, np.float32)
        total = np.zeros(len(light), np.float32)
        it = ctypes.c_int(0)
        _check(self.lib.avr_graph_propagate(self.h, len(light), row_ptr.ctypes.data_as(c_int_p),
                                            col.ctypes.data_as(c_int_p), _fp(val), _fp(light), int(bounces),
                                            _fp(total), ctypes.byref(it)))
        return total, it.value

    def graph_connect(self, index, points):
        """ConnectToGraph on the device for (n, 3) graph-space points: (light, counts), bitwise
        GraphIndex.connect's."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        light = np.zeros(len(p), np.float32)
        counts = np.zeros(len(p), np.int32)
        _check(self.lib.avr_graph_connect(self.h, index.h, len(p), _fp(p), _fp(light), counts.ctypes.data_as(c_int_p)))
        return light, counts

    def graph_knn(self, index, k):
        """GetNClosest for every vertex on the device: (ids, d2), (n, k) each, row = vertex id;
        bitwise GraphIndex.knn's."""
        ids = np.zeros((index.num_vertices, max(int(k), 0)), np.int32)
        d2 = np.zeros(ids.shape, np.float32)
        _check(self.lib.avr_graph_knn(self.h, index.h, int(k), ids.ctypes.data_as(c_int_p), _fp(d2)))
        return ids, d2

    def graph_search_ranges(self, index, k):
        """ComputeSearchRanges on the device: renderSearchRange per vertex id, bitwise
        GraphIndex.search_ranges'."""
        out = np.zeros(index.num_vertices, np.float32)
        _check(self.lib.avr_graph_search_ranges(self.h, index.h, int(k), _fp(out)))
        return out

    def graph_render(self, index, spp_begin, spp_end, seed, graph_from_render=None):
        """GraphIntegrator::Li (free graph) for sample indices [spp_begin, spp_end) into the film."""
        m = None if graph_from_render is None else np.ascontiguousarray(graph_from_render, np.float32).reshape(16)
        _check(self.lib.avr_graph_render(self.h, index.h, _fp(m), int(spp_begin), int(spp_end), int(seed)))

    def graph_uniform_lookup(self, uniform, points):
        """GraphUniform.lookup on the device for (n, 3) graph-space points: (ids, light), bitwise
        the host's."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        ids = np.zeros(len(p), np.int32)
        light = np.zeros(len(p), np.float32)
        _check(self.lib.avr_graph_uniform_lookup_device(self.h, uniform.h, len(p), _fp(p), ids.ctypes.data_as(c_int_p),
                                                        _fp(light)))
        return ids, light

    def graph_uniform_trace(self, uniform, o, d):
        """GraphUniform.trace on the device for (n, 3) graph-space rays: (ids, hit0, hit1), bitwise
        the host's."""
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        if len(o) != len(d):
            raise ValueError("graph_uniform_trace: one direction per origin")
        ids = np.zeros(len(o), np.int32)
        hit0, hit1 = np.zeros(len(o), np.float32), np.zeros(len(o), np.float32)
        _check(self.lib.avr_graph_uniform_trace_device(self.h, uniform.h, len(o), _fp(o), _fp(d),
                                                       ids.ctypes.data_as(c_int_p), _fp(hit0), _fp(hit1)))
        return ids, hit0, hit1

    def graph_capture(self, origin, direction, xvec, yvec, num_steps):
        """VoxelBoundary::CaptureBoundary's ray bundles on the device (avr_graph_capture): per
        bundle an origin, a direction (used as given, not normalised) and the two step vectors,
        (n, 3) each; (2 num_steps + 1)^2 rays per bundle, (i, j) with i outer. Returns (points
        (n_rays, 3), captured (n_rays,) bool, n_captured) in ray order."""
        arrs = [np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (origin, direction, xvec, yvec)]
        nb = len(arrs[0])
        if any(len(a) != nb for a in arrs):
            raise ValueError("graph_capture: one direction and one pair of step vectors per origin")
        side = 2 * int(num_steps) + 1
        n = max(0, nb * side * side) if int(num_steps) >= 0 else 0
        out = np.zeros((n, 4), np.float32) if n <= 2 ** 31 - 1 else np.zeros((1, 4), np.float32)
        cnt = ctypes.c_longlong(0)
        _check(self.lib.avr_graph_capture(self.h, nb, _fp(arrs[0]), _fp(arrs[1]), _fp(arrs[2]), _fp(arrs[3]),
                                          int(num_steps), _fp(out), ctypes.byref(cnt)))
        return np.ascontiguousarray(out[:, :3]), out[:, 3] != 0, cnt.value

    def graph_uniform_count(self, points, spacing):
        """The number of distinct voxels of `spacing` among (n, 3) points, on the device
        (avr_graph_uniform_count_device): GraphUniform.from_points(...).num_vertices."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        cnt = ctypes.c_longlong(0)
        _check(self.lib.avr_graph_uniform_count_device(self.h, len(p), _fp(p), float(spacing), ctypes.byref(cnt)))
        return cnt.value

    def graph_render_uniform(self, uniform, spp_begin, spp_end, seed, graph_from_render=None, view=0,
                             light_scale=INV_4PI):
        """GraphIntegrator::Li (uniform graph) for sample indices [spp_begin, spp_end) into the
        film; view 1 is --graph-debug's voxel view. light_scale: the reference's Inv4Pi by
        default; a graph lit by LightingCalculator already carries it and takes 1."""
        m = None if graph_from_render is None else np.ascontiguousarray(graph_from_render, np.float32).reshape(16)
        _check(self.lib.avr_graph_render_uniform(self.h, uniform.h, _fp(m), int(spp_begin), int(spp_end), int(seed),
                                                 int(view), float(light_scale)))

    def graph_last_pass(self, npix, max_samples):
        """The last graph pass per sample (indexed as last_pass_samples): camera ray o, d, the
        scatter point in render space ((n, 3) each) and the vertices averaged (-1: no scatter)."""
        n = npix * max_samples
        o, d, pts = (np.zeros((n, 3), np.float32) for _ in range(3))
        counts = np.zeros(n, np.int32)
        _check(self.lib.avr_graph_last_pass(self.h, _fp(o), _fp(d), _fp(pts), counts.ctypes.data_as(c_int_p), n))
        return o, d, pts, counts

    def graph_coverage(self, index, points):
        """IntegrationAnalyzer's Analyze on the device for (n, 3) graph-space points: (node,
        in_range, range_sum), bitwise GraphIndex.coverage's."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        node = np.zeros(len(p), np.int32)
        in_range = np.zeros(len(p), np.int32)
        range_sum = np.zeros(len(p), np.float32)
        _check(self.lib.avr_graph_coverage(self.h, index.h, len(p), _fp(p), node.ctypes.data_as(c_int_p),
                                           in_range.ctypes.data_as(c_int_p), _fp(range_sum)))
        return node, in_range, range_sum

    def graph_analyze(self, index, spp_begin, spp_end, seed, max_depth, graph_from_render=None, detail=False):
        """IntegrationAnalyzer::AnalyzeRay for sample indices [spp_begin, spp_end), added to the
        per-pixel sums (graph_analysis_read); detail keeps the last pass's scatters too."""
        m = None if graph_from_render is None else np.ascontiguousarray(graph_from_render, np.float32).reshape(16)
        _check(self.lib.avr_graph_analyze(self.h, index.h, _fp(m), int(spp_begin), int(spp_end), int(seed),
                                          int(max_depth), 1 if detail else 0))

    def graph_analysis_read(self, npix):
        """The analysis' per-pixel sums: (total, node, search, in_range) uint64 and range_sum fp64."""
        out = [np.zeros(npix, np.uint64) for _ in range(4)]
        rs = np.zeros(npix, np.float64)
        _check(self.lib.avr_graph_analysis_read(self.h, *[a.ctypes.data_as(c_u64_p) for a in out],
                                                rs.ctypes.data_as(c_double_p)))
        return out[0], out[1], out[2], out[3], rs

    def graph_analysis_clear(self):
        _check(self.lib.avr_graph_analysis_clear(self.h))

    def graph_analyze_last_pass(self, npix, max_samples, max_depth):
        """The last analysis pass with detail (indexed as last_pass_samples): camera ray o, d
        (n, 3), scatters analysed (n), and per sample max_depth entries of the scatter point
        in render space (n, max_depth, 3), node, in_range and range_sum (n, max_depth)."""
        n, md = npix * max_samples, int(max_depth)
        o, d = (np.zeros((n, 3), np.float32) for _ in range(2))
        counts = np.zeros(n, np.int32)
        pts = np.zeros((n, md, 3), np.float32)
        node, in_range = (np.zeros((n, md), np.int32) for _ in range(2))
        range_sum = np.zeros((n, md), np.float32)
        _check(self.lib.avr_graph_analyze_last_pass(self.h, _fp(o), _fp(d), counts.ctypes.data_as(c_int_p), _fp(pts),
                                                    node.ctypes.data_as(c_int_p), in_range.ctypes.data_as(c_int_p),
                                                    _fp(range_sum), n, md))
        return o, d, counts, pts, node, in_range, range_sum

    def film_export_device(self, d_dst_ptr):
        _check(self.lib.avr_film_export_device(self.h, ctypes.c_void_p(d_dst_ptr)))

    METRICS = {"MSE": 0, "MAE": 1, "MRSE": 2, "ME": 3}

    def flip(self, test_rgb, reference_rgb, ppd=0.0):
        """FLIP error map (H, W) of two (H, W, 3) sRGB-encoded images (ComputeFLIPError)."""
        t = np.ascontiguousarray(test_rgb, np.float32)
        r = np.ascontiguousarray(reference_rgb, np.float32)
        if t.shape != r.shape or t.ndim != 3 or t.shape[2] != 3:
            raise ValueError("FLIP needs two (H, W, 3) images of the same resolution")
        out = np.zeros(t.shape[:2], np.float32)
        _check(self.lib.avr_flip(self.h, _fp(t), _fp(r), t.shape[1], t.shape[0], float(ppd), _fp(out)))
        return out

    def film_image_device(self, d_out_ptr, output_from_sensor, fp16=True):
        m = np.ascontiguousarray(output_from_sensor, np.float32).reshape(9)
        _check(self.lib.avr_film_image_device(self.h, _fp(m), 1 if fp16 else 0, ctypes.c_void_p(d_out_ptr)))

    def film_set_reference(self, reference_rgb, output_from_sensor, fp16=True):
        ref = np.ascontiguousarray(reference_rgb, np.float32)
        x0, y0, x1, y1 = self.film_bounds()
        if ref.size != 3 * (x1 - x0) * (y1 - y0):
            raise ValueError(f"reference image must hold the film's pixel bounds: {(y1 - y0, x1 - x0, 3)}")
        m = np.ascontiguousarray(output_from_sensor, np.float32).reshape(9)
        _check(self.lib.avr_film_set_reference(self.h, _fp(ref), _fp(m), 1 if fp16 else 0))

    def film_metric(self, metric="MSE"):
        """Per-channel metric of the film's image against the reference (ME: (3, 3) rows
        absolute / positive / negative)."""
        out = np.zeros(9, np.float32)
        _check(self.lib.avr_film_metric(self.h, self.METRICS[metric], _fp(out)))
        return out.reshape(3, 3) if metric == "ME" else out[:3].copy()

    def film_device_ptrs(self):
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        _check(self.lib.avr_film_device_ptrs(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value


class Graph:
    """Host FreeGraph assembly (avr_graph_*): walks merged in order, transport CSR."""

    def __init__(self, vertex_radius):
        self.lib = load()
        h = ctypes.c_void_p()
        _check(self.lib.avr_graph_create(float(vertex_radius), ctypes.byref(h)))
        self.h = h
        self.radius = float(vertex_radius)

    def close(self):
        if self.h:
            self.lib.avr_graph_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_walks(self, points, counts, max_depth):
        points = np.ascontiguousarray(points, np.float32)
        counts = np.ascontiguousarray(counts, np.int32)
        _check(self.lib.avr_graph_add_walks(self.h, len(counts), int(max_depth), _fp(points),
                                            counts.ctypes.data_as(c_int_p)))

    def add_walks_from(self, points, counts, max_depth, start_vertex):
        points = np.ascontiguousarray(points, np.float32)
        counts = np.ascontiguousarray(counts, np.int32)
        sv = np.ascontiguousarray(start_vertex, np.int32)
        _check(self.lib.avr_graph_add_walks_from(self.h, len(counts), int(max_depth), _fp(points),
                                                 counts.ctypes.data_as(c_int_p), sv.ctypes.data_as(c_int_p)))

    @staticmethod
    def _walks(points, counts, max_depth, start_vertex):
        points = np.ascontiguousarray(points, np.float32)
        counts = np.ascontiguousarray(counts, np.int32)
        if points.size != len(counts) * int(max_depth) * 3:
            raise ValueError("points must hold n_walks x max_depth x 3 floats")
        sv = None if start_vertex is None else np.ascontiguousarray(start_vertex, np.int32)
        if sv is not None and len(sv) != len(counts):
            raise ValueError("one start vertex per walk")
        return points, counts, sv, (sv.ctypes.data_as(c_int_p) if sv is not None else None)

    def merge_assign(self, points, counts, max_depth, start_vertex=None, ctx=None):
        """The vertex merge in rounds (avr_graph_merge_assign; with a Context
        avr_graph_merge_assign_device, the rounds on the GPU): (vertex_of_point (n_walks,
        max_depth) int32, -1 past a walk's count, and the rounds run). The graph is unchanged;
        the ids are the ones add_walks / add_walks_from would give these walks."""
        points, counts, sv, svp = self._walks(points, counts, max_depth, start_vertex)
        out = np.full((len(counts), int(max_depth)), -1, np.int32)
        rounds = ctypes.c_int(0)
        if ctx is None:
            _check(self.lib.avr_graph_merge_assign(self.h, len(counts), int(max_depth), _fp(points),
                                                   counts.ctypes.data_as(c_int_p), svp, out.ctypes.data_as(c_int_p),
                                                   ctypes.byref(rounds)))
        else:
            _check(self.lib.avr_graph_merge_assign_device(ctx.h, self.h, len(counts), int(max_depth), _fp(points),
                                                          counts.ctypes.data_as(c_int_p), svp,
                                                          out.ctypes.data_as(c_int_p), ctypes.byref(rounds)))
        return out, rounds.value

    def merge_assign_device(self, ctx, points, counts, max_depth, start_vertex=None):
        return self.merge_assign(points, counts, max_depth, start_vertex, ctx=ctx)

    def add_walks_assigned(self, points, counts, max_depth, vertex_of_point, start_vertex=None):
        """add_walks / add_walks_from with every point's vertex given (merge_assign's ids)."""
        points, counts, sv, svp = self._walks(points, counts, max_depth, start_vertex)
        vop = np.ascontiguousarray(vertex_of_point, np.int32)
        if vop.size != len(counts) * int(max_depth):
            raise ValueError("vertex_of_point must hold n_walks x max_depth ids")
        _check(self.lib.avr_graph_add_walks_assigned(self.h, len(counts), int(max_depth), _fp(points),
                                                     counts.ctypes.data_as(c_int_p), svp, vop.ctypes.data_as(c_int_p)))

    def add_walks_device(self, ctx, points, counts, max_depth, start_vertex=None):
        """add_walks / add_walks_from with the merge on the GPU (avr_graph_add_walks_device):
        the same graph; returns the call's avr_graph_merge_stats as a dict."""
        points, counts, sv, svp = self._walks(points, counts, max_depth, start_vertex)
        stats = AvrGraphMergeStats()
        _check(self.lib.avr_graph_add_walks_device(ctx.h, self.h, len(counts), int(max_depth), _fp(points),
                                                   counts.ctypes.data_as(c_int_p), svp, ctypes.byref(stats)))
        return stats.as_dict()

    def out_degrees(self):
        nv, _ = self.size()
        out = np.zeros(nv, np.int32)
        _check(self.lib.avr_graph_out_degrees(self.h, out.ctypes.data_as(c_int_p)))
        return out

    def count_in_radius(self, ids, radius):
        ids = np.ascontiguousarray(ids, np.int32)
        out = np.zeros(len(ids), np.int32)
        _check(self.lib.avr_graph_count_in_radius(self.h, len(ids), ids.ctypes.data_as(c_int_p), float(radius),
                                                  out.ctypes.data_as(c_int_p)))
        return out

    def size(self):
        nv, ne = ctypes.c_longlong(), ctypes.c_longlong()
        _check(self.lib.avr_graph_size(self.h, ctypes.byref(nv), ctypes.byref(ne)))
        return nv.value, ne.value

    def vertices(self):
        nv, _ = self.size()
        xyz = np.zeros((nv, 3), np.float32)
        smp = np.zeros(nv, np.int32)
        _check(self.lib.avr_graph_vertices(self.h, _fp(xyz), smp.ctypes.data_as(c_int_p)))
        return xyz, smp

    def edges(self):
        _, ne = self.size()
        f, t, s = (np.zeros(ne, np.int32) for _ in range(3))
        _check(self.lib.avr_graph_edges(self.h, f.ctypes.data_as(c_int_p), t.ctypes.data_as(c_int_p),
                                        s.ctypes.data_as(c_int_p)))
        return f, t, s

    def transport(self):
        nv, ne = self.size()
        rp = np.zeros(nv + 1, np.int32)
        col = np.zeros(ne, np.int32)
        val = np.zeros(ne, np.float32)
        _check(self.lib.avr_graph_transport(self.h, rp.ctypes.data_as(c_int_p), col.ctypes.data_as(c_int_p),
                                            _fp(val)))
        return rp, col, val

    def in_node_path_length(self):
        a, n = ctypes.c_float(), ctypes.c_longlong()
        _check(self.lib.avr_graph_in_node_path_length(self.h, ctypes.byref(a), ctypes.byref(n)))
        return a.value, n.value


class GraphIndex:
    """The graph render's vertex index (avr_graph_index_*): vertices (n, 3), their lightScalar,
    optionally their renderSearchRange, and the vertex radius. Host code; Context.graph_render
    and Context.graph_connect upload it to the device on first use."""

    def __init__(self, points, light_scalar, search_range=None, radius=None):
        if radius is None:
            raise ValueError("GraphIndex needs the graph's vertex radius")
        self.lib = load()
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        light = np.ascontiguousarray(light_scalar, np.float32).reshape(-1)
        rng = None if search_range is None else np.ascontiguousarray(search_range, np.float32).reshape(-1)
        if len(light) != len(p) or (rng is not None and len(rng) != len(p)):
            raise ValueError("GraphIndex: one light scalar (and search range) per vertex")
        h = ctypes.c_void_p()
        self.h = None
        _check(self.lib.avr_graph_index_create(len(p), _fp(p), _fp(light), _fp(rng), float(radius), ctypes.byref(h)))
        self.h = h
        self.num_vertices = len(p)
        self.radius = float(radius)
        self.has_search_range = rng is not None

    def connect(self, points):
        """ConnectToGraph on the host for (n, 3) graph-space points: (light, counts)."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        light = np.zeros(len(p), np.float32)
        counts = np.zeros(len(p), np.int32)
        _check(self.lib.avr_graph_index_connect(self.h, len(p), _fp(p), _fp(light), counts.ctypes.data_as(c_int_p)))
        return light, counts

    def coverage(self, points):
        """IntegrationAnalyzer's Analyze on the host for (n, 3) graph-space points: node (a
        vertex within the vertex radius), in_range (vertices within their own search range)
        and range_sum (the float sum of their distances, nearest first)."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        node = np.zeros(len(p), np.int32)
        in_range = np.zeros(len(p), np.int32)
        range_sum = np.zeros(len(p), np.float32)
        _check(self.lib.avr_graph_index_coverage(self.h, len(p), _fp(p), node.ctypes.data_as(c_int_p),
                                                 in_range.ctypes.data_as(c_int_p), _fp(range_sum)))
        return node, in_range, range_sum

    def knn(self, k):
        """GetNClosest for every vertex on the host: the k nearest other vertices in ascending
        (d2, id), as (ids, d2), (n, k) each, row = vertex id."""
        ids = np.zeros((self.num_vertices, max(int(k), 0)), np.int32)
        d2 = np.zeros(ids.shape, np.float32)
        _check(self.lib.avr_graph_index_knn(self.h, int(k), ids.ctypes.data_as(c_int_p), _fp(d2)))
        return ids, d2

    def search_ranges(self, k):
        """ComputeSearchRanges on the host: renderSearchRange per vertex id."""
        out = np.zeros(self.num_vertices, np.float32)
        _check(self.lib.avr_graph_index_search_ranges(self.h, int(k), _fp(out)))
        return out

    def close(self):
        if self.h:
            self.lib.avr_graph_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GraphUniform:
    """The uniform (voxel) lighting graph (avr_graph_uniform_*): vertices on the integer lattice
    of `spacing`, one lightScalar each, behind one hash table. GraphUniform(coors, light_scalar,
    spacing) takes (m, 3) integer coordinates; GraphUniform.from_points converts free-graph
    vertices. Host code; Context.graph_render_uniform, graph_uniform_lookup and
    graph_uniform_trace upload the table to the device on first use."""

    def __init__(self, coors, light_scalar, spacing):
        self.lib = load()
        self.h = None
        c = np.asarray(coors)
        if c.dtype.kind not in "iu":
            raise ValueError("GraphUniform: integer lattice coordinates (GraphUniform.from_points takes points)")
        c64 = c.reshape(-1, 3).astype(np.int64)
        c = np.ascontiguousarray(np.clip(c64, -2 ** 31, 2 ** 31 - 1), np.int32)   # out of range either way
        light = np.ascontiguousarray(light_scalar, np.float32).reshape(-1)
        if len(light) != len(c):
            raise ValueError("GraphUniform: one light scalar per vertex")
        h = ctypes.c_void_p()
        _check(self.lib.avr_graph_uniform_create(len(c), c.ctypes.data_as(c_int_p), _fp(light), float(spacing),
                                                 ctypes.byref(h)))
        self._adopt(h)

    def _adopt(self, h):
        self.h = h
        n, s = ctypes.c_longlong(), ctypes.c_float()
        _check(self.lib.avr_graph_uniform_size(h, ctypes.byref(n), ctypes.byref(s)))
        self.num_vertices = n.value
        self.spacing = np.float32(s.value)
        self.coors = np.zeros((n.value, 3), np.int32)
        self.light_scalar = np.zeros(n.value, np.float32)
        _check(self.lib.avr_graph_uniform_get(h, self.coors.ctypes.data_as(c_int_p), _fp(self.light_scalar)))

    @classmethod
    def from_points(cls, points, light_scalar, spacing, reduce="first"):
        """FreeGraph::ToUniform's vertices: the points in ascending id, one new vertex per voxel
        at its first appearance; reduce "first" keeps that point's light, "mean" the float mean
        of the voxel's lights. The old -> new id map is left in .vertex_of."""
        if reduce not in ("first", "mean"):
            raise ValueError('GraphUniform.from_points: reduce is "first" or "mean"')
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        light = np.ascontiguousarray(light_scalar, np.float32).reshape(-1)
        if len(light) != len(p):
            raise ValueError("GraphUniform: one light scalar per vertex")
        self = cls.__new__(cls)
        self.lib = load()
        self.h = None
        vertex_of = np.zeros(len(p), np.int32)
        h = ctypes.c_void_p()
        _check(self.lib.avr_graph_uniform_from_points(len(p), _fp(p), _fp(light), float(spacing),
                                                      1 if reduce == "mean" else 0, vertex_of.ctypes.data_as(c_int_p),
                                                      ctypes.byref(h)))
        self._adopt(h)
        self.vertex_of = vertex_of
        return self

    @classmethod
    def from_points_device(cls, ctx, points, spacing):
        """from_points(points, zeros, spacing) with the voxel set built on the device
        (avr_graph_uniform_from_points_device): bitwise the same coordinates, ids and vertex_of."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        self = cls.__new__(cls)
        self.lib = load()
        self.h = None
        vertex_of = np.zeros(len(p), np.int32)
        h = ctypes.c_void_p()
        _check(self.lib.avr_graph_uniform_from_points_device(ctx.h if ctx is not None else None, len(p), _fp(p),
                                                             float(spacing), ctypes.byref(h),
                                                             vertex_of.ctypes.data_as(c_int_p)))
        self._adopt(h)
        self.vertex_of = vertex_of
        return self

    @property
    def points(self):
        """The vertices' points, (float)coors * spacing (graph.cpp:555)."""
        return (self.coors.astype(np.float32) * self.spacing).astype(np.float32)

    def lookup(self, points):
        """UniformGraph::GetVertexConst on the host for (n, 3) graph-space points: (ids, light);
        id -1 and light 0 without a vertex."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        ids = np.zeros(len(p), np.int32)
        light = np.zeros(len(p), np.float32)
        _check(self.lib.avr_graph_uniform_lookup(self.h, len(p), _fp(p), ids.ctypes.data_as(c_int_p), _fp(light)))
        return ids, light

    def trace(self, o, d):
        """The lit voxel each graph-space ray enters first, on the host: (ids, hit0, hit1) of
        IntersectP for its box; id -1 without one."""
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        if len(o) != len(d):
            raise ValueError("GraphUniform.trace: one direction per origin")
        ids = np.zeros(len(o), np.int32)
        hit0, hit1 = np.zeros(len(o), np.float32), np.zeros(len(o), np.float32)
        _check(self.lib.avr_graph_uniform_trace(self.h, len(o), _fp(o), _fp(d), ids.ctypes.data_as(c_int_p), _fp(hit0),
                                                _fp(hit1)))
        return ids, hit0, hit1

    def close(self):
        if self.h:
            self.lib.avr_graph_uniform_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


VOXEL_VERTEX, VOXEL_OUTSIDE, VOXEL_CAST, VOXEL_SINGLE, VOXEL_FILLED = 1, 2, 4, 8, 16
VOXEL_FILL_START = {None: -1, "lowest": -1, "all": -2}


class GraphVoxels:
    """The voxel boundary's flood state (avr_graph_voxels_*): one byte per cell of the dense
    lattice over FitBounds(pmin, pmax, spacing), x fastest; bits VOXEL_VERTEX, _OUTSIDE, _CAST,
    _SINGLE, _FILLED. single_layer / fill take a Context for the device, None for the host: the
    two leave the same bytes."""

    def __init__(self, pmin, pmax, spacing, coors):
        self.lib = load()
        self.h = None
        lo = np.ascontiguousarray(pmin, np.float32).reshape(3)
        hi = np.ascontiguousarray(pmax, np.float32).reshape(3)
        c = np.asarray(coors)
        if c.dtype.kind not in "iu":
            raise ValueError("GraphVoxels: integer lattice coordinates")
        c = np.ascontiguousarray(np.clip(c.reshape(-1, 3).astype(np.int64), -2 ** 31, 2 ** 31 - 1), np.int32)
        h = ctypes.c_void_p()
        _check(self.lib.avr_graph_voxels_create(_fp(lo), _fp(hi), float(spacing), len(c), c.ctypes.data_as(c_int_p),
                                                ctypes.byref(h)))
        self.h = h
        self.coors = c
        self.spacing = np.float32(spacing)
        self.lo, self.n = np.zeros(3, np.int32), np.zeros(3, np.int32)
        _check(self.lib.avr_graph_voxels_state(h, self.lo.ctypes.data_as(c_int_p), self.n.ctypes.data_as(c_int_p), None, 0))
        self.cells = int(np.prod(self.n.astype(np.int64)))

    def single_layer(self, ctx=None):
        """ToSingleLayerAndSaveCast; returns the number of levels the flood ran."""
        lv = ctypes.c_int(0)
        _check(self.lib.avr_graph_voxels_single_layer(ctx.h if ctx is not None else None, self.h, ctypes.byref(lv)))
        return lv.value

    def fill(self, ctx=None, start=None):
        """FillInside from the single-layer vertex `start` (an index into this state's
        vertices), None / "lowest" or "all"; returns the number of levels."""
        s = VOXEL_FILL_START[start] if start in VOXEL_FILL_START else start
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or s < -2:
            raise ValueError('fill start: a single-layer vertex id, None / "lowest" or "all"')
        lv = ctypes.c_int(0)
        _check(self.lib.avr_graph_voxels_fill(ctx.h if ctx is not None else None, self.h, int(s), ctypes.byref(lv)))
        return lv.value

    def state(self):
        """The state bytes, shaped (nz, ny, nx)."""
        s = np.zeros(self.cells, np.uint8)
        _check(self.lib.avr_graph_voxels_state(self.h, None, None, s.ctypes.data_as(ctypes.c_void_p), len(s)))
        return s.reshape(int(self.n[2]), int(self.n[1]), int(self.n[0]))

    def counts(self):
        """(visited, cast, single layer, filled) cell counts."""
        v = [ctypes.c_longlong(0) for _ in range(4)]
        _check(self.lib.avr_graph_voxels_visited(self.h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def cells_with(self, bit):
        """Lattice coordinates (k, 3) of the cells with `bit`, in ascending (z, y, x)."""
        z, y, x = np.nonzero(self.state() & bit)
        return (np.stack([x, y, z], axis=1).astype(np.int32) + self.lo).astype(np.int32)

    def vertex_bits(self):
        """The state byte of each vertex's cell, in vertex order."""
        s = self.state()
        c = self.coors - self.lo
        return s[c[:, 2], c[:, 1], c[:, 0]]

    def close(self):
        if self.h:
            self.lib.avr_graph_voxels_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def film_reduce_rccl(contexts, root=0):
    """avr_film_reduce_rccl: SUM the films of `contexts` (one per GPU) into contexts[root]."""
    lib = load()
    arr = (ctypes.c_void_p * len(contexts))(*[c.h.value if hasattr(c.h, "value") else c.h for c in contexts])
    _check(lib.avr_film_reduce_rccl(arr, len(contexts), int(root)))
