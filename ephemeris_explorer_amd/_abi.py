"""The C ABI of include/ephemeris_amd.h as ctypes sees it: the structures, ONE table of signatures and the loader.

SIGNATURES is the only place a function's restype / argtypes are written; _lib() applies it in a loop, ABI_SYMBOLS is its
key list, and tests/test_abi.py holds both against the header (names, argument counts, pointer / scalar kinds, widths)."""
import ctypes as C
import os
from pathlib import Path

# (the evaluation order of the point-mass term is a run-time choice now: set_pair_variant(k) / EPH_PAIR_VARIANT=k)
LIB_PATH = Path(__file__).resolve().parent / "libephemeris_amd.so"
if os.environ.get("EPH_AMD_LIBRARY"):             # tuning builds (scripts/): another build of the same sources
    LIB_PATH = Path(os.environ["EPH_AMD_LIBRARY"])

EXCHANGE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_void_p)

_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_u32p = C.POINTER(C.c_uint32)
_i32p = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)
_i64p = C.POINTER(C.c_int64)
_u64p = C.POINTER(C.c_uint64)
_vpp = C.POINTER(C.c_void_p)      # eph_* **out: where a creating call leaves the new handle


class PlotView(C.Structure):
    """eph_plot_view: camera position, the floating-origin grid's affine map and the simulation time."""
    _fields_ = [("camera_position", C.c_double * 3), ("grid_matrix3", C.c_double * 9), ("grid_translation", C.c_double * 3),
                ("cell_offset", C.c_double * 3), ("current", C.c_double)]


class PlotRequest(C.Structure):
    """eph_plot_request = PlotConfig + PlotSource (ephemeris_explorer/src/ui/world/plot.rs:15-83)."""
    _fields_ = [("source_body", C.c_int32), ("reference_body", C.c_int32), ("knot_first", C.c_int64),
                ("knot_count", C.c_int64), ("start", C.c_double), ("end", C.c_double), ("bound", C.c_int32),
                ("enabled", C.c_int32), ("tan2_angular_resolution", C.c_double), ("max_points", C.c_int64)]


class OrbitPlotConfig(C.Structure):
    """eph_orbit_plot_config = OrbitPlotConfig (ephemeris_explorer/src/analysis.rs:132-142) without its colour."""
    _fields_ = [("start", C.c_double), ("end", C.c_double), ("bound", C.c_int32), ("enabled", C.c_int32),
                ("tan2_angular_resolution", C.c_double), ("max_points_per_segment", C.c_int64), ("reference_body", C.c_int32)]


class PlotSegment(C.Structure):
    """eph_plot_segment: one plot setup_segment_plotting spawns (analysis.rs:229-292)."""
    _fields_ = [("plot", C.c_int64), ("transition", C.c_int32), ("timeline_segment", C.c_int32), ("soi_body", C.c_int32),
                ("reference_body", C.c_int32), ("kind", C.c_int32), ("is_burn", C.c_int32), ("overlapping", C.c_int32),
                ("start", C.c_double), ("end", C.c_double)]


class MarkerRequest(C.Structure):
    """eph_marker_request: one plot whose event markers are asked for (PlotSource.reference + PlotPoints::contains)."""
    _fields_ = [("reference_body", C.c_int32), ("kinds", C.c_int32), ("first", C.c_double), ("last", C.c_double)]


class PlotMarker(C.Structure):
    """eph_plot_marker: one marker of a plot (ephemeris_explorer/src/ui/world/tooltip.rs:84-245)."""
    _fields_ = [("request", C.c_int64), ("kind", C.c_int32), ("index", C.c_int32), ("body", C.c_int32), ("status", C.c_int32),
                ("time", C.c_double), ("position", C.c_double * 3), ("distance", C.c_double), ("apsis_distance", C.c_double),
                ("frame", C.c_double * 9)]


class SeparationRequest(C.Structure):
    """eph_separation_request: one closest-separation search of target plotting (ephemeris_explorer/src/analysis.rs:344-348)."""
    _fields_ = [("source_body", C.c_int32), ("target_body", C.c_int32), ("source_knot_first", C.c_int64),
                ("source_knot_count", C.c_int64), ("target_knot_first", C.c_int64), ("target_knot_count", C.c_int64),
                ("left", C.c_double), ("right", C.c_double), ("precision", C.c_double), ("max_iterations", C.c_int64),
                ("metric", C.c_int32)]


class AdaptiveParams(C.Structure):
    """eph_adaptive_params = integration::AdaptiveMethodParams; defaults = the app's INITIAL_ADAPTIVE_PARAMS
    (ephemeris_explorer/src/load/mod.rs:472-486)."""
    _fields_ = [("h_init", C.c_double), ("h_max", C.c_double), ("tol_position", C.c_double),
                ("tol_velocity", C.c_double), ("fac_min", C.c_double), ("fac_max", C.c_double), ("fac", C.c_double),
                ("n_max", C.c_uint32)]

    @classmethod
    def default(cls, tolerance=1e-3):
        return cls(60.0, 1.7976931348623157e308, tolerance, tolerance, 1.0 / 5.0, 5.0 / 1.0, 9.0 / 10.0, 1_000_000)


def _signatures():
    vp, i32, i64, u32, u64, f64, text = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_double, C.c_char_p
    view, plots, searches, params = C.POINTER(PlotView), C.POINTER(PlotRequest), C.POINTER(SeparationRequest), C.POINTER(AdaptiveParams)
    configs, segments = C.POINTER(OrbitPlotConfig), C.POINTER(PlotSegment)
    marker_requests, markers = C.POINTER(MarkerRequest), C.POINTER(PlotMarker)
    knots = [i64, _dp, _dp, _dp]                                  # a (count, t, pos, vel) knot triple
    separation_out = [_u8p, _dp, _dp, _i32p, _i32p, _dp]          # found, time, distance, iterations, status, failed_at
    plot_out = [i64, _dp, _fp, _i64p, _i32p, _dp]                 # capacity, t, xyz, count, status, failed_at
    burns = [_dp, _dp, _dp, _i32p]                                # start, end, acceleration, reference body
    # name: (restype, argtypes) for every function include/ephemeris_amd.h declares, in the header's order of topics
    return {
        "eph_abi_version": (i32, []),
        "eph_pair_variant": (i32, []),
        "eph_set_pair_variant": (i32, [i32]),
        "eph_release_cached_memory": (i32, [_u64p]),
        "eph_status_string": (text, [i32]),
        "eph_last_error": (text, []),
        "eph_device_count": (i32, [_i32p]),
        "eph_set_device": (i32, [i32]),
        "eph_device_name": (i32, [text, i32]),
        "eph_srkn_coeffs": (i32, [text, _i32p, _i32p, _dp, _dp]),
        "eph_elm2_coeffs": (i32, [text, _i32p, _dp, _dp, _dp, _dp, _dp]),
        "eph_accel_eval": (i32, [i32, _dp, _dp, _dp]),
        "eph_least_squares_fit": (i32, [i32, i32, i64, _dp, _dp, _i32p]),
        # NBodyIntegration
        "eph_nbody_create": (i32, [i32, _dp, _dp, _dp, f64, f64, text, _vpp]),
        "eph_nbody_advance": (i32, [vp, i64]),
        "eph_nbody_advance_many": (i32, [_vpp, i32, i64]),
        "eph_nbody_get_state": (i32, [vp, _dp, _dp, _dp, _u32p]),
        "eph_nbody_get_acc": (i32, [vp, _dp]),
        "eph_nbody_set_bound": (i32, [vp, f64]),
        "eph_nbody_clone": (i32, [vp, _vpp]),
        "eph_nbody_destroy": (None, [vp]),
        "eph_nbody_eval_count": (i32, [vp, _u64p]),
        "eph_nbody_set_path": (i32, [vp, i32]),
        "eph_nbody_kernel_time": (i32, [vp, _dp, _u64p]),
        "eph_nbody_enable_timing": (i32, [vp, i32]),
        "eph_nbody_sync": (i32, [vp]),
        # sharding and its transports
        "eph_rccl_unique_id": (i32, [vp]),
        "eph_nbody_shard": (i32, [vp, i32, i32, vp, EXCHANGE_FN, vp]),
        "eph_nbody_shard_info": (i32, [vp, _i32p, _i32p, _u64p]),
        "eph_prop_shard": (i32, [vp, i32, i32, vp, EXCHANGE_FN, vp]),
        "eph_peer_create": (i32, [i32, i32, u64, _vpp]),
        "eph_peer_create_ex": (i32, [i32, i32, u64, i32, _vpp]),
        "eph_peer_memory_form": (i32, [vp, _i32p]),
        "eph_peer_handle": (i32, [vp, vp]),
        "eph_peer_connect": (i32, [vp, vp]),
        "eph_peer_destroy": (i32, [vp]),
        "eph_nbody_shard_peer": (i32, [vp, vp]),
        "eph_prop_shard_peer": (i32, [vp, vp]),
        # NBodyPropagator
        "eph_prop_create": (i32, [i32, _dp, _dp, _dp, f64, f64, i32, text, _u32p, _u32p, _vpp]),
        "eph_prop_step": (i32, [vp]),
        "eph_prop_step_n": (i32, [vp, i64]),
        "eph_prop_step_n_many": (i32, [_vpp, i32, i64]),
        "eph_prop_step_to": (i32, [vp, f64]),
        "eph_prop_time": (i32, [vp, _dp]),
        "eph_prop_has_reached": (i32, [vp, f64, _i32p]),
        "eph_prop_integrator_time": (i32, [vp, _dp]),
        "eph_prop_get_state": (i32, [vp, _dp, _dp, _dp, _u32p]),
        "eph_prop_take_solution": (i32, [vp, _vpp]),
        "eph_prop_propagate": (i32, [vp, f64, _vpp]),
        "eph_prop_clone": (i32, [vp, _vpp]),
        "eph_prop_destroy": (None, [vp]),
        "eph_prop_integrator": (vp, [vp]),
        # Solution
        "eph_solution_bodies": (i32, [vp, _i32p]),
        "eph_solution_info": (i32, [vp, i32, _dp, _dp, _i64p]),
        "eph_solution_coeffs": (i32, [vp, i32, _dp, _i32p]),
        "eph_solution_eval": (i32, [vp, i32, i64, _dp, _dp, _dp, _u8p]),
        "eph_solution_append": (i32, [vp, vp, i32]),
        "eph_solution_create": (i32, [i32, _dp, _dp, _i64p, _dp, _i32p, _vpp]),
        "eph_solution_clear": (i32, [vp, i32, f64, i32]),
        "eph_solution_between": (i32, [vp, f64, f64, _vpp]),
        "eph_solution_destroy": (None, [vp]),
        # Ephemeris
        "eph_ephemeris_create": (i32, [vp, _dp, _vpp]),
        "eph_ephemeris_destroy": (None, [vp]),
        "eph_ephemeris_append": (i32, [vp, vp, i32]),
        "eph_ephemeris_merge": (i32, [vp, vp, i32]),
        "eph_ephemeris_clear": (i32, [vp, i32, f64, i32]),
        "eph_ephemeris_info": (i32, [vp, i32, _dp, _dp, _i64p, _u64p]),
        "eph_ephemeris_is_valid_at": (i32, [vp, f64, _i32p]),
        "eph_ephemeris_export": (i32, [vp, vp, u64, _u64p]),
        "eph_ephemeris_import": (i32, [vp, u64, _vpp]),
        "eph_ephemeris_interpolation_errors": (i32, [vp, vp, i64, _dp, _i64p]),
        # SpacecraftBatch
        "eph_craft_batch_create": (i32, [vp, i64, _dp, _dp, _dp, text, params, _i64p, *burns, i32, _vpp]),
        "eph_craft_batch_set_body_order": (i32, [vp, _i32p]),
        "eph_craft_batch_propagate": (i32, [vp, f64]),
        "eph_craft_batch_step_n": (i32, [vp, u32]),
        "eph_craft_batch_retry_failed": (i32, [vp]),
        "eph_craft_batch_status": (i32, [vp, _i32p, _i32p, _u32p, _u32p]),
        "eph_craft_batch_state": (i32, [vp, _dp, _dp, _dp, _dp]),
        "eph_craft_batch_summary": (i32, [vp, vp]),
        "eph_craft_batch_knots": (i32, [vp, i64, _dp, _dp, _dp]),
        "eph_craft_batch_kernel_time": (i32, [vp, _dp]),
        "eph_craft_batch_clone": (i32, [vp, _vpp]),
        "eph_craft_batch_gather": (i32, [i32, _vpp, i64, _i32p, _i64p, _vpp]),
        "eph_craft_batch_knot_slabs": (i32, [vp, i32, i32, _dp, _dp]),
        "eph_craft_batch_eval": (i32, [vp, i64, _dp, i32, i32, _dp, _u8p]),
        "eph_craft_batch_plot_points": (i32, [vp, view, i64, plots, _i64p, *plot_out]),
        "eph_craft_batch_plot_segments": (i32, [vp, i64, configs, _i64p, _i32p, i64, segments, _i64p, view, *plot_out]),
        "eph_craft_batch_plot_markers": (i32, [vp, i64, marker_requests, _i64p, i64, markers, _i64p]),
        "eph_craft_batch_closest_separation": (i32, [vp, i64, searches, _i64p, _i64p, *separation_out]),
        "eph_craft_batch_restart": (i32, [vp, _u8p, _i64p, *burns, _dp, params, _dp, _i32p]),
        "eph_craft_batch_reset_knots": (i32, [vp]),
        "eph_craft_batch_reset_events": (i32, [vp]),
        "eph_craft_batch_enable_events": (i32, [vp, _dp, i32, i32]),
        "eph_craft_batch_event_counts": (i32, [vp, _i32p, _i32p, _i32p]),
        "eph_craft_batch_events": (i32, [vp, i64, _dp, _i32p, _dp, _dp, _i32p, _i32p]),
        "eph_craft_batch_destroy": (None, [vp]),
        # knot arrays on the host side of the boundary
        "eph_timeline_divergence_time": (i32, [i64, *burns, i64, *burns, f64, _dp]),
        "eph_hermite_eval": (i32, [*knots, i64, _dp, _dp, _dp, _u8p]),
        "eph_hermite_join": (i32, [*knots, *knots, *knots, _i64p]),
        "eph_transitions_join": (i32, [i64, _dp, _i32p, i64, _dp, _i32p, f64, i64, _dp, _i32p, _i64p]),
        "eph_apsides_join": (i32, [i64, _dp, _dp, _i32p, _i32p, i64, _dp, _dp, _i32p, _i32p, f64, i64, _dp, _dp, _i32p, _i32p, _i64p]),
        "eph_plot_points": (i32, [vp, view, i64, plots, *knots, *plot_out]),
        "eph_closest_separation": (i32, [vp, i64, searches, *knots, *separation_out]),
    }


SIGNATURES = _signatures()
ABI_SYMBOLS = list(SIGNATURES)    # every symbol include/ephemeris_amd.h declares (tests check the .so exports exactly these)
_L = None


def _lib():
    """Loads libephemeris_amd.so; raises if it has not been built (no fallback of any kind)."""
    global _L
    if _L is not None:
        return _L
    if not LIB_PATH.exists():
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc, gfx950). ephemeris_explorer_amd has no CPU fallback.")
    L = C.CDLL(str(LIB_PATH))
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if L.eph_abi_version() != 3:
        raise ImportError("libephemeris_amd.so ABI version mismatch")
    _L = L
    return L


def hip_runtime():
    """The HIP runtime libephemeris_amd.so is bound to IN THIS PROCESS, as a ctypes object with hipMemcpy and
    hipStreamSynchronize: symbols looked up through the library's own handle (dlsym searches its dependencies), not through
    whatever "libamdhip64.so" resolves to -- a process that also imported PyTorch may carry a second, bundled runtime, and
    device pointers / streams of one mean nothing to the other. For host programs (and tests) that touch the library's device
    buffers themselves, e.g. inside an eph_exchange_fn."""
    lib = _lib()
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    lib.hipMemcpy.restype = C.c_int
    lib.hipStreamSynchronize.argtypes = [C.c_void_p]
    lib.hipStreamSynchronize.restype = C.c_int
    return lib
