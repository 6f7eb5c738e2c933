"""nbody_llm_amd -- ctypes binding of libnbody_hip.so (include/nbody_hip.h) and a thin host-side
mirror of the reference's `Simulation` trait (src/shared.rs:80-97) for tests and bench.py.

The directory is named `nbody-llm_amd`; load it under the module name `nbody_llm_amd` with
`__graft_entry__.load_package()` (a hyphen cannot be imported directly).

There is NO fallback: if libnbody_hip.so is missing this module raises at import, and without a
HIP device `Simulation(...)` raises NbodyError(NBODY_ERR_NO_DEVICE).  Nothing here touches
oracle/.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# NBODY_HIP_LIBRARY: another build of the same ABI -- libnbody_hip_tuning.so carries the experimental walks and the
# in-kernel stamps the release library leaves out (make -C nbody-llm_amd/csrc tuning; __graft_entry__.load_package(tuning=True))
LIB_PATH = os.environ.get("NBODY_HIP_LIBRARY") or os.path.join(_HERE, "libnbody_hip.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build it with `make -C nbody-llm_amd/csrc` (or __graft_entry__.build()); "
        "there is no Python/CPU fallback for the HIP engine"
    )

lib = C.CDLL(LIB_PATH, mode=C.RTLD_LOCAL)   # (two builds of the library may live in one process: nothing is resolved across them)

# ---- constants (include/nbody_hip.h) ----------------------------------------------------------
NBODY_OK = 0
NBODY_ERR_INVALID = -1
NBODY_ERR_HIP = -2
NBODY_ERR_CAPACITY = -3
NBODY_ERR_TREE_DEPTH = -4
NBODY_ERR_COMM = -5
NBODY_ERR_NO_DEVICE = -6
BRUTE_FORCE, BARNES_HUT = 0, 1
STRICT, FAST = 0, 1
LEAF_REFERENCE = 0   # src/manual: a leaf failing the opening test contributes nothing
LEAF_DIRECT = 1      # the src/llm walk on the same tree: such a leaf is evaluated directly
TREE_HOST, TREE_DEVICE, TREE_AUTO = 0, 1, 2   # AUTO: fast math -> device build, strict -> host build
COMM_ID_BYTES = 128

#: PointParticle<f32,3>, #[repr(C)] (src/shared.rs:151-158)
PARTICLE_DTYPE = np.dtype(
    [("position", "<f4", 3), ("velocity", "<f4", 3), ("acceleration", "<f4", 3), ("mass", "<f4")]
)
assert PARTICLE_DTYPE.itemsize == 40
#: PointParticle<f64,3> (the instantiation the reference's own driver uses, src/main.rs:52-105): NBODY_F64 handles
PARTICLE_DTYPE64 = np.dtype(
    [("position", "<f8", 3), ("velocity", "<f8", 3), ("acceleration", "<f8", 3), ("mass", "<f8")]
)
assert PARTICLE_DTYPE64.itemsize == 80
F32, F64 = 0, 1
POTENTIAL_PAIRS, POTENTIAL_TREE = 0, 1   # nbody_potentials / nbody_energy_world: the exact pair sum | the monopole sum over the tree
POTENTIAL_TREE_QUADRUPOLE = 2            # ... | POTENTIAL_TREE with the quadrupole term of every accepted internal cell
MULTIPOLE_MONOPOLE, MULTIPOLE_QUADRUPOLE = 1, 2   # nbody_set_multipole: order of the Barnes-Hut force walk's expansion
LEAPFROG, HERMITE4 = 0, 1   # nbody_set_integrator: the reference's leapfrog | fourth-order Hermite (f64 brute force, one rank)
SHARD_INDEX, SHARD_SPATIAL = 0, 1   # index blocks + all-gather | Morton-key ranges + halo exchange (Barnes-Hut, fast math)
EXTERNAL_MAX = 8   # nbody_set_external_field: components of a static external field, and their kinds
EXT_PLUMMER, EXT_HERNQUIST, EXT_MIYAMOTO_NAGAI, EXT_LOGARITHMIC = 0, 1, 2, 3
SEARCH_ALL_PAIRS, SEARCH_CELLS = 0, 1   # nbody_set_pair_search: how the fixed-radius calls (fof_*, contacts, neighbors_within, density*, pair_counts) find their pairs
KERNEL_TOP_HAT, KERNEL_CUBIC_SPLINE = 0, 1   # nbody_density / nbody_density_center: the mass in the sphere over its volume | the M4 spline
KNN_MAX_K = 32   # nbody_knn, nbody_knn_density, nbody_knn_density_center: the largest k (NBODY_KNN_MAX_K)
PAIR_COUNT_MAX_BINS = 1024   # nbody_pair_counts / nbody_pair_counts_at: the most bins of one call (NBODY_PAIR_COUNT_MAX_BINS)
DEPOSIT_NGP, DEPOSIT_CIC, DEPOSIT_TSC = 0, 1, 2   # nbody_deposit: the assignment scheme (1, 2 or 3 cells an axis)
# nbody_deposit: the quantity q of a body: m | m vx | m vy | m vz | m ((vx vx + vy vy) + vz vz) | 1.0
DEPOSIT_MASS, DEPOSIT_MOMENTUM_X, DEPOSIT_MOMENTUM_Y, DEPOSIT_MOMENTUM_Z, DEPOSIT_MV2, DEPOSIT_NUMBER = 0, 1, 2, 3, 4, 5
DEPOSIT_MAX_CELLS = 1 << 27   # nbody_deposit: the most cells of a grid (NBODY_DEPOSIT_MAX_CELLS)
# nbody_grid_sample: the grid's value [n][fields] | its gradient by central differences of order 2 | of order 4 [n][3]
SAMPLE_VALUE, SAMPLE_GRADIENT2, SAMPLE_GRADIENT4 = 0, 1, 2
SAMPLE_MAX_FIELDS = 4   # nbody_grid_sample: the most fields of a grid (NBODY_SAMPLE_MAX_FIELDS)
# nbody_grid_poisson, periodic: -k^2 of the continuous Laplacian | the 7-point Laplacian, the mate of SAMPLE_GRADIENT2
POISSON_SPECTRAL, POISSON_DIFF2 = 0, 1
POISSON_MAX_AXIS = 4096        # nbody_grid_poisson: the longest transform length of an axis, after padding (NBODY_POISSON_MAX_AXIS)
POISSON_MAX_POINTS = 1 << 27   # nbody_grid_poisson: the most complex points, after padding (NBODY_POISSON_MAX_POINTS)

#: every symbol include/nbody_hip.h declares (tests check the library exports all of them)
DECLARED_SYMBOLS = [
    "nbody_tracers_upload", "nbody_tracers_download", "nbody_tracers_count", "nbody_tracer_stats", "nbody_host_tracer_plan",
    "nbody_create", "nbody_destroy", "nbody_clone", "nbody_upload", "nbody_download", "nbody_count",
    "nbody_count_global", "nbody_add_point", "nbody_remove_point", "nbody_set_settings", "nbody_get_settings",
    "nbody_set_bounds", "nbody_init", "nbody_step_by", "nbody_steps", "nbody_update_forces", "nbody_elapsed",
    "nbody_sync", "nbody_set_profiling", "nbody_stats", "nbody_reset_stats", "nbody_energy", "nbody_tree_export",
    "nbody_last_error", "nbody_comm_unique_id", "nbody_comm_init", "nbody_local_range", "nbody_ic_plummer",
    "nbody_ic_disc", "nbody_host_build_tree", "nbody_abi_version", "nbody_device_count",
    "nbody_debug_step_begin", "nbody_debug_import_segment", "nbody_debug_step_forces",
    "nbody_debug_import_partials", "nbody_debug_step_end", "nbody_host_cross_plan",
    "nbody_set_settings_f64", "nbody_get_settings_f64", "nbody_set_bounds_f64", "nbody_step_by_f64", "nbody_elapsed_f64",
    "nbody_tree_export_f64", "nbody_ic_plummer_f64", "nbody_ic_disc_f64",
    "nbody_download_ids", "nbody_let_stats", "nbody_debug_let_phase", "nbody_debug_let_exchange", "nbody_debug_let_set_prune",
    "nbody_debug_let_bounds", "nbody_debug_let_set_balance", "nbody_debug_let_export_held",
    "nbody_comm_local_id", "nbody_comm_transport", "nbody_host_exchange_layout",
    "nbody_set_tuning", "nbody_get_tuning", "nbody_is_tuning_build", "nbody_tree_export_cells", "nbody_host_launch_plan",
    "nbody_get_config", "nbody_potentials", "nbody_energy_world", "nbody_field_at", "nbody_tidal_at",
    "nbody_set_multipole", "nbody_get_multipole", "nbody_tree_export_quadrupoles",
    "nbody_set_integrator", "nbody_get_integrator", "nbody_download_jerk", "nbody_suggest_dt",
    "nbody_set_block_steps", "nbody_get_block_steps", "nbody_download_levels", "nbody_block_step_counts",
    "nbody_debug_hermite_forces_of",
    "nbody_set_external_field", "nbody_get_external_field", "nbody_external_potentials", "nbody_external_energy",
    "nbody_external_at", "nbody_host_external_eval",
    "nbody_moments", "nbody_lagrangian_radii",
    "nbody_partners", "nbody_bound_pairs",
    "nbody_nearest", "nbody_contacts", "nbody_merge_contacts",
    "nbody_fof_labels", "nbody_fof_groups", "nbody_fof_bound_groups",
    "nbody_neighbors_within", "nbody_density", "nbody_density_center",
    "nbody_knn", "nbody_knn_density", "nbody_knn_density_center",
    "nbody_pair_counts", "nbody_pair_counts_at",
    "nbody_deposit", "nbody_host_deposit", "nbody_deposit_stats",
    "nbody_grid_sample", "nbody_grid_sample_at", "nbody_host_grid_sample", "nbody_grid_sample_stats",
    "nbody_grid_poisson", "nbody_host_grid_poisson", "nbody_host_poisson_twiddles", "nbody_grid_poisson_stats",
    "nbody_pm_field", "nbody_pm_field_at", "nbody_host_pm_field", "nbody_pm_field_stats",
    "nbody_p3m_field", "nbody_p3m_field_at", "nbody_host_p3m_field", "nbody_host_p3m_table", "nbody_p3m_field_stats",
    "nbody_set_mesh_gravity", "nbody_get_mesh_gravity", "nbody_mesh_gravity_stats",
    "nbody_set_pair_search", "nbody_get_pair_search", "nbody_pair_search_stats", "nbody_host_cell_grid",
]


class NbodyConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("method", C.c_int32), ("math_mode", C.c_int32), ("leaf_mode", C.c_int32),
        ("device", C.c_int32), ("rank", C.c_int32), ("world_size", C.c_int32), ("host_threads", C.c_int32),
        ("capacity", C.c_uint64), ("tree_build", C.c_int32), ("dtype", C.c_int32), ("shard_mode", C.c_int32), ("reserved", C.c_int32),
    ]


class NbodyLetStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("steps", "bodies_migrated", "nodes_local", "nodes_global", "nodes_sent", "nodes_received",
                                          "bytes_sent", "bytes_allgather_equivalent")] + [("phase_ms", C.c_double * 5)] + \
               [(k, C.c_uint64) for k in ("host_syncs", "migrant_respills", "node_array_peak_bytes", "node_array_bytes")]


class GridSpec(C.Structure):
    """NbodyGridSpec (include/nbody_hip.h, "grid deposit"): the grid, the scheme and the quantity of one nbody_deposit call."""
    _fields_ = [("origin", C.c_double * 3), ("spacing", C.c_double), ("dims", C.c_int32 * 3), ("scheme", C.c_int32), ("quantity", C.c_int32),
                ("periodic", C.c_int32), ("project_axis", C.c_int32), ("reserved", C.c_int32)]


def grid_spec(origin, spacing, dims, scheme=DEPOSIT_CIC, quantity=DEPOSIT_MASS, periodic=False, project_axis=-1) -> GridSpec:
    """A GridSpec from plain values (origin [3], dims [3])."""
    o = [float(v) for v in origin]
    d = [int(v) for v in dims]
    return GridSpec((C.c_double * 3)(*o), float(spacing), (C.c_int32 * 3)(*d), int(scheme), int(quantity), int(bool(periodic)), int(project_axis), 0)


class NbodyPoissonSpec(C.Structure):
    """NbodyPoissonSpec (include/nbody_hip.h, "grid Poisson"): the constants of one nbody_grid_poisson call."""
    _fields_ = [("g", C.c_double), ("soften", C.c_double), ("green", C.c_int32), ("deconvolve", C.c_int32), ("reserved", C.c_int32 * 2)]


class NbodyPmSpec(C.Structure):
    """NbodyPmSpec (include/nbody_hip.h, "particle-mesh field"): the Poisson constants and the gradient of one nbody_pm_field call."""
    _fields_ = [("poisson", NbodyPoissonSpec), ("gradient", C.c_int32), ("reserved", C.c_int32 * 3)]


P3M_TABLE_INTERVALS = 4096
P3M_BOTH, P3M_MESH_ONLY, P3M_SHORT_ONLY = 0, 1, 2


class NbodyP3mSpec(C.Structure):
    """NbodyP3mSpec (include/nbody_hip.h, "P3M field"): the PM spec, the split scale, the cutoff, the softening and the terms."""
    _fields_ = [("pm", NbodyPmSpec), ("r_split", C.c_double), ("r_cut", C.c_double), ("soften", C.c_double), ("terms", C.c_int32),
                ("reserved", C.c_int32)]


class NbodyExternalComponent(C.Structure):
    """One component of a static external field: kind EXT_*, centre, p = the kind's parameters (include/nbody_hip.h)."""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("center", C.c_double * 3), ("p", C.c_double * 4)]


class BoundPair(C.Structure):
    """One mutual bound pair of nbody_bound_pairs (NbodyBoundPair, include/nbody_hip.h "binary census")."""
    _fields_ = [("i", C.c_int32), ("j", C.c_int32), ("energy", C.c_double), ("binding", C.c_double), ("semi_major", C.c_double),
                ("eccentricity", C.c_double), ("period", C.c_double), ("separation", C.c_double)]


#: the same record as a numpy dtype: what Simulation.bound_pairs() returns
BOUND_PAIR_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("energy", "<f8"), ("binding", "<f8"), ("semi_major", "<f8"),
                             ("eccentricity", "<f8"), ("period", "<f8"), ("separation", "<f8")])
assert BOUND_PAIR_DTYPE.itemsize == C.sizeof(BoundPair) == 56


class NbodyContact(C.Structure):
    """One mutual contact of nbody_contacts / nbody_merge_contacts (include/nbody_hip.h "sticky mergers")."""
    _fields_ = [("i", C.c_int32), ("j", C.c_int32), ("into", C.c_int32), ("reserved", C.c_int32), ("separation", C.c_double),
                ("mass", C.c_double), ("dkinetic", C.c_double)]


#: the same record as a numpy dtype: what Simulation.contacts() and Simulation.merge_contacts() return
CONTACT_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("into", "<i4"), ("reserved", "<i4"), ("separation", "<f8"), ("mass", "<f8"),
                          ("dkinetic", "<f8")])
assert CONTACT_DTYPE.itemsize == C.sizeof(NbodyContact) == 40


class NbodyGroup(C.Structure):
    """One listed group of nbody_fof_groups (include/nbody_hip.h "friends-of-friends groups")."""
    _fields_ = [("first", C.c_int32), ("count", C.c_int32), ("offset", C.c_int32), ("reserved", C.c_int32), ("mass", C.c_double),
                ("mx", C.c_double * 3), ("mv", C.c_double * 3)]


#: the same record as a numpy dtype: what Simulation.fof_groups() returns
GROUP_DTYPE = np.dtype([("first", "<i4"), ("count", "<i4"), ("offset", "<i4"), ("reserved", "<i4"), ("mass", "<f8"),
                        ("mx", "<f8", (3,)), ("mv", "<f8", (3,))])
assert GROUP_DTYPE.itemsize == C.sizeof(NbodyGroup) == 72


class NbodyBoundGroup(C.Structure):
    """One reported group of nbody_fof_bound_groups (include/nbody_hip.h "self-bound subsets of friends-of-friends groups")."""
    _fields_ = [("first", C.c_int32), ("fof_count", C.c_int32), ("count", C.c_int32), ("offset", C.c_int32),
                ("iterations", C.c_int32), ("converged", C.c_int32), ("mass", C.c_double), ("mx", C.c_double * 3),
                ("mv", C.c_double * 3), ("kinetic", C.c_double), ("potential", C.c_double)]


#: the same record as a numpy dtype: what Simulation.fof_bound_groups() returns
BOUND_GROUP_DTYPE = np.dtype([("first", "<i4"), ("fof_count", "<i4"), ("count", "<i4"), ("offset", "<i4"), ("iterations", "<i4"),
                              ("converged", "<i4"), ("mass", "<f8"), ("mx", "<f8", (3,)), ("mv", "<f8", (3,)), ("kinetic", "<f8"),
                              ("potential", "<f8")])
assert BOUND_GROUP_DTYPE.itemsize == C.sizeof(NbodyBoundGroup) == 96


class NbodyStats(C.Structure):
    _fields_ = [
        ("steps", C.c_uint64), ("interactions", C.c_uint64), ("node_visits", C.c_uint64), ("tree_nodes", C.c_uint64),
        ("force_launches", C.c_uint64), ("force_kernel_interactions", C.c_uint64), ("force_kernel_ms", C.c_double), ("tree_build_ms", C.c_double),
        ("tree_copy_ms", C.c_double), ("exchange_ms", C.c_double),
    ]


_H = C.c_void_p
_f, _sz, _i = C.c_float, C.c_size_t, C.c_int
_pf = C.POINTER(C.c_float)


def _sig(name, restype, *argtypes):
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = list(argtypes)
    return fn


_sig("nbody_create", _i, C.POINTER(NbodyConfig), C.POINTER(_H))
_sig("nbody_destroy", None, _H)
_sig("nbody_clone", _i, _H, C.POINTER(_H))
_sig("nbody_upload", _i, _H, C.c_void_p, _sz, _sz)
_sig("nbody_download", _i, _H, C.c_void_p, _sz, _sz, C.POINTER(_sz))
_sig("nbody_count", _i, _H, C.POINTER(_sz))
_sig("nbody_count_global", _i, _H, C.POINTER(_sz))
_sig("nbody_add_point", _i, _H, C.c_void_p)
_sig("nbody_remove_point", _i, _H, _sz)
_sig("nbody_set_settings", _i, _H, _f, _f, _f, _f)
_sig("nbody_get_settings", _i, _H, _pf, _pf, _pf, _pf)
_sig("nbody_set_bounds", _i, _H, _pf, _f)
_sig("nbody_init", _i, _H)
_sig("nbody_step_by", _i, _H, _f)
_sig("nbody_steps", _i, _H, _i)
_sig("nbody_update_forces", _i, _H)
_sig("nbody_elapsed", _i, _H, _pf)
_sig("nbody_sync", _i, _H)
_sig("nbody_set_profiling", _i, _H, _i)
_sig("nbody_stats", _i, _H, C.POINTER(NbodyStats))
_sig("nbody_reset_stats", _i, _H)
_sig("nbody_energy", _i, _H, C.POINTER(C.c_double), C.POINTER(C.c_double))
_sig("nbody_potentials", _i, _H, _i, C.c_void_p, _sz, C.POINTER(_sz), C.POINTER(C.c_uint64))
_sig("nbody_energy_world", _i, _H, _i, C.POINTER(C.c_double), C.POINTER(C.c_double))
_sig("nbody_field_at", _i, _H, _i, C.c_void_p, _sz, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64))
_sig("nbody_tidal_at", _i, _H, _i, C.c_void_p, _sz, C.c_void_p, C.POINTER(C.c_uint64))
_sig("nbody_tree_export", _i, _H, C.c_void_p, C.c_void_p, C.c_void_p, _sz, C.POINTER(_sz))
_sig("nbody_set_multipole", _i, _H, _i)
_sig("nbody_get_multipole", _i, _H, C.POINTER(_i))
_sig("nbody_tree_export_quadrupoles", _i, _H, C.c_void_p, _sz, C.POINTER(_sz))
_sig("nbody_set_integrator", _i, _H, _i)
_sig("nbody_get_integrator", _i, _H, C.POINTER(_i))
_sig("nbody_download_jerk", _i, _H, C.c_void_p, _sz, C.POINTER(_sz))
_sig("nbody_suggest_dt", _i, _H, C.c_double, C.POINTER(C.c_double))
_sig("nbody_set_block_steps", _i, _H, C.c_double, _i)
_sig("nbody_get_block_steps", _i, _H, C.POINTER(C.c_double), C.POINTER(_i))
_sig("nbody_download_levels", _i, _H, C.c_void_p, _sz, C.POINTER(_sz))
_sig("nbody_block_step_counts", _i, _H, C.POINTER(C.c_uint64))
_sig("nbody_debug_hermite_forces_of", _i, _H, C.c_void_p, _sz, C.c_void_p, C.c_void_p)
_sig("nbody_tree_export_cells", _i, _H, C.c_void_p, C.c_void_p, _sz, C.POINTER(_sz))
_sig("nbody_last_error", C.c_char_p, _H)
_sig("nbody_comm_unique_id", _i, C.c_void_p)
_sig("nbody_comm_init", _i, _H, C.c_void_p)
_sig("nbody_comm_local_id", _i, C.c_void_p)
_sig("nbody_comm_transport", _i, _H, C.c_char_p, _sz)
_sig("nbody_local_range", _i, _H, C.POINTER(_sz), C.POINTER(_sz))
_sig("nbody_ic_plummer", _i, C.c_void_p, _sz, _sz, C.c_uint64)
_sig("nbody_ic_disc", _i, C.c_void_p, _sz, _sz, C.c_uint64)
_sig("nbody_host_build_tree", _i, C.c_void_p, _sz, _pf, _f, _i, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, _sz, C.POINTER(_sz))
_sig("nbody_debug_step_begin", _i, _H, _f)
_sig("nbody_debug_import_segment", _i, _H, _H)
_sig("nbody_debug_step_forces", _i, _H, _f)
_sig("nbody_debug_import_partials", _i, _H, _H)
_sig("nbody_debug_step_end", _i, _H, _f)
_sig("nbody_host_cross_plan", _i, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.c_void_p, C.POINTER(_i),
     C.c_void_p)
_d = C.c_double
_pd = C.POINTER(C.c_double)
_sig("nbody_set_settings_f64", _i, _H, _d, _d, _d, _d)
_sig("nbody_get_settings_f64", _i, _H, _pd, _pd, _pd, _pd)
_sig("nbody_set_bounds_f64", _i, _H, _pd, _d)
_sig("nbody_step_by_f64", _i, _H, _d)
_sig("nbody_elapsed_f64", _i, _H, _pd)
_sig("nbody_tree_export_f64", _i, _H, C.c_void_p, C.c_void_p, C.c_void_p, _sz, C.POINTER(_sz))
_sig("nbody_ic_plummer_f64", _i, C.c_void_p, _sz, _sz, C.c_uint64)
_sig("nbody_ic_disc_f64", _i, C.c_void_p, _sz, _sz, C.c_uint64)
_sig("nbody_download_ids", _i, _H, C.c_void_p, _sz, C.POINTER(_sz))
_sig("nbody_let_stats", _i, _H, C.POINTER(NbodyLetStats))
_sig("nbody_debug_let_phase", _i, _H, _i, _f)
_sig("nbody_debug_let_exchange", _i, _H, _H, _i)
_sig("nbody_debug_let_set_prune", _i, _H, _i)
_sig("nbody_debug_let_bounds", _i, _H, C.c_void_p)
_sig("nbody_debug_let_set_balance", _i, _H, _i)
_sig("nbody_debug_let_export_held", _i, _H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t))
_sig("nbody_host_exchange_layout", _i, C.c_void_p, _i, _i, C.c_longlong, _i, _sz, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_sz))
_sig("nbody_host_launch_plan", _i, _sz, _f, _i, C.POINTER(_i))
_sig("nbody_tracers_upload", _i, _H, C.c_void_p, _sz, _sz, _sz)
_sig("nbody_tracers_download", _i, _H, C.c_void_p, _sz, _sz, C.POINTER(_sz))
_sig("nbody_tracers_count", _i, _H, C.POINTER(_sz))
_sig("nbody_tracer_stats", _i, _H, C.POINTER(C.c_uint64))
_sig("nbody_host_tracer_plan", _i, _sz, _sz, C.POINTER(_i))
_pc = C.POINTER(NbodyExternalComponent)
_sig("nbody_set_external_field", _i, _H, _pc, _sz)
_sig("nbody_get_external_field", _i, _H, _pc, _sz, C.POINTER(_sz))
_sig("nbody_external_potentials", _i, _H, C.c_void_p, _sz, C.POINTER(_sz))
_sig("nbody_external_energy", _i, _H, C.POINTER(C.c_double))
_sig("nbody_external_at", _i, _H, C.c_void_p, _sz, C.c_void_p, C.c_void_p)
_sig("nbody_host_external_eval", _i, _pc, _sz, C.c_double, C.c_void_p, _sz, C.c_void_p, C.c_void_p)
_sig("nbody_moments", _i, _H, C.POINTER(C.c_double))
_sig("nbody_lagrangian_radii", _i, _H, C.c_void_p, C.c_void_p, _sz, C.c_void_p, C.POINTER(C.c_double))
_sig("nbody_partners", _i, _H, C.c_void_p, C.c_void_p, _sz, C.POINTER(_sz))
_sig("nbody_bound_pairs", _i, _H, C.c_void_p, _sz, C.POINTER(_sz), C.POINTER(C.c_double))
_sig("nbody_nearest", _i, _H, C.c_void_p, C.c_void_p, _sz, C.POINTER(_sz))
_sig("nbody_contacts", _i, _H, C.c_double, C.c_void_p, _sz, C.POINTER(_sz))
_sig("nbody_merge_contacts", _i, _H, C.c_double, C.c_void_p, _sz, C.POINTER(_sz))
_sig("nbody_fof_labels", _i, _H, C.c_double, C.c_void_p, _sz, C.POINTER(_sz), C.POINTER(_sz))
_sig("nbody_fof_groups", _i, _H, C.c_double, _i, C.c_void_p, _sz, C.POINTER(_sz), C.c_void_p, _sz, C.POINTER(_sz))
_sig("nbody_fof_bound_groups", _i, _H, C.c_double, _i, _i, C.c_void_p, _sz, C.POINTER(_sz), C.c_void_p, _sz, C.POINTER(_sz), C.c_void_p)
_sig("nbody_neighbors_within", _i, _H, C.c_double, C.c_void_p, _sz, C.c_void_p, _sz, C.POINTER(_sz), C.POINTER(C.c_uint64))
_sig("nbody_density", _i, _H, C.c_double, _i, C.c_void_p, C.c_void_p, _sz, C.POINTER(_sz))
_sig("nbody_density_center", _i, _H, C.c_double, _i, C.POINTER(C.c_double), C.POINTER(C.c_double))
_sig("nbody_knn", _i, _H, _i, C.c_double, C.c_void_p, C.c_void_p, _sz, C.POINTER(_sz), C.POINTER(C.c_uint64))
_sig("nbody_knn_density", _i, _H, _i, C.c_double, C.c_void_p, C.c_void_p, _sz, C.POINTER(_sz))
_sig("nbody_knn_density_center", _i, _H, _i, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double))
_sig("nbody_pair_counts", _i, _H, C.c_void_p, _i, C.c_void_p, C.c_void_p)
_sig("nbody_pair_counts_at", _i, _H, C.c_void_p, _sz, C.c_void_p, _i, C.c_void_p, C.c_void_p)
_sig("nbody_deposit", _i, _H, C.POINTER(GridSpec), C.c_void_p, _sz, C.c_void_p)
_sig("nbody_host_deposit", _i, C.c_void_p, C.c_void_p, _sz, C.POINTER(GridSpec), C.c_void_p, _sz, C.c_void_p)
_sig("nbody_deposit_stats", _i, _H, C.POINTER(C.c_uint64))
_sig("nbody_grid_sample", _i, _H, C.POINTER(GridSpec), C.c_void_p, _i, _i, C.c_void_p, C.c_void_p, _sz, C.POINTER(_sz), C.c_void_p)
_sig("nbody_grid_sample_at", _i, _H, C.POINTER(GridSpec), C.c_void_p, _i, _i, C.c_void_p, _sz, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("nbody_host_grid_sample", _i, C.c_void_p, _sz, C.POINTER(GridSpec), C.c_void_p, _i, _i, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("nbody_grid_sample_stats", _i, _H, C.POINTER(C.c_uint64))
_sig("nbody_grid_poisson", _i, _H, C.POINTER(GridSpec), C.POINTER(NbodyPoissonSpec), C.c_void_p, C.c_void_p, _sz)
_sig("nbody_host_grid_poisson", _i, C.POINTER(GridSpec), C.POINTER(NbodyPoissonSpec), C.c_void_p, C.c_void_p, _sz)
_sig("nbody_host_poisson_twiddles", _i, _i, C.c_void_p)
_sig("nbody_grid_poisson_stats", _i, _H, C.POINTER(C.c_uint64))
_sig("nbody_pm_field", _i, _H, C.POINTER(GridSpec), C.POINTER(NbodyPmSpec), C.c_void_p, C.c_void_p, C.c_void_p, _sz, C.POINTER(_sz), C.c_void_p)
_sig("nbody_pm_field_at", _i, _H, C.POINTER(GridSpec), C.POINTER(NbodyPmSpec), C.c_void_p, _sz, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("nbody_host_pm_field", _i, C.c_void_p, C.c_void_p, _sz, C.POINTER(GridSpec), C.POINTER(NbodyPmSpec), C.c_void_p, _sz, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p)
_sig("nbody_pm_field_stats", _i, _H, C.POINTER(C.c_uint64))
_sig("nbody_p3m_field", _i, _H, C.POINTER(GridSpec), C.POINTER(NbodyP3mSpec), C.c_void_p, C.c_void_p, C.c_void_p, _sz, C.POINTER(_sz), C.c_void_p)
_sig("nbody_p3m_field_at", _i, _H, C.POINTER(GridSpec), C.POINTER(NbodyP3mSpec), C.c_void_p, _sz, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("nbody_host_p3m_field", _i, C.c_void_p, C.c_void_p, _sz, C.POINTER(GridSpec), C.POINTER(NbodyP3mSpec), C.c_void_p, _sz, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p)
_sig("nbody_host_p3m_table", _i, C.c_double, C.c_double, C.c_void_p)
_sig("nbody_p3m_field_stats", _i, _H, C.POINTER(C.c_uint64))
_sig("nbody_set_mesh_gravity", _i, _H, C.POINTER(GridSpec), C.POINTER(NbodyPmSpec))
_sig("nbody_get_mesh_gravity", _i, _H, C.POINTER(GridSpec), C.POINTER(NbodyPmSpec), C.POINTER(C.c_int))
_sig("nbody_mesh_gravity_stats", _i, _H, C.POINTER(C.c_uint64))
_sig("nbody_set_pair_search", _i, _H, _i)
_sig("nbody_get_pair_search", _i, _H, C.POINTER(_i))
_sig("nbody_pair_search_stats", _i, _H, C.POINTER(C.c_uint64))
_sig("nbody_host_cell_grid", _i, C.c_void_p, _sz, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p, C.POINTER(_i))
_sig("nbody_set_tuning", _i, _H, C.c_char_p, _i)
_sig("nbody_get_tuning", _i, _H, C.c_char_p, C.POINTER(_i))
_sig("nbody_is_tuning_build", _i)
_sig("nbody_get_config", _i, _H, C.POINTER(NbodyConfig))
_sig("nbody_abi_version", _i)
_sig("nbody_device_count", _i)


#: knobs every Simulation created from here on starts with (host-side convenience of this mirror; the library itself
#: keeps its knobs per handle): `with tuning_defaults(bh_walk_split=4): ...`
_default_tuning: dict = {}


class tuning_defaults:
    def __init__(self, **knobs):
        self.knobs = knobs

    def __enter__(self):
        self.saved = dict(_default_tuning)
        _default_tuning.update(self.knobs)
        return self

    def __exit__(self, *a):
        _default_tuning.clear()
        _default_tuning.update(self.saved)


def launch_plan(n_bodies: int, theta2: float = 0.25, fast_math: bool = True) -> dict:
    """The launch shapes the library derives from a body count with its default knobs (nbody_host_launch_plan)."""
    out = (C.c_int * 3)()
    rc = lib.nbody_host_launch_plan(int(n_bodies), float(theta2), int(bool(fast_math)), out)
    if rc != 0:
        raise NbodyError(rc, "nbody_host_launch_plan")
    return {"walk_bodies_per_lane": out[0], "walk_segments": out[1], "sym_bodies_per_lane": out[2]}


def host_tracer_plan(n_tracers: int, n_bodies: int) -> dict:
    """The fast tracer pass's shape for that many tracers and bodies (nbody_host_tracer_plan; no device needed): slice k of
    the bodies is [k * slice_len, min(n_bodies, (k + 1) * slice_len))."""
    out = (C.c_int * 4)()
    rc = lib.nbody_host_tracer_plan(int(n_tracers), int(n_bodies), out)
    if rc != 0:
        raise NbodyError(rc, "nbody_host_tracer_plan")
    return {"tracers_per_lane": out[0], "groups": out[1], "slices": out[2], "slice_len": out[3]}


def is_tuning_build() -> bool:
    return bool(lib.nbody_is_tuning_build())


class NbodyError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"nbody error {code}: {msg}")
        self.code = code


def external_component(kind: int, p, center=(0.0, 0.0, 0.0), reserved: int = 0) -> NbodyExternalComponent:
    """kind EXT_PLUMMER p = (M, b) | EXT_HERNQUIST (M, a) | EXT_MIYAMOTO_NAGAI (M, a, b) | EXT_LOGARITHMIC (v0, rc, qy, qz);
    parameters the kind does not use are 0."""
    p = [float(v) for v in p] + [0.0] * (4 - len(p))
    return NbodyExternalComponent(int(kind), int(reserved), (C.c_double * 3)(*[float(v) for v in center]), (C.c_double * 4)(*p))


def _component_array(comps):
    comps = list(comps)
    return (NbodyExternalComponent * max(1, len(comps)))(*comps), len(comps)


def host_external_eval(comps, g: float, points, acc: bool = True, phi: bool = True):
    """(acc [M, 3] f64 | None, phi [M] f64 | None) of the components at the M points, on the host in f64
    (nbody_host_external_eval; no device needed): the code nbody_external_at runs on the device."""
    arr, n = _component_array(comps)
    xyz = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    m = len(xyz)
    a = np.zeros((m, 3), np.float64) if acc else None
    v = np.zeros(m, np.float64) if phi else None
    rc = lib.nbody_host_external_eval(arr, n, float(g), xyz.ctypes.data if m else None, m, a.ctypes.data if acc else None,
                                      v.ctypes.data if phi else None)
    if rc:
        raise NbodyError(rc, (lib.nbody_last_error(None) or b"").decode())
    return a, v


def cell_grid(points, length: float, keys: bool = True) -> dict:
    """The uniform grid NBODY_SEARCH_CELLS would draw for the points [n, 3] (f64) and a linking length or radius
    (nbody_host_cell_grid; no device needed): dict(lo [3] f64, side, usable, keys [n] uint64 | None).  A point with a NaN or
    infinite coordinate, and every point of a grid that is not usable, has the all-ones key."""
    xyz = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    n = len(xyz)
    lo = (C.c_double * 3)()
    side, usable = C.c_double(0.0), C.c_int(0)
    key = np.zeros(n, np.uint64) if keys else None
    rc = lib.nbody_host_cell_grid(xyz.ctypes.data if n else None, n, float(length), lo, C.byref(side), key.ctypes.data if keys and n else None,
                                  C.byref(usable))
    if rc:
        raise NbodyError(rc, "nbody_host_cell_grid: the length must be finite and > 0")
    return dict(lo=np.array(lo[:], np.float64), side=float(side.value), usable=bool(usable.value), keys=key)


def host_deposit(points, q, origin, spacing, dims, scheme=DEPOSIT_CIC, periodic=False, project_axis=-1) -> tuple[np.ndarray, np.ndarray]:
    """(grid [nx, ny, nz] f64, counts [4] uint64 = inside, partial, outside, skipped): points [n][3] with the quantities q [n]
    assigned to a regular grid in 64-bit fixed point -- nbody_deposit's arithmetic on the host (nbody_host_deposit; no device
    needed).  The same points give the same bits in any order."""
    xyz = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    qq = np.ascontiguousarray(np.asarray(q, np.float64).reshape(-1))
    if len(qq) != len(xyz):
        raise ValueError("host_deposit: q must hold one value per point")
    spec = grid_spec(origin, spacing, dims, scheme, DEPOSIT_MASS, periodic, project_axis)
    shape = tuple(max(int(v), 0) for v in dims)
    grid = np.zeros(shape, np.float64)
    counts = np.zeros(4, np.uint64)
    n = len(xyz)
    rc = lib.nbody_host_deposit(xyz.ctypes.data if n else None, qq.ctypes.data if n else None, n, C.byref(spec),
                                grid.ctypes.data if grid.size else None, grid.size, counts.ctypes.data)
    if rc:
        raise NbodyError(rc, "nbody_host_deposit: the spec is not valid (include/nbody_hip.h lists what is refused)")
    return grid, counts


def _sample_grid(grid, origin, spacing, scheme, op, periodic, project_axis):
    """(grid as contiguous f64 [fields][nx][ny][nz], fields, its GridSpec, the doubles of a row of out) of a grid_sample call"""
    g = np.ascontiguousarray(grid, np.float64)
    if g.ndim == 3:
        g = g[None]
    if g.ndim != 4:
        raise ValueError("grid_sample: grid must be [nx, ny, nz] or [fields, nx, ny, nz]")
    fields = int(g.shape[0])
    spec = grid_spec(origin, spacing, g.shape[1:], scheme, DEPOSIT_MASS, periodic, project_axis)
    return g, fields, spec, fields if int(op) == SAMPLE_VALUE else 3


def host_grid_sample(points, grid, origin, spacing, scheme=DEPOSIT_CIC, op=SAMPLE_VALUE, periodic=False, project_axis=-1) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(out [n, fields] or [n, 3] f64, cls [n] uint8, counts [4] uint64 = inside, partial, outside, skipped): the grid ([nx, ny,
    nz] or [fields, nx, ny, nz]) read back at points [n][3] with the deposit's weights -- nbody_grid_sample's arithmetic on the
    host (nbody_host_grid_sample; no device needed)."""
    xyz = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    g, fields, spec, width = _sample_grid(grid, origin, spacing, scheme, op, periodic, project_axis)
    n = len(xyz)
    out = np.zeros((n, width), np.float64)
    cls = np.zeros(n, np.uint8)
    counts = np.zeros(4, np.uint64)
    rc = lib.nbody_host_grid_sample(xyz.ctypes.data if n else None, n, C.byref(spec), g.ctypes.data if g.size else None, fields, int(op),
                                    out.ctypes.data if out.size else None, cls.ctypes.data if n else None, counts.ctypes.data)
    if rc:
        raise NbodyError(rc, "nbody_host_grid_sample: the call is not valid (include/nbody_hip.h lists what is refused)")
    return out, cls, counts


def _poisson_call(mass, spacing, g, periodic, green, soften, deconvolve, scheme):
    """(mass as contiguous f64 [nx][ny][nz], its GridSpec, the NbodyPoissonSpec) of a grid_poisson call"""
    m = np.ascontiguousarray(mass, np.float64)
    if m.ndim != 3:
        raise ValueError("grid_poisson: mass must be [nx, ny, nz]")
    spec = grid_spec((0.0, 0.0, 0.0), spacing, m.shape, scheme, DEPOSIT_MASS, periodic, -1)
    ps = NbodyPoissonSpec(float(g), float(soften), int(green), int(deconvolve), (C.c_int32 * 2)(0, 0))
    return m, spec, ps


def host_grid_poisson(mass, spacing, g, periodic=False, green=POISSON_SPECTRAL, soften=0.0, deconvolve=0, scheme=DEPOSIT_CIC) -> np.ndarray:
    """phi [nx, ny, nz] f64 at the cell centres from the mass per cell [nx, ny, nz] (what host_deposit returns for DEPOSIT_MASS;
    powers of two) -- nbody_grid_poisson's arithmetic on the host (nbody_host_grid_poisson; no device needed).  periodic: green =
    POISSON_SPECTRAL or POISSON_DIFF2 and deconvolve = 0, 1 or 2 powers of the scheme's window; isolated: soften >= 0."""
    m, spec, ps = _poisson_call(mass, spacing, g, periodic, green, soften, deconvolve, scheme)
    phi = np.zeros(m.shape, np.float64)
    rc = lib.nbody_host_grid_poisson(C.byref(spec), C.byref(ps), m.ctypes.data if m.size else None, phi.ctypes.data if phi.size else None, phi.size)
    if rc:
        raise NbodyError(rc, "nbody_host_grid_poisson: the call is not valid (include/nbody_hip.h lists what is refused)")
    return phi


def host_poisson_twiddles(length: int) -> np.ndarray:
    """[length / 2, 2] f64: the table {cos, -sin}((2 pi k) / length) every transform of that length reads, on the device as on
    the host (nbody_host_poisson_twiddles); length a power of two in 2 .. POISSON_MAX_AXIS."""
    out = np.zeros((max(int(length) // 2, 1), 2), np.float64)
    rc = lib.nbody_host_poisson_twiddles(int(length), out.ctypes.data)
    if rc:
        raise NbodyError(rc, "nbody_host_poisson_twiddles: length must be a power of two in 2 .. 4096")
    return out


def pm_spec(g, gradient=SAMPLE_GRADIENT2, green=POISSON_SPECTRAL, soften=0.0, deconvolve=0) -> NbodyPmSpec:
    """An NbodyPmSpec from plain values: the constants of grid_poisson and SAMPLE_GRADIENT2 or SAMPLE_GRADIENT4."""
    ps = NbodyPoissonSpec(float(g), float(soften), int(green), int(deconvolve), (C.c_int32 * 2)(0, 0))
    return NbodyPmSpec(ps, int(gradient), (C.c_int32 * 3)(0, 0, 0))


def mesh_gravity_specs(value) -> tuple[GridSpec, NbodyPmSpec]:
    """The (GridSpec, NbodyPmSpec) pair Simulation.mesh_gravity takes, from such a pair or from a dict of pm_field's keywords.  No
    device needed; what the pair must satisfy is checked by nbody_set_mesh_gravity."""
    if isinstance(value, dict):
        known = {"origin", "spacing", "dims", "g", "scheme", "gradient", "periodic", "green", "soften", "deconvolve", "project_axis"}
        extra = set(value) - known
        if extra:
            raise ValueError(f"mesh_gravity: unknown keys {sorted(extra)}")
        missing = {"origin", "spacing", "dims"} - set(value)
        if missing:
            raise ValueError(f"mesh_gravity: missing keys {sorted(missing)}")
        spec = grid_spec(value["origin"], value["spacing"], value["dims"], value.get("scheme", DEPOSIT_CIC), DEPOSIT_MASS,
                         value.get("periodic", False), value.get("project_axis", -1))
        pm = pm_spec(value.get("g", 1.0), value.get("gradient", SAMPLE_GRADIENT2), value.get("green", POISSON_SPECTRAL),
                     value.get("soften", 0.0), value.get("deconvolve", 0))
        return spec, pm
    try:
        spec, pm = value
    except (TypeError, ValueError):
        raise TypeError("mesh_gravity: a dict, a (GridSpec, NbodyPmSpec) pair or None") from None
    if not isinstance(spec, GridSpec) or not isinstance(pm, NbodyPmSpec):
        raise TypeError("mesh_gravity: a dict, a (GridSpec, NbodyPmSpec) pair or None")
    return spec, pm


def host_pm_field(bodies, mass, origin, spacing, dims, g, scheme=DEPOSIT_CIC, gradient=SAMPLE_GRADIENT2, periodic=False, green=POISSON_SPECTRAL,
                  soften=0.0, deconvolve=0, project_axis=-1, points=None, phi=True) -> tuple[np.ndarray, np.ndarray | None, np.ndarray, np.ndarray]:
    """(acc [n, 3] f64, phi [n] f64 | None, cls [n] uint8, counts [8] uint64 = the deposit's four and the gradient sample's four): the
    particle-mesh field of the bodies [nb][3] with masses [nb] at the bodies themselves, or at points [n][3] -- host_deposit,
    host_grid_poisson and host_grid_sample composed, acc = 0.0 - grad (nbody_host_pm_field; no device needed)."""
    bxyz = np.ascontiguousarray(np.asarray(bodies, np.float64).reshape(-1, 3))
    bm = np.ascontiguousarray(np.asarray(mass, np.float64).reshape(-1))
    if len(bm) != len(bxyz):
        raise ValueError("host_pm_field: mass must hold one value per body")
    spec = grid_spec(origin, spacing, dims, scheme, DEPOSIT_MASS, periodic, project_axis)
    pm = pm_spec(g, gradient, green, soften, deconvolve)
    xyz = None if points is None else np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    n = len(bxyz) if xyz is None else len(xyz)
    acc = np.zeros((n, 3), np.float64)
    val = np.zeros(n, np.float64) if phi else None
    cls = np.zeros(n, np.uint8)
    counts = np.zeros(8, np.uint64)
    # (a non-NULL xyz even for no point: NULL means the bodies)
    hold = np.zeros(3, np.float64)
    xp = None if xyz is None else (xyz.ctypes.data if len(xyz) else hold.ctypes.data)
    rc = lib.nbody_host_pm_field(bxyz.ctypes.data if len(bxyz) else None, bm.ctypes.data if len(bm) else None, len(bxyz), C.byref(spec), C.byref(pm),
                                 xp, 0 if xyz is None else len(xyz), acc.ctypes.data if n else None, val.ctypes.data if phi and n else None,
                                 cls.ctypes.data if n else None, counts.ctypes.data)
    if rc:
        raise NbodyError(rc, "nbody_host_pm_field: the call is not valid (include/nbody_hip.h lists what is refused)")
    return acc, val, cls, counts


def p3m_spec(g, r_split, r_cut, gradient=SAMPLE_GRADIENT2, green=POISSON_SPECTRAL, deconvolve=0, soften=0.0, terms=P3M_BOTH) -> NbodyP3mSpec:
    """An NbodyP3mSpec from plain values: pm_spec's constants (the mesh's own soften is 0: periodic grids only), the split scale
    r_split, the cutoff r_cut, the Plummer softening of the short-range term and P3M_BOTH, P3M_MESH_ONLY or P3M_SHORT_ONLY."""
    return NbodyP3mSpec(pm_spec(g, gradient, green, 0.0, deconvolve), float(r_split), float(r_cut), float(soften), int(terms), 0)


def host_p3m_table(r_split, r_cut) -> np.ndarray:
    """[4097, 2] f64: the split factors {F, P} at x_k = k (r_cut / r_split) / 4096 (nbody_host_p3m_table; no device needed)."""
    out = np.zeros((P3M_TABLE_INTERVALS + 1, 2), np.float64)
    rc = lib.nbody_host_p3m_table(float(r_split), float(r_cut), out.ctypes.data)
    if rc:
        raise NbodyError(rc, "nbody_host_p3m_table: r_split must be finite and > 0 and r_cut finite in r_split .. 8 r_split")
    return out


def host_p3m_field(bodies, mass, origin, spacing, dims, g, r_split, r_cut, scheme=DEPOSIT_CIC, gradient=SAMPLE_GRADIENT2, green=POISSON_SPECTRAL,
                   deconvolve=0, soften=0.0, terms=P3M_BOTH, points=None, phi=True) -> tuple[np.ndarray, np.ndarray | None, np.ndarray, np.ndarray]:
    """(acc [n, 3] f64, phi [n] f64 | None, cls [n] uint8, counts [8] uint64): the P3M field of the bodies [nb][3] with masses [nb]
    on a periodic grid, at the bodies themselves or at points [n][3] -- host_pm_field with the Gaussian split of scale r_split in
    its Green stage plus the minimum-image pair sum of the bodies closer than r_cut (nbody_host_p3m_field; no device needed)."""
    bxyz = np.ascontiguousarray(np.asarray(bodies, np.float64).reshape(-1, 3))
    bm = np.ascontiguousarray(np.asarray(mass, np.float64).reshape(-1))
    if len(bm) != len(bxyz):
        raise ValueError("host_p3m_field: mass must hold one value per body")
    spec = grid_spec(origin, spacing, dims, scheme, DEPOSIT_MASS, True, -1)
    p3m = p3m_spec(g, r_split, r_cut, gradient, green, deconvolve, soften, terms)
    xyz = None if points is None else np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    n = len(bxyz) if xyz is None else len(xyz)
    acc = np.zeros((n, 3), np.float64)
    val = np.zeros(n, np.float64) if phi else None
    cls = np.zeros(n, np.uint8)
    counts = np.zeros(8, np.uint64)
    hold = np.zeros(3, np.float64)   # (a non-NULL xyz even for no point: NULL means the bodies)
    xp = None if xyz is None else (xyz.ctypes.data if len(xyz) else hold.ctypes.data)
    rc = lib.nbody_host_p3m_field(bxyz.ctypes.data if len(bxyz) else None, bm.ctypes.data if len(bm) else None, len(bxyz), C.byref(spec),
                                  C.byref(p3m), xp, 0 if xyz is None else len(xyz), acc.ctypes.data if n else None,
                                  val.ctypes.data if phi and n else None, cls.ctypes.data if n else None, counts.ctypes.data)
    if rc:
        raise NbodyError(rc, "nbody_host_p3m_field: the call is not valid (include/nbody_hip.h lists what is refused)")
    return acc, val, cls, counts


def tidal_matrices(t6) -> np.ndarray:
    """[n, 3, 3] symmetric matrices from Simulation.tidal_at's [n, 6] rows {xx, xy, xz, yy, yz, zz}."""
    t6 = np.asarray(t6, np.float64).reshape(-1, 6)
    return t6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def device_count() -> int:
    return int(lib.nbody_device_count())


def plummer(n: int, seed: int = 20250523, f64: bool = False) -> np.ndarray:
    """Plummer sphere in Henon units as PointParticle records (host side; generated in f64, rounded to f32 unless f64)."""
    if f64:
        out = np.zeros(n, dtype=PARTICLE_DTYPE64)
        rc = lib.nbody_ic_plummer_f64(out.ctypes.data, n, 80, seed)
        if rc:
            raise NbodyError(rc, "nbody_ic_plummer_f64")
        return out
    out = np.zeros(n, dtype=PARTICLE_DTYPE)
    rc = lib.nbody_ic_plummer(out.ctypes.data, n, 40, seed)
    if rc:
        raise NbodyError(rc, "nbody_ic_plummer")
    return out


def disc(n_disc: int, seed: int = 20250523, f64: bool = False) -> np.ndarray:
    """The reference's self-gravitating disc (src/main.rs:52-89): 1 star + n_disc bodies."""
    if f64:
        out = np.zeros(n_disc + 1, dtype=PARTICLE_DTYPE64)
        rc = lib.nbody_ic_disc_f64(out.ctypes.data, n_disc, 80, seed)
        if rc:
            raise NbodyError(rc, "nbody_ic_disc_f64")
        return out
    out = np.zeros(n_disc + 1, dtype=PARTICLE_DTYPE)
    rc = lib.nbody_ic_disc(out.ctypes.data, n_disc, 40, seed)
    if rc:
        raise NbodyError(rc, "nbody_ic_disc")
    return out


def host_build_tree(pos4: np.ndarray, center, width: float, threads: int = 1):
    """Host-only octree build (no device).  Returns dict(com_mass, width, skip, leaf_body, order)."""
    pos4 = np.ascontiguousarray(pos4, dtype=np.float32).reshape(-1, 4)
    n = pos4.shape[0]
    c = (C.c_float * 3)(*[float(x) for x in center])
    nn = C.c_size_t(0)
    rc = lib.nbody_host_build_tree(pos4.ctypes.data, n, c, width, threads, None, None, None, None, None, 0, C.byref(nn))
    if rc:
        raise NbodyError(rc, "nbody_host_build_tree")
    m = nn.value
    com = np.zeros((m, 4), np.float32)
    w = np.zeros(m, np.float32)
    skip = np.zeros(m, np.int32)
    body = np.zeros(m, np.int32)
    order = np.zeros(n, np.int32)
    rc = lib.nbody_host_build_tree(pos4.ctypes.data, n, c, width, threads, com.ctypes.data, w.ctypes.data,
                                   skip.ctypes.data, body.ctypes.data, order.ctypes.data, m, C.byref(nn))
    if rc:
        raise NbodyError(rc, "nbody_host_build_tree")
    return dict(com_mass=com, width=w, skip=skip, leaf_body=body, order=order)


#: Simulation.moments(): M, the centre of mass X / M, P, L about the origin, and the raw X = sum m x (all f64; com is NaN when M == 0)
Moments = namedtuple("Moments", ["mass", "com", "momentum", "angular_momentum", "mass_dipole"])


@dataclass
class Settings:
    """SimulationSettings (src/shared.rs:61-78)."""
    g: float = 1.0
    g_soft: float = 0.0
    dt: float = 1e-3
    theta2: float = 0.5


class Simulation:
    """Host-side mirror of the reference's `Simulation` trait over the C ABI.

    `Simulation(points, center, width, method=...)` is `Simulation::new(points, LeapFrogIntegrator,
    Bounds::new(center, width))`; methods keep the trait's names and meaning.
    """

    def __init__(self, points: np.ndarray, center=(0.0, 0.0, 0.0), width: float = 1.0, *, method: int = BRUTE_FORCE,
                 math_mode: int = STRICT, capacity: int | None = None, device: int = -1, rank: int = 0,
                 world_size: int = 1, host_threads: int = 0, tree_build: int = TREE_AUTO, leaf_mode: int = LEAF_REFERENCE,
                 f64: bool | None = None, shard_mode: int = SHARD_INDEX, tuning: dict | None = None, _handle=None, _f64: bool = False):
        self._h = _H()
        self.f64 = bool(_f64)
        self.rank, self.world_size = int(rank), int(world_size)
        if _handle is not None:
            self._h = _handle
            return
        # F = f64 when the records are PointParticle<f64,3> (or asked for): NBODY_F64 handle, 80-byte records
        self.f64 = bool(f64) if f64 is not None else (getattr(points, "dtype", None) == PARTICLE_DTYPE64)
        self.dtype = PARTICLE_DTYPE64 if self.f64 else PARTICLE_DTYPE
        points = np.ascontiguousarray(points, dtype=self.dtype)
        cfg = NbodyConfig(C.sizeof(NbodyConfig), method, math_mode, leaf_mode, device, rank, world_size,
                          host_threads, int(capacity if capacity is not None else max(1, points.shape[0])), tree_build,
                          F64 if self.f64 else F32, shard_mode, 0)
        rc = lib.nbody_create(C.byref(cfg), C.byref(self._h))
        if rc:
            self._h = _H()
            raise NbodyError(rc, (lib.nbody_last_error(None) or b"").decode())
        for name, value in {**_default_tuning, **(tuning or {})}.items():
            self.set_tuning(name, value)
        self.set_bounds(center, width)
        self._check(lib.nbody_upload(self._h, points.ctypes.data, points.shape[0], self.dtype.itemsize))

    # -- plumbing
    def _check(self, rc: int):
        if rc:
            raise NbodyError(rc, (lib.nbody_last_error(self._h) or b"").decode())

    def close(self):
        if self._h:
            lib.nbody_destroy(self._h)
            self._h = _H()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- the trait surface (shared.rs:80-97)
    def init(self):
        self._check(lib.nbody_init(self._h))

    def step(self):
        self._check(lib.nbody_steps(self._h, 1))

    def steps(self, k: int):
        self._check(lib.nbody_steps(self._h, int(k)))

    def step_by(self, dt: float):
        self._check(lib.nbody_step_by_f64(self._h, float(dt)) if self.f64 else lib.nbody_step_by(self._h, float(dt)))

    def update_forces(self):
        self._check(lib.nbody_update_forces(self._h))

    def upload(self, points: np.ndarray):
        """Replace the bodies (nbody_upload: at most the capacity; a rank of a sharded world keeps its index block)."""
        points = np.ascontiguousarray(points, dtype=self.dtype)
        self._check(lib.nbody_upload(self._h, points.ctypes.data, points.shape[0], self.dtype.itemsize))

    def add_point(self, particle: np.ndarray):
        p = np.ascontiguousarray(particle, dtype=self.dtype).reshape(1)
        self._check(lib.nbody_add_point(self._h, p.ctypes.data))

    def remove_point(self, index: int):
        self._check(lib.nbody_remove_point(self._h, int(index)))

    def get_points(self) -> np.ndarray:
        n = C.c_size_t(0)
        self._check(lib.nbody_count(self._h, C.byref(n)))
        out = np.zeros(n.value, dtype=self.dtype)
        self._check(lib.nbody_download(self._h, out.ctypes.data, n.value, self.dtype.itemsize, C.byref(n)))
        return out[: n.value]

    # -- tracers: massless particles in the bodies' field (nbody_tracers_*; PointParticle<f32,3> records, mass ignored)
    def set_tracers(self, rec: np.ndarray, capacity: int | None = None):
        """Replace the tracer set (an empty array removes it); capacity = the most tracers the handle may ever hold."""
        rec = np.ascontiguousarray(rec, dtype=PARTICLE_DTYPE)
        self._check(lib.nbody_tracers_upload(self._h, rec.ctypes.data, rec.shape[0], PARTICLE_DTYPE.itemsize, int(capacity or 0)))

    def get_tracers(self) -> np.ndarray:
        """The live tracers; `acceleration` holds the last tracer force pass, `mass` 0."""
        n = C.c_size_t(0)
        self._check(lib.nbody_tracers_count(self._h, C.byref(n)))
        out = np.zeros(n.value, dtype=PARTICLE_DTYPE)
        self._check(lib.nbody_tracers_download(self._h, out.ctypes.data, n.value, PARTICLE_DTYPE.itemsize, C.byref(n)))
        return out[: n.value]

    @property
    def n_tracers(self) -> int:
        n = C.c_size_t(0)
        self._check(lib.nbody_tracers_count(self._h, C.byref(n)))
        return int(n.value)

    def tracer_stats(self) -> tuple[int, int]:
        """(directed interactions, or accepted nodes under Barnes-Hut; opening tests) of the tracer force passes since reset_stats."""
        out = (C.c_uint64 * 2)()
        self._check(lib.nbody_tracer_stats(self._h, out))
        return int(out[0]), int(out[1])

    # -- a static external field acting on bodies and tracers (nbody_set_external_field; leapfrog handles of a one-rank world)
    @property
    def external_field(self) -> list:
        """The components of the handle's external field as given ([]: none).  Assigning a list of NbodyExternalComponent
        (external_component(...)) replaces it, [] removes it; clone() carries it."""
        arr = (NbodyExternalComponent * EXTERNAL_MAX)()
        n = C.c_size_t(0)
        self._check(lib.nbody_get_external_field(self._h, arr, EXTERNAL_MAX, C.byref(n)))
        return [external_component(c.kind, list(c.p), list(c.center), c.reserved) for c in arr[: n.value]]

    @external_field.setter
    def external_field(self, comps):
        arr, n = _component_array(comps)
        self._check(lib.nbody_set_external_field(self._h, arr, n))

    def external_potentials(self) -> np.ndarray:
        """phi_ext [n] f64 of the bodies at their current positions, in get_points() order (nbody_external_potentials)."""
        cfg = NbodyConfig()
        self._check(lib.nbody_get_config(self._h, C.byref(cfg)))
        n = C.c_size_t(0)
        phi = np.zeros(max(int(cfg.capacity), 1), np.float64)
        self._check(lib.nbody_external_potentials(self._h, phi.ctypes.data, len(phi), C.byref(n)))
        return phi[: n.value]

    def external_energy(self) -> float:
        """sum m_i phi_ext(x_i): the conserved total is KE + PE + this (energy() stays self-gravity only)."""
        v = C.c_double(0)
        self._check(lib.nbody_external_energy(self._h, C.byref(v)))
        return float(v.value)

    def external_at(self, points, acc: bool = True, phi: bool = True):
        """(acc [M, 3] f64 | None, phi [M] f64 | None) of the external field alone at the M points (nbody_external_at)."""
        xyz = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
        m = len(xyz)
        a = np.zeros((m, 3), np.float64) if acc else None
        v = np.zeros(m, np.float64) if phi else None
        self._check(lib.nbody_external_at(self._h, xyz.ctypes.data if m else None, m, a.ctypes.data if acc else None,
                                          v.ctypes.data if phi else None))
        return a, v

    # -- diagnostics of the state as a whole (nbody_moments, nbody_lagrangian_radii): f64, read-only, one-rank index-block handles
    def moments(self) -> Moments:
        """Moments(mass, com, momentum, angular_momentum, mass_dipole) of the bodies as get_points() would report them: M = sum m,
        P = sum m v, L = sum m (x cross v) about the origin, mass_dipole = X = sum m x and com = X / M (nbody_moments; summed on
        the device in a fixed order, the same input gives the same bits).  Tracers are not counted."""
        out = (C.c_double * 10)()
        self._check(lib.nbody_moments(self._h, out))
        v = np.array(out[:], np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            com = v[1:4] / v[0]
        return Moments(float(v[0]), com, v[4:7].copy(), v[7:10].copy(), v[1:4].copy())

    def lagrangian_radii(self, fractions, center=None) -> tuple[np.ndarray, float]:
        """(radii [K] f64, mass): radii[k] is the distance from `center` (None: the centre of mass) within which the fraction
        fractions[k] of the bodies' mass lies -- the distance of the first body, in ascending (distance, index) order, whose
        cumulative mass reaches fractions[k] * mass (nbody_lagrangian_radii).  Bodies at a NaN distance are left out."""
        fr = np.ascontiguousarray(np.asarray(fractions, np.float64).reshape(-1))
        k = len(fr)
        radii = np.zeros(k, np.float64)
        mass = C.c_double(0)
        c = None if center is None else np.ascontiguousarray(np.asarray(center, np.float64).reshape(3))
        self._check(lib.nbody_lagrangian_radii(self._h, None if c is None else c.ctypes.data, fr.ctypes.data if k else None, k,
                                               radii.ctypes.data if k else None, C.byref(mass)))
        return radii, float(mass.value)

    # -- binary census (nbody_partners, nbody_bound_pairs): f64, read-only, O(N^2) pair energies on the device
    def partners(self) -> tuple[np.ndarray, np.ndarray]:
        """(partner [n] int32, energy [n] f64): for every body, in get_points() order, the other body of least two-body energy
        e_ij = w^2 / 2 - g (m_i + m_j) / sqrt(r^2 + g_soft^2) (the lowest index among equal energies) and that energy; -1 and
        +inf for a body without a partner (nbody_partners)."""
        n = C.c_size_t(0)
        self._check(lib.nbody_partners(self._h, None, None, 0, C.byref(n)))
        partner = np.full(n.value, -1, np.int32)
        energy = np.full(n.value, np.inf, np.float64)
        self._check(lib.nbody_partners(self._h, partner.ctypes.data if n.value else None, energy.ctypes.data if n.value else None,
                                       n.value, C.byref(n)))
        return partner[: n.value], energy[: n.value]

    def bound_pairs(self) -> tuple[np.ndarray, float]:
        """(pairs, binding_sum): the mutual bound pairs -- each the other's partners(), e < 0 -- as a BOUND_PAIR_DTYPE array in
        ascending i (i < j) with their orbital elements, and the sum of their binding energies in that order
        (nbody_bound_pairs)."""
        n = C.c_size_t(0)
        self._check(lib.nbody_partners(self._h, None, None, 0, C.byref(n)))   # (counts only: n bodies hold at most n // 2 pairs)
        pairs = np.zeros(n.value // 2 + 1, BOUND_PAIR_DTYPE)
        total = C.c_double(0)
        self._check(lib.nbody_bound_pairs(self._h, pairs.ctypes.data, len(pairs), C.byref(n), C.byref(total)))
        return pairs[: n.value].copy(), float(total.value)

    # -- sticky mergers (nbody_nearest, nbody_contacts, nbody_merge_contacts): f64 distances, O(N^2) on the device
    def nearest(self) -> tuple[np.ndarray, np.ndarray]:
        """(nearest [n] int32, dist2 [n] f64): for every body, in get_points() order, the other body at the least unsoftened
        squared distance (the lowest index among equal distances) and that r2; -1 and +inf for a body without one
        (nbody_nearest)."""
        n = C.c_size_t(0)
        self._check(lib.nbody_nearest(self._h, None, None, 0, C.byref(n)))
        nearest = np.full(n.value, -1, np.int32)
        dist2 = np.full(n.value, np.inf, np.float64)
        self._check(lib.nbody_nearest(self._h, nearest.ctypes.data if n.value else None, dist2.ctypes.data if n.value else None,
                                      n.value, C.byref(n)))
        return nearest[: n.value], dist2[: n.value]

    def _contact_list(self, call, radius: float) -> np.ndarray:
        n = C.c_size_t(0)
        self._check(lib.nbody_nearest(self._h, None, None, 0, C.byref(n)))   # (counts only: n bodies hold at most n // 2 contacts)
        out = np.zeros(n.value // 2 + 1, CONTACT_DTYPE)
        self._check(call(self._h, float(radius), out.ctypes.data, len(out), C.byref(n)))
        return out[: n.value].copy()

    def contacts(self, radius: float) -> np.ndarray:
        """The mutual nearest pairs closer than `radius` (strictly) as a CONTACT_DTYPE array in ascending i (i < j); read-only
        (nbody_contacts)."""
        return self._contact_list(lib.nbody_contacts, radius)

    def merge_contacts(self, radius: float) -> np.ndarray:
        """Merges every contacts(radius) pair into one body at its centre of mass (total mass, momentum, mass-weighted
        acceleration) in row i, removes row j, keeps everybody else's order, and returns the list.  One call merges disjoint
        pairs: repeat while the list is not empty (nbody_merge_contacts)."""
        return self._contact_list(lib.nbody_merge_contacts, radius)

    # -- friends-of-friends groups (nbody_fof_labels, nbody_fof_groups): f64 distances, read-only, O(N^2 / 2) on the device
    def fof_labels(self, b: float) -> tuple[np.ndarray, int]:
        """(labels [n] int32, n_groups): labels[i] is the lowest index of i's group, in get_points() order -- two bodies closer
        than the linking length `b` (strictly) are friends, a group is a connected component of friendship; n_groups counts the
        groups, singletons included (nbody_fof_labels)."""
        n, groups = C.c_size_t(0), C.c_size_t(0)
        self._check(lib.nbody_fof_labels(self._h, float(b), None, 0, C.byref(n), None))   # (the bodies only)
        labels = np.full(n.value, -1, np.int32)
        self._check(lib.nbody_fof_labels(self._h, float(b), labels.ctypes.data if n.value else None, n.value, C.byref(n), C.byref(groups)))
        return labels[: n.value], int(groups.value)

    def fof_groups(self, b: float, min_members: int = 2) -> tuple[np.ndarray, np.ndarray]:
        """(groups, members): the friends-of-friends groups of linking length `b` with at least min_members bodies as a
        GROUP_DTYPE array in ascending `first` (= the group's fof_labels() label), and their bodies [int32], group after group,
        each in ascending index: group k's are members[offset : offset + count].  mass = sum m, mx = sum m x, mv = sum m v, summed
        in a fixed order; the centre of mass is mx / mass (nbody_fof_groups)."""
        n = C.c_size_t(0)
        self._check(lib.nbody_fof_labels(self._h, float(b), None, 0, C.byref(n), None))   # (the bodies only: an upper bound of both)
        groups = np.zeros(n.value // max(int(min_members), 1) + 1, GROUP_DTYPE)
        members = np.full(n.value + 1, -1, np.int32)
        ng, nm = C.c_size_t(0), C.c_size_t(0)
        self._check(lib.nbody_fof_groups(self._h, float(b), int(min_members), groups.ctypes.data, len(groups), C.byref(ng),
                                         members.ctypes.data, len(members), C.byref(nm)))
        return groups[: ng.value].copy(), members[: nm.value].copy()

    def fof_bound_groups(self, b: float, min_members: int = 2, max_iterations: int = 32) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(groups, members, energy): the self-bound subsets of the fof_groups(b, min_members) groups.  Every member's energy
        e = 0.5 u2 + phi is evaluated inside its own group (u relative to the group's mean velocity, phi softened, from the
        group's members only), all members with !(e < 0) are stripped at once, and the pass repeats until nobody is unbound or
        max_iterations passes have run; a group left with fewer than min_members bodies is dropped.  groups is a
        BOUND_GROUP_DTYPE array in ascending `first` (the FoF label, which need not be a bound member), members [int32] the
        bound bodies, group after group in ascending index, energy [f64] their e from the group's last pass
        (nbody_fof_bound_groups)."""
        n = C.c_size_t(0)
        self._check(lib.nbody_fof_labels(self._h, float(b), None, 0, C.byref(n), None))   # (the bodies only: an upper bound of both)
        groups = np.zeros(n.value // max(int(min_members), 1) + 1, BOUND_GROUP_DTYPE)
        members = np.full(n.value + 1, -1, np.int32)
        energy = np.zeros(n.value + 1, np.float64)
        ng, nm = C.c_size_t(0), C.c_size_t(0)
        self._check(lib.nbody_fof_bound_groups(self._h, float(b), int(min_members), int(max_iterations), groups.ctypes.data, len(groups),
                                               C.byref(ng), members.ctypes.data, len(members), C.byref(nm), energy.ctypes.data))
        return groups[: ng.value].copy(), members[: nm.value].copy(), energy[: nm.value].copy()

    # -- neighbours within a radius (nbody_neighbors_within, nbody_density, nbody_density_center): f64, read-only, on the device
    def neighbors_within(self, radius: float) -> tuple[np.ndarray, np.ndarray]:
        """(offset [n + 1] uint64, neighbor [offset[n]] int32): a CSR list -- the bodies closer to body i than `radius` (strictly;
        unsoftened f64 distances) are neighbor[offset[i] : offset[i + 1]], in ascending index, in get_points() order; offset[n]
        is twice the number of pairs inside the radius (nbody_neighbors_within)."""
        n, total = C.c_size_t(0), C.c_uint64(0)
        self._check(lib.nbody_neighbors_within(self._h, float(radius), None, 0, None, 0, C.byref(n), C.byref(total)))   # (counts only)
        offset = np.zeros(n.value + 1, np.uint64)
        neighbor = np.full(total.value, -1, np.int32)
        self._check(lib.nbody_neighbors_within(self._h, float(radius), offset.ctypes.data, n.value, neighbor.ctypes.data if total.value else None,
                                               total.value, C.byref(n), C.byref(total)))
        return offset[: n.value + 1], neighbor[: total.value]

    def density(self, radius: float, kernel: int = KERNEL_CUBIC_SPLINE) -> tuple[np.ndarray, np.ndarray]:
        """(rho [n] f64, count [n] int32): the density at every body from its neighbours within `radius` and the body itself --
        KERNEL_TOP_HAT: their mass over the sphere's volume; KERNEL_CUBIC_SPLINE: the M4 spline with support `radius` -- summed
        in ascending index, and the number of terms (>= 1) (nbody_density)."""
        n = C.c_size_t(0)
        self._check(lib.nbody_density(self._h, float(radius), int(kernel), None, None, 0, C.byref(n)))   # (the bodies)
        rho = np.zeros(n.value, np.float64)
        count = np.zeros(n.value, np.int32)
        self._check(lib.nbody_density(self._h, float(radius), int(kernel), rho.ctypes.data if n.value else None,
                                      count.ctypes.data if n.value else None, n.value, C.byref(n)))
        return rho[: n.value], count[: n.value]

    def density_center(self, radius: float, kernel: int = KERNEL_CUBIC_SPLINE) -> tuple[np.ndarray, float]:
        """(center [3] f64, rho_sum): the density-weighted centre sum rho_i x_i / sum rho_i of Casertano & Hut with density()'s
        rho, summed in moments()' fixed order -- what lagrangian_radii(fractions, center=...) wants (nbody_density_center)."""
        center = (C.c_double * 3)()
        total = C.c_double(0)
        self._check(lib.nbody_density_center(self._h, float(radius), int(kernel), center, C.byref(total)))
        return np.array(center[:], np.float64), float(total.value)

    # -- k nearest neighbours (nbody_knn, nbody_knn_density, nbody_knn_density_center): f64, exact, read-only, on the device
    def knn(self, k: int, radius_hint: float = 0.0) -> tuple[np.ndarray, np.ndarray]:
        """(neighbor [n, k] int32, dist2 [n, k] f64): row i holds the k bodies j != i that come first in the order (unsoftened f64
        squared distance ascending, then index ascending) and those r2, in get_points() order; a row with fewer than k bodies at
        a finite distance is padded with -1 and +inf.  1 <= k <= KNN_MAX_K.  radius_hint (0, or finite and > 0) never changes the
        result: under SEARCH_CELLS the rows that find k bodies closer than the hint are answered from the 27 cells around them,
        the others by the all-pairs pass -- knn_stats() says how many of each (nbody_knn)."""
        n = C.c_size_t(0)
        self._check(lib.nbody_knn(self._h, int(k), float(radius_hint), None, None, 0, C.byref(n), None))   # (counts only)
        neighbor = np.full((n.value, int(k)), -1, np.int32)
        dist2 = np.full((n.value, int(k)), np.inf, np.float64)
        stats = (C.c_uint64 * 2)()
        self._check(lib.nbody_knn(self._h, int(k), float(radius_hint), neighbor.ctypes.data if n.value else None,
                                  dist2.ctypes.data if n.value else None, n.value, C.byref(n), stats))
        self._knn_stats = (int(stats[0]), int(stats[1]))
        return neighbor[: n.value], dist2[: n.value]

    def knn_stats(self) -> tuple[int, int]:
        """(rows answered from the cells, rows answered by the all-pairs pass) of this object's last knn() call; (0, 0) before
        the first (the `stats` of nbody_knn)."""
        return getattr(self, "_knn_stats", (0, 0))

    def knn_density(self, k: int, radius_hint: float = 0.0) -> tuple[np.ndarray, np.ndarray]:
        """(rho [n] f64, rk2 [n] f64): Casertano & Hut's density at every body from its k nearest neighbours (k >= 2) -- the mass
        of the first k - 1, summed in list order, over the volume of the sphere that reaches the k-th -- and the squared distance
        to the k-th; +0.0 and +inf for a body with fewer than k neighbours (nbody_knn_density)."""
        n = C.c_size_t(0)
        self._check(lib.nbody_knn_density(self._h, int(k), float(radius_hint), None, None, 0, C.byref(n)))   # (the bodies)
        rho = np.zeros(n.value, np.float64)
        rk2 = np.full(n.value, np.inf, np.float64)
        self._check(lib.nbody_knn_density(self._h, int(k), float(radius_hint), rho.ctypes.data if n.value else None,
                                          rk2.ctypes.data if n.value else None, n.value, C.byref(n)))
        return rho[: n.value], rk2[: n.value]

    def knn_density_center(self, k: int, radius_hint: float = 0.0) -> tuple[np.ndarray, float]:
        """(center [3] f64, rho_sum): the density-weighted centre sum rho_i x_i / sum rho_i of Casertano & Hut with knn_density()'s
        rho, summed in moments()' fixed order -- what lagrangian_radii(fractions, center=...) wants (nbody_knn_density_center)."""
        center = (C.c_double * 3)()
        total = C.c_double(0)
        self._check(lib.nbody_knn_density_center(self._h, int(k), float(radius_hint), center, C.byref(total)))
        return np.array(center[:], np.float64), float(total.value)

    # -- pair-separation counts (nbody_pair_counts, nbody_pair_counts_at): integers, read-only, on the device
    def pair_counts(self, edges) -> tuple[np.ndarray, np.ndarray]:
        """(counts [n_bins] uint64, outside [2] uint64): the unordered pairs i < j of bodies whose unsoftened f64 squared
        separation r2 has edges[b]**2 <= r2 < edges[b + 1]**2; outside = the pairs below edges[0]**2 and everything else
        (beyond the last edge, or not finite).  counts.sum() + outside.sum() == n (n - 1) / 2.  Honours pair_search
        (nbody_pair_counts)."""
        edges = np.ascontiguousarray(edges, np.float64).reshape(-1)
        n_bins = len(edges) - 1
        counts = np.zeros(max(n_bins, 0), np.uint64)
        outside = np.zeros(2, np.uint64)
        self._check(lib.nbody_pair_counts(self._h, edges.ctypes.data, n_bins, counts.ctypes.data, outside.ctypes.data))
        return counts, outside

    def pair_counts_at(self, points, edges) -> tuple[np.ndarray, np.ndarray]:
        """(counts [n_bins] uint64, outside [2] uint64): the same over every (body, point) pair, d = point - body, for points
        [m][3] f64; always over all pairs.  counts.sum() + outside.sum() == n m (nbody_pair_counts_at)."""
        points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        edges = np.ascontiguousarray(edges, np.float64).reshape(-1)
        n_bins = len(edges) - 1
        counts = np.zeros(max(n_bins, 0), np.uint64)
        outside = np.zeros(2, np.uint64)
        self._check(lib.nbody_pair_counts_at(self._h, points.ctypes.data if len(points) else None, len(points), edges.ctypes.data, n_bins,
                                             counts.ctypes.data, outside.ctypes.data))
        return counts, outside

    # -- grid deposit (nbody_deposit): the bodies assigned to a regular grid in 64-bit fixed point, read-only, on the device
    def deposit(self, origin, spacing, dims, scheme=DEPOSIT_CIC, quantity=DEPOSIT_MASS, periodic=False, project_axis=-1) -> tuple[np.ndarray, np.ndarray]:
        """(grid [nx, ny, nz] f64, counts [4] uint64 = inside, partial, outside, skipped): the bodies' quantity (DEPOSIT_MASS,
        DEPOSIT_MOMENTUM_X/Y/Z, DEPOSIT_MV2, DEPOSIT_NUMBER) assigned to the cells of edge `spacing` from the low corner `origin`
        by DEPOSIT_NGP, DEPOSIT_CIC or DEPOSIT_TSC; periodic wraps every axis, else what falls off the grid is dropped;
        project_axis = 0, 1 or 2 ignores that axis (dims there must be 1): a column map.  The same state gives the same bits
        (nbody_deposit)."""
        spec = grid_spec(origin, spacing, dims, scheme, quantity, periodic, project_axis)
        grid = np.zeros(tuple(max(int(v), 0) for v in dims), np.float64)
        counts = np.zeros(4, np.uint64)
        self._check(lib.nbody_deposit(self._h, C.byref(spec), grid.ctypes.data if grid.size else None, grid.size, counts.ctypes.data))
        return grid, counts

    def deposit_stats(self) -> np.ndarray:
        """[4] uint64: {1 once a deposit reached the device, the last one's plan (deposit_sort | deposit_combine << 1 |
        deposit_lds << 2), its terms on the grid, the 64-bit atomics it sent to global memory} (nbody_deposit_stats)."""
        out = (C.c_uint64 * 4)()
        self._check(lib.nbody_deposit_stats(self._h, out))
        return np.array(out[:], np.uint64)

    # -- grid sample (nbody_grid_sample, nbody_grid_sample_at): a grid read back with the deposit's weights, read-only, on the device
    def grid_sample(self, grid, origin, spacing, scheme=DEPOSIT_CIC, op=SAMPLE_VALUE, periodic=False, project_axis=-1,
                    points=None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(out [n, fields] or [n, 3] f64, cls [n] uint8, counts [4] uint64 = inside, partial, outside, skipped): the grid ([nx,
        ny, nz] or [fields, nx, ny, nz], cells of edge `spacing` from the low corner `origin`) read back at the bodies, in
        get_points() order, or at points [n][3], with the weights of DEPOSIT_NGP, DEPOSIT_CIC or DEPOSIT_TSC -- the transpose of
        deposit().  SAMPLE_VALUE: the fields' values; SAMPLE_GRADIENT2 / SAMPLE_GRADIENT4: +grad of one field by central
        differences of order 2 / 4.  The same input gives the same bits as host_grid_sample (nbody_grid_sample,
        nbody_grid_sample_at)."""
        g, fields, spec, width = _sample_grid(grid, origin, spacing, scheme, op, periodic, project_axis)
        counts = np.zeros(4, np.uint64)
        if points is not None:
            xyz = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
            n = len(xyz)
            out = np.zeros((n, width), np.float64)
            cls = np.zeros(n, np.uint8)
            self._check(lib.nbody_grid_sample_at(self._h, C.byref(spec), g.ctypes.data if g.size else None, fields, int(op),
                                                 xyz.ctypes.data if n else None, n, out.ctypes.data if out.size else None,
                                                 cls.ctypes.data if n else None, counts.ctypes.data))
            return out, cls, counts
        # (sized from the capacity, not from nbody_count, which would refresh the host's view of the body count: potentials())
        cfg = NbodyConfig()
        self._check(lib.nbody_get_config(self._h, C.byref(cfg)))
        cap = max(int(cfg.capacity), 1)
        out = np.zeros((cap, width), np.float64)
        cls = np.zeros(cap, np.uint8)
        n = C.c_size_t(0)
        self._check(lib.nbody_grid_sample(self._h, C.byref(spec), g.ctypes.data if g.size else None, fields, int(op), out.ctypes.data,
                                          cls.ctypes.data, cap, C.byref(n), counts.ctypes.data))
        return out[: n.value], cls[: n.value], counts

    def grid_sample_stats(self) -> np.ndarray:
        """[4] uint64: {1 once a grid sample reached the device, the plan the last one used (sample_sort | sample_pregrad << 1),
        the grid reads its sample kernel issued, 0} (nbody_grid_sample_stats)."""
        out = (C.c_uint64 * 4)()
        self._check(lib.nbody_grid_sample_stats(self._h, out))
        return np.array(out[:], np.uint64)

    # -- grid Poisson (nbody_grid_poisson): the potential of a mass grid by the library's own f64 FFT, read-only, on the device
    def grid_poisson(self, mass, spacing, g, periodic=False, green=POISSON_SPECTRAL, soften=0.0, deconvolve=0, scheme=DEPOSIT_CIC) -> np.ndarray:
        """phi [nx, ny, nz] f64 at the cell centres from the mass per cell [nx, ny, nz] (what deposit() returns for DEPOSIT_MASS;
        powers of two).  periodic: green = POISSON_SPECTRAL or POISSON_DIFF2, deconvolve = 0, 1 or 2 powers of the scheme's
        window; isolated: zero padding, soften >= 0.  grid_sample(phi, ..., op=SAMPLE_GRADIENT2) then gives +grad phi.  The
        handle lends its stream and its memory only.  The same input gives the same bits as host_grid_poisson
        (nbody_grid_poisson)."""
        m, spec, ps = _poisson_call(mass, spacing, g, periodic, green, soften, deconvolve, scheme)
        phi = np.zeros(m.shape, np.float64)
        self._check(lib.nbody_grid_poisson(self._h, C.byref(spec), C.byref(ps), m.ctypes.data if m.size else None,
                                           phi.ctypes.data if phi.size else None, phi.size))
        return phi

    def grid_poisson_stats(self) -> np.ndarray:
        """[4] uint64: {1 once a grid Poisson solve reached the device, the plan the last one used (poisson_lds | poisson_tile
        << 1), its butterfly launches, the complex points it transformed} (nbody_grid_poisson_stats)."""
        out = (C.c_uint64 * 4)()
        self._check(lib.nbody_grid_poisson_stats(self._h, out))
        return np.array(out[:], np.uint64)

    # -- particle-mesh field (nbody_pm_field, nbody_pm_field_at): deposit, solve and sample in one call, the grid never leaves the device
    def pm_field(self, origin, spacing, dims, g, scheme=DEPOSIT_CIC, gradient=SAMPLE_GRADIENT2, periodic=False, green=POISSON_SPECTRAL,
                 soften=0.0, deconvolve=0, project_axis=-1, points=None, phi=True) -> tuple[np.ndarray, np.ndarray | None, np.ndarray, np.ndarray]:
        """(acc [n, 3] f64, phi [n] f64 | None, cls [n] uint8, counts [8] uint64 = the deposit's four and the gradient sample's
        four): the mesh acceleration -grad phi and the potential of the handle's bodies -- deposit(DEPOSIT_MASS), grid_poisson and
        grid_sample(gradient) composed on the device -- at the bodies, in get_points() order, or at points [n][3].  The same
        bits as host_pm_field, whatever the plan (nbody_pm_field, nbody_pm_field_at)."""
        spec = grid_spec(origin, spacing, dims, scheme, DEPOSIT_MASS, periodic, project_axis)
        pm = pm_spec(g, gradient, green, soften, deconvolve)
        counts = np.zeros(8, np.uint64)
        if points is not None:
            xyz = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
            n = len(xyz)
            acc = np.zeros((n, 3), np.float64)
            val = np.zeros(n, np.float64) if phi else None
            cls = np.zeros(n, np.uint8)
            self._check(lib.nbody_pm_field_at(self._h, C.byref(spec), C.byref(pm), xyz.ctypes.data if n else None, n, acc.ctypes.data if n else None,
                                              val.ctypes.data if phi and n else None, cls.ctypes.data if n else None, counts.ctypes.data))
            return acc, val, cls, counts
        # (sized from the capacity, not from nbody_count, which would refresh the host's view of the body count: potentials())
        cfg = NbodyConfig()
        self._check(lib.nbody_get_config(self._h, C.byref(cfg)))
        cap = max(int(cfg.capacity), 1)
        acc = np.zeros((cap, 3), np.float64)
        val = np.zeros(cap, np.float64) if phi else None
        cls = np.zeros(cap, np.uint8)
        n = C.c_size_t(0)
        self._check(lib.nbody_pm_field(self._h, C.byref(spec), C.byref(pm), acc.ctypes.data, val.ctypes.data if phi else None, cls.ctypes.data, cap,
                                       C.byref(n), counts.ctypes.data))
        return acc[: n.value], None if val is None else val[: n.value], cls[: n.value], counts

    def pm_field_stats(self) -> np.ndarray:
        """[4] uint64: {1 once a particle-mesh call reached the device, the plan the last one used (pm_gather | pm_share_sort << 1),
        the grid reads of its gather, the radix sorts it enqueued} (nbody_pm_field_stats)."""
        out = (C.c_uint64 * 4)()
        self._check(lib.nbody_pm_field_stats(self._h, out))
        return np.array(out[:], np.uint64)

    # -- P3M field (nbody_p3m_field, nbody_p3m_field_at): the mesh field with a Gaussian split plus the short-range pair sum
    def p3m_field(self, origin, spacing, dims, g, r_split, r_cut, scheme=DEPOSIT_CIC, gradient=SAMPLE_GRADIENT2, green=POISSON_SPECTRAL,
                  deconvolve=0, soften=0.0, terms=P3M_BOTH, points=None, phi=True) -> tuple[np.ndarray, np.ndarray | None, np.ndarray, np.ndarray]:
        """(acc [n, 3] f64, phi [n] f64 | None, cls [n] uint8, counts [8] uint64): the P3M field of the handle's bodies on a periodic
        grid, at the bodies, in get_points() order, or at points [n][3].  The same bits as host_p3m_field, whatever the plan
        (nbody_p3m_field, nbody_p3m_field_at)."""
        spec = grid_spec(origin, spacing, dims, scheme, DEPOSIT_MASS, True, -1)
        p3m = p3m_spec(g, r_split, r_cut, gradient, green, deconvolve, soften, terms)
        counts = np.zeros(8, np.uint64)
        if points is not None:
            xyz = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
            n = len(xyz)
            acc = np.zeros((n, 3), np.float64)
            val = np.zeros(n, np.float64) if phi else None
            cls = np.zeros(n, np.uint8)
            self._check(lib.nbody_p3m_field_at(self._h, C.byref(spec), C.byref(p3m), xyz.ctypes.data if n else None, n, acc.ctypes.data if n else None,
                                               val.ctypes.data if phi and n else None, cls.ctypes.data if n else None, counts.ctypes.data))
            return acc, val, cls, counts
        # (sized from the capacity, not from nbody_count, which would refresh the host's view of the body count: potentials())
        cfg = NbodyConfig()
        self._check(lib.nbody_get_config(self._h, C.byref(cfg)))
        cap = max(int(cfg.capacity), 1)
        acc = np.zeros((cap, 3), np.float64)
        val = np.zeros(cap, np.float64) if phi else None
        cls = np.zeros(cap, np.uint8)
        n = C.c_size_t(0)
        self._check(lib.nbody_p3m_field(self._h, C.byref(spec), C.byref(p3m), acc.ctypes.data, val.ctypes.data if phi else None, cls.ctypes.data, cap,
                                        C.byref(n), counts.ctypes.data))
        return acc[: n.value], None if val is None else val[: n.value], cls[: n.value], counts

    def p3m_field_stats(self) -> np.ndarray:
        """[4] uint64: {1 once a P3M call reached the device, the plan the last one used (p3m_lds | pm_field_stats's plan word << 1),
        the partners its pair sum looked at, the terms with r2 < R2} (nbody_p3m_field_stats)."""
        out = (C.c_uint64 * 4)()
        self._check(lib.nbody_p3m_field_stats(self._h, out))
        return np.array(out[:], np.uint64)

    # -- mesh gravity (nbody_set_mesh_gravity): the particle-mesh field as the self-gravity of every step and of update_forces
    @property
    def mesh_gravity(self):
        """None while mesh gravity is off, else the (GridSpec, NbodyPmSpec) pair as set.  Set it from such a pair or from a dict of
        pm_field's keywords (origin, spacing, dims and, optionally, g, scheme, gradient, periodic, green, soften, deconvolve,
        project_axis); None clears it.  While set, the self-gravity pass of steps and of update_forces is the mesh field of
        pm_field with g := the handle's g, rounded once to the handle's dtype; no pair kernel runs.  clone() carries it."""
        spec, pm, on = GridSpec(), NbodyPmSpec(), C.c_int(0)
        self._check(lib.nbody_get_mesh_gravity(self._h, C.byref(spec), C.byref(pm), C.byref(on)))
        return (spec, pm) if on.value else None

    @mesh_gravity.setter
    def mesh_gravity(self, value):
        if value is None:
            self._check(lib.nbody_set_mesh_gravity(self._h, None, None))
            return
        spec, pm = mesh_gravity_specs(value)
        self._check(lib.nbody_set_mesh_gravity(self._h, C.byref(spec), C.byref(pm)))

    def mesh_gravity_stats(self) -> np.ndarray:
        """[4] uint64: {mesh passes enqueued, the plan the last one used (mesh_kick_fuse | mesh_keep_kernel << 1 | pm_field_stats's
        plan word << 2), 3-D transforms enqueued in total, allocations of the resident mesh state} (nbody_mesh_gravity_stats)."""
        out = (C.c_uint64 * 4)()
        self._check(lib.nbody_mesh_gravity_stats(self._h, out))
        return np.array(out[:], np.uint64)

    # -- pair search (nbody_set_pair_search): all pairs, or the 27 cells around a body's own; the results are the same bits
    @property
    def pair_search(self) -> int:
        """How fof_labels, fof_groups, contacts, merge_contacts, neighbors_within, density, density_center and pair_counts find their pairs: SEARCH_ALL_PAIRS (0, the default) or
        SEARCH_CELLS (1: bodies sorted by the cell of a uniform grid).  It changes no result; clone() carries it."""
        v = C.c_int(0)
        self._check(lib.nbody_get_pair_search(self._h, C.byref(v)))
        return int(v.value)

    @pair_search.setter
    def pair_search(self, mode: int):
        self._check(lib.nbody_set_pair_search(self._h, int(mode)))

    def pair_search_stats(self) -> tuple[int, int, int, int]:
        """(1 if the last fixed-radius call ran the cell search else 0, bodies gridded, occupied cells, candidate pairs)
        (nbody_pair_search_stats)."""
        out = (C.c_uint64 * 4)()
        self._check(lib.nbody_pair_search_stats(self._h, out))
        return tuple(int(v) for v in out)

    def __len__(self) -> int:
        n = C.c_size_t(0)
        self._check(lib.nbody_count(self._h, C.byref(n)))
        return int(n.value)

    def count_global(self) -> int:
        n = C.c_size_t(0)
        self._check(lib.nbody_count_global(self._h, C.byref(n)))
        return int(n.value)

    def elapsed(self) -> float:
        if self.f64:
            d = C.c_double(0)
            self._check(lib.nbody_elapsed_f64(self._h, C.byref(d)))
            return float(d.value)
        v = C.c_float(0)
        self._check(lib.nbody_elapsed(self._h, C.byref(v)))
        return float(v.value)

    @property
    def settings(self) -> Settings:
        if self.f64:
            g, e, dt, t2 = C.c_double(), C.c_double(), C.c_double(), C.c_double()
            self._check(lib.nbody_get_settings_f64(self._h, C.byref(g), C.byref(e), C.byref(dt), C.byref(t2)))
            return Settings(g.value, e.value, dt.value, t2.value)
        g, e, dt, t2 = C.c_float(), C.c_float(), C.c_float(), C.c_float()
        self._check(lib.nbody_get_settings(self._h, C.byref(g), C.byref(e), C.byref(dt), C.byref(t2)))
        return Settings(g.value, e.value, dt.value, t2.value)

    @settings.setter
    def settings(self, s: Settings):
        if self.f64:
            self._check(lib.nbody_set_settings_f64(self._h, float(s.g), float(s.g_soft), float(s.dt), float(s.theta2)))
        else:
            self._check(lib.nbody_set_settings(self._h, float(s.g), float(s.g_soft), float(s.dt), float(s.theta2)))

    def set_bounds(self, center, width: float):
        if self.f64:
            self._check(lib.nbody_set_bounds_f64(self._h, (C.c_double * 3)(*[float(x) for x in center]), float(width)))
        else:
            self._check(lib.nbody_set_bounds(self._h, (C.c_float * 3)(*[float(x) for x in center]), float(width)))

    @property
    def config(self) -> dict:
        """The configuration the handle runs with (nbody_get_config): tree_build after TREE_AUTO, math_mode as it runs."""
        cfg = NbodyConfig()
        self._check(lib.nbody_get_config(self._h, C.byref(cfg)))
        return {name: getattr(cfg, name) for name, _ in NbodyConfig._fields_}

    def clone(self) -> "Simulation":
        h = _H()
        rc = lib.nbody_clone(self._h, C.byref(h))
        if rc:
            raise NbodyError(rc, (lib.nbody_last_error(None) or b"").decode())
        twin = Simulation(None, rank=self.rank, world_size=self.world_size, _handle=h, _f64=self.f64)
        twin.dtype = self.dtype
        return twin

    # -- diagnostics / multi-GPU
    def sync(self):
        self._check(lib.nbody_sync(self._h))

    def set_profiling(self, on):
        """False / True: HIP events around every force-kernel launch; an int k > 1: around every k-th."""
        self._check(lib.nbody_set_profiling(self._h, int(on)))

    def stats(self) -> NbodyStats:
        s = NbodyStats()
        self._check(lib.nbody_stats(self._h, C.byref(s)))
        return s

    def reset_stats(self):
        self._check(lib.nbody_reset_stats(self._h))

    def energy(self) -> tuple[float, float]:
        ke, pe = C.c_double(), C.c_double()
        self._check(lib.nbody_energy(self._h, C.byref(ke), C.byref(pe)))
        return float(ke.value), float(pe.value)

    def potentials(self, mode: int = POTENTIAL_PAIRS) -> tuple[np.ndarray, tuple[int, int]]:
        """(phi [n] f64 of this rank's bodies in get_points() order, (terms summed, opening tests)) at the current positions;
        collective on a multi-rank world.  POTENTIAL_TREE: Barnes-Hut handles, O(N log N).  POTENTIAL_TREE_QUADRUPOLE: the
        same walk with the accepted internal cells' quadrupole terms (f32 single-shard Barnes-Hut handles)."""
        # (sized from the capacity, not from nbody_count: that call refreshes the host's view of the body count, which a chain
        # of steps enqueued without read-back sizes its launches from -- nbody_potentials itself leaves the view as it was)
        cfg = NbodyConfig()
        self._check(lib.nbody_get_config(self._h, C.byref(cfg)))
        n = C.c_size_t(0)
        phi = np.zeros(max(int(cfg.capacity), 1), np.float64)
        counts = (C.c_uint64 * 2)()
        self._check(lib.nbody_potentials(self._h, int(mode), phi.ctypes.data, len(phi), C.byref(n), counts))
        return phi[: n.value], (int(counts[0]), int(counts[1]))

    def field_at(self, points, mode: int = POTENTIAL_PAIRS, acc: bool = True, phi: bool = True):
        """(acc [M, 3] f64 | None, phi [M] f64 | None, (terms summed, opening tests)) of ALL bodies of the world at the M
        given points (any array-like [M, 3]), at the current positions; collective on a multi-rank world.  An f32 handle
        evaluates at the points rounded to f32.  mode: POTENTIAL_PAIRS, POTENTIAL_TREE, or POTENTIAL_TREE_QUADRUPOLE (the tree
        sum with the accepted internal cells' quadrupole terms: f32 single-shard Barnes-Hut handles)."""
        xyz = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
        m = len(xyz)
        a = np.zeros((m, 3), np.float64) if acc else None
        p = np.zeros(m, np.float64) if phi else None
        counts = (C.c_uint64 * 2)()
        self._check(lib.nbody_field_at(self._h, int(mode), xyz.ctypes.data if m else None, m, a.ctypes.data if acc else None,
                                       p.ctypes.data if phi else None, counts))
        return a, p, (int(counts[0]), int(counts[1]))

    def tidal_at(self, points, mode: int = POTENTIAL_PAIRS, counts: bool = False):
        """The tidal tensor d acc_a / d x_b of ALL bodies of the world at the M given points (any array-like [M, 3]), at the
        current positions: [M, 6] f64 rows {xx, xy, xz, yy, yz, zz} (tidal_matrices() expands them); counts=True: (rows,
        (terms summed, opening tests)).  Self-gravity only; collective on a multi-rank world.  An f32 handle evaluates at the
        points rounded to f32.  mode: POTENTIAL_PAIRS or POTENTIAL_TREE (monopole terms over field_at's tree and tests)."""
        xyz = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
        m = len(xyz)
        t6 = np.zeros((m, 6), np.float64)
        c = (C.c_uint64 * 2)()
        self._check(lib.nbody_tidal_at(self._h, int(mode), xyz.ctypes.data if m else None, m, t6.ctypes.data, c))
        return (t6, (int(c[0]), int(c[1]))) if counts else t6

    def energy_world(self, mode: int = POTENTIAL_PAIRS) -> tuple[float, float]:
        """(KE, PE) of the whole world, the same on every rank; collective.  mode as potentials(): POTENTIAL_TREE_QUADRUPOLE
        builds PE from the potentials with quadrupole terms."""
        ke, pe = C.c_double(), C.c_double()
        self._check(lib.nbody_energy_world(self._h, int(mode), C.byref(ke), C.byref(pe)))
        return float(ke.value), float(pe.value)

    def tree(self):
        n = C.c_size_t(0)
        export = lib.nbody_tree_export_f64 if self.f64 else lib.nbody_tree_export
        ft = np.float64 if self.f64 else np.float32
        self._check(export(self._h, None, None, None, 0, C.byref(n)))
        m = n.value
        com = np.zeros((m, 4), ft)
        w = np.zeros(m, ft)
        skip = np.zeros(m, np.int32)
        self._check(export(self._h, com.ctypes.data, w.ctypes.data, skip.ctypes.data, m, C.byref(n)))
        return dict(com_mass=com, width=w, skip=skip)

    @property
    def multipole(self) -> int:
        """Order of the Barnes-Hut force walk's expansion: MULTIPOLE_MONOPOLE (1, the default) or MULTIPOLE_QUADRUPOLE (2:
        f32 fast-math single-shard Barnes-Hut handles only).  Takes effect at the next force pass; clone() carries it."""
        v = C.c_int(0)
        self._check(lib.nbody_get_multipole(self._h, C.byref(v)))
        return int(v.value)

    @multipole.setter
    def multipole(self, order: int):
        self._check(lib.nbody_set_multipole(self._h, int(order)))

    @property
    def integrator(self) -> int:
        """LEAPFROG (0, the default) or HERMITE4 (1: brute-force f64 handles of a one-rank world only): what step(), steps()
        and step_by() advance the bodies with.  clone() carries it."""
        v = C.c_int(0)
        self._check(lib.nbody_get_integrator(self._h, C.byref(v)))
        return int(v.value)

    @integrator.setter
    def integrator(self, which: int):
        self._check(lib.nbody_set_integrator(self._h, int(which)))

    def jerk(self) -> np.ndarray:
        """[n, 3] f64: the jerk a Hermite handle holds, in get_points() order (nbody_download_jerk).  Refused on a leapfrog
        handle and while the held acceleration and jerk are stale (after upload, add_point, remove_point, a settings change,
        init() or a change of integrator, until the next step, update_forces() or suggest_dt())."""
        cfg = NbodyConfig()
        self._check(lib.nbody_get_config(self._h, C.byref(cfg)))
        n = C.c_size_t(0)
        out = np.zeros((max(int(cfg.capacity), 1), 3), np.float64)
        self._check(lib.nbody_download_jerk(self._h, out.ctypes.data, len(out), C.byref(n)))
        return out[: n.value]

    def suggest_dt(self, eta: float) -> float:
        """eta * min_i |a_i| / |j_i| of a Hermite handle (nbody_suggest_dt): +inf when no body has a jerk."""
        d = C.c_double(0)
        self._check(lib.nbody_suggest_dt(self._h, float(eta), C.byref(d)))
        return float(d.value)

    @property
    def block_steps(self) -> tuple[float, int]:
        """(eta, max_level) of a Hermite handle's block individual time steps (nbody_set_block_steps); (0.0, 0): off, the
        default.  With them on, step_by(dt) is a macro step of 2**max_level ticks in which body i advances by dt * 2**-level_i
        and only the due bodies are evaluated; steps() then synchronises with the host.  clone() carries the setting."""
        eta, lv = C.c_double(0), C.c_int(0)
        rc = lib.nbody_get_block_steps(self._h, C.byref(eta), C.byref(lv))
        if rc:
            raise NbodyError(rc, "nbody_get_block_steps: the handle runs the leapfrog integrator (nbody_set_integrator)")
        return float(eta.value), int(lv.value)

    @block_steps.setter
    def block_steps(self, eta_levels):
        eta, levels = eta_levels
        self._check(lib.nbody_set_block_steps(self._h, float(eta), int(levels)))

    def levels(self) -> np.ndarray:
        """[n] i32: the block-step level of every body, in get_points() order (nbody_download_levels).  Refused while the
        levels are invalid: until the first macro step or update_forces() after whatever made them so."""
        cfg = NbodyConfig()
        self._check(lib.nbody_get_config(self._h, C.byref(cfg)))
        n = C.c_size_t(0)
        out = np.zeros(max(int(cfg.capacity), 1), np.int32)
        self._check(lib.nbody_download_levels(self._h, out.ctypes.data, len(out), C.byref(n)))
        return out[: n.value]

    def block_step_counts(self) -> tuple[int, int]:
        """(block steps, body updates) since reset_stats() (nbody_block_step_counts)."""
        out = (C.c_uint64 * 2)()
        self._check(lib.nbody_block_step_counts(self._h, out))
        return int(out[0]), int(out[1])

    def hermite_forces_of(self, ids) -> tuple[np.ndarray, np.ndarray]:
        """Test hook (nbody_debug_hermite_forces_of): (a [k, 3], j [k, 3]) f64 of the listed bodies at the current state,
        through the active-set kernels."""
        ids = np.ascontiguousarray(ids, np.int32)
        a, j = np.zeros((len(ids), 3), np.float64), np.zeros((len(ids), 3), np.float64)
        self._check(lib.nbody_debug_hermite_forces_of(self._h, ids.ctypes.data, len(ids), a.ctypes.data, j.ctypes.data))
        return a, j

    def tree_quadrupoles(self) -> np.ndarray:
        """[n_nodes, 6] f32 {xx, xy, xz, yy, yz, zz} of every node of the tree tree() reports (nbody_tree_export_quadrupoles):
        only after a force pass that walked with quadrupoles, or a potentials / field_at / energy_world call in
        POTENTIAL_TREE_QUADRUPOLE that built the tree."""
        n = C.c_size_t(0)
        self._check(lib.nbody_tree_export_quadrupoles(self._h, None, 0, C.byref(n)))
        q = np.zeros((n.value, 6), np.float32)
        self._check(lib.nbody_tree_export_quadrupoles(self._h, q.ctypes.data, n.value, C.byref(n)))
        return q

    def tree_cells(self):
        """(min_max [n, 6] f32, depth [n] i32) of every node of the last tree, pre-order: what the reference's renderer draws."""
        n = C.c_size_t(0)
        self._check(lib.nbody_tree_export_cells(self._h, None, None, 0, C.byref(n)))
        mm = np.zeros((n.value, 6), np.float32)
        depth = np.zeros(n.value, np.int32)
        self._check(lib.nbody_tree_export_cells(self._h, mm.ctypes.data, depth.ctypes.data, n.value, C.byref(n)))
        return mm, depth

    def download_ids(self) -> np.ndarray:
        """NBODY_SHARD_SPATIAL: index in the uploaded vector of every body get_points() returns, in the same order."""
        n = C.c_size_t(0)
        self._check(lib.nbody_count(self._h, C.byref(n)))
        ids = np.zeros(n.value, np.int32)
        self._check(lib.nbody_download_ids(self._h, ids.ctypes.data, n.value, C.byref(n)))
        return ids[: n.value]

    def let_stats(self) -> NbodyLetStats:
        s = NbodyLetStats()
        self._check(lib.nbody_let_stats(self._h, C.byref(s)))
        return s

    def let_bounds(self) -> np.ndarray:
        """NBODY_SHARD_SPATIAL: the key-range bounds the next classification uses ([world_size + 1] uint64)."""
        out = np.zeros(self.world_size + 1, np.uint64)
        self._check(lib.nbody_debug_let_bounds(self._h, out.ctypes.data))
        return out

    def set_balance(self, by_work: bool):
        """NBODY_SHARD_SPATIAL: redraw the bounds at the quantiles of the last walk's visit counts (default) or of the body count."""
        self._check(lib.nbody_debug_let_set_balance(self._h, int(bool(by_work))))

    def let_held(self) -> dict:
        """NBODY_SHARD_SPATIAL test hook (nbody_debug_let_export_held): the node array this rank's last force pass walked, in the
        walk's order.  `com_mass` [m, 4] f32, `width` [m] f32, `skip` [m] i32 (positions in this array: what oracle.bh_walk_list
        follows), `global_index` [m] i32, `leaf` [m] bool, `origin` [m] i32 (0 slice, 1 import, 2 own spanning cell, 3 imported
        spanning cell)."""
        n = C.c_size_t(0)
        self._check(lib.nbody_debug_let_export_held(self._h, None, None, None, None, None, None, 0, C.byref(n)))
        m = n.value
        com, width = np.zeros((m, 4), np.float32), np.zeros(m, np.float32)
        skip, gi, leaf, origin = (np.zeros(m, np.int32) for _ in range(4))
        self._check(lib.nbody_debug_let_export_held(self._h, com.ctypes.data, width.ctypes.data, skip.ctypes.data, gi.ctypes.data,
                                                    leaf.ctypes.data, origin.ctypes.data, m, C.byref(n)))
        return dict(com_mass=com, width=width, skip=skip, global_index=gi, leaf=leaf.astype(bool), origin=origin)

    def set_prune(self, on: bool):
        self._check(lib.nbody_debug_let_set_prune(self._h, int(bool(on))))

    def local_range(self) -> tuple[int, int]:
        a, b = C.c_size_t(0), C.c_size_t(0)
        self._check(lib.nbody_local_range(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def comm_init(self, id_bytes: bytes):
        buf = C.create_string_buffer(bytes(id_bytes), COMM_ID_BYTES)
        self._check(lib.nbody_comm_init(self._h, buf))

    def set_tuning(self, name: str, value: int):
        """One launch-shape / scheme knob of this handle (include/nbody_hip.h nbody_set_tuning)."""
        self._check(lib.nbody_set_tuning(self._h, name.encode(), int(value)))

    def get_tuning(self, name: str) -> int:
        v = C.c_int(0)
        self._check(lib.nbody_get_tuning(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    def comm_transport(self) -> str:
        buf = C.create_string_buffer(16)
        self._check(lib.nbody_comm_transport(self._h, buf, 16))
        return buf.value.decode()


def sharded_step(sims: list, dt: float | None = None):
    """One step of a world of len(sims) shards living in this process (test harness: what the RCCL
    all-gather of positions and the send/recv round of partial sums perform is done with
    device-to-device copies)."""
    dts = [float(s.settings.dt if dt is None else dt) for s in sims]
    for s, d in zip(sims, dts):
        s._check(lib.nbody_debug_step_begin(s._h, d))
    for s in sims:
        for peer in sims:
            if peer is not s:
                s._check(lib.nbody_debug_import_segment(s._h, peer._h))
    for s, d in zip(sims, dts):
        s._check(lib.nbody_debug_step_forces(s._h, d))
    for s in sims:
        for peer in sims:
            if peer is not s:
                s._check(lib.nbody_debug_import_partials(s._h, peer._h))
    for s, d in zip(sims, dts):
        s._check(lib.nbody_debug_step_end(s._h, d))


def spatial_step(sims: list, dt: float | None = None, forces_only: bool = False):
    """One step (or, forces_only, one update_forces) of a world of len(sims) NBODY_SHARD_SPATIAL handles living in this
    process: the five phases of nbody_let.cpp with the four RCCL exchanges done as device-to-device copies."""
    dts = [float(s.settings.dt if dt is None else dt) for s in sims]
    first, last = (10, 14) if forces_only else (0, 4)
    for phase in (first, 1, 2, 3, last):
        for s, d in zip(sims, dts):
            s._check(lib.nbody_debug_let_phase(s._h, phase, d))
        if phase == last:
            break
        which = {first: 0, 1: 1, 2: 2, 3: 3}[phase]
        for s in sims:
            for peer in sims:
                if peer is not s:
                    s._check(lib.nbody_debug_let_exchange(s._h, peer._h, which))


def spatial_gather(sims: list, n: int):
    """The world's bodies back in the uploaded vector's order: (records, indices that survived)."""
    parts, ids = [], []
    for s in sims:
        parts.append(s.get_points())
        ids.append(s.download_ids())
    rec = np.concatenate(parts)
    idx = np.concatenate(ids)
    order = np.argsort(idx, kind="stable")
    return rec[order], idx[order]


def host_cross_plan(rank: int, world: int, seg_cap: int, n_own: int) -> dict:
    """Host-only: the plan of the symmetric scheme across shards for one rank."""
    ipt, a, npart, nrecv = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    parts = np.zeros((8, 5), np.int32)
    recv = np.zeros(8, np.int32)
    rc = lib.nbody_host_cross_plan(rank, world, seg_cap, n_own, C.byref(ipt), C.byref(a), C.byref(npart),
                                   parts.ctypes.data, C.byref(nrecv), recv.ctypes.data)
    if rc:
        raise NbodyError(rc, "nbody_host_cross_plan")
    return dict(ipt=ipt.value, n_sets=a.value, parts=parts[: npart.value].copy(), recv_from=recv[: nrecv.value].copy())


def host_exchange_layout(matrix: np.ndarray, rank: int, clamp: int, packed_send: bool, send_stride: int = 0) -> dict:
    """Host-only: message offsets and counts of a variable-size round of the spatial step, for one rank."""
    m = np.ascontiguousarray(matrix, dtype=np.int32)
    G = m.shape[0]
    arr = {k: np.zeros(G, np.uint64) for k in ("out_at", "n_out", "in_at", "n_in")}
    tot = C.c_size_t(0)
    rc = lib.nbody_host_exchange_layout(m.ctypes.data, G, rank, int(clamp), int(bool(packed_send)), int(send_stride), arr["out_at"].ctypes.data,
                                        arr["n_out"].ctypes.data, arr["in_at"].ctypes.data, arr["n_in"].ctypes.data, C.byref(tot))
    if rc:
        raise NbodyError(rc, "nbody_host_exchange_layout")
    return dict({k: v.astype(np.int64) for k, v in arr.items()}, total_in=int(tot.value))


def comm_unique_id() -> bytes:
    """Id of an RCCL communicator (NBODY_TRANSPORT=ipc in the environment: of the one-device transport)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = lib.nbody_comm_unique_id(buf)
    if rc:
        raise NbodyError(rc, (lib.nbody_last_error(None) or b"").decode())
    return buf.raw


def comm_local_id() -> bytes:
    """Id of the one-device transport: ranks (processes or threads) that share a GPU."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = lib.nbody_comm_local_id(buf)
    if rc:
        raise NbodyError(rc, (lib.nbody_last_error(None) or b"").decode())
    return buf.raw


def shard_range(n: int, rank: int, world_size: int) -> tuple[int, int]:
    """Index block [lo, hi) that nbody_upload gives `rank` (contiguous blocks of ceil(n/G))."""
    blk = (n + world_size - 1) // world_size
    lo = min(n, rank * blk)
    return lo, min(n, lo + blk)
