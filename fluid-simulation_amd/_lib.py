"""ctypes binding of include/fluid_hip.h (one function per C entry point; no logic here)."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libfluid_hip.so")
if not os.path.exists(_SO):
    raise ImportError(
        f"{_SO} is missing: build it with `make -C {_HERE}` (hipcc --offload-arch=gfx950). "
        "This package has no CPU path.")
lib = C.CDLL(_SO)


class FluidError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libfluid_hip error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    """fluid_params_t (include/fluid_hip.h); defaults = the reference's literals (fluid.cc:1357-1367)."""
    _fields_ = [("n", C.c_int32), ("device", C.c_int32), ("dx", C.c_double), ("rho", C.c_double),
                ("gravity", C.c_double * 3), ("max_dt", C.c_double), ("outer_tol", C.c_double),
                ("update_frac", C.c_double), ("cg_tol", C.c_double), ("cg_max_iters", C.c_int32),
                ("max_outer_passes", C.c_int32), ("precision", C.c_int32), ("preconditioner", C.c_int32),
                ("flip_blend", C.c_double), ("solve_start", C.c_int32), ("mg_precision", C.c_int32),
                ("dist_solve", C.c_int32), ("pad_", C.c_int32)]


class StepStats(C.Structure):
    """fluid_step_stats_t."""
    _fields_ = [("dt_in", C.c_double), ("dt_out", C.c_double), ("error", C.c_double), ("max_speed", C.c_double),
                ("relres", C.c_double), ("num_active", C.c_int64), ("outer_passes", C.c_int32),
                ("cg_iters", C.c_int32), ("cg_iters_last", C.c_int32), ("box_lo", C.c_int32 * 3),
                ("box_hi", C.c_int32 * 3), ("paths", C.c_int32)]

    def as_dict(self):
        return {"dt_in": self.dt_in, "dt_out": self.dt_out, "error": self.error, "max_speed": self.max_speed,
                "relres": self.relres, "num_active": self.num_active, "outer_passes": self.outer_passes,
                "cg_iters": self.cg_iters, "cg_iters_last": self.cg_iters_last,
                "box_lo": list(self.box_lo), "box_hi": list(self.box_hi), "paths": self.paths}


class Source(C.Structure):
    """fluid_source_t: a persistent particle source (include/fluid_hip.h, "particle sources and sinks")."""
    _fields_ = [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("per_cell", C.c_int32), ("mode", C.c_int32),
                ("every", C.c_int32), ("vel_mode", C.c_int32), ("vel", C.c_double * 3), ("seed", C.c_uint64)]


class LeafGridC(C.Structure):
    """fluid_leaf_grid_t: a grid as the list of its non-zero 8^3 leaves (include/fluid_hip.h, "output as non-zero leaves")."""
    _fields_ = [("n", C.c_int32), ("n_leaves", C.c_int32), ("origin", C.c_void_p), ("values", C.c_void_p)]


class SdfParams(C.Structure):
    """fluid_sdf_params_t: sphere radius and half width of the band, in voxels (include/fluid_hip.h, "liquid surface")."""
    _fields_ = [("radius", C.c_double), ("half_width", C.c_double)]


class SdfGridC(C.Structure):
    """fluid_sdf_grid_t: the narrow-band level set of the particles as the list of its 8^3 leaves."""
    _fields_ = [("n", C.c_int32), ("n_leaves", C.c_int32), ("background", C.c_float), ("radius", C.c_float),
                ("half_width", C.c_float), ("origin", C.c_void_p), ("values", C.c_void_p), ("active", C.c_void_p)]


class SdfFilter(C.Structure):
    """fluid_sdf_filter_t: box filter width, iterations and offset (include/fluid_hip.h, "liquid surface, smoothed")."""
    _fields_ = [("width", C.c_int32), ("iterations", C.c_int32), ("offset", C.c_double)]


class SdfTrack(C.Structure):
    """fluid_sdf_track_t: normalisation passes per track, trim, scheme (include/fluid_hip.h, "liquid surface, renormalised")."""
    _fields_ = [("normalize", C.c_int32), ("trim", C.c_int32), ("scheme", C.c_int32)]


class SdfSurface(C.Structure):
    """fluid_sdf_surface_t: which level set the particles give (include/fluid_hip.h, "liquid surface, averaged positions")."""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("influence", C.c_double)]


class SdfTrails(C.Structure):
    """fluid_sdf_trails_t: shutter time, spacing factor, end radius (voxels) and the most instances of a particle (include/fluid_hip.h,
    "liquid surface, velocity trails")."""
    _fields_ = [("shutter", C.c_double), ("delta", C.c_double), ("radius_min", C.c_double), ("max_instances", C.c_int32), ("reserved", C.c_int32)]


class MeshC(C.Structure):
    """fluid_mesh_t: the surface nets of the level set (include/fluid_hip.h, "liquid surface as a mesh")."""
    _fields_ = [("n", C.c_int32), ("n_vertices", C.c_int64), ("n_quads", C.c_int64), ("radius", C.c_float),
                ("half_width", C.c_float), ("background", C.c_float), ("vertices", C.c_void_p), ("quads", C.c_void_p)]


class SdfAttrC(C.Structure):
    """fluid_sdf_attr_t: the closest particle's id and velocity per voxel of a leaf list ("liquid surface, attributes")."""
    _fields_ = [("n_leaves", C.c_int32), ("id", C.c_void_p), ("velocity", C.c_void_p)]


class SdfAttrPartC(C.Structure):
    """fluid_sdf_attr_part_t: a rank's record of ids, velocities and squared distances ("liquid surface, attributes (decomposed runs)")."""
    _fields_ = [("n_leaves", C.c_int32), ("id", C.c_void_p), ("velocity", C.c_void_p), ("dist2", C.c_void_p)]


class SdfAvgPartC(C.Structure):
    """fluid_sdf_avg_part_t: a rank's record of squared distances and weighted sums ("liquid surface, averaged positions (decomposed runs)")."""
    _fields_ = [("n", C.c_int32), ("n_leaves", C.c_int32), ("background", C.c_float), ("radius", C.c_float), ("half_width", C.c_float),
                ("dx", C.c_float), ("influence", C.c_float), ("origin", C.c_void_p), ("dist2", C.c_void_p), ("sums", C.c_void_p)]


class MeshAttrC(C.Structure):
    """fluid_mesh_attr_t: a velocity per mesh vertex."""
    _fields_ = [("n_vertices", C.c_int64), ("velocity", C.c_void_p)]


class MeshExC(C.Structure):
    """fluid_mesh_ex_t: the optional parts of a mesh — velocities, normals, triangles ("normals and triangles")."""
    _fields_ = [("velocity", C.c_void_p), ("normals", C.c_void_p), ("triangles", C.c_void_p), ("n_triangles", C.c_int64)]


class MESH:
    VELOCITY, NORMALS, TRIANGLES = 1, 2, 4


class Camera(C.Structure):
    """fluid_camera_t: eye, the direction of pixel (-0.5, -0.5) and its change per column and row, in index space; the march
    (include/fluid_hip.h, "liquid surface as an image")."""
    _fields_ = [("eye", C.c_float * 3), ("dir00", C.c_float * 3), ("du", C.c_float * 3), ("dv", C.c_float * 3),
                ("width", C.c_int32), ("height", C.c_int32), ("t_near", C.c_float), ("step", C.c_float), ("n_steps", C.c_int32)]


class Shade(C.Structure):
    """fluid_shade_t: the diffuse base colour of a hit and the bytes of a miss."""
    _fields_ = [("base", C.c_float * 3), ("background", C.c_uint8 * 3), ("pad_", C.c_uint8)]


class ImageC(C.Structure):
    """fluid_image_t: the parts of a render snapshot."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("n_hit", C.c_int64), ("rgb", C.c_void_p), ("depth", C.c_void_p),
                ("normals", C.c_void_p)]


class RENDER:
    RGB, DEPTH, NORMALS = 1, 2, 4


class MpmParams(C.Structure):
    """mpm_params_t (include/mpm_hip.h); defaults = the literals of mpm.cc."""
    _fields_ = [("B", C.c_int32), ("W", C.c_int32), ("device", C.c_int32), ("cg_max_iters", C.c_int32),
                ("dx", C.c_double), ("gravity", C.c_double * 3), ("youngs_modulus", C.c_double),
                ("poisson_ratio", C.c_double), ("beta", C.c_double), ("hardening", C.c_double),
                ("theta_c", C.c_double), ("theta_s", C.c_double), ("max_dt", C.c_double), ("dt0", C.c_double),
                ("cg_tol", C.c_double), ("transpose_system", C.c_int32), ("pad_", C.c_int32)]


class MpmStepStats(C.Structure):
    """mpm_step_stats_t."""
    _fields_ = [("dt_in", C.c_double), ("dt_out", C.c_double), ("cg_error", C.c_double), ("max_speed", C.c_double),
                ("max_grad", C.c_double), ("max_fp", C.c_double), ("max_fe", C.c_double), ("max_force", C.c_double * 3),
                ("max_mi", C.c_double), ("max_force_coeff2", C.c_double), ("num_active", C.c_int32),
                ("cg_iters", C.c_int32), ("any_active", C.c_int32), ("cg_status", C.c_int32),
                ("ms_transfer", C.c_double), ("ms_forces", C.c_double), ("ms_solve", C.c_double),
                ("ms_deform", C.c_double), ("ms_advect", C.c_double), ("ms_apply_avg", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("max_force", "pad_")}
        d["max_force"] = list(self.max_force)
        return d


class FIELD:
    CONTAINER, WEIGHTS, VEL, VEL_BEFORE, INDICES, RHS, DIVER, PRESSURE, OUTPUT, SOLID = range(10)
    DIVER2, SEARCH, Q, FLAGS = 14, 15, 16, 17


class PROF:
    PCG_SQ, PCG_XR, P2G, G2P, SORT, SOLVE, MG_UP0 = range(7)


# every symbol include/fluid_hip.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = [
    ("fluid_default_params", C.c_int, [C.POINTER(Params)]),
    ("fluid_create", C.c_int, [C.POINTER(Params), C.POINTER(_P)]),
    ("fluid_destroy", C.c_int, [_P]),
    ("fluid_last_error", C.c_char_p, []),
    ("fluid_version", C.c_char_p, []),
    ("fluid_set_solid", C.c_int, [_P, _P]),
    ("fluid_upload_particles", C.c_int, [_P, C.c_int64, _P, _P]),
    ("fluid_download_particles", C.c_int, [_P, _P, _P]),
    ("fluid_num_particles", C.c_int64, [_P]),
    ("fluid_set_dt", C.c_int, [_P, C.c_double]),
    ("fluid_get_dt", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("fluid_scene_water_cube_drop", C.c_int64, [C.c_int32, C.c_int32, C.c_uint64, _P]),
    ("fluid_scene_uniform_scatter", C.c_int64, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_float, C.c_uint32, C.c_int32, _P]),
    ("fluid_step", C.c_int, [_P, C.POINTER(StepStats)]),
    ("fluid_p2g", C.c_int, [_P]),
    ("fluid_flags_index", C.c_int, [_P]),
    ("fluid_rhs_div", C.c_int, [_P, C.c_int]),
    ("fluid_solve", C.c_int, [_P]),
    ("fluid_vel_update", C.c_int, [_P]),
    ("fluid_pressure_pass", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("fluid_flip_advect", C.c_int, [_P]),
    ("fluid_get_stats", C.c_int, [_P, C.POINTER(StepStats)]),
    ("fluid_download_field", C.c_int, [_P, C.c_int, _P, C.c_size_t]),
    ("fluid_upload_field", C.c_int, [_P, C.c_int, _P, C.c_size_t]),
    ("fluid_stencil_apply", C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    ("fluid_extrapolate", C.c_int, [_P, C.POINTER(C.c_int32)]),
    ("fluid_resample", C.c_int, [_P, C.c_int32, C.POINTER(C.c_int64)]),
    ("fluid_get_droplets", C.c_int, [_P, C.POINTER(C.c_int32), _P, C.c_int32]),
    ("fluid_add_particles", C.c_int, [_P, C.c_int64, _P, _P]),
    ("fluid_set_source", C.c_int, [_P, C.c_int32, C.POINTER(Source)]),
    ("fluid_set_sink", C.c_int, [_P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("fluid_get_source_stats", C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("fluid_dist_set_source", C.c_int, [_P, C.c_int32, C.POINTER(Source)]),
    ("fluid_dist_set_sink", C.c_int, [_P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("fluid_dist_get_source_stats", C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("fluid_dist_add_particles", C.c_int, [_P, C.c_int64, _P, _P, _P]),
    ("fluid_stencil_apply_hbm", C.c_int, [_P, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    ("fluid_profile_enable", C.c_int, [_P, C.c_int]),
    ("fluid_profile_read", C.c_int, [_P, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("fluid_profile_reset", C.c_int, [_P]),
    ("fluid_spline_eval", C.c_int, [C.c_int32, C.c_int32, C.c_int64, _P, _P]),
    ("fluid_dot_eval", C.c_int, [C.c_int32, C.c_int64, _P, _P, _P]),
    ("fluid_scan_eval", C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P]),
    ("fluid_write_vdb", C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(_P)]),
    ("fluid_write_vdb_ex", C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(_P), C.c_int32]),
    ("fluid_vdb_open", C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P)]),
    ("fluid_vdb_append", C.c_int, [_P, _P]),
    ("fluid_vdb_close", C.c_int, [_P]),
    ("fluid_output_snapshot", C.c_int, [_P]),
    ("fluid_output_wait", C.c_int, [_P, C.POINTER(LeafGridC)]),
    ("fluid_output_stats", C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("fluid_leaves_to_dense", C.c_int, [C.POINTER(LeafGridC), _P]),
    ("fluid_vdb_append_leaves", C.c_int, [C.POINTER(_P), C.c_int32, C.POINTER(LeafGridC)]),
    ("fluid_write_vdb_leaves", C.c_int, [C.c_char_p, C.POINTER(LeafGridC), C.c_int32]),
    ("fluid_dist_output_snapshot", C.c_int, [_P]),
    ("fluid_dist_output_wait", C.c_int, [_P, C.POINTER(LeafGridC)]),
    ("fluid_dist_output_stats", C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("fluid_dist_output_every", C.c_int, [_P, C.c_int32]),
    ("fluid_leaf_grids_merge", C.c_int64, [C.POINTER(LeafGridC), C.c_int32, C.c_int64, _P, _P]),
    ("fluid_sdf_snapshot", C.c_int, [_P, C.POINTER(SdfParams)]),
    ("fluid_sdf_wait", C.c_int, [_P, C.POINTER(SdfGridC)]),
    ("fluid_sdf_stats", C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("fluid_sdf_to_dense", C.c_int, [C.POINTER(SdfGridC), _P, _P]),
    ("fluid_write_vdb_sdf", C.c_int, [C.c_char_p, C.POINTER(SdfGridC), C.c_int32]),
    ("fluid_dist_sdf_snapshot", C.c_int, [_P, C.POINTER(SdfParams)]),
    ("fluid_dist_sdf_wait", C.c_int, [_P, C.POINTER(SdfGridC)]),
    ("fluid_dist_sdf_stats", C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("fluid_sdf_grids_merge", C.c_int64, [C.POINTER(SdfGridC), C.c_int32, C.c_int64, _P, _P, _P]),
    ("fluid_sdf_snapshot_filtered", C.c_int, [_P, C.POINTER(SdfParams), C.POINTER(SdfFilter)]),
    ("fluid_mesh_snapshot_filtered", C.c_int, [_P, C.POINTER(SdfParams), C.POINTER(SdfFilter)]),
    ("fluid_sdf_filter", C.c_int, [C.POINTER(SdfGridC), C.POINTER(SdfFilter), _P]),
    ("fluid_sdf_set_track", C.c_int, [_P, C.POINTER(SdfTrack)]),
    ("fluid_sdf_filter_tracked", C.c_int64, [C.POINTER(SdfGridC), C.POINTER(SdfFilter), C.POINTER(SdfTrack), C.c_int64, _P, _P, _P, _P]),
    ("fluid_sdf_set_track_grow", C.c_int, [_P, C.c_int32]),
    ("fluid_sdf_filter_grown", C.c_int64, [C.POINTER(SdfGridC), C.POINTER(SdfAttrC), C.POINTER(SdfFilter), C.POINTER(SdfTrack), C.c_int64, _P, _P, _P,
                                           _P, _P]),
    ("fluid_sdf_set_filter_kind", C.c_int, [_P, C.c_int32]),
    ("fluid_sdf_flow", C.c_int64, [C.POINTER(SdfGridC), C.POINTER(SdfAttrC), C.c_int32, C.POINTER(SdfFilter), C.POINTER(SdfTrack), C.c_int32, C.c_int64,
                                   _P, _P, _P, _P, _P]),
    ("fluid_sdf_set_surface", C.c_int, [_P, C.POINTER(SdfSurface)]),
    ("fluid_particles_surface", C.c_int, [C.c_int32, C.c_double, C.c_int64, _P, C.POINTER(SdfParams), C.POINTER(SdfSurface), _P, _P]),
    ("fluid_sdf_set_trails", C.c_int, [_P, C.POINTER(SdfTrails)]),
    ("fluid_sdf_trails_stats", C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("fluid_particles_trails", C.c_int64, [C.c_int64, _P, _P, C.POINTER(SdfParams), C.POINTER(SdfTrails), C.c_int64, _P, _P]),
    ("fluid_spheres_surface", C.c_int, [C.c_int32, C.c_double, C.c_int64, _P, _P, C.POINTER(SdfParams), _P, _P]),
    ("fluid_mesh_snapshot", C.c_int, [_P, C.POINTER(SdfParams)]),
    ("fluid_mesh_wait", C.c_int, [_P, C.POINTER(MeshC)]),
    ("fluid_mesh_stats", C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("fluid_sdf_mesh", C.c_int64, [C.POINTER(SdfGridC), C.c_int64, C.c_int64, _P, _P, C.POINTER(C.c_int64)]),
    ("fluid_write_ply_mesh", C.c_int, [C.c_char_p, C.POINTER(MeshC), C.c_float]),
    ("fluid_sdf_snapshot_attr", C.c_int, [_P, C.POINTER(SdfParams), C.POINTER(SdfFilter)]),
    ("fluid_sdf_wait_attr", C.c_int, [_P, C.POINTER(SdfGridC), C.POINTER(SdfAttrC)]),
    ("fluid_mesh_snapshot_attr", C.c_int, [_P, C.POINTER(SdfParams), C.POINTER(SdfFilter)]),
    ("fluid_mesh_wait_attr", C.c_int, [_P, C.POINTER(MeshC), C.POINTER(MeshAttrC)]),
    ("fluid_sdf_mesh_attr", C.c_int64, [C.POINTER(SdfGridC), C.POINTER(SdfAttrC), C.c_int64, _P]),
    ("fluid_sdf_attr_to_dense", C.c_int, [C.POINTER(SdfGridC), C.POINTER(SdfAttrC), _P, _P]),
    ("fluid_write_ply_mesh_attr", C.c_int, [C.c_char_p, C.POINTER(MeshC), C.POINTER(MeshAttrC), C.c_float, C.c_float]),
    ("fluid_dist_sdf_snapshot_attr", C.c_int, [_P, C.POINTER(SdfParams)]),
    ("fluid_dist_sdf_wait_attr", C.c_int, [_P, C.POINTER(SdfGridC), C.POINTER(SdfAttrPartC)]),
    ("fluid_sdf_attr_grids_merge", C.c_int64, [C.POINTER(SdfGridC), C.POINTER(SdfAttrPartC), C.c_int32, C.c_int64, _P, _P, _P, _P, _P]),
    ("fluid_dist_sdf_snapshot_avg", C.c_int, [_P, C.POINTER(SdfParams), C.POINTER(SdfSurface)]),
    ("fluid_dist_sdf_wait_avg", C.c_int, [_P, C.POINTER(SdfAvgPartC)]),
    ("fluid_sdf_avg_grids_merge", C.c_int64, [C.POINTER(SdfAvgPartC), C.c_int32, C.c_int64, _P, _P, _P]),
    ("fluid_dist_sdf_snapshot_trails", C.c_int, [_P, C.POINTER(SdfParams), C.POINTER(SdfTrails)]),
    ("fluid_dist_sdf_trails_stats", C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("fluid_mesh_snapshot_ex", C.c_int, [_P, C.POINTER(SdfParams), C.POINTER(SdfFilter), C.c_uint32]),
    ("fluid_mesh_wait_ex", C.c_int, [_P, C.POINTER(MeshC), C.POINTER(MeshExC)]),
    ("fluid_sdf_mesh_normals", C.c_int64, [C.POINTER(SdfGridC), C.c_int64, _P]),
    ("fluid_mesh_triangles", C.c_int64, [C.POINTER(MeshC), C.c_int64, _P]),
    ("fluid_write_ply_mesh_ex", C.c_int, [C.c_char_p, C.POINTER(MeshC), C.POINTER(MeshExC), C.c_float, C.c_float]),
    ("fluid_render_snapshot", C.c_int, [_P, C.POINTER(SdfParams), C.POINTER(SdfFilter), C.POINTER(Camera), C.POINTER(Shade), C.c_uint32]),
    ("fluid_render_wait", C.c_int, [_P, C.POINTER(ImageC)]),
    ("fluid_render_stats", C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("fluid_sdf_render", C.c_int, [C.POINTER(SdfGridC), C.POINTER(Camera), C.POINTER(Shade), C.c_uint32, _P, _P, _P, C.POINTER(C.c_int64)]),
    ("fluid_camera_look_at", C.c_int, [C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_int32,
                                        C.c_int32, C.c_double, C.POINTER(Camera)]),
    ("fluid_write_png", C.c_int, [C.c_char_p, C.c_int32, C.c_int32, _P]),
    # the snow-MPM step (include/mpm_hip.h)
    ("mpm_default_params", C.c_int, [C.POINTER(MpmParams)]),
    ("mpm_create", C.c_int, [C.POINTER(MpmParams), C.POINTER(_P)]),
    ("mpm_destroy", C.c_int, [_P]),
    ("mpm_upload_particles", C.c_int, [_P, C.c_int64, _P, _P, C.POINTER(C.c_int64)]),
    ("mpm_num_particles", C.c_int64, [_P]),
    ("mpm_num_active", C.c_int32, [_P]),
    ("mpm_set_state", C.c_int, [_P, _P, _P, _P, C.c_int32]),
    ("mpm_set_dt", C.c_int, [_P, C.c_double]),
    ("mpm_get_dt", C.c_double, [_P]),
    ("mpm_step", C.c_int, [_P, C.POINTER(MpmStepStats)]),
    ("mpm_step_solve", C.c_int, [_P, C.POINTER(MpmStepStats)]),
    ("mpm_step_advance", C.c_int, [_P, C.POINTER(MpmStepStats)]),
    ("mpm_download_particles", C.c_int, [_P, C.c_int32, _P]),
    ("mpm_download_field", C.c_int, [_P, C.c_int32, _P]),
    ("mpm_download_system", C.c_int, [_P, _P, _P, C.c_int64]),
    ("mpm_apply_matrix", C.c_int, [_P, _P, _P]),
    ("mpm_eval", C.c_int, [C.c_int32, C.c_int64, _P, _P, C.c_double, C.c_double, C.c_double, _P, _P]),
    ("mpm_scene_cone", C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_uint32, _P]),
    # multi-GPU (argtypes with the comm struct are completed in dist.py)
    ("fluid_create_dist", C.c_int, None),
    ("fluid_window", C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("fluid_upload_particles_ids", C.c_int, [_P, C.c_int64, _P, _P, _P]),
    ("fluid_download_particles_ids", C.c_int64, [_P, _P, _P, _P]),
    ("fluid_partition_blocks", C.c_int, [C.c_int32, C.c_int64, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("fluid_local_group_create", C.c_int, [C.c_int32, C.POINTER(_P)]),
    ("fluid_local_group_destroy", C.c_int, [_P]),
    ("fluid_local_group_abort", C.c_int, [_P]),
    ("fluid_local_comm_create", C.c_int, None),
    ("fluid_rccl_unique_id", C.c_int, None),
    ("fluid_rccl_comm_create", C.c_int, None),
    ("fluid_rccl_comm_destroy", C.c_int, None),
    ("fluid_rccl_last_error", C.c_char_p, None),
]
for _name, _res, _args in SYMBOLS:
    _f = getattr(lib, _name)  # AttributeError here = header/library mismatch: fail loudly
    _f.restype = _res
    if _args is not None:
        _f.argtypes = _args


def check(rc):
    if rc != 0:
        raise FluidError(rc, lib.fluid_last_error().decode())
