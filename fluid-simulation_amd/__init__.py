"""MI355X-native PIC/FLIP step: Python host-side mirror of the reference's step surface.

The reference (Aakash1312/Fluid-Simulation, ``fluid.cc``) is one ``main()`` whose loop body
(``fluid.cc:1368-1507``) is the hot path.  This package binds the C ABI of
``libfluid_hip.so`` (``include/fluid_hip.h``) with ctypes: plumbing only — all compute is
hand-written HIP for gfx950.  There is NO CPU fallback: if the shared library is missing,
import fails; if no GPU is visible, ``FluidSim(...)`` raises.
"""
from ._lib import lib, check, FluidError, Params, StepStats, Source, LeafGridC, SdfParams, SdfGridC, SdfFilter, SdfTrack, SdfSurface, SdfTrails, MeshC, SdfAttrC, MeshAttrC, SdfAttrPartC, SdfAvgPartC, MeshExC, MESH, Camera, Shade, ImageC, RENDER, FIELD, PROF, MpmParams, MpmStepStats  # noqa: F401
from .mpm import MpmSim, snow_cone, mpm_eval, MPM_P, MPM_F  # noqa: F401
from .sim import FluidSim, water_cube_drop, reference_scatter, grid_bounds, write_vdb, VdbStream, LeafGrid, leaves_to_dense, write_vdb_leaves, merge_leaf_grids, merge_sdf_grids, SdfGrid, sdf_to_dense, write_vdb_sdf, Mesh, sdf_mesh, sdf_filter, sdf_filter_tracked, sdf_filter_grown, sdf_flow, SDF_FILTER_KINDS, SDF_TRACK_SCHEMES, SDF_SURFACE_KINDS, particles_surface, particles_trails, spheres_surface, write_ply_mesh, SdfAttr, sdf_mesh_attr, sdf_attr_to_dense, SdfAttrPart, merge_sdf_attr_grids, SdfAvgPart, merge_sdf_avg_grids, sdf_mesh_normals, mesh_triangles, camera, camera_look_at, sdf_render, write_png  # noqa: F401

def load_dist():
    """torch is imported only when the multi-GPU path is used."""
    from . import dist
    return dist


__all__ = ["MpmParams", "MpmStepStats", "MpmSim", "snow_cone", "mpm_eval", "MPM_P", "MPM_F", "load_dist", "FluidSim", "FluidError", "Params", "StepStats", "Source", "LeafGridC", "FIELD", "PROF", "water_cube_drop", "reference_scatter", "grid_bounds", "write_vdb", "VdbStream", "LeafGrid", "leaves_to_dense", "write_vdb_leaves", "merge_leaf_grids", "merge_sdf_grids", "SdfParams", "SdfGridC", "SdfGrid", "sdf_to_dense", "write_vdb_sdf", "MeshC", "Mesh", "sdf_mesh", "SdfFilter", "sdf_filter", "sdf_filter_tracked", "sdf_filter_grown", "sdf_flow", "SDF_FILTER_KINDS", "SdfTrack", "SdfSurface", "SDF_SURFACE_KINDS", "particles_surface", "SdfTrails", "particles_trails", "spheres_surface", "write_ply_mesh", "SdfAttrC", "MeshAttrC", "SdfAttr", "sdf_mesh_attr", "sdf_attr_to_dense", "SdfAvgPartC", "SdfAvgPart", "merge_sdf_avg_grids", "MeshExC", "MESH", "sdf_mesh_normals", "mesh_triangles", "Camera", "Shade", "ImageC", "RENDER", "camera", "camera_look_at", "sdf_render", "write_png", "lib", "check"]
