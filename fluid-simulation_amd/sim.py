"""FluidSim: the reference's step loop surface (fluid.cc:1368-1507) over the C ABI."""
import ctypes as C
import numpy as np

from ._lib import lib, check, FluidError, Params, StepStats, FIELD, Source, LeafGridC, SdfParams, SdfGridC, SdfFilter, SdfTrack, SdfSurface, SdfTrails, MeshC, SdfAttrC, MeshAttrC, SdfAttrPartC, SdfAvgPartC, MeshExC, MESH, Camera, Shade, ImageC, RENDER

_FIELD_DTYPE = {
    FIELD.CONTAINER: (np.float32, 1), FIELD.WEIGHTS: (np.float32, 1), FIELD.OUTPUT: (np.float32, 1),
    FIELD.VEL: (np.float64, 3), FIELD.VEL_BEFORE: (np.float64, 3), FIELD.INDICES: (np.int32, 1),
    FIELD.RHS: (np.float32, 1), FIELD.DIVER: (np.float32, 1), FIELD.DIVER2: (np.float32, 1),
    FIELD.PRESSURE: (np.float64, 1), FIELD.SOLID: (np.uint8, 1), FIELD.FLAGS: (np.uint8, 1),
}


def grid_bounds(n):
    """(lo, hi) cell coordinates for n cells per axis; n=121 -> (-60, 60) like fluid.cc:1159."""
    lo = -(n // 2)
    return lo, lo + n - 1


_VDB_COMPRESSION = {"zip": 3, "active_mask": 2}


def write_vdb(path, grids, compression="zip"):
    """Write dense float32 (n,n,n) arrays as the unnamed FloatGrids of fluid.cc:1161-1164,1503 (OpenVDB file format 224);
    compression "zip" = ZIP | ACTIVE_MASK (the library's default), "active_mask" = ACTIVE_MASK only."""
    import ctypes as C
    if isinstance(grids, np.ndarray) and grids.ndim == 3:
        grids = [grids]
    arrs = [np.ascontiguousarray(g, dtype=np.float32) for g in grids]
    n = arrs[0].shape[0]
    assert all(a.shape == (n, n, n) for a in arrs)
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    check(lib.fluid_write_vdb_ex(str(path).encode(), n, len(arrs), ptrs, _VDB_COMPRESSION[compression]))


class VdbStream:
    """The final mygrids.vdb of the reference (every step's grid, fluid.cc:1366,1450,1508) written one grid at a time."""

    def __init__(self, path, n, n_grids, compression="zip"):
        import ctypes as C
        self._h = C.c_void_p()
        self.n = n
        check(lib.fluid_vdb_open(str(path).encode(), n, n_grids, _VDB_COMPRESSION[compression], C.byref(self._h)))

    def append(self, grid):
        a = np.ascontiguousarray(grid, dtype=np.float32)
        assert a.shape == (self.n,) * 3
        check(lib.fluid_vdb_append(self._h, a.ctypes.data))

    def append_leaves(self, leaves, also=()):
        """Append the grid a LeafGrid describes: the bytes of append(leaves_to_dense(leaves)).  `also`: more open streams of the
        same n and compression that receive the same grid in the same call (the listed leaves are compressed once)."""
        ws = [self, *also]
        hs = (C.c_void_p * len(ws))(*[w._h.value for w in ws])
        check(lib.fluid_vdb_append_leaves(hs, len(ws), C.byref(leaves._c())))

    def close(self):
        h, self._h = self._h, None
        if h:
            check(lib.fluid_vdb_close(h))


class LeafGrid:
    """fluid_leaf_grid_t on the host: n cells per axis, origin (k, 3) int32 — index-space origins of the listed 8^3 leaves,
    multiples of 8, ascending (x, y, z) — and values (k, 512) float32, ((x&7)*8 + (y&7))*8 + (z&7), +0 outside [lo,hi]^3."""

    def __init__(self, n, origin, values):
        self.n = int(n)
        self.origin = np.ascontiguousarray(origin, dtype=np.int32).reshape(-1, 3)
        self.values = np.ascontiguousarray(values, dtype=np.float32).reshape(-1, 512)
        assert self.origin.shape[0] == self.values.shape[0]

    @property
    def n_leaves(self):
        return self.origin.shape[0]

    def _c(self):
        return LeafGridC(self.n, self.n_leaves, self.origin.ctypes.data, self.values.ctypes.data)


def leaves_to_dense(leaves):
    """The dense float32 (n, n, n) array a LeafGrid describes (fluid_leaves_to_dense: host only)."""
    out = np.empty((leaves.n,) * 3, dtype=np.float32)
    check(lib.fluid_leaves_to_dense(C.byref(leaves._c()), out.ctypes.data_as(C.c_void_p)))
    return out


def write_vdb_leaves(path, leaves, compression="zip"):
    """write_vdb(path, leaves_to_dense(leaves)) without the dense array: the same file."""
    check(lib.fluid_write_vdb_leaves(str(path).encode(), C.byref(leaves._c()), _VDB_COMPRESSION[compression]))


def _leaf_grid_copy(g):
    """LeafGrid copied out of the buffers a fluid_leaf_grid_t points into."""
    k = g.n_leaves
    if k == 0:
        return LeafGrid(g.n, np.empty((0, 3), np.int32), np.empty((0, 512), np.float32))
    org = np.ctypeslib.as_array(C.cast(g.origin, C.POINTER(C.c_int32)), shape=(k, 3)).copy()
    val = np.ctypeslib.as_array(C.cast(g.values, C.POINTER(C.c_float)), shape=(k, 512)).copy()
    return LeafGrid(g.n, org, val)


def merge_leaf_grids(parts):
    """The LeafGrid of the whole grid from the blocks' LeafGrids (DistFluidSim.output_wait of every rank): the union of their
    leaves, ascending; a leaf a cut plane splits is the bitwise OR of the ranks' records (fluid_leaf_grids_merge: host only)."""
    parts = list(parts)
    arr = (LeafGridC * len(parts))(*[p._c() for p in parts])
    k = lib.fluid_leaf_grids_merge(arr, len(parts), 0, None, None)
    if k < 0:
        raise FluidError(-k, "fluid_leaf_grids_merge: the parts do not merge (different n, a bad list, or a voxel two parts hold)")
    org, val = np.empty((k, 3), np.int32), np.empty((k, 512), np.float32)
    if k and lib.fluid_leaf_grids_merge(arr, len(parts), k, org.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p)) != k:
        raise FluidError(1, "fluid_leaf_grids_merge: the second call disagrees with the count")
    return LeafGrid(parts[0].n, org, val)


class SdfGrid:
    """fluid_sdf_grid_t on the host: the narrow-band level set of the particles as the list of its 8^3 leaves.  origin (k, 3)
    int32, ascending (x, y, z); values (k, 512) float32, ((x&7)*8 + (y&7))*8 + (z&7); active (k, 512) bool in the same order;
    background = (float)dx * half_width; radius and half_width as floats, as used."""

    def __init__(self, n, origin, values, active, background, radius, half_width):
        self.n = int(n)
        self.origin = np.ascontiguousarray(origin, dtype=np.int32).reshape(-1, 3)
        self.values = np.ascontiguousarray(values, dtype=np.float32).reshape(-1, 512)
        self.active = np.ascontiguousarray(active, dtype=bool).reshape(-1, 512)
        assert self.origin.shape[0] == self.values.shape[0] == self.active.shape[0]
        self.background, self.radius, self.half_width = np.float32(background), np.float32(radius), np.float32(half_width)

    @property
    def n_leaves(self):
        return self.origin.shape[0]

    def _c(self):
        """(struct, the arrays it points into): bit off & 63 of word off >> 6 (OpenVDB's NodeMask order)."""
        words = np.packbits(self.active, axis=1, bitorder="little").view("<u8").reshape(-1, 8)
        words = np.ascontiguousarray(words)
        return SdfGridC(self.n, self.n_leaves, self.background, self.radius, self.half_width, self.origin.ctypes.data,
                        self.values.ctypes.data, words.ctypes.data), words


def _sdf_grid_copy(g):
    """SdfGrid copied out of the buffers a fluid_sdf_grid_t points into."""
    k = g.n_leaves
    if k == 0:
        return SdfGrid(g.n, np.empty((0, 3), np.int32), np.empty((0, 512), np.float32), np.empty((0, 512), bool),
                       g.background, g.radius, g.half_width)
    org = np.ctypeslib.as_array(C.cast(g.origin, C.POINTER(C.c_int32)), shape=(k, 3)).copy()
    val = np.ctypeslib.as_array(C.cast(g.values, C.POINTER(C.c_float)), shape=(k, 512)).copy()
    words = np.ctypeslib.as_array(C.cast(g.active, C.POINTER(C.c_uint64)), shape=(k, 8)).copy()
    act = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little").astype(bool)
    return SdfGrid(g.n, org, val, act, g.background, g.radius, g.half_width)


def merge_sdf_grids(parts):
    """The SdfGrid of the whole particle set from the ranks' SdfGrids (DistFluidSim.sdf_wait of every rank): the union of their
    leaves, ascending; per voxel inactive -background wins, then the smallest active value, else inactive +background
    (fluid_sdf_grids_merge: host only)."""
    parts = list(parts)
    cs = [p._c() for p in parts]           # (struct, mask words): the words must outlive the calls
    arr = (SdfGridC * len(parts))(*[c for c, _ in cs])
    k = lib.fluid_sdf_grids_merge(arr, len(parts), 0, None, None, None)
    if k < 0:
        raise FluidError(-k, "fluid_sdf_grids_merge: the parts do not merge (different n or parameters, a bad list, or an inactive "
                             "value that is neither +background nor -background)")
    org, val, words = np.empty((k, 3), np.int32), np.empty((k, 512), np.float32), np.zeros((k, 8), np.uint64)
    if k and lib.fluid_sdf_grids_merge(arr, len(parts), k, org.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p),
                                       words.ctypes.data_as(C.c_void_p)) != k:
        raise FluidError(1, "fluid_sdf_grids_merge: the second call disagrees with the count")
    act = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little").astype(bool).reshape(k, 512)
    p0 = parts[0]
    return SdfGrid(p0.n, org, val, act, p0.background, p0.radius, p0.half_width)


def sdf_to_dense(grid):
    """(values float32 (n, n, n), active bool (n, n, n)) of an SdfGrid: +background / inactive outside the listed leaves
    (fluid_sdf_to_dense: host only)."""
    val = np.empty((grid.n,) * 3, dtype=np.float32)
    act = np.empty((grid.n,) * 3, dtype=np.uint8)
    c, _keep = grid._c()
    check(lib.fluid_sdf_to_dense(C.byref(c), val.ctypes.data_as(C.c_void_p), act.ctypes.data_as(C.c_void_p)))
    return val, act.astype(bool)


def write_vdb_sdf(path, grid, compression="zip"):
    """One FloatGrid "surface" of class "level set" whose leaves are the listed ones (fluid_write_vdb_sdf: host only)."""
    c, _keep = grid._c()
    check(lib.fluid_write_vdb_sdf(str(path).encode(), C.byref(c), _VDB_COMPRESSION[compression]))


def _sdf_filter_of(smooth):
    """fluid_sdf_filter_t of a (width, iterations[, offset]) tuple."""
    if len(smooth) not in (2, 3):
        raise ValueError("smooth must be (width, iterations) or (width, iterations, offset)")
    return SdfFilter(int(smooth[0]), int(smooth[1]), float(smooth[2]) if len(smooth) == 3 else 0.0)


def sdf_filter(grid, width, iterations, offset=0.0):
    """The SdfGrid with `iterations` box filters of `width` and then `offset` applied to its active voxels; masks, leaves and
    inactive values stay (fluid_sdf_filter: host only).  A decomposed run smooths sdf_filter(merge_sdf_grids(parts), ...)."""
    c, _keep = grid._c()
    f = SdfFilter(int(width), int(iterations), float(offset))
    val = np.empty((grid.n_leaves, 512), np.float32)
    rc = lib.fluid_sdf_filter(C.byref(c), C.byref(f), val.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise FluidError(rc, "fluid_sdf_filter: a bad leaf list or filter (width 1..4, iterations 0..16, finite offset)")
    return SdfGrid(grid.n, grid.origin, val, grid.active, grid.background, grid.radius, grid.half_width)


SDF_TRACK_SCHEMES = {"first": 0, "hjweno5": 4}   # FLUID_SDF_TRACK_FIRST_BIAS, FLUID_SDF_TRACK_HJWENO5: the library's own numbers


def _sdf_scheme_of(scheme):
    """The scheme's number: "first" (the default), "hjweno5", or a number passed on as it is (the library refuses what it lacks)."""
    if isinstance(scheme, str):
        if scheme not in SDF_TRACK_SCHEMES:
            raise ValueError(f"scheme must be one of {sorted(SDF_TRACK_SCHEMES)} or a number")
        return SDF_TRACK_SCHEMES[scheme]
    return int(scheme)


def _sdf_track_of(track):
    """fluid_sdf_track_t of None (off), a pass count, or (normalize[, trim[, scheme]]); the trim defaults to on, the scheme to
    "first"."""
    if track is None:
        return None
    if isinstance(track, (tuple, list)):
        if len(track) not in (1, 2, 3):
            raise ValueError("track must be None, normalize, (normalize, trim) or (normalize, trim, scheme)")
        return SdfTrack(int(track[0]), int(bool(track[1])) if len(track) >= 2 else 1, _sdf_scheme_of(track[2]) if len(track) == 3 else 0)
    return SdfTrack(int(track), 1, 0)


def sdf_filter_tracked(grid, filt, track):
    """(SdfGrid, kept): the tracked filter of an SdfGrid (fluid_sdf_filter_tracked: host only).  filt = (width, iterations[,
    offset]); track = None, normalize, (normalize, trim) or (normalize, trim, scheme): after every box iteration and every offset
    step the level set is renormalised and trimmed (include/fluid_hip.h, "liquid surface, renormalised"), with scheme "first"
    (the default) or "hjweno5" ("liquid surface, renormalised: HJWENO5").  The trim can unlist leaves: kept[i] is the
    index in `grid` of leaf i of the result.  A decomposed run tracks sdf_filter_tracked(merge_sdf_grids(parts), ...)."""
    c, _keep = grid._c()
    f, t = _sdf_filter_of(filt), _sdf_track_of(track)
    pt = None if t is None else C.byref(t)
    k = lib.fluid_sdf_filter_tracked(C.byref(c), C.byref(f), pt, 0, None, None, None, None)
    if k < 0:
        raise FluidError(-k, "fluid_sdf_filter_tracked: a bad leaf list, filter (width 1..4, iterations 0..16, finite offset) or "
                             "track (normalize 0..8; |offset| <= background)")
    org, val, words = np.empty((k, 3), np.int32), np.empty((k, 512), np.float32), np.zeros((k, 8), np.uint64)
    kept = np.empty(k, np.int32)
    if k and lib.fluid_sdf_filter_tracked(C.byref(c), C.byref(f), pt, k, org.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p),
                                          words.ctypes.data_as(C.c_void_p), kept.ctypes.data_as(C.c_void_p)) != k:
        raise FluidError(1, "fluid_sdf_filter_tracked: the second call disagrees with the count")
    act = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little").astype(bool).reshape(k, 512)
    return SdfGrid(grid.n, org, val, act, grid.background, grid.radius, grid.half_width), kept


def sdf_filter_grown(grid, filt, track, attr=None):
    """The grown filter of an SdfGrid (fluid_sdf_filter_grown: host only): the tracked filter whose every track begins with a
    dilation of the band (include/fluid_hip.h, "liquid surface, grown band").  filt = (width, iterations[, offset]), |offset| <=
    4 dx; track = normalize (1..8), (normalize, True) or (normalize, True, scheme).  Returns the new SdfGrid, which can list leaves
    `grid` does not, or with attr (an SdfAttr of `grid`'s leaves) the pair (SdfGrid, SdfAttr).  A decomposed run grows the merged list."""
    c, _keep = grid._c()
    f, t = _sdf_filter_of(filt), _sdf_track_of(track)
    pt = None if t is None else C.byref(t)
    pa = None
    if attr is not None:
        ac = attr._c()
        pa = C.byref(ac)
    k = lib.fluid_sdf_filter_grown(C.byref(c), pa, C.byref(f), pt, 0, None, None, None, None, None)
    if k < 0:
        raise FluidError(-k, "fluid_sdf_filter_grown: a bad leaf list or attributes, filter (width 1..4, iterations 0..16, |offset| <= 4 dx) "
                             "or track (normalize 1..8 with the trim)")
    org, val, words = np.empty((k, 3), np.int32), np.empty((k, 512), np.float32), np.zeros((k, 8), np.uint64)
    ids = np.empty((k, 512), np.uint32) if attr is not None else None
    vel = np.empty((k, 3, 512), np.float32) if attr is not None else None
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    if k and lib.fluid_sdf_filter_grown(C.byref(c), pa, C.byref(f), pt, k, p(org), p(val), p(words), p(ids), p(vel)) != k:
        raise FluidError(1, "fluid_sdf_filter_grown: the second call disagrees with the count")
    act = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little").astype(bool).reshape(k, 512)
    out = SdfGrid(grid.n, org, val, act, grid.background, grid.radius, grid.half_width)
    return out if attr is None else (out, SdfAttr(ids, vel))


SDF_SURFACE_KINDS = {"spheres": 0, "averaged": 1}   # FLUID_SDF_SURFACE_*


def _sdf_surface_of(kind, influence):
    """fluid_sdf_surface_t of a name of SDF_SURFACE_KINDS (or a number, passed on as it is) and an influence radius in voxels."""
    k = SDF_SURFACE_KINDS[kind] if isinstance(kind, str) else int(kind)
    if k != 0 and influence is None:
        raise ValueError("the averaged surface needs an influence radius (voxels)")
    return SdfSurface(k, 0, 0.0 if influence is None else float(influence))


def particles_surface(pos, n, R, w, dx, kind="spheres", influence=None):
    """(values float32 (n, n, n), active bool (n, n, n)): the dense level set of the particles `pos` (k, 3) on the grid of n^3
    voxels of size dx, spheres of radius R and a band of half width w (voxels); kind "spheres" or "averaged" with its influence
    radius (include/fluid_hip.h, "liquid surface, averaged positions"; fluid_particles_surface: host only, brute force)."""
    p = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    val = np.empty((n,) * 3, dtype=np.float32)
    act = np.empty((n,) * 3, dtype=np.uint8)
    prm, sf = SdfParams(float(R), float(w)), _sdf_surface_of(kind, influence)
    check(lib.fluid_particles_surface(int(n), float(dx), len(p), p.ctypes.data_as(C.c_void_p), C.byref(prm), C.byref(sf),
                                      val.ctypes.data_as(C.c_void_p), act.ctypes.data_as(C.c_void_p)))
    return val, act.astype(bool)


def particles_trails(pos, vel, R, w, shutter, delta=1.0, radius_min=None, max_instances=16):
    """(positions float64 (k, 3), radii float32 (k,)): the particles `pos` (np, 3) with velocities `vel` (voxels per time) expanded
    into the instances of their velocity trails, in particle order; radius_min None: R / 2 (include/fluid_hip.h, "liquid surface,
    velocity trails"; fluid_particles_trails: host only)."""
    p = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    v = np.ascontiguousarray(vel, dtype=np.float64).reshape(-1, 3)
    if v.shape != p.shape:
        raise ValueError("one velocity per particle")
    prm = SdfParams(float(R), float(w))
    t = SdfTrails(float(shutter), float(delta), float(R) / 2 if radius_min is None else float(radius_min), int(max_instances), 0)
    pp, vp = p.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)
    k = lib.fluid_particles_trails(len(p), pp, vp, C.byref(prm), C.byref(t), 0, None, None)
    if k < 0:
        check(int(-k))
    out, rad = np.empty((k, 3), dtype=np.float64), np.empty(k, dtype=np.float32)
    got = lib.fluid_particles_trails(len(p), pp, vp, C.byref(prm), C.byref(t), k, out.ctypes.data_as(C.c_void_p), rad.ctypes.data_as(C.c_void_p))
    if got != k:
        check(int(-got) if got < 0 else 1)
    return out, rad


def spheres_surface(pos, radius, n, R, w, dx):
    """(values float32 (n, n, n), active bool (n, n, n)): the dense level set of the spheres at `pos` (k, 3) with their own radii
    `radius` (k,), each in (0, R], and a band of half width w (voxels), on the grid of n^3 voxels of size dx (include/fluid_hip.h,
    "liquid surface, velocity trails"; fluid_spheres_surface: host only, brute force)."""
    p = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    r = np.ascontiguousarray(radius, dtype=np.float32).reshape(-1)
    if len(r) != len(p):
        raise ValueError("one radius per position")
    val = np.empty((n,) * 3, dtype=np.float32)
    act = np.empty((n,) * 3, dtype=np.uint8)
    prm = SdfParams(float(R), float(w))
    check(lib.fluid_spheres_surface(int(n), float(dx), len(p), p.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), C.byref(prm),
                                    val.ctypes.data_as(C.c_void_p), act.ctypes.data_as(C.c_void_p)))
    return val, act.astype(bool)


SDF_FILTER_KINDS = {"box": 0, "median": 1, "laplacian": 2, "curvature": 3}   # FLUID_SDF_FILTER_*


def _sdf_kind_of(kind):
    """FLUID_SDF_FILTER_* of a name of SDF_FILTER_KINDS; an integer is passed on as it is (the library checks it)."""
    return SDF_FILTER_KINDS[kind] if isinstance(kind, str) else int(kind)


def sdf_flow(grid, kind, filt, track=None, grow=False, attr=None):
    """The filter of `kind` ("box", "median", "laplacian", "curvature", or a FLUID_SDF_FILTER_* number) of an SdfGrid
    (fluid_sdf_flow: host only; include/fluid_hip.h, "liquid surface, flows").  filt = (width, iterations[, offset]): a median
    takes width 1 or 2, a Laplacian or mean-curvature flow width 1.  track = None (untracked), normalize, (normalize, trim) or (normalize, trim, scheme);
    grow=True: every track begins with a dilation of the band.  Returns the new SdfGrid, or with attr (an SdfAttr of `grid`'s
    leaves) the pair (SdfGrid, SdfAttr).  A decomposed run filters the merged list."""
    c, _keep = grid._c()
    f, t = _sdf_filter_of(filt), _sdf_track_of(track)
    pt = None if t is None else C.byref(t)
    pa = None
    if attr is not None:
        ac = attr._c()
        pa = C.byref(ac)
    kd = _sdf_kind_of(kind)
    k = lib.fluid_sdf_flow(C.byref(c), pa, kd, C.byref(f), pt, int(grow), 0, None, None, None, None, None)
    if k < 0:
        raise FluidError(-k, "fluid_sdf_flow: a bad leaf list or attributes, kind, filter (median: width 1..2; laplacian, curvature: "
                             "width 1; iterations 0..16) or track (the offset's limit is that of the form that runs)")
    org, val, words = np.empty((k, 3), np.int32), np.empty((k, 512), np.float32), np.zeros((k, 8), np.uint64)
    ids = np.empty((k, 512), np.uint32) if attr is not None else None
    vel = np.empty((k, 3, 512), np.float32) if attr is not None else None
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    if k and lib.fluid_sdf_flow(C.byref(c), pa, kd, C.byref(f), pt, int(grow), k, p(org), p(val), p(words), p(ids), p(vel)) != k:
        raise FluidError(1, "fluid_sdf_flow: the second call disagrees with the count")
    act = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little").astype(bool).reshape(k, 512)
    out = SdfGrid(grid.n, org, val, act, grid.background, grid.radius, grid.half_width)
    return out if attr is None else (out, SdfAttr(ids, vel))


class Mesh:
    """fluid_mesh_t on the host: the surface nets of the level set (include/fluid_hip.h, "liquid surface as a mesh").  vertices
    (nv, 3) float32 in index space, quads (nq, 4) uint32 vertex numbers, counter-clockwise seen from outside the liquid."""

    def __init__(self, n, vertices, quads, background=0.0, radius=0.0, half_width=0.0):
        self.n = int(n)
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        self.quads = np.ascontiguousarray(quads, dtype=np.uint32).reshape(-1, 4)
        self.background, self.radius, self.half_width = np.float32(background), np.float32(radius), np.float32(half_width)

    def _c(self):
        nv, nq = len(self.vertices), len(self.quads)
        return MeshC(self.n, nv, nq, self.radius, self.half_width, self.background, self.vertices.ctypes.data if nv else None,
                     self.quads.ctypes.data if nq else None)


def sdf_mesh(grid):
    """The Mesh of an SdfGrid, every unlisted leaf being +background (fluid_sdf_mesh: host only).  A decomposed run gets its mesh
    as sdf_mesh(merge_sdf_grids(parts))."""
    c, _keep = grid._c()
    nq = C.c_int64()
    nv = lib.fluid_sdf_mesh(C.byref(c), 0, 0, None, None, C.byref(nq))
    if nv < 0:
        raise FluidError(-nv, "fluid_sdf_mesh: a bad leaf list, or more than 2^31 - 1 vertices or quads")
    v, q = np.empty((nv, 3), np.float32), np.empty((nq.value, 4), np.uint32)
    if nv:
        nq2 = C.c_int64(-1)
        nv2 = lib.fluid_sdf_mesh(C.byref(c), nv, len(q), v.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), C.byref(nq2))
        if nv2 < 0:
            raise FluidError(-nv2, "fluid_sdf_mesh: the second call was refused")
        if (nv2, nq2.value) != (nv, len(q)):
            raise RuntimeError(f"fluid_sdf_mesh: the second call gives {nv2} vertices and {nq2.value} quads, the first gave {nv} and {len(q)}")
    return Mesh(grid.n, v, q, grid.background, grid.radius, grid.half_width)


def write_ply_mesh(path, mesh, voxel_size, velocity=None, velocity_scale=1.0, normals=None, triangles=None):
    """Binary little-endian PLY of a Mesh (or of a (vertices, quads) pair); positions are index space times voxel_size
    (fluid_write_ply_mesh: host only).  velocity (nv, 3): vx / vy / vz per vertex as well, times velocity_scale
    (fluid_write_ply_mesh_attr).  normals (nv, 3): nx / ny / nz per vertex, unscaled; triangles (2 nq, 3): the faces are these
    instead of the quads (fluid_write_ply_mesh_ex)."""
    if not isinstance(mesh, Mesh):
        mesh = Mesh(0, mesh[0], mesh[1])
    if normals is not None or triangles is not None:
        nv = len(mesh.vertices)
        keep = [np.zeros(4, np.float32)]                     # an empty part still selects its header lines: any non-NULL pointer
        ex = MeshExC(None, None, None, 0)
        for name, arr, dt, rows in (("velocity", velocity, np.float32, nv), ("normals", normals, np.float32, nv), ("triangles", triangles, np.uint32, None)):
            if arr is None:
                continue
            a = np.ascontiguousarray(arr, dtype=dt).reshape(-1, 3)
            if rows is not None and len(a) != rows:
                raise FluidError(1, f"fluid_write_ply_mesh_ex: {len(a)} {name} for {rows} vertices")
            keep.append(a)
            setattr(ex, name, a.ctypes.data if len(a) else keep[0].ctypes.data)
            if name == "triangles":
                ex.n_triangles = len(a)
        rc = lib.fluid_write_ply_mesh_ex(str(path).encode(), C.byref(mesh._c()), C.byref(ex), float(voxel_size), float(velocity_scale))
        if rc != 0:
            raise FluidError(rc, "fluid_write_ply_mesh_ex: a bad mesh, a triangle count that is not twice the quad count, an entry beyond the vertices, a bad scale or path")
        return
    if velocity is None:
        check(lib.fluid_write_ply_mesh(str(path).encode(), C.byref(mesh._c()), float(voxel_size)))
        return
    vel = np.ascontiguousarray(velocity, dtype=np.float32).reshape(-1, 3)
    at = MeshAttrC(len(vel), vel.ctypes.data if len(vel) else None)
    rc = lib.fluid_write_ply_mesh_attr(str(path).encode(), C.byref(mesh._c()), C.byref(at), float(voxel_size), float(velocity_scale))
    if rc != 0:
        raise FluidError(rc, "fluid_write_ply_mesh_attr: a bad mesh, a velocity count that is not the vertex count, a bad scale or path")


class SdfAttr:
    """fluid_sdf_attr_t on the host ("liquid surface, attributes"): per voxel of an SdfGrid's leaves the closest particle's id
    (k, 512) uint32 — 0xffffffff where the voxel is not active — and velocity (k, 3, 512) float32."""
    NO_ID = 0xFFFFFFFF

    def __init__(self, id, velocity):
        self.id = np.ascontiguousarray(id, dtype=np.uint32).reshape(-1, 512)
        self.velocity = np.ascontiguousarray(velocity, dtype=np.float32).reshape(-1, 3, 512)
        assert self.id.shape[0] == self.velocity.shape[0]

    @property
    def n_leaves(self):
        return self.id.shape[0]

    def _c(self):
        k = self.n_leaves
        return SdfAttrC(k, self.id.ctypes.data if k else None, self.velocity.ctypes.data if k else None)


class SdfAttrPart:
    """fluid_sdf_attr_part_t on the host ("liquid surface, attributes (decomposed runs)"): a rank's record beside its SdfGrid.
    id (k, 512) uint32 and velocity (k, 3, 512) float32 as SdfAttr's, over the rank's live particles; dist2 (k, 512) float32, the
    squared distance to the closest of them where the voxel is active, +inf elsewhere."""

    def __init__(self, id, velocity, dist2):
        self.id = np.ascontiguousarray(id, dtype=np.uint32).reshape(-1, 512)
        self.velocity = np.ascontiguousarray(velocity, dtype=np.float32).reshape(-1, 3, 512)
        self.dist2 = np.ascontiguousarray(dist2, dtype=np.float32).reshape(-1, 512)
        assert self.id.shape[0] == self.velocity.shape[0] == self.dist2.shape[0]

    @property
    def n_leaves(self):
        return self.id.shape[0]

    def _c(self):
        k = self.n_leaves
        return SdfAttrPartC(k, self.id.ctypes.data if k else None, self.velocity.ctypes.data if k else None,
                            self.dist2.ctypes.data if k else None)


def _sdf_attr_part_copy(a):
    """SdfAttrPart copied out of the buffers a fluid_sdf_attr_part_t points into, or None when it points nowhere with leaves
    (the snapshot was taken without a record)."""
    k = a.n_leaves
    if k == 0:
        return SdfAttrPart(np.empty((0, 512), np.uint32), np.empty((0, 3, 512), np.float32), np.empty((0, 512), np.float32))
    if not a.id or not a.velocity or not a.dist2:
        return None
    return SdfAttrPart(np.ctypeslib.as_array(C.cast(a.id, C.POINTER(C.c_uint32)), shape=(k, 512)).copy(),
                       np.ctypeslib.as_array(C.cast(a.velocity, C.POINTER(C.c_float)), shape=(k, 3, 512)).copy(),
                       np.ctypeslib.as_array(C.cast(a.dist2, C.POINTER(C.c_float)), shape=(k, 512)).copy())


def merge_sdf_attr_grids(parts, attrs):
    """(SdfGrid, SdfAttr) of the whole particle set from the ranks' SdfGrids and SdfAttrParts (DistFluidSim.sdf_wait_attr of every
    rank): the geometry of merge_sdf_grids; per active voxel the id and velocity of the part with the smallest dist2, then the
    smallest id (fluid_sdf_attr_grids_merge: host only)."""
    parts, attrs = list(parts), list(attrs)
    assert len(parts) == len(attrs)
    cs = [p._c() for p in parts]           # (struct, mask words): the words must outlive the calls
    arr = (SdfGridC * len(parts))(*[c for c, _ in cs])
    aarr = (SdfAttrPartC * len(attrs))(*[a._c() for a in attrs])
    k = lib.fluid_sdf_attr_grids_merge(arr, aarr, len(parts), 0, None, None, None, None, None)
    if k < 0:
        raise FluidError(-k, "fluid_sdf_attr_grids_merge: the parts do not merge (what fluid_sdf_grids_merge refuses, records of "
                             "another list, an active voxel without id or finite dist2, or dist2 that contradicts the values)")
    org, val, words = np.empty((k, 3), np.int32), np.empty((k, 512), np.float32), np.zeros((k, 8), np.uint64)
    ids, vel = np.empty((k, 512), np.uint32), np.empty((k, 3, 512), np.float32)
    if k and lib.fluid_sdf_attr_grids_merge(arr, aarr, len(parts), k, *[x.ctypes.data_as(C.c_void_p) for x in (org, val, words, ids, vel)]) != k:
        raise FluidError(1, "fluid_sdf_attr_grids_merge: the second call disagrees with the count")
    act = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little").astype(bool).reshape(k, 512)
    p0 = parts[0]
    return SdfGrid(p0.n, org, val, act, p0.background, p0.radius, p0.half_width), SdfAttr(ids, vel)


class SdfAvgPart:
    """fluid_sdf_avg_part_t on the host ("liquid surface, averaged positions (decomposed runs)"): a rank's record of its live
    particles, owning its arrays.  origin (k, 3) int32 ascending; dist2 (k, 512) float32: the squared distance to the closest
    particle inside (min2, max(max2, h2)), +0 at or below min2, +inf elsewhere; sums (k, 4, 512) uint64: SW, SX, SY, SZ."""

    def __init__(self, n, origin, dist2, sums, background, radius, half_width, dx, influence):
        self.n = int(n)
        self.origin = np.ascontiguousarray(origin, dtype=np.int32).reshape(-1, 3)
        self.dist2 = np.ascontiguousarray(dist2, dtype=np.float32).reshape(-1, 512)
        self.sums = np.ascontiguousarray(sums, dtype=np.uint64).reshape(-1, 4, 512)
        assert self.origin.shape[0] == self.dist2.shape[0] == self.sums.shape[0]
        self.background, self.radius, self.half_width = np.float32(background), np.float32(radius), np.float32(half_width)
        self.dx, self.influence = np.float32(dx), np.float32(influence)

    @property
    def n_leaves(self):
        return self.origin.shape[0]

    def _c(self):
        k = self.n_leaves
        return SdfAvgPartC(self.n, k, self.background, self.radius, self.half_width, self.dx, self.influence,
                           self.origin.ctypes.data if k else None, self.dist2.ctypes.data if k else None,
                           self.sums.ctypes.data if k else None)


def _sdf_avg_part_copy(a):
    """SdfAvgPart copied out of the buffers a fluid_sdf_avg_part_t points into."""
    k = a.n_leaves
    if k == 0:
        org, d2, sums = np.empty((0, 3), np.int32), np.empty((0, 512), np.float32), np.empty((0, 4, 512), np.uint64)
    else:
        org = np.ctypeslib.as_array(C.cast(a.origin, C.POINTER(C.c_int32)), shape=(k, 3)).copy()
        d2 = np.ctypeslib.as_array(C.cast(a.dist2, C.POINTER(C.c_float)), shape=(k, 512)).copy()
        sums = np.ctypeslib.as_array(C.cast(a.sums, C.POINTER(C.c_uint64)), shape=(k, 4, 512)).copy()
    return SdfAvgPart(a.n, org, d2, sums, a.background, a.radius, a.half_width, a.dx, a.influence)


def merge_sdf_avg_grids(parts):
    """The SdfGrid of the averaged-position surface of the whole particle set from the ranks' SdfAvgParts (sdf_wait_avg of every
    rank): per voxel the minimum of dist2 and the wrapping sums of the sums, finished as on one GPU
    (fluid_sdf_avg_grids_merge: host only)."""
    parts = list(parts)
    arr = (SdfAvgPartC * max(len(parts), 1))(*[p._c() for p in parts])
    k = lib.fluid_sdf_avg_grids_merge(arr, len(parts), 0, None, None, None)
    if k < 0:
        raise FluidError(-k, "fluid_sdf_avg_grids_merge: the parts do not merge (no part, records of different parameters, a bad "
                             "leaf list, a dist2 that is NaN or negative, or sums beside a dist2 of +0 or +inf)")
    org, val, words = np.empty((k, 3), np.int32), np.empty((k, 512), np.float32), np.zeros((k, 8), np.uint64)
    if k and lib.fluid_sdf_avg_grids_merge(arr, len(parts), k, *[x.ctypes.data_as(C.c_void_p) for x in (org, val, words)]) != k:
        raise FluidError(1, "fluid_sdf_avg_grids_merge: the second call disagrees with the count")
    act = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little").astype(bool).reshape(k, 512)
    p0 = parts[0]
    return SdfGrid(p0.n, org, val, act, p0.background, p0.radius, p0.half_width)


def sdf_mesh_attr(grid, attr):
    """velocity (nv, 3) float32: the vertex velocities of sdf_mesh(grid), in its vertex order (fluid_sdf_mesh_attr: host only)."""
    c, _keep = grid._c()
    a = attr._c()
    nv = lib.fluid_sdf_mesh_attr(C.byref(c), C.byref(a), 0, None)
    if nv < 0:
        raise FluidError(-nv, "fluid_sdf_mesh_attr: a bad leaf list, or attributes of another list")
    vel = np.empty((nv, 3), np.float32)
    if nv and lib.fluid_sdf_mesh_attr(C.byref(c), C.byref(a), nv, vel.ctypes.data_as(C.c_void_p)) != nv:
        raise FluidError(1, "fluid_sdf_mesh_attr: the second call disagrees with the count")
    return vel


def sdf_mesh_normals(grid):
    """normals (nv, 3) float32: the unit vertex normals of sdf_mesh(grid), in its vertex order (fluid_sdf_mesh_normals: host only)."""
    c, _keep = grid._c()
    nv = lib.fluid_sdf_mesh_normals(C.byref(c), 0, None)
    if nv < 0:
        raise FluidError(-nv, "fluid_sdf_mesh_normals: a bad leaf list")
    nrm = np.empty((nv, 3), np.float32)
    if nv and lib.fluid_sdf_mesh_normals(C.byref(c), nv, nrm.ctypes.data_as(C.c_void_p)) != nv:
        raise FluidError(1, "fluid_sdf_mesh_normals: the second call disagrees with the count")
    return nrm


def mesh_triangles(vertices, quads):
    """triangles (2 nq, 3) uint32: every quad cut along its shorter diagonal, in quad order (fluid_mesh_triangles: host only)."""
    m = Mesh(0, vertices, quads)
    tri = np.empty((2 * len(m.quads), 3), np.uint32)
    k = lib.fluid_mesh_triangles(C.byref(m._c()), len(tri), tri.ctypes.data_as(C.c_void_p) if len(tri) else None)
    if k != len(tri):
        raise FluidError(1 if k >= 0 else -k, "fluid_mesh_triangles: a bad mesh (a quad entry beyond the vertices?)")
    return tri


def camera(eye, dir00, du, dv, width, height, t_near, step, n_steps):
    """A Camera (fluid_camera_t) from plain sequences; every float is narrowed once."""
    c = Camera()
    for name, v in (("eye", eye), ("dir00", dir00), ("du", du), ("dv", dv)):
        setattr(c, name, (C.c_float * 3)(*[float(x) for x in v]))
    c.width, c.height, c.t_near, c.step, c.n_steps = int(width), int(height), float(t_near), float(step), int(n_steps)
    return c


def _shade_of(shade):
    """fluid_shade_t of None, a Shade, or a (base (3 floats), background (3 bytes)) pair."""
    if shade is None or isinstance(shade, Shade):
        return shade
    base, background = shade
    return Shade((C.c_float * 3)(*[float(x) for x in base]), (C.c_uint8 * 3)(*[int(x) for x in background]), 0)


def _render_what(rgb, depth, normals):
    return (RENDER.RGB if rgb else 0) | (RENDER.DEPTH if depth else 0) | (RENDER.NORMALS if normals else 0)


def camera_look_at(n, eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov_y_degrees=40.0, width=640, height=360, step=0.5):
    """The pinhole Camera of a grid of n^3 cells that looks from `eye` at `target` (fluid_camera_look_at: host only)."""
    c = Camera()
    d3 = lambda v: (C.c_double * 3)(*[float(x) for x in v])   # noqa: E731
    rc = lib.fluid_camera_look_at(int(n), d3(eye), d3(target), d3(up), float(fov_y_degrees), int(width), int(height), float(step), C.byref(c))
    if rc != 0:
        raise FluidError(rc, "fluid_camera_look_at: a degenerate view or a size, field of view or step outside the limits")
    return c


def sdf_render(grid, camera, shade=None, rgb=True, depth=False, normals=False):
    """The image of an SdfGrid, every unlisted leaf being +background (fluid_sdf_render: host only): {"rgb" (H, W, 3) uint8,
    "depth" (H, W) float32, "normals" (H, W, 3) float32, "n_hit"}, None for a part that is not asked for.  A decomposed run renders
    sdf_render(merge_sdf_grids(parts), ...)."""
    c, _keep = grid._c()
    sh = _shade_of(shade)
    H, W = camera.height, camera.width
    ok = 1 <= W <= 8192 and 1 <= H <= 8192
    out = {"rgb": np.empty((H, W, 3), np.uint8) if rgb and ok else None, "depth": np.empty((H, W), np.float32) if depth and ok else None,
           "normals": np.empty((H, W, 3), np.float32) if normals and ok else None}
    n_hit = C.c_int64(0)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = lib.fluid_sdf_render(C.byref(c), C.byref(camera), None if sh is None else C.byref(sh), _render_what(rgb, depth, normals),
                              ptr(out["rgb"]), ptr(out["depth"]), ptr(out["normals"]), C.byref(n_hit))
    if rc != 0:
        raise FluidError(rc, "fluid_sdf_render: a bad leaf list, camera, shade or choice of parts")
    out["n_hit"] = n_hit.value
    return out


def write_png(path, rgb):
    """An 8-bit RGB PNG of rgb (H, W, 3) uint8 (fluid_write_png: host only)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("rgb must be (height, width, 3)")
    rc = lib.fluid_write_png(str(path).encode(), rgb.shape[1], rgb.shape[0], rgb.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise FluidError(rc, "fluid_write_png: a size outside 1..8192 or a path that cannot be written")


def sdf_attr_to_dense(grid, attr):
    """(id uint32 (n, n, n), velocity float32 (3, n, n, n)) of an SdfGrid's attributes: 0xffffffff / +0 outside the listed leaves
    (fluid_sdf_attr_to_dense: host only)."""
    ids = np.empty((grid.n,) * 3, dtype=np.uint32)
    vel = np.empty((3,) + (grid.n,) * 3, dtype=np.float32)
    c, _keep = grid._c()
    a = attr._c()
    check_rc = lib.fluid_sdf_attr_to_dense(C.byref(c), C.byref(a), ids.ctypes.data_as(C.c_void_p), vel.ctypes.data_as(C.c_void_p))
    if check_rc != 0:
        raise FluidError(check_rc, "fluid_sdf_attr_to_dense: a bad leaf list, or attributes of another list")
    return ids, vel


def water_cube_drop(n, ppc, seed=0):
    """Synthetic input of SURVEY.md 8(d) (generalises fluid.cc:1176,1349): (npart,3) float64 positions."""
    cnt = lib.fluid_scene_water_cube_drop(n, ppc, seed, None)
    if cnt < 0:
        raise ValueError("bad scene arguments")
    pos = np.empty((cnt, 3), dtype=np.float64)
    got = lib.fluid_scene_water_cube_drop(n, ppc, seed, pos.ctypes.data_as(C.c_void_p))
    assert got == cnt
    return pos


def reference_scatter(lo=-20, hi=20, points_per_volume=10.0, seed=0, boundary=60):
    """The reference's own initial particles (fluid.cc:1176,1347-1350: fill(CoordBBox(lo,hi)) + UniformPointScatter with
    std::mt19937(seed)), restated on the host (csrc/scene_scatter.cpp): (npart,3) float64 positions.  The defaults are the
    reference's scene on its 121^3 grid: 689210 particles."""
    l3 = (C.c_int32 * 3)(*([lo] * 3 if np.isscalar(lo) else lo))
    h3 = (C.c_int32 * 3)(*([hi] * 3 if np.isscalar(hi) else hi))
    cnt = lib.fluid_scene_uniform_scatter(l3, h3, points_per_volume, seed, boundary, None)
    if cnt < 0:
        raise ValueError("bad scene arguments")
    pos = np.empty((cnt, 3), dtype=np.float64)
    got = lib.fluid_scene_uniform_scatter(l3, h3, points_per_volume, seed, boundary, pos.ctypes.data_as(C.c_void_p))
    assert got == cnt
    return pos


def source_methods(prefix):
    """set_source, clear_source, set_sink, clear_sink and source_stats of a handle ``self._h`` over the entry points of its kind
    (include/fluid_hip.h): "fluid_" on one GPU, "fluid_dist_" on a decomposed handle, where the boxes are global, the set calls
    collective (the same slots on every rank before the same step) and ids are never renumbered.  Each class binds its own."""
    c_set_source, c_set_sink, c_stats = (getattr(lib, prefix + f) for f in ("set_source", "set_sink", "get_source_stats"))

    def set_source(self, slot, lo, hi, per_cell, mode="add", every=1, vel=None, seed=0):
        """A persistent source over the inclusive index box [lo, hi]: mode "add" puts per_cell new points in every eligible
        cell, "fill" tops every eligible cell up to per_cell; at the end of step t iff t % every == 0.  vel=None: the
        velocity is interpolated from the grid; else the fixed (x, y, z)."""
        src = Source()
        src.lo[:] = [int(x) for x in lo]
        src.hi[:] = [int(x) for x in hi]
        src.per_cell = int(per_cell)
        src.mode = {"add": 0, "fill": 1}[mode]
        src.every = int(every)
        src.vel_mode = 1 if vel is None else 0
        if vel is not None:
            src.vel[:] = [float(x) for x in vel]
        src.seed = int(seed)
        check(c_set_source(self._h, int(slot), C.byref(src)))

    def clear_source(self, slot):
        check(c_set_source(self._h, int(slot), None))

    def set_sink(self, slot, lo, hi):
        """Remove, at the end of every step, the particles whose base cell round(p) lies in the inclusive index box [lo, hi]."""
        l3 = (C.c_int32 * 3)(*[int(x) for x in lo])
        h3 = (C.c_int32 * 3)(*[int(x) for x in hi])
        check(c_set_sink(self._h, int(slot), l3, h3))

    def clear_sink(self, slot):
        check(c_set_sink(self._h, int(slot), None, None))

    def source_stats(self):
        """(On a decomposed handle: global numbers, the same on every rank.)"""
        v = [C.c_int64() for _ in range(4)]
        check(c_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("emitted_last", "removed_last", "emitted_total", "removed_total"), (x.value for x in v)))

    return set_source, clear_source, set_sink, clear_sink, source_stats


class FluidSim:
    """One simulation on one MI355X.  Mirrors what main() owns in the reference:
    grids + PointList + dt, and one ``step()`` = one iteration of fluid.cc:1378-1490."""

    def __init__(self, n=121, device=0, precision="fp64", **kw):
        p = Params()
        check(lib.fluid_default_params(C.byref(p)))
        p.n = n
        p.device = device
        p.precision = {"fp64": 0, "fp32": 1}[precision]
        for k, v in kw.items():
            if k == "gravity":
                p.gravity[0], p.gravity[1], p.gravity[2] = v
            elif k == "preconditioner":
                p.preconditioner = {"mg": 0, "jacobi": 1}[v]
            elif k == "solve_start":
                p.solve_start = {"warm": 0, "zero": 1}[v]
            elif k == "mg_precision":
                p.mg_precision = {"fp32": 0, "fp64": 1}[v]
            elif k == "dist_solve":
                p.dist_solve = {"auto": 0, "decomposed": 1, "replicated": 2}[v]
            elif hasattr(p, k):
                setattr(p, k, v)
            else:
                raise TypeError(f"unknown parameter {k}")
        self.params = p
        self.n = n
        self.precision = precision
        self.lo, self.hi = grid_bounds(n)
        self._h = C.c_void_p()
        check(lib.fluid_create(C.byref(p), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.fluid_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- scene -------------------------------------------------------------------------
    def set_solid(self, solid):
        s = np.ascontiguousarray(solid, dtype=np.uint8).reshape(-1)
        assert s.size == self.n ** 3
        check(lib.fluid_set_solid(self._h, s.ctypes.data_as(C.c_void_p)))

    def upload_particles(self, pos, vel=None):
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        v = None
        if vel is not None:
            vel = np.ascontiguousarray(vel, dtype=np.float64).reshape(-1, 3)
            assert vel.shape == pos.shape
            v = vel.ctypes.data_as(C.c_void_p)
        check(lib.fluid_upload_particles(self._h, pos.shape[0], pos.ctypes.data_as(C.c_void_p), v))

    def upload_particles_ids(self, pos, vel, ids):
        """Like upload_particles with caller-chosen ids (uint32, unique): the ids, not the upload order, break the ties of
        the counting sort, so the same set uploaded in another order with the same ids gives the same sums bit for bit."""
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        vel = np.ascontiguousarray(vel, dtype=np.float64).reshape(-1, 3)
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        assert vel.shape == pos.shape and ids.shape[0] == pos.shape[0]
        check(lib.fluid_upload_particles_ids(self._h, pos.shape[0], pos.ctypes.data_as(C.c_void_p), vel.ctypes.data_as(C.c_void_p),
                                             ids.ctypes.data_as(C.c_void_p)))

    def download_particles(self):
        n = lib.fluid_num_particles(self._h)
        pos = np.empty((n, 3), dtype=np.float64)
        vel = np.empty((n, 3), dtype=np.float64)
        check(lib.fluid_download_particles(self._h, pos.ctypes.data_as(C.c_void_p), vel.ctypes.data_as(C.c_void_p)))
        return pos, vel

    @property
    def num_particles(self):
        return lib.fluid_num_particles(self._h)

    @property
    def dt(self):
        d = C.c_double()
        check(lib.fluid_get_dt(self._h, C.byref(d)))
        return d.value

    @dt.setter
    def dt(self, v):
        check(lib.fluid_set_dt(self._h, float(v)))

    # ---- particle sources and sinks (single GPU; include/fluid_hip.h) ---------------------
    def add_particles(self, pos, vel=None):
        """Append particles after the live ones (pids np .. np+n-1).  vel=None: the reference's interpFromGrid
        (fluid.cc:883-894) over the grid velocities of the last completed step."""
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        v = None
        if vel is not None:
            vel = np.ascontiguousarray(vel, dtype=np.float64).reshape(-1, 3)
            assert vel.shape == pos.shape
            v = vel.ctypes.data_as(C.c_void_p)
        check(lib.fluid_add_particles(self._h, pos.shape[0], pos.ctypes.data_as(C.c_void_p), v))

    set_source, clear_source, set_sink, clear_sink, source_stats = source_methods("fluid_")

    # ---- step + phases -----------------------------------------------------------------
    def step(self):
        st = StepStats()
        check(lib.fluid_step(self._h, C.byref(st)))
        return st.as_dict()

    def p2g(self):
        check(lib.fluid_p2g(self._h))

    def flags_index(self):
        check(lib.fluid_flags_index(self._h))

    def rhs_div(self, which=0):
        check(lib.fluid_rhs_div(self._h, which))

    def solve(self):
        check(lib.fluid_solve(self._h))

    def vel_update(self):
        check(lib.fluid_vel_update(self._h))

    def pressure_pass(self):
        e = C.c_double()
        check(lib.fluid_pressure_pass(self._h, C.byref(e)))
        return e.value

    def flip_advect(self):
        check(lib.fluid_flip_advect(self._h))

    def stats(self):
        st = StepStats()
        check(lib.fluid_get_stats(self._h, C.byref(st)))
        return st.as_dict()

    # ---- fields ------------------------------------------------------------------------
    def _solver_dtype(self):
        return np.float64 if self.precision == "fp64" else np.float32

    def field(self, fid):
        if fid in (FIELD.SEARCH, FIELD.Q):
            dt, comps = self._solver_dtype(), 1
        else:
            dt, comps = _FIELD_DTYPE[fid]
        n = self.n
        arr = np.empty((comps, n, n, n) if comps > 1 else (n, n, n), dtype=dt)
        check(lib.fluid_download_field(self._h, fid, arr.ctypes.data_as(C.c_void_p), arr.nbytes))
        return arr

    def upload_field(self, fid, arr):
        if fid in (FIELD.SEARCH, FIELD.Q):
            dt = self._solver_dtype()
        else:
            dt = _FIELD_DTYPE[fid][0]
        a = np.ascontiguousarray(arr, dtype=dt)
        check(lib.fluid_upload_field(self._h, fid, a.ctypes.data_as(C.c_void_p), a.nbytes))

    # ---- output as non-zero leaves (single GPU; include/fluid_hip.h) -----------------------
    def output_snapshot(self):
        """Enqueue a leaf snapshot of FIELD.OUTPUT as it is now; a step() called next overlaps its copy to the host."""
        check(lib.fluid_output_snapshot(self._h))

    def output_wait(self):
        """The oldest snapshot not yet waited for, as a LeafGrid (copied out of the handle's pinned buffer)."""
        g = LeafGridC()
        check(lib.fluid_output_wait(self._h, C.byref(g)))
        return _leaf_grid_copy(g)

    def output_stats(self):
        v = [C.c_int64() for _ in range(3)]
        check(lib.fluid_output_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("leaves_in_grid", "leaves_listed", "bytes_to_host"), (x.value for x in v)))

    # ---- liquid surface: narrow-band level set of the particles (single GPU; include/fluid_hip.h) ----
    def sdf_snapshot(self, radius, half_width, smooth=None, attr=False):
        """Enqueue the level set of the particles as they are now (spheres of `radius`, band of `half_width`, both in voxels);
        a step() called next overlaps the copy to the host.  smooth=(width, iterations[, offset]): box-filtered and offset on
        the device first (include/fluid_hip.h, "liquid surface, smoothed").  attr=True: with the closest particle's id and
        velocity per voxel ("liquid surface, attributes"; sdf_wait_attr returns them)."""
        p = SdfParams(float(radius), float(half_width))
        if attr:
            f = None if smooth is None else C.byref(_sdf_filter_of(smooth))
            check(lib.fluid_sdf_snapshot_attr(self._h, C.byref(p), f))
        elif smooth is None:
            check(lib.fluid_sdf_snapshot(self._h, C.byref(p)))
        else:
            check(lib.fluid_sdf_snapshot_filtered(self._h, C.byref(p), C.byref(_sdf_filter_of(smooth))))

    def sdf_set_track(self, normalize, trim=True, grow=False, scheme="first"):
        """A setting of the handle: every later snapshot given smooth= renormalises (`normalize` passes, 0..8; the library's
        default is 3) and, with `trim`, trims the level set after every box iteration and every offset step (include/fluid_hip.h,
        "liquid surface, renormalised").  sdf_set_track(None): off, the default.  grow=True: every track begins with a dilation of
        the band ("liquid surface, grown band"; it needs normalize >= 1 and the trim, which the next filtered snapshot checks);
        grow is passed on as it is, so an integer other than 0 / 1 is the library's FLUID_ERR_ARG.  scheme: "first" (first-order
        upwind, the default), "hjweno5" (the library's own default, "liquid surface, renormalised: HJWENO5") or a number, passed
        on as it is."""
        t = None if normalize is None else SdfTrack(int(normalize), int(bool(trim)), _sdf_scheme_of(scheme))
        check(lib.fluid_sdf_set_track(self._h, None if t is None else C.byref(t)))
        check(lib.fluid_sdf_set_track_grow(self._h, int(grow)))

    def sdf_set_filter_kind(self, kind):
        """A setting of the handle: every later snapshot given smooth= runs the passes of `kind` ("box", the default; "median",
        "laplacian", "curvature"; or a FLUID_SDF_FILTER_* number) in place of the box passes (include/fluid_hip.h, "liquid
        surface, flows").  The width the kind admits is checked by the next filtered snapshot."""
        check(lib.fluid_sdf_set_filter_kind(self._h, _sdf_kind_of(kind)))

    def sdf_set_surface(self, kind="spheres", influence=None):
        """A setting of the handle: every later level-set, mesh and render snapshot takes the level set of `kind`: "spheres" (the
        default: the union of spheres) or "averaged" (the distance to the weighted average of the particle positions within
        `influence` voxels, 0 < influence <= 4, never outside the spheres; include/fluid_hip.h, "liquid surface, averaged
        positions").  A number is passed on as it is.  Under "averaged" attr=True snapshots are the library's FLUID_ERR_STATE."""
        if kind is None:
            check(lib.fluid_sdf_set_surface(self._h, None))
            return
        sf = _sdf_surface_of(kind, influence)
        check(lib.fluid_sdf_set_surface(self._h, C.byref(sf)))

    def sdf_set_trails(self, shutter, delta=1.0, radius_min=0.5, max_instances=16):
        """A setting of the handle: every later level-set, mesh and render snapshot stamps each particle as a chain of at most
        `max_instances` spheres along -velocity over the time `shutter` (the step's dt: the path of the last step), spaced by
        `delta` radii / 2 and shrinking from the snapshot's radius to `radius_min` voxels, which must not exceed it
        (include/fluid_hip.h, "liquid surface, velocity trails").  sdf_set_trails(None): off, the default.  Under trails attr=True
        snapshots are the library's FLUID_ERR_STATE."""
        if shutter is None:
            check(lib.fluid_sdf_set_trails(self._h, None))
            return
        t = SdfTrails(float(shutter), float(delta), float(radius_min), int(max_instances), 0)
        check(lib.fluid_sdf_set_trails(self._h, C.byref(t)))

    def sdf_trails_stats(self):
        """Of the last snapshot under sdf_set_trails: the live particles expanded and the instances made (before the in-grid test)."""
        a, b = C.c_int64(), C.c_int64()
        check(lib.fluid_sdf_trails_stats(self._h, C.byref(a), C.byref(b)))
        return {"particles": a.value, "instances": b.value}

    def sdf_snapshot_trails(self, radius, half_width, shutter, delta=1.0, radius_min=0.5, max_instances=16):
        """Enqueue the level set of the velocity trails of the particles as they are now (of a DistFluidSim: this rank's live
        particles, global origins, every leaf their instances reach), the trails given here and not by a setting: no setting of the
        handle is read or changed (include/fluid_hip.h, "liquid surface, velocity trails (decomposed runs)").  A plain record in the
        level set's two slots: sdf_wait() takes it and merge_sdf_grids joins the ranks' exactly."""
        p = SdfParams(float(radius), float(half_width))
        t = SdfTrails(float(shutter), float(delta), float(radius_min), int(max_instances), 0)
        check(lib.fluid_dist_sdf_snapshot_trails(self._h, C.byref(p), C.byref(t)))

    def sdf_dist_trails_stats(self):
        """Of the last sdf_snapshot_trails: the live particles expanded and the instances made (before the in-grid test); zeros
        before the first.  sdf_trails_stats keeps reporting the last snapshot under sdf_set_trails."""
        a, b = C.c_int64(), C.c_int64()
        check(lib.fluid_dist_sdf_trails_stats(self._h, C.byref(a), C.byref(b)))
        return {"particles": a.value, "instances": b.value}

    def sdf_snapshot_avg(self, radius, half_width, influence):
        """Enqueue the rank record of the averaged-position surface of the particles as they are now: squared distances and
        weighted sums per voxel, the surface given here and not by a setting (include/fluid_hip.h, "liquid surface, averaged
        positions (decomposed runs)").  Shares the level set's two slots with sdf_snapshot."""
        p, sf = SdfParams(float(radius), float(half_width)), SdfSurface(1, 0, float(influence))
        check(lib.fluid_dist_sdf_snapshot_avg(self._h, C.byref(p), C.byref(sf)))

    def sdf_wait_avg(self):
        """The oldest level-set snapshot not yet waited for, which must be one of sdf_snapshot_avg, as an SdfAvgPart
        (merge_sdf_avg_grids joins the ranks')."""
        a = SdfAvgPartC()
        check(lib.fluid_dist_sdf_wait_avg(self._h, C.byref(a)))
        return _sdf_avg_part_copy(a)

    def sdf_wait(self):
        """The oldest level-set snapshot not yet waited for, as an SdfGrid (copied out of the handle's pinned buffer)."""
        g = SdfGridC()
        check(lib.fluid_sdf_wait(self._h, C.byref(g)))
        return _sdf_grid_copy(g)

    def sdf_wait_attr(self):
        """(SdfGrid, SdfAttr) of the oldest level-set snapshot not yet waited for; the SdfAttr is None if that snapshot was
        taken without attr=True (or lists no leaf)."""
        g, a = SdfGridC(), SdfAttrC()
        check(lib.fluid_sdf_wait_attr(self._h, C.byref(g), C.byref(a)))
        grid = _sdf_grid_copy(g)
        if not a.id:
            return grid, None
        k = a.n_leaves
        ids = np.ctypeslib.as_array(C.cast(a.id, C.POINTER(C.c_uint32)), shape=(k, 512)).copy()
        vel = np.ctypeslib.as_array(C.cast(a.velocity, C.POINTER(C.c_float)), shape=(k, 3, 512)).copy()
        return grid, SdfAttr(ids, vel)

    def sdf_stats(self):
        v = [C.c_int64() for _ in range(3)]
        check(lib.fluid_sdf_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("leaves_in_grid", "leaves_listed", "bytes_to_host"), (x.value for x in v)))

    # ---- liquid surface as a mesh: surface nets of the level set (single GPU; include/fluid_hip.h) ----
    def mesh_snapshot(self, radius, half_width, smooth=None, attr=False, normals=False, triangles=False):
        """Enqueue the surface nets of the level set of the particles as they are now (parameters as sdf_snapshot, `smooth`
        included); a step() called next overlaps the copy to the host.  attr=True: with a velocity per vertex (mesh_wait_attr).
        normals=True / triangles=True: with a unit normal per vertex / two triangles per quad (mesh_wait_ex)."""
        p = SdfParams(float(radius), float(half_width))
        if normals or triangles:
            f = None if smooth is None else C.byref(_sdf_filter_of(smooth))
            what = (MESH.VELOCITY if attr else 0) | (MESH.NORMALS if normals else 0) | (MESH.TRIANGLES if triangles else 0)
            check(lib.fluid_mesh_snapshot_ex(self._h, C.byref(p), f, what))
        elif attr:
            f = None if smooth is None else C.byref(_sdf_filter_of(smooth))
            check(lib.fluid_mesh_snapshot_attr(self._h, C.byref(p), f))
        elif smooth is None:
            check(lib.fluid_mesh_snapshot(self._h, C.byref(p)))
        else:
            check(lib.fluid_mesh_snapshot_filtered(self._h, C.byref(p), C.byref(_sdf_filter_of(smooth))))

    def mesh_wait(self):
        """The oldest mesh snapshot not yet waited for: (vertices (nv, 3) float32 in index space, quads (nq, 4) uint32), copied
        out of the handle's pinned buffer."""
        m = MeshC()
        check(lib.fluid_mesh_wait(self._h, C.byref(m)))
        v, q = np.empty((m.n_vertices, 3), np.float32), np.empty((m.n_quads, 4), np.uint32)
        if m.n_vertices:
            v[:] = np.ctypeslib.as_array(C.cast(m.vertices, C.POINTER(C.c_float)), shape=(m.n_vertices, 3))
        if m.n_quads:
            q[:] = np.ctypeslib.as_array(C.cast(m.quads, C.POINTER(C.c_uint32)), shape=(m.n_quads, 4))
        return v, q

    def mesh_wait_attr(self):
        """(vertices, quads, velocity (nv, 3) float32) of the oldest mesh snapshot not yet waited for; velocity is None if that
        snapshot was taken without attr=True (or has no vertex)."""
        m, a = MeshC(), MeshAttrC()
        check(lib.fluid_mesh_wait_attr(self._h, C.byref(m), C.byref(a)))
        v, q = np.empty((m.n_vertices, 3), np.float32), np.empty((m.n_quads, 4), np.uint32)
        if m.n_vertices:
            v[:] = np.ctypeslib.as_array(C.cast(m.vertices, C.POINTER(C.c_float)), shape=(m.n_vertices, 3))
        if m.n_quads:
            q[:] = np.ctypeslib.as_array(C.cast(m.quads, C.POINTER(C.c_uint32)), shape=(m.n_quads, 4))
        vel = None
        if a.velocity:
            vel = np.ctypeslib.as_array(C.cast(a.velocity, C.POINTER(C.c_float)), shape=(m.n_vertices, 3)).copy()
        return v, q, vel

    def mesh_wait_ex(self):
        """(vertices, quads, {"velocity", "normals", "triangles"}) of the oldest mesh snapshot not yet waited for: (nv, 3) float32,
        (nv, 3) float32, (2 nq, 3) uint32, each None if that snapshot was taken without it (or has no vertex / no quad)."""
        m, e = MeshC(), MeshExC()
        check(lib.fluid_mesh_wait_ex(self._h, C.byref(m), C.byref(e)))
        v, q = np.empty((m.n_vertices, 3), np.float32), np.empty((m.n_quads, 4), np.uint32)
        if m.n_vertices:
            v[:] = np.ctypeslib.as_array(C.cast(m.vertices, C.POINTER(C.c_float)), shape=(m.n_vertices, 3))
        if m.n_quads:
            q[:] = np.ctypeslib.as_array(C.cast(m.quads, C.POINTER(C.c_uint32)), shape=(m.n_quads, 4))
        parts = {"velocity": None, "normals": None, "triangles": None}
        for name in ("velocity", "normals"):
            if getattr(e, name):
                parts[name] = np.ctypeslib.as_array(C.cast(getattr(e, name), C.POINTER(C.c_float)), shape=(m.n_vertices, 3)).copy()
        if e.triangles:
            parts["triangles"] = np.ctypeslib.as_array(C.cast(e.triangles, C.POINTER(C.c_uint32)), shape=(e.n_triangles, 3)).copy()
        return v, q, parts

    def mesh_stats(self):
        v = [C.c_int64() for _ in range(3)]
        check(lib.fluid_mesh_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("vertices", "quads", "bytes_to_host"), (x.value for x in v)))

    # ---- liquid surface as an image: the level set ray-cast on the device (single GPU; include/fluid_hip.h) ----
    def render_snapshot(self, radius, half_width, camera, smooth=None, shade=None, rgb=True, depth=False, normals=False):
        """Enqueue an image of the level set of the particles as they are now (parameters as sdf_snapshot, `smooth` included),
        seen through `camera` (a Camera: camera() or camera_look_at()); a step() called next overlaps the copy to the host.
        shade: None (white on black), a Shade, or (base, background)."""
        p = SdfParams(float(radius), float(half_width))
        f = None if smooth is None else C.byref(_sdf_filter_of(smooth))
        sh = _shade_of(shade)
        check(lib.fluid_render_snapshot(self._h, C.byref(p), f, C.byref(camera), None if sh is None else C.byref(sh),
                                        _render_what(rgb, depth, normals)))

    def render_wait(self):
        """The oldest render snapshot not yet waited for: {"rgb" (H, W, 3) uint8, "depth" (H, W) float32, "normals" (H, W, 3)
        float32, "n_hit"}, copied out of the handle's pinned buffer; None for a part the snapshot was taken without."""
        m = ImageC()
        check(lib.fluid_render_wait(self._h, C.byref(m)))
        H, W = m.height, m.width
        out = {"rgb": None, "depth": None, "normals": None, "n_hit": m.n_hit}
        if m.rgb:
            out["rgb"] = np.ctypeslib.as_array(C.cast(m.rgb, C.POINTER(C.c_uint8)), shape=(H, W, 3)).copy()
        if m.depth:
            out["depth"] = np.ctypeslib.as_array(C.cast(m.depth, C.POINTER(C.c_float)), shape=(H, W)).copy()
        if m.normals:
            out["normals"] = np.ctypeslib.as_array(C.cast(m.normals, C.POINTER(C.c_float)), shape=(H, W, 3)).copy()
        return out

    def render_stats(self):
        v = [C.c_int64() for _ in range(3)]
        check(lib.fluid_render_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("pixels", "hits", "bytes_to_host"), (x.value for x in v)))

    def extrapolate(self):
        """fluid.cc:705-802 after p2g(): velocities for every cell inside W (dead code in the reference; optional here).  Returns the passes run."""
        n = C.c_int32()
        check(lib.fluid_extrapolate(self._h, C.byref(n)))
        return n.value

    def droplets(self):
        """The closed pockets of the last step's pressure system that were solved apart (include/fluid_hip.h, fluid_get_droplets):
        an (n, 64) int64 array of cell indices per component, ascending, padded with -1."""
        n = C.c_int32(0)
        check(lib.fluid_get_droplets(self._h, C.byref(n), None, 0))
        cells = np.full((max(n.value, 0), 64), -1, dtype=np.int64)
        if n.value > 0:
            check(lib.fluid_get_droplets(self._h, C.byref(n), cells.ctypes.data_as(C.c_void_p), n.value))
        return cells

    def resample(self, per_cell):
        """fluid.cc:1053-1080: at most per_cell particles per base cell (upload order); returns how many were parked outside the grid."""
        n = C.c_int64()
        check(lib.fluid_resample(self._h, int(per_cell), C.byref(n)))
        return n.value

    def stencil_apply(self, reps=1, box=0):
        ms = C.c_float()
        check(lib.fluid_stencil_apply(self._h, reps, box, C.byref(ms)))
        return ms.value

    def stencil_apply_hbm(self, reps=1, box=0, footprint_bytes=1 << 30):
        """The same sweep rotating over separate copies of (s, q, flags) that together exceed `footprint_bytes`
        (well above the 256 MiB Infinity Cache): returns (ms per launch, sets used)."""
        ms, ns = C.c_float(), C.c_int32()
        check(lib.fluid_stencil_apply_hbm(self._h, reps, box, footprint_bytes, C.byref(ns), C.byref(ms)))
        return ms.value, ns.value

    # ---- profiling -----------------------------------------------------------------------
    def profile_enable(self, sample_every):
        check(lib.fluid_profile_enable(self._h, sample_every))

    def profile_reset(self):
        check(lib.fluid_profile_reset(self._h))

    def profile_read(self, klass):
        nl, ns = C.c_int64(), C.c_int64()
        ms, cells = C.c_double(), C.c_double()
        check(lib.fluid_profile_read(self._h, klass, C.byref(nl), C.byref(ns), C.byref(ms), C.byref(cells)))
        return {"launches": nl.value, "sampled": ns.value, "total_ms": ms.value, "cells": cells.value}
