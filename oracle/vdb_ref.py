"""ORACLE — TEST INFRASTRUCTURE ONLY (see oracle/vdb_ref.cpp header).

ctypes wrapper of OpenVDB's own level-set operators over a mock dense grid (oracle/_ref/libvdb_ref.so, compiled at build time
from the reference's math/FiniteDifference.h, Stencils.h, Operators.h and tools/LevelSetTracker.h, LevelSetFilter.h).  `ref` is
None where that library was not built.  Every pass takes a dense C-order (n, n, n) float32 `val`, a bool `act`, the background and
dx, and returns the new values: active voxels from the pass (Jacobi), inactive ones copied.  Imported only by tests/.
"""
import ctypes as C
import os

import numpy as np

_SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_ref", "libvdb_ref.so")
_P, _F, _I, _L = C.c_void_p, C.c_float, C.c_int, C.c_long
F = np.float32
FIRST, HJWENO5 = 0, 4


def _ptr(a):
    return a.ctypes.data_as(_P)


class VdbRef:
    def __init__(self, path=_SO):
        l = self._l = C.CDLL(path)
        l.vdb_ref_normalize.argtypes = [_P, _P, _I, _F, _F, _I, _P]
        l.vdb_ref_normalize.restype = _I
        l.vdb_ref_laplacian.argtypes = [_P, _P, _I, _F, _F, _P]
        l.vdb_ref_laplacian.restype = None
        l.vdb_ref_curvature.argtypes = [_P, _P, _I, _F, _F, _P]
        l.vdb_ref_curvature.restype = None
        l.vdb_ref_median.argtypes = [_P, _P, _I, _F, _I, _P]
        l.vdb_ref_median.restype = None
        l.vdb_ref_median_of_eight.argtypes = [_P, _P, _I, _F, _P]
        l.vdb_ref_median_of_eight.restype = None
        l.vdb_ref_box.argtypes = [_P, _P, _I, _F, _I, _I, _P]
        l.vdb_ref_box.restype = _I
        l.vdb_ref_box_order.argtypes = [_P, _P]
        l.vdb_ref_box_order.restype = None
        l.vdb_ref_offset_steps.argtypes = [_F, _F, _P, _I]
        l.vdb_ref_offset_steps.restype = _I
        l.vdb_ref_consts.argtypes = [_F, _P]
        l.vdb_ref_consts.restype = None
        l.vdb_ref_weno5.argtypes = [_P] * 5 + [_L, _P]
        l.vdb_ref_weno5.restype = None
        l.vdb_ref_axis_diffs.argtypes = [_P, _L, _P, _P]
        l.vdb_ref_axis_diffs.restype = None
        l.vdb_ref_voxel.argtypes = [_P, _P, _P, _L, _F, _I, _P]
        l.vdb_ref_voxel.restype = _I

    @staticmethod
    def _grid(val, act):
        val = np.ascontiguousarray(val, dtype=F)
        n = val.shape[0]
        assert val.shape == (n, n, n) and np.shape(act) == (n, n, n)
        return val, np.ascontiguousarray(act, dtype=np.uint8), n, np.empty_like(val)

    def norm_pass(self, val, act, bg, dx, scheme=FIRST):
        val, a, n, out = self._grid(val, act)
        assert self._l.vdb_ref_normalize(_ptr(val), _ptr(a), n, F(bg), F(dx), scheme, _ptr(out)) == 0
        return out

    def laplacian_pass(self, val, act, bg, dx):
        val, a, n, out = self._grid(val, act)
        self._l.vdb_ref_laplacian(_ptr(val), _ptr(a), n, F(bg), F(dx), _ptr(out))
        return out

    def curvature_pass(self, val, act, bg, dx):
        val, a, n, out = self._grid(val, act)
        self._l.vdb_ref_curvature(_ptr(val), _ptr(a), n, F(bg), F(dx), _ptr(out))
        return out

    def median_pass(self, val, act, bg, W):
        val, a, n, out = self._grid(val, act)
        self._l.vdb_ref_median(_ptr(val), _ptr(a), n, F(bg), int(W), _ptr(out))
        return out

    def median_of_eight(self, val, act, bg):
        """BaseStencil::median of the eight values at (i..i+1, j..j+1, k..k+1): the rank an even count takes."""
        val, a, n, out = self._grid(val, act)
        self._l.vdb_ref_median_of_eight(_ptr(val), _ptr(a), n, F(bg), _ptr(out))
        return out

    def box_pass(self, val, act, bg, W, axis):
        val, a, n, out = self._grid(val, act)
        assert self._l.vdb_ref_box(_ptr(val), _ptr(a), n, F(bg), int(axis), int(W), _ptr(out)) == 0
        return out

    def box_order(self):
        """(passes, names): the axes of the first, second and third pass of an iteration, and the axes boxX, boxY, boxZ average."""
        p, m = np.full(3, -1, np.int32), np.full(3, -1, np.int32)
        self._l.vdb_ref_box_order(_ptr(p), _ptr(m))
        return tuple(int(x) for x in p), tuple(int(x) for x in m)

    def offset_steps(self, offset, dx):
        buf = np.empty(4096, F)
        k = self._l.vdb_ref_offset_steps(F(offset), F(dx), _ptr(buf), len(buf))
        assert 0 <= k <= len(buf)
        return [buf[i] for i in range(k)]

    def consts(self, dx):
        """(the normaliser's dt, its 1 / dx, the Laplacian flow's dt, the curvature flow's dt), float32."""
        out = np.empty(4, F)
        self._l.vdb_ref_consts(F(dx), _ptr(out))
        return tuple(out)

    def weno5(self, v1, v2, v3, v4, v5):
        v = [np.ascontiguousarray(x, dtype=F).ravel() for x in (v1, v2, v3, v4, v5)]
        out = np.empty_like(v[0])
        self._l.vdb_ref_weno5(*[_ptr(x) for x in v], len(out), _ptr(out))
        return out

    def axis_diffs(self, u):
        u = np.ascontiguousarray(u, dtype=F)
        assert u.ndim == 2 and u.shape[0] == 7
        dm, dp = np.empty(u.shape[1], F), np.empty(u.shape[1], F)
        self._l.vdb_ref_axis_diffs(_ptr(u), u.shape[1], _ptr(dm), _ptr(dp))
        return dm, dp

    def voxel_value(self, ux, uy, uz, dx, scheme=HJWENO5):
        ux, uy, uz = (np.ascontiguousarray(u, dtype=F) for u in (ux, uy, uz))
        assert ux.ndim == 2 and ux.shape[0] == 7 and uy.shape == ux.shape and uz.shape == ux.shape
        out = np.empty(ux.shape[1], F)
        assert self._l.vdb_ref_voxel(_ptr(ux), _ptr(uy), _ptr(uz), ux.shape[1], F(dx), scheme, _ptr(out)) == 0
        return out


ref = VdbRef() if os.path.exists(_SO) else None
