#!/usr/bin/env python3
"""Generates tests/golden/spline_ref.npz: outputs of the reference's own spline() (fluid.cc:22-37, compiled as it is into
oracle/_ref/libspline_ref.so by `make -C oracle ref`) on every 7th point of test_kat.sweep() and on its branch-edge points,
so that the spline known-answer tests run where oracle/_ref was not built."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import oracle  # noqa: E402
from test_kat import sweep, sweep_edges  # noqa: E402

x, e = sweep()[::7], sweep_edges()
ref, ref_e = oracle.ref_spline(x), oracle.ref_spline(e)
assert ref is not None, "build oracle/_ref first: make -C oracle ref"
np.savez_compressed(os.path.join(HERE, "spline_ref.npz"), x_count=x.size, x_sum=x.sum(), spline_every7=ref, edges=e, spline_edges=ref_e)
print("spline_ref.npz", os.path.getsize(os.path.join(HERE, "spline_ref.npz")))
