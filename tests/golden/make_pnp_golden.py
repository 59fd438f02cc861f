#!/usr/bin/env python3
"""Records what the REAL reference PnP solve (oracle/_ref::ref_pnp_solve: vendored Ceres + IMUFactorPnP +
PerspectiveFactor, built from /root/reference) returns on the cases of tests/test_pnp.py -- CASES under c<seed>_*, the
edge windows under e_<name>_* -- into tests/golden/pnp_windows.npz. Only the reference's outputs are stored; the tests
regenerate the inputs from their seeds. Run where /root/reference exists:
    make -C oracle ref && python tests/golden/make_pnp_golden.py"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers as H
import test_pnp as T

lib = H.ref_lib_or_none()
assert lib is not None and hasattr(lib, "ref_pnp_solve"), "build oracle/_ref first"
cfg = H.abi.default_config()
out = {}
windows = [("c%d_" % c[0], c[0], T.make_window(cfg, *c)) for c in T.CASES]
windows += [("e_%s_" % name, name, w) for name, w in T.edge_windows(cfg).items()]
for pre, key, w in windows:
    ref, rs = T.reference(cfg, key, w)
    out[pre + "pose"], out[pre + "speed"] = ref.pose, ref.speed
    for k in T.EDGE_STAT_KEYS:
        out[pre + k] = np.asarray(rs[k])
np.savez_compressed(T.GOLDEN, **out)
print("wrote", T.GOLDEN, len(out), "arrays")
