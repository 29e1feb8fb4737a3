"""
ORACLE tooling (test infrastructure): golden fixture for the host-side data assembly of a STEADY 2D problem
(ADPDE's default, timeDependent=False: no time column, no IC rows, no dNt table) -- PolygonDomain2D, two- and
three-point Gauss (integNum 16 and 36), variable diffusivity / velocity / source.

It runs the reference's own NumPy code by the TF-placeholder procedure of oracle/gen_golden_assembly.py, which it
imports, and writes tests/golden/assembly_steady.npz (same key layout as assembly.npz, which it leaves untouched).
Runs only where the reference sources are present (GPU tests never read them); the .npz is committed.

    python oracle/gen_golden_steady.py
"""
import os
import sys

sys.dont_write_bytecode = True      # importing the reference must not write __pycache__ into its (read-only) tree

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import gen_golden_assembly as ga  # noqa: E402

VERTS = np.array([[0.0, -0.5], [0.0, -0.2], [0.0, 0.2], [0.0, 0.5], [2.0, 0.5], [2.0, -0.5]])


def pde_kwargs():
    """Steady 2D data, shared with tests/test_assembly_golden.py (functions of x alone; t keeps the reference's default)."""
    return dict(
        BCs=[[], [0.0, 1.0, 1.0], [], [], [], []],
        diff=lambda x, t=0: 1e-2 * (1.0 + x[:, 1:2] ** 2),
        vel=lambda x, t=0: np.hstack([1.0 + 0.0 * x[:, 0:1], 0.1 * x[:, 0:1]]),
        source=lambda x, t=0: np.sin(x[:, 0:1]) * (1.0 + x[:, 1:2]),
        d_diff=lambda x, t=0: np.hstack([0.0 * x[:, 0:1], 2e-2 * x[:, 1:2]]),
        cEx=lambda x, t=0: np.sin(x[:, 0:1]) * (1.0 + x[:, 1:2]))


KEYS = ('2d_steady_ip2', '2d_steady_ip3')


def main():
    RV, RVU, RD, RA = ga.load_reference()
    st = {}
    ga.PU[0] = 1
    for key, ip in zip(KEYS, (2, 3)):
        vn = RV.VarNet(RA.ADPDE(RD.PolygonDomain2D(VERTS), **pde_kwargs()), layerWidth=[5], discNum=[4, 3], bDiscNum=3,
                       tDiscNum=[], integPnum=ip)
        assert not vn.PDE.timeDependent
        ga.record(st, key, vn, RVU, None, None, 1)
    path = os.path.join(ga.OUT, 'assembly_steady.npz')
    np.savez_compressed(path, **st)
    print('wrote', path, len(st), 'arrays')


if __name__ == '__main__':
    main()
