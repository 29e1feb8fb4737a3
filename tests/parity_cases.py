"""
Host-side tables of the parity suite: the engine and steady cases, their seeded inputs and the fp64 / fp32 oracle evaluations
of them.  Plain module (no GPU, no pytest marks): the GPU parity tests (tests/test_engine_gpu.py and the modules that borrow its
cases) and the CPU tests of the per-block gradient check (tests/test_gradcheck.py) both use it.
"""
import numpy as np
import torch

from oracle import tf1_graph as og

LOSS_RTOL = 1e-5
GRAD_RTOL = 1e-4
LVEC_RTOL = 1e-4


def synth(seed, d_in, dim, widths, integNum, n_k, nB, bDof, source=False, integW=False, detJvec=False):
    rng = np.random.default_rng(seed)
    n = n_k * integNum
    d = dict(
        Input=rng.uniform(-1, 1, (n, d_in)).astype(np.float32),
        gcoef=rng.standard_normal((n, dim)).astype(np.float32),
        source=rng.standard_normal((n, 1)).astype(np.float32) if source else None,
        N1=rng.uniform(0, 1, integNum).astype(np.float32),
        dNt1=rng.standard_normal(integNum).astype(np.float32),
        integW=rng.uniform(0.5, 1.0, (1, integNum)).astype(np.float32) if integW else None,
        detJ=(rng.uniform(0.1, 0.2, (n_k, 1)).astype(np.float32) if detJvec else np.float32(0.137)),
        biInput=rng.uniform(-1, 1, (nB, d_in)).astype(np.float32),
        biLabel=rng.standard_normal((nB, 1)).astype(np.float32),
        w=np.array([3.0, 2.0, 5.0]),
    )
    d['N'] = np.tile(d['N1'], n_k).reshape(n, 1)
    d['dNt'] = np.tile(d['dNt1'], n_k).reshape(n, 1)
    return d


def oracle_eval(flat, d, d_in, dim, widths, integNum, n_k, bDof, source, integW, detJvec, time_dependent=True,
                dtype=torch.float64):
    """The oracle in fp64 (the reference), or in fp32 (dtype=torch.float32: the conditioning estimate of tests/gradcheck.py)."""
    f = np.float64 if dtype == torch.float64 else np.float32
    kw = dict(Input=d['Input'].astype(f), gcoef=d['gcoef'].astype(f),
              source=None if d['source'] is None else d['source'].astype(f),
              N=d['N'].astype(f), dNt=d['dNt'].astype(f),
              integW=None if d['integW'] is None else d['integW'].astype(f),
              intShape=[n_k, integNum],
              detJ=(d['detJ'].astype(f) if detJvec else float(d['detJ'])), detJvec=detJvec,
              biInput=d['biInput'].astype(f), biLabel=d['biLabel'].astype(f),
              bDof=bDof, biDimVal=2.0, w=d['w'], dim=dim, time_dependent=time_dependent,
              is_source=source, integWflag=integW)
    return og.loss_and_grad(flat.astype(f), d_in, widths, dtype, **kw)


CASES = [
    # d_in dim widths            integNum n_k  nB  bDof source integW detJvec
    (2, 1, [20, 20, 20],         16,      40,  50, 30,  False, False, False),
    (3, 2, [50, 50, 50, 50, 50], 64,      9,   77, 40,  False, False, False),
    (3, 2, [10, 20],             64,      5,   33, 20,  True,  False, False),
    (3, 1, [10, 20, 30],         16,      21,  19, 7,   False, False, False),   # MOR-style extra input
    (2, 1, [7],                  36,      11,  40, 13,  True,  True,  True),
    (3, 2, [64, 64, 64],         216,     3,   5,  2,   False, True,  False),
    (3, 2, [50, 50, 50, 50, 50], 64,      300, 1000, 600, False, False, False),
    (2, 1, [50, 50, 50, 50],     16,      801, 450, 400, True,  False, True),     # config-2 shaped
    (3, 2, [20, 20, 20],         64,      33,  70,  30,  True,  False, False),
    (3, 2, [32, 17],             32,      50,  10,  4,   False, True,  True),
    (2, 1, [20, 20, 20],         36,      41,  25,  9,   True,  True,  False),    # 3-point Gauss, 1D+t
    (3, 2, [50, 50, 50],         36,      17,  12,  5,   False, True,  True),
    (3, 2, [50, 50, 50],         216,     7,   40,  22,  True,  True,  False),   # 3-point Gauss, 2D+t: two-pass fused
    (3, 2, [20, 20, 20, 20],     216,     5,   9,   4,   False, True,  True),
    (3, 2, [60, 60, 60, 60],     64,      30,  50,  20,  False, False, False),   # widths 51..63: KS = 16 fused tiles
    (3, 2, [51, 63, 57],         36,      17,  12,  5,   True,  True,  True),
    (2, 1, [63, 63],             16,      90,  33,  11,  True,  False, False),
    (3, 2, [60, 60, 60, 60, 60], 64,      9,   77,  40,  False, False, False),
    (3, 2, [64, 64],             64,      6,   20,  8,   False, False, False),   # 64 wide: bias gradient by thin_bias
    (2, 1, [20],                 16,      300, 40,  25,  False, False, False),   # one hidden layer (Operator_1Dt.py:156)
    (3, 2, [50],                 64,      40,  30,  10,  True,  False, True),
    (3, 2, [60],                 36,      21,  30,  10,  False, True,  False),
    (3, 2, [50] * 6,             64,      12,  30,  10,  False, False, False),   # six hidden layers, 50 wide
    (3, 2, [64, 64, 64, 64],     64,      40,  70,  30,  True,  False, True),    # 64 wide, several tiles
    (2, 1, [64, 40, 64],         16,      77,  33,  11,  False, False, False),   # 64 wide next to narrower layers
    (3, 2, [64],                 36,      21,  30,  10,  False, True,  False),   # one 64-wide layer: output bias per lane
    (3, 2, [64] * 6,             64,      12,  30,  10,  True,  False, False),   # six 64-wide layers: flush image over the weight images
    (3, 2, [60, 64, 51, 64, 56, 63], 36,  17,  12,  5,   False, True,  True),
    # KS = 8 (widths 21..32): padding-only k-steps / row tiles are branched over on the layers' real widths, the bias row rides at the
    # position of feature 31 unless the input side is exactly 32 wide (then thin_bias + the serial flush): ADVICE r3
    (3, 2, [31, 32, 17],         64,      21,  30,  10,  False, False, False),
    (2, 1, [17, 32, 32, 21],     16,      90,  33,  11,  True,  False, True),
    (3, 1, [32, 32],             16,      40,  19,  7,   False, True,  False),
    # 4..8 inputs, MOR-shaped (VarNet.inpDim = dim + time + MOR parameters): d_in > 3 leaves thin_wgrad_in for the cooperative
    # input-layer tiles of vn_fused16, and inputs 4..7 ride in the second input k-step (KS0 = 2); deep nets make W1's gradient
    # small, so the per-block check of tests/gradcheck.py is what judges the input layer here
    (4, 1, [20, 20, 20],         16,      40,  50,  30,  True,  False, False),   # 1D+t + 2 parameters
    (5, 2, [50, 50, 50, 50, 50], 64,      30,  77,  40,  False, False, False),   # the bench network, 2D+t + 2 parameters
    (6, 2, [64, 64, 64],         216,     5,   40,  22,  True,  True,  False),   # 2D+t + 3 parameters, two-pass route
    (7, 3, [50] * 6,             64,      12,  30,  10,  False, False, True),    # six hidden layers, 3D+t + 3 parameters
    (8, 3, [20, 20, 20, 20],     216,     4,   20,  9,   False, True,  True),    # 3D+t + 4 parameters, two-pass route
    (6, 1, [33, 50, 41, 64],     16,      50,  33,  11,  True,  False, True),    # ragged
    (5, 1, [50] * 6,             16,      90,  40,  20,  True,  True,  False),   # six hidden layers, 1D+t + 3 parameters
    (8, 2, [50, 50],             64,      21,  30,  10,  True,  True,  True),
    (7, 2, [60, 64, 51, 64, 56, 63], 36,  17,  12,  5,   False, True,  True),    # six ragged layers, widths 51..64
    (8, 3, [20, 20, 20],         16,      60,  40,  20,  False, False, False),
    (6, 2, [32, 32, 32],         64,      20,  30,  10,  True,  False, False),   # KS = 8 widths
]


STEADY = [
    # time-independent: no IC rows, no dNt term (TFModel.py:537,646-650); nonzero dNt tables and rows behind bDof are fed
    # all the same (a route that read them would be caught: the oracle ignores both for a steady problem)
    # d_in dim widths        integNum n_k nB  bDof act        integW detJvec
    (1, 1, [20, 20],         4,       37, 2,  2,   'sigmoid', False, False),
    (2, 2, [20, 20, 20],     16,      50, 60, 60,  'sigmoid', False, False),
    (2, 2, [50, 50, 50],     16,      129, 33, 33, 'sigmoid', False, False),
    (2, 2, [7, 9],           36,      11, 20, 20,  'sigmoid', True,  False),
    (1, 1, [20],             6,       40, 2,  2,   'sigmoid', True,  False),   # 1D three-point Gauss: 21 test functions per 128-row tile
    (1, 1, [50] * 5,         6,       77, 2,  2,   'tanh',    True,  True),
    (2, 2, [64, 64, 64],     16,      60, 40, 25,  'sigmoid', False, True),    # rows behind bDof: ignored by a steady loss
    (2, 2, [60, 64, 51],     36,      30, 30, 12,  'tanh',    True,  False),   # widths 51..64
    (3, 2, [20, 20, 20],     16,      40, 30, 20,  'sigmoid', False, False),   # d_in = dim + 1: the extra column is NOT time
    (3, 2, [60, 64, 51],     36,      17, 20, 20,  'sigmoid', True,  True),
    (2, 1, [64, 64, 64],     4,       300, 2, 2,   'tanh',    False, True),    # d_in = dim + 1 in 1D
    (2, 2, [50] * 5,         36,      400, 60, 60, 'sigmoid', True,  False),   # several hundred test functions
    (2, 2, [128, 128],       16,      30, 40, 20,  'sigmoid', False, False),   # beyond the kernels: layer by layer
    (1, 1, [300],            6,       25, 2,  2,   'tanh',    True,  True),
    (8, 3, [50, 50, 50, 50],     16,  30, 40, 20,  'sigmoid', True,  True),    # d_in = dim + 5 MOR parameters
    (6, 2, [64, 51, 64],     36,      20, 30, 12,  'tanh',    False, False),   # d_in = dim + 4
]


def steady_inputs(case, seed=7):
    """Inputs and parameters of a STEADY case (host only)."""
    d_in, dim, widths, q, n_k, nB, bDof, act, has_w, detJvec = case
    rng = np.random.default_rng(seed)
    n = n_k * q
    d = dict(Input=rng.uniform(-1, 1, (n, d_in)).astype(np.float32),
             gcoef=rng.standard_normal((n, dim)).astype(np.float32),
             source=rng.standard_normal((n, 1)).astype(np.float32),
             N1=rng.uniform(0, 1, q).astype(np.float32))
    d['integW'] = rng.uniform(0.5, 1, (1, q)).astype(np.float32) if has_w else None
    d['biInput'] = rng.uniform(-1, 1, (nB, d_in)).astype(np.float32)
    d['biLabel'] = rng.standard_normal((nB, 1)).astype(np.float32)
    d['dNt1'] = rng.standard_normal(q).astype(np.float32)
    d['detJ'] = rng.uniform(0.01, 0.03, (n_k, 1)).astype(np.float32) if detJvec else np.float32(0.02)
    d['w'] = np.array([4.0, 0.0, 3.0])                              # VarNet.py:1132: IC weight 0
    flat = og.glorot_init(d_in, widths, 2)                          # = the engine's init_params(seed=2), bit for bit
    flat = flat + 0.05 * np.random.default_rng(5).standard_normal(flat.size).astype(np.float32)
    return d, flat


def steady_oracle(flat, d, case, dtype=torch.float64):
    d_in, dim, widths, q, n_k, nB, bDof, act, has_w, detJvec = case
    n = n_k * q
    f = np.float64 if dtype == torch.float64 else np.float32
    f64 = lambda a: None if a is None else a.astype(f)
    return og.loss_and_grad(
        flat.astype(f), d_in, widths, dtype, Input=f64(d['Input']), gcoef=f64(d['gcoef']),
        source=f64(d['source']), N=np.tile(d['N1'], n_k).reshape(n, 1).astype(f),
        dNt=np.tile(d['dNt1'], n_k).reshape(n, 1).astype(f), integW=f64(d['integW']), intShape=[n_k, q],
        detJ=f64(d['detJ']) if detJvec else float(d['detJ']), detJvec=detJvec, biInput=f64(d['biInput']),
        biLabel=f64(d['biLabel']), bDof=bDof, biDimVal=1.5, w=d['w'], dim=dim, time_dependent=False, is_source=True,
        integWflag=has_w, activation=act)

