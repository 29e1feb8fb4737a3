"""
Cases of the learnt weight scales (vn_set_reparam): networks, shapes, modes, seeded inputs, synthetic step sequences and the fp64
reference of (g_V, g_s) on the oracle.  Plain module (no GPU, no pytest marks), shared by tests/test_reparam_host.py and
tests/test_reparam_gpu.py.

Networks: one hidden neuron, five, [20, 20, 20] tanh, ragged [10, 20, 30], the bench network 5 x 50, two 64-wide layers (every lane
of the stage's waves owns a column, sixteen rows per wave) and 8 x 50 (nine workgroups; beyond the generic kernels).  d_in 2 and 3;
(n_k, q) = (1, 4): one test function, (3, 6): rows no multiple of anything, (2, 216): the two-pass route; nB = 33.
"""
import numpy as np
import torch

from oracle import tf1_graph as og
from tests import reparam_ref as rr

NB, BDOF, BIDIMVAL, DETJ = 33, 20, 2.0, 0.137
W = np.array([3.0, 2.0, 5.0])
LR, LR_S = 1e-3, 2e-3                       # the scales' rate differs from the network's: a mixed-up rate shows
STEPS = 8

CASES = [
    # d_in dim widths             act        n_k  q
    (2, 1, [1],                   'sigmoid', 1,   4),
    (3, 2, [5],                   'sigmoid', 3,   6),
    (2, 1, [20, 20, 20],          'tanh',    3,   6),
    (3, 2, [10, 20, 30],          'sigmoid', 2,   216),
    (3, 2, [50, 50, 50, 50, 50],  'sigmoid', 3,   6),
    (2, 1, [64, 64],              'sigmoid', 1,   4),
    (3, 2, [64, 64],              'tanh',    2,   216),
    (3, 2, [50] * 8,              'sigmoid', 3,   6),
    (2, 1, [50] * 8,              'tanh',    1,   4),
]
IDS = ['%din_%s_%s_%dx%d' % (c[0], 'x'.join(map(str, c[2])) if len(set(c[2])) > 1 or len(c[2]) < 4 else '%dx%d' % (len(c[2]), c[2][0]),
                            c[3], c[4], c[5]) for c in CASES]
GENERIC_OK = [i for i, c in enumerate(CASES) if len(c[2]) <= 6]           # the generic kernels take at most six hidden layers

MODES = [('rwf', 'neuron', 1.0)] + [('slope', per, n) for per in ('neuron', 'layer') for n in (1.0, 2.0, 5.0, 10.0)]
MODE_IDS = ['rwf' if m == 'rwf' else 'slope_%s_n%g' % (per, n) for m, per, n in MODES]
# (case, mode) pairs of the trajectory tests: every mode family, one to nine workgroups, tied layers 30 and 50 wide
TRAJECTORIES = [(0, 0), (2, 0), (5, 0), (4, 3), (1, 2), (3, 8), (7, 6)]


def layout(i, k):
    mode, per, n = MODES[k]
    return rr.Layout(mode, per, n, CASES[i][0], CASES[i][2])


def inputs(i):
    d_in, dim, widths, act, n_k, q = CASES[i]
    rng = np.random.default_rng(100 + i)
    n = n_k * q
    d = dict(Input=rng.uniform(-1, 1, (n, d_in)).astype(np.float32), gcoef=rng.standard_normal((n, dim)).astype(np.float32),
             N1=rng.uniform(0, 1, q).astype(np.float32), dNt1=rng.standard_normal(q).astype(np.float32),
             biInput=rng.uniform(-1, 1, (NB, d_in)).astype(np.float32), biLabel=rng.standard_normal((NB, 1)).astype(np.float32))
    d['N'] = np.tile(d['N1'], n_k).reshape(n, 1)
    d['dNt'] = np.tile(d['dNt1'], n_k).reshape(n, 1)
    return d


def theta(i):
    """glorot weights with non-zero biases (a bias of zero would hide whether it is in a group)."""
    d_in, widths = CASES[i][0], CASES[i][2]
    flat = og.glorot_init(d_in, widths, 3 + i)
    return (flat + 0.05 * np.random.default_rng(200 + i).standard_normal(flat.size)).astype(np.float32)


def scales(i, k):
    return rr.default_s(layout(i, k), np.random.default_rng(300 + 16 * i + k))


def loss_of(i, lay, V, s, dtype=torch.float64, d=None):
    """The oracle loss as a torch function of (V, s): theta_eff = f(s)[group] * V, unflattened without leaving the graph.
    d: other inputs than inputs(i) (the de-duplicated batch's rows)."""
    d_in, dim, widths, act, n_k, q = CASES[i]
    d = inputs(i) if d is None else d
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    fs = torch.exp(s) if lay.mode == 'rwf' else lay.n * s
    grp = torch.as_tensor(np.maximum(lay.group, 0))
    fe = torch.where(torch.as_tensor(lay.group >= 0), fs[grp], torch.ones((), dtype=dtype))
    th = fe * V
    params, off = [], 0
    for fi, fo in rr.layer_dims(d_in, widths):
        params.append((th[off:off + fi * fo].reshape(fi, fo), th[off + fi * fo:off + fi * fo + fo]))
        off += fi * fo + fo
    return og.loss_fun(params, T(d['Input']), T(d['gcoef']), None, T(d['N']), T(d['dNt']), None, [n_k, q], DETJ, False, T(d['biInput']),
                       T(d['biLabel']), BDOF, BIDIMVAL, W, dim, time_dependent=True, is_source=False, integWflag=False, activation=act)


def autograd_of(i, lay, V, s, dtype=torch.float64, d=None):
    """(components, d loss / d V, d loss / d s) by torch autograd through theta_eff(V, s)."""
    Vt = torch.as_tensor(np.asarray(V), dtype=dtype).clone().requires_grad_(True)
    st = torch.as_tensor(np.asarray(s), dtype=dtype).clone().requires_grad_(True)
    out = loss_of(i, lay, Vt, st, dtype, d)
    out['loss'].backward()
    res = {k: float(out[k].detach()) for k in ('loss', 'BCloss', 'ICloss', 'varLoss')}
    return res, Vt.grad.numpy().astype(np.float64), st.grad.numpy().astype(np.float64)


def oracle_grad(i, theta_eff, dtype=torch.float64):
    """(components, d loss / d theta_eff) of the plain oracle at theta_eff."""
    d_in, dim, widths, act, n_k, q = CASES[i]
    d = inputs(i)
    f = np.float64 if dtype == torch.float64 else np.float32
    return og.loss_and_grad(np.asarray(theta_eff).astype(f), d_in, widths, dtype, Input=d['Input'].astype(f), gcoef=d['gcoef'].astype(f),
                            source=None, N=d['N'].astype(f), dNt=d['dNt'].astype(f), integW=None, intShape=[n_k, q], detJ=DETJ,
                            detJvec=False, biInput=d['biInput'].astype(f), biLabel=d['biLabel'].astype(f), bDof=BDOF,
                            biDimVal=BIDIMVAL, w=W, dim=dim, time_dependent=True, is_source=False, integWflag=False, activation=act)


def sequence(i, k, steps=STEPS):
    """A synthetic sequence for the step alone: V from theta(i) factorised with scales(i, k), and per step a gradient of mixed
    sizes (a slowly turning direction plus noise, per-entry scales over three decades), as fp32."""
    lay = layout(i, k)
    rng = np.random.default_rng(400 + 16 * i + k)
    s0 = scales(i, k)
    V0 = lay.factorise(theta(i), s0).astype(np.float32)
    size = 10.0 ** rng.uniform(-3, 0, lay.P)
    base = rng.standard_normal(lay.P)
    gs = [(size * (base + 0.5 * rng.standard_normal(lay.P))).astype(np.float32) for _ in range(steps)]
    return lay, V0, s0, gs
