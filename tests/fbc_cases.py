"""
Host-side tables of the flux-boundary-identification tests (vn_set_fluxbc_basis, vn_set_fluxbc_learn): the five cases of
tests/test_flux_bc_gpu.py (nF = 1, 30, 40, 60, 25) and three copies of its 1D+t case at nF = 2, 33 and 257 (an odd count, no
multiple of 4: the one-row mix kernel; 257: a second row block), their seeded basis streams and amplitudes, the fp64 reference of
tests/fbc_ref.py computed once per (case, J_l, J_c) and never modified, and the bar of the amplitude gradient.  Plain module (no
GPU, no pytest marks), shared by tests/test_fbc_host.py and tests/test_fbc_gpu.py.

Inputs: those of tests/test_flux_bc_gpu.setup (seed 11: tests/parity_cases.synth; flux rows flux_rows(12, ...), rounded to fp32 as the
engine holds them); parameters glorot seed 3 plus the 0.05 N(0, 1) perturbation of that setup.

Basis (the formula of tests/bic_cases.basis on x = the flux rows' X[:, :dim], default_rng(SEED0 + 97 i + 64 J_l + J_c)): stream j
is, by j % 3, a Gaussian bump, a wave sin(k_j . x + p_j), or a bump times (x_0 - c_j0) / s_j (J = 1: the last).  Layout [J_l + J_c, nF],
"flux, then robin"; every stream runs over all nF rows (the engine does not know a wall from a Robin edge).  Amplitudes N(0, 1).
Both rounded to fp32.

(J_l, J_c) = (2, 1) runs on every case; (1, 0), (0, 1), (40, 24), (37, 27) and (5, 4) with mask [1,0,1,0,0, 1,0,0,1] on cases 1 and
2 only.  (40, 24) fills the cap of 64 with the part boundary between two groups of eight streams (40 = 5 x 8); (37, 27) puts it
inside the fifth group, as (2, 1) and (5, 4) have it inside the first.

Large-row cases (indices N_CASES + k, not in PAIRS): the 1D+t case with the network [24, 31] and nF = 65 538 -- just above the 256 x
256 rows a capped reduction grid takes one row per thread of, nF % 4 == 2 -- and 262 152; (J_l, J_c) = (8, 1) and (5, 4), entries 0,
7 and 8 learnt (both sides of the boundary between the stream groups of eight; with (5, 4) entry 7 and 8 are Robin streams, with
(8, 1) entry 7 is the last flux stream).

The bar, per component j:   |g_j - g64_j| <= GRAD_RTOL * max(|g64_j|, COND_FLOOR * S_j)
with S_j = sum_k |row contribution| (tests/fbc_ref.py).  The floor may be the binding branch for at most BINDING_FRAC of all
components over all (case, J_l, J_c); tests/test_fbc_host.py asserts that, and that the reference evaluated in fp32 on the CPU stays
within the bar, from the CPU numbers alone.
"""
import functools

import numpy as np
import torch

from oracle import tf1_graph as og
from tests import fbc_ref
from tests import test_flux_bc_gpu as fg
from tests.bic_cases import BINDING_FRAC, COND_FLOOR          # noqa: F401  (the project's floor and binding fraction)
from tests.parity_cases import GRAD_RTOL, synth

SEED0 = 211
BI_DIM_VAL = 2.0                                # as tests/test_flux_bc_gpu.setup registers the rows


def _with_nF(case, nF, widths=None):
    c = list(case)
    c[7] = nF
    if widths is not None:
        c[2] = widths
    return tuple(c)


CASES = list(fg.CASES) + [_with_nF(fg.CASES[1], n) for n in (2, 33, 257)]
IDS = list(fg.IDS) + ['1dt_nF2', '1dt_nF33', '1dt_nF257']
N_CASES = len(CASES)
WIDE = [1, 2]                                   # the cases that also run the J variants
MASK9 = [1, 0, 1, 0, 0, 1, 0, 0, 1]             # of (5, 4)
VARIANTS = [(1, 0), (0, 1), (40, 24), (37, 27), (5, 4)]
PAIRS = [(i, 2, 1) for i in range(N_CASES)] + [(i, Jl, Jc) for i in WIDE for (Jl, Jc) in VARIANTS]
BIG = [_with_nF(fg.CASES[1], n, [24, 31]) for n in (65538, 262152)]
BIG_IDS = ['1dt_nF65538', '1dt_nF262152']
BIG_J = [(8, 1), (5, 4)]
BIG_MASK = [1, 0, 0, 0, 0, 0, 0, 1, 1]
BIG_PAIRS = [(N_CASES + k, Jl, Jc) for k in range(len(BIG)) for (Jl, Jc) in BIG_J]


def case(i):
    return CASES[i] if i < N_CASES else BIG[i - N_CASES]


def case_id(i):
    return IDS[i] if i < N_CASES else BIG_IDS[i - N_CASES]


def mask_of(i, Jl, Jc):
    if i >= N_CASES:
        return list(BIG_MASK)
    return list(MASK9) if (Jl, Jc) == (5, 4) else [1] * (Jl + Jc)


@functools.lru_cache(maxsize=None)
def inputs(i):
    """(d, fx): the interior / BC data of tests/parity_cases.synth and the flux rows, fp32, read-only."""
    d_in, dim, widths, q, n_k, nB, bDof, nF, td, act, integW = case(i)
    d = synth(11, d_in, dim, widths, q, n_k, nB, bDof, integW=integW)
    fx = {k: np.asarray(v).astype(np.float32) for k, v in fg.flux_rows(12, d_in, dim, nF).items()}
    for v in fx.values():
        v.setflags(write=False)
    return d, fx


@functools.lru_cache(maxsize=None)
def theta(i):
    """The parameters tests/test_flux_bc_gpu.setup gives the engine (init_params(seed=3) is og.glorot_init, bit for bit)."""
    d_in, widths = case(i)[0], case(i)[2]
    flat = og.glorot_init(d_in, widths, 3)
    flat = flat + 0.05 * np.random.default_rng(5).standard_normal(flat.size).astype(np.float32)
    flat.setflags(write=False)
    return flat


@functools.lru_cache(maxsize=None)
def basis(i, Jl, Jc):
    """(S [Jl + Jc, nF] fp32 stream-major, amp [Jl + Jc] fp32-exact doubles) of case i."""
    dim, J = case(i)[1], Jl + Jc
    x = inputs(i)[1]['X'][:, :dim].astype(np.float64)
    rng = np.random.default_rng(SEED0 + 97 * i + 64 * Jl + Jc)
    S = np.empty((J, x.shape[0]), dtype=np.float32)
    for j in range(J):
        c, s = rng.uniform(-0.7, 0.7, dim), rng.uniform(0.3, 0.8)
        k, p = rng.uniform(1.0, 3.0, dim), rng.uniform(0.0, 2.0 * np.pi)
        bump = np.exp(-np.sum((x - c) ** 2, axis=1) / (2.0 * s * s))
        kind = 2 if J == 1 else j % 3
        S[j] = (bump, np.sin(x @ k + p), bump * (x[:, 0] - c[0]) / s)[kind]
    amp = rng.standard_normal(J).astype(np.float32).astype(np.float64)
    S.setflags(write=False)
    amp.setflags(write=False)
    return S, amp


def mixed(i, Jl, Jc, amp=None):
    """(coef, label) = (coef0 + H^T a, label0 + Gamma^T a) in fp64."""
    S, a = basis(i, Jl, Jc)
    a = a if amp is None else np.asarray(amp, dtype=np.float64)
    fx = inputs(i)[1]
    S64 = S.astype(np.float64)
    return fx['coef'].astype(np.float64) + a[Jl:] @ S64[Jl:], fx['label'].astype(np.float64) + a[:Jl] @ S64[:Jl]


def fma_mix(base, streams, amp):
    """What vn_learnt_mix_kernel forms, restated: fp32, from base, j ascending, one fused multiply-add per stream (the product of
    two fp32 numbers is exact in fp64, so each step is one fp64 addition rounded to fp32, as in tests/bic_cases.fma_mix)."""
    s = np.asarray(base, dtype=np.float32).reshape(-1)
    for j in range(len(streams)):
        s = (np.float64(np.float32(amp[j])) * streams[j].astype(np.float64) + s.astype(np.float64)).astype(np.float32)
    return s


def fma_mixed(i, Jl, Jc, amp):
    """(coef, label) as the engine mixes them in fp32."""
    S = basis(i, Jl, Jc)[0]
    fx = inputs(i)[1]
    return fma_mix(fx['coef'], S[Jl:], amp[Jl:]), fma_mix(fx['label'], S[:Jl], amp[:Jl])


def evaluate(i, Jl, Jc, amp=None, dtype=torch.float64, flat=None):
    """tests/fbc_ref.evaluate of case i at the amplitudes amp (default: the case's) and the parameters flat (default: the case's)."""
    d_in, dim, widths, act = case(i)[0], case(i)[1], case(i)[2], case(i)[9]
    S, a = basis(i, Jl, Jc)
    d, fx = inputs(i)
    f = np.float64 if dtype == torch.float64 else np.float32
    return fbc_ref.evaluate((theta(i) if flat is None else flat).astype(f), d_in, widths, dim, fx['X'].astype(f), fx['normal'].astype(f),
                            fx['coef'].astype(f), fx['label'].astype(f), S.astype(f), Jl, (a if amp is None else np.asarray(amp)).astype(f),
                            BI_DIM_VAL, float(d['w'][0]), act, dtype)


@functools.lru_cache(maxsize=None)
def reference64(i, Jl, Jc):
    """(F, dF/dtheta, amplitude gradient [J], S [J]) of case i in fp64 at the case's own amplitudes."""
    out = evaluate(i, Jl, Jc)
    for a in out[1:]:
        a.setflags(write=False)
    return out


def bars(g64, S):
    """The allowed |g - g64| per component."""
    return GRAD_RTOL * np.maximum(np.abs(g64), COND_FLOOR * S)
