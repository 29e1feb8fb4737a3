"""
Host-side tables of the field-identification tests (vn_set_field_basis, vn_set_field_learn): the eleven cases of
tests/source_cases.py (variant 'all': the three polynomial terms, D(u) = (0.7, 0.4, 0.3) among them, registered next to the
source), their seeded basis streams and amplitudes, the fp64 reference of tests/field_ref.py computed once per (case, J) and never
modified, and the bar of the amplitude gradient.  Plain module (no GPU, no pytest marks), shared by tests/test_field_host.py and
tests/test_field_gpu.py.

Basis (default_rng(SEED + 97 i + J), in the case's own coordinates x = Input[:, :dim] in [-1, 1]^dim), laid out [J, nT, dim].  A
scalar profile f(x; kind) is, by kind,
  0  a Gaussian bump exp(-|x - c|^2 / (2 s^2)), c in U(-0.7, 0.7), s in U(0.3, 0.8);
  1  a wave sin(k . x + p), k in U(1, 3) per dimension: sign-changing, so the row sum carries cancellation;
  2  a bump times (x_0 - c_0) / s: sign-changing around its own centre.
Stream j with j even is of the diffusivity kind, G_j[r, :] = f_j(x_r) gcoef[r, :] (chi dN/dx: the direction of the case's own
gcoef); j odd is of the velocity kind, G_j[r, d] = gscale f_{j,d}(x_r) with an independent profile per component and the scale of
the case's gcoef -- so that leaving the basis out moves every output far beyond its bar (tests/test_field_host.py).
The kind of profile is j % 3 (J = 1: kind 2).  Amplitudes: N(0, 1).  Both rounded to fp32: the engine registers fp32.

J = 3 runs on every case; J of 1, 32 and 5 (mask [1, 0, 1, 0, 0]) on cases 0 and 6 only.

The bar, per component j:   |g_j - g64_j| <= GRAD_RTOL * max(|g64_j|, COND_FLOOR * S_j)
with S_j = sum_r |row contribution| (tests/field_ref.py).  The floor may be the binding branch for at most BINDING_FRAC of all
components over all (case, J); tests/test_field_host.py asserts that, and that the reference evaluated in fp32 on the CPU stays
within the bar, from the CPU numbers alone.
"""
import functools

import numpy as np
import torch

from tests import field_ref
from tests import source_cases as sc
from tests.parity_cases import GRAD_RTOL

COND_FLOOR = 0.01
BINDING_FRAC = 0.05
SEED = 83                                      # (chosen so that the conditions of tests/test_field_host.py hold: DESIGN.md section 23)
N_CASES = sc.N_CASES
IDS = list(sc.IDS)
EMPTY = list(sc.EMPTY)
WIDE = [0, 6]                                  # the cases that also run J = 1, 32 and 5
MASK5 = [1, 0, 1, 0, 0]
JMAX = 32
# (case, J) of every gradient check
PAIRS = [(i, 3) for i in range(N_CASES)] + [(i, J) for i in WIDE for J in (1, JMAX, 5)]

case, inputs, theta, ref_kw, terms_of, coefs_of, s0_of = sc.case, sc.inputs, sc.theta, sc.ref_kw, sc.terms_of, sc.coefs_of, sc.s0_of


def _profile(rng, x, kind):
    dim = x.shape[1]
    c, s = rng.uniform(-0.7, 0.7, dim), rng.uniform(0.3, 0.8)
    k, p = rng.uniform(1.0, 3.0, dim), rng.uniform(0.0, 2.0 * np.pi)
    bump = np.exp(-np.sum((x - c) ** 2, axis=1) / (2.0 * s * s))
    return (bump, np.sin(x @ k + p), bump * (x[:, 0] - c[0]) / s)[kind]


@functools.lru_cache(maxsize=None)
def basis(i, J):
    """(G [J, nT, dim] fp32 stream-major, amp [J] fp32-exact doubles) of case i."""
    dim = case(i)[1]
    gscale = sc.dt.CASES[sc.base(i)][13]
    d = inputs(i)
    x = d['Input'][:, :dim].astype(np.float64)
    g0 = d['gcoef'].astype(np.float64)
    rng = np.random.default_rng(SEED + 97 * i + J)
    G = np.empty((J, x.shape[0], dim), dtype=np.float32)
    for j in range(J):
        kind = 2 if J == 1 else j % 3
        if j % 2 == 0:
            G[j] = _profile(rng, x, kind)[:, None] * g0
        else:
            for dd in range(dim):
                G[j, :, dd] = gscale * _profile(rng, x, kind)
    amp = rng.standard_normal(J).astype(np.float32).astype(np.float64)
    G.setflags(write=False)
    amp.setflags(write=False)
    return G, amp


def mixed(i, J, amp=None):
    """g0 + sum_j b_j G_j in fp64, [nT, dim]."""
    G, b = basis(i, J)
    b = b if amp is None else np.asarray(amp, dtype=np.float64)
    return inputs(i)['gcoef'].astype(np.float64) + np.tensordot(b, G.astype(np.float64), axes=1)


def fma_mix(i, J, amp, g0=None):
    """The stream the engine's mix kernel forms, restated: fp32, from g0, j ascending, one fused multiply-add per stream (the
    product of two fp32 numbers is exact in fp64, so each step is one fp64 addition rounded to fp32 -- up to double rounding, which
    the bitwise tests would show)."""
    G = basis(i, J)[0]
    g = (inputs(i)['gcoef'] if g0 is None else g0).astype(np.float32)
    for j in range(J):
        g = (np.float64(np.float32(amp[j])) * G[j].astype(np.float64) + g.astype(np.float64)).astype(np.float32)
    return g


def evaluate(i, J, amp=None, dtype=torch.float64, nldiff_coef=None, with_basis=True):
    G, b = basis(i, J)
    nldiff, nlflux, reaction = terms_of(i)
    coef = coefs_of(i).copy()
    if nldiff_coef is not None:
        coef[6:9] = nldiff_coef
    return field_ref.evaluate(theta(i), case(i)[0], case(i)[2], inputs(i)['gcoef'], G if with_basis else None, b if amp is None else amp,
                              coef, nldiff, nlflux, reaction, dtype, **ref_kw(i, dtype))


@functools.lru_cache(maxsize=None)
def reference64(i, J):
    """(loss pieces, theta-gradient, amplitude gradient [J], S [J]) of case i in fp64 at the case's own amplitudes."""
    out = evaluate(i, J)
    for a in out[1:]:
        a.setflags(write=False)
    return out


def bars(g64, S):
    """The allowed |g - g64| per component."""
    return GRAD_RTOL * np.maximum(np.abs(g64), COND_FLOOR * S)
