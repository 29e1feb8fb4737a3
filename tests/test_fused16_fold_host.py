"""
Arithmetic of the folded edge tile (vn_fused16_common.h, three_folded / fold_rows), emulated in numpy: every f32 operand is cut
exactly into three bf16 pieces by truncation (split2), the other row tiles sum six of the nine piece products (hh, hm, mh, hl, lh,
mm), the folded tile sums all nine.  For a 50-term dot product (one out-feature of a 50-wide layer) over random rows:
  * the two forms differ by no more than the dropped terms' bound, 2^-24 * sum |w x|;
  * the folded form is never further from the exact product than the six-term form.
The sums are taken exactly (math.fsum over exactly representable products), so the bounds are those of the split alone.
"""
import math

import numpy as np

K, ROWS = 50, 10000


def trunc_bf16(x):
    return (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def split3(x):
    """h + m + l == x exactly: 3 x 8 significand bits, each piece the truncation of what the previous ones left"""
    h = trunc_bf16(x)
    r = x - h
    m = trunc_bf16(r)
    s = r - m
    return h, m, trunc_bf16(s)


def test_split_is_exact():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(100000) * np.exp(rng.uniform(-8, 8, 100000))).astype(np.float32)
    h, m, l = split3(x)
    assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), x.astype(np.float64))
    for p in (h, m, l):
        assert np.array_equal(trunc_bf16(p), p)                      # every piece is a bf16 value


def test_folded_nine_terms_against_six_terms_and_exact():
    rng = np.random.default_rng(1)
    w = (rng.standard_normal((ROWS, K)) * 0.4).astype(np.float32)    # weights of one out-feature
    x = rng.uniform(-1, 1, (ROWS, K)).astype(np.float32)             # activations (tanh range; sigmoid's lies inside)
    W = [p.astype(np.float64) for p in split3(w)]
    X = [p.astype(np.float64) for p in split3(x)]
    prod = {(i, j): W[i] * X[j] for i in range(3) for j in range(3)}  # bf16 x bf16: exact in f64
    six_terms = [(1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0)]
    exact_p = w.astype(np.float64) * x.astype(np.float64)            # f32 x f32: exact in f64
    scale = np.abs(exact_p).sum(axis=1)
    nine_p = np.concatenate([prod[ij] for ij in prod], axis=1)
    six_p = np.concatenate([prod[ij] for ij in six_terms], axis=1)
    worst_diff = worst_nine = worst_six = 0.0
    for r in range(ROWS):
        exact = math.fsum(exact_p[r])
        nine = math.fsum(nine_p[r])
        six = math.fsum(six_p[r])
        e9, e6 = abs(nine - exact), abs(six - exact)
        assert abs(nine - six) <= 2.0 ** -24 * scale[r], (r, nine, six, scale[r])
        assert e9 <= e6, (r, e9, e6)
        worst_diff = max(worst_diff, abs(nine - six) / scale[r])
        worst_nine = max(worst_nine, e9 / scale[r])
        worst_six = max(worst_six, e6 / scale[r])
    print('folded - six-term %.2e, folded - exact %.2e, six-term - exact %.2e (relative to sum |w x|)' % (worst_diff, worst_nine, worst_six))
