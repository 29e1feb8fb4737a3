"""
Per-tensor gradient comparison (test infrastructure, imported by the tests; not a conftest).

The suite's original gradient bar is ONE number over the flat parameter vector, |g - g_ref|_inf / |g_ref|_inf.  The output
layer's gradient sets that maximum; a deep sigmoid net's input-layer gradient is orders of magnitude smaller, so an input-layer
gradient that is zero, has the wrong sign or has two input rows swapped can pass it.  Here every block of the flat layout
(oracle/tf1_graph.layer_dims: [W_1 (row-major [in,out]), b_1, ..., w_o, b_o]) is judged against its OWN size:

    err_b = max|g_b - g_ref_b| / max(|g_ref_b|_inf, FLOOR * |g_ref|_inf),      FLOOR = 1e-7

The floor only guards blocks whose reference is (nearly) exactly zero: a W_1 row at 1e-6 of the maximum is still judged
relative to its own size.  Blocks: one per input row of W_1, named by its input column (x0, x1, x2, then t for a
time-dependent problem, then p0, p1, ... for the remaining, MOR-parameter, columns; in0, in1, ... when the caller does not
say which columns are space), then b1, W2, b2, ..., W<L>, b<L>, then Wo, bo (the output layer).

A block above the bar passes only under the fp32-conditioning rule of tests/fuzz_routes.py, applied per block: when the
oracle's own fp32 evaluation deviates from its fp64 evaluation on that block by dev32_b, the block may deviate by up to
2 x dev32_b.  The fp32 oracle is evaluated only when some block misses the bar.
"""
import numpy as np

FLOOR = 1e-7


def input_names(d_in, dim=None, td=True):
    """Names of the input columns: x0.. (space), t (time, when td), p0.. (the rest); in0.. when dim is None."""
    if dim is None:
        return ['in%d' % k for k in range(d_in)]
    names = ['x%d' % k for k in range(min(dim, d_in))]
    if td and len(names) < d_in:
        names.append('t')
    names += ['p%d' % k for k in range(d_in - len(names))]
    return names


def param_blocks(d_in, widths, dim=None, td=True):
    """(name, slice) pairs that partition [0, param_count(d_in, widths)) in the flat parameter layout."""
    blocks = []
    off = 0
    fan_in = d_in
    L = len(widths)
    for l, h in enumerate(list(widths) + [1]):
        out = l == L
        if l == 0:
            for k, name in enumerate(input_names(d_in, dim, td)):
                blocks.append(('W1.' + name, slice(off + k * h, off + (k + 1) * h)))
        else:
            blocks.append(('Wo' if out else 'W%d' % (l + 1), slice(off, off + fan_in * h)))
        off += fan_in * h
        blocks.append(('bo' if out else 'b%d' % (l + 1), slice(off, off + h)))
        off += h
        fan_in = h
    return blocks


def _scale(gref):
    return max(float(np.max(np.abs(gref))) if np.size(gref) else 0.0, 1e-300)


def block_errors(g, gref, d_in, widths, dim=None, td=True):
    """{block name: max|g_b - gref_b| / max(|gref_b|_inf, 1e-7 |gref|_inf)} in layout order (g may carry trailing loss
    scalars: only the first param_count entries are read)."""
    blocks = param_blocks(d_in, widths, dim, td)
    P = blocks[-1][1].stop
    g = np.asarray(g, dtype=np.float64)[:P]
    gref = np.asarray(gref, dtype=np.float64)[:P]
    floor = FLOOR * _scale(gref)
    return {name: float(np.max(np.abs(g[s] - gref[s]))) / max(float(np.max(np.abs(gref[s]))), floor, 1e-300)
            for name, s in blocks}


def global_error(g, gref):
    gref = np.asarray(gref, dtype=np.float64)
    P = gref.size
    return float(np.max(np.abs(np.asarray(g, dtype=np.float64)[:P] - gref))) / _scale(gref)


def _check(g, gref, d_in, widths, bar, dev32, dim, td, global_bar, what, rec):
    P = param_blocks(d_in, widths, dim, td)[-1][1].stop
    g, gref = np.asarray(g, dtype=np.float64)[:P], np.asarray(gref, dtype=np.float64)[:P]    # drop trailing loss scalars
    gerr = global_error(g, gref)
    errs = block_errors(g, gref, d_in, widths, dim, td)
    worst = max(errs, key=errs.get)
    rec = {} if rec is None else rec          # filled before any assertion: a failing case still leaves its record
    rec.update(grad_global=gerr, worst_block=worst, worst_block_err=errs[worst])
    gb = bar if global_bar is None else global_bar
    assert gerr <= gb, '%s: global gradient error %.3e > %.1e' % (what, gerr, gb)
    over = [b for b, e in errs.items() if e > bar]
    if not over:
        return rec
    d32 = dev32() if dev32 is not None else None
    sc = _scale(gref)
    shares = {name: float(np.max(np.abs(gref[s]))) / sc
              for name, s in param_blocks(d_in, widths, dim, td)}
    for b in over:
        allowed = bar if d32 is None else max(bar, 2.0 * d32[b])
        assert errs[b] <= allowed, (
            '%s: gradient block %s deviates by %.3e of its own size > bar %.1e%s (block holds %.2e of |g_ref|_inf)'
            % (what, b, errs[b], bar, '' if d32 is None else ' (fp32 oracle on this block: %.2e)' % d32[b], shares[b]))
        rec.setdefault('conditioned', {})[b] = {'err': errs[b], 'fp32_oracle': d32[b]}
    return rec


def assert_grad_close(g, gref, d_in, widths, bar, g32=None, dim=None, td=True, global_bar=None, what='gradient', rec=None):
    """g against the fp64 oracle's gradient gref: the global bar (global_bar, default bar) AND every block <= bar, or
    <= 2 x the fp32 oracle's deviation on that block (g32: a callable returning the fp32 oracle's gradient, evaluated only
    when a block misses the bar).  Returns the record (also written into `rec` when given, before any assertion): global error,
    worst block and its error, and under 'conditioned' the blocks that needed the fp32 rule."""
    dev32 = None if g32 is None else (lambda: block_errors(g32(), gref, d_in, widths, dim, td))
    return _check(g, gref, d_in, widths, bar, dev32, dim, td, global_bar, what, rec)


def assert_pair_close(ga, gb, d_in, widths, bar, dev32=None, dim=None, td=True, global_bar=None, what='gradient pair',
                      rec=None):
    """Pairwise form (route against route, sum of shards against the full gradient): ga against gb, each block on gb's
    scale.  dev32: a callable returning the fp32 oracle's per-block deviation from fp64 (fp32_deviation), evaluated only when
    a block misses the bar."""
    return _check(ga, gb, d_in, widths, bar, dev32, dim, td, global_bar, what, rec)


def fp32_deviation(g32, g64, d_in, widths, dim=None, td=True):
    """Per-block deviation of the oracle's fp32 gradient from its fp64 gradient: the conditioning of each block."""
    return block_errors(g32, g64, d_in, widths, dim, td)


def column_errors(v, vref):
    """Per column of [n, k] arrays (e.g. grad u, one spatial direction per column): max|v_c - vref_c| / max(|vref_c|_inf,
    1e-7 |vref|_inf)."""
    v = np.asarray(v, dtype=np.float64).reshape(len(vref), -1)
    vref = np.asarray(vref, dtype=np.float64).reshape(len(vref), -1)
    floor = FLOOR * _scale(vref)
    return [float(np.max(np.abs(v[:, c] - vref[:, c]))) / max(float(np.max(np.abs(vref[:, c]))), floor, 1e-300)
            for c in range(vref.shape[1])]


def assert_columns_close(v, vref, bar, what='grad u', v32=None):
    """Every column of v on its own scale (column_errors) <= bar, or <= 2 x the fp32 oracle's deviation on that column (v32: a
    callable returning the fp32 oracle's values, evaluated only when a column misses the bar); returns the worst column error."""
    errs = column_errors(v, vref)
    d32 = column_errors(v32(), vref) if v32 is not None and max(errs, default=0.0) > bar else None
    for c, e in enumerate(errs):
        allowed = bar if d32 is None else max(bar, 2.0 * d32[c])
        assert e <= allowed, '%s: column %d deviates by %.3e of its own size > bar %.1e%s' % (
            what, c, e, bar, '' if d32 is None else ' (fp32 oracle on this column: %.2e)' % d32[c])
    return max(errs) if errs else 0.0
