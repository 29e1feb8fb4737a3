"""
fp64 restatement of the learnt weight scales (vn_set_reparam; vn_reparam.hip, driven by apply_impl in vn_api.hip): the groups of
each mode, factorise / effective, the chain rule, the joint Adam step on (V, s) and its fp32 NumPy twin, named wrong variants, and
the bars between the device and the restatement.  Plain module (no GPU, no pytest marks), shared by tests/test_reparam_host.py and
tests/test_reparam_gpu.py; follows tests/learnt_adam_ref.py and reuses its ulp32, lr_t_of and bar.

The network the kernels evaluate is theta_eff[p] = f(s_group(p)) V[p]; an entry in no group has theta_eff = V.
    rwf    f(s) = exp(s);  one group per output neuron of EVERY layer (the output layer included); column j of W_l, weights only
    slope  f(s) = n s;     hidden layers only; column j of W_l AND b_l[j] ('neuron'), or all of W_l and b_l ('layer')
With g = d loss / d theta_eff:
    g_V[p] = f(s_group(p)) g[p],        g_s[group] = f'(s_group) sum_{p in group} V[p] g[p]
One step at counter t (lr_t of the network's rate, lr_s_t of the scales' own, both formed in double and handed over as fp32):
    Adam on V with g_V (slots m, v), Adam on s with g_s (slots ms, vs); g_V uses the scale of BEFORE the step
    theta_eff = fl32(f(s_new)) * V_new                      the scale of AFTER it, f rounded once to fp32
`Joint64` is that in double with the hyper-parameters as the kernel receives them (beta1, beta2, eps, lr_t, lr_s_t rounded to fp32,
g rounded to fp32 and widened); tests/test_reparam_host.py holds it to oracle.tf1_graph.TF1Adam at f == 1.  `Joint32` is the same in
NumPy fp32, operation by operation in the kernel's order (g_V and g_s rounded once from double, as the kernel forms them).

Bars of one step.  Values (V and s):  |device - Joint64| <= bar(before, after, lr_t) = ulp32(max(|before|, |after|)) / 2 + C lr_t,
C = C_FACTOR x MEASURED_C, MEASURED_C the largest (|Joint32 - Joint64| - ulp / 2) / lr_t over every step of every sequence of
tests/reparam_cases.py, Joint64 started from Joint32's state at each step (tests/test_reparam_host.py measures it again and fails
when it is stale).  The factor 4 covers the fused multiply-adds the device compiler may contract and NumPy does not.
Slots: slot_bar = 4.5 ulp32(max(|before|, |after|, |(1 - beta) g^k|)).  A slot is beta old + (1 - beta) g (first moment) or
beta old + (1 - beta) g g (second).  Worst case of the second, every term bounded by that scale and a relative error of 2^-24 being
at most one ulp32: the rounding of g_V / g_s themselves to fp32 moves g^2 by 2 x 2^-24 of itself (2 ulp); the product (1 - beta) g is
rounded (2^-24 relative, carried through the second product: 1 ulp); the second product, beta old and the sum are rounded once each
(3 x ulp / 2).  The first moment has fewer roundings.  (1 - beta) is exact in fp32 and in double for beta = fl32(0.9), fl32(0.999).
The NumPy twin reaches 2.9 ulp on the cases' sequences (tests/test_reparam_host.py prints it); nothing is derived from that figure.

MUTANTS: each a plausible slip of the kernel or the host path, as a variant of Joint64.
  a  bias inside an rwf group
  b  output layer left out of rwf / included in slope
  c  f' dropped from g_s
  d  `layer` granularity not tied: the scale of a layer sees the sum of its first neuron's column only
  e  g_V scaled with the scale of AFTER the step
  f  theta_eff rebuilt with the scale of BEFORE the step
  g  the s slots not carried
  h  s stepped with lr_t of t - 1 / t + 1
"""
import numpy as np

from tests.learnt_adam_ref import BETA1, BETA2, EPS, bar as _bar, f32, lr_t_of, ulp32  # noqa: F401  (re-exported)

C_FACTOR = 4.0
MEASURED_C = 1.3904592369635008e-06          # (3in_64x64_tanh_2x216, slope_neuron_n5: tests/test_reparam_host.py prints it)
C = C_FACTOR * MEASURED_C
SLOT_ULPS = 4.5

MODES = ('rwf', 'slope')
PERS = ('neuron', 'layer')


def bar(before, after, lr_t, c=None):
    return _bar(before, after, lr_t, C if c is None else c)


def slot_bar(before, after, term):
    scale = np.maximum(np.maximum(np.abs(before), np.abs(after)), np.abs(term))
    return SLOT_ULPS * ulp32(scale)


def layer_dims(d_in, widths):
    dims, fi = [], d_in
    for h in list(widths) + [1]:
        dims.append((fi, h))
        fi = h
    return dims


class Layout:
    """Groups of a mode on the network d_in -> widths -> 1, in the flat parameter layout (W_l row-major [in, out], then b_l).
    group[p]: scale index of entry p, -1: in no group; col[p]: output neuron of entry p; layer_s[l]: slice of s of layer l (empty
    where the layer is in no group).  The keyword flags build the wrong layouts of mutants a and b."""

    def __init__(self, mode, per, n, d_in, widths, rwf_bias_in=False, rwf_skip_output=False, slope_with_output=False):
        assert mode in MODES and per in PERS
        self.mode, self.per, self.n = mode, ('neuron' if mode == 'rwf' else per), float(n)
        self.d_in, self.widths = d_in, list(widths)
        self.tied = mode == 'slope' and per == 'layer'
        dims = layer_dims(d_in, widths)
        self.P = sum(i * o + o for i, o in dims)
        self.group = np.full(self.P, -1, dtype=np.int64)
        self.col = np.zeros(self.P, dtype=np.int64)
        self.layer_s, self.layer_p = [], []
        off = S = 0
        for l, (fi, fo) in enumerate(dims):
            out = l == len(dims) - 1
            if mode == 'rwf':
                grouped, with_bias = not (out and rwf_skip_output), rwf_bias_in
            else:
                grouped, with_bias = (not out) or slope_with_output, True
            cols = np.tile(np.arange(fo), fi)
            self.col[off:off + fi * fo] = cols
            self.col[off + fi * fo:off + fi * fo + fo] = np.arange(fo)
            cnt = (1 if self.tied else fo) if (grouped or (mode == 'rwf' and out)) else 0     # (mutant b keeps rwf's S)
            if grouped:
                self.group[off:off + fi * fo] = S + (0 if self.tied else cols)
                if with_bias:
                    self.group[off + fi * fo:off + fi * fo + fo] = S + (0 if self.tied else np.arange(fo))
            self.layer_s.append(slice(S, S + cnt))
            self.layer_p.append(slice(off, off + fi * fo + fo))
            S += cnt
            off += fi * fo + fo
        self.S = S

    def f(self, s):
        s = np.asarray(s, dtype=np.float64)
        return np.exp(s) if self.mode == 'rwf' else self.n * s

    def fprime(self, s):
        s = np.asarray(s, dtype=np.float64)
        return np.exp(s) if self.mode == 'rwf' else np.full(s.shape, self.n)

    def spread(self, fs):
        """The factor of every entry from the S factors fs (1 where the entry is in no group)."""
        fs = np.asarray(fs, dtype=np.float64)
        return np.where(self.group >= 0, fs[np.maximum(self.group, 0)], 1.0)

    def effective(self, V, s):
        return self.spread(self.f(s)) * np.asarray(V, dtype=np.float64)

    def factorise(self, theta, s):
        return np.asarray(theta, dtype=np.float64) / self.spread(self.f(s))

    def sums(self, V, g, first_column_only=False):
        """sum_{p in group} V[p] g[p] per scale."""
        on = self.group >= 0
        if first_column_only:
            on = on & (self.col == 0)
        return np.bincount(self.group[on], weights=(np.asarray(V, dtype=np.float64) * np.asarray(g, dtype=np.float64))[on], minlength=self.S)

    def chain(self, V, s, g):
        """(g_V, g_s) from g = d loss / d theta_eff."""
        return self.spread(self.f(s)) * np.asarray(g, dtype=np.float64), self.fprime(s) * self.sums(V, g)

    def abs_sums(self, V, g):
        on = self.group >= 0
        return np.bincount(self.group[on], weights=np.abs(np.asarray(V, dtype=np.float64) * np.asarray(g, dtype=np.float64))[on], minlength=self.S)


def default_s(lay, rng=None, spread=0.2):
    """Scales near f == 1: rwf s ~ N(0, spread); slope s = (1 + spread N(0, 1)) / n, rounded to fp32."""
    z = np.zeros(lay.S) if rng is None else rng.standard_normal(lay.S)
    s = spread * z if lay.mode == 'rwf' else (1.0 + spread * z) / lay.n
    return s.astype(np.float32)


class Joint64:
    """The joint step in fp64.  rounded=False keeps hyper-parameters and gradient in double (the comparison with TF1Adam).
    `mutant`: one of MUTANTS (None: the step as specified)."""

    def __init__(self, lay, lr=1e-3, lr_s=None, rounded=True, mutant=None):
        r = f32 if rounded else (lambda x: np.asarray(x, dtype=np.float64))
        self.lay, self.lr, self.lr_s, self.rounded, self.mutant = lay, lr, (lr if lr_s is None else lr_s), rounded, mutant
        self.b1, self.b2, self.eps = float(r(BETA1)), float(r(BETA2)), float(r(EPS))
        self.m, self.v = np.zeros(lay.P), np.zeros(lay.P)
        self.ms, self.vs = np.zeros(lay.S), np.zeros(lay.S)
        self.gV, self.gs = np.zeros(lay.P), np.zeros(lay.S)

    def load(self, m, v, ms, vs):
        self.m, self.v, self.ms, self.vs = (np.asarray(a, dtype=np.float64).copy() for a in (m, v, ms, vs))

    def _adam(self, x, g, m, v, lr_t):
        m = self.b1 * m + (1.0 - self.b1) * g
        v = self.b2 * v + (1.0 - self.b2) * g * g
        return x - lr_t * m / (np.sqrt(v) + self.eps), m, v

    def step(self, V, s, g, t):
        """(V, s, theta_eff) after step t from (V, s) with g = d loss / d theta_eff; moves the four slots."""
        lay, mu = self.lay, self.mutant
        V, s = np.asarray(V, dtype=np.float64), np.asarray(s, dtype=np.float64)
        g = f32(g) if self.rounded else np.asarray(g, dtype=np.float64)
        ts = {'h_lr_s_of_t_minus_1': max(t - 1, 1), 'h_lr_s_of_t_plus_1': t + 1}.get(mu, t)
        lr_t, lr_s_t = lr_t_of(self.lr, t, self.rounded), lr_t_of(self.lr_s, ts, self.rounded)
        gs = lay.sums(V, g, first_column_only=(mu == 'd_layer_not_tied' and lay.tied))
        if mu != 'c_fprime_dropped':
            gs = lay.fprime(s) * gs
        if mu == 'g_s_slots_not_carried':
            self.ms, self.vs = np.zeros(lay.S), np.zeros(lay.S)
        s_new, self.ms, self.vs = self._adam(s, gs, self.ms, self.vs, lr_s_t)
        gV = lay.spread(lay.f(s_new if mu == 'e_gV_with_scale_after' else s)) * g
        V_new, self.m, self.v = self._adam(V, gV, self.m, self.v, lr_t)
        f_new = lay.f(s if mu == 'f_theta_with_scale_before' else (f32(s_new) if self.rounded else s_new))
        theta = lay.spread(f32(f_new) if self.rounded else f_new) * (f32(V_new) if self.rounded else V_new)
        self.gV, self.gs = gV, gs
        return V_new, s_new, theta


class Joint32:
    """The same step in NumPy fp32, one rounding per operation, in the kernel's order: the sums and f in double, g_V and g_s
    rounded once to fp32, Adam's recurrences in fp32, theta_eff one fp32 multiply."""

    def __init__(self, lay, lr=1e-3, lr_s=None):
        F = np.float32
        self.lay, self.lr, self.lr_s = lay, lr, (lr if lr_s is None else lr_s)
        self.b1, self.b2, self.eps = F(BETA1), F(BETA2), F(EPS)
        self.m, self.v = np.zeros(lay.P, dtype=F), np.zeros(lay.P, dtype=F)
        self.ms, self.vs = np.zeros(lay.S, dtype=F), np.zeros(lay.S, dtype=F)

    def _adam(self, x, g, m, v, lr_t):
        F = np.float32
        mi = self.b1 * m + (F(1.0) - self.b1) * g
        vi = self.b2 * v + (F(1.0) - self.b2) * g * g
        xn = x - lr_t * mi / (np.sqrt(vi) + self.eps)
        assert xn.dtype == F and mi.dtype == F and vi.dtype == F
        return xn, mi, vi

    def step(self, V, s, g, t):
        F, lay = np.float32, self.lay
        V, s, g = np.asarray(V, dtype=F), np.asarray(s, dtype=F), np.asarray(g, dtype=F)
        lr_t, lr_s_t = F(lr_t_of(self.lr, t)), F(lr_t_of(self.lr_s, t))
        gV, gs = lay.chain(V, s, g)                                     # double, from the fp32 values
        s_new, self.ms, self.vs = self._adam(s, gs.astype(F), self.ms, self.vs, lr_s_t)
        V_new, self.m, self.v = self._adam(V, gV.astype(F), self.m, self.v, lr_t)
        theta = lay.spread(lay.f(s_new).astype(F)).astype(F) * V_new
        assert theta.dtype == F
        return V_new, s_new, theta


def mutant_layout(name, lay):
    """The layout a mutant steps on (a and b change the groups; the others keep them), or None where the mutant does not apply
    to lay's mode."""
    kw = dict(mode=lay.mode, per=lay.per, n=lay.n, d_in=lay.d_in, widths=lay.widths)
    if name == 'a_rwf_bias_in_group':
        return Layout(rwf_bias_in=True, **kw) if lay.mode == 'rwf' else None
    if name == 'b_rwf_output_left_out':
        return Layout(rwf_skip_output=True, **kw) if lay.mode == 'rwf' else None
    if name == 'b_slope_output_included':
        return Layout(slope_with_output=True, **kw) if lay.mode == 'slope' else None
    if name == 'd_layer_not_tied':
        return lay if lay.tied and max(lay.widths) > 1 else None
    if name == 'c_fprime_dropped' and lay.mode == 'slope' and lay.n == 1.0:
        return None                                                     # f' == 1: no different step
    return lay


MUTANTS = ['a_rwf_bias_in_group', 'b_rwf_output_left_out', 'b_slope_output_included', 'c_fprime_dropped', 'd_layer_not_tied',
           'e_gV_with_scale_after', 'f_theta_with_scale_before', 'g_s_slots_not_carried', 'h_lr_s_of_t_minus_1', 'h_lr_s_of_t_plus_1']


def replay(name, lay, steps, lr, lr_s):
    """Teacher-forced run of mutant `name` next to Joint64 over `steps`: dicts with t, V, s, g and the slots m, v, ms, vs of BEFORE
    the step (the device's, or Joint32's).  Returns the largest err / bar over V, s and theta_eff (theta_eff on the bar of a value
    one ulp wide: ulp32 of the reference), over all steps; None where the mutant does not apply.  The mutant carries its own s
    slots from step to step (that is what g drops); everything else restarts from the observed state."""
    mlay = mutant_layout(name, lay)
    if mlay is None:
        return None
    ref, mut = Joint64(lay, lr, lr_s), Joint64(mlay, lr, lr_s, mutant=name)
    worst = 0.0
    for k, st in enumerate(steps):
        s_mut = np.asarray(st['s'], dtype=np.float64)
        if mlay.S != lay.S:                                             # (b, slope: the extra scale of the output layer at f == 1)
            s_mut = np.concatenate([s_mut, np.full(mlay.S - lay.S, 1.0 / lay.n)])
        pad = lambda a: np.concatenate([np.asarray(a, dtype=np.float64), np.zeros(mlay.S - lay.S)])
        ref.load(st['m'], st['v'], st['ms'], st['vs'])
        mut.load(st['m'], st['v'], pad(st['ms']), pad(st['vs']))
        Vr, sr, thr = ref.step(st['V'], st['s'], st['g'], st['t'])
        Vm, sm, thm = mut.step(st['V'], s_mut, st['g'], st['t'])
        lr_t, lr_s_t = lr_t_of(lr, st['t']), lr_t_of(lr_s, st['t'])
        worst = max(worst,
                    float(np.max(np.abs(Vm - Vr) / bar(st['V'], Vr, lr_t))),
                    float(np.max(np.abs(sm[:lay.S] - sr) / bar(st['s'], sr, lr_s_t))),
                    float(np.max(np.abs(thm - thr) / (ulp32(thr) + C * lr_t))))
    return worst
