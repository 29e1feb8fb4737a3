"""
TEST-ONLY NumPy fp64 restatement of the L-BFGS iteration of include/varnet_hip.h (vn_lbfgs_step) as a plain two-loop
recursion over vectors -- the independent implementation the device's Gram form is checked against -- and a subclass of
the oracle-backed test engine that adds `lbfgs_step` on top of its `grad()`, so that the host logic of
`VarNet(..., optimizer='lbfgs')` runs in the CPU tier.
"""
import numpy as np

from tests.oracle_engine import OracleEngine

HISTORY = 10
C1 = 1e-4            # Armijo constant
CURV = 1e-10         # a pair enters the ring iff s.y > CURV |s| |y|


def two_loop(g, pairs):
    """-H g for the pairs [(s, y), ...] (oldest first), initial scaling s.y / y.y of the newest pair."""
    q = np.array(g, dtype=np.float64)
    if not pairs:
        return -q
    alphas = []
    for s, y in reversed(pairs):
        rho = 1.0 / np.dot(s, y)
        a = rho * np.dot(s, q)
        q = q - a * y
        alphas.append((a, rho))
    s, y = pairs[-1]
    r = (np.dot(s, y) / np.dot(y, y)) * q
    for (s, y), (a, rho) in zip(pairs, reversed(alphas)):
        b = rho * np.dot(y, r)
        r = r + (a - b) * s
    return -r


def direction(g, pairs):
    """(d, g.d, pairs used): the two-loop direction; the ring is dropped (in place) when it is no descent direction."""
    g = np.asarray(g, dtype=np.float64)
    d = two_loop(g, pairs)
    gd = float(np.dot(g, d))
    if not gd < 0.0:
        del pairs[:]
        d = -g
        gd = float(np.dot(g, d))
    return d, gd, len(pairs)


def first_step(g, npairs):
    if npairs:
        return 1.0
    g1 = float(np.sum(np.abs(np.asarray(g, dtype=np.float64))))
    return min(1.0, 1.0 / g1) if g1 > 0.0 else 1.0


def keeps_pair(s, y):
    s, y = np.asarray(s, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return float(np.dot(s, y)) > CURV * float(np.linalg.norm(s)) * float(np.linalg.norm(y))


def push_pair(pairs, s, y):
    """The ring rule: the pair enters (evicting the oldest) iff it passes the curvature test.  Returns whether it did."""
    if not keeps_pair(s, y):
        return False
    pairs.append((np.asarray(s, dtype=np.float64), np.asarray(y, dtype=np.float64)))
    if len(pairs) > HISTORY:
        del pairs[0]
    return True


def armijo(f_k, f_t, t, gd):
    return bool(np.isfinite(f_t) and f_t <= f_k + C1 * t * gd)


class Lbfgs:
    """The optimizer over a function fun(theta) -> (scalars [loss, BC, IC, var], gradient).  `fl` rounds what the device
    keeps in fp32 (np.float32), or is the identity for an fp64 run."""

    def __init__(self, fun, theta, fl=None):
        self.fun = fun
        self.fl = (lambda a: a) if fl is None else (lambda a: np.asarray(a).astype(fl).astype(np.float64))
        self.theta = np.array(theta, dtype=np.float64)
        self.pairs, self.valid, self.steps, self.evals = [], False, 0, 0
        self.f = self.g = None

    def invalidate(self):
        self.valid = False
        del self.pairs[:]

    def evaluate(self, theta):
        self.evals += 1
        sc, g = self.fun(theta)
        return [float(v) for v in sc], self.fl(np.asarray(g, dtype=np.float64))

    def step(self, max_trials=20):
        if not self.valid:
            self.f, self.g = self.evaluate(self.theta)
            self.valid = True
        d, gd, used = direction(self.g, self.pairs)
        t0 = first_step(self.g, used)
        f_k = self.f[0]
        info = {'status': 0, 'f_k': f_k, 'gd': gd, 'pairs': used, 'trials': 0, 't': 0.0}
        for j in range(max_trials):
            t = t0 * 0.5 ** j
            trial = self.fl(self.theta + t * d)
            f_t, g_t = self.evaluate(trial)
            info['trials'] = j + 1
            if armijo(f_k, f_t[0], t, gd):
                push_pair(self.pairs, self.fl(trial - self.theta), self.fl(g_t - self.g))
                self.theta, self.f, self.g = trial, f_t, g_t
                self.steps += 1
                info.update(t=t, f_next=f_t[0], BCloss=f_t[1], ICloss=f_t[2], varLoss=f_t[3])
                return info
        info.update(status=1 if used else 2, f_next=f_k, BCloss=self.f[1], ICloss=self.f[2], varLoss=self.f[3])
        del self.pairs[:]
        return info


class LbfgsOracleEngine(OracleEngine):
    """OracleEngine whose optimizer may be 'lbfgs': the interface of varnet_amd.engine.VNEngine for that case."""

    def __init__(self, *a, optimizer_name='adam', **kw):
        super().__init__(*a, optimizer_name=optimizer_name, **kw)
        self.optimizer_name = optimizer_name.lower()
        self.lb = None
        self.lb_batch, self.lb_w, self.lb_steps = None, None, 0
        self.force_status = None          # test hook: the next lbfgs_step reports this status without moving

    def _lbfgs_only(self, what):
        if self.optimizer_name == 'lbfgs':
            raise RuntimeError('%s is a first-order optimizer step: an L-BFGS engine advances by lbfgs_step only' % what)

    def _drop(self, batch=None):
        if self.lb is not None and (batch is None or batch == self.lb_batch):
            self.lb.invalidate()

    @property
    def step(self):
        return self.lb_steps if self.optimizer_name == 'lbfgs' else self.adam.t

    def init_params(self, seed=0):
        super().init_params(seed)
        self.lb_steps = 0
        self._drop()

    def set_params(self, flat):
        super().set_params(flat)
        self._drop()

    def export_state(self):
        if self.optimizer_name != 'lbfgs':
            return super().export_state()
        step = np.array([self.lb_steps], dtype=np.int64).view(np.uint8)
        body = np.concatenate([self.theta, np.zeros(2 * self.P)]).astype(np.float32).view(np.uint8)
        return np.concatenate([step, body])

    def import_state(self, buf):
        if self.optimizer_name != 'lbfgs':
            return super().import_state(buf)
        buf = np.asarray(buf, dtype=np.uint8)
        self.lb_steps = int(buf[:8].view(np.int64)[0])
        self.theta = buf[8:].view(np.float32).astype(self.dtype)[:self.P].copy()
        self._drop()

    def state_snapshot(self):
        self._lbfgs_only('state_snapshot')
        super().state_snapshot()

    def state_rollback(self):
        self._lbfgs_only('state_rollback')
        super().state_rollback()

    def apply(self):
        self._lbfgs_only('apply')
        super().apply()

    def train_step(self, batch=0, loss_out=None):
        self._lbfgs_only('train_step')
        super().train_step(batch, loss_out)

    def set_interior(self, batch, *a, **kw):
        super().set_interior(batch, *a, **kw)
        self._drop(batch)

    def set_bic(self, *a, **kw):
        super().set_bic(*a, **kw)
        self._drop()

    def set_batch_bic(self, batch, *a, **kw):
        super().set_batch_bic(batch, *a, **kw)
        self._drop(batch)

    def lbfgs_step(self, batch=0, max_trials=20):
        if self.optimizer_name != 'lbfgs':
            raise RuntimeError('lbfgs_step needs an engine made with optimizer_name=\'lbfgs\'')

        def fun(theta):
            keep = self.theta
            self.theta = np.asarray(theta, dtype=self.dtype)
            try:
                self.grad(batch)
            finally:
                self.theta = keep
            gb = self.gradbuf.numpy()
            return gb[self.P:].copy(), gb[:self.P].copy()

        if self.lb is None:
            self.lb = Lbfgs(fun, self.theta)
        self.lb.fun = fun
        if batch != self.lb_batch or self.lb_w is None or not np.array_equal(self.lb_w, self.w):
            self.lb.invalidate()
        if not self.lb.valid:
            self.lb.theta = np.array(self.theta, dtype=np.float64)
        self.lb_batch, self.lb_w = batch, np.array(self.w, dtype=float)
        if self.force_status is not None:
            if not self.lb.valid:
                self.lb.f, self.lb.g = self.lb.evaluate(self.lb.theta)
                self.lb.valid = True
            st, self.force_status = self.force_status, None
            f = self.lb.f
            del self.lb.pairs[:]
            return {'status': st, 'f_k': f[0], 'f_next': f[0], 'BCloss': f[1], 'ICloss': f[2], 'varLoss': f[3], 't': 0.0,
                    'trials': max_trials, 'gd': 0.0, 'pairs': 0}
        info = self.lb.step(max_trials)
        self.theta = self.lb.theta.astype(self.dtype)
        self.lb_steps += 1 if info['status'] == 0 else 0
        return info
