"""
ORACLE tooling (test infrastructure): golden fixtures for the reference's host-side DATA ASSEMBLY --
SURVEY.md 8(c) items (7) and (8) -- produced by running the reference's own NumPy code:

    VarNet.__init__ -> FIXData -> setInputData -> setFEdata          (VarNet.py:70-203, VarNetUtility.py:204-463)
    trainingPoints('uniform'), biTrainPoints, biTrainData, PDEinpData  (VarNet.py:504-774)
    trainData -> gcoef = diff*dNx + vel*N -> ManageTrainData.updateData / trainDicts   (VarNet.py:778-857,
                                                                                        VarNetUtility.py:619-857)
    updateDictFields('trainW')   (BC/IC weights / batchNum / puNum, VarNetUtility.py:872-953)
    trainWeight                  (three branches, VarNet.py:1094-1146)

    MPLBACKEND=Agg python oracle/gen_golden_assembly.py      ->  tests/golden/assembly.npz

Runs ONLY in the build container (the reference never travels to the GPU box); the .npz is committed.

How the TF half is kept out.  `VarNet.py`, `VarNetUtility.py` and `TFModel.py` do `import tensorflow` at
module level (TensorFlow 1.10 is not installable here).  This script puts EMPTY placeholder modules named
`tensorflow`, `tensorflow.keras(.models/.layers)`, `tensorflow.python.client(.device_lib)` into
`sys.modules` so that those import statements succeed, and replaces the name `TFNN` inside the reference's
`VarNet` module by a data-only record (number of towers + placeholder keys).  The placeholders contain NO
functionality: any attribute access on them raises, so nothing that would need TensorFlow can run
silently -- only the reference's own NumPy statements execute, unmodified, from /root/reference.  The
device graph (TFModel.py) is never built; `ManageTrainData.splitLoss` (a `sess.run`) is replaced by fixed
loss triples when `trainWeight`'s arithmetic is recorded.  This is the procedure the survey session
verified ("Partial workaround verified").
"""
import os
import sys
import types

sys.dont_write_bytecode = True      # importing the reference must not write __pycache__ into /root/reference (read-only input)

import numpy as np

REF = '/root/reference'
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden')


class _Empty(types.ModuleType):
    """Placeholder module: importable, nothing inside."""

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        raise AttributeError('TensorFlow is not available here: `%s.%s` was touched -- only the NumPy half of the '
                             'reference may run in oracle/gen_golden_assembly.py' % (self.__name__, name))


def install_placeholders():
    names = ['tensorflow', 'tensorflow.keras', 'tensorflow.keras.models', 'tensorflow.keras.layers',
             'tensorflow.python', 'tensorflow.python.client', 'tensorflow.python.client.device_lib']
    mods = {n: _Empty(n) for n in names}
    # `from tensorflow.keras.models import Sequential`, `from tensorflow.keras import layers`,
    # `from tensorflow.python.client import device_lib` (TFModel.py:45-47) must bind *names*; they bind None.
    mods['tensorflow.keras.models'].__dict__['Sequential'] = None
    mods['tensorflow.keras'].__dict__['layers'] = mods['tensorflow.keras.layers']
    mods['tensorflow.keras'].__dict__['models'] = mods['tensorflow.keras.models']
    mods['tensorflow'].__dict__['keras'] = mods['tensorflow.keras']
    mods['tensorflow.python.client'].__dict__['device_lib'] = mods['tensorflow.python.client.device_lib']
    sys.modules.update(mods)


class Tower:
    """Keys of one tower's feed dict (the reference uses TF placeholders as dict keys, VarNetUtility.py:840-854)."""
    FIELDS = ('Input', 'biInput', 'biLabel', 'gcoef', 'source', 'N', 'dNt', 'bDof', 'intShape', 'integW',
              'biDimVal', 'detJvec', 'detJ', 'w', 'residual', 'diff', 'vel', 'diff_dx', 'BCloss', 'ICloss')

    def __init__(self, i):
        for f in self.FIELDS:
            setattr(self, f, 't%d.%s' % (i, f))


PU = [1]


def OPT_RESIDUAL(X):
    """Stand-in for |strong residual| on rows [x, y, t] (smpScheme='optimal' fixture)."""
    return np.abs(np.sin(3.0 * X[:, 0:1]) * (0.2 + X[:, 2:3]) + 0.3 * X[:, 1:2]) + 0.05


def MON_MODEL(X):
    """Stand-in for the model value on monitor rows (any number of input columns)."""
    X = np.asarray(X, dtype=float)
    return 0.3 * np.cos(2.0 * X[:, 0:1]) + 0.1 * X[:, -1:] + 0.05 * np.sum(X, axis=1, keepdims=True)


def MON_RESIDUAL(X, diff, vel, source, diff_dx, dim):
    """Stand-in for the strong-residual node: a closed form of EVERYTHING the reference feeds it, so that a wrong
    feed shows in the value (TFModel.py:743-754 takes the same five arrays)."""
    X = np.asarray(X, dtype=float)
    adv = np.sum((np.asarray(vel, dtype=float) - np.asarray(diff_dx, dtype=float)) * X[:, :dim], axis=1, keepdims=True)
    return np.asarray(diff, dtype=float) * np.sin(X[:, 0:1]) - adv + np.asarray(source, dtype=float) + 0.1 * X[:, -1:]


class MonitorSess:
    """`sess.run` of ManageTrainData.runSession (VarNetUtility.py:1098-1142): records what is fed, answers in closed form."""

    def __init__(self, tower, dim):
        self.t, self.dim, self.feeds = tower, dim, []

    def run(self, fetches, feed_dict=None):
        f = feed_dict
        self.feeds.append({k: (None if v is None else np.array(v, dtype=float)) for k, v in f.items()})
        out = []
        for node in fetches:
            if node == self.t.residual:
                out.append(MON_RESIDUAL(f[self.t.Input], f[self.t.diff], f[self.t.vel], f[self.t.source], f[self.t.diff_dx], self.dim))
            else:
                assert node[0] == 'model'
                out.append(MON_MODEL(f[node[1]]))
        return out


class TrainSess:
    """`sess` for a whole run of the reference's VarNet.train (VarNet.py:1193-1421): every graph node the loop fetches is
    answered from a script -- the training losses from a prescribed list, the loss components and the loss field as closed
    forms of what is fed, model and strong residual as in MonitorSess -- and every training step is logged."""

    def __init__(self, tfd, dim, losses):
        self.tf, self.t, self.dim, self.losses, self.k, self.steps = tfd, tfd.compTowers[0], dim, list(losses), 0, []

    def run(self, fetches, feed_dict=None):
        f = feed_dict
        if isinstance(fetches, tuple) and len(fetches) == 2 and fetches[0] == 'model':      # sess.run(model(Input), {...})
            return MON_MODEL(f[fetches[1]])
        out = []
        for node in fetches:
            if isinstance(node, list) and not node:                     # lossVec_tf = [] when the field is not wanted
                out.append([])
            elif node == self.tf.optMinimize:
                out.append(None)
            elif node == self.tf.loss:
                X = np.asarray(f[self.t.Input])
                self.steps.append([X.shape[0], float(X[0, 0]), float(X[-1, -1]), float(np.asarray(f[self.t.biInput])[0, 0])])
                out.append(self.losses[self.k])
                self.k += 1
            elif node == self.t.BCloss:
                out.append(2.0)
            elif node == self.t.ICloss:
                out.append(3.0)
            elif node == self.tf.varLoss:
                out.append(1e-3 * np.asarray(f[self.t.Input]).shape[0])
            elif node == self.tf.lossVec:
                n_k, q = [int(v) for v in f[self.t.intShape]]
                out.append(np.asarray(f[self.t.Input])[::q, 0:1][:n_k].copy())
            elif node == self.t.residual:
                out.append(MON_RESIDUAL(f[self.t.Input], f[self.t.diff], f[self.t.vel], f[self.t.source], f[self.t.diff_dx], self.dim))
            else:
                assert node[0] == 'model', node
                out.append(MON_MODEL(f[node[1]]))
        return out


class SaverRec:
    def __init__(self):
        self.saved = []

    def save(self, sess, path, global_step=None):
        self.saved.append(int(global_step))


def OPT_MODEL(X):
    """Stand-in for the model value on boundary / initial rows [x, y, t]."""
    return 0.3 * np.cos(2.0 * X[:, 0:1]) + 0.1 * X[:, 2:3] - 0.2 * X[:, 1:2]


class TowerRecord:
    """Stands where the reference constructs TFNN (VarNet.py:200): only `processorNum` and `compTowers` are read
    by the host code exercised here (VarNetUtility.py:832-833)."""

    def __init__(self, *a, **k):
        self.processorNum = PU[0]
        self.compTowers = [Tower(i) for i in range(PU[0])]
        if len(a) > 1:
            self.dim, self.inpDim = a[0], a[1]             # TFNN(dim, inpDim, ...) keeps its arguments (VarNet.py:201)


class Log:
    def writeCase(self, s):
        pass


class ParamCount:
    """`tfData.model.count_params()` is the one thing initializeCase asks of the Keras model (VarNetUtility.py:1288)."""

    def __init__(self, n):
        self.n = n

    def count_params(self):
        return self.n


def record(store, key, vn, RVU, batchNum, batchLen, pu):
    """Run the reference assembly for one problem and store every array the device would be fed."""
    PU[0] = pu
    vn.tfData = TowerRecord()
    fd = vn.fixData
    fd.setFEdata()
    Input, _, biInput, biDof = vn.trainingPoints('uniform')
    tData = RVU.ManageTrainData(Input, biInput, batchNum=batchNum, batchLen=batchLen)
    tData = vn.trainData(0, None, tData)
    InpuTot, biInpuTot, biLabel, gcoef, sourceVal = tData.getTrainData()
    g = key + '_'
    store[g + 'Input'], store[g + 'biInput'], store[g + 'biDof'] = InpuTot, biInpuTot, np.array(biDof)
    store[g + 'biLabel'], store[g + 'gcoef'], store[g + 'source'] = biLabel, gcoef, sourceVal
    store[g + 'diff'], store[g + 'vel'] = tData.diff, tData.vel
    store[g + 'N'], store[g + 'dNx'], store[g + 'dNt'] = fd.N, fd.dNx, fd.dNt
    store[g + 'scalars'] = np.array([fd.nt, fd.nT, fd.integNum, fd.detJ, fd.bDofsum, fd.biDimVal,
                                     tData.batchNum, tData.batchLen, tData.puNum], dtype=float)
    store[g + 'hVec'] = np.reshape(fd.hVec, -1)
    store[g + 'integW'] = np.zeros(0) if fd.integW is None else np.asarray(fd.integW, dtype=float)
    store[g + 'uniform_input'] = fd.uniform_input
    # what the monitors feed (VarNetUtility.py:370-411): exact field, PDE data and grad(diffusivity) on uniform_input
    store[g + 'cEx'] = np.zeros(0) if fd.cEx is None else np.asarray(fd.cEx, dtype=float)
    uid = fd.uniform_inpData
    for nm, arr in zip(('u_diff', 'u_vel', 'u_src'), uid):
        store[g + nm] = np.zeros(0) if arr is None else np.asarray(arr, dtype=float)
    store[g + 'd_diff'] = np.asarray(fd.d_diff, dtype=float)
    # per (mini-batch, tower) feed: rows of Input / gcoef and the intShape the tower receives
    for bi, fdict in enumerate(tData.optimFeedicts):
        for ti, tw in enumerate(vn.tfData.compTowers):
            h = g + 'b%d_t%d_' % (bi, ti)
            store[h + 'Input'] = fdict[tw.Input]
            store[h + 'gcoef'] = fdict[tw.gcoef]
            store[h + 'intShape'] = np.array(fdict[tw.intShape])
            store[h + 'N'] = fdict[tw.N]
            store[h + 'dNt'] = np.asarray(fdict[tw.dNt])
            store[h + 'detJ'] = np.asarray(fdict[tw.detJ], dtype=float)
    # BC/IC weight rule (in place on the caller's array, VarNetUtility.py:900-901)
    tw_in = np.array([3.0, 2.0, 5.0])
    tData.updateDictFields('trainW', tw_in)
    store[g + 'trainW_fed'] = np.array(tData.optimFeedicts[0][vn.tfData.compTowers[0].w], dtype=float)
    return tData


def load_reference():
    """Import the reference's NumPy half behind the TF placeholders: returns its VarNet, VarNetUtility, Domain and ADPDE
    modules (oracle/gen_golden_steady.py reuses this procedure)."""
    os.environ.setdefault('MPLBACKEND', 'Agg')
    sys.path.insert(0, REF)
    install_placeholders()
    if not hasattr(np, 'asscalar'):
        # the reference was written against NumPy < 1.23 (`np.asscalar` in VarNet.py:328, Domain.py); the call it made
        np.asscalar = lambda a: np.asarray(a).item()
    for _alias, _ty in (('int', int), ('float', float), ('bool', bool), ('complex', complex), ('int0', np.intp)):
        if not hasattr(np, _alias):                   # ... and the scalar aliases NumPy 1.24 removed (UtilityFunc.py:857)
            setattr(np, _alias, _ty)
    import VarNet as RV                      # the reference's own module, unmodified
    import VarNetUtility as RVU
    import Domain as RD
    import ADPDE as RA
    RV.TFNN = TowerRecord
    return RV, RVU, RD, RA


def main():
    RV, RVU, RD, RA = load_reference()
    os.makedirs(OUT, exist_ok=True)
    st = {}

    def pde1(td=True):
        if td:
            return RA.ADPDE(RD.Domain1D(), diff=0.1 / np.pi, vel=1.0, timeDependent=True, tInterval=[0, 2.0],
                            IC=lambda x: -np.sin(np.pi * x), cEx=lambda x, t: -np.sin(np.pi * (x - t)) * np.exp(-0.3 * t))
        return RA.ADPDE(RD.Domain1D(), diff=0.1 / np.pi, vel=1.0, source=lambda x: 1.0 + x ** 2,
                        timeDependent=False, BCs=[[0., 1., 0.5], [0., 2., 1.0]], cEx=lambda x: 0.5 + 0.25 * (x + 1.0) ** 2)

    def pde2(source=False):
        verts = np.array([[0.0, -0.5], [0.0, -0.2], [0.0, 0.2], [0.0, 0.5], [2.0, 0.5], [2.0, -0.5]])
        BC = [[], [0.0, 1.0, 1.0], [], [], [], []]
        kw = {}
        if source:
            kw['source'] = lambda x, t: np.sin(x[:, 0:1]) * (1.0 + t)
            kw['diff'] = lambda x, t: 1e-3 * (1.0 + x[:, 1:2] ** 2)
            kw['vel'] = lambda x, t: np.hstack([1.0 + 0.0 * t, 0.1 * x[:, 0:1]])
            kw['d_diff'] = lambda x, t: np.hstack([0.0 * x[:, 0:1], 2e-3 * x[:, 1:2]])
            kw['cEx'] = lambda x, t: np.exp(-t) * np.sin(x[:, 0:1]) * (1.0 + x[:, 1:2])
        else:
            kw['diff'], kw['vel'] = 1e-3, [1., 0.]
        return RA.ADPDE(RD.PolygonDomain2D(verts), tInterval=[0, 1.5], BCs=BC, IC=0.0, **kw)

    # (7) down-scaled 1D+t (discNum=5, tDiscNum=6) and 2D+t ([4,3], bDisc=3, tDisc=4), integPnum 2 and 3,
    #     one tower / two towers, one batch / three mini-batches / batchLen
    for ip in (2, 3):
        for (bn, bl, pu) in ((None, None, 1), (3, None, 1), (None, None, 2), (3, None, 2), (None, 7, 2)):
            key = '1dt_ip%d_bn%s_bl%s_pu%d' % (ip, bn, bl, pu)
            PU[0] = pu
            vn = RV.VarNet(pde1(), layerWidth=[5], discNum=5, bDiscNum=None, tDiscNum=6, integPnum=ip)
            record(st, key, vn, RVU, bn, bl, pu)
            key = '2dt_ip%d_bn%s_bl%s_pu%d' % (ip, bn, bl, pu)
            vn = RV.VarNet(pde2(), layerWidth=[5], discNum=[4, 3], bDiscNum=3, tDiscNum=4, integPnum=ip)
            record(st, key, vn, RVU, bn, bl, pu)
    # variable coefficients + source term (gcoef with non-constant diff / vel; source feed)
    PU[0] = 1
    vn = RV.VarNet(pde2(source=True), layerWidth=[5], discNum=[4, 3], bDiscNum=3, tDiscNum=4, integPnum=2)
    record(st, '2dt_var', vn, RVU, None, None, 1)
    # steady 1D problem with a source (time-independent branch of every routine)
    vn_s = RV.VarNet(pde1(td=False), layerWidth=[5], discNum=7, bDiscNum=None, tDiscNum=[], integPnum=2)
    record(st, '1d_steady', vn_s, RVU, None, None, 1)

    # shuffleTrainData (VarNetUtility.py:957-1017) from a fixed NumPy seed: the feeds of every (mini-batch, tower) after
    # one and after two shuffles -- test-function order AND the per-feed permutation of the boundary/initial rows
    for pu in (1, 2):
        PU[0] = pu
        vn_s2 = RV.VarNet(pde1(), layerWidth=[5], discNum=5, bDiscNum=None, tDiscNum=6, integPnum=2)
        tD = record(st, '1dt_shuf_pu%d' % pu, vn_s2, RVU, 3, None, pu)
        np.random.seed(4711)
        for rnd in range(2):
            tD.shuffleTrainData(vn_s2.fixData)
            st['1dt_shuf_pu%d_r%d_batchInd' % (pu, rnd)] = tD.batchInd.copy()
            for bi, fdict in enumerate(tD.optimFeedicts):
                for ti, tw in enumerate(vn_s2.tfData.compTowers):
                    h = '1dt_shuf_pu%d_r%d_b%d_t%d_' % (pu, rnd, bi, ti)
                    st[h + 'Input'], st[h + 'gcoef'] = fdict[tw.Input], fdict[tw.gcoef]
                    st[h + 'biInput'], st[h + 'biLabel'] = fdict[tw.biInput], fdict[tw.biLabel]

    # smpScheme='random' (VarNet.py:519-566: timeDisc / getMesh with rfrac, global NumPy stream) from a fixed seed
    for key, mk in (('1dt', lambda: RV.VarNet(pde1(), layerWidth=[5], discNum=5, bDiscNum=None, tDiscNum=6, integPnum=2)),
                    ('2dt', lambda: RV.VarNet(pde2(), layerWidth=[5], discNum=[4, 3], bDiscNum=3, tDiscNum=4, integPnum=2))):
        PU[0] = 1
        vr = mk()
        vr.fixData.setFEdata()
        np.random.seed(99)
        try:
            Input, _, biInput, biDof = vr.trainingPoints('random', frac=0.5)
        except ValueError as e:
            # Domain1D.getMesh(rfrac > 0) hstacks a 1-D with a 2-D array (Domain.py:678): the reference's own 1-D random
            # branch raises; recorded as absent
            assert key == '1dt' and 'same number of dimensions' in str(e), e
            continue
        st['rand_%s_Input' % key], st['rand_%s_biInput' % key], st['rand_%s_biDof' % key] = Input, biInput, np.array(biDof)

    # smpScheme='optimal' (VarNet.py:1696-1966): the reference's own optTrainPoints / optBiTrainPoints / updateOptimData
    # from a fixed NumPy seed, with the two device fields they consult replaced by closed-form stand-ins -- |strong
    # residual| (self.residual) and the model value on boundary rows (sess.run(model(Input))) -- so that the host policy
    # (thinning / adding, rejection sampling per segment, support scaling, sorting, FE rows of the added points) is what
    # gets pinned.  (2D+t only: the reference's 1-D random meshes raise, see above.)
    class FakeSess:
        def run(self, fetch, feed):
            tag, key = fetch
            assert tag == 'model'
            return OPT_MODEL(feed[key])

    # (the thinning branch, addTrainPts=False, needs a grid on which ceil(frac2 * discNum) really drops points: on the
    # 4 x 3 grid nothing is dropped, biDof1 is all zeros and the reference's rejectionSampling raises on its empty lists)
    for name, (frac, add, supp, disc, bdisc, tdisc) in (('add', (0.25, True, 1.0, [4, 3], 3, 4)), ('add_supp', (0.25, True, 0.5, [4, 3], 3, 4)),
                                                        ('keep', (0.5, False, 1.0, [8, 6], 6, 8))):
        PU[0] = 1
        vo = RV.VarNet(pde2(), layerWidth=[5], discNum=disc, bDiscNum=bdisc, tDiscNum=tdisc, integPnum=2)
        fdo = vo.fixData
        fdo.setFEdata()
        vo.residual = lambda Input=None, *a, _v=vo, **k: (None, OPT_RESIDUAL(_v.fixData.uniform_input if Input is None else Input), None, None)
        vo.tfData.model = lambda t: ('model', t)
        vo.tfData.sess = FakeSess()
        np.random.seed(2024)
        Input, _, biInput, biDof = vo.optTrainPoints(frac, add, supp)
        g = 'opt_%s_' % name
        st[g + 'Input'], st[g + 'biInput'], st[g + 'biDof'] = Input, biInput, np.array(biDof)
        st[g + 'scalars'] = np.array([fdo.nt, fdo.nT, fdo.bDofsum, float(bool(fdo.detJvec))], dtype=float)
        st[g + 'detJ'] = np.reshape(np.asarray(fdo.detJ, dtype=float), -1)
        st[g + 'N'], st[g + 'dNx'], st[g + 'dNt'] = fdo.N, fdo.dNx, np.asarray(fdo.dNt, dtype=float)
        st[g + 'fd_biDof'] = np.array(fdo.biDof)

    # evaluate / residual (VarNet.py:1510-1692): the host side of the monitors -- which rows, PDE data and grad(kappa)
    # reach the graph (uniform grid, user points, one time, MOR batch or explicit MOR arguments) and what is made of
    # the answer (norm over the grid, l2 error, average over the MOR batches) -- with the graph replaced by MonitorSess
    def monitor_calls(vn, tag, calls):
        tw = vn.tfData.compTowers[0]
        sess = MonitorSess(tw, vn.dim)
        vn.tfData.sess, vn.tfData.model = sess, (lambda t: ('model', t))
        vn.fixData.setFEdata()
        for name, fn in calls:
            sess.feeds.clear()
            out = fn(vn)
            g = 'mon_%s_%s_' % (tag, name)
            if isinstance(out, tuple):                       # residual(): (res, resVec, err, cApp)
                st[g + 'res'] = np.float64(out[0])
                st[g + 'resVec'], st[g + 'cApp'] = out[1], out[3]
                st[g + 'err'] = np.float64(np.nan if out[2] is None else out[2])
            else:
                st[g + 'cApp'] = out
            st[g + 'ncalls'] = np.int64(len(sess.feeds))
            for i, fdict in enumerate(sess.feeds):
                for fld in ('Input', 'diff', 'vel', 'source', 'diff_dx'):
                    v = fdict.get(getattr(tw, fld))
                    if v is not None:
                        st[g + 'c%d_%s' % (i, fld)] = v

    xs2 = np.array([[0.3, -0.1], [1.7, 0.4], [0.9, 0.0], [1.2, -0.45]])
    rows2 = np.hstack([xs2, np.array([[0.2], [1.1], [0.7], [1.4]])])
    PU[0] = 1
    vn_v = RV.VarNet(pde2(source=True), layerWidth=[5], discNum=[4, 3], bDiscNum=3, tDiscNum=4, integPnum=2)
    monitor_calls(vn_v, '2dt_var', [
        ('eval_grid', lambda v: v.evaluate()),
        ('eval_pts_t', lambda v: v.evaluate(xs2, 0.37)),
        ('eval_pts_tvec', lambda v: v.evaluate(xs2, rows2[:, 2:3])),
        ('eval_space_only', lambda v: v.evaluate(t=0.5)),
        ('res_grid', lambda v: v.residual()),
        ('res_rows', lambda v: v.residual(rows2)),
    ])
    vn_st = RV.VarNet(pde1(td=False), layerWidth=[5], discNum=7, bDiscNum=None, tDiscNum=[], integPnum=2)
    monitor_calls(vn_st, '1d_steady', [
        ('eval_grid', lambda v: v.evaluate()),
        ('eval_pts', lambda v: v.evaluate(np.array([[-0.5], [0.25], [0.8]]))),
        ('res_grid', lambda v: v.residual()),
    ])

    # MOR batches (Operator_1DtMOR.py:166-204 in small): kappa as third network input, 3 values; the reference walks
    # the batches through trainData(batch, MORdiscArg, tData) -- first pass computes, with saveMORdata=True the
    # second pass reloads the stored fields (VarNetUtility.py:660-752).  Recorded per batch: what the towers are fed.
    import MOR as RM

    def diffFun(x, t=0, D=0.01):
        return D * np.ones([np.shape(x)[0], 1])

    def disc(discNum=3):
        return np.array([0.003 * (11 ** (n / (discNum - 1))) for n in range(discNum)])[np.newaxis].T

    for save in (False, True):
        PU[0] = 1
        mor = RM.MOR(diffFun, ['D'], [[0.003, 0.033]])
        pde_m = RA.ADPDE(RD.Domain1D(), diff=diffFun, vel=1.0, timeDependent=True, tInterval=[0, 2.0],
                         IC=lambda x: -np.sin(np.pi * x), MORvar=mor)
        vn_m = RV.VarNet(pde_m, layerWidth=[5], discNum=5, bDiscNum=None, tDiscNum=6, MORdiscScheme=disc, integPnum=2)
        vn_m.tfData = TowerRecord()
        fdm = vn_m.fixData
        fdm.setFEdata()
        Input, _, biInput, biDof = vn_m.trainingPoints('uniform')
        tD = RVU.ManageTrainData(Input, biInput, batchNum=2, saveMORdata=save, MORbatchNum=fdm.MORbatchNum)
        for rnd in range(2):                               # second round: the stored-data path when save=True
            for b in range(fdm.MORbatchNum):
                tD = vn_m.trainData(b, fdm.MORdiscArg, tD)
                InpuTot, biInpuTot, biLabel, gcoef, sourceVal = tD.getTrainData()
                g = '1dt_mor_save%d_r%d_b%d_' % (int(save), rnd, b)
                st[g + 'Input'], st[g + 'biInput'], st[g + 'biLabel'], st[g + 'gcoef'] = InpuTot, biInpuTot, biLabel, gcoef
                fd0 = tD.optimFeedicts[1][vn_m.tfData.compTowers[0].Input]
                st[g + 'mb1_Input'] = fd0
        st['1dt_mor_scalars'] = np.array([fdm.MORbatchNum, fdm.nt, fdm.integNum, tD.batchNum, tD.batchLen], dtype=float)
        st['1dt_mor_disc'] = fdm.MORdiscArg[0]
    # the monitors of the parametric problem: one batch, explicit MOR arguments, and the average over all batches
    mor = RM.MOR(diffFun, ['D'], [[0.003, 0.033]])
    pde_m = RA.ADPDE(RD.Domain1D(), diff=diffFun, vel=1.0, timeDependent=True, tInterval=[0, 2.0],
                     IC=lambda x: -np.sin(np.pi * x), MORvar=mor, cEx=lambda x, t: -np.sin(np.pi * (x - t)) * np.exp(-0.3 * t))
    vn_mm = RV.VarNet(pde_m, layerWidth=[5], discNum=5, bDiscNum=None, tDiscNum=6, MORdiscScheme=disc, integPnum=2)
    vn_mm.tfData = TowerRecord(1, 3)
    xs1 = np.array([[-0.6], [0.1], [0.75]])
    monitor_calls(vn_mm, '1dt_mor', [
        ('eval_batch1', lambda v: v.evaluate(batch=1)),
        ('eval_pts_arg', lambda v: v.evaluate(xs1, 0.8, MORarg=np.array([[0.012]]))),
        ('res_batch2', lambda v: v.residual(batch=2)),
        ('res_all', lambda v: v.residual()),
    ])

    # caseData.txt as the reference's TrainResult.initializeCase writes it (VarNetUtility.py:1217-1464): the case header of a
    # 1D+t run with mini-batches and of a 2D+t run with non-uniform sampling options -- kept as text lines (an OUTPUT
    # file of the reference), used to check the build's section / field order
    import tempfile
    for key, mk, targ in (
            ('1dt', lambda: RV.VarNet(pde1(), layerWidth=[6, 5], discNum=5, bDiscNum=None, tDiscNum=6, integPnum=2),
             dict(smpScheme='uniform', batchNum=3, shuffleData=True, shuffleFreq=2, weight=[10., 10., 1.])),
            ('2dt', lambda: RV.VarNet(pde2(), layerWidth=[5], discNum=[4, 3], bDiscNum=3, tDiscNum=4, integPnum=2),
             dict(smpScheme='optimal', batchNum=None, shuffleData=False, shuffleFreq=1, weight=[5., 1., 1.]))):
        PU[0] = 1
        v = mk()
        v.fixData.setFEdata()
        t = v.tfData = TowerRecord()
        t.inpDim, t.layerWidth, t.activationFun = v.dim + 1, list(v.layerWidth if hasattr(v, 'layerWidth') else [5]), ['sigmoid']
        widths = [6, 5] if key == '1dt' else [5]
        t.layerWidth = widths
        fan, P = v.dim + 1, 0
        for h in widths + [1]:
            P += fan * h + h
            fan = h
        t.model = ParamCount(P)
        t.processors, t.controller, t.optimizer_name, t.learning_rate = ['/device:GPU:0'], '/device:GPU:0', 'Adam', 0.001
        folder = tempfile.mkdtemp()
        tr = RVU.TrainResult(folder, False, verbose=False, saveFreq=100, pltReplace=True)
        arg = dict(epochNum=1000, tol=0.1, smpScheme=targ['smpScheme'], frac=0.5, addTrainPts=True, suppFactor=1.0,
                   multiTrainUpd=False, trainUpdelay=20000, tolUpd=0.01, reinitrain=True, weight=targ['weight'],
                   updateWeights=False, normalizeW=False, adjustWeight=True, useOriginalW=False, saveMORdata=False,
                   batchNum=targ['batchNum'], batchLen=None, shuffleData=targ['shuffleData'], shuffleFreq=targ['shuffleFreq'])
        tr.initializeCase(v, arg)
        lines = open(os.path.join(folder, 'caseData.txt')).read().split('\n')
        lines = ['Simulation date: <date>' if ln.startswith('Simulation date') else ln for ln in lines]   # keep the fixture stable
        st['case_%s_lines' % key] = np.array(lines)
        if key == '1dt':
            # per-epoch reporting: iterOutput over 25 epochs with saveFreq = 10 (VarNetUtility.py:1560-1631) -> the lines
            # appended to caseData.txt, the sampled histories and the keys of the trainData.vn pickle
            import contextlib, io, pickle
            tr.saveFreq = 10
            tr.trainWeight = np.array([1.0, 2.0, 3.0])
            with contextlib.redirect_stdout(io.StringIO()):
                for ep in range(1, 26):
                    tr.iterOutput(ep, 1000.0 / ep, 900.0 / ep, 0.25 * ep, 0.5 / ep, 0.1 / ep, np.array([[1.0], [2.0], [3.0]]) / ep, None)
            allines = open(os.path.join(folder, 'caseData.txt')).read().split('\n')
            st['iter_lines'] = np.array(allines[len(lines) - 1:])
            st['iter_iterSmp'], st['iter_loss'] = np.array(tr.iterSmp), np.array(tr.loss)
            st['iter_lossComp'], st['iter_residual'] = np.array(tr.lossComp), np.array(tr.residual)
            st['iter_avgtime'] = np.array([tr.avgtime0, tr.avgtime])
            dump = pickle.load(open(os.path.join(folder, 'trainData.vn'), 'rb'))
            st['iter_pickle_keys'] = np.array(sorted(dump.keys()))

    # The epoch loop itself (VarNet.py:1193-1421) against a scripted session: the order of the training steps, the
    # shuffle points, the stop rule, the checkpoint policy, what iterOutput records, and -- in the residual-driven case --
    # when the training points are redrawn, the re-weighting (adjustWeight) and the rebuilt feeds.
    import contextlib as _ctx, io as _io, time as _time
    if not hasattr(_time, 'clock'):
        _time.clock = _time.perf_counter                  # the reference was written for Python < 3.8 (VarNet.py:1349)

    def scripted_train(tag, mk, losses, dim, **targ):
        PU[0] = 1
        v = mk()
        t = v.tfData
        t.loss, t.optMinimize, t.varLoss, t.lossVec, t.graph = 'loss', 'optMinimize', 'varLoss', 'lossVec', None
        t.layerWidth, t.activationFun = [5], ['sigmoid']
        t.model_count = ParamCount((v.dim + 1) * 5 + 5 + 5 + 1)
        t.processors, t.controller, t.optimizer_name, t.learning_rate = ['/device:GPU:0'], '/device:GPU:0', 'Adam', 0.001
        t.saver = SaverRec()
        sess = TrainSess(t, dim, losses)
        t.sess = sess

        class ModelBoth:                                   # tfData.model: callable on a placeholder AND asked for count_params
            def __call__(self, key):
                return ('model', key)

            def count_params(self):
                return t.model_count.count_params()
        t.model = ModelBoth()
        folder = tempfile.mkdtemp()
        np.random.seed(31337)
        with _ctx.redirect_stdout(_io.StringIO()):
            v.train(folder, verbose=False, **targ)
        tr = v.trainRes
        g = 'loop_%s_' % tag
        st[g + 'steps'] = np.array(sess.steps, dtype=float)
        st[g + 'saved'] = np.array(t.saver.saved, dtype=float)
        st[g + 'iterSmp'], st[g + 'loss'] = np.array(tr.iterSmp, dtype=float), np.array(tr.loss, dtype=float)
        st[g + 'lossComp'] = np.array([np.reshape(c, -1) for c in tr.lossComp], dtype=float)
        st[g + 'residual'] = np.array(tr.residual, dtype=float)
        st[g + 'error'] = np.array(getattr(tr, 'error', []), dtype=float)
        st[g + 'inpIter'] = np.array(tr.inpIter, dtype=float)
        st[g + 'trainWeight'] = np.array(tr.trainWeight, dtype=float)
        st[g + 'nsteps'] = np.float64(sess.k)
        lv = tr.lossVec                                   # list over MOR batches of the stacked loss field (or None)
        st[g + 'lossVec_len'] = np.float64(-1 if lv is None else len(lv))
        if lv is not None:
            st[g + 'lossVec0'] = np.asarray(lv[0], dtype=float)

    L = 1000.0 / (1.0 + np.arange(400.0))                 # the scripted training losses, one per sess.run of a mini-batch
    scripted_train('uniform', lambda: RV.VarNet(pde1(), layerWidth=[5], discNum=5, bDiscNum=None, tDiscNum=6, integPnum=2), L, 1,
                   weight=[10., 10., 1.], smpScheme='uniform', epochNum=9, tol=2 * 1000.0 / 14.5, saveFreq=2, batchNum=2,
                   shuffleData=True, shuffleFreq=3)
    scripted_train('optimal', lambda: RV.VarNet(pde2(), layerWidth=[5], discNum=[4, 3], bDiscNum=3, tDiscNum=4, integPnum=2), L, 2,
                   weight=[5., 1., 1.], smpScheme='optimal', frac=0.25, addTrainPts=True, suppFactor=1.0, epochNum=8, tol=1e-9,
                   saveFreq=2, multiTrainUpd=False, trainUpdelay=3, tolUpd=1e9, reinitrain=False, adjustWeight=True)
    # (saveFreq=1 cannot be scripted: TrainResult.iterOutput then never sets avgtime0 and raises, VarNetUtility.py:1582,1607)
    # parametric problem: the kappa batches inside an epoch, mini-batches inside a kappa batch, one reshuffle for all
    # batches, the saveMORdata store (VarNet.py:1350-1357)
    import MOR as RM_

    def diffFun_(x, t=0, D=0.01):
        return D * np.ones([np.shape(x)[0], 1])

    def disc_(discNum=3):
        return np.array([0.003 * (11 ** (n / (discNum - 1))) for n in range(discNum)])[np.newaxis].T

    def mk_mor():
        pde_ = RA.ADPDE(RD.Domain1D(), diff=diffFun_, vel=1.0, timeDependent=True, tInterval=[0, 2.0],
                        IC=lambda x: -np.sin(np.pi * x), MORvar=RM_.MOR(diffFun_, ['D'], [[0.003, 0.033]]))
        v = RV.VarNet(pde_, layerWidth=[5], discNum=5, bDiscNum=None, tDiscNum=6, MORdiscScheme=disc_, integPnum=2)
        v.tfData = TowerRecord(1, 3)
        return v
    scripted_train('mor', mk_mor, L, 1, weight=[10., 10., 1.], smpScheme='uniform', epochNum=5, tol=1e-9, saveFreq=2,
                   batchNum=2, shuffleData=True, shuffleFreq=2, saveMORdata=True)

    # saveNNparam (VarNet.py:2179-2260): per-layer [W (out x in), b (out x 1)], the timeFirst column move, the MATLAB and
    # Diffpack files.  The trainable variables come from `tf.trainable_variables()` + `sess.run`: a list of named tokens
    # and a session that hands out fixed arrays stand in for them.
    class Var:
        def __init__(self, name, val):
            self.name, self.val = name, val

    class VarSess:
        def run(self, v):
            return np.array(v.val)            # a session hands out copies

    class NullCtx:
        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

    class GraphRec:
        def as_default(self):
            return NullCtx()

    import scipy.io as _spio
    PU[0] = 1
    v = RV.VarNet(pde1(), layerWidth=[6, 5], discNum=5, bDiscNum=None, tDiscNum=6, integPnum=2)
    rngp = np.random.default_rng(12)
    vars_, fan = [], 2
    for i, h in enumerate([6, 5, 1]):
        nm = 'output' if i == 2 else 'dense_%d' % i
        vars_ += [Var(nm + '/kernel:0', rngp.standard_normal((fan, h))), Var(nm + '/bias:0', rngp.standard_normal(h))]
        fan = h
    st['nnp_theta'] = np.concatenate([x.val.reshape(-1) for x in vars_])
    t = v.tfData
    t.depth, t.sess, t.graph = 2, VarSess(), GraphRec()
    RV.tf = types.SimpleNamespace(trainable_variables=lambda: list(vars_))       # the one tf call of this routine
    folder = tempfile.mkdtemp()
    v.trainRes = types.SimpleNamespace(folderpath=folder)
    for tfirst in (False, True):
        layers = v.saveNNparam(dpOut=True, matOut=True, verbose=False, timeFirst=tfirst)
        for li, (W, b) in enumerate(layers):
            st['nnp_tf%d_W%d' % (int(tfirst), li)], st['nnp_tf%d_b%d' % (int(tfirst), li)] = W, b
        files = sorted(os.listdir(os.path.join(folder, 'NN_parameters')))
        st['nnp_files'] = np.array(files)
        st['nnp_tf%d_W1_m' % int(tfirst)] = np.array(open(os.path.join(folder, 'NN_parameters', 'W1.m')).read().split('\n'))
        st['nnp_tf%d_B2_m' % int(tfirst)] = np.array(open(os.path.join(folder, 'NN_parameters', 'B2.m')).read().split('\n'))
        st['nnp_tf%d_W1_mat' % int(tfirst)] = _spio.loadmat(os.path.join(folder, 'NN_parameters', 'W1.mat'))['W1']
        st['nnp_tf%d_B3_mat' % int(tfirst)] = _spio.loadmat(os.path.join(folder, 'NN_parameters', 'B3.mat'))['B3']
    RV.tf = sys.modules['tensorflow']

    # Error behaviour of the kept constructor / methods: exception class and message of the reference for a list of
    # invalid calls (tests/test_assembly_golden.py replays the same list on the build).
    def err_of(fn):
        try:
            with _ctx.redirect_stdout(_io.StringIO()):
                fn()
        except Exception as e:                               # noqa: BLE001 -- the class is what is recorded
            return '%s: %s' % (type(e).__name__, e)
        return 'no error'

    PU[0] = 1
    v1 = RV.VarNet(pde1(), layerWidth=[5], discNum=5, bDiscNum=None, tDiscNum=6, integPnum=2)
    v1.tfData.sess, v1.tfData.model = MonitorSess(v1.tfData.compTowers[0], 1), (lambda t: ('model', t))
    v1.tfData.graph, v1.tfData.saver = None, SaverRec()
    v1.fixData.setFEdata()
    vm_ = RV.VarNet(pde_m, layerWidth=[5], discNum=5, bDiscNum=None, tDiscNum=6, MORdiscScheme=disc, integPnum=2)
    vm_.tfData = TowerRecord(1, 3)
    vm_.tfData.sess, vm_.tfData.model = MonitorSess(vm_.tfData.compTowers[0], 1), (lambda t: ('model', t))
    vm_.fixData.setFEdata()
    tmpf = tempfile.mkdtemp()
    calls = {
        'ctor_layerWidth_not_list': lambda: RV.VarNet(pde1(), layerWidth=5, discNum=5, bDiscNum=None, tDiscNum=6),
        'ctor_unknown_model': lambda: RV.VarNet(pde1(), layerWidth=[5], modelId='CNN', discNum=5, bDiscNum=None, tDiscNum=6),
        'ctor_no_tDiscNum': lambda: RV.VarNet(pde1(), layerWidth=[5], discNum=5, bDiscNum=None, tDiscNum=[]),
        'ctor_bDiscNum_list': lambda: RV.VarNet(pde1(), layerWidth=[5], discNum=5, tDiscNum=6),
        'ctor_mor_without_scheme': lambda: RV.VarNet(pde_m, layerWidth=[5], discNum=5, bDiscNum=None, tDiscNum=6),
        'ctor_integPnum_4': lambda: RV.VarNet(pde1(), layerWidth=[5], discNum=5, bDiscNum=None, tDiscNum=6, integPnum=4),
        'train_bad_scheme': lambda: v1.train(tmpf, smpScheme='adaptive', epochNum=1),
        'train_weight_length': lambda: v1.train(tmpf, weight=[1., 2.], epochNum=1),
        'train_batchNum_and_batchLen': lambda: v1.train(tmpf, weight=[1., 1., 1.], epochNum=1, batchNum=2, batchLen=5),
        'eval_wrong_dim': lambda: v1.evaluate(np.zeros([3, 2]), 0.5),
        'eval_t_mismatch': lambda: v1.evaluate(np.zeros([3, 1]), np.zeros([2, 1])),
        'eval_mor_nothing_given': lambda: vm_.evaluate(),
        'eval_mor_batch_too_high': lambda: vm_.evaluate(batch=7),
        'eval_mor_arg_dim': lambda: vm_.evaluate(np.zeros([3, 1]), 0.5, MORarg=np.zeros([1, 2])),
        'res_batch_too_high': lambda: vm_.residual(batch=7),
        'simres_no_plotpath': lambda: RV.VarNet(pde1(), layerWidth=[5], discNum=5, bDiscNum=None, tDiscNum=6).simRes(),
        'load_no_folder': lambda: RV.VarNet(pde1(), layerWidth=[5], discNum=5, bDiscNum=None, tDiscNum=6).loadModel(),
    }
    calls.update({
        'pde_diff_type': lambda: RA.ADPDE(RD.Domain1D(), diff='k', vel=1.0),
        'pde_vel_type': lambda: RA.ADPDE(RD.Domain1D(), diff=1.0, vel='v'),
        'pde_source_type': lambda: RA.ADPDE(RD.Domain1D(), diff=1.0, vel=1.0, source='s'),
        'pde_bcs_not_list': lambda: RA.ADPDE(RD.Domain1D(), diff=1.0, vel=1.0, BCs=(1, 2)),
        'pde_bcs_count': lambda: RA.ADPDE(RD.Domain1D(), diff=1.0, vel=1.0, BCs=[[0., 1., 0.]]),
        'pde_no_ic': lambda: RA.ADPDE(RD.Domain1D(), diff=1.0, vel=1.0, tInterval=[0, 1.0]),
        'pde_cex_type': lambda: RA.ADPDE(RD.Domain1D(), diff=1.0, vel=1.0, cEx=3.0),
        'pde_ddiff_type': lambda: RA.ADPDE(RD.Domain1D(), diff=1.0, vel=1.0, d_diff='g'),
        'dom1d_interval': lambda: RD.Domain1D(np.array([[0., 1.], [2., 3.]])),
        'dom1d_discnum': lambda: RD.Domain1D().getMesh([4, 5]),
        'dom2d_vertices': lambda: RD.PolygonDomain2D(np.array([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.]])),
        'dom2d_obstacle': lambda: RD.PolygonDomain2D(np.array([[0., 0.], [1., 0.], [0., 1.]]), np.array([[.2, .2], [.3, .2], [.2, .3]])),
        'dom2d_discnum': lambda: RD.PolygonDomain2D(np.array([[0., 0.], [1., 0.], [0., 1.]])).getMesh([4, 5, 6], 3),
        'dom2d_isinside_dim': lambda: RD.PolygonDomain2D(np.array([[0., 0.], [1., 0.], [0., 1.]])).isInside(np.zeros([3, 3])),
        'mor_handles_not_list': lambda: RM.MOR(diffFun, ['D'], [[0.003, 0.033]]) and RM.MOR('f', ['D'], [[0.003, 0.033]]),
        'mor_handle_not_callable': lambda: RM.MOR([3.0], ['D'], [[0.003, 0.033]]),
    })
    for name, fn in calls.items():
        st['err_' + name] = np.array(err_of(fn))

    # (8) trainWeight arithmetic: the three branches on fixed loss triples, time-dependent and steady
    triples = np.array([[0.37, 1.9, 42.0], [1e-3, 5.0, 0.2], [12.5, 0.04, 3.3e3]])
    weights = [[10., 10., 1.], [5., 1., 1.], [1., 2., 3.]]
    PU[0] = 1
    vn = RV.VarNet(pde1(), layerWidth=[5], discNum=5, bDiscNum=None, tDiscNum=6, integPnum=2)
    vn.trainRes = Log()
    vn_s.trainRes = Log()
    tw = {}
    for i, tr in enumerate(triples):
        for j, wt in enumerate(weights):
            for branch, (nw, uo) in (('default', (False, False)), ('normalize', (True, False)), ('original', (False, True))):
                for name, v, wts, trip in (('td', vn, wt, tr), ('steady', vn_s, wt[:2], tr)):
                    comp = np.reshape(trip, [3, 1]).copy()
                    if name == 'steady':
                        comp[1, 0] = 0.0                    # no initial condition
                    # ManageTrainData.splitLoss is a sess.run (VarNetUtility.py:1080-1088): fixed values instead
                    v.splitLoss = lambda tData, MORdiscArg=None, _c=comp: (_c.copy(), tData, None)
                    import contextlib
                    import io
                    try:
                        with contextlib.redirect_stdout(io.StringIO()):
                            trainW, _, lossVal = v.trainWeight(list(wts), None, None, nw, uo)
                    except ValueError as e:
                        # the reference itself fails here (normalizeW on a time-dependent problem: uf.vstack is
                        # handed an ndarray, VarNet.py:1127 / UtilityFunc.py:146): recorded as NaN
                        assert 'must be a list' in str(e), e
                        trainW = [np.nan] * 3
                    tw['%s_%s_t%d_w%d' % (name, branch, i, j)] = np.array(trainW, dtype=float)
    st['tw_triples'], st['tw_weights'] = triples, np.array(weights)
    for k, val in tw.items():
        st['tw_' + k] = val
    np.savez_compressed(os.path.join(OUT, 'assembly.npz'), **st)
    print('wrote', os.path.join(OUT, 'assembly.npz'), len(st), 'arrays')


if __name__ == '__main__':
    main()
