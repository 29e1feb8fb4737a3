"""
`VarNet` -- trainer / data assembly for the variational (weak-form) loss, with the reference's
constructor and `train / evaluate / residual / loadModel` surface
(/root/reference/VarNet.py:67-203, 1197-1692), re-designed around a GPU-resident engine:

  reference (TF1)                                   here (MI355X)
  ------------------------------------------------  ------------------------------------------
  nT-row fp64 NumPy arrays re-fed host->device on   built once on the host in fp64 (same
  EVERY step through sess.run(feed_dict)            arithmetic, so the fp32 values the device
  (VarNetUtility.py:840-854, 1044)                  sees are identical), uploaded once, resident
  N / dNt tiled to nT rows (FiniteElement.py:426)   period-integNum tables inside the engine
  towers in one process, grads summed on a          one process per GPU, contiguous test-function
  controller (TFModel.py:342-377)                   shard per rank, SUM all-reduce of the flat
                                                    gradient over RCCL (torch.distributed)
  loss read back every step (VarNetUtility.py:1044) accumulated on device, read once per epoch

Out of scope here: modelId='RNN', updateWeights (its working form is train(balance=...)), plots.
"""
import collections
import math
import os
import pickle
from datetime import datetime
import time
import warnings

import numpy as np

from . import balance as balance_rules
from .finite_element import FE
from .utility import UF

uf = UF()
shape = np.shape
size = np.size

# `train(dedup='auto')`: time model of one step in either formulation, fitted to 36 measured (grid, net) pairs on one MI355X
# (tools/dedup_auto_perf.py -> profiles/r6_dedup_auto_perf.txt; every pair the model sends to the de-duplicated formulation was
# measured faster there, and no pair it keeps row-wise was more than 4 % faster de-duplicated).  S = sum of the hidden widths:
#   row-wise        rows * row_ps * S
#   de-duplicated   unique points * point_ps * S + rows * asm_ps (the two assembly kernels) + fixed_us + param_ns * P
#                   (three more kernel boundaries and a second prologue that images the P parameters into LDS)
DEDUP_MODEL = {'row_ps': 4.5, 'point_ps': 6.2, 'asm_ps': 10.0, 'fixed_us': 20.0, 'param_ns': 2.2}


def unique_points(Input, feDim, hVec, device=None):
    """
    Unique quadrature points of an `Input` block (rows = test function x quadrature point).
    On the uniform grid the 2^feDim hat functions around an element share its quadrature points
    (VarNet.py:576-588), so rows repeat; coordinates reached from different nodes differ only by
    fp64 rounding and are merged on a lattice of h/4096.  Returns (first-occurrence row of every
    unique point, uid [n] row -> unique point, rowptr [U+1], rowidx [n] CSR inverse).
    With a CUDA `device` the sorts run there (torch.unique / stable argsort: the same maps, bit for bit, as the NumPy path --
    unique keys ascending, first occurrences, rows of a point in increasing order; 1.4 s -> 0.1 s at 15.4 M rows).
    """
    X = np.asarray(Input)[:, :feDim]
    h = np.reshape(np.asarray(hVec, dtype=float), (1, feDim))
    if device is not None and getattr(device, 'type', None) == 'cuda':
        import torch
        Xd = torch.as_tensor(np.ascontiguousarray(X, dtype=np.float64), device=device)
        k = torch.round((Xd - Xd.min(dim=0, keepdim=True).values) / torch.as_tensor(h, device=device) * 4096.0).to(torch.int64)
        kmax = k.max(dim=0).values.tolist()
        bits = [int(np.ceil(np.log2(max(int(m), 1) + 1))) for m in kmax]
        if sum(bits) <= 62:
            key = torch.zeros(k.shape[0], dtype=torch.int64, device=device)
            for d in range(feDim):
                key = (key << bits[d]) | k[:, d]
            _, uid = torch.unique(key, sorted=True, return_inverse=True)
            U = int(uid.max().item()) + 1
            n = uid.shape[0]
            first = torch.full((U,), n, dtype=torch.int64, device=device).scatter_reduce_(
                0, uid, torch.arange(n, dtype=torch.int64, device=device), reduce='amin', include_self=True)
            rowidx = torch.argsort(uid, stable=True)
            rowptr = torch.zeros(U + 1, dtype=torch.int64, device=device)
            rowptr[1:] = torch.cumsum(torch.bincount(uid, minlength=U), 0)
            return (first.cpu().numpy(), uid.to(torch.int32).cpu().numpy(), rowptr.to(torch.int32).cpu().numpy(),
                    rowidx.to(torch.int32).cpu().numpy())
    k = np.rint((X - X.min(axis=0, keepdims=True)) / h * 4096.0).astype(np.int64)
    bits = [int(np.ceil(np.log2(max(int(k[:, d].max()), 1) + 1))) for d in range(feDim)]
    if sum(bits) <= 62:
        key = np.zeros(X.shape[0], dtype=np.int64)
        for d in range(feDim):
            key = (key << bits[d]) | k[:, d]
        _, first, uid = np.unique(key, return_index=True, return_inverse=True)
    else:
        _, first, uid = np.unique(k, axis=0, return_index=True, return_inverse=True)
    uid = np.reshape(uid, -1).astype(np.int32)
    U = first.shape[0]
    rowidx = np.argsort(uid, kind='stable').astype(np.int32)
    rowptr = np.zeros(U + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(np.bincount(uid, minlength=U))
    return first, uid, rowptr, rowidx


# ======================================================================================
class FIXData:
    """
    Static discretisation data (/root/reference/VarNetUtility.py:204-463).  Differences from
    the reference: `N`, `dNx`, `dNt` are the period-`integNum` tables ([integNum], [integNum,dim],
    [integNum]) instead of nT-row tilings -- `rows()` materialises the tiled form on demand.
    """

    def __init__(self, vn, integPnum=2):
        dim = vn.dim
        PDE = vn.PDE
        domain = PDE.domain
        MORvar = PDE.MORvar
        timeDependent = PDE.timeDependent
        if timeDependent:
            feDim = dim + 1
            tDiscNum = vn.tDiscNum
            ht, t_coord = vn.timeDisc()
        else:
            feDim = dim
            tDiscNum = 1
            t_coord = []
        mesh = domain.getMesh(vn.discNum, vn.bDiscNum)
        dof = mesh.dof
        he = np.reshape(mesh.he, [dim, 1])
        hVec = np.vstack([he, ht]) if timeDependent else he
        uniform_biInput, biDof = vn.biTrainPoints(mesh, t_coord)
        nt = dof * tDiscNum
        biDimVal = domain.measure                                   # VarNetUtility.py:293

        lossVecflag = True
        if nt > 1e6:                                                # VarNetUtility.py:300-303
            lossVecflag = False
            mesh = domain.getMesh(discNum=100, bDiscNum=50)
            if timeDependent:
                _, t_coord = vn.timeDisc(tdof=100)
        coord = mesh.coordinates
        uniform_input = uf.pairMats(coord, t_coord) if timeDependent else coord
        if nt > 1e6:
            uniform_biInput, _ = vn.biTrainPoints(mesh, t_coord)

        if MORvar is not None:
            discArg = MORvar.discretizeArg(vn.MORdiscScheme)
            argInd = MORvar.argIndex(discArg)
            batchNum = len(argInd)
            if batchNum > 16:
                lossVecflag = False
        else:
            discArg, argInd, batchNum = None, None, 1

        self.dim, self.feDim, self.timeDependent = dim, feDim, timeDependent
        self.integPnum = integPnum
        self.dof, self.bdof = dof, mesh.bdof
        self.biDof0, self.nt0 = biDof, nt
        self.hVec, self.biDimVal = hVec, biDimVal
        self.detJvec = False
        self.lossVecflag = lossVecflag
        self.uniform_input, self.uniform_biInput = uniform_input, uniform_biInput
        self.MORbatchNum, self.MORargInd, self.MORdiscArg = batchNum, argInd, discArg
        self.cEx = self.uniform_inpData = self.d_diff = None
        self.integNum = self.biDof = self.bDofsum = self.nt = self.nT = None
        self.delta = self.integW = self.detJ = self.N = self.dNx = self.dNt = None

    def setInputData(self, vn):
        """Exact solution, PDE fields and grad(kappa) on `uniform_input` (VarNetUtility.py:364-411)."""
        dim, PDE = self.dim, vn.PDE
        ui = self.uniform_input
        Coord = ui[:, :dim]
        targ = [ui[:, dim:dim + 1]] if self.timeDependent else []
        self.cEx = PDE.cEx(Coord, *targ) if PDE.cEx is not None else None
        self.uniform_inpData = vn.PDEinpData(ui) if PDE.MORvar is None else [None] * 3
        self.d_diff = PDE.d_diffFun(Coord, *targ)

    def setFEdata(self):
        """FE tables of the initial uniform sampling (VarNetUtility.py:415-462)."""
        biDof = self.biDof0
        self.bDofsum = int(np.sum(biDof[:-1])) if self.timeDependent else int(np.sum(biDof))
        fe = FE(self.feDim, self.integPnum)
        integNum, detJ, delta, integW, N, dN = fe.basisTable(self.hVec)
        self.integNum, self.biDof = integNum, biDof
        self.segments, self.detJvec = None, False
        self.nt, self.nT = self.nt0, self.nt0 * integNum
        self.delta, self.integW, self.detJ = delta, integW, detJ
        self.N = N
        self.dNx = dN[:, 0:self.dim]
        self.dNt = dN[:, self.dim] if self.timeDependent else np.zeros(integNum)

    def rows(self, nt=None):
        """Tiled [nT,1], [nT,dim], [nT,1] forms of N, dNx, dNt (what the reference stores).  After
        `updateOptimData` with a support scaling the rows of the added (optimal) test functions
        come first and use their own tables (VarNetUtility.py:506-523)."""
        if getattr(self, 'segments', None):
            Ns, dNxs, dNts = [], [], []
            for cnt, N, dNx, dNt in self.segments:
                Ns.append(np.tile(N.reshape(-1, 1), (cnt, 1)))
                dNxs.append(np.tile(dNx, (cnt, 1)))
                dNts.append(np.tile(dNt.reshape(-1, 1), (cnt, 1)))
            return np.vstack(Ns), np.vstack(dNxs), np.vstack(dNts)
        nt = self.nt if nt is None else nt
        return (np.tile(self.N.reshape(-1, 1), (nt, 1)), np.tile(self.dNx, (nt, 1)),
                np.tile(self.dNt.reshape(-1, 1), (nt, 1)))

    def updateOptimData(self, frac, suppFactor):
        """
        Fixed data after `ceil(frac*nt0)` residual-driven test functions were ADDED in front of
        the uniform ones (VarNetUtility.py:466-545): new nt/nT/biDof/bDofsum; with a support scaling
        (`suppFactor != 1`) the added test functions get their own element sizes, so `detJ`
        becomes a per-test-function vector (`detJvec=True`) and N/dN per-row.
        """
        if self.nt > self.nt0:
            return
        nt0 = self.nt0
        nt1 = math.ceil(frac * nt0)
        scaled = np.abs(suppFactor - 1.0) > 1.e-15
        self.nt = nt0 + nt1
        self.nT = self.nt * self.integNum
        if scaled:
            fe = FE(self.feDim, self.integPnum)
            _, detJ1, _, _, N1, dN1 = fe.basisTable(suppFactor * self.hVec)
            dNt1 = dN1[:, self.dim] if self.timeDependent else np.zeros(self.integNum)
            self.segments = [(nt1, N1, dN1[:, 0:self.dim], dNt1), (nt0, self.N, self.dNx, self.dNt)]
            self.detJ = np.vstack([detJ1 * np.ones([nt1, 1]), self.detJ * np.ones([nt0, 1])])
            self.detJvec = True
        biDof = [b + math.ceil(frac * b) for b in self.biDof0]
        self.biDof = biDof
        self.bDofsum = int(np.sum(biDof[:-1])) if self.timeDependent else int(np.sum(biDof))


# ======================================================================================
class TrainResult:
    """
    Training record on disk with the reference's file formats (/root/reference/VarNetUtility.py:1149-1631),
    so existing post-processing keeps working:

      * `<folder>/caseData.txt` -- banner, date, problem header, the sections "Boundary condition
        information", "Neural Network architecture", "Processor information", "Optimizer information",
        "Space-time discretization information", "Sampling scheme ...", "Batch-optimization
        information", "Weighting information", "Stopping criteria", then "Training iterations:" followed
        by one "Epoch %2d: loss = %2.5f" line per reported epoch (:1217-1464, :1574-1588);
      * `<folder>/trainData.vn` -- pickle (HIGHEST_PROTOCOL) of the instance `__dict__` with the keys
        `casepath, plotpath, caseSimline, saveFreq, verbose, pltReplace, trainWeight, loss, lossComp,
        avgtime0, avgtime, residual, iterSmp, inpIter, error, lossVec, option_stopping,
        option_trainPoint, option_weighting, option_batchOptim` (:1512-1556);
      * histories are sampled every `saveFreq` epochs (`iterSmp`), epochs before the first `saveFreq` are
        only logged (:1577-1583).
    Plots (`iterPlot`) are out of scope; the `plots` folder is still created.
    """

    def __init__(self, folderpath, cExFlg=False, verbose=True, saveFreq=100, pltReplace=True):
        self.folderpath = folderpath
        self.verbose = verbose
        self.saveFreq = saveFreq
        self.pltReplace = pltReplace
        self.trainWeight = None
        self.casepath = None
        self.plotpath = None
        self.caseSimline = 0
        if folderpath is not None:
            self.plotpath = os.path.join(folderpath, 'plots')
            os.makedirs(self.plotpath, exist_ok=True)
            self.casepath = os.path.join(folderpath, 'caseData.txt')
        self.loss = []                    # total loss at the sampled epochs
        self.lossAll = []                 # (extension) total loss of every epoch
        self.lossComp = []                # [BC, IC, variational] at the sampled epochs
        self.avgtime0 = None              # reference iteration time from the first saveFreq epochs
        self.avgtime = 0
        self.residual = []
        self.iterSmp = []
        self.inpIter = []
        self.error = [] if not uf.isnone(cExFlg) else None      # (always a list: callers pass a bool)
        self.lossVec = None
        self.balanceHist = []             # (extension) one (epoch, weights, norms, cosines, skipped) per probe of train(balance=...)
        self.tfAdaptHist = []             # (extension) one (epoch, [stats of every batch]) per monitor of a run with tfAdapt=...
        self.bicAdaptHist = []            # (extension) one (epoch, {part: stats}) per monitor of a run with bicWeights= / bicAdapt=
        self.option_stopping = self.option_trainPoint = self.option_weighting = self.option_batchOptim = None

    # -- case file ------------------------------------------------------------------------------------
    def initializeCase(self, varNet, trainArg):
        g = trainArg.get
        self.option_stopping = {'epochNum': g('epochNum'), 'tol': g('tol')}
        self.option_trainPoint = {k: g(k) for k in ('smpScheme', 'frac', 'addTrainPts', 'suppFactor', 'multiTrainUpd',
                                                    'trainUpdelay', 'tolUpd', 'reinitrain')}
        self.option_weighting = {k: g(k) for k in ('weight', 'updateWeights', 'normalizeW', 'adjustWeight', 'useOriginalW')}
        self.option_batchOptim = {k: g(k) for k in ('saveMORdata', 'batchNum', 'batchLen', 'shuffleData', 'shuffleFreq')}
        if self.folderpath is None:
            return
        PDE, fd = varNet.PDE, varNet.fixData
        td, dim = PDE.timeDependent, varNet.dim
        MORoff = uf.isnone(PDE.MORvar)
        smp = g('smpScheme')
        bar = '-' * 79 + '\n'
        L = [bar, '=' * 31 + ' VarNet Library ' + '=' * 32 + '\n', bar,
             'MI355X-native engine (varnet_amd); file layout of the VarNet library, arXiv:1912.07443\n\n', bar]
        d, t = datetime.now().strftime('%d/%m/%Y %H:%M:%S').split()
        L.append('Simulation date: ' + d + ' - time: ' + t + '\n\n')
        L.append('%dD %s Advection-Diffusion problem %s model-order-reduction.\n\n'
                 % (dim, 'time-dependent' if td else 'steady-state', 'without' if MORoff else 'with'))
        L.append('Boundary condition information:\n')
        if dim == 1:
            L.append('\ttype:' + PDE.BCtype[0] + ', ' + PDE.BCtype[1] + '\n')
        else:
            geom = PDE.domain.boundryGeom.tolist()
            for bi in range(PDE.domain.bIndNum):
                L.append('\tBC%d: %s - vertices: %s\n' % (bi + 1, PDE.BCtype[bi], geom[bi]))
        for bInd, kind, rows in (varNet.fluxRows or {}).get('edges', []):
            L.append('\tBC%d: %s condition enforced as a boundary flux term on %d rows\n' % (bInd + 1, kind, rows))
        if getattr(varNet, 'obsRows', None) is not None:
            r = varNet.obsRows
            L.append('\tObservations: %d (%d points%s), weight %s\n'
                     % (len(r['value']), len(r['X']), '' if r['dir'] is None else ', with a derivative part', repr(float(varNet.obsWeight))))
        for A, B, rows in (getattr(varNet, 'periodicRows', None) or {}).get('pairs', []):
            L.append('\tBC%d and BC%d: periodic pair enforced on %d rows each, derivative weight %s\n'
                     % (A + 1, B + 1, rows, repr(float(varNet.periodicDeriv))))
        L.append('\n')
        if getattr(PDE, 'reaction', None) is not None:
            L.append('Reaction term: rate*(c1 c + c2 c^2 + c3 c^3), coefficients %s\n\n' % str(list(PDE.reactionCoef)))
        if getattr(PDE, 'nlflux', None) is not None:
            L.append('Flux term: -div(w*(f1 c + f2 c^2 + f3 c^3)), coefficients %s\n\n' % str(list(PDE.nlfluxCoef)))
        if getattr(PDE, 'nldiff', None) is not None:
            L.append('Solution-dependent diffusivity: div(diff*(d0 + d1 c + d2 c^2) grad c), coefficients %s\n\n'
                     % str(list(PDE.nldiffCoef)))
        if getattr(varNet, 'causal', None) is not None:
            L.append('Causal time-slab loss weights: eps = %s, %d slabs\n\n' % (repr(float(varNet.causal)), varNet.causalSlabNum()))
        if getattr(varNet, 'tfAdapt', None) is not None:
            ad = varNet.tfAdapt
            L.append('Self-adaptive test-function weights: rule %s, %s\n\n'
                     % (ad['rule'], ', '.join('%s = %r' % (k, ad[k]) for k in sorted(ad) if k != 'rule')))
        if getattr(varNet, 'bicWeights', None) is not None or getattr(varNet, 'bicAdapt', None) is not None:
            what = []
            for part in ('bc', 'ic'):
                ad = (varNet.bicAdapt or {}).get(part)
                if ad is not None:
                    what.append('%s: rule %s, %s' % (part, ad['rule'], ', '.join('%s = %r' % (k, ad[k]) for k in sorted(ad) if k != 'rule')))
                elif varNet.bicWeights is not None and part in varNet.bicWeights:
                    what.append('%s: static' % part)
            L.append('Weights on the boundary and initial rows: %s\n\n' % '; '.join(what))
        for stem, pr in (getattr(varNet, 'learntPrior', None) or {}).items():
            for key, b in pr['blocks'].items():
                L.append('Prior on the learnt %s%s: weight %s, matrix %s, mean %s, l1 %s\n\n'
                         % (stem, '' if key is None else '[%r]' % key, repr(b['weight']),
                            'identity' if np.array_equal(b['R'], np.eye(len(b['mean']))) else
                            'difference' if np.array_equal(b['R'], VarNet.priorMatrix('difference', len(b['mean']))) else
                            '%d x %d given' % b['R'].shape, [float(x) for x in b['mean']], [float(x) for x in b['l1']]))
        L.append('Neural Network architecture:\n')
        L.append('\ttype: ' + str(varNet.modelId) + '\n')
        L.append('\tnumber of inputs: ' + str(varNet.inpDim) + '\n')
        L.append('\tnumber of layers: ' + str(len(varNet.layerWidth)) + '\n')
        L.append('\tnumber of nodes in each layer: ' + str(varNet.layerWidth) + '\n')
        L.append('\tactivation function for each layer: ' + str(varNet.activationFun) + '\n')
        L.append('\ttotal number of trainable parameters: ' + str(varNet.engine.P) + '\n\n')
        L.append('Processor information:\n')
        if varNet.world > 1:
            L.append('\tparallel replicated training on %d processors\n' % varNet.world)
            L.append('\tutilized processors: ' + ' and '.join('GPU:%d' % r for r in range(varNet.world)) + '\n')
            L.append('master controller:GPU:0\n\n')
        else:
            L.append('\tutilized processor: GPU:0\n\n')
        L.append('Optimizer information:\n')
        if str(varNet.optimizer).lower() == 'lbfgs':
            L.append('\ttype: L-BFGS quasi-Newton algorithm (history 10, backtracking Armijo line search)\n\n')
        else:
            L.append('\ttype: %s stochastic gradient descent algorithm\n'
                     % ('RMSProp' if str(varNet.optimizer).lower() == 'rmsprop' else 'Adam'))
            L.append('\tlearning rate: ' + str(varNet.learning_rate) + '\n')
            if getattr(varNet, 'reparam', None) is not None:
                L.append('\tlearnt weight scales: %s, learning rate %s\n' % (varNet.reparam, varNet.reparamLr))
            L.append('\n')
        L.append('Space-time discretization information:\n')
        L.append('\tspatial domain interior discretization number: ' + str(varNet.discNum) + '\n')
        L.append('\tspatial domain boundary discretization density: ' + str(varNet.bDiscNum) + '\n')
        if td:
            L.append('\ttemporal discretization number: ' + str(varNet.tDiscNum) + '\n')
        L.append('\tnumber of training points: ' + str(fd.nt) + '\n')
        L.append('\tnumber of training points for BCs: ' + str(list(fd.biDof)[:-1]) + '\n')
        L.append('\ttotal number of BC training points: ' + str(fd.bDofsum) + '\n')
        if td:
            L.append('\tnumber of training points for IC: ' + str(list(fd.biDof)[-1]) + '\n')
        L.append('\n')
        L.append('Sampling scheme for training points: ' + str(smp) + '\n')
        if smp != 'uniform':
            L.append('\tfraction of non-uniform points: ' + str(g('frac')) + '\n')
            if g('addTrainPts'):
                L.append('\tnon-uniform points are added without replacement\n')
            if g('multiTrainUpd'):
                L.append('\tnon-uniform points updated every ' + str(g('trainUpdelay')) + ' epochs ...\n')
                L.append('\t... if decrease in 5 consecutive loss values is less than ' + str(g('tolUpd')) + '\n')
            else:
                L.append('\tnon-uniform points updated once after ' + str(g('trainUpdelay')) + ' epochs\n')
                L.append('\tif decrease in 5 consecutive loss values is less than ' + str(g('tolUpd')) + '\n')
            if smp == 'optimal' and np.abs(g('suppFactor') - 1.0) > 1.e-15:
                L.append('\tsupport of optimal training points is scaled by a factor of ' + str(g('suppFactor')) + '\n')
            if g('reinitrain'):
                L.append('\ttrainable variables are re-initialized after update of training points\n')
            L.append('Note: since for non-uniform grid the training points and possibly weights are updated\n'
                     '      the loss component plots will not necessarily match total loss plot!\n')
        L.append('\n')
        bN, bL = g('batchNum'), g('batchLen')
        if not (MORoff and uf.isnone(bN) and uf.isnone(bL)):
            L.append('Batch-optimization information:\n')
            if not MORoff:
                L.append('\tnumber of MOR batches: ' + str(fd.MORbatchNum) + '\n')
                if g('saveMORdata'):
                    L.append('\tMOR fields are stored for faster training.\n')
            if not uf.isnone(bN):
                L.append('\tnumber of training batches: ' + str(bN) + '\n')
            elif not uf.isnone(bL):
                L.append('\tlength of training batches: ' + str(bL) + '\n')
            if g('shuffleData'):
                L.append('\tshuffle training data every ' + str(g('shuffleFreq')) + ' epochs\n')
            if not (uf.isnone(bN) and uf.isnone(bL)):
                L.append('Note: for batch-optimization loss component values will not match total loss\n'
                         '      since intermediate iterations change total loss unlike loss components!\n')
            L.append('\n')
        L.append('Weighting information:\n')
        L.append('\trequested weights: ' + str(g('weight')) + '\n')
        if g('updateWeights'):
            L.append('\tweights updated to maintain the requested balance between terms\n')
        if g('balance') is not None:
            b = balance_rules.parse_balance(g('balance'))
            L.append('\tweights rebalanced from per-term gradient norms: rule %s, every %d epochs, alpha %s, cap %s, keepLoss %s\n'
                     % (b['rule'], b['freq'], repr(b['alpha']), repr(b['cap']), b['keepLoss']))
        if g('normalizeW'):
            L.append('\tweights normalized by values so that weight times values have requested weights\n')
        if smp != 'uniform' and g('adjustWeight'):
            L.append('\tweights on boundary-initial conditions updated after addition of non-uniform points\n')
        if g('useOriginalW'):
            L.append('\trequested weights applied without any modification\n')
        L.append('\n')
        L.append('Stopping criteria:\n')
        L.append('\tmaximum number of epochs: ' + str(g('epochNum')) + '\n')
        L.append('\tstopping tolerance: ' + str(g('tol')) + '\n\n')
        L.append('=' * 58 + '\n')
        L.append('Training iterations:\n\n')
        with open(self.casepath, 'w') as f:
            f.write(''.join(L))
        with open(self.casepath) as f:
            self.caseSimline = len(f.readlines()) - 4      # comments are inserted above the iteration header

    def writeCase(self, text):
        if not isinstance(text, str):
            raise ValueError('the input must be a string!')
        if self.casepath is None:
            return
        with open(self.casepath, 'a+') as f:
            f.write(text)

    def writeComment(self, text):
        """Insert `text` above the training iterations (post-simulation notes at the top of the case file)."""
        if not isinstance(text, str):
            raise ValueError('the input must be a string!')
        if self.casepath is None:
            return
        lines = [ln + '\n' for ln in text.split('\n')]
        with open(self.casepath) as f:
            data = f.readlines()
        data[self.caseSimline:self.caseSimline] = lines
        with open(self.casepath, 'w') as f:
            f.writelines(data)

    # -- pickle ----------------------------------------------------------------------------------------
    def saveData(self):
        if self.folderpath is None:
            return
        with open(os.path.join(self.folderpath, 'trainData.vn'), 'wb') as f:
            pickle.dump(self.__dict__, f, pickle.HIGHEST_PROTOCOL)

    def loadData(self):
        with open(os.path.join(self.folderpath, 'trainData.vn'), 'rb') as f:
            dump = pickle.load(f)
        for key in ('casepath', 'plotpath', 'caseSimline', 'saveFreq', 'verbose', 'pltReplace', 'trainWeight', 'loss',
                    'lossComp', 'avgtime0', 'avgtime', 'residual', 'iterSmp', 'inpIter', 'error', 'lossVec'):
            setattr(self, key, dump[key])
        try:                                                   # files written before the options were stored
            for key in ('option_stopping', 'option_trainPoint', 'option_weighting', 'option_batchOptim'):
                setattr(self, key, dump[key])
        except KeyError:
            warnings.warn('train() arguments not loaded!')

    # -- per-epoch report ------------------------------------------------------------------------------
    def iterOutput(self, epoch, current_loss, min_loss, epoch_time, resVal, err, lossSplit, lossVec):
        saveFreq = self.saveFreq
        self.lossAll.append(current_loss)
        if not (epoch < saveFreq or epoch % saveFreq == 0):
            return
        line = 'Epoch %2d: loss = %2.5f\n' % (epoch, current_loss)
        self.writeCase(line)
        if self.verbose:
            print(line, end='')
        if epoch < saveFreq:
            if epoch == saveFreq - 1:
                self.avgtime0 = epoch_time / epoch
            return
        self.iterSmp.append(epoch)
        self.loss.append(current_loss)
        self.lossComp.append(np.reshape(lossSplit, 3))
        self.residual.append(resVal)
        if self.error is not None:
            self.error.append(err)
        self.avgtime = epoch_time / epoch
        self.lossVec = lossVec
        self.saveData()
        if epoch % (10 * saveFreq) == 0:
            msg = '\nbest model loss: %2.5f\naverage iteration time: %2.5fs\n\n' % (min_loss, epoch_time / epoch)
            if self.verbose:
                print(msg, end='')
            self.writeCase(msg)
            # The reference redraws its five figures here (1.2 s at 300 dpi).  Its epochs take seconds; here 10 * saveFreq
            # epochs can pass in milliseconds, so a refresh is skipped while the last one is younger than `plotEvery`
            # seconds and VarNet.train flushes the pending one when it returns: same files, same final content.
            self._plot_dirty = True
            if time.perf_counter() - getattr(self, '_plot_last', -1e30) >= getattr(self, 'plotEvery', 30.0):
                self.iterPlot()

    def flushPlots(self):
        if getattr(self, '_plot_dirty', False):
            self.iterPlot()

    def iterPlot(self, plotpath=None, pltFrmt='png'):
        """
        Convergence plots the reference refreshes every 10 * saveFreq epochs (VarNetUtility.py:1634-1756), same file
        names: `loss`, `lossComp`, `scaled_lossComp`, `res_history` and, with an exact solution, `error` (prefixed by
        the epoch when pltReplace is False); dashed red lines mark the epochs at which the training set was redrawn.
        """
        if pltFrmt not in ('png', 'jpg', 'pdf', 'eps'):
            raise ValueError('invalid plot format!')
        self._plot_dirty = False
        self._plot_last = time.perf_counter()
        if self.folderpath is None or not self.iterSmp:          # a tower other than rank 0 keeps no files
            return
        try:
            import matplotlib
            matplotlib.use('Agg', force=False)
            import matplotlib.pyplot as plt
        except ImportError:                                   # no plotting library: the records in trainData.vn remain
            return
        ext = '.' + pltFrmt
        plotpath = self.plotpath if plotpath is None else plotpath
        os.makedirs(plotpath, exist_ok=True)
        pre = '' if self.pltReplace else '{}_'.format(self.iterSmp[-1])
        png = pltFrmt == 'png'
        it = np.asarray(self.iterSmp, dtype=float)
        it0 = np.concatenate([[0.0], it])
        comp = np.array([np.reshape(c, -1) for c in self.lossComp], dtype=float)

        def finish(fig, name, ylabel, title, legend=None):
            ax = fig.gca()
            ax.set_xlabel('epochs')
            ax.set_ylabel(ylabel)
            ax.set_title(title if png else '')
            if legend:
                ax.legend(legend)
            ax.grid(True)
            fig.savefig(os.path.join(plotpath, pre + name + ext), dpi=300)
            plt.close(fig)

        fig = plt.figure()
        fig.gca().semilogy(it, np.asarray(self.loss, dtype=float))
        for i in (self.inpIter or []):
            fig.gca().axvline(i, color='r', linestyle='--')
        finish(fig, 'loss', 'loss function', 'convergence plot (variable grid)')
        fig = plt.figure()
        for col, c in zip(range(3), 'brg'):
            fig.gca().semilogy(it0, comp[:, col], c)
        finish(fig, 'lossComp', 'loss components', 'loss components plot', ['BC', 'IC', 'integral term'])
        fig = plt.figure()
        tot = np.asarray(self.trainWeight, dtype=float) * comp
        for col, c in zip(range(3), 'brg'):
            fig.gca().semilogy(it0, tot[:, col], c)
        fig.gca().semilogy(it0, np.sum(tot, axis=1), 'k')
        finish(fig, 'scaled_lossComp', 'loss components', 'scaled loss components plot', ['BC', 'IC', 'integral term', 'total loss'])
        fig = plt.figure()
        fig.gca().semilogy(it, np.asarray(self.residual, dtype=float))
        finish(fig, 'res_history', 'residual', 'residual convergence plot')
        if self.error is not None:
            fig = plt.figure()
            fig.gca().semilogy(it, np.asarray(self.error, dtype=float))
            finish(fig, 'error', 'error', 'normalized solution error')


# ======================================================================================
# An adaptive weight state on the host, whoever holds it (a batch, or a part of the boundary and initial rows), is the arrays a
# checkpoint keeps of it under a key prefix: <prefix>lambda, <prefix>tau and, for the sa rule, <prefix>slots.
def _adapt_arrays(states):
    """{prefix: a state as engine.tf_adapt / engine.bic_adapt read it} -> those arrays, in one dict."""
    out = {}
    for prefix, st in states.items():
        out[prefix + 'lambda'], out[prefix + 'tau'] = st['lambda'], np.int64(st['stats']['tau'])
        if st['slots'] is not None:
            out[prefix + 'slots'] = st['slots']
    return out


def _adapt_put_back(arrays, prefix, put, key, n):
    """... and back into the registration of `key` with n weights (put: engine.set_*_adapt_state), if `arrays` has that many."""
    if arrays and prefix + 'lambda' in arrays and np.size(arrays[prefix + 'lambda']) == n:
        put(key, arrays[prefix + 'lambda'], arrays.get(prefix + 'slots'), int(arrays[prefix + 'tau']))


# ======================================================================================
class ManageTrainData:
    """
    Device-resident training set, sharded and batched the way the reference's feed dicts are
    (/root/reference/VarNetUtility.py:563-1017): whole test functions only, mini-batch x tower
    blocks of `batchLen = ceil(nt/batchNum/puNum)` consecutive test functions, BC/IC set
    replicated with its weights divided by batchNum*puNum.
    """

    def __init__(self, vn, mor_data, batchNum=None, batchLen=None):
        if batchNum is not None and batchLen is not None:
            raise ValueError('Only one of batch number or length properties must be provided!')
        self.vn = vn
        self.mor = mor_data                      # list (per MOR batch) of dicts of device tensors
        fd = vn.fixData
        self.nt, self.integNum = fd.nt, fd.integNum
        # snapshot of the fixed data this set was built with (the trainer may later re-sample)
        self.detJ, self.bDofsum, self.biDimVal = fd.detJ, fd.bDofsum, fd.biDimVal
        puNum = vn.world
        if batchNum is None and batchLen is None:
            batchNum = 1
        if batchNum is None:
            batchLen = min(int(batchLen), self.nt)
            batchNum = int(np.ceil(self.nt / batchLen / puNum))
        else:
            batchNum = int(batchNum)
            batchLen = int(np.ceil(self.nt / batchNum / puNum))
        self.batchNum, self.batchLen, self.puNum = batchNum, batchLen, puNum
        self.batchInd = np.arange(self.nt)
        self.shuffled = False
        self.dedup_on, self.dedup_reason = False, None
        self._register()

    def block(self, bi, tower=None):
        """[n0,n1) test-function range of a tower (default: this rank's) in mini-batch bi."""
        j = bi * self.puNum + (self.vn.rank if tower is None else tower)
        n0 = min(j * self.batchLen, self.nt)
        return n0, min(n0 + self.batchLen, self.nt)

    def engine_batch(self, mor_b, bi):
        return mor_b * self.batchNum + bi

    def towerWeights(self, trainW):
        """Weights one tower is fed: BC/IC terms divided by batchNum*puNum because every (mini-batch, tower)
        feed repeats the whole BC/IC set (updateDictFields('trainW'), VarNetUtility.py:900-901)."""
        w = np.array(trainW, dtype=float)
        w[:-1] = w[:-1] / self.batchNum / self.puNum
        return w

    def _register(self):
        eng, q = self.vn.engine, self.integNum
        torch = eng.torch
        adapt = getattr(self.vn, 'tfAdapt', None)
        if adapt is not None:
            # vn_set_interior clears the adaptive registrations: the set that holds them now (this one again, or the training set
            # while a monitor borrows the engine) keeps its state on the host and takes it back at its next registration
            owner = getattr(self.vn, '_adapt_owner', None)
            if owner is not None:
                own = {owner.engine_batch(mb, bi) for mb in range(len(owner.mor)) for bi in range(owner.batchNum)}
                owner._adapt_saved = _adapt_arrays({'%d_' % b: eng.tf_adapt(b) for b in eng.adapt_batches() if b in own})
        if self.shuffled:                         # one upload of the permutation per shuffle, not one per block
            perm_dev = self._upload_perm(torch, eng.device)
            rows_all = (perm_dev[:, None] * q + torch.arange(q, device=eng.device)[None, :]).reshape(-1)
        for mb, d in enumerate(self.mor):
            if self.shuffled:                     # one gather per array and parameter batch; the blocks are views of it
                d = dict(d)
                for key in ('Input', 'gcoef', 'source', 'N_rows', 'dNt_rows', 'rate', 'phi', 'psi'):
                    if d.get(key) is not None:
                        d[key] = d[key].index_select(0, rows_all)
                for key in ('srcphi', 'fldG'):    # [J, nT] and [J, nT, dim]: the rows are the second axis
                    if d.get(key) is not None:
                        d[key] = d[key].index_select(1, rows_all)
                for key in ('detJ', 'slab'):      # one entry per test function
                    if d.get(key) is not None:
                        d[key] = d[key].index_select(0, perm_dev)
            for bi in range(self.batchNum):
                n0, n1 = self.block(bi)
                pick = lambda t: None if t is None else t[n0 * q:n1 * q]
                pick_k = lambda t: None if t is None else t[n0:n1]
                detJ = pick_k(d.get('detJ'))
                eng.set_interior(self.engine_batch(mb, bi), pick(d['Input']), pick(d['gcoef']), pick(d['source']),
                                 n_k=n1 - n0, detJ=self.detJ if detJ is None else detJ,
                                 N_rows=pick(d.get('N_rows')), dNt_rows=pick(d.get('dNt_rows')))
                if d.get('az') is not None and n1 > n0:             # the ansatz streams of these rows (vn_set_ansatz)
                    eng.set_ansatz(self.engine_batch(mb, bi), *[pick(t) for t in d['az']])
                if d.get('reactCoef') is not None and n1 > n0:      # the reaction term of these rows (vn_set_reaction)
                    eng.set_reaction(self.engine_batch(mb, bi), pick(d.get('rate')), d['reactCoef'])
                if d.get('phi') is not None and n1 > n0:            # the flux term of these rows (vn_set_nlflux)
                    eng.set_nlflux(self.engine_batch(mb, bi), pick(d['phi']), d['nlfluxCoef'])
                if d.get('nldiffCoef') is not None and n1 > n0:     # the diffusivity D(u) of these rows (vn_set_nldiff)
                    eng.set_nldiff(self.engine_batch(mb, bi), pick(d.get('psi')), d['nldiffCoef'])
                if d.get('srcphi') is not None and n1 > n0:         # the source basis of these rows (vn_set_source_basis)
                    eng.set_source_basis(self.engine_batch(mb, bi), d['srcphi'][:, n0 * q:n1 * q].contiguous())
                if d.get('fldG') is not None and n1 > n0:           # the field basis of these rows (vn_set_field_basis)
                    eng.set_field_basis(self.engine_batch(mb, bi), d['fldG'][:, n0 * q:n1 * q].contiguous())
                if d.get('slab') is not None and n1 > n0 and self.vn.causal is not None:      # causal weights (vn_set_causal)
                    eng.set_causal(self.engine_batch(mb, bi), pick_k(d['slab']), self.vn.causalSlabNum(), float(self.vn.causal))
                if adapt is not None and n1 > n0:                    # self-adaptive weights (vn_set_tf_adapt), state carried
                    b = self.engine_batch(mb, bi)
                    eng.set_tf_adapt(b, adapt)
                    _adapt_put_back(getattr(self, '_adapt_saved', None), '%d_' % b, eng.set_tf_adapt_state, b, n1 - n0)
                perm = getattr(self, 'biPerm', {}).get(bi)
                if perm is not None and hasattr(eng, 'set_batch_bic'):
                    ix = torch.as_tensor(perm, device=eng.device, dtype=torch.long)
                    eng.set_batch_bic(self.engine_batch(mb, bi), d['biInput'].index_select(0, ix),
                                      d['biLabel'].index_select(0, ix))
                    if d.get('bicB') is not None:         # the copy's basis: the same permutation of the columns
                        eng.set_bic_basis(self.engine_batch(mb, bi), d['bicB'].index_select(1, ix).contiguous())
        if adapt is not None:
            self.vn._adapt_owner = self

    def _upload_perm(self, torch, device):
        """Test-function permutation -> device.  On the GPU through one of two persistent pinned buffers and an
        asynchronous copy (a pageable upload would wait for the running epoch; allocating pinned memory per shuffle costs
        tens of ms); a buffer is rewritten only after the event behind its last copy has completed."""
        if device.type != 'cuda':
            return torch.as_tensor(self.batchInd, device=device, dtype=torch.long)
        if not hasattr(self, '_pin'):
            n = len(self.batchInd)
            self._pin = [torch.empty(n, dtype=torch.long).pin_memory() for _ in range(2)]
            self._pin_ev = [None, None]
            self._pin_i = 0
        i = self._pin_i = 1 - self._pin_i
        if self._pin_ev[i] is not None:
            self._pin_ev[i].synchronize()
        self._pin[i].numpy()[:] = self.batchInd
        out = self._pin[i].to(device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        self._pin_ev[i] = ev
        return out

    def shuffleTrainData(self):
        """
        Reshuffle the mini-batches exactly like the reference (VarNetUtility.py:957-1017), drawing from the global NumPy
        stream in its call order, so that the same `np.random.seed` gives the same feeds: one permutation of the
        test-function order, then -- per (mini-batch, tower), cumulatively -- a permutation of ALL boundary/initial rows
        that the feed uses in place of the ordered set.  (That second permutation crosses the BC/IC split, so the rows
        that enter the BC mean and the IC mean change; with MOR it is overwritten by the next `trainData` call of every
        batch, VarNetUtility.py:921-926, and therefore has no effect there -- both reproduced.)  With towers, rank 0's
        seed is broadcast first so that every rank draws the same permutations.
        """
        self.vn._sync_sampling()
        np.random.shuffle(self.batchInd)
        nB = int(self.mor[0]['biInput'].shape[0])
        biInd = np.arange(nB)
        self.biPerm = {}
        for bi in range(self.batchNum):
            for tower in range(self.puNum):
                np.random.shuffle(biInd)
                if tower == self.vn.rank:
                    self.biPerm[bi] = biInd.copy()
        if self.vn.PDE.MORvar is not None:
            self.biPerm = {}                        # reset by updateDictFields before the batch is used
        self.shuffled = True
        self.dedup_on = False                       # vn_set_interior drops the registrations; a shuffled set is row-wise
        self._register()

    def activate(self):
        """(Re-)register this set's batches with the engine (after another set used it)."""
        self._register()
        if self.dedup_on:
            self.enable_dedup()

    def dedup_applies(self):
        """None when the de-duplicated formulation can serve this set, else the reason it cannot (a sentence)."""
        vn = self.vn
        fd = vn.fixData
        if self.shuffled:
            return 'the mini-batches are shuffled (the point map of every block would have to be rebuilt at each shuffle)'
        if fd.detJvec:
            return ('the training set is non-uniform (per-test-function supports, detJvec=True, VarNetUtility.py:466-545): '
                    'its rows share no quadrature points')
        if vn.dim > 3:
            return 'the problem has dim = %d > 3 space coordinates' % vn.dim
        if not hasattr(vn.engine, 'set_dedup'):
            return 'this engine has no vn_set_dedup'
        if not getattr(vn.engine, 'dedup_supported', lambda: True)():
            return ('the network %s with integNum = %d is outside the 8-wave fused kernel family the formulation runs on '
                    '(widths <= 64, <= 8 layers, integNum <= 256)' % (list(vn.layerWidth), self.integNum))
        return None

    def dedup_pays(self):
        """
        The rule behind `train(dedup='auto')`: True when the de-duplicated step is expected to be the faster one.
        It costs 8 F_pt per unique point in five launches against 6 F_pt per row in two, so it wins whenever the step is
        work-bound (up to 5.2 x on BASELINE config 3) and loses on steps so small that its three extra kernel boundaries and
        second prologue outweigh the work saved (0.5 x on an 8 000-row step).  Deterministic -- a function of the grid and
        the network, never of a timing -- so that a run is reproducible: DEDUP_MODEL, evaluated on the smallest block.
        """
        m = DEDUP_MODEL
        lw = [self.vn.inpDim] + list(self.vn.layerWidth) + [1]
        P = sum(a * b + b for a, b in zip(lw[:-1], lw[1:]))
        S = float(sum(self.vn.layerWidth))
        rows = min([(n1 - n0) * self.integNum for n0, n1 in map(self.block, range(self.batchNum)) if n1 > n0] or [0])
        if rows == 0:
            return False
        # the exact count of unique points is known only once the map is built (seconds of host work at 6.4 M rows): the
        # decision uses the grid's own ratio, 2^feDim rows per point reached from below
        U = rows / self.rows_per_point_estimate()
        t_row = rows * m['row_ps'] * S * 1e-6
        t_dd = U * m['point_ps'] * S * 1e-6 + rows * m['asm_ps'] * 1e-6 + m['fixed_us'] + m['param_ns'] * P * 1e-3
        return t_row >= t_dd

    def rows_per_point_estimate(self):
        """Rows per unique quadrature point of one block on the uniform grid, without building the map: per dimension a
        run of n consecutive hat functions covers n + 1 elements, so 2n element visits hit n + 1 distinct elements."""
        n0, n1 = self.block(0)
        nk = max(n1 - n0, 1)
        tdn = int(self.vn.tDiscNum) if self.vn.PDE.timeDependent else 1
        if self.vn.PDE.timeDependent:                 # blocks are contiguous in (space-major, time-minor) order
            nt_t = min(nk, tdn)
            ns = max(nk // tdn, 1)
        else:
            nt_t, ns = 1, nk
        r = 2.0 * nt_t / (nt_t + 1.0) if self.vn.PDE.timeDependent else 1.0
        per = max(ns ** (1.0 / self.vn.dim), 1.0)
        r *= (2.0 * per / (per + 1.0)) ** self.vn.dim
        return max(r, 1.0)

    def enable_dedup(self):
        """
        Switch every registered batch to the de-duplicated formulation (`vn_set_dedup`): one network
        evaluation per unique quadrature point instead of one per (test function, point) row.
        Needs the periodic FE tables (uniform supports) and an unshuffled set; returns the total
        number of unique points, or 0 if it does not apply -- `self.dedup_reason` then says why.
        """
        vn = self.vn
        fd = vn.fixData
        self.dedup_reason = self.dedup_applies()
        if self.dedup_reason is not None:
            return 0
        q, total = self.integNum, 0
        cache = getattr(self, '_dd_cache', {})
        for mb, d in enumerate(self.mor):
            for bi in range(self.batchNum):
                n0, n1 = self.block(bi)
                if n1 == n0:
                    continue
                key = (mb, bi)
                if key not in cache:
                    blk = d['Input_host'][n0 * q:n1 * q]
                    first, uid, rowptr, rowidx = unique_points(blk, fd.feDim, fd.hVec, getattr(vn.engine, 'device', None))
                    pts = None
                    if getattr(vn.PDE, 'ansatz', None) is not None:     # A, B and their gradients at the unique points
                        Xp = np.asarray(blk[first], dtype=np.float64)[:, :fd.feDim]
                        pts = tuple(vn.engine.dev(vn.PDE.ansatz_values(k, Xp, n)) for k, n in
                                    (('A', 1), ('B', 1), ('dA', vn.dim), ('dB', vn.dim)))
                    cache[key] = (vn.engine.dev(blk[first]), uid, rowptr, rowidx, pts)
                Xu, uid, rowptr, rowidx, pts = cache[key]
                # not applicable was decided above; an engine error here is a real failure and propagates
                vn.engine.set_dedup(self.engine_batch(mb, bi), Xu, uid, rowptr, rowidx)
                if pts is not None:
                    vn.engine.set_ansatz_points(self.engine_batch(mb, bi), *pts)
                total += Xu.shape[0]
        self._dd_cache = cache
        self.dedup_on = True
        return total

    def disable_dedup(self):
        """Back to the row-wise formulation for every registered batch (`vn_set_dedup` with no points)."""
        if not self.dedup_on:
            return
        for mb in range(len(self.mor)):
            for bi in range(self.batchNum):
                n0, n1 = self.block(bi)
                if n1 > n0:
                    self.vn.engine.set_dedup(self.engine_batch(mb, bi))
        self.dedup_on = False

    def select_mor(self, mb):
        # (called once per epoch and MOR batch: skipped while the engine still holds THIS set's rows of batch mb -- any other
        # set_bic, from another training set or a direct caller, clears the engine's note)
        eng = self.vn.engine
        key = getattr(self, '_bic_token', None)
        if key is None:
            key = self._bic_token = object()
        if getattr(eng, '_bic_key', None) == (key, mb):
            return
        d = self.mor[mb]
        self.vn._bic_weights_save()               # vn_set_bic clears the rows' weights: the set that holds them keeps its state
        eng.set_bic(d['biInput'], d['biLabel'], self.bDofsum, self.biDimVal)
        self.vn._bic_weights_register(self, d)    # bicWeights= / bicAdapt= on these rows, this set's own state carried
        if d.get('az_bic') is not None:           # the ansatz streams of these rows (vn_set_ansatz_rows)
            eng.set_ansatz_rows('bic', *d['az_bic'])
        if d.get('bicB') is not None:             # the basis of these labels (vn_set_bic_basis, the shared set)
            eng.set_bic_basis(-1, d['bicB'])
        eng._bic_key = (key, mb)


def parse_reparam(reparam):
    """The `reparam` option of VarNet as a full dict, or None.  'rwf' | 'slope' | {'kind': 'rwf', 'mean': 1.0, 'std': 0.1} |
    {'kind': 'slope', 'n': 10.0, 'per': 'layer' | 'neuron'}; anything else is a ValueError."""
    if reparam is None:
        return None
    if isinstance(reparam, str):
        reparam = {'kind': reparam}
    if not isinstance(reparam, dict) or reparam.get('kind') not in ('rwf', 'slope'):
        raise ValueError("reparam=%r: expected None, 'rwf', 'slope' or a dict with 'kind': 'rwf' | 'slope'" % (reparam,))
    kind = reparam['kind']
    allowed = {'rwf': ('kind', 'mean', 'std'), 'slope': ('kind', 'n', 'per')}[kind]
    extra = sorted(set(reparam) - set(allowed))
    if extra:
        raise ValueError('reparam=%r: unknown keys %s for kind %r (known: %s)' % (reparam, extra, kind, list(allowed)))
    num = lambda key, dflt: float(reparam.get(key, dflt))
    try:
        if kind == 'rwf':
            out = dict(kind='rwf', mean=num('mean', 1.0), std=num('std', 0.1), per='neuron', n=1.0)
            if not np.isfinite(out['mean']) or not np.isfinite(out['std']) or out['std'] < 0.0:
                raise ValueError('reparam=%r: mean must be finite and std finite and >= 0' % (reparam,))
        else:
            out = dict(kind='slope', n=num('n', 1.0), per=reparam.get('per', 'neuron'), mean=None, std=None)
            if not np.isfinite(out['n']) or out['n'] < 1.0:
                raise ValueError('reparam=%r: the slope factor n must be finite and >= 1' % (reparam,))
            if out['per'] not in ('neuron', 'layer'):
                raise ValueError("reparam=%r: per must be 'neuron' or 'layer'" % (reparam,))
    except TypeError:
        raise ValueError('reparam=%r: mean, std and n must be numbers' % (reparam,))
    return out


# ======================================================================================
class VarNet:
    def __init__(self, PDE, layerWidth=[20], modelId='MLP', activationFun=None, discNum=20,
                 bDiscNum=[], tDiscNum=[], MORdiscScheme=None, processors=None, controller=None,
                 integPnum=2, optimizer='adam', learning_rate=0.001, fluxBC=False, lbfgsLoss64=False,
                 causal=None, causalSlabs=None, periodicDeriv=None, observations=None, obsWeight=None,
                 learnCoef=None, coefLr=None, coefBounds=None, learnSource=None, sourceLr=None, sourceBounds=None,
                 learnField=None, fieldLr=None, fieldBounds=None, learnBic=None, bicLr=None, bicBounds=None,
                 learnFluxBC=None, fluxBCLr=None, fluxBCBounds=None, learntPrior=None, reparam=None, reparamLr=None,
                 tfAdapt=None, bicWeights=None, bicAdapt=None):
        dim = PDE.dim
        timeDependent = PDE.timeDependent
        MORvar = PDE.MORvar
        # argument checks: /root/reference/VarNet.py:147-171
        if size(discNum) != 1 and size(discNum) != dim:
            raise ValueError('dimension of the number of discretizations does not match dimension of the domain!')
        elif size(discNum) == 1:
            discNum = [int(np.reshape(discNum, -1)[0])] * dim
        if size(bDiscNum) != 1:
            raise ValueError('density of boundary discretizations must be a scalar!')
        if modelId == 'RNN':
            raise NotImplementedError('modelId=\'RNN\' is unfinished in the reference (TFModel.py:225,763) '
                                      'and out of scope here')
        if modelId != 'MLP':
            raise ValueError('unknown modelId!')
        if timeDependent and uf.isempty(tDiscNum):
            raise ValueError('time discretization number must be provided for time-dependent PDEs!')
        if activationFun is None:
            activationFun = 'sigmoid'
        if not isinstance(layerWidth, list):
            raise ValueError('layer widths should be given in a list!')
        if MORvar is not None and MORdiscScheme is None:
            raise ValueError('\'MORdiscScheme\' must be given for MOR!')
        if learning_rate < 0.0:
            raise ValueError('learning rate must be positive!')
        if optimizer.lower() == 'rms':
            optimizer = 'rmsprop'
        if optimizer.lower() not in ('adam', 'rmsprop', 'lbfgs'):
            raise ValueError('unknown optimizer requested!')
        if lbfgsLoss64 and optimizer.lower() != 'lbfgs':
            raise ValueError('lbfgsLoss64=True is an option of optimizer=\'lbfgs\' (the line search on the fp64 loss)')
        # reparam=... (extension; no reference counterpart): learnt weight scales theta_eff = f(s) (.) V -- random weight
        # factorization or adaptive activation slopes -- stepped jointly by Adam (`parse_reparam`, VNEngine.set_reparam)
        self.reparam = parse_reparam(reparam)
        self.reparamLr = None
        if self.reparam is None:
            if reparamLr is not None:
                raise ValueError('reparamLr=%r is an option of reparam=...' % (reparamLr,))
        else:
            self.reparamLr = float(learning_rate if reparamLr is None else reparamLr)
            if not np.isfinite(self.reparamLr) or self.reparamLr < 0.0:
                raise ValueError('reparamLr=%r must be a finite number >= 0' % (reparamLr,))
            if optimizer.lower() != 'adam':
                raise NotImplementedError('reparam=%r with optimizer=%r: the joint step on (V, s) is built for Adam only' % (reparam, optimizer))
            if isinstance(processors, (list, tuple)) and len(processors) > 1:
                raise NotImplementedError('reparam=%r with towers is not supported: the scales\' gradient after the all-reduce is not built' % (reparam,))
            if len(layerWidth) > 8 or max(layerWidth) > 64:
                raise NotImplementedError('reparam=%r on the layer-by-layer route is not supported: layerWidth=%s lies outside the fused / '
                                          'generic kernels\' range (8 layers, 64 wide)' % (reparam, list(layerWidth)))
        # causal=eps (extension; no reference counterpart): the variational loss of every test function is weighted by
        # exp(-eps * accumulated mean loss of the earlier time slabs), recomputed at every step and held constant for the
        # gradient (causal training, Wang, Sankaran, Perdikaris 2022); causalSlabs: number of slabs (default tDiscNum)
        if causal is not None:
            self._check_causal_eps(causal)
            if not timeDependent:
                raise ValueError('causal=%r needs a time-dependent PDE: a steady problem has no time slabs' % (causal,))
            if optimizer.lower() == 'lbfgs':
                raise ValueError('causal=%r with optimizer=\'lbfgs\': the causal weights move with the parameters but are held '
                                 'constant for the gradient, so the search direction is not the gradient of the reported loss and '
                                 'an Armijo test on it means nothing' % (causal,))
            if causalSlabs is not None and not (isinstance(causalSlabs, (int, np.integer)) and 1 <= int(causalSlabs) <= 4096):
                raise ValueError('causalSlabs must be an integer in [1, 4096]')
        elif causalSlabs is not None:
            raise ValueError('causalSlabs is an option of causal=eps')
        # tfAdapt=... (extension; no reference counterpart): one self-adaptive weight per test function, moved on the device at
        # every step from that step's own loss field (`tf_adapt_spec`, VNEngine.set_tf_adapt)
        self.tfAdapt = self._check_tf_adapt(tfAdapt, causal is not None, optimizer.lower() == 'lbfgs', MORvar is not None,
                                            isinstance(processors, (list, tuple)) and len(processors) > 1)
        # bicWeights=..., bicAdapt=... (extension; no reference counterpart): one weight per Dirichlet and initial row, static or
        # moved on the device at every step from that step's own errors (VNEngine.set_bic_weights / set_bic_adapt, DESIGN.md
        # section 35)
        self.bicWeights, self.bicAdapt = self._check_bic_weights(
            bicWeights, bicAdapt, optimizer.lower() == 'lbfgs', MORvar is not None,
            isinstance(processors, (list, tuple)) and len(processors) > 1, getattr(PDE, 'ansatz', None) is not None, timeDependent)
        self._bicw_owner = None
        if fluxBC and MORvar is not None:
            raise NotImplementedError('fluxBC=True with model-order reduction is not supported: the flux rows carry one label '
                                      'g/a per boundary point, shared by all batches, while a MOR problem needs per-batch labels '
                                      'and per-batch network inputs on them')

        # periodicDeriv=gamma (extension; no reference counterpart): weight of the normal-derivative match of the periodic pairs
        # of `PDE.periodic` against their value match; default 1, 0 matches values only
        if periodicDeriv is not None:
            if getattr(PDE, 'periodic', None) is None:
                raise ValueError('periodicDeriv=%r is an option of a PDE with periodic boundaries (ADPDE(..., periodic=[(A, B)]))'
                                 % (periodicDeriv,))
            if not isinstance(periodicDeriv, (int, float, np.integer, np.floating)) or isinstance(periodicDeriv, bool) \
                    or not np.isfinite(float(periodicDeriv)) or float(periodicDeriv) < 0.0:
                raise ValueError('periodicDeriv=%r must be a finite number >= 0' % (periodicDeriv,))

        learnt = {'learnCoef': (learnCoef, coefLr, coefBounds), 'learnSource': (learnSource, sourceLr, sourceBounds),
                  'learnField': (learnField, fieldLr, fieldBounds), 'learnBic': (learnBic, bicLr, bicBounds),
                  'learnFluxBC': (learnFluxBC, fluxBCLr, fluxBCBounds)}
        # fluxBasis / robinBasis (ADPDE) live on the flux rows: without fluxBC=True nothing would ever evaluate them
        if sum(self._keyed_sizes(self._FBC, PDE)) > 0 and not fluxBC:
            raise ValueError('the PDE carries a fluxBasis / robinBasis, which is data of the boundary-flux rows: it needs fluxBC=True')
        for lv in self.LEARNT:
            if learnt[lv.option][0] is not None and MORvar is not None:
                raise NotImplementedError('%s with model-order reduction is not supported: neither %s nor the observations it needs '
                                          'are' % (lv.option, lv.mor_lacks))
        # observations=... (extension; no reference counterpart): sensor data as linear functionals of the solution, fitted by a
        # misfit term obsWeight * O next to the PDE's loss (`obsData`)
        if observations is None:
            if obsWeight is not None:
                raise ValueError('obsWeight=%r is an option of observations=...' % (obsWeight,))
        else:
            if MORvar is not None:
                raise NotImplementedError('observations with model-order reduction are not supported: the observed points are '
                                          'assembled once, for all parameter batches, and carry no parameter inputs')
            self._check_obs_weight(1.0 if obsWeight is None else obsWeight)

        # ADPDE(..., ansatz={...}) (extension; no reference counterpart): the hard-constraint ansatz c = A + B N; what it does not
        # combine with is refused here, one sentence each
        if getattr(PDE, 'ansatz', None) is not None:
            if isinstance(processors, (list, tuple)) and len(processors) > 1:
                raise NotImplementedError('an ansatz with towers is not supported: the shards of the ansatz streams per rank are '
                                          'not built')
            if lbfgsLoss64:
                raise NotImplementedError('an ansatz with lbfgsLoss64=True is not supported: the fp64 objective does not carry the '
                                          'ansatz stage')
            for opt, (val, _, _) in learnt.items():
                if val is not None:
                    raise NotImplementedError('an ansatz with %s is not supported: the sums of a learnt vector next to the ansatz '
                                              'stage are not built' % opt)
        # learnCoef=..., learnSource=..., learnField=..., learnBic=... (extensions; no reference counterpart): inverse mode, source,
        # field and boundary data identification -- the masked polynomial coefficients of the PDE's reaction / flux / diffusivity,
        # the masked amplitudes of its source basis, those of its diffusivity and velocity bases and those of its Dirichlet and
        # initial bases are learnt next to the network from the observations (`coefLearnData`, `sourceLearnData`, `fieldLearnData`,
        # `bicLearnData`); learnFluxBC=...: flux boundary identification, likewise the masked amplitudes of its flux-datum and
        # Robin-coefficient bases (`fluxBCLearnData`)
        for lv in self.LEARNT:
            data = getattr(self, lv.parser)(PDE, *learnt[lv.option], learning_rate)
            setattr(self, lv.attr, data)
            if data is None:
                continue
            if observations is None:
                raise ValueError('%s needs observations=...: without interior data every %s admits a solution of the boundary value '
                                 'problem, so the loss cannot tell one value from another' % (lv.option, lv.noun))
            if optimizer.lower() != 'adam':
                raise NotImplementedError('%s with optimizer=%r: the %ss are updated by the Adam step only (an L-BFGS search over '
                                          '(parameters, %ss) and an RMSProp update are not built)'
                                          % (lv.option, optimizer, lv.noun, lv.noun))
            if causal is not None:
                raise NotImplementedError('%s with causal=%r: the causal weights are applied after the seeds the %s gradient is '
                                          'reduced from' % (lv.option, causal, lv.noun))
            if self.tfAdapt is not None:
                raise NotImplementedError('%s with tfAdapt=%r: the weights are applied after the seeds the %s gradient is '
                                          'reduced from' % (lv.option, tfAdapt, lv.noun))
            if self.bicWeights is not None or self.bicAdapt is not None:
                raise NotImplementedError('%s with bicWeights= / bicAdapt=: the %s sums next to the rows\' own pass are not built%s'
                                          % (lv.option, lv.noun, ', and learnt boundary data would move the labels the weights follow'
                                             if lv.option == 'learnBic' else ''))
        # learntPrior={stem: spec} (extension; no reference counterpart): a quadratic prior and L1 shrinkage on the learnt vectors
        # (`priorData`)
        self.learntPrior = self.priorData(PDE, learntPrior, {lv.stem: getattr(self, lv.attr) for lv in self.LEARNT})

        inpDim = dim + (1 if timeDependent else 0)
        if MORvar is not None:
            inpDim += int(np.sum(MORvar.varNum))
        lossOpt = {'integWflag': integPnum != 2}
        lossOpt['isSource'] = not (hasattr(PDE, 'source') and PDE.source == 0.0)   # VarNet.py:184
        if getattr(PDE, 'sourceBasis', None) is not None:
            lossOpt['isSource'] = True          # a basis is a source also when `source` itself is 0

        self.dim, self.discNum, self.bDiscNum, self.tDiscNum = dim, discNum, bDiscNum, tDiscNum
        self.MORdiscScheme = MORdiscScheme
        self.modelId, self.PDE = modelId, PDE
        self.layerWidth, self.inpDim, self.lossOpt = list(layerWidth), inpDim, lossOpt
        self.activationFun, self.optimizer, self.learning_rate = activationFun, optimizer, learning_rate
        self.processors, self.controller = processors, controller
        self.fluxBC, self.fluxRows = bool(fluxBC), None
        self.periodicDeriv = (1.0 if periodicDeriv is None else float(periodicDeriv)) \
            if getattr(PDE, 'periodic', None) is not None else None
        self.periodicRows = None
        self.obsRows = None if observations is None else self.obsData(observations, dim, inpDim)
        self.obsWeight = None if observations is None else (1.0 if obsWeight is None else float(obsWeight))
        self._obs_scale = 1.0            # factor of the last train() on the variational weight (trainWeight), applied to obsWeight
        self.lbfgsLoss64 = bool(lbfgsLoss64)
        self.causal = None if causal is None else float(causal)
        self.causalSlabs = None if causalSlabs is None else int(causalSlabs)

        self.fixData = FIXData(self, integPnum)
        self.fixData.setInputData(self)
        self.fixData.setFEdata()

        # distributed context: one process per GPU; world_size plays the reference's puNum
        self.rank, self.world, self.dist = 0, 1, None
        self._towers = None
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                self.dist, self.rank, self.world = dist, dist.get_rank(), dist.get_world_size()
        except ImportError:
            pass
        if self.tfAdapt is not None and self.world > 1:
            self._check_tf_adapt(tfAdapt, False, False, False, True)
        if (self.bicWeights is not None or self.bicAdapt is not None) and self.world > 1:
            self._check_bic_weights(bicWeights, bicAdapt, False, False, True, False, timeDependent)
        if self.causal is not None and (self.world > 1 or (isinstance(processors, (list, tuple)) and len(processors) > 1)):
            raise NotImplementedError('causal=%r with towers: a rank\'s slab means would cover only its shard of the test '
                                      'functions, so the ranks together would train another objective than one rank'
                                      % (causal,))
        for lv in self.LEARNT:
            if getattr(self, lv.attr) is not None and (self.world > 1 or (isinstance(processors, (list, tuple)) and len(processors) > 1)):
                raise NotImplementedError('%s with towers: %s are not part of the all-reduced buffer, so every rank would follow its '
                                          'own shard' % (lv.option, lv.grads))
        if isinstance(processors, (list, tuple)) and len(processors) > 1 and self.world == 1:
            # the reference's single-process multi-GPU call (TFModel.py:120-165): this process becomes the
            # controller of one forked child per GPU (varnet_amd/towers.py); it never touches the GPU itself
            from .towers import TowerGroup
            kw = dict(layerWidth=layerWidth, modelId=modelId, activationFun=activationFun, discNum=discNum,
                      bDiscNum=bDiscNum, tDiscNum=tDiscNum, MORdiscScheme=MORdiscScheme, processors=list(processors),
                      controller=controller, integPnum=integPnum, optimizer=optimizer, learning_rate=learning_rate,
                      fluxBC=fluxBC, lbfgsLoss64=lbfgsLoss64, causal=causal, causalSlabs=causalSlabs)
            if periodicDeriv is not None:
                kw['periodicDeriv'] = periodicDeriv
            if observations is not None:
                kw['observations'], kw['obsWeight'] = observations, obsWeight
            self._towers = TowerGroup(type(self), (PDE,), kw, list(processors))
            self.world = self._towers.world
            self.engine = self.tfData = None
            return
        self._rng = np.random.default_rng(12345)
        self.engine = self._make_engine(processors)
        if self.reparam is not None and self.world > 1:
            raise NotImplementedError('reparam=%r with towers is not supported: the scales\' gradient after the all-reduce is not built' % (reparam,))
        self._init_params(0)
        if getattr(PDE, 'ansatz', None) is not None:
            if self.world > 1:
                raise NotImplementedError('an ansatz with towers is not supported: the shards of the ansatz streams per rank are '
                                          'not built')
            from .engine import VN_KERNEL_LAYERED
            if hasattr(self.engine, 'kernel_path') and self.engine.kernel_path()[0] == VN_KERNEL_LAYERED:
                raise NotImplementedError('an ansatz on the layer-by-layer route is not supported: the network %s lies outside the '
                                          'hand-written kernels that run the ansatz stage\'s BC/IC and edge passes'
                                          % (list(layerWidth),))
        if self.lbfgsLoss64:
            self.engine.lbfgs_loss64(True)      # refused (VNError) where the fp64 objective is
        # tower gradient SUM (TFModel.py:342-377): by default an RCCL communicator inside the engine, so a
        # step is gradient -> all-reduce -> optimizer on one stream with one host call; VN_COMM=torch keeps the
        # collective in torch.distributed (three host calls per step)
        self.comm, self.comm_why = 'none', ''
        if self.world > 1:
            self.comm = 'torch'
            # auto: in-engine RCCL whenever the ranks own distinct GPUs (nccl backend); rccl: required; try: attempted
            # whatever the backend, falling back to torch.distributed; torch: never
            mode = os.environ.get('VN_COMM', 'auto')
            if hasattr(self.engine, 'comm_init_from_torch') and \
                    (mode in ('rccl', 'try') or (mode == 'auto' and self.dist.get_backend() == 'nccl')):
                # every rank must end up on the SAME route; the bootstrap itself is collective-safe (a rank that cannot
                # load RCCL makes ALL ranks skip it: VNEngine.comm_init_from_torch), so the decision needs no extra vote
                ok, why = self.engine.comm_init_from_torch(self.dist)
                self.comm_why = why                 # why the in-engine communicator was skipped ('' when it is up)
                if ok:
                    self.comm = 'rccl'
                else:
                    if mode == 'rccl':
                        raise RuntimeError('VN_COMM=rccl but the in-engine RCCL communicator did not come up on every rank'
                                           + (': ' + why if why else ''))
                    warnings.warn('in-engine RCCL communicator unavailable (%s): gradient SUM stays in torch.distributed'
                                  % (why or 'another rank failed'))
            else:
                self.comm_why = 'not attempted: VN_COMM=%s on the %s backend' % (mode, self.dist.get_backend())
        fd = self.fixData
        self.engine.set_fe_table(fd.N, fd.dNt, None if fd.integW is None else fd.integW)
        if self.fluxBC:
            # fixed for the whole run (the uniform boundary set; optimal re-draws resample Dirichlet rows only): registered once.
            # A network outside the kernels that run the flux pass is refused here, with the engine's sentence.
            self.fluxRows = self.fluxTrainData()
            r = self.fluxRows
            if r['X'].shape[0] > 0:
                self.engine.set_flux_bc(r['X'], r['normal'], r['coef'], r['label'], fd.biDimVal)
                if getattr(self.PDE, 'ansatz', None) is not None:       # u and its normal derivative under the ansatz
                    self.engine.set_ansatz_rows('flux', *self._ansatz_rows(r['X'], r['normal']))
                if r.get('basis') is not None:        # learnt flux and Robin amplitudes: the engine mixes coef and label itself
                    self.engine.set_fluxbc_basis(r['basis'], r['J_flux'])
        if getattr(self.PDE, 'periodic', None) is not None:
            # fixed for the whole run like the flux rows (optimal re-draws leave them on the uniform set): registered once; a
            # network outside the kernels that run the periodic pass is refused here, with the engine's sentence
            self.periodicRows = self.periodicTrainData()
            r = self.periodicRows
            self.engine.set_periodic(r['X'], r['dir'], self.periodicDeriv, fd.biDimVal)
            if getattr(self.PDE, 'ansatz', None) is not None:
                self.engine.set_ansatz_rows('periodic', *self._ansatz_rows(r['X'], r['dir'] if self.periodicDeriv > 0 else None))
        if self.obsRows is not None:
            # fixed for the whole run and replicated in every feed and on every rank like the Dirichlet rows (optimal re-draws leave
            # them alone): registered once; a network outside the kernels that run the pass is refused here, with the engine's sentence
            r = self.obsRows
            self.engine.set_observations(r['X'], r['value'], q=r['q'], dir=r['dir'], rowptr=r['rowptr'], wgt=r['wgt'],
                                         weight=self.obsWeight / self.world)
            if getattr(self.PDE, 'ansatz', None) is not None:
                self.engine.set_ansatz_rows('obs', *self._ansatz_rows(r['X'], r['dir']))
        for lv in self.LEARNT:
            # the engine owns a learnt vector from here on: every batch registered later reads the nine coefficients from its device
            # vector, and carries the basis streams of the source [J, nT], the field [J, nT, dim] and the BC/IC rows [J, nB]; those of
            # the flux and Robin amplitudes [J, nF] were registered with the flux rows above
            d = getattr(self, lv.attr)
            if d is not None:
                getattr(self.engine, 'set_%s_learn' % lv.kind)(d['mask'], d['init'], d['lo'], d['hi'], d['lr'])
                if lv.stem in self.learntPrior:
                    self._register_prior(lv)
        self.tfData = self.engine       # name kept for scripts that poke at `VarNet.tfData`
        from .launch import mark_stage
        mark_stage('engine_ready')      # past the launcher's bootstrap deadline: a rank that trains for hours is healthy

    # -- engine ----------------------------------------------------------------------------
    def _make_engine(self, processors):
        from .engine import VNEngine
        device = 0
        if isinstance(processors, (list, tuple)):
            if len(processors) > 1:
                # deliberate divergence (INTEGRATION.md "Multi-GPU"): TF-1 drives all towers from ONE process
                # (TFModel.py:120-165, 253-289); here every GPU has its own process.  Inside a launched rank the
                # list is accepted and this rank takes its own entry.
                if self.world > 1 and len(processors) == self.world:
                    processors = processors[self.rank]
                else:
                    raise ValueError('processors=%s lists %d GPUs but %d ranks are running: pass one entry per rank'
                                     % (processors, len(processors), self.world))
            else:
                processors = processors[0]
        if isinstance(processors, str):
            kind, _, idx = processors.partition(':')
            if kind.upper() != 'GPU':
                raise ValueError('requested processor %s is unavailable!' % processors)
            device = int(idx or 0)
        elif 'LOCAL_RANK' in os.environ:
            device = int(os.environ['LOCAL_RANK'])
        fd = self.fixData
        return VNEngine(self.dim, self.inpDim, self.layerWidth, self.PDE.timeDependent, fd.integNum,
                        isSource=self.lossOpt['isSource'], integWflag=self.lossOpt['integWflag'],
                        learning_rate=self.learning_rate, device=device, activationFun=self.activationFun,
                        optimizer_name=self.optimizer)

    # -- inverse mode: learnt PDE coefficients (extension) ------------------------------------------
    COEF_KEYS = ('reaction', 'nlflux', 'nldiff')

    @staticmethod
    def _pde_coefs(PDE):
        """(user-scale coefficients [9], engine scale [9]) of PDE: index 0..2 reaction, 3..5 flux, 6..8 diffusivity.  The engine
        carries rate * c for a reaction with a scalar rate (`_assemble` folds it in), c itself with a rate field."""
        c, scale = np.zeros(9), np.ones(9)
        c[6] = 1.0
        for g, (key, attr) in enumerate((('reaction', 'reactionCoef'), ('nlflux', 'nlfluxCoef'), ('nldiff', 'nldiffCoef'))):
            if getattr(PDE, key, None) is not None:
                v = [float(x) for x in getattr(PDE, attr)]
                c[3 * g:3 * g + 3] = (v + [0.0] * 3)[:3]
        if getattr(PDE, 'reaction', None) is not None and PDE.reactionRate is not None:
            scale[0:3] = float(PDE.reactionRate)
        return c, scale

    # -- the vectors learnt next to the network, in the engine's order: the option, its parser, the attribute that keeps the parsed
    # registration, the noun of an entry, what model-order reduction lacks for it, what towers lack, the checkpoint key, the stem
    # of the engine's get_* / set_* methods, the title of train()'s closing line, the kind in the engine's set_<kind>_learn, for
    # a vector made of two keyed parts its KeyedVector (else None), and the stem learntPrior={stem: ...} names it by
    LearntVector = collections.namedtuple('LearntVector', 'option parser attr noun mor_lacks grads key engine title kind keyed stem')
    # a vector of two parts, each the amplitudes of one basis of the PDE, which keeps part `key` as <key>Basis / <key>Amp: the stem
    # of its options (<stem>Lr, <stem>Bounds) and methods (<stem>Amplitudes, <stem>Grad, set<Stem>Amplitudes), the two keys in the
    # vector's order, the names of the two sizes in the parsed registration, and how messages call its bases and its amplitudes
    KeyedVector = collections.namedtuple('KeyedVector', 'stem keys sizes bases amps')
    LEARNT = (
        LearntVector('learnCoef', 'coefLearnData', 'coefLearn', 'coefficient', 'the three polynomial terms',
                     'the nine coefficient gradients', 'pde_coefficients', 'coefs', 'Learnt coefficients', 'coef', None, 'coef'),
        LearntVector('learnSource', 'sourceLearnData', 'srcLearn', 'amplitude', 'the source basis',
                     'the amplitude gradients', 'source_amplitudes', 'source_amps', 'Learnt source amplitudes', 'source', None,
                     'source'),
        LearntVector('learnField', 'fieldLearnData', 'fldLearn', 'amplitude', 'the field bases',
                     'the amplitude gradients', 'field_amplitudes', 'field_amps', 'Learnt field amplitudes (diff, then vel)', 'field',
                     KeyedVector('field', ('diff', 'vel'), ('Jk', 'Jv'), 'field', 'field amplitudes'), 'field'),
        LearntVector('learnBic', 'bicLearnData', 'bicLearn', 'amplitude', 'the boundary and initial bases',
                     'the amplitude gradients', 'bic_amplitudes', 'bic_amps', 'Learnt boundary and initial amplitudes (bc, then ic)', 'bic',
                     KeyedVector('bic', ('bc', 'ic'), ('Jb', 'Ji'), 'Dirichlet or initial', 'boundary or initial amplitudes'), 'bic'),
        # (its rows are an edge row set's, not a batch's or the BC/IC set's)
        LearntVector('learnFluxBC', 'fluxBCLearnData', 'fbcLearn', 'amplitude', 'the boundary-flux rows',
                     'the amplitude gradients', 'fluxbc_amplitudes', 'fluxbc_amps', 'Learnt flux and Robin amplitudes (flux, then robin)',
                     'fluxbc', KeyedVector('fluxBC', ('flux', 'robin'), ('Jl', 'Jc'), 'flux or Robin', 'flux or Robin amplitudes'), 'fluxBC'))
    _FIELD, _BIC, _FBC = LEARNT[2:]

    # -- what the learnt vectors' options share (coefLearnData, sourceLearnData and the keyed vectors') --
    @staticmethod
    def _learn_mask(sel, n, err):
        """A mask selection: True (all n entries) or a list of n 0/1/bool values; anything else raises ValueError(err)."""
        if sel is True:
            return np.ones(n, dtype=bool)
        isbool = lambda x: isinstance(x, (bool, np.bool_)) or (isinstance(x, (int, np.integer)) and x in (0, 1))
        if not isinstance(sel, (list, tuple, np.ndarray)) or len(sel) != n or not all(isbool(x) for x in sel):
            raise ValueError(err)
        return np.array([bool(x) for x in sel])

    @staticmethod
    def _learn_bounds(bounds, label, mask, init, noun, option, err, pair=True, scale=None):
        """A bounds selection over the entries of `mask` as (lo, hi) arrays: with `pair` one (lo, hi) for every learnt entry, or a
        list of one entry per mask entry, each None or (lo, hi) with None for an open side; any other shape raises
        ValueError(err).  `label` prefixes the messages about entry j (label[j]), `noun` and `option` name what it bounds; `scale`
        takes the bounds (checked against `init` as given) to the engine's scale."""
        n = len(mask)
        lo, hi = np.full(n, -np.inf), np.full(n, np.inf)
        if bounds is None:
            return lo, hi
        free = lambda x: x is None or (isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool))
        if pair and isinstance(bounds, (list, tuple)) and len(bounds) == 2 and all(free(x) for x in bounds):
            entries = [tuple(bounds) if mask[j] else None for j in range(n)]      # one pair: every learnt entry
        elif isinstance(bounds, (list, tuple)) and len(bounds) == n:
            entries = list(bounds)
        else:
            raise ValueError(err)
        for j, bd in enumerate(entries):
            if bd is None:
                continue
            if not mask[j]:
                raise ValueError('%s[%d] bounds %s that %s does not select' % (label, j, noun, option))
            if not isinstance(bd, (list, tuple)) or len(bd) != 2:
                raise ValueError('%s[%d] must be None or (lo, hi), got %r' % (label, j, bd))
            a = -np.inf if bd[0] is None else bd[0]
            b = np.inf if bd[1] is None else bd[1]
            for x in (a, b):
                if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or np.isnan(x):
                    raise ValueError('%s[%d] must hold numbers or None, got %r' % (label, j, bd))
            if a > b:
                raise ValueError('%s[%d]: lower bound %r above upper bound %r' % (label, j, a, b))
            if not a <= init[j] <= b:
                raise ValueError('%s[%d] = %r excludes the initial guess %r' % (label, j, bd, float(init[j])))
            ea, eb = float(a) * (1.0 if scale is None else scale[j]), float(b) * (1.0 if scale is None else scale[j])
            lo[j], hi[j] = min(ea, eb), max(ea, eb)
        return lo, hi

    @staticmethod
    def _learn_rate(lr, name, learning_rate):
        """The Adam rate of a learnt vector: option `name`, by default the network's learning rate."""
        lr = learning_rate if lr is None else lr
        if isinstance(lr, bool) or not isinstance(lr, (int, float, np.integer, np.floating)) or not np.isfinite(lr) or lr <= 0:
            raise ValueError('%s=%r must be a finite number > 0' % (name, lr))
        return float(lr)

    @staticmethod
    def coefLearnData(PDE, learnCoef, coefLr=None, coefBounds=None, learning_rate=0.001):
        """(No reference counterpart: `VarNet(..., learnCoef=...)`.)  The registration of `vn_set_coef_learn` in the engine's
        scale, or None without learnCoef: mask, init, lo, hi (nine entries each), lr, and `scale`, by which `coefficients()`
        divides (the rate of a reaction with a scalar rate, 1 elsewhere).  learnCoef = {'reaction' | 'nlflux' | 'nldiff': True or
        a 3-mask}; the PDE's own coefficients are the initial guess; coefLr defaults to the network's learning rate;
        coefBounds = {key: [None | (lo, hi) x 3]} with None for an open side."""
        keys = VarNet.COEF_KEYS
        if learnCoef is None:
            if coefLr is not None:
                raise ValueError('coefLr=%r is an option of learnCoef=...' % (coefLr,))
            if coefBounds is not None:
                raise ValueError('coefBounds is an option of learnCoef=...')
            return None
        if not isinstance(learnCoef, dict) or not learnCoef:
            raise ValueError('learnCoef must be a dict with keys among %s' % (keys,))
        mask = np.zeros(9, dtype=bool)
        for key, val in learnCoef.items():
            if key not in keys:
                raise ValueError('learnCoef: unknown key %r (the keys are %s)' % (key, keys))
            if getattr(PDE, key, None) is None:
                raise ValueError('learnCoef: the PDE has no %s term (ADPDE(..., %s=...))' % (key, key))
            g = keys.index(key)
            mask[3 * g:3 * g + 3] = VarNet._learn_mask(val, 3, 'learnCoef[%r] must be True or a mask of three booleans, got %r' % (key, val))
        if not mask.any():
            raise ValueError('learnCoef selects no coefficient')
        lr = VarNet._learn_rate(coefLr, 'coefLr', learning_rate)
        c, scale = VarNet._pde_coefs(PDE)
        if mask[0:3].any() and scale[0] == 0.0:
            raise ValueError('learnCoef[\'reaction\'] with a reaction rate of 0: the engine learns rate * c and coefficients() '
                             'divides by the rate')
        lo, hi = np.full(9, -np.inf), np.full(9, np.inf)
        if coefBounds is not None:
            if not isinstance(coefBounds, dict):
                raise ValueError('coefBounds must be a dict with keys among %s' % (keys,))
            for key, val in coefBounds.items():
                if key not in keys:
                    raise ValueError('coefBounds: unknown key %r (the keys are %s)' % (key, keys))
                t = slice(3 * keys.index(key), 3 * keys.index(key) + 3)
                lo[t], hi[t] = VarNet._learn_bounds(val, 'coefBounds[%r]' % (key,), mask[t], c[t], 'a coefficient', 'learnCoef',
                                                    'coefBounds[%r] must list three entries, each None or (lo, hi)' % (key,),
                                                    pair=False, scale=scale[t])
        return dict(mask=[int(x) for x in mask], init=c * scale, lo=lo, hi=hi, lr=lr, scale=scale)

    def _coef_dict(self, v):
        return {k: [float(x) for x in v[3 * g:3 * g + 3]] for g, k in enumerate(self.COEF_KEYS)}

    def coefficients(self):
        """{'reaction': [c1, c2, c3], 'nlflux': [f1, f2, f3], 'nldiff': [d0, d1, d2]} at the current state: the learnt values
        with learnCoef (a reaction with a scalar rate is divided by it: the engine learns rate * c), else the PDE's own."""
        if self.coefLearn is None:
            return self._coef_dict(self._pde_coefs(self.PDE)[0])
        return self._coef_dict(self.engine.get_coefs() / self.coefLearn['scale'])

    def coefGrad(self):
        """d loss / d coefficient of the last gradient evaluation, in the layout of `coefficients()` (zeros where not learnt)."""
        if self.coefLearn is None:
            raise ValueError('coefGrad: this instance learns no coefficients (learnCoef=...)')
        return self._coef_dict(self.engine.get_coefs(grad=True)[1] * self.coefLearn['scale'])

    def setCoefficients(self, coef):
        """Overwrite coefficients between train() calls: {'reaction' | 'nlflux' | 'nldiff': three numbers}; keys left out keep
        their values.  Not clamped to coefBounds (the next update is)."""
        if self.coefLearn is None:
            raise ValueError('setCoefficients: this instance learns no coefficients (learnCoef=...)')
        if not isinstance(coef, dict):
            raise ValueError('setCoefficients takes a dict with keys among %s' % (self.COEF_KEYS,))
        v = self.engine.get_coefs() / self.coefLearn['scale']
        for key, val in coef.items():
            if key not in self.COEF_KEYS:
                raise ValueError('setCoefficients: unknown key %r (the keys are %s)' % (key, self.COEF_KEYS))
            a = np.asarray(val, dtype=np.float64).reshape(-1)
            if a.size != 3 or not np.all(np.isfinite(a)):
                raise ValueError('setCoefficients[%r] must hold three finite numbers, got %r' % (key, val))
            g = self.COEF_KEYS.index(key)
            v[3 * g:3 * g + 3] = a
        self.engine.set_coefs(v * self.coefLearn['scale'])

    # -- source identification: learnt amplitudes of a source basis (extension) ------------------------
    @staticmethod
    def sourceLearnData(PDE, learnSource, sourceLr=None, sourceBounds=None, learning_rate=0.001):
        """(No reference counterpart: `VarNet(..., learnSource=...)`.)  The registration of `vn_set_source_learn`, or None without
        learnSource: mask, init, lo, hi (J entries each) and lr.  learnSource = True or a mask of J booleans; the PDE's sourceAmp
        is the initial guess; sourceLr defaults to the network's learning rate; sourceBounds = (lo, hi) for every learnt
        amplitude or a list of J entries, each None or (lo, hi), with None for an open side."""
        if learnSource is None or learnSource is False:
            if sourceLr is not None:
                raise ValueError('sourceLr=%r is an option of learnSource=...' % (sourceLr,))
            if sourceBounds is not None:
                raise ValueError('sourceBounds is an option of learnSource=...')
            return None
        basis = getattr(PDE, 'sourceBasis', None)
        if basis is None:
            raise ValueError('learnSource: the PDE has no source basis (ADPDE(..., sourceBasis=[phi_1, ..., phi_J]))')
        J = len(basis)
        mask = VarNet._learn_mask(learnSource, J, 'learnSource must be True or a mask of %d booleans (one per function of sourceBasis), '
                                  'got %r' % (J, learnSource))
        if not mask.any():
            raise ValueError('learnSource selects no amplitude')
        lr = VarNet._learn_rate(sourceLr, 'sourceLr', learning_rate)
        a0 = np.asarray(PDE.sourceAmp, dtype=np.float64)
        lo, hi = VarNet._learn_bounds(sourceBounds, 'sourceBounds', mask, a0, 'an amplitude', 'learnSource',
                                      'sourceBounds must be (lo, hi) or a list of %d entries, each None or (lo, hi), got %r'
                                      % (J, sourceBounds))
        return dict(mask=[int(x) for x in mask], init=a0.copy(), lo=lo, hi=hi, lr=lr)

    def _source_basis(self, Input):
        """The basis functions of the PDE's source at the rows of Input, [n, J] in fp64, evaluated like the source (PDEinpData)."""
        dim, PDE = self.dim, self.PDE
        targ = [Input[:, dim][np.newaxis].T] if PDE.timeDependent else []
        n = Input.shape[0]
        cols = []
        for j, f in enumerate(PDE.sourceBasis):
            v = np.asarray(f(Input[:, 0:dim], *targ), dtype=np.float64)
            if v.size != n:
                raise ValueError('sourceBasis[%d] must return one value per point (a column), got shape %s for %d points'
                                 % (j, v.shape, n))
            cols.append(v.reshape(n))
        return np.stack(cols, axis=1)

    def sourceAmplitudes(self):
        """The J amplitudes of the PDE's source basis at the current state: the learnt values with learnSource, else the PDE's."""
        if getattr(self.PDE, 'sourceBasis', None) is None:
            raise ValueError('sourceAmplitudes: the PDE has no source basis (ADPDE(..., sourceBasis=[...]))')
        if getattr(self, 'srcLearn', None) is None or getattr(self, 'engine', None) is None:
            return np.array(self.PDE.sourceAmp, dtype=np.float64)
        return np.asarray(self.engine.get_source_amps(J=len(self.PDE.sourceBasis)), dtype=np.float64)

    def sourceGrad(self):
        """d loss / d amplitude of the last gradient evaluation, J values (zeros where not learnt)."""
        if self.srcLearn is None:
            raise ValueError('sourceGrad: this instance learns no source amplitudes (learnSource=...)')
        return np.asarray(self.engine.get_source_amps(grad=True, J=len(self.PDE.sourceBasis))[1], dtype=np.float64)

    def setSourceAmplitudes(self, a):
        """Overwrite the J amplitudes between train() calls.  Not clamped to sourceBounds (the next update is)."""
        if self.srcLearn is None:
            raise ValueError('setSourceAmplitudes: this instance learns no source amplitudes (learnSource=...)')
        J = len(self.PDE.sourceBasis)
        try:
            v = np.asarray(a, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            v = np.empty(0)
        if v.size != J or not np.all(np.isfinite(v)):
            raise ValueError('setSourceAmplitudes takes %d finite numbers, got %r' % (J, a))
        self.engine.set_source_amps(v)

    # -- the vectors of two keyed parts (field, boundary data and flux boundary identification): one path, taking the LEARNT row --
    @staticmethod
    def _keyed_sizes(lv, PDE):
        """The number of functions of the PDE's two bases of the keyed vector `lv` (0 without one)."""
        return tuple(len(getattr(PDE, key + 'Basis', None) or []) for key in lv.keyed.keys)

    @staticmethod
    def _keyed_learn_data(lv, PDE, learn, lr, bounds, learning_rate):
        """The registration of the keyed vector `lv`, or None without its option: what fieldLearnData, bicLearnData and
        fluxBCLearnData return."""
        kv, option = lv.keyed, lv.option
        lrName, bName = kv.stem + 'Lr', kv.stem + 'Bounds'
        if learn is None or learn is False:
            if lr is not None:
                raise ValueError('%s=%r is an option of %s=...' % (lrName, lr, option))
            if bounds is not None:
                raise ValueError('%s is an option of %s=...' % (bName, option))
            return None
        keys = kv.keys
        if not isinstance(learn, dict) or not learn or any(k not in keys for k in learn):
            raise ValueError('%s must be a dict {%r: True | mask, %r: True | mask}, got %r' % (option, keys[0], keys[1], learn))
        if bounds is not None and (not isinstance(bounds, dict) or any(k not in keys for k in bounds)):
            raise ValueError('%s must be a dict {%r: ..., %r: ...}, got %r' % (bName, keys[0], keys[1], bounds))
        Js = VarNet._keyed_sizes(lv, PDE)
        masks, a0s, los, his = [], [], [], []
        for key, J in zip(keys, Js):
            sel = learn.get(key)
            if sel is not None and sel is not False and J == 0:
                raise ValueError('%s[%r]: the PDE has no %s basis (ADPDE(..., %sBasis=[...]))' % (option, key, key, key))
            if J == 0:
                if bounds is not None and bounds.get(key) is not None:
                    raise ValueError('%s[%r]: the PDE has no %s basis (ADPDE(..., %sBasis=[...]))' % (bName, key, key, key))
                continue
            if sel is None or sel is False:
                mask = np.zeros(J, dtype=bool)
            else:
                mask = VarNet._learn_mask(sel, J, '%s[%r] must be True or a mask of %d booleans (one per function of %sBasis), '
                                          'got %r' % (option, key, J, key, sel))
            a0 = np.asarray(getattr(PDE, key + 'Amp'), dtype=np.float64)
            bd = None if bounds is None else bounds.get(key)
            lo, hi = VarNet._learn_bounds(bd, '%s[%r]' % (bName, key), mask, a0, 'an amplitude', option,
                                          '%s[%r] must be (lo, hi) or a list of %d entries, each None or (lo, hi), got %r'
                                          % (bName, key, J, bd))
            masks.append(mask); a0s.append(a0); los.append(lo); his.append(hi)
        if not any(m.any() for m in masks):
            raise ValueError('%s selects no amplitude' % option)
        lr = VarNet._learn_rate(lr, lrName, learning_rate)
        return dict(mask=[int(x) for x in np.concatenate(masks)], init=np.concatenate(a0s), lo=np.concatenate(los),
                    hi=np.concatenate(his), lr=lr, **dict(zip(kv.sizes, Js)))

    def _keyed_vector(self, lv):
        """The amplitudes of the keyed vector `lv` as one vector, first key first: the engine's if learnt, else the PDE's."""
        if getattr(self, lv.attr, None) is not None and getattr(self, 'engine', None) is not None:
            return np.asarray(getattr(self.engine, 'get_' + lv.engine)(J=sum(self._keyed_sizes(lv, self.PDE))), dtype=np.float64)
        return np.concatenate([np.asarray(getattr(self.PDE, key + 'Amp', []), dtype=np.float64) for key in lv.keyed.keys])

    def _keyed_dict(self, lv, v):
        """The vector v of `lv` as {key: its part}."""
        (k0, k1), J0 = lv.keyed.keys, self._keyed_sizes(lv, self.PDE)[0]
        return {k0: v[:J0].copy(), k1: v[J0:].copy()}

    def _keyed_amplitudes(self, lv):
        kv = lv.keyed
        if sum(self._keyed_sizes(lv, self.PDE)) == 0:
            raise ValueError('%sAmplitudes: the PDE has no %s basis (ADPDE(..., %sBasis=[...], %sBasis=[...]))'
                             % (kv.stem, kv.bases, *kv.keys))
        return self._keyed_dict(lv, self._keyed_vector(lv))

    def _keyed_grad(self, lv):
        if getattr(self, lv.attr) is None:
            raise ValueError('%sGrad: this instance learns no %s (%s=...)' % (lv.keyed.stem, lv.keyed.amps, lv.option))
        J = sum(self._keyed_sizes(lv, self.PDE))
        return self._keyed_dict(lv, np.asarray(getattr(self.engine, 'get_' + lv.engine)(grad=True, J=J)[1], dtype=np.float64))

    def _keyed_set(self, lv, amps):
        kv = lv.keyed
        name = 'set%s%sAmplitudes' % (kv.stem[0].upper(), kv.stem[1:])
        if getattr(self, lv.attr) is None:
            raise ValueError('%s: this instance learns no %s (%s=...)' % (name, kv.amps, lv.option))
        if not isinstance(amps, dict) or not amps or any(k not in kv.keys for k in amps):
            raise ValueError('%s takes a dict {%r: [...], %r: [...]}, got %r' % (name, *kv.keys, amps))
        cur, i0 = self._keyed_vector(lv), 0
        for key, J in zip(kv.keys, self._keyed_sizes(lv, self.PDE)):
            i0 += J
            if key not in amps:
                continue
            try:
                v = np.asarray(amps[key], dtype=np.float64).reshape(-1)
            except (TypeError, ValueError):
                v = np.empty(0)
            if J == 0 or v.size != J or not np.all(np.isfinite(v)):
                raise ValueError('%s[%r] takes %d finite numbers, got %r' % (name, key, J, amps[key]))
            cur[i0 - J:i0] = v
        getattr(self.engine, 'set_' + lv.engine)(cur)

    def _edge_basis(self, X, span, names):
        """The (bInd, f) entries of the PDE's bases `names`, in that order, at the rows X: [J, n] in fp64, every function
        evaluated like the `g` of a boundary condition on the rows span[bInd] = (first, end) of its own indicator and zero
        elsewhere; a wrong shape names the entry."""
        dim, PDE = self.dim, self.PDE
        entries = [(name, j, e) for name in names for j, e in enumerate(getattr(PDE, name, None) or [])]
        S = np.zeros((len(entries), X.shape[0]), dtype=np.float64)
        for row, (name, j, (bInd, f)) in enumerate(entries):
            r0, r1 = span[bInd]
            x = X[r0:r1]
            targ = [x[:, dim:dim + 1]] if PDE.timeDependent else []
            v = np.asarray(f(x[:, :dim], *targ), dtype=np.float64)
            if v.size != r1 - r0:
                raise ValueError('%s[%d] must return one value per point (a column), got shape %s for %d points'
                                 % (name, j, v.shape, r1 - r0))
            S[row, r0:r1] = v.reshape(-1)
        return S

    # -- field identification: learnt amplitudes of a diffusivity and a velocity basis (extension) -----
    @staticmethod
    def fieldLearnData(PDE, learnField, fieldLr=None, fieldBounds=None, learning_rate=0.001):
        """(No reference counterpart: `VarNet(..., learnField=...)`.)  The registration of `vn_set_field_learn`, or None without
        learnField: mask, init, lo, hi (J = J_kappa + J_v entries each, the diffusivity streams first), lr, Jk and Jv.  learnField =
        {'diff': True | mask, 'vel': True | mask} (a key left out: none of that basis is learnt); the PDE's diffAmp / velAmp are the
        initial guess; fieldLr defaults to the network's learning rate; fieldBounds = {'diff': ..., 'vel': ...}, each (lo, hi) for
        every learnt amplitude of that basis or a list with one entry per function, each None or (lo, hi), None for an open side."""
        return VarNet._keyed_learn_data(VarNet._FIELD, PDE, learnField, fieldLr, fieldBounds, learning_rate)

    def _field_basis(self, Input, grad=False):
        """(chi [Jk, n, 1], grad chi [Jk, n, dim] or None without `grad`, omega [Jv, n, dim]) of the PDE's field bases at the rows
        of Input, fp64."""
        dim, PDE = self.dim, self.PDE
        targ = [Input[:, dim][np.newaxis].T] if PDE.timeDependent else []
        X = Input[:, 0:dim]
        val = PDE.field_basis_values
        return (val(getattr(PDE, 'diffBasis', None) or [], 'diffBasis', 1, X, targ),
                val(getattr(PDE, 'd_diffBasis', None) or [], 'd_diffBasis', dim, X, targ) if grad else None,
                val(getattr(PDE, 'velBasis', None) or [], 'velBasis', dim, X, targ))

    def fieldAmplitudes(self):
        """{'diff': J_kappa amplitudes, 'vel': J_v amplitudes} of the PDE's field bases at the current state: the learnt values
        with learnField, else the PDE's."""
        return self._keyed_amplitudes(self._FIELD)

    def fieldGrad(self):
        """d loss / d amplitude of the last gradient evaluation as {'diff': ..., 'vel': ...} (zeros where not learnt)."""
        return self._keyed_grad(self._FIELD)

    def setFieldAmplitudes(self, amps):
        """Overwrite amplitudes between train() calls: {'diff': [...], 'vel': [...]} (a key left out keeps its values).  Not
        clamped to fieldBounds (the next update is)."""
        self._keyed_set(self._FIELD, amps)

    # -- boundary data identification: learnt amplitudes of a Dirichlet and an initial basis (extension) -----
    @staticmethod
    def bicLearnData(PDE, learnBic, bicLr=None, bicBounds=None, learning_rate=0.001):
        """(No reference counterpart: `VarNet(..., learnBic=...)`.)  The registration of `vn_set_bic_learn`, or None without
        learnBic: mask, init, lo, hi (J = J_bc + J_ic entries each, the Dirichlet streams first), lr, Jb and Ji.  learnBic =
        {'bc': True | mask, 'ic': True | mask} (a key left out: none of that basis is learnt); the PDE's bcAmp / icAmp are the
        initial guess; bicLr defaults to the network's learning rate; bicBounds = {'bc': ..., 'ic': ...}, each (lo, hi) for
        every learnt amplitude of that basis or a list with one entry per function, each None or (lo, hi), None for an open side."""
        return VarNet._keyed_learn_data(VarNet._BIC, PDE, learnBic, bicLr, bicBounds, learning_rate)

    def _bic_basis(self, biInput, biDof):
        """The PDE's Dirichlet and initial basis functions at the BC/IC rows, [J_bc + J_ic, nB] in fp64 (the Dirichlet streams
        first): a gamma_j evaluated like `g` on the rows of its own indicator and zero elsewhere, an iota_j evaluated like `IC`
        on the initial rows and zero on the boundary rows."""
        dim, PDE = self.dim, self.PDE
        nB = biInput.shape[0]
        span, indp = {}, 0
        # the rows of each Dirichlet indicator, as biTrainData walks them (with time, biDof ends in the initial rows' count)
        for bInd, n in zip([b for b in range(PDE.domain.bIndNum) if PDE.BCtype[b] == 'Dirichlet'], biDof):
            span[bInd] = (indp, indp + n)
            indp += n
        Jb, Ji = self._keyed_sizes(self._BIC, PDE)
        B = np.zeros((Jb + Ji, nB), dtype=np.float64)
        B[:Jb] = self._edge_basis(biInput, span, ('bcBasis',))
        for j, f in enumerate(getattr(PDE, 'icBasis', None) or []):
            v = np.asarray(f(biInput[indp:, :dim]), dtype=np.float64)
            if v.size != nB - indp:
                raise ValueError('icBasis[%d] must return one value per point (a column), got shape %s for %d points'
                                 % (j, v.shape, nB - indp))
            B[Jb + j, indp:] = v.reshape(-1)
        return B

    def bicAmplitudes(self):
        """{'bc': J_bc amplitudes, 'ic': J_ic amplitudes} of the PDE's Dirichlet and initial bases at the current state: the
        learnt values with learnBic, else the PDE's."""
        return self._keyed_amplitudes(self._BIC)

    def bicGrad(self):
        """d loss / d amplitude of the last gradient evaluation as {'bc': ..., 'ic': ...} (zeros where not learnt)."""
        return self._keyed_grad(self._BIC)

    def setBicAmplitudes(self, amps):
        """Overwrite amplitudes between train() calls: {'bc': [...], 'ic': [...]} (a key left out keeps its values).  Not
        clamped to bicBounds (the next update is)."""
        self._keyed_set(self._BIC, amps)

    # -- flux boundary identification: learnt amplitudes of a flux-datum and a Robin-coefficient basis (extension) -----
    @staticmethod
    def fluxBCLearnData(PDE, learnFluxBC, fluxBCLr=None, fluxBCBounds=None, learning_rate=0.001):
        """(No reference counterpart: `VarNet(..., learnFluxBC=...)`.)  The registration of `vn_set_fluxbc_learn`, or None without
        learnFluxBC: mask, init, lo, hi (J = J_flux + J_robin entries each, the flux-datum streams first), lr, Jl and Jc.
        learnFluxBC = {'flux': True | mask, 'robin': True | mask} (a key left out: none of that basis is learnt); the PDE's fluxAmp /
        robinAmp are the initial guess; fluxBCLr defaults to the network's learning rate; fluxBCBounds = {'flux': ..., 'robin':
        ...}, each (lo, hi) for every learnt amplitude of that basis or a list with one entry per function, each None or (lo, hi),
        None for an open side."""
        return VarNet._keyed_learn_data(VarNet._FBC, PDE, learnFluxBC, fluxBCLr, fluxBCBounds, learning_rate)

    def fluxBCAmplitudes(self):
        """{'flux': J_flux amplitudes, 'robin': J_robin amplitudes} of the PDE's flux-datum and Robin-coefficient bases at the
        current state: the learnt values with learnFluxBC, else the PDE's."""
        return self._keyed_amplitudes(self._FBC)

    def fluxBCGrad(self):
        """d loss / d amplitude of the last gradient evaluation as {'flux': ..., 'robin': ...} (zeros where not learnt)."""
        return self._keyed_grad(self._FBC)

    def setFluxBCAmplitudes(self, amps):
        """Overwrite amplitudes between train() calls: {'flux': [...], 'robin': [...]} (a key left out keeps its values).  Not
        clamped to fluxBCBounds (the next update is)."""
        self._keyed_set(self._FBC, amps)

    # -- regularisation of the learnt vectors: quadratic prior and L1 shrinkage (extension) ---------------------
    PRIOR_KEYS = ('weight', 'matrix', 'mean', 'l1')

    @staticmethod
    def priorMatrix(kind, n):
        """The named matrices of a prior block of n amplitudes: 'identity', or 'difference' = D^T D of the first differences
        (D a)_i = a_{i+1} - a_i in amplitude order (zero on constants; the 1 x 1 block is 0)."""
        if kind == 'identity':
            return np.eye(n)
        if kind == 'difference':
            D = np.diff(np.eye(n), axis=0)
            return D.T @ D
        raise ValueError('learntPrior: matrix must be \'identity\', \'difference\' or a symmetric positive semi-definite array, got %r' % (kind,))

    @staticmethod
    def _prior_block(where, spec, init):
        """One block of a prior from its spec, for the amplitudes whose starting values are `init`: dict(weight, R [n, n], mean [n],
        l1 [n]); every refusal names `where`."""
        n = len(init)
        if not isinstance(spec, dict) or any(k not in VarNet.PRIOR_KEYS for k in spec):
            raise ValueError('%s must be a dict with keys among %s, got %r' % (where, ', '.join(VarNet.PRIOR_KEYS), spec))

        def number(x):
            return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)
        w = spec.get('weight', 0.0)
        if not number(w) or not np.isfinite(w):
            raise ValueError('%s: weight must be a finite number, got %r' % (where, w))
        if w < 0:
            raise ValueError('%s: weight %r is negative (the prior 1/2 weight d^T R d must be bounded below)' % (where, w))
        m = spec.get('matrix', 'identity')
        if isinstance(m, str):
            R = VarNet.priorMatrix(m, n)
        else:
            try:
                R = np.array(m, dtype=np.float64)
            except (TypeError, ValueError):
                R = np.empty(0)
            if R.shape != (n, n) or not np.all(np.isfinite(R)):
                raise ValueError('%s: matrix must be %d x %d finite numbers (one row per amplitude), got shape %s' % (where, n, n, R.shape))
            big = float(np.max(np.abs(R))) if n else 0.0
            if np.max(np.abs(R - R.T), initial=0.0) > 1e-12 * big:
                i, j = np.unravel_index(np.argmax(np.abs(R - R.T)), R.shape)
                raise ValueError('%s: matrix is not symmetric (entry (%d, %d) = %r, entry (%d, %d) = %r)' % (where, i, j, R[i, j], j, i, R[j, i]))
            R = 0.5 * (R + R.T)                           # (the engine takes exact symmetry only)
            ev = np.linalg.eigvalsh(R)
            if ev[0] < -1e-10 * max(ev[-1], 0.0) or ev[-1] < 0.0:
                raise ValueError('%s: matrix is indefinite (smallest eigenvalue %r, largest %r): the prior would be unbounded below'
                                 % (where, float(ev[0]), float(ev[-1])))

        def vector(key, default, scalar_ok):
            v = spec.get(key)
            if v is None:
                return default
            try:
                v = np.asarray(v, dtype=np.float64)
            except (TypeError, ValueError):
                v = np.empty((0, 0))
            if scalar_ok and v.ndim == 0:
                v = np.full(n, float(v))
            if v.shape != (n,) or not np.all(np.isfinite(v)):
                raise ValueError('%s: %s must be %s%d finite numbers (one per amplitude), got %r' % (where, key, 'a number or ' if scalar_ok else '', n, spec.get(key)))
            return v.copy()
        mean = vector('mean', np.asarray(init, dtype=np.float64).copy(), False)
        l1 = vector('l1', np.zeros(n), True)
        if np.any(l1 < 0):
            raise ValueError('%s: l1 weight %r is negative' % (where, float(l1.min())))
        return dict(weight=float(w), R=R, mean=mean, l1=l1)

    @staticmethod
    def priorData(PDE, learntPrior, learnt):
        """(No reference counterpart: `VarNet(..., learntPrior={stem: spec})`.)  The parsed priors, {stem: {'blocks': {key: block}}}
        with a block = dict(weight, R, mean, l1) of `_prior_block`; `learnt`: {stem: the parsed registration of that vector, or
        None}.  Stems: coef, source, field, bic, fluxBC.  A spec is a dict with the keys weight (alpha >= 0, default 0), matrix
        ('identity', the default; 'difference'; or a symmetric positive semi-definite array), mean (default: the starting values)
        and l1 (a number or one per entry, >= 0).  For the keyed vectors (field, bic, fluxBC) the spec is a dict by key -- {'diff':
        spec, 'vel': spec} and so on -- each block built on its own and placed on the diagonal; a key left out gets a zero
        block.  The unkeyed vectors have the one block None."""
        if learntPrior is None:
            return {}
        stems = [lv.stem for lv in VarNet.LEARNT]
        if not isinstance(learntPrior, dict):
            raise ValueError('learntPrior must be a dict {stem: spec} with stems among %s, got %r' % (', '.join(stems), learntPrior))
        out = {}
        for stem, spec in learntPrior.items():
            if stem not in stems:
                raise ValueError('learntPrior: unknown stem %r (one of %s)' % (stem, ', '.join(stems)))
            lv = VarNet.LEARNT[stems.index(stem)]
            data = learnt.get(stem)
            if data is None:
                raise ValueError('learntPrior[%r]: this instance does not learn that vector (%s=...)' % (stem, lv.option))
            init = np.asarray(data['init'], dtype=np.float64)
            if lv.keyed is None:
                out[stem] = {'blocks': {None: VarNet._prior_block('learntPrior[%r]' % stem, spec, init)}}
                continue
            keys = lv.keyed.keys
            if not isinstance(spec, dict) or not spec or any(k not in keys for k in spec):
                raise ValueError('learntPrior[%r] must be a dict by key {%r: spec, %r: spec}, got %r' % (stem, keys[0], keys[1], spec))
            blocks, i0 = {}, 0
            for key, n in zip(keys, (data[z] for z in lv.keyed.sizes)):
                if key in spec:
                    if n == 0:
                        raise ValueError('learntPrior[%r][%r]: the PDE has no %s basis (ADPDE(..., %sBasis=[...]))' % (stem, key, key, key))
                    blocks[key] = VarNet._prior_block('learntPrior[%r][%r]' % (stem, key), spec[key], init[i0:i0 + n])
                i0 += n
            out[stem] = {'blocks': blocks}
        return out

    @staticmethod
    def priorArrays(lv, blocks, data):
        """(weight, R or None, mean, l1 or None) the engine takes for the prior of the LEARNT row `lv` with the parsed `blocks` and
        the vector's parsed registration `data`: the one block as it stands (the identity as None), the blocks of a keyed vector
        times their weights on the diagonal under the weight 1."""
        if lv.keyed is None:
            b = blocks[None]
            ident = np.array_equal(b['R'], np.eye(len(b['mean'])))
            return b['weight'], None if ident else b['R'], b['mean'], b['l1'] if np.any(b['l1'] > 0) else None
        sizes = [data[z] for z in lv.keyed.sizes]
        J = sum(sizes)
        R, mean, l1, i0 = np.zeros((J, J)), np.zeros(J), np.zeros(J), 0
        for key, n in zip(lv.keyed.keys, sizes):
            b = blocks.get(key)
            if b is not None:
                R[i0:i0 + n, i0:i0 + n] = b['weight'] * b['R']
                mean[i0:i0 + n], l1[i0:i0 + n] = b['mean'], b['l1']
            i0 += n
        return (1.0 if np.any(R != 0.0) else 0.0), R, mean, l1 if np.any(l1 > 0) else None

    def _register_prior(self, lv):
        w, R, mean, l1 = self.priorArrays(lv, self.learntPrior[lv.stem]['blocks'], getattr(self, lv.attr))
        self.engine.set_learnt_prior(lv.kind, w, None if w == 0.0 else R, None if w == 0.0 else mean, l1)

    def priorPenalty(self):
        """{stem: (Q, l1)} of every vector with a prior at the current values: Q = 1/2 weight d^T R d and l1 = sum_j lambda_j |a_j|.
        Neither is part of the losses train() reports."""
        return {lv.stem: self.engine.learnt_prior(lv.kind) for lv in self.LEARNT if lv.stem in self.learntPrior}

    def setPriorWeight(self, stem, weight=None, l1=None):
        """New weights for the prior of `stem` between train() calls (the Adam slots and the values stay): weight and l1 as in
        learntPrior, None keeps what is registered; for a keyed vector each a number for every registered key or a dict by key."""
        if stem not in self.learntPrior:
            raise ValueError('setPriorWeight: no prior on %r (VarNet(learntPrior={%r: ...}))' % (stem, stem))
        lv = next(v for v in self.LEARNT if v.stem == stem)
        blocks = self.learntPrior[stem]['blocks']
        for name, new in (('weight', weight), ('l1', l1)):
            if new is None:
                continue
            per_key = isinstance(new, dict) and lv.keyed is not None
            if per_key and any(k not in blocks for k in new):
                raise ValueError('setPriorWeight: %s names a key without a prior block (registered: %s)' % (name, ', '.join(blocks)))
            for key, b in blocks.items():
                if per_key and key not in new:
                    continue
                where = 'setPriorWeight(%r)' % stem if key is None else 'setPriorWeight(%r)[%r]' % (stem, key)
                b.update({k: v for k, v in self._prior_block(where, {name: new[key] if per_key else new, 'matrix': b['R'], 'mean': b['mean']},
                                                             b['mean']).items() if k == name})
        self._register_prior(lv)

    # -- self-adaptive test-function weights (extension) --------------------------------------------
    @staticmethod
    def _check_tf_adapt(spec, causal, lbfgs, mor, towers):
        """The full dict of a `tfAdapt` option (None: off), after the refusals every way in shares."""
        from .engine import tf_adapt_spec
        full = tf_adapt_spec(spec)
        if full is None:
            return None
        if causal:
            raise ValueError('tfAdapt=%r with causal=...: a batch carries one per-test-function registration, and the two replace '
                             'each other' % (spec,))
        if lbfgs:
            raise ValueError('tfAdapt=%r with optimizer=\'lbfgs\': the weights move from step to step but are held constant for the '
                             'gradient, so an Armijo test across steps means nothing' % (spec,))
        if mor:
            raise NotImplementedError('tfAdapt=%r with model-order reduction is not supported: every MOR batch is another objective '
                                      'with a state of its own, which the monitors and checkpoints do not carry' % (spec,))
        if towers:
            raise NotImplementedError('tfAdapt=%r with towers: a rank\'s max, mean and Z would cover only its shard of the test '
                                      'functions, so the ranks together would train another objective than one rank' % (spec,))
        return full

    def setTfAdapt(self, spec):
        """Another rule or other parameters for the self-adaptive weights (None switches them off), re-registered on the training
        set of the last train() call from the rule's initial state: the option can change between train() calls."""
        full = self._check_tf_adapt(spec, self.causal is not None, self._is_lbfgs(), not uf.isnone(self.PDE.MORvar),
                                    self.world > 1 or self._towers is not None)
        if full is not None:
            for lv in self.LEARNT:
                if getattr(self, lv.attr, None) is not None:
                    raise NotImplementedError('%s with tfAdapt=%r: the weights are applied after the seeds the %s gradient is '
                                              'reduced from' % (lv.option, spec, lv.noun))
        self.tfAdapt = full
        self._adapt_owner = None                          # no state is carried over to the new registration
        tData = getattr(self, 'tData', None)
        if tData is not None:
            tData._adapt_saved = None
            tData.activate()

    def tfWeights(self, tData=None):
        """Per batch of `tData` (default: the set of the last train() call, else a freshly built full-batch set) the committed
        state {'omega', 'lambda' [n_k], 'stats': {'min', 'max', 'mean', 'share', 'Z', 'tau'}} of the self-adaptive weights."""
        if self.tfAdapt is None:
            raise ValueError('tfWeights: the self-adaptive weights are off (VarNet(tfAdapt=...) or setTfAdapt(...))')
        if tData is None:
            tData = getattr(self, 'tData', None) or self._build_tdata()
        if getattr(self, '_adapt_owner', None) is not tData:
            tData.activate()
        out = []
        for bi in range(tData.batchNum):
            s = self.engine.tf_adapt(tData.engine_batch(0, bi))
            out.append({'omega': s['omega'], 'lambda': s['lambda'], 'stats': s['stats']})
        return out

    # -- weights on the boundary and initial rows (extension) ----------------------------------------
    BIC_PARTS = ('bc', 'ic')

    @classmethod
    def _check_bic_weights(cls, weights, adapt, lbfgs, mor, towers, ansatz, timeDependent):
        """(bicWeights, bicAdapt) as dicts by part (None: off), after the refusals every way in shares.  bicWeights: an array
        [nB] (stored under 'rows') or {'bc': array | callable(x[, t]), 'ic': ..., 'normalize': bool}; bicAdapt: 'rba' | 'sa' (the
        'ic' part of a time-dependent problem, else 'bc') or {'bc': spec, 'ic': spec}."""
        from .engine import tf_adapt_spec
        if weights is None and adapt is None:
            return None, None
        w = None
        if weights is not None:
            if isinstance(weights, dict):
                bad = [k for k in weights if k not in cls.BIC_PARTS + ('normalize',)]
                if bad or not any(k in weights for k in cls.BIC_PARTS):
                    raise ValueError("bicWeights: a dict takes the keys 'bc', 'ic' and 'normalize' (got %r)" % (sorted(weights),))
                w = dict(weights)
            else:
                w = {'rows': np.asarray(weights, dtype=np.float64).reshape(-1)}
            w['normalize'] = bool(w.get('normalize', False))
            for k in cls.BIC_PARTS + ('rows',):
                if k in w and not callable(w[k]):
                    w[k] = np.asarray(w[k], dtype=np.float64).reshape(-1)
                    if not (np.all(np.isfinite(w[k])) and np.all(w[k] >= 0.0)):
                        raise ValueError('bicWeights: every weight must be finite and >= 0 (%r)' % (k,))
        a = None
        if adapt is not None:
            if isinstance(adapt, dict) and 'rule' not in adapt:
                bad = [k for k in adapt if k not in cls.BIC_PARTS]
                if bad or not adapt:
                    raise ValueError("bicAdapt: a dict by part takes the keys 'bc' and 'ic' (got %r)" % (sorted(adapt),))
                a = {k: tf_adapt_spec(v) for k, v in adapt.items() if v is not None}
            else:
                a = {'ic' if timeDependent else 'bc': tf_adapt_spec(adapt)}
            if 'ic' in a and not timeDependent:
                raise ValueError("bicAdapt: a steady problem has no initial rows, so no 'ic' part")
            if not a:
                a = None
        if w is not None and not timeDependent and 'ic' in w:
            raise ValueError("bicWeights: a steady problem has no initial rows, so no 'ic' part")
        if w is not None and a is not None:
            both = [k for k in a if k in w or 'rows' in w]
            if both and 'rows' not in w:
                raise ValueError('bicWeights and bicAdapt both name the %r part: a static and an adaptive registration of a part '
                                 'replace each other' % (both[0],))
        if a is not None and lbfgs:
            raise ValueError('bicAdapt=%r with optimizer=\'lbfgs\': the weights move from step to step but are held constant for the '
                             'gradient, so an Armijo test across steps means nothing; static bicWeights= work' % (adapt,))
        if mor:
            raise NotImplementedError('bicWeights= / bicAdapt= with model-order reduction is not supported: every MOR batch has rows '
                                      'and labels of its own, and the engine keeps one state per row of one set')
        if towers:
            raise NotImplementedError('bicWeights= / bicAdapt= with towers: a rank\'s max, mean and Z would follow its own shard\'s '
                                      'steps, so the ranks together would train another objective than one rank')
        if ansatz:
            raise NotImplementedError('bicWeights= / bicAdapt= with a hard-constraint ansatz: the rows\' error is zero by '
                                      'construction, there is nothing to weight')
        return w, a

    def _bic_weights_save(self):
        """Before a vn_set_bic: the adaptive state of the set that holds the rows' weights is kept on the host."""
        owner = getattr(self, '_bicw_owner', None)
        if owner is None or (self.bicAdapt is None and self.bicWeights is None):
            return
        parts = self.engine.bic_parts()
        owner._bicw_saved = _adapt_arrays({p + '_': self.engine.bic_adapt(p) for p, v in parts.items() if isinstance(v, dict)})
        self._bicw_owner = None

    def _bic_static_rows(self, X, nbc):
        """bicWeights= evaluated on the rows X [nB, dim (+1)] of a training set: one weight per row."""
        w = self.bicWeights
        if 'rows' in w:
            if w['rows'].size != X.shape[0]:
                raise ValueError('bicWeights: expected one weight per boundary / initial row (%d), got %d' % (X.shape[0], w['rows'].size))
            return w['rows']
        out = np.ones(X.shape[0])
        for part, sl in (('bc', slice(0, nbc)), ('ic', slice(nbc, None))):
            v = w.get(part)
            if v is None:
                continue
            if callable(v):
                Xp = X[sl]
                args = (Xp[:, :self.dim], Xp[:, self.dim:self.dim + 1]) if self.PDE.timeDependent else (Xp[:, :self.dim],)
                try:
                    v = v(*args)
                except TypeError:
                    v = v(args[0])
                v = np.broadcast_to(np.asarray(v, dtype=np.float64).reshape(-1), (Xp.shape[0],)) if np.size(v) == 1 \
                    else np.asarray(v, dtype=np.float64).reshape(-1)
            if v.size != out[sl].size:
                raise ValueError('bicWeights[%r]: expected %d weights, got %d' % (part, out[sl].size, v.size))
            if not (np.all(np.isfinite(v)) and np.all(v >= 0.0)):
                raise ValueError('bicWeights[%r]: every weight must be finite and >= 0' % (part,))
            out[sl] = v
        return out

    def _bic_weights_register(self, tData, d):
        """After a vn_set_bic of tData's rows: the static weights, then the adaptive parts (which replace a static registration of
        their part), then the state this set kept while another one used the engine."""
        if self.bicWeights is None and self.bicAdapt is None:
            return
        eng = self.engine
        if self.bicWeights is not None:
            X = d['biInput']
            X = np.asarray(X.cpu() if hasattr(X, 'cpu') else X, dtype=np.float64)
            nbc = int(tData.bDofsum)
            om = self._bic_static_rows(X, nbc)
            if not self.PDE.timeDependent:
                om = om[:nbc]
            eng.set_bic_weights(om.astype(np.float32), normalize=self.bicWeights['normalize'])
        for part, spec in (self.bicAdapt or {}).items():
            if eng.bic_rows(part) <= 0:
                continue
            eng.set_bic_adapt(part, spec)
            _adapt_put_back(getattr(tData, '_bicw_saved', None), part + '_', eng.set_bic_adapt_state, part, eng.bic_rows(part))
        self._bicw_owner = tData

    def setBicAdapt(self, bicAdapt=None, bicWeights=None):
        """Other rules, parameters or static weights for the boundary and initial rows (both None switches them off),
        re-registered on the training set of the last train() call from the initial state: the options can change between
        train() calls."""
        w, a = self._check_bic_weights(bicWeights, bicAdapt, self._is_lbfgs(), not uf.isnone(self.PDE.MORvar),
                                       self.world > 1 or self._towers is not None, getattr(self.PDE, 'ansatz', None) is not None,
                                       self.PDE.timeDependent)
        if w is not None or a is not None:
            for lv in self.LEARNT:
                if getattr(self, lv.attr, None) is not None:
                    raise NotImplementedError('%s with bicWeights= / bicAdapt=: the %s sums next to the rows\' own pass are not built'
                                              % (lv.option, lv.noun))
        self.bicWeights, self.bicAdapt = w, a
        self._bicw_owner = None                           # no state is carried over to the new registration
        tData = getattr(self, 'tData', None)
        if tData is not None:
            tData._bicw_saved = None
            self.engine._bic_key = None                   # the rows are registered again, and the weights with them
            tData.select_mor(0)

    def bicRowWeights(self, tData=None):
        """Per registered part ('bc', 'ic') of the training set of the last train() call (default; else `tData`, else a freshly
        built full-batch set): {'x': the rows' coordinates [n_s, dim (+1)], 'omega', 'lambda', 'l': the unweighted e_i^2 of the
        last evaluation, 'stats'}.  A read-back of the set that holds the engine's rows (after train(): the training set).  Asked for
        another set, it first registers that set's rows with the engine (a vn_set_bic: the holder keeps its adaptive state on the
        host and takes it back at its next registration), as every monitor on another set does."""
        if self.bicWeights is None and self.bicAdapt is None:
            raise ValueError('bicRowWeights: the rows carry no weights (VarNet(bicWeights=..., bicAdapt=...) or setBicAdapt(...))')
        if tData is None:
            tData = getattr(self, 'tData', None) or self._build_tdata()
        if getattr(self, '_bicw_owner', None) is not tData:
            self.engine._bic_key = None
            tData.select_mor(0)
        X = tData.mor[0]['biInput']
        X = np.asarray(X.cpu() if hasattr(X, 'cpu') else X)
        nbc = int(tData.bDofsum)
        out = {}
        for part in self.engine.bic_parts():
            s = self.engine.bic_adapt(part)
            rows = X[:nbc] if part == 'bc' else X[nbc:]
            out[part] = {'x': rows, 'omega': s['omega'], 'lambda': s['lambda'], 'l': s['lossfield'], 'stats': s['stats']}
        return out

    # -- causal time-slab weights (extension) ------------------------------------------------------
    @staticmethod
    def _check_causal_eps(eps):
        if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)) or not np.isfinite(eps) or eps < 0:
            raise ValueError('causal must be a finite float >= 0 (the eps of exp(-eps * accumulated loss)), got %r' % (eps,))

    def causalSlabNum(self):
        """S: the number of time slabs of the causal mode (causalSlabs, default tDiscNum)."""
        return int(self.causalSlabs or self.tDiscNum)

    def causalSlabIds(self, Input):
        """Slab id of every test function of the rows `Input` [nt*integNum, >= dim+1]: a test function centred at t_k (the mean
        time of its quadrature points) lies in slab clip(floor((t_k - t0 - h/2) / h), 0, S-1), h = (T - t0) / S.  On the uniform
        set with S = tDiscNum that is k % tDiscNum; it also serves residual-driven sets and `frac`-thinned grids."""
        q, S = self.fixData.integNum, self.causalSlabNum()
        t0, T = [float(x) for x in self.PDE.tInterval]
        h = (T - t0) / S
        tk = np.asarray(Input, dtype=np.float64)[:, self.dim].reshape(-1, q).mean(axis=1)
        # (half a slab below the node, and a relative 1e-9 above the rounding of t_k: nodes sit at slab ends)
        return np.clip(np.floor((tk - t0 - 0.5 * h) / h + 1e-9), 0, S - 1).astype(np.int32)

    def setCausal(self, eps):
        """A new eps for the causal mode (None switches it off), re-registered on the training set of the last train() call:
        eps can be annealed between train() calls."""
        if eps is not None:
            self._check_causal_eps(eps)
            if getattr(self, 'tfAdapt', None) is not None:
                raise ValueError('causal=%r with tfAdapt=...: a batch carries one per-test-function registration, and the two '
                                 'replace each other' % (eps,))
            if not self.PDE.timeDependent:
                raise ValueError('causal=%r needs a time-dependent PDE: a steady problem has no time slabs' % (eps,))
            if self._is_lbfgs():
                raise ValueError('causal=%r with optimizer=\'lbfgs\': the search direction would not be the gradient of the '
                                 'reported loss' % (eps,))
            if self.world > 1 or self._towers is not None:
                raise NotImplementedError('causal=%r with towers: a rank\'s slab means would cover only its shard' % (eps,))
        self.causal = None if eps is None else float(eps)
        tData = getattr(self, 'tData', None)
        if tData is not None:
            if self.causal is not None:
                for d in tData.mor:                   # a set assembled while the mode was off has no ids yet
                    if d.get('slab') is None:
                        d['slab'] = self._slab_tensor(d['Input_host'])
            tData.activate()

    def _slab_tensor(self, Input):
        torch = self.engine.torch
        return torch.as_tensor(self.causalSlabIds(Input), dtype=torch.int32, device=self.engine.device)

    def causalWeights(self, tData=None):
        """omega_s [S] of block 0 of `tData` (default: the set of the last train() call, else a freshly built full-batch set) at
        the current parameters: min omega -> 1 as the early slabs converge and release the late ones."""
        if self.causal is None:
            raise ValueError('causalWeights: the causal mode is off (VarNet(causal=eps) or setCausal(eps))')
        if tData is None:
            tData = getattr(self, 'tData', None) or self._build_tdata()
        tData.select_mor(0)
        return self.engine.causal_weights(tData.engine_batch(0, 0))

    # -- discretisation ----------------------------------------------------------------------
    def timeDisc(self, tdof=None, rfrac=0, sortflg=True, discTol=None):
        """t nodes linspace(t0+ht, T, tdof), ht=(T-t0)/tdof (VarNet.py:297-338)."""
        PDE = self.PDE
        if not PDE.timeDependent:
            raise Exception('The problem is time-independent!')
        rfrac = min(max(rfrac, 0), 1)
        if tdof is None:
            tdof = self.tDiscNum
        tlim = PDE.tInterval
        ht = (tlim[1] - tlim[0]) / tdof
        tol = ht if discTol is None else float(np.reshape(discTol, -1)[0])
        dof1 = math.floor(tdof * rfrac)
        t1 = np.random.uniform(tlim[0] + tol, tlim[1], dof1)
        t2 = np.linspace(tlim[0] + tol, tlim[1], tdof - dof1)
        t = np.hstack([t1, t2]) if dof1 else t2
        if rfrac > 0 and sortflg:
            t = np.sort(t)
        return ht, np.reshape(t, [tdof, 1])

    def trainingPoints(self, smpScheme='uniform', frac=0.5, addTrainPts=True, suppFactor=1.0):
        """
        Quadrature-point coordinates of every test function (VarNet.py:504-600):
        Input[k*integNum+p, d] = x_k[d] + he[d]*delta[d,p],  Input[., dim] = t_k + ht*delta[-1,p];
        test functions ordered space-major, time-minor.
        """
        if smpScheme == 'optimal':
            return self.optTrainPoints(frac, addTrainPts, suppFactor)
        rfrac = frac if smpScheme == 'random' else 0.
        dim, PDE, fd = self.dim, self.PDE, self.fixData
        domain = PDE.domain
        dof, nt, nT, delta = fd.dof, fd.nt, fd.nT, fd.delta
        if PDE.timeDependent:
            tDiscNum = self.tDiscNum
            ht, t_coord = self.timeDisc(rfrac=rfrac)
        else:
            tDiscNum, t_coord = 1, []
        mesh = domain.getMesh(self.discNum, self.bDiscNum, rfrac=rfrac)
        if smpScheme == 'random' and mesh.dof < dof:
            coord = mesh.coordinates
            while coord.shape[0] < dof:
                coord = uf.vstack([coord, domain.getMesh(self.discNum, self.bDiscNum, rfrac=1.).coordinates])
            mesh.dof, mesh.coordinates = dof, coord[:dof, :]
        he = np.reshape(mesh.he, -1)
        coord = mesh.coordinates
        Coord = np.empty([nT, dim])
        for d in range(dim):
            c = np.repeat(coord[:, d], tDiscNum).reshape(nt, 1) + he[d] * delta[d, :]
            Coord[:, d] = c.reshape(nT)
        if PDE.timeDependent:
            tC = np.tile(t_coord, [dof, 1]) + ht * delta[-1, :]
            Input = np.concatenate([Coord, tC.reshape(nT, 1)], axis=1)
        else:
            Input = Coord
        biInput, biDof = self.biTrainPoints(mesh, t_coord)
        return Input, [], biInput, biDof

    def optTrainPoints(self, frac=0.25, addTrainPts=True, suppFactor=1.0):
        """
        Residual-driven ("optimal") training points (VarNet.py:1696-1868): keep (or thin) the uniform
        test functions and draw the others by rejection sampling with acceptance probability
        |PDE residual| / max|residual on the uniform grid|; optionally shrink the support of the
        added ones by `suppFactor`.  The residual field comes from the device (`vn_residual`).
        """
        dim, PDE, fd = self.dim, self.PDE, self.fixData
        td, domain = PDE.timeDependent, PDE.domain
        feDim, integNum, nt, nT, hVec, delta = fd.feDim, fd.integNum, fd.nt0, fd.nT, fd.hVec, fd.delta
        frac2 = 1 if addTrainPts else (1 - frac) ** (1 / feDim)
        if td:
            tDiscNum2 = math.ceil(frac2 * self.tDiscNum)
            _, t_coord = self.timeDisc(tDiscNum2)
        else:
            tDiscNum2, t_coord = 1, []
        discNum2 = [math.ceil(frac2 * d) for d in self.discNum]
        mesh = domain.getMesh(discNum2, self.bDiscNum)
        input2 = uf.pairMats(mesh.coordinates, t_coord)
        nt1 = math.ceil(frac * nt) if addTrainPts else nt - mesh.dof * tDiscNum2
        scaled = np.abs(suppFactor - 1.0) > 1.e-15
        tole = suppFactor * hVec[:dim] if scaled else None
        tolt = suppFactor * hVec[-1] if (scaled and td) else None

        def resfun(inpuT=None):
            _, resVec, _, _ = self.residual(inpuT)
            return np.abs(resVec)

        def smpfun():
            tc = self.timeDisc(rfrac=1, sortflg=False, discTol=tolt)[1] if td else []
            m = domain.getMesh(self.discNum, self.bDiscNum, rfrac=1, sortflg=False, discTol=tole)
            return uf.pairMats(m.coordinates, tc)

        input1 = uf.rejectionSampling(resfun, smpfun, nt1)
        if addTrainPts:
            nt = nt1 + nt
            nT = nt * integNum
        inpuT = np.vstack([input1, input2])
        coord = inpuT[:, :dim]
        if td and not scaled:                                        # sort by time only for equal supports
            t_coord = inpuT[:, dim:dim + 1]
            ind = np.reshape(np.argsort(t_coord, axis=0), nt)
            coord, t_coord = coord[ind], t_coord[ind]
        elif td:
            t_coord = inpuT[:, dim:dim + 1]
        biInput, biDof, _, _ = self.optBiTrainPoints(frac, addTrainPts)

        he = np.reshape(hVec[:dim], -1)
        suppScale = 1.0
        if scaled:
            suppScale = np.ones([nt, 1])
            suppScale[:nt1, :] = suppFactor
        Coord = np.empty([nT, dim])
        for d in range(dim):
            Coord[:, d] = (np.reshape(coord[:, d], [nt, 1]) + he[d] * delta[d, :] * suppScale).reshape(nT)
        if td:
            tC = t_coord + float(np.reshape(hVec[-1], -1)[0]) * delta[-1, :] * suppScale
            Input = np.concatenate([Coord, tC.reshape(nT, 1)], axis=1)
        else:
            Input = Coord
        if addTrainPts:
            fd.updateOptimData(frac, suppFactor)
        return Input, [], biInput, biDof

    def optBiTrainPoints(self, frac=0.25, addTrainPts=True):
        """Optimal boundary / initial points (VarNet.py:1872-1966): rejection sampling per
        Dirichlet edge and for the initial slice with density (model - label)^2."""
        dim, PDE, fd = self.dim, self.PDE, self.fixData
        td, domain = PDE.timeDependent, PDE.domain
        biDof = fd.biDof0
        frac2 = 1 if addTrainPts else (1 - frac) ** (1 / (fd.feDim - 1))
        t_coord = self.timeDisc(math.ceil(frac2 * self.tDiscNum))[1] if td else []
        discNum2 = [math.ceil(frac2 * d) for d in self.discNum]
        bDisc = self.bDiscNum
        bDisc2 = math.ceil(frac2 * bDisc) if isinstance(bDisc, (int, float)) else bDisc
        mesh = domain.getMesh(discNum2, bDisc2)
        biInput2, biDof2 = self.biTrainPoints(mesh, t_coord)
        if addTrainPts:
            biDof1 = [math.ceil(frac * b) for b in biDof]
        else:
            biDof1 = list(np.array(biDof) - np.array(biDof2))

        def resfun(biInpuT=None):
            if biInpuT is None:
                biInpuT = fd.uniform_biInput
            val = self._model_on(biInpuT)
            return (val - self.biTrainData(biInpuT, biDof)) ** 2

        def smpfun():
            tc = self.timeDisc(rfrac=1, sortflg=False)[1] if td else []
            m = domain.getMesh(self.discNum, self.bDiscNum, rfrac=1, sortflg=False)
            return self.biTrainPoints(m, tc)[0]

        biInput1 = uf.rejectionSampling(resfun, smpfun, biDof1, biDof)
        biDofNew = list(np.array(biDof1) + np.array(biDof2)) if addTrainPts else list(biDof)
        seg1 = uf.listSegment(biInput1, biDof1)
        seg2 = uf.listSegment(biInput2, biDof2)
        out = []
        for i in range(len(biDof1)):
            b = uf.vstack([seg1[i], seg2[i]])
            if td:
                ind = np.reshape(np.argsort(b[:, dim:dim + 1], axis=0), biDofNew[i])
                b = b[ind]
            out.append(b)
        return uf.vstack(out), [int(v) for v in biDofNew], biInput1, biInput2

    def _model_on(self, Input):
        """model(Input) for space-time rows without MOR columns (VarNet.py:1930) -> [n,1]."""
        return self.engine.forward(Input).cpu().numpy().astype(np.float64).reshape(-1, 1)

    def biTrainPoints(self, mesh, t_coord):
        """Dirichlet-edge x time points, then IC points [x,0] (VarNet.py:604-645)."""
        PDE = self.PDE
        bInput, biDof = [], []
        for bInd in range(PDE.domain.bIndNum):
            if PDE.BCtype[bInd] == 'Dirichlet':
                b = uf.pairMats(mesh.bCoordinates[bInd], t_coord)
                biDof.append(len(b))
                bInput.append(b)
        bInput = uf.vstack(bInput)
        iInput = []
        if PDE.timeDependent:
            iInput = np.concatenate([mesh.coordinates, np.zeros([mesh.dof, 1])], axis=1)
            biDof.append(mesh.dof)
        return uf.vstack([bInput, iInput]), biDof

    def fluxTrainData(self):
        """
        (No reference counterpart: `fluxBC=True`.)  Flux rows of every Neumann / Robin boundary indicator, assembled once on the
        host in fp64: the uniform boundary points `mesh.bCoordinates[bInd]` (paired with the time nodes like the Dirichlet rows),
        the indicator's outward unit normal n, coef = b/a and label = g(x[,t])/a, so that the row's residual is
        n . grad_x u + coef u - label (DESIGN.md "Boundary flux term").  Returns dict(X, normal, coef, label, edges) with
        edges = [(bInd, BCtype, rows)] in indicator order.  With a fluxBasis / robinBasis (ADPDE) also basis = [J_flux + J_robin, nF]
        in fp64, "flux, then robin" -- every function on the rows of its own indicator, zero elsewhere -- and J_flux; the sums at
        the PDE's amplitudes are folded into label and coef here unless the amplitudes are learnt (`learnFluxBC`: the engine mixes
        them, and coef / label stay b/a and g/a).
        """
        PDE, dim = self.PDE, self.dim
        td = PDE.timeDependent
        domain = PDE.domain
        t_coord = self.timeDisc()[1] if td else []
        mesh = domain.getMesh(self.discNum, self.bDiscNum)
        normals = np.asarray(domain.boundaryNormals(), dtype=float)
        X, nrm, coef, label, edges = [], [], [], [], []
        for bInd in range(domain.bIndNum):
            if PDE.BCtype[bInd] in ('Dirichlet', 'Periodic'):
                continue
            a, b, g = PDE.BCs[bInd]
            x = np.asarray(uf.pairMats(mesh.bCoordinates[bInd], t_coord), dtype=float)
            targ = [x[:, dim:dim + 1]] if td else []
            n = x.shape[0]
            X.append(x)
            nrm.append(np.tile(normals[bInd], (n, 1)))
            coef.append(np.full(n, float(b) / float(a)))
            label.append(np.reshape(g(x[:, :dim], *targ), -1).astype(float) / float(a))
            edges.append((bInd, PDE.BCtype[bInd], n))
        if not X:
            return dict(X=np.zeros([0, self.inpDim]), normal=np.zeros([0, dim]), coef=np.zeros(0), label=np.zeros(0), edges=[])
        out = dict(X=np.vstack(X), normal=np.vstack(nrm), coef=np.concatenate(coef), label=np.concatenate(label), edges=edges)
        Jl, Jc = self._keyed_sizes(self._FBC, PDE)
        if Jl + Jc > 0:
            span, i0 = {}, 0
            for bInd, _, n in edges:
                span[bInd] = (i0, i0 + n)
                i0 += n
            S = self._edge_basis(out['X'], span, ('fluxBasis', 'robinBasis'))
            out['basis'], out['J_flux'] = S, Jl
            if getattr(self, 'fbcLearn', None) is None:
                a = self._keyed_vector(self._FBC)
                out['label'] = out['label'] + a[:Jl] @ S[:Jl]
                out['coef'] = out['coef'] + a[Jl:] @ S[Jl:]
                out['basis'] = None
        return out

    @staticmethod
    def _check_obs_weight(lam):
        if not isinstance(lam, (int, float, np.integer, np.floating)) or isinstance(lam, bool) \
                or not np.isfinite(float(lam)) or float(lam) < 0.0:
            raise ValueError('obsWeight=%r must be a finite number >= 0' % (lam,))

    @staticmethod
    def obsData(observations, dim, inpDim):
        """
        (No reference counterpart: `VarNet(..., observations=...)`.)  The observations in the engine's layout, assembled in fp64
        (the engine rounds every array once, to fp32).  `observations` is (X, c) or (X, c, sigma) for point sensors -- X [nO, inpDim]
        with rows [x..., t] as `biInput` has them, c the measured values, sigma their standard deviations (scalar or [nO]) -- or,
        for linear functionals, a dict with X [n, inpDim], value [nO], rowptr [nO + 1] (observation i owns the points
        rowptr[i] .. rowptr[i+1]-1) and optionally q [n] (quadrature weights, default 1), dir [n, dim] (a derivative part
        dir_j . grad_x u(x_j), default none) and sigma.  The functional is l_i = sum_j (q_j u(x_j) + dir_j . grad_x u(x_j)), the
        misfit O = mean_i[(l_i - value_i)^2 / sigma_i^2].  ValueError names the field that is malformed.
        Returns dict(X, value, q, dir, rowptr, wgt) with wgt = 1 / sigma^2 formed in fp64 (None: all 1); q, dir, rowptr None if absent.
        """
        def arr(name, a, shape=None):
            try:
                a = np.array(a, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError('observations: %s must be a numeric array' % name)
            if shape is not None:
                if a.size != int(np.prod(shape)):
                    raise ValueError('observations: %s has %d entries, expected shape %s' % (name, a.size, list(shape)))
                a = a.reshape(shape)
            if not np.all(np.isfinite(a)):
                raise ValueError('observations: %s has non-finite entries' % name)
            return a

        if isinstance(observations, dict):
            unknown = set(observations) - {'X', 'value', 'rowptr', 'q', 'dir', 'sigma'}
            if unknown:
                raise ValueError('observations: unknown field(s) %s' % sorted(unknown))
            for k in ('X', 'value', 'rowptr'):
                if observations.get(k) is None:
                    raise ValueError('observations: the field %s is required (X, value, rowptr; optional q, dir, sigma)' % k)
            X, value, sigma = observations['X'], observations['value'], observations.get('sigma')
            rowptr, q, dirs = observations['rowptr'], observations.get('q'), observations.get('dir')
        elif isinstance(observations, (tuple, list)) and len(observations) in (2, 3):
            X, value = observations[0], observations[1]
            sigma = observations[2] if len(observations) == 3 else None
            rowptr = q = dirs = None
        else:
            raise ValueError('observations must be (X, c), (X, c, sigma) or a dict with X, value, rowptr and optional q, dir, sigma')
        X = arr('X', X)
        if X.ndim == 1 and inpDim == 1:
            X = X.reshape(-1, 1)
        if X.ndim != 2 or X.shape[1] != inpDim or X.shape[0] == 0:
            raise ValueError('observations: X has shape %s, expected [n, %d] with rows [x..., t] and n >= 1' % (list(X.shape), inpDim))
        n = X.shape[0]
        value = arr('value', value).reshape(-1)
        nO = value.shape[0]
        if rowptr is None:
            if nO != n:
                raise ValueError('observations: value has %d entries for %d point sensors' % (nO, n))
        else:
            rp = np.asarray(rowptr)
            if rp.ndim != 1 or rp.shape[0] != nO + 1 or not np.issubdtype(rp.dtype, np.integer):
                raise ValueError('observations: rowptr must hold %d integers (one more than value)' % (nO + 1))
            if nO == 0 or rp[0] != 0 or rp[-1] != n or np.any(np.diff(rp) <= 0):
                raise ValueError('observations: rowptr must increase strictly from 0 to %d (no empty segment)' % n)
            rowptr = rp.astype(np.int32)
        if nO == 0:
            raise ValueError('observations: value is empty')
        if q is not None:
            q = arr('q', q, (n,))
        if dirs is not None:
            dirs = arr('dir', dirs, (n, dim))
        wgt = None
        if sigma is not None:
            sigma = arr('sigma', sigma)
            if sigma.size not in (1, nO):
                raise ValueError('observations: sigma has %d entries, expected 1 or %d' % (sigma.size, nO))
            sigma = np.broadcast_to(sigma.reshape(-1), (nO,)) if sigma.size == 1 else sigma.reshape(nO)
            if np.any(sigma <= 0.0):
                raise ValueError('observations: sigma must be positive')
            with np.errstate(divide='ignore', over='ignore'):
                wgt = 1.0 / (sigma * sigma)
            if not np.all(np.isfinite(wgt)):
                raise ValueError('observations: sigma is too small, 1/sigma^2 overflows')
        return dict(X=X, value=value, q=q, dir=dirs, rowptr=rowptr, wgt=wgt)

    def setObsWeight(self, obsWeight):
        """The weight of the observation misfit, between train() calls: on the scale of `train(weight=[...])`, rescaled by the
        next train() like the value given to the constructor."""
        if self.obsRows is None:
            raise ValueError('setObsWeight: this instance has no observations')
        self._check_obs_weight(obsWeight)
        self.obsWeight = float(obsWeight)
        if self._towers is not None:
            self._towers.call('setObsWeight', obsWeight)
            return
        self.engine.set_obs_weight(self.obsWeight * self._obs_scale / self.world)

    def obsMisfit(self):
        """The unweighted misfit O = mean_i[(l_i(u) - value_i)^2 / sigma_i^2] at the current parameters."""
        if self.obsRows is None:
            raise ValueError('obsMisfit: this instance has no observations')
        if self._towers is not None:                  # every tower holds all observations: rank 0 answers
            return self._towers.call('obsMisfit')
        tData = getattr(self, 'tData', None) or self._build_tdata()
        tData.select_mor(0)
        self.engine.eval_loss(tData.engine_batch(0, 0))
        return self.engine.obs_misfit()

    def periodicTrainData(self):
        """
        (No reference counterpart: `ADPDE(..., periodic=[(A, B), ...])`.)  The paired rows of every periodic pair, assembled once
        on the host in fp64.  Side A: the uniform boundary points `mesh.bCoordinates[A]` paired with the time nodes like the
        Dirichlet rows.  Side B: the same rows with the space columns shifted by the translation s that maps edge A onto edge B,
        taken from the vertices (polygon edges of a pair run in opposite senses: s = v_{B,next} - v_A; 1D: the other end minus
        this one), not from the ordering of `mesh.bCoordinates[B]`.  Both sides carry A's outward unit normal as direction.
        Returns dict(X, dir, pairs): X [2 nP, inpDim] with every pair's side-A rows first, then every pair's side-B rows in the
        same order (row i pairs with row i + nP), dir [2 nP, dim], pairs = [(A, B, rows)].
        """
        PDE, dim = self.PDE, self.dim
        td = PDE.timeDependent
        domain = PDE.domain
        t_coord = self.timeDisc()[1] if td else []
        mesh = domain.getMesh(self.discNum, self.bDiscNum)
        normals = np.asarray(domain.boundaryNormals(), dtype=float)
        XA, XB, dirs, pairs = [], [], [], []
        for A, B in PDE.periodic:
            if dim == 1:
                lim = np.reshape(np.asarray(domain.lim, dtype=float), -1)
                s = np.array([lim[B] - lim[A]])
            else:
                g = np.asarray(domain.boundryGeom, dtype=float)
                s = g[B, 1] - g[A, 0]
            xa = np.array(uf.pairMats(mesh.bCoordinates[A], t_coord), dtype=float)
            xb = xa.copy()
            xb[:, :dim] += s
            XA.append(xa)
            XB.append(xb)
            dirs.append(np.tile(normals[A], (xa.shape[0], 1)))
            pairs.append((A, B, xa.shape[0]))
        d = np.vstack(dirs)
        return dict(X=np.vstack(XA + XB), dir=np.vstack([d, d]), pairs=pairs)

    def biTrainData(self, biInput, biDof, biArg=[], basis=True):
        """Labels g/beta on Dirichlet edges, IC(x) on the initial slice (VarNet.py:649-722).  With a Dirichlet or an initial basis
        the sums at the current amplitudes (`bicAmplitudes`) are part of the labels; basis=False: `g/beta` and `IC` alone."""
        dim, PDE = self.dim, self.PDE
        td = PDE.timeDependent
        nb = PDE.domain.bIndNum
        if uf.isempty(biArg):
            biArg = [{} for _ in range(nb)] + ([{}] if td else [])
        labels, indp, j = [], 0, 0
        ind = 0
        for bInd in range(nb):
            if PDE.BCtype[bInd] != 'Dirichlet':
                continue
            ind = indp + biDof[j]
            j += 1
            beta, g = PDE.BCs[bInd][1], PDE.BCs[bInd][2]
            targ = [biInput[indp:ind, dim][np.newaxis].T] if td else []
            arg = biArg[bInd] if biArg[bInd] is not None else {}
            labels.append(g(biInput[indp:ind, :dim], *targ, **arg) / beta)
            indp = ind
        out = uf.vstack(labels)
        if td:
            arg = biArg[-1] if biArg[-1] is not None else {}
            out = uf.vstack([out, PDE.IC(biInput[ind:, :dim], **arg)])
        if basis and sum(self._keyed_sizes(self._BIC, PDE)) > 0:
            out = np.asarray(out, dtype=np.float64).reshape(-1, 1) + (self._keyed_vector(self._BIC) @ self._bic_basis(biInput, biDof)).reshape(-1, 1)
        return out

    def PDEinpData(self, Input, inpArg=[], basis=True, field=True):
        """kappa, v, s at the rows of Input (VarNet.py:726-774).  With a source basis s = source + sum_j a_j phi_j at the current
        amplitudes (`sourceAmplitudes`); basis=False: `source` alone.  With field bases kappa and v are the sums at the current
        amplitudes (`fieldAmplitudes`); field=False: `diff` and `vel` alone."""
        dim, PDE = self.dim, self.PDE
        if uf.isempty(inpArg):
            diffArg, velArg, sourceArg = {}, {}, {}
        else:
            diffArg, velArg, sourceArg = [a if a is not None else {} for a in inpArg]
        targ = [Input[:, dim][np.newaxis].T] if PDE.timeDependent else []
        X = Input[:, 0:dim]
        src = PDE.sourceFun(X, *targ, **sourceArg)
        if basis and getattr(PDE, 'sourceBasis', None) is not None:
            src = np.asarray(src, dtype=np.float64).reshape(-1, 1) + self._source_basis(Input) @ self.sourceAmplitudes().reshape(-1, 1)
        Jk, Jv = self._keyed_sizes(self._FIELD, PDE)
        if Jk + Jv == 0:
            return PDE.diffFun(X, *targ, **diffArg), PDE.velFun(X, *targ, **velArg), src
        # (a basis excludes MOR: no extra arguments) the plain fields, plus the sums at the current amplitudes
        diff = np.asarray((PDE.diffFun0 if Jk else PDE.diffFun)(X, *targ), dtype=np.float64).reshape(-1, 1)
        vel = np.asarray((PDE.velFun0 if Jv else PDE.velFun)(X, *targ), dtype=np.float64).reshape(-1, dim)
        if field:
            b = self._keyed_vector(self._FIELD)
            chi, _, omega = self._field_basis(Input)
            diff = diff + np.tensordot(b[:Jk], chi, axes=1)
            vel = vel + np.tensordot(b[Jk:], omega, axes=1)
        return diff, vel, src

    def diffGradData(self, Input):
        """grad kappa at the rows of Input, [n, dim]: with a diffusivity basis at the current amplitudes (`fieldAmplitudes`)."""
        dim, PDE = self.dim, self.PDE
        targ = [Input[:, dim][np.newaxis].T] if PDE.timeDependent else []
        X = Input[:, 0:dim]
        Jk = self._keyed_sizes(self._FIELD, PDE)[0]
        if Jk == 0:
            return PDE.d_diffFun(X, *targ)
        g = np.asarray(PDE.d_diffFun0(X, *targ), dtype=np.float64).reshape(-1, dim)
        return g + np.tensordot(self._keyed_vector(self._FIELD)[:Jk], self._field_basis(Input, grad=True)[1], axes=1)

    def _reaction_rate(self, Input):
        """Reaction rate at the rows of Input (a column), evaluated like the source (PDEinpData)."""
        dim, PDE = self.dim, self.PDE
        targ = [Input[:, dim][np.newaxis].T] if PDE.timeDependent else []
        rate = np.asarray(PDE.reactionRateFun(Input[:, 0:dim], *targ), dtype=np.float64)
        if rate.size != Input.shape[0]:
            raise ValueError('the reaction rate must return one value per point (a column), got shape %s for %d points'
                             % (rate.shape, Input.shape[0]))
        return rate.reshape(-1, 1)

    def _nlflux_field(self, Input):
        """(w [n, dim], div w [n, 1] or None) of the flux term at the rows of Input, evaluated like the velocity (PDEinpData)."""
        dim, PDE = self.dim, self.PDE
        targ = [Input[:, dim][np.newaxis].T] if PDE.timeDependent else []
        n = Input.shape[0]
        w = np.asarray(PDE.nlfluxWFun(Input[:, 0:dim], *targ), dtype=np.float64)
        if w.size != n * dim:
            raise ValueError('the flux field w must return [n, dim] values, got shape %s for %d points in %d dimension(s)'
                             % (w.shape, n, dim))
        div = None
        if PDE.nlfluxDivFun is not None:
            div = np.asarray(PDE.nlfluxDivFun(Input[:, 0:dim], *targ), dtype=np.float64)
            if div.size != n:
                raise ValueError('div_w must return one value per point (a column), got shape %s for %d points' % (div.shape, n))
            div = div.reshape(-1, 1)
        return w.reshape(n, dim), div

    def _vel_div(self, Input):
        """div vel [n, 1] at the rows of Input, or None (taken as zero): the `div_vel` callable of `ADPDE(nldiff=...)`."""
        dim, PDE = self.dim, self.PDE
        if getattr(PDE, 'nldiffDivFun', None) is None:
            return None
        targ = [Input[:, dim][np.newaxis].T] if PDE.timeDependent else []
        div = np.asarray(PDE.nldiffDivFun(Input[:, 0:dim], *targ), dtype=np.float64)
        if div.size != Input.shape[0]:
            raise ValueError('div_vel must return one value per point (a column), got shape %s for %d points'
                             % (div.shape, Input.shape[0]))
        return div.reshape(-1, 1)

    def MORargExtract(self, batch, MORdiscArg):
        """Keyword arguments of every parametric callable for MOR batch `batch`, and the extra
        network inputs, in the reference's order (VarNet.py:901-1049): BC functions, IC, diff,
        vel, source."""
        PDE = self.PDE
        fi = PDE.MORfunInd
        names = PDE.MORvar.ArgNames
        argInd = self.fixData.MORargInd
        nb = PDE.domain.bIndNum
        inpNN = []

        def kw(find):
            vals = MORdiscArg[find][int(argInd[batch, find]), :]
            inpNN.extend(vals)
            return uf.buildDict(names[find], vals)

        biArg = [{} for _ in range(nb)] + ([{}] if PDE.timeDependent else [])
        if fi['biData']:
            for bInd in range(nb):
                if PDE.BCtype[bInd] == 'Dirichlet' and fi['BCs'][bInd] is not None:
                    biArg[bInd] = kw(fi['BCs'][bInd])
            if fi['IC'] is not None:
                biArg[-1] = kw(fi['IC'])
        inpArg = [{}, {}, {}]
        if fi['inpData']:
            for j, key in enumerate(('diff', 'vel', 'source')):
                if fi[key] is not None:
                    inpArg[j] = kw(fi[key])
        return biArg, inpArg, np.reshape(np.asarray(inpNN, dtype=float), [1, len(inpNN)])

    # -- device-resident data -----------------------------------------------------------------
    def _ansatz_rows(self, X, G=None):
        """The four streams (A, B, a, b) of the ansatz c = A + B N at the rows X in fp64 (uploaded as fp32): a = grad_x A . G and
        b = grad_x B . G along the rows' directions G [n, dim]; G None: a set without directions (a = b = None)."""
        PDE, dim = self.PDE, self.dim
        X = np.asarray(X, dtype=np.float64)
        A, B = PDE.ansatz_values('A', X)[:, 0], PDE.ansatz_values('B', X)[:, 0]
        if G is None:
            return A, B, None, None
        G = np.asarray(G, dtype=np.float64).reshape(-1, dim)
        return A, B, (PDE.ansatz_values('dA', X, dim) * G).sum(1), (PDE.ansatz_values('dB', X, dim) * G).sum(1)

    def _assemble(self, Input, biInput, biDof, batch, MORdiscArg):
        """Host fp64 assembly of one MOR batch -> dict of device tensors (VarNet.py:778-857)."""
        fd, eng = self.fixData, self.engine
        if MORdiscArg is None:
            biArg, inpArg, MORinp = [], [], None
        else:
            biArg, inpArg, MORinp = self.MORargExtract(batch, MORdiscArg)
        # learnt boundary and initial amplitudes: the engine mixes label0 and the basis streams itself; else the sums are folded
        # into the labels here
        biLabel = self.biTrainData(biInput, biDof, biArg, basis=self.bicLearn is None)
        bicB = None
        if self.bicLearn is not None:
            bicB = eng.dev(np.ascontiguousarray(self._bic_basis(biInput, biDof)))       # [J, nB], stream-major, fp64 then fp32
        # learnt amplitudes: the engine mixes s0 and the basis streams itself; else the sum is folded into the source here
        srcphi = None
        # ... and likewise g0 and the basis streams of gcoef
        diff, vel, src = self.PDEinpData(Input, inpArg, basis=self.srcLearn is None, field=self.fldLearn is None)
        if self.srcLearn is not None:
            srcphi = eng.dev(np.ascontiguousarray(self._source_basis(Input).T))         # [J, nT], stream-major, fp32
        nt, q, dim = fd.nt, fd.integNum, self.dim
        N_rows = dNt_rows = None
        psi = nldiffCoef = None
        if getattr(self.PDE, 'nldiff', None) is not None:
            # D(u) scales the diffusion part of the one tangent the engine carries: gcoef = kappa dN/dx alone, and the advection
            # goes to the value side as -u psi, psi = sum_d v_d dN/dx_d + N div v (fp64 here, uploaded as fp32; None: vel == 0)
            nldiffCoef = list(self.PDE.nldiffCoef)
            div = self._vel_div(Input)
            vel = np.asarray(vel, dtype=np.float64).reshape(-1, dim)
            if fd.detJvec:
                Nr, dNxr, dNtr = fd.rows()
                psi = (vel * dNxr).sum(1, keepdims=True) + (0.0 if div is None else div * Nr.reshape(-1, 1))
            else:
                psi = (vel.reshape(nt, q, dim) * fd.dNx[None]).sum(-1)
                if div is not None:
                    psi = psi + div.reshape(nt, q) * np.reshape(fd.N, -1)[None, :]
            psi = eng.dev(np.asarray(psi, dtype=np.float64).reshape(-1)) if np.any(psi) else None
            vel = np.zeros_like(vel)
        if fd.detJvec:
            # non-uniform supports: per-row tables (VarNetUtility.py:506-523)
            Nr, dNxr, dNtr = fd.rows()
            gcoef = diff * dNxr + vel * Nr                          # VarNet.py:837
            N_rows, dNt_rows = eng.dev(Nr.reshape(-1)), eng.dev(dNtr.reshape(-1))
        else:
            # gcoef = kappa*dNx + v*N  (VarNet.py:837) with the period tables broadcast over test functions
            gcoef = (diff.reshape(nt, q, 1) * fd.dNx[None, :, :] +
                     vel.reshape(nt, q, dim) * fd.N[None, :, None]).reshape(nt * q, dim)
        az = az_bic = None
        if getattr(self.PDE, 'ansatz', None) is not None:
            # the ansatz streams beside gcoef, in fp64, contracted with the very gcoef that is uploaded (with D(u): kappa dN/dx alone;
            # psi reads the transformed u, so nothing else moves); the BC/IC rows have no direction
            az = tuple(eng.dev(v) for v in self._ansatz_rows(Input, gcoef))
            az_bic = tuple(None if v is None else eng.dev(v) for v in self._ansatz_rows(biInput))
        fldG = None
        if self.fldLearn is not None:
            # G_j = chi_j dN/dx (diffusivity streams, first) or omega_j N (velocity streams): [J, nT, dim], stream-major, evaluated
            # in fp64 like gcoef and rounded once on upload
            chi, _, omega = self._field_basis(Input)
            if fd.detJvec:
                G = np.concatenate([chi * dNxr[None], omega * Nr.reshape(1, -1, 1)])
            else:
                G = np.concatenate([(chi.reshape(-1, nt, q, 1) * fd.dNx[None, None]).reshape(-1, nt * q, dim),
                                    (omega.reshape(-1, nt, q, dim) * np.reshape(fd.N, -1)[None, None, :, None]).reshape(-1, nt * q, dim)])
            fldG = eng.dev(np.ascontiguousarray(G))
        if MORinp is not None:
            Input = np.hstack([Input, np.tile(MORinp, [Input.shape[0], 1])])
            biInput = np.hstack([biInput, np.tile(MORinp, [biInput.shape[0], 1])])
        rate = reactCoef = None
        if getattr(self.PDE, 'reaction', None) is not None:
            # rate at the rows of Input in fp64, uploaded as fp32 (a constant rate is folded into the coefficients: no stream)
            reactCoef = list(self.PDE.reactionCoef)
            if self.PDE.reactionRate is not None:
                reactCoef = [self.PDE.reactionRate * c for c in reactCoef]
            else:
                rate = eng.dev(np.asarray(self._reaction_rate(Input), dtype=np.float64).reshape(-1))
        phi = nlfluxCoef = None
        if getattr(self.PDE, 'nlflux', None) is not None:
            # phi = sum_d w_d dN/dx_d at the rows of Input in fp64, beside gcoef; uploaded as fp32
            w = self._nlflux_field(Input)[0]
            if fd.detJvec:
                phi = (w * dNxr).sum(1)
            else:
                phi = (w.reshape(nt, q, dim) * fd.dNx[None]).sum(-1)
            phi = eng.dev(np.asarray(phi, dtype=np.float64).reshape(-1))
            nlfluxCoef = list(self.PDE.nlfluxCoef)
        slab = self._slab_tensor(Input) if self.causal is not None else None   # (time column dim: the same ids for every MOR batch)
        return dict(Input=eng.dev(Input), Input_host=Input, gcoef=eng.dev(gcoef), rate=rate, reactCoef=reactCoef, slab=slab,
                    phi=phi, nlfluxCoef=nlfluxCoef, psi=psi, nldiffCoef=nldiffCoef, srcphi=srcphi, fldG=fldG, bicB=bicB,
                    az=az, az_bic=az_bic,
                    source=eng.dev(src.reshape(-1)) if self.lossOpt['isSource'] else None,
                    biInput=eng.dev(biInput), biLabel=eng.dev(biLabel.reshape(-1)),
                    N_rows=N_rows, dNt_rows=dNt_rows,
                    detJ=eng.dev(np.reshape(fd.detJ, -1)) if fd.detJvec else None)

    def _sync_sampling(self):
        """Towers must draw ONE training set (the reference samples once and slices it per tower,
        VarNetUtility.py:819-857): rank 0 draws a seed from its NumPy stream, every rank re-seeds with it."""
        if self.world == 1 or self.dist is None:
            return
        box = [int(np.random.randint(0, 2 ** 31 - 1)) if self.rank == 0 else None]
        self.dist.broadcast_object_list(box, src=0)
        np.random.seed(box[0])

    def _build_tdata(self, batchNum=None, batchLen=None, smpScheme='uniform', frac=0.5, addTrainPts=True,
                     suppFactor=1.0):
        fd = self.fixData
        if smpScheme != 'uniform':
            self._sync_sampling()
        Input, _, biInput, biDof = self.trainingPoints(smpScheme, frac, addTrainPts, suppFactor)
        if smpScheme == 'optimal' and not addTrainPts:
            fd.biDof = [int(b) for b in biDof]
        MORdiscArg = fd.MORdiscArg
        mor = [self._assemble(Input, biInput, biDof, b, MORdiscArg) for b in range(fd.MORbatchNum)]
        return ManageTrainData(self, mor, batchNum, batchLen)

    # -- loss components / weights ----------------------------------------------------------------
    def _allreduce(self, t):
        if self.dist is not None and self.world > 1:
            self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)

    def _gather_lossVec(self, lv, tData, bi):
        """Loss field of mini-batch `bi` as the reference's controller sees it: the towers' fields concatenated in
        tower order (`tf.concat([compTowers[pu].lossVec ...], axis=0)`, TFModel.py:319), one entry per test function
        of the blocks `ManageTrainData.block(bi, pu)`.  One all-gather of `batchLen` floats per rank (ragged and empty
        last blocks are padded for the collective and cut afterwards); every rank returns the same column."""
        torch = self.engine.torch
        if self.world == 1 or self.dist is None:
            return lv.cpu().numpy().reshape(-1, 1)
        L = int(tData.batchLen)
        # gloo gathers host tensors only; RCCL gathers where the field lies
        dev = lv.device if self.dist.get_backend() == 'nccl' else torch.device('cpu')
        mine = torch.zeros(L, dtype=lv.dtype, device=dev)
        mine[:lv.numel()] = lv.reshape(-1).to(dev)
        parts = [torch.empty_like(mine) for _ in range(self.world)]
        self.dist.all_gather(parts, mine)
        cols = []
        for pu in range(self.world):
            n0, n1 = tData.block(bi, pu)
            cols.append(parts[pu][:n1 - n0])
        return torch.cat(cols).cpu().numpy().reshape(-1, 1)

    def _refuse_fp64_on_towers(self, what):
        if self._towers is not None:
            raise NotImplementedError(
                '%s: the fp64 objective is evaluated by the process that owns the engine and the training set; this instance is '
                'the controller of forked towers and holds neither.  Build the instance with one processor (or call it on a '
                'rank of a launched job) to evaluate in double precision -- an fp32 result is never returned in its place' % what)

    def _refuse_fp64_on_ansatz(self, what):
        if getattr(self.PDE, 'ansatz', None) is not None:
            raise NotImplementedError('%s with an ansatz: the fp64 objective does not carry the ansatz stage -- an fp32 result is '
                                      'never returned in its place' % what)

    def splitLoss(self, tData, W=None, fp64=False):
        """BC, IC and variational loss summed over MOR batches (VarNet.py:1053-1090).  fp64=True: the components (and the loss
        field) from the device's double-precision evaluation of the same objective (VNEngine.objective64)."""
        if fp64:
            self._refuse_fp64_on_towers('splitLoss(fp64=True)')
            self._refuse_fp64_on_ansatz('splitLoss(fp64=True)')
        ekw = {'fp64': True} if fp64 else {}
        if W is None:
            W = np.eye(3)
        eng, fd = self.engine, self.fixData
        torch = eng.torch
        comp = np.zeros([3, 1])
        lossVec = [] if fd.lossVecflag else None
        for mb in range(fd.MORbatchNum):
            tData.select_mor(mb)
            var = 0.0
            lv_b = []
            for bi in range(tData.batchNum):
                out, lv = eng.eval_loss(tData.engine_batch(mb, bi), lossVec=fd.lossVecflag, **ekw)
                bc, ic = out[1], out[2]
                var += out[3]
                if lv is not None:
                    lv_b.append(self._gather_lossVec(lv, tData, bi))
            if self.world > 1:
                t = torch.tensor([var], dtype=torch.float64, device=eng.device)
                self._allreduce(t)
                var = float(t.item())
            comp += np.array([[bc, ic, var]]).T
            if lossVec is not None and lv_b:
                lossVec.append(np.vstack(lv_b))
        return np.matmul(W, comp), tData, lossVec

    def precisionReport(self, tData=None):
        """How far the fp32 training step is from a double-precision evaluation of the same objective, at the current
        parameters and on the training set `tData` (default: the set of the last train() call, else a freshly built full-batch set).
        Per mini-batch the fp32 gradient call (VNEngine.grad: the step train() runs, on the route and formulation recorded
        below) is compared with VNEngine.objective64; the sums over the mini-batches are judged:
            'loss'        {loss, BCloss, ICloss, varLoss: |f32 - f64| / |f64|}
            'grad_global' ||g32 - g64||_inf / ||g64||_inf
            'grad_blocks' {parameter tensor: max|g32 - g64| over the tensor / max(||g64 tensor||_inf, 1e-7 ||g64||_inf)}
            'route'       kernel family of the fp32 side (vn_kernel_path), 'two_pass', 'dedup' (the formulation: dedup_on)
            'fp32', 'fp64' the summed components themselves, 'batches' the number of mini-batches.
        Diagnostic only: nothing in train() calls it, and it leaves parameters and optimizer state as they are."""
        self._refuse_fp64_on_towers('precisionReport')
        self._refuse_fp64_on_ansatz('precisionReport')
        if self.world > 1:
            raise NotImplementedError('precisionReport compares one rank\'s step with its fp64 evaluation: run it on one rank')
        if tData is None:
            tData = getattr(self, 'tData', None) or self._build_tdata()
        eng, fd = self.engine, self.fixData
        P = eng.P
        gb = eng.bind_grad_buffer()
        f32, f64 = np.zeros(4), np.zeros(4)
        g32, g64 = np.zeros(P), np.zeros(P)
        nb = 0
        for mb in range(fd.MORbatchNum):
            tData.select_mor(mb)
            for bi in range(tData.batchNum):
                b = tData.engine_batch(mb, bi)
                eng.grad(b)
                a = gb.detach().cpu().numpy().astype(np.float64)
                out, g, _ = eng.objective64(b, grad=True)
                g32 += a[:P]
                f32 += a[P:P + 4]
                g64 += g.detach().cpu().numpy().astype(np.float64)
                f64 += np.asarray(out, dtype=np.float64)
                nb += 1
        rel = lambda x, y: abs(x - y) / max(abs(y), 1e-300)
        names = ['loss', 'BCloss', 'ICloss', 'varLoss']
        scale = max(float(np.max(np.abs(g64))), 1e-300)
        blocks, off, fan = {}, 0, self.inpDim
        for l, h in enumerate(list(self.layerWidth) + [1]):
            tag = 'o' if l == len(self.layerWidth) else str(l + 1)
            for name, n in (('W' + tag, fan * h), ('b' + tag, h)):
                s = slice(off, off + n)
                blocks[name] = float(np.max(np.abs(g32[s] - g64[s]))) / max(float(np.max(np.abs(g64[s]))), 1e-7 * scale)
                off += n
            fan = h
        kp = eng.kernel_path() if hasattr(eng, 'kernel_path') else (None, None)
        fam = {0: 'auto', 1: 'generic', 2: 'fused (4-wave)', 3: 'fused16 (8-wave)', 4: 'layered'}
        return {'loss': {k: rel(f32[i], f64[i]) for i, k in enumerate(names)},
                'grad_global': float(np.max(np.abs(g32 - g64))) / scale,
                'grad_blocks': blocks,
                'route': fam.get(kp[0], kp[0]), 'kernel': kp[0], 'two_pass': bool(kp[1]) if kp[1] is not None else None,
                'dedup': bool(getattr(tData, 'dedup_on', False)),
                'fp32': dict(zip(names, f32.tolist())), 'fp64': dict(zip(names, f64.tolist())), 'batches': nb}

    def trainWeight(self, weight, tData, normalizeW=False, useOriginalW=False, lossTot=1.e6):
        """Initial penalty weights (VarNet.py:1094-1146): default branch scales `weight` so the
        weighted initial loss is 1e6."""
        td = self.PDE.timeDependent
        lossVal, tData, _ = self.splitLoss(tData)
        lossVal = np.reshape(lossVal, 3)
        lossTmp = lossVal if td else np.array([lossVal[0], lossVal[2]])
        if useOriginalW:
            trainW = np.array(weight, dtype=float)
        elif normalizeW:
            nw = len(weight)
            W = np.tile(weight, [nw, 1]) / np.reshape(weight, [nw, 1])
            W = np.sum(W, axis=1, keepdims=True) * np.reshape(lossTmp, [nw, 1])
            trainW = np.reshape(lossTot / W, nw)
        else:
            trainW = lossTot / np.sum(np.array(weight) * np.array(lossTmp)) * np.array(weight, dtype=float)
        if not td:
            trainW = np.array([trainW[0], 0., trainW[1]])
        s = 'Training weight information:\n'
        s += '\tboundary condition loss value: %.4e\n\tinitial condition loss value: %.4e\n' % (lossVal[0], lossVal[1])
        s += '\tintegral loss value: %.4e\n\trequested weight on each term: %s\n' % (lossVal[2], str(weight))
        s += '\tcorresponding training weights: %s\n\n' % np.array2string(np.array(trainW), precision=4)
        if self.trainRes.verbose and self.rank == 0:
            print(s)
        self.trainRes.writeCase(s)
        return np.array(trainW, dtype=float), tData, lossVal

    # -- training -------------------------------------------------------------------------------------
    def optimIter(self, tData, mb, loss_acc):
        """One pass over the mini-batches of MOR batch mb (VarNetUtility.py:1021-1047):
        gradient, tower SUM (all-reduce), TF-1 Adam; the pre-update loss is added to the
        device scalar `loss_acc`."""
        eng = self.engine
        P = eng.P
        if self._is_lbfgs():
            # one L-BFGS iteration (train() has refused everything but one full batch); the epoch's loss is f_k, the loss at
            # the parameters the epoch started from, as an Adam epoch records its pre-update loss
            info = eng.lbfgs_step(tData.engine_batch(mb, 0))
            self._lbfgs_info = info
            loss_acc += float(info['f_k'])
            return
        if (self.world == 1 or self.comm == 'rccl') and hasattr(eng, 'train_epoch'):
            # the whole pass in one host call (no per-mini-batch Python / launch-queue gaps); with towers the
            # engine's own RCCL communicator sums the gradient between the two kernels
            ids = tData._epoch_ids.get(mb) if hasattr(tData, '_epoch_ids') else None
            if ids is None:
                if not hasattr(tData, '_epoch_ids'):
                    tData._epoch_ids = {}
                ids = tData._epoch_ids[mb] = tuple(tData.engine_batch(mb, bi) for bi in range(tData.batchNum))
            eng.train_epoch(ids, loss_acc)
            return
        gb = eng.bind_grad_buffer()
        for bi in range(tData.batchNum):
            eng.grad(tData.engine_batch(mb, bi))
            self._allreduce(gb)
            eng.apply()
            loss_acc += gb[P]

    def _is_lbfgs(self):
        return str(self.optimizer).lower() == 'lbfgs'

    def termGradients(self, batches=None):
        """The per-term gradients of the objective at the current parameters, as a diagnostic (vn_term_grads): {'terms', 'norms',
        'values', 'cosines'} over ('bc', 'ic', 'var', 'obs') at unit weights, summed over `batches` (engine batch ids; default: the
        mini-batches of the current training set).  A cosine near -1 says that two terms pull against each other; a term without
        rows holds zeros.  The engine's weights are left as they are; its gradient buffer is overwritten."""
        if self._towers is not None or self.world > 1:
            raise NotImplementedError('termGradients with towers is not supported: each term\'s gradient would need its own all-reduce.')
        if self._is_lbfgs():
            raise NotImplementedError('termGradients with optimizer=\'lbfgs\' is not supported: the evaluations would disturb the '
                                      'optimizer\'s gradient pair.')
        tData = getattr(self, 'tData', None)
        if tData is None:
            tData = self.tData = self._build_tdata()
        if batches is None:
            tData.select_mor(0)
            batches = tuple(tData.engine_batch(0, bi) for bi in range(tData.batchNum))
        r = self.engine.term_grads(tuple(batches))
        return {'terms': balance_rules.TERMS, 'norms': np.sqrt(r['sumsq']), 'values': np.array(r['value'], dtype=float),
                'cosines': balance_rules.cosines(r['gram'])}

    def _lbfgs_refusals(self, batchNum, batchLen, shuffleData):
        """optimizer='lbfgs' builds its curvature pairs from consecutive gradients of ONE objective: whatever makes consecutive
        iterations see different ones is refused, with its reason."""
        fd = self.fixData
        if self.world > 1 or self._towers is not None:
            raise ValueError('optimizer=\'lbfgs\' runs on one rank: with towers every rank would have to take the same '
                             'line-search decision from an all-reduced loss, which is not built')
        many = (batchNum is not None and int(batchNum) > 1) or (batchLen is not None and int(batchLen) < fd.nt)
        if many:
            raise ValueError('optimizer=\'lbfgs\' needs the full batch (batchNum / batchLen give more than one mini-batch): '
                             'consecutive iterations would see different objectives')
        if shuffleData:
            raise ValueError('optimizer=\'lbfgs\' with shuffleData=True: a shuffle changes the objective between iterations')
        if fd.MORbatchNum > 1:
            raise ValueError('optimizer=\'lbfgs\' with %d MOR batches: consecutive iterations would see different objectives'
                             % fd.MORbatchNum)

    def _choose_formulation(self, tData, dedup, shuffleData=False):
        """Apply `train(dedup=...)` to a training set; returns {'requested', 'on', 'unique_points', 'reason'} and records the
        decision in caseData.txt.  A request that cannot be served is a warning (`dedup=True`) or a recorded sentence
        ('auto'), never a silent row-wise run."""
        state = {'requested': dedup, 'on': False, 'unique_points': 0, 'reason': None}
        if dedup is False:
            state['reason'] = 'dedup=False was requested'
        elif shuffleData:
            state['reason'] = 'shuffleData=True: ' + \
                'the mini-batches are shuffled (the point map of every block would have to be rebuilt at each shuffle)'
        else:
            state['reason'] = tData.dedup_applies()
            if state['reason'] is None and dedup == 'auto' and not tData.dedup_pays():
                state['reason'] = ('the step is too small for it to pay (three more kernel launches and a second prologue '
                                   'against the work saved: DEDUP_MODEL); dedup=True forces it')
            if state['reason'] is None:
                state['unique_points'] = int(tData.enable_dedup())
                state['on'] = state['unique_points'] > 0
                state['reason'] = tData.dedup_reason
        if state['on']:
            msg = ('interior term: de-duplicated formulation, %d unique quadrature points for %d rows per epoch '
                   '(dedup=%r)\n\n' % (state['unique_points'], self.fixData.nT * self.fixData.MORbatchNum, dedup))
        else:
            msg = 'interior term: row-wise formulation (dedup=%r): %s\n\n' % (dedup, state['reason'])
            if dedup is True:
                warnings.warn('dedup=True cannot be served, training row-wise: ' + state['reason'])
        if getattr(self, 'trainRes', None) is not None:
            if self.trainRes.verbose and self.rank == 0:
                print(msg)
            self.trainRes.writeCase(msg)
        return state

    def train(self, folderpath, weight=None, smpScheme='uniform', epochNum=500000, tol=1.e-1,
              verbose=True, saveFreq=100, pltReplace=True, saveMORdata=False, frac=None,
              addTrainPts=True, suppFactor=1.0, multiTrainUpd=False, trainUpdelay=2e4, tolUpd=0.01,
              reinitrain=True, updateWeights=False, normalizeW=False, adjustWeight=False,
              useOriginalW=False, batchNum=None, batchLen=None, shuffleData=False, shuffleFreq=1,
              dedup='auto', lossLag=None, balance=None):
        """Training loop of /root/reference/VarNet.py:1197-1421 (uniform, random and residual-driven
        "optimal" sampling with re-initialisation and re-weighting).

        With `observations` the misfit joins the loss as obsWeight * O: obsWeight is on the scale of `weight`, multiplied by
        the factor trainWeight applies to the variational weight (`useOriginalW` leaves it unscaled); `adjustWeight` (which
        raises the BC/IC weights at a re-draw) leaves it alone, and re-draws leave the observed points alone.

        `balance` (extension; what the reference's `updateWeights` was meant to do): None | 'gradnorm' | 'maxmean' | {'rule',
        'freq': 1000, 'alpha': 0.9, 'cap': 1e4, 'keepLoss': True}.  Before epoch 1 and before every epoch e with (e - 1) % freq == 0
        the engine measures the gradient of every active term over the batches of the epoch (vn_term_grads) and the rule of
        varnet_amd/balance.py moves the train weights; a lossLag block ends there, a re-draw restarts the moving average from the
        weights it sets, and `trainRes.balanceHist` and the case file record every probe.  Refused with towers, L-BFGS and MOR."""
        bal = balance_rules.parse_balance(balance)
        if bal is not None:
            if self._towers is not None or self.world > 1:
                raise NotImplementedError('balance= with towers is not supported: each term\'s gradient would need its own all-reduce.')
            if self._is_lbfgs():
                raise NotImplementedError('balance= with optimizer=\'lbfgs\' is not supported: a probe would change the objective '
                                          'between two iterations and disturb the optimizer\'s gradient pair.')
            if not uf.isnone(self.PDE.MORvar):
                raise NotImplementedError('balance= with model-order reduction is not supported: every MOR batch is another objective '
                                          'and would need its own weights.')
        if self._is_lbfgs():
            self._lbfgs_refusals(batchNum, batchLen, shuffleData)
        if self._towers is not None:                  # controller of forked towers: every tower runs the loop
            kw = {k: v for k, v in locals().items() if k not in ('self', 'folderpath', 'bal')}
            self.folderpath = folderpath
            self.trainRes = self._towers.call('train', folderpath, **kw)
            return self.trainRes
        if uf.isnone(folderpath) or uf.isempty(folderpath):
            raise ValueError('a folder path must be provided to backup the trained model!')
        self.folderpath = folderpath
        td = self.PDE.timeDependent
        if weight is None:
            weight = [1., 1., 1.] if td else [1., 1.]
        elif td and len(weight) != 3:
            raise ValueError('weight dimension does not match!')
        elif not td and len(weight) != 2:
            raise ValueError('weight dimension does not match!')
        if smpScheme not in ('uniform', 'random', 'optimal'):
            raise ValueError('sampling scheme is not valid!')
        if self.obsRows is not None and float(weight[-1]) == 0.0:
            raise ValueError('observations with a zero variational weight: obsWeight is scaled by the factor train() puts on the '
                             'variational weight, which a zero weight leaves undefined')
        if updateWeights:
            raise NotImplementedError('updateWeights=True is broken in the reference (VarNet.py:1373)')
        self.smpScheme = smpScheme
        if frac is None:
            frac = 0.50 if addTrainPts else 0.25
        if batchNum is None and batchLen is None and shuffleData:
            warnings.warn('shuffling data is possible for batch-optimization, setting \'shuffleData\' to False!')
            shuffleData = False
        if shuffleData and self.tfAdapt is not None:
            raise NotImplementedError('tfAdapt=... with shuffleData=True is not supported: a shuffle changes which test function is k, '
                                      'and the state lambda_k belongs to the test function')
        if shuffleData and (self.bicWeights is not None or self.bicAdapt is not None):
            raise NotImplementedError('bicWeights= / bicAdapt= with shuffleData=True is not supported: a shuffle permutes the BC/IC rows '
                                      'per feed (a per-batch copy), and the weights belong to the rows as they were registered')
        if shuffleData and getattr(self.PDE, 'ansatz', None) is not None:
            raise NotImplementedError('an ansatz with shuffleData=True is not supported: a shuffle permutes the BC/IC rows per feed '
                                      '(a per-batch copy), and the ansatz streams belong to the rows as they were registered')
        argDict = {k: v for k, v in locals().items() if k not in ('self', 'bal')}

        if not addTrainPts and np.abs(suppFactor - 1.0) > 1.e-15:
            warnings.warn('\'suppFactor\' is set to 1.0 since the number of training points does not change!')
            suppFactor = 1.0
        eng, fd = self.engine, self.fixData
        torch = eng.torch
        self._adapt_owner = self._bicw_owner = None          # the adaptive states of an earlier train() call are not carried over
        if getattr(self, 'tData', None) is not None:
            self.tData._bicw_saved = self.tData._adapt_saved = None
        tData = self._build_tdata(batchNum, batchLen)        # first set is always uniform (VarNet.py:1300)
        trainRes = TrainResult(folderpath if self.rank == 0 else None, fd.cEx is not None, verbose, saveFreq, pltReplace)
        trainRes.initializeCase(self, argDict)
        trainRes._plot_last = time.perf_counter()            # the convergence plots are refreshed at most every `plotEvery` seconds and
        self.trainRes = trainRes                             # flushed when train() returns: a short run draws them once (1.1 s at 300 dpi)
        # Formulation of the interior term (extension; the arithmetic is the reference's either way, VarNet.py:576-588 and
        # TFModel.py:653-664): 'auto' (default) evaluates the network once per UNIQUE quadrature point wherever that applies
        # and pays, True asks for it and warns when it cannot be had, False keeps one evaluation per (test function, point) row.
        if dedup not in (True, False, 'auto'):
            raise ValueError('dedup must be True, False or \'auto\'!')
        self.dedup_state = self._choose_formulation(tData, dedup, shuffleData)

        def set_train_weights(tD, wts):
            eng.set_weights([1.0, 1.0, 1.0])
            tW, tD, lv = self.trainWeight(wts, tD, normalizeW, useOriginalW)
            w_e = tD.towerWeights(tW)                                 # VarNetUtility.py:900-901
            eng.set_weights(w_e)
            if self.obsRows is not None:
                # obsWeight is on the scale of `weight`: it takes the factor trainWeight put on the variational weight (1 with
                # useOriginalW), and, the observed points being replicated in every feed like the BC/IC rows, their division
                self._obs_scale = 1.0 if useOriginalW else float(tW[-1]) / float(wts[-1])
                eng.set_obs_weight(self.obsWeight * self._obs_scale / tD.batchNum / tD.puNum)
            return tW, w_e, lv

        trainW, w_eff, lossVal = set_train_weights(tData, weight)
        if bal is not None:
            # the train-scale weights of the four terms (bc, ic, var, obs) are what the rule moves
            bal_rows = np.array([fd.bDofsum > 0 or bool((self.fluxRows or {}).get('edges'))
                                 or bool((getattr(self, 'periodicRows', None) or {}).get('pairs')), bool(td), True,
                                 self.obsRows is not None])

            def balance_start(tW, wts):
                """(w, w0, active, rho) from what trainWeight made of the requested weights `wts`: rho_k = weight_k / weight_var is
                the user's stated preference (after a re-draw: with what adjustWeight made of it)."""
                w4 = np.array([tW[0], tW[1], tW[2], self.obsWeight * self._obs_scale if self.obsRows is not None else 0.0], dtype=float)
                w_user = np.array([wts[0], wts[1] if td else 0.0, wts[-1], self.obsWeight if self.obsRows is not None else 0.0],
                                  dtype=float)
                if not w_user[2] > 0.0:
                    raise ValueError('balance= needs a variational weight > 0: the other weights are stated relative to it.')
                return w4, w4.copy(), bal_rows & (w4 > 0.0), w_user / w_user[2]
            bal_w, bal_w0, bal_active, bal_rho = balance_start(trainW, weight)
            if int(np.sum(bal_active)) < 2:
                raise ValueError('balance= needs at least two active terms (a weight > 0 and rows); this problem has %d.'
                                 % int(np.sum(bal_active)))

            def balance_probe(e):
                nonlocal w_eff, bal_w
                tData.select_mor(0)
                ids = tuple(tData.engine_batch(0, bi) for bi in range(tData.batchNum))
                names = [t for t, a in zip(balance_rules.TERMS, bal_active) if a]
                r = eng.term_grads(ids, terms=names)
                # BC, IC and observation rows are repeated in every (mini-batch, tower) feed and their engine weights divided by
                # batchNum * puNum (towerWeights): the same factor makes the measured figures those of the epoch objective
                f = 1.0 / (tData.batchNum * tData.puNum)
                sc = np.array([f, f, 1.0, f])
                new, skipped = balance_rules.update(bal['rule'], bal_w, bal_w0, bal_rho, bal_active, r['sumsq'] * sc * sc,
                                                    r['max_abs'] * sc, r['mean_abs'] * sc, r['value'] * sc, bal['alpha'],
                                                    bal['cap'], bal['keepLoss'])
                if not skipped:
                    bal_w = new
                    w_eff = tData.towerWeights(bal_w[:3])
                    eng.set_weights(w_eff)
                    if self.obsRows is not None:
                        self._obs_scale = float(bal_w[3]) / float(self.obsWeight) if self.obsWeight else self._obs_scale
                        eng.set_obs_weight(self.obsWeight * self._obs_scale / tData.batchNum / tData.puNum)
                norms = np.sqrt(r['sumsq']) * sc
                trainRes.balanceHist.append((e, bal_w.copy(), norms, balance_rules.cosines(r['gram']), skipped))
                trainRes.writeCase('epoch %d: balance (%s)%s weights %s, gradient norms %s\n'
                                   % (e, bal['rule'], ' skipped (a zero or non-finite gradient norm),' if skipped else '',
                                      np.array2string(bal_w, precision=4), np.array2string(norms, precision=4)))
        # what the reference stores is the array `updateDictFields('trainW', ...)` has divided IN PLACE by batchNum * puNum
        # (VarNet.py:1324-1325 keeps a reference to it, VarNetUtility.py:900-901 rewrites its BC/IC entries): the record in
        # trainData.vn therefore holds the per-feed weights, not trainWeight's return value
        trainRes.trainWeight = np.array(w_eff, dtype=float)
        trainRes.lossComp.append(lossVal)
        self.tData = tData
        tData0 = tData                                         # uniform set for universal cost comparison

        min_loss = float('inf')
        epoch_time = 0.0
        tp_epoch, tp_updates = 1, 0
        resVal = err = lossComp = lossVec = None
        # `lossLag` (extension): the reference reads the loss back after every epoch (VarNetUtility.py:1044); with lossLag = k > 1
        # up to k epochs are enqueued before ONE read-back of their k losses, so small problems (an epoch of 30 us of GPU work
        # behind a 20 us host round trip) keep the GPU busy.  It is a read-back SCHEDULE, not another algorithm: blocks end at
        # every epoch that acts on the state (saveFreq monitors / checkpoints, shuffles), and since round 6 the stopping test
        # `loss < tol` is exact too -- the engine snapshots its state on the device at the start of a block, and when the test
        # fires inside the block the state is rolled back and the epochs up to the one that met the tolerance are replayed (the
        # steps are bitwise reproducible): same losses, same checkpoints, same final parameters and step count as k = 0
        # (tests/test_varnet_host.py::test_loss_lag_is_only_a_readback_schedule).  Default (None): 8 with an engine that can
        # snapshot, else 0.
        can_snap = hasattr(eng, 'state_snapshot') and not self._is_lbfgs()
        if self._is_lbfgs():
            lossLag = 0                                           # every L-BFGS iteration ends in a read-back anyway
        if lossLag is None:
            lossLag = 8 if can_snap else 0
        # Non-uniform sampling: the re-draw test of VarNet.py:1385-1421 runs after every epoch, but what it looks at -- the losses
        # sampled at the monitors, the epochs since the last re-draw -- changes only at monitor epochs (where blocks end anyway) and
        # with the epoch count, so the first epoch at which it can fire inside a block is known when the block is sized
        # (`redraw_at` below) and the block ends there.  A schedule without the engine's snapshot cannot make the stop exact: 0.
        lag = max(0, int(lossLag)) if (smpScheme == 'uniform' or can_snap) else 0

        def redraw_at(e0):
            """First epoch >= e0 at which the re-draw test fires if no monitor intervenes, or None."""
            if smpScheme == 'uniform' or not (multiTrainUpd or tp_updates == 0):
                return None
            t_loss = np.array(trainRes.loss[-5:])
            if len(t_loss) == 0:
                return None
            conv = t_loss[:-1] - t_loss[1:]
            if not (np.sum(conv[conv > 0]) / t_loss[-1] < tolUpd):
                return None
            return max(e0, int(math.ceil(tp_epoch + trainUpdelay - 1)))
        loss_buf = torch.zeros(max(lag, 1), dtype=torch.float32, device=eng.device)
        epoch = 1
        done = False
        while epoch <= epochNum and not done:
            nblk = 1
            if bal is not None and (epoch - 1) % bal['freq'] == 0:
                balance_probe(epoch)
            if lag > 1:
                nblk = min(lag, epochNum - epoch + 1, saveFreq - (epoch - 1) % saveFreq)
                if bal is not None:                                  # a block ends where the next probe sits, as it does at a re-draw
                    nblk = min(nblk, bal['freq'] - (epoch - 1) % bal['freq'])
                if shuffleData:
                    nblk = min(nblk, shuffleFreq - (epoch - 1) % shuffleFreq)
                e_f = redraw_at(epoch)
                if e_f is not None:
                    nblk = max(1, min(nblk, e_f - epoch + 1))
            t0 = time.perf_counter()
            loss_buf.zero_()
            if nblk > 1 and can_snap:
                eng.state_snapshot()                                 # device-side, on the engine's stream, no synchronisation
            for i in range(nblk):
                for mb in range(fd.MORbatchNum):
                    tData.select_mor(mb)
                    self.optimIter(tData, mb, loss_buf[i])
            # The reshuffle that follows this epoch (VarNetUtility.py:957-1017 at VarNet.py:1354) is prepared BEFORE the
            # loss is read back: its host work and gathers then run while the GPU is still busy with the epoch.  Safe:
            # engine and gathers share one stream (old buffers are reused in stream order), the NumPy draws keep their
            # order (no other consumer between the two points with uniform sampling).
            early_shuffle = (nblk == 1 and smpScheme == 'uniform' and shuffleData and epoch % shuffleFreq == 0)
            if early_shuffle:
                tData.shuffleTrainData()
            losses = loss_buf[:nblk].tolist()                        # one host sync per block (per epoch when lossLag = 0)
            if nblk > 1 and can_snap:
                hit = next((i for i in range(nblk - 1) if float(losses[i]) < tol), None)
                if hit is not None:
                    # the stopping test fires at epoch first + hit, inside the block: back to the block's start, then exactly the
                    # epochs the reference would have run (their losses are the ones already read)
                    eng.state_rollback()
                    scratch = torch.zeros(1, dtype=torch.float32, device=eng.device)
                    for i in range(hit + 1):
                        for mb in range(fd.MORbatchNum):
                            tData.select_mor(mb)
                            self.optimIter(tData, mb, scratch[0])
            blk_time = time.perf_counter() - t0
            first = epoch
            for i in range(nblk):
                epoch = first + i
                current_loss = float(losses[i])
                epoch_time += blk_time / nblk
                if shuffleData and epoch % shuffleFreq == 0 and not early_shuffle:
                    tData.shuffleTrainData()

                if epoch % saveFreq == 0:
                    if min_loss > current_loss:
                        min_loss = current_loss
                        self.saveModel(epoch)
                    resVal, _, err, _ = self.residual()
                    eng.set_weights([1.0, 1.0, 1.0])
                    if tData0 is not tData:
                        tData0.activate()
                    lossComp, _, lossVec = self.splitLoss(tData0)       # VarNet.py:1365
                    if tData0 is not tData:
                        tData.activate()
                    eng.set_weights(w_eff)
                    if self.tfAdapt is not None:
                        trainRes.tfAdaptHist.append((epoch, [eng.tf_adapt(tData.engine_batch(0, bi), arrays=False)['stats']
                                                             for bi in range(tData.batchNum)]))
                    if self.bicWeights is not None or self.bicAdapt is not None:
                        trainRes.bicAdaptHist.append((epoch, {p: eng.bic_adapt(p, arrays=False)['stats'] for p in eng.bic_parts()}))
                trainRes.iterOutput(epoch, current_loss, min_loss, epoch_time, resVal, err, lossComp, lossVec)

                if current_loss < tol:
                    trainRes.writeCase('Training completed!')
                    if verbose and self.rank == 0:
                        print('Training completed!')
                    done = True
                    break
                if self._is_lbfgs() and self._lbfgs_info['status'] != 0:
                    if self._lbfgs_info['status'] == 1:
                        trainRes.writeCase('epoch %d: L-BFGS line search found no acceptable step, history dropped '
                                           '(the next iteration is a steepest-descent one).' % epoch)
                    else:
                        msg = ('epoch %d: L-BFGS stalled (no acceptable step along the steepest-descent direction), '
                               'training ended.' % epoch)
                        trainRes.writeCase(msg)
                        if verbose and self.rank == 0:
                            print(msg)
                        done = True
                        break

                # regenerate the training set (VarNet.py:1385-1421)
                if smpScheme != 'uniform' and (multiTrainUpd or tp_updates == 0) and (epoch - tp_epoch) >= (trainUpdelay - 1):
                    t_loss = np.array(trainRes.loss[-5:])                # sampled every saveFreq epochs, as the reference
                    tp_conv = t_loss[:-1] - t_loss[1:]
                    tp_conv = np.sum(tp_conv[tp_conv > 0])
                    if len(t_loss) > 0 and tp_conv / t_loss[-1] < tolUpd:
                        min_loss = float('inf')
                        tp_epoch = epoch
                        tp_updates += 1
                        trainRes.inpIter.append(epoch)
                        tData = self._build_tdata(batchNum, batchLen, smpScheme, frac, addTrainPts, suppFactor)
                        self.tData = tData
                        msg = '\n\n==========================================================\nTraining points updated.\n\n'
                        if reinitrain:
                            self._init_params(tp_updates)               # global_variables_initializer, VarNet.py:1412
                            msg += 'trainable variables reinitialized.\n\n'
                        if self.tfAdapt is not None:                    # the new set's test functions are other ones
                            msg += 'self-adaptive test-function weights reset to their initial state.\n\n'
                            trainRes.tfAdaptHist.append((epoch, 'reset'))
                        if verbose and self.rank == 0:
                            print(msg)
                        trainRes.writeCase(msg)
                        if adjustWeight:
                            weight = [5 * wv for wv in weight[:-1]] + [weight[-1]]
                        trainW, w_eff, _ = set_train_weights(tData, weight)
                        if bal is not None:                          # the moving average restarts from the weights of the re-draw
                            bal_w, bal_w0, bal_active, bal_rho = balance_start(trainW, weight)
            epoch = first + nblk
        trainRes.flushPlots()
        for lv in self.LEARNT:
            data = getattr(self, lv.attr)
            if data is not None and self.rank == 0:
                scale = data.get('scale', 1.0)           # (coefficients are reported in the user's scale: `coefficients()`)
                trainRes.writeCase('%s: mask %s, initial %s, final %s\n'
                                   % (lv.title, data['mask'], [float(x) for x in data['init'] / scale],
                                      [float(x) for x in getattr(self.engine, 'get_' + lv.engine)() / scale]))
        return trainRes

    # -- checkpoints ----------------------------------------------------------------------------------
    # Checkpoint layout.  tf.train.Saver writes every global variable of the graph under its TF name
    # (TFModel.py:307; VarNet.py:1362): the Keras kernels / biases `dense_<i>/kernel` [in,out], `dense_<i>/bias`,
    # `output/kernel`, `output/bias` (TFModel.py:208-242), the Adam slots `<var>/Adam` (m) and `<var>/Adam_1` (v),
    # `beta1_power`, `beta2_power` and the step counter.  `best_model-<epoch>.npz` holds exactly those arrays under
    # those names (RMSProp: `<var>/RMSProp` = mean square, `<var>/RMSProp_1` = momentum), so a TF-side converter is a
    # loop over names.  TF's own files (`best_model-<n>.index/.meta/.data-*`) cannot be restored here -- reading them
    # needs TensorFlow -- and loadModel says so instead of reporting "nothing found" (Checkpoints).
    def _var_names(self):
        names = ['dense_%d' % i for i in range(len(self.layerWidth))] + ['output']
        return names

    def _init_params(self, seed):
        """init_params(seed), then the weight scales of `reparam` registered on the fresh parameters: rwf draws s_init from
        np.random.RandomState(seed).normal(mean, std, S), slope starts at s = 1 / n (f == 1)."""
        self.engine.init_params(seed=seed)
        rp = self.reparam
        if rp is None:
            return
        from .engine import reparam_count
        S = reparam_count(rp['kind'], rp['per'], self.inpDim, self.layerWidth)
        s_init = np.random.RandomState(seed).normal(rp['mean'], rp['std'], S) if rp['kind'] == 'rwf' else np.full(S, 1.0 / rp['n'])
        self.engine.set_reparam(rp['kind'], per=rp['per'], n=rp['n'], s_init=s_init, lr=self.reparamLr)

    def scales(self):
        """The per-layer arrays of f(s) of `reparam` (rwf: every layer, the output layer last; slope: the hidden layers), or None."""
        if self.reparam is None:
            return None
        from .engine import reparam_layers
        f = self.engine.get_reparam()['f']
        out, off = [], 0
        for n_ in reparam_layers(self.reparam['kind'], self.reparam['per'], self.layerWidth):
            out.append(f[off:off + n_].copy())
            off += n_
        return out

    def checkpoint_arrays(self):
        """{TF variable name: array} for the current engine state (see the layout note above)."""
        buf = np.asarray(self.engine.export_state(), dtype=np.uint8)
        step = int(buf[:8].view(np.int64)[0])
        P = self.engine.P
        flat = buf[8:].view(np.float32)
        theta, m, v = flat[:P], flat[P:2 * P], flat[2 * P:3 * P]
        slot = ('RMSProp_1', 'RMSProp') if str(self.optimizer).lower() == 'rmsprop' else ('Adam', 'Adam_1')
        out, off, fan = {}, 0, self.inpDim
        for name, h in zip(self._var_names(), self.layerWidth + [1]):
            for part, n, shp in (('kernel', fan * h, (fan, h)), ('bias', h, (h,))):
                key = '%s/%s' % (name, part)
                out[key] = theta[off:off + n].reshape(shp).copy()
                out[key + '/' + slot[0]] = m[off:off + n].reshape(shp).copy()
                out[key + '/' + slot[1]] = v[off:off + n].reshape(shp).copy()
                off += n
            fan = h
        out['global_step'] = np.int64(step)
        if slot[0] == 'Adam':
            out['beta1_power'] = np.float32(0.9 ** (step + 1))       # TF keeps beta^(t+1) for the next update
            out['beta2_power'] = np.float32(0.999 ** (step + 1))
        for lv in self.LEARNT:
            if getattr(self, lv.attr, None) is not None:
                # the values in the engine's scale (vn_get_*: the nine coefficients, the J source amplitudes, the J field amplitudes
                # with the diffusivity streams first); their Adam slots have no entry point and restart from zero
                out[lv.key] = np.asarray(getattr(self.engine, 'get_' + lv.engine)(), dtype=np.float64)
        if getattr(self.PDE, 'ansatz', None) is not None:
            out['ansatz'] = np.int64(1)                              # the parameters are those of N in c = A + B N
        if self.reparam is not None:
            # the TF-named kernels and biases above hold theta_eff (a saved model is a plain MLP); these restore the joint state
            st = self.engine.get_reparam()
            out['reparam_mode'] = np.array('%s/%s/%r' % (self.reparam['kind'], self.reparam['per'], self.reparam['n']))
            out['reparam_V'], out['reparam_s'], out['reparam_slots'] = st['V'], st['s'], st['slots']
        if getattr(self, 'tfAdapt', None) is not None:
            # (the parameters above are the first 3 P floats of the exported state whatever follows them)
            batches = self.engine.adapt_batches()
            out['tfadapt_rule'] = np.array(self.tfAdapt['rule'])
            out['tfadapt_batches'] = np.array(batches, dtype=np.int64)
            out.update(_adapt_arrays({'tfadapt_%d_' % b: self.engine.tf_adapt(b) for b in batches}))
        if getattr(self, 'bicAdapt', None) is not None:
            for part, spec in self.engine.bic_parts().items():
                if not isinstance(spec, dict):
                    continue
                out['bicadapt_%s_rule' % part] = np.array(spec['rule'])
                out.update(_adapt_arrays({'bicadapt_%s_' % part: self.engine.bic_adapt(part)}))
        return out

    def restore_arrays(self, arrays):
        """Inverse of `checkpoint_arrays`: load {TF variable name: array} into the engine."""
        has = getattr(self.PDE, 'ansatz', None) is not None
        if ('ansatz' in arrays) != has:
            raise ValueError('checkpoint %s an ansatz (c = A + B N) but the PDE of this model %s: the parameters of the one are not '
                             'a solution of the other!' % (('was trained with', 'has none') if not has else ('was trained without', 'has one')))
        mode = None if self.reparam is None else '%s/%s/%r' % (self.reparam['kind'], self.reparam['per'], self.reparam['n'])
        saved = str(arrays['reparam_mode']) if 'reparam_mode' in arrays else None
        if saved != mode or (mode is not None and np.size(arrays['reparam_s']) != np.size(self.engine.get_reparam()['s'])):
            raise ValueError('checkpoint was trained with reparam %s but this model has %s: the optimizer state of the one is not that '
                             'of the other!' % (saved, mode))
        slot = ('RMSProp_1', 'RMSProp') if str(self.optimizer).lower() == 'rmsprop' else ('Adam', 'Adam_1')
        th, m, v, fan = [], [], [], self.inpDim
        for name, h in zip(self._var_names(), self.layerWidth + [1]):
            for part, shp in (('kernel', (fan, h)), ('bias', (h,))):
                key = '%s/%s' % (name, part)
                if key not in arrays:
                    raise ValueError('checkpoint does not match the network architecture (no variable %s)!' % key)
                a = np.asarray(arrays[key], dtype=np.float32)
                if a.shape != shp:
                    raise ValueError('checkpoint does not match the network architecture (%s is %s, expected %s)!'
                                     % (key, a.shape, shp))
                th.append(a.reshape(-1))
                m.append(np.asarray(arrays.get(key + '/' + slot[0], np.zeros(shp)), dtype=np.float32).reshape(-1))
                dflt = np.ones(shp) if slot[1] == 'RMSProp' else np.zeros(shp)
                v.append(np.asarray(arrays.get(key + '/' + slot[1], dflt), dtype=np.float32).reshape(-1))
            fan = h
        step = np.array([int(arrays['global_step']) if 'global_step' in arrays else 0], dtype=np.int64)
        blob = np.concatenate([step.view(np.uint8), np.concatenate(th + m + v).astype(np.float32).view(np.uint8)])
        rule = None if getattr(self, 'tfAdapt', None) is None else self.tfAdapt['rule']
        saved_rule = str(arrays['tfadapt_rule']) if 'tfadapt_rule' in arrays else None
        bic_parts = self.engine.bic_parts() if hasattr(self.engine, 'bic_parts') else {}
        if rule is not None or bic_parts:
            # the adaptive states follow the optimizer state in the engine's layout: as they stand for the import, then (when the
            # checkpoint carries the rule's state for the registered batches) from the checkpoint
            blob = np.concatenate([blob, np.asarray(self.engine.export_state(), dtype=np.uint8)[blob.size:]])
        self.engine.import_state(blob)
        if rule is not None and saved_rule == rule:
            for b in [int(x) for x in arrays['tfadapt_batches']]:
                if b in self.engine.adapt_batches():
                    _adapt_put_back(arrays, 'tfadapt_%d_' % b, self.engine.set_tf_adapt_state, b, self.engine._n_k(b))
        for part, spec in bic_parts.items():
            key = 'bicadapt_%s_' % part
            if isinstance(spec, dict) and key + 'rule' in arrays and str(arrays[key + 'rule']) == spec['rule']:
                _adapt_put_back(arrays, key, self.engine.set_bic_adapt_state, part, self.engine.bic_rows(part))
        if mode is not None:
            self.engine.set_reparam_state(arrays['reparam_V'], arrays['reparam_s'], arrays['reparam_slots'])
        for lv in self.LEARNT:
            if getattr(self, lv.attr, None) is not None and lv.key in arrays:
                getattr(self.engine, 'set_' + lv.engine)(np.asarray(arrays[lv.key], dtype=np.float64).reshape(-1))

    def saveModel(self, epoch):
        """`saver.save(sess, 'best_model', global_step=epoch)` with max_to_keep=2 (TFModel.py:307,
        VarNet.py:1359-1362) -> `best_model-<epoch>.npz` + the `checkpoint` text file TF keeps beside it."""
        if self.rank != 0:
            return
        path = os.path.join(self.folderpath, 'best_model-%d.npz' % epoch)
        np.savez(path, **self.checkpoint_arrays())
        kept = getattr(self, '_ckpts', [])
        kept.append(path)
        while len(kept) > 2:
            old = kept.pop(0)
            if os.path.exists(old):
                os.remove(old)
        self._ckpts = kept
        self._write_checkpoint_file(self.folderpath, epoch, [int(os.path.basename(k)[len('best_model-'):-4]) for k in kept])

    @staticmethod
    def _write_checkpoint_file(folderpath, current, kept):
        with open(os.path.join(folderpath, 'checkpoint'), 'w') as f:
            f.write('model_checkpoint_path: ' + repr(os.path.join(folderpath, 'best_model-%d' % current)))
            for n in kept:
                f.write('\nall_model_checkpoint_paths: ' + repr(os.path.join(folderpath, 'best_model-%d' % n)))
            f.write('\n')

    def loadModel(self, iterNum=None, folderpath=None):
        """Restore the newest (or requested) `best_model-<n>` checkpoint (VarNet.py:1426-1506): without `iterNum`
        the stored iterations are tried newest first; the `checkpoint` file is rewritten to point at the restored
        one, as the reference does."""
        if self._towers is not None:
            if folderpath is None and hasattr(self, 'folderpath'):
                folderpath = self.folderpath
            return self._towers.call('loadModel', iterNum, folderpath)
        if folderpath is None:
            if not hasattr(self, 'folderpath'):
                raise ValueError('\'folderpath\' must be provided!')
            folderpath = self.folderpath
        else:
            self.folderpath = folderpath
            self.trainRes = TrainResult(folderpath)
            if os.path.exists(os.path.join(folderpath, 'trainData.vn')):
                self.trainRes.loadData()
        tf_only = []
        if iterNum is None:
            nums = []
            for f in os.listdir(folderpath):
                if f.startswith('best_model-') and f.endswith('.npz'):
                    nums.append(int(f[len('best_model-'):-4]))
                elif f.startswith('best_model-') and f.endswith('.index'):
                    tf_only.append(f)
            nums.sort(reverse=True)
        else:
            nums = [iterNum]
            if os.path.isfile(os.path.join(folderpath, 'best_model-%d.index' % iterNum)):
                tf_only.append('best_model-%d.index' % iterNum)
        for n in nums:
            path = os.path.join(folderpath, 'best_model-%d.npz' % n)
            if os.path.isfile(path):
                z = np.load(path)
                if 'state' in z.files:                               # files written by round-1 builds
                    if list(z['layerWidth']) != self.layerWidth or int(z['inpDim']) != self.inpDim:
                        raise ValueError('checkpoint does not match the network architecture!')
                    self.engine.import_state(z['state'])
                else:
                    self.restore_arrays({k: z[k] for k in z.files})
                if self.rank == 0:
                    self._write_checkpoint_file(folderpath, n, [n])
                return n
        if tf_only:
            raise ValueError('only TensorFlow saver files (%s ...) were found: they cannot be read without TensorFlow; '
                             'convert them to best_model-<n>.npz with the variable names of '
                             'VarNet.checkpoint_arrays() (INTEGRATION.md, "Checkpoints")' % tf_only[0])
        raise ValueError('no restorable checkpoint data found!')

    def saveNNparam(self, dpOut=False, matOut=False, verbose=False, timeFirst=False, path=None):
        """
        Trained kernels and biases per layer (VarNet.py:2179-2260): list of `[W, b]` with `W [out,in]`,
        `b [out,1]` so that `o = W i + b`; `timeFirst` moves the temporal input column in front of the
        spatial ones in the first layer.  `matOut` writes `NN_parameters/W<n>.mat, B<n>.mat` (MATLAB),
        `dpOut` the Diffpack-readable `W<n>.m, B<n>.m`; `path` additionally writes one `.npz`.
        """
        if self._towers is not None:
            return self._towers.call('saveNNparam', dpOut, matOut, verbose, timeFirst, path)
        flat = self.engine.get_params()
        td = self.PDE.timeDependent
        if not td:
            timeFirst = False
        folder = None
        if dpOut or matOut:
            folder = os.path.join(self.trainRes.folderpath, 'NN_parameters')
            os.makedirs(folder, exist_ok=True)
        layers, npz, off, fan = [], {}, 0, self.inpDim
        for l, h in enumerate(self.layerWidth + [1]):
            W = flat[off:off + fan * h].reshape(fan, h).T.copy()
            off += fan * h
            b = flat[off:off + h].reshape(h, 1).copy()
            off += h
            fan = h
            if l == 0 and timeFirst:
                dim = self.dim
                Wt = W.copy()
                W[:, 0] = Wt[:, dim]
                W[:, 1:dim + 1] = Wt[:, :dim]
            layers.append([W, b])
            npz['W%d' % l], npz['b%d' % l] = W.T.copy(), b[:, 0].copy()
            if verbose:
                print('Layer %d: weight %s, bias %s' % (l, W.shape, b.shape))
            if dpOut:
                uf.mat2diffpack(os.path.join(folder, 'W%d.m' % (l + 1)), 'W%d' % (l + 1), W)
                uf.mat2diffpack(os.path.join(folder, 'B%d.m' % (l + 1)), 'B%d' % (l + 1), b)
            if matOut:
                import scipy.io as spio
                spio.savemat(os.path.join(folder, 'W%d.mat' % (l + 1)), {'W%d' % (l + 1): W})
                spio.savemat(os.path.join(folder, 'B%d.mat' % (l + 1)), {'B%d' % (l + 1): b})
        if path is not None:
            np.savez(path, **npz)
        return layers

    # -- reporting --------------------------------------------------------------------------------------
    def simRes(self, batch=None, tcoord=None, plotpath=None, pltFrmt='png', plot=False):
        """
        Simulation results on the plotting grid (/root/reference/VarNet.py:1970-2175): for every time in `tcoord`
        (default 5 snapshots over the time interval) the fields the reference draws -- approximate solution `cApp`,
        exact solution `cEx` and error `cErr` (when the PDE has `cEx`), strong residual `res`, interpolated loss field
        `lossField` (when the last training run kept `lossVec`) -- as arrays: [51, 51] contour fields in 2D, curves on
        the 51-point x grid in 1D.  Returned as {'t': [...], 'grid': ContourPlot, 'cApp': [...], ..., 'l2Err': [...]}.
        With `plot=True` (and matplotlib present) the same figures are also written under `plotpath` with the
        reference's file names (cApp-t=0.00s.png, cEx-..., cErr-..., res-..., lossField-... / cApp.png, cErr.png,
        residual.png, lossField.png in 1D).
        """
        from .contour import ContourPlot
        if self._towers is not None:
            out = self._towers.call('simRes', batch, tcoord, plotpath, pltFrmt, plot)
            out['grid'] = ContourPlot(self.PDE.domain, self.PDE.tInterval if self.PDE.timeDependent else None)
            return out
        if not hasattr(self, 'trainRes') and uf.isnone(plotpath) and plot:
            raise ValueError('\'plotpath\' must be provided!')
        elif uf.isnone(plotpath) and hasattr(self, 'trainRes'):
            plotpath = self.trainRes.plotpath
        if pltFrmt not in ('png', 'jpg', 'pdf', 'eps'):
            raise ValueError('invalid plot format!')
        suffix = ('.' if uf.isnone(batch) else '-b=' + str(int(batch)) + '.') + pltFrmt
        dim, PDE = self.dim, self.PDE
        td, tInterval, cExact = PDE.timeDependent, PDE.tInterval, PDE.cEx
        if td and uf.isnone(tcoord):
            tcoord = np.linspace(tInterval[0], tInterval[1], num=5)
        elif not td:
            tcoord = [0.]
        if dim > 2:
            raise ValueError('simRes is available for 1D and 2D domains!')
        cp = ContourPlot(PDE.domain, tInterval if td else None)
        cAppFun = lambda x, t=None: self.evaluate(x, t, batch)

        def resFun(x, t=None):
            Input = np.concatenate([x, t * np.ones([len(x), 1])], axis=1) if td else x
            return self.residual(Input, None, batch)[1]

        cExFun = cErrFun = None
        if not uf.isnone(cExact):
            cExFun = (lambda x, t: cExact(x, t * np.ones([len(x), 1]))) if td else (lambda x, t=None: cExact(x))
            cErrFun = lambda x, t=None: cExFun(x, t) - cAppFun(x, t)
        lossFun = None
        lv = getattr(getattr(self, 'trainRes', None), 'lossVec', None)
        if not uf.isnone(lv) and len(lv) > 0:
            from scipy import interpolate
            lossVec = lv[0] if uf.isnone(batch) else lv[batch]
            ui = self.fixData.uniform_input
            if ui.shape[1] == 1:
                lossField = lambda X: np.interp(X[:, 0], ui[:, 0], np.reshape(lossVec, -1), left=0.0, right=0.0).reshape(-1, 1)
            else:
                lossField = interpolate.LinearNDInterpolator(ui, lossVec, fill_value=0.0)
            lossFun = lambda x, t=None: lossField(uf.hstack([x, t * np.ones([len(x), 1])]) if td else x)
        funs = {'cApp': cAppFun, 'cEx': cExFun, 'cErr': cErrFun, 'res': resFun, 'lossField': lossFun}
        out = {'t': [float(t) for t in tcoord], 'grid': cp, 'l2Err': []}
        for name, f in funs.items():
            if f is None:
                continue
            if dim == 1:
                out[name] = [np.asarray(cp.snap(f, float(t))[1], dtype=float).reshape(-1, 1) for t in tcoord]
            else:
                out[name] = [cp.field(f, float(t) if td else None) for t in tcoord]
        if cExFun is not None:
            out['l2Err'] = [uf.l2Err(e, a) for e, a in zip(out['cEx'], out['cApp'])]
        if plot:
            self._simres_figures(out, cp, plotpath, suffix)
        return out

    def _simres_figures(self, out, cp, plotpath, suffix):
        """Draw and save what simRes computed, with the reference's file names (VarNet.py:2066-2172)."""
        try:
            import matplotlib
            matplotlib.use('Agg')
            import matplotlib.pyplot as plt
        except ImportError:
            warnings.warn('matplotlib is not available: simRes figures are not written')
            return
        os.makedirs(plotpath, exist_ok=True)
        ts = out['t']
        if self.dim == 1:
            names = {'cErr': 'cErr', 'res': 'residual', 'lossField': 'lossField'}
            if 'cEx' in out:
                for i, t in enumerate(ts):
                    plt.figure()
                    plt.plot(cp.x_coord, out['cEx'][i], 'b')
                    plt.plot(cp.x_coord, out['cApp'][i], 'r')
                    plt.legend(['exact solution', 'approximate solution'])
                    plt.savefig(os.path.join(plotpath, 'cApp-' + 't={0:.2f}s'.format(t) + suffix), dpi=300)
                    plt.close()
            else:
                names['cApp'] = 'cApp'
            for key, fname in names.items():
                if key not in out:
                    continue
                plt.figure()
                for i, t in enumerate(ts):
                    plt.plot(cp.x_coord, out[key][i])
                plt.legend(['t={0:.2f}s'.format(t) for t in ts])
                plt.savefig(os.path.join(plotpath, fname + suffix), dpi=300)
                plt.close()
        else:
            for key in ('cApp', 'cEx', 'cErr', 'res', 'lossField'):
                if key not in out:
                    continue
                for i, t in enumerate(ts):
                    plt.figure()
                    c = plt.contourf(cp.xx, cp.yy, out[key][i])
                    plt.colorbar(c)
                    plt.axis('scaled')
                    plt.savefig(os.path.join(plotpath, key + '-' + 't={0:.2f}s'.format(t) + suffix), dpi=300)
                    plt.close()

    # -- evaluation -------------------------------------------------------------------------------------
    def _mor_columns(self, batch, n):
        fd = self.fixData
        if self.PDE.MORvar is None:
            return None, [], []
        biArg, inpArg, MORinp = self.MORargExtract(batch, fd.MORdiscArg)
        return np.tile(MORinp, [n, 1]), biArg, inpArg

    def evaluate(self, x=None, t=None, batch=None, MORarg=None):
        """NN approximation of the PDE solution at (x,t[,mu]) (VarNet.py:1510-1595) -> [n,1]."""
        if self._towers is not None:
            return self._towers.call('evaluate', x, t, batch, MORarg)
        dim, PDE, fd = self.dim, self.PDE, self.fixData
        td = PDE.timeDependent
        MORvar = PDE.MORvar
        if x is None:
            if (td and t is None) or not td:
                Input = fd.uniform_input
                dof = Input.shape[0]
            else:
                dof = fd.dof
                x = fd.uniform_input[:dof, :dim]                     # as the reference (VarNet.py:1545)
        elif shape(x)[1] != dim:
            raise ValueError('spatial coordinates dimension does not match domain!')
        else:
            dof = shape(x)[0]
        if td and t is not None and not (size(t) == 1 or shape(t)[0] == dof):
            raise ValueError('temporal discretrization does not match spatial discretization!')
        if td and t is not None and size(t) == 1:
            t = float(np.reshape(t, -1)[0]) * np.ones([dof, 1])
        if MORvar is not None and batch is None and MORarg is None:
            raise ValueError('batch number or argument values must be given for MOR!')
        if MORvar is not None and batch is None and shape(MORarg)[1] != self.inpDim - fd.feDim:
            raise ValueError('MOR argument dimension does not match the NN input size!')
        if MORvar is not None and batch is not None and batch > fd.MORbatchNum - 1:
            raise ValueError('requested batch number is higher than total available batches!')
        if x is not None:
            Input = np.concatenate([x, t], axis=1) if (td and t is not None) else x
        if MORvar is not None:
            if batch is None:
                MORarg = np.asarray(MORarg, dtype=float)
                if MORarg.shape[0] == 1:
                    MORarg = np.tile(MORarg, [dof, 1])
                Input = np.hstack([Input, MORarg])
            else:
                cols, _, _ = self._mor_columns(batch, Input.shape[0])
                Input = np.hstack([Input, cols])
        N = self.engine.forward(Input).cpu().numpy().astype(np.float64).reshape(-1, 1)
        if getattr(PDE, 'ansatz', None) is not None:                 # the constrained solution A + B N
            Xs = np.asarray(Input, dtype=np.float64)[:, :fd.feDim]
            return PDE.ansatz_values('A', Xs) + PDE.ansatz_values('B', Xs) * N
        return N

    def residual(self, Input=None, tDiscIND=None, batch=None, fp64=False):
        """
        Strong PDE residual norm on `uniform_input` (or `Input`) and, when an exact solution is
        known, the normalised l2 error (VarNet.py:1599-1692):
            res = sqrt(sum(resVec^2) * prod(hVec)), err = l2Err(cEx, cApp), averaged over MOR batches.
        Returns (res, resVec, err, cApp).
        """
        if self._towers is not None:
            return self._towers.call('residual', Input, tDiscIND, batch, fp64)
        dim, PDE, fd = self.dim, self.PDE, self.fixData
        td = PDE.timeDependent
        az = getattr(PDE, 'ansatz', None)
        if az is not None:
            # with c = A + B N the strong residual is composed from one forward_grad and one residual call with zero source:
            # R(c) = B R0(N) + [-A_t + kappa Lap A - (v - grad kappa) . grad A] + N [-B_t + kappa Lap B - (v - grad kappa) . grad B]
            #        + 2 kappa grad B . grad N + s
            need = [k for k in (('A_t', 'B_t') if td else ()) + ('lapA', 'lapB') if k not in az]
            if need:
                raise NotImplementedError('the strong residual of a PDE with an ansatz needs ansatz[%s] (the time derivatives and '
                                          'Laplacians of A and B): residual() and smpScheme=\'optimal\' are not available without them'
                                          % ', '.join(repr(k) for k in need))
            if any(getattr(PDE, k, None) is not None for k in ('reaction', 'nlflux', 'nldiff')):
                raise NotImplementedError('the strong residual of a PDE with an ansatz and a polynomial term is not built')
            if fp64:
                raise NotImplementedError('residual(fp64=True) with an ansatz: the fp64 composition is not built -- an fp32 result '
                                          'is never returned in its place')
        elemSize = np.prod(fd.hVec)
        nb = fd.MORbatchNum
        if batch is not None:
            if batch > nb - 1:
                raise ValueError('requested batch number is higher than total available batches!')
            batchRange, nb = range(batch, batch + 1), 1
        else:
            batchRange = range(nb)
        noInput = Input is None
        cEx = None
        if noInput:
            Input, cEx = fd.uniform_input, fd.cEx
        elif PDE.cEx is not None:
            cEx = PDE.cEx(Input[:, :dim], Input[:, dim:dim + 1]) if td else PDE.cEx(Input[:, :dim])
        targ = [Input[:, dim:dim + 1]] if td else []
        learnt_field = getattr(self, 'fldLearn', None) is not None       # kappa, v and grad kappa move with the amplitudes
        diff_dx = fd.d_diff if noInput and not learnt_field else self.diffGradData(Input)
        res, err = 0., (0. if PDE.cEx is not None else None)
        resVec = cApp = None
        for b in batchRange:
            if PDE.MORvar is None:
                if noInput and fd.uniform_inpData[0] is not None and getattr(self, 'srcLearn', None) is None and not learnt_field:
                    diff, vel, src = fd.uniform_inpData
                else:
                    diff, vel, src = self.PDEinpData(Input)
                Inp = Input
            else:
                cols, _, inpArg = self._mor_columns(b, Input.shape[0])
                diff, vel, src = self.PDEinpData(Input, inpArg)
                Inp = np.hstack([Input, cols])
            rkw = {}
            cur = self.coefficients() if getattr(self, 'coefLearn', None) is not None else None      # learnt: the current values
            if getattr(PDE, 'reaction', None) is not None:           # res += rate p(u)
                rkw['reaction'] = (self._reaction_rate(Input).reshape(-1), cur['reaction'] if cur else PDE.reactionCoef)
            if getattr(PDE, 'nlflux', None) is not None:             # res -= F'(u) w . grad u + F(u) div w
                w_rows, divw_rows = self._nlflux_field(Input)
                rkw['nlflux'] = (w_rows, cur['nlflux'] if cur else PDE.nlfluxCoef, divw_rows)
            if getattr(PDE, 'nldiff', None) is not None:             # div(kappa D(u) grad u); the advection stays v . grad u
                rkw['nldiff'] = cur['nldiff'] if cur else PDE.nldiffCoef
            if az is not None:
                n = Inp.shape[0]
                _, r0 = self.engine.residual(Inp, diff, vel, np.zeros(n), diff_dx)
                N, gN = self.engine.forward_grad(Inp)
                f64 = lambda a, cols: np.asarray(a.cpu().numpy() if hasattr(a, 'cpu') else a, dtype=np.float64).reshape(n, cols)
                r0, N, gN = f64(r0, 1), f64(N, 1), f64(gN, dim)
                kap, w = f64(diff, 1), f64(vel, dim) - f64(diff_dx, dim)
                Xs = np.asarray(Input, dtype=np.float64)[:, :fd.feDim]
                val = lambda k, cols=1: PDE.ansatz_values(k, Xs, cols)
                A, B, dA, dB = val('A'), val('B'), val('dA', dim), val('dB', dim)
                At, Bt = (val('A_t'), val('B_t')) if td else (0.0, 0.0)
                resVec = (B * r0 + (-At + kap * val('lapA') - (w * dA).sum(1, keepdims=True))
                          + N * (-Bt + kap * val('lapB') - (w * dB).sum(1, keepdims=True))
                          + 2.0 * kap * (dB * gN).sum(1, keepdims=True) + f64(src, 1))
                cApp = A + B * N
            else:
                u, r = self.engine.residual(Inp, diff, vel, src, diff_dx, fp64=fp64, **rkw)
                cApp = u.cpu().numpy().astype(np.float64).reshape(-1, 1)
                resVec = r.cpu().numpy().astype(np.float64).reshape(-1, 1)
            if PDE.cEx is not None:
                err += uf.l2Err(cEx, cApp)
            res += np.sqrt(np.sum(resVec ** 2) * elemSize)
        res = res / nb
        if PDE.cEx is not None:
            err = err / nb
        return res, resVec, err, cApp
