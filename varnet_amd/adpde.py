"""
Advection-diffusion(-reaction) PDE container: `ADPDE(domain, diff, vel, source, timeDependent, tInterval,
BCs, IC, cEx, MORvar, d_diff, reaction, nlflux, nldiff, periodic, sourceBasis, sourceAmp, diffBasis, diffAmp, d_diffBasis, velBasis,
velAmp, bcBasis, bcAmp, icBasis, icAmp, fluxBasis, fluxAmp, robinBasis, robinAmp, ansatz)` -- the reference's ADPDE.py:56-246 restated (plot helpers are out of scope).

    c_t = div(diff D(c) grad c) - vel . grad c - div(w F(c)) + source + rate * p(c),    a * dc/dn + b * c = g  on each edge,

with the optional polynomial reaction p(c) = c1 c + c2 c^2 + c3 c^3 (`reaction=(rate, [c1, c2, c3])`), the optional
polynomial flux F(c) = f1 c + f2 c^2 + f3 c^3 (`nlflux=(w, [f1, f2, f3])`) and the optional solution-dependent diffusivity
D(c) = d0 + d1 c + d2 c^2 (`nldiff=[d0, d1, d2]`; D = 1 without it); none has a reference counterpart, all are absent by default.
`periodic=[(bIndA, bIndB), ...]` ties boundary indicators in pairs (c and its normal derivative agree across each pair) instead
of giving them an [a, b, g]; it has no reference counterpart either.

Constants are wrapped into callables f(x[, t]) returning column arrays; every BC is normalised
to [a, b, g(x,t)] and classified Dirichlet / Neumann / Robin; with a `MOR` instance a lookup
table records which PDE callable each parametric function is.
"""
import numpy as np

from .utility import UF

uf = UF()


class ADPDE:
    """
    c_t = div(diff grad c) - vel . grad c + source + rate * (c1 c + c2 c^2 + c3 c^3),    a * dc/dn + b * c = g  on each edge.

    reaction=(rate, [c1, c2, c3]) adds the polynomial reaction term on the source side (first-order decay: (lam, [-1]);
    Fisher-KPP: (r, [1, -1]); Allen-Cahn: (1 / eps^2, [1, 0, -1])).  `rate` is a number or a callable f(x[, t]) returning a
    column, like `source`; a shorter coefficient list is zero-padded.  None (the default): no reaction term.

    nlflux=(w, [f1, f2, f3]) or (w, [f1, f2, f3], div_w) adds the conservative flux term -div(w F(c)), F(c) = f1 c + f2 c^2 +
    f3 c^3 (Burgers' equation: vel=0, nlflux=(1.0, [0, 0.5]); LWR traffic: (1.0, [1, -1])).  `w` is a number (1D), a list of
    `dim` numbers or a callable f(x[, t]) returning [n, dim], like `vel`.  `div_w` is an optional callable f(x[, t]) returning
    the divergence of w as a column; only the strong residual uses it, and without it the divergence is taken as zero: `w`
    must then be constant or divergence-free.  Inviscid problems (shocks) are the user's responsibility.  None: no flux term.

    nldiff=[d0, d1, d2] or ([d0, d1, d2], div_vel) makes the diffusion quasilinear: div(diff D(c) grad c) with D(c) = d0 + d1 c +
    d2 c^2 (porous medium c_t = Lap(c^2): diff=1, nldiff=[0, 2]; conductivity k0 (1 + b c): diff=k0, nldiff=[1, b]).  `diff`
    keeps its meaning as kappa(x, t); a shorter list is zero-padded, every entry is finite.  With the term the advection is
    integrated by parts onto the test function, -int c (vel . grad N + N div vel): `div_vel` is an optional callable f(x[, t])
    returning the divergence of vel as a column, and without it the divergence is taken as zero: `vel` must then be constant
    or divergence-free.  D(c) = 0 somewhere (degenerate diffusion) is allowed; D(c) < 0 is the user's responsibility.
    None (the default): no term, D = 1.

    periodic=[(bIndA, bIndB), ...] makes boundary indicator B the periodic image of indicator A: c(x_A) = c(x_A + s) and
    dc/dn(x_A) = dc/dn(x_A + s) with s the translation that maps edge A onto edge B.  `Domain1D`: the pair is (0, 1), in either
    order.  `PolygonDomain2D`: the two edges have equal length and opposite outward normals.  A paired indicator has no [a, b, g]:
    its `BCs` entry stays empty, and `BCtype` reports 'Periodic' for it.  None (the default): no pairs.

    sourceBasis=[phi_1, ..., phi_J] with sourceAmp=[a_1, ..., a_J] (default: zeros) makes the source `source + sum_j a_j phi_j`:
    every phi_j is a callable f(x[, t]) returning a column, evaluated like `source`; 1 <= J <= 64.  The amplitudes can be learnt
    from observations (`VarNet(..., learnSource=...)`: source identification); without that the sum is part of the source.

    diffBasis=[chi_1, ..., chi_Jk] with diffAmp=[...] (default: zeros) makes the diffusivity `diff + sum_j diffAmp_j chi_j`, and
    velBasis=[omega_1, ..., omega_Jv] with velAmp=[...] the velocity `vel + sum_j velAmp_j omega_j`.  A chi_j is a number or a
    callable f(x[, t]) returning a column, like `diff`; an omega_j is a number, a list of `dim` numbers or a callable returning
    [n, dim], like `vel`; Jk + Jv <= 32.  d_diffBasis=[grad chi_1, ...] follows the `d_diff` convention (numbers or callables
    returning [n, dim], default zero): only the strong residual uses it, so without it the chi_j must be constant for the residual
    to be right.  The amplitudes can be learnt from observations (`VarNet(..., learnField=...)`: field identification); without
    that the sums are part of `diffFun`, `velFun` and `d_diffFun`.  velBasis with nldiff is not supported.

    bcBasis=[(bInd, gamma_1), ..., (bInd, gamma_Jb)] with bcAmp=[...] (default: zeros) makes the Dirichlet value on boundary
    indicator bInd `g/beta + sum_j bcAmp_j gamma_j` over the entries of that indicator: every gamma_j is a callable f(x[, t])
    returning a column, evaluated like `g`, and counts on the rows of its own indicator only.  icBasis=[iota_1, ..., iota_Ji] with
    icAmp=[...] makes the initial condition `IC + sum_j icAmp_j iota_j`, every iota_j a callable f(x) evaluated like `IC`
    (time-dependent problems only).  Jb + Ji <= 64.  The amplitudes can be learnt from observations (`VarNet(..., learnBic=...)`:
    boundary data identification); without that the sums are part of the boundary and initial labels.

    fluxBasis=[(bInd, gamma_1), ..., (bInd, gamma_Jl)] with fluxAmp=[...] (default: zeros) makes the flux datum of the Neumann /
    Robin condition `a dc/dn + b c = g` on boundary indicator bInd `g/a + sum_j fluxAmp_j gamma_j`, and robinBasis=[(bInd, eta_1),
    ..., (bInd, eta_Jc)] with robinAmp=[...] makes its transfer coefficient `b/a + sum_j robinAmp_j eta_j`: every function is a
    callable f(x[, t]) returning a column, evaluated like `g`, and counts on the rows of its own indicator only (a robinBasis on a
    Neumann indicator, b = 0, is allowed).  Jl + Jc <= 64.  Both are data of the boundary-flux rows (`VarNet(..., fluxBC=True)`);
    the amplitudes can be learnt from observations (`VarNet(..., learnFluxBC=...)`: flux boundary identification), without that
    the sums are part of the rows' label and coefficient.

    ansatz={'A': f, 'B': f, 'dA': f, 'dB': f[, 'A_t': f, 'B_t': f, 'lapA': f, 'lapB': f]} imposes Dirichlet and initial data as
    hard constraints: the solution is written as c = A + B N with N the network output, A carrying the data and B vanishing where
    they must hold (A = IC(x), B = t: an exact initial state; A = g, B = 1 - x^2: exact Dirichlet walls on [-1, 1]).  'A' and 'B'
    are callables f(x[, t]) returning a column, 'dA' and 'dB' their spatial gradients [n, dim]; both gradients are checked against
    central differences at construction.  The four optional callables (time derivatives and Laplacians, columns) serve the strong
    residual only.  The data then hold to rounding at every epoch and their loss weights can be 0.  Not with model-order
    reduction.  None (the default): every condition is a penalty.
    """
    SRC_MAX = 64
    FLD_MAX = 32
    BIC_MAX = 64
    FBC_MAX = 64

    def __init__(self, domain, diff, vel, source=0.0, timeDependent=False, tInterval=None,
                 BCs=None, IC=None, cEx=None, MORvar=None, d_diff=None, reaction=None, nlflux=None, nldiff=None, periodic=None,
                 sourceBasis=None, sourceAmp=None, diffBasis=None, diffAmp=None, d_diffBasis=None, velBasis=None, velAmp=None,
                 bcBasis=None, bcAmp=None, icBasis=None, icAmp=None, fluxBasis=None, fluxAmp=None, robinBasis=None, robinAmp=None,
                 ansatz=None):
        # the reference ignores the `timeDependent` argument (ADPDE.py:108-109)
        timeDependent = tInterval is not None

        if not uf.isnumber(diff) and not callable(diff):
            raise ValueError('diffusivity field must be constant or callable!')
        if not uf.isnumber(vel) and not callable(vel):
            raise ValueError('velocity field must be constant or callable!')
        if not uf.isnumber(source) and not callable(source):
            raise ValueError('source function must be constant or callable!')
        if BCs is not None and not isinstance(BCs, list):
            raise ValueError('BCs must be empty or a list of [a, b, g(x,t)]!')
        if BCs is not None and len(BCs) != domain.bIndNum:
            raise ValueError('number of BCs does not match number of boundaries in domain!')
        if timeDependent and IC is None:
            raise ValueError('initial condition must be provided for time-dependent problems!')
        if cEx is not None and not callable(cEx):
            raise ValueError('exact solution must be a callable function!')
        if d_diff is not None and not uf.isnumber(d_diff) and not callable(d_diff):
            raise ValueError('diffusivity gradient must be constant or callable!')

        if reaction is not None:
            if not isinstance(reaction, (tuple, list)) or len(reaction) != 2:
                raise ValueError('reaction must be given as (rate, [c1, c2, c3])!')
            rate, coef = reaction
            if not uf.isnumber(rate) and not callable(rate):
                raise ValueError('reaction rate must be constant or callable!')
            try:
                coef = [float(c) for c in np.reshape(np.asarray(coef, dtype=float), -1)]
            except (TypeError, ValueError):
                raise ValueError('reaction coefficients must be a list of up to three numbers [c1, c2, c3]!')
            if not 1 <= len(coef) <= 3 or not np.all(np.isfinite(coef)):
                raise ValueError('reaction coefficients must be a list of up to three finite numbers [c1, c2, c3]!')
            if uf.isnumber(rate) and not np.isfinite(float(rate)):
                raise ValueError('reaction rate must be finite!')
            if MORvar is not None:
                raise NotImplementedError('a reaction term with model-order reduction is not supported: parametric reaction '
                                          'rates are out of scope (the rate stream is assembled once, for all parameter batches)')
            coef = coef + [0.0] * (3 - len(coef))

        if nlflux is not None:
            if not isinstance(nlflux, (tuple, list)) or len(nlflux) not in (2, 3):
                raise ValueError('nlflux must be given as (w, [f1, f2, f3]) or (w, [f1, f2, f3], div_w)!')
            fw, fcoef = nlflux[0], nlflux[1]
            fdiv = nlflux[2] if len(nlflux) == 3 else None
            if not callable(fw):
                try:
                    fw = np.reshape(np.asarray(fw, dtype=float), -1)
                except (TypeError, ValueError):
                    raise ValueError('nlflux field w must be a number, a list of `dim` numbers or callable!')
                if fw.size != domain.dim:
                    raise ValueError('nlflux field w must have one entry per space dimension (%d), got %d!' % (domain.dim, fw.size))
                if not np.all(np.isfinite(fw)):
                    raise ValueError('nlflux field w must be finite!')
            try:
                fcoef = [float(c) for c in np.reshape(np.asarray(fcoef, dtype=float), -1)]
            except (TypeError, ValueError):
                raise ValueError('nlflux coefficients must be a list of up to three numbers [f1, f2, f3]!')
            if not 1 <= len(fcoef) <= 3 or not np.all(np.isfinite(fcoef)):
                raise ValueError('nlflux coefficients must be a list of up to three finite numbers [f1, f2, f3]!')
            if fdiv is not None and not callable(fdiv):
                raise ValueError('nlflux divergence div_w must be callable (or left out: w constant or divergence-free)!')
            if MORvar is not None:
                raise NotImplementedError('a flux term with model-order reduction is not supported: a parametric field w is out of '
                                          'scope (the phi stream is assembled once, for all parameter batches)')
            fcoef = fcoef + [0.0] * (3 - len(fcoef))

        if nldiff is not None:
            if not isinstance(nldiff, (tuple, list, np.ndarray)) or len(nldiff) == 0:
                raise ValueError('nldiff must be given as [d0, d1, d2] or ([d0, d1, d2], div_vel)!')
            dcoef, ddiv = nldiff, None
            if isinstance(nldiff, (tuple, list)) and len(nldiff) == 2 and isinstance(nldiff[0], (tuple, list, np.ndarray)):
                dcoef, ddiv = nldiff
            try:
                dcoef = [float(c) for c in np.reshape(np.asarray(dcoef, dtype=float), -1)]
            except (TypeError, ValueError):
                raise ValueError('nldiff coefficients must be a list of up to three numbers [d0, d1, d2]!')
            if not 1 <= len(dcoef) <= 3 or not np.all(np.isfinite(dcoef)):
                raise ValueError('nldiff coefficients must be a list of up to three finite numbers [d0, d1, d2]!')
            if ddiv is not None and not callable(ddiv):
                raise ValueError('nldiff divergence div_vel must be callable (or left out: vel constant or divergence-free)!')
            if MORvar is not None:
                raise NotImplementedError('a solution-dependent diffusivity with model-order reduction is not supported: the psi '
                                          'stream of the advection is assembled once, for all parameter batches')
            dcoef = dcoef + [0.0] * (3 - len(dcoef))

        if periodic is not None:
            periodic = self._check_periodic(periodic, domain, BCs)
            if MORvar is not None:
                raise NotImplementedError('periodic boundaries with model-order reduction are not supported: the paired rows are '
                                          'assembled once, for all parameter batches, and carry no parameter inputs')

        if sourceBasis is None:
            if sourceAmp is not None:
                raise ValueError('sourceAmp is an option of sourceBasis=[phi_1, ..., phi_J]!')
        else:
            if not isinstance(sourceBasis, (list, tuple)) or len(sourceBasis) == 0:
                raise ValueError('sourceBasis must be a non-empty list of callables [phi_1, ..., phi_J]!')
            if len(sourceBasis) > self.SRC_MAX:
                raise ValueError('sourceBasis holds %d functions, at most %d are supported!' % (len(sourceBasis), self.SRC_MAX))
            for j, f in enumerate(sourceBasis):
                if not callable(f):
                    raise ValueError('sourceBasis[%d] must be callable, like a source function!' % j)
            if sourceAmp is None:
                sourceAmp = np.zeros(len(sourceBasis))
            try:
                sourceAmp = np.array(np.reshape(np.asarray(sourceAmp, dtype=float), -1))
            except (TypeError, ValueError):
                raise ValueError('sourceAmp must be a list of %d numbers, one per function of sourceBasis!' % len(sourceBasis))
            if sourceAmp.size != len(sourceBasis):
                raise ValueError('sourceAmp holds %d values for the %d functions of sourceBasis!' % (sourceAmp.size, len(sourceBasis)))
            if not np.all(np.isfinite(sourceAmp)):
                raise ValueError('sourceAmp must be finite!')
            if MORvar is not None:
                raise NotImplementedError('a source basis with model-order reduction is not supported: parametric basis functions '
                                          'are out of scope (the basis streams are assembled once, for all parameter batches)')
            sourceBasis = list(sourceBasis)

        dim = domain.dim

        def const_field(val, ncol):
            return lambda x, t=0: val * np.ones([np.shape(x)[0], ncol])

        diffBasis, diffAmp = self._check_field_basis('diffBasis', 'diffAmp', diffBasis, diffAmp, MORvar, 1, const_field)
        velBasis, velAmp = self._check_field_basis('velBasis', 'velAmp', velBasis, velAmp, MORvar, dim, const_field)
        if d_diffBasis is not None and diffBasis is None:
            raise ValueError('d_diffBasis is an option of diffBasis=[chi_1, ..., chi_J]!')
        if diffBasis is not None:
            if d_diffBasis is None:
                d_diffBasis = [None] * len(diffBasis)
            if not isinstance(d_diffBasis, (list, tuple)) or len(d_diffBasis) != len(diffBasis):
                raise ValueError('d_diffBasis must be a list of %d entries, one gradient per function of diffBasis!' % len(diffBasis))
            d_diffBasis, _ = self._check_field_basis('d_diffBasis', 'diffAmp', [0.0 if f is None else f for f in d_diffBasis], None,
                                                     MORvar, dim, const_field)
        if (0 if diffBasis is None else len(diffBasis)) + (0 if velBasis is None else len(velBasis)) > self.FLD_MAX:
            raise ValueError('diffBasis and velBasis hold %d functions together, at most %d are supported!'
                             % (len(diffBasis or []) + len(velBasis or []), self.FLD_MAX))
        if velBasis is not None and nldiff is not None:
            raise NotImplementedError('velBasis with nldiff is not supported: with a solution-dependent diffusivity the advection lives '
                                      'in the psi stream on the value side, which carries no basis; diffBasis with nldiff works')

        if callable(diff):
            self.diffFun = diff
        else:
            self.diff = diff
            self.diffFun = const_field(diff, 1)
        if callable(vel):
            self.velFun = vel
        else:
            self.vel = vel
            self.velFun = const_field(np.asarray(vel, dtype=float), dim)
        if callable(source):
            self.sourceFun = source
        else:
            self.source = source
            self.sourceFun = const_field(source, 1)
        if callable(d_diff):
            self.d_diffFun = d_diff
        else:
            d_diff = 0.0 if d_diff is None else d_diff
            self.d_diff = d_diff
            self.d_diffFun = const_field(np.asarray(d_diff, dtype=float), dim)

        # field bases: the callables and their amplitudes (the initial guess when they are learnt); no attributes without one.
        # diffFun, velFun and d_diffFun become the sums at the PDE's amplitudes, the plain fields stay in diffFun0, velFun0, d_diffFun0
        if diffBasis is not None:
            self.diffBasis, self.diffAmp, self.d_diffBasis = diffBasis, diffAmp, d_diffBasis
            self.diffFun0, self.d_diffFun0 = self.diffFun, self.d_diffFun
            self.diffFun = lambda x, *t: self._field_sum(self.diffFun0, self.diffBasis, self.diffAmp, 'diffBasis', 1, x, t)
            self.d_diffFun = lambda x, *t: self._field_sum(self.d_diffFun0, self.d_diffBasis, self.diffAmp, 'd_diffBasis', dim, x, t)
        if velBasis is not None:
            self.velBasis, self.velAmp = velBasis, velAmp
            self.velFun0 = self.velFun
            self.velFun = lambda x, *t: self._field_sum(self.velFun0, self.velBasis, self.velAmp, 'velBasis', dim, x, t)

        # reaction term: rate as a callable like the source, the three coefficients; None without one
        self.reaction = None
        if reaction is not None:
            if callable(rate):
                self.reactionRate = None
                self.reactionRateFun = rate
            else:
                self.reactionRate = float(rate)
                self.reactionRateFun = const_field(float(rate), 1)
            self.reactionCoef = coef
            self.reaction = (rate, coef)

        # flux term -div(w F(c)): w as a callable like the velocity, the three coefficients, the optional divergence; None without one
        self.nlflux = None
        if nlflux is not None:
            if callable(fw):
                self.nlfluxW = None
                self.nlfluxWFun = fw
            else:
                self.nlfluxW = fw
                self.nlfluxWFun = const_field(fw, dim)
            self.nlfluxCoef = fcoef
            self.nlfluxDivFun = fdiv
            self.nlflux = (nlflux[0], fcoef) if fdiv is None else (nlflux[0], fcoef, fdiv)

        # solution-dependent diffusivity D(c) = d0 + d1 c + d2 c^2: the three coefficients, the optional divergence of vel; None without
        self.nldiff = None
        if nldiff is not None:
            self.nldiffCoef = dcoef
            self.nldiffDivFun = ddiv
            self.nldiff = dcoef if ddiv is None else (dcoef, ddiv)

        # boundary conditions -> [a, b, g]
        bIndNum = domain.bIndNum
        if BCs is None:
            BCs = [[] for _ in range(bIndNum)]
        BCs = list(BCs)
        # Reference quirk kept for parity (ADPDE.py:180-182): the lambda wrapping a constant g
        # closes over a loop variable, so when several BCs carry constant values ALL of them
        # evaluate to the value of the LAST constant BC in the list.
        last_const = {}
        for bInd in range(bIndNum):
            bc = BCs[bInd]
            if uf.isempty(bc):
                BCs[bInd] = [0.0, 1.0, lambda x, t=0: np.zeros([len(x), 1])]
            elif len(bc) != 3:
                raise ValueError('BCs must be specified as a list of [a, b, g(x,t)]!')
            elif not callable(bc[2]):
                last_const['g'] = bc[2]
                BCs[bInd] = [bc[0], bc[1], lambda x, t=0: last_const['g'] * np.ones([len(x), 1])]
        paired = set() if periodic is None else {b for pair in periodic for b in pair}
        BCtype = []
        for bInd in range(bIndNum):
            if bInd in paired:
                BCtype.append('Periodic')
            elif BCs[bInd][0] == 0:
                BCtype.append('Dirichlet')
            elif BCs[bInd][1] == 0:
                BCtype.append('Neumann')
            else:
                BCtype.append('Robin')

        if timeDependent and uf.isempty(IC):
            IC = lambda x, t=0: np.zeros([len(x), 1])
        elif timeDependent and not callable(IC):
            ICval = IC
            IC = lambda x, t=0: ICval * np.ones([len(x), 1])

        # MOR lookup table (ADPDE.py:200-236)
        if MORvar is not None:
            BCind = [None] * bIndNum
            bDataFlg = False
            tab = {'diff': None, 'vel': None, 'source': None, 'IC': None, 'd_diff': None}
            for i, fh in enumerate(MORvar.funcHandles):
                if fh == self.diffFun:
                    tab['diff'] = i
                elif fh == self.velFun:
                    tab['vel'] = i
                elif fh == self.sourceFun:
                    tab['source'] = i
                elif fh == IC:
                    tab['IC'] = i
                elif fh == self.d_diffFun:
                    tab['d_diff'] = i
                else:
                    for bInd in range(bIndNum):
                        if fh == BCs[bInd][2]:
                            BCind[bInd] = i
                            bDataFlg = True
            if tab['diff'] is not None and callable(d_diff) and tab['d_diff'] is None:
                raise ValueError('\'diff\' has extra input arguments but \'d_diff\' does not!')
            tab['BCs'] = BCind
            inp = any(tab[k] is not None for k in ('diff', 'vel', 'source'))
            tab['inpData'] = True if inp else None
            tab['biData'] = True if (bDataFlg or tab['IC'] is not None) else None
            self.MORfunInd = tab

        self.dim = dim
        self.domain = domain
        self.timeDependent = timeDependent
        self.tInterval = tInterval
        self.BCs = BCs
        self.BCtype = BCtype
        self.IC = IC
        self.cEx = cEx
        self.MORvar = MORvar
        self.periodic = periodic
        # source basis: the J callables and their amplitudes (the initial guess when they are learnt); no attributes without one
        if sourceBasis is not None:
            self.sourceBasis = sourceBasis
            self.sourceAmp = sourceAmp
        # boundary and initial bases: likewise ((bInd, callable) pairs for the Dirichlet data)
        bcBasis, bcAmp = self._check_bic_basis('bcBasis', 'bcAmp', bcBasis, bcAmp, MORvar, True)
        icBasis, icAmp = self._check_bic_basis('icBasis', 'icAmp', icBasis, icAmp, MORvar, False)
        if len(bcBasis or []) + len(icBasis or []) > self.BIC_MAX:
            raise ValueError('bcBasis and icBasis hold %d functions together, at most %d are supported!'
                             % (len(bcBasis or []) + len(icBasis or []), self.BIC_MAX))
        if bcBasis is not None:
            self.bcBasis, self.bcAmp = bcBasis, bcAmp
        if icBasis is not None:
            self.icBasis, self.icAmp = icBasis, icAmp
        # flux-datum and Robin-coefficient bases: likewise, on the Neumann / Robin indicators
        fluxBasis, fluxAmp = self._check_fbc_basis('fluxBasis', 'fluxAmp', fluxBasis, fluxAmp, MORvar)
        robinBasis, robinAmp = self._check_fbc_basis('robinBasis', 'robinAmp', robinBasis, robinAmp, MORvar)
        if len(fluxBasis or []) + len(robinBasis or []) > self.FBC_MAX:
            raise ValueError('fluxBasis and robinBasis hold %d functions together, at most %d are supported!'
                             % (len(fluxBasis or []) + len(robinBasis or []), self.FBC_MAX))
        if fluxBasis is not None:
            self.fluxBasis, self.fluxAmp = fluxBasis, fluxAmp
        if robinBasis is not None:
            self.robinBasis, self.robinAmp = robinBasis, robinAmp
        # hard-constraint ansatz c = A + B N: the dict of callables; no attribute without one
        if ansatz is not None:
            self.ansatz = self._check_ansatz(ansatz, MORvar)

    ANSATZ_KEYS = ('A', 'B', 'dA', 'dB')
    ANSATZ_OPTIONAL = ('A_t', 'B_t', 'lapA', 'lapB')

    def ansatz_values(self, key, X, ncol=1):
        """The ansatz callable `key` at the rows X = [x, t] (t: time-dependent problems) as an fp64 [n, ncol] array."""
        X = np.asarray(X, dtype=np.float64)
        targ = [X[:, self.dim:self.dim + 1]] if self.timeDependent else []
        v = np.asarray(self.ansatz[key](X[:, :self.dim], *targ), dtype=np.float64)
        if v.size != X.shape[0] * ncol:
            raise ValueError('ansatz[%r] must return %s per point, got shape %s for %d points'
                             % (key, 'one value' if ncol == 1 else '%d values' % ncol, v.shape, X.shape[0]))
        v = v.reshape(X.shape[0], ncol)
        if not np.all(np.isfinite(v)):
            raise ValueError('ansatz[%r] must be finite on the domain!' % key)
        return v

    def _check_ansatz(self, ansatz, MORvar):
        if not isinstance(ansatz, dict):
            raise ValueError('ansatz must be a dict of callables with the keys \'A\', \'B\', \'dA\', \'dB\' '
                             '(and optionally \'A_t\', \'B_t\', \'lapA\', \'lapB\')!')
        unknown = sorted(set(ansatz) - set(self.ANSATZ_KEYS) - set(self.ANSATZ_OPTIONAL), key=str)
        if unknown:
            raise ValueError('ansatz has unknown keys %s!' % unknown)
        for k in self.ANSATZ_KEYS:
            if not callable(ansatz.get(k)):
                raise ValueError('ansatz[%r] must be a callable f(x[, t])!' % k)
        for k in self.ANSATZ_OPTIONAL:
            if k in ansatz and not callable(ansatz[k]):
                raise ValueError('ansatz[%r] must be a callable f(x[, t]) (or left out)!' % k)
        if MORvar is not None:
            raise NotImplementedError('an ansatz with model-order reduction is not supported: parametric A and B are out of scope')
        self.ansatz = dict(ansatz)                   # (ansatz_values reads it during the check below)
        try:
            return self._check_ansatz_gradients()
        except Exception:
            del self.ansatz
            raise

    def _check_ansatz_gradients(self):
        # dA, dB against fp64 central differences of A, B at 64 seeded points of the domain: a wrong gradient would train another
        # PDE without any sign of it
        dim, lim = self.dim, np.asarray(self.domain.lim, dtype=np.float64).reshape(2, -1)
        rng = np.random.default_rng(0)
        x = lim[0] + (lim[1] - lim[0]) * rng.uniform(0.05, 0.95, (4096, dim))
        inside = np.reshape(self.domain.isInside(x), -1).astype(bool)
        x = (x[inside] if inside.sum() >= 64 else x)[:64]
        X = x
        if self.timeDependent:
            t0, t1 = float(self.tInterval[0]), float(self.tInterval[1])
            X = np.hstack([x, t0 + (t1 - t0) * rng.uniform(0.05, 0.95, (x.shape[0], 1))])
        h = 1e-5 * np.maximum(lim[1] - lim[0], 1e-300)
        for f, df in (('A', 'dA'), ('B', 'dB')):
            g = self.ansatz_values(df, X, dim)
            fd = np.zeros_like(g)
            for d in range(dim):
                Xp, Xm = X.copy(), X.copy()
                Xp[:, d] += h[d]
                Xm[:, d] -= h[d]
                fd[:, d] = (self.ansatz_values(f, Xp)[:, 0] - self.ansatz_values(f, Xm)[:, 0]) / (2.0 * h[d])
            scale = max(float(np.max(np.abs(fd))), float(np.max(np.abs(g))), 1e-300)
            err = float(np.max(np.abs(g - fd))) / scale
            if err > 1e-6:
                raise ValueError('ansatz[%r] is not the spatial gradient of ansatz[%r]: it deviates from central differences by '
                                 '%.3g of its size at 64 points of the domain (tolerance 1e-6)!' % (df, f, err))
        return self.ansatz

    def _check_basis(self, name, ampName, basis, amp, MORvar, cap, shape_text, entry, hint='[...]'):
        """(checked entries, amplitudes) of one basis option, or (None, None) without one; ValueError names the option.  The basis is
        a non-empty list (`shape_text` says of what) of at most `cap` entries; `entry(j, e)` checks entry j and returns what is kept
        of it; the amplitudes default to zeros."""
        if basis is None:
            if amp is not None:
                raise ValueError('%s is an option of %s=%s!' % (ampName, name, hint))
            return None, None
        if not isinstance(basis, (list, tuple)) or len(basis) == 0:
            raise ValueError('%s must be a non-empty list %s!' % (name, shape_text))
        if len(basis) > cap:
            raise ValueError('%s holds %d functions, at most %d are supported!' % (name, len(basis), cap))
        out = [entry(j, e) for j, e in enumerate(basis)]
        if amp is None:
            amp = np.zeros(len(out))
        try:
            amp = np.array(np.reshape(np.asarray(amp, dtype=float), -1))
        except (TypeError, ValueError):
            raise ValueError('%s must be a list of %d numbers, one per function of %s!' % (ampName, len(out), name))
        if amp.size != len(out):
            raise ValueError('%s holds %d values for the %d functions of %s!' % (ampName, amp.size, len(out), name))
        if not np.all(np.isfinite(amp)):
            raise ValueError('%s must be finite!' % ampName)
        if MORvar is not None:
            raise NotImplementedError('%s with model-order reduction is not supported: parametric basis functions are out of scope '
                                      '(the basis streams are assembled once, for all parameter batches)' % name)
        return out, amp

    def _edge_entry(self, name, sym, fun, refused, only):
        """The entry check of a basis on boundary indicators (bcBasis, fluxBasis, robinBasis): a pair (bInd, callable) whose
        indicator is not periodic and carries no condition among `refused`.  `sym` and `fun` name the callable, `only` says which
        data has such a basis.  Used at the end of __init__: BCtype and periodic are set."""
        def entry(j, e):
            if not isinstance(e, (list, tuple)) or len(e) != 2 or isinstance(e[0], bool) or not isinstance(e[0], (int, np.integer)):
                raise ValueError('%s[%d] must be a pair (bInd, %s) of a boundary indicator and a callable!' % (name, j, sym))
            bInd, f = int(e[0]), e[1]
            if not callable(f):
                raise ValueError('%s[%d]: %s must be callable, like the g of a boundary condition!' % (name, j, fun))
            if not 0 <= bInd < self.domain.bIndNum:
                raise ValueError('%s[%d]: boundary indicator %d outside [0, %d)!' % (name, j, bInd, self.domain.bIndNum))
            if self.BCtype[bInd] == 'Periodic':
                raise ValueError('%s[%d]: boundary indicator %d is paired by `periodic`, it carries no boundary data!' % (name, j, bInd))
            if self.BCtype[bInd] in refused:
                raise ValueError('%s[%d]: boundary indicator %d carries a %s condition, %s!' % (name, j, bInd, self.BCtype[bInd], only))
            return bInd, f
        return entry

    def _check_fbc_basis(self, name, ampName, basis, amp, MORvar):
        """fluxBasis / robinBasis: (bInd, callable) pairs on the Neumann and Robin indicators."""
        return self._check_basis(name, ampName, basis, amp, MORvar, self.FBC_MAX, '[(bInd, f_1), ..., (bInd, f_J)]',
                                 self._edge_entry(name, 'f', 'the function', ('Dirichlet',),
                                                  'only Neumann and Robin data has a flux basis (bcBasis is the Dirichlet one)'))

    def _check_bic_basis(self, name, ampName, basis, amp, MORvar, edges):
        """bcBasis (`edges`: (bInd, callable) pairs on the Dirichlet indicators) / icBasis (callables, of a time-dependent problem)."""
        if edges:
            return self._check_basis(name, ampName, basis, amp, MORvar, self.BIC_MAX, '[(bInd, gamma_1), ..., (bInd, gamma_J)]',
                                     self._edge_entry(name, 'gamma', 'gamma', ('Neumann', 'Robin'), 'only Dirichlet data has a basis'))

        def entry(j, e):
            if not self.timeDependent:
                raise ValueError('icBasis needs a time-dependent problem: a steady problem has no initial condition!')
            if not callable(e):
                raise ValueError('icBasis[%d] must be callable, like an initial condition!' % j)
            return e
        return self._check_basis(name, ampName, basis, amp, MORvar, self.BIC_MAX, '[iota_1, ..., iota_J]', entry)

    def _check_field_basis(self, name, ampName, basis, amp, MORvar, ncol, const_field):
        """diffBasis / velBasis / d_diffBasis: an entry is a number, a list of `ncol` numbers (ncol > 1) or a callable, and is kept
        as a callable."""
        def entry(j, f):
            if callable(f):
                return f
            try:
                v = np.reshape(np.asarray(f, dtype=float), -1)
            except (TypeError, ValueError):
                v = np.empty(0)
            if isinstance(f, bool) or v.size not in (1, ncol) or not np.all(np.isfinite(v)):
                raise ValueError('%s[%d] must be callable, a finite number%s!'
                                 % (name, j, '' if ncol == 1 else ' or a list of %d finite numbers' % ncol))
            return const_field(v if v.size == ncol else float(v[0]), ncol)
        return self._check_basis(name, ampName, basis, amp, MORvar, self.FLD_MAX, 'of numbers or callables [f_1, ..., f_J]', entry,
                                 hint='[f_1, ..., f_J]')

    @staticmethod
    def field_basis_values(basis, name, ncol, x, t=()):
        """The functions of one field basis at the points x (and times t): [J, n, ncol] in fp64; a wrong shape names the entry."""
        n = np.shape(x)[0]
        out = np.empty((len(basis), n, ncol), dtype=np.float64)
        for j, f in enumerate(basis):
            v = np.asarray(f(x, *t), dtype=np.float64)
            if v.size != n * ncol:
                raise ValueError('%s[%d] must return %s per point, got shape %s for %d points'
                                 % (name, j, 'one value (a column)' if ncol == 1 else '%d values ([n, %d])' % (ncol, ncol), v.shape, n))
            out[j] = v.reshape(n, ncol)
        return out

    def _field_sum(self, base, basis, amp, name, ncol, x, t):
        """base + sum_j amp_j f_j at the points x: what diffFun, velFun and d_diffFun return when the PDE has a basis."""
        v = np.asarray(base(x, *t), dtype=np.float64).reshape(-1, ncol)
        return v + np.tensordot(np.asarray(amp, dtype=np.float64), self.field_basis_values(basis, name, ncol, x, t), axes=1)

    @staticmethod
    def _check_periodic(periodic, domain, BCs):
        """The pairs as a list of (A, B) integer tuples, or ValueError: indices in range and distinct, every indicator in at most
        one pair, no [a, b, g] on a paired indicator, and edges that are translates of each other."""
        if not isinstance(periodic, (list, tuple)) or len(periodic) == 0:
            raise ValueError('periodic must be a non-empty list of boundary indicator pairs [(bIndA, bIndB), ...]!')
        nb = domain.bIndNum
        pairs, seen = [], set()
        for pair in periodic:
            if not isinstance(pair, (list, tuple)) or len(pair) != 2 or \
                    not all(isinstance(b, (int, np.integer)) and not isinstance(b, bool) for b in pair):
                raise ValueError('periodic must be a non-empty list of boundary indicator pairs [(bIndA, bIndB), ...]!')
            A, B = int(pair[0]), int(pair[1])
            for b in (A, B):
                if not 0 <= b < nb:
                    raise ValueError('periodic pair (%d, %d): boundary indicator %d outside [0, %d)!' % (A, B, b, nb))
            if A == B:
                raise ValueError('periodic pair (%d, %d): the two boundary indicators must be distinct!' % (A, B))
            for b in (A, B):
                if b in seen:
                    raise ValueError('periodic pair (%d, %d): boundary indicator %d appears in more than one pair!' % (A, B, b))
                seen.add(b)
            if BCs is not None:
                for b in (A, B):
                    if not uf.isempty(BCs[b]):
                        raise ValueError('periodic pair (%d, %d): BCs[%d] must be empty, a periodic edge has no [a, b, g]!' % (A, B, b))
            if domain.dim == 1:
                if {A, B} != {0, 1}:                # (unreachable while Domain1D has two indicators; kept for the message)
                    raise ValueError('periodic pair (%d, %d): a 1D domain pairs its two ends, (0, 1)!' % (A, B))
            else:
                if A >= domain.vertexNum or B >= domain.vertexNum:
                    raise ValueError('periodic pair (%d, %d): obstacle edges cannot be paired!' % (A, B))
                g = np.asarray(domain.boundryGeom, dtype=float)
                lA, lB = np.linalg.norm(g[A, 1] - g[A, 0]), np.linalg.norm(g[B, 1] - g[B, 0])
                if abs(lA - lB) > 1e-12 * max(lA, lB):
                    raise ValueError('periodic pair (%d, %d): edges %d and %d have unequal lengths (%.17g and %.17g), they are '
                                     'not translates of each other!' % (A, B, A, B, lA, lB))
                n = np.asarray(domain.boundaryNormals(), dtype=float)
                if np.max(np.abs(n[A] + n[B])) > 1e-12:
                    raise ValueError('periodic pair (%d, %d): the outward normals of edges %d and %d are not opposite (%s and %s), '
                                     'they are not translates of each other!' % (A, B, A, B, n[A], n[B]))
            pairs.append((A, B))
        return pairs
