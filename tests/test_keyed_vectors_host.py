"""
CPU tier of the keyed learnt vectors (`learnField`, `learnBic`, `learnFluxBC`): the three option parsers are one function taking a
table row, so every kind must parse the same selections into the same arrays and refuse the same mistakes in the same sentences,
up to its own names.  Each case below is written once, with placeholders for the names, and run for every kind.  No engine.
"""
import re
import types

import numpy as np
import pytest

from varnet_amd.varnet import VarNet

# kind -> (parser, option, Lr name, Bounds name, the two keys, the two size entries of the parsed dict)
KINDS = {
    'field': ('fieldLearnData', 'learnField', 'fieldLr', 'fieldBounds', ('diff', 'vel'), ('Jk', 'Jv')),
    'bic': ('bicLearnData', 'learnBic', 'bicLr', 'bicBounds', ('bc', 'ic'), ('Jb', 'Ji')),
    'fluxbc': ('fluxBCLearnData', 'learnFluxBC', 'fluxBCLr', 'fluxBCBounds', ('flux', 'robin'), ('Jl', 'Jc')),
}
A0, A1 = [0.5, -1.0], [2.0, 0.25]
INF = np.inf


class Kind:
    def __init__(self, kind):
        parser, self.option, self.lr, self.bounds, self.keys, self.sizes = KINDS[kind]
        self.parser = getattr(VarNet, parser)

    def pde(self, first=True, second=True):
        """A PDE with two functions (the parser reads only their number) and the amplitudes A0 / A1 for each basis it has."""
        f = lambda *a: None
        d = {}
        for key, has, amp in zip(self.keys, (first, second), (A0, A1)):
            if has:
                d[key + 'Basis'], d[key + 'Amp'] = [f, f], list(amp)
        return types.SimpleNamespace(**d)

    def named(self, d):
        """{'K0': ..., 'K1': ...} with this kind's keys (any other key stays); whatever is no dict passes through."""
        return d if not isinstance(d, dict) else {dict(K0=self.keys[0], K1=self.keys[1]).get(k, k): v for k, v in d.items()}

    def parse(self, pde, learn, lr=None, bounds=None, **kw):
        return self.parser(pde, self.named(learn), lr, self.named(bounds), **kw)

    def sentence(self, pde, learn, lr=None, bounds=None):
        """The ValueError of a refused call, with this kind's names replaced by OPT, LR, BOUNDS, K0 and K1."""
        with pytest.raises(ValueError) as e:
            self.parse(pde, learn, lr, bounds)
        s = str(e.value)
        for name, tag in ((self.option, 'OPT'), (self.lr, 'LR'), (self.bounds, 'BOUNDS')):
            s = s.replace(name, tag)
        for key, tag in zip(self.keys, ('K0', 'K1')):
            s = re.sub(r'\b%s(Basis)?\b' % key, tag + r'\1', s)
        return s


@pytest.fixture(params=sorted(KINDS))
def k(request):
    return Kind(request.param)


def check(k, reg, mask, lo, hi, lr, init=A0 + A1, sizes=(2, 2)):
    assert list(reg) == ['mask', 'init', 'lo', 'hi', 'lr'] + list(k.sizes)
    assert reg['mask'] == mask and all(type(x) is int for x in reg['mask'])
    for name, want in (('init', init), ('lo', lo), ('hi', hi)):
        assert reg[name].dtype == np.float64
        np.testing.assert_array_equal(reg[name], want)
    assert reg['lr'] == lr and type(reg['lr']) is float
    assert (reg[k.sizes[0]], reg[k.sizes[1]]) == sizes


def test_selections(k):
    open4 = ([-INF] * 4, [INF] * 4)
    check(k, k.parse(k.pde(), {'K0': True, 'K1': [0, 1]}), [1, 1, 0, 1], *open4, 0.001)
    check(k, k.parse(k.pde(), {'K0': [True, False]}, 0.5), [1, 0, 0, 0], *open4, 0.5)                    # a key left out
    check(k, k.parse(k.pde(), {'K0': False, 'K1': True}, learning_rate=0.25), [0, 0, 1, 1], *open4, 0.25)
    check(k, k.parse(k.pde(), {'K0': None, 'K1': np.array([True, False])}), [0, 0, 1, 0], *open4, 0.001)
    # a PDE with one basis only: the vector is that basis alone
    check(k, k.parse(k.pde(second=False), {'K0': True, 'K1': False}), [1, 1], [-INF] * 2, [INF] * 2, 0.001, init=A0, sizes=(2, 0))
    check(k, k.parse(k.pde(first=False), {'K1': [0, 1]}), [0, 1], [-INF] * 2, [INF] * 2, 0.001, init=A1, sizes=(0, 2))
    for off in (None, False):
        assert k.parse(k.pde(), off) is None


def test_bounds(k):
    learn = {'K0': True, 'K1': [0, 1]}
    # one pair covers every learnt entry of its basis; a list names the entries one by one, None for an open side or entry
    check(k, k.parse(k.pde(), learn, bounds={'K0': (-2, 3), 'K1': [None, (None, 1.0)]}),
          [1, 1, 0, 1], [-2, -2, -INF, -INF], [3, 3, INF, 1.0], 0.001)
    check(k, k.parse(k.pde(), learn, bounds={'K0': [(-2, 3), (-2, 3)]}), [1, 1, 0, 1], [-2, -2, -INF, -INF], [3, 3, INF, INF], 0.001)
    check(k, k.parse(k.pde(), learn, bounds={'K1': (0, None)}), [1, 1, 0, 1], [-INF, -INF, -INF, 0], [INF] * 4, 0.001)
    # an entry that is not learnt takes no bounds; the pair form skips it, the list form must say None
    assert k.sentence(k.pde(), learn, bounds={'K1': [(0, 3), None]}) == "BOUNDS['K1'][0] bounds an amplitude that OPT does not select"
    assert k.sentence(k.pde(), {'K0': True}, bounds={'K1': [None, (0, 3)]}) == "BOUNDS['K1'][1] bounds an amplitude that OPT does not select"
    assert k.sentence(k.pde(), learn, bounds={'K0': [(0, 1)]}) == \
        "BOUNDS['K0'] must be (lo, hi) or a list of 2 entries, each None or (lo, hi), got [(0, 1)]"
    assert k.sentence(k.pde(), learn, bounds={'K0': (1.0, None)}) == "BOUNDS['K0'][0] = (1.0, None) excludes the initial guess 0.5"
    assert k.sentence(k.pde(), learn, bounds={'K2': (0, 1)}) == "BOUNDS must be a dict {'K0': ..., 'K1': ...}, got {'K2': (0, 1)}"


def test_a_basis_the_pde_lacks(k):
    lacks = 'the PDE has no K1 basis (ADPDE(..., K1Basis=[...]))'
    assert k.sentence(k.pde(second=False), {'K0': True}, bounds={'K1': (0, 1)}) == "BOUNDS['K1']: " + lacks
    assert k.sentence(k.pde(second=False), {'K1': True}) == "OPT['K1']: " + lacks
    assert k.sentence(k.pde(second=False), {'K0': True, 'K1': [1, 0]}) == "OPT['K1']: " + lacks
    # (switched off, or bounds of None, for the basis it lacks: nothing to refuse)
    check(k, k.parse(k.pde(second=False), {'K0': True, 'K1': None}, bounds={'K0': (-1, 1), 'K1': None}), [1, 1], [-1, -1], [1, 1], 0.001,
          init=A0, sizes=(2, 0))


def test_the_empty_selection(k):
    for pde, learn in ((k.pde(), {'K0': False}), (k.pde(), {'K0': [0, 0], 'K1': False}), (k.pde(), {'K1': [False, False]}),
                       (k.pde(second=False), {'K0': [0, 0]}), (k.pde(False, False), {'K0': False}), (k.pde(False, False), {'K1': None})):
        assert k.sentence(pde, learn) == 'OPT selects no amplitude'


def test_malformed_selections(k):
    for learn in (True, {}, {'K2': True}, [True, True]):
        assert k.sentence(k.pde(), learn) == "OPT must be a dict {'K0': True | mask, 'K1': True | mask}, got %r" % (learn,)
    for sel in ([True], [1, 2], 'all'):
        assert k.sentence(k.pde(), {'K1': sel}) == \
            "OPT['K1'] must be True or a mask of 2 booleans (one per function of K1Basis), got %r" % (sel,)
    assert k.sentence(k.pde(), {'K0': True}, lr=0.0) == 'LR=0.0 must be a finite number > 0'


def test_lr_and_bounds_without_the_option(k):
    for off in (None, False):
        assert k.sentence(k.pde(), off, lr=0.1) == 'LR=0.1 is an option of OPT=...'
        assert k.sentence(k.pde(), off, bounds={'K0': (0, 1)}) == 'BOUNDS is an option of OPT=...'
