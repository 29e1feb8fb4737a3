"""1D+t advection-diffusion travelling wave, trained with self-adaptive weights on the initial rows.

    python examples/operator_1dt_icsa.py [folder] [epochs] [rule]

u* = exp(-kappa pi^2 t) sin(pi (x - vel t)) on [-1, 1] x [0, 1] with its Dirichlet data, diff = 0.1, vel = 0.5, net [20] tanh: the
problem of tests/test_bicadapt_train_gpu.py, whose initial profile is the hard part.  bicAdapt={'ic': 'sa'} keeps one weight per
initial row on the device and moves it by gradient ascent on the row's own squared error (an Adam step of its own, McClenny &
Braga-Neto 2023); 'rba' is the residual-based attention rule, lambda'_i = gamma lambda_i + eta sqrt(l_i) / max sqrt(l); a dict sets
the parameters, e.g. {'ic': {'rule': 'sa', 'lr': 0.01}, 'bc': 'rba'}; bicWeights={'bc': lambda x, t: ...} gives static ones.
Prints the l2 error against u*, the weights' statistics and the rows the weights ended up on."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.varnet import VarNet

folder = sys.argv[1] if len(sys.argv) > 1 else 'operator_1dt_icsa_out'
epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
rule = sys.argv[3] if len(sys.argv) > 3 else 'sa'
kappa, vel, pi = 0.1, 0.5, np.pi


def cEx(x, t=0):
    return np.exp(-kappa * pi ** 2 * t) * np.sin(pi * (x - vel * t))


pde = ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=kappa, vel=vel, tInterval=[0, 1.0], IC=lambda x: cEx(x, 0.0), cEx=cEx,
            BCs=[[0.0, 1.0, cEx], [0.0, 1.0, cEx]])
np.random.seed(0)
vn = VarNet(pde, layerWidth=[20], discNum=20, bDiscNum=None, tDiscNum=10, activationFun='tanh', learning_rate=0.01,
            bicAdapt={'ic': rule})
res = vn.train(folder, epochNum=epochs, tol=0.0, saveFreq=max(1, epochs // 10), verbose=False)
print('l2 error against u*: %.4f' % float(vn.residual()[2]))
w = vn.bicRowWeights()['ic']
st = w['stats']
print('omega on the %d initial rows: min %.3f, max %.3f, mean %.3f, effective sample share %.3f after %d updates'
      % (w['omega'].size, st['min'], st['max'], st['mean'], st['share'], int(st['tau'])))
for i in np.argsort(-w['omega'])[:5]:
    print('  x = %+.3f: omega %.3f, squared error %.3e' % (w['x'][i, 0], w['omega'][i], w['l'][i]))
print('statistics per monitor:', [(e, round(h['ic']['max'], 3)) for e, h in res.bicAdaptHist])
vn.engine.close()
