"""1D+t advection-diffusion travelling wave, trained with self-adaptive test-function weights.

    python examples/operator_1dt_rba.py [folder] [epochs] [rule]

u* = exp(-kappa pi^2 t) sin(pi (x - vel t)) on [-1, 1] x [0, 0.5] with its Dirichlet data, diff = 0.1, vel = 0.5, net [20] tanh: the
problem of tests/test_adapt_train_gpu.py.  tfAdapt='rba' keeps one weight per test function on the device, lambda'_k =
gamma lambda_k + eta sqrt(l_k) / max sqrt(l) after every step (residual-based attention); 'sa' moves lambda by gradient ascent
with an Adam step of its own; a dict sets the parameters, e.g. {'rule': 'rba', 'eta': 0.05, 'every': 10}.
Prints the l2 error against u*, the weights' statistics and their correlation with the final loss field."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.varnet import VarNet

folder = sys.argv[1] if len(sys.argv) > 1 else 'operator_1dt_rba_out'
epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
rule = sys.argv[3] if len(sys.argv) > 3 else 'rba'
kappa, vel, pi = 0.1, 0.5, np.pi


def cEx(x, t=0):
    return np.exp(-kappa * pi ** 2 * t) * np.sin(pi * (x - vel * t))


pde = ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=kappa, vel=vel, tInterval=[0, 0.5], IC=lambda x: cEx(x, 0.0), cEx=cEx,
            BCs=[[0.0, 1.0, cEx], [0.0, 1.0, cEx]])
np.random.seed(0)
vn = VarNet(pde, layerWidth=[20], discNum=20, bDiscNum=None, tDiscNum=10, activationFun='tanh', learning_rate=0.01, tfAdapt=rule)
res = vn.train(folder, epochNum=epochs, tol=0.0, saveFreq=max(1, epochs // 10), verbose=False)
print('l2 error against u*: %.4f' % float(vn.residual()[2]))
w = vn.tfWeights()[0]
print('omega: min %.3f, max %.3f, mean %.3f, effective sample share %.3f after %d updates'
      % (w['stats']['min'], w['stats']['max'], w['stats']['mean'], w['stats']['share'], int(w['stats']['tau'])))
vn.tData.select_mor(0)
lv = vn.engine.eval_loss(0, lossVec=True)[1].cpu().numpy().reshape(-1)
print('correlation of omega_k with the loss field l_k: %.3f' % float(np.corrcoef(w['omega'], lv)[0, 1]))
for epoch, stats in res.tfAdaptHist:
    print('epoch %6d: share %.3f, max omega %.3f' % (epoch, stats[0]['share'], stats[0]['max']))
vn.engine.close()
