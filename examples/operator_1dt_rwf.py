"""1D+t diffusion with a manufactured solution, trained with learnt weight scales.

    python examples/operator_1dt_rwf.py [folder] [epochs]

u* = exp(-t) sin(pi x) on [-1, 1] x [0, 1], diff = 0.1, the source manufactured from u*, net [20] tanh: the problem of
tests/test_reparam_train_gpu.py.  reparam='rwf' writes every dense layer as W = V diag(exp s) with one learnt log-scale per output
neuron (random weight factorization); {'kind': 'slope', 'n': 10, 'per': 'layer'} learns one activation slope per hidden layer instead.
Prints the l2 error against u* and the final scales exp(s) per layer."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from varnet_amd.adpde import ADPDE
from varnet_amd.domain import Domain1D
from varnet_amd.varnet import VarNet

folder = sys.argv[1] if len(sys.argv) > 1 else 'operator_1dt_rwf_out'
epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
kappa, pi = 0.1, np.pi


def cEx(x, t=0):
    return np.exp(-t) * np.sin(pi * x)


def source(x, t=0):
    return -cEx(x, t) + kappa * pi ** 2 * cEx(x, t)


pde = ADPDE(Domain1D(np.array([-1.0, 1.0])), diff=kappa, vel=0.0, source=source, tInterval=[0, 1.0], IC=lambda x: cEx(x, 0.0), cEx=cEx,
            BCs=[[0.0, 1.0, cEx], [0.0, 1.0, cEx]])
np.random.seed(0)
vn = VarNet(pde, layerWidth=[20], discNum=20, bDiscNum=None, tDiscNum=10, activationFun='tanh', learning_rate=0.01, reparam='rwf')
vn.train(folder, weight=[1.0, 1.0, 1.0], epochNum=epochs, tol=0.0, saveFreq=epochs, verbose=False)
print('l2 error against u*: %.4f' % float(vn.residual()[2]))
for l, f in enumerate(vn.scales(), 1):
    print('layer %d: exp(s) in [%.3f, %.3f]' % (l, f.min(), f.max()))
vn.engine.close()
