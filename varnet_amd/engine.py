"""
ctypes binding of libvarnet_hip.so (include/varnet_hip.h) -- the object that takes the place
of the reference's `TFNN` (/root/reference/TFModel.py:54-436) behind `VarNet`.

PyTorch is used only as plumbing: device memory (tensors whose `data_ptr()` is handed to the
C ABI), the current HIP stream, and `torch.distributed` for the tower gradient SUM
(TFModel.py:342-377).  There is no CPU fallback: constructing an engine without the library or
without a GPU raises.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# VARNET_HIP_LIB selects a diagnostic build of the same ABI (tools/): never a different backend
LIB_PATH = os.environ.get('VARNET_HIP_LIB', os.path.join(_HERE, 'libvarnet_hip.so'))
# the tests' cross-check build: the product objects + the 4-wave geometry of the fused kernel (VN_KERNEL_FUSED), which serves no
# automatic route and is therefore not in the product library (varnet_amd/csrc/Makefile, target xcheck)
XCHECK_LIB_PATH = os.path.join(_HERE, 'libvarnet_hip_xcheck.so')
_xlib = None

VN_MAX_LAYERS = 16          # what a vn_config may describe (include/varnet_hip.h); beyond the kernels' own range
VN_MAX_WIDTH = 2048         # (6 layers x 64 wide, 8 inputs) the engine runs layer by layer (VN_KERNEL_LAYERED)
VN_MAX_DIN = 32
VN_KMAX_LAYERS, VN_KMAX_WIDTH, VN_KMAX_DIN = 6, 64, 8
VN_KERNEL_AUTO, VN_KERNEL_GENERIC, VN_KERNEL_FUSED, VN_KERNEL_FUSED16, VN_KERNEL_LAYERED = 0, 1, 2, 3, 4
VN_OPT_ADAM, VN_OPT_RMSPROP, VN_OPT_LBFGS = 0, 1, 2
VN_LBFGS_HISTORY = 10
LBFGS_INFO = ('status', 'f_k', 'f_next', 'BCloss', 'ICloss', 'varLoss', 't', 'trials', 'gd', 'pairs')
VN_COMM_ID_BYTES = 128
VN_ABI_VERSION = 7          # include/varnet_hip.h: load_library refuses a library that reports another number


class VnConfig(C.Structure):
    _fields_ = [('dim', C.c_int32), ('d_in', C.c_int32), ('n_layers', C.c_int32),
                ('widths', C.c_int32 * VN_MAX_LAYERS), ('activation', C.c_int32),
                ('integ_num', C.c_int32), ('time_dependent', C.c_int32),
                ('has_source', C.c_int32), ('has_integw', C.c_int32), ('device', C.c_int32),
                ('optimizer', C.c_int32), ('kernel', C.c_int32),
                ('lr', C.c_double), ('beta1', C.c_double), ('beta2', C.c_double),
                ('eps', C.c_double), ('layer_act', C.c_int32 * VN_MAX_LAYERS)]


_lib = None

_SIGS = {
    'vn_last_error': (C.c_char_p, []),
    'vn_abi_version': (C.c_int, []),
    'vn_create': (C.c_int, [C.POINTER(VnConfig), C.POINTER(C.c_void_p)]),
    'vn_destroy': (C.c_int, [C.c_void_p]),
    'vn_set_stream': (C.c_int, [C.c_void_p, C.c_void_p]),
    'vn_param_count': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    'vn_params_init': (C.c_int, [C.c_void_p, C.c_uint64]),
    'vn_params_get': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'vn_params_set': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'vn_state_size': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    'vn_state_export': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'vn_state_import': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'vn_set_fe_table': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'vn_set_interior': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_int64, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]),
    'vn_set_dedup': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    'vn_set_bic': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_double]),
    'vn_set_batch_bic': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'vn_set_flux_bc': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double]),
    'vn_set_periodic': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double]),
    'vn_set_observations': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                      C.c_int64, C.c_double]),
    'vn_set_obs_weight': (C.c_int, [C.c_void_p, C.c_double]),
    'vn_get_obs_misfit': (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    'vn_set_ansatz': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'vn_set_ansatz_points': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'vn_set_ansatz_rows': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'vn_set_reaction': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_double)]),
    'vn_set_nlflux': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_double)]),
    'vn_set_nldiff': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_double)]),
    'vn_set_tf_weights': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    'vn_set_causal': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double]),
    'vn_causal_weights': (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.c_int32]),
    'vn_set_tf_adapt': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_void_p]),
    'vn_get_tf_adapt': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    'vn_set_tf_adapt_state': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64]),
    'vn_set_bic_weights': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    'vn_set_bic_adapt': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_void_p]),
    'vn_get_bic_adapt': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    'vn_set_bic_adapt_state': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64]),
    'vn_set_coef_learn': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), C.c_double]),
    'vn_get_coefs': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    'vn_set_coefs': (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    'vn_set_source_basis': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    'vn_set_source_learn': (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.c_double]),
    'vn_get_source_amps': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32]),
    'vn_set_source_amps': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int32]),
    'vn_set_field_basis': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    'vn_set_field_learn': (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.c_double]),
    'vn_get_field_amps': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32]),
    'vn_set_field_amps': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int32]),
    'vn_set_bic_basis': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    'vn_set_bic_learn': (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                   C.POINTER(C.c_double), C.c_double]),
    'vn_get_bic_amps': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32]),
    'vn_set_bic_amps': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int32]),
    'vn_set_fluxbc_basis': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    'vn_set_fluxbc_learn': (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.c_double]),
    'vn_get_fluxbc_amps': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32]),
    'vn_set_fluxbc_amps': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int32]),
    'vn_set_learnt_prior': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double)]),
    'vn_get_learnt_prior': (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double)]),
    'vn_set_reparam': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.POINTER(C.c_double), C.c_int32, C.c_double]),
    'vn_get_reparam': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'vn_set_reparam_state': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'vn_reparam_grad': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'vn_set_weights': (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    'vn_bind_grad_buffer': (C.c_int, [C.c_void_p, C.c_void_p]),
    'vn_grad': (C.c_int, [C.c_void_p, C.c_int32]),
    'vn_term_stats': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    'vn_term_grads': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_uint32, C.POINTER(C.c_double),
                                C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p]),
    'vn_apply': (C.c_int, [C.c_void_p]),
    'vn_train_step': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    'vn_train_epoch': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p]),
    'vn_lbfgs_step': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    'vn_lbfgs_loss64': (C.c_int, [C.c_void_p, C.c_int]),
    'vn_eval_loss': (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.c_void_p]),
    'vn_objective_f64': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    'vn_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'vn_forward_grad': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    'vn_debug_calibrate': (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    'vn_forward_f64': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'vn_residual': (C.c_int, [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p, C.c_void_p]),
    'vn_residual_f64': (C.c_int, [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p, C.c_void_p]),
    'vn_comm_available': (C.c_int, []),
    'vn_comm_version': (C.c_int, [C.POINTER(C.c_int32)]),
    'vn_comm_unique_id': (C.c_int, [C.c_void_p]),
    'vn_comm_init': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    'vn_comm_size': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'vn_comm_destroy': (C.c_int, [C.c_void_p]),
    'vn_comm_abandon': (C.c_int, [C.c_void_p]),
    'vn_allreduce_grad': (C.c_int, [C.c_void_p]),
    'vn_get_step': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    'vn_profile_comm': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'vn_kernel_path': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'vn_debug_stamps': (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    'vn_debug_point_route': (C.c_int, [C.c_void_p, C.c_int32]),
    'vn_state_snapshot': (C.c_int, [C.c_void_p]),
    'vn_state_rollback': (C.c_int, [C.c_void_p]),
    'vn_debug_calibrate_f64': (C.c_int, [C.c_void_p, C.c_double, C.POINTER(C.c_double)]),
    'vn_profile_begin': (C.c_int, [C.c_void_p]),
    'vn_profile_end': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                 C.c_char_p, C.c_int32]),
}

ABI_SYMBOLS = tuple(_SIGS.keys())

# the row sets of vn_set_ansatz_rows (VN_ANSATZ_*): the _keep key of the set's own registration
ANSATZ_SETS = {'bic': (0, 'bic'), 'flux': (1, 'flux'), 'periodic': (2, 'periodic'), 'obs': (3, 'obs')}

# the _keep keys of the three polynomial terms, in the order of the coefficient index (vn_set_coef_learn)
COEF_TERMS = ('react', 'nlflux', 'nldiff')
# the learnt vectors, in the order of VN_LEARNT_* (the `kind` of vn_set_learnt_prior): the name vn_get_* / vn_set_* carry, and
# the fixed length (None: the ABI takes the length J)
LEARNT = {'coef': ('coefs', 9), 'source': ('source_amps', None), 'field': ('field_amps', None), 'bic': ('bic_amps', None),
          'fluxbc': ('fluxbc_amps', None)}

# learnt weight scales (vn_set_reparam): VN_REPARAM_* and VN_REPARAM_PER_*
REPARAM_MODES = {'rwf': 1, 'slope': 2}
REPARAM_PER = {'neuron': 0, 'layer': 1}

# self-adaptive test-function weights (vn_set_tf_adapt): the rules, their own keys with defaults, and the keys both share
ADAPT_RULES = {'rba': 1, 'sa': 2}
ADAPT_OWN = {'rba': {'gamma': 0.999, 'eta': 0.01},
             'sa': {'lr': 0.005, 'beta1': 0.9, 'beta2': 0.999, 'eps': 1e-8, 'cap': 1e3}}
ADAPT_SHARED = {'power': 2, 'init': 1.0, 'normalize': True, 'every': 1}


def tf_adapt_spec(spec):
    """None | 'rba' | 'sa' | {'rule': ..., key: value} -> None or the full dict of the rule's parameters (defaults filled in).
    ValueError for an unknown rule, an unknown key or a key of the other rule, and for values the engine would refuse."""
    if spec is None:
        return None
    if isinstance(spec, str):
        spec = {'rule': spec}
    if not isinstance(spec, dict):
        raise ValueError("tfAdapt must be None, 'rba', 'sa' or a dict with a 'rule' (got %r)" % (spec,))
    rule = spec.get('rule')
    if rule not in ADAPT_RULES:
        raise ValueError("tfAdapt rule must be 'rba' or 'sa' (got %r)" % (rule,))
    out = {'rule': rule}
    out.update(ADAPT_OWN[rule])
    out.update(ADAPT_SHARED)
    for k, v in spec.items():
        if k == 'rule':
            continue
        if k not in out:
            other = [r for r in ADAPT_OWN if r != rule and k in ADAPT_OWN[r]]
            raise ValueError("tfAdapt: %r is %s" % (k, "a key of the %r rule, not of %r" % (other[0], rule) if other else
                                                    'no key of the adaptive weights (%s)' % ', '.join(sorted(out))))
        out[k] = v
    out['normalize'] = bool(out['normalize'])
    num = {k: float(v) for k, v in out.items() if k not in ('rule', 'normalize')}
    if not all(np.isfinite(v) for v in num.values()):
        raise ValueError('tfAdapt: every parameter must be finite (got %r)' % (out,))
    if out['power'] not in (1, 2):
        raise ValueError('tfAdapt: power must be 1 or 2 (got %r)' % (out['power'],))
    if num['every'] < 1 or num['every'] != int(num['every']):
        raise ValueError('tfAdapt: every must be a whole number >= 1 (got %r)' % (out['every'],))
    if num['init'] < 0:
        raise ValueError('tfAdapt: init must be >= 0 (got %r)' % (out['init'],))
    if rule == 'rba':
        if not 0.0 <= num['gamma'] <= 1.0 or num['eta'] < 0:
            raise ValueError('tfAdapt rba: gamma must lie in [0, 1] and eta be >= 0 (got %r, %r)' % (out['gamma'], out['eta']))
    else:
        if num['lr'] < 0 or num['cap'] <= 0 or num['eps'] <= 0 or not 0.0 <= num['beta1'] < 1.0 or not 0.0 <= num['beta2'] < 1.0:
            raise ValueError('tfAdapt sa: lr >= 0, cap > 0, eps > 0 and beta1, beta2 in [0, 1) are required (got %r)' % (out,))
    out['power'], out['every'] = int(out['power']), int(out['every'])
    return out


def tf_adapt_par(spec):
    """(rule id, par[10]) of vn_set_tf_adapt for a full dict of tf_adapt_spec."""
    own = (spec['gamma'], spec['eta'], 0.0, 0.0, 0.0) if spec['rule'] == 'rba' else \
        (spec['lr'], spec['cap'], spec['beta1'], spec['beta2'], spec['eps'])
    par = [float(x) for x in own] + [float(spec['power']), float(spec['init']), 1.0 if spec['normalize'] else 0.0,
                                     float(spec['every']), 0.0]
    return ADAPT_RULES[spec['rule']], par


def reparam_count(mode, per, inpDim, layerWidth):
    """Number of scales S of a mode on the network inpDim -> layerWidth -> 1 (include/varnet_hip.h, vn_set_reparam)."""
    if mode == 'rwf':
        return int(sum(layerWidth)) + 1
    return len(layerWidth) if per == 'layer' else int(sum(layerWidth))


def reparam_layers(mode, per, layerWidth):
    """Per-layer lengths of the scale vector, in its order (rwf: the output layer last)."""
    if mode == 'rwf':
        return [int(w) for w in layerWidth] + [1]
    return [1] * len(layerWidth) if per == 'layer' else [int(w) for w in layerWidth]


# the terms of the objective as vn_term_grads numbers them (VN_TERM_*)
TERMS = ('bc', 'ic', 'var', 'obs')


class VNError(RuntimeError):
    pass


def load_library(path=None):
    """dlopen libvarnet_hip.so and attach the prototypes.  Raises if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError('%s not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                           '(there is no CPU fallback for the VarNet engine)' % p)
    lib = C.CDLL(p)
    # a stale side build (VARNET_HIP_LIB / tools/build_variant.sh) would misread vn_config: check before binding anything else
    lib.vn_abi_version.restype = C.c_int
    lib.vn_abi_version.argtypes = []
    got = lib.vn_abi_version()
    if got != VN_ABI_VERSION:
        raise VNError('%s reports ABI version %d, this binding is written for %d: rebuild it from this tree' % (p, got, VN_ABI_VERSION))
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _ptr(t):
    """Device/host address of a torch tensor or numpy array (None -> NULL)."""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        return t.ctypes.data
    return t.data_ptr()


_exit_guard = {'armed': False, 'code': 0, 'threads': []}


def _exit_without_waiting(pending=None):
    """After an abandoned communicator a helper thread may sit inside ncclCommInitRank for ever, and RCCL's own exit handlers
    can wait for it.  Arm, once per process, an `atexit` hook that flushes the standard streams and leaves through
    `os._exit` with the status the interpreter was going to return (1 after an uncaught exception, the argument of
    `sys.exit`); registered last, so it runs FIRST and nothing of the normal teardown touches the wedged library.  The
    process is never re-executed.  Only when a `pending` helper thread is in fact still alive at exit: otherwise the
    interpreter leaves the normal way."""
    if pending is not None:
        _exit_guard['threads'].append(pending)
    if _exit_guard['armed']:
        return
    _exit_guard['armed'] = True
    import atexit
    import sys
    old_hook, old_exit = sys.excepthook, sys.exit

    def hook(tp, val, tb):
        _exit_guard['code'] = 1
        old_hook(tp, val, tb)

    def exit_(code=0):
        _exit_guard['code'] = code if isinstance(code, int) else (0 if code is None else 1)
        old_exit(code)

    def leave():
        if not any(t.is_alive() for t in _exit_guard['threads']):
            return
        for f in (sys.stdout, sys.stderr):
            try:
                f.flush()
            except Exception:                        # noqa: BLE001
                pass
        os._exit(_exit_guard['code'])
    sys.excepthook, sys.exit = hook, exit_
    atexit.register(leave)


class VNEngine:
    """
    One engine per GPU / process.  Mirrors what `VarNet` needs from `TFNN`:
    parameters + optimiser state, loss / gradient / update on registered batches, model and
    residual evaluation.
    """

    def __init__(self, dim, inpDim, layerWidth, timeDependent, integNum, isSource=False,
                 integWflag=False, learning_rate=0.001, device=0, activationFun='sigmoid',
                 optimizer_name='adam', kernel=VN_KERNEL_AUTO, xcheck=False):
        import torch
        self.torch = torch
        # xcheck: an engine of the tests' cross-check library (the product objects + the 4-wave kernel + the f32-MFMA forms of the
        # point kernels for the networks the bf16-piece kernels serve: debug_point_route(2)); never set by the product path
        if kernel == VN_KERNEL_FUSED or xcheck:
            global _xlib
            if _xlib is None:
                _xlib = load_library(XCHECK_LIB_PATH)
            self.lib = _xlib
        else:
            self.lib = load_library()
        if not torch.cuda.is_available():
            raise VNError('no GPU visible: the VarNet HIP engine has no CPU fallback')
        # a name for all hidden layers, a one-entry list, or one entry per layer (TFModel.py:113-119)
        depth = len(layerWidth)
        if isinstance(activationFun, str):
            acts = [activationFun] * depth
        elif isinstance(activationFun, (list, tuple)) and len(activationFun) == 1:
            acts = list(activationFun) * depth
        elif len(activationFun) != depth:
            raise ValueError('activation function list is incompatible with number of layers!')
        else:
            acts = list(activationFun)
        acts = [str(a).lower() for a in acts]
        if any(a not in ('sigmoid', 'tanh') for a in acts):
            raise ValueError('activation function must be \'sigmoid\' or \'tanh\' (VarNet.py:97)')
        if optimizer_name.lower() not in ('adam', 'rmsprop', 'lbfgs'):
            raise ValueError('unknown optimizer requested!')           # TFModel.py:133-134
        if learning_rate < 0.0:
            raise ValueError('learning rate must be positive!')        # TFModel.py:130
        if len(layerWidth) > VN_MAX_LAYERS or max(layerWidth) > VN_MAX_WIDTH or inpDim > VN_MAX_DIN:
            raise ValueError('network exceeds engine limits (%d layers x %d, %d inputs)'
                             % (VN_MAX_LAYERS, VN_MAX_WIDTH, VN_MAX_DIN))
        cfg = VnConfig()
        cfg.dim, cfg.d_in, cfg.n_layers = dim, inpDim, len(layerWidth)
        for i, wd in enumerate(layerWidth):
            cfg.widths[i] = int(wd)
        if all(a == acts[0] for a in acts):
            cfg.activation = 1 if acts[0] == 'tanh' else 0
        else:                                        # different entries: the engine runs such a net layer by layer
            cfg.activation = 2
        for i, a in enumerate(acts):
            cfg.layer_act[i] = 1 if a == 'tanh' else 0
        cfg.integ_num = int(integNum)
        cfg.time_dependent = int(bool(timeDependent))
        cfg.has_source = int(bool(isSource))
        cfg.has_integw = int(bool(integWflag))
        cfg.device = int(device)
        cfg.optimizer = {'adam': VN_OPT_ADAM, 'rmsprop': VN_OPT_RMSPROP, 'lbfgs': VN_OPT_LBFGS}[optimizer_name.lower()]
        self.optimizer_name = optimizer_name.lower()
        cfg.kernel = kernel
        cfg.lr, cfg.beta1, cfg.beta2, cfg.eps = learning_rate, 0.9, 0.999, 1e-8
        self.cfg = cfg
        self.device = torch.device('cuda', device)
        self.dim, self.inpDim, self.layerWidth = dim, inpDim, list(layerWidth)
        self.integNum = int(integNum)
        self.h = C.c_void_p()
        self._ck(self.lib.vn_create(C.byref(cfg), C.byref(self.h)))
        n = C.c_int64()
        self._ck(self.lib.vn_param_count(self.h, C.byref(n)))
        self.P = n.value
        self._keep = {}            # python references to registered device tensors
        self._epoch_arrays = {}    # ctypes id arrays of train_epoch, by tuple of batch ids
        self._bic_key = None       # whose BC/IC rows are registered (ManageTrainData.select_mor's note; any set_bic clears it)
        self.gradbuf = None
        self.use_current_stream()

    # -- plumbing ------------------------------------------------------------------------
    def _ck(self, rc):
        if rc != 0:
            msg = 'varnet_hip error %d: %s' % (rc, self.lib.vn_last_error().decode())
            # under a launcher the failing rank's breadcrumb says what failed (launch.spawn_ranks reports it when it ends
            # the peers this rank left in a collective: include/varnet_hip.h, "Failure under a communicator")
            from .launch import mark_stage
            mark_stage('engine_error: ' + msg[:160].replace('\n', ' '))
            raise VNError(msg)

    def close(self):
        if getattr(self, 'h', None) is not None and self.h:
            if getattr(self, '_comm_abandoned', False):
                self.h = None                        # vn_destroy would call ncclCommDestroy on a communicator whose peer is wedged
                return
            self.lib.vn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def use_current_stream(self):
        s = self.torch.cuda.current_stream(self.device).cuda_stream
        self._ck(self.lib.vn_set_stream(self.h, C.c_void_p(s)))

    def dev(self, a, dtype=None):
        """numpy / tensor -> contiguous device tensor (fp32 by default: TFModel.py:531,602-619)."""
        torch = self.torch
        dtype = dtype or torch.float32
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=self.device).contiguous()

    # -- parameters ----------------------------------------------------------------------
    def init_params(self, seed=0):
        self._ck(self.lib.vn_params_init(self.h, C.c_uint64(seed)))

    def get_params(self):
        out = np.empty(self.P, dtype=np.float32)
        self._ck(self.lib.vn_params_get(self.h, out.ctypes.data, self.P))
        return out

    def set_params(self, flat):
        flat = np.ascontiguousarray(flat, dtype=np.float32)
        self._ck(self.lib.vn_params_set(self.h, flat.ctypes.data, flat.size))

    def export_state(self):
        n = C.c_int64()
        self._ck(self.lib.vn_state_size(self.h, C.byref(n)))
        buf = np.empty(n.value, dtype=np.uint8)
        self._ck(self.lib.vn_state_export(self.h, buf.ctypes.data, n.value))
        return buf

    def import_state(self, buf):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        self._ck(self.lib.vn_state_import(self.h, buf.ctypes.data, buf.size))

    def state_snapshot(self):
        """Device-side snapshot of (parameters, optimizer slots, step counter): no host copy, no synchronisation."""
        self._ck(self.lib.vn_state_snapshot(self.h))

    def state_rollback(self):
        self._ck(self.lib.vn_state_rollback(self.h))

    @property
    def step(self):
        s = C.c_int64()
        self._ck(self.lib.vn_get_step(self.h, C.byref(s)))
        return s.value

    # -- data registration ---------------------------------------------------------------
    def set_fe_table(self, N, dNt, integW=None):
        N = np.ascontiguousarray(np.reshape(N, -1), dtype=np.float32)
        dNt = np.ascontiguousarray(np.reshape(dNt, -1), dtype=np.float32)
        W = None if integW is None else np.ascontiguousarray(np.reshape(integW, -1), dtype=np.float32)
        assert N.size == self.integNum and dNt.size == self.integNum
        self._ck(self.lib.vn_set_fe_table(self.h, N.ctypes.data, dNt.ctypes.data, _ptr(W)))

    def set_interior(self, batch, Input, gcoef, source=None, n_k=None, detJ=1.0, N_rows=None,
                     dNt_rows=None):
        torch = self.torch

        def flat(a):
            if a is None:
                return None
            if isinstance(a, torch.Tensor):
                return self.dev(a.reshape(-1))
            return self.dev(np.reshape(a, -1))

        Input = self.dev(Input)
        gcoef = self.dev(gcoef)
        source = flat(source)
        nT = Input.shape[0]
        if n_k is None:
            n_k = nT // self.integNum
        assert n_k * self.integNum == nT, 'rows must be whole test functions'
        assert Input.shape[1] == self.inpDim and gcoef.shape == (nT, self.dim)
        detJv, detJ_s = None, 0.0
        if isinstance(detJ, torch.Tensor) or np.size(detJ) > 1:
            detJv = flat(detJ)
            assert detJv.numel() == n_k
        else:
            detJ_s = float(np.reshape(detJ, -1)[0]) if not np.isscalar(detJ) else float(detJ)
        Nr, dNr = flat(N_rows), flat(dNt_rows)
        self._keep[('int', batch)] = (Input, gcoef, source, detJv, Nr, dNr)
        self._ck(self.lib.vn_set_interior(self.h, batch, _ptr(Input), _ptr(gcoef), _ptr(source), n_k,
                                          _ptr(detJv), detJ_s, _ptr(Nr), _ptr(dNr)))
        for key in ('react', 'nlflux', 'nldiff', 'tfw', 'causal', 'adapt', 'srcbasis', 'fldbasis', 'bicbasis', 'ansatz', 'ansatzpts'):   # vn_set_interior cleared the
            self._keep.pop((key, batch), None)      # batch's three polynomial terms, its per-test-function loss weights, its source
                                                    # and field bases, the basis of its own BC/IC copy and its ansatz streams

    def set_dedup(self, batch, Xu=None, uid=None, rowptr=None, rowidx=None):
        """Register (or, with Xu=None, clear) the de-duplicated formulation of `batch`."""
        t = self.torch
        self._keep.pop(('ansatzpts', batch), None)   # vn_set_dedup clears the ansatz streams at the previous map's points
        if Xu is None:
            self._keep.pop(('dd', batch), None)
            self._ck(self.lib.vn_set_dedup(self.h, batch, None, 0, None, None, None))
            return
        Xu = self.dev(Xu)
        i32 = lambda a: (a if isinstance(a, t.Tensor) else t.as_tensor(np.ascontiguousarray(a))).to(
            device=self.device, dtype=t.int32).contiguous()
        uid, rowptr, rowidx = i32(uid), i32(rowptr), i32(rowidx)
        # the ABI carries pointers only: the lengths the validator and every later kernel rely on are checked here
        kept = self._keep.get(('int', batch))
        nT = None if kept is None else int(kept[0].shape[0])
        assert rowptr.numel() == Xu.shape[0] + 1 and uid.numel() == rowidx.numel()
        assert nT is None or uid.numel() == nT, 'uid / rowidx must have one entry per interior row (%s != %s)' % (uid.numel(), nT)
        old = self._keep.pop(('dd', batch), None)
        try:
            self._ck(self.lib.vn_set_dedup(self.h, batch, _ptr(Xu), Xu.shape[0], _ptr(uid), _ptr(rowptr), _ptr(rowidx)))
        finally:
            del old           # the engine dropped the previous registration before validating this one (vn_set_dedup)
        self._keep[('dd', batch)] = (Xu, uid, rowptr, rowidx)

    def set_bic(self, biInput, biLabel, bDof, biDimVal):
        self._bic_key = None
        self._keep.pop('bicw', None)               # vn_set_bic clears the rows' weights (set_bic_weights, set_bic_adapt)
        nB = 0 if biInput is None else int(len(biInput))
        self._bic_rows = (int(bDof) if nB else 0, (nB - int(bDof)) if nB and self.cfg.time_dependent else 0)   # rows of (bc, ic)
        self._keep.pop(('ansatzrows', 'bic'), None)   # vn_set_bic drops the rows' ansatz streams
        self._keep.pop(('bicbasis', -1), None)     # vn_set_bic clears the shared set's basis
        if biInput is None or len(biInput) == 0:
            self._keep['bic'] = None
            self._ck(self.lib.vn_set_bic(self.h, None, None, 0, 0, float(biDimVal)))
            return
        biInput = self.dev(biInput)
        biLabel = self.dev(np.reshape(biLabel, -1) if isinstance(biLabel, np.ndarray) else biLabel.reshape(-1))
        self._keep['bic'] = (biInput, biLabel)
        self._ck(self.lib.vn_set_bic(self.h, _ptr(biInput), _ptr(biLabel), biInput.shape[0], int(bDof),
                                     float(biDimVal)))

    def set_batch_bic(self, batch, biInput=None, biLabel=None):
        """Per-batch copy of the BC/IC rows (the reference's shuffle permutes them per feed); None returns to the shared set."""
        self._keep.pop(('bicbasis', batch), None)  # vn_set_batch_bic clears the copy's basis
        if biInput is None:
            self._keep.pop(('bbic', batch), None)
            self._ck(self.lib.vn_set_batch_bic(self.h, batch, None, None))
            return
        biInput = self.dev(biInput)
        biLabel = self.dev(np.reshape(biLabel, -1) if isinstance(biLabel, np.ndarray) else biLabel.reshape(-1))
        self._keep[('bbic', batch)] = (biInput, biLabel)
        self._ck(self.lib.vn_set_batch_bic(self.h, batch, _ptr(biInput), _ptr(biLabel)))

    def _set_edge(self, key, fn, tensors, *scalars):
        """One registration call of an edge row set (vn_edge.h): fn(h, pointers of `tensors`, *scalars).  tensors None clears the
        set; else the device tensors are kept alive under `key` in place of the previous registration's."""
        self._keep.pop(('ansatzrows', key), None)    # a registration of the set drops its ansatz streams (edge_drop)
        if tensors is None:
            self._keep[key] = None
            self._ck(fn(self.h, *[None] * (len(fn.argtypes) - 1 - len(scalars)), *scalars))
            return
        old = self._keep.pop(key, None)
        try:
            self._ck(fn(self.h, *[_ptr(x) for x in tensors], *scalars))
        finally:
            del old           # the engine dropped the previous registration before checking this one
        self._keep[key] = tensors

    def set_flux_bc(self, X=None, normal=None, coef=None, label=None, biDimVal=1.0):
        """Register (or, with X=None, clear) the boundary-flux rows of Neumann / Robin edges (vn_set_flux_bc): X [nF, inpDim],
        outward unit normals [nF, dim], coef = b/a [nF], label = g/a [nF]."""
        self._keep.pop(('fbcbasis', -1), None)     # vn_set_flux_bc clears the rows' basis
        if X is None or len(X) == 0:
            return self._set_edge('flux', self.lib.vn_set_flux_bc, None, 0, float(biDimVal))
        X, normal = self.dev(X), self.dev(normal)
        coef, label = self.dev(np.reshape(coef, -1)), self.dev(np.reshape(label, -1))
        nF = X.shape[0]
        # the ABI carries pointers only: the lengths every kernel of the pass relies on are checked here
        assert X.shape == (nF, self.inpDim) and normal.shape == (nF, self.dim), (tuple(X.shape), tuple(normal.shape))
        assert coef.numel() == nF and label.numel() == nF
        self._set_edge('flux', self.lib.vn_set_flux_bc, (X, normal, coef, label), nF, float(biDimVal))

    def set_periodic(self, X=None, dir=None, gamma=1.0, biDimVal=1.0):
        """Register (or, with X=None, clear) the periodic boundary pairs (vn_set_periodic): X [2 nP, inpDim] and unit directions
        dir [2 nP, dim], rows i and i + nP being the two images of one point with the same direction; gamma >= 0 weights the
        derivative match (0: values only)."""
        if X is None or len(X) == 0:
            return self._set_edge('periodic', self.lib.vn_set_periodic, None, 0, float(gamma), float(biDimVal))
        X, dir = self.dev(X), self.dev(dir)
        rows = X.shape[0]
        # the ABI carries pointers only: the lengths every kernel of the pass relies on are checked here
        assert rows % 2 == 0, rows
        assert X.shape == (rows, self.inpDim) and dir.shape == (rows, self.dim), (tuple(X.shape), tuple(dir.shape))
        self._set_edge('periodic', self.lib.vn_set_periodic, (X, dir), rows // 2, float(gamma), float(biDimVal))

    def set_observations(self, X=None, value=None, q=None, dir=None, rowptr=None, wgt=None, weight=1.0):
        """Register (or, with X=None, clear) the observations (vn_set_observations): points X [n, inpDim] in nO segments
        rowptr [nO + 1] (None: point sensors, one point each), measured values value [nO], optional quadrature weights q [n]
        (None: 1), directions dir [n, dim] of a derivative part (None: values only) and weights wgt [nO] = 1 / sigma^2 (None: 1);
        weight = lambda, the factor of the misfit O = mean_i[wgt_i r_i^2] in the loss."""
        t = self.torch
        if X is None or len(X) == 0:
            return self._set_edge('obs', self.lib.vn_set_observations, None, 0, 0, float(weight))
        X, value = self.dev(X), self.dev(value).reshape(-1)
        n, nO = X.shape[0], value.shape[0]
        q = None if q is None else self.dev(q).reshape(-1)
        dir = None if dir is None else self.dev(dir)
        wgt = None if wgt is None else self.dev(wgt).reshape(-1)
        if rowptr is not None:
            rowptr = (rowptr if isinstance(rowptr, t.Tensor) else t.as_tensor(np.ascontiguousarray(rowptr))).to(
                device=self.device, dtype=t.int32).contiguous()
        # the ABI carries pointers only: the lengths the validator and every kernel of the pass rely on are checked here
        assert X.shape == (n, self.inpDim), tuple(X.shape)
        assert q is None or q.shape[0] == n, (tuple(q.shape), n)
        assert dir is None or dir.shape == (n, self.dim), (tuple(dir.shape), n)
        assert wgt is None or wgt.shape[0] == nO, (tuple(wgt.shape), nO)
        assert (rowptr.numel() == nO + 1) if rowptr is not None else (n == nO), (n, nO)
        self._set_edge('obs', self.lib.vn_set_observations, (X, q, dir, rowptr, value, wgt), n, nO, float(weight))

    def _set_ansatz(self, key, fn, index, streams, shapes):
        """One registration of ansatz streams (vn_ansatz.hip): fn(h, index, A, B, a, b).  streams = (A, B, a, b), each None or
        an array of the matching entry of `shapes` (None: length unknown here); all None clears.  The device tensors are kept
        alive under `key` in place of the previous registration's."""
        t = self.torch
        dev = []
        for x, shape in zip(streams, shapes):
            if x is None:
                dev.append(None)
                continue
            x = self.dev(x if isinstance(x, t.Tensor) else np.asarray(x))
            # the ABI carries pointers only: the lengths the kernels rely on are checked here
            if shape is not None:
                if x.numel() != int(np.prod(shape)):
                    raise ValueError('ansatz stream of %d entries where %s are registered' % (x.numel(), tuple(shape)))
                x = x.reshape(shape)
            dev.append(x.contiguous())
        old = self._keep.pop(key, None)
        try:
            self._ck(fn(self.h, int(index), *[_ptr(x) for x in dev]))
        finally:
            del old           # the engine dropped the previous registration before checking this one
        if any(x is not None for x in dev):
            self._keep[key] = tuple(dev)

    def set_ansatz(self, batch, A=None, B=None, a=None, b=None):
        """Register (or, with all None, clear) the hard-constraint ansatz u = A + B n on the interior rows of `batch`
        (vn_set_ansatz), after set_interior of that batch: one value per interior row each; a = grad_x A . gcoef and
        b = grad_x B . gcoef with the very gcoef of set_interior.  A, a, b may be None (zero); B is required."""
        kept = self._keep.get(('int', batch))
        n = None if kept is None else (int(kept[0].shape[0]),)
        self._set_ansatz(('ansatz', batch), self.lib.vn_set_ansatz, batch, (A, B, a, b), (n, n, n, n))

    def set_ansatz_points(self, batch, A=None, B=None, gA=None, gB=None):
        """... at the unique points of the de-duplication map of `batch` (vn_set_ansatz_points), after set_dedup: A, B [U] and
        their spatial gradients gA, gB [U, dim]."""
        kept = self._keep.get(('dd', batch))
        U = None if kept is None else int(kept[0].shape[0])
        n, g = (None, None) if U is None else ((U,), (U, self.dim))
        self._set_ansatz(('ansatzpts', batch), self.lib.vn_set_ansatz_points, batch, (A, B, gA, gB), (n, n, g, g))

    def set_ansatz_rows(self, which, A=None, B=None, a=None, b=None):
        """... on one of the engine's other row sets (vn_set_ansatz_rows): which in 'bic', 'flux', 'periodic', 'obs'; one value
        per row of the set's registration; a, b the derivatives of A, B along the set's own direction (None for a set without
        directions)."""
        if which not in ANSATZ_SETS:
            raise ValueError('ansatz rows: %r is none of %s' % (which, sorted(ANSATZ_SETS)))
        index, key = ANSATZ_SETS[which]
        kept = self._keep.get(key)
        n = None if not kept else (int(kept[0].shape[0]),)
        self._set_ansatz(('ansatzrows', key), self.lib.vn_set_ansatz_rows, index, (A, B, a, b), (n, n, n, n))

    def set_obs_weight(self, weight):
        """lambda of the observation term, without re-registering (vn_set_obs_weight)."""
        self._ck(self.lib.vn_set_obs_weight(self.h, float(weight)))

    def obs_misfit(self):
        """The unweighted misfit O = mean_i[wgt_i r_i^2] of the last evaluation (grad, train_step, eval_loss, objective64, ...)."""
        out = C.c_double(0.0)
        self._ck(self.lib.vn_get_obs_misfit(self.h, C.byref(out)))
        return float(out.value)

    def _set_term(self, key, fn, takes, stream_name, batch, stream, coef, clears):
        """One of the three polynomial terms of `batch` (vn_terms.hip): coef normalised to three doubles; clears(c, stream) tells
        whether the call unregisters the term; else `stream` (one value per interior row, or None) is uploaded and kept alive."""
        c = [] if coef is None else [float(x) for x in np.reshape(np.asarray(coef, dtype=np.float64), -1)]
        if len(c) > 3:
            raise ValueError('%s, got %d' % (takes, len(c)))
        c = c + [0.0] * (3 - len(c))
        # (a term with a learnt coefficient stays registered whatever its values: set_coef_learn)
        mask = getattr(self, '_learnt_coef', None)
        learnt = mask is not None and any(mask[3 * COEF_TERMS.index(key):3 * COEF_TERMS.index(key) + 3])
        if coef is None or (clears(c, stream) and not learnt):
            self._keep.pop((key, batch), None)
            self._ck(fn(self.h, int(batch), None, None))
            return
        if stream is not None:
            t = self.torch
            stream = self.dev(stream.reshape(-1) if isinstance(stream, t.Tensor) else np.reshape(stream, -1))
            # the ABI carries a pointer only: the length the kernels rely on is checked here
            kept = self._keep.get(('int', batch))
            assert kept is None or stream.numel() == kept[0].shape[0], \
                '%s must have one entry per interior row (%s != %s)' % (stream_name, stream.numel(), kept[0].shape[0])
        self._ck(fn(self.h, int(batch), _ptr(stream), (C.c_double * 3)(*c)))
        self._keep[(key, batch)] = stream

    def set_reaction(self, batch, rate=None, coef=None):
        """Register (or, with coef=None or all zero, clear) the reaction term rate * (c1 u + c2 u^2 + c3 u^3) of `batch`
        (vn_set_reaction), after set_interior of that batch: rate one value per interior row or None (rate = 1), coef up to
        three numbers (a shorter list is zero-padded)."""
        self._set_term('react', self.lib.vn_set_reaction, 'a reaction takes at most three coefficients (c1, c2, c3)', 'rate',
                       batch, rate, coef, lambda c, s: not any(c))

    def set_nlflux(self, batch, phi=None, coef=None):
        """Register (or, with coef=None or all zero, clear) the flux term -div(w F(u)), F(u) = f1 u + f2 u^2 + f3 u^3, of `batch`
        (vn_set_nlflux), after set_interior of that batch: phi = sum_d w_d dN/dx_d, one value per interior row, coef up to three
        numbers (a shorter list is zero-padded)."""
        self._set_term('nlflux', self.lib.vn_set_nlflux, 'a flux term takes at most three coefficients (f1, f2, f3)', 'phi',
                       batch, phi, coef, lambda c, s: not any(c))

    def set_nldiff(self, batch, psi=None, coef=None):
        """Register (or, with coef=None, or coef (1, 0, 0) and psi=None, clear) the diffusivity D(u) = d0 + d1 u + d2 u^2 of the
        quasilinear diffusion div(kappa D(u) grad u) of `batch` (vn_set_nldiff), after set_interior of that batch.  The batch's
        gcoef must then be kappa dN/dx alone; psi = sum_d v_d dN/dx_d + N div v, one value per interior row, carries the
        advection (None: no advection).  coef: up to three numbers (a shorter list is zero-padded)."""
        self._set_term('nldiff', self.lib.vn_set_nldiff, 'a diffusivity takes at most three coefficients (d0, d1, d2)', 'psi',
                       batch, psi, coef, lambda c, s: c == [1.0, 0.0, 0.0] and s is None)

    def _set_learn(self, kind, mask, init, lo, hi, lr):
        """Register one learnt vector (vn_set_<kind>_learn): mask, init, lo and hi as vectors of its length n -- nine for the
        coefficients, else the length of `mask` -- with lo / hi defaulting to unbounded; mask=None switches it off."""
        fn, fixed = getattr(self.lib, 'vn_set_%s_learn' % kind), LEARNT[kind][1]
        lead = () if fixed else (0,)
        if mask is None:
            self._ck(fn(self.h, *lead, None, None, None, None, 0.0))
            setattr(self, '_learnt_' + kind, None)
            return
        m = [1 if x else 0 for x in np.asarray(mask).reshape(-1)]
        n = fixed or len(m)
        entries = 'nine entries (reaction, flux, diffusivity: three each)' if fixed else 'one entry per amplitude (%d)' % n

        def vec(a, fill, name):
            v = np.full(n, fill, dtype=np.float64) if a is None else np.asarray(a, dtype=np.float64).reshape(-1)
            if v.size != n:
                raise ValueError('%s must have %s, got %d' % (name, entries, v.size))
            return v
        vec(m, 0, 'mask')
        if init is None or lr is None:
            raise ValueError('set_%s_learn needs init (%s) and lr' % (kind, 'nine values' if fixed else 'one value per amplitude'))
        v0, l, u = vec(init, 0.0, 'init'), vec(lo, -np.inf, 'lo'), vec(hi, np.inf, 'hi')
        dbl = C.c_double * max(n, 1)
        self._ck(fn(self.h, *(() if fixed else (n,)), (C.c_int32 * max(n, 1))(*m), dbl(*v0), dbl(*l), dbl(*u), float(lr)))
        setattr(self, '_learnt_' + kind, m)            # (the mask of a vector that is on)

    def _get_learnt(self, kind, grad, J=None):
        """The values of one learnt vector at the current state (vn_get_*); grad=True: (values, gradient of the last gradient
        evaluation).  J: the length the caller expects (default: the registered one)."""
        name, fixed = LEARNT[kind]
        n = fixed or int(J if J is not None else (len(getattr(self, '_learnt_' + kind, None) or ()) or 1))
        a, g = (C.c_double * n)(), (C.c_double * n)()
        self._ck(getattr(self.lib, 'vn_get_' + name)(self.h, a, g if grad else None, *(() if fixed else (n,))))
        a = np.array(list(a), dtype=np.float64)
        return (a, np.array(list(g), dtype=np.float64)) if grad else a

    def _set_learnt(self, kind, values):
        """Overwrite the values of one learnt vector (vn_set_*)."""
        name, fixed = LEARNT[kind]
        v = np.asarray(values, dtype=np.float64).reshape(-1)
        if fixed and v.size != fixed:
            raise ValueError('coef must have nine entries (reaction, flux, diffusivity: three each), got %d' % v.size)
        self._ck(getattr(self.lib, 'vn_set_' + name)(self.h, (C.c_double * max(v.size, 1))(*v), *(() if fixed else (int(v.size),))))

    def set_learnt_prior(self, kind, weight=0.0, matrix=None, mean=None, l1=None):
        """Regularise the learnt vector `kind` (a key of LEARNT; vn_set_learnt_prior): the quadratic prior
        1/2 weight (a - mean)^T matrix (a - mean) -- matrix [J, J] symmetric positive semi-definite (None: the identity), mean [J]
        (None: zeros) -- whose gradient joins the masked entries' folded gradient in fp64, and the L1 weights l1 [J] (or one number
        for all; None: none) of the proximal shrinkage by lr_t l1[j] that ends their step.  weight=0 with l1=None clears the prior;
        so does every set_<kind>_learn.  The reported losses do not contain either term: learnt_prior(kind) reads them."""
        if kind not in LEARNT:
            raise ValueError('unknown learnt vector %r (one of %s)' % (kind, ', '.join(LEARNT)))
        if getattr(self, '_learnt_' + kind, None) is None:         # (not learnt: the engine's sentence)
            self._ck(self.lib.vn_set_learnt_prior(self.h, list(LEARNT).index(kind), 0, 0.0, None, None, None))
        n = len(getattr(self, '_learnt_' + kind))

        def arr(a, shape, name):
            if a is None:
                return None
            v = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), shape) if np.ndim(a) == 0 and name == 'l1'
                                     else np.asarray(a, dtype=np.float64))
            if v.shape != shape:
                raise ValueError('%s of the %s prior must have shape %s, got %s' % (name, kind, shape, v.shape))
            return v
        R, mu, lam = arr(matrix, (n, n), 'matrix'), arr(mean, (n,), 'mean'), arr(l1, (n,), 'l1')
        dp = lambda v: None if v is None else v.ctypes.data_as(C.POINTER(C.c_double))
        self._ck(self.lib.vn_set_learnt_prior(self.h, list(LEARNT).index(kind), n, float(weight), dp(R), dp(mu), dp(lam)))

    def learnt_prior(self, kind):
        """(Q, sum_j l1[j] |a_j|) of the learnt vector `kind` at its current values (vn_get_learnt_prior); (0, 0) without a prior."""
        if kind not in LEARNT:
            raise ValueError('unknown learnt vector %r (one of %s)' % (kind, ', '.join(LEARNT)))
        out = (C.c_double * 2)()
        self._ck(self.lib.vn_get_learnt_prior(self.h, list(LEARNT).index(kind), out))
        return float(out[0]), float(out[1])

    def _set_basis(self, key, fn, batch, streams, trailing):
        """Register (streams=None: clear) the J basis streams of `batch`, uploaded as [J, rows, *trailing] and kept alive."""
        if streams is None:
            self._keep.pop((key, batch), None)
            self._ck(fn(self.h, int(batch), None, 0))
            return
        if not isinstance(streams, self.torch.Tensor):
            streams = np.asarray(streams, dtype=np.float32)
        # the rows a stream runs over: the batch's interior rows, for the BC/IC labels the rows of the set they belong to, for the
        # flux datum and Robin coefficient the flux rows
        kept = (self._keep.get('bic') if batch < 0 else self._keep.get(('bbic', batch))) if key == 'bicbasis' \
            else self._keep.get('flux') if key == 'fbcbasis' else self._keep.get(('int', batch))
        J = int(streams.shape[0])
        streams = self.dev(streams.reshape(J, -1, *trailing))
        # the ABI carries a pointer only: the length the kernels rely on is checked here
        assert kept is None or streams.shape[1] == kept[0].shape[0], \
            'every basis stream must have one entry per %s row (%s != %s)' % (
                {'bicbasis': 'BC/IC', 'fbcbasis': 'flux'}.get(key, 'interior'), streams.shape[1], kept[0].shape[0])
        self._keep.pop((key, batch), None)         # (a failed call leaves the batch without a basis)
        self._ck(fn(self.h, int(batch), _ptr(streams), J))
        self._keep[(key, batch)] = streams

    def set_coef_learn(self, mask=None, init=None, lo=None, hi=None, lr=None):
        """Inverse mode (vn_set_coef_learn): learn the masked entries of the nine polynomial coefficients -- index 0..2 reaction
        (c1, c2, c3), 3..5 flux (f1, f2, f3), 6..8 diffusivity (d0, d1, d2) -- next to the parameters.  init: the nine starting
        values, which every registered term of every batch then reads from the engine's device vector; lo / hi: the clamp (None:
        unbounded; entries may be +-inf); lr: their Adam rate.  mask=None switches learning off and frees everything."""
        self._set_learn('coef', mask, init, lo, hi, lr)

    def get_coefs(self, grad=False):
        """The nine coefficients at the current state (vn_get_coefs); grad=True: (coef, gradient of the last gradient evaluation)."""
        return self._get_learnt('coef', grad)

    def set_coefs(self, coef):
        """Overwrite the nine coefficients (vn_set_coefs): rounded to fp32, not clamped; the Adam slots stay."""
        self._set_learnt('coef', coef)

    def set_source_basis(self, batch, phi=None):
        """Register (phi=None: clear) the source basis of `batch` (vn_set_source_basis), after set_interior of that batch: phi is
        [J, rows] (or J arrays of one value per interior row), J <= 64.  The engine must have been created with isSource=True."""
        self._set_basis('srcbasis', self.lib.vn_set_source_basis, batch, phi, ())

    def set_source_learn(self, mask=None, init=None, lo=None, hi=None, lr=None):
        """Source identification (vn_set_source_learn): learn the masked amplitudes a_j of the batches' source bases next to the
        parameters.  mask: J booleans; init: the J starting values (unmasked entries keep theirs); lo / hi: the clamp (None:
        unbounded; entries may be +-inf); lr: their Adam rate.  mask=None switches learning off and frees everything."""
        self._set_learn('source', mask, init, lo, hi, lr)

    def get_source_amps(self, grad=False, J=None):
        """The amplitudes at the current state (vn_get_source_amps); grad=True: (amp, gradient of the last gradient evaluation)."""
        return self._get_learnt('source', grad, J)

    def set_source_amps(self, amp):
        """Overwrite the amplitudes (vn_set_source_amps): rounded to fp32, not clamped; the Adam slots stay."""
        self._set_learnt('source', amp)

    def set_field_basis(self, batch, G=None):
        """Register (G=None: clear) the field basis of `batch` (vn_set_field_basis), after set_interior of that batch: G is
        [J, rows, dim] (J streams laid out like gcoef), J <= 32."""
        self._set_basis('fldbasis', self.lib.vn_set_field_basis, batch, G, (self.dim,))

    def set_field_learn(self, mask=None, init=None, lo=None, hi=None, lr=None):
        """Field identification (vn_set_field_learn): learn the masked amplitudes b_j of the batches' field bases next to the
        parameters.  mask: J booleans; init: the J starting values (unmasked entries keep theirs); lo / hi: the clamp (None:
        unbounded; entries may be +-inf); lr: their Adam rate.  mask=None switches learning off and frees everything."""
        self._set_learn('field', mask, init, lo, hi, lr)

    def get_field_amps(self, grad=False, J=None):
        """The amplitudes at the current state (vn_get_field_amps); grad=True: (amp, gradient of the last gradient evaluation)."""
        return self._get_learnt('field', grad, J)

    def set_field_amps(self, amp):
        """Overwrite the amplitudes (vn_set_field_amps): rounded to fp32, not clamped; the Adam slots stay."""
        self._set_learnt('field', amp)

    def set_bic_basis(self, batch, B=None):
        """Register (B=None: clear) the basis of the BC/IC labels (vn_set_bic_basis): batch=-1 for the rows of set_bic, else the
        batch's own copy (after set_batch_bic of that batch).  B is [J, nB] (or J arrays of one value per BC/IC row), J <= 64."""
        self._set_basis('bicbasis', self.lib.vn_set_bic_basis, batch, B, ())

    def set_bic_learn(self, mask=None, init=None, lo=None, hi=None, lr=None):
        """Boundary data identification (vn_set_bic_learn): learn the masked amplitudes a_j of the BC/IC label bases next to the
        parameters.  mask: J booleans; init: the J starting values (unmasked entries keep theirs); lo / hi: the clamp (None:
        unbounded; entries may be +-inf); lr: their Adam rate.  mask=None switches learning off and frees everything."""
        self._set_learn('bic', mask, init, lo, hi, lr)

    def get_bic_amps(self, grad=False, J=None):
        """The amplitudes at the current state (vn_get_bic_amps); grad=True: (amp, gradient of the last gradient evaluation)."""
        return self._get_learnt('bic', grad, J)

    def set_bic_amps(self, amp):
        """Overwrite the amplitudes (vn_set_bic_amps): rounded to fp32, not clamped; the Adam slots stay."""
        self._set_learnt('bic', amp)

    def set_fluxbc_basis(self, S=None, J_flux=0):
        """Register (S=None: clear) the basis of the flux rows' datum and Robin coefficient (vn_set_fluxbc_basis), after
        set_flux_bc: S is [J, nF] (or J arrays of one value per flux row), J <= 64 -- the first J_flux streams belong to the flux
        datum g/a, the other J - J_flux to the coefficient b/a."""
        J_flux = int(J_flux)

        def fn(h, batch, ptr, J):      # (the flux rows are engine-wide: no batch index in the ABI)
            return self.lib.vn_set_fluxbc_basis(h, ptr, J_flux if J else 0, J - J_flux if J else 0)
        if S is not None and not 0 <= J_flux <= len(S):
            raise ValueError('J_flux = %d must lie in [0, %d], the number of streams' % (J_flux, len(S)))
        self._set_basis('fbcbasis', fn, -1, S, ())

    def set_fluxbc_learn(self, mask=None, init=None, lo=None, hi=None, lr=None):
        """Flux boundary identification (vn_set_fluxbc_learn): learn the masked amplitudes a_j of the flux rows' bases (flux datum
        first, then Robin coefficient) next to the parameters.  mask: J booleans; init: the J starting values (unmasked entries
        keep theirs); lo / hi: the clamp (None: unbounded; entries may be +-inf); lr: their Adam rate.  mask=None switches learning
        off and frees everything."""
        self._set_learn('fluxbc', mask, init, lo, hi, lr)

    def get_fluxbc_amps(self, grad=False, J=None):
        """The amplitudes at the current state (vn_get_fluxbc_amps); grad=True: (amp, gradient of the last gradient evaluation)."""
        return self._get_learnt('fluxbc', grad, J)

    def set_fluxbc_amps(self, amp):
        """Overwrite the amplitudes (vn_set_fluxbc_amps): rounded to fp32, not clamped; the Adam slots stay."""
        self._set_learnt('fluxbc', amp)

    def _n_k(self, batch):
        kept = self._keep.get(('int', batch))
        return None if kept is None else int(kept[0].shape[0]) // self.integNum

    def set_tf_weights(self, batch, omega=None):
        """Register (or, with omega=None, clear) per-test-function loss weights of `batch` (vn_set_tf_weights), after set_interior
        of that batch: var = sum_k omega_k lossVec[k], omega held constant for the gradient, lossVec itself stays unweighted.
        omega: one value >= 0 per test function; a device tensor is registered as it is (also a view that is not 16-byte
        aligned), anything else is uploaded.  Replaces a causal registration of the batch."""
        if omega is None:
            self._ck(self.lib.vn_set_tf_weights(self.h, int(batch), None))
            self._keep.pop(('tfw', batch), None)
            return
        t = self.torch
        if isinstance(omega, t.Tensor) and omega.device == self.device and omega.dtype == t.float32 and omega.is_contiguous():
            omega = omega.reshape(-1)
        else:
            omega = self.dev(omega.reshape(-1) if isinstance(omega, t.Tensor) else np.reshape(omega, -1))
        # the ABI carries a pointer only: the length the kernels rely on is checked here
        n_k = self._n_k(batch)
        assert n_k is None or omega.numel() == n_k, 'omega must have one entry per test function (%s != %s)' % (omega.numel(), n_k)
        self._ck(self.lib.vn_set_tf_weights(self.h, int(batch), _ptr(omega)))
        self._keep[('tfw', batch)] = omega
        self._keep.pop(('causal', batch), None)
        self._keep.pop(('adapt', batch), None)

    def set_causal(self, batch, slab=None, n_slabs=None, eps=0.0):
        """Register (or, with slab=None, clear) the causal time-slab weights of `batch` (vn_set_causal), after set_interior of
        that batch: slab one id in [0, n_slabs) per test function (n_slabs None: max id + 1), omega_k = exp(-eps * sum of the
        mean losses of the earlier slabs), recomputed on the device at every step.  The ids are validated and copied by the
        call.  Replaces a static registration of the batch."""
        if slab is None:
            self._ck(self.lib.vn_set_causal(self.h, int(batch), None, 0, 0.0))
            self._keep.pop(('causal', batch), None)
            return
        t = self.torch
        slab = (slab if isinstance(slab, t.Tensor) else t.as_tensor(np.ascontiguousarray(slab))).to(
            device=self.device, dtype=t.int32).reshape(-1).contiguous()
        n_k = self._n_k(batch)
        assert n_k is None or slab.numel() == n_k, 'slab must have one entry per test function (%s != %s)' % (slab.numel(), n_k)
        if n_slabs is None:
            n_slabs = int(slab.max().item()) + 1 if slab.numel() else 1
        self._ck(self.lib.vn_set_causal(self.h, int(batch), _ptr(slab), int(n_slabs), float(eps)))
        self._keep[('causal', batch)] = (int(n_slabs), float(eps))      # (the engine copied the ids)
        self._keep.pop(('tfw', batch), None)
        self._keep.pop(('adapt', batch), None)

    def causal_weights(self, batch=0):
        """omega_s [n_slabs] float64 of the batch's causal registration at the current parameters (vn_causal_weights): one
        loss-only evaluation.  Changes no engine state."""
        kept = self._keep.get(('causal', batch))
        n = kept[0] if kept is not None else 1                          # (no registration: the engine says so)
        out = (C.c_double * n)()
        self._ck(self.lib.vn_causal_weights(self.h, int(batch), out, n))
        return np.array(out, dtype=np.float64)

    # -- self-adaptive test-function weights -------------------------------------------------
    # What the adaptive states of the batches and of the BC/IC rows' parts share: `n` is the holder's count (None: not known here,
    # the engine checks), `key` its batch or part index.
    def _adapt_lambda_init(self, lambda_init, n, exc, text):
        """lambda_init as a flat float32 device tensor (one that already is one is handed through, no copy), or None; `exc(text %
        (its length, n))` when the length is not n."""
        if lambda_init is None:
            return None
        lam = self.dev(lambda_init.reshape(-1) if isinstance(lambda_init, self.torch.Tensor) else np.reshape(lambda_init, -1))
        if n is not None and lam.numel() != n:
            raise exc(text % (lam.numel(), n))
        return lam

    def _adapt_read(self, get, key, n, spec, arrays, extra=()):
        """The dict of tf_adapt / bic_adapt around one get call: 'lambda', 'omega', 'slots' (sa, else None), the `extra` [n]
        arrays behind them, 'stats'."""
        names = ('lambda', 'omega', 'slots') + extra
        st = (C.c_double * 6)()
        out = dict.fromkeys(names)
        if arrays:
            for k in names:
                if k != 'slots':
                    out[k] = np.empty(n, np.float32)
            if isinstance(spec, dict) and spec['rule'] == 'sa':
                out['slots'] = np.empty((2, n), np.float32)
        self._ck(get(self.h, key, *[None if out[k] is None else out[k].ctypes.data for k in names], st))
        out['stats'] = dict(zip(('min', 'max', 'mean', 'share', 'Z', 'tau'), [float(x) for x in st]))
        return out

    def _adapt_write(self, put, key, who, n, lam, slots, tau):
        """lam [n] and slots [2, n] (or None) as flat float32 host arrays of checked length around one put call."""
        lam = np.ascontiguousarray(lam, dtype=np.float32).ravel()
        if n is not None and lam.size != n:
            raise ValueError('%s: expected %d lambdas, got %d' % (who, n, lam.size))
        if slots is not None:
            slots = np.ascontiguousarray(slots, dtype=np.float32).ravel()
            if slots.size != 2 * lam.size:
                raise ValueError('%s: expected %d slot values, got %d' % (who, 2 * lam.size, slots.size))
        self._ck(put(self.h, key, lam.ctypes.data, None if slots is None else slots.ctypes.data, int(tau)))

    def set_tf_adapt(self, batch, spec=None, lambda_init=None):
        """Register (or, with spec=None, clear) self-adaptive weights of `batch` (vn_set_tf_adapt), after set_interior of that
        batch.  spec: 'rba', 'sa' or a dict (tf_adapt_spec).  lambda_init: one value >= 0 per test function (a device tensor of
        any alignment is passed as it is; validated and copied by the call), default: spec's init everywhere.  Replaces a static
        or causal registration of the batch."""
        spec = tf_adapt_spec(spec)
        if spec is None:
            self._ck(self.lib.vn_set_tf_adapt(self.h, int(batch), 0, None, None))
            self._keep.pop(('adapt', batch), None)
            return
        lam = self._adapt_lambda_init(lambda_init, self._n_k(batch), AssertionError,
                                      'lambda_init must have one entry per test function (%s != %s)')
        rule, par = tf_adapt_par(spec)
        self._ck(self.lib.vn_set_tf_adapt(self.h, int(batch), rule, (C.c_double * 10)(*par), _ptr(lam)))
        self._keep[('adapt', batch)] = spec                              # (the engine copied the initial values)
        self._keep.pop(('tfw', batch), None)
        self._keep.pop(('causal', batch), None)

    def adapt_batches(self):
        """The batches that carry an adaptive registration, in increasing order."""
        return sorted(k[1] for k in self._keep if isinstance(k, tuple) and k[0] == 'adapt')

    def tf_adapt(self, batch=0, arrays=True):
        """The committed adaptive state of `batch` (vn_get_tf_adapt): {'lambda', 'omega' [n_k] float32, 'slots' [2, n_k] (sa) or
        None, 'stats': {'min', 'max', 'mean', 'share', 'Z', 'tau'}}; arrays=False reads the statistics alone.  Synchronises;
        changes no engine state."""
        spec = self._keep.get(('adapt', batch))
        return self._adapt_read(self.lib.vn_get_tf_adapt, int(batch), self._n_k(batch) or 0, spec, arrays)

    def set_tf_adapt_state(self, batch, lam, slots=None, tau=0):
        """Puts an adaptive state back (vn_set_tf_adapt_state): lambda [n_k], slots [2, n_k] (sa; None: zeros), tau.  omega, Z and
        the statistics are rebuilt on the device.  Synchronises."""
        self._adapt_write(self.lib.vn_set_tf_adapt_state, int(batch), 'set_tf_adapt_state', self._n_k(batch), lam, slots, tau)

    # -- weights on the BC/IC rows -------------------------------------------------------------
    BIC_PARTS = {'bc': 0, 'ic': 1}

    def _bic_part(self, part):
        if part not in self.BIC_PARTS and part not in (0, 1):
            raise ValueError("the part of the BC/IC rows must be 'bc' (0) or 'ic' (1) (got %r)" % (part,))
        return self.BIC_PARTS.get(part, part)

    def bic_rows(self, part):
        """Rows of a part of the registered BC/IC rows as the engine counts them (a steady engine has no 'ic' rows)."""
        return getattr(self, '_bic_rows', (0, 0))[self._bic_part(part)]

    def bic_parts(self):
        """{part name: 'static' or the adaptive spec} of the parts that carry a registration."""
        return dict(self._keep.get('bicw') or {})

    def set_bic_weights(self, omega=None, normalize=False):
        """Register (or, with omega=None, clear -- both parts, whatever they hold) static weights on the BC/IC rows
        (vn_set_bic_weights), after set_bic: one value >= 0 per row the engine counts, validated and copied by the call;
        normalize applies per part.  Replaces every registration of the parts that have rows."""
        if omega is None:
            self._ck(self.lib.vn_set_bic_weights(self.h, None, 0))
            self._keep.pop('bicw', None)
            return
        t = self.torch
        om = self.dev(omega.reshape(-1) if isinstance(omega, t.Tensor) else np.reshape(omega, -1))
        n = sum(getattr(self, '_bic_rows', (0, 0)))
        if om.numel() != n:
            raise ValueError('set_bic_weights: expected one weight per BC/IC row (%d), got %d' % (n, om.numel()))
        self._ck(self.lib.vn_set_bic_weights(self.h, _ptr(om), 1 if normalize else 0))
        self._keep['bicw'] = {name: 'static' for name, s in self.BIC_PARTS.items() if self._bic_rows[s] > 0}

    def set_bic_adapt(self, part, spec=None, lambda_init=None):
        """Register (or, with spec=None, clear) self-adaptive weights on one part ('bc' / 'ic') of the BC/IC rows
        (vn_set_bic_adapt), after set_bic.  spec and lambda_init as for set_tf_adapt, with the part's rows in place of the test
        functions.  Replaces a static or an adaptive registration of that part."""
        s = self._bic_part(part)
        name = ('bc', 'ic')[s]
        spec = tf_adapt_spec(spec)
        kept = dict(self._keep.get('bicw') or {})
        if spec is None:
            self._ck(self.lib.vn_set_bic_adapt(self.h, s, 0, None, None))
            kept.pop(name, None)
        else:
            lam = self._adapt_lambda_init(lambda_init, self.bic_rows(s), ValueError,
                                          'set_bic_adapt: lambda_init must have one entry per ' + name + ' row (%d != %d)')
            rule, par = tf_adapt_par(spec)
            self._ck(self.lib.vn_set_bic_adapt(self.h, s, rule, (C.c_double * 10)(*par), _ptr(lam)))
            kept[name] = spec                                             # (the engine copied the initial values)
        if kept:
            self._keep['bicw'] = kept
        else:
            self._keep.pop('bicw', None)

    def bic_adapt(self, part, arrays=True):
        """The committed state of a registered part (vn_get_bic_adapt): {'lambda', 'omega', 'lossfield' [n_s] float32 (the
        unweighted l_i of the last evaluation), 'slots' [2, n_s] (sa) or None, 'stats': {'min', 'max', 'mean', 'share', 'Z',
        'tau'}}; arrays=False reads the statistics alone.  Synchronises; changes no engine state."""
        s = self._bic_part(part)
        spec = (self._keep.get('bicw') or {}).get(('bc', 'ic')[s])
        return self._adapt_read(self.lib.vn_get_bic_adapt, s, self.bic_rows(s), spec, arrays, ('lossfield',))

    def set_bic_adapt_state(self, part, lam, slots=None, tau=0):
        """Puts the state of an adaptive part back (vn_set_bic_adapt_state): lambda [n_s], slots [2, n_s] (sa; None: zeros), tau.
        omega, Z and the statistics are rebuilt on the device.  Synchronises."""
        s = self._bic_part(part)
        self._adapt_write(self.lib.vn_set_bic_adapt_state, s, 'set_bic_adapt_state', self.bic_rows(s), lam, slots, tau)

    # -- learnt weight scales --------------------------------------------------------------
    def set_reparam(self, mode=None, per='neuron', n=1.0, s_init=None, lr=None):
        """Learnt weight scales theta_eff = f(s) (.) V (include/varnet_hip.h, vn_set_reparam).  mode 'rwf': f = exp(s), one scale
        per output neuron of every layer, weights only; 'slope': f = n s, hidden layers, weights and bias, `per` 'neuron' or
        'layer'.  s_init: the S initial scales, or a scalar for all (default: 0 for rwf, 1 / n for slope, both f = 1).  lr: the
        scales' learning rate (default: the network's).  mode None clears the registration."""
        if mode is None:
            self._ck(self.lib.vn_set_reparam(self.h, 0, 0, 1.0, None, 0, 0.0))
            self._reparam = None
            return
        if mode not in REPARAM_MODES:
            raise ValueError("reparam mode must be 'rwf' or 'slope' (got %r)" % (mode,))
        if per not in REPARAM_PER:
            raise ValueError("reparam granularity must be 'neuron' or 'layer' (got %r)" % (per,))
        S = reparam_count(mode, per, self.inpDim, self.layerWidth)
        if s_init is None:
            s_init = 0.0 if mode == 'rwf' else 1.0 / float(n)
        s0 = np.ascontiguousarray(np.broadcast_to(np.asarray(s_init, dtype=np.float64), (S,)) if np.ndim(s_init) == 0
                                  else np.asarray(s_init, dtype=np.float64).ravel())
        lr = self.cfg.lr if lr is None else float(lr)
        self._ck(self.lib.vn_set_reparam(self.h, REPARAM_MODES[mode], REPARAM_PER[per], float(n),
                                         s0.ctypes.data_as(C.POINTER(C.c_double)), int(s0.size), lr))
        self._reparam = (mode, per, float(n), S)

    @property
    def reparam(self):
        """(mode, per, n, S) of the registered weight scales, or None."""
        return getattr(self, '_reparam', None)

    def get_reparam(self):
        """{'V': [P], 's': [S], 'f': [S] fl32(f(s)) as last formed, 'slots': [2, S]} of the registered scales (synchronises)."""
        S = self.reparam[3] if self.reparam else 0
        out = {'V': np.empty(self.P, np.float32), 's': np.empty(S, np.float32), 'f': np.empty(S, np.float32),
               'slots': np.empty((2, S), np.float32)}
        self._ck(self.lib.vn_get_reparam(self.h, out['V'].ctypes.data, out['s'].ctypes.data, out['f'].ctypes.data,
                                         out['slots'].ctypes.data))
        return out

    def set_reparam_state(self, V=None, s=None, slots=None):
        """Overwrites V, s and / or the scale slots [2, S], then rebuilds theta_eff (synchronises)."""
        S = self.reparam[3] if self.reparam else 0
        arrs = []
        for a, n_ in ((V, self.P), (s, S), (slots, 2 * S)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float32).ravel()
                if a.size != n_:
                    raise ValueError('set_reparam_state: expected %d values, got %d' % (n_, a.size))
            arrs.append(a)
        self._ck(self.lib.vn_set_reparam_state(self.h, *[None if a is None else a.ctypes.data for a in arrs]))

    def reparam_grad(self):
        """(g_V [P], g_s [S]) of the gradient buffer as it stands, by the stage's dry form (synchronises; no state changes)."""
        S = self.reparam[3] if self.reparam else 0
        gV, gs = np.empty(self.P, np.float32), np.empty(S, np.float32)
        self._ck(self.lib.vn_reparam_grad(self.h, gV.ctypes.data, gs.ctypes.data))
        return gV, gs

    def set_weights(self, w):
        arr = (C.c_double * 3)(*[float(x) for x in w])
        self._ck(self.lib.vn_set_weights(self.h, arr))

    # -- compute -------------------------------------------------------------------------
    def bind_grad_buffer(self):
        """Torch-owned [P+4] gradient buffer so torch.distributed can all-reduce it."""
        if self.gradbuf is None:
            self.gradbuf = self.torch.zeros(self.P + 4, dtype=self.torch.float32, device=self.device)
            self._ck(self.lib.vn_bind_grad_buffer(self.h, _ptr(self.gradbuf)))
        return self.gradbuf

    def grad(self, batch=0):
        self._ck(self.lib.vn_grad(self.h, batch))

    def apply(self):
        self._ck(self.lib.vn_apply(self.h))

    # -- per-term gradients (adaptive loss balancing) ---------------------------------------
    def term_stats(self, T):
        """Statistics of K <= 4 fp32 device vectors T [K, n] (vn_term_stats): {'stats': [K, 3] = (sumsq, sumabs, maxabs),
        'gram': [K, K]}, fp64, reduced on the device in an order that depends on n alone.  Synchronises."""
        if T is None:
            K, n, ptr = 1, 1, None                 # (a null pointer is the library's to refuse)
        else:
            if T.dim() == 1:
                T = T.reshape(1, -1)
            if T.dtype != self.torch.float32 or not T.is_contiguous() or T.dim() != 2:
                raise ValueError('term_stats: T must be a contiguous float32 tensor [K, n]')
            K, n, ptr = int(T.shape[0]), int(T.shape[1]), _ptr(T)
        stats, gram = np.zeros((max(K, 1), 3)), np.zeros((max(K, 1), max(K, 1)))
        self._ck(self.lib.vn_term_stats(self.h, ptr, K, n, stats.ctypes.data_as(C.POINTER(C.c_double)),
                                        gram.ctypes.data_as(C.POINTER(C.c_double))))
        return {'stats': stats, 'gram': gram}

    def term_grads(self, batches=(0,), terms=None, grads=False):
        """Per-term gradients G_k of the objective over `batches` and their statistics (vn_term_grads): G_k is what grad() leaves
        under the one-hot weights of term k ('bc', 'ic', 'var', 'obs'), summed over the batches.  Returns {'terms': TERMS,
        'norm2', 'mean_abs', 'max_abs', 'value', 'sumsq', 'sumabs': [4], 'gram': [4, 4], 'G': [4, P] tensor (grads=True)}; a term that is not
        in `terms` (default: all) or has no rows holds zeros.  The weights are the caller's afterwards; the gradient buffer and the
        loss scalars are clobbered until the next grad().  Synchronises once."""
        if terms is None:
            mask = (1 << len(TERMS)) - 1
        elif isinstance(terms, int):
            mask = int(terms)
        else:
            mask = 0
            for t in terms:
                if t not in TERMS:
                    raise ValueError('term_grads: unknown term %r (one of %s)' % (t, ', '.join(TERMS)))
                mask |= 1 << TERMS.index(t)
        batches = [int(b) for b in batches]
        arr = (C.c_int32 * max(len(batches), 1))(*batches)
        n_t = len(TERMS)
        stats, gram, value = np.zeros((n_t, 3)), np.zeros((n_t, n_t)), np.zeros(n_t)
        G = self.torch.empty((n_t, self.P), dtype=self.torch.float32, device=self.device) if grads else None
        dp = C.POINTER(C.c_double)
        self._ck(self.lib.vn_term_grads(self.h, arr, len(batches), mask, stats.ctypes.data_as(dp), gram.ctypes.data_as(dp),
                                        value.ctypes.data_as(dp), _ptr(G)))
        out = {'terms': TERMS, 'sumsq': stats[:, 0].copy(), 'norm2': np.sqrt(stats[:, 0]), 'sumabs': stats[:, 1].copy(),
               'mean_abs': stats[:, 1] / self.P,
               'max_abs': stats[:, 2].copy(), 'value': value, 'gram': gram}
        if grads:
            out['G'] = G
        return out

    def train_step(self, batch=0, loss_out=None):
        self._ck(self.lib.vn_train_step(self.h, batch, _ptr(loss_out)))

    def train_epoch(self, batches, loss_acc=None):
        """len(batches) optimizer steps in one host call; each step's pre-update loss is added to the
        device scalar `loss_acc` (VarNetUtility.py:1043-1045)."""
        arr = self._epoch_arrays.get(batches) if isinstance(batches, tuple) else None       # (a tuple of ids: its ctypes array is kept)
        if arr is None:
            arr = (C.c_int32 * len(batches))(*[int(b) for b in batches])
            if isinstance(batches, tuple) and len(self._epoch_arrays) < 4096:
                self._epoch_arrays[batches] = arr
        self._ck(self.lib.vn_train_epoch(self.h, arr, len(batches), _ptr(loss_acc)))

    def lbfgs_step(self, batch=0, max_trials=20):
        """One L-BFGS iteration on the objective `grad(batch)` (vn_lbfgs_step; engines made with optimizer_name='lbfgs').
        Returns the `info` fields by name (LBFGS_INFO): status 0 accepted, 1 no trial accepted and the ring dropped, 2 stalled;
        f_k, f_next and the components at the new parameters, the accepted step t, trials used, g.d, pairs in the ring."""
        out = (C.c_double * 10)()
        self._ck(self.lib.vn_lbfgs_step(self.h, int(batch), int(max_trials), out))
        info = dict(zip(LBFGS_INFO, out))
        for k in ('status', 'trials', 'pairs'):
            info[k] = int(info[k])
        return info

    def lbfgs_loss64(self, on=True):
        """L-BFGS engines: take f_k and every trial's loss of lbfgs_step from the fp64 objective (vn_lbfgs_loss64); default off."""
        self._ck(self.lib.vn_lbfgs_loss64(self.h, 1 if on else 0))

    def objective64(self, batch=0, theta=None, grad=True, lossVec=False):
        """The objective of `grad(batch)` and its gradient in double precision on the device (vn_objective_f64).
        theta: float64 tensor of P entries, or None for the engine's own parameters widened.  Returns
        ([loss, BC, IC, var], gradient [P] float64 or None, lossVec [n_k] float64 or None).  Changes no engine state."""
        t = self.torch
        out = (C.c_double * 4)()
        th = None
        if theta is not None:
            th = self.dev(theta, t.float64).reshape(-1)
            if th.numel() != self.P:
                raise ValueError('theta must hold P = %d entries, got %d' % (self.P, th.numel()))
        g = t.empty(self.P, dtype=t.float64, device=self.device) if grad else None
        lv = None
        if lossVec:
            n_k = self._keep[('int', batch)][0].shape[0] // self.integNum
            lv = t.empty(n_k, dtype=t.float64, device=self.device)
        self._ck(self.lib.vn_objective_f64(self.h, int(batch), _ptr(th), _ptr(g), _ptr(lv), out))
        return list(out), g, lv

    def eval_loss(self, batch=0, lossVec=False, fp64=False):
        if fp64:
            out, _, lv = self.objective64(batch, grad=False, lossVec=lossVec)
            return out, lv
        out = (C.c_double * 4)()
        lv = None
        if lossVec:
            n_k = self._keep[('int', batch)][0].shape[0] // self.integNum
            lv = self.torch.empty(n_k, dtype=self.torch.float32, device=self.device)
        self._ck(self.lib.vn_eval_loss(self.h, batch, out, _ptr(lv)))
        return list(out), lv

    def forward(self, X):
        X = self.dev(X)
        u = self.torch.empty(X.shape[0], dtype=self.torch.float32, device=self.device)
        self._ck(self.lib.vn_forward(self.h, _ptr(X), X.shape[0], _ptr(u)))
        return u

    def forward_grad(self, X):
        """(u [n], du/dx [n, dim]) at X: tf.gradients(model(Input), Input) of TFModel.py:536-541, one pass."""
        X = self.dev(X)
        u = self.torch.empty(X.shape[0], dtype=self.torch.float32, device=self.device)
        g = self.torch.empty((X.shape[0], self.dim), dtype=self.torch.float32, device=self.device)
        self._ck(self.lib.vn_forward_grad(self.h, _ptr(X), X.shape[0], _ptr(u), _ptr(g)))
        return u, g

    def forward_f64(self, X):
        t = self.torch
        X = self.dev(X, t.float64)
        u = t.empty(X.shape[0], dtype=t.float64, device=self.device)
        self._ck(self.lib.vn_forward_f64(self.h, _ptr(X), X.shape[0], _ptr(u)))
        return u

    def _grad_u(self, X, fp64):
        """(u [n], du/dx [n, dim]) at X for the residual's nonlinear terms.  fp32: forward_grad.  fp64: vn_residual_f64 is affine in
        vel with slope -du/dx_d, so `dim` calls with unit velocities against one call with vel = 0 give the gradient."""
        t = self.torch
        if not fp64:
            return self.forward_grad(X)
        n = X.shape[0]
        one = t.ones(n, dtype=t.float64, device=self.device)
        vel = t.zeros((n, self.dim), dtype=t.float64, device=self.device)
        u = t.empty(n, dtype=t.float64, device=self.device)
        r0 = t.empty(n, dtype=t.float64, device=self.device)
        self._ck(self.lib.vn_residual_f64(self.h, _ptr(X), _ptr(one), _ptr(vel), None, None, n, _ptr(u), _ptr(r0)))
        g = t.empty((n, self.dim), dtype=t.float64, device=self.device)
        rd = t.empty(n, dtype=t.float64, device=self.device)
        for d in range(self.dim):
            vel.zero_()
            vel[:, d] = 1.0
            self._ck(self.lib.vn_residual_f64(self.h, _ptr(X), _ptr(one), _ptr(vel), None, None, n, _ptr(u), _ptr(rd)))
            g[:, d] = r0 - rd
        return u, g

    def residual(self, X, diff, vel, source=None, diff_dx=None, fp64=False, reaction=None, nlflux=None, nldiff=None):
        """(u, strong residual) at X.  reaction=(rate, coef): the residual gains rate * (c1 u + c2 u^2 + c3 u^3), rate a number,
        one value per point or None (1).  nlflux=(w, coef, div_w): the residual gains -(F'(u) w . grad u + F(u) div w),
        F(u) = f1 u + f2 u^2 + f3 u^3, w [n, dim] (or `dim` numbers), div_w one value per point, a number or None (0).
        nldiff=coef (d0, d1, d2): the diffusion term becomes div(diff D(u) grad u), D(u) = d0 + d1 u + d2 u^2, with no new kernel:
        the residual entry point runs with diff -> diff D(u) and diff_dx -> D(u) diff_dx, and D'(u) diff |grad u|^2 is added;
        u and grad u come from forward_grad (fp32) or from `dim` + 1 calls of vn_residual_f64 with unit velocities (fp64)."""
        t = self.torch
        dt = t.float64 if fp64 else t.float32
        X = self.dev(X, dt)
        n = X.shape[0]
        diff = self.dev(np.reshape(diff, -1), dt)
        vel = self.dev(np.reshape(vel, (n, self.dim)), dt)
        source = None if source is None else self.dev(np.reshape(source, -1), dt)
        diff_dx = None if diff_dx is None else self.dev(np.reshape(diff_dx, (n, self.dim)), dt)
        u = t.empty(n, dtype=dt, device=self.device)
        r = t.empty(n, dtype=dt, device=self.device)
        fu = dterm = None
        if nldiff is not None:
            dc = [float(x) for x in np.reshape(np.asarray(nldiff, dtype=np.float64), -1)]
            dc = dc + [0.0] * (3 - len(dc))
            u0, gu = self._grad_u(X, fp64)
            Du = dc[0] + u0 * (dc[1] + u0 * dc[2])
            # div(kappa D(u) grad u) = D kappa Lap u + D grad kappa . grad u + D'(u) kappa |grad u|^2
            dterm = (dc[1] + 2.0 * dc[2] * u0) * diff * (gu * gu).sum(1)
            diff = diff * Du
            if diff_dx is not None:
                diff_dx = diff_dx * Du.unsqueeze(1)
        if nlflux is not None:
            # the residual is affine in vel: the flux term's F'(u) w . grad u rides as an extra velocity, with u from the forward
            w, fcoef, div_w = nlflux
            f = [float(x) for x in np.reshape(np.asarray(fcoef, dtype=np.float64), -1)]
            f = f + [0.0] * (3 - len(f))
            w = w if isinstance(w, t.Tensor) else np.asarray(w, dtype=np.float64)
            w = self.dev(w.reshape(-1, self.dim), dt)                # [n, dim] or [1, dim]
            u0 = self.forward_f64(X) if fp64 else self.forward(X)
            vel = vel + (f[0] + u0 * (2.0 * f[1] + 3.0 * f[2] * u0)).unsqueeze(1) * w
            if div_w is not None:
                fu = u0 * (f[0] + u0 * (f[1] + u0 * f[2]))
                fu = fu * (float(div_w) if np.ndim(div_w) == 0 and not isinstance(div_w, t.Tensor) else self.dev(
                    div_w.reshape(-1) if isinstance(div_w, t.Tensor) else np.reshape(div_w, -1), dt))
        fn = self.lib.vn_residual_f64 if fp64 else self.lib.vn_residual
        self._ck(fn(self.h, _ptr(X), _ptr(diff), _ptr(vel), _ptr(source), _ptr(diff_dx), n, _ptr(u), _ptr(r)))
        if reaction is not None:
            rate, coef = reaction
            c = [float(x) for x in np.reshape(np.asarray(coef, dtype=np.float64), -1)]
            c = c + [0.0] * (3 - len(c))
            pu = u * (c[0] + u * (c[1] + u * c[2]))
            if rate is not None:
                pu = pu * (float(rate) if np.ndim(rate) == 0 and not isinstance(rate, t.Tensor) else self.dev(
                    rate.reshape(-1) if isinstance(rate, t.Tensor) else np.reshape(rate, -1), dt))
            r = r + pu
        if fu is not None:
            r = r - fu
        if dterm is not None:
            r = r + dterm
        return u, r

    # -- towers: RCCL communicator inside the engine (TFModel.py:253-289, 342-377) ---------------
    @staticmethod
    def comm_available():
        """True if RCCL loads in this process (local probe: no collective, no GPU work)."""
        return load_library().vn_comm_available() == 0

    @staticmethod
    def comm_version():
        """ncclGetVersion of the RCCL this process loaded (e.g. 22205), or None when it cannot be loaded."""
        v = C.c_int32()
        return int(v.value) if load_library().vn_comm_version(C.byref(v)) == 0 else None

    @staticmethod
    def comm_unique_id():
        """128 opaque bytes (ncclUniqueId) made on ONE rank; ship them to every rank, then `comm_init`."""
        lib = load_library()
        buf = C.create_string_buffer(VN_COMM_ID_BYTES)
        rc = lib.vn_comm_unique_id(buf)
        if rc != 0:
            raise VNError('varnet_hip error %d: %s' % (rc, lib.vn_last_error().decode()))
        return bytes(buf.raw)

    def comm_init(self, rank, world, unique_id):
        """Join the RCCL communicator (collective over all ranks).  Afterwards `train_step` /
        `train_epoch` run gradient -> SUM all-reduce -> optimizer on the engine stream."""
        assert len(unique_id) == VN_COMM_ID_BYTES
        buf = C.create_string_buffer(bytes(unique_id), VN_COMM_ID_BYTES)
        self._ck(self.lib.vn_comm_init(self.h, int(rank), int(world), buf))

    def _gpu_identity(self, ordinal):
        """What distinguishes one physical GPU from another across ranks: (host name, device UUID + PCI address, visibility
        mask, ordinal).  A device ORDINAL is only unique within one node and one visibility mask: with per-rank
        HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES (SLURM --gpus-per-task: every rank sees its card as cuda:0) or with several
        nodes, distinct GPUs share an ordinal."""
        import socket
        p = self.torch.cuda.get_device_properties(ordinal)
        uuid = getattr(p, 'uuid', None)
        bus = [getattr(p, a, None) for a in ('pci_domain_id', 'pci_bus_id', 'pci_device_id')]
        ident = 'uuid:%s|pci:%s' % (uuid, ':'.join('%x' % b for b in bus) if all(b is not None for b in bus) else None)
        mask = '%s|%s' % (os.environ.get('HIP_VISIBLE_DEVICES', ''), os.environ.get('ROCR_VISIBLE_DEVICES', ''))
        return (socket.gethostname(), ident, mask, int(ordinal))

    def _make_current(self, ordinal):
        self.torch.cuda.set_device(ordinal)          # what vn_comm_init's hipSetDevice would fail on

    @staticmethod
    def shared_gpus(identities):
        """Pairs of ranks that name the SAME physical GPU, from (host, device identifiers, visibility mask, ordinal) tuples:
        on one host, under one visibility mask, the ordinal decides (equal ordinal = same card, different ordinal = different
        cards whatever the identifiers say: a runtime that reports a degenerate UUID must not cost the ranks their RCCL
        communicator); under different masks, or with two-field (host, identifier) tuples, equal identifiers decide; ranks on
        different hosts never share a card."""
        ids = [tuple(i) if isinstance(i, (list, tuple)) else (i,) for i in identities]
        dup = []
        for r in range(len(ids)):
            for q in range(r):
                a, b = ids[q], ids[r]
                if a[0] != b[0]:
                    continue
                if len(a) >= 4 and len(b) >= 4 and a[2] == b[2]:
                    same = a[3] == b[3]
                else:
                    same = a[1:2] == b[1:2]
                if same:
                    dup.append((q, r))
                    break
        return dup

    def comm_init_from_torch(self, dist):
        """Bootstrap through an initialised torch.distributed group.  Every rank walks through the SAME sequence of
        collectives up to `comm_init`, and everything that can fail on ONE rank alone is checked before any rank enters
        ncclCommInitRank (which has no timeout: a rank that never arrives leaves its peers inside it):
          1. every rank probes locally, no collective: RCCL loads, the engine has no communicator yet, its GPU can be made
             current; the (ok, physical GPU identity) pairs are all-gathered;
          2. all ranks skip RCCL together if any probe failed, or if two ranks name the same PHYSICAL GPU -- the same
             (host name, device UUID / PCI address), not the same ordinal: ordinals repeat across nodes and across per-rank
             visibility masks (RCCL refuses a device that appears twice in a communicator: ranks sharing a card over gloo,
             VN_COMM=try);
          3. rank 0 makes the id inside try/except and ALWAYS broadcasts an (ok, id) pair;
          4. all ranks call comm_init together -- each on a helper thread it waits for at most $VN_COMM_INIT_TIMEOUT_S (90 s) --
             then agree (MIN) that it came up everywhere; else all destroy, or, if any rank's call has not come back, all
             ABANDON the communicator (no ncclCommDestroy against a wedged peer) and keep the SUM in torch.distributed.
        What is NOT covered: a rank that DIES between 3 and 4 leaves its peers' helper threads in RCCL's bootstrap (they fall
        back after the timeout, then fail in torch's own collective); the launcher (varnet_amd/launch.py: deadline + stage
        breadcrumbs, towers.py) ends the peers of a dead rank and says where every rank last was.
        Returns (True, '') when the communicator is up on every rank, (False, reason) when all ranks skipped it.  Leaves the
        breadcrumb `comm_done` (past the launcher's bootstrap deadline, varnet_amd/launch.py) whatever the outcome."""
        from .launch import mark_stage
        try:
            return VNEngine._comm_bootstrap(self, dist)     # (unbound: tests drive this with a scripted stand-in engine)
        finally:
            mark_stage('comm_done')

    def _comm_bootstrap(self, dist):
        from .launch import mark_stage
        rank, world = dist.get_rank(), dist.get_world_size()
        t = self.torch
        dev = self.device if dist.get_backend() == 'nccl' else 'cpu'

        def all_ok(ok):
            flag = t.tensor([1 if ok else 0], dtype=t.int32, device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            return int(flag.item()) == 1

        mark_stage('probe')
        why, ident = '', None
        try:
            mine = self.comm_available()
            if not mine:
                why = self.lib.vn_last_error().decode()
            elif self.comm_size()[0] != 1:
                mine, why = False, 'this engine already has a communicator'
            else:
                ordinal = int(self.device.index)
                self._make_current(ordinal)
                ident = self._gpu_identity(ordinal)
        except Exception as e:                       # noqa: BLE001  (a probe must not raise past the collective)
            mine, why = False, str(e)
        probes = [None] * world
        dist.all_gather_object(probes, (bool(mine), ident, why))
        bad = [(r, p[2]) for r, p in enumerate(probes) if not p[0]]
        if bad:
            return False, why or 'RCCL is not usable on rank %d: %s' % bad[0]
        dup = self.shared_gpus([p[1] for p in probes])
        if dup:
            return False, ('ranks %s share a physical GPU %s: RCCL needs one device per rank'
                           % (' and '.join(str(r) for r in dup[0]), probes[dup[0][0]][1]))
        mark_stage('id_bcast')
        box = [None]
        if rank == 0:
            try:
                box = [(1, self.comm_unique_id())]
            except Exception as e:                   # noqa: BLE001
                box = [(0, str(e))]
        dist.broadcast_object_list(box, src=0)       # always, also on failure
        ok0, payload = box[0]
        if not ok0:
            return False, 'rank 0 could not create the RCCL id: %s' % payload
        mark_stage('comm_init')
        # ncclCommInitRank has no timeout of its own.  The call runs on a helper thread that this rank waits for at most
        # $VN_COMM_INIT_TIMEOUT_S (default 90 s; 0 = wait for ever on the calling thread): a rank whose call does not come
        # back reports that, ALL ranks then keep the gradient SUM in torch.distributed (whose own communicator is up already),
        # and a communicator that came up on some ranks while a peer is wedged is ABANDONED, not destroyed -- ncclCommDestroy
        # could block on the wedged peer; `close()` then leaves the handle to the process exit.
        import threading
        limit = float(os.environ.get('VN_COMM_INIT_TIMEOUT_S', '90'))
        box = {}

        def _join():
            try:
                self.comm_init(rank, world, payload)
                box['ok'] = True
            except Exception as e:                   # noqa: BLE001
                box['err'] = str(e)
        up, why, late, th = True, '', False, None
        if limit > 0:
            th = threading.Thread(target=_join, daemon=True)
            th.start()
            th.join(limit)
            if th.is_alive():
                up, late, why = False, True, 'vn_comm_init (ncclCommInitRank) did not return within %g s on rank %d' % (limit, rank)
        else:
            _join()
        if not late and 'err' in box:
            up, why = False, box['err']
        mark_stage('comm_agree')
        flags = t.tensor([1 if up else 0, 0 if late else 1], dtype=t.int32, device=dev)      # MIN: all up? nobody late?
        dist.all_reduce(flags, op=dist.ReduceOp.MIN)
        if int(flags[0].item()) == 1:
            return True, ''
        if int(flags[1].item()) == 0:
            # a peer (or this rank) is still inside the bootstrap: withdraw the communicator inside the engine, so that no
            # vn_train_* ever enqueues a collective on it -- also when this rank's helper thread returns later
            self.comm_abandon(th)
            return False, why or 'ncclCommInitRank did not return on another rank: communicator abandoned'
        if up:
            self.comm_destroy()
        return False, why or 'ncclCommInitRank failed on another rank'

    def comm_size(self):
        w, r = C.c_int32(), C.c_int32()
        self._ck(self.lib.vn_comm_size(self.h, C.byref(w), C.byref(r)))
        return w.value, r.value

    def comm_destroy(self):
        self._ck(self.lib.vn_comm_destroy(self.h))

    def comm_abandon(self, pending=None):
        """Give up on a communicator whose bootstrap did not finish on every rank (vn_comm_abandon): the engine stops
        using it and never destroys it; `close()` leaves the handle to the process exit, and the interpreter's exit
        no longer waits for a helper thread inside ncclCommInitRank (`_exit_without_waiting`)."""
        self._ck(self.lib.vn_comm_abandon(self.h))
        self._comm_abandoned = True
        _exit_without_waiting(pending)               # `pending`: the helper thread that may still sit in ncclCommInitRank

    def allreduce_grad(self):
        self._ck(self.lib.vn_allreduce_grad(self.h))

    def kernel_path(self):
        """(VN_KERNEL_* the engine resolved to, two-pass route flag)."""
        k, tp = C.c_int32(), C.c_int32()
        self._ck(self.lib.vn_kernel_path(self.h, C.byref(k), C.byref(tp)))
        return k.value, bool(tp.value)

    def dedup_supported(self):
        """The de-duplicated formulation needs a network of the 8-wave fused kernel; it has no tiles of whole test functions, so it
        also serves the two-pass route's integNum (216: three-point Gauss in 2D+t) up to the seed kernel's 256-row chunk."""
        k, tp = self.kernel_path()
        return k == VN_KERNEL_FUSED16 and (not tp or self.integNum <= 256)

    def calibrate(self):
        """Sustained fp32 MFMA rate and fp32 vector issue cost of this GPU (vn_calib.hip): dict for bench.py."""
        out = (C.c_double * 5)()
        self._ck(self.lib.vn_debug_calibrate(self.h, out))
        return {"mfma_f32_tflops": out[0], "mfma_launch_ms": out[1], "cycles_per_vector_instruction_2_waves_per_simd": out[2],
                "clock_ghz_implied_by_the_mfma_loop": out[3], "valu_launch_ms": out[4]}

    def calibrate_f64(self, ghz=0.0):
        """Sustained fp64 MFMA rate of this GPU (v_mfma_f64_16x16x4_f64 loop, vn_calib.hip): dict for bench.py."""
        out = (C.c_double * 3)()
        self._ck(self.lib.vn_debug_calibrate_f64(self.h, float(ghz), out))
        return {"mfma_f64_tflops": out[0], "launch_ms": out[1], "cycles_per_mfma_f64_16x16x4": out[2]}

    def debug_point_route(self, route):
        """Test aid: residual / fp64 entry points of this engine on the per-thread kernels (True / 1), forward / residual on the
        f32-MFMA kernels where the bf16-piece kernels would run (2: cross-check library only), or the automatic route (False / 0);
        | 4: vn_set_dedup keeps the CSR-ordered copy of gcoef although it is periodic (the general path of the assembly kernels)."""
        self._ck(self.lib.vn_debug_point_route(self.h, int(route)))

    def debug_stamps(self):
        out = (C.c_uint64 * 8)()
        self._ck(self.lib.vn_debug_stamps(self.h, out))
        return list(out)

    # -- profiling -----------------------------------------------------------------------
    def profile_begin(self):
        self._ck(self.lib.vn_profile_begin(self.h))

    def profile_comm(self):
        ms, n = C.c_double(), C.c_int64()
        self._ck(self.lib.vn_profile_comm(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_end(self):
        ms, n = C.c_double(), C.c_int64()
        name = C.create_string_buffer(128)
        self._ck(self.lib.vn_profile_end(self.h, C.byref(ms), C.byref(n), name, 128))
        return ms.value, n.value, name.value.decode()
