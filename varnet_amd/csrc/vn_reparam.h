// Host-side declarations of vn_reparam.hip: learnt weight scales theta_eff = f(s) (.) V between the gradient reduction and the
// parameters (maths and order contract: that file's header).  Kept out of vn_internal.h, which every kernel's source hash covers.
#pragma once
#include <hip/hip_runtime.h>

#define VN_RP_MAX_LAYERS 9                   // 8 hidden layers + the output layer: the range of the fused / generic kernels
#define VN_RP_MAX_WIDTH 64

// One record serves the step, its dry form, the factorisation and the rebuild.  Layer slot k = 0 .. nl-1 is layer l = k + 1 of
// VnNet: W_l row-major [fi, fo] at woff, b_l [fo] at boff.
struct VnReparamArgs {
  int mode = 0;                              // VN_REPARAM_RWF: f(s) = exp(s), weights only | VN_REPARAM_SLOPE: f(s) = n s, weights and bias
  int tied = 0;                              // 1: one scale per layer (slope, granularity `layer`), 0: one per output neuron
  double n = 1.0;                            // the slope mode's fixed factor
  int nl = 0, P = 0, S = 0;
  int fi[VN_RP_MAX_LAYERS], fo[VN_RP_MAX_LAYERS], woff[VN_RP_MAX_LAYERS], boff[VN_RP_MAX_LAYERS];
  int soff[VN_RP_MAX_LAYERS];                // offset of the layer's scales in s, or -1: the layer is in no group
  float* theta = nullptr;                    // [P] theta_eff, what every compute kernel reads           (written by the step)
  float* V = nullptr;                        // [P] the raw parameters
  float *m = nullptr, *v = nullptr;          // [P] Adam slots of V (the engine's own)
  float *s = nullptr, *ms = nullptr, *vs = nullptr;   // [S] scales and their Adam slots
  float* f = nullptr;                        // [S] fl32(f(s)) as last formed
  const float* g = nullptr;                  // [P + 4] gradient buffer: d loss / d theta_eff | loss, BC, IC, var
  float lr_t = 0.f, lr_s_t = 0.f, b1 = 0.f, b2 = 0.f, eps = 0.f;   // bias-corrected rates of V and of s, and Adam's constants
  float* loss_acc = nullptr;                 // += g[P] (device scalar) or nullptr
  float *gV = nullptr, *gs = nullptr;        // dry form only: [P] and [S] outputs
};

// One joint Adam step on (V, s), then theta_eff = fl32(f(s_new)) * V_new: one launch of nl workgroups.
hipError_t vn_reparam_step_launch(const VnReparamArgs& a, hipStream_t s);
// The same sums without the step: g_V into a.gV, g_s into a.gs; no state is touched.
hipError_t vn_reparam_grad_launch(const VnReparamArgs& a, hipStream_t s);
// f = fl32(f(s));  V = theta / f on grouped entries, V = theta elsewhere.
hipError_t vn_reparam_factorise_launch(const VnReparamArgs& a, const int* group, hipStream_t s);
// f = fl32(f(s));  theta = f * V on grouped entries, theta = V elsewhere.
hipError_t vn_reparam_rebuild_launch(const VnReparamArgs& a, const int* group, hipStream_t s);
