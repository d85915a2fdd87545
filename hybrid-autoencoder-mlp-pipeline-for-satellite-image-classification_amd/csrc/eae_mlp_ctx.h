// The MLP context behind the opaque eae_mlp handle, shared by the two units that serve it: eae_mlp.hip (the entry points and the
// fixed 128 / 64 kernel, eae_mlp_create) and eae_mlp_arch.hip (the layer-table kernel for any architecture, eae_mlp_create_ex).
#pragma once
#include "eae_mlp.hip.h"

constexpr int EAE_MLP_MAX_HIDDEN = 4, EAE_MLP_MAX_WIDTH = 512;

struct eae_mlp {
  int IN, C, Bm;
  long long off[11] = {}, bnoff[5] = {};
  float *P = nullptr, *G = nullptr, *M = nullptr, *V = nullptr, *bnrun = nullptr;
  long long* nbt = nullptr;
  long long adam_step = 0;
  void* ws = nullptr;
  float *h1 = nullptr, *a1 = nullptr, *h2 = nullptr, *a2 = nullptr, *dlog = nullptr, *g2 = nullptr, *g1 = nullptr;
  const float* class_w = nullptr;              // eae_mlp_set_class_weights: caller-owned [C] or nullptr
  long long ignore_index = EAE_NO_IGNORE;
  bool wce() const { return class_w != nullptr || ignore_index != EAE_NO_IGNORE; }
  long long* valid_acc = nullptr;              // eae_mlp_set_valid_counter: += counted rows of every step that accumulates stats
  // eae_mlp_create_ex (general = 1): the layer table of the kernel in eae_mlp_arch.hip; off / bnoff / h1 .. g1 above stay zero
  int general = 0;
  int nh = 0, hw[EAE_MLP_MAX_HIDDEN] = {0, 0, 0, 0};
  float pdrop[EAE_MLP_MAX_HIDDEN] = {0.f, 0.f, 0.f, 0.f};
  long long poff_ex[4 * EAE_MLP_MAX_HIDDEN + 3], bnoff_ex[2 * EAE_MLP_MAX_HIDDEN + 1];
  float *hx[EAE_MLP_MAX_HIDDEN], *ax[EAE_MLP_MAX_HIDDEN], *gx[EAE_MLP_MAX_HIDDEN];   // workspace [max_batch][w_l] per layer
  int ncu = 256;                               // compute units of the device the parameter arena lives on (eae_mlp_arch_bound): eval mode
                                               // spreads the rows over them
};

// eae_mlp_arch.hip: launches the layer-table kernel for a general context from the argument block eae_mlp.hip filled (x, labels, B,
// the arenas, the mode flags, Adam's scalars, seed / step, drop_mask, dlog_in, logits, stats and the predict epilogue; its off, h1 .. g1
// and p_drop are not read).  weighted: class_w / ignore_index / valid apply (labels set, no external dlogits).
int eae_mlp_arch_launch(eae_mlp* m, hipStream_t st, const MlpArgs& a, int weighted, const float* class_w, long long ignore_index,
                        long long* valid);
// eae_mlp_bind of a general context: takes the compute-unit count from the device that holds the parameter arena
void eae_mlp_arch_bound(eae_mlp* m);
