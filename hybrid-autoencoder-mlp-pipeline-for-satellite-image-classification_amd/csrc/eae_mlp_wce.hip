// The external MLP's step kernel with class-weighted CrossEntropyLoss and ignored labels (eae_mlp_set_class_weights):
// eae_mlp_kernel.hip.h with MLP_WCE 1, in a translation unit of its own (the helpers' inlining in eae_mlp.hip stays what it was).
#include "eae_mlp.hip.h"

namespace {
#define MLP_WCE 1
#include "eae_mlp_kernel.hip.h"
#undef MLP_WCE
}  // namespace

// a: the argument block eae_mlp.hip filled (labels set, no external dlogits)
void eae_mlp_launch_wce(hipStream_t st, int grid, const MlpArgs& a, const float* class_w, long long ignore_index, long long* valid) {
  const MlpArgsW w = {a, class_w, ignore_index, valid};
  hipLaunchKernelGGL(mlp_kernel_wce, dim3(grid), dim3(T), 0, st, w);
}
