// External latent-space classifier of the reference (R.md:2549-2566):
//   Linear(in,128) -> BatchNorm1d(128) -> ReLU -> Dropout(0.3) -> Linear(128,64) -> BatchNorm1d(64) -> ReLU -> Linear(64,C)
// and its training / evaluation steps (R.md:2639-2668).  17 K MAC per sample: everything is launch latency, so one
// training iteration (zero_grad, forward, CrossEntropy, backward, Adam with L2 weight decay, accuracy bookkeeping) is ONE
// kernel launch executed by a single 1024-thread workgroup (BatchNorm1d needs whole-batch statistics anyway); weights
// stay L1/L2-resident, activations live in a small global workspace, arithmetic is fp32 (matches the reference's dtype).
// Evaluation (running statistics, rows independent) uses one block per 64 rows.
// This unit holds every eae_mlp_* entry point and the fixed 128 / 64 kernel.  A context made by eae_mlp_create_ex (any architecture,
// eae_mlp_ctx.h: general = 1) passes the same checks here and is then handed to the layer-table kernel of eae_mlp_arch.hip.
#include "eae_internal.h"
#include "eae_common.hip.h"
#include <cmath>

#include "eae_mlp.hip.h"
#include "eae_mlp_ctx.h"

namespace {
#define MLP_WCE 0
#include "eae_mlp_kernel.hip.h"
#undef MLP_WCE
}  // namespace

static long long r4(long long n) { return (n + 3) & ~3LL; }

extern "C" int eae_mlp_layout(int input_dim, int num_classes, long long* param_off, long long* bn_off) {
  if (input_dim <= 0 || input_dim > 1024 || num_classes <= 0 || num_classes > 16) return eae_set_error(EAE_ERR_ARG, "mlp: input_dim in 1..1024, classes in 1..16");
  const long long sz[10] = {128LL * input_dim, 128, 128, 128, 64 * 128, 64, 64, 64, 64LL * num_classes, num_classes};
  long long o = 0;
  for (int i = 0; i < 10; ++i) { if (param_off) param_off[i] = o; o += r4(sz[i]); }
  if (param_off) param_off[10] = o;
  if (bn_off) { bn_off[0] = 0; bn_off[1] = 128; bn_off[2] = 256; bn_off[3] = 320; bn_off[4] = 384; }
  return 0;
}

extern "C" int eae_mlp_create(int input_dim, int num_classes, int max_batch, eae_mlp** out) {
  if (!out || max_batch <= 0) return eae_set_error(EAE_ERR_ARG, "mlp_create: bad argument");
  eae_mlp* m = new eae_mlp();
  if (int rc = eae_mlp_layout(input_dim, num_classes, m->off, m->bnoff)) { delete m; return rc; }
  m->IN = input_dim; m->C = num_classes; m->Bm = max_batch;
  size_t n = (size_t)max_batch * (128 * 3 + 64 * 3 + 16) * 4;
  hipError_t e = hipMalloc(&m->ws, n);
  if (e != hipSuccess) { delete m; return eae_set_error(EAE_ERR_HIP, hipGetErrorString(e)); }
  float* p = (float*)m->ws;
  m->h1 = p; p += (size_t)max_batch * 128; m->a1 = p; p += (size_t)max_batch * 128; m->g1 = p; p += (size_t)max_batch * 128;
  m->h2 = p; p += (size_t)max_batch * 64; m->a2 = p; p += (size_t)max_batch * 64; m->g2 = p; p += (size_t)max_batch * 64;
  m->dlog = p;
  *out = m;
  return 0;
}

extern "C" int eae_mlp_destroy(eae_mlp* m) {
  if (!m) return 0;
  hipDeviceSynchronize();
  if (m->ws) hipFree(m->ws);
  delete m;
  return 0;
}

extern "C" int eae_mlp_bind(eae_mlp* m, float* params, float* grads, float* adam_m, float* adam_v, float* bn_running, long long* bn_nbt) {
  if (!m || !params || !bn_running) return eae_set_error(EAE_ERR_ARG, "mlp_bind: ctx, params and bn_running are required");
  m->P = params; m->G = grads; m->M = adam_m; m->V = adam_v; m->bnrun = bn_running; m->nbt = bn_nbt;
  if (m->general) eae_mlp_arch_bound(m);
  return 0;
}
extern "C" int eae_mlp_set_adam_step(eae_mlp* m, long long s) { if (!m) return eae_set_error(EAE_ERR_ARG, "mlp is NULL"); m->adam_step = s; return 0; }

static int mlp_launch(eae_mlp* m, hipStream_t st, const float* x, const long long* labels, int B, int train, int backward, int adam,
                      float lr, float wd, unsigned long long seed, const float* drop_mask, float* logits, float* stats,
                      const float* dlog_in = nullptr) {
  if (!m || !x) return eae_set_error(EAE_ERR_ARG, "mlp: NULL argument");
  if (!m->P) return eae_set_error(EAE_ERR_STATE, "eae_mlp_bind has not been called");
  if (B <= 0 || B > m->Bm) return eae_set_error(EAE_ERR_ARG, "mlp: batch size outside 1..max_batch");
  if (train && B < 2) return eae_set_error(EAE_ERR_ARG, "mlp: BatchNorm1d in training mode needs more than 1 sample per batch");
  if (backward && (!m->G || (!labels && !dlog_in))) return eae_set_error(EAE_ERR_STATE, "mlp: gradient arena and labels (or dlogits) required");
  if (adam && (!m->M || !m->V)) return eae_set_error(EAE_ERR_STATE, "mlp: Adam moment arenas required");
  MlpArgs a;
  a.x = x; a.labels = labels; a.B = B; a.IN = m->IN; a.C = m->C;
  a.P = m->P; a.G = m->G; a.M = m->M; a.V = m->V;
  for (int i = 0; i < 11; ++i) a.off[i] = m->off[i];
  a.bnrun = m->bnrun; a.nbt = train ? m->nbt : nullptr;
  a.h1 = m->h1; a.a1 = m->a1; a.h2 = m->h2; a.a2 = m->a2; a.dlog = m->dlog; a.g2 = m->g2; a.g1 = m->g1;
  a.train = train; a.backward = backward; a.adam = adam;
  a.b1 = 0.9f; a.b2 = 0.999f; a.omb1 = (float)(1.0 - 0.9); a.omb2 = (float)(1.0 - 0.999); a.eps = 1e-8f; a.wd = wd; a.step_size = 0.f; a.bc2_sqrt = 1.f;
  if (adam) {
    m->adam_step += 1;
    double bc1 = 1.0 - std::pow(0.9, (double)m->adam_step), bc2 = 1.0 - std::pow(0.999, (double)m->adam_step);
    a.step_size = (float)(lr / bc1); a.bc2_sqrt = (float)std::sqrt(bc2);
  }
  a.seed = seed; a.step = (unsigned long long)m->adam_step; a.drop_mask = drop_mask; a.p_drop = 0.3f;
  a.logits = logits; a.stats = stats; a.dlog_in = dlog_in; a.update_running = dlog_in ? 0 : 1;
  a.ldx = m->IN; a.probs = nullptr; a.plabels = nullptr; a.win0 = 0; a.plane = 0; a.index = nullptr;
  const int grid = train ? 1 : (B + 63) / 64;
  if (m->general) {
    const int weighted = m->wce() && labels && !dlog_in;
    return eae_mlp_arch_launch(m, st, a, weighted, m->class_w, m->ignore_index, stats ? m->valid_acc : nullptr);
  }
  if (m->wce() && labels && !dlog_in) {
    eae_mlp_launch_wce(st, grid, a, m->class_w, m->ignore_index, stats ? m->valid_acc : nullptr);
  } else {
    hipLaunchKernelGGL(mlp_kernel, dim3(grid), dim3(T), 0, st, a);
  }
  EAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int eae_mlp_set_class_weights(eae_mlp* m, const float* weights, long long ignore_index) {
  if (!m) return eae_set_error(EAE_ERR_ARG, "mlp is NULL");
  m->class_w = weights; m->ignore_index = ignore_index;
  return 0;
}

extern "C" int eae_mlp_set_valid_counter(eae_mlp* m, long long* counter) {
  if (!m) return eae_set_error(EAE_ERR_ARG, "mlp is NULL");
  m->valid_acc = counter;
  return 0;
}

extern "C" int eae_mlp_forward(eae_mlp* m, void* stream, const float* x, int B, int train, unsigned long long seed,
                               const float* drop_mask, float* logits) {
  return mlp_launch(m, (hipStream_t)stream, x, nullptr, B, train, 0, 0, 0.f, 0.f, seed, drop_mask, logits, nullptr);
}
extern "C" int eae_mlp_train_step(eae_mlp* m, void* stream, const float* x, const long long* labels, int B, float lr, float weight_decay,
                                  unsigned long long seed, const float* drop_mask, float* logits, float* stats) {
  return mlp_launch(m, (hipStream_t)stream, x, labels, B, 1, 1, 1, lr, weight_decay, seed, drop_mask, logits, stats);
}
extern "C" int eae_mlp_eval_step(eae_mlp* m, void* stream, const float* x, const long long* labels, int B, float* logits, float* stats) {
  return mlp_launch(m, (hipStream_t)stream, x, labels, B, 0, 0, 0, 0.f, 0.f, 0, nullptr, logits, stats);
}

// loss.backward() for a torch-side loss on the logits (R.md:2644-2645): recomputes the train-mode forward of the SAME batch
// (same dropout mask: the Philox key is (seed, optimisation step); running statistics are not touched again) and
// back-propagates the supplied dL/dlogits; gradients land in the gradient arena.
extern "C" int eae_mlp_backward(eae_mlp* m, void* stream, const float* x, int B, unsigned long long seed, const float* drop_mask,
                                const float* dlogits) {
  if (!dlogits) return eae_set_error(EAE_ERR_ARG, "mlp_backward: dlogits is NULL");
  return mlp_launch(m, (hipStream_t)stream, x, nullptr, B, 1, 1, 0, 0.f, 0.f, seed, drop_mask, nullptr, nullptr, dlogits);
}

int eae_mlp_dims(const eae_mlp* m, int* input_dim, int* classes, int* max_batch) {
  if (!m) return eae_set_error(EAE_ERR_ARG, "mlp is NULL");
  *input_dim = m->IN; *classes = m->C; *max_batch = m->Bm;
  return 0;
}

// Eval-mode pass over B rows of a strided latent (the AE engine's workspace rows, stride Lp): the logits are those of
// eae_mlp_eval_step; the epilogue writes softmax and argmax at windows win0.. of the scene grid, or with an index at windows
// index[win0 ..] (win0 then counts rows of the index).  B is split at max_batch.
int eae_mlp_predict(eae_mlp* m, hipStream_t st, const float* x, int ldx, int B, long long win0, long long plane, float* probs,
                    long long* labels, const long long* index) {
  if (!m || !x || !probs || !labels) return eae_set_error(EAE_ERR_ARG, "mlp_predict: NULL argument");
  if (!m->P) return eae_set_error(EAE_ERR_STATE, "eae_mlp_bind has not been called");
  if (ldx < m->IN || B <= 0 || win0 < 0 || (!index && win0 + B > plane)) return eae_set_error(EAE_ERR_ARG, "mlp_predict: bad shape");
  for (int b0 = 0; b0 < B; b0 += m->Bm) {
    const int nb = B - b0 < m->Bm ? B - b0 : m->Bm;
    MlpArgs a;
    a.x = x + (size_t)b0 * ldx; a.labels = nullptr; a.B = nb; a.IN = m->IN; a.C = m->C;
    a.P = m->P; a.G = nullptr; a.M = nullptr; a.V = nullptr;
    for (int i = 0; i < 11; ++i) a.off[i] = m->off[i];
    a.bnrun = m->bnrun; a.nbt = nullptr;
    a.h1 = m->h1; a.a1 = m->a1; a.h2 = m->h2; a.a2 = m->a2; a.dlog = m->dlog; a.g2 = m->g2; a.g1 = m->g1;
    a.train = 0; a.backward = 0; a.adam = 0;
    a.b1 = 0.9f; a.b2 = 0.999f; a.omb1 = 0.1f; a.omb2 = 0.001f; a.eps = 1e-8f; a.wd = 0.f; a.step_size = 0.f; a.bc2_sqrt = 1.f;
    a.seed = 0; a.step = 0; a.drop_mask = nullptr; a.p_drop = 0.3f;
    a.logits = nullptr; a.stats = nullptr; a.dlog_in = nullptr; a.update_running = 0;
    a.ldx = ldx; a.probs = probs; a.plabels = labels; a.win0 = win0 + b0; a.plane = plane; a.index = index;
    if (m->general) {
      if (int rc = eae_mlp_arch_launch(m, st, a, 0, nullptr, EAE_NO_IGNORE, nullptr)) return rc;
      continue;
    }
    hipLaunchKernelGGL(mlp_kernel, dim3((nb + 63) / 64), dim3(T), 0, st, a);
    EAE_LAUNCH_CHECK();
  }
  return 0;
}
