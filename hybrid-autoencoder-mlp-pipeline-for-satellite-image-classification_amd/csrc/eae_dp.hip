// ---------------------------------------------------------------------------------------------------------------------
// Data parallel over RCCL, driven by the engine (eae_dp_init / eae_dp_allreduce_bucket; 8e).  librccl is bound at
// run time with dlopen -- the copy torch has already loaded if there is one, so the process holds ONE RCCL --, libeae.so itself
// keeps no link-time dependency on it.  One communicator per context, one process per GPU.
//   eae_dp_unique_id   rank 0 draws the 128-byte id (the caller ships it to the other ranks by whatever means it has)
//   eae_dp_init        every rank: ncclCommInitRank on the context's device
//   eae_dp_allreduce_bucket   sum over the ranks of gradient-arena elements [off, off + count), in place, on `stream`
//   eae_ae_dp_train_step      forward + loss + backward + all-reduce + Adam(grad_scale = 1/world) enqueued by ONE call.  overlap=1:
//                      the decoder-side bucket (gradient tensors 18..37, 3.3 MB at latent 64) is all-reduced on the engine's
//                      hand-off stream as soon as those tensors are complete, while the encoder half of the backward still runs;
//                      the encoder-side bucket follows on the caller's stream after the join.  overlap=0: one all-reduce of the
//                      whole arena after the backward.
// ---------------------------------------------------------------------------------------------------------------------
#include "eae_ctx.h"
#include "eae_common.hip.h"      // EAE_NO_PK
#include <chrono>
#include <cstring>
#include <cstdlib>
#include <future>
#include <memory>
#include <string>
#include <thread>
#include <dlfcn.h>
#include <rccl/rccl.h>          // types and prototypes only; every symbol is resolved with dlsym
namespace {
struct RcclApi {
  void* h = nullptr;
  decltype(&ncclGetUniqueId) getUniqueId = nullptr;
  decltype(&ncclCommInitRank) commInitRank = nullptr;
  decltype(&ncclCommDestroy) commDestroy = nullptr;
  decltype(&ncclAllReduce) allReduce = nullptr;
  decltype(&ncclBroadcast) broadcast = nullptr;
  decltype(&ncclGetErrorString) getErrorString = nullptr;
  // optional (older libraries lack them): grouped launches
  decltype(&ncclGroupStart) groupStart = nullptr;
  decltype(&ncclGroupEnd) groupEnd = nullptr;
  std::string err;
};
RcclApi* rccl_api() {
  static RcclApi api = [] {
    RcclApi a;
    const char* names[] = {"librccl.so.1", "librccl.so"};
    for (const char* n : names) if (!a.h) a.h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);      // the copy already in the process (torch's)
    for (const char* n : names) if (!a.h) a.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (!a.h) a.h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!a.h) { a.err = std::string("librccl not found: ") + (dlerror() ? dlerror() : "?"); return a; }
    a.getUniqueId = reinterpret_cast<decltype(a.getUniqueId)>(dlsym(a.h, "ncclGetUniqueId"));
    a.commInitRank = reinterpret_cast<decltype(a.commInitRank)>(dlsym(a.h, "ncclCommInitRank"));
    a.commDestroy = reinterpret_cast<decltype(a.commDestroy)>(dlsym(a.h, "ncclCommDestroy"));
    a.allReduce = reinterpret_cast<decltype(a.allReduce)>(dlsym(a.h, "ncclAllReduce"));
    a.broadcast = reinterpret_cast<decltype(a.broadcast)>(dlsym(a.h, "ncclBroadcast"));
    a.getErrorString = reinterpret_cast<decltype(a.getErrorString)>(dlsym(a.h, "ncclGetErrorString"));
    if (!a.getUniqueId || !a.commInitRank || !a.commDestroy || !a.allReduce || !a.broadcast || !a.getErrorString) a.err = "librccl lacks a required symbol";
    a.groupStart = reinterpret_cast<decltype(a.groupStart)>(dlsym(a.h, "ncclGroupStart"));
    a.groupEnd = reinterpret_cast<decltype(a.groupEnd)>(dlsym(a.h, "ncclGroupEnd"));
    return a;
  }();
  return &api;
}
int rccl_fail(RcclApi* r, ncclResult_t e, const char* what) {
  std::string m = std::string(what) + ": " + (r->getErrorString ? r->getErrorString(e) : "rccl error");
  return eae_set_error(EAE_ERR_HIP, m.c_str());
}
#define RCCL(x, what) do { ncclResult_t e__ = (x); if (e__ != ncclSuccess) return rccl_fail(r, e__, what); } while (0)
}  // namespace

extern "C" int eae_dp_unique_id(void* id128) {
  if (!id128) return eae_set_error(EAE_ERR_ARG, "dp_unique_id: NULL");
  RcclApi* r = rccl_api();
  if (!r->err.empty()) return eae_set_error(EAE_ERR_STATE, r->err.c_str());
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  ncclUniqueId id;
  RCCL(r->getUniqueId(&id), "ncclGetUniqueId");
  memcpy(id128, &id, 128);
  return 0;
}
extern "C" int eae_dp_init(eae_ctx* c, int rank, int world, const void* id128) {
  if (!c || !id128 || world < 1 || rank < 0 || rank >= world) return eae_set_error(EAE_ERR_ARG, "dp_init: bad argument");
  if (c->dp_comm) return eae_set_error(EAE_ERR_STATE, "dp_init: this context already owns a communicator");
  RcclApi* r = rccl_api();
  if (!r->err.empty()) return eae_set_error(EAE_ERR_STATE, r->err.c_str());
  ncclUniqueId id;
  memcpy(&id, id128, 128);
  ncclComm_t comm = nullptr;
  // Time-bounded bring-up (EAE_DP_INIT_TIMEOUT_S, default 120; 0 = plain blocking call): ncclCommInitRank is a rendezvous of all ranks
  // and blocks for ever when a peer never arrives.  It runs on a helper thread and the caller waits for it with a deadline; on a
  // time-out the call returns an error (dp.py: every rank falls back together) and the helper is left behind, still blocked.
  // (Not ncclCommInitRankConfig(blocking = 0): that makes EVERY later call on the communicator non-blocking -- an all-reduce may then
  //  return ncclInProgress and has to be polled -- which the enqueue-only train step does not want.)
  static const double limit_s = getenv("EAE_DP_INIT_TIMEOUT_S") ? atof(getenv("EAE_DP_INIT_TIMEOUT_S")) : 120.0;
  if (limit_s > 0) {
    int dev = 0;
    EAE_HIP(hipGetDevice(&dev));
    struct Box { std::promise<ncclResult_t> done; ncclComm_t comm = nullptr; };
    auto box = std::make_shared<Box>();
    std::future<ncclResult_t> fut = box->done.get_future();
    auto fn = r->commInitRank;
    std::thread([box, fn, world, id, rank, dev]() {
      ncclResult_t e = ncclSystemError;
      if (hipSetDevice(dev) == hipSuccess) e = fn(&box->comm, world, id, rank);
      box->done.set_value(e);
    }).detach();
    if (fut.wait_for(std::chrono::duration<double>(limit_s)) != std::future_status::ready)
      return eae_set_error(EAE_ERR_STATE, "dp_init: the communicator did not come up within EAE_DP_INIT_TIMEOUT_S (a peer never joined?)");
    const ncclResult_t e = fut.get();
    if (e != ncclSuccess) return rccl_fail(r, e, "ncclCommInitRank");
    comm = box->comm;
  } else {
    RCCL(r->commInitRank(&comm, world, id, rank), "ncclCommInitRank");
  }
  c->dp_comm = comm; c->dp_rank = rank; c->dp_world = world;
  if (!c->ev_dp_done) EAE_HIP(hipEventCreateWithFlags(&c->ev_dp_done, EV_FLAGS));
  return 0;
}
extern "C" int eae_dp_world(eae_ctx* c) { return c ? c->dp_world : 0; }
extern "C" int eae_dp_destroy(eae_ctx* c) {
  if (!c || !c->dp_comm) return 0;
  RcclApi* r = rccl_api();
  hipDeviceSynchronize();
  if (r->commDestroy) r->commDestroy(static_cast<ncclComm_t>(c->dp_comm));
  c->dp_comm = nullptr; c->dp_world = 0;
  if (c->ev_dp_done) { hipEventDestroy(c->ev_dp_done); c->ev_dp_done = nullptr; }
  return 0;
}
extern "C" int eae_dp_allreduce_bucket(eae_ctx* c, void* stream, long long elem_off, long long count) {
  if (!c || !c->dp_comm) return eae_set_error(EAE_ERR_STATE, "dp_allreduce_bucket: eae_dp_init has not been called");
  if (!c->G || elem_off < 0 || count <= 0 || elem_off + count > c->arena_len()) return eae_set_error(EAE_ERR_ARG, "dp_allreduce_bucket: range outside the gradient arena");
  RcclApi* r = rccl_api();
  RCCL(r->allReduce(c->G + elem_off, c->G + elem_off, (size_t)count, ncclFloat, ncclSum, static_cast<ncclComm_t>(c->dp_comm), (hipStream_t)stream),
       "ncclAllReduce");
  return 0;
}
// identical replicas: `bytes` of any device buffer from rank `root` (parameters, running statistics, Adam moments at start-up)
extern "C" int eae_dp_broadcast(eae_ctx* c, void* stream, void* buf, long long bytes, int root) {
  if (!c || !c->dp_comm) return eae_set_error(EAE_ERR_STATE, "dp_broadcast: eae_dp_init has not been called");
  if (!buf || bytes <= 0 || root < 0 || root >= c->dp_world) return eae_set_error(EAE_ERR_ARG, "dp_broadcast: bad argument");
  RcclApi* r = rccl_api();
  RCCL(r->broadcast(buf, buf, (size_t)bytes, ncclChar, root, static_cast<ncclComm_t>(c->dp_comm), (hipStream_t)stream), "ncclBroadcast");
  c->packed = false;
  return 0;
}
// The "optimizer refuses to update" switches (a gate that timed out: sticky; a non-finite BatchNorm statistic: this step) are local to a
// rank, but a synchronous data-parallel step must take the decision for ALL ranks or the replicas diverge silently: every
// rank publishes (timeout | poison) != 0 into one device word, the word is max-reduced over the ranks next to the last gradient bucket
// (one grouped launch where the library has ncclGroupStart), and the optimizer kernel reads the REDUCED word.
static __global__ EAE_NO_PK void dp_flag_kernel(const unsigned* a, const unsigned* b, unsigned* out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {      // out[0]: stale (gate time-out), out[1]: diverged (non-finite statistics) -- kept apart:
    out[0] = (a != nullptr && __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) ? 1u : 0u;      // the optimizer
    out[1] = (b != nullptr && __hip_atomic_load(b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) ? 1u : 0u;      // treats them differently
  }
}
// sigwords[12..13]: this rank's two flags, then the reduced ones (same words, all-reduced in place)
static unsigned* dp_flag_word(eae_ctx* c) { return c->sigwords + 12; }
extern "C" int eae_dp_local_bad(eae_ctx* c, void* stream, unsigned* out_dev) {
  if (!c || !out_dev) return eae_set_error(EAE_ERR_ARG, "dp_local_bad: NULL argument");
  hipLaunchKernelGGL(dp_flag_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, c->sigwords + 8, poison_word(c), out_dev);
  EAE_LAUNCH_CHECK();
  return 0;
}
// optimizer.step() of a data-parallel replica whose peers' flags were reduced by the caller (torch.distributed path): `peer_bad` is a
// pair of device words (stale, diverged), non-zero = some rank must not update -> no rank updates
extern "C" int eae_adam_step_dp(eae_ctx* c, void* stream, float lr, float weight_decay, float grad_scale, const unsigned* peer_bad) {
  return optimizer_step(c, (hipStream_t)stream, lr, weight_decay, grad_scale, peer_bad, peer_bad ? peer_bad + 1 : nullptr);
}

extern "C" int eae_ae_dp_train_step(eae_ctx* c, void* stream, const eae_step_io* io, float lr, int overlap) {
  RC(check_io(c, io, true));
  if (!c->dp_comm) return eae_set_error(EAE_ERR_STATE, "dp_train_step: eae_dp_init has not been called");
  if (!c->M || !c->V) return eae_set_error(EAE_ERR_STATE, "adam: moment arenas must be bound");
  hipStream_t st = (hipStream_t)stream;
  const bool ov = overlap != 0 && c->use_side;
  RC(streams_distinct(c, st));
  if (ov && !eae_dp_stream(c, 0)) return eae_set_error(EAE_ERR_HIP, "dp_train_step: cannot create the hand-off stream");
  RC(forward_impl(c, st, io, true));
  RC(backward_impl(c, st, io));             // with a hand-off stream: dp_stream[0] is now ordered after gradient tensors 18..37
  c->adam_step += 1;                        // (behind the launches that can fail: a failed step must not advance the bias correction)
  const long long cut = c->poff[CUT_ENC_DEC], total = c->arena_len();
  RcclApi* r = rccl_api();
  unsigned* flag = dp_flag_word(c);
  hipLaunchKernelGGL(dp_flag_kernel, dim3(1), dim3(64), 0, st, c->sigwords + 8, poison_word(c), flag);
  EAE_LAUNCH_CHECK();
  const bool grp = r->groupStart && r->groupEnd;
  if (ov) {
    RC(eae_dp_allreduce_bucket(c, c->dp_stream[0], cut, total - cut));
    EAE_HIP(hipEventRecord(c->ev_dp_done, c->dp_stream[0]));
  }
  if (grp) RCCL(r->groupStart(), "ncclGroupStart");
  {
    int rc = eae_dp_allreduce_bucket(c, st, 0, ov ? cut : total);
    if (!rc) {
      ncclResult_t e = r->allReduce(flag, flag, 2, ncclUint32, ncclMax, static_cast<ncclComm_t>(c->dp_comm), st);
      if (e != ncclSuccess) rc = rccl_fail(r, e, "ncclAllReduce (flag)");
    }
    if (grp) { ncclResult_t e = r->groupEnd(); if (!rc && e != ncclSuccess) rc = rccl_fail(r, e, "ncclGroupEnd"); }
    RC(rc);
  }
  if (ov) EAE_HIP(hipStreamWaitEvent(st, c->ev_dp_done, 0));
  RC(launch_adam(c, st, c->arena_len(), lr, 0.f, 1.0f / (float)c->dp_world, flag, flag + 1));
  after_optimizer(c, 0);
  return 0;
}
