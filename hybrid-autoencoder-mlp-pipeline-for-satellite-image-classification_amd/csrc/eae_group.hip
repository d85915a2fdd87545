// Grouped step (eae_group.h): the recorder's thread-local state and the driver that zips the members' recordings.
#include "eae_ctx.h"
#include <chrono>
#include <cstdlib>

thread_local GroupRec* eae_rec = nullptr;        // eae_group.h
thread_local int eae_geo_mult = 1;
int eae_rec_fail(const char* what) {
  if (eae_rec && !eae_rec->error) eae_rec->error = EAE_ERR_STATE;
  return eae_set_error(EAE_ERR_STATE, what);
}

// ---------------------------------------------------------------------------------------------------------------------
// Grouped train step (eae_group.h): K contexts of one shape -- the grid of (alpha, lr) configurations the reference trains one
// after the other at batch 64 (R.md:599-711) -- stepped by ONE sequence of launches.  Every member's step logic runs with the recorder
// installed (its own state advances exactly as in eae_ae_train_step's eager path), the K recordings are zipped and enqueued on the
// FIRST member's streams.  The members must agree in everything that shapes the launches (configuration, batch size, which
// outputs are requested); what they need not share: parameters, statistics, inputs, labels, alpha, lr.
// ---------------------------------------------------------------------------------------------------------------------
namespace {
int group_slot_of(void* ctx, hipStream_t user, hipStream_t st) {
  eae_ctx* c = static_cast<eae_ctx*>(ctx);
  if (st == user) return 0;
  if (st == c->side) return 1;
  for (int i = 0; i < c->nx; ++i) if (st == c->sidex[i]) return 2 + i;
  return -1;
}
hipStream_t group_stream(eae_ctx* c, hipStream_t user, int slot) { return slot == 0 ? user : slot == 1 ? c->side : c->sidex[slot - 2]; }

}  // namespace

extern "C" int eae_set_geometry_mult(int mult) {
  if (mult < 1 || mult > 64) return eae_set_error(EAE_ERR_ARG, "geometry_mult: 1..64");
  eae_geo_mult = mult;
  return 0;
}

namespace {
// what = 0: eae_ae_train_step's eager path (lrs required); 1: eae_ae_forward
int group_run(int what, eae_ctx* const* ctxs, int n, int mult, void* stream, const eae_step_io* ios, const float* lrs) {
  if (!ctxs || !ios || (what == 0 && !lrs) || n < 1 || n > 64) return eae_set_error(EAE_ERR_ARG, "group call: 1..64 contexts, one io block (and one lr) each");
  if (mult == 0) mult = n;
  if (mult < n || mult > 64) return eae_set_error(EAE_ERR_ARG, "group call: geometry_mult must be 0 (= n) or n..64");
  if (eae_rec) return eae_set_error(EAE_ERR_STATE, "group call: already recording on this thread");
  hipStream_t user = (hipStream_t)stream;
  eae_ctx* c0 = ctxs[0];
  for (int k = 0; k < n; ++k) {
    eae_ctx* c = ctxs[k];
    RC(check_io(c, &ios[k], what == 0));
    if (what == 0 && (!c->M || !c->V)) return eae_set_error(EAE_ERR_STATE, "adam: moment arenas must be bound");
    if (c->prof_on || c->fp8 || c->dp_comm || c->use_gates != c0->use_gates || c->use_side != c0->use_side || c->nx != c0->nx)
      return eae_set_error(EAE_ERR_STATE, "group call: members must share the stream layout, with profiling, fp8 and data parallel off");
    if (c->Cin != c0->Cin) return eae_set_error(EAE_ERR_ARG, "group call: members must share in_channels");
    if (c->wce() != c0->wce())       // one head kernel serves the whole group (each member with its own vector and ignore_index)
      return eae_set_error(EAE_ERR_ARG, "group call: class weights / ignore_index must be set on every member or on none");
    if (what == 0 && c->clip_on() != c0->clip_on())      // one optimizer kernel serves the whole group (each member with its own max_norm and norm_out)
      return eae_set_error(EAE_ERR_ARG, "group call: gradient clipping must be on in every member or in none (+inf measures without clipping)");
    for (int j = 0; j < k; ++j) if (ctxs[j] == c) return eae_set_error(EAE_ERR_ARG, "group call: a context appears twice");
  }
  RC(streams_distinct(c0, user));
  static thread_local std::vector<GroupRec> recs;
  if ((int)recs.size() < n) recs.resize(n);
  static const bool timing = getenv("EAE_GROUP_TIMING") != nullptr;      // diagnostic: host microseconds of the phases, every 100th call
  static thread_local double t_acc[3] = {0, 0, 0};
  static thread_local int t_n = 0;
  const auto tp0 = std::chrono::steady_clock::now();
  // (recording a member costs ~3 us of host time -- the step logic without its launches; a thread pool that recorded the members side
  //  by side was measured slower than this loop: waking a worker costs more than the work it takes)
  const int mult0 = eae_geo_mult;
  eae_geo_mult = mult;
  for (int k = 0; k < n; ++k) {
    GroupRec& r = recs[k];
    r.clear();
    r.ctx = ctxs[k]; r.user = user; r.slot_of = &group_slot_of;
    eae_rec = &r;
    const int rc = what == 0 ? train_step_eager(ctxs[k], user, &ios[k], lrs[k]) : forward_impl(ctxs[k], user, &ios[k], false);
    eae_rec = nullptr;
    if (rc && !r.error) r.error = rc;
    if (r.error) r.msg = eae_last_error();
  }
  eae_geo_mult = mult0;
  // (on a failure the members have advanced their host-side state all the same: the group is unusable, as a context is after a failed step)
  for (int k = 0; k < n; ++k) if (recs[k].error) return eae_set_error(recs[k].error, recs[k].msg.c_str());
  const auto tp1 = std::chrono::steady_clock::now();
  // zip
  const size_t len = recs[0].items.size();
  for (int k = 1; k < n; ++k) {
    if (recs[k].items.size() != len) return eae_set_error(EAE_ERR_STATE, "group call: the members' launch sequences differ in length (different shapes or state)");
    for (size_t i = 0; i < len; ++i) {
      const GroupItem& a = recs[0].items[i];
      const GroupItem& b = recs[k].items[i];
      if (a.kind != b.kind || a.slot != b.slot || a.kg != b.kg || (a.kind == GroupItem::LAUNCH &&
          (a.grid.x != b.grid.x || a.grid.y != b.grid.y || a.grid.z != b.grid.z || a.block.x != b.block.x || a.smem != b.smem || a.arg_size != b.arg_size)))
        return eae_set_error(EAE_ERR_STATE, "group call: the members' launch sequences differ (different shapes or state)");
    }
  }
  const auto tp2 = std::chrono::steady_clock::now();
  const unsigned char* argv[64];
  for (size_t i = 0; i < len; ++i) {
    const GroupItem& a = recs[0].items[i];
    hipStream_t st = group_stream(c0, user, a.slot);
    switch (a.kind) {
      case GroupItem::LAUNCH:
        for (int k = 0; k < n; ++k) argv[k] = recs[k].argbuf.data() + recs[k].items[i].arg_off;
        if (a.fn(a.kg, a.grid, a.block, a.smem, st, argv, n)) return eae_set_error(EAE_ERR_HIP, "group call: a grouped launch failed");
        break;
      case GroupItem::EV_RECORD: EAE_HIP(hipEventRecord(a.ev, st)); break;
      case GroupItem::EV_WAIT: EAE_HIP(hipStreamWaitEvent(st, a.ev, 0)); break;
      case GroupItem::OP:
        for (int k = 0; k < n; ++k) if (int e = recs[k].items[i].op(st)) return eae_set_error(EAE_ERR_HIP, "group call: a copy / memset failed"), e;
        break;
    }
  }
  if (timing) {
    const auto tp3 = std::chrono::steady_clock::now();
    t_acc[0] += std::chrono::duration<double, std::micro>(tp1 - tp0).count();
    t_acc[1] += std::chrono::duration<double, std::micro>(tp2 - tp1).count();
    t_acc[2] += std::chrono::duration<double, std::micro>(tp3 - tp2).count();
    if (++t_n == 100) {
      fprintf(stderr, "[eae group] n=%d items=%zu  record %.1f us  zip %.1f us  enqueue %.1f us\n", n, len, t_acc[0] / 100, t_acc[1] / 100, t_acc[2] / 100);
      t_acc[0] = t_acc[1] = t_acc[2] = 0; t_n = 0;
    }
  }
  return 0;
}
}  // namespace

extern "C" int eae_group_train_step(eae_ctx* const* ctxs, int n, int geometry_mult, void* stream, const eae_step_io* ios, const float* lrs) {
  return group_run(0, ctxs, n, geometry_mult, stream, ios, lrs);
}
extern "C" int eae_group_forward(eae_ctx* const* ctxs, int n, int geometry_mult, void* stream, const eae_step_io* ios) {
  return group_run(1, ctxs, n, geometry_mult, stream, ios, nullptr);
}
