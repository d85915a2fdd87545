// Side streams of a context: device-side hand-overs and joins, and the hardware-queue probe.
#include "eae_ctx.h"
#include <chrono>
#include <cstdlib>
#include <mutex>

// ---------------------------------------------------------------------------------------------------------------------
// Hand-overs to the side streams.  Side work (the classification head, the loss bookkeeping, weight gradients and their slice
// reductions) only feeds the optimizer, so it runs on engine-owned streams beside the dependency chain of the caller's stream.
// Round 1 ordered every hand-over with an event record on the caller's stream: ~5 us of bubble each, 9-10 per step
// (tools/timeline.py).  Now the order is kept on the DEVICE:
//   sq_push   queue a launch (optionally pinned to side stream 0, whose order the head -> loss bookkeeping chain needs);
//   sq_fork   the queued group may start once the caller's stream has completed everything enqueued so far: it gets the next
//             progress value, which the NEXT kernel enqueued on the caller's stream publishes when it starts (take_sig);
//   sq_commit called right after that kernel has been enqueued: a one-wave gate kernel that polls the progress word goes to
//             every side stream that receives a member, then the members (round robin; each stream has its own split-K scratch).
// The gate is always enqueued AFTER the kernel that releases it, so streams that share a hardware queue cannot dead-lock, and its
// spin is bounded (eae_gate_timeouts).  EAE_FORK_EVENTS=1, and hipGraph capture, use event records instead.
// ---------------------------------------------------------------------------------------------------------------------
namespace {
bool gates_now(const eae_ctx* c) { return c->use_gates && !c->capturing; }
hipStream_t side_stream(eae_ctx* c, int k) { return k == 0 ? c->side : c->sidex[k - 1]; }
}  // namespace
void sq_push(eae_ctx* c, std::function<int(hipStream_t, float*)> f, int pin) { c->sq_items.push_back({std::move(f), pin}); }
void sq_fork(eae_ctx* c) {
  if (c->sq_items.empty() || c->sq_forked) return;
  c->sq_forked = true;
  if (!c->use_side || !gates_now(c)) return;
  c->sq_wait = ++c->sig_seq;
  c->pending_sig = c->sq_wait;
}
// the kernel about to be enqueued on the caller's stream publishes the pending progress value
void take_sig(eae_ctx* c, ConvArgs& a) {
  if (!c->pending_sig) return;
  a.sig = c->sigwords; a.sig_val = c->pending_sig;
  c->pending_sig = 0;
}
int sq_commit(eae_ctx* c, hipStream_t st) {
  c->sq_forked = false;
  if (c->sq_items.empty()) return 0;
  int rc = 0;
  if (!c->use_side) {
    for (auto& it : c->sq_items) if (!rc) rc = it.fn(st, c->wscratch);
    c->sq_items.clear();
    return rc;
  }
  const int ns = 1 + c->nx;
  // members -> streams
  std::vector<int> where(c->sq_items.size());
  unsigned used = 0;
  for (size_t i = 0; i < c->sq_items.size(); ++i) {
    where[i] = c->sq_items[i].pin >= 0 ? c->sq_items[i].pin : (c->side_rr++ % ns);
    used |= 1u << where[i];
  }
  if (gates_now(c)) {
    if (!c->sq_wait) { c->sq_wait = ++c->sig_seq; c->pending_sig = c->sq_wait; }      // commit without a fork: order after `st` as it stands
    if (c->pending_sig) {                      // no kernel of the caller's stream carried the value: publish it with a kernel of its own
      RC(eae_launch_signal(st, c->sigwords, c->pending_sig));
      c->pending_sig = 0;
    }
    GateArgs g = GateArgs();
    g.word[0] = c->sigwords; g.want[0] = c->sq_wait; g.n = 1; g.timeout = c->sigwords + 8; g.limit_ticks = c->gate_limit;
    for (int k = 0; k < ns; ++k) if (used & (1u << k)) RC(eae_launch_gate(side_stream(c, k), g));
  } else {
    hipEvent_t ev = c->ev_fork[c->ev_i];
    c->ev_i = (c->ev_i + 1) % eae_ctx::NEV;
    EAE_HIP(eae_event_record(ev, st));
    for (int k = 0; k < ns; ++k) if (used & (1u << k)) EAE_HIP(eae_stream_wait_event(side_stream(c, k), ev));
  }
  c->sq_wait = 0;
  c->side_used |= used;
  for (size_t i = 0; i < c->sq_items.size(); ++i)
    if (!rc) rc = c->sq_items[i].fn(side_stream(c, where[i]), where[i] == 0 ? c->wscratch : c->wscratchx[where[i] - 1]);
  c->sq_items.clear();
  return rc;
}
// everything enqueued so far on the extra side streams completes before later work on the first one (the DP path hands
// `side` to the all-reduce)
int fold_side2(eae_ctx* c) {
  if (!c->use_side) return 0;
  for (int i = 0; i < c->nx; ++i) {
    EAE_HIP(eae_event_record(c->ev_sx[i], c->sidex[i]));
    EAE_HIP(eae_stream_wait_event(c->side, c->ev_sx[i]));
  }
  return 0;
}
// join: work enqueued on `st` from now on starts after everything enqueued so far on the side streams.  With gates: every side
// stream that received work publishes a done-counter with a one-thread kernel, ONE gate on `st` waits for all of them.
// join_side_begin: first half of the gated join -- commits the pending side groups, publishes the side streams' done-counters and
// returns the gate that waits for them in *g (g->n == 0: nothing to wait for, or the event path is in use and join_side must follow).
// A caller that has one more kernel to enqueue on `st` hands the gate to that kernel's tail instead of paying a launch for it.
int join_side_begin(eae_ctx* c, hipStream_t st, GateArgs* g) {
  *g = GateArgs();
  if (!c->use_side || !gates_now(c)) return 0;
  RC(sq_commit(c, st));
  const int ns = 1 + c->nx;
  g->timeout = c->sigwords + 8; g->limit_ticks = c->gate_limit;
  for (int k = 0; k < ns; ++k) {
    if (!(c->side_used & (1u << k))) continue;
    c->side_done_seq[k] += 1;
    RC(eae_launch_signal(side_stream(c, k), c->sigwords + 1 + k, c->side_done_seq[k]));
    g->word[g->n] = c->sigwords + 1 + k; g->want[g->n] = c->side_done_seq[k]; g->n++;
  }
  c->side_used = 0;
  return 0;
}
int join_side(eae_ctx* c, hipStream_t st) {
  if (!c->use_side) return 0;
  if (gates_now(c)) {
    GateArgs g;
    RC(join_side_begin(c, st, &g));
    if (g.n) RC(eae_launch_gate(st, g));
    return 0;
  }
  RC(sq_commit(c, st));
  EAE_HIP(eae_event_record(c->ev_join, c->side));
  EAE_HIP(eae_stream_wait_event(st, c->ev_join));
  for (int i = 0; i < c->nx; ++i) {
    EAE_HIP(eae_event_record(c->ev_joinx[i], c->sidex[i]));
    EAE_HIP(eae_stream_wait_event(st, c->ev_joinx[i]));
  }
  c->side_used = 0;
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The caller's stream and the side streams must reach the GPU through DIFFERENT hardware queues: ROCm multiplexes a process's streams
// onto 4 hardware queues, which one a stream gets depends on the streams alive when it was created, and two streams that share a
// queue run one after the other (measured: the grouped B=64 step 0.73 instead of 0.62 ms in a process that had trained other
// contexts from worker threads before; bench.py's grid leg).  Checked once per (context, caller's stream) before the first step:
// a gate on stream A waits (bounded, 0.3 ms) for a word that a kernel enqueued AFTERWARDS on stream B publishes -- it times out exactly
// when B's kernel cannot start beside it.  A side stream that collides is replaced by a fresh one (created while the colliding one
// is still alive, so it lands elsewhere), up to 16 candidates.  EAE_STREAM_PROBE=0 switches the check off, =2 reports what it found.
// ---------------------------------------------------------------------------------------------------------------------
namespace {
// (two device words: [0] the word the gate waits for, [1] its time-out flag -- not the sticky word the optimizer looks at)
bool streams_share_queue(unsigned* w, hipStream_t a, hipStream_t b) {
  if (a == b) return true;
  if (hipMemsetAsync(w, 0, 8, a) != hipSuccess || hipStreamSynchronize(a) != hipSuccess) return false;
  GateArgs g = GateArgs();
  g.word[0] = w; g.want[0] = 1; g.n = 1; g.timeout = w + 1; g.limit_ticks = 30000ULL;      // 0.3 ms of the 100 MHz clock (a kernel that CAN start beside the gate does so within microseconds)
  if (eae_launch_gate(a, g) || eae_launch_signal(b, w, 1)) return false;
  hipStreamSynchronize(a); hipStreamSynchronize(b);
  unsigned to = 0;
  if (hipMemcpy(&to, w + 1, 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
  return to != 0;
}
bool streams_clash(unsigned* w, hipStream_t a, hipStream_t b) { return streams_share_queue(w, a, b) || streams_share_queue(w, b, a); }
// Streams that steps are running on, process-wide: the caller's streams of probed contexts, their side streams, and streams a
// driver has reserved for its worker threads (eae_reserve_stream: train.run_concurrent).  A context's side streams also keep clear of
// these -- two groups stepped from two threads use four streams, and the GPU has four hardware queues.  One probe at a time.
struct StreamRegistry {
  std::mutex mu;
  std::vector<std::pair<hipStream_t, const void*>> used;       // (stream, owner: a context, or nullptr for a reserved stream)
};
StreamRegistry& stream_registry() { static StreamRegistry r; return r; }
}  // namespace
int streams_distinct(eae_ctx* c, hipStream_t user) {
  static const int mode = getenv("EAE_STREAM_PROBE") ? atoi(getenv("EAE_STREAM_PROBE")) : 1;
  if (mode == 0 || !c->use_side || !c->use_gates || c->capturing || c->streams_exposed || eae_rec) return 0;
  const long long now_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
  c->last_step_ns.store(now_ns, std::memory_order_relaxed);
  if (c->probed && c->probed_user == user) return 0;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(user, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return 0;     // (not inside somebody's capture)
  StreamRegistry& reg = stream_registry();
  std::lock_guard<std::mutex> lock(reg.mu);
  c->probed = true; c->probed_user = user;
  EAE_HIP(hipDeviceSynchronize());
  unsigned* w = c->sigwords + 14;
  // forget this context's earlier claims (a new caller's stream), collect the others'
  for (size_t i = reg.used.size(); i-- > 0;) if (reg.used[i].second == c) reg.used.erase(reg.used.begin() + i);
  std::vector<hipStream_t> others;
  for (const auto& u : reg.used) {
    if (u.first == user) continue;
    const eae_ctx* o = static_cast<const eae_ctx*>(u.second);        // (a context that has not stepped for half a second is not in anybody's way)
    if (o && now_ns - o->last_step_ns.load(std::memory_order_relaxed) > 500000000LL) continue;
    others.push_back(u.first);
  }
  const int ns = 1 + c->nx;
  int replaced = 0, left = 0, left_other = 0;
  std::vector<hipStream_t> drop;
  for (int k = 0; k < ns; ++k) {
    hipStream_t* slot = k == 0 ? &c->side : &c->sidex[k - 1];
    for (int attempt = 0; attempt < 16; ++attempt) {
      bool clash = streams_clash(w, *slot, user);
      for (int j = 0; j < k && !clash; ++j) clash = streams_clash(w, *slot, j == 0 ? c->side : c->sidex[j - 1]);
      bool clash_other = false;
      for (size_t j = 0; j < others.size() && !clash && !clash_other; ++j) clash_other = streams_clash(w, *slot, others[j]);
      if (!clash && !clash_other) break;
      // (with the others' streams the four queues may simply be taken: after 12 candidates only collisions inside the context count.
      //  Four were not enough: two groups stepped from two threads need the ONE queue the other three streams leave free, and the
      //  runs in which the second group gave up early measured 0.72 instead of 0.94 M images/s)
      if (!clash && attempt >= 11) { left_other++; break; }
      if (attempt == 15) { left++; break; }
      hipStream_t fresh = nullptr;
      EAE_HIP(hipStreamCreateWithPriority(&fresh, hipStreamNonBlocking, 0));
      drop.push_back(*slot);            // destroyed at the end: while it lives, the next candidate goes to another queue
      *slot = fresh;
      replaced++;
    }
  }
  for (hipStream_t st : drop) hipStreamDestroy(st);
  reg.used.emplace_back(user, c);
  for (int k = 0; k < ns; ++k) reg.used.emplace_back(k == 0 ? c->side : c->sidex[k - 1], c);
  if (mode >= 2) fprintf(stderr, "[eae] stream probe: %d side stream(s) replaced, %d still share a hardware queue inside the context, %d with another context's (%zu other streams in use)\n", replaced, left, left_other, others.size());
  return 0;
}
void streams_forget(const eae_ctx* c) {
  StreamRegistry& reg = stream_registry();
  std::lock_guard<std::mutex> lock(reg.mu);
  for (size_t i = reg.used.size(); i-- > 0;) if (reg.used[i].second == c) reg.used.erase(reg.used.begin() + i);
}

extern "C" void* eae_side_stream(eae_ctx* c) { if (c) c->streams_exposed = true; return c ? (void*)c->side : nullptr; }
extern "C" void* eae_dp_stream(eae_ctx* c, int which) {
  if (!c || !c->use_side || which < 0 || which > 1) return nullptr;
  if (!c->dp_stream[which]) {
    if (hipStreamCreateWithFlags(&c->dp_stream[which], hipStreamNonBlocking) != hipSuccess) { c->dp_stream[which] = nullptr; return nullptr; }
    if (hipEventCreateWithFlags(&c->ev_part[which], EV_FLAGS) != hipSuccess) {
      hipStreamDestroy(c->dp_stream[which]); c->dp_stream[which] = nullptr; return nullptr;
    }
  }
  return (void*)c->dp_stream[which];
}
// Do two streams reach the GPU through the same hardware queue (1), through different ones (0)?  Synchronises the device; < 0: error.
extern "C" int eae_streams_share_queue(void* a, void* b) {
  static thread_local unsigned* w = nullptr;
  static thread_local int w_dev = -1;
  int dev = 0;
  EAE_HIP(hipGetDevice(&dev));
  if (!w || w_dev != dev) { EAE_HIP(hipMalloc(reinterpret_cast<void**>(&w), 64)); w_dev = dev; }      // (a few bytes per thread and device, kept)
  StreamRegistry& reg = stream_registry();
  std::lock_guard<std::mutex> lock(reg.mu);
  EAE_HIP(hipDeviceSynchronize());
  return streams_clash(w, (hipStream_t)a, (hipStream_t)b) ? 1 : 0;
}
// A driver that steps contexts from several threads reserves its worker streams (on = 1) before the first step: the contexts' side
// streams then keep clear of them too.  on = 0 releases.
extern "C" int eae_reserve_stream(void* stream, int on) {
  StreamRegistry& reg = stream_registry();
  std::lock_guard<std::mutex> lock(reg.mu);
  for (size_t i = reg.used.size(); i-- > 0;)
    if (reg.used[i].first == (hipStream_t)stream && reg.used[i].second == nullptr) reg.used.erase(reg.used.begin() + i);
  if (on) reg.used.emplace_back((hipStream_t)stream, nullptr);
  return 0;
}
