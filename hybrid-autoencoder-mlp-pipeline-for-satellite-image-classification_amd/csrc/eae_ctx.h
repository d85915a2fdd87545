// Internal: the engine context and what the translation units of the C API share.
#pragma once
#include "eae_internal.h"
#include "eae_args.h"
#include "eae_layers.h"
#include "eae_wgrad_plan.h"
#include <atomic>
#include <functional>
#include <vector>

#define RC(x) do { int rc__ = (x); if (rc__) return rc__; } while (0)

constexpr float BN_EPS = 1e-5f, BN_MOM = 0.1f;

struct eae_ctx {
  eae_config cfg;
  int H, W, L, C, Bm;
  int Cin = 3, CP = 4;             // image bands (eae_config::in_channels) and their padded width in the edge kernels (edge_cp)
  // The latent-projection kernels work on a latent width padded to a multiple of 64 (Lp): the padded weight rows / columns are
  // zero in the packs, so the padded latent columns are exactly zero.  When Lp != L (`lpad`) the kernels that produce gradients in
  // parameter layout write padded shadows (gs_*), which compact_* copies into the gradient arena; with Lp == L they write the arena.
  int Lp = 0;
  bool lpad = false;
  float *gs_encw = nullptr, *gs_encb = nullptr, *gs_decw = nullptr, *gs_head = nullptr, *zstage = nullptr;
  size_t pk_w1p = 0, pk_bep = 0;     // lpad: fp32 copies of classifier.0.weight [128][Lp] and enc.fc.bias [Lp]
  // fp8 variant of the six 3x3 layers' GEMMs (eae_config::quant = 1, BASELINE config 5): e4m3 weight packs + delayed-scaling state
  bool fp8 = false;
  size_t pk8_p1[6] = {}, pk8_p2[6] = {};
  Fp8State* q = nullptr;
  float* bn_save = nullptr;          // eae_fp8_calibrate: copy of the running statistics + num_batches_tracked
  long long Pn, K;                 // pixels of the 256-channel map, flattened features
  long long poff[T_COUNT + 1], bnoff[2 * N_BN + 1];
  float *P = nullptr, *G = nullptr, *M = nullptr, *V = nullptr, *bnrun = nullptr;
  long long* nbt = nullptr;
  long long adam_step = 0;
  bool packed = false;
  bool fwd_ready = false;          // a train-mode forward with gradient staging is resident in the workspace
  bool fwd_eval_ready = false;     // ... or an eval-mode one (BatchNorm with running statistics): eae_ae_backward differentiates that too
  bool has_enc = true, has_dec = true;   // halves of the model the bound arenas really hold (eae_set_halves; a stand-alone Encoder's engine has no decoder)
  int enc_ready = 0, dec_ready = 0; // stand-alone eae_encoder_forward / eae_decoder_forward resident: 0 no, 1 train mode, 2 eval mode
  bool bwd_eval = false;           // the running backward differentiates an eval-mode forward: BatchNorm is a per-channel affine map
  bool prebn_dirty = false;        // an eval-mode backward wrote the gradients of the biases in front of the BatchNorms (train mode: zero)
  int fwd_B = 0, fwd_head = 0;
  const float* fwd_x = nullptr;    // only used between eae_ae_grad_step_begin / _end (the caller keeps the batch alive in between)
  long long fwd_gen = 0;           // bumped by every forward: eae_ae_backward refuses to differentiate a forward that is no longer resident
  // workspace
  void* ws = nullptr;
  bf16_t *y[4], *u[3], *d0, *gy[4], *gu[3], *gd0, *g4;
  // dy = BatchNorm-backward-applied gradients, written by the backward-data kernels while they stage them (ConvArgs::dy_out) and
  // read by the weight-gradient kernels: dyy[i] has the shape of gy[i] (i = 1..3), dyu[i] that of gu[i]
  bf16_t *dyy[4], *dyu[3];
  float *z, *dz, *dzc, *coef_f[7], *coef_b[7], *stat, *wscratch, *fcpart, *msepart, *cepart, *headpart, *lossbuf;
  long long wscratch_floats, head_stride;
  uint8_t* pack = nullptr;
  size_t pack_bytes = 0;           // length of the pack arena (eae_debug_fill_packs)
  PackDesc* descs_dev = nullptr;
  int ndesc = 0;
  unsigned short* blkmap = nullptr;   // flattened pack launch (eae_pack_assign_blocks): workgroup -> descriptor; blk_tot workgroups
  int blk_tot = 0;
  size_t pk_c1, pk_p1[6], pk_p2[6], pk_d4j, pk_d4k, pk_we1, pk_we2, pk_wd1, pk_wd2, pk_bd;
  // second stream: weight-gradient kernels, the classifier head and the slice reductions do not sit on the
  // forward / backward-data dependency chain, so they run concurrently with it (fork/join through events)
  hipStream_t side = nullptr;
  // extra side streams: weight-gradient groups go round-robin over side + these, each with its own split-K scratch, so a
  // layer's slice reduction overlaps the next layers' wgrad kernels
  static constexpr int MAXX = 3;
  int nx = 0;
  hipStream_t sidex[MAXX] = {};
  hipEvent_t ev_joinx[MAXX] = {}, ev_sx[MAXX] = {};
  float* wscratchx[MAXX] = {};
  float* wscratch_main = nullptr;      // conv1's weight gradient: EAE_EDGE_WGRAD_SCRATCH_SLICES partials (eae_wgrad_plan.h)
  long long wscratch_main_floats = 0;
  // data-parallel hand-off streams: after a gradient step #0 is ordered after gradient tensors 18..37 (classifier, decoder,
  // dec.fc) and #1 after tensors 8..17 (enc.fc, conv4, conv3); tensors 0..7 are complete when the step's join is reached
  hipStream_t dp_stream[2] = {nullptr, nullptr};
  hipEvent_t ev_part[2] = {nullptr, nullptr};
  // RCCL communicator owned by the engine (eae_dp_init): the gradient all-reduce is enqueued by the engine itself, no host
  // code between the backward and the collective
  void* dp_comm = nullptr;
  int dp_rank = 0, dp_world = 0;
  hipEvent_t ev_dp_done = nullptr;
  // folded BatchNorm finalize (forward): fixed-point statistics accumulators per BN layer
  unsigned long long* accf[7] = {};
  int acc_copies[7] = {};
  unsigned long long* accb[7] = {};      // BatchNorm-backward accumulators (same region and layout, behind the forward ones)
  bool fold_bwd = true;
  uint8_t* acc_base = nullptr;
  size_t poison_off = 0;       // byte offset of the step-wide non-finite word inside the accumulator region (cleared with it)
  size_t acc_bytes = 0;
  bool acc_clean = false;          // all zero (cleared by the engine's own Adam launch or at creation)
  bool bwd_dirty = false;          // the BACKWARD half of the accumulators holds the sums of an earlier backward (no clear since)
  size_t acc_half = 0;             // byte offset of the backward half inside the accumulator region
  // synchronized BatchNorm across data-parallel replicas (eae_set_sync_bn): the batch statistics of every BN layer are summed
  // over the replicas through the caller's hook (forward: the fixed-point accumulators; backward: the fp64 sums) before the
  // consumers turn them into coefficients with the GLOBAL element count
  int sync_world = 1;
  eae_sync_fn sync_fn = nullptr;
  void* sync_user = nullptr;
  double* sync_sums = nullptr;     // caller-owned device buffer [7][2][256] fp64
  bool fold_fwd = true;
  int side_rr = 0;
  // Hand-overs to the side streams (sq_* below): queued launches, the progress value their group waits for, the value the next
  // kernel of the caller's stream has to publish, and the device words: [0] progress of the caller's stream, [1 + k] work done
  // by side stream k, [8] gate time-out report, [10] unused, [12..13] data-parallel flags, [14..15] the queue probe.
  struct SideItem { std::function<int(hipStream_t, float*)> fn; int pin; };
  std::vector<SideItem> sq_items;
  unsigned sig_seq = 0, sq_wait = 0, pending_sig = 0;
  bool sq_forked = false;          // the queued group has been released (sq_fork): commit it behind the next kernel of the caller's stream
  unsigned* sigwords = nullptr;
  unsigned side_done_seq[1 + MAXX] = {};
  unsigned side_used = 0;          // bit k: side stream k received work since the last join
  // Per layer: does the backward-data kernel store dy (ConvArgs::dy_out) for the weight gradient, which then runs BEHIND it on one
  // plain tensor, or does the weight gradient transform g and y itself and run BESIDE the backward-data kernel?  bit i (1..3) =
  // enc.conv(i+1), bit 4 + i (0..2) = dec.deconv(i+1).  EAE_DY_MASK overrides (diagnostic A/B).
  unsigned dy_mask = 0;
  int nan_exact = 0;               // EAE_NAN_EXACT=1: a diverged step writes NaN into every parameter and moment like the reference's does
  bool skip_wgrad = false;         // EAE_SKIP_WGRAD=1 (diagnostic): the six 3x3 weight gradients are not launched (main chain alone)
  bool use_gates = true;           // device-side gates instead of event records on the caller's stream (EAE_FORK_EVENTS=1: events)
  unsigned long long gate_limit = 3000000000ULL;     // gate spin bound in 100 MHz ticks (30 s; EAE_GATE_TIMEOUT_MS, 0 = unbounded)
  float* last_loss = nullptr;      // the caller's loss_last buffer of the most recent step: poisoned with NaN when a gate has timed out
  std::atomic<long long> last_step_ns{0};   // steady-clock time of the last step that went through streams_distinct (idle contexts' claims are ignored)
  bool streams_exposed = false;     // eae_side_stream() handed a side stream to the caller: it is never replaced afterwards
  hipStream_t probed_user = nullptr; bool probed = false;   // streams_distinct(): the caller's stream the side streams were checked against
  hipStream_t own_main = nullptr;  // capture is not permitted on the legacy default stream: graphs run here, bracketed by events
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  static constexpr int NEV = 16;
  hipEvent_t ev_fork[NEV] = {};
  hipEvent_t ev_join = nullptr;
  hipEvent_t ev_head = nullptr;    // classification head finished on the side stream
  bool head_pending = false;
  int ev_i = 0;
  bool use_side = true;
  // hipGraph replay of the whole train step: ~80 launches + fork/join events per step make the eager path host-bound
  struct GraphKey {
    const void *x, *labels, *x_hat, *accum, *last;
    int B, head; float alpha;
    bool operator==(const GraphKey& o) const {
      return x == o.x && labels == o.labels && x_hat == o.x_hat && accum == o.accum && last == o.last && B == o.B && head == o.head && alpha == o.alpha;
    }
  };
  struct GraphEntry { GraphKey key; int seen = 0; hipGraphExec_t exec = nullptr; hipGraph_t graph = nullptr; };
  static constexpr int NGRAPH = 8;
  GraphEntry graphs[NGRAPH];
  int ngraphs = 0;
  bool use_graph = true;
  bool capturing = false;
  // class-weighted CrossEntropyLoss with ignored labels (eae_set_class_weights): the head runs its weighted kernels when either is set
  const float* class_w = nullptr;  // caller-owned device fp32 [C], or nullptr (all ones)
  long long ignore_index = EAE_NO_IGNORE;
  bool wce() const { return class_w != nullptr || ignore_index != EAE_NO_IGNORE; }
  long long* valid_acc = nullptr;  // eae_set_valid_counter: caller-owned device word, += counted rows of every step that accumulates its loss
  // global gradient-norm clipping (eae_set_grad_clip): every optimizer launch of the context is preceded by the sum-of-squares kernel
  float clip_max = 0.f;            // 0 = off; > 0 or +inf = on
  float* clip_out = nullptr;       // caller-owned device float[2] (total, coef), or nullptr
  double* clip_part = nullptr;     // workspace: EAE_CLIP_MAX_PARTS fp64 partials
  long long psize[T_COUNT];        // elements of the 38 tensors without the layout's rounding
  bool clip_on() const { return clip_max != 0.f; }
  float* dyn = nullptr;            // device: lr/bc1, sqrt(bc2) of the current Adam step (graph path)
  // optional in-situ timing of ONE launch site (eae_profile_enable(ctx, site); sites: include/eae.h) with HIP events on the
  // stream that launch goes to
  static constexpr int PROF_RING = 64;
  bool prof_on = false;
  int prof_site = 0;
  int prof_n = 0;
  hipEvent_t prof_ev[3 * PROF_RING] = {};     // per sample: before, after, after an EMPTY bracket (calibration)
  EaeProfHook prof_hook = {};
  long long act_elems(int lvl) const {   // per-image elements of the map after `lvl` stride-2 stages (1..4)
    return (long long)(H >> lvl) * (W >> lvl) * enc_channels(lvl);
  }
  // the arenas by tensor (eae_layers.h: EaeTensor); numel = the tensor's length in the arena (rounded up to 4)
  float* param(int t) const { return P + poff[t]; }
  float* grad(int t) const { return G + poff[t]; }
  long long numel(int t) const { return poff[t + 1] - poff[t]; }
  long long arena_len() const { return poff[T_COUNT]; }
  // ... and by BatchNorm layer l (0..6)
  float* bn_gamma(int l) const { return param(BN_LAYERS[l].gamma); }
  float* bn_beta(int l) const { return param(BN_LAYERS[l].gamma + 1); }
  float* bn_dgamma(int l) const { return grad(BN_LAYERS[l].gamma); }
  float* bn_dbeta(int l) const { return grad(BN_LAYERS[l].gamma + 1); }
  float* bn_rmean(int l) const { return bnrun + bnoff[2 * l]; }
  float* bn_rvar(int l) const { return bnrun + bnoff[2 * l + 1]; }
  float* prebn_dbias(int l) const { return grad(BN_LAYERS[l].bias); }
  // the raw output of BatchNorm layer l (y[0..3], u[0..2]), its gradient and the dy tensor of its 3x3 layer
  bf16_t* act(int l) const { return l < 4 ? y[l] : u[l - 4]; }
  bf16_t* gact(int l) const { return l < 4 ? gy[l] : gu[l - 4]; }
  bf16_t*& dyact(int l) { return l < 4 ? dyy[l] : dyu[l - 4]; }
};

// a forward (full, or one half alone) is no longer resident: no backward may differentiate it
inline void invalidate_forward(eae_ctx* c) { c->fwd_ready = false; c->fwd_eval_ready = false; c->enc_ready = 0; c->dec_ready = 0; }
// host-side state behind an optimizer launch (rc = its status).  The step's loss_last buffer is the caller's: it is written (NaN, when
// the update is refused) by THAT launch only.  The packs are stale, and the optimizer kernel has cleared the accumulators when it ran.
inline void after_optimizer(eae_ctx* c, int rc) {
  c->last_loss = nullptr;
  c->packed = false; c->acc_clean = (rc == 0); c->bwd_dirty = !c->acc_clean;
}
inline long long r4(long long n) { return (n + 3) & ~3LL; }
inline unsigned* poison_word(const eae_ctx* c) { return reinterpret_cast<unsigned*>(c->acc_base + c->poison_off); }
inline SrcDesc src_raw(const bf16_t* p) { SrcDesc s; s.p0 = p; s.p1 = nullptr; s.coef = nullptr; return s; }
inline SrcDesc src_bnrelu(const bf16_t* y, const float* coef) { SrcDesc s; s.p0 = y; s.p1 = nullptr; s.coef = coef; return s; }
inline SrcDesc src_bnbwd(const bf16_t* g, const bf16_t* y, const float* coef) { SrcDesc s; s.p0 = g; s.p1 = y; s.coef = coef; return s; }
inline SrcDesc src_f32(const float* p) { SrcDesc s; s.p0 = reinterpret_cast<const bf16_t*>(p); s.p1 = nullptr; s.coef = nullptr; return s; }

extern const unsigned EV_FLAGS;     // eae_ctx.hip: flags of every event the engine creates

// eae_streams.hip
void sq_push(eae_ctx* c, std::function<int(hipStream_t, float*)> f, int pin = -1);
void sq_fork(eae_ctx* c);
void take_sig(eae_ctx* c, ConvArgs& a);
int sq_commit(eae_ctx* c, hipStream_t st);
int fold_side2(eae_ctx* c);
int join_side_begin(eae_ctx* c, hipStream_t st, GateArgs* g);
int join_side(eae_ctx* c, hipStream_t st);
int streams_distinct(eae_ctx* c, hipStream_t user);
void streams_forget(const eae_ctx* c);

// eae_step.hip
int ensure_packed(eae_ctx* c, hipStream_t st);
int prep_accumulators(eae_ctx* c, hipStream_t st, bool train);
int copy_latent_out(eae_ctx* c, hipStream_t st, float* dst, const float* src_padded, int B);
int run_encoder(eae_ctx* c, hipStream_t st, const float* x, int B, bool train, const eae_scene* scene = nullptr, const SceneSrc* ssrc = nullptr);
int run_decoder_trunk(eae_ctx* c, hipStream_t st, const float* z, int B, bool train, Deconv4Args& d);
int check_io(eae_ctx* c, const eae_step_io* io, bool need_grad);
int forward_impl(eae_ctx* c, hipStream_t st, const eae_step_io* io, bool want_grad);
int backward_impl(eae_ctx* c, hipStream_t st, const eae_step_io* io, const float* dz_ext = nullptr, int part = 0);
int train_step_eager(eae_ctx* c, hipStream_t st, const eae_step_io* io, float lr);
// the engine's Adam over the first n arena elements, behind the sum-of-squares launch when eae_set_grad_clip is on; bad / bad2 = the
// words that make it refuse the update (default: the context's own); dyn = the graph path's form (scalars from c->dyn)
int launch_adam(eae_ctx* c, hipStream_t st, long long n, float lr, float wd, float grad_scale, const unsigned* bad = nullptr,
                const unsigned* bad2 = nullptr, bool dyn = false);
// optimizer.step(): launch_adam over the whole arena and the host-side state behind it
int optimizer_step(eae_ctx* c, hipStream_t st, float lr, float wd, float grad_scale, const unsigned* bad = nullptr, const unsigned* bad2 = nullptr);
// dL/d(pre-sigmoid) from (x_hat, dx_hat) into g (bf16 NHWC-CP), then deconv4's bias gradient db from the per-block partials in `part`
int sigmoid_bwd_bias(hipStream_t st, const float* x_hat, const float* dx_hat, int C, int B, int H, int W, void* g, float* db, float* part);
