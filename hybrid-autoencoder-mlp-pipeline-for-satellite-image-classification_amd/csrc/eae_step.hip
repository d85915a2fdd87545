// Forward, backward and optimizer step of the supervised autoencoder, and the C entry points over them.
#include "eae_ctx.h"
#include <cmath>
#include <cstdlib>

// ---- helpers of this file
namespace {

// HIP-event bracket around ONE launch on the stream it goes to (bench.py's `roofline`): before / after, then an EMPTY bracket
// recorded right behind it, which measures what the two event records cost by themselves on that stream.
static void prof_hook_begin(void* u, hipStream_t st) {
  eae_ctx* c = static_cast<eae_ctx*>(u);
  hipEventRecord(c->prof_ev[3 * c->prof_n], st);
}
static void prof_hook_end(void* u, hipStream_t st) {
  eae_ctx* c = static_cast<eae_ctx*>(u);
  hipEventRecord(c->prof_ev[3 * c->prof_n + 1], st);
  hipEventRecord(c->prof_ev[3 * c->prof_n + 2], st);
  c->prof_n++;
}
// hook for launchers that enqueue a second kernel behind the timed one; nullptr when `site` is not the one being profiled
static const EaeProfHook* prof_hook_for(eae_ctx* c, int site) {
  if (!(c->prof_on && c->prof_site == site && c->prof_n < eae_ctx::PROF_RING && !c->capturing)) return nullptr;
  c->prof_hook = EaeProfHook{prof_hook_begin, prof_hook_end, c};
  return &c->prof_hook;
}
struct ProfBracket {
  eae_ctx* c; hipStream_t st; bool on;
  ProfBracket(eae_ctx* c_, int site, hipStream_t st_) : c(c_), st(st_), on(prof_hook_for(c_, site) != nullptr) {
    if (on) prof_hook_begin(c, st);
  }
  ~ProfBracket() { if (on) prof_hook_end(c, st); }
};

// split-K of the latent projections: K range per slice (eae_wgrad_plan.h) under this process's EAE_FC_SLICES
int fc_klen(const eae_ctx* c) {
  static const int slices = getenv("EAE_FC_SLICES") ? atoi(getenv("EAE_FC_SLICES")) : 64;
  return eae_fc_klen(c->K, slices);
}

// the [C] sticky non-finite flag words of BN layer l sit behind the layer's [acc_copies][2][C] accumulators (forward or backward half)
unsigned long long* acc_flag(const eae_ctx* c, unsigned long long* acc, int l) { return acc + (size_t)c->acc_copies[l] * 2 * BN_LAYERS[l].c; }
// 2^24: a workgroup's sums of y and y^2 stay below 2^38 / (workgroups per channel x SyncBN world), or the channel is flagged and the
// step reads NaN (eae_bn_acc.h).  At batch 512 conv1 has 4096 workgroups per channel: sum y^2 < 2^26 over a tile of 128 positions, an
// rms of y below 2^9.5 = 724; conv4 (64 workgroups of 128) reaches 2^12.5.  Below the limit the sums are exact to 2^-25 each.
constexpr float ACC_SCALE_FWD = BN_ACC_SCALE_FWD;

// fp8 variant: weight pack, scales and the amax word of 3x3 layer j (W3 order) for a forward / backward-data launch
void fp8_conv_args(eae_ctx* c, ConvArgs& a, int j, bool forward, bool p1) {
  if (!c->fp8) return;
  a.wpack = (const bf16_t*)(c->pack + (p1 ? c->pk8_p1[j] : c->pk8_p2[j]));
  a.qs = forward ? c->q->qs_fwd[j] : c->q->qs_bwd[j];
  a.amax = forward ? c->q->amax_act[j] : c->q->amax_grad[j];
  a.amax_mask = FP8_AMAX_SLOTS - 1; a.amax_stride = FP8_AMAX_STRIDE;
}

// producer side of the folded forward finalize of BN layer l
void fold_producer(eae_ctx* c, ConvArgs& a, int l, bool train) {
  if (!train || !c->fold_fwd) return;
  a.bacc.acc = c->accf[l]; a.bacc.copies = c->acc_copies[l]; a.bacc.scale = ACC_SCALE_FWD; a.bacc.flag = acc_flag(c, c->accf[l], l);
  a.bacc.world = c->sync_world;       // (the launcher turns it into the limit of one contribution: bn_acc_set_limit)
  a.stat_part = nullptr;
}
// consumer side: coefficient table of BN layer l from its accumulators
// SyncBN: sum layer l's forward accumulators over the replicas (order-independent integer sums: every replica ends with the
// same bits) between its producer and its first consumer
int sync_fwd(eae_ctx* c, hipStream_t st, int l, bool train) {
  if (!train || c->sync_world <= 1) return 0;
  if (!c->fold_fwd) return eae_set_error(EAE_ERR_STATE, "SyncBN needs the folded forward finalize (unset EAE_NO_FOLD_FWD)");
  const long long off = (long long)(c->accf[l] - reinterpret_cast<unsigned long long*>(c->acc_base));
  if (c->sync_fn(c->sync_user, 0, off, (long long)c->acc_copies[l] * 2 * BN_LAYERS[l].c + BN_LAYERS[l].c, (void*)st) != 0)      // (+C: the non-finite flag words)
    return eae_set_error(EAE_ERR_STATE, "SyncBN: the exchange hook failed (forward statistics)");
  return 0;
}
void fold_consumer(eae_ctx* c, BnFold& f, int l, long long count, bool train) {
  f = BnFold();
  if (!train || !c->fold_fwd) return;
  count *= c->sync_world;
  f.acc = c->accf[l]; f.copies = c->acc_copies[l]; f.inv_scale = 1.0f / ACC_SCALE_FWD; f.count = (float)count; f.flag = acc_flag(c, c->accf[l], l);
  f.poison = poison_word(c);
  f.momentum = BN_MOM; f.eps = BN_EPS;
  f.gamma = c->bn_gamma(l); f.beta = c->bn_beta(l);
  f.rm = c->bn_rmean(l); f.rv = c->bn_rvar(l); f.nbt = c->nbt ? c->nbt + l : nullptr;
  f.coef_out = c->coef_f[l];
}

// The BACKWARD accumulators must be zero when their producers start (the forward ones: prep_accumulators).  A train-mode forward with the folded finalize has just cleared the
// whole region (or the optimizer kernel did); what is left are the sequences that reach a backward without either: eval-mode
// backward after eval-mode backward (autograd with frozen statistics and an external optimizer), EAE_NO_FOLD_FWD -- their sums
// used to pile up (found by the EAE_NO_FOLD_FWD x fp8-calibration sweep: 8 gradient steps, gradients 92x too large)
int prep_bwd_accumulators(eae_ctx* c, hipStream_t st) {
  if (!c->fold_bwd) return 0;
  if (c->bwd_dirty) EAE_HIP(eae_memset_async(c->acc_base + c->acc_half, 0, c->poison_off - c->acc_half, st));
  c->bwd_dirty = true; c->acc_clean = false;
  return 0;
}

int bn_fwd_finalize(eae_ctx* c, hipStream_t st, int l, int ntiles, long long count, bool train) {
  if (train && c->fold_fwd) return 0;       // folded into the producer (accumulators) and the next kernel (prologue)
  if (train) return eae_launch_bn_finalize(st, c->stat, ntiles, BN_LAYERS[l].c, count, c->bn_gamma(l), c->bn_beta(l), c->bn_rmean(l), c->bn_rvar(l),
                                           c->nbt ? c->nbt + l : nullptr, BN_MOM, BN_EPS, c->coef_f[l]);
  return eae_launch_bn_eval_coef(st, BN_LAYERS[l].c, c->bn_gamma(l), c->bn_beta(l), c->bn_rmean(l), c->bn_rvar(l), BN_EPS, c->coef_f[l]);
}

constexpr float ACC_SCALE_BWD = BN_ACC_SCALE_BWD;   // 2^42 (eae_common.hip.h, BnBwdFold; range: eae_bn_acc.h)
bool bwd_folded(const eae_ctx* c, int l) { (void)l; return c->fold_bwd && c->sync_world <= 1; }
int bwd_copies(const eae_ctx* c, int l) { return std::min(c->acc_copies[l], BN_FOLD_KB * (256 / BN_LAYERS[l].c)); }
// producer side of the folded BatchNorm-backward finalize of layer l: call before launching the kernel whose epilogue takes the sums
void fold_bwd_producer(eae_ctx* c, ConvArgs& a, int l) {
  if (!bwd_folded(c, l)) return;
  a.stat_part = nullptr;
  a.bacc.acc = c->accb[l]; a.bacc.copies = bwd_copies(c, l); a.bacc.scale = ACC_SCALE_BWD; a.bacc.flag = acc_flag(c, c->accb[l], l);
  a.bacc.world = 1;                   // (folded only without SyncBN: bwd_folded)
}
// consumer side: the kernels that read layer l's (g, y) pair with SRC_BNBWD build A, B, Cc from the accumulators; `writer`: the
// main-stream consumer, whose workgroup 0 also stores dgamma / dbeta and the table
void fold_bwd_consumer(eae_ctx* c, BnBwdFold& f, int l, long long count, bool writer) {
  f = BnBwdFold();
  if (!bwd_folded(c, l)) return;
  f.acc = c->accb[l]; f.copies = bwd_copies(c, l); f.inv_scale = 1.0f / ACC_SCALE_BWD; f.flag = acc_flag(c, c->accb[l], l);
  f.poison = poison_word(c);
  f.count = c->bwd_eval ? __builtin_inff() : (float)count;
  f.gamma = c->bn_gamma(l); f.coef_fwd = c->coef_f[l];
  if (writer) {
    f.dgamma = c->bn_dgamma(l); f.dbeta = c->bn_dbeta(l); f.coef_out = c->coef_b[l];
    if (c->bwd_eval) f.dbias = c->prebn_dbias(l);
  }
}

int bn_bwd_fin(eae_ctx* c, hipStream_t st, int l, int ntiles, long long count) {
  if (bwd_folded(c, l)) return 0;           // folded into the producer (accumulators) and its consumers (prologue)
  if (c->bwd_eval) count = 1LL << 40;       // eval-mode BatchNorm: no batch-size terms (see eae_ae_backward)
  if (c->sync_world > 1) {
    double* sums = c->sync_sums + (size_t)l * 512;
    RC(eae_launch_bn_bwd_reduce(st, c->stat, ntiles, BN_LAYERS[l].c, sums, c->bn_dgamma(l), c->bn_dbeta(l)));
    if (c->sync_fn(c->sync_user, 1, (long long)l * 512, 2LL * BN_LAYERS[l].c, (void*)st) != 0)
      return eae_set_error(EAE_ERR_STATE, "SyncBN: the exchange hook failed (backward sums)");
    return eae_launch_bn_bwd_coef(st, sums, BN_LAYERS[l].c, count * c->sync_world, c->bn_gamma(l), c->coef_f[l], c->coef_b[l]);
  }
  return eae_launch_bn_bwd_finalize(st, c->stat, ntiles, BN_LAYERS[l].c, count, c->bn_gamma(l), c->coef_f[l], c->bn_dgamma(l), c->bn_dbeta(l), c->coef_b[l]);
}

int copy_latent_in(eae_ctx* c, hipStream_t st, float* dst_padded, const float* src, int B) {      // padding columns of dst stay as they are (zero)
  if (!c->lpad) { EAE_HIP(hipMemcpyAsync(dst_padded, src, (size_t)B * c->L * 4, hipMemcpyDeviceToDevice, st)); return 0; }
  EAE_HIP(hipMemcpy2DAsync(dst_padded, (size_t)c->Lp * 4, src, (size_t)c->L * 4, (size_t)c->L * 4, B, hipMemcpyDeviceToDevice, st));
  return 0;
}
const float* stage_latent_in(eae_ctx* c, hipStream_t st, const float* src, int B, int* rc) {
  *rc = 0;
  if (!c->lpad || !src) return src;
  hipError_t e = hipMemcpy2DAsync(c->zstage, (size_t)c->Lp * 4, src, (size_t)c->L * 4, (size_t)c->L * 4, B, hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) { *rc = eae_set_error(EAE_ERR_HIP, hipGetErrorString(e)); return nullptr; }
  return c->zstage;          // padding columns stay zero (cleared once at creation, never written)
}

int run_decoder(eae_ctx* c, hipStream_t st, const float* z, int B, bool train, const float* target, float gscale, float* x_hat,
                bool want_grad, bool want_loss) {
  Deconv4Args d;
  RC(run_decoder_trunk(c, st, z, B, train, d));
  d.x = target; d.x_hat = x_hat; d.g4 = want_grad ? c->g4 : nullptr; d.loss_part = (want_loss || want_grad) ? c->msepart : nullptr;
  d.gscale = gscale;
  {
    ProfBracket pb(c, EAE_PROF_DECONV4_LOSS, st);
    RC(eae_launch_deconv4_loss(st, SRC_BNRELU, d));
  }
  return 0;
}

int run_head(eae_ctx* c, hipStream_t st, int B, const long long* labels, float* logits, bool want_grad, const float* dlogits_in,
             bool count_valid = false) {
  HeadArgs h = HeadArgs();
  h.dlogits_in = dlogits_in;
  h.z = c->z; h.w1 = c->lpad ? (const float*)(c->pack + c->pk_w1p) : c->param(T_CLS0_W); h.b1 = c->param(T_CLS0_B); h.w2 = c->param(T_CLS2_W); h.b2 = c->param(T_CLS2_B);
  h.labels = labels; h.B = B; h.L = c->Lp; h.C = c->C; h.inv_batch = 1.0f / (float)B;
  h.logits = logits; h.dz = c->dzc; h.grad_part = want_grad ? c->headpart : nullptr; h.grad_stride = c->head_stride;
  h.loss_part = c->cepart;
  if (c->wce()) return eae_launch_head_w(st, h, c->class_w, c->ignore_index, count_valid ? c->valid_acc : nullptr);     // (labels NULL or external dlogits: the plain kernels)
  return eae_launch_head(st, h);
}

// ---- the six 3x3 stride-2 layers (eae_layers.h: L3[j]).  What differs between them comes from the table row: conv layers use the
//      p1 packs forward and the transposed launcher with the p2 packs backward, transposed layers the other way round; deconv1's
//      input d0 is raw (no BatchNorm in front of it).

// the layer's input as a source: BatchNorm + ReLU of the layer in front applied on load, or d0 as it is
SrcDesc l3_input(const eae_ctx* c, const Layer3& r) { return r.bn_in < 0 ? src_raw(c->d0) : src_bnrelu(c->act(r.bn_in), c->coef_f[r.bn_in]); }

// forward: raw output (bf16) + the statistics of its BatchNorm
int l3_forward(eae_ctx* c, hipStream_t st, int j, int B, bool train) {
  const Layer3& r = L3[j];
  const bool conv = r.kind == L3_CONV;
  ConvArgs a = ConvArgs();
  a.src = l3_input(c, r);
  a.wpack = (const bf16_t*)(c->pack + (conv ? c->pk_p1[j] : c->pk_p2[j])); a.bias = c->param(r.b); a.out = c->act(r.bn_out);
  a.stat_part = train ? c->stat : nullptr;
  a.B = B; a.Hin = c->H >> r.in_lvl(); a.Win = c->W >> r.in_lvl();
  fold_producer(c, a, r.bn_out, train);
  if (r.bn_in >= 0) fold_consumer(c, a.fold, r.bn_in, (long long)B * a.Hin * a.Win, train);
  fp8_conv_args(c, a, j, true, conv);
  {
    ProfBracket pb(c, EAE_PROF_SITE(r.site, 0), st);
    RC((conv ? eae_launch_conv_s2 : eae_launch_deconv_s2)(a, r.cin, r.cout, r.bn_in < 0 ? SRC_RAW : SRC_BNRELU, EPI_FWD, st));
  }
  RC(sync_fwd(c, st, r.bn_out, train));
  return bn_fwd_finalize(c, st, r.bn_out, eae_conv_s2_ntiles(r.kind, r.cin, r.cout, B, a.Hin, a.Win),
                         (long long)B * (c->H >> r.out_lvl()) * (c->W >> r.out_lvl()), train);
}

// backward: the weight gradient (queued for a side stream) and backward-data into the BatchNorm + ReLU of the layer in front (deconv1:
// plainly into gd0).  dy mode: backward-data first -- while it stages dy = BatchNorm-backward(g, y) of this layer's output it also
// stores it (dy_out); the weight gradient queued behind it reads that one tensor and is released when the NEXT kernel of the chain
// starts.  Otherwise the weight gradient transforms g and y itself and is released together with the backward-data kernel.
int l3_backward(eae_ctx* c, hipStream_t st, int j, int B) {
  const Layer3& r = L3[j];
  const bool conv = r.kind == L3_CONV;
  const int cs = r.cs(), cb = r.cb(), lo = r.bn_out;
  const int Hs = c->H >> r.lvl, Ws = c->W >> r.lvl;                                  // the small map
  const int Ho = c->H >> r.out_lvl(), Wo = c->W >> r.out_lvl();                      // the map of the output and its gradient
  const bool dym = (c->dy_mask >> r.dy_bit) & 1u;
  auto push_wgrad = [&]() {
    if (c->skip_wgrad) return;
    sq_push(c, [=](hipStream_t s2, float* scr) {
      const Layer3& lr = L3[j];
      const SrcDesc g = dym ? src_raw(c->dyact(lo)) : src_bnbwd(c->gact(lo), c->act(lo), c->coef_b[lo]), x = l3_input(c, lr);
      const int gk = dym ? SRC_RAWG : SRC_BNBWD, xk = lr.bn_in < 0 ? SRC_RAW : SRC_BNRELU;
      WgradArgs w = WgradArgs();
      w.small = conv ? g : x; w.big = conv ? x : g;         // a conv's small side is its output, a transposed conv's its input
      w.B = B; w.Hs = Hs; w.Ws = Ws;
      if (!dym) fold_bwd_consumer(c, w.bfold, lo, (long long)B * Ho * Wo, false);
      if (c->fp8) w.qs = c->q->qs_wg[j];
      return eae_launch_wgrad_s2(s2, w, cs, cb, conv ? gk : xk, conv ? xk : gk, scr, c->wscratch_floats, c->grad(lr.w),
                                 prof_hook_for(c, EAE_PROF_SITE(lr.site, 2)));
    });
    sq_fork(c);              // released by the next kernel of the chain (dy mode, conv2: by conv1's weight gradient)
  };
  if (!dym) push_wgrad();
  ConvArgs a = ConvArgs();
  a.src = src_bnbwd(c->gact(lo), c->act(lo), c->coef_b[lo]);
  a.dy_out = dym ? c->dyact(lo) : nullptr;
  a.wpack = (const bf16_t*)(c->pack + (conv ? c->pk_p2[j] : c->pk_p1[j]));
  a.B = B; a.Hin = Ho; a.Win = Wo;
  fold_bwd_consumer(c, a.bfold, lo, (long long)B * Ho * Wo, true);
  fp8_conv_args(c, a, j, false, !conv);
  const int li = r.bn_in;
  if (li >= 0) {
    a.out = c->gact(li); a.stat_part = c->stat; a.yprev = c->act(li); a.prev_coef = c->coef_f[li];
    fold_bwd_producer(c, a, li);
  } else {
    a.out = c->gd0;
  }
  take_sig(c, a);
  {                          // backward-data of a conv is a transposed conv cout -> cin, and the other way round
    ProfBracket pb(c, EAE_PROF_SITE(r.site, 1), st);
    RC((conv ? eae_launch_deconv_s2 : eae_launch_conv_s2)(a, r.cout, r.cin, SRC_BNBWD, li >= 0 ? EPI_MASK : EPI_PLAIN, st));
  }
  if (c->sq_forked) RC(sq_commit(c, st));
  if (li >= 0)
    RC(bn_bwd_fin(c, st, li, eae_conv_s2_ntiles(conv ? L3_DECONV : L3_CONV, r.cout, r.cin, B, Ho, Wo),
                  (long long)B * (c->H >> r.in_lvl()) * (c->W >> r.in_lvl())));
  if (dym) push_wgrad();
  return 0;
}

}  // namespace

int ensure_packed(eae_ctx* c, hipStream_t st) {
  if (c->packed) return 0;
  // (the pack kernel also clears the step-wide non-finite word: the optimizer kernel that clears the accumulators READS that word)
  RC(eae_launch_pack_flat(st, c->descs_dev, c->blkmap, 0, c->blk_tot, c->P, c->pack, c->fp8 ? c->q : nullptr, poison_word(c)));
  c->packed = true;
  return 0;
}

// the statistics accumulators of a train-mode forward must be zero when its producers start: the engine's own Adam clears them
// as a side job, any other sequence (forward only, external optimizer, encoder / decoder alone) pays one memset here
int prep_accumulators(eae_ctx* c, hipStream_t st, bool train) {
  if (!train || !c->fold_fwd) return 0;
  if (!c->acc_clean || c->capturing) { EAE_HIP(eae_memset_async(c->acc_base, 0, c->acc_bytes, st)); c->bwd_dirty = false; }   // a captured step always carries it
  c->acc_clean = false;
  return 0;
}

// latent-width padding (eae_ctx::Lp): copies between the caller's [B][L] tensors and the padded [B][Lp] workspace rows
int copy_latent_out(eae_ctx* c, hipStream_t st, float* dst, const float* src_padded, int B) {
  if (!c->lpad) { EAE_HIP(hipMemcpyAsync(dst, src_padded, (size_t)B * c->L * 4, hipMemcpyDeviceToDevice, st)); return 0; }
  EAE_HIP(hipMemcpy2DAsync(dst, (size_t)c->L * 4, src_padded, (size_t)c->Lp * 4, (size_t)c->L * 4, B, hipMemcpyDeviceToDevice, st));
  return 0;
}

// ---- encoder: x -> y[0..3] (raw, bf16) + BN coefficients -> z (fp32)
// scene (eval mode only): conv1 reads windows of a device-resident scene instead of the fp32 batch x; every later layer is unchanged
int run_encoder(eae_ctx* c, hipStream_t st, const float* x, int B, bool train, const eae_scene* scene, const SceneSrc* ssrc) {
  const int H = c->H, W = c->W;
  {
    EdgeArgs a;
    a.src3 = x; a.B = B; a.H = H; a.W = W; a.C = c->Cin;
    a.c = ConvArgs();
    a.c.wpack = (const bf16_t*)(c->pack + c->pk_c1); a.c.bias = c->param(T_CONV1_B); a.c.out = c->y[0];
    a.c.stat_part = train ? c->stat : nullptr; a.c.B = B;
    fold_producer(c, a.c, 0, train);
    {
      ProfBracket pb(c, EAE_PROF_SITE(0, 0), st);
      if (scene) RC(eae_launch_edge_conv_scene(st, eae_scene_src3_kind(scene), a, *ssrc));
      else RC(eae_launch_edge_conv(st, SRC3_NCHW_F32, EPI_FWD, a));
    }
    RC(sync_fwd(c, st, 0, train));
    RC(bn_fwd_finalize(c, st, 0, eae_edge_tiles(B, H, W), (long long)B * (H / 2) * (W / 2), train));
  }
  for (int j = 0; j < L3_FIRST_DECONV; ++j) RC(l3_forward(c, st, j, B, train));      // conv2, conv3, conv4
  FcNtArgs f = FcNtArgs();
  f.a = src_bnrelu(c->y[3], c->coef_f[3]);
  f.w = (const bf16_t*)(c->pack + c->pk_we1);
  f.M = B; f.N = c->Lp; f.K = (int)c->K; f.klen = fc_klen(c); f.part = c->fcpart;
  fold_consumer(c, f.c.fold, 3, (long long)B * c->Pn, train);
  const int ksplit = (int)(c->K / f.klen);
  RC(eae_launch_fc_nt(st, f, SRC_BNRELU, FCE_PARTIAL, ksplit));
  RC(eae_launch_fc_reduce(st, c->fcpart, ksplit, B, c->Lp, c->lpad ? (const float*)(c->pack + c->pk_bep) : c->param(T_ENCFC_B), nullptr,
                          nullptr, c->z));
  return 0;
}

// ---- decoder: z (fp32 [B][L]) -> d0, u[0..2] -> deconv4 + sigmoid (+ MSE and its gradient)

// z -> d0 -> u[0..2]: everything in front of deconv4; fills deconv4's arguments except its epilogue outputs
int run_decoder_trunk(eae_ctx* c, hipStream_t st, const float* z, int B, bool train, Deconv4Args& d) {
  const int H = c->H, W = c->W;

  {
    FcNtArgs f = FcNtArgs();
    f.a = src_f32(z);
    f.w = (const bf16_t*)(c->pack + c->pk_wd1);
    f.M = B; f.N = (int)c->K; f.K = c->Lp; f.klen = c->Lp;
    f.c = ConvArgs();
    f.c.out = c->d0; f.c.bias = (const float*)(c->pack + c->pk_bd);
    take_sig(c, f.c);
    RC(eae_launch_fc_nt(st, f, SRC_F32, FCE_BIAS_BF16, 1));
    RC(sq_commit(c, st));          // the classification head (queued by forward_impl) starts beside the decoder
  }
  for (int j = L3_FIRST_DECONV; j < N_L3; ++j) RC(l3_forward(c, st, j, B, train));    // deconv1, deconv2, deconv3
  d = Deconv4Args();
  d.src = src_bnrelu(c->u[2], c->coef_f[6]);
  d.wjoint = (const bf16_t*)(c->pack + c->pk_d4j); d.bias = c->param(T_DECONV4_B);
  d.B = B; d.Hin = H / 2; d.Win = W / 2; d.C = c->Cin;
  fold_consumer(c, d.fold, 6, (long long)B * (H / 2) * (W / 2), train);
  return 0;
}

// A backward that differentiates an eval-mode forward (eae_ctx::bwd_eval), for as long as it is being enqueued; it writes the
// gradients of the biases in front of the BatchNorms, which a later train-mode backward has to clear again (prebn_dirty)
struct EvalBackward {
  eae_ctx* c;
  EvalBackward(eae_ctx* c_, bool eval) : c(c_) { c->bwd_eval = eval; if (eval) c->prebn_dirty = true; }
  ~EvalBackward() { c->bwd_eval = false; }
};

// the arenas are bound and the batch fits the workspace
static int check_bound_batch(const eae_ctx* c, int B) {
  if (!c->P || !c->bnrun) return eae_set_error(EAE_ERR_STATE, "eae_bind has not been called");
  if (B <= 0 || B > c->Bm) return eae_set_error(EAE_ERR_ARG, "batch size outside 1..max_batch");
  return 0;
}
int sigmoid_bwd_bias(hipStream_t st, const float* x_hat, const float* dx_hat, int C, int B, int H, int W, void* g, float* db, float* part) {
  RC(eae_launch_sigmoid_bwd(st, x_hat, dx_hat, g, part, B, H, W, C));
  const int nblk = (int)(((long long)B * H * W + 255) / 256);
  return eae_launch_loss_finalize(st, part, nblk, nullptr, 0, 0.f, 1.0, B, db, nullptr, nullptr, nullptr, C);
}

int check_io(eae_ctx* c, const eae_step_io* io, bool need_grad) {
  if (!c || !io) return eae_set_error(EAE_ERR_ARG, "ctx / io is NULL");
  RC(check_bound_batch(c, io->B));
  if (!io->x) return eae_set_error(EAE_ERR_ARG, "io->x is NULL");
  if (need_grad) {
    if (!c->G) return eae_set_error(EAE_ERR_STATE, "no gradient arena bound");
    if (io->head && !io->labels) return eae_set_error(EAE_ERR_ARG, "labels required when head=1");
    if (!io->train) return eae_set_error(EAE_ERR_ARG, "gradient step requires train=1 (BatchNorm batch statistics)");
  }
  return 0;
}

int forward_impl(eae_ctx* c, hipStream_t st, const eae_step_io* io, bool want_grad) {
  const int B = io->B;
  const bool train = io->train != 0;
  c->fwd_ready = train; c->fwd_eval_ready = !train; c->enc_ready = 0; c->dec_ready = 0; c->fwd_B = B; c->fwd_head = io->head; c->fwd_x = io->x; c->fwd_gen += 1;
  if (want_grad) c->last_loss = io->loss_last;
  RC(ensure_packed(c, st));
  RC(prep_accumulators(c, st, train));
  RC(run_encoder(c, st, io->x, B, train));
  const double numel = (double)B * c->Cin * c->H * c->W;
  const float gscale = (float)(2.0 * io->alpha / numel);
  const bool want_loss = io->loss_accum || io->loss_last;
  const bool head = io->head != 0;
  // The head only needs z: in a gradient step it runs on the side stream beside the decoder; the backward waits for it
  // (ev_head) right before dz_cls is added to dz.  (head_kernel is built without packed-FP32 instructions, see EAE_NO_PK.)
  if (head) {
    if (want_grad && c->use_side) {
      const long long* labels = io->labels;
      float* logits = io->logits;
      const bool count = io->loss_accum != nullptr;      // the labelled-sample count goes with the loss accumulators
      sq_push(c, [=](hipStream_t hs, float*) {
        RC(run_head(c, hs, B, labels, logits, true, nullptr, count));
        EAE_HIP(eae_event_record(c->ev_head, hs));
        return 0;
      }, 0);
      sq_fork(c);                  // released by the decoder's first kernel (run_decoder commits behind it)
      c->head_pending = true;
    } else {
      RC(run_head(c, st, B, io->labels, io->logits, want_grad, nullptr, io->loss_accum != nullptr));
    }
  }
  RC(run_decoder(c, st, c->z, B, train, (want_loss || want_grad) ? io->x : nullptr, gscale, io->x_hat, want_grad, want_loss));
  if (io->z) RC(copy_latent_out(c, st, io->z, c->z, B));
  if (want_loss || want_grad) {
    const int n_ce = (head && io->labels) ? eae_head_blocks(B, c->Lp) : 0;
    // in a gradient step nothing on the main stream reads what this kernel writes (deconv4 bias gradient, loss scalars):
    // it goes to the side stream, which backward_impl joins before the optimizer
    if (want_grad && c->use_side) {
      const float alpha = io->alpha;
      float *accum = io->loss_accum, *last = io->loss_last;
      const int ntile = eae_edge_tiles(B, c->H, c->W);
      sq_push(c, [=](hipStream_t ls, float*) {
        return eae_launch_loss_finalize(ls, c->msepart, ntile, c->cepart, n_ce, alpha, numel, B, c->grad(T_DECONV4_B), accum, last, poison_word(c),
                                        c->Cin);
      }, 0);
      sq_fork(c);                  // released by the first kernel of the backward-data chain (backward_impl commits behind it)
    } else {
      RC(eae_launch_loss_finalize(st, c->msepart, eae_edge_tiles(B, c->H, c->W), c->cepart, n_ce, io->alpha, numel, B,
                                  want_grad ? c->grad(T_DECONV4_B) : nullptr, io->loss_accum, io->loss_last, poison_word(c), c->Cin));
    }
  }
  return 0;
}

// part 0 = everything, 1 = classifier + decoder + dec.fc (gradient tensors 18..37), 2 = enc.fc + encoder (tensors 0..17)
int backward_impl(eae_ctx* c, hipStream_t st, const eae_step_io* io, const float* dz_ext, int part) {
  const int B = io->B, H = c->H, W = c->W;
  // (part 2 = the encoder half: behind part 1 of a split backward -- whose side-stream consumers may still be reading the decoder
  //  layers' sums -- nothing is cleared; the stand-alone encoder backward clears before it calls)
  if (part != 2) RC(prep_bwd_accumulators(c, st));
  if (c->prebn_dirty && !c->bwd_eval) {      // train mode again: those biases have an identically zero gradient, never written
    for (int l = 0; l < N_BN; ++l) EAE_HIP(eae_memset_async(c->prebn_dbias(l), 0, (size_t)c->numel(BN_LAYERS[l].bias) * 4, st));
    c->prebn_dirty = false;
  }
  const bool head = io->head != 0;
  const bool dp = part != 0 || c->dp_stream[0] != nullptr || c->dp_stream[1] != nullptr;
  if (part != 2) {
    // ---- first group (side stream 0, behind the loss bookkeeping forward_impl queued): classifier weight gradients from the
    //      head kernel's partials, deconv4's weight gradient.  Released by the first kernel of the backward-data chain.
    c->side_rr = 1;                // the round robin of the later groups starts at side stream #1
    if (head) {
      sq_push(c, [=](hipStream_t ss, float*) {
        const int nb = eae_head_blocks(B, c->Lp);
        RC(eae_launch_reduce_slices(ss, c->headpart, nb, (long)(c->head_stride / 4), c->lpad ? c->gs_head : c->grad(T_CLS0_W), 1.0f));
        if (c->lpad) {     // padded shadow -> arena: classifier.0.weight [128][L], then bias / classifier.2 (contiguous, the arena's last)
          EAE_NO_GROUP("a latent width that needs the padded classifier shadow");
          EAE_HIP(hipMemcpy2DAsync(c->grad(T_CLS0_W), (size_t)c->L * 4, c->gs_head, (size_t)c->Lp * 4, (size_t)c->L * 4, CLS_HIDDEN,
                                   hipMemcpyDeviceToDevice, ss));
          EAE_HIP(hipMemcpyAsync(c->grad(T_CLS0_B), c->gs_head + (long long)CLS_HIDDEN * c->Lp, (size_t)(c->grad(T_COUNT) - c->grad(T_CLS0_B)) * 4,
                                 hipMemcpyDeviceToDevice, ss));
        }
        return 0;
      }, 0);
    } else {
      sq_push(c, [=](hipStream_t ss, float*) {
        EAE_HIP(eae_memset_async(c->grad(T_CLS0_W), 0, (size_t)(c->grad(T_COUNT) - c->grad(T_CLS0_W)) * 4, ss));
        return 0;
      }, 0);
    }
    sq_push(c, [=](hipStream_t ss, float* scr) {
      return eae_launch_edge_wgrad(ss, SRC3_NHWCP_BF16, c->g4, B, H, W, src_bnrelu(c->u[2], c->coef_f[6]), SRC_BNRELU, scr,
                                   c->wscratch_floats, c->grad(T_DECONV4_W), prof_hook_for(c, EAE_PROF_SITE(7, 2)), nullptr, nullptr, 0,
                                   nullptr, nullptr, c->Cin);
    }, 0);
    sq_fork(c);
    // ---- deconv4: backward-data into u[2]'s BN+ReLU
    {
      EdgeArgs a;
      a.src3 = c->g4; a.B = B; a.H = H; a.W = W; a.C = c->Cin;
      a.c = ConvArgs();
      a.c.wpack = (const bf16_t*)(c->pack + c->pk_d4k); a.c.out = c->gu[2]; a.c.stat_part = c->stat;
      a.c.yprev = c->u[2]; a.c.prev_coef = c->coef_f[6]; a.c.B = B;
      fold_bwd_producer(c, a.c, 6);
      take_sig(c, a.c);
      {
        ProfBracket pb(c, EAE_PROF_DECONV4_BWD, st);
        RC(eae_launch_edge_conv(st, SRC3_NHWCP_BF16, EPI_MASK, a));
      }
      RC(sq_commit(c, st));
      RC(bn_bwd_fin(c, st, 6, eae_edge_tiles(B, H, W), (long long)B * (H / 2) * (W / 2)));
    }
    // ---- deconv3, deconv2, deconv1: weight gradients queued, handed over together before the last dgrad
    for (int j = N_L3 - 1; j >= L3_FIRST_DECONV; --j) RC(l3_backward(c, st, j, B));
    // ---- dec.fc: weight/bias gradient (queued: needs gd0) and dz
    sq_push(c, [=](hipStream_t s2, float*) {
      FcTnArgs t = FcTnArgs();
      t.p = src_raw(c->gd0); t.q = src_f32(c->z); t.Bt = B; t.I = (int)c->K; t.J = c->Lp;
      t.out = c->lpad ? c->gs_decw : c->grad(T_DECFC_W); t.colsum = c->grad(T_DECFC_B); t.out_mode = 0; t.Pn = (int)c->Pn;
      RC(eae_launch_fc_tn(s2, t, SRC_RAW, SRC_F32));
      if (c->lpad) EAE_HIP(hipMemcpy2DAsync(c->grad(T_DECFC_W), (size_t)c->L * 4, c->gs_decw, (size_t)c->Lp * 4, (size_t)c->L * 4,
                                            (size_t)c->K, hipMemcpyDeviceToDevice, s2));
      return 0;
    });
    sq_fork(c);
    {
      FcNtArgs f = FcNtArgs();
      f.a = src_raw(c->gd0); f.w = (const bf16_t*)(c->pack + c->pk_wd2);
      f.M = B; f.N = c->Lp; f.K = (int)c->K; f.klen = fc_klen(c); f.part = c->fcpart;
      f.c = ConvArgs();
      take_sig(c, f.c);
      const int ksplit = (int)(c->K / f.klen);
      RC(eae_launch_fc_nt(st, f, SRC_RAW, FCE_PARTIAL, ksplit));
      if (c->sq_forked) RC(sq_commit(c, st));
      if (c->head_pending) { EAE_HIP(eae_stream_wait_event(st, c->ev_head)); c->head_pending = false; }
      int src_rc = 0;
      const float* dze = stage_latent_in(c, st, dz_ext, B, &src_rc);      // caller's [B][L] gradient -> padded rows
      RC(src_rc);
      RC(eae_launch_fc_reduce(st, c->fcpart, ksplit, B, c->Lp, nullptr, head ? c->dzc : nullptr, dze, c->dz));
    }
    if (dp) RC(sq_commit(c, st));  // the hand-off below covers gradient tensors 18..37 only (ordered after `st` as it stands)
  }   // part != 2
  if (part == 1) return fold_side2(c);     // the caller may now all-reduce gradient tensors 18..37 behind the side stream
  if (part == 0 && c->dp_stream[0]) {      // same hand-off without splitting the call: see eae_dp_stream()
    RC(fold_side2(c));
    EAE_HIP(hipEventRecord(c->ev_part[0], c->side));
    EAE_HIP(hipStreamWaitEvent(c->dp_stream[0], c->ev_part[0], 0));
  }
  // ---- enc.fc: weight/bias gradient (queued with the dec.fc one: needs dz) and backward-data into y[3]'s BN+ReLU
  sq_push(c, [=](hipStream_t s2, float*) {
    FcTnArgs t = FcTnArgs();
    t.p = src_f32(c->dz); t.q = src_bnrelu(c->y[3], c->coef_f[3]); t.Bt = B; t.I = c->Lp; t.J = (int)c->K;
    t.out = c->lpad ? c->gs_encw : c->grad(T_ENCFC_W); t.colsum = c->lpad ? c->gs_encb : c->grad(T_ENCFC_B); t.out_mode = 1; t.Pn = (int)c->Pn;
    RC(eae_launch_fc_tn(s2, t, SRC_F32, SRC_BNRELU));
    if (c->lpad) {       // the first L rows of the padded shadows are the arena tensors
      EAE_HIP(eae_memcpy_d2d_async(c->grad(T_ENCFC_W), c->gs_encw, (size_t)c->L * c->K * 4, s2));
      EAE_HIP(eae_memcpy_d2d_async(c->grad(T_ENCFC_B), c->gs_encb, (size_t)c->L * 4, s2));
    }
    return 0;
  });
  sq_fork(c);
  {
    FcNtArgs f = FcNtArgs();
    f.a = src_f32(c->dz); f.w = (const bf16_t*)(c->pack + c->pk_we2);
    f.M = B; f.N = (int)c->K; f.K = c->Lp; f.klen = c->Lp;
    f.c = ConvArgs();
    f.c.out = c->gy[3]; f.c.stat_part = c->stat; f.c.yprev = c->y[3]; f.c.prev_coef = c->coef_f[3];
    fold_bwd_producer(c, f.c, 3);
    take_sig(c, f.c);
    RC(eae_launch_fc_nt(st, f, SRC_F32, FCE_MASK, 1));
    RC(sq_commit(c, st));
    RC(bn_bwd_fin(c, st, 3, ((B + 127) / 128) * (int)c->Pn, (long long)B * c->Pn));
  }
  // ---- conv4, conv3, conv2: weight gradient (queued; conv4 + conv3 go together, conv2 before the last dgrad so
  //      that it runs beside it and beside conv1's weight gradient) + backward-data
  for (int j = L3_FIRST_DECONV - 1; j >= 0; --j) {
    RC(l3_backward(c, st, j, B));
    if (L3[j].w == T_CONV3_W && part == 0 && c->dp_stream[1]) {     // enc.fc, conv4 and conv3 weight gradients: enqueued by the commit below
      RC(sq_commit(c, st));
      RC(fold_side2(c));
      EAE_HIP(hipEventRecord(c->ev_part[1], c->side));
      EAE_HIP(hipStreamWaitEvent(c->dp_stream[1], c->ev_part[1], 0));
    }
  }
  // ---- conv1 weight gradient: nothing is left for the main stream to do, so the last weight gradient runs there (no fork
  //      latency in the tail of the step) while the side streams drain
  BnBwdFold bf0;
  fold_bwd_consumer(c, bf0, 0, (long long)B * (H / 2) * (W / 2), true);
  {
    ConvArgs sg = ConvArgs();                          // carries the progress value that releases conv2's weight gradient
    take_sig(c, sg);
    // the join with the side streams rides in the tail of this weight gradient's slice reduction (one launch less in the step's
    // tail).  The side groups are committed BETWEEN the two launches: gates go behind the kernel that releases them (see sq_commit).
    struct Mid { eae_ctx* c; hipStream_t st; } mid = {c, st};
    auto mid_fn = [](void* u, GateArgs* g) { Mid* m = static_cast<Mid*>(u); return join_side_begin(m->c, m->st, g); };
    RC(eae_launch_edge_wgrad(st, SRC3_NCHW_F32, io->x, B, H, W, src_bnbwd(c->gy[0], c->y[0], c->coef_b[0]), SRC_BNBWD, c->wscratch_main,
                             c->wscratch_main_floats, c->grad(T_CONV1_W), prof_hook_for(c, EAE_PROF_CONV1_WGRAD), &bf0, sg.sig, sg.sig_val,
                             +mid_fn, &mid, c->Cin));
  }
  RC(join_side(c, st));                                 // (nothing left to wait for when the gate went with the reduction)
  if (c->fp8) RC(eae_launch_fp8_scales(st, c->q));      // every reader of this step's scales has finished: derive the next step's
  // Biases in front of a BatchNorm have an identically zero gradient (the reference computes ~1e-9 rounding noise);
  // their slots in the gradient arena are zeroed once in eae_bind and never written.
  return 0;
}


extern "C" int eae_ae_forward(eae_ctx* c, void* stream, const eae_step_io* io) {
  RC(check_io(c, io, false));
  return forward_impl(c, (hipStream_t)stream, io, false);
}

// Backward of the most recent TRAIN-mode eae_ae_forward for externally supplied output gradients (the autograd path:
// `loss.backward()` on a torch loss built from x_hat / logits / z, R.md:649-653).  Activations of that forward are still
// resident in the workspace; the INPUT batch is not (conv1's weight gradient reads it): the caller passes it again, together
// with the generation id of the forward it differentiates.  Any of dlogits / dz may be NULL (= zero).
extern "C" long long eae_forward_generation(eae_ctx* c) { return c ? c->fwd_gen : -1; }
extern "C" int eae_ae_backward(eae_ctx* c, void* stream, long long generation, const float* x, const float* x_hat, const float* dx_hat,
                               const float* dlogits, const float* dz) {
  if (!c || !c->G) return eae_set_error(EAE_ERR_STATE, "backward: no gradient arena bound");
  if (!c->fwd_ready && !c->fwd_eval_ready) return eae_set_error(EAE_ERR_STATE, "backward: no forward is resident (call eae_ae_forward first)");
  if (generation != c->fwd_gen)
    return eae_set_error(EAE_ERR_STATE, "backward: a later forward has replaced the activations of the forward being differentiated "
                                        "(one backward per forward, in order)");
  if (!x || !x_hat || !dx_hat) return eae_set_error(EAE_ERR_ARG, "backward: x, x_hat and dx_hat are required");
  hipStream_t st = (hipStream_t)stream;
  const int B = c->fwd_B;
  eae_step_io io = eae_step_io();
  io.x = x; io.B = B; io.train = 1; io.head = (dlogits != nullptr) ? 1 : 0;
  RC(sigmoid_bwd_bias(st, x_hat, dx_hat, c->Cin, B, c->H, c->W, c->g4, c->grad(T_DECONV4_B), c->msepart));
  if (dlogits) RC(run_head(c, st, B, nullptr, nullptr, true, dlogits));
  // An eval-mode forward normalises with the running statistics: y -> gamma*(y - rm)*invstd_r + beta is affine per channel, so its
  // backward is dy = gamma*invstd_r * g with dgamma = sum g*xhat_r, dbeta = sum g -- the same kernels with the batch-size terms
  // (B and C of the BatchNorm-backward transform, both ~ 1/count) switched off by an infinite count.
  if (c->fwd_eval_ready && !(c->fold_bwd && c->sync_world <= 1))
    return eae_set_error(EAE_ERR_STATE, "backward of an eval-mode forward needs the folded BatchNorm-backward finalize (no EAE_NO_FOLD_BWD, no SyncBN)");
  EvalBackward eb(c, c->fwd_eval_ready);
  const int rc = backward_impl(c, st, &io, dz);
  invalidate_forward(c);
  return rc;
}

extern "C" int eae_ae_grad_step(eae_ctx* c, void* stream, const eae_step_io* io) {
  RC(check_io(c, io, true));
  hipStream_t st = (hipStream_t)stream;
  RC(streams_distinct(c, st));
  RC(forward_impl(c, st, io, true));
  return backward_impl(c, st, io);
}

// fp8 variant: settle the delayed scales before the first real step.  Every iteration is a gradient step without the optimizer (the
// fp8 packs are rebuilt with the current weight scale each time); a scale is right once the tensors upstream of it were computed with
// right scales, so the backward chain of 6 layers needs 7 iterations.  BatchNorm running statistics and num_batches_tracked are
// restored afterwards; the gradient arena holds the last iteration's gradients.
extern "C" int eae_fp8_calibrate(eae_ctx* c, void* stream, const eae_step_io* io, int iters) {
  RC(check_io(c, io, true));
  if (!c->fp8) return eae_set_error(EAE_ERR_STATE, "fp8_calibrate: the context was not created with quant = 1");
  if (iters <= 0) iters = 7;
  hipStream_t st = (hipStream_t)stream;
  eae_step_io t = *io;
  t.x_hat = nullptr; t.logits = nullptr; t.z = nullptr; t.loss_accum = nullptr; t.loss_last = nullptr;
  const size_t bn_bytes = (size_t)c->bnoff[14] * 4;
  EAE_HIP(hipMemcpyAsync(c->bn_save, c->bnrun, bn_bytes, hipMemcpyDeviceToDevice, st));
  if (c->nbt) EAE_HIP(hipMemcpyAsync(c->bn_save + c->bnoff[14], c->nbt, 7 * 8, hipMemcpyDeviceToDevice, st));
  for (int it = 0; it < iters; ++it) {
    c->packed = false;
    RC(forward_impl(c, st, &t, true));
    RC(backward_impl(c, st, &t));
  }
  EAE_HIP(hipMemcpyAsync(c->bnrun, c->bn_save, bn_bytes, hipMemcpyDeviceToDevice, st));
  if (c->nbt) EAE_HIP(hipMemcpyAsync(c->nbt, c->bn_save + c->bnoff[14], 7 * 8, hipMemcpyDeviceToDevice, st));
  c->packed = false; invalidate_forward(c);
  return 0;
}
// current scales: s_act[6], s_grad[6], s_w[6] (3x3 layers in the order conv2, conv3, conv4, deconv1, deconv2, deconv3); synchronises
extern "C" int eae_fp8_scales(eae_ctx* c, float* out18) {
  if (!c || !out18) return eae_set_error(EAE_ERR_ARG, "fp8_scales: NULL argument");
  if (!c->fp8) return eae_set_error(EAE_ERR_STATE, "fp8_scales: the context was not created with quant = 1");
  EAE_HIP(hipDeviceSynchronize());
  Fp8State h;
  EAE_HIP(hipMemcpy(&h, c->q, sizeof(h), hipMemcpyDeviceToHost));
  for (int i = 0; i < 6; ++i) { out18[i] = h.s_act[i]; out18[6 + i] = h.s_grad[i]; out18[12 + i] = h.s_w[i]; }
  return 0;
}

// dyn: the form a captured step replays -- step size and bias correction come from c->dyn (eae_launch_set_dyn ran on this stream), the
// step's own memset clears the accumulators and nan_exact is not honoured
int launch_adam(eae_ctx* c, hipStream_t st, long long n, float lr, float wd, float grad_scale, const unsigned* bad, const unsigned* bad2, bool dyn) {
  AdamLaunch a;
  a.p = c->P; a.g = c->G; a.m = c->M; a.v = c->V; a.n = n;
  a.lr = lr; a.wd = wd; a.step = c->adam_step; a.gscale = grad_scale;
  a.bad = bad ? bad : c->sigwords + 8; a.bad2 = bad2 ? bad2 : poison_word(c); a.nan_out = c->last_loss;
  if (dyn) a.dyn = c->dyn;
  else { a.zero_buf = c->acc_base; a.zero_bytes = (long long)c->poison_off; a.nan_fill = c->nan_exact; }
  if (c->clip_on()) {      // eae_set_grad_clip: the partial sums of g^2 over the 38 tensors, on this stream and right in front of the optimizer
    RC(eae_launch_grad_sumsq(st, c->G, c->poff, c->psize, c->clip_part));
    a.clip = {c->clip_part, eae_grad_sumsq_parts(c->arena_len()), c->clip_max, c->clip_out};
  }
  return eae_launch_adam(st, a);
}
int optimizer_step(eae_ctx* c, hipStream_t st, float lr, float wd, float grad_scale, const unsigned* bad, const unsigned* bad2) {
  if (!c || !c->P || !c->G || !c->M || !c->V) return eae_set_error(EAE_ERR_STATE, "adam: parameter, gradient and moment arenas must be bound");
  c->adam_step += 1;
  const int rc = launch_adam(c, st, c->arena_len(), lr, wd, grad_scale, bad, bad2);
  after_optimizer(c, rc);
  return rc;
}
extern "C" int eae_adam_step(eae_ctx* c, void* stream, float lr, float weight_decay) { return eae_adam_step_scaled(c, stream, lr, weight_decay, 1.0f); }

// Data-parallel pieces: the gradient step in two halves so that the all-reduce of the first half's gradients (tensors
// 18..37: dec.fc, decoder, classifier) can run behind the side stream while the encoder half is still being computed.
extern "C" int eae_ae_grad_step_begin(eae_ctx* c, void* stream, const eae_step_io* io) {
  RC(check_io(c, io, true));
  hipStream_t st = (hipStream_t)stream;
  RC(forward_impl(c, st, io, true));
  return backward_impl(c, st, io, nullptr, 1);
}
extern "C" int eae_ae_grad_step_end(eae_ctx* c, void* stream) {
  if (!c || !c->fwd_ready) return eae_set_error(EAE_ERR_STATE, "grad_step_end without grad_step_begin");
  eae_step_io io = eae_step_io();
  io.x = c->fwd_x; io.B = c->fwd_B; io.train = 1; io.head = c->fwd_head;
  int rc = backward_impl(c, (hipStream_t)stream, &io, nullptr, 2);
  invalidate_forward(c);
  return rc;
}
// optimizer.step() on gradients that are SUMS over `1/grad_scale` replicas (grad_scale = 1/world_size)
extern "C" int eae_adam_step_scaled(eae_ctx* c, void* stream, float lr, float weight_decay, float grad_scale) {
  return optimizer_step(c, (hipStream_t)stream, lr, weight_decay, grad_scale);
}

// The plain eager step: Adam takes its bias-correction scalars by value (one launch less on the critical path).
int train_step_eager(eae_ctx* c, hipStream_t st, const eae_step_io* io, float lr) {
  RC(streams_distinct(c, st));
  int rc = forward_impl(c, st, io, true);
  if (!rc) rc = backward_impl(c, st, io);
  if (!rc) {
    c->adam_step += 1;               // (taken back when the launch fails: a failed step must not advance the bias correction)
    rc = launch_adam(c, st, c->arena_len(), lr, 0.f, 1.0f);
    if (rc) c->adam_step -= 1;
  }
  after_optimizer(c, rc);
  return rc;
}

// One iteration of the batch loop.  Steady state (same buffers, batch size and alpha as the previous calls, parameters
// last touched by this engine's own Adam): the whole step -- pack, forward, loss, backward on two streams, Adam -- is replayed
// from a captured hipGraph; the only per-step host work is one tiny launch that refreshes Adam's bias-correction scalars.
extern "C" int eae_ae_train_step(eae_ctx* c, void* stream, const eae_step_io* io, float lr) {
  RC(check_io(c, io, true));
  if (!c->M || !c->V) return eae_set_error(EAE_ERR_STATE, "adam: moment arenas must be bound");
  hipStream_t user = (hipStream_t)stream, st = user;
  const bool graph_ok = c->use_graph && (c->use_side || user != nullptr) && c->fold_fwd && c->fold_bwd && !c->prof_on && !c->packed && io->logits == nullptr && io->z == nullptr;
  if (graph_ok && user == nullptr) {      // legacy default stream: run on the engine's own stream, ordered by events
    st = c->own_main;
    EAE_HIP(hipEventRecord(c->ev_in, user));
    EAE_HIP(hipStreamWaitEvent(st, c->ev_in, 0));
  }
  struct Rejoin {                          // order the caller's stream after the step on every exit path
    eae_ctx* c; hipStream_t user, st;
    ~Rejoin() { if (st != user) { hipEventRecord(c->ev_out, st); hipStreamWaitEvent(user, c->ev_out, 0); } }
  } rejoin{c, user, st};
  eae_ctx::GraphEntry* ent = nullptr;
  if (graph_ok) {
    eae_ctx::GraphKey key{io->x, io->labels, io->x_hat, io->loss_accum, io->loss_last, io->B, io->head, io->alpha};
    for (int i = 0; i < c->ngraphs; ++i) if (c->graphs[i].key == key) ent = &c->graphs[i];
    if (!ent && c->ngraphs < eae_ctx::NGRAPH) { ent = &c->graphs[c->ngraphs++]; ent->key = key; }
    if (ent) ent->seen++;
  }
  if (!ent) return train_step_eager(c, st, io, lr);
  c->adam_step += 1;
  RC(eae_launch_set_dyn(st, c->dyn, lr, 0.9, 0.999, c->adam_step));
  if (ent && ent->exec) {
    EAE_HIP(hipGraphLaunch(ent->exec, st));
    invalidate_forward(c); c->packed = false; c->acc_clean = false;
    return 0;
  }
  const bool capture = ent && ent->seen >= 3;      // two eager warm-up steps with this key first (lazy kernel attributes etc.)
  if (capture) EAE_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
  c->capturing = capture;
  int rc = forward_impl(c, st, io, true);
  if (!rc) rc = backward_impl(c, st, io);
  if (!rc) rc = launch_adam(c, st, c->arena_len(), lr, 0.f, 1.0f, nullptr, nullptr, true);
  c->capturing = false;
  c->packed = false;
  if (capture) {
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(st, &g);
    if (rc) { if (g) hipGraphDestroy(g); return rc; }
    if (e != hipSuccess) return eae_set_error(EAE_ERR_HIP, hipGetErrorString(e));
    e = hipGraphInstantiate(&ent->exec, g, nullptr, nullptr, 0);
    if (e != hipSuccess) { hipGraphDestroy(g); ent->exec = nullptr; return eae_set_error(EAE_ERR_HIP, hipGetErrorString(e)); }
    ent->graph = g;
    EAE_HIP(hipGraphLaunch(ent->exec, st));
  }
  return rc;
}

extern "C" int eae_encoder_forward(eae_ctx* c, void* stream, const float* x, int B, int train, float* z) {
  if (!c || !x || !z) return eae_set_error(EAE_ERR_ARG, "encoder_forward: NULL argument");
  RC(check_bound_batch(c, B));
  hipStream_t st = (hipStream_t)stream;
  invalidate_forward(c);
  RC(ensure_packed(c, st));
  RC(prep_accumulators(c, st, train != 0));
  RC(run_encoder(c, st, x, B, train != 0));
  c->enc_ready = train ? 1 : 2; c->fwd_B = B; c->fwd_gen += 1;
  return copy_latent_out(c, st, z, c->z, B);
}

namespace {
int half_backward_checks(eae_ctx* c, int ready, long long generation) {
  if (!c || !c->G) return eae_set_error(EAE_ERR_STATE, "backward: no gradient arena bound");
  if (!ready) return eae_set_error(EAE_ERR_STATE, "backward: the matching stand-alone forward is not resident");
  if (generation != c->fwd_gen)
    return eae_set_error(EAE_ERR_STATE, "backward: a later forward has replaced the activations of the forward being differentiated");
  if (ready == 2 && !(c->fold_bwd && c->sync_world <= 1))
    return eae_set_error(EAE_ERR_STATE, "backward of an eval-mode forward needs the folded BatchNorm-backward finalize (no EAE_NO_FOLD_BWD, no SyncBN)");
  return 0;
}
}  // namespace

// Backward of a stand-alone Encoder (z = enc(x); ... ; z.backward(dz)): the encoder half of the gradient step for an externally supplied
// dL/dz [B][L].  x = the forward's input batch (conv1's weight gradient reads it), generation as for eae_ae_backward.
extern "C" int eae_encoder_backward(eae_ctx* c, void* stream, long long generation, const float* x, const float* dz) {
  RC(half_backward_checks(c, c ? c->enc_ready : 0, generation));
  if (!x || !dz) return eae_set_error(EAE_ERR_ARG, "encoder_backward: x and dz are required");
  hipStream_t st = (hipStream_t)stream;
  RC(copy_latent_in(c, st, c->dz, dz, c->fwd_B));
  eae_step_io io = eae_step_io();
  io.x = x; io.B = c->fwd_B; io.train = 1; io.head = 0;
  EvalBackward eb(c, c->enc_ready == 2);
  RC(prep_bwd_accumulators(c, st));            // (a stand-alone backward: backward_impl leaves part 2 alone)
  const int rc = backward_impl(c, st, &io, nullptr, 2);
  c->enc_ready = 0;
  return rc;
}

// Backward of a stand-alone Decoder (x_hat = dec(z); ... ; x_hat.backward(dx_hat)): decoder + dec.fc gradients and dL/dz -> dz_out [B][L].
extern "C" int eae_decoder_backward(eae_ctx* c, void* stream, long long generation, const float* x_hat, const float* dx_hat, float* dz_out) {
  RC(half_backward_checks(c, c ? c->dec_ready : 0, generation));
  if (!x_hat || !dx_hat) return eae_set_error(EAE_ERR_ARG, "decoder_backward: x_hat and dx_hat are required");
  hipStream_t st = (hipStream_t)stream;
  const int B = c->fwd_B;
  eae_step_io io = eae_step_io();
  io.B = B; io.train = 1; io.head = 0;
  RC(sigmoid_bwd_bias(st, x_hat, dx_hat, c->Cin, B, c->H, c->W, c->g4, c->grad(T_DECONV4_B), c->msepart));
  EvalBackward eb(c, c->dec_ready == 2);
  int rc = backward_impl(c, st, &io, nullptr, 1);
  c->dec_ready = 0;
  if (!rc) rc = join_side(c, st);
  if (!rc && dz_out) rc = copy_latent_out(c, st, dz_out, c->dz, B);
  return rc;
}

extern "C" int eae_decoder_forward(eae_ctx* c, void* stream, const float* z, int B, int train, float* x_hat) {
  if (!c || !x_hat || !z) return eae_set_error(EAE_ERR_ARG, "decoder_forward: NULL argument");
  RC(check_bound_batch(c, B));
  hipStream_t st = (hipStream_t)stream;
  invalidate_forward(c);
  RC(ensure_packed(c, st));
  RC(prep_accumulators(c, st, train != 0));
  RC(copy_latent_in(c, st, c->z, z, B));       // resident for the backward (dec.fc's weight gradient reads z again)
  RC(run_decoder(c, st, c->z, B, train != 0, nullptr, 0.f, x_hat, false, false));
  c->dec_ready = train ? 1 : 2; c->fwd_B = B; c->fwd_gen += 1;
  return 0;
}
