// C ABI of libeae.so (include/eae.h): error string, arena layout, creation and destruction of the context, binding, diagnostics.
#include "eae_ctx.h"
#include <string>
#include <cstring>
#include <cstdlib>

static thread_local std::string g_err;
int eae_set_error(int code, const char* msg) { g_err = msg ? msg : "unknown error"; return code; }
extern "C" const char* eae_last_error(void) { return g_err.c_str(); }
extern "C" int eae_version(void) { return 100; }

// fork/join events only order kernels of THIS device: no timing, and no system-scope fence when they complete (the agent-scope
// release at the end of every kernel is what makes its results visible to the other streams' kernels)
const unsigned EV_FLAGS = hipEventDisableTiming | (getenv("EAE_EVENT_SYSTEM_FENCE") ? 0u : hipEventDisableSystemFence);

namespace {

int bands_of(const eae_config& c) { return c.in_channels == 0 ? DEFAULT_BANDS : c.in_channels; }

void param_sizes(const eae_config& c, long long* sz) { eae_param_sizes(c.image_h, c.image_w, c.latent_dim, c.num_classes, bands_of(c), sz); }

int check_cfg(const eae_config* c) {
  if (!c) return eae_set_error(EAE_ERR_ARG, "config is NULL");
  if (c->image_h <= 0 || c->image_w <= 0 || c->image_h % 64 || c->image_w % 64) return eae_set_error(EAE_ERR_ARG, "image size must be a positive multiple of 64");
  if (c->latent_dim <= 0 || c->latent_dim > 256) return eae_set_error(EAE_ERR_ARG, "latent_dim must be in 1..256");
  if (c->num_classes <= 0 || c->num_classes > 64) return eae_set_error(EAE_ERR_ARG, "num_classes must be in 1..64");
  if (c->max_batch <= 0) return eae_set_error(EAE_ERR_ARG, "max_batch must be positive");
  if (c->quant != 0 && c->quant != 1) return eae_set_error(EAE_ERR_ARG, "quant must be 0 (bf16) or 1 (fp8 conv GEMMs)");
  if (c->in_channels < 0 || c->in_channels > 16) return eae_set_error(EAE_ERR_ARG, "in_channels must be in 1..16 (0 = 3)");
  if (c->quant == 1 && bands_of(*c) != 3) return eae_set_error(EAE_ERR_ARG, "quant=1 (fp8) supports in_channels = 3 only");
  if (c->quant == 1 && (c->image_h % 128 || c->image_w % 256))
    return eae_set_error(EAE_ERR_ARG, "quant=1: the fp8 kernels are built for 16 x 8 tiles on every map (image height % 128 == 0, width % 256 == 0)");
  return 0;
}

}  // namespace

extern "C" int eae_ae_layout(const eae_config* cfg, long long* param_off, long long* bn_off) {
  if (int rc = check_cfg(cfg)) return rc;
  long long sz[T_COUNT];
  param_sizes(*cfg, sz);
  long long o = 0;
  for (int i = 0; i < T_COUNT; ++i) { if (param_off) param_off[i] = o; o += r4(sz[i]); }
  if (param_off) param_off[T_COUNT] = o;
  o = 0;
  for (int l = 0; l < N_BN; ++l) {
    if (bn_off) { bn_off[2 * l] = o; bn_off[2 * l + 1] = o + BN_LAYERS[l].c; }
    o += 2 * BN_LAYERS[l].c;
  }
  if (bn_off) bn_off[2 * N_BN] = o;
  return 0;
}

extern "C" int eae_create(const eae_config* cfg, eae_ctx** out) {
  if (!out) return eae_set_error(EAE_ERR_ARG, "out is NULL");
  if (int rc = check_cfg(cfg)) return rc;
  eae_ctx* c = new eae_ctx();
  c->cfg = *cfg; c->H = cfg->image_h; c->W = cfg->image_w; c->L = cfg->latent_dim; c->C = cfg->num_classes; c->Bm = cfg->max_batch;
  c->Cin = bands_of(*cfg); c->CP = edge_cp(c->Cin);
  c->Lp = (c->L + 63) / 64 * 64; c->lpad = c->Lp != c->L;
  c->Pn = (long long)(c->H / 16) * (c->W / 16); c->K = FC_CHANNELS * c->Pn;
  eae_ae_layout(cfg, c->poff, c->bnoff);
  param_sizes(*cfg, c->psize);
  const long long Bm = c->Bm;
  // ---- carve one allocation
  size_t off = 0;
  auto carve = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  size_t o_y[4], o_u[3], o_gy[4], o_gu[3], o_dy[N_L3];
  for (int i = 0; i < 4; ++i) { o_y[i] = carve(Bm * c->act_elems(i + 1) * 2); o_gy[i] = carve(Bm * c->act_elems(i + 1) * 2); }
  for (int i = 0; i < 3; ++i) { o_u[i] = carve(Bm * c->act_elems(3 - i) * 2); o_gu[i] = carve(Bm * c->act_elems(3 - i) * 2); }
  const unsigned dy_mask_env = (getenv("EAE_DY_MASK") ? (unsigned)strtoul(getenv("EAE_DY_MASK"), nullptr, 0) : 0u) & 0x3cu;
  for (int j = 0; j < N_L3; ++j) o_dy[j] = ((dy_mask_env >> L3[j].dy_bit) & 1u) ? carve(Bm * c->act_elems(L3[j].out_lvl()) * 2) : 0;
  size_t o_d0 = carve(Bm * c->K * 2), o_gd0 = carve(Bm * c->K * 2), o_g4 = carve(Bm * (size_t)c->H * c->W * c->CP * 2);
  size_t o_z = carve(Bm * c->Lp * 4), o_dz = carve(Bm * c->Lp * 4), o_dzc = carve(Bm * c->Lp * 4);
  size_t o_cf[7], o_cb[7];
  for (int l = 0; l < 7; ++l) { o_cf[l] = carve(4 * BN_LAYERS[l].c * 4); o_cb[l] = carve(3 * BN_LAYERS[l].c * 4); }
  // statistics partials: the largest producer is conv1 / deconv4-backward (tiles x 2 x 32) or enc.fc backward (mtiles*P x 2 x 256)
  long long stat_floats = 0;
  {
    long long t1 = (long long)eae_edge_tiles((int)Bm, c->H, c->W) * 2 * 32;
    long long t2 = (long long)eae_conv_s2_ntiles(0, 32, 64, (int)Bm, c->H / 2, c->W / 2) * 2 * 64;
    long long t3 = ((Bm + 127) / 128) * c->Pn * 2 * 256;
    long long t4 = (long long)eae_conv_s2_ntiles(1, 64, 32, (int)Bm, c->H / 4, c->W / 4) * 2 * 32;
    long long t5 = (long long)eae_conv_s2_ntiles(1, 128, 64, (int)Bm, c->H / 8, c->W / 8) * 2 * 64 + (long long)Bm * 2 * 256;
    stat_floats = std::max(std::max(t1, t2), std::max(t3, std::max(t4, t5))) + 1024;
  }
  size_t o_stat = carve(stat_floats * 4);
  c->wscratch_floats = 6LL * 1024 * 1024;    // 24 MB of fp32 split-K partials
  size_t o_wscr = carve(c->wscratch_floats * 4), o_wscrx[eae_ctx::MAXX];
  {
    // Three side streams + the caller's stream = the GPU's four hardware queues (round 4: 0.4655 vs 0.4731 ms per B=512 step with two,
    // 0.505 with four -- five streams on four queues; c2 0.322 vs 0.326, config-5 shape unchanged).  Rounds 1-3 measured no gain from a
    // third one: its queue was whichever the runtime handed out, often the caller's (streams_distinct below now checks and repairs).
    // Grouped steps keep two (train.py: 0.596 vs 0.604 ms per group step), concurrent groups one each.
    const char* e = getenv("EAE_SIDE_STREAMS");
    int ns = e ? atoi(e) : 3;
    if (cfg->side_streams > 0) ns = cfg->side_streams;
    c->nx = ns < 1 ? 0 : (ns - 1 > eae_ctx::MAXX ? eae_ctx::MAXX : ns - 1);
  }
  for (int i = 0; i < c->nx; ++i) o_wscrx[i] = carve(c->wscratch_floats * 4);
  c->wscratch_main_floats = EAE_EDGE_WGRAD_SCRATCH_SLICES * eae_edge_wgrad_slice_floats(c->Cin);
  size_t o_wscrm = carve((size_t)c->wscratch_main_floats * 4);
  size_t o_acc[7], acc_total = 0;
  {
    const int Bi = (int)Bm;
    int nt[N_BN] = {eae_edge_tiles(Bi, c->H, c->W)};      // workgroups of the layer's forward producer: conv1, then the six 3x3 layers
    for (const Layer3& r : L3) nt[r.bn_out] = eae_conv_s2_ntiles(r.kind, r.cin, r.cout, Bi, c->H >> r.in_lvl(), c->W >> r.in_lvl());
    for (int l = 0; l < 7; ++l) {
      int cp = 8;
      while (cp < 64 && cp * 2 * 16 <= nt[l]) cp *= 2;        // about one accumulator set per 16 producer workgroups ...
      while (cp > BN_FOLD_K * (256 / BN_LAYERS[l].c)) cp /= 2;       // ... but at most BN_FOLD_K sets per consumer thread
      if (const char* e = getenv("EAE_ACC_COPIES_MAX")) { int mx = atoi(e); while (mx >= 1 && cp > mx) cp /= 2; }
      c->acc_copies[l] = cp;
      o_acc[l] = acc_total;
      acc_total += (size_t)cp * 2 * BN_LAYERS[l].c * 8 + (size_t)BN_LAYERS[l].c * 8;        // + the layer's [C] sticky non-finite flag words (BnAcc::flag)
    }
  }
  size_t o_accb = carve(2 * acc_total + 32);  // forward accumulators, then the backward ones (cleared together)   // conv1 weight gradient (last kernel of the backward, runs on the main stream)
  const int ksplit = (int)(c->K / EAE_FC_KLEN_MIN);      // the most slices eae_fc_klen can ask for
  size_t o_fcp = carve((size_t)ksplit * Bm * c->Lp * 4);
  size_t o_mse = carve(std::max((size_t)eae_edge_tiles((int)Bm, c->H, c->W), (size_t)((Bm * c->H * c->W + 255) / 256)) * edge_lp_stride(c->Cin) * 4);
  const long long hb = eae_head_blocks((int)Bm, 256);     // (the narrow-row variant of wide latents has the most blocks)
  c->head_stride = r4(128LL * c->Lp) + 128 + r4(128LL * c->C) + r4(c->C);
  size_t o_gsew = 0, o_gseb = 0, o_gsdw = 0, o_gsh = 0, o_zst = 0;
  if (c->lpad) {
    o_gsew = carve((size_t)c->Lp * c->K * 4); o_gseb = carve((size_t)c->Lp * 4); o_gsdw = carve((size_t)c->K * c->Lp * 4);
    o_gsh = carve((size_t)c->head_stride * 4); o_zst = carve(Bm * c->Lp * 4);
  }
  size_t o_ce = carve(hb * 2 * 4), o_head = carve(hb * c->head_stride * 4), o_loss = carve(64 * 4), o_dyn = carve(64), o_sig = carve(64);
  size_t o_clip = carve(EAE_CLIP_MAX_PARTS * sizeof(double));
  // ---- pack arena
  size_t poffb = 0;
  auto pcarve = [&](size_t bytes) { size_t o = poffb; poffb += (bytes + 255) & ~(size_t)255; return o; };
  std::vector<PackDesc> descs;
  auto add = [&](long long src, size_t dst, long long cnt, int mode, int d0, int d1, int d2, int f32) {
    PackDesc d; d.src_off = src; d.dst_off = (long long)dst; d.count = cnt; d.mode = mode; d.d0 = d0; d.d1 = d1; d.d2 = d2; d.out_f32 = f32;
    d.lv = d0; d.q_layer = -1;
    descs.push_back(d);
  };
  const int KP = (9 * c->CP + 31) / 32 * 32;      // conv1 / deconv4-backward pack [32][KP] (edge_conv_kernel)
  c->pk_c1 = pcarve(32 * KP * 2); add(c->poff[T_CONV1_W], c->pk_c1, 32 * KP, PACK_KCP, 32, c->Cin, c->CP, 0);
  for (int i = 0; i < N_L3; ++i) {
    const int cs = L3[i].cs(), cb = L3[i].cb();      // the weight is [cs][cb][3][3]
    const long long n = (long long)cs * cb * 9, src = c->poff[L3[i].w];
    c->pk_p1[i] = pcarve(n * 2); add(src, c->pk_p1[i], n, PACK_3x3_P1, cs, cb, 0, 0);
    c->pk_p2[i] = pcarve(n * 2); add(src, c->pk_p2[i], n, PACK_3x3_P2, cs, cb, 0, 0);
    if (cfg->quant == 1) {
      c->pk8_p1[i] = pcarve(n); add(src, c->pk8_p1[i], n, PACK_3x3_P1, cs, cb, 0, 0); descs.back().q_layer = i;
      c->pk8_p2[i] = pcarve(n); add(src, c->pk8_p2[i], n, PACK_3x3_P2, cs, cb, 0, 0); descs.back().q_layer = i;
    }
  }
  c->fp8 = cfg->quant == 1;
  c->pk_d4j = pcarve(4 * c->CP * 128 * 2); add(c->poff[T_DECONV4_W], c->pk_d4j, 4 * c->CP * 128, PACK_DECONV4_JOINT, 0, c->Cin, 0, 0);
  c->pk_d4k = pcarve(32 * KP * 2); add(c->poff[T_DECONV4_W], c->pk_d4k, 32 * KP, PACK_KCP, 32, c->Cin, c->CP, 0);
  const long long LK = c->Lp * c->K;      // d0 = padded latent width, lv = the real one (rows / columns beyond it are zero)
  c->pk_we1 = pcarve(LK * 2); add(c->poff[T_ENCFC_W], c->pk_we1, LK, PACK_FC_ROWMAJOR_KPERM, c->Lp, 256, (int)c->Pn, 0);
  c->pk_we2 = pcarve(LK * 2); add(c->poff[T_ENCFC_W], c->pk_we2, LK, PACK_FC_TRANS_KPERM, c->Lp, 256, (int)c->Pn, 0);
  c->pk_wd1 = pcarve(LK * 2); add(c->poff[T_DECFC_W], c->pk_wd1, LK, PACK_FC_ROWPERM, c->Lp, 256, (int)c->Pn, 0);
  c->pk_wd2 = pcarve(LK * 2); add(c->poff[T_DECFC_W], c->pk_wd2, LK, PACK_FC_ROWPERM_TRANS, c->Lp, 256, (int)c->Pn, 0);
  for (int k = 0; k < 4; ++k) descs[descs.size() - 1 - k].lv = c->L;
  if (c->lpad) {
    c->pk_w1p = pcarve(128LL * c->Lp * 4); add(c->poff[T_CLS0_W], c->pk_w1p, 128LL * c->Lp, PACK_PAD_COLS, c->Lp, 0, 0, 1); descs.back().lv = c->L;
    c->pk_bep = pcarve(c->Lp * 4); add(c->poff[T_ENCFC_B], c->pk_bep, c->Lp, PACK_PAD_COLS, c->Lp, 0, 0, 1); descs.back().lv = c->L;
  }
  c->pk_bd = pcarve(c->K * 4); add(c->poff[T_DECFC_B], c->pk_bd, c->K, PACK_FC_ROWPERM, 1, 256, (int)c->Pn, 1);
  c->ndesc = (int)descs.size();
  std::vector<unsigned short> blkmap(descs.size() * 1024);
  c->blk_tot = eae_pack_assign_blocks(descs.data(), (int)descs.size(), blkmap.data(), (int)blkmap.size());
  c->pack_bytes = poffb;
  size_t o_pack = carve(poffb), o_desc = carve(descs.size() * sizeof(PackDesc)), o_q = carve(sizeof(Fp8State)), o_bns = carve(2048 * 4 + 64);
  size_t o_bmap = carve((size_t)(c->blk_tot > 0 ? c->blk_tot : 1) * sizeof(unsigned short));
  hipError_t e = hipMalloc(&c->ws, off);
  if (e != hipSuccess) { delete c; return eae_set_error(EAE_ERR_HIP, hipGetErrorString(e)); }
  uint8_t* b = static_cast<uint8_t*>(c->ws);
  for (int i = 0; i < 4; ++i) { c->y[i] = (bf16_t*)(b + o_y[i]); c->gy[i] = (bf16_t*)(b + o_gy[i]); }
  for (int i = 0; i < 3; ++i) { c->u[i] = (bf16_t*)(b + o_u[i]); c->gu[i] = (bf16_t*)(b + o_gu[i]); }
  c->dyy[0] = nullptr;
  for (int j = 0; j < N_L3; ++j) c->dyact(L3[j].bn_out) = ((dy_mask_env >> L3[j].dy_bit) & 1u) ? (bf16_t*)(b + o_dy[j]) : nullptr;
  c->d0 = (bf16_t*)(b + o_d0); c->gd0 = (bf16_t*)(b + o_gd0); c->g4 = (bf16_t*)(b + o_g4);
  c->z = (float*)(b + o_z); c->dz = (float*)(b + o_dz); c->dzc = (float*)(b + o_dzc);
  if (c->lpad) {
    c->gs_encw = (float*)(b + o_gsew); c->gs_encb = (float*)(b + o_gseb); c->gs_decw = (float*)(b + o_gsdw);
    c->gs_head = (float*)(b + o_gsh); c->zstage = (float*)(b + o_zst);
  }
  for (int l = 0; l < 7; ++l) { c->coef_f[l] = (float*)(b + o_cf[l]); c->coef_b[l] = (float*)(b + o_cb[l]); }
  c->stat = (float*)(b + o_stat); c->wscratch = (float*)(b + o_wscr); c->wscratch_main = (float*)(b + o_wscrm);
  c->acc_base = b + o_accb; c->poison_off = (2 * acc_total + 15) & ~(size_t)15; c->acc_bytes = c->poison_off + 16; c->acc_half = acc_total;      // + the step-wide poison word
  for (int l = 0; l < 7; ++l) c->accf[l] = (unsigned long long*)(b + o_accb + o_acc[l]);
  for (int l = 0; l < 7; ++l) c->accb[l] = (unsigned long long*)(b + o_accb + acc_total + o_acc[l]);
  for (int i = 0; i < c->nx; ++i) c->wscratchx[i] = (float*)(b + o_wscrx[i]); c->fcpart = (float*)(b + o_fcp);
  c->msepart = (float*)(b + o_mse); c->cepart = (float*)(b + o_ce); c->headpart = (float*)(b + o_head); c->lossbuf = (float*)(b + o_loss);
  c->pack = b + o_pack; c->descs_dev = (PackDesc*)(b + o_desc); c->blkmap = (unsigned short*)(b + o_bmap);
  c->dyn = (float*)(b + o_dyn);
  c->clip_part = (double*)(b + o_clip);
  c->sigwords = (unsigned*)(b + o_sig);
  c->q = (Fp8State*)(b + o_q);
  c->bn_save = (float*)(b + o_bns);
  {
    Fp8State h;
    eae_fp8_state_init(&h);
    hipError_t eq = hipMemcpy(c->q, &h, sizeof(h), hipMemcpyHostToDevice);
    if (eq != hipSuccess) { hipFree(c->ws); delete c; return eae_set_error(EAE_ERR_HIP, hipGetErrorString(eq)); }
  }
  // Gate kernels need the kernel they wait for to be able to start while they spin.  rocprofv3's counter collection (--pmc) runs one
  // kernel at a time on the device: under it (ROCPROF_COUNTER_COLLECTION=1 in the environment) the hand-overs fall back to events.
  const char* rcc = getenv("ROCPROF_COUNTER_COLLECTION");
  c->use_gates = getenv("EAE_FORK_EVENTS") == nullptr && !(rcc && atoi(rcc) != 0);
  if (const char* gt = getenv("EAE_GATE_TIMEOUT_MS")) c->gate_limit = (unsigned long long)(atof(gt) * 1e5);
  // hipGraph replay is opt-in (EAE_GRAPH=1): on ROCm 7.2 the replayed graph ran its two branches one after the other
  // (0.80 ms/step) while the eager two-stream launch sequence overlaps them (0.71 ms/step)
  c->use_graph = getenv("EAE_GRAPH") != nullptr;
  e = hipMemcpy(c->descs_dev, descs.data(), descs.size() * sizeof(PackDesc), hipMemcpyHostToDevice);
  if (e == hipSuccess && c->blk_tot > 0) e = hipMemcpy(c->blkmap, blkmap.data(), (size_t)c->blk_tot * sizeof(unsigned short), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(c->g4, 0, Bm * (size_t)c->H * c->W * c->CP * 2);
  if (e == hipSuccess && c->lpad) e = hipMemset(c->zstage, 0, Bm * (size_t)c->Lp * 4);
  if (e == hipSuccess) e = hipMemset(c->z, 0, Bm * (size_t)c->Lp * 4);
  if (e == hipSuccess) e = hipMemset(c->dz, 0, Bm * (size_t)c->Lp * 4);
  if (e == hipSuccess) e = hipMemset(c->acc_base, 0, c->acc_bytes);
  if (e == hipSuccess) e = hipMemset(c->sigwords, 0, 64);
  c->acc_clean = true; c->bwd_dirty = false;
  // Default OFF (round 4, measured): with dy the weight-gradient kernels lose a third of their stand-alone time (31-35 -> 27-32 us),
  // but they start one kernel later and the backward-data kernels -- the critical chain -- carry the extra stores: ms per step at
  // B=512 with dy for no layer / conv3+conv4 / deconv1+deconv2 / all four: 0.4840 / 0.4833 / 0.4861 / 0.4933.  The 32 <-> 64-channel
  // layers' backward-data kernels are built without the store (eae_igemm.hip.h: DY), so bits 1 and 6 are never honoured.
  c->dy_mask = (getenv("EAE_DY_MASK") ? (unsigned)strtoul(getenv("EAE_DY_MASK"), nullptr, 0) : 0u) & 0x3cu;
  c->skip_wgrad = getenv("EAE_SKIP_WGRAD") != nullptr;
  c->nan_exact = (getenv("EAE_NAN_EXACT") && atoi(getenv("EAE_NAN_EXACT")) != 0) ? 1 : 0;
  c->fold_fwd = getenv("EAE_NO_FOLD_FWD") == nullptr;
  c->fold_bwd = getenv("EAE_NO_FOLD_BWD") == nullptr;
  if (e != hipSuccess) { hipFree(c->ws); delete c; return eae_set_error(EAE_ERR_HIP, hipGetErrorString(e)); }
  c->use_side = getenv("EAE_NO_SIDE_STREAM") == nullptr && cfg->side_streams >= 0;
  if (c->use_side) {
    // (priority 0 like the caller's stream: a lower one was measured and removed)
    e = hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, 0);
    for (int i = 0; i < c->nx && e == hipSuccess; ++i) {
      e = hipStreamCreateWithPriority(&c->sidex[i], hipStreamNonBlocking, 0);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_joinx[i], EV_FLAGS);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_sx[i], EV_FLAGS);
    }
    for (int i = 0; i < eae_ctx::NEV && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&c->ev_fork[i], EV_FLAGS);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_join, EV_FLAGS);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_head, EV_FLAGS);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->own_main, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_in, EV_FLAGS);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_out, EV_FLAGS);
    if (e != hipSuccess) { hipFree(c->ws); delete c; return eae_set_error(EAE_ERR_HIP, hipGetErrorString(e)); }
  }
  *out = c;
  return 0;
}

// diagnostic: copy an internal fp32 workspace buffer to `dst` (0 = z, 1 = dz, 2 = dzc, 3 = headpart, 4 = cepart)
extern "C" int eae_debug_copy(eae_ctx* c, int which, float* dst, long long n) {
  if (!c || !dst) return eae_set_error(EAE_ERR_ARG, "debug_copy: NULL");
  const float* src = which == 0 ? c->z : which == 1 ? c->dz : which == 2 ? c->dzc : which == 3 ? c->headpart : c->cepart;
  EAE_HIP(hipDeviceSynchronize());
  EAE_HIP(hipMemcpy(dst, src, (size_t)n * 4, hipMemcpyDeviceToDevice));
  return 0;
}

extern "C" int eae_profile_enable(eae_ctx* c, int site) {
  if (!c) return eae_set_error(EAE_ERR_ARG, "ctx is NULL");
  if (site < 0 || site >= EAE_PROF_NSITES) return eae_set_error(EAE_ERR_ARG, "profile: unknown launch site");
  if (site && !c->prof_ev[0])
    for (int i = 0; i < 3 * eae_ctx::PROF_RING; ++i) EAE_HIP(hipEventCreate(&c->prof_ev[i]));
  c->prof_on = site != 0;
  c->prof_site = site;
  c->prof_n = 0;
  return 0;
}

extern "C" int eae_profile_read2(eae_ctx* c, double* total_ms, double* empty_ms, long long* count) {
  if (!c || !total_ms || !count) return eae_set_error(EAE_ERR_ARG, "profile_read: NULL argument");
  double tot = 0.0, emp = 0.0;
  for (int i = 0; i < c->prof_n; ++i) {
    float ms = 0.f;
    EAE_HIP(hipEventSynchronize(c->prof_ev[3 * i + 2]));
    EAE_HIP(hipEventElapsedTime(&ms, c->prof_ev[3 * i], c->prof_ev[3 * i + 1]));
    tot += ms;
    EAE_HIP(hipEventElapsedTime(&ms, c->prof_ev[3 * i + 1], c->prof_ev[3 * i + 2]));
    emp += ms;
  }
  *total_ms = tot; *count = c->prof_n;
  if (empty_ms) *empty_ms = emp;
  c->prof_n = 0;
  return 0;
}
extern "C" int eae_profile_read(eae_ctx* c, double* total_ms, long long* count) { return eae_profile_read2(c, total_ms, nullptr, count); }

static int drop_graphs(eae_ctx* c, bool drain);
extern "C" int eae_destroy(eae_ctx* c) {
  if (!c) return 0;
  hipDeviceSynchronize();
  streams_forget(c);
  eae_dp_destroy(c);
  if (c->prof_ev[0]) for (int i = 0; i < 3 * eae_ctx::PROF_RING; ++i) hipEventDestroy(c->prof_ev[i]);
  drop_graphs(c, false);           // (the device has drained above)
  if (c->side) {
    for (int i = 0; i < eae_ctx::NEV; ++i) hipEventDestroy(c->ev_fork[i]);
    hipEventDestroy(c->ev_join);
    if (c->ev_head) hipEventDestroy(c->ev_head);
    hipStreamDestroy(c->side);
    for (int i = 0; i < 2; ++i) if (c->dp_stream[i]) { hipStreamDestroy(c->dp_stream[i]); hipEventDestroy(c->ev_part[i]); }
    for (int i = 0; i < c->nx; ++i)
      if (c->sidex[i]) { hipStreamDestroy(c->sidex[i]); hipEventDestroy(c->ev_joinx[i]); hipEventDestroy(c->ev_sx[i]); }
    if (c->own_main) { hipStreamDestroy(c->own_main); hipEventDestroy(c->ev_in); hipEventDestroy(c->ev_out); }
  }
  if (c->ws) hipFree(c->ws);
  delete c;
  return 0;
}

extern "C" int eae_bind(eae_ctx* c, float* params, float* grads, float* adam_m, float* adam_v, float* bn_running, long long* bn_nbt) {
  if (!c || !params || !bn_running) return eae_set_error(EAE_ERR_ARG, "bind: ctx, params and bn_running are required");
  c->P = params; c->G = grads; c->M = adam_m; c->V = adam_v; c->bnrun = bn_running; c->nbt = bn_nbt;
  c->packed = false; invalidate_forward(c);
  if (grads)
    for (int l = 0; l < N_BN; ++l) EAE_HIP(hipMemset(c->prebn_dbias(l), 0, (size_t)c->numel(BN_LAYERS[l].bias) * 4));
  return 0;
}
// Synchronized BatchNorm (new work, SURVEY.md 8e "Equivalence to test": R ranks x B/R with SyncBN == 1 rank x B).
extern "C" long long eae_sync_bn_acc_elems(eae_ctx* c) { return c ? (long long)(c->acc_bytes / 8) : -1; }
extern "C" int eae_set_sync_bn(eae_ctx* c, int world, eae_sync_fn fn, void* user, void* acc_i64, void* sums_f64) {
  if (!c) return eae_set_error(EAE_ERR_ARG, "ctx is NULL");
  if (world <= 1 || !fn) { c->sync_world = 1; c->sync_fn = nullptr; return 0; }
  if (!acc_i64 || !sums_f64) return eae_set_error(EAE_ERR_ARG, "sync_bn: the accumulator and sums buffers are required");
  if (!c->fold_fwd) return eae_set_error(EAE_ERR_STATE, "SyncBN needs the folded forward finalize (unset EAE_NO_FOLD_FWD)");
  // the forward accumulators move into the caller's buffer (same layout), so that the hook can hand tensor views of it to the collective
  uint8_t* nb = static_cast<uint8_t*>(acc_i64);
  for (int l = 0; l < 7; ++l) {
    c->accf[l] = reinterpret_cast<unsigned long long*>(nb + (reinterpret_cast<uint8_t*>(c->accf[l]) - c->acc_base));
    c->accb[l] = reinterpret_cast<unsigned long long*>(nb + (reinterpret_cast<uint8_t*>(c->accb[l]) - c->acc_base));
  }
  c->acc_base = nb;
  c->acc_clean = false;
  c->sync_world = world; c->sync_fn = fn; c->sync_user = user; c->sync_sums = static_cast<double*>(sums_f64);
  return 0;
}
// Diagnostic (synchronises the device): 0, or the progress value a gate kernel gave up waiting for after its bounded spin
// (include/eae.h); the step in which that happened produced wrong gradients.
// Clear the sticky time-out word (after the caller has dealt with the failed step); synchronises the device.
extern "C" int eae_gate_timeouts_clear(eae_ctx* c) {
  if (!c) return eae_set_error(EAE_ERR_ARG, "ctx is NULL");
  EAE_HIP(hipDeviceSynchronize());
  EAE_HIP(hipMemset(c->sigwords + 8, 0, 4));
  return 0;
}
// The same word WITHOUT synchronising the device: for callers that have just synchronised the stream they step on (every gate of
// a completed step has run by then) and share the device with other contexts -- the concurrent grid driver (train.py) must not
// stall every configuration at each epoch end of one of them.
extern "C" long long eae_gate_timeouts_nosync(eae_ctx* c) {
  if (!c) return -1;
  unsigned v = 0;
  if (hipMemcpy(&v, c->sigwords + 8, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (long long)v;
}
extern "C" long long eae_gate_timeouts(eae_ctx* c) {
  if (!c) return -1;
  unsigned v = 0;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy(&v, c->sigwords + 8, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (long long)v;
}
// hipGraph replay of eae_ae_train_step on/off for this context (default: the EAE_GRAPH environment switch at creation).  One replay per
// step instead of ~70 launches: the single-configuration step at B=512 is faster eager, but K small configurations
// stepped concurrently from K host threads are bound by the host's launch rate -- there the replay wins (train.run_concurrent).
extern "C" int eae_set_graph(eae_ctx* c, int on) {
  if (!c) return eae_set_error(EAE_ERR_ARG, "ctx is NULL");
  c->use_graph = on != 0;
  return 0;
}
// A captured step graph holds the head kernel and the pointers of the setting it was captured under: dropped (after the device has
// drained: one may be in flight) whenever the setting changes; the next steps capture again.
static int drop_graphs(eae_ctx* c, bool drain) {
  if (!c->ngraphs) return 0;
  if (drain) EAE_HIP(hipDeviceSynchronize());
  for (int i = 0; i < c->ngraphs; ++i) {
    if (c->graphs[i].exec) EAE_HIP(hipGraphExecDestroy(c->graphs[i].exec));
    if (c->graphs[i].graph) EAE_HIP(hipGraphDestroy(c->graphs[i].graph));
    c->graphs[i] = eae_ctx::GraphEntry();
  }
  c->ngraphs = 0;
  return 0;
}
// Class weights / ignore_index of the fused CrossEntropyLoss (include/eae.h).
extern "C" int eae_set_class_weights(eae_ctx* c, const float* weights, long long ignore_index) {
  if (!c) return eae_set_error(EAE_ERR_ARG, "ctx is NULL");
  if (c->capturing) return eae_set_error(EAE_ERR_STATE, "set_class_weights: a step is being captured");
  RC(drop_graphs(c, true));
  c->class_w = weights; c->ignore_index = ignore_index;
  return 0;
}
// Global gradient-norm clipping in front of every optimizer launch (include/eae.h).
extern "C" int eae_set_grad_clip(eae_ctx* c, float max_norm, float* norm_out) {
  if (!c) return eae_set_error(EAE_ERR_ARG, "ctx is NULL");
  if (!(max_norm >= 0.f)) return eae_set_error(EAE_ERR_ARG, "set_grad_clip: max_norm must be 0 (off), positive or +inf");
  if (c->capturing) return eae_set_error(EAE_ERR_STATE, "set_grad_clip: a step is being captured");
  RC(drop_graphs(c, true));
  c->clip_max = max_norm; c->clip_out = max_norm != 0.f ? norm_out : nullptr;
  return 0;
}
extern "C" int eae_set_valid_counter(eae_ctx* c, long long* counter) {
  if (!c) return eae_set_error(EAE_ERR_ARG, "ctx is NULL");
  if (c->capturing) return eae_set_error(EAE_ERR_STATE, "set_valid_counter: a step is being captured");
  RC(drop_graphs(c, true));
  c->valid_acc = counter;
  return 0;
}
extern "C" int eae_params_changed(eae_ctx* c) { if (!c) return eae_set_error(EAE_ERR_ARG, "ctx is NULL"); c->packed = false; invalidate_forward(c); return 0; }
extern "C" int eae_set_adam_step(eae_ctx* c, long long s) { if (!c) return eae_set_error(EAE_ERR_ARG, "ctx is NULL"); c->adam_step = s; return 0; }
extern "C" long long eae_get_adam_step(eae_ctx* c) { return c ? c->adam_step : -1; }
// Test / diagnostic access to the engine's workspace tensors of the most recent step (device synchronised first; bf16 NHWC, sized
// for the context's max_batch): kind 0 = y[idx] (idx 0..3), 1 = gy[idx], 2 = u[idx] (0..2), 3 = gu[idx], 4 = dyy[idx] (1..3), 5 = dyu[idx].
// Copies up to `bytes` to `host_dst`, returns the number of bytes copied or a negative status.
// kind 6 (EAE_DEBUG_PACK) = one pack of the pack arena, idx in the enumeration of include/eae.h: returns the pack's full length.
namespace {
// offset and length in bytes of pack `idx` inside the pack arena; 0 = found, else the status to return
int pack_entry(eae_ctx* c, int idx, size_t* off, long long* len) {
  const long long KP = (9 * c->CP + 31) / 32 * 32, LK = (long long)c->Lp * c->K;
  if (idx == EAE_PACK_CONV1) { *off = c->pk_c1; *len = 32 * KP * 2; return 0; }
  if (idx >= EAE_PACK_P1 && idx < EAE_PACK_P1 + 12) {
    const int i = (idx - EAE_PACK_P1) % 6;
    *off = idx < EAE_PACK_P2 ? c->pk_p1[i] : c->pk_p2[i]; *len = (long long)L3[i].cin * L3[i].cout * 9 * 2; return 0;
  }
  if (idx == EAE_PACK_DECONV4_JOINT) { *off = c->pk_d4j; *len = 4LL * c->CP * 128 * 2; return 0; }
  if (idx == EAE_PACK_DECONV4_KCP) { *off = c->pk_d4k; *len = 32 * KP * 2; return 0; }
  if (idx >= EAE_PACK_WE1 && idx <= EAE_PACK_WD2) {
    *off = idx == EAE_PACK_WE1 ? c->pk_we1 : idx == EAE_PACK_WE2 ? c->pk_we2 : idx == EAE_PACK_WD1 ? c->pk_wd1 : c->pk_wd2; *len = LK * 2; return 0;
  }
  if (idx == EAE_PACK_W1P || idx == EAE_PACK_BEP) {
    if (!c->lpad) return eae_set_error(EAE_ERR_STATE, "debug_read: w1p / bep exist only with latent padding (latent_dim % 64 != 0)");
    *off = idx == EAE_PACK_W1P ? c->pk_w1p : c->pk_bep; *len = (idx == EAE_PACK_W1P ? 128LL : 1LL) * c->Lp * 4; return 0;
  }
  if (idx == EAE_PACK_BD) { *off = c->pk_bd; *len = c->K * 4; return 0; }
  if (idx >= EAE_PACK_FP8_P1 && idx < EAE_PACK_FP8_P1 + 12) {
    if (!c->fp8) return eae_set_error(EAE_ERR_STATE, "debug_read: the fp8 packs exist only with quant = 1");
    const int i = (idx - EAE_PACK_FP8_P1) % 6;
    *off = idx < EAE_PACK_FP8_P2 ? c->pk8_p1[i] : c->pk8_p2[i]; *len = (long long)L3[i].cin * L3[i].cout * 9; return 0;
  }
  return eae_set_error(EAE_ERR_ARG, "debug_read: no such pack");
}
}  // namespace
extern "C" long long eae_debug_read(eae_ctx* c, int kind, int idx, void* host_dst, long long bytes) {
  if (c && kind == EAE_DEBUG_PACK) {
    size_t off = 0; long long have = 0;
    if (int rc = pack_entry(c, idx, &off, &have)) return rc;
    if (bytes > have) bytes = have;
    if (bytes > 0 && !host_dst) return eae_set_error(EAE_ERR_ARG, "debug_read: null argument");
    EAE_HIP(hipDeviceSynchronize());
    if (bytes > 0) EAE_HIP(hipMemcpy(host_dst, c->pack + off, (size_t)bytes, hipMemcpyDeviceToHost));
    return have;
  }
  if (!c || !host_dst) return eae_set_error(EAE_ERR_ARG, "debug_read: null argument");
  const bool enc = kind == 0 || kind == 1 || kind == 4;
  if (kind < 0 || kind > 5 || idx < 0 || idx > (enc ? 3 : 2) || (kind == 4 && idx == 0)) return eae_set_error(EAE_ERR_ARG, "debug_read: no such tensor");
  const bf16_t* p = kind == 0 ? c->y[idx] : kind == 1 ? c->gy[idx] : kind == 2 ? c->u[idx] : kind == 3 ? c->gu[idx] : kind == 4 ? c->dyy[idx] : c->dyu[idx];
  if (!p) return eae_set_error(EAE_ERR_STATE, "debug_read: this context keeps no dy tensor for that layer (EAE_DY_MASK)");
  const long long have = (long long)c->Bm * c->act_elems(enc ? idx + 1 : 3 - idx) * 2;
  if (bytes > have) bytes = have;
  EAE_HIP(hipDeviceSynchronize());
  EAE_HIP(hipMemcpy(host_dst, p, (size_t)bytes, hipMemcpyDeviceToHost));
  return bytes;
}
// Test / diagnostic: set every byte of the pack arena and mark the packs stale, so that the next forward packs again (synchronises)
extern "C" int eae_debug_fill_packs(eae_ctx* c, int byte) {
  if (!c) return eae_set_error(EAE_ERR_ARG, "ctx is NULL");
  EAE_HIP(hipDeviceSynchronize());
  EAE_HIP(hipMemset(c->pack, byte & 0xff, c->pack_bytes));
  EAE_HIP(hipDeviceSynchronize());
  c->packed = false; invalidate_forward(c);
  return 0;
}
extern "C" int eae_set_halves(eae_ctx* c, int encoder, int decoder) {
  if (!c) return eae_set_error(EAE_ERR_ARG, "set_halves: NULL context");
  c->has_enc = encoder != 0; c->has_dec = decoder != 0;
  return 0;
}
