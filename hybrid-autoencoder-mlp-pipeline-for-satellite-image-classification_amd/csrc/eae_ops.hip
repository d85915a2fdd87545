// Thin per-op wrappers over the launchers, used by the kernel-level parity tests.
#include "eae_ctx.h"
#include "eae_stage.h"

namespace {
SrcDesc to_src(const eae_src& s) {
  SrcDesc d; d.p0 = (const bf16_t*)s.p0; d.p1 = (const bf16_t*)s.p1; d.coef = s.coef; return d;
}
}  // namespace

#ifdef EAE_STAMPS
static unsigned long long* g_dbg = nullptr; static int g_dbg_block = 0;
extern "C" int eae_debug_set(void* p, int block) { g_dbg = (unsigned long long*)p; g_dbg_block = block; return 0; }
#endif
static int op_conv_s2(void* stream, int kind, eae_src src, int cin, int cout, int B, int Hin, int Win, const void* wpack, const float* bias,
                      void* out, float* stat_part, int epilogue, const void* yprev, const float* prev_coef, const float* qs, unsigned* amax,
                      int amax_slots = 1, int amax_stride = 0) {
  ConvArgs a = ConvArgs();
  a.src = to_src(src); a.wpack = (const bf16_t*)wpack; a.bias = bias; a.out = (bf16_t*)out; a.stat_part = stat_part;
  a.yprev = (const bf16_t*)yprev; a.prev_coef = prev_coef; a.B = B; a.Hin = Hin; a.Win = Win;
  a.qs = qs; a.amax = amax; a.amax_mask = amax_slots - 1; a.amax_stride = amax_stride;
#ifdef EAE_STAMPS
  if (!qs) { a.dbg = g_dbg; a.dbg_block = g_dbg_block; }
#endif
  if (kind == 0) return eae_launch_conv_s2(a, cin, cout, src.mode, epilogue, (hipStream_t)stream);
  return eae_launch_deconv_s2(a, cin, cout, src.mode, epilogue, (hipStream_t)stream);
}
extern "C" int eae_op_conv_s2(void* stream, int kind, eae_src src, int cin, int cout, int B, int Hin, int Win, const void* wpack,
                              const float* bias, void* out, float* stat_part, int epilogue, const void* yprev, const float* prev_coef) {
  return op_conv_s2(stream, kind, src, cin, cout, B, Hin, Win, wpack, bias, out, stat_part, epilogue, yprev, prev_coef, nullptr, nullptr);
}
extern "C" int eae_op_conv_s2_ntiles(int kind, int cin, int B, int Hin, int Win) {
  return eae_conv_s2_ntiles(kind, cin, kind == 0 ? 2 * cin : cin / 2, B, Hin, Win);     // every instantiated conv layer doubles the channels, every transposed one halves them
}
// fp8 variant of the same op (16 x 8-tileable maps only): wpack = e4m3 bytes [cout][9][cin] of w * s_w;  qs (device) = {1/s_pixel,
// 1/(s_pixel * s_w)};  amax (device, may be NULL) receives max |staged pixel operand| as float bits (atomicMax)
extern "C" int eae_op_conv_s2_fp8(void* stream, int kind, eae_src src, int cin, int cout, int B, int Hin, int Win, const void* wpack_e4m3,
                                  const float* bias, void* out, float* stat_part, int epilogue, const void* yprev, const float* prev_coef,
                                  const float* qs, unsigned* amax) {
  if (!qs) return eae_set_error(EAE_ERR_ARG, "conv_s2_fp8: qs is NULL");
  return op_conv_s2(stream, kind, src, cin, cout, B, Hin, Win, wpack_e4m3, bias, out, stat_part, epilogue, yprev, prev_coef, qs, amax);
}
// the same op reporting into amax_slots words (a power of two) amax_stride words apart, as the engine's launches do: workgroup
// tile t reports into word (t & (amax_slots - 1)) * amax_stride
extern "C" int eae_op_conv_s2_fp8_slots(void* stream, int kind, eae_src src, int cin, int cout, int B, int Hin, int Win, const void* wpack_e4m3,
                                        const float* bias, void* out, float* stat_part, int epilogue, const void* yprev, const float* prev_coef,
                                        const float* qs, unsigned* amax, int amax_slots, int amax_stride) {
  if (!qs || !amax) return eae_set_error(EAE_ERR_ARG, "conv_s2_fp8_slots: qs or amax is NULL");
  if (amax_slots < 1 || (amax_slots & (amax_slots - 1)) || amax_stride < (amax_slots > 1 ? 1 : 0))
    return eae_set_error(EAE_ERR_ARG, "conv_s2_fp8_slots: amax_slots must be a power of two and amax_stride positive");
  return op_conv_s2(stream, kind, src, cin, cout, B, Hin, Win, wpack_e4m3, bias, out, stat_part, epilogue, yprev, prev_coef, qs, amax,
                    amax_slots, amax_stride);
}
// fp8_scales_kernel on a state built for the call: amax_bits [3][6][FP8_AMAX_SLOTS] (act, grad, w; slot s of a row sits at word
// s * FP8_AMAX_STRIDE of the state's row, every other word is 0), scales_in [18] = s_act, s_grad, s_w.  One launch, then the state
// comes back: scales_out [18], qs_out [6][8] = qs_fwd[2], qs_bwd[2], qs_wg[4] per layer, amax_left = the slot words after the
// launch.  Every pointer is host memory; synchronises the stream.
extern "C" int eae_op_fp8_scales(void* stream, const unsigned* amax_bits, const float* scales_in, float* scales_out, float* qs_out,
                                 unsigned* amax_left) {
  if (!amax_bits || !scales_in || !scales_out || !qs_out || !amax_left) return eae_set_error(EAE_ERR_ARG, "fp8_scales: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  Fp8State* h = new Fp8State;
  eae_fp8_state_init(h);
  unsigned (*rows[3])[FP8_AMAX_SLOTS * FP8_AMAX_STRIDE] = {h->amax_act, h->amax_grad, h->amax_w};
  float* sc[3] = {h->s_act, h->s_grad, h->s_w};
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 6; ++i) {
      sc[k][i] = scales_in[k * 6 + i];
      for (int s = 0; s < FP8_AMAX_SLOTS; ++s) rows[k][i][s * FP8_AMAX_STRIDE] = amax_bits[(k * 6 + i) * FP8_AMAX_SLOTS + s];
    }
  Fp8State* dev = nullptr;
  hipError_t e = hipMalloc(&dev, sizeof(Fp8State));
  if (e != hipSuccess) { delete h; return eae_set_error(EAE_ERR_HIP, hipGetErrorString(e)); }
  int rc = 0;
  e = hipMemcpyAsync(dev, h, sizeof(Fp8State), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);          // (pageable source: the copy must be done before h is written again)
  if (e == hipSuccess) rc = eae_launch_fp8_scales(st, dev);
  if (e == hipSuccess && rc == 0) e = hipMemcpyAsync(h, dev, sizeof(Fp8State), hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);
  hipFree(dev);
  if (e == hipSuccess && rc == 0 && es == hipSuccess) {
    for (int k = 0; k < 3; ++k)
      for (int i = 0; i < 6; ++i) {
        scales_out[k * 6 + i] = sc[k][i];
        for (int s = 0; s < FP8_AMAX_SLOTS; ++s) amax_left[(k * 6 + i) * FP8_AMAX_SLOTS + s] = rows[k][i][s * FP8_AMAX_STRIDE];
      }
    for (int i = 0; i < 6; ++i) {
      float* q = qs_out + i * 8;
      q[0] = h->qs_fwd[i][0]; q[1] = h->qs_fwd[i][1]; q[2] = h->qs_bwd[i][0]; q[3] = h->qs_bwd[i][1];
      for (int j = 0; j < 4; ++j) q[4 + j] = h->qs_wg[i][j];
    }
  }
  delete h;
  if (e != hipSuccess) return eae_set_error(EAE_ERR_HIP, hipGetErrorString(e));
  if (rc) return rc;
  if (es != hipSuccess) return eae_set_error(EAE_ERR_HIP, hipGetErrorString(es));
  return 0;
}

// C-band forms of the four edge ops (in_channels 1..16), and the 3-band forms: these at C = 3
extern "C" int eae_op_edge_conv_c(void* stream, int src_kind, const void* src, int C, int B, int H, int W, const void* wpack,
                                  const float* bias, void* out, float* stat_part, int epilogue, const void* yprev, const float* prev_coef) {
  EdgeArgs a;
  a.src3 = src; a.B = B; a.H = H; a.W = W; a.C = C;
  a.c = ConvArgs();
  a.c.wpack = (const bf16_t*)wpack; a.c.bias = bias; a.c.out = (bf16_t*)out; a.c.stat_part = stat_part;
  a.c.yprev = (const bf16_t*)yprev; a.c.prev_coef = prev_coef; a.c.B = B;
  return eae_launch_edge_conv((hipStream_t)stream, src_kind, epilogue, a);
}
extern "C" int eae_op_edge_wgrad_c(void* stream, int src_kind, const void* src, int C, int B, int H, int W, eae_src side, float* scratch,
                                   long long scratch_floats, float* dw) {
  return eae_launch_edge_wgrad((hipStream_t)stream, src_kind, src, B, H, W, to_src(side), side.mode, scratch, scratch_floats, dw,
                               nullptr, nullptr, nullptr, 0, nullptr, nullptr, C);
}
extern "C" int eae_op_deconv4_loss_c(void* stream, eae_src a3, int C, int B, int Hin, int Win, const void* wjoint, const float* bias,
                                     const float* x, float gscale, float* x_hat, void* g, float* loss_part) {
  Deconv4Args d = Deconv4Args();
  d.src = to_src(a3); d.wjoint = (const bf16_t*)wjoint; d.bias = bias; d.x = x; d.x_hat = x_hat; d.g4 = (bf16_t*)g;
  d.loss_part = loss_part; d.gscale = gscale; d.B = B; d.Hin = Hin; d.Win = Win; d.C = C;
  return eae_launch_deconv4_loss((hipStream_t)stream, a3.mode, d);
}
extern "C" int eae_op_sigmoid_bwd_c(void* stream, const float* x_hat, const float* dx_hat, int C, int B, int H, int W, void* g, float* db,
                                    float* scratch) {
  return sigmoid_bwd_bias((hipStream_t)stream, x_hat, dx_hat, C, B, H, W, g, db, scratch);
}
extern "C" int eae_op_edge_conv(void* stream, int src3_kind, const void* src3, int B, int H, int W, const void* wpack, const float* bias,
                                void* out, float* stat_part, int epilogue, const void* yprev, const float* prev_coef) {
  return eae_op_edge_conv_c(stream, src3_kind, src3, 3, B, H, W, wpack, bias, out, stat_part, epilogue, yprev, prev_coef);
}
extern "C" int eae_op_edge_wgrad(void* stream, int src3_kind, const void* src3, int B, int H, int W, eae_src side, float* scratch,
                                 long long scratch_floats, float* dw) {
  return eae_op_edge_wgrad_c(stream, src3_kind, src3, 3, B, H, W, side, scratch, scratch_floats, dw);
}
extern "C" int eae_op_deconv4_loss(void* stream, eae_src a3, int B, int Hin, int Win, const void* wjoint, const float* bias,
                                   const float* x, float gscale, float* x_hat, void* g4, float* loss_part) {
  return eae_op_deconv4_loss_c(stream, a3, 3, B, Hin, Win, wjoint, bias, x, gscale, x_hat, g4, loss_part);
}
extern "C" int eae_op_sigmoid_bwd(void* stream, const float* x_hat, const float* dx_hat, int B, int H, int W, void* g4, float* db,
                                  float* scratch) {
  return eae_op_sigmoid_bwd_c(stream, x_hat, dx_hat, 3, B, H, W, g4, db, scratch);
}
extern "C" int eae_op_pack_edge(void* stream, const float* w, int C, void* wpack, void* wjoint) {
  // the engine's own conv1 / deconv4 pack descriptors (eae_create) in a two-entry table allocated for the call; synchronises its stream
  if (C < 1 || C > 16) return eae_set_error(EAE_ERR_ARG, "pack_edge: in_channels must be in 1..16");
  if (!w || !wpack) return eae_set_error(EAE_ERR_ARG, "pack_edge: w and wpack are required");
  const int CP = edge_cp(C), KP = (9 * CP + 31) / 32 * 32;
  PackDesc d[2];
  d[0] = PackDesc{0, 0, 32LL * KP, PACK_KCP, 32, C, CP, 0, 0, -1};
  d[1] = PackDesc{0, wjoint ? (long long)((char*)wjoint - (char*)wpack) : 0, 4LL * CP * 128, PACK_DECONV4_JOINT, 0, C, 0, 0, 0, -1};
  PackDesc* dev = nullptr;
  EAE_HIP(hipMalloc(&dev, sizeof(d)));
  hipError_t e = hipMemcpyAsync(dev, d, sizeof(d), hipMemcpyHostToDevice, (hipStream_t)stream);
  int rc = e == hipSuccess ? eae_launch_pack_all((hipStream_t)stream, dev, wjoint ? 2 : 1, w, wpack) : 0;
  const hipError_t es = hipStreamSynchronize((hipStream_t)stream);     // the table is freed below: the launch must have finished
  hipFree(dev);
  if (e != hipSuccess) return eae_set_error(EAE_ERR_HIP, hipGetErrorString(e));
  if (rc) return rc;
  if (es != hipSuccess) return eae_set_error(EAE_ERR_HIP, hipGetErrorString(es));
  return 0;
}
// fp8 variant (qs != NULL): qs (device) = {1/s_small, 1/s_big, 1/(s_small * s_big)}; the SRC_BNBWD operand is converted to e5m2, the other to e4m3
static int op_wgrad_s2(void* stream, eae_src small_src, eae_src big_src, int cs, int cb, int B, int Hs, int Ws, float* scratch,
                       long long scratch_floats, float* dw, const float* qs) {
  WgradArgs w = WgradArgs();
  w.small = to_src(small_src); w.big = to_src(big_src); w.B = B; w.Hs = Hs; w.Ws = Ws; w.qs = qs;
  return eae_launch_wgrad_s2((hipStream_t)stream, w, cs, cb, small_src.mode, big_src.mode, scratch, scratch_floats, dw);
}
extern "C" int eae_op_wgrad_s2(void* stream, eae_src small_src, eae_src big_src, int cs, int cb, int B, int Hs, int Ws, float* scratch,
                               long long scratch_floats, float* dw) {
  return op_wgrad_s2(stream, small_src, big_src, cs, cb, B, Hs, Ws, scratch, scratch_floats, dw, nullptr);
}
extern "C" int eae_op_wgrad_s2_fp8(void* stream, eae_src small_src, eae_src big_src, int cs, int cb, int B, int Hs, int Ws, float* scratch,
                                   long long scratch_floats, float* dw, const float* qs) {
  if (!qs) return eae_set_error(EAE_ERR_ARG, "wgrad_s2_fp8: qs is NULL");
  return op_wgrad_s2(stream, small_src, big_src, cs, cb, B, Hs, Ws, scratch, scratch_floats, dw, qs);
}
extern "C" int eae_op_bn_finalize(void* stream, const float* stat_part, int ntiles, int C, long long count, const float* gamma,
                                  const float* beta, float* rm, float* rv, long long* nbt, float momentum, float eps, float* coef) {
  return eae_launch_bn_finalize((hipStream_t)stream, stat_part, ntiles, C, count, gamma, beta, rm, rv, nbt, momentum, eps, coef);
}
extern "C" int eae_op_bn_eval_coef(void* stream, int C, const float* gamma, const float* beta, const float* rm, const float* rv,
                                   float eps, float* coef) {
  return eae_launch_bn_eval_coef((hipStream_t)stream, C, gamma, beta, rm, rv, eps, coef);
}
extern "C" int eae_op_bn_bwd_finalize(void* stream, const float* stat_part, int ntiles, int C, long long count, const float* gamma,
                                      const float* coef_fwd, float* dgamma, float* dbeta, float* coef_bwd) {
  return eae_launch_bn_bwd_finalize((hipStream_t)stream, stat_part, ntiles, C, count, gamma, coef_fwd, dgamma, dbeta, coef_bwd);
}
extern "C" int eae_op_fc_splitk(void* stream, eae_src a, const void* w, int M, int N, int K, const float* bias, const float* addend,
                                float* scratch, long long scratch_floats, float* out) {
  if (a.mode != SRC_RAW && a.mode != SRC_BNRELU) return eae_set_error(EAE_ERR_ARG, "fc_splitk: source mode must be 0 or 1");
  if (K % 128 || (long long)(K / 128) * M * N > scratch_floats) return eae_set_error(EAE_ERR_ARG, "fc_splitk: K % 128 != 0 or scratch too small");
  FcNtArgs f = FcNtArgs();
  f.a = to_src(a); f.w = (const bf16_t*)w; f.M = M; f.N = N; f.K = K; f.klen = 128; f.part = scratch;
  RC(eae_launch_fc_nt((hipStream_t)stream, f, a.mode, FCE_PARTIAL, K / 128));
  return eae_launch_fc_reduce((hipStream_t)stream, scratch, K / 128, M, N, bias, addend, nullptr, out);
}
extern "C" int eae_op_fc_bias_bf16(void* stream, const float* a_f32, const void* w, int M, int N, int K, const float* bias, void* out) {
  FcNtArgs f = FcNtArgs();
  f.a = src_f32(a_f32); f.w = (const bf16_t*)w; f.M = M; f.N = N; f.K = K; f.klen = K;
  f.c = ConvArgs(); f.c.out = (bf16_t*)out; f.c.bias = bias;
  return eae_launch_fc_nt((hipStream_t)stream, f, SRC_F32, FCE_BIAS_BF16, 1);
}
extern "C" int eae_op_fc_wgrad(void* stream, int mode, eae_src p, eae_src q, int Bt, int I, int J, int Pn, float* dw, float* colsum) {
  FcTnArgs t = FcTnArgs();
  t.p = to_src(p); t.q = to_src(q); t.Bt = Bt; t.I = I; t.J = J; t.out = dw; t.colsum = colsum; t.out_mode = mode; t.Pn = Pn;
  if (mode == 0) return eae_launch_fc_tn((hipStream_t)stream, t, SRC_RAW, SRC_F32);
  if (mode == 1) return eae_launch_fc_tn((hipStream_t)stream, t, SRC_F32, SRC_BNRELU);
  return eae_set_error(EAE_ERR_ARG, "fc_wgrad: mode must be 0 (dec.fc) or 1 (enc.fc)");
}
static long long head_stride_of(int L, int C) { return r4(128LL * L) + 128 + r4(128LL * C) + r4(C); }
extern "C" long long eae_op_head_scratch_floats(int B, int L, int C) {
  return (long long)eae_head_blocks(B, L) * (head_stride_of(L, C) + 2) + 64;
}
static int op_head_ce(void* stream, const float* z, const float* w1, const float* b1, const float* w2, const float* b2,
                      const long long* labels, int B, int L, int C, float* logits, float* dz, float* grads, float* loss2,
                      float* scratch, long long scratch_floats, bool wce, const float* class_w, long long ignore_index) {
  if (!z || !w1 || !b1 || !w2 || !b2 || !scratch) return eae_set_error(EAE_ERR_ARG, "head_ce: NULL argument");
  if (scratch_floats < eae_op_head_scratch_floats(B, L, C)) return eae_set_error(EAE_ERR_ARG, "head_ce: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  const long long stride = head_stride_of(L, C);
  const int nb = eae_head_blocks(B, L);
  float* ce_part = scratch;                         // [nb][2]
  float* gpart = scratch + (((long long)nb * 2 + 3) & ~3LL);
  HeadArgs h = HeadArgs();
  h.z = z; h.w1 = w1; h.b1 = b1; h.w2 = w2; h.b2 = b2; h.labels = labels; h.B = B; h.L = L; h.C = C; h.inv_batch = 1.0f / (float)B;
  h.logits = logits; h.dz = dz; h.grad_part = (labels && grads) ? gpart : nullptr; h.grad_stride = stride; h.loss_part = ce_part;
  if (wce) RC(eae_launch_head_w(st, h, class_w, ignore_index));
  else RC(eae_launch_head(st, h));
  if (labels && grads) RC(eae_launch_reduce_slices(st, gpart, nb, (long)(stride / 4), grads, 1.0f));
  if (labels && loss2) RC(eae_launch_ce_mean(st, ce_part, nb, B, loss2));
  return 0;
}
extern "C" int eae_op_head_ce(void* stream, const float* z, const float* w1, const float* b1, const float* w2, const float* b2,
                              const long long* labels, int B, int L, int C, float* logits, float* dz, float* grads, float* loss2,
                              float* scratch, long long scratch_floats) {
  return op_head_ce(stream, z, w1, b1, w2, b2, labels, B, L, C, logits, dz, grads, loss2, scratch, scratch_floats, false, nullptr, 0);
}
extern "C" int eae_op_head_ce_w(void* stream, const float* z, const float* w1, const float* b1, const float* w2, const float* b2,
                                const long long* labels, int B, int L, int C, float* logits, float* dz, float* grads, float* loss2,
                                float* scratch, long long scratch_floats, const float* class_w, long long ignore_index) {
  return op_head_ce(stream, z, w1, b1, w2, b2, labels, B, L, C, logits, dz, grads, loss2, scratch, scratch_floats,
                    class_w != nullptr || ignore_index != EAE_NO_IGNORE, class_w, ignore_index);
}
extern "C" int eae_op_pack3x3(void* stream, const float* w, int A, int B, void* p1, void* p2) {
  // one-off helper for tests: builds a 2-entry descriptor table on the fly (synchronous upload)
  PackDesc d[2];
  long long n = (long long)A * B * 9;
  d[0] = PackDesc{0, 0, n, PACK_3x3_P1, A, B, 0, 0, 0, -1};
  d[1] = PackDesc{0, (long long)((char*)p2 - (char*)p1), n, PACK_3x3_P2, A, B, 0, 0, 0, -1};
  PackDesc* dev = nullptr;
  EAE_HIP(hipMalloc(&dev, sizeof(d)));
  EAE_HIP(hipMemcpy(dev, d, sizeof(d), hipMemcpyHostToDevice));
  int rc = eae_launch_pack_all((hipStream_t)stream, dev, 2, w, p1);
  hipStreamSynchronize((hipStream_t)stream);
  hipFree(dev);
  return rc;
}
extern "C" int eae_stage_bands(void* stream, const void* src, int elem_bytes, long long N, int C, int H, int W, const long long* index,
                               int B, const float* divisor, float* out, int train, float noise_std, unsigned long long seed,
                               unsigned long long step, const int* params, const float* noise) {
  return eae_launch_stage_bands((hipStream_t)stream, src, elem_bytes, N, C, H, W, index, B, divisor, out, train, noise_std, seed, step, params,
                                noise);
}
extern "C" int eae_augment(void* stream, const void* in_u8, float* out, int B, int H, int W, int train, float noise_std,
                           unsigned long long seed, unsigned long long step, const int* params, const float* noise) {
  return eae_launch_augment((hipStream_t)stream, in_u8, out, B, H, W, train, noise_std, seed, step, params, noise);
}
extern "C" int eae_op_adam(void* stream, float* p, const float* g, float* m, float* v, long long n, double lr, double b1, double b2,
                           double eps, double wd, long long step) {
  AdamLaunch a;
  a.p = p; a.g = g; a.m = m; a.v = v; a.n = n; a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = eps; a.wd = wd; a.step = step;
  return eae_launch_adam((hipStream_t)stream, a);
}
