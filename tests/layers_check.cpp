// Stand-alone check of csrc/eae_layers.h (compiled and run by test_layers.py): everything derived from the layer tables equals the
// literal arrays and the positional list of 38 sizes that the engine used before the tables existed.  Prints every difference and
// returns their number.
#include "eae_layers.h"
#include <cstdio>

static int bad = 0;
static void eq(const char* what, int i, long long got, long long want) {
  if (got == want) return;
  std::printf("%s[%d]: table %lld, literal %lld\n", what, i, got, want);
  ++bad;
}

int main() {
  const int ENC_C[5] = {3, 32, 64, 128, 256};
  const int BN_C[7] = {32, 64, 128, 256, 128, 64, 32};
  const int BN_GAMMA_IDX[7] = {2, 6, 10, 14, 22, 26, 30};
  const int W3_PARAM[6] = {4, 8, 12, 20, 24, 28};      // conv2, conv3, conv4, deconv1, deconv2, deconv3
  const int W3_A[6] = {64, 128, 256, 256, 128, 64};
  const int W3_B[6] = {32, 64, 128, 128, 64, 32};
  const int PREBN_BIAS[7] = {1, 5, 9, 13, 21, 25, 29};
  const int dec_cin[3] = {256, 128, 64};               // the decoder loops' local arrays (forward and backward)

  eq("T_COUNT", 0, T_COUNT, 38);
  eq("N_BN", 0, N_BN, 7);
  eq("N_L3", 0, N_L3, 6);
  eq("ENC_C", 0, DEFAULT_BANDS, ENC_C[0]);
  for (int lvl = 1; lvl <= 4; ++lvl) eq("ENC_C", lvl, enc_channels(lvl), ENC_C[lvl]);
  for (int l = 0; l < 7; ++l) {
    eq("BN_C", l, BN_LAYERS[l].c, BN_C[l]);
    eq("BN_GAMMA_IDX", l, BN_LAYERS[l].gamma, BN_GAMMA_IDX[l]);
    eq("PREBN_BIAS", l, BN_LAYERS[l].bias, PREBN_BIAS[l]);
  }
  for (int j = 0; j < 6; ++j) {
    eq("W3_PARAM", j, L3[j].w, W3_PARAM[j]);
    eq("W3_A", j, L3[j].cs(), W3_A[j]);
    eq("W3_B", j, L3[j].cb(), W3_B[j]);
    eq("W3 kind", j, L3[j].kind, j < 3 ? L3_CONV : L3_DECONV);
  }
  for (int i = 1; i < 4; ++i) {                        // encoder layer i = conv(i + 1): what the loops computed from i
    const Layer3& r = L3[i - 1];
    eq("enc cin", i, r.cin, ENC_C[i]);
    eq("enc cout", i, r.cout, ENC_C[i + 1]);
    eq("enc bias", i, r.b, 4 * i + 1);
    eq("enc weight", i, r.w, 4 * i);
    eq("enc bn_out", i, r.bn_out, i);
    eq("enc bn_in", i, r.bn_in, i - 1);
    eq("enc dy bit", i, r.dy_bit, i);
    eq("enc site", i, r.site, i);
    eq("enc 64 >> in", i, 64 >> r.in_lvl(), 64 >> i);
    eq("enc 64 >> small", i, 64 >> r.lvl, 64 >> (i + 1));
    eq("enc 64 >> out", i, 64 >> r.out_lvl(), (64 >> i) / 2);
  }
  for (int i = 0; i < 3; ++i) {                        // decoder layer i = deconv(i + 1)
    const Layer3& r = L3[3 + i];
    eq("dec cin", i, r.cin, dec_cin[i]);
    eq("dec cout", i, r.cout, dec_cin[i] / 2);
    eq("dec bias", i, r.b, 21 + 4 * i);
    eq("dec weight", i, r.w, 20 + 4 * i);
    eq("dec bn_out", i, r.bn_out, 4 + i);
    eq("dec bn_in", i, r.bn_in, i == 0 ? -1 : 3 + i);
    eq("dec dy bit", i, r.dy_bit, 4 + i);
    eq("dec site", i, r.site, 4 + i);
    eq("dec 64 >> in", i, 64 >> r.in_lvl(), 64 >> (4 - i));
    eq("dec 64 >> small", i, 64 >> r.lvl, 64 >> (4 - i));
    eq("dec 64 >> out", i, 64 >> r.out_lvl(), (64 >> (4 - i)) * 2);
  }
  eq("CUT_CONVS_FC", 0, CUT_CONVS_FC, 16);
  eq("CUT_ENC_DEC", 0, CUT_ENC_DEC, 18);
  eq("CUT_FC_DECONVS", 0, CUT_FC_DECONVS, 20);
  eq("T_ENCFC_B", 0, T_ENCFC_B, 17);
  eq("T_DECFC_B", 0, T_DECFC_B, 19);
  eq("T_DECONV4_W", 0, T_DECONV4_W, 32);
  eq("T_DECONV4_B", 0, T_DECONV4_B, 33);
  eq("T_CLS0_W", 0, T_CLS0_W, 34);
  eq("T_CLS0_B", 0, T_CLS0_B, 35);
  eq("T_CLS2_W", 0, T_CLS2_W, 36);
  eq("T_CLS2_B", 0, T_CLS2_B, 37);

  const int latents[5] = {1, 48, 64, 128, 256}, classes[3] = {1, 10, 64}, bands[3] = {1, 3, 16}, images[2][2] = {{64, 64}, {128, 256}};
  int configs = 0;
  for (int Li : latents) for (int Ci : classes) for (int Ni : bands) for (const int* hw : images) {
    const long long P = (long long)(hw[0] / 16) * (hw[1] / 16), K = 256 * P, L = Li, C = Ci, N = Ni;
    const long long want[38] = {32 * 9 * N, 32, 32, 32, 64 * 32 * 9, 64, 64, 64, 128 * 64 * 9, 128, 128, 128, 256 * 128 * 9, 256, 256, 256,
                                L * K, L, K * L, K, 256 * 128 * 9, 128, 128, 128, 128 * 64 * 9, 64, 64, 64, 64 * 32 * 9, 32, 32, 32,
                                32 * 9 * N, N, 128 * L, 128, C * 128, C};
    long long got[T_COUNT];
    for (long long& g : got) g = -1;                   // a tensor the tables forget stays -1
    eae_param_sizes(hw[0], hw[1], Li, Ci, Ni, got);
    for (int t = 0; t < 38; ++t) eq("size", t, got[t], want[t]);
    ++configs;
  }
  std::printf("%d configurations, %d differences\n", configs, bad);
  return bad ? 1 : 0;
}
