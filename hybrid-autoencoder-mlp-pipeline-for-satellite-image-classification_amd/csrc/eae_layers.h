// The supervised autoencoder described once: its 38 parameter tensors in arena order, its seven BatchNorm layers and its six 3x3
// stride-2 layers.  Everything that addresses the model by layer or tensor (arena layout, packs, the step's forward and backward,
// the data-parallel cut points) reads it HERE; the static_asserts at the end tie the tables together.  Plain host code, nothing
// from HIP.
#pragma once

// ---- the 38 tensors, in arena order (= named_parameters() order of the module)
enum EaeTensor {
  T_CONV1_W, T_CONV1_B, T_CONV1_GAMMA, T_CONV1_BETA, T_CONV2_W, T_CONV2_B, T_CONV2_GAMMA, T_CONV2_BETA,
  T_CONV3_W, T_CONV3_B, T_CONV3_GAMMA, T_CONV3_BETA, T_CONV4_W, T_CONV4_B, T_CONV4_GAMMA, T_CONV4_BETA,
  T_ENCFC_W, T_ENCFC_B, T_DECFC_W, T_DECFC_B,
  T_DECONV1_W, T_DECONV1_B, T_DECONV1_GAMMA, T_DECONV1_BETA, T_DECONV2_W, T_DECONV2_B, T_DECONV2_GAMMA, T_DECONV2_BETA,
  T_DECONV3_W, T_DECONV3_B, T_DECONV3_GAMMA, T_DECONV3_BETA, T_DECONV4_W, T_DECONV4_B,
  T_CLS0_W, T_CLS0_B, T_CLS2_W, T_CLS2_B, T_COUNT
};
// Cut points of the data-parallel buckets (the backward completes the arena from its end: classifier, decoder, dec.fc, enc.fc, encoder)
enum {
  CUT_CONVS_FC = T_ENCFC_W,        // encoder convolutions | the two latent projections
  CUT_ENC_DEC = T_DECFC_W,         // encoder half (tensors below: conv1..4, enc.fc) | decoder half (dec.fc, decoder, classifier)
  CUT_FC_DECONVS = T_DECONV1_W     // the two latent projections | transposed convolutions and classifier
};

constexpr int DEFAULT_BANDS = 3;   // eae_config::in_channels = 0: RGB
constexpr int CLS_HIDDEN = 128;    // width of the classifier's hidden layer

// ---- the seven BatchNorm layers: behind conv1..4 (0..3) and deconv1..3 (4..6)
// channels; tensor of the scale (the shift follows it); bias of the layer in front: BatchNorm removes it, so its gradient is zero in train mode
struct BnLayer { int c, gamma, bias; };
constexpr int N_BN = 7;
constexpr BnLayer BN_LAYERS[N_BN] = {
  {32, T_CONV1_GAMMA, T_CONV1_B},      {64, T_CONV2_GAMMA, T_CONV2_B},     {128, T_CONV3_GAMMA, T_CONV3_B}, {256, T_CONV4_GAMMA, T_CONV4_B},
  {128, T_DECONV1_GAMMA, T_DECONV1_B}, {64, T_DECONV2_GAMMA, T_DECONV2_B}, {32, T_DECONV3_GAMMA, T_DECONV3_B}};

// ---- the six 3x3 stride-2 layers in the order of the weight packs and fp8 scale slots ("W3 order")
enum { L3_CONV = 0, L3_DECONV = 1 };   // = S2_CONV / S2_DECONV (eae_conv_plan.h)
struct Layer3 {
  int kind;            // L3_CONV: big map -> small map; L3_DECONV (transposed): small map -> big map
  int cin, cout;
  int w, b;            // weight and bias tensors
  int bn_out;          // BatchNorm layer of the output (also the index of the layer's output among the activations y[0..3], u[0..2])
  int bn_in;           // BatchNorm layer of the input, -1: the input is raw (deconv1 reads d0)
  int lvl;             // the SMALL map is (H >> lvl) x (W >> lvl), the big one twice that
  int dy_bit, site;    // bit of eae_ctx::dy_mask, layer number of EAE_PROF_SITE
  // the weight is [cs][cb][3][3]: cs = channels on the small map, cb = channels on the big map
  constexpr int cs() const { return kind == L3_CONV ? cout : cin; }
  constexpr int cb() const { return kind == L3_CONV ? cin : cout; }
  constexpr int in_lvl() const { return kind == L3_CONV ? lvl - 1 : lvl; }
  constexpr int out_lvl() const { return kind == L3_CONV ? lvl : lvl - 1; }
};
constexpr int N_L3 = 6;
constexpr Layer3 L3[N_L3] = {      // kind, cin, cout, w, b, bn_out, bn_in, lvl, dy_bit, site
  {L3_CONV, 32, 64, T_CONV2_W, T_CONV2_B, 1, 0, 2, 1, 1},
  {L3_CONV, 64, 128, T_CONV3_W, T_CONV3_B, 2, 1, 3, 2, 2},
  {L3_CONV, 128, 256, T_CONV4_W, T_CONV4_B, 3, 2, 4, 3, 3},
  {L3_DECONV, 256, 128, T_DECONV1_W, T_DECONV1_B, 4, -1, 4, 4, 4},
  {L3_DECONV, 128, 64, T_DECONV2_W, T_DECONV2_B, 5, 4, 3, 5, 5},
  {L3_DECONV, 64, 32, T_DECONV3_W, T_DECONV3_B, 6, 5, 2, 6, 6}};
constexpr int L3_FIRST_DECONV = 3;

// channels of the encoder's map after `lvl` stride-2 stages (1..4); the latent projections flatten the last one
constexpr int enc_channels(int lvl) { return BN_LAYERS[lvl - 1].c; }
constexpr int FC_CHANNELS = enc_channels(4);

// elements of the 38 tensors (without the arena's rounding) for H x W images of N bands, latent width L, C classes
inline void eae_param_sizes(int H, int W, int L, int C, int N, long long* sz) {
  const long long K = (long long)FC_CHANNELS * (H / 16) * (W / 16);
  for (int l = 0; l < N_BN; ++l) sz[BN_LAYERS[l].bias] = sz[BN_LAYERS[l].gamma] = sz[BN_LAYERS[l].gamma + 1] = BN_LAYERS[l].c;
  for (int j = 0; j < N_L3; ++j) sz[L3[j].w] = (long long)L3[j].cin * L3[j].cout * 9;
  sz[T_CONV1_W] = (long long)BN_LAYERS[0].c * N * 9;            // [32][N][3][3]
  sz[T_DECONV4_W] = (long long)L3[N_L3 - 1].cout * N * 9;       // [32][N][3][3] ([Cin][Cout][kh][kw])
  sz[T_DECONV4_B] = N;
  sz[T_ENCFC_W] = L * K; sz[T_ENCFC_B] = L; sz[T_DECFC_W] = K * L; sz[T_DECFC_B] = K;
  sz[T_CLS0_W] = (long long)CLS_HIDDEN * L; sz[T_CLS0_B] = CLS_HIDDEN; sz[T_CLS2_W] = (long long)C * CLS_HIDDEN; sz[T_CLS2_B] = C;
}

// ---- the tables agree with one another
constexpr bool layers_consistent() {
  for (int l = 0; l < N_BN; ++l)
    if (BN_LAYERS[l].bias != BN_LAYERS[l].gamma - 1) return false;                     // {.., bias, gamma, beta}
  if (BN_LAYERS[0].bias != T_CONV1_W + 1) return false;
  for (int j = 0; j < N_L3; ++j) {
    const Layer3& r = L3[j];
    if (r.b != r.w + 1 || BN_LAYERS[r.bn_out].bias != r.b) return false;                // {weight, bias, gamma, beta} are consecutive
    if (r.cout != BN_LAYERS[r.bn_out].c) return false;
    if (r.bn_out != j + 1 || r.dy_bit != r.bn_out || r.site != r.bn_out) return false;  // layer numbers: conv1 is 0
    if (r.cs() != 2 * r.cb()) return false;
    // the channel counts and map levels chain from layer to layer; deconv1 continues from conv4's map through the two projections
    const int cin = r.bn_in >= 0 ? BN_LAYERS[r.bn_in].c : FC_CHANNELS;
    if (r.cin != cin || (r.bn_in >= 0 && r.bn_in != r.bn_out - 1)) return false;
    if (j > 0 && r.in_lvl() != L3[j - 1].out_lvl()) return false;
  }
  return L3[0].in_lvl() == 1 && L3[N_L3 - 1].out_lvl() == 1 && L3[0].cin == BN_LAYERS[0].c && L3[L3_FIRST_DECONV].bn_in < 0 &&
         L3[L3_FIRST_DECONV - 1].kind == L3_CONV && L3[L3_FIRST_DECONV].kind == L3_DECONV;
}
static_assert(T_COUNT == 38 && CUT_CONVS_FC == 16 && CUT_ENC_DEC == 18 && CUT_FC_DECONVS == 20, "arena order");
static_assert(T_DECONV4_W == 32 && T_CLS0_W == 34 && T_CLS2_B == 37, "arena order");
static_assert(layers_consistent(), "BN_LAYERS and L3 disagree");
