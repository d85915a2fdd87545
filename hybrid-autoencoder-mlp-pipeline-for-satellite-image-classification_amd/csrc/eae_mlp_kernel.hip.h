// The MLP step kernel (eae_mlp.hip), included inside an unnamed namespace once per translation unit with MLP_WCE 0 (mlp_kernel, eae_mlp.hip)
// or 1 (mlp_kernel_wce, eae_mlp_wce.hip).  A textual switch, not a template: the plain kernel then is the very function it was before the
// weighted one existed, and is compiled to the same instructions.  Whoever edits this body rebuilds BOTH units and compares the
// device assembly of mlp_kernel with the previous build's (hipcc --cuda-device-only -S): a change meant for one kernel lands in both.
// MLP_WCE: class-weighted CrossEntropyLoss with ignored labels (include/eae.h, eae_mlp_set_class_weights; launched with labels only).
// A row counts when its label is not `ign` and lies in [0, C); W = sum of cw[label] over the counted rows of the WHOLE batch -- in eval
// mode every block sums all B rows in the same fixed order, so the blocks agree bitwise; dlogits = (softmax - onehot) * cw[label] / W,
// an exact zero row for a row that does not count; stats[0] += the block's share of CE * B, stats[2] += the counted correct rows.
// W == 0: loss and gradients are zero.  BatchNorm statistics stay over all rows.  The same pass counts the counted rows; block 0
// adds the count to the device word `valid`.
#if MLP_WCE
__global__ EAE_NO_PK __launch_bounds__(T) void mlp_kernel_wce(MlpArgsW w) {
  const MlpArgs& a = w.a;
  const float* cw = w.class_w;
  const long long ign = w.ignore_index;
#else
__global__ EAE_NO_PK __launch_bounds__(T) void mlp_kernel(MlpArgs a) {
#endif
  __shared__ float red[2 * T];
  __shared__ float mean1[H1], var1[H1], inv1[H1], mean2[H2], var2[H2], inv2[H2], c1[H1], c2[H1];
  const int tid = threadIdx.x;
  const int IN = a.IN, C = a.C;
  // rows handled by this block (training: the whole batch in block 0; eval: 64 rows per block)
  const int r0 = a.train ? 0 : blockIdx.x * 64;
  const int nb = a.train ? a.B : min(64, a.B - r0);
  const int ldx = a.ldx;
  const float* x = a.x + (size_t)r0 * ldx;
  const float *W1 = a.P + a.off[0], *b1 = a.P + a.off[1], *g1w = a.P + a.off[2], *be1 = a.P + a.off[3];
  const float *W2 = a.P + a.off[4], *b2 = a.P + a.off[5], *g2w = a.P + a.off[6], *be2 = a.P + a.off[7];
  const float *W3 = a.P + a.off[8], *b3 = a.P + a.off[9];
  float *h1 = a.h1 + (size_t)r0 * H1, *a1 = a.a1 + (size_t)r0 * H1, *h2 = a.h2 + (size_t)r0 * H2, *a2 = a.a2 + (size_t)r0 * H2;
  float* dlog = a.dlog + (size_t)r0 * 16;
  // ---- layer 1
  for (int i = tid; i < nb * H1; i += T) {
    int b = i / H1, j = i % H1;
    float s = b1[j];
    for (int k = 0; k < IN; ++k) s = fmaf(x[(size_t)b * ldx + k], W1[j * IN + k], s);
    h1[i] = s;
  }
  __syncthreads();
  if (a.train) {
    col_stats(h1, nb, H1, mean1, var1, red);
    if (tid < H1) {
      inv1[tid] = 1.0f / sqrtf(var1[tid] + BN_EPS);
      float unb = nb > 1 ? var1[tid] * nb / (nb - 1) : var1[tid];
      if (a.update_running) {
        a.bnrun[tid] = (1.f - BN_MOM) * a.bnrun[tid] + BN_MOM * mean1[tid];
        a.bnrun[H1 + tid] = (1.f - BN_MOM) * a.bnrun[H1 + tid] + BN_MOM * unb;
      }
    }
    if (tid == 0 && a.nbt && a.update_running) { a.nbt[0] += 1; a.nbt[1] += 1; }
  } else if (tid < H1) {
    mean1[tid] = a.bnrun[tid];
    inv1[tid] = 1.0f / sqrtf(a.bnrun[H1 + tid] + BN_EPS);
  }
  __syncthreads();
  const float keep_scale = 1.0f / (1.0f - a.p_drop);
  for (int i = tid; i < nb * H1; i += T) {
    int j = i % H1;
    float o = fmaf(g1w[j], (h1[i] - mean1[j]) * inv1[j], be1[j]);
    float v = fmaxf(o, 0.f);
    if (a.train && a.p_drop > 0.f) {
      float keep;
      if (a.drop_mask) keep = a.drop_mask[(size_t)r0 * H1 + i];
      else keep = philox_uniform(a.seed, a.step, (uint32_t)i) >= a.p_drop ? 1.f : 0.f;
      v = v * keep * keep_scale;
    }
    a1[i] = v;
  }
  __syncthreads();
  // ---- layer 2
  for (int i = tid; i < nb * H2; i += T) {
    int b = i / H2, j = i % H2;
    float s = b2[j];
    for (int k = 0; k < H1; ++k) s = fmaf(a1[b * H1 + k], W2[j * H1 + k], s);
    h2[i] = s;
  }
  __syncthreads();
  if (a.train) {
    col_stats(h2, nb, H2, mean2, var2, red);
    if (tid < H2) {
      inv2[tid] = 1.0f / sqrtf(var2[tid] + BN_EPS);
      float unb = nb > 1 ? var2[tid] * nb / (nb - 1) : var2[tid];
      if (a.update_running) {
        a.bnrun[2 * H1 + tid] = (1.f - BN_MOM) * a.bnrun[2 * H1 + tid] + BN_MOM * mean2[tid];
        a.bnrun[2 * H1 + H2 + tid] = (1.f - BN_MOM) * a.bnrun[2 * H1 + H2 + tid] + BN_MOM * unb;
      }
    }
  } else if (tid < H2) {
    mean2[tid] = a.bnrun[2 * H1 + tid];
    inv2[tid] = 1.0f / sqrtf(a.bnrun[2 * H1 + H2 + tid] + BN_EPS);
  }
  __syncthreads();
  for (int i = tid; i < nb * H2; i += T) {
    int j = i % H2;
    a2[i] = fmaxf(fmaf(g2w[j], (h2[i] - mean2[j]) * inv2[j], be2[j]), 0.f);
  }
  __syncthreads();
  // ---- layer 3 + softmax / CE
  for (int i = tid; i < nb * C; i += T) {
    int b = i / C, c = i % C;
    float s = b3[c];
    for (int k = 0; k < H2; ++k) s = fmaf(a2[b * H2 + k], W3[c * H2 + k], s);
    dlog[b * 16 + c] = s;
    if (a.logits) a.logits[(size_t)(r0 + b) * C + c] = s;
  }
  __syncthreads();
  if (a.dlog_in) {
    for (int i = tid; i < nb * C; i += T) dlog[(i / C) * 16 + (i % C)] = a.dlog_in[(size_t)r0 * C + i];
    __syncthreads();
  }
  if (a.probs) {             // predict epilogue (eval mode): class probabilities and label of each row at its window's grid position
    for (int b = tid; b < nb; b += T) {
      const float* l = dlog + b * 16;
      float mx = l[0]; int am = 0;
      for (int c = 1; c < C; ++c) if (l[c] > mx) { mx = l[c]; am = c; }
      float se = 0.f;
      for (int c = 0; c < C; ++c) se += expf(l[c] - mx);
      long long w = a.win0 + r0 + b;
      if (a.index) {
        w = a.index[w];
        if (w < 0 || w >= a.plane) continue;
      }
      for (int c = 0; c < C; ++c) a.probs[c * a.plane + w] = expf(l[c] - mx) / se;
      a.plabels[w] = am;
    }
  }
  if (!a.labels && !a.dlog_in) return;
  float loss = 0.f, corr = 0.f;
#if MLP_WCE
  float inv_w = 0.f;
  {
    float s = 0.f;
    int n = 0;
    for (int b = tid; b < a.B; b += T) {
      const long long lab = a.labels[b];
      if (lab != ign && lab >= 0 && lab < C) { s += cw ? cw[(int)lab] : 1.f; ++n; }
    }
    for (int o = 32; o >= 1; o >>= 1) { s += __shfl_xor(s, o, 64); n += __shfl_xor(n, o, 64); }
    if ((tid & 63) == 0) { red[tid >> 6] = s; red[T + (tid >> 6)] = (float)n; }      // (a wave counts at most B / 16 rows: exact in fp32 up to 2^24)
    __syncthreads();
    float wt = 0.f;
    for (int i = 0; i < T / 64; ++i) wt += red[i];
    if (tid == 0 && blockIdx.x == 0 && w.valid) {
      long long cnt = 0;
      for (int i = 0; i < T / 64; ++i) cnt += (long long)red[T + i];
      *w.valid += cnt;
    }
    inv_w = wt > 0.f ? 1.0f / wt : 0.f;
    __syncthreads();          // red takes the loss partials below
  }
#endif
  if (!a.dlog_in)
  for (int b = tid; b < nb; b += T) {
    float* l = dlog + b * 16;
    float mx = l[0]; int am = 0;
    for (int c = 1; c < C; ++c) if (l[c] > mx) { mx = l[c]; am = c; }
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(l[c] - mx);
    float lse = logf(se) + mx;
#if MLP_WCE
    const long long lab64 = a.labels[r0 + b];
    if (lab64 != ign && lab64 >= 0 && lab64 < C) {
      const int lab = (int)lab64;
      const float wl = cw ? cw[lab] : 1.f;
      loss += wl * (lse - l[lab]) * ((float)a.B * inv_w);
      corr += (am == lab) ? 1.f : 0.f;
      const float sc = wl * inv_w;
      for (int c = 0; c < C; ++c) l[c] = (expf(l[c] - lse) - (c == lab ? 1.f : 0.f)) * sc;
    } else {
      for (int c = 0; c < C; ++c) l[c] = 0.f;
    }
#else
    int lab = (int)a.labels[r0 + b];
    loss += lse - l[lab];
    corr += (am == lab) ? 1.f : 0.f;
    for (int c = 0; c < C; ++c) l[c] = (expf(l[c] - lse) - (c == lab ? 1.f : 0.f)) / (float)a.B;
#endif
  }
  red[tid] = loss; red[T + tid] = corr;
  __syncthreads();
  if (tid == 0 && a.stats) {
    double sd = 0.0;         // up to 1024 partial sums: a serial fp32 sum loses sqrt(lim) ulps of the mean loss
    float cr = 0.f;
    const int lim = nb < T ? nb : T;
    for (int i = 0; i < lim; ++i) { sd += (double)red[i]; cr += red[T + i]; }
    const float s = (float)sd;
    if (a.train) { a.stats[0] += s; a.stats[1] += (float)nb; a.stats[2] += cr; }   // sum_b CE_b = mean CE * B
    else { atomicAdd(&a.stats[0], s); atomicAdd(&a.stats[1], (float)nb); atomicAdd(&a.stats[2], cr); }
  }
  if (!a.backward) return;
  // =========================================================================================== backward (train only)
  float *G = a.G;
  float *g2 = a.g2, *g1 = a.g1;
  // layer 3: dW3, db3, da2 -> do2
  for (int i = tid; i < C * H2; i += T) {
    int c = i / H2, k = i % H2;
    float s = 0.f;
    for (int b = 0; b < nb; ++b) s = fmaf(dlog[b * 16 + c], a2[b * H2 + k], s);
    G[a.off[8] + i] = s;
  }
  if (tid < C) { float s = 0.f; for (int b = 0; b < nb; ++b) s += dlog[b * 16 + tid]; G[a.off[9] + tid] = s; }
  for (int i = tid; i < nb * H2; i += T) {
    int b = i / H2, k = i % H2;
    float s = 0.f;
    for (int c = 0; c < C; ++c) s = fmaf(dlog[b * 16 + c], W3[c * H2 + k], s);
    g2[i] = a2[i] > 0.f ? s : 0.f;
  }
  __syncthreads();
  // BN2 backward
  col_sums2(g2, h2, mean2, inv2, nb, H2, c1, c2, red);     // c1 = dbeta, c2 = dgamma
  if (tid < H2) { G[a.off[7] + tid] = c1[tid]; G[a.off[6] + tid] = c2[tid]; }
  for (int i = tid; i < nb * H2; i += T) {
    int j = i % H2;
    float xh = (h2[i] - mean2[j]) * inv2[j];
    g2[i] = g2w[j] * inv2[j] / nb * (nb * g2[i] - c1[j] - xh * c2[j]);
  }
  __syncthreads();
  // layer 2: dW2, db2, da1 -> do1
  for (int i = tid; i < H2 * H1; i += T) {
    int j = i / H1, k = i % H1;
    float s = 0.f;
    for (int b = 0; b < nb; ++b) s = fmaf(g2[b * H2 + j], a1[b * H1 + k], s);
    G[a.off[4] + i] = s;
  }
  if (tid < H2) { float s = 0.f; for (int b = 0; b < nb; ++b) s += g2[b * H2 + tid]; G[a.off[5] + tid] = s; }
  for (int i = tid; i < nb * H1; i += T) {
    int b = i / H1, k = i % H1;
    float s = 0.f;
    for (int j = 0; j < H2; ++j) s = fmaf(g2[b * H2 + j], W2[j * H1 + k], s);
    // d(ReLU o Dropout): a1 > 0 iff the unit was kept and its BN output was positive
    float keep = (!a.train || a.p_drop <= 0.f) ? 1.f : keep_scale;
    g1[i] = a1[i] > 0.f ? s * keep : 0.f;
  }
  __syncthreads();
  col_sums2(g1, h1, mean1, inv1, nb, H1, c1, c2, red);
  if (tid < H1) { G[a.off[3] + tid] = c1[tid]; G[a.off[2] + tid] = c2[tid]; }
  for (int i = tid; i < nb * H1; i += T) {
    int j = i % H1;
    float xh = (h1[i] - mean1[j]) * inv1[j];
    g1[i] = g1w[j] * inv1[j] / nb * (nb * g1[i] - c1[j] - xh * c2[j]);
  }
  __syncthreads();
  for (int i = tid; i < H1 * IN; i += T) {
    int j = i / IN, k = i % IN;
    float s = 0.f;
    for (int b = 0; b < nb; ++b) s = fmaf(g1[b * H1 + j], x[(size_t)b * ldx + k], s);
    G[a.off[0] + i] = s;
  }
  if (tid < H1) { float s = 0.f; for (int b = 0; b < nb; ++b) s += g1[b * H1 + tid]; G[a.off[1] + tid] = s; }
  __syncthreads();
  if (!a.adam) return;
  // ---- Adam with coupled L2 weight decay (torch.optim.Adam(lr, weight_decay=1e-4), R.md:2625)
  for (long i = tid; i < a.off[10]; i += T) {
    float p = a.P[i], g = G[i] + a.wd * p, m = a.M[i], v = a.V[i];
    m = m + a.omb1 * (g - m);
    v = a.b2 * v + a.omb2 * g * g;
    a.P[i] = p - a.step_size * (m / (sqrtf(v) / a.bc2_sqrt + a.eps));
    a.M[i] = m; a.V[i] = v;
  }
}
