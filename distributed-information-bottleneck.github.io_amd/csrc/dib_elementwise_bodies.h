// dib_elementwise_bodies.h - the bodies of three kernels of csrc/dib_elementwise.h as text (each kernel includes this file once,
// DIB_ELEMENTWISE_BODY selecting the body): the single kernels run them on their arguments, the ensemble kernels
// (csrc/dib_ensemble.h, one replica per grid index) on locals of the same names that point at the replica's slices.
// Text, not a shared device function: the code generated for the single kernels stays what it was.
//   1  reparameterisation + KL forward: enc_out, U, kl_partial, row_idx, row0, batch, F, E, seed, step, deterministic, step_dev,
//      lv_off  (workgroup blockIdx.x of feature blockIdx.y; leaves `tot`, the workgroup's KL partial, and `f` in scope)
//   2  its backward: enc_out, GU, U, dout, beta_dev, inv_bg, batch, F, E, lv_off
//   3  task loss + gradient: kind, pred, out_dim, Y, ldy, row_idx, row0, batch, inv_bg, out_act, g_pred, partial
#if DIB_ELEMENTWISE_BODY == 1
  __shared__ float red[4];
  if (step_dev) step = step_dev[0];
  const int E4 = (E + 3) >> 2;
  const int rows_per_block = 256 / E4;
  const int f = blockIdx.y;
  const int r = threadIdx.x / E4, q = threadIdx.x - r * E4;
  const int b = blockIdx.x * rows_per_block + r;
  float klp = 0.f;
  if (r < rows_per_block && b < batch) {
    const long long grow = row_idx ? (long long)row_idx[b] : row0 + b;
    const float* mu_p = enc_out + ((long long)f * batch + b) * (2ll * E) + 4 * q;  // enc_out is [F][B][2E]
    const float* lv_p = mu_p + E;
    float* u_p = U + (long long)b * ((long long)F * E) + (long long)f * E + 4 * q;
    float eps[4] = {0.f, 0.f, 0.f, 0.f};
    if (!deterministic) dib_eps4(seed, step, (uint32_t)grow, (uint32_t)f, (uint32_t)q, eps);
    if ((E & 3) == 0) {
      const float4 mu = *reinterpret_cast<const float4*>(mu_p);
      float4 lv = *reinterpret_cast<const float4*>(lv_p);
      lv.x += lv_off; lv.y += lv_off; lv.z += lv_off; lv.w += lv_off;
      float4 u;
      u.x = mu.x + expf(0.5f * lv.x) * eps[0];
      u.y = mu.y + expf(0.5f * lv.y) * eps[1];
      u.z = mu.z + expf(0.5f * lv.z) * eps[2];
      u.w = mu.w + expf(0.5f * lv.w) * eps[3];
      *reinterpret_cast<float4*>(u_p) = u;
      klp = 0.5f * ((mu.x * mu.x + expf(lv.x) - lv.x - 1.f) + (mu.y * mu.y + expf(lv.y) - lv.y - 1.f) +
                    (mu.z * mu.z + expf(lv.z) - lv.z - 1.f) + (mu.w * mu.w + expf(lv.w) - lv.w - 1.f));
    } else {
      for (int j = 0; j < 4; ++j) {
        if (4 * q + j < E) {
          const float mu = mu_p[j], lv = lv_p[j] + lv_off;
          u_p[j] = mu + expf(0.5f * lv) * eps[j];
          klp += 0.5f * (mu * mu + expf(lv) - lv - 1.f);
        }
      }
    }
  }
  const float tot = dib_block_sum_256(klp, red);
  if (threadIdx.x == 0) kl_partial[(long long)blockIdx.x * F + f] = tot;
#elif DIB_ELEMENTWISE_BODY == 2
  const int E4 = (E + 3) >> 2;
  const int rows_per_block = 256 / E4;
  const int f = blockIdx.y;
  const int r = threadIdx.x / E4, q = threadIdx.x - r * E4;
  const int b = blockIdx.x * rows_per_block + r;
  if (r >= rows_per_block || b >= batch) return;
  const float kb = beta_dev[0] * inv_bg;
  const long long o = ((long long)f * batch + b) * (2ll * E) + 4 * q;  // enc_out / dout are [F][B][2E]
  const long long so = (long long)b * ((long long)F * E) + (long long)f * E + 4 * q;
  const float* gu_p = GU + so;
  const float* u_p = U + so;
  if ((E & 3) == 0) {
    const float4 mu = *reinterpret_cast<const float4*>(enc_out + o);
    float4 lv = *reinterpret_cast<const float4*>(enc_out + o + E);
    lv.x += lv_off; lv.y += lv_off; lv.z += lv_off; lv.w += lv_off;
    const float4 gu = *reinterpret_cast<const float4*>(gu_p);
    const float4 u = *reinterpret_cast<const float4*>(u_p);
    float4 dm, dl;
    dm.x = gu.x + kb * mu.x; dm.y = gu.y + kb * mu.y; dm.z = gu.z + kb * mu.z; dm.w = gu.w + kb * mu.w;
    dl.x = gu.x * (u.x - mu.x) * 0.5f + kb * 0.5f * (expf(lv.x) - 1.f);
    dl.y = gu.y * (u.y - mu.y) * 0.5f + kb * 0.5f * (expf(lv.y) - 1.f);
    dl.z = gu.z * (u.z - mu.z) * 0.5f + kb * 0.5f * (expf(lv.z) - 1.f);
    dl.w = gu.w * (u.w - mu.w) * 0.5f + kb * 0.5f * (expf(lv.w) - 1.f);
    *reinterpret_cast<float4*>(dout + o) = dm;
    *reinterpret_cast<float4*>(dout + o + E) = dl;
  } else {
    for (int j = 0; j < 4; ++j) {
      if (4 * q + j < E) {
        const float mu = enc_out[o + j], lv = enc_out[o + E + j] + lv_off, gu = gu_p[j];
        dout[o + j] = gu + kb * mu;
        dout[o + E + j] = gu * (u_p[j] - mu) * 0.5f + kb * 0.5f * (expf(lv) - 1.f);
      }
    }
  }
#elif DIB_ELEMENTWISE_BODY == 3
  __shared__ float red[4];
  const int b = blockIdx.x * 256 + threadIdx.x;
  float lsum = 0.f, correct = 0.f;
  if (b < batch) {
    const long long row = row_idx ? (long long)row_idx[b] : row0 + b;
    const float* p = pred + (long long)b * out_dim;
    float* g = g_pred + (long long)b * out_dim;
    const float* y = Y + row * ldy;
    if (kind == 0 || kind == 1 || kind == 3) {
      const float sc = inv_bg / (float)out_dim;
      float nright = 0.f;
      for (int o = 0; o < out_dim; ++o) {
        const float z = p[o], yy = y[o];
        float l, gg;
        if (kind == 0) {
          l = fmaxf(z, 0.f) - z * yy + log1pf(expf(-fabsf(z)));
          gg = 1.0f / (1.0f + expf(-z)) - yy;
        } else if (kind == 1) {
          const float pc = fminf(fmaxf(z, 1e-7f), 1.0f - 1e-7f);
          l = -(yy * logf(pc) + (1.f - yy) * logf(1.f - pc));
          gg = (z < 1e-7f || z > 1.0f - 1e-7f) ? 0.f : (-(yy / pc) + (1.f - yy) / (1.f - pc));
        } else {
          const float d = z - yy;
          l = d * d;
          gg = 2.f * d;
        }
        lsum += l;
        g[o] = gg * sc * dib_act_grad(out_act, z);
        nright += ((z > 0.5f ? 1.f : 0.f) == yy) ? 1.f : 0.f;
      }
      lsum /= (float)out_dim;
      correct = nright / (float)out_dim;
    } else {  // sparse categorical cross-entropy from logits
      const int lab = (int)y[0];
      float m = -INFINITY;
      int am = 0;
      for (int o = 0; o < out_dim; ++o)
        if (p[o] > m) { m = p[o]; am = o; }
      float se = 0.f;
      for (int o = 0; o < out_dim; ++o) se += expf(p[o] - m);
      const float lse = m + logf(se);
      lsum = lse - p[lab];
      for (int o = 0; o < out_dim; ++o) g[o] = (expf(p[o] - lse) - (o == lab ? 1.f : 0.f)) * inv_bg;
      correct = (am == lab) ? 1.f : 0.f;
    }
  }
  const float tl = dib_block_sum_256(lsum, red);
  const float tc = dib_block_sum_256(correct, red);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = tl;
    partial[2 * blockIdx.x + 1] = tc;
  }
#else
#error "DIB_ELEMENTWISE_BODY: 1 (reparameterisation forward), 2 (its backward) or 3 (task loss)"
#endif
