// host/input_grad.h - dL/dx of the encoder bank (csrc/dib_input_grad.h): what has to be in memory before the one launch, and the launch.

template <int NB>
static int launch_input_grad(const DibInputGradArgs& a, int gx, int F, size_t lds, hipStream_t st) {
  return launch_lds<&dib_input_grad_kernel<NB>>(dim3(gx, F), dim3(DIB_IG_THREADS), lds, st, a);
}

extern "C" {

// G = dL/d(pre-activation of encoder layer 0) is ws[g_enc_h[0]] (the last layer's dout for an encoder without hidden layers).  The
// grouped-GEMM backward wrote it; the fused and the row-tile backward contract d(W1|b1) in-kernel and leave the region - which
// WsMap allocates in every regime - unwritten: there the layer-1 dgrad GEMM of the unfused path (encoder_bank_bwd_stages) runs first,
// on the dh2 those kernels did write, after the first hidden layer has been materialised if the forward left it to the weight
// gradient's recompute.
int dib_encoder_bank_input_grad(dib_layout* l, const float* x, int64_t ldx, const int32_t* row_idx, int64_t row0, int batch,
                                const float* params, void* ws, float* dx, int64_t lddx, dib_stream_t stream) {
  if (!l || !x || !params || !ws || !dx || batch <= 0 || lddx < l->sum_d) return DIB_E_ARG;
  if (!l->dev_groups) return DIB_E_WORKSPACE;
  {
    std::lock_guard<std::mutex> lk(l->wg_mu);
    auto it = l->fwd_training.find(ws);
    if (it == l->fwd_training.end() || !it->second) return DIB_E_WORKSPACE;   // no forward, or DIB_FWD_INFERENCE: no stashes
  }
  hipStream_t st = (hipStream_t)stream;
  const auto m = l->map(batch);
  float* w = (float*)ws;
  DibInputGradArgs a;
  if (l->n_enc == 0) {
    a.G = w + m.dout; a.H = 2 * l->E;
  } else {
    a.G = w + m.g_enc_h[0]; a.H = l->enc_units[0];
    const bool small = use_small_enc(l, batch);
    if (small || fused_bwd_ok(l)) {
      if (!small && h1_plan_of(l, ws).recompute) {
        int rc = dib_workspace_h1_materialize(l, batch, params, ws, stream);
        if (rc) return rc;
      }
      int rc = launch_gemm<1>(l, l->enc_dgrad[1], w + m.g_enc_h[1], params, w + m.g_enc_h[0], nullptr, w + m.enc_h[0], nullptr, batch,
                              l->act, 1, 0, 0, st);
      if (rc) return rc;
    }
  }
  a.params = params; a.w_off = l->dev_fused_offs; a.featmap = l->dev_featmap;
  a.X = x; a.ldx = ldx; a.row_idx = (const int*)row_idx; a.row0 = row0; a.batch = batch; a.n_blocks = l->n_blocks;
  a.kc = dib_input_grad_kc(a.H, l->n_blocks);
  a.dx = dx; a.lddx = lddx;
  const size_t lds = (size_t)dib_input_grad_lds_bytes(a.H, l->n_blocks);
  // enough workgroups for eight per CU, each packing its feature's weights once and walking its share of the 16-row tiles
  const int gx = std::max(1, std::min(cdiv(cdiv(batch, 16), DIB_IG_WAVES), cdiv(2048, l->F)));
  ProfScope ps(kProfOther, st);
  switch (std::min(l->n_blocks, DIB_IG_NB)) {
    case 1: return launch_input_grad<1>(a, gx, l->F, lds, st);
    case 2: return launch_input_grad<2>(a, gx, l->F, lds, st);
    case 3: return launch_input_grad<3>(a, gx, l->F, lds, st);
    case 4: return launch_input_grad<4>(a, gx, l->F, lds, st);
    case 5: return launch_input_grad<5>(a, gx, l->F, lds, st);
    case 6: return launch_input_grad<6>(a, gx, l->F, lds, st);
    case 7: return launch_input_grad<7>(a, gx, l->F, lds, st);
    default: return launch_input_grad<8>(a, gx, l->F, lds, st);
  }
}

}  // extern "C"
