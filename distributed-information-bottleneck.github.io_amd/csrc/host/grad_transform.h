// host/grad_transform.h - gradient clipping and learning-rate schedules (include/dib_grad_transform.h, csrc/dib_grad_transform.h):
// the host-only variable table (segments of a layout, the tile work-list), the argument checks and the launches.

static_assert(sizeof(DibGradTile) == sizeof(dib_grad_tile) && sizeof(dib_grad_tile) == 16, "tile work-list entry");
static_assert(sizeof(DibLrSchedule) == sizeof(dib_lr_schedule), "schedule descriptor");
static_assert(kGradTile == DIB_GRAD_TILE, "tile size");

namespace {

inline bool gt_aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// the table's three arrays are there and the segment range lies in it; *tile_first / *tile_count: the range's tiles
int gt_check_range(const dib_grad_table* t, int seg_first, int seg_count, int* tile_first, int* tile_count) {
  if (!t || t->n_segments < 0 || t->n_tiles < 0 || t->n_tiles > INT32_MAX || !t->seg_tile0) return DIB_E_ARG;
  if (seg_first < 0 || seg_count < 0 || (int64_t)seg_first + seg_count > t->n_segments) return DIB_E_ARG;
  const int32_t a = t->seg_tile0[seg_first], b = t->seg_tile0[seg_first + seg_count];
  if (a < 0 || b < a || b > t->n_tiles) return DIB_E_ARG;
  if (b > a && (!t->tiles_dev || !t->seg_tile0_dev)) return DIB_E_ARG;
  *tile_first = a;
  *tile_count = b - a;
  return DIB_OK;
}

// clipvalue: 0 (off) or a finite positive threshold
inline bool gt_clipvalue_ok(float c) { return c >= 0.f && std::isfinite(c); }

}  // namespace

extern "C" {

int dib_grad_table_from_layout(const dib_layout* l, int64_t* offsets, int64_t* counts, int capacity) {
  if (!l) return DIB_E_ARG;
  const int LE = l->n_enc + 1, LI = l->n_int + 1;
  const int n = 2 * (LE * l->F + LI);
  if (!offsets && !counts) return n;
  if (!offsets || !counts || capacity < n) return DIB_E_ARG;
  int k = 0;
  for (int ly = 0; ly < LE; ++ly)
    for (int f = 0; f < l->F; ++f) {
      const int64_t win = ly == 0 ? l->in_dim[f] : l->enc_width[ly - 1];
      const int64_t wout = l->enc_width[ly];
      offsets[k] = l->enc_w_off[ly][f]; counts[k++] = win * wout;
      offsets[k] = l->enc_b_off[ly][f]; counts[k++] = wout;
    }
  for (int ly = 0; ly < LI; ++ly) {
    const int64_t win = ly == 0 ? (int64_t)l->F * l->E : l->int_width[ly - 1];
    const int64_t wout = l->int_width[ly];
    offsets[k] = l->int_w_off[ly]; counts[k++] = win * wout;
    offsets[k] = l->int_b_off[ly]; counts[k++] = wout;
  }
  return n;
}

int64_t dib_grad_table_tiles(const int64_t* offsets, const int64_t* counts, int n_segments, int64_t buffer_elems,
                             dib_grad_tile* tiles, int64_t tile_capacity, int32_t* seg_tile0) {
  if (n_segments < 0 || buffer_elems < 0 || (n_segments > 0 && (!offsets || !counts))) return DIB_E_ARG;
  if ((tiles == nullptr) != (seg_tile0 == nullptr)) return DIB_E_ARG;
  int64_t total = 0;
  for (int s = 0; s < n_segments; ++s) {
    if (offsets[s] < 0 || counts[s] < 0 || offsets[s] > buffer_elems || counts[s] > buffer_elems - offsets[s]) return DIB_E_ARG;
    for (int r = 0; r < s; ++r)   // two variables never share an element (empty ones share nothing)
      if (counts[s] > 0 && counts[r] > 0 && offsets[s] < offsets[r] + counts[r] && offsets[r] < offsets[s] + counts[s])
        return DIB_E_ARG;
    total += counts[s] / DIB_GRAD_TILE + (counts[s] % DIB_GRAD_TILE != 0);   // (no rounding-up add: counts[s] may be near INT64_MAX)
    if (total > INT32_MAX) return DIB_E_ARG;
  }
  if (!tiles) return total;
  if (tile_capacity < total) return DIB_E_ARG;
  int64_t k = 0;
  for (int s = 0; s < n_segments; ++s) {
    seg_tile0[s] = (int32_t)k;
    for (int64_t done = 0; done < counts[s]; done += DIB_GRAD_TILE) {
      tiles[k].start = offsets[s] + done;
      tiles[k].count = (int32_t)std::min<int64_t>(DIB_GRAD_TILE, counts[s] - done);
      tiles[k].segment = s;
      ++k;
    }
  }
  seg_tile0[n_segments] = (int32_t)k;
  return total;
}

int dib_grad_sumsq(const dib_grad_table* table, int seg_first, int seg_count, const float* grads, float grad_scale, float clipvalue,
                   double* partials, double* ss, dib_stream_t stream) {
  int tile_first = 0, tile_count = 0;
  if (int rc = gt_check_range(table, seg_first, seg_count, &tile_first, &tile_count)) return rc;
  if (!grads || !partials || !ss || !gt_aligned(grads, 16) || !gt_aligned(partials, 8) || !gt_aligned(ss, 8)) return DIB_E_ARG;
  if (!gt_clipvalue_ok(clipvalue)) return DIB_E_ARG;
  if (seg_count == 0) return DIB_OK;
  if (!table->seg_tile0_dev) return DIB_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(kProfOther, st);
  if (tile_count > 0)
    DIB_LAUNCH(dib_grad_sumsq_tile_kernel, dim3(tile_count), dim3(256), 0, st, (const DibGradTile*)table->tiles_dev, tile_first,
               grads, grad_scale, clipvalue, partials);
  // (segments without elements have no tile: the finish kernel writes their ss = 0)
  DIB_LAUNCH(dib_grad_sumsq_finish_kernel, dim3(cdiv(seg_count, 256)), dim3(256), 0, st, (const int*)table->seg_tile0_dev,
             seg_first, seg_count, (const double*)partials, ss);
  return (int)hipGetLastError();
}

int dib_grad_clip_apply(const dib_grad_table* table, int seg_first, int seg_count, float* grads, float grad_scale, float clipvalue,
                        int mode, float norm, const double* ss, const double* ss_all, int n_ss, dib_stream_t stream) {
  int tile_first = 0, tile_count = 0;
  if (int rc = gt_check_range(table, seg_first, seg_count, &tile_first, &tile_count)) return rc;
  if (!grads || !gt_aligned(grads, 16) || !gt_clipvalue_ok(clipvalue)) return DIB_E_ARG;
  if (mode == DIB_CLIP_NONE) {
    if (!(clipvalue > 0.f)) return DIB_E_ARG;   // nothing to apply
  } else if (mode == DIB_CLIP_NORM) {
    if (!(norm > 0.f) || !std::isfinite(norm) || !ss || !gt_aligned(ss, 8)) return DIB_E_ARG;
  } else if (mode == DIB_CLIP_GLOBAL_NORM) {
    if (!(norm > 0.f) || !std::isfinite(norm) || !ss_all || !gt_aligned(ss_all, 8) || n_ss <= 0) return DIB_E_ARG;
  } else {
    return DIB_E_ARG;
  }
  if (tile_count == 0) return DIB_OK;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(kProfOther, st);
  const DibGradClip c{grad_scale, clipvalue, mode == DIB_CLIP_NONE ? 0.f : norm, mode};
  DIB_LAUNCH(dib_grad_clip_apply_kernel, dim3(tile_count), dim3(256), 0, st, (const DibGradTile*)table->tiles_dev, tile_first, grads,
             c, ss, ss_all, n_ss);
  return (int)hipGetLastError();
}

int dib_lr_schedule_check(const dib_lr_schedule* s) {
  if (!s || !std::isfinite(s->initial)) return DIB_E_ARG;
  const bool steps_ok = s->decay_steps > 0.f && std::isfinite(s->decay_steps);
  switch (s->kind) {
    case DIB_LR_INVERSE_DECAY: return (s->rate >= 0.f && std::isfinite(s->rate)) ? DIB_OK : DIB_E_ARG;
    case DIB_LR_EXPONENTIAL: return (steps_ok && s->rate >= 0.f && std::isfinite(s->rate)) ? DIB_OK : DIB_E_ARG;
    case DIB_LR_INVERSE_TIME: return (steps_ok && s->rate >= 0.f && std::isfinite(s->rate)) ? DIB_OK : DIB_E_ARG;
    case DIB_LR_POLYNOMIAL: return (steps_ok && std::isfinite(s->end) && std::isfinite(s->power) && s->power > 0.f) ? DIB_OK : DIB_E_ARG;
    case DIB_LR_COSINE: return (steps_ok && std::isfinite(s->alpha)) ? DIB_OK : DIB_E_ARG;
    case DIB_LR_PIECEWISE:
      if (s->n_boundaries < 1 || s->n_boundaries > DIB_LR_MAX_BOUNDARIES) return DIB_E_ARG;
      for (int i = 0; i <= s->n_boundaries; ++i)
        if (!std::isfinite(s->values[i])) return DIB_E_ARG;
      for (int i = 1; i < s->n_boundaries; ++i)
        if (s->boundaries[i] <= s->boundaries[i - 1]) return DIB_E_ARG;
      return DIB_OK;
    default: return DIB_E_ARG;
  }
}

int dib_lr_schedule_eval(const dib_lr_schedule* s, const int64_t* t_dev, float* lr_dev, dib_stream_t stream) {
  if (int rc = dib_lr_schedule_check(s)) return rc;
  if (!t_dev || !lr_dev || !gt_aligned(t_dev, 8) || !gt_aligned(lr_dev, 4)) return DIB_E_ARG;
  DibLrSchedule d;
  std::memcpy(&d, s, sizeof(d));
  ProfScope ps(kProfOther, (hipStream_t)stream);
  DIB_LAUNCH(dib_lr_schedule_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, d, (const long long*)t_dev, lr_dev);
  return (int)hipGetLastError();
}

}  // extern "C"
