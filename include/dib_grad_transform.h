/* dib_grad_transform.h - C ABI of what Keras optimizer_v2 does to the gradient and to the learning rate BEFORE the update rule
 * sees them: clipvalue, clipnorm (per variable), global_clipnorm (over all variables), the legacy `decay` and the learning-rate
 * schedules.  TensorFlow is not a dependency of this project: the semantics are pinned to the statement below and to
 * its float64 restatement in tests/_oracle_grad_transforms.py, not to an executed reference.
 *
 * With g = grads[i] * grad_scale (float32), in this order:
 *   clipvalue c > 0        g = min(max(g, -c), c)
 *   clipnorm c > 0         per variable: ss = sum g^2 (float64), n = ss > 0 ? (float)sqrt(ss) : 0, g = (g * c) / max(n, c)
 *   global_clipnorm c > 0  N = (float)sqrt(sum of every ss given, in index order), scale = c * min(1 / N, 1 / c) + (N - N),
 *                          g = g * scale.  (N - N) is 0 for a finite N and NaN otherwise: a non-finite norm makes every
 *                          gradient NaN, as tf.clip_by_global_norm does.)
 * clipnorm and global_clipnorm exclude each other; clipvalue combines with either.  The gradient buffer is rewritten IN PLACE
 * with grad_scale folded in: the update that follows is called with grad_scale = 1.
 *
 * The variable table.  A variable is one contiguous segment (offset, count) of a flat fp32 buffer; the elements between
 * segments (alignment gaps) belong to none and are neither read nor written.  dib_grad_table_from_layout lists the segments of a
 * dib_layout - one per Dense kernel or bias, in the order (net, layer, feature, what) of dib_layout_param_block, so that every
 * gradient bucket of dib_layout_part_range is one contiguous range of segments; any other buffer passes its own (offset, count)
 * arrays.  dib_grad_table_tiles cuts every segment, from its start, into tiles of at most DIB_GRAD_TILE elements (one workgroup
 * each) and fills seg_tile0[s] = index of segment s's first tile, seg_tile0[n_segments] = number of tiles.  Both are host-only
 * (callable without a GPU, like dib_optimizer_slots).  The caller uploads `tiles` and `seg_tile0` once and describes the three
 * arrays in a dib_grad_table.  The cut depends on the table alone - never on the range a call covers or on a grid size - so
 * reducing a buffer in ranges (gradient buckets), in any order, gives the bits of reducing it whole.
 *
 * dib_grad_sumsq (two launches): ss[s] = sum (clip(grads[i] * grad_scale))^2 for the segments [seg_first, seg_first + seg_count):
 * one workgroup per tile accumulates in float64 in a fixed order (no atomics) into partials[tile]; one thread per segment then
 * adds its tiles' partials in index order.  `partials` (n_tiles doubles) and `ss` (n_segments doubles) are indexed by the
 * table's own tile / segment numbers; the ss arrays of several buffers may be slices of one device array, which the global mode
 * of dib_grad_clip_apply then sums as a whole.  clipvalue = 0: no value clip.
 * dib_grad_clip_apply (one launch): the transformed g for the tiles of the same kind of range.  mode DIB_CLIP_NONE (clipvalue
 * alone; ss unused), DIB_CLIP_NORM (reads ss[s] of the table's segment numbers), DIB_CLIP_GLOBAL_NORM (reads ss_all[0 .. n_ss)).
 * dib_lr_schedule_eval (one thread): *lr_dev = schedule(*t_dev) in float32 - `iterations`, the step count BEFORE this step's
 * increment - so a captured step replays with an advancing learning rate.  Launch it before the step's first reader of lr_dev.
 *
 * Every entry returns int, never allocates, never synchronises, reads nothing from the environment and can be captured into a
 * hipGraph; the caller owns every buffer.  DIB_E_ARG: a NULL table / array / pointer the mode needs, a range outside the table,
 * grads not 16-byte aligned, partials / ss not 8-byte aligned, a threshold that is not > 0 (clipvalue: < 0), clipvalue / norm
 * not finite, an unknown mode or schedule kind, a schedule whose fields are out of range (dib_lr_schedule_check says which
 * are).  A refused call launches nothing and writes nothing; a range without elements is DIB_OK without a launch.
 * Part of libdib_hip.so; additions only within DIB_ABI_VERSION 7 of dib_hip.h. */
#ifndef DIB_GRAD_TRANSFORM_H
#define DIB_GRAD_TRANSFORM_H
#include <stdint.h>
#include "dib_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DIB_GRAD_TILE 4096   /* elements of one tile: 256 threads x 4 float4 */

#define DIB_CLIP_NONE 0
#define DIB_CLIP_NORM 1
#define DIB_CLIP_GLOBAL_NORM 2

typedef struct dib_grad_tile {
  int64_t start;     /* first element, in floats from the buffer's base */
  int32_t count;     /* 1 .. DIB_GRAD_TILE */
  int32_t segment;   /* the variable it is part of */
} dib_grad_tile;

typedef struct dib_grad_table {
  int32_t n_segments;
  int32_t reserved;                /* 0 */
  int64_t n_tiles;
  const int32_t* seg_tile0;        /* HOST, n_segments + 1 */
  const dib_grad_tile* tiles_dev;  /* device, n_tiles */
  const int32_t* seg_tile0_dev;    /* device, n_segments + 1 */
} dib_grad_table;

/* number of variables of the layout (DIB_E_ARG: NULL); fills offsets / counts [capacity >= that number] when both are given */
int dib_grad_table_from_layout(const dib_layout* l, int64_t* offsets, int64_t* counts, int capacity);
/* number of tiles (>= 0) or DIB_E_ARG: a negative offset or count, a segment past buffer_elems, two segments that overlap, more
 * than 2^31 - 1 tiles, tile_capacity too small.  tiles == NULL and seg_tile0 == NULL: only counts. */
int64_t dib_grad_table_tiles(const int64_t* offsets, const int64_t* counts, int n_segments, int64_t buffer_elems,
                             dib_grad_tile* tiles, int64_t tile_capacity, int32_t* seg_tile0);

int dib_grad_sumsq(const dib_grad_table* table, int seg_first, int seg_count, const float* grads, float grad_scale, float clipvalue,
                   double* partials, double* ss, dib_stream_t stream);
int dib_grad_clip_apply(const dib_grad_table* table, int seg_first, int seg_count, float* grads, float grad_scale, float clipvalue,
                        int mode, float norm, const double* ss, const double* ss_all, int n_ss, dib_stream_t stream);

#define DIB_LR_INVERSE_DECAY 1   /* legacy `decay`: initial / (1 + rate * step) */
#define DIB_LR_EXPONENTIAL 2     /* initial * rate^p, p = step / decay_steps (floored: DIB_LR_STAIRCASE) */
#define DIB_LR_INVERSE_TIME 3    /* initial / (1 + rate * p) */
#define DIB_LR_POLYNOMIAL 4      /* (initial - end) * (1 - step / decay_steps)^power + end; step = min(step, decay_steps), or with
                                    DIB_LR_CYCLE decay_steps *= max(1, ceil(step / decay_steps)) */
#define DIB_LR_PIECEWISE 5       /* values[i] for boundaries[i - 1] < step <= boundaries[i]; values[n_boundaries] beyond */
#define DIB_LR_COSINE 6          /* initial * ((1 - alpha) * 0.5 * (1 + cos(pi * step / decay_steps)) + alpha), step = min(step, decay_steps) */
#define DIB_LR_STAIRCASE 1
#define DIB_LR_CYCLE 2
#define DIB_LR_MAX_BOUNDARIES 8

typedef struct dib_lr_schedule {
  int32_t kind;
  int32_t flags;
  float initial;
  float decay_steps;   /* > 0 where the kind divides by it */
  float rate;          /* decay_rate; `decay` for DIB_LR_INVERSE_DECAY */
  float end;           /* polynomial */
  float power;         /* polynomial */
  float alpha;         /* cosine */
  int32_t n_boundaries;
  int32_t reserved;    /* 0 */
  int64_t boundaries[DIB_LR_MAX_BOUNDARIES];   /* strictly increasing */
  float values[DIB_LR_MAX_BOUNDARIES + 1];
  float reserved2;     /* 0 */
} dib_lr_schedule;

int dib_lr_schedule_check(const dib_lr_schedule* s);   /* host-only: DIB_OK or DIB_E_ARG */
int dib_lr_schedule_eval(const dib_lr_schedule* s, const int64_t* t_dev, float* lr_dev, dib_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIB_GRAD_TRANSFORM_H */
