// dib_ctw_levels.h - the context-tree-weighting (CTW) entropy-rate estimator built level by level on the device
// (include/dib_ctw_device.h; the host estimator is csrc/dib_ctw.cpp).
//
// The tree csrc/dib_ctw.cpp builds position by position does not depend on the order of insertion (DESIGN.md "CTW on the
// device"): with x[0..N) a window, position t has symbol x[t] and context x[t-1], x[t-2], ..., x[0];
//   - level 0 is the root, its group is every position;
//   - a member t of a group at level d moves to level d + 1 iff t > d and (d = 0 or the group has >= 2 members); the movers of a
//     group split by x[t-d-1], every non-empty part is a child; a node's counts[s] = the number of its members with x[t] = s.
// All windows of a call are built together (a root per window).  A child of ONE member is a leaf whose code length is the same
// constant for every symbol (lgamma(0 + beta) - lgamma(beta) = 0 exactly), so only nodes with >= 2 members ("big" nodes; every
// root counts as one) get an id, a record and a segment of the element list; a leaf is two bits in its parent's mask.
//
// A level step d -> d + 1 over the list of (t, node) pairs, grouped by node (node ids ascend along the list):
//   count     hist_sym[node][x[t]] += 1 for every element, hist_ctx[node][x[t-d-1]] += 1 for every mover: integer atomics, folded
//             in LDS over the keys of the nodes a workgroup's 1024 elements span when those are <= 4096 (always for A <= 8: a big
//             node has >= 2 elements), one global atomic per non-zero key and workgroup; past that straight to global memory (the
//             keys are then spread).  Level 512 counts no contexts: a mover there marks its window DEEP instead.
//   scan      one thread per node: exclusive sums over the keys, in key order, of [child is big] and of the big children's sizes
//             (reduce per workgroup, one workgroup scans the workgroup sums, finalize rescans locally) = the ids of the next
//             level's nodes (siblings contiguous, in symbol order) and the offsets of their segments.  Finalize also turns
//             hist_sym into the node's local code length L_e with the host's expression, term by term and in its order (lgamma
//             from the host's table below 65 536, the device's lgamma beyond), and writes the node's record.
//   place     every mover into its child's segment: slot = segment offset + rank, the rank from an LDS atomic and one global
//             atomic per key and workgroup (or one per element past the LDS fold).  The order inside a segment is arbitrary and
//             no result depends on it: every output is a function of integer counts.
// Bottom-up, deepest level first: one thread per node sums its children's L_w serially in symbol order (float64) and applies the
// mixture; it also sums the subtree's node count.  No float atomics anywhere; the doubles depend on the counts alone, so they do
// not depend on the launch, the chunk of windows or the run.
#pragma once
#include "dib_common.h"

#define DIB_CTW_THREADS 256
#define DIB_CTW_TILE 1024               // elements of the list per workgroup in count / place (4 per lane)
#define DIB_CTW_LDS_KEYS 4096           // keys a workgroup folds in LDS
#define DIB_CTW_LAST_LEVEL 512          // csrc/dib_ctw.cpp kMaxDepth
#define DIB_CTW_TABLE 65536             // lgamma table entries (csrc/dib_ctw.cpp kMemo)
#define DIB_CTW_ST_DEEP 1               // include/dib_ctw_device.h status bits
#define DIB_CTW_ST_OVERFLOW 2
#define DIB_CTW_ST_BAD_SYMBOL 4

struct DibCtwParams {
  int A, W;
  double beta, ab, lg_ab, lg_b, ln2, leaf;   // leaf: L_e = L_w of a node with one member
};

struct DibCtwLevelRec {   // what the host reads back per level
  int next_nodes, next_elems, overflow, reserved;
};

// ---- the list of level 0: every position of every window, node = the window's root -----------------------------------------------
__global__ __launch_bounds__(DIB_CTW_THREADS) void dib_ctw_init_kernel(const int* __restrict__ win_off, int W, int E,
                                                                       int* __restrict__ el_t, int* __restrict__ el_node,
                                                                       int* __restrict__ node_win, int* __restrict__ status) {
  const long long at = (long long)blockIdx.x * DIB_CTW_THREADS + threadIdx.x;
  if (at < W) {
    node_win[at] = (int)at;
    status[at] = 0;
  }
  if (at >= E) return;
  const int i = (int)at;
  int lo = 0, hi = W - 1;   // the last window with win_off[w] <= i (empty windows share an offset with their successor)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (win_off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  el_t[i] = i - win_off[lo];
  el_node[i] = lo;
}

// the first node of the elements [base, base + TILE) of the list, and the keys of the nodes they span when those fit the LDS
// fold (0: they do not)
__device__ __forceinline__ int dib_ctw_tile_keys(const int* __restrict__ el_node, int base, int M, int A, int& n0) {
  n0 = el_node[base];
  const int n1 = el_node[(M - base > DIB_CTW_TILE ? base + DIB_CTW_TILE : M) - 1];
  const long long keys = (long long)(n1 - n0 + 1) * A;
  return keys <= DIB_CTW_LDS_KEYS ? (int)keys : 0;
}

__global__ __launch_bounds__(DIB_CTW_THREADS) void dib_ctw_count_kernel(
    const unsigned char* __restrict__ x, const long long* __restrict__ win_start, const int* __restrict__ el_t,
    const int* __restrict__ el_node, const int* __restrict__ node_win, int M, int d, int A, int last_level,
    int* __restrict__ hist_sym, int* __restrict__ hist_ctx, int* __restrict__ status) {
  __shared__ int lds_sym[DIB_CTW_LDS_KEYS], lds_ctx[DIB_CTW_LDS_KEYS];
  const int tid = threadIdx.x, base = blockIdx.x * DIB_CTW_TILE;
  int n0;
  const int keys = dib_ctw_tile_keys(el_node, base, M, A, n0);
  const bool fold = keys > 0;
  for (int k = tid; k < keys; k += DIB_CTW_THREADS) {
    lds_sym[k] = 0;
    lds_ctx[k] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < DIB_CTW_TILE / DIB_CTW_THREADS; ++j) {
    const int i = base + j * DIB_CTW_THREADS + tid;   // base + TILE - 1 < 2^31
    if (i < M) {
      const int t = el_t[i], n = el_node[i], w = node_win[n];
      const unsigned char* xs = x + win_start[w];
      int s = xs[t];
      if (d == 0 && s >= A) atomicOr(&status[w], DIB_CTW_ST_BAD_SYMBOL);
      s = min(s, A - 1);
      const bool mover = t > d;
      if (fold) atomicAdd(&lds_sym[(n - n0) * A + s], 1);
      else atomicAdd(&hist_sym[(size_t)n * A + s], 1);
      if (mover && last_level) {
        if (!(status[w] & DIB_CTW_ST_DEEP)) atomicOr(&status[w], DIB_CTW_ST_DEEP);
      } else if (mover) {
        const int c = min((int)xs[t - d - 1], A - 1);
        if (fold) atomicAdd(&lds_ctx[(n - n0) * A + c], 1);
        else atomicAdd(&hist_ctx[(size_t)n * A + c], 1);
      }
    }
  }
  __syncthreads();
  for (int k = tid; k < keys; k += DIB_CTW_THREADS) {
    const int vs = lds_sym[k], vc = lds_ctx[k];
    if (vs) atomicAdd(&hist_sym[(size_t)n0 * A + k], vs);
    if (vc) atomicAdd(&hist_ctx[(size_t)n0 * A + k], vc);
  }
}

// ---- scan over the keys, one thread per node -----------------------------------------------------------------------------------
// (x, y) = (number of big children, their elements) of node n
__device__ __forceinline__ int2 dib_ctw_node_sums(const int* __restrict__ hist_ctx, int n, int A) {
  int2 s = make_int2(0, 0);
  const int* row = hist_ctx + (size_t)n * A;
  for (int c = 0; c < A; ++c) {
    const int v = row[c];
    if (v >= 2) {
      s.x += 1;
      s.y += v;
    }
  }
  return s;
}

// exclusive scan of one int2 per lane over the workgroup; total = the workgroup's sum (every lane)
__device__ __forceinline__ int2 dib_ctw_block_scan(int2 v, int2& total) {
  __shared__ int2 wave_sum[DIB_CTW_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int2 inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int ux = __shfl_up(inc.x, o, 64), uy = __shfl_up(inc.y, o, 64);
    if (lane >= o) {
      inc.x += ux;
      inc.y += uy;
    }
  }
  if (lane == 63) wave_sum[wave] = inc;
  __syncthreads();
  int2 before = make_int2(0, 0);
  total = make_int2(0, 0);
#pragma unroll
  for (int k = 0; k < DIB_CTW_THREADS / 64; ++k) {
    const int2 ws = wave_sum[k];
    if (k < wave) {
      before.x += ws.x;
      before.y += ws.y;
    }
    total.x += ws.x;
    total.y += ws.y;
  }
  __syncthreads();
  return make_int2(before.x + inc.x - v.x, before.y + inc.y - v.y);
}

__global__ __launch_bounds__(DIB_CTW_THREADS) void dib_ctw_scan_reduce_kernel(const int* __restrict__ hist_ctx, int nb, int A,
                                                                              int2* __restrict__ block_sums) {
  const int n = blockIdx.x * DIB_CTW_THREADS + threadIdx.x;
  const int2 v = n < nb ? dib_ctw_node_sums(hist_ctx, n, A) : make_int2(0, 0);
  int2 total;
  dib_ctw_block_scan(v, total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// one workgroup: block_sums -> their exclusive scan, in place; the level's record
__global__ __launch_bounds__(1024) void dib_ctw_scan_blocks_kernel(int2* __restrict__ block_sums, int n_blocks, long long next_base,
                                                                   long long node_capacity, int level_capacity,
                                                                   DibCtwLevelRec* __restrict__ rec) {
  __shared__ int2 part[1024];
  __shared__ int2 carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = make_int2(0, 0);
  __syncthreads();
  for (int b0 = 0; b0 < n_blocks; b0 += 1024) {
    const int b = b0 + tid;
    const int2 v = b < n_blocks ? block_sums[b] : make_int2(0, 0);
    part[tid] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {   // Hillis-Steele, inclusive
      int2 u = make_int2(0, 0);
      if (tid >= o) u = part[tid - o];
      __syncthreads();
      part[tid].x += u.x;
      part[tid].y += u.y;
      __syncthreads();
    }
    const int2 c = carry, inc = part[tid];
    if (b < n_blocks) block_sums[b] = make_int2(c.x + inc.x - v.x, c.y + inc.y - v.y);
    __syncthreads();
    if (tid == 1023) carry = make_int2(c.x + inc.x, c.y + inc.y);
    __syncthreads();
  }
  if (tid == 0) {
    const int2 c = carry;
    rec->next_nodes = c.x;
    rec->next_elems = c.y;
    rec->overflow = (next_base + c.x > node_capacity || c.x > level_capacity) ? 1 : 0;
    rec->reserved = 0;
  }
}

// lgamma(k + offset) for a count k: the host's table below DIB_CTW_TABLE, the device's lgamma beyond
__device__ __forceinline__ double dib_ctw_lgamma(const double* __restrict__ table, int k, double offset) {
  return k < DIB_CTW_TABLE ? table[k] : lgamma((double)k + offset);
}

// the records of the level's nodes; per key the child's segment offset (-1: no big child) and id within the next level
__global__ __launch_bounds__(DIB_CTW_THREADS) void dib_ctw_finalize_kernel(
    const int* __restrict__ hist_sym, const int* __restrict__ hist_ctx, const int2* __restrict__ block_sums, int nb,
    DibCtwParams p, const double* __restrict__ table_beta, const double* __restrict__ table_ab, const DibCtwLevelRec* __restrict__ rec,
    long long node_base, long long next_base, const int* __restrict__ node_win, int* __restrict__ next_win,
    int2* __restrict__ key_info, double* __restrict__ node_L, unsigned* __restrict__ node_mask, int* __restrict__ node_first,
    int* __restrict__ status) {
  const int n = blockIdx.x * DIB_CTW_THREADS + threadIdx.x, A = p.A;
  const int2 v = n < nb ? dib_ctw_node_sums(hist_ctx, n, A) : make_int2(0, 0);
  int2 total;
  int2 at = dib_ctw_block_scan(v, total);
  if (n >= nb) return;
  const int2 off = block_sums[blockIdx.x];
  at.x += off.x;
  at.y += off.y;
  const bool overflow = rec->overflow != 0;
  const int w = node_win[n];
  // local code length: csrc/dib_ctw.cpp ContextTree::rate, expression by expression
  const int* sym = hist_sym + (size_t)n * A;
  int tot = 0;
  for (int s = 0; s < A; ++s) tot += sym[s];
  double local = dib_ctw_lgamma(table_ab, tot, p.ab) - p.lg_ab;
  for (int s = 0; s < A; ++s) local -= dib_ctw_lgamma(table_beta, sym[s], p.beta) - p.lg_b;
  local /= p.ln2;
  unsigned mask = 0;
  bool any = false;
  const int* ctx = hist_ctx + (size_t)n * A;
  const int first = at.x;
  for (int c = 0; c < A; ++c) {
    const int size = ctx[c];
    int2 info = make_int2(-1, 0);
    if (size > 0) any = true;
    if (!overflow) {
      if (size == 1) mask |= 1u << (2 * c);
      if (size >= 2) {
        mask |= 2u << (2 * c);
        info = make_int2(at.y, at.x);
        next_win[at.x] = w;
        at.x += 1;
        at.y += size;
      }
    }
    key_info[(size_t)n * A + c] = info;
  }
  if (overflow && any) atomicOr(&status[w], DIB_CTW_ST_OVERFLOW);
  node_L[node_base + n] = local;
  node_mask[node_base + n] = mask;
  node_first[node_base + n] = (int)(next_base + first);
}

__global__ __launch_bounds__(DIB_CTW_THREADS) void dib_ctw_place_kernel(
    const unsigned char* __restrict__ x, const long long* __restrict__ win_start, const int* __restrict__ el_t,
    const int* __restrict__ el_node, const int* __restrict__ node_win, int M, int d, int A, const DibCtwLevelRec* __restrict__ rec,
    int* __restrict__ hist_ctx, const int2* __restrict__ key_info, int* __restrict__ out_t, int* __restrict__ out_node) {
  __shared__ int lds_cnt[DIB_CTW_LDS_KEYS];
  if (rec->overflow) return;   // uniform
  const int tid = threadIdx.x, base = blockIdx.x * DIB_CTW_TILE;
  int n0;
  const int keys = dib_ctw_tile_keys(el_node, base, M, A, n0);
  const bool fold = keys > 0;
  for (int k = tid; k < keys; k += DIB_CTW_THREADS) lds_cnt[k] = 0;
  __syncthreads();
  int t[DIB_CTW_TILE / DIB_CTW_THREADS], rank[DIB_CTW_TILE / DIB_CTW_THREADS];
  long long key[DIB_CTW_TILE / DIB_CTW_THREADS];
#pragma unroll
  for (int j = 0; j < DIB_CTW_TILE / DIB_CTW_THREADS; ++j) {
    const int i = base + j * DIB_CTW_THREADS + tid;
    key[j] = -1;
    if (i < M) {
      t[j] = el_t[i];
      if (t[j] > d) {
        const int n = el_node[i];
        const int c = min((int)x[win_start[node_win[n]] + t[j] - d - 1], A - 1);
        const long long k = (long long)n * A + c;
        if (key_info[k].x >= 0) {   // the child is big: it has a segment
          key[j] = k;
          rank[j] = fold ? atomicAdd(&lds_cnt[(n - n0) * A + c], 1) : atomicSub(&hist_ctx[k], 1) - 1;
        }
      }
    }
  }
  __syncthreads();
  // this workgroup's run of slots in every child it feeds: hist_ctx counts down from the child's size
  for (int k = tid; k < keys; k += DIB_CTW_THREADS) {
    const int cnt = lds_cnt[k];
    if (cnt) lds_cnt[k] = atomicSub(&hist_ctx[(size_t)n0 * A + k], cnt) - cnt;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < DIB_CTW_TILE / DIB_CTW_THREADS; ++j) {
    if (key[j] >= 0) {
      const int2 info = key_info[key[j]];
      const int slot = info.x + rank[j] + (fold ? lds_cnt[(int)(key[j] - (long long)n0 * A)] : 0);
      out_t[slot] = t[j];
      out_node[slot] = info.y;
    }
  }
}

// ---- bottom-up: the mixture of one level's nodes (their children are final) -------------------------------------------------------
__global__ __launch_bounds__(DIB_CTW_THREADS) void dib_ctw_mix_kernel(long long node_base, int nb, int A, double leaf,
                                                                      double* __restrict__ node_L, const unsigned* __restrict__ node_mask,
                                                                      const int* __restrict__ node_first,
                                                                      long long* __restrict__ node_count) {
  const int n = blockIdx.x * DIB_CTW_THREADS + threadIdx.x;
  if (n >= nb) return;
  const long long id = node_base + n;
  const unsigned mask = node_mask[id];
  long long count = 1;
  if (mask != 0u) {   // a node with a child has more than one member
    const double local = node_L[id];
    long long child = node_first[id];
    double kids = 0;
    for (int c = 0; c < A; ++c) {
      const unsigned st = (mask >> (2 * c)) & 3u;
      if (st == 1u) {
        kids += leaf;
        count += 1;
      } else if (st == 2u) {
        kids += node_L[child];
        count += node_count[child];
        ++child;
      }
    }
    node_L[id] = 1 + fmin(kids, local) - log2(1 + exp2(-fabs(local - kids)));
  }
  node_count[id] = count;
}

__global__ __launch_bounds__(DIB_CTW_THREADS) void dib_ctw_output_kernel(const double* __restrict__ node_L,
                                                                         const long long* __restrict__ node_count,
                                                                         const int* __restrict__ win_len, const int* __restrict__ ws_status,
                                                                         int W, double* __restrict__ code_bits, double* __restrict__ rates,
                                                                         long long* __restrict__ nodes, int* __restrict__ status) {
  const int w = blockIdx.x * DIB_CTW_THREADS + threadIdx.x;
  if (w >= W) return;
  const double L = node_L[w];   // the roots are the nodes 0 .. W-1
  code_bits[w] = L;
  rates[w] = (double)(float)(L / (double)win_len[w]);   // 0 / 0 = NaN for an empty window, as on the host
  nodes[w] = node_count[w];
  status[w] = ws_status[w];
}
