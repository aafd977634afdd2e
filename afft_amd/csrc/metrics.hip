// Training / evaluation metrics on the device: the rank of the label's score among the scores of its row, and the integer
// counters of the mean top-k recall; the row-wise sorted top-k of the submission path (afft_topk_rows).  Semantics: common/runner.py:54-92 (MixUp adjustment of the logits, acc1 / acc5 through
// common/utils.py:59-86) and common/metric_tracking.py:22-29 (per-class true positives / counts); tie rule and the handling
// of labels outside [0, C) are this project's (include/afft_hip.h).
#include "common.h"

namespace {

// (value, class) candidates of an arg-max; idx < 0 = no candidate.  Among equal values the LOWER class index wins.
struct Cand { float v; int i; };
__device__ __forceinline__ Cand better(Cand a, Cand b) {
  if (b.i < 0) return a;
  if (a.i < 0) return b;
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
__device__ __forceinline__ Cand block_argmax(Cand c, Cand* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Cand t;
    t.v = __shfl_xor(c.v, o, 64);
    t.i = __shfl_xor(c.i, o, 64);
    c = better(c, t);
  }
  __syncthreads();
  if (lane == 0) sh[wave] = c;
  __syncthreads();
  Cand r = sh[0];
  for (int w = 1; w < 4; ++w) r = better(r, sh[w]);
  return r;
}
__device__ __forceinline__ int block_sum_int(int v, int* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// fn(c, row[c]) for every c in [0, C), thread-strided; 16-byte loads where the row allows them (vec: host-verified alignment)
template <typename Fn>
__device__ __forceinline__ void walk_row(const float* __restrict__ x, int C, bool vec, Fn fn) {
  const int tid = threadIdx.x;
  if (vec) {
    const int C4 = C & ~3;
    for (int c = tid * 4; c < C4; c += 1024) {
      const f32x4 v = *(const f32x4*)(x + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) fn(c + e, v[e]);
    }
    for (int c = C4 + tid; c < C; c += 256) fn(c, x[c]);
  } else {
    for (int c = tid; c < C; c += 256) fn(c, x[c]);
  }
}

// One workgroup per row.  Hard labels: the scores are the logits.  Soft targets: i1 = arg-max of the target row, i2 = arg-max
// over c != i1, scores = logits with s[i1] += s[i2], then s[i2] = 0, label = i1; the adjusted row exists in registers only.
__global__ __launch_bounds__(256) void label_rank_kernel(const float* __restrict__ logits, int64_t row_stride, int C,
                                                         const int64_t* __restrict__ labels, const float* __restrict__ soft,
                                                         int64_t lds, int vec_x, int vec_t, int32_t* __restrict__ rank,
                                                         int64_t* __restrict__ label_out) {
  __shared__ Cand shc[4];
  __shared__ int shi[4];
  const int64_t row = blockIdx.x;
  const float* x = logits + row * row_stride;
  int64_t lab;
  int i1 = -1, i2 = -1;
  if (soft) {
    const float* t = soft + row * lds;
    Cand a = {0.f, -1}, b = {0.f, -1};      // this thread's best and second best target
    walk_row(t, C, vec_t != 0, [&](int c, float v) {
      const Cand n = {v, c};
      // candidates arrive in ascending class order, so an equal value never displaces an earlier one
      if (a.i < 0 || v > a.v) { b = a; a = n; }
      else if (b.i < 0 || v > b.v) b = n;
    });
    const Cand top = block_argmax(a, shc);
    i1 = top.i;
    const Cand second = block_argmax(a.i == i1 ? b : a, shc);
    i2 = second.i;      // -1 when C == 1: nothing to fold in
    lab = i1;
  } else {
    lab = labels[row];
  }
  const bool valid = lab >= 0 && lab < C;       // uniform per block
  if (!valid) {      // never a hit; nothing is read at the label's position
    if (threadIdx.x == 0) { rank[row] = C; label_out[row] = lab; }
    return;
  }
  const int l = (int)lab;
  const float folded = i2 >= 0 ? x[i1] + x[i2] : 0.f;      // i2 >= 0: soft targets, and l == i1
  const float sl = i2 >= 0 ? folded : x[l];
  int n = 0;
  walk_row(x, C, vec_x != 0, [&](int c, float v) {
    if (i2 >= 0) v = c == i2 ? 0.f : c == i1 ? folded : v;
    n += (c != l && (v > sl || (v == sl && c < l))) ? 1 : 0;
  });
  n = block_sum_int(n, shi);
  if (threadIdx.x == 0) { rank[row] = n; label_out[row] = lab; }
}

// acc[0] = #{rank < 1} * scale, acc[1] = #{rank < k} * scale: one workgroup, integer counts
__global__ __launch_bounds__(256) void rank_hits_kernel(const int32_t* __restrict__ rank, int rows, int k, float scale,
                                                        float* __restrict__ acc) {
  __shared__ int shi[4];
  int h1 = 0, hk = 0;
  for (int64_t r = threadIdx.x; r < rows; r += 256) {
    const int v = rank[r];
    h1 += v < 1 ? 1 : 0;
    hk += v < k ? 1 : 0;
  }
  h1 = block_sum_int(h1, shi);
  hk = block_sum_int(hk, shi);
  if (threadIdx.x == 0) { acc[0] = (float)h1 * scale; acc[1] = (float)hk * scale; }
}

__global__ __launch_bounds__(256) void recall_accumulate_kernel(const int32_t* __restrict__ rank, const int64_t* __restrict__ label,
                                                                int rows, int C, int k, int32_t* __restrict__ tps,
                                                                int32_t* __restrict__ nums) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const int64_t l = label[r];
  if (l < 0 || l >= C) return;
  atomicAdd(nums + l, 1);
  if (rank[r] < k) atomicAdd(tps + l, 1);
}

// ----------------------------------------------------------------------------- late-fusion weight search (afft_fused_label_rank)
// WT weight sets share one pass over the n rows.  The accumulation is weighted_sum_fwd_kernel's (elementwise.hip) with the contraction
// hipcc applies there written out: s = 0, then s = fma(w[i], x_i, s) in run order (v_fmac_f32 in the built library).
constexpr int FLR_WT = 8;
struct FusePtrs { const float* x[8]; };

template <int N>
__device__ __forceinline__ float fuse_scores(const float (&w)[N], const float (&x)[N]) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) s = __fmaf_rn(w[i], x[i], s);
  return s;
}

// walk_row over N rows at once: fn(c, {x_0[c], ..., x_{N-1}[c]}) for every c in [0, C), the same 16-byte / scalar split
template <int N, typename Fn>
__device__ __forceinline__ void walk_rows(const float* const (&x)[N], int C, bool vec, Fn fn) {
  const int tid = threadIdx.x;
  float v[N];
  if (vec) {
    const int C4 = C & ~3;
    for (int64_t c = tid * 4; c < C4; c += 1024) {      // 64-bit: c + 1024 may pass 2^31 on the last trip
      f32x4 q[N];
#pragma unroll
      for (int i = 0; i < N; ++i) q[i] = *(const f32x4*)(x[i] + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = q[i][e];
        fn((int)c + e, v);
      }
    }
    for (int64_t c = C4 + tid; c < C; c += 256) {
#pragma unroll
      for (int i = 0; i < N; ++i) v[i] = x[i][c];
      fn((int)c, v);
    }
  } else {
    for (int64_t c = tid; c < C; c += 256) {
#pragma unroll
      for (int i = 0; i < N; ++i) v[i] = x[i][c];
      fn((int)c, v);
    }
  }
}

// One workgroup per (row, tile of FLR_WT weight sets).  The weights and the label scores depend on blockIdx only (wave-uniform: the
// weights are read by scalar loads and stay in SGPRs); per lane: the N x 4 loaded scores, FLR_WT sums in flight and FLR_WT counters.
// The surplus sets of a partial last tile repeat the last set's weights (nothing is read past w) and are never stored.
// hipcc -O3 --offload-arch=gfx950 (kernel-resource-usage), FLR_WT = 8: N = 8: 59 VGPRs, 106 SGPRs, scratch 0, 7 waves / SIMD; the 64 weights
// and the compare masks exceed the SGPR file, so 66 SGPRs are parked in VGPR lanes (v_readlane inside the loop; no memory).  N = 3: 43 VGPRs,
// 106 SGPRs, scratch 0, the parked SGPRs are touched outside the loop only; the sums of two sets share one v_pk_fma_f32.
template <int N>
__global__ __launch_bounds__(256) void fused_label_rank_kernel(FusePtrs p, int64_t ldx, const float* __restrict__ w, int64_t ldw,
                                                               int nsets, int C, int vec, const int64_t* __restrict__ labels,
                                                               int32_t* __restrict__ rank, int64_t ldr) {
  __shared__ int shi[4];
  const int64_t row = blockIdx.x;
  const int j0 = blockIdx.y * FLR_WT;
  const int64_t lab = labels[row];
  if (lab < 0 || lab >= C) {      // uniform per block: never a hit; nothing is read at the label's position
    if (threadIdx.x < FLR_WT && j0 + (int)threadIdx.x < nsets) rank[(int64_t)(j0 + threadIdx.x) * ldr + row] = C;
    return;
  }
  const int l = (int)lab;
  float wt[FLR_WT][N];
#pragma unroll
  for (int j = 0; j < FLR_WT; ++j) {
    const int64_t js = j0 + j < nsets ? j0 + j : nsets - 1;
#pragma unroll
    for (int i = 0; i < N; ++i) wt[j][i] = w[js * ldw + i];
  }
  const float* xr[N];
  float xl[N];
#pragma unroll
  for (int i = 0; i < N; ++i) { xr[i] = p.x[i] + row * ldx; xl[i] = xr[i][l]; }
  float sl[FLR_WT];
  int cnt[FLR_WT];
#pragma unroll
  for (int j = 0; j < FLR_WT; ++j) { sl[j] = fuse_scores<N>(wt[j], xl); cnt[j] = 0; }
  walk_rows<N>(xr, C, vec != 0, [&](int c, const float (&v)[N]) {
    const bool other = c != l, lower = c < l;
#pragma unroll
    for (int j = 0; j < FLR_WT; ++j) {
      const float s = fuse_scores<N>(wt[j], v);
      cnt[j] += (other && (s > sl[j] || (s == sl[j] && lower))) ? 1 : 0;
    }
  });
#pragma unroll
  for (int j = 0; j < FLR_WT; ++j) {
    const int n = block_sum_int(cnt[j], shi);
    if (threadIdx.x == 0 && j0 + j < nsets) rank[(int64_t)(j0 + j) * ldr + row] = n;
  }
}

// grid (row blocks, sets): thread = one (row, set).  hits: one pair of integer atomics per workgroup; tps: one per top-k row; nums: the
// workgroups of set 0 only, so that every row counts once.
__global__ __launch_bounds__(256) void rank_counts_sets_kernel(const int32_t* __restrict__ rank, int64_t ldr, int nsets,
                                                               const int64_t* __restrict__ label, int rows, int C, int k,
                                                               int32_t* __restrict__ hits, int32_t* __restrict__ tps,
                                                               int32_t* __restrict__ nums) {
  __shared__ int shi[4];
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = r < rows;
  const int64_t l = live ? label[r] : -1;
  const bool counted = l >= 0 && l < C;
  if (blockIdx.y == 0 && counted) atomicAdd(nums + l, 1);
  for (int j = blockIdx.y; j < nsets; j += gridDim.y) {      // gridDim.y < nsets only beyond 65535 sets
    const int v = live ? rank[(int64_t)j * ldr + r] : k;
    if (counted && v < k) atomicAdd(tps + (int64_t)j * C + l, 1);
    const int h1 = block_sum_int(live && v < 1 ? 1 : 0, shi);
    const int hk = block_sum_int(live && v < k ? 1 : 0, shi);
    if (threadIdx.x == 0) {
      if (h1) atomicAdd(hits + 2 * (int64_t)j, h1);
      if (hk) atomicAdd(hits + 2 * (int64_t)j + 1, hk);
    }
  }
}

// rank_counts_sets_kernel with the counters kept per row group: bit g of member[r] puts row r into group g (member == nullptr: every row
// is in group 0, the only one).  `present` (the groups with a row in this workgroup) is uniform, so the reductions of an absent group
// are skipped as a whole and it gets no atomic.  The two hit counts of a (set, group) are at most 256 each and share one reduction:
// #{rank < 1} in the low half of the word, #{rank < k} in the high half.
__global__ __launch_bounds__(256) void rank_counts_groups_kernel(const int32_t* __restrict__ rank, int64_t ldr, int nsets,
                                                                 const int64_t* __restrict__ label,
                                                                 const uint32_t* __restrict__ member, int ngroups, int rows, int C, int k,
                                                                 int32_t* __restrict__ hits, int32_t* __restrict__ tps,
                                                                 int32_t* __restrict__ nums, int32_t* __restrict__ group_rows) {
  __shared__ int shi[4];
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = r < rows;
  const int64_t l = live ? label[r] : -1;
  const bool counted = l >= 0 && l < C;
  const unsigned m = !live ? 0u : member ? member[r] & ((1u << ngroups) - 1u) : 1u;      // ngroups <= 8: the shift is defined
  unsigned present = 0;
  for (int g = 0; g < ngroups; ++g) {
    const int n = block_sum_int((int)((m >> g) & 1u), shi);
    if (!n) continue;
    present |= 1u << g;
    if (blockIdx.y == 0 && threadIdx.x == 0) atomicAdd(group_rows + g, n);
  }
  if (blockIdx.y == 0 && counted)
    for (unsigned b = m; b; b &= b - 1) atomicAdd(nums + (int64_t)(__ffs((int)b) - 1) * C + l, 1);
  for (int j = blockIdx.y; j < nsets; j += gridDim.y) {      // gridDim.y < nsets only beyond 65535 sets
    const int v = live ? rank[(int64_t)j * ldr + r] : k;
    const int mine = (v < 1 ? 1 : 0) | (v < k ? 1 << 16 : 0);
    if (counted && v < k)
      for (unsigned b = m; b; b &= b - 1) atomicAdd(tps + ((int64_t)j * ngroups + (__ffs((int)b) - 1)) * C + l, 1);
    for (int g = 0; g < ngroups; ++g) {
      if (!((present >> g) & 1u)) continue;
      const int h = block_sum_int(((m >> g) & 1u) ? mine : 0, shi);
      if (threadIdx.x == 0) {
        int32_t* at = hits + 2 * ((int64_t)j * ngroups + g);
        if (h & 0xffff) atomicAdd(at, h & 0xffff);
        if (h >> 16) atomicAdd(at + 1, h >> 16);
      }
    }
  }
}

// Sort key of one score: high word = an unsigned image of the float that orders as the ORDER of include/afft_hip.h says (-0.0 folded
// onto +0.0 first, NaN -> 0, below the image 0x007fffff of -inf), low word = ~class, so that among equal scores the LOWER class has the
// LARGER key.  Integer arithmetic only: nothing here depends on the denormal mode.  Key 0 pads the row: below every real key.
__device__ __forceinline__ uint64_t topk_key(float v, int c) {
  unsigned u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  const unsigned img = (u & 0x7fffffffu) > 0x7f800000u ? 0u : (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)img << 32) | (uint64_t)(~(unsigned)c);
}

// One workgroup per row: the row as P = 2^p >= C keys in LDS, a descending bitonic sort over all P, the first k written out.
// The values are read back from the row itself, so that the sign of a zero and the payload of a NaN survive.
__global__ __launch_bounds__(256) void topk_rows_kernel(const float* __restrict__ xs, int64_t ldx, int C, int P, int k, int vec,
                                                        float* __restrict__ vals, int64_t ldv, int32_t* __restrict__ idx, int64_t ldi) {
  extern __shared__ uint64_t topk_keys[];
  const int64_t row = blockIdx.x;
  const float* x = xs + row * ldx;
  walk_row(x, C, vec != 0, [&](int c, float v) { topk_keys[c] = topk_key(v, c); });
  for (int c = C + threadIdx.x; c < P; c += 256) topk_keys[c] = 0;
  __syncthreads();
  for (int span = 2; span <= P; span <<= 1) {
    for (int j = span >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += 256) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));      // the lower element of pair t: bit j clear; i + j < P
        const uint64_t a = topk_keys[i], b = topk_keys[i + j];
        if ((i & span) == 0 ? a < b : a > b) { topk_keys[i] = b; topk_keys[i + j] = a; }
      }
      __syncthreads();
    }
  }
  for (int j = threadIdx.x; j < k; j += 256) {      // k <= C: the first k keys are real ones, their class lies in [0, C)
    const int c = (int)~(unsigned)topk_keys[j];
    idx[row * ldi + j] = c;
    vals[row * ldv + j] = x[c];
  }
}

}  // namespace

extern "C" int afft_topk_rows(const float* x, int64_t ldx, int32_t rows, int32_t C, int32_t k, float* vals, int64_t ldv, int32_t* idx,
                              int64_t ldi, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AFFT_CHECK(rows >= 1, "topk_rows: rows >= 1 (got %d)", rows);
  AFFT_CHECK(k >= 1 && k <= C && C <= AFFT_TOPK_MAX_C, "topk_rows: 1 <= k <= C <= %d (got k = %d, C = %d)", AFFT_TOPK_MAX_C, k, C);
  AFFT_CHECK(ldx >= C, "topk_rows: ldx %lld < C = %d", (long long)ldx, C);
  AFFT_CHECK(ldv >= k, "topk_rows: ldv %lld < k = %d", (long long)ldv, k);
  AFFT_CHECK(ldi >= k, "topk_rows: ldi %lld < k = %d", (long long)ldi, k);
  AFFT_CHECK(x && vals && idx, "topk_rows: null x / vals / idx");
  int P = 1;
  while (P < C) P <<= 1;
  const size_t lds = (size_t)P * sizeof(uint64_t);
  static std::atomic<uint64_t> attr_done{0};
  if (lds > 48 * 1024)      // raised once to what the limit needs: the attribute belongs to the kernel, not to the launch
    if (int rc = afft_ensure_dynamic_lds(reinterpret_cast<const void*>(topk_rows_kernel), (size_t)AFFT_TOPK_MAX_C * sizeof(uint64_t), &attr_done))
      return rc;
  const int vec = ((uintptr_t)x & 15) == 0 && (ldx & 3) == 0;
  hipLaunchKernelGGL(topk_rows_kernel, dim3(rows), dim3(256), lds, stream, x, ldx, C, P, k, vec, vals, ldv, idx, ldi);
  AFFT_LAUNCH_CHECK();
  return 0;
}

extern "C" int afft_label_rank(const float* logits, int64_t row_stride, int32_t rows, int32_t C, const int64_t* labels,
                               const float* soft, int64_t lds, int32_t k, float acc_scale, int32_t* rank, int64_t* label_out,
                               float* acc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AFFT_CHECK(logits && rank && label_out, "label_rank: null logits / rank / label_out");
  AFFT_CHECK((labels != nullptr) != (soft != nullptr), "label_rank: give exactly one of labels / soft targets");
  AFFT_CHECK(rows >= 1 && C >= 1, "label_rank: rows >= 1 and C >= 1 (got %d, %d)", rows, C);
  AFFT_CHECK(k >= 1 && k <= C, "label_rank: 1 <= k <= C (got k = %d, C = %d)", k, C);
  AFFT_CHECK(row_stride >= C, "label_rank: row_stride %lld < C = %d", (long long)row_stride, C);
  AFFT_CHECK(!soft || lds >= C, "label_rank: soft-target row stride %lld < C = %d", (long long)lds, C);
  const int vec_x = ((uintptr_t)logits & 15) == 0 && (row_stride & 3) == 0;
  const int vec_t = soft && ((uintptr_t)soft & 15) == 0 && (lds & 3) == 0;
  hipLaunchKernelGGL(label_rank_kernel, dim3(rows), dim3(256), 0, stream, logits, row_stride, C, labels, soft, lds, vec_x, vec_t,
                     rank, label_out);
  AFFT_LAUNCH_CHECK();
  if (acc) {
    hipLaunchKernelGGL(rank_hits_kernel, dim3(1), dim3(256), 0, stream, rank, rows, k, acc_scale, acc);
    AFFT_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int afft_fused_label_rank(const float* const* x, int64_t ldx, int32_t n, const float* w, int64_t ldw, int32_t nsets,
                                     int32_t rows, int32_t C, const int64_t* labels, int32_t* rank, int64_t ldr, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AFFT_CHECK(n >= 1 && n <= 8, "fused_label_rank: 1 <= n <= 8 runs (got %d)", n);
  AFFT_CHECK(rows >= 1 && C >= 1, "fused_label_rank: rows >= 1 and C >= 1 (got %d, %d)", rows, C);
  AFFT_CHECK(nsets >= 1 && nsets <= 65535 * FLR_WT, "fused_label_rank: 1 <= nsets <= %d (got %d)", 65535 * FLR_WT, nsets);
  AFFT_CHECK(ldx >= C, "fused_label_rank: ldx %lld < C = %d", (long long)ldx, C);
  AFFT_CHECK(ldw >= n, "fused_label_rank: ldw %lld < n = %d", (long long)ldw, n);
  AFFT_CHECK(ldr >= rows, "fused_label_rank: ldr %lld < rows = %d", (long long)ldr, rows);
  AFFT_CHECK(x && w && labels && rank, "fused_label_rank: null x / w / labels / rank");
  FusePtrs p;
  int vec = (ldx & 3) == 0;
  for (int i = 0; i < 8; ++i) {
    p.x[i] = i < n ? x[i] : nullptr;
    AFFT_CHECK(i >= n || x[i], "fused_label_rank: x[%d] is null", i);
    vec = vec && ((uintptr_t)p.x[i] & 15) == 0;
  }
  const dim3 grid((unsigned)rows, (unsigned)((nsets + FLR_WT - 1) / FLR_WT));
#define AFFT_FLR_LAUNCH(N)                                                                                                          \
  case N:                                                                                                                           \
    hipLaunchKernelGGL(fused_label_rank_kernel<N>, grid, dim3(256), 0, stream, p, ldx, w, ldw, nsets, C, vec, labels, rank, ldr); \
    break;
  switch (n) {
    AFFT_FLR_LAUNCH(1) AFFT_FLR_LAUNCH(2) AFFT_FLR_LAUNCH(3) AFFT_FLR_LAUNCH(4)
    AFFT_FLR_LAUNCH(5) AFFT_FLR_LAUNCH(6) AFFT_FLR_LAUNCH(7) AFFT_FLR_LAUNCH(8)
  }
#undef AFFT_FLR_LAUNCH
  AFFT_LAUNCH_CHECK();
  return 0;
}

extern "C" int afft_rank_counts_sets(const int32_t* rank, int64_t ldr, int32_t nsets, const int64_t* label, int32_t rows, int32_t C,
                                     int32_t k, int32_t* hits, int32_t* tps, int32_t* nums, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AFFT_CHECK(rank && label && hits && tps && nums, "rank_counts_sets: null pointer");
  AFFT_CHECK(rows >= 1 && C >= 1, "rank_counts_sets: rows >= 1 and C >= 1 (got %d, %d)", rows, C);
  AFFT_CHECK(k >= 1 && k <= C, "rank_counts_sets: 1 <= k <= C (got k = %d, C = %d)", k, C);
  AFFT_CHECK(nsets >= 1, "rank_counts_sets: nsets >= 1 (got %d)", nsets);
  AFFT_CHECK(ldr >= rows, "rank_counts_sets: ldr %lld < rows = %d", (long long)ldr, rows);
  const dim3 grid((unsigned)(((int64_t)rows + 255) / 256), (unsigned)(nsets < 65535 ? nsets : 65535));
  hipLaunchKernelGGL(rank_counts_sets_kernel, grid, dim3(256), 0, stream, rank, ldr, nsets, label, rows, C, k, hits, tps, nums);
  AFFT_LAUNCH_CHECK();
  return 0;
}

extern "C" int afft_rank_counts_groups(const int32_t* rank, int64_t ldr, int32_t nsets, const int64_t* label, const uint32_t* member,
                                       int32_t ngroups, int32_t rows, int32_t C, int32_t k, int32_t* hits, int32_t* tps, int32_t* nums,
                                       int32_t* group_rows, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AFFT_CHECK(ngroups >= 1 && ngroups <= 8, "rank_counts_groups: 1 <= ngroups <= 8 (got %d)", ngroups);
  AFFT_CHECK(rank && label && hits && tps && nums && group_rows, "rank_counts_groups: null pointer");
  AFFT_CHECK(member || ngroups == 1, "rank_counts_groups: null member with ngroups = %d (allowed with one group only)", ngroups);
  AFFT_CHECK(rows >= 1 && C >= 1, "rank_counts_groups: rows >= 1 and C >= 1 (got %d, %d)", rows, C);
  AFFT_CHECK(k >= 1 && k <= C, "rank_counts_groups: 1 <= k <= C (got k = %d, C = %d)", k, C);
  AFFT_CHECK(nsets >= 1, "rank_counts_groups: nsets >= 1 (got %d)", nsets);
  AFFT_CHECK(ldr >= rows, "rank_counts_groups: ldr %lld < rows = %d", (long long)ldr, rows);
  const dim3 grid((unsigned)(((int64_t)rows + 255) / 256), (unsigned)(nsets < 65535 ? nsets : 65535));
  hipLaunchKernelGGL(rank_counts_groups_kernel, grid, dim3(256), 0, stream, rank, ldr, nsets, label, member, ngroups, rows, C, k, hits, tps,
                     nums, group_rows);
  AFFT_LAUNCH_CHECK();
  return 0;
}

extern "C" int afft_recall_accumulate(const int32_t* rank, const int64_t* label, int32_t rows, int32_t C, int32_t k, int32_t* tps,
                                      int32_t* nums, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AFFT_CHECK(rank && label && tps && nums, "recall_accumulate: null pointer");
  AFFT_CHECK(rows >= 1 && C >= 1, "recall_accumulate: rows >= 1 and C >= 1 (got %d, %d)", rows, C);
  AFFT_CHECK(k >= 1 && k <= C, "recall_accumulate: 1 <= k <= C (got k = %d, C = %d)", k, C);
  hipLaunchKernelGGL(recall_accumulate_kernel, dim3((unsigned)(((int64_t)rows + 255) / 256)), dim3(256), 0, stream, rank, label, rows,
                     C, k, tps, nums);
  AFFT_LAUNCH_CHECK();
  return 0;
}
