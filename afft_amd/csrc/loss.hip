// Fused softmax cross-entropy (forward + gradient in one pass over the logits) and MSE.
// Semantics: common/runner.py:13-37 (MultiDimCrossEntropy, reduction='none', ignore_index=-1 or a
// boolean row filter for soft targets), :164-166 (MSELoss, both arguments carry gradient).
#include "common.h"

namespace {

__device__ __forceinline__ float block_reduce(float v, float* sh, bool is_max) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = is_max ? wave_max(v) : wave_sum(v);
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  float r = sh[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = is_max ? fmaxf(r, sh[w]) : r + sh[w];
  return r;
}

// a_c of the weighted / smoothed cross-entropy (include/afft_hip.h): soft target t: w_c ((1 - eps) t_c + eps / C); hard label y:
// (eps / C) w_c + (1 - eps) w_y [c == y] (own = (1 - eps) w_y, 0 for a label out of range).  w NULL = all ones.
__device__ __forceinline__ float ce_coef(const float* __restrict__ w, const float* __restrict__ t, int c, int64_t lab, float unif,
                                         float sharp, float own) {
  const float wc = w ? w[c] : 1.f;
  return t ? wc * (sharp * t[c] + unif) : unif * wc + (c == lab ? own : 0.f);
}

// W = false: plain cross-entropy (no class weights, no smoothing; `weight` and `smoothing` are not read).  W = true: the row's
// per-class coefficient a_c (ce_coef), A = sum_c a_c:  loss = lse * A - sum_c a_c x_c,  dloss/dx_j = p_j * A - a_j.
template <bool W>
__global__ __launch_bounds__(256) void softmax_ce_kernel(const float* __restrict__ logits, int64_t ldl, int C,
                                                         const int64_t* __restrict__ labels,
                                                         const float* __restrict__ soft, int64_t lds,
                                                         const uint8_t* __restrict__ keep, float gscale,
                                                         const float* __restrict__ row_g,
                                                         void* __restrict__ dlogits,
                                                         int64_t ldd, int d_dtype, float* __restrict__ row_loss,
                                                         int period, int64_t lgs, int64_t dgs,
                                                         const float* __restrict__ weight, float smoothing) {
  // row r = frame r % period of clip r / period: logits at clip * lgs + frame * ldl, its gradient at clip * dgs + frame * ldd
  // (a (B, n, C) slice of a wider (B, L, C) tensor is walked where it lies; period = rows: plain [rows, C])
  __shared__ float sh[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int clip = row / period, frame = row - clip * period;
  const float* x = logits + (int64_t)clip * lgs + (int64_t)frame * ldl;
  const int64_t drow = (int64_t)clip * dgs + (int64_t)frame * ldd;
  bool kept = true;
  int64_t lab = -1;
  if (labels) { lab = labels[row]; kept = lab != -1; }
  // a label outside [-1, C) (torch raises a device-side assert there): nothing out of bounds is read, and the row's loss
  // and gradient come out NaN so that the total cannot look healthy
  const bool bad = labels && (lab >= C || lab < -1);
  if (keep) kept = kept && keep[row] != 0;
  if (!kept) {  // uniform per block
    if (dlogits) for (int c = tid; c < ldd; c += 256) st_any(dlogits, drow + c, d_dtype, 0.f);
    if (row_loss && tid == 0) row_loss[row] = 0.f;
    return;
  }
  float m = -INFINITY;
  for (int c = tid; c < C; c += 256) m = fmaxf(m, x[c]);
  m = block_reduce(m, sh, true);
  const float* t = soft ? soft + (int64_t)row * lds : nullptr;
  if constexpr (W) {
    // smoothing / C for every class, (1 - smoothing) on the target; the label's own weight is ONE load, and a label out of range reads
    // none.  weight (<= 15 KB at C = 3806) is read in the same column loops as x and stays in cache.
    const float unif = smoothing / (float)C, sharp = 1.f - smoothing;
    const float own = t || bad ? 0.f : sharp * (weight ? weight[lab] : 1.f);
    float se = 0.f, asum = 0.f, ax = 0.f;
    for (int c = tid; c < C; c += 256) {
      se += expf(x[c] - m);
      const float a = ce_coef(weight, t, c, lab, unif, sharp, own);
      asum += a;
      ax += a * x[c];
    }
    se = block_reduce(se, sh, false);
    asum = block_reduce(asum, sh, false);
    ax = block_reduce(ax, sh, false);
    const float lse = m + logf(se);
    if (tid == 0 && row_loss) row_loss[row] = bad ? NAN : lse * asum - ax;
    if (dlogits) {
      const float inv = 1.0f / se;
      if (row_g) gscale *= row_g[row];
      for (int c = tid; c < ldd; c += 256) {
        float g = 0.f;
        if (c < C) {
          const float p = expf(x[c] - m) * inv;
          g = bad ? NAN : gscale * (p * asum - ce_coef(weight, t, c, lab, unif, sharp, own));
        }
        st_any(dlogits, drow + c, d_dtype, g);
      }
    }
    return;
  }
  float se = 0.f, tsum = 0.f, tx = 0.f;
  for (int c = tid; c < C; c += 256) {
    se += expf(x[c] - m);
    if (t) { tsum += t[c]; tx += t[c] * x[c]; }
  }
  se = block_reduce(se, sh, false);
  const float lse = m + logf(se);
  float loss;
  if (t) {
    tsum = block_reduce(tsum, sh, false);
    tx = block_reduce(tx, sh, false);
    loss = lse * tsum - tx;
  } else {
    tsum = 1.f;
    loss = bad ? NAN : lse - x[lab];
  }
  if (tid == 0 && row_loss) row_loss[row] = loss;
  if (dlogits) {
    const float inv = 1.0f / se;
    if (row_g) gscale *= row_g[row];
    for (int c = tid; c < ldd; c += 256) {
      float g = 0.f;
      if (c < C) {
        const float p = expf(x[c] - m) * inv;
        const float tc = t ? t[c] : (c == lab ? 1.f : 0.f);
        g = bad ? NAN : gscale * (p * tsum - tc);
      }
      st_any(dlogits, drow + c, d_dtype, g);
    }
  }
}

// The row's maximum WITH its index: ties go to the lower index, whatever the order of the combine (lane tree, then the four waves front
// to back), so the class that focal_terms treats as the arg-max is a function of the row alone.
__device__ __forceinline__ void block_argmax(float& m, int& idx, float* shv, int* shi) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (om > m || (om == m && oi < idx)) { m = om; idx = oi; }
  }
  __syncthreads();
  if (lane == 0) { shv[wave] = m; shi[wave] = idx; }
  __syncthreads();
  m = shv[0]; idx = shi[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) {
    const float om = shv[w];
    const int oi = shi[w];
    if (om > m || (om == m && oi < idx)) { m = om; idx = oi; }
  }
}

// One class of a focal row (include/afft_hip.h): p, q = 1 - p, f = q^gamma l, g = q^gamma + gamma p q^(gamma - 1) l, with l = lse - z.
// r = sum over the classes other than the arg-max of exp(z - m), inv = 1 / (1 + r), l1p = log1p(r).  The arg-max is the one class
// whose 1 - p cancels: its q and l come from r; every other class has p <= 1/2.
__device__ __forceinline__ void focal_terms(float z, bool is_max, float m, float r, float inv, float l1p, float gamma,
                                            float& p, float& q, float& f, float& g) {
  // q^gamma: the arg-max's q may be tiny (its relative accuracy is what a dominant row's loss has), so it takes powf -- once per row;
  // elsewhere q lies in [1/2, 1], |log2 q| <= 1, and exp2(gamma log2 q) on the hardware's log2 / exp2 is good to ~gamma ulp
  float l, qg;
  if (is_max) {
    p = inv; q = r * inv; l = l1p;
    qg = gamma == 0.f ? 1.f : powf(q, gamma);
  } else {
    p = expf(z - m) * inv; q = 1.f - p; l = (m - z) + l1p;
    qg = gamma == 0.f ? 1.f : __builtin_amdgcn_exp2f(gamma * __builtin_amdgcn_logf(q));
  }
  f = qg * l;
  g = qg + (q > 0.f ? gamma * p * qg * (l / q) : 0.f);
}

// Focal / logit-adjusted cross-entropy: z = x + adjust, row_loss = sum_c a_c q_c^gamma l_c, dlogits[j] = p_j G - a_j g_j with
// G = sum_c a_c g_c (a_c: ce_coef, as in softmax_ce_kernel<true>).  Passes over the row: arg-max; r and A; the loss and G; the gradient.
// A hard label without smoothing has ONE non-zero a_c: its loss and G are one term, the third pass is skipped and the gradient pass
// takes no power.  The arg-max's own gradient element is p (G - a g) - q a g: no 1 - p there either.
__global__ __launch_bounds__(256) void softmax_ce_focal_kernel(const float* __restrict__ logits, int64_t ldl, int C,
                                                               const int64_t* __restrict__ labels,
                                                               const float* __restrict__ soft, int64_t lds,
                                                               const uint8_t* __restrict__ keep, float gscale,
                                                               const float* __restrict__ row_g,
                                                               void* __restrict__ dlogits,
                                                               int64_t ldd, int d_dtype, float* __restrict__ row_loss,
                                                               int period, int64_t lgs, int64_t dgs,
                                                               const float* __restrict__ weight, float smoothing,
                                                               const float* __restrict__ adjust, float gamma) {
  __shared__ float sh[4];
  __shared__ int shi[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int clip = row / period, frame = row - clip * period;
  const float* x = logits + (int64_t)clip * lgs + (int64_t)frame * ldl;
  const int64_t drow = (int64_t)clip * dgs + (int64_t)frame * ldd;
  bool kept = true;
  int64_t lab = -1;
  if (labels) { lab = labels[row]; kept = lab != -1; }
  const bool bad = labels && (lab >= C || lab < -1);      // as in softmax_ce_kernel: nothing is read at `lab`, the row comes out NaN
  if (keep) kept = kept && keep[row] != 0;
  if (!kept) {  // uniform per block
    if (dlogits) for (int c = tid; c < ldd; c += 256) st_any(dlogits, drow + c, d_dtype, 0.f);
    if (row_loss && tid == 0) row_loss[row] = 0.f;
    return;
  }
  float m = -INFINITY;
  int am = 0x7fffffff;
  for (int c = tid; c < C; c += 256) {
    const float z = x[c] + (adjust ? adjust[c] : 0.f);
    if (z > m) { m = z; am = c; }
  }
  block_argmax(m, am, sh, shi);
  const float* t = soft ? soft + (int64_t)row * lds : nullptr;
  const float unif = smoothing / (float)C, sharp = 1.f - smoothing;
  const float own = t || bad ? 0.f : sharp * (weight ? weight[lab] : 1.f);
  const bool single = !t && unif == 0.f;      // a hard label, no smoothing: a_c = own [c == lab]
  float r = 0.f, asum = 0.f;
  for (int c = tid; c < C; c += 256) {
    const float z = x[c] + (adjust ? adjust[c] : 0.f);
    r += c == am ? 0.f : expf(z - m);
    if (!single) asum += ce_coef(weight, t, c, lab, unif, sharp, own);
  }
  r = block_reduce(r, sh, false);
  asum = single ? own : block_reduce(asum, sh, false);
  const float inv = 1.0f / (1.0f + r), l1p = log1pf(r);
  // loss; G in two parts: the arg-max's own term a g (g_max) and the sum of the others (g_rest)
  float loss = 0.f, g_rest = 0.f, g_max = 0.f, g_lab = 0.f;
  if (single) {
    const float z = bad ? 0.f : x[lab] + (adjust ? adjust[lab] : 0.f);
    float p, q, f, g;
    focal_terms(z, lab == am, m, r, inv, l1p, gamma, p, q, f, g);
    loss = own * f;
    g_lab = own * g;
    if (lab == am) g_max = g_lab; else g_rest = g_lab;
  } else {
    for (int c = tid; c < C; c += 256) {
      const float z = x[c] + (adjust ? adjust[c] : 0.f);
      const float a = ce_coef(weight, t, c, lab, unif, sharp, own);
      float p, q, f, g;
      focal_terms(z, c == am, m, r, inv, l1p, gamma, p, q, f, g);
      loss += a * f;
      if (c == am) g_max = a * g; else g_rest += a * g;
    }
    if (row_loss) loss = block_reduce(loss, sh, false);
    if (dlogits) {
      g_rest = block_reduce(g_rest, sh, false);
      g_max = block_reduce(g_max, sh, false);      // one non-zero term: exact
    }
  }
  if (tid == 0 && row_loss) row_loss[row] = bad ? NAN : loss;
  if (dlogits) {
    const float gsum = g_rest + g_max;
    if (row_g) gscale *= row_g[row];
    for (int c = tid; c < ldd; c += 256) {
      float d = 0.f;
      if (c < C) {
        const float z = x[c] + (adjust ? adjust[c] : 0.f);
        if (c == am) {
          d = inv * g_rest - r * inv * g_max;
        } else if (single) {
          d = expf(z - m) * inv * gsum - (c == lab ? g_lab : 0.f);
        } else {
          float p, q, f, g;
          focal_terms(z, false, m, r, inv, l1p, gamma, p, q, f, g);
          d = p * gsum - ce_coef(weight, t, c, lab, unif, sharp, own) * g;
        }
        d = bad ? NAN : gscale * d;
      }
      st_any(dlogits, drow + c, d_dtype, d);
    }
  }
}

// Marginal cross-entropy over class groups (include/afft_hip.h): the classes of a row belong to G groups (group_of; -1: none), the
// target is a group, loss = T lse - sum_g t_g lse_g, dlogits[c] = T p_c - t_g(c) exp(x_c - m_g(c)) / s_g(c) with m_g the group's OWN
// maximum and s_g = sum_{c in g} exp(x_c - m_g): a group far below the row's top logit keeps its full precision.
// Passes: row max, row sum (as softmax_ce_kernel); the groups, strided over the four waves, each group's members (CSR: offs, members)
// strided over the wave's lanes, wave_max / wave_sum -- lane 0 leaves m_g and t_g / s_g in LDS and every wave keeps the sum of its own
// t_g lse_g, groups front to back; the four sums and T in fixed order; the gradient.  A hard label is the soft target [g == y] and
// visits group y alone (by the wave that a full walk gives it to).  Groups with t_g == 0 are not visited and may be empty.
__global__ __launch_bounds__(256) void softmax_ce_groups_kernel(const float* __restrict__ logits, int64_t ldl, int C, int G,
                                                                const int32_t* __restrict__ group_of,
                                                                const int32_t* __restrict__ members,
                                                                const int32_t* __restrict__ offs,
                                                                const int64_t* __restrict__ glabels,
                                                                const float* __restrict__ gsoft, int64_t ldgs,
                                                                const uint8_t* __restrict__ keep, float gscale,
                                                                const float* __restrict__ row_g, void* __restrict__ dlogits,
                                                                int64_t ldd, int d_dtype, float* __restrict__ row_loss,
                                                                int period, int64_t lgs, int64_t dgs) {
  __shared__ float sh[4];
  __shared__ float sh_m[AFFT_CE_GROUPS_MAX], sh_c[AFFT_CE_GROUPS_MAX];      // m_g and t_g / s_g (0: the group takes no part)
  __shared__ int sh_empty;                                                  // a targeted group without members: the row is bad
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int clip = row / period, frame = row - clip * period;
  const float* x = logits + (int64_t)clip * lgs + (int64_t)frame * ldl;
  const int64_t drow = (int64_t)clip * dgs + (int64_t)frame * ldd;
  bool kept = true;
  int64_t lab = -1;
  if (glabels) { lab = glabels[row]; kept = lab != -1; }
  bool bad = glabels && (lab >= G || lab < -1);      // as in softmax_ce_kernel: nothing is read at `lab`, the row comes out NaN
  if (keep) kept = kept && keep[row] != 0;
  if (!kept) {  // uniform per block
    if (dlogits) for (int c = tid; c < ldd; c += 256) st_any(dlogits, drow + c, d_dtype, 0.f);
    if (row_loss && tid == 0) row_loss[row] = 0.f;
    return;
  }
  if (tid == 0) sh_empty = 0;      // the barriers of the two block reductions below stand between this and the waves' own stores
  float m = -INFINITY;
  for (int c = tid; c < C; c += 256) m = fmaxf(m, x[c]);
  m = block_reduce(m, sh, true);
  float se = 0.f;
  for (int c = tid; c < C; c += 256) se += expf(x[c] - m);
  se = block_reduce(se, sh, false);
  const float lse = m + logf(se);
  const float* t = gsoft ? gsoft + (int64_t)row * ldgs : nullptr;
  const int g0 = t ? 0 : (bad ? 0 : (int)lab), g1 = t ? G : (bad ? 0 : (int)lab + 1);
  float part = 0.f;      // this wave's sum of t_g lse_g: the same value in all of its lanes
  for (int g = g0 + wave; g < g1; g += 4) {      // everything in this loop is uniform per wave
    const float tg = t ? t[g] : 1.f;
    const int beg = offs[g], end = offs[g + 1];
    if (tg == 0.f || end <= beg) {
      if (lane == 0) { sh_c[g] = 0.f; if (tg != 0.f) sh_empty = 1; }
      continue;
    }
    float mg = -INFINITY;
    for (int i = beg + lane; i < end; i += 64) mg = fmaxf(mg, x[members[i]]);
    mg = wave_max(mg);
    float sg = 0.f;
    for (int i = beg + lane; i < end; i += 64) sg += expf(x[members[i]] - mg);
    sg = wave_sum(sg);
    part += tg * (mg + logf(sg));
    if (lane == 0) { sh_m[g] = mg; sh_c[g] = tg / sg; }
  }
  float tsum = 1.f;
  if (t) {
    tsum = 0.f;
    for (int g = tid; g < G; g += 256) tsum += t[g];
    tsum = block_reduce(tsum, sh, false);
  }
  const float tl = block_reduce(lane == 0 ? part : 0.f, sh, false);      // sh[0] + sh[1] + sh[2] + sh[3]; its barrier publishes sh_m / sh_c
  bad = bad || sh_empty != 0;
  if (tid == 0 && row_loss) row_loss[row] = bad ? NAN : lse * tsum - tl;
  if (dlogits) {
    const float inv = 1.0f / se;
    if (row_g) gscale *= row_g[row];
    for (int c = tid; c < ldd; c += 256) {
      float g = 0.f;
      if (c < C) {
        const float p = expf(x[c] - m) * inv;
        const int gi = group_of[c];
        float q = 0.f;
        if (!bad && gi >= 0 && (t || gi == lab)) {
          const float coef = sh_c[gi];
          if (coef != 0.f) q = coef * expf(x[c] - sh_m[gi]);
        }
        g = bad ? NAN : gscale * (p * tsum - q);
      }
      st_any(dlogits, drow + c, d_dtype, g);
    }
  }
}

__global__ __launch_bounds__(256) void mse_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ b,
                                                  int64_t ldb, int rows, int d, float gscale,
                                                  const float* __restrict__ g_dev, float lscale,
                                                  float* __restrict__ loss_sum, float* __restrict__ partials,
                                                  float* __restrict__ da, int64_t ldda, float* __restrict__ db,
                                                  int64_t lddb, int accumulate) {
  __shared__ float sh[4];
  float acc = 0.f;
  const int64_t total = (int64_t)rows * d;
  if (g_dev) gscale *= g_dev[0];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int r = (int)(i / d), c = (int)(i - (int64_t)r * d);
    const float diff = a[(int64_t)r * lda + c] - b[(int64_t)r * ldb + c];
    acc += diff * diff;
    const float g = 2.f * gscale * diff;
    if (da) da[(int64_t)r * ldda + c] += g;
    if (db) db[(int64_t)r * lddb + c] -= g;
  }
  if (!loss_sum) return;
  acc = block_reduce(acc, sh, false);
  // one workgroup: it IS the sum.  More: the partial goes to the caller's scratch and ordered_sum_kernel adds them up in
  // workgroup order behind this kernel (no float atomics: the loss scalar has the same bits on every run)
  if (threadIdx.x == 0) {
    if (gridDim.x == 1) *loss_sum = (accumulate ? *loss_sum : 0.f) + acc * lscale; else partials[blockIdx.x] = acc;
  }
}

// Backward of the MSE between frame ranges of two (clips, frames, C) tensors: the FULL gradients of both are written in one pass
// -- 2 g (a - b) inside the ranges, zeros outside -- so that no fill kernel runs in front and no slice-backward behind.
__global__ __launch_bounds__(256) void mse_frames_bwd_kernel(const float* __restrict__ a, int64_t a_cs, int a_off, int a_len,
                                                             const float* __restrict__ b, int64_t b_cs, int b_off, int b_len,
                                                             int clips, int n, float gscale, const float* __restrict__ g_dev,
                                                             float* __restrict__ da, float* __restrict__ db) {
  if (g_dev) gscale *= g_dev[0];
  const int clip = blockIdx.y;
  const float* ar = a + (int64_t)clip * a_cs;
  const float* br = b + (int64_t)clip * b_cs;
  float* dar = da ? da + (int64_t)clip * a_len : nullptr;
  float* dbr = db ? db + (int64_t)clip * b_len : nullptr;
  const int span = max(a_len, b_len);
  for (int i = (blockIdx.x * 256 + threadIdx.x) * 4; i < span; i += gridDim.x * 1024) {      // lengths and offsets are multiples of 4
    if (dar && i < a_len) {
      const int j = i - a_off;
      f32x4 g = {0.f, 0.f, 0.f, 0.f};
      if (j >= 0 && j < n) {
        const f32x4 x = *(const f32x4*)(ar + i), y = *(const f32x4*)(br + b_off + j);
        for (int e = 0; e < 4; ++e) g[e] = 2.f * gscale * (x[e] - y[e]);
      }
      *(f32x4*)(dar + i) = g;
    }
    if (dbr && i < b_len) {
      const int j = i - b_off;
      f32x4 g = {0.f, 0.f, 0.f, 0.f};
      if (j >= 0 && j < n) {
        const f32x4 x = *(const f32x4*)(ar + a_off + j), y = *(const f32x4*)(br + i);
        for (int e = 0; e < 4; ++e) g[e] = -2.f * gscale * (x[e] - y[e]);
      }
      *(f32x4*)(dbr + i) = g;
    }
  }
}

// Runner._reduce_loss in one launch: term i = n[i] floats at x[i]; means[i] = their mean (lane-strided partial sums, then a fixed
// tree: the same bits on every run), total = sum_i w[i] * means[i].  One workgroup (the terms are a few thousand values).
struct LossTerms { const float* x[8]; float* g[8]; int64_t n[8]; float w[8]; int nterms; };
__global__ __launch_bounds__(256) void loss_reduce_kernel(const LossTerms t, float* __restrict__ means, float* __restrict__ total) {
  __shared__ float sh[4];
  float tot = 0.f;
  for (int i = 0; i < t.nterms; ++i) {
    float s = 0.f;
    for (int64_t j = threadIdx.x; j < t.n[i]; j += 256) s += t.x[i][j];
    s = block_reduce(s, sh, false);
    const float m = t.n[i] > 0 ? s / (float)t.n[i] : 0.f;
    if (threadIdx.x == 0 && means) means[i] = m;
    if (t.w[i] != 0.f) tot += t.w[i] * m;     // a weight of 0 DROPS the term (runner.py:205-207): its NaN / inf must not reach the total
  }
  if (threadIdx.x == 0) *total = tot;
}
// its backward: g[i][:] = g_total * w[i] / n[i]
__global__ __launch_bounds__(256) void loss_reduce_bwd_kernel(const LossTerms t, const float* __restrict__ g_total,
                                                              const float* __restrict__ total, float* __restrict__ ok) {
  const float go = g_total ? g_total[0] : 1.f;
  const int i = blockIdx.y;
  // the first kernel of a backward pass: "is this step finite" for the optimizer kernels that follow it (afft_sgd_fused_t.ok)
  if (ok && blockIdx.x == 0 && i == 0 && threadIdx.x == 0) *ok = (!total || isfinite(total[0])) && isfinite(go) ? 1.f : 0.f;
  if (!t.g[i] || t.n[i] <= 0) return;
  const float v = go * t.w[i] / (float)t.n[i];
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < t.n[i]; j += (int64_t)gridDim.x * 256) t.g[i][j] = v;
}

}  // namespace

extern "C" int afft_loss_reduce(const float* const* x, const int64_t* n, const float* w, int32_t nterms, float* means, float* total,
                                void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AFFT_CHECK(x && n && w && total, "loss_reduce: null pointer");
  AFFT_CHECK(nterms >= 1 && nterms <= 8, "loss_reduce: 1..8 terms (got %d)", nterms);
  LossTerms t = {};
  t.nterms = nterms;
  for (int i = 0; i < nterms; ++i) { AFFT_CHECK(x[i] || n[i] == 0, "loss_reduce: null term"); t.x[i] = x[i]; t.n[i] = n[i]; t.w[i] = w[i]; }
  hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(256), 0, stream, t, means, total);
  AFFT_LAUNCH_CHECK();
  return 0;
}

extern "C" int afft_loss_reduce_bwd(float* const* g, const int64_t* n, const float* w, int32_t nterms, const float* g_total,
                                    void* stream_) {
  return afft_loss_reduce_bwd_ok(g, n, w, nterms, g_total, nullptr, nullptr, stream_);
}

extern "C" int afft_loss_reduce_bwd_ok(float* const* g, const int64_t* n, const float* w, int32_t nterms, const float* g_total,
                                       const float* total, float* ok, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AFFT_CHECK(g && n && w, "loss_reduce_bwd: null pointer");
  AFFT_CHECK(nterms >= 1 && nterms <= 8, "loss_reduce_bwd: 1..8 terms (got %d)", nterms);
  LossTerms t = {};
  t.nterms = nterms;
  int64_t nmax = 1;
  for (int i = 0; i < nterms; ++i) { t.g[i] = g[i]; t.n[i] = n[i]; t.w[i] = w[i]; nmax = n[i] > nmax ? n[i] : nmax; }
  const int gx = (int)((nmax + 255) / 256 > 64 ? 64 : (nmax + 255) / 256);
  hipLaunchKernelGGL(loss_reduce_bwd_kernel, dim3(gx, nterms), dim3(256), 0, stream, t, g_total, total, ok);
  AFFT_LAUNCH_CHECK();
  return 0;
}

// One cross-entropy call, whichever of the six entry points below it came through: they only fill this in, in the order of the
// frames form's arguments.  The row form is period = rows with clip strides 0; an entry without an option passes its neutral value.
struct CeCall {
  const float* logits; int64_t lgs, ldl;      // clip stride, frame (row) stride
  int32_t rows, period, C;                    // rows = clips * frames, period = frames
  const int64_t* labels; const float* soft; int64_t lds; const uint8_t* keep; float gscale; const float* row_g;
  void* dlogits; int64_t dgs, ldd; int32_t d_dtype; float* row_loss;
  const float* weight; float smoothing; const float* adjust; float gamma;
  float* loss_sum;                            // row form only: the ordered sum of row_loss
  bool frames;                                // the caller's form: it names the entry in the messages, and wants period > 0
  void* stream;
};

static int ce_launch(const CeCall& c) {
  hipStream_t stream = (hipStream_t)c.stream;
  static const char* const names[2][3] = {{"softmax_ce", "softmax_ce_w", "softmax_ce_focal"},
                                          {"softmax_ce_frames", "softmax_ce_frames_w", "softmax_ce_frames_focal"}};
  AFFT_CHECK(c.gamma >= 0.f && c.gamma < INFINITY, "%s: gamma must be finite and >= 0 (got %g)", names[c.frames][2], (double)c.gamma);
  // The kernel is the narrowest one that serves the options, and so are its bits: 2 = softmax_ce_focal_kernel (an adjustment or a
  // focal exponent), 1 = softmax_ce_kernel<true> (class weights or smoothing), 0 = softmax_ce_kernel<false>.  The messages carry the
  // name of the entry point of that kernel, whichever entry the call came through.
  const int kern = c.adjust || c.gamma != 0.f ? 2 : c.weight || c.smoothing != 0.f ? 1 : 0;
  const char* name = names[c.frames][kern];
  AFFT_CHECK(c.smoothing >= 0.f && c.smoothing <= 1.f, "%s: smoothing must lie in [0, 1] (got %g)", name, (double)c.smoothing);
  AFFT_CHECK(c.logits, "%s: null logits", name);
  AFFT_CHECK((c.labels != nullptr) != (c.soft != nullptr), "%s: give exactly one of labels / soft targets", name);
  AFFT_CHECK(c.C > 0 && c.ldl >= c.C && (!c.dlogits || c.ldd >= c.C) && (!c.frames || c.period > 0), "%s: bad sizes", name);
  AFFT_CHECK(!c.loss_sum || c.row_loss, "%s: loss_sum is the ordered sum of row_loss: give row_loss as well", name);
  if (c.rows == 0) return 0;
  auto launch = [&](auto kernel, auto... options) {
    hipLaunchKernelGGL(kernel, dim3(c.rows), dim3(256), 0, stream, c.logits, c.ldl, c.C, c.labels, c.soft, c.lds, c.keep, c.gscale,
                       c.row_g, c.dlogits, c.ldd, c.d_dtype, c.row_loss, c.period, c.lgs, c.dgs, options...);
  };
  if (kern == 0) launch(softmax_ce_kernel<false>, (const float*)nullptr, 0.f);
  else if (kern == 1) launch(softmax_ce_kernel<true>, c.weight, c.smoothing);
  else launch(softmax_ce_focal_kernel, c.weight, c.smoothing, c.adjust, c.gamma);
  AFFT_LAUNCH_CHECK();
  if (c.loss_sum) {
    hipLaunchKernelGGL(ordered_sum_kernel, dim3(1), dim3(256), 0, stream, c.row_loss, (int64_t)c.rows, 1.0f, c.loss_sum, 1);
    AFFT_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int afft_softmax_ce(const float* logits, int64_t ldl, int32_t rows, int32_t C, const int64_t* labels,
                               const float* soft, int64_t lds, const uint8_t* keep, float gscale, const float* row_g,
                               float* loss_sum, void* dlogits, int64_t ldd, int32_t d_dtype, float* row_loss,
                               void* stream_) {
  return afft_softmax_ce_focal(logits, ldl, rows, C, labels, soft, lds, keep, gscale, row_g, loss_sum, dlogits, ldd, d_dtype, row_loss,
                               nullptr, 0.f, nullptr, 0.f, stream_);
}

extern "C" int afft_softmax_ce_frames(const float* logits, int64_t clip_stride, int64_t ldl, int32_t clips, int32_t frames, int32_t C,
                                      const int64_t* labels, const float* soft, int64_t lds, const uint8_t* keep, float gscale,
                                      const float* row_g, void* dlogits, int64_t d_clip_stride, int64_t ldd, int32_t d_dtype,
                                      float* row_loss, void* stream_) {
  return afft_softmax_ce_frames_focal(logits, clip_stride, ldl, clips, frames, C, labels, soft, lds, keep, gscale, row_g, dlogits,
                                      d_clip_stride, ldd, d_dtype, row_loss, nullptr, 0.f, nullptr, 0.f, stream_);
}

// Class weights and label smoothing.  A null weight with smoothing == 0 IS the plain loss: the sibling's launch, the sibling's bits.
extern "C" int afft_softmax_ce_w(const float* logits, int64_t ldl, int32_t rows, int32_t C, const int64_t* labels,
                                 const float* soft, int64_t lds, const uint8_t* keep, float gscale, const float* row_g,
                                 float* loss_sum, void* dlogits, int64_t ldd, int32_t d_dtype, float* row_loss,
                                 const float* weight, float smoothing, void* stream_) {
  return afft_softmax_ce_focal(logits, ldl, rows, C, labels, soft, lds, keep, gscale, row_g, loss_sum, dlogits, ldd, d_dtype, row_loss,
                               weight, smoothing, nullptr, 0.f, stream_);
}

extern "C" int afft_softmax_ce_frames_w(const float* logits, int64_t clip_stride, int64_t ldl, int32_t clips, int32_t frames, int32_t C,
                                        const int64_t* labels, const float* soft, int64_t lds, const uint8_t* keep, float gscale,
                                        const float* row_g, void* dlogits, int64_t d_clip_stride, int64_t ldd, int32_t d_dtype,
                                        float* row_loss, const float* weight, float smoothing, void* stream_) {
  return afft_softmax_ce_frames_focal(logits, clip_stride, ldl, clips, frames, C, labels, soft, lds, keep, gscale, row_g, dlogits,
                                      d_clip_stride, ldd, d_dtype, row_loss, weight, smoothing, nullptr, 0.f, stream_);
}

// Focal exponent and logit adjustment.  gamma == 0 with a null adjust IS the weighted loss: the sibling's launch, the sibling's bits.
extern "C" int afft_softmax_ce_focal(const float* logits, int64_t ldl, int32_t rows, int32_t C, const int64_t* labels,
                                     const float* soft, int64_t lds, const uint8_t* keep, float gscale, const float* row_g,
                                     float* loss_sum, void* dlogits, int64_t ldd, int32_t d_dtype, float* row_loss,
                                     const float* weight, float smoothing, const float* adjust, float gamma, void* stream_) {
  return ce_launch({logits, 0, ldl, rows, rows, C, labels, soft, lds, keep, gscale, row_g, dlogits, 0, ldd, d_dtype, row_loss,
                    weight, smoothing, adjust, gamma, loss_sum, false, stream_});
}

extern "C" int afft_softmax_ce_frames_focal(const float* logits, int64_t clip_stride, int64_t ldl, int32_t clips, int32_t frames, int32_t C,
                                            const int64_t* labels, const float* soft, int64_t lds, const uint8_t* keep, float gscale,
                                            const float* row_g, void* dlogits, int64_t d_clip_stride, int64_t ldd, int32_t d_dtype,
                                            float* row_loss, const float* weight, float smoothing, const float* adjust, float gamma,
                                            void* stream_) {
  return ce_launch({logits, clip_stride, ldl, clips * frames, frames, C, labels, soft, lds, keep, gscale, row_g, dlogits, d_clip_stride,
                    ldd, d_dtype, row_loss, weight, smoothing, adjust, gamma, nullptr, true, stream_});
}

// One marginal cross-entropy call, from either of its two entry points (as CeCall / ce_launch above).
struct CeGroupsCall {
  const float* logits; int64_t lgs, ldl;
  int32_t rows, period, C, G;
  const int32_t* group_of; const int32_t* members; const int32_t* offs;
  const int64_t* glabels; const float* gsoft; int64_t ldgs; const uint8_t* keep; float gscale; const float* row_g;
  void* dlogits; int64_t dgs, ldd; int32_t d_dtype; float* row_loss;
  float* loss_sum;
  bool frames;
  void* stream;
};

static int ce_groups_launch(const CeGroupsCall& c) {
  hipStream_t stream = (hipStream_t)c.stream;
  const char* name = c.frames ? "softmax_ce_frames_groups" : "softmax_ce_groups";
  AFFT_CHECK(c.G >= 1 && c.G <= AFFT_CE_GROUPS_MAX, "%s: the number of groups G must lie in [1, %d] (got %d)", name, AFFT_CE_GROUPS_MAX, c.G);
  AFFT_CHECK(c.logits, "%s: null logits", name);
  AFFT_CHECK((c.glabels != nullptr) != (c.gsoft != nullptr), "%s: give exactly one of group labels / soft group targets", name);
  AFFT_CHECK(c.C > 0 && c.ldl >= c.C && (!c.dlogits || c.ldd >= c.C) && (!c.gsoft || c.ldgs >= c.G) && (!c.frames || c.period > 0),
             "%s: bad sizes", name);
  // members may be null: no class is in any group (every offset is 0, nothing is read through it)
  AFFT_CHECK(c.group_of && c.offs, "%s: null group_of / offs", name);
  AFFT_CHECK((((uintptr_t)c.group_of | (uintptr_t)c.members | (uintptr_t)c.offs) & 3) == 0,
             "%s: group_of, members and offs must be 4-byte aligned", name);
  AFFT_CHECK(!c.loss_sum || c.row_loss, "%s: loss_sum is the ordered sum of row_loss: give row_loss as well", name);
  if (c.rows == 0) return 0;
  hipLaunchKernelGGL(softmax_ce_groups_kernel, dim3(c.rows), dim3(256), 0, stream, c.logits, c.ldl, c.C, c.G, c.group_of, c.members,
                     c.offs, c.glabels, c.gsoft, c.ldgs, c.keep, c.gscale, c.row_g, c.dlogits, c.ldd, c.d_dtype, c.row_loss, c.period,
                     c.lgs, c.dgs);
  AFFT_LAUNCH_CHECK();
  if (c.loss_sum) {
    hipLaunchKernelGGL(ordered_sum_kernel, dim3(1), dim3(256), 0, stream, c.row_loss, (int64_t)c.rows, 1.0f, c.loss_sum, 1);
    AFFT_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int afft_softmax_ce_groups(const float* logits, int64_t ldl, int32_t rows, int32_t C, int32_t G, const int32_t* group_of,
                                      const int32_t* members, const int32_t* offs, const int64_t* glabels, const float* gsoft,
                                      int64_t ldgs, const uint8_t* keep, float gscale, const float* row_g, float* loss_sum,
                                      void* dlogits, int64_t ldd, int32_t d_dtype, float* row_loss, void* stream_) {
  return ce_groups_launch({logits, 0, ldl, rows, rows, C, G, group_of, members, offs, glabels, gsoft, ldgs, keep, gscale, row_g,
                           dlogits, 0, ldd, d_dtype, row_loss, loss_sum, false, stream_});
}

extern "C" int afft_softmax_ce_frames_groups(const float* logits, int64_t clip_stride, int64_t ldl, int32_t clips, int32_t frames,
                                             int32_t C, int32_t G, const int32_t* group_of, const int32_t* members,
                                             const int32_t* offs, const int64_t* glabels, const float* gsoft, int64_t ldgs,
                                             const uint8_t* keep, float gscale, const float* row_g, void* dlogits,
                                             int64_t d_clip_stride, int64_t ldd, int32_t d_dtype, float* row_loss, void* stream_) {
  return ce_groups_launch({logits, clip_stride, ldl, clips * frames, frames, C, G, group_of, members, offs, glabels, gsoft, ldgs, keep,
                           gscale, row_g, dlogits, d_clip_stride, ldd, d_dtype, row_loss, nullptr, true, stream_});
}

extern "C" int afft_mse_frames_bwd(const float* a, int64_t a_clip_stride, int32_t a_off, int32_t a_len, const float* b,
                                   int64_t b_clip_stride, int32_t b_off, int32_t b_len, int32_t clips, int32_t n, float gscale,
                                   const float* g_dev, float* da, float* db, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AFFT_CHECK(a && b, "mse_frames_bwd: null pointer");
  AFFT_CHECK(((a_off | a_len | b_off | b_len | n) & 3) == 0 && (a_clip_stride & 3) == 0 && (b_clip_stride & 3) == 0,
             "mse_frames_bwd: offsets, lengths and clip strides must be multiples of 4 floats");
  AFFT_CHECK(a_off >= 0 && b_off >= 0 && a_off + n <= a_len && b_off + n <= b_len, "mse_frames_bwd: the frame range leaves the tensor");
  AFFT_CHECK((((uintptr_t)a | (uintptr_t)b | (uintptr_t)da | (uintptr_t)db) & 15) == 0, "mse_frames_bwd: 16-byte aligned pointers");
  if (clips == 0 || (!da && !db)) return 0;
  const int span = a_len > b_len ? a_len : b_len;
  int gx = (span / 4 + 255) / 256;
  if (gx > 64) gx = 64;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(mse_frames_bwd_kernel, dim3(gx, clips), dim3(256), 0, stream, a, a_clip_stride, a_off, a_len, b, b_clip_stride,
                     b_off, b_len, clips, n, gscale, g_dev, da, db);
  AFFT_LAUNCH_CHECK();
  return 0;
}

static int mse_launch(const float* a, int64_t lda, const float* b, int64_t ldb, int32_t rows, int32_t d,
                      float gscale, const float* g_dev, float lscale, float* loss_sum, float* da, int64_t ldda,
                      float* db, int64_t lddb, void* workspace, int64_t workspace_bytes, int accumulate, hipStream_t stream) {
  AFFT_CHECK(a && b, "mse: null pointer");
  if (rows == 0 || d == 0) return 0;
  const int64_t total = (int64_t)rows * d;
  int grid = (int)((total + 255) / 256);
  if (grid > AFFT_REDUCE_PARTIALS) grid = AFFT_REDUCE_PARTIALS;
  AFFT_CHECK(!loss_sum || grid == 1 || (workspace && workspace_bytes >= AFFT_GEMM_WS_HEADER + 4 * (int64_t)grid),
             "mse: the loss sum needs the stream's workspace (header + AFFT_REDUCE_PARTIALS floats)");
  float* scratch = workspace ? (float*)((char*)workspace + AFFT_GEMM_WS_HEADER) : nullptr;
  hipLaunchKernelGGL(mse_kernel, dim3(grid), dim3(256), 0, stream, a, lda, b, ldb, rows, d, gscale, g_dev, lscale, loss_sum,
                     scratch, da, ldda, db, lddb, accumulate);
  AFFT_LAUNCH_CHECK();
  if (loss_sum && grid > 1) {
    hipLaunchKernelGGL(ordered_sum_kernel, dim3(1), dim3(256), 0, stream, scratch, (int64_t)grid, lscale, loss_sum, accumulate);
    AFFT_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int afft_mse(const float* a, int64_t lda, const float* b, int64_t ldb, int32_t rows, int32_t d,
                        float gscale, const float* g_dev, float lscale, float* loss_sum, float* da, int64_t ldda,
                        float* db, int64_t lddb, void* workspace, int64_t workspace_bytes, void* stream_) {
  return mse_launch(a, lda, b, ldb, rows, d, gscale, g_dev, lscale, loss_sum, da, ldda, db, lddb, workspace, workspace_bytes, 1,
                    (hipStream_t)stream_);
}

extern "C" int afft_mse_loss(const float* a, int64_t lda, const float* b, int64_t ldb, int32_t rows, int32_t d, float lscale,
                             float* loss, void* workspace, int64_t workspace_bytes, void* stream_) {
  AFFT_CHECK(loss, "mse_loss: null output");
  return mse_launch(a, lda, b, ldb, rows, d, 0.f, nullptr, lscale, loss, nullptr, 0, nullptr, 0, workspace, workspace_bytes, 0,
                    (hipStream_t)stream_);
}
