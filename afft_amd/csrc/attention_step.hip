// Causal attention of Lq new rows per sequence against a key / value cache, and the append of those rows to the cache, in one launch:
// the step of a GPT-2 roll-out (models/future_prediction.py:395-412 -- the first pass runs the T observed frames and keeps every layer's
// keys and values, each further frame is one new row per clip attending to them).  Query row i sits at position past + i, past = Lk - Lq,
// and sees keys 0 .. past + i: rows [0, past) of the cache, then the new rows themselves.
// One workgroup per (sequence, head, tile of STEP_QT new rows).  A workgroup writes rows [past + i0, past + i0 + rows) of ITS head's hd
// columns of both caches and reads the new keys and values from k_new / v_new, never back from the cache: no workgroup reads what
// another one writes, so the append needs no ordering.  fp32 VALU arithmetic (one query row is a sixteenth of an MFMA tile; the kernel
// is bound by the Lk x hd bytes it reads): K and V go straight to registers in 16-byte loads, lanes stride the head dimension, sums run
// in a fixed order (per lane front to back, the wave's xor tree, waves 0..3) -- no atomics, two runs give the same bits.
// Which form runs (16-byte or element loads), LDS bytes and grid are attn_plan.h's decision (plan_attention_step).
// DROP (afft_attention_step_fwd_drop with p > 0): attention-probability dropout by attention.hip's convention -- probs receives the
// PRE-dropout probabilities, the product uses P' = P o M, M = 1 / (1 - p) for a kept element and 0 for a dropped one, decided by
// drop_keep on the element's index in probs[nseq, H, Lq, Lk].  DROP = false is the kernel as it was, bit for bit.
// Storage (the kernel's first template parameter): Dense<float> / Dense<bf16_t> -- every operand in one dtype, the append a copy of bits;
// Planes (afft_attention_step_fwd_split, the "fp16x2" forward) -- q / k_new / v_new as fp16 hi planes with an optional lo plane in_lo
// elements behind (value float(hi) + float(lo)), fp32 caches that take that value, out as fp16 hi (+ lo, out_lo elements behind:
// hi = fp16(x), lo = fp16(x - hi)).  The arithmetic between load and store is the same code.
// The backward (attn_step_bwd_kernel) is at the end of the file.
#include "common.h"
#include "attn_plan.h"

using namespace afft_attn_detail;

namespace {

struct StepArgs {
  const void *q, *kn, *vn;
  int64_t ldq, ldk, ldv;
  void *kc, *vc;
  int64_t ldc, cseq;
  void* out;
  int64_t ldo;
  float* probs;
  int Lq, Lk, H, hd, ntiles, LkP;
  float scale;
  unsigned dthresh, dkey;      // make_drop's: threshold (0: off), key, 1 / (1 - p), the device salt
  float dinv;
  const unsigned* salt;
  int64_t in_lo, out_lo;       // Planes: distance (elements) to the lo planes of q / k_new / v_new and of out; 0: none
};

template <typename T> struct StepElem;      // N: elements of one 16-byte access
template <> struct StepElem<float> { static constexpr int N = 4; };
template <> struct StepElem<bf16_t> { static constexpr int N = 8; };

// x = p[c .. c + N) as fp32: one 16-byte load (V: hd is a multiple of N), else element loads that stop at hd
template <typename T, bool V>
__device__ __forceinline__ void ld_cols(const T* p, int c, int hd, float (&x)[StepElem<T>::N]) {
  if constexpr (V) {
    if constexpr (StepElem<T>::N == 4) load4(p, c, AFFT_F32, x); else load8(p, c, AFFT_BF16, x);
  } else {
#pragma unroll
    for (int e = 0; e < StepElem<T>::N; ++e) x[e] = c + e < hd ? Elem<T>::ld(p + c + e) : 0.f;
  }
}
template <typename T, bool V>
__device__ __forceinline__ void st_cols(T* p, int c, int hd, const float (&x)[StepElem<T>::N]) {
  if constexpr (V) {
    if constexpr (StepElem<T>::N == 4) store4(p, c, AFFT_F32, x); else store8(p, c, AFFT_BF16, x);
  } else {
#pragma unroll
    for (int e = 0; e < StepElem<T>::N; ++e)
      if (c + e < hd) Elem<T>::st(p + c + e, x[e]);
  }
}
// dst[c .. c + N) = src[c .. c + N), the bits as they are
template <typename T, bool V>
__device__ __forceinline__ void copy_cols(T* dst, const T* src, int c, int hd) {
  if constexpr (V) {
    *(uint4*)(dst + c) = *(const uint4*)(src + c);
  } else {
#pragma unroll
    for (int e = 0; e < StepElem<T>::N; ++e)
      if (c + e < hd) dst[c + e] = src[c + e];
  }
}

// fp32 rows (the backward's gradient caches, the caches of Planes): x = p[c .. c + N) (V: N / 4 16-byte accesses)
template <int N, bool V>
__device__ __forceinline__ void ldf_cols(const float* p, int c, int hd, float (&x)[N]) {
#pragma unroll
  for (int e = 0; e < N; e += 4) {
    if constexpr (V) {
      const float4 f = *(const float4*)(p + c + e);
      x[e] = f.x; x[e + 1] = f.y; x[e + 2] = f.z; x[e + 3] = f.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) x[e + u] = c + e + u < hd ? p[c + e + u] : 0.f;
    }
  }
}
template <int N, bool V>
__device__ __forceinline__ void stf_cols(float* p, int c, int hd, const float (&x)[N]) {
#pragma unroll
  for (int e = 0; e < N; e += 4) {
    if constexpr (V) {
      *(float4*)(p + c + e) = make_float4(x[e], x[e + 1], x[e + 2], x[e + 3]);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (c + e + u < hd) p[c + e + u] = x[e + u];
    }
  }
}


// ---- storage of a step's rows (see the head of the file): element types, the elements N a lane takes per access, a key / value row
// (from the cache below `past`, else from the new rows), loads to fp32, the append, the store of out
template <typename T> struct Dense {
  using In = T; using Cache = T; using Out = T;
  static constexpr int N = StepElem<T>::N;
  using Row = const T*;
  static __device__ __forceinline__ Row row(const T* ch, int64_t ldc, const T* nh, int64_t ldn, int j, int past) {
    return j < past ? ch + (int64_t)j * ldc : nh + (int64_t)(j - past) * ldn;
  }
  template <bool V> static __device__ __forceinline__ void ld_new(const T* p, int c, int hd, int64_t, float (&x)[N]) { ld_cols<T, V>(p, c, hd, x); }
  template <bool V> static __device__ __forceinline__ void ld_row(Row r, int c, int hd, int64_t, float (&x)[N]) { ld_cols<T, V>(r, c, hd, x); }
  template <bool V> static __device__ __forceinline__ void append(T* dst, const T* src, int c, int hd, int64_t) { copy_cols<T, V>(dst, src, c, hd); }
  template <bool V> static __device__ __forceinline__ void st(T* p, int c, int hd, int64_t, const float (&x)[N]) { st_cols<T, V>(p, c, hd, x); }
};
struct Planes {
  using In = bf16_t; using Cache = float; using Out = bf16_t;      // (fp16 bits in 16-bit words, as common.h carries them)
  static constexpr int N = 8;
  struct Row { const float* c; const bf16_t* n; };                  // one of the two
  static __device__ __forceinline__ Row row(const float* ch, int64_t ldc, const bf16_t* nh, int64_t ldn, int j, int past) {
    return j < past ? Row{ch + (int64_t)j * ldc, nullptr} : Row{nullptr, nh + (int64_t)(j - past) * ldn};
  }
  template <bool V> static __device__ __forceinline__ void ld_new(const bf16_t* p, int c, int hd, int64_t lo, float (&x)[N]) {
    if constexpr (V) {
      load8(p, c, AFFT_F16, x);
      if (lo) {
        float l[N];
        load8(p, c + lo, AFFT_F16, l);
#pragma unroll
        for (int e = 0; e < N; ++e) x[e] += l[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < N; ++e) x[e] = c + e < hd ? (lo ? h2f(p[c + e]) + h2f(p[c + e + lo]) : h2f(p[c + e])) : 0.f;
    }
  }
  template <bool V> static __device__ __forceinline__ void ld_row(Row r, int c, int hd, int64_t lo, float (&x)[N]) {
    if (r.c) ldf_cols<N, V>(r.c, c, hd, x); else ld_new<V>(r.n, c, hd, lo, x);
  }
  template <bool V> static __device__ __forceinline__ void append(float* dst, const bf16_t* src, int c, int hd, int64_t lo) {
    float x[N];
    ld_new<V>(src, c, hd, lo, x);
    stf_cols<N, V>(dst, c, hd, x);
  }
  template <bool V> static __device__ __forceinline__ void st(bf16_t* p, int c, int hd, int64_t lo, const float (&x)[N]) {
    if constexpr (V) {
      if (lo) store_split<N>(p, c, lo, x); else store8(p, c, AFFT_F16, x);
    } else {
#pragma unroll
      for (int e = 0; e < N; ++e)
        if (c + e < hd) {
          const bf16_t h = f2h(x[e]);
          p[c + e] = h;
          if (lo) p[c + e + lo] = f2h(x[e] - h2f(h));
        }
    }
  }
};

template <typename IO, bool V, bool DROP>
__global__ __launch_bounds__(256) void attn_step_kernel(const StepArgs a) {
  using TI = typename IO::In;
  using TC = typename IO::Cache;
  constexpr int N = IO::N, NT = 1024 / (64 * N);      // a lane owns columns (lane + 64 t) N .. + N, t < NT: hd <= 1024
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int tile = blockIdx.x % a.ntiles, sh = blockIdx.x / a.ntiles, h = sh % a.H, seq = sh / a.H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Lq = a.Lq, Lk = a.Lk, hd = a.hd, LkP = a.LkP, past = Lk - Lq;
  const int i0 = tile * STEP_QT, nr = min(STEP_QT, Lq - i0);      // this workgroup's new rows i0 .. i0 + nr
  const int rows = min(STEP_QT, Lq), hdP = (hd + 7) & ~7;         // the LDS carve is the plan's: the same for every tile
  float* sc = reinterpret_cast<float*>(smem_raw);                 // [rows][LkP] scores, then probabilities
  float* part = sc + rows * LkP;                                  // [3][rows][hdP] P V partial sums of waves 1..3

  const int64_t new0 = (int64_t)seq * Lq, hcol = (int64_t)h * hd;
  const TI* qh = (const TI*)a.q + new0 * a.ldq + hcol;
  const TI* knh = (const TI*)a.kn + new0 * a.ldk + hcol;
  const TI* vnh = (const TI*)a.vn + new0 * a.ldv + hcol;
  TC* kch = (TC*)a.kc + seq * a.cseq + hcol;
  TC* vch = (TC*)a.vc + seq * a.cseq + hcol;

  // the append: rows past + i of both caches become rows i of k_new / v_new (i < Lq, so past + i < Lk <= cap)
  const int nv = (hd + N - 1) / N;
  for (int idx = tid; idx < nr * nv; idx += 256) {
    const int i = i0 + idx / nv, c = (idx % nv) * N;
    IO::template append<V>(kch + (int64_t)(past + i) * a.ldc, knh + (int64_t)i * a.ldk, c, hd, a.in_lo);
    IO::template append<V>(vch + (int64_t)(past + i) * a.ldc, vnh + (int64_t)i * a.ldv, c, hd, a.in_lo);
  }

  // scores: a wave takes (row, 4 keys) at a time -- the row in registers, the 4 x NT loads of the keys independent of each other
  const int nchunk = (Lk + 3) / 4;
  for (int item = wave; item < nr * nchunk; item += 4) {
    const int r = item / nchunk, j0 = (item % nchunk) * 4, i = i0 + r, last = past + i;      // row i sees keys 0 .. last
    if (j0 > last) continue;
    float qv[NT][N];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = (lane + 64 * t) * N;
      if (c < hd) {
        IO::template ld_new<V>(qh + (int64_t)i * a.ldq, c, hd, a.in_lo, qv[t]);
      } else {
#pragma unroll
        for (int e = 0; e < N; ++e) qv[t][e] = 0.f;
      }
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u;
      if (j <= last) {
        const typename IO::Row kr = IO::row(kch, a.ldc, knh, a.ldk, j, past);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int c = (lane + 64 * t) * N;
          if (c < hd) {
            float kx[N];
            IO::template ld_row<V>(kr, c, hd, a.in_lo, kx);
#pragma unroll
            for (int e = 0; e < N; ++e) acc[u] += qv[t][e] * kx[e];
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u;
      if (j <= last) {
        const float s = wave_sum(acc[u]) * a.scale;
        if (lane == 0) sc[r * LkP + j] = s;
      }
    }
  }
  __syncthreads();

  // softmax over the whole row in fp32, one wave per row; keys behind `last` are masked: probability exactly 0
  if (wave < nr) {
    const int i = i0 + wave, last = past + i;
    float* row = sc + wave * LkP;
    float m = -INFINITY;
    for (int j = lane; j <= last; j += 64) m = fmaxf(m, row[j]);
    m = wave_max(m);
    float sum = 0.f;
    for (int j = lane; j <= last; j += 64) {
      const float e = expf(row[j] - m);
      row[j] = e;
      sum += e;
    }
    const float inv = 1.0f / wave_sum(sum);
    float* pr = a.probs ? a.probs + ((((int64_t)seq * a.H + h) * Lq + i) * Lk) : nullptr;
    if constexpr (DROP) {
      const unsigned dkey = a.salt ? a.dkey ^ *a.salt : a.dkey, base = (unsigned)((((int64_t)seq * a.H + h) * Lq + i) * Lk);
      for (int j = lane; j < Lk; j += 64) {
        const float p = j <= last ? row[j] * inv : 0.f;
        if (pr) pr[j] = p;      // pre-dropout probabilities (the backward regenerates the mask)
        row[j] = (a.dthresh && !drop_keep(dkey, base + j, a.dthresh)) ? 0.f : p * a.dinv;
      }
    } else {
      for (int j = lane; j < Lk; j += 64) {
        const float p = j <= last ? row[j] * inv : 0.f;
        row[j] = p;
        if (pr) pr[j] = p;
      }
    }
  }
  __syncthreads();

  // P V: wave w takes keys w, w + 4, .. for every row of the tile (a masked key has p = 0 and a finite, new value row)
  float acc[STEP_QT][NT][N];
#pragma unroll
  for (int r = 0; r < STEP_QT; ++r)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int e = 0; e < N; ++e) acc[r][t][e] = 0.f;
  const int jend = past + i0 + nr;      // the keys the tile's last row sees
#pragma unroll 2
  for (int j = wave; j < jend; j += 4) {
    const typename IO::Row vr = IO::row(vch, a.ldc, vnh, a.ldv, j, past);
    float pj[STEP_QT];
#pragma unroll
    for (int r = 0; r < STEP_QT; ++r) pj[r] = r < nr ? sc[r * LkP + j] : 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = (lane + 64 * t) * N;
      if (c < hd) {
        float vx[N];
        IO::template ld_row<V>(vr, c, hd, a.in_lo, vx);
#pragma unroll
        for (int r = 0; r < STEP_QT; ++r)
#pragma unroll
          for (int e = 0; e < N; ++e) acc[r][t][e] += pj[r] * vx[e];
      }
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < STEP_QT; ++r)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int c = (lane + 64 * t) * N;
        if (r < nr && c < hd) {
          float* dst = part + ((wave - 1) * rows + r) * hdP + c;
#pragma unroll
          for (int e = 0; e < N; ++e) dst[e] = acc[r][t][e];
        }
      }
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int r = 0; r < STEP_QT; ++r)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int c = (lane + 64 * t) * N;
        if (r < nr && c < hd) {
          for (int w = 0; w < 3; ++w) {
            const float* src = part + (w * rows + r) * hdP + c;
#pragma unroll
            for (int e = 0; e < N; ++e) acc[r][t][e] += src[e];
          }
          IO::template st<V>((typename IO::Out*)a.out + (new0 + i0 + r) * a.ldo + hcol, c, hd, a.out_lo, acc[r][t]);
        }
      }
  }
}

template <typename IO, bool V, bool DROP>
int launch_step(const StepArgs& a, const AttnPlan& p, hipStream_t stream) {
  auto kern = attn_step_kernel<IO, V, DROP>;
  static std::atomic<uint64_t> attr{0};
  if (p.lds > 48 * 1024)
    if (int rc = afft_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), p.lds, &attr)) return rc;
  hipLaunchKernelGGL(kern, dim3(p.grid), dim3(256), p.lds, stream, a);
  return 0;
}

// ---- the backward of the step.  One workgroup owns a (sequence, head): its hd columns of every row it writes, so no two workgroups
// touch the same address and nothing is atomic.  With past = Lk - Lq and query row i seeing keys 0 .. past + i:
//   dP' = dO V^T, dP = dP' o M, r_i = sum_j P_ij dP_ij, dS = P o (dP - r), dq = scale dS K, cK = scale dS^T Q, cV = P'^T dO.
// Two passes, as attention_long.hip forms dP twice.  The query pass walks tiles of STEP_QT rows with the forward's three stages and its
// LDS carve (dP of the tile -> dS, one wave per row, which also leaves r_i in LDS -> dS K over waves 0..3), the key pass gives wave w
// the keys w, w + 4, ..: per key it recomputes dP_ij against the value row it holds in registers, for every query row that sees the key,
// front to back.  Write rule: rows j < past of the fp32 gradient caches take += cK / cV (later steps have left theirs there already);
// rows past <= j < Lk are read, never written: dk_new[j - past] = gk_cache[j] + cK[j] in the storage dtype, dv_new alike.
struct StepBwdArgs {
  const void *dout, *q, *kc, *vc;
  int64_t lddo, ldq, ldc, cseq;
  const float* probs;
  void *dq, *dk, *dv;
  int64_t lddq, lddk, lddv;
  float *gk, *gv;
  int64_t ldg, gseq;
  int Lq, Lk, H, hd, LkP;
  float scale;
  unsigned dthresh, dkey;
  float dinv;
  const unsigned* salt;
};

template <typename T, bool V>
__global__ __launch_bounds__(256) void attn_step_bwd_kernel(const StepBwdArgs a) {
  constexpr int N = StepElem<T>::N, NT = 1024 / (64 * N);
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int h = blockIdx.x % a.H, seq = blockIdx.x / a.H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Lq = a.Lq, Lk = a.Lk, hd = a.hd, LkP = a.LkP, past = Lk - Lq;
  const int rows = min(STEP_QT, Lq), hdP = (hd + 7) & ~7;
  float* sc = reinterpret_cast<float*>(smem_raw);      // [rows][LkP] dP' of the tile, then dS
  float* part = sc + rows * LkP;                       // [3][rows][hdP] dS K partial sums of waves 1..3
  float* rterm = part + 3 * rows * hdP;                // [Lq] r_i
  const unsigned dkey = a.dthresh && a.salt ? a.dkey ^ *a.salt : a.dkey;

  const int64_t new0 = (int64_t)seq * Lq, hcol = (int64_t)h * hd;
  const T* doh = (const T*)a.dout + new0 * a.lddo + hcol;
  const T* qh = (const T*)a.q + new0 * a.ldq + hcol;
  const T* kch = (const T*)a.kc + seq * a.cseq + hcol;
  const T* vch = (const T*)a.vc + seq * a.cseq + hcol;
  const int64_t pbase = ((int64_t)seq * a.H + h) * Lq * Lk;      // this head's [Lq][Lk] block of probs; the index the mask is drawn on
  const float* ph = a.probs + pbase;

  // ---- the query pass: r_i and dq, a tile of STEP_QT rows at a time
  const int nchunk = (Lk + 3) / 4;
  for (int i0 = 0; i0 < Lq; i0 += STEP_QT) {
    const int nr = min(STEP_QT, Lq - i0);
    // dP'[i][j] = dO_i . V_j: a wave takes (row, 4 keys) at a time, as the forward's scores
    for (int item = wave; item < nr * nchunk; item += 4) {
      const int r = item / nchunk, j0 = (item % nchunk) * 4, i = i0 + r, last = past + i;
      if (j0 > last) continue;
      float dv_[NT][N];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int c = (lane + 64 * t) * N;
        if (c < hd) {
          ld_cols<T, V>(doh + (int64_t)i * a.lddo, c, hd, dv_[t]);
        } else {
#pragma unroll
          for (int e = 0; e < N; ++e) dv_[t][e] = 0.f;
        }
      }
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u;
        if (j <= last) {
          const T* vr = vch + (int64_t)j * a.ldc;
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const int c = (lane + 64 * t) * N;
            if (c < hd) {
              float vx[N];
              ld_cols<T, V>(vr, c, hd, vx);
#pragma unroll
              for (int e = 0; e < N; ++e) acc[u] += dv_[t][e] * vx[e];
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u;
        if (j <= last) {
          const float s = wave_sum(acc[u]);
          if (lane == 0) sc[r * LkP + j] = s;
        }
      }
    }
    __syncthreads();
    // one wave per row: dP = dP' o M, r = sum_j P dP (per lane front to back, then the xor tree), dS = scale P (dP - r); 0 behind `last`
    if (wave < nr) {
      const int i = i0 + wave, last = past + i;
      float* row = sc + wave * LkP;
      const float* pr = ph + (int64_t)i * Lk;
      const unsigned base = (unsigned)(pbase + (int64_t)i * Lk);
      float dot = 0.f;
      for (int j = lane; j <= last; j += 64) {
        const float m = (a.dthresh && !drop_keep(dkey, base + j, a.dthresh)) ? 0.f : a.dinv;
        const float dp = row[j] * m;
        row[j] = dp;
        dot += pr[j] * dp;
      }
      dot = wave_sum(dot);
      for (int j = lane; j < Lk; j += 64) row[j] = j <= last ? pr[j] * (row[j] - dot) * a.scale : 0.f;
      if (lane == 0) rterm[i] = dot;
    }
    __syncthreads();
    // dq = dS K: wave w takes keys w, w + 4, .. for every row of the tile
    float acc[STEP_QT][NT][N];
#pragma unroll
    for (int r = 0; r < STEP_QT; ++r)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < N; ++e) acc[r][t][e] = 0.f;
    const int jend = past + i0 + nr;
#pragma unroll 2
    for (int j = wave; j < jend; j += 4) {
      const T* kr = kch + (int64_t)j * a.ldc;
      float sj[STEP_QT];
#pragma unroll
      for (int r = 0; r < STEP_QT; ++r) sj[r] = r < nr ? sc[r * LkP + j] : 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int c = (lane + 64 * t) * N;
        if (c < hd) {
          float kx[N];
          ld_cols<T, V>(kr, c, hd, kx);
#pragma unroll
          for (int r = 0; r < STEP_QT; ++r)
#pragma unroll
            for (int e = 0; e < N; ++e) acc[r][t][e] += sj[r] * kx[e];
        }
      }
    }
    if (wave > 0) {
#pragma unroll
      for (int r = 0; r < STEP_QT; ++r)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int c = (lane + 64 * t) * N;
          if (r < nr && c < hd) {
            float* dst = part + ((wave - 1) * rows + r) * hdP + c;
#pragma unroll
            for (int e = 0; e < N; ++e) dst[e] = acc[r][t][e];
          }
        }
    }
    __syncthreads();      // (also: every wave is done with the tile's dS before the next tile's dP' lands on it)
    if (wave == 0) {
#pragma unroll
      for (int r = 0; r < STEP_QT; ++r)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int c = (lane + 64 * t) * N;
          if (r < nr && c < hd) {
            for (int w = 0; w < 3; ++w) {
              const float* src = part + (w * rows + r) * hdP + c;
#pragma unroll
              for (int e = 0; e < N; ++e) acc[r][t][e] += src[e];
            }
            st_cols<T, V>((T*)a.dq + (new0 + i0 + r) * a.lddq + hcol, c, hd, acc[r][t]);
          }
        }
    }
    // wave 0 reads `part` while the others go on: they write it again only behind the next tile's two barriers
  }
  __syncthreads();

  // ---- the key pass: wave w owns keys w, w + 4, ..; key j is seen by query rows max(0, j - past) .. Lq - 1
  for (int j = wave; j < Lk; j += 4) {
    float vx[NT][N], ak[NT][N], av[NT][N];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = (lane + 64 * t) * N;
#pragma unroll
      for (int e = 0; e < N; ++e) vx[t][e] = ak[t][e] = av[t][e] = 0.f;
      if (c < hd) ld_cols<T, V>(vch + (int64_t)j * a.ldc, c, hd, vx[t]);
    }
    for (int i = j > past ? j - past : 0; i < Lq; ++i) {
      float dx[NT][N], s = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int c = (lane + 64 * t) * N;
        if (c < hd) {
          ld_cols<T, V>(doh + (int64_t)i * a.lddo, c, hd, dx[t]);
#pragma unroll
          for (int e = 0; e < N; ++e) s += dx[t][e] * vx[t][e];
        } else {
#pragma unroll
          for (int e = 0; e < N; ++e) dx[t][e] = 0.f;
        }
      }
      s = wave_sum(s);
      const float m = (a.dthresh && !drop_keep(dkey, (unsigned)(pbase + (int64_t)i * Lk + j), a.dthresh)) ? 0.f : a.dinv;
      const float p = ph[(int64_t)i * Lk + j];
      const float ds = p * (s * m - rterm[i]) * a.scale, pm = p * m;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int c = (lane + 64 * t) * N;
        if (c < hd) {
          float qx[N];
          ld_cols<T, V>(qh + (int64_t)i * a.ldq, c, hd, qx);
#pragma unroll
          for (int e = 0; e < N; ++e) {
            ak[t][e] += ds * qx[e];
            av[t][e] += pm * dx[t][e];
          }
        }
      }
    }
    float* gkr = a.gk + seq * a.gseq + (int64_t)j * a.ldg + hcol;
    float* gvr = a.gv + seq * a.gseq + (int64_t)j * a.ldg + hcol;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = (lane + 64 * t) * N;
      if (c < hd) {
        float gk_[N], gv_[N];
        ldf_cols<N, V>(gkr, c, hd, gk_);
        ldf_cols<N, V>(gvr, c, hd, gv_);
#pragma unroll
        for (int e = 0; e < N; ++e) {
          gk_[e] += ak[t][e];
          gv_[e] += av[t][e];
        }
        if (j < past) {
          stf_cols<N, V>(gkr, c, hd, gk_);
          stf_cols<N, V>(gvr, c, hd, gv_);
        } else {
          st_cols<T, V>((T*)a.dk + (new0 + j - past) * a.lddk + hcol, c, hd, gk_);
          st_cols<T, V>((T*)a.dv + (new0 + j - past) * a.lddv + hcol, c, hd, gv_);
        }
      }
    }
  }
}

template <typename T, bool V>
int launch_step_bwd(const StepBwdArgs& a, const AttnPlan& p, hipStream_t stream) {
  auto kern = attn_step_bwd_kernel<T, V>;
  static std::atomic<uint64_t> attr{0};
  if (p.lds > 48 * 1024)
    if (int rc = afft_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), p.lds, &attr)) return rc;
  hipLaunchKernelGGL(kern, dim3(p.grid), dim3(256), p.lds, stream, a);
  return 0;
}

template <typename T, bool V>
int launch_step_fwd(const StepArgs& a, const AttnPlan& p, hipStream_t stream) {
  return p.p1 ? launch_step<Dense<T>, V, true>(a, p, stream) : launch_step<Dense<T>, V, false>(a, p, stream);
}

}  // namespace

int launch_attention_step(const AttnCall& c, const AttnPlan& p, hipStream_t stream) {
  afft_dropout_t dd = {c.drop_p, c.drop_key, 0.f, 0u, 1};
  const DropParams dp = make_drop(&dd);
  const bool f32 = c.dtype == AFFT_F32;
  int rc;
  if (p.family == kStepBwdVec) {
    const StepBwdArgs a = {c.dout, c.q, c.k_cache, c.v_cache, c.lddo, c.ldq, c.ldc, c.cache_seq, c.probs, c.dq, c.dk, c.dv, c.lddq, c.lddk,
                           c.lddv, c.gk_cache, c.gv_cache, c.ldg, c.grad_seq, c.Lq, c.L, c.H, c.hd, p.Lp, c.scale, dp.thresh, dp.key,
                           dp.inv_keep, dp.salt};
    rc = f32 ? (p.p0 ? launch_step_bwd<float, true>(a, p, stream) : launch_step_bwd<float, false>(a, p, stream))
             : (p.p0 ? launch_step_bwd<bf16_t, true>(a, p, stream) : launch_step_bwd<bf16_t, false>(a, p, stream));
  } else {
    const StepArgs a = {c.q, c.k, c.v, c.ldq, c.ldk, c.ldv, c.k_cache, c.v_cache, c.ldc, c.cache_seq, c.out, c.ldo, c.probs,
                        c.Lq, c.L, c.H, c.hd, p.ntiles, p.Lp, c.scale, dp.thresh, dp.key, dp.inv_keep, dp.salt, c.in_lo, c.out_lo};
    rc = p.family == kStepSplit ? (p.p0 ? launch_step<Planes, true, false>(a, p, stream) : launch_step<Planes, false, false>(a, p, stream))
       : f32 ? (p.p0 ? launch_step_fwd<float, true>(a, p, stream) : launch_step_fwd<float, false>(a, p, stream))
             : (p.p0 ? launch_step_fwd<bf16_t, true>(a, p, stream) : launch_step_fwd<bf16_t, false>(a, p, stream));
  }
  if (rc) return rc;
  AFFT_LAUNCH_CHECK();
  return 0;
}

// the step plan of a dense problem as its arguments describe it (one sequence, one head, rows of hd elements rounded up to whole
// 16-byte units at 16-byte aligned addresses -- or, pitch_alignment_ok = 0, rows that no 16-byte load can take)
extern "C" int afft_attention_step_plan_for(int32_t dtype, int32_t Lq, int32_t Lk, int32_t hd, int32_t pitch_alignment_ok, int64_t* lds_and_tiles) {
  const int64_t ld = (hd + 7) / 8 * 8 + (pitch_alignment_ok ? 0 : 1);
  void* x = reinterpret_cast<void*>(uintptr_t{4096});      // never dereferenced
  const AttnCall c = attn_step_call(x, ld, x, ld, x, ld, x, x, ld, ld * (Lk > 0 ? Lk : 1), dtype, 1, Lq, Lk, Lk, 1, hd, 1.f, x, ld, nullptr);
  const AttnPlan p = plan_attention(c);
  if (!p.family) { afft_set_error("%s", p.refusal); return -1; }
  if (lds_and_tiles) { lds_and_tiles[0] = (int64_t)p.lds; lds_and_tiles[1] = p.ntiles; }
  return p.family * 10000 + p.p0 * 10 + p.p1;
}

extern "C" int afft_attention_step_fwd(const void* q, int64_t ldq, const void* k_new, int64_t ldk, const void* v_new, int64_t ldv,
                                       void* k_cache, void* v_cache, int64_t ldc, int64_t cache_seq, int32_t dtype, int32_t nseq,
                                       int32_t Lq, int32_t Lk, int32_t cap, int32_t H, int32_t hd, float scale, void* out, int64_t ldo,
                                       float* probs, void* stream_) {
  const AttnCall c = attn_step_call(q, ldq, k_new, ldk, v_new, ldv, k_cache, v_cache, ldc, cache_seq, dtype, nseq, Lq, Lk, cap, H, hd, scale,
                                    out, ldo, probs);
  return run_attention("attention_step", c, kChkPtrs | kLenAll | kChkBatch | kChkHd | kChkDtype | kChkStep, 0, (hipStream_t)stream_);
}

extern "C" int afft_attention_step_fwd_drop(const void* q, int64_t ldq, const void* k_new, int64_t ldk, const void* v_new, int64_t ldv,
                                            void* k_cache, void* v_cache, int64_t ldc, int64_t cache_seq, int32_t dtype, int32_t nseq,
                                            int32_t Lq, int32_t Lk, int32_t cap, int32_t H, int32_t hd, float scale, float drop_p,
                                            uint32_t drop_key, void* out, int64_t ldo, float* probs, void* stream_) {
  const AttnCall c = attn_step_call(q, ldq, k_new, ldk, v_new, ldv, k_cache, v_cache, ldc, cache_seq, dtype, nseq, Lq, Lk, cap, H, hd, scale,
                                    out, ldo, probs, drop_p, drop_key);
  return run_attention("attention_step_drop", c, kChkPtrs | kLenAll | kChkDrop | kChkBatch | kChkHd | kChkDtype | kChkStep, 0, (hipStream_t)stream_);
}

extern "C" int afft_attention_step_bwd(const void* dout, int64_t lddo, const void* q, int64_t ldq, const void* k_cache, const void* v_cache,
                                       int64_t ldc, int64_t cache_seq, int32_t dtype, const float* probs, int32_t nseq, int32_t Lq,
                                       int32_t Lk, int32_t cap, int32_t H, int32_t hd, float scale, float drop_p, uint32_t drop_key,
                                       void* dq, int64_t lddq, void* dk_new, int64_t lddk, void* dv_new, int64_t lddv, float* gk_cache,
                                       float* gv_cache, int64_t ldg, int64_t grad_seq, void* stream_) {
  const AttnCall c = attn_step_bwd_call(dout, lddo, q, ldq, k_cache, v_cache, ldc, cache_seq, dtype, probs, nseq, Lq, Lk, cap, H, hd, scale,
                                        drop_p, drop_key, dq, lddq, dk_new, lddk, dv_new, lddv, gk_cache, gv_cache, ldg, grad_seq);
  return run_attention("attention_step_bwd", c, kChkPtrs | kLenAll | kChkDrop | kChkBatch | kChkHd | kChkDtype | kChkStep, 0, (hipStream_t)stream_);
}

// the plan of the fp16x2 step as afft_attention_step_plan_for describes a problem; in_lo / out_lo: are there lo planes (their offset does
// not change the kernel, only whether 16-byte accesses reach them, which pitch_alignment_ok states)
extern "C" int afft_attention_step_split_plan_for(int32_t Lq, int32_t Lk, int32_t hd, int32_t in_lo, int32_t out_lo, int32_t pitch_alignment_ok,
                                                  int64_t* lds_and_tiles) {
  const int64_t ld = (hd + 7) / 8 * 8 + (pitch_alignment_ok ? 0 : 1);
  void* x = reinterpret_cast<void*>(uintptr_t{4096});      // never dereferenced
  const int64_t plane = ld * (Lq > 0 ? Lq : 1);
  const AttnCall c = attn_step_split_call(x, ld, x, ld, x, ld, in_lo ? plane : 0, (float*)x, (float*)x, ld, ld * (Lk > 0 ? Lk : 1), 1, Lq, Lk, Lk, 1,
                                          hd, 1.f, x, ld, out_lo ? plane : 0, nullptr);
  const AttnPlan p = plan_attention(c);
  if (!p.family) { afft_set_error("%s", p.refusal); return -1; }
  if (lds_and_tiles) { lds_and_tiles[0] = (int64_t)p.lds; lds_and_tiles[1] = p.ntiles; }
  return p.family * 10000 + p.p0 * 10 + p.p1;
}

extern "C" int afft_attention_step_fwd_split(const void* q, int64_t ldq, const void* k_new, int64_t ldk, const void* v_new, int64_t ldv,
                                             int64_t in_lo, float* k_cache, float* v_cache, int64_t ldc, int64_t cache_seq, int32_t nseq,
                                             int32_t Lq, int32_t Lk, int32_t cap, int32_t H, int32_t hd, float scale, void* out_hi,
                                             int64_t ldo, int64_t out_lo, float* probs, void* stream_) {
  const AttnCall c = attn_step_split_call(q, ldq, k_new, ldk, v_new, ldv, in_lo, k_cache, v_cache, ldc, cache_seq, nseq, Lq, Lk, cap, H, hd, scale,
                                          out_hi, ldo, out_lo, probs);
  return run_attention("attention_step_split", c, kChkPtrs | kLenAll | kChkBatch | kChkHd | kChkStep | kChkStepPlanes, 0, (hipStream_t)stream_);
}
