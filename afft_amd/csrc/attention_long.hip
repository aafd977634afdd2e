// Attention for sequences of 129..512 tokens (the T-SA-Fuser at M*T > 128: models/fusion.py:121-215), forward and backward.
//
// The two short kernels keep a whole sequence in one workgroup (attention.hip: an L x L fp32 score matrix in LDS; attention_mfma.hip:
// L <= 64 in registers).  Here the work is tiled: one workgroup per (sequence, head, tile of QT = 32 rows).  Every kernel is built from
// two primitives around an fp32 "strip" [32][Lp] in LDS (Lp = L rounded up to 64; 66 KiB at L = 512):
//   dots   : strip[r][j] = A[tile row r] . B[row j]        (32 x L dot products over the head dimension)
//   matmul : out[r][c]   = sum_j strip[r][j] B[j][c]       (the strip times L rows of the head)
//   forward        (query tile) : dots(Q, K) -> mask, softmax over the whole strip, probs out, dropout -> matmul(V)     = out
//   backward, dQ   (query tile) : dots(dO, V) = dP' -> row term sum_j P dP (stored: row_term), dS -> matmul(K)          = dQ
//   backward, dK dV (key tile)  : strip = P'^T (from probs) -> matmul(dO) = dV ; dots(V, dO) = dP'^T -> dS^T -> matmul(Q) = dK
// The probabilities are materialised anyway (the fusers return the attention maps), so there is no online softmax, and the backward
// pass is two passes without a single atomic: the same inputs give the same bits.  dP is formed twice (once per pass, row-wise and
// column-wise); the row term is formed once and handed over through row_term (fp32 [nseq, H, L], caller's scratch).
//
// fp32 storage: fp32 arithmetic throughout (lanes stride the head dimension, as attention.hip).  bf16 storage with hd % 64 == 0 and
// 16-byte aligned rows: both primitives on v_mfma_f32_16x16x32_bf16, operands staged in LDS in hd chunks of <= 256 channels with the
// swizzle of attention_mfma.hip (row fragments by ds_read_b128, transposed fragments by ds_read_b64_tr_b16); any other bf16 shape, or
// AFFT_ATTN_GENERIC=1, takes the generic form with bf16 loads.
// Semantics are those of attention.hip: probs = PRE-dropout probabilities, masked entries exactly 0, dropout mask from (key, index).
// The additive bias of the forward pass is read through element strides (0 = broadcast over batch / head / row: afft_attention_long_fwd_bias);
// its gradient, for every L from 1 to 512, is the first half of the dQ pass without the score scale plus an ordered sum over the
// broadcast dimensions (afft_attention_bias_bwd: bias_bwd_ds_kernel, bias_bwd_reduce_kernel).
#include <stdlib.h>

#include "common.h"

namespace {

constexpr int LLO = 129, LHI = 512;
constexpr int QT = 32;            // rows of a tile
constexpr int KB = 64;            // rows of the other operand staged at a time (MFMA form)

struct LongArgs {
  const void *q, *k, *v, *dout;
  int64_t ldq, ldk, ldv, lddo;
  void *out, *dq, *dk, *dv;
  int64_t ldo, lddq, lddk, lddv;
  float* probs;           // fwd: written (may be null); bwd: read
  const float* addm;      // fwd: additive fp32 bias or null, element (seq, h, i, j) at addm[seq*sb + h*sh + i*si + j]
  int64_t sb, sh, si;     //      (a stride of 0 broadcasts; the [L][L] table is sb = sh = 0, si = L)
  float* dbias;           // bias gradient: dS of (seq, h, i, j) to dbias[seq*ob + h*oh + i*oi + j]
  int64_t ob, oh, oi;
  float* row_term;        // bwd: sum_j P_ij dP_ij, [nseq, H, L]
  int L, Lp, H, hd, hc, ntiles;
  float scale;
  int mask, period;
  unsigned dthresh, dkey;
  float dinv;
  const unsigned* salt;
};

__device__ __forceinline__ bool masked(int mask, int period, int i, int j) {
  return (mask == AFFT_MASK_DIAG && i == j) || (mask == AFFT_MASK_CAUSAL && j > i) ||
         (mask == AFFT_MASK_BLOCKCAUSAL && (j % period) > (i % period));
}

// ---- LDS operand tiles [R][hc] bf16, 32-byte unit u of row r stored at unit u ^ (r & 7) (the layout of attention_mfma.hip)
__device__ __forceinline__ int swz(int row, int row_bytes) { return row & 7 & ((row_bytes >> 5) - 1); }
__device__ __forceinline__ int tile_off(int row, int chunk16, int row_bytes) {
  return row * row_bytes + ((chunk16 ^ (swz(row, row_bytes) << 1)) << 4);
}
// rows [0, R) of src (offset by the caller to its first row, head and hd chunk); rows >= rows_valid are staged as zeros, never read
__device__ __forceinline__ void load_tile(const bf16_t* __restrict__ src, int64_t ld, int rows_valid, int R, int hc, char* lds) {
  const int cpr = hc >> 3;
  for (int idx = threadIdx.x; idx < R * cpr; idx += 256) {
    const int row = idx / cpr, ch = idx - row * cpr;
    uint4 val = make_uint4(0u, 0u, 0u, 0u);
    if (row < rows_valid) val = *(const uint4*)(src + (int64_t)row * ld + ch * 8);
    *(uint4*)(lds + tile_off(row, ch, hc * 2)) = val;
  }
}
__device__ __forceinline__ bf16x8 row_frag(const char* lds, int row, int chunk16, int row_bytes) {
  return *(const bf16x8*)(lds + tile_off(row, chunk16, row_bytes));
}
// lane (g, i) gets tile[row0 + 4g + j][16 cb + i], j = 0..3
__device__ __forceinline__ bf16x4 tr_frag(const char* lds, int row0, int cb, int lane, int row_bytes) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int r = row0 + 4 * g + q;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((AFFT_LDS bf16x4*)(lds + r * row_bytes + ((cb ^ swz(r, row_bytes)) << 5) + p * 8));
}
__device__ __forceinline__ void store_o4(bf16_t* dst, const f32x4& a) {
  uint2 u;
  u.x = (unsigned)f2bf(a[0]) | ((unsigned)f2bf(a[1]) << 16);
  u.y = (unsigned)f2bf(a[2]) | ((unsigned)f2bf(a[3]) << 16);
  *(uint2*)dst = u;
}

// ---- dots, MFMA: strip[r][j] = A[r] . B[j], r < 32, j < Lp.  A, B point at (first row, head); rows >= a_valid / b_valid count as zero.
// S^T tiles: the 16 B rows of a wave are the MFMA's A operand (rows on (lane >> 4, register)), the tile rows its B operand (lane & 15).
// The A chunk is staged once per hd chunk, the B rows pass in blocks of 64 (16 per wave); all Lp / 64 <= 8 accumulator pairs stay in
// registers across the hd chunks.
__device__ __forceinline__ void dots_mfma(const bf16_t* __restrict__ A, int64_t lda, int a_valid, const bf16_t* __restrict__ B,
                                          int64_t ldb, int b_valid, int hd, int hc, int Lp, float* strip, int sld, char* stage) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c15 = lane & 15;
  const int rb = hc * 2;
  char* As = stage;
  char* Bs = stage + QT * rb;
  f32x4 acc[LHI / KB][2];
#pragma unroll
  for (int kb = 0; kb < LHI / KB; ++kb) { acc[kb][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[kb][1] = acc[kb][0]; }
  for (int c = 0; c < hd; c += hc) {
    __syncthreads();                       // whoever used the stage before is done
    load_tile(A + c, lda, a_valid, QT, hc, As);
#pragma unroll
    for (int kb = 0; kb < LHI / KB; ++kb) {
      if (kb * KB < Lp) {
        if (kb) __syncthreads();           // the previous block has been consumed by every wave
        load_tile(B + (int64_t)kb * KB * ldb + c, ldb, b_valid - kb * KB, KB, hc, Bs);
        __syncthreads();
        for (int ks = 0; ks < hc / 32; ++ks) {
          const int ch = ks * 4 + g;
          const bf16x8 bf = row_frag(Bs, wave * 16 + c15, ch, rb);
          const bf16x8 a0 = row_frag(As, c15, ch, rb), a1 = row_frag(As, 16 + c15, ch, rb);
          acc[kb][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf, a0, acc[kb][0], 0, 0, 0);
          acc[kb][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf, a1, acc[kb][1], 0, 0, 0);
        }
      }
    }
  }
  // D[B row 4g + r][tile row c15] -> strip[tile row][4 consecutive columns]
#pragma unroll
  for (int kb = 0; kb < LHI / KB; ++kb)
    if (kb * KB < Lp) {
#pragma unroll
      for (int t = 0; t < 2; ++t) *(f32x4*)(strip + (t * 16 + c15) * sld + kb * KB + wave * 16 + 4 * g) = acc[kb][t];
    }
  __syncthreads();
}

// ---- matmul, MFMA: out[r][c] = sum_j strip[r][j] B[j][c], computed as out^T = B^T strip^T: B^T by transposed LDS reads (two of them
// fill the 8 reduction slots of a lane group: rows 4g..4g+3 and 16+4g..16+4g+3 of a 32-row step), strip^T converted to bf16 on the way
// to its registers.  The waves split the 16-channel blocks of an hd chunk.
__device__ __forceinline__ void matmul_mfma(const float* strip, int sld, int Lp, const bf16_t* __restrict__ B, int64_t ldb, int b_valid,
                                            int hd, int hc, char* stage, bf16_t* __restrict__ out, int64_t ldo, int out_valid) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c15 = lane & 15;
  const int rb = hc * 2, ncb = hc >> 4;
  for (int c = 0; c < hd; c += hc) {
    f32x4 o[4][2];
#pragma unroll
    for (int u = 0; u < 4; ++u) { o[u][0] = f32x4{0.f, 0.f, 0.f, 0.f}; o[u][1] = o[u][0]; }
    for (int kb = 0; kb < Lp; kb += KB) {
      __syncthreads();
      load_tile(B + (int64_t)kb * ldb + c, ldb, b_valid - kb, KB, hc, stage);
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < KB; kk += 32) {
        bf16x8 pf[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const float* sp = strip + (t * 16 + c15) * sld + kb + kk + 4 * g;
          const f32x4 lo = *(const f32x4*)sp, hi = *(const f32x4*)(sp + 16);
#pragma unroll
          for (int e = 0; e < 4; ++e) { pf[t][e] = (short)f2bf(lo[e]); pf[t][4 + e] = (short)f2bf(hi[e]); }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int cb = wave + 4 * u;
          if (cb < ncb) {
            const bf16x4 t0 = tr_frag(stage, kk, cb, lane, rb), t1 = tr_frag(stage, kk + 16, cb, lane, rb);
            const bf16x8 af = __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
            o[u][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, pf[0], o[u][0], 0, 0, 0);
            o[u][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, pf[1], o[u][1], 0, 0, 0);
          }
        }
      }
    }
    // D[channel 4g + r][tile row c15]
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int cb = wave + 4 * u;
      if (cb < ncb) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int r = t * 16 + c15;
          if (r < out_valid) store_o4(out + (int64_t)r * ldo + c + cb * 16 + 4 * g, o[u][t]);
        }
      }
    }
  }
}

// ---- dots, generic: a wave owns 8 tile rows, two at a time in registers (lanes stride the head dimension), 4 B rows per reduction
template <typename T>
__device__ __forceinline__ void dots_generic(const T* __restrict__ A, int64_t lda, int a_valid, const T* __restrict__ B, int64_t ldb,
                                             int b_valid, int hd, int Lp, float* strip, int sld) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int NQ = 16;                               // hd <= 64 * NQ = 1024
  for (int rr = 0; rr < QT / 4; rr += 2) {
    const int i0 = wave * (QT / 4) + rr;
    float qa[NQ], qb[NQ];
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
      const bool in = (lane + 64 * t) < hd;
      qa[t] = (in && i0 < a_valid) ? Elem<T>::ld(A + (int64_t)i0 * lda + lane + 64 * t) : 0.f;
      qb[t] = (in && i0 + 1 < a_valid) ? Elem<T>::ld(A + (int64_t)(i0 + 1) * lda + lane + 64 * t) : 0.f;
    }
    for (int j0 = 0; j0 < Lp; j0 += 4) {
      float a4[4] = {0.f, 0.f, 0.f, 0.f}, b4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u;
        if (j < b_valid) {
#pragma unroll
          for (int t = 0; t < NQ; ++t)
            if ((lane + 64 * t) < hd) {
              const float kv = Elem<T>::ld(B + (int64_t)j * ldb + lane + 64 * t);
              a4[u] += qa[t] * kv;
              b4[u] += qb[t] * kv;
            }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float sa = wave_sum(a4[u]), sb = wave_sum(b4[u]);
        if (lane == 0) { strip[i0 * sld + j0 + u] = sa; strip[(i0 + 1) * sld + j0 + u] = sb; }
      }
    }
  }
  __syncthreads();
}

// ---- matmul, generic: a thread owns one channel for 32 / rg tile rows (rg row groups share the 256 threads when hd < 256); the strip
// is read as broadcast float4, B rows coalesced
template <typename T>
__device__ __forceinline__ void matmul_generic(const float* strip, int sld, int Lp, const T* __restrict__ B, int64_t ldb, int b_valid,
                                               int hd, T* __restrict__ out, int64_t ldo, int out_valid) {
  const int nc = hd > 128 ? 256 : hd > 64 ? 128 : hd > 32 ? 64 : hd > 16 ? 32 : 16;
  const int rpg = QT / (256 / nc);                     // rows per thread: 32, 16, 8, 4, 2
  const int ci = threadIdx.x % nc, r0 = (threadIdx.x / nc) * rpg;
  for (int c = ci; c < hd; c += nc) {
    float acc[QT];
#pragma unroll
    for (int ii = 0; ii < QT; ++ii) acc[ii] = 0.f;
    for (int j = 0; j < Lp; j += 4) {
      float bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) bv[u] = (j + u) < b_valid ? Elem<T>::ld(B + (int64_t)(j + u) * ldb + c) : 0.f;
#pragma unroll
      for (int ii = 0; ii < QT; ++ii)
        if (ii < rpg) {
          const f32x4 s = *(const f32x4*)(strip + (r0 + ii) * sld + j);
          acc[ii] += s[0] * bv[0] + s[1] * bv[1] + s[2] * bv[2] + s[3] * bv[3];
        }
    }
#pragma unroll
    for (int ii = 0; ii < QT; ++ii)
      if (ii < rpg && r0 + ii < out_valid) Elem<T>::st(out + (int64_t)(r0 + ii) * ldo + c, acc[ii]);
  }
}

template <typename T, bool MFMA>
__device__ __forceinline__ void dots(const void* A, int64_t lda, int a_valid, const void* B, int64_t ldb, int b_valid, const LongArgs& a,
                                     float* strip, int sld, char* stage) {
  if constexpr (MFMA) dots_mfma((const bf16_t*)A, lda, a_valid, (const bf16_t*)B, ldb, b_valid, a.hd, a.hc, a.Lp, strip, sld, stage);
  else dots_generic<T>((const T*)A, lda, a_valid, (const T*)B, ldb, b_valid, a.hd, a.Lp, strip, sld);
}
template <typename T, bool MFMA>
__device__ __forceinline__ void matmul(const float* strip, int sld, const void* B, int64_t ldb, int b_valid, const LongArgs& a, char* stage,
                                       void* out, int64_t ldo, int out_valid) {
  if constexpr (MFMA) matmul_mfma(strip, sld, a.Lp, (const bf16_t*)B, ldb, b_valid, a.hd, a.hc, stage, (bf16_t*)out, ldo, out_valid);
  else matmul_generic<T>(strip, sld, a.Lp, (const T*)B, ldb, b_valid, a.hd, (T*)out, ldo, out_valid);
}

// blockIdx.x = (seq * H + h) * ntiles + tile
#define LONG_PROLOGUE()                                                                           \
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];                                 \
  const int L = a.L, H = a.H, hd = a.hd, sld = a.Lp + 4;                                          \
  float* strip = reinterpret_cast<float*>(smem_raw);                                              \
  char* stage = smem_raw + (size_t)QT * sld * sizeof(float);                                      \
  const int tile = blockIdx.x % a.ntiles, sh = blockIdx.x / a.ntiles, seq = sh / H, h = sh % H;   \
  const int t0 = tile * QT, tv = min(QT, L - t0);                                                 \
  const int64_t row0 = (int64_t)seq * L;                                                          \
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;                                     \
  const unsigned dkey = a.dkey ^ (a.salt ? *a.salt : 0u);                                         \
  (void)hd; (void)stage; (void)lane; (void)wave; (void)dkey; (void)tv

template <typename T, bool MFMA>
__global__ __launch_bounds__(256) void long_fwd_kernel(const LongArgs a) {
  LONG_PROLOGUE();
  const T* qt = (const T*)a.q + (row0 + t0) * a.ldq + (int64_t)h * hd;
  const T* kh = (const T*)a.k + row0 * a.ldk + (int64_t)h * hd;
  const T* vh = (const T*)a.v + row0 * a.ldv + (int64_t)h * hd;
  const float* addh = a.addm ? a.addm + seq * a.sb + h * a.sh : nullptr;
  dots<T, MFMA>(qt, a.ldq, tv, kh, a.ldk, L, a, strip, sld, stage);
  // masked softmax over the whole strip: a wave owns 8 rows, lanes stride the keys
  for (int r = wave * (QT / 4); r < (wave + 1) * (QT / 4); ++r) {
    float* sr = strip + r * sld;
    const int i = t0 + r;
    if (i >= L) {
      for (int j = lane; j < a.Lp; j += 64) sr[j] = 0.f;
      continue;
    }
    float m = -INFINITY;
    for (int j = lane; j < L; j += 64) {
      float sv = masked(a.mask, a.period, i, j) ? -INFINITY : sr[j] * a.scale;
      if (addh) sv += addh[i * a.si + j];      // models/transformerblock.py:27-28: attn = attn + attn_mask (any values, -inf included)
      sr[j] = sv;
      m = fmaxf(m, sv);
    }
    m = wave_max(m);
    float sum = 0.f;
    for (int j = lane; j < L; j += 64) {
      const float e = sr[j] == -INFINITY ? 0.f : expf(sr[j] - m);
      sr[j] = e;
      sum += e;
    }
    const float inv = 1.0f / wave_sum(sum);
    const int64_t pbase = (((int64_t)seq * H + h) * L + i) * L;
    float* pr = a.probs ? a.probs + pbase : nullptr;
    for (int j = lane; j < a.Lp; j += 64) {
      float p = 0.f;
      if (j < L) {
        p = sr[j] * inv;
        if (pr) pr[j] = p;  // pre-dropout probabilities (backward regenerates the mask)
        p = (a.dthresh && !drop_keep(dkey, (unsigned)pbase + j, a.dthresh)) ? 0.f : p * a.dinv;
      }
      sr[j] = p;
    }
  }
  __syncthreads();
  matmul<T, MFMA>(strip, sld, vh, a.ldv, L, a, stage, (T*)a.out + (row0 + t0) * a.ldo + (int64_t)h * hd, a.ldo, tv);
}

// dQ for one tile of query rows; leaves the row term sum_j P_ij dP_ij of its rows in row_term
template <typename T, bool MFMA>
__global__ __launch_bounds__(256) void long_bwd_q_kernel(const LongArgs a) {
  LONG_PROLOGUE();
  const T* dot_ = (const T*)a.dout + (row0 + t0) * a.lddo + (int64_t)h * hd;
  const T* kh = (const T*)a.k + row0 * a.ldk + (int64_t)h * hd;
  const T* vh = (const T*)a.v + row0 * a.ldv + (int64_t)h * hd;
  dots<T, MFMA>(dot_, a.lddo, tv, vh, a.ldv, L, a, strip, sld, stage);     // dP' (gradient of the dropped-out probabilities)
  for (int r = wave * (QT / 4); r < (wave + 1) * (QT / 4); ++r) {
    float* sr = strip + r * sld;
    const int i = t0 + r;
    if (i >= L) {
      for (int j = lane; j < a.Lp; j += 64) sr[j] = 0.f;
      continue;
    }
    const int64_t pbase = (((int64_t)seq * H + h) * L + i) * L;
    const float* pr = a.probs + pbase;
    float dsum = 0.f;
    for (int j = lane; j < L; j += 64) {
      const float m = (a.dthresh && !drop_keep(dkey, (unsigned)pbase + j, a.dthresh)) ? 0.f : a.dinv;
      const float dp = sr[j] * m;               // dP = dP' * m / (1 - p)
      sr[j] = dp;
      dsum += pr[j] * dp;
    }
    dsum = wave_sum(dsum);
    if (lane == 0) a.row_term[((int64_t)seq * H + h) * L + i] = dsum;
    for (int j = lane; j < a.Lp; j += 64) sr[j] = j < L ? pr[j] * (sr[j] - dsum) * a.scale : 0.f;
  }
  __syncthreads();
  matmul<T, MFMA>(strip, sld, kh, a.ldk, L, a, stage, (T*)a.dq + (row0 + t0) * a.lddq + (int64_t)h * hd, a.lddq, tv);
}

// dK and dV for one tile of key rows: the strip is [32 keys][Lp queries]
template <typename T, bool MFMA>
__global__ __launch_bounds__(256) void long_bwd_kv_kernel(const LongArgs a) {
  LONG_PROLOGUE();
  const T* doh = (const T*)a.dout + row0 * a.lddo + (int64_t)h * hd;
  const T* qh = (const T*)a.q + row0 * a.ldq + (int64_t)h * hd;
  const T* vt = (const T*)a.v + (row0 + t0) * a.ldv + (int64_t)h * hd;
  const int64_t pbase = ((int64_t)seq * H + h) * L * L;
  const float* pr = a.probs + pbase;
  const int jj = threadIdx.x & 31, j = t0 + jj;        // 32 consecutive keys per query row: 128-byte runs of probs
  // dV[j] = sum_i P'[i][j] dO[i]
  for (int i = threadIdx.x >> 5; i < a.Lp; i += 8) {
    float p = 0.f;
    if (i < L && j < L) {
      p = pr[(int64_t)i * L + j];
      if (a.dthresh) p = drop_keep(dkey, (unsigned)pbase + (unsigned)(i * L + j), a.dthresh) ? p * a.dinv : 0.f;
    }
    strip[jj * sld + i] = p;
  }
  __syncthreads();
  matmul<T, MFMA>(strip, sld, doh, a.lddo, L, a, stage, (T*)a.dv + (row0 + t0) * a.lddv + (int64_t)h * hd, a.lddv, tv);
  // dK[j] = sum_i dS[i][j] q[i]
  __syncthreads();                                                          // every wave is done reading P'^T
  dots<T, MFMA>(vt, a.ldv, tv, doh, a.lddo, L, a, strip, sld, stage);       // dP'^T
  const float* rt = a.row_term + ((int64_t)seq * H + h) * L;
  for (int i = threadIdx.x >> 5; i < a.Lp; i += 8) {
    float ds = 0.f;
    if (i < L && j < L) {
      const float m = (a.dthresh && !drop_keep(dkey, (unsigned)pbase + (unsigned)(i * L + j), a.dthresh)) ? 0.f : a.dinv;
      ds = pr[(int64_t)i * L + j] * (strip[jj * sld + i] * m - rt[i]) * a.scale;
    }
    strip[jj * sld + i] = ds;
  }
  __syncthreads();
  matmul<T, MFMA>(strip, sld, qh, a.ldq, L, a, stage, (T*)a.dk + (row0 + t0) * a.lddk + (int64_t)h * hd, a.lddk, tv);
}

// dS = P (dP - sum_j P dP) of one tile of query rows, WITHOUT the score scale: the gradient of an additive bias (it is added after the
// scaling).  The first half of long_bwd_q_kernel, for 1 <= L <= 512; every (seq, h, i, j) is written once, to the caller's strides.
template <typename T, bool MFMA>
__global__ __launch_bounds__(256) void bias_bwd_ds_kernel(const LongArgs a) {
  LONG_PROLOGUE();
  const T* dot_ = (const T*)a.dout + (row0 + t0) * a.lddo + (int64_t)h * hd;
  const T* vh = (const T*)a.v + row0 * a.ldv + (int64_t)h * hd;
  dots<T, MFMA>(dot_, a.lddo, tv, vh, a.ldv, L, a, strip, sld, stage);     // dP' (gradient of the dropped-out probabilities)
  for (int r = wave * (QT / 4); r < (wave + 1) * (QT / 4); ++r) {
    float* sr = strip + r * sld;
    const int i = t0 + r;
    if (i >= L) continue;
    const int64_t pbase = (((int64_t)seq * H + h) * L + i) * L;
    const float* pr = a.probs + pbase;
    float dsum = 0.f;
    for (int j = lane; j < L; j += 64) {
      const float m = (a.dthresh && !drop_keep(dkey, (unsigned)pbase + j, a.dthresh)) ? 0.f : a.dinv;
      const float dp = sr[j] * m;               // dP = dP' * m / (1 - p)
      sr[j] = dp;
      dsum += pr[j] * dp;
    }
    dsum = wave_sum(dsum);
    float* dst = a.dbias + seq * a.ob + h * a.oh + i * a.oi;
    for (int j = lane; j < L; j += 64) dst[j] = pr[j] * (sr[j] - dsum);
  }
}

// dbias = the sum of ds [nseq, H, L, L] over the broadcast dimensions (rb / rh / ri: batch / head / row is summed), one output row
// per blockIdx.x and 64 columns per blockIdx.y.  Wave w adds the terms w, w + 4, .. in that order and the four partial sums are
// combined in a fixed order: the same input gives the same bits.
__global__ __launch_bounds__(256) void bias_bwd_reduce_kernel(const float* __restrict__ ds, float* __restrict__ dbias, int nseq, int H,
                                                              int L, int rb, int rh, int ri, int64_t ob, int64_t oh, int64_t oi) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.y * 64 + lane;
  int row = blockIdx.x;
  const int io = ri ? 0 : row % L;
  row /= ri ? 1 : L;
  const int ho = rh ? 0 : row % H;
  const int bo = row / (rh ? 1 : H);
  const int nb = rb ? nseq : 1, nh = rh ? H : 1, ni = ri ? L : 1;
  float acc = 0.f;
  if (j < L)
    for (int t = wave; t < nb * nh * ni; t += 4) {
      const int i = t % ni, hh = (t / ni) % nh, b = t / (ni * nh);
      acc += ds[((((int64_t)(bo + b)) * H + ho + hh) * L + io + i) * L + j];
    }
  part[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && j < L) dbias[bo * ob + ho * oh + io * oi + j] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
bool al8(const void* p) { return (((uintptr_t)p) & 7) == 0; }
bool use_mfma_attention() {
  static int v = -1;
  if (v < 0) { const char* e = getenv("AFFT_ATTN_GENERIC"); v = (e && e[0] == '1') ? 0 : 1; }
  return v == 1;
}

template <typename KernT>
int launch_long(KernT kern, std::atomic<uint64_t>* attr_done, const LongArgs& a, int nseq, bool mfma, hipStream_t stream) {
  const size_t lds = (size_t)QT * (a.Lp + 4) * sizeof(float) + (mfma ? (size_t)(QT + KB) * a.hc * 2 : 0);
  // the attribute is set once per (kernel, device): ask for the most any shape needs (L = 512, hd chunks of 256: 112.5 KiB)
  constexpr size_t lds_max = (size_t)QT * (LHI + 4) * sizeof(float) + (size_t)(QT + KB) * 256 * 2;
  if (int rc = afft_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds_max, attr_done)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)nseq * a.H * a.ntiles)), dim3(256), lds, stream, a);
  return 0;
}
#define LONG_LAUNCH(KERN)                                                      \
  do {                                                                         \
    static std::atomic<uint64_t> attr_done{0};                                 \
    if (int rc_ = launch_long(KERN, &attr_done, a, nseq, mfma, stream)) return rc_; \
  } while (0)

void fill_common(LongArgs& a, int L, int H, int hd, float scale, float drop_p, unsigned drop_key) {
  a.L = L; a.Lp = (L + KB - 1) / KB * KB; a.H = H; a.hd = hd; a.ntiles = (L + QT - 1) / QT;
  a.hc = hd % 256 == 0 ? 256 : hd % 128 == 0 ? 128 : 64;
  a.scale = scale;
  afft_dropout_t dd = {drop_p, drop_key, 0.f, 0u, 1};
  const DropParams dp = make_drop(&dd);
  a.dthresh = dp.thresh; a.dkey = dp.key; a.dinv = dp.inv_keep; a.salt = dp.salt;
}

}  // namespace

static int attention_long_fwd_impl(const char* who, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                   int32_t dtype, int32_t nseq, int32_t L, int32_t H, int32_t hd, float scale, int32_t mask,
                                   int32_t mask_period, const float* bias, int64_t sb, int64_t sh, int64_t si, float drop_p,
                                   uint32_t drop_key, void* out, int64_t ldo, float* probs, hipStream_t stream) {
  AFFT_CHECK(q && k && v && out, "%s: null pointer", who);
  AFFT_CHECK(L >= LLO && L <= LHI, "%s: sequence length %d outside %d..%d", who, L, LLO, LHI);
  AFFT_CHECK(mask >= AFFT_MASK_NONE && mask <= AFFT_MASK_BLOCKCAUSAL, "%s: bad mask %d", who, mask);
  AFFT_CHECK(mask != AFFT_MASK_BLOCKCAUSAL || (mask_period >= 1 && L % mask_period == 0),
             "%s: block-causal mask needs a period that divides L (L=%d, period=%d)", who, L, mask_period);
  AFFT_CHECK(drop_p >= 0.f && drop_p < 1.f, "%s: dropout p outside [0,1)", who);
  AFFT_CHECK(hd >= 1 && hd <= 1024, "%s: head dimension %d outside 1..1024", who, hd);
  AFFT_CHECK(dtype == AFFT_F32 || dtype == AFFT_BF16, "%s: bad dtype %d", who, dtype);
  AFFT_CHECK(nseq >= 0 && H >= 1, "%s: bad nseq %d / H %d", who, nseq, H);
  if (nseq == 0) return 0;
  const int64_t es_ = dtype == AFFT_F32 ? 4 : 2, rw_ = (int64_t)nseq * L * H * hd, pb_ = probs ? (int64_t)nseq * H * L * L * 4 : 0;
  AfftKernelScope ktrace(AFFT_K_ATTN_FWD, nseq * L, H * hd, 4 * es_ * rw_ + pb_, 4 * (int64_t)nseq * H * L * L * hd, stream);
  LongArgs a = {};
  a.q = q; a.k = k; a.v = v; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv;
  a.out = out; a.ldo = ldo; a.probs = probs; a.addm = bias; a.sb = sb; a.sh = sh; a.si = si;
  a.mask = mask; a.period = mask == AFFT_MASK_BLOCKCAUSAL ? mask_period : 1;
  fill_common(a, L, H, hd, scale, drop_p, drop_key);
  const bool mfma = dtype == AFFT_BF16 && use_mfma_attention() && hd % 64 == 0 && ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 &&
                    al16(q) && al16(k) && al16(v) && ldo % 4 == 0 && al8(out);
  if (dtype == AFFT_F32) LONG_LAUNCH((long_fwd_kernel<float, false>));
  else if (mfma) LONG_LAUNCH((long_fwd_kernel<bf16_t, true>));
  else LONG_LAUNCH((long_fwd_kernel<bf16_t, false>));
  AFFT_LAUNCH_CHECK();
  return 0;
}

extern "C" int afft_attention_long_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                       int32_t dtype, int32_t nseq, int32_t L, int32_t H, int32_t hd, float scale, int32_t mask,
                                       int32_t mask_period, const float* mask_table, float drop_p, uint32_t drop_key, void* out,
                                       int64_t ldo, float* probs, void* stream_) {
  return attention_long_fwd_impl("attention_long_fwd", q, ldq, k, ldk, v, ldv, dtype, nseq, L, H, hd, scale, mask, mask_period,
                                 mask_table, 0, 0, L, drop_p, drop_key, out, ldo, probs, (hipStream_t)stream_);
}

extern "C" int afft_attention_long_fwd_bias(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                            int32_t dtype, int32_t nseq, int32_t L, int32_t H, int32_t hd, float scale,
                                            const float* bias, int64_t sb, int64_t sh, int64_t si, float drop_p, uint32_t drop_key,
                                            void* out, int64_t ldo, float* probs, void* stream_) {
  AFFT_CHECK(bias, "attention_long_fwd_bias: null pointer");
  AFFT_CHECK(sb >= 0 && sh >= 0 && si >= 0, "attention_long_fwd_bias: negative bias stride (sb=%lld, sh=%lld, si=%lld)", (long long)sb,
             (long long)sh, (long long)si);
  AFFT_CHECK((((uintptr_t)bias) & 3) == 0, "attention_long_fwd_bias: bias pointer %p is not 4-byte aligned", (const void*)bias);
  return attention_long_fwd_impl("attention_long_fwd_bias", q, ldq, k, ldk, v, ldv, dtype, nseq, L, H, hd, scale, AFFT_MASK_NONE, 0, bias,
                                 sb, sh, si, drop_p, drop_key, out, ldo, probs, (hipStream_t)stream_);
}

extern "C" int afft_attention_long_bwd(const void* dout, int64_t lddo, const void* q, int64_t ldq, const void* k, int64_t ldk,
                                       const void* v, int64_t ldv, int32_t dtype, const float* probs, int32_t nseq, int32_t L,
                                       int32_t H, int32_t hd, float scale, float drop_p, uint32_t drop_key, void* dq,
                                       int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, float* row_term, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AFFT_CHECK(dout && q && k && v && probs && dq && dk && dv && row_term, "attention_long_bwd: null pointer");
  AFFT_CHECK(L >= LLO && L <= LHI, "attention_long_bwd: sequence length %d outside %d..%d", L, LLO, LHI);
  AFFT_CHECK(drop_p >= 0.f && drop_p < 1.f, "attention_long_bwd: dropout p outside [0,1)");
  AFFT_CHECK(hd >= 1 && hd <= 1024, "attention_long_bwd: head dimension %d outside 1..1024", hd);
  AFFT_CHECK(dtype == AFFT_F32 || dtype == AFFT_BF16, "attention_long_bwd: bad dtype %d", dtype);
  AFFT_CHECK(nseq >= 0 && H >= 1, "attention_long_bwd: bad nseq %d / H %d", nseq, H);
  if (nseq == 0) return 0;
  // bytes: the algorithmic ones of attention_bwd; flops: the four products (dP is formed twice here, once per pass: 10 L^2 hd are executed)
  const int64_t es_ = dtype == AFFT_F32 ? 4 : 2, rw_ = (int64_t)nseq * L * H * hd, pb_ = (int64_t)nseq * H * L * L * 4;
  AfftKernelScope ktrace(AFFT_K_ATTN_BWD, nseq * L, H * hd, 7 * es_ * rw_ + pb_, 8 * (int64_t)nseq * H * L * L * hd, stream);
  LongArgs a = {};
  a.dout = dout; a.q = q; a.k = k; a.v = v; a.lddo = lddo; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv;
  a.dq = dq; a.dk = dk; a.dv = dv; a.lddq = lddq; a.lddk = lddk; a.lddv = lddv;
  a.probs = const_cast<float*>(probs); a.row_term = row_term;
  a.mask = AFFT_MASK_NONE; a.period = 1;
  fill_common(a, L, H, hd, scale, drop_p, drop_key);
  const bool mfma = dtype == AFFT_BF16 && use_mfma_attention() && hd % 64 == 0 && lddo % 8 == 0 && ldq % 8 == 0 && ldk % 8 == 0 &&
                    ldv % 8 == 0 && al16(dout) && al16(q) && al16(k) && al16(v) && lddq % 4 == 0 && lddk % 4 == 0 && lddv % 4 == 0 &&
                    al8(dq) && al8(dk) && al8(dv);
  if (dtype == AFFT_F32) { LONG_LAUNCH((long_bwd_q_kernel<float, false>)); LONG_LAUNCH((long_bwd_kv_kernel<float, false>)); }
  else if (mfma) { LONG_LAUNCH((long_bwd_q_kernel<bf16_t, true>)); LONG_LAUNCH((long_bwd_kv_kernel<bf16_t, true>)); }
  else { LONG_LAUNCH((long_bwd_q_kernel<bf16_t, false>)); LONG_LAUNCH((long_bwd_kv_kernel<bf16_t, false>)); }
  AFFT_LAUNCH_CHECK();
  return 0;
}

extern "C" int afft_attention_bias_bwd(const void* dout, int64_t lddo, const void* v, int64_t ldv, int32_t dtype, const float* probs,
                                       int32_t nseq, int32_t L, int32_t H, int32_t hd, float drop_p, uint32_t drop_key, float* dbias,
                                       int64_t sb, int64_t sh, int64_t si, float* scratch, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AFFT_CHECK(dout && v && probs && dbias, "attention_bias_bwd: null pointer");
  AFFT_CHECK(L >= 1 && L <= LHI, "attention_bias_bwd: sequence length %d outside 1..%d", L, LHI);
  AFFT_CHECK(drop_p >= 0.f && drop_p < 1.f, "attention_bias_bwd: dropout p outside [0,1)");
  AFFT_CHECK(hd >= 1 && hd <= 1024, "attention_bias_bwd: head dimension %d outside 1..1024", hd);
  AFFT_CHECK(dtype == AFFT_F32 || dtype == AFFT_BF16, "attention_bias_bwd: bad dtype %d", dtype);
  AFFT_CHECK(nseq >= 0 && H >= 1, "attention_bias_bwd: bad nseq %d / H %d", nseq, H);
  AFFT_CHECK(sb >= 0 && sh >= 0 && si >= 0, "attention_bias_bwd: negative bias stride (sb=%lld, sh=%lld, si=%lld)", (long long)sb,
             (long long)sh, (long long)si);
  AFFT_CHECK((((uintptr_t)dbias) & 3) == 0, "attention_bias_bwd: dbias pointer %p is not 4-byte aligned", (void*)dbias);
  const bool reduce = sb == 0 || sh == 0 || si == 0;
  AFFT_CHECK(!reduce || (scratch && (((uintptr_t)scratch) & 3) == 0),
             "attention_bias_bwd: a broadcast bias needs 4-byte aligned scratch of nseq*H*L*L floats (scratch=%p)", (void*)scratch);
  if (nseq == 0) return 0;
  const int64_t es_ = dtype == AFFT_F32 ? 4 : 2, rw_ = (int64_t)nseq * L * H * hd, pb_ = (int64_t)nseq * H * L * L * 4;
  AfftKernelScope ktrace(AFFT_K_ATTN_BWD, nseq * L, H * hd, 2 * es_ * rw_ + (reduce ? 3 : 2) * pb_, 2 * (int64_t)nseq * H * L * L * hd, stream);
  LongArgs a = {};
  a.dout = dout; a.v = v; a.lddo = lddo; a.ldv = ldv;
  a.probs = const_cast<float*>(probs);
  a.mask = AFFT_MASK_NONE; a.period = 1;
  if (reduce) { a.dbias = scratch; a.ob = (int64_t)H * L * L; a.oh = (int64_t)L * L; a.oi = L; }
  else { a.dbias = dbias; a.ob = sb; a.oh = sh; a.oi = si; }
  fill_common(a, L, H, hd, 1.0f, drop_p, drop_key);
  const bool mfma = dtype == AFFT_BF16 && use_mfma_attention() && hd % 64 == 0 && lddo % 8 == 0 && ldv % 8 == 0 && al16(dout) && al16(v);
  if (dtype == AFFT_F32) LONG_LAUNCH((bias_bwd_ds_kernel<float, false>));
  else if (mfma) LONG_LAUNCH((bias_bwd_ds_kernel<bf16_t, true>));
  else LONG_LAUNCH((bias_bwd_ds_kernel<bf16_t, false>));
  if (reduce) {
    const int64_t rows = (int64_t)(sb ? nseq : 1) * (sh ? H : 1) * (si ? L : 1);
    hipLaunchKernelGGL(bias_bwd_reduce_kernel, dim3((unsigned)rows, (unsigned)((L + 63) / 64)), dim3(256), 0, stream, scratch, dbias,
                       nseq, H, L, (int)(sb == 0), (int)(sh == 0), (int)(si == 0), sb, sh, si);
  }
  AFFT_LAUNCH_CHECK();
  return 0;
}
