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
// swizzle of attention_tiles.h (row fragments by ds_read_b128, transposed fragments by ds_read_b64_tr_b16); any other bf16 shape, or
// AFFT_ATTN_GENERIC=1, takes the generic form with bf16 loads (attn_plan.h decides; it also holds QT, KB and the length band).
// Semantics are those of attention.hip: probs = PRE-dropout probabilities, masked entries exactly 0, dropout mask from (key, index).
// The additive bias of the forward pass is read through element strides (0 = broadcast over batch / head / row: afft_attention_long_fwd_bias);
// its gradient, for every L from 1 to 512, is the first half of the dQ pass without the score scale plus an ordered sum over the
// broadcast dimensions (afft_attention_bias_bwd: bias_bwd_ds_kernel, bias_bwd_reduce_kernel).
#include "attention_tiles.h"
#include "attn_plan.h"

using namespace afft_attn_detail;

namespace {

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
    load_tile(A + c, lda, 0, a_valid, QT, hc, As);
#pragma unroll
    for (int kb = 0; kb < LHI / KB; ++kb) {
      if (kb * KB < Lp) {
        if (kb) __syncthreads();           // the previous block has been consumed by every wave
        load_tile(B + (int64_t)kb * KB * ldb + c, ldb, 0, b_valid - kb * KB, KB, hc, Bs);
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
      load_tile(B + (int64_t)kb * ldb + c, ldb, 0, b_valid - kb, KB, hc, stage);
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

// one kernel of a long plan: the attribute is set once per (kernel, device): ask for the most any shape needs (L = 512, hd chunks of 256: 112.5 KiB)
template <typename KernT>
int launch_long(KernT kern, std::atomic<uint64_t>* attr_done, const LongArgs& a, const AttnPlan& p, hipStream_t stream) {
  constexpr size_t lds_max = (size_t)QT * (LHI + 4) * sizeof(float) + (size_t)(QT + KB) * 256 * 2;
  if (int rc = afft_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds_max, attr_done)) return rc;
  hipLaunchKernelGGL(kern, dim3(p.grid), dim3(256), p.lds, stream, a);
  return 0;
}
#define LONG_LAUNCH(KERN)                                                       \
  do {                                                                          \
    static std::atomic<uint64_t> attr_done{0};                                  \
    if (int rc_ = launch_long(KERN, &attr_done, a, p, stream)) return rc_;      \
  } while (0)

}  // namespace

int launch_attention_long(const AttnCall& c, const AttnPlan& p, hipStream_t stream) {
  const bool reduce = c.dir == kBiasBwd && bias_grad_reduces(c);
  LongArgs a = {};
  a.q = c.q; a.k = c.k; a.v = c.v; a.dout = c.dout; a.ldq = c.ldq; a.ldk = c.ldk; a.ldv = c.ldv; a.lddo = c.lddo;
  a.out = c.out; a.dq = c.dq; a.dk = c.dk; a.dv = c.dv; a.ldo = c.ldo; a.lddq = c.lddq; a.lddk = c.lddk; a.lddv = c.lddv;
  a.probs = c.probs; a.addm = c.bias; a.sb = c.sb; a.sh = c.sh; a.si = c.si; a.row_term = c.row_term;
  if (reduce) { a.dbias = c.scratch; a.ob = (int64_t)c.H * c.L * c.L; a.oh = (int64_t)c.L * c.L; a.oi = c.L; }      // every (seq, h, i, j) first
  else { a.dbias = c.dbias; a.ob = c.dsb; a.oh = c.dsh; a.oi = c.dsi; }
  a.L = c.L; a.Lp = p.Lp; a.H = c.H; a.hd = c.hd; a.hc = p.hc; a.ntiles = p.ntiles;
  a.scale = c.scale;
  a.mask = c.mask; a.period = c.mask == AFFT_MASK_BLOCKCAUSAL ? c.period : 1;
  afft_dropout_t dd = {c.drop_p, c.drop_key, 0.f, 0u, 1};
  const DropParams dp = make_drop(&dd);
  a.dthresh = dp.thresh; a.dkey = dp.key; a.dinv = dp.inv_keep; a.salt = dp.salt;
  switch (p.family) {
    case kLongF32:
      if (c.dir == kFwd) LONG_LAUNCH((long_fwd_kernel<float, false>));
      else { LONG_LAUNCH((long_bwd_q_kernel<float, false>)); LONG_LAUNCH((long_bwd_kv_kernel<float, false>)); }
      break;
    case kLongBf16:
      if (c.dir == kFwd) LONG_LAUNCH((long_fwd_kernel<bf16_t, false>));
      else { LONG_LAUNCH((long_bwd_q_kernel<bf16_t, false>)); LONG_LAUNCH((long_bwd_kv_kernel<bf16_t, false>)); }
      break;
    case kLongMfma:
      if (c.dir == kFwd) LONG_LAUNCH((long_fwd_kernel<bf16_t, true>));
      else { LONG_LAUNCH((long_bwd_q_kernel<bf16_t, true>)); LONG_LAUNCH((long_bwd_kv_kernel<bf16_t, true>)); }
      break;
    case kBiasF32: LONG_LAUNCH((bias_bwd_ds_kernel<float, false>)); break;
    case kBiasBf16: LONG_LAUNCH((bias_bwd_ds_kernel<bf16_t, false>)); break;
    default: LONG_LAUNCH((bias_bwd_ds_kernel<bf16_t, true>)); break;
  }
  if (reduce) {
    const int64_t rows = (int64_t)(c.dsb ? c.nseq : 1) * (c.dsh ? c.H : 1) * (c.dsi ? c.L : 1);
    hipLaunchKernelGGL(bias_bwd_reduce_kernel, dim3((unsigned)rows, (unsigned)((c.L + 63) / 64)), dim3(256), 0, stream, c.scratch, c.dbias,
                       c.nseq, c.H, c.L, (int)(c.dsb == 0), (int)(c.dsh == 0), (int)(c.dsi == 0), c.dsb, c.dsh, c.dsi);
  }
  AFFT_LAUNCH_CHECK();
  return 0;
}

constexpr unsigned kLongChecks = kChkPtrs | kLenLong | kChkMask | kChkDrop | kChkHd | kChkDtype | kChkBatch;

extern "C" int afft_attention_long_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                       int32_t dtype, int32_t nseq, int32_t L, int32_t H, int32_t hd, float scale, int32_t mask,
                                       int32_t mask_period, const float* mask_table, float drop_p, uint32_t drop_key, void* out,
                                       int64_t ldo, float* probs, void* stream_) {
  AttnCall c = attn_fwd_call(q, ldq, k, ldk, v, ldv, dtype, nseq, L, H, hd, scale, drop_p, drop_key, out, ldo, probs);
  c.mask = mask; c.period = mask_period;
  c.bias = mask_table; c.si = L;
  return run_attention("attention_long_fwd", c, kLongChecks, 0, (hipStream_t)stream_);
}

extern "C" int afft_attention_long_fwd_bias(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                            int32_t dtype, int32_t nseq, int32_t L, int32_t H, int32_t hd, float scale,
                                            const float* bias, int64_t sb, int64_t sh, int64_t si, float drop_p, uint32_t drop_key,
                                            void* out, int64_t ldo, float* probs, void* stream_) {
  AttnCall c = attn_fwd_call(q, ldq, k, ldk, v, ldv, dtype, nseq, L, H, hd, scale, drop_p, drop_key, out, ldo, probs);
  c.bias = bias; c.sb = sb; c.sh = sh; c.si = si;
  if (int rc = check_attention("attention_long_fwd_bias", c, kChkBias | kChkBiasArgs)) return rc;
  return run_attention("attention_long_fwd_bias", c, kLongChecks, 0, (hipStream_t)stream_);
}

extern "C" int afft_attention_long_bwd(const void* dout, int64_t lddo, const void* q, int64_t ldq, const void* k, int64_t ldk,
                                       const void* v, int64_t ldv, int32_t dtype, const float* probs, int32_t nseq, int32_t L,
                                       int32_t H, int32_t hd, float scale, float drop_p, uint32_t drop_key, void* dq,
                                       int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, float* row_term, void* stream_) {
  AttnCall c = attn_bwd_call(dout, lddo, q, ldq, k, ldk, v, ldv, dtype, probs, nseq, L, H, hd, scale, drop_p, drop_key, dq, lddq, dk, lddk, dv, lddv);
  c.row_term = row_term;
  return run_attention("attention_long_bwd", c, (kLongChecks & ~kChkMask) | kChkRowTerm, 0, (hipStream_t)stream_);
}

extern "C" int afft_attention_bias_bwd(const void* dout, int64_t lddo, const void* v, int64_t ldv, int32_t dtype, const float* probs,
                                       int32_t nseq, int32_t L, int32_t H, int32_t hd, float drop_p, uint32_t drop_key, float* dbias,
                                       int64_t sb, int64_t sh, int64_t si, float* scratch, void* stream_) {
  AttnCall c = {};
  c.dir = kBiasBwd; c.dtype = dtype;
  c.dout = dout; c.lddo = lddo; c.v = v; c.ldv = ldv; c.probs = const_cast<float*>(probs);
  c.nseq = nseq; c.L = L; c.H = H; c.hd = hd; c.scale = 1.0f; c.drop_p = drop_p; c.drop_key = drop_key;      // the bias is added after the score scale
  c.dbias = dbias; c.dsb = sb; c.dsh = sh; c.dsi = si; c.scratch = scratch;
  return run_attention("attention_bias_bwd", c, kChkPtrs | kLenAll | kChkDrop | kChkHd | kChkDtype | kChkBatch | kChkBiasArgs | kChkScratch, 0,
                       (hipStream_t)stream_);
}
