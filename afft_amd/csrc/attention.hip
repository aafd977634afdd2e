// Small-sequence attention, forward and backward, generic over storage type (fp32 parity mode / bf16).
// One workgroup per (sequence, head); L <= 128 tokens (the T-SA-Fuser attends over M*T tokens: models/fusion.py:121-215),
// so the whole score matrix lives in LDS (template LM = 32 / 64 / 128 rows) and the mask is applied in-register while
// the scores are produced.  HBM-bound by construction (reads q,k,v once
// through L1/L2, writes out once): attention is < 0.2 % of the path's FLOPs.
//   softmax(q k^T * hd^-0.5 + mask) v : models/transformerblock.py:24-33,64-73 ; HF GPT-2 eager attention.
// The mask rule is attention_tiles.h's; which kernel runs a call is attn_plan.h's decision.  The ten entry points' shared body
// (run_attention) and the short ones are at the end of this file.
#include "attention_tiles.h"
#include "attn_plan.h"

using namespace afft_attn_detail;

namespace {

template <typename T, int LM>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const T* __restrict__ q, int64_t ldq, const T* __restrict__ k,
                                                       int64_t ldk, const T* __restrict__ v, int64_t ldv, int L, int H,
                                                       int hd, float scale, int mask, int period, unsigned dthresh,
                                                       unsigned dkey, float dinv, const unsigned* __restrict__ salt,
                                                       T* __restrict__ out, int64_t ldo, float* __restrict__ probs,
                                                       const float* __restrict__ addm, int64_t sb, int64_t sh,
                                                       int64_t si) {      // addm: additive fp32 bias or null; element (seq, h, i, j) at addm[seq*sb + h*sh + i*si + j] (a stride of 0 broadcasts; the [L][L] table is sb = sh = 0, si = L)
  if (salt) dkey ^= *salt;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float (*sc)[LM + 1] = reinterpret_cast<float (*)[LM + 1]>(smem_raw);
  const int seq = blockIdx.x / H, h = blockIdx.x % H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)seq * L;
  const T* qh = q + row0 * ldq + (int64_t)h * hd;
  const T* kh = k + row0 * ldk + (int64_t)h * hd;
  const T* vh = v + row0 * ldv + (int64_t)h * hd;
  const float* addh = addm ? addm + seq * sb + h * sh : nullptr;
  // scores: a wave owns query rows i = wave, wave + 4, ...: the row is read once into registers (lanes stride the head
  // dimension) and dotted with 4 key rows at a time, so 4 x hd/64 independent loads are in flight per reduction
  // (one (i, j) pair per iteration was a chain of dependent L2 round trips: 1.8 ms per launch at L = 64, hd = 512)
  constexpr int NQ = 16;                               // hd <= 64 * NQ = 1024
  for (int i = wave; i < L; i += 4) {
    float qv[NQ];
#pragma unroll
    for (int t = 0; t < NQ; ++t) qv[t] = (lane + 64 * t) < hd ? Elem<T>::ld(qh + i * ldq + lane + 64 * t) : 0.f;
    for (int j0 = 0; j0 < L; j0 += 4) {
      float acc4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u;
        if (j < L && !masked(mask, period, i, j)) {
#pragma unroll
          for (int t = 0; t < NQ; ++t)
            if ((lane + 64 * t) < hd) acc4[u] += qv[t] * Elem<T>::ld(kh + j * ldk + lane + 64 * t);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u;
        if (j < L) {
          float sv = masked(mask, period, i, j) ? -INFINITY : wave_sum(acc4[u]) * scale;
          if (addh) sv += addh[i * si + j];      // models/transformerblock.py:27-28: attn = attn + attn_mask (any values, -inf included)
          if (lane == 0) sc[i][j] = sv;
        }
      }
    }
  }
  __syncthreads();
  if (tid < L) {
    const int i = tid;
    float m = -INFINITY;
    for (int j = 0; j < L; ++j) m = fmaxf(m, sc[i][j]);
    float sum = 0.f;
    for (int j = 0; j < L; ++j) {
      const float e = sc[i][j] == -INFINITY ? 0.f : expf(sc[i][j] - m);
      sc[i][j] = e;
      sum += e;
    }
    const float inv = 1.0f / sum;
    float* pr = probs ? probs + (((int64_t)seq * H + h) * L + i) * L : nullptr;
    const unsigned base = (unsigned)((((int64_t)seq * H + h) * L + i) * L);
    for (int j = 0; j < L; ++j) {
      const float p = sc[i][j] * inv;
      if (pr) pr[j] = p;  // pre-dropout probabilities (backward regenerates the mask)
      sc[i][j] = (dthresh && !drop_keep(dkey, base + j, dthresh)) ? 0.f : p * dinv;
    }
  }
  __syncthreads();
  for (int c = tid; c < hd; c += 256) {
    float vc[LM];
#pragma unroll
    for (int j = 0; j < LM; ++j) vc[j] = j < L ? Elem<T>::ld(vh + j * ldv + c) : 0.f;
    for (int i = 0; i < L; ++i) {
      float o = 0.f;
#pragma unroll
      for (int j = 0; j < LM; ++j) o += (j < L ? sc[i][j] : 0.f) * vc[j];
      Elem<T>::st(out + (row0 + i) * ldo + (int64_t)h * hd + c, o);
    }
  }
}

template <typename T, int LM>
__global__ __launch_bounds__(256) void attn_bwd_kernel(const T* __restrict__ dout, int64_t lddo, const T* __restrict__ q,
                                                       int64_t ldq, const T* __restrict__ k, int64_t ldk,
                                                       const T* __restrict__ v, int64_t ldv,
                                                       const float* __restrict__ probs, int L, int H, int hd, float scale,
                                                       unsigned dthresh, unsigned dkey, float dinv,
                                                       const unsigned* __restrict__ salt,
                                                       T* __restrict__ dq, int64_t lddq, T* __restrict__ dk, int64_t lddk,
                                                       T* __restrict__ dv, int64_t lddv) {
  if (salt) dkey ^= *salt;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float (*pp)[LM + 1] = reinterpret_cast<float (*)[LM + 1]>(smem_raw);                  // probabilities (pre-dropout), later the dropped-out P' used by dV
  float (*ds)[LM + 1] = reinterpret_cast<float (*)[LM + 1]>(smem_raw) + LM;             // dP, then dS*scale
  const int seq = blockIdx.x / H, h = blockIdx.x % H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)seq * L;
  const T* doh = dout + row0 * lddo + (int64_t)h * hd;
  const T* qh = q + row0 * ldq + (int64_t)h * hd;
  const T* kh = k + row0 * ldk + (int64_t)h * hd;
  const T* vh = v + row0 * ldv + (int64_t)h * hd;
  const float* pr = probs + ((int64_t)seq * H + h) * L * L;
  for (int idx = tid; idx < L * L; idx += 256) pp[idx / L][idx % L] = pr[idx];
  // dP[i][j] = sum_c dO[i][c] v[j][c]: same row-in-registers, 4-keys-at-a-time scheme as the forward scores
  constexpr int NQ = 16;
  for (int i = wave; i < L; i += 4) {
    float dv_[NQ];
#pragma unroll
    for (int t = 0; t < NQ; ++t) dv_[t] = (lane + 64 * t) < hd ? Elem<T>::ld(doh + i * lddo + lane + 64 * t) : 0.f;
    for (int j0 = 0; j0 < L; j0 += 4) {
      float acc4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u;
        if (j < L) {
#pragma unroll
          for (int t = 0; t < NQ; ++t)
            if ((lane + 64 * t) < hd) acc4[u] += dv_[t] * Elem<T>::ld(vh + j * ldv + lane + 64 * t);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u;
        if (j < L) {
          const float sv = wave_sum(acc4[u]);
          if (lane == 0) ds[i][j] = sv;
        }
      }
    }
  }
  __syncthreads();
  if (tid < L) {
    const int i = tid;
    const unsigned base = (unsigned)((((int64_t)seq * H + h) * L + i) * L);
    float dot = 0.f;
    for (int j = 0; j < L; ++j) {
      // ds holds dP' (gradient of the dropped-out probabilities); dP = dP' * m/(1-p)
      const float m = (dthresh && !drop_keep(dkey, base + j, dthresh)) ? 0.f : dinv;
      ds[i][j] *= m;
      dot += pp[i][j] * ds[i][j];
    }
    for (int j = 0; j < L; ++j) {
      const float m = (dthresh && !drop_keep(dkey, base + j, dthresh)) ? 0.f : dinv;
      ds[i][j] = pp[i][j] * (ds[i][j] - dot) * scale;
      pp[i][j] *= m;  // P' for dV
    }
  }
  __syncthreads();
  for (int c = tid; c < hd; c += 256) {
    float a[LM];
    // dV[j][c] = sum_i P[i][j] dO[i][c]
#pragma unroll
    for (int i = 0; i < LM; ++i) a[i] = i < L ? Elem<T>::ld(doh + i * lddo + c) : 0.f;
    for (int j = 0; j < L; ++j) {
      float o = 0.f;
#pragma unroll
      for (int i = 0; i < LM; ++i) o += (i < L ? pp[i][j] : 0.f) * a[i];
      Elem<T>::st(dv + (row0 + j) * lddv + (int64_t)h * hd + c, o);
    }
    // dQ[i][c] = sum_j dS[i][j] k[j][c]
#pragma unroll
    for (int j = 0; j < LM; ++j) a[j] = j < L ? Elem<T>::ld(kh + j * ldk + c) : 0.f;
    for (int i = 0; i < L; ++i) {
      float o = 0.f;
#pragma unroll
      for (int j = 0; j < LM; ++j) o += (j < L ? ds[i][j] : 0.f) * a[j];
      Elem<T>::st(dq + (row0 + i) * lddq + (int64_t)h * hd + c, o);
    }
    // dK[j][c] = sum_i dS[i][j] q[i][c]
#pragma unroll
    for (int i = 0; i < LM; ++i) a[i] = i < L ? Elem<T>::ld(qh + i * ldq + c) : 0.f;
    for (int j = 0; j < L; ++j) {
      float o = 0.f;
#pragma unroll
      for (int i = 0; i < LM; ++i) o += (i < L ? ds[i][j] : 0.f) * a[i];
      Elem<T>::st(dk + (row0 + j) * lddk + (int64_t)h * hd + c, o);
    }
  }
}


// one instantiation pair: forward or backward by the call's direction, LDS bytes and grid from the plan
template <typename T, int LM>
int launch_short(const AttnCall& c, const AttnPlan& p, hipStream_t stream) {
  afft_dropout_t dd = {c.drop_p, c.drop_key, 0.f, 0u, 1};
  const DropParams dp = make_drop(&dd);
  const dim3 grid(p.grid);
  static std::atomic<uint64_t> fwd_attr{0}, bwd_attr{0};
  if (c.dir == kFwd) {
    auto kern = attn_fwd_kernel<T, LM>;
    if (p.lds > 48 * 1024)
      if (int rc = afft_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), p.lds, &fwd_attr)) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(256), p.lds, stream, (const T*)c.q, c.ldq, (const T*)c.k, c.ldk, (const T*)c.v, c.ldv, c.L, c.H, c.hd,
                       c.scale, c.mask, c.period, dp.thresh, dp.key, dp.inv_keep, dp.salt, (T*)c.out, c.ldo, c.probs, c.bias, c.sb, c.sh, c.si);
  } else {
    auto kern = attn_bwd_kernel<T, LM>;
    if (p.lds > 48 * 1024)
      if (int rc = afft_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), p.lds, &bwd_attr)) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(256), p.lds, stream, (const T*)c.dout, c.lddo, (const T*)c.q, c.ldq, (const T*)c.k, c.ldk, (const T*)c.v,
                       c.ldv, c.probs, c.L, c.H, c.hd, c.scale, dp.thresh, dp.key, dp.inv_keep, dp.salt, (T*)c.dq, c.lddq, (T*)c.dk, c.lddk,
                       (T*)c.dv, c.lddv);
  }
  return 0;
}
template <typename T>
int launch_short_lm(const AttnCall& c, const AttnPlan& p, hipStream_t stream) {
  return p.p0 == 32 ? launch_short<T, 32>(c, p, stream) : p.p0 == 64 ? launch_short<T, 64>(c, p, stream) : launch_short<T, 128>(c, p, stream);
}

}  // namespace

int launch_attention_generic(const AttnCall& c, const AttnPlan& p, hipStream_t stream) {
  if (int rc = c.dtype == AFFT_F32 ? launch_short_lm<float>(c, p, stream) : launch_short_lm<bf16_t>(c, p, stream)) return rc;
  AFFT_LAUNCH_CHECK();
  return 0;
}

int run_attention(const char* who, const AttnCall& c, unsigned which, unsigned late, hipStream_t stream) {
  if (int rc = check_attention(who, c, which)) return rc;
  if (c.nseq == 0) return 0;
  const AttnTraffic t = attention_traffic(c);
  const bool step = c.dir == kStep || c.dir == kStepBwd;
  AfftKernelScope ktrace(c.dir == kFwd || c.dir == kStep ? AFFT_K_ATTN_FWD : AFFT_K_ATTN_BWD, c.nseq * (step ? c.Lq : c.L), c.H * c.hd, t.bytes,
                         t.flops, stream);
  if (int rc = check_attention(who, c, late)) return rc;
  const AttnPlan p = plan_attention(c);
  AFFT_CHECK(!p.refusal[0], "%s", p.refusal);
  if (p.family == kGenericShort) return launch_attention_generic(c, p, stream);
  if (p.family == kStepVec || p.family == kStepBwdVec || p.family == kStepSplit) return launch_attention_step(c, p, stream);
  return p.family <= kSlicedBwd ? launch_attention_mfma(c, p, stream) : launch_attention_long(c, p, stream);
}

// the plan of a dense problem as its arguments describe it: one sequence, one head, rows of hd elements (rounded up to whole
// 16-byte units) at 16-byte aligned addresses -- or, pitch_alignment_ok = 0, rows that no 16-byte load can take
extern "C" int afft_attention_plan_for(int32_t direction, int32_t dtype, int32_t L, int32_t hd, int32_t planes, int32_t in_lo,
                                       int32_t pitch_alignment_ok) {
  const int64_t ld = (hd + 7) / 8 * 8 + (pitch_alignment_ok ? 0 : 1);
  void* x = reinterpret_cast<void*>(uintptr_t{4096});      // never dereferenced
  AttnCall c = direction == kFwd ? attn_fwd_call(x, ld, x, ld, x, ld, dtype, 1, L, 1, hd, 1.f, 0.f, 0u, x, ld, nullptr)
                                 : attn_bwd_call(x, ld, x, ld, x, ld, x, ld, dtype, (const float*)x, 1, L, 1, hd, 1.f, 0.f, 0u, x, ld, x, ld, x, ld);
  c.dir = direction;
  if (direction == kBiasBwd) { c.q = c.k = nullptr; c.dq = c.dk = c.dv = nullptr; c.ldq = c.ldk = c.lddq = c.lddk = c.lddv = 0; }
  c.planes = planes != 0;
  c.in_lo = in_lo ? 8 * ld : 0;
  const AttnPlan p = direction >= kFwd && direction <= kBiasBwd ? plan_attention(c) : AttnPlan{};
  if (!p.family) { afft_set_error("%s", p.refusal[0] ? p.refusal : "afft_attention_plan_for: bad direction"); return -1; }
  return p.family * 10000 + p.p0 * 10 + p.p1;
}

extern "C" int afft_attention_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                  int32_t dtype, int32_t nseq, int32_t L, int32_t H, int32_t hd, float scale,
                                  int32_t mask, int32_t mask_period, float drop_p, uint32_t drop_key, void* out,
                                  int64_t ldo, float* probs, void* stream_) {
  AttnCall c = attn_fwd_call(q, ldq, k, ldk, v, ldv, dtype, nseq, L, H, hd, scale, drop_p, drop_key, out, ldo, probs);
  c.mask = mask; c.period = mask_period;
  return run_attention("attention_fwd", c, kChkPtrs | kLenShort | kChkMask | kChkDiag | kChkDrop | kChkHd, kChkDtype, (hipStream_t)stream_);
}

// the arbitrary additive bias: element (seq, h, i, j) at bias[seq*sb + h*sh + i*si + j]; the generic kernel at every shape
static int attention_fwd_bias_impl(const char* who, const AttnCall& c, hipStream_t stream) {
  return run_attention(who, c, kChkPtrs | kChkBias | kLenShort | kChkDrop | kChkHd | kChkDtype, 0, stream);
}

extern "C" int afft_attention_fwd_table(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                        int32_t dtype, int32_t nseq, int32_t L, int32_t H, int32_t hd, float scale,
                                        const float* mask_table, float drop_p, uint32_t drop_key, void* out, int64_t ldo,
                                        float* probs, void* stream_) {
  AttnCall c = attn_fwd_call(q, ldq, k, ldk, v, ldv, dtype, nseq, L, H, hd, scale, drop_p, drop_key, out, ldo, probs);
  c.bias = mask_table; c.si = L;
  return attention_fwd_bias_impl("attention_fwd_table", c, (hipStream_t)stream_);
}

extern "C" int afft_attention_fwd_bias(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                       int32_t dtype, int32_t nseq, int32_t L, int32_t H, int32_t hd, float scale,
                                       const float* bias, int64_t sb, int64_t sh, int64_t si, float drop_p, uint32_t drop_key,
                                       void* out, int64_t ldo, float* probs, void* stream_) {
  AttnCall c = attn_fwd_call(q, ldq, k, ldk, v, ldv, dtype, nseq, L, H, hd, scale, drop_p, drop_key, out, ldo, probs);
  c.bias = bias; c.sb = sb; c.sh = sh; c.si = si;
  if (int rc = check_attention("attention_fwd_bias", c, kChkBiasArgs)) return rc;
  return attention_fwd_bias_impl("attention_fwd_bias", c, (hipStream_t)stream_);
}

extern "C" int afft_attention_fwd_split(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int64_t in_lo,
                                        int32_t nseq, int32_t L, int32_t H, int32_t hd, float scale, int32_t mask, int32_t mask_period,
                                        float drop_p, uint32_t drop_key, void* out_hi, int64_t ldo, int64_t out_lo, void* out_bf16,
                                        int64_t ldob, float* probs, void* out_lo8, void* stream_) {
  AttnCall c = attn_fwd_call(q, ldq, k, ldk, v, ldv, AFFT_F16, nseq, L, H, hd, scale, drop_p, drop_key, out_hi, ldo, probs);
  c.mask = mask; c.period = mask_period;
  c.planes = 1; c.in_lo = in_lo; c.out_lo = out_lo; c.out_b = out_bf16; c.ldob = ldob; c.out_lo8 = out_lo8;
  return run_attention("attention_fwd_split", c, kChkPtrs | kLenSplit | kChkMask | kChkDiag | kChkDrop | kChkPlanes, 0, (hipStream_t)stream_);
}

extern "C" int afft_attention_bwd(const void* dout, int64_t lddo, const void* q, int64_t ldq, const void* k, int64_t ldk,
                                  const void* v, int64_t ldv, int32_t dtype, const float* probs, int32_t nseq, int32_t L,
                                  int32_t H, int32_t hd, float scale, float drop_p, uint32_t drop_key, void* dq,
                                  int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, void* stream_) {
  const AttnCall c = attn_bwd_call(dout, lddo, q, ldq, k, ldk, v, ldv, dtype, probs, nseq, L, H, hd, scale, drop_p, drop_key, dq, lddq, dk, lddk, dv, lddv);
  return run_attention("attention_bwd", c, kChkPtrs | kLenShort | kChkDrop | kChkHd, kChkDtype, (hipStream_t)stream_);
}
