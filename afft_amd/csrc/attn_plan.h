// The dispatch plan of attention: what an entry point was asked (AttnCall), whether the arguments are acceptable (check_attention),
// which kernel instantiation runs it with which launch geometry (plan_attention), and what the kernel trace records (attention_traffic).
// Pure host arithmetic over shapes, pitches and pointer alignments -- no HIP runtime call, no global state but the one cached read of
// AFFT_ATTN_GENERIC (compiles with the plain host compiler) -- and the ONE place that decides: the thirteen entry points (attention.hip,
// attention_long.hip, attention_step.hip) check, plan, open the trace scope and hand the plan to the launcher of the family's file, which only maps it to
// a template instantiation; afft_attention_plan_for reports it.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/afft_hip.h"

void afft_set_error(const char* fmt, ...);      // elementwise.hip (as common.h declares it)

#ifndef AFFT_ATTN_PL_LDS_KB
#define AFFT_ATTN_PL_LDS_KB 48
#endif

namespace afft_attn_detail {

constexpr int LMAX = 128;              // the short kernels: a whole sequence per workgroup
constexpr int LLO = 129, LHI = 512;    // the long kernels (attention_long.hip)
constexpr int QT = 32;                 //   rows of a tile
constexpr int KB = 64;                 //   rows of the other operand staged at a time (MFMA form)
constexpr int STEP_QT = 4;             // the cached step (attention_step.hip): query rows of a workgroup, one per wave in its softmax

enum AttnDir { kFwd = 0, kBwd = 1, kBiasBwd = 2, kStep = 3, kStepBwd = 4 };

// what an entry point was asked to do; fields an entry point does not have stay zero
struct AttnCall {
  int dir, dtype;                      // dtype: AFFT_F32 / AFFT_BF16 (planes: AFFT_F16, not looked at)
  const void *q, *k, *v, *dout;
  int64_t ldq, ldk, ldv, lddo;
  void *out, *dq, *dk, *dv;
  int64_t ldo, lddq, lddk, lddv;
  float* probs;                        // fwd: written (may be null); bwd: read
  int nseq, L, H, hd;
  float scale;
  int mask, period;                    // period: the caller's mask_period (meaningful for AFFT_MASK_BLOCKCAUSAL only)
  float drop_p;
  uint32_t drop_key;
  const float* bias;                   // additive fp32 bias or null: element (seq, h, i, j) at bias[seq*sb + h*sh + i*si + j]
  int64_t sb, sh, si;
  int planes;                          // fp16x2 forward (afft_attention_fwd_split, afft_attention_step_fwd_split): q / k / v / out are hi planes
  int64_t in_lo, out_lo;
  void* out_b;
  int64_t ldob;
  void* out_lo8;
  float* dbias;                        // bias gradient, element strides dsb / dsh / dsi (0: summed over that dimension, through scratch)
  int64_t dsb, dsh, dsi;
  float *scratch, *row_term;
  // the cached step (kStep): Lq new rows per sequence -- q / k / v above are their rows [nseq * Lq, .] -- against L keys, of which the
  // first L - Lq are rows of the caches [nseq, cap, H * hd] (row pitch ldc, sequence stride cache_seq, elements) and the rest are appended
  void *k_cache, *v_cache;
  int64_t ldc, cache_seq;
  int Lq, cap;
  // its backward (kStepBwd): the caches hold all L keys; dq / dk / dv are the gradients of the Lq new rows; the fp32 gradient caches
  // [nseq, cap, H * hd] (row pitch ldg, sequence stride grad_seq) collect what later steps owe earlier keys
  float *gk_cache, *gv_cache;
  int64_t ldg, grad_seq;
};

inline AttnCall attn_fwd_call(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int dtype, int nseq, int L,
                              int H, int hd, float scale, float drop_p, uint32_t drop_key, void* out, int64_t ldo, float* probs) {
  AttnCall c = {};
  c.dir = kFwd; c.dtype = dtype;
  c.q = q; c.k = k; c.v = v; c.ldq = ldq; c.ldk = ldk; c.ldv = ldv;
  c.out = out; c.ldo = ldo; c.probs = probs;
  c.nseq = nseq; c.L = L; c.H = H; c.hd = hd; c.scale = scale; c.drop_p = drop_p; c.drop_key = drop_key;
  return c;
}
inline AttnCall attn_bwd_call(const void* dout, int64_t lddo, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                              int64_t ldv, int dtype, const float* probs, int nseq, int L, int H, int hd, float scale, float drop_p,
                              uint32_t drop_key, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv) {
  AttnCall c = attn_fwd_call(q, ldq, k, ldk, v, ldv, dtype, nseq, L, H, hd, scale, drop_p, drop_key, nullptr, 0, const_cast<float*>(probs));
  c.dir = kBwd;
  c.dout = dout; c.lddo = lddo;
  c.dq = dq; c.dk = dk; c.dv = dv; c.lddq = lddq; c.lddk = lddk; c.lddv = lddv;
  return c;
}

inline AttnCall attn_step_call(const void* q, int64_t ldq, const void* k_new, int64_t ldk, const void* v_new, int64_t ldv, void* k_cache,
                               void* v_cache, int64_t ldc, int64_t cache_seq, int dtype, int nseq, int Lq, int Lk, int cap, int H, int hd,
                               float scale, void* out, int64_t ldo, float* probs, float drop_p = 0.f, uint32_t drop_key = 0u) {
  AttnCall c = attn_fwd_call(q, ldq, k_new, ldk, v_new, ldv, dtype, nseq, Lk, H, hd, scale, drop_p, drop_key, out, ldo, probs);
  c.dir = kStep;
  c.k_cache = k_cache; c.v_cache = v_cache; c.ldc = ldc; c.cache_seq = cache_seq; c.Lq = Lq; c.cap = cap;
  return c;
}
// the step of the "fp16x2" forward (afft_attention_step_fwd_split): q / k_new / v_new / out are fp16 hi planes, the caches fp32
inline AttnCall attn_step_split_call(const void* q, int64_t ldq, const void* k_new, int64_t ldk, const void* v_new, int64_t ldv, int64_t in_lo,
                                     float* k_cache, float* v_cache, int64_t ldc, int64_t cache_seq, int nseq, int Lq, int Lk, int cap, int H,
                                     int hd, float scale, void* out_hi, int64_t ldo, int64_t out_lo, float* probs) {
  AttnCall c = attn_step_call(q, ldq, k_new, ldk, v_new, ldv, k_cache, v_cache, ldc, cache_seq, AFFT_F16, nseq, Lq, Lk, cap, H, hd, scale, out_hi,
                              ldo, probs);
  c.planes = 1; c.in_lo = in_lo; c.out_lo = out_lo;
  return c;
}
inline AttnCall attn_step_bwd_call(const void* dout, int64_t lddo, const void* q, int64_t ldq, const void* k_cache, const void* v_cache,
                                   int64_t ldc, int64_t cache_seq, int dtype, const float* probs, int nseq, int Lq, int Lk, int cap, int H,
                                   int hd, float scale, float drop_p, uint32_t drop_key, void* dq, int64_t lddq, void* dk_new, int64_t lddk,
                                   void* dv_new, int64_t lddv, float* gk_cache, float* gv_cache, int64_t ldg, int64_t grad_seq) {
  AttnCall c = attn_bwd_call(dout, lddo, q, ldq, nullptr, 0, nullptr, 0, dtype, probs, nseq, Lk, H, hd, scale, drop_p, drop_key, dq, lddq,
                             dk_new, lddk, dv_new, lddv);
  c.dir = kStepBwd;
  c.k_cache = const_cast<void*>(k_cache); c.v_cache = const_cast<void*>(v_cache); c.ldc = ldc; c.cache_seq = cache_seq; c.Lq = Lq; c.cap = cap;
  c.gk_cache = gk_cache; c.gv_cache = gv_cache; c.ldg = ldg; c.grad_seq = grad_seq;
  return c;
}

// the bias gradient sums over the dimensions its bias broadcast over (a second kernel, through scratch)
inline bool bias_grad_reduces(const AttnCall& c) { return c.dsb == 0 || c.dsh == 0 || c.dsi == 0; }

// ---- argument checks: `which` selects them, the order is the one below.  An entry point whose checks come in another order (the
// bias entry points look at the bias first) asks twice.
enum : unsigned {
  kChkPtrs = 1u << 0,       // the direction's operands and results
  kChkBias = 1u << 1,       // the bias (table) is not optional
  kChkRowTerm = 1u << 2,
  kChkMask = 1u << 3,       // mask id, block-causal period
  kChkDiag = 1u << 4,       // the diagonal mask needs a second key
  kChkDrop = 1u << 5,
  kChkPlanes = 1u << 6,     // in_lo, out_lo8
  kChkHd = 1u << 7,
  kChkDtype = 1u << 8,
  kChkBatch = 1u << 9,      // nseq, H
  kChkBiasArgs = 1u << 10,  // strides and alignment of the bias (bias gradient: of dbias)
  kChkScratch = 1u << 11,   // a bias gradient that sums needs scratch
  kLenShort = 1u << 12, kLenSplit = 1u << 13, kLenLong = 1u << 14, kLenAll = 1u << 15,      // the entry point's length band
  kChkStep = 1u << 16,      // the cached step: new rows, keys and capacity in order, pitches that hold a row and a sequence's rows
  kChkStepPlanes = 1u << 17,   // its fp16x2 form: lo planes behind their hi planes, alignment of the element types
};

#define AFFT_ATTN_CHECK(cond, ...) \
  do {                             \
    if (!(cond)) {                 \
      afft_set_error(__VA_ARGS__); \
      return 1;                    \
    }                              \
  } while (0)

inline int check_attention(const char* who, const AttnCall& c, unsigned which) {
  const bool ptrs = c.dir == kFwd ? c.q && c.k && c.v && c.out
                    : c.dir == kStep ? c.q && c.k && c.v && c.out && c.k_cache && c.v_cache
                    : c.dir == kStepBwd ? c.dout && c.q && c.k_cache && c.v_cache && c.probs && c.dq && c.dk && c.dv && c.gk_cache && c.gv_cache
                    : c.dir == kBwd ? c.dout && c.q && c.k && c.v && c.probs && c.dq && c.dk && c.dv
                                    : c.dout && c.v && c.probs && c.dbias;
  AFFT_ATTN_CHECK((!(which & kChkPtrs) || ptrs) && (!(which & kChkBias) || c.bias) && (!(which & kChkRowTerm) || c.row_term),
                  "%s: null pointer", who);
  if (which & (kLenShort | kLenSplit | kLenLong | kLenAll)) {
    const int lo = which & kLenLong ? LLO : 1, hi = which & kLenShort ? LMAX : which & kLenSplit ? 64 : LHI;
    AFFT_ATTN_CHECK(c.L >= lo && c.L <= hi, "%s: sequence length %d outside %d..%d%s", who, c.L, lo, hi, which & kLenSplit ? " (MFMA path only)" : "");
  }
  if (which & kChkMask) {
    AFFT_ATTN_CHECK(c.mask >= AFFT_MASK_NONE && c.mask <= AFFT_MASK_BLOCKCAUSAL, "%s: bad mask %d", who, c.mask);
    AFFT_ATTN_CHECK(c.mask != AFFT_MASK_BLOCKCAUSAL || (c.period >= 1 && c.L % c.period == 0),
                    "%s: block-causal mask needs a period that divides L (L=%d, period=%d)", who, c.L, c.period);
  }
  if (which & kChkDiag) AFFT_ATTN_CHECK(!(c.mask == AFFT_MASK_DIAG && c.L == 1), "%s: diagonal mask with L=1 masks every key", who);
  if (which & kChkDrop) AFFT_ATTN_CHECK(c.drop_p >= 0.f && c.drop_p < 1.f, "%s: dropout p outside [0,1)", who);
  if (which & kChkPlanes) {
    AFFT_ATTN_CHECK(c.in_lo >= 0, "%s: in_lo is the distance to the inputs' lo planes (0: one fp16 plane each)", who);
    AFFT_ATTN_CHECK(!c.out_lo8 || (c.out_lo == 0 && (((uintptr_t)c.out_lo8) & 3) == 0), "%s: out_lo8 excludes out_lo and must be 4-byte aligned", who);
  }
  if (which & kChkHd) AFFT_ATTN_CHECK(c.hd >= 1 && c.hd <= 1024, "%s: head dimension %d outside 1..1024", who, c.hd);
  if (which & kChkDtype) AFFT_ATTN_CHECK(c.dtype == AFFT_F32 || c.dtype == AFFT_BF16, "%s: bad dtype %d", who, c.dtype);
  if (which & kChkBatch) AFFT_ATTN_CHECK(c.nseq >= 0 && c.H >= 1, "%s: bad nseq %d / H %d", who, c.nseq, c.H);
  if (which & kChkStep) {
    AFFT_ATTN_CHECK(c.Lq >= 1 && c.Lq <= c.L, "%s: %d new rows against %d keys (1 <= Lq <= Lk)", who, c.Lq, c.L);
    AFFT_ATTN_CHECK(c.L <= c.cap, "%s: %d keys do not fit a cache of %d rows", who, c.L, c.cap);
    const int64_t w = (int64_t)c.H * c.hd;
    const bool pitches = c.dir == kStep ? c.ldq >= w && c.ldk >= w && c.ldv >= w && c.ldo >= w && c.ldc >= w
                                        : c.lddo >= w && c.ldq >= w && c.ldc >= w && c.lddq >= w && c.lddk >= w && c.lddv >= w && c.ldg >= w;
    AFFT_ATTN_CHECK(pitches, "%s: a row pitch is below H * hd = %lld", who, (long long)w);
    AFFT_ATTN_CHECK(c.cache_seq >= (int64_t)(c.cap - 1) * c.ldc + w, "%s: cache sequence stride %lld does not hold %d rows of pitch %lld", who,
                    (long long)c.cache_seq, c.cap, (long long)c.ldc);
    if (c.dir == kStepBwd) {
      AFFT_ATTN_CHECK(c.grad_seq >= (int64_t)(c.cap - 1) * c.ldg + w, "%s: gradient cache sequence stride %lld does not hold %d rows of pitch %lld",
                      who, (long long)c.grad_seq, c.cap, (long long)c.ldg);
      AFFT_ATTN_CHECK(((((uintptr_t)c.gk_cache) | ((uintptr_t)c.gv_cache) | ((uintptr_t)c.probs)) & 3) == 0,
                      "%s: the gradient caches and probs must be 4-byte aligned", who);
    }
  }
  if (which & kChkStepPlanes) {      // a lo plane starts behind the last element of its hi plane: an offset inside the hi plane would make
    // two lanes write one address (out) or read a value as its own correction (in); 0 = no lo plane
    const int64_t w = (int64_t)c.H * c.hd, rows = (int64_t)c.nseq * c.Lq;
    const int64_t ldin = c.ldq > c.ldk ? (c.ldq > c.ldv ? c.ldq : c.ldv) : (c.ldk > c.ldv ? c.ldk : c.ldv);
    AFFT_ATTN_CHECK(c.in_lo == 0 || (rows > 0 && c.in_lo >= (rows - 1) * ldin + w),
                    "%s: in_lo %lld lies inside the hi plane (0: no lo plane, else at least (nseq * Lq - 1) * pitch + H * hd = %lld)", who,
                    (long long)c.in_lo, (long long)((rows - 1) * ldin + w));
    AFFT_ATTN_CHECK(c.out_lo == 0 || (rows > 0 && c.out_lo >= (rows - 1) * c.ldo + w),
                    "%s: out_lo %lld lies inside the hi plane (0: no lo plane, else at least (nseq * Lq - 1) * pitch + H * hd = %lld)", who,
                    (long long)c.out_lo, (long long)((rows - 1) * c.ldo + w));
    AFFT_ATTN_CHECK(((((uintptr_t)c.q) | ((uintptr_t)c.k) | ((uintptr_t)c.v) | ((uintptr_t)c.out)) & 1) == 0 &&
                    ((((uintptr_t)c.k_cache) | ((uintptr_t)c.v_cache) | ((uintptr_t)c.probs)) & 3) == 0,
                    "%s: fp16 planes must be 2-byte aligned, the fp32 caches and probs 4-byte aligned", who);
  }
  if (which & kChkBiasArgs) {
    const bool grad = c.dir == kBiasBwd;
    const int64_t sb = grad ? c.dsb : c.sb, sh = grad ? c.dsh : c.sh, si = grad ? c.dsi : c.si;
    const void* p = grad ? (const void*)c.dbias : (const void*)c.bias;
    AFFT_ATTN_CHECK(sb >= 0 && sh >= 0 && si >= 0, "%s: negative bias stride (sb=%lld, sh=%lld, si=%lld)", who, (long long)sb, (long long)sh,
                    (long long)si);
    AFFT_ATTN_CHECK((((uintptr_t)p) & 3) == 0, "%s: %s pointer %p is not 4-byte aligned", who, grad ? "dbias" : "bias", p);
  }
  if (which & kChkScratch)
    AFFT_ATTN_CHECK(!bias_grad_reduces(c) || (c.scratch && (((uintptr_t)c.scratch) & 3) == 0),
                    "%s: a broadcast bias needs 4-byte aligned scratch of nseq*H*L*L floats (scratch=%p)", who, (void*)c.scratch);
  return 0;
}
#undef AFFT_ATTN_CHECK

// ---- the trace record of a call (AfftKernelScope): algorithmic bytes (operands read once, results written once) and MFMA-shaped flops
struct AttnTraffic { int64_t bytes, flops; };
inline AttnTraffic attention_traffic(const AttnCall& c) {
  const int64_t es = c.dtype == AFFT_F32 ? 4 : 2, rw = (int64_t)c.nseq * c.L * c.H * c.hd, pb = (int64_t)c.nseq * c.H * c.L * c.L * 4;
  const int64_t product = 2 * (int64_t)c.nseq * c.H * c.L * c.L * c.hd;      // one L x L x hd product
  if (c.dir == kStep && c.planes) {      // the same with fp16 planes in and out (2 bytes each, those that are there) and fp32 caches
    const int64_t row = (int64_t)c.nseq * c.H * c.hd, past = c.L - c.Lq;
    return {row * (c.Lq * (3 * (c.in_lo ? 4 : 2) + 8 + (c.out_lo ? 4 : 2)) + 8 * past) + (c.probs ? (int64_t)c.nseq * c.H * c.Lq * c.L * 4 : 0),
            4 * (int64_t)c.nseq * c.H * c.Lq * c.L * c.hd};
  }
  if (c.dir == kStep) {      // q, k_new, v_new read, both appended, the past read, out and probs written
    const int64_t row = es * c.nseq * c.H * c.hd, past = c.L - c.Lq;
    return {row * (6 * c.Lq + 2 * past) + (c.probs ? (int64_t)c.nseq * c.H * c.Lq * c.L * 4 : 0), 4 * (int64_t)c.nseq * c.H * c.Lq * c.L * c.hd};
  }
  if (c.dir == kStepBwd) {   // dout, q read, the L keys and values read, dq / dk_new / dv_new written; the fp32 gradient caches: the past read
    const int64_t row = (int64_t)c.nseq * c.H * c.hd, past = c.L - c.Lq;      // and written, the new rows read; probs read
    return {es * row * (5 * c.Lq + 2 * c.L) + 4 * row * (4 * past + 2 * c.Lq) + (int64_t)c.nseq * c.H * c.Lq * c.L * 4,
            8 * (int64_t)c.nseq * c.H * c.Lq * c.L * c.hd};
  }
  if (c.dir == kBiasBwd) return {2 * es * rw + (bias_grad_reduces(c) ? 3 : 2) * pb, product};
  // backward: the four products (the long form makes dP twice, once per pass: 10 L^2 hd are executed)
  if (c.dir == kBwd) return {7 * es * rw + pb, 4 * product};
  if (c.planes)      // three fp16 products per product; the planes that are there
    return {(3 * (c.in_lo ? 4 : 2) + (c.out_lo ? 4 : c.out_lo8 ? 3 : 2) + (c.out_b ? 2 : 0)) * rw + (c.probs ? pb : 0), 3 * 2 * product};
  return {4 * es * rw + (c.probs ? pb : 0), 2 * product};
}

// ---- the plan
enum AttnFamily {
  kGenericShort = 1,        // attention.hip attn_fwd_kernel / attn_bwd_kernel<T, LM = p0>
  kMfmaFwd = 2,             // attention_mfma.hip attn_fwd_mfma_kernel<NT = p0, PL = p1>
  kMfmaBwd = 3,             //                    attn_bwd_mfma_kernel<NT = p0>
  kSlicedBwd = 4,           //                    attn_bwd_sliced_kernel<NT = p0>
  kLongF32 = 5, kLongBf16 = 6, kLongMfma = 7,      // attention_long.hip long_fwd_kernel / long_bwd_q_kernel + long_bwd_kv_kernel
  kBiasF32 = 8, kBiasBf16 = 9, kBiasMfma = 10,     //                    bias_bwd_ds_kernel (+ bias_bwd_reduce_kernel)
  kStepVec = 11,            // attention_step.hip attn_step_kernel<T, V = p0, DROP = p1>: p0 = 1, 16-byte loads; 0, element loads
  kStepBwdVec = 12,         //                    attn_step_bwd_kernel<T, V = p0>
  kStepSplit = 13,          //                    attn_step_kernel<Planes, V = p0, false>: fp16 planes in and out, fp32 caches; p0 as family 11
};

struct AttnPlan {
  int family;               // AttnFamily
  int p0, p1;               // template parameters: LM or NT; PL
  int hc;                   // head-dimension chunk staged in LDS at a time (MFMA families)
  int G;                    // short MFMA: sequences packed into one workgroup's 16 NT rows
  int Lp, ntiles;           // long: L rounded up to KB; tiles of QT rows.  step: L rounded up to 4; tiles of STEP_QT query rows
  size_t lds;               // dynamic LDS bytes of the launch
  unsigned grid;
  char refusal[160];        // not empty: the call fails with this message (the fp16x2 forward is the only one without a fallback)
};

// AFFT_ATTN_GENERIC=1: bf16 on the generic kernels (A/B runs, tests); read once
inline bool attn_generic_forced() {
  static int v = -1;
  if (v < 0) { const char* e = getenv("AFFT_ATTN_GENERIC"); v = (e && e[0] == '1') ? 1 : 0; }
  return v == 1;
}

inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
inline bool al8(const void* p) { return (((uintptr_t)p) & 7) == 0; }

// what the MFMA kernels need of their operands: 16-byte loads of the inputs, 8-byte stores of the results (absent ones are null / 0)
inline bool mfma_operands_ok(const AttnCall& c) {
  const bool in = c.ldq % 8 == 0 && c.ldk % 8 == 0 && c.ldv % 8 == 0 && c.lddo % 8 == 0 && al16(c.q) && al16(c.k) && al16(c.v) && al16(c.dout);
  const bool out = c.ldo % 4 == 0 && c.lddq % 4 == 0 && c.lddk % 4 == 0 && c.lddv % 4 == 0 && al8(c.out) && al8(c.dq) && al8(c.dk) && al8(c.dv);
  const bool planes = !c.planes || (c.in_lo % 8 == 0 && c.in_lo >= 0 && c.out_lo % 4 == 0 && c.ldob % 4 == 0 && al8(c.out_b));
  return in && out && planes;
}

// L <= 64 on the MFMA kernels of attention_mfma.hip; false: not theirs
inline bool plan_short_mfma(const AttnCall& c, AttnPlan& p) {
  const bool bwd = c.dir == kBwd;
  const int hd = c.hd;
  if (c.L > 64 || hd % 64 != 0 || hd > 1024 || (c.planes && c.dir != kFwd) || c.bias || !mfma_operands_ok(c)) return false;      // (these kernels add no bias)
  const int NT = c.L > 32 ? 4 : c.L > 16 ? 2 : 1;
  // the whole head dimension in LDS when it fits (3 tiles forward, 4 backward); else chunks of the head dimension,
  // the scores / dP accumulate over the chunks and the operand tiles are re-staged (2 tiles forward, 3 backward)
  int hc = hd;
  const int np = (c.planes && c.in_lo) ? 2 : 1;       // fp16x2 forward: every operand tile is two planes (in_lo = 0: the hi plane alone)
  size_t lds = (size_t)(bwd ? 4 : 3) * np * 16 * NT * hd * 2;
  // planes (fp16x2 forward): the two-plane tiles of a whole head (96 KiB at hd = 512) leave ONE workgroup per CU, whose load -> barrier ->
  // compute -> store runs with nothing beside it (2.75 TB/s); chunks that fit 48 KiB keep three workgroups per CU in flight
  const size_t budget = (c.planes && !bwd) ? (size_t)(AFFT_ATTN_PL_LDS_KB) * 1024 : (size_t)160 * 1024;
  if (lds > budget) {
    hc = 0;
    for (int cand = hd / 2; cand >= 64; cand /= 2)
      if (hd % cand == 0 && cand % 64 == 0 && (size_t)(bwd ? 3 : 2) * np * 16 * NT * cand * 2 <= budget) { hc = cand; break; }
    if (!hc) return false;
    lds = (size_t)(bwd ? 3 : 2) * np * 16 * NT * hc * 2;
  }
  p.family = bwd ? kMfmaBwd : kMfmaFwd;
  p.p0 = NT;
  p.p1 = !c.planes ? 0 : c.in_lo ? 1 : 2;
  if (bwd && NT <= 2 && hd % 128 == 0 && hd <= 512 && c.lddq % 8 == 0 && c.lddk % 8 == 0 && c.lddv % 8 == 0 && al16(c.dq) && al16(c.dk) && al16(c.dv)) {
    // column-sliced backward (attn_bwd_sliced_kernel): 2 wave-private buffers of [16 NT][hd / 4] bf16 per wave + the partial dP tiles
    p.family = kSlicedBwd;
    lds = (size_t)4 * 2 * 16 * NT * (hd / 4) * 2 + (size_t)4 * 2 * NT * NT * 64 * 16;
  }
  p.hc = hc;
  p.lds = lds;
  p.G = (16 * NT) / c.L;
  p.grid = (unsigned)(((c.nseq + p.G - 1) / p.G) * c.H);
  return true;
}

// the cached step: one workgroup per (sequence, head, tile of STEP_QT new rows); LDS = the tile's fp32 scores [rows][Lp] and the P V
// partial sums of waves 1..3, [3][rows][hd rounded up to 8].  Its backward: one workgroup per (sequence, head) that walks the tiles with
// the same carve (dP, then dS; the dS K partial sums) plus the Lq row terms the key pass reads
inline AttnPlan plan_attention_step(const AttnCall& c) {
  AttnPlan p = {};
  const bool f32 = c.dtype == AFFT_F32;
  const bool planes = c.planes && c.dir == kStep;      // afft_attention_step_fwd_split
  if (c.Lq < 1 || c.Lq > c.L || c.L > LHI || c.hd < 1 || c.hd > 1024 || (!planes && !f32 && c.dtype != AFFT_BF16) || (c.planes && !planes)) {
    snprintf(p.refusal, sizeof p.refusal, "attention_step: no kernel for Lq = %d, Lk = %d, head dimension %d, dtype %d", c.Lq, c.L, c.hd, c.dtype);
    return p;
  }
  const int vec = f32 ? 4 : 8;      // elements of a 16-byte load
  const int rows = c.Lq < STEP_QT ? c.Lq : STEP_QT;
  p.Lp = (c.L + 3) / 4 * 4;
  p.ntiles = (c.Lq + STEP_QT - 1) / STEP_QT;
  p.lds = sizeof(float) * rows * ((size_t)p.Lp + 3 * (size_t)((c.hd + 7) / 8 * 8));
  if (c.dir == kStepBwd) {      // (fp32 gradient-cache rows start at a column that is a multiple of vec >= 4: float4 accesses need ldg % 4 only)
    const bool pitches = c.lddo % vec == 0 && c.ldq % vec == 0 && c.ldc % vec == 0 && c.cache_seq % vec == 0 && c.lddq % vec == 0 &&
                         c.lddk % vec == 0 && c.lddv % vec == 0 && c.ldg % 4 == 0 && c.grad_seq % 4 == 0;
    p.family = kStepBwdVec;
    p.p0 = c.hd % vec == 0 && pitches && al16(c.dout) && al16(c.q) && al16(c.k_cache) && al16(c.v_cache) && al16(c.dq) && al16(c.dk) &&
           al16(c.dv) && al16(c.gk_cache) && al16(c.gv_cache);
    p.lds += sizeof(float) * (size_t)c.Lq;
    p.grid = (unsigned)((int64_t)c.nseq * c.H);
    return p;
  }
  if (planes) {      // 8 elements a lane: one 16-byte load of an fp16 plane, two of an fp32 cache row (head columns start at a multiple of hd)
    const bool pitches = c.ldq % 8 == 0 && c.ldk % 8 == 0 && c.ldv % 8 == 0 && c.ldo % 8 == 0 && c.in_lo % 8 == 0 && c.out_lo % 8 == 0 &&
                         c.ldc % 4 == 0 && c.cache_seq % 4 == 0;
    p.family = kStepSplit;
    p.p0 = c.hd % 8 == 0 && pitches && al16(c.q) && al16(c.k) && al16(c.v) && al16(c.k_cache) && al16(c.v_cache) && al16(c.out);
    p.grid = (unsigned)((int64_t)c.nseq * c.H * p.ntiles);
    return p;
  }
  const bool pitches = c.ldq % vec == 0 && c.ldk % vec == 0 && c.ldv % vec == 0 && c.ldc % vec == 0 && c.cache_seq % vec == 0 && c.ldo % vec == 0;
  p.family = kStepVec;
  p.p0 = c.hd % vec == 0 && pitches && al16(c.q) && al16(c.k) && al16(c.v) && al16(c.k_cache) && al16(c.v_cache) && al16(c.out);
  p.p1 = c.drop_p > 0.f;
  p.grid = (unsigned)((int64_t)c.nseq * c.H * p.ntiles);
  return p;
}

inline AttnPlan plan_attention(const AttnCall& c) {
  if (c.dir == kStep || c.dir == kStepBwd) return plan_attention_step(c);
  AttnPlan p = {};
  const bool f32 = c.dtype == AFFT_F32, bf16 = c.dtype == AFFT_BF16;
  if (c.L < 1 || c.L > LHI || (!c.planes && (c.hd < 1 || c.hd > 1024 || (!f32 && !bf16)))) {
    snprintf(p.refusal, sizeof p.refusal, "attention: no kernel for L = %d, head dimension %d, dtype %d", c.L, c.hd, c.dtype);
    return p;
  }
  const bool mfma = bf16 && !attn_generic_forced();      // the fp16x2 forward has no generic form: it does not ask
  if ((c.planes || (mfma && c.dir != kBiasBwd)) && plan_short_mfma(c, p)) return p;
  if (c.planes) {
    snprintf(p.refusal, sizeof p.refusal,
             "attention_fwd_split: shape not handled by the MFMA path (hd %d must be a multiple of 64 and <= 1024, 16-byte aligned rows)", c.hd);
    return p;
  }
  if (c.dir == kBiasBwd || c.L > LMAX) {      // tiles of QT rows around an fp32 strip [QT][Lp] (attention_long.hip); the bias gradient at every L
    const bool long_mfma = mfma && c.hd % 64 == 0 && mfma_operands_ok(c);
    p.family = (c.dir == kBiasBwd ? kBiasF32 : kLongF32) + (f32 ? 0 : long_mfma ? 2 : 1);
    p.Lp = (c.L + KB - 1) / KB * KB;
    p.ntiles = (c.L + QT - 1) / QT;
    p.hc = c.hd % 256 == 0 ? 256 : c.hd % 128 == 0 ? 128 : 64;
    p.lds = (size_t)QT * (p.Lp + 4) * sizeof(float) + (long_mfma ? (size_t)(QT + KB) * p.hc * 2 : 0);
    p.grid = (unsigned)((int64_t)c.nseq * c.H * p.ntiles);
    return p;
  }
  p.family = kGenericShort;      // the L x L fp32 scores (backward: P and dP) of a sequence in LDS, LM + 1 floats a row
  p.p0 = c.L <= 32 ? 32 : c.L <= 64 ? 64 : 128;
  p.lds = sizeof(float) * (c.dir == kBwd ? 2 : 1) * p.p0 * (p.p0 + 1);
  p.grid = (unsigned)(c.nseq * c.H);
  return p;
}

}  // namespace afft_attn_detail

#ifdef __HIPCC__      // the launchers of the four files: a switch from plan to template instantiation each
int launch_attention_generic(const afft_attn_detail::AttnCall& c, const afft_attn_detail::AttnPlan& p, hipStream_t stream);      // attention.hip
int launch_attention_mfma(const afft_attn_detail::AttnCall& c, const afft_attn_detail::AttnPlan& p, hipStream_t stream);         // attention_mfma.hip
int launch_attention_long(const afft_attn_detail::AttnCall& c, const afft_attn_detail::AttnPlan& p, hipStream_t stream);         // attention_long.hip
int launch_attention_step(const afft_attn_detail::AttnCall& c, const afft_attn_detail::AttnPlan& p, hipStream_t stream);         // attention_step.hip
// check -> nseq == 0 -> trace scope -> `late` checks -> plan -> launch: the body of every entry point (attention.hip)
int run_attention(const char* who, const afft_attn_detail::AttnCall& c, unsigned which, unsigned late, hipStream_t stream);
#endif
