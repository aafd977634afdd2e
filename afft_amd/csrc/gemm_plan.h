// The dispatch plan of afft_gemm's MFMA fast path: which kernel instantiation runs a problem and how many K-slices it gets.
// Pure host arithmetic over shapes, pitches and the tuning words -- no HIP runtime call, no global state (compiles with the plain
// host compiler) -- and the ONE place that decides: afft_gemm launches what plan_gemm returns, the trace hook and afft_gemm_plan_for
// report it, the afft_gemm_*_for queries ask it (gemm.hip).  The launchers (gemm.hip launch_fast, gemm_pp.hip, gemm_bd.hip) only map
// the plan to a template instantiation.
// The build switches below (AFFT_G2, AFFT_PP2, AFFT_PP2_X3_OFF, AFFT_PP2_PLANES_OFF, AFFT_PP_NT_ONLY, AFFT_EXPERIMENT_Q4) are read
// where the plan is made: they belong on gemm.hip's command line (AFFT_PP_NT_ONLY on gemm_pp.hip's as well).
#pragma once
#include <stdint.h>

#include <algorithm>

#include "../../include/afft_hip.h"

namespace afft_gemm_detail {

constexpr int BK = 64;

// what the decision reads of an afft_gemm_t that passed the fast-path gate
struct GemmProblem {
  int M, N, K;              // K: the logical one (afft_gemm_t.K); GemmPlan.K counts every segment of the split modes
  bool a_ks, b_ks;          // operand is k-strided (A[K][M] / B[K][N]) rather than k-contiguous
  int64_t lda, ldb;         // row pitches in elements
  int64_t lda8, ldb8;       // split3 = 3: pitches of the e4m3 byte planes in bf16_t units (afft_gemm_t.a8_ld / 2)
  int64_t a_lo, b_lo;
  int split3;               // afft_gemm_t.split3
  bool b_packed;            // a usable fragment-packed B was given (afft_gemm_t.b_packed set and ldb == K)
  int64_t ws_bytes;         // split-K workspace offered (0: none)
};

struct GemmTuning {
  int variant;              // afft_set_gemm_variant: 0 auto, 1 = 128x128 tile, 2 = 256x128 tile, 3 = 256x256 ping-pong (tuning / tests)
  int splitk_mode;          // 128x128 kernel: 0 off, 1 auto, 2 / 4: force that many slices wherever the shape allows (tests, tuning)
  int bd_mode;              // AFFT_BD_MODE: 0 = never, 1 = by the model (default), 2 = whenever the shape is eligible
  int ncu;                  // CUs of the current device
};

struct GemmPlan {
  int kernel;               // afft_gemm_trace_rec_t.variant: 1 / 12 / 4 (gemm.hip), 3 / 13 (gemm_pp.hip), 7-10 (gemm_bd.hip), 11 (AFFT_EXPERIMENT_Q4)
  int x3;                   // the instantiation's X3: split3 with the one fp16 pass (4) on the two-pass instantiation (2)
  int splitk;               // K-slices (1 = no split-K)
  int K;                    // GemmFast.K: every segment, in 64-wide K-tiles of 128 B per row
  bool b_from_packed;       // B is read from afft_gemm_t.b_packed (the B-direct shortcut), not from afft_gemm_t.B
  const char* refusal;      // not null: afft_gemm fails with this message
};

#ifndef AFFT_G2
#define AFFT_G2 1      // 0: every 128x128 launch on gemm_bf16_kernel (A/B builds)
#endif
#ifndef AFFT_PP2
#define AFFT_PP2 1      // 0: every shape on gemm_bf16_pp_kernel (A/B builds)
#endif

// Split-K workspace: provided by the caller per launch (afft_gemm_t.workspace, private to the stream): AFFT_GEMM_WS_HEADER
// bytes of arrival counters (zero between launches) followed by the fp32 partial tiles.  Nothing is allocated here.
constexpr int kMaxSplitTiles = AFFT_GEMM_WS_HEADER / (int)sizeof(int);

// the running K offset lives in a 32-bit VGPR (k-strided operands: K rows of `ld` elements): the whole walk must stay below 4 GiB
inline bool walk_fits32(bool ks, int K, int64_t ld) { return ks ? (int64_t)(K + 8) * ld * 2 < (1LL << 32) : (8 * ld + K) * 2 < (1LL << 32); }

// gemm_bf16_g2_kernel: whole tiles, even K-tile count per slice: the steady-state kernel
inline bool g2_shape(int M, int N, int K, int splitk) {
  return AFFT_G2 && M % 128 == 0 && N % 128 == 0 && K % (BK * splitk) == 0 && (K / BK / splitk) % 2 == 0 && K / BK / splitk >= 2;
}

inline bool pp2_shape(int M, int N, int K) { return AFFT_PP2 && M % 256 == 0 && N % 256 == 0 && K % (2 * BK) == 0 && K >= 4 * BK; }

// fp16 + fp8 forward (X3 = 3): K counts both segments in 64-wide K-tiles (nk_seg + nk_seg / 2); pairs in both: nk_seg % 4 == 0, nk_seg >= 4
inline bool pp2x3_takes(const GemmProblem& p, int K) {
#ifdef AFFT_PP2_X3_OFF
  return false;
#else
  const int nk_seg = p.K / BK;
  return AFFT_PP2 && p.M % 256 == 0 && p.N % 256 == 0 && nk_seg % 4 == 0 && nk_seg >= 4 && K == nk_seg * BK + nk_seg * BK / 2 &&
         walk_fits32(false, nk_seg * BK, p.lda) && walk_fits32(false, nk_seg * BK, p.ldb) && walk_fits32(false, nk_seg * BK, p.lda8) &&
         walk_fits32(false, nk_seg * BK, p.ldb8);
#endif
}

// bf16x3 / fp16 two-pass (X3 = 1 / 2): K counts all segments; whole tiles, an even number of K-tiles per segment (pairs never straddle a
// segment), every plane inside the 32-bit walk
inline bool pp2planes_takes(const GemmProblem& p, int x3, int K) {
#ifdef AFFT_PP2_PLANES_OFF
  return false;
#else
  const int nk_seg = p.K / BK;
  const int64_t span = ((int64_t)(p.a_lo > p.b_lo ? p.a_lo : p.b_lo)) * 2;
  const bool one_pass = x3 == 2 && K == nk_seg * BK && nk_seg >= 4;      // afft_gemm_t.split3 = 4: the first segment alone (no jump is ever taken)
  return AFFT_PP2 && p.M % 256 == 0 && p.N % 256 == 0 && nk_seg % 2 == 0 && nk_seg >= 2 && (K == (x3 == 1 ? 3 : 2) * nk_seg * BK || one_pass) &&
         span < (1LL << 30) && walk_fits32(p.a_ks, nk_seg * BK, p.lda) && walk_fits32(p.b_ks, nk_seg * BK, p.ldb) &&
         (p.a_ks ? (int64_t)nk_seg * BK * p.lda * 2 : (int64_t)8 * p.lda * 2) + span < (1LL << 31) &&
         (p.b_ks ? (int64_t)nk_seg * BK * p.ldb * 2 : (int64_t)8 * p.ldb * 2) + span < (1LL << 31);
#endif
}

// the 256x256 ping-pong tile: 13 = the steady-state kernel (gemm_bf16_pp2_kernel), 3 = the general one (gemm_bf16_pp_kernel)
inline int pp_kernel(const GemmProblem& p, int x3, int K) {
#ifndef AFFT_PP_NT_ONLY   // development switch: build only the plain NT instantiation (compile time)
  if (x3 == 3) return pp2x3_takes(p, K) ? 13 : 3;
  if (x3) return pp2planes_takes(p, x3, K) ? 13 : 3;
#endif
  return pp2_shape(p.M, p.N, K) && walk_fits32(p.a_ks, K, p.lda) && walk_fits32(p.b_ks, K, p.ldb) ? 13 : 3;
}

// the 128x128 tile, 2 stages, plain bf16 or fp16 operands (X3 = 0 / 2): 12 = the steady-state kernel (gemm_bf16_g2_kernel), 1 = the general one (gemm_bf16_kernel)
inline int g128_kernel(const GemmProblem& p, int x3, int K, int splitk) {
  const bool fits32 = walk_fits32(p.a_ks, K, p.lda) && walk_fits32(p.b_ks, K, p.ldb);      // the running K offset is a 32-bit VGPR
  const bool one_segment = x3 == 0 || K == p.K / BK * BK;      // X3 = 2: only the one-pass form (split3 = 4) -- the kernel has no operand planes
  return fits32 && one_segment && g2_shape(p.M, p.N, K, splitk) ? 12 : 1;
}

// "B direct" kernel on a fragment-packed weight (afft_gemm_t.b_packed, gemm_bd.hip) against the 256x256 ping-pong kernel: a cost
// model in us fitted to both kernels alone on one MI355X (profiles/r04_gemm_bd.txt).  Ping-pong: one workgroup per CU, a K-tile
// of a full round costs ~1.9 us, of a last round with <= 160 busy CUs 1.4 us (the part is power-limited), + 10 us; B-direct
// 160x256 tiles: 1.09 us per K-tile and round + 8.8 us per round (prologue drain + epilogue, one workgroup per CU and no
// overlap between tiles).  Taken only when its grid is ONE round (N = 2048 outputs of M = 5120 rows: 256 tiles on 256 CUs where
// 256-row tiles give 160): inside the model's forward pass the multi-round shapes measured slower than the ping-pong kernel
// (fc1 with its GELU epilogue 229 vs 201 us: four rounds of epilogues with nothing beside them), the one-round shapes faster
// (fc2 162 vs 184 us, projection 64 vs 67 us; profiles/r04_gemm_bd.txt "in the step").
// AFFT_BD_MODE: 0 = never, 1 = by the model (default), 2 = whenever the shape is eligible.
inline bool bd_packed_wins(int M, int N, int K, const GemmTuning& t) {
  if (t.bd_mode == 0 || N % 16 != 0 || N < 256 || K % 64 != 0) return false;
  const int ncu = t.ncu, nk = K / BK;
  const int64_t t160 = (int64_t)((M + 159) / 160) * ((N + 255) / 256), t256 = (int64_t)((M + 255) / 256) * ((N + 255) / 256);
  if (t256 < 160) return false;                      // small grids: the 128x128 kernel's territory
  if (t.bd_mode >= 2) return true;
  const int64_t r160 = (t160 + ncu - 1) / ncu, r256 = (t256 + ncu - 1) / ncu;
  if (r160 != 1) return false;
  const int64_t busy = t256 - (r256 - 1) * ncu;
  const double last = 1.4 + 0.5 * (double)std::max<int64_t>(0, busy - 160) / 96.0;
  const double pp_us = nk * ((double)(r256 - 1) * 1.9 + last) + 10.0;
  const double bd_us = (double)r160 * (nk * 1.09 + 8.8);
  return bd_us < pp_us;
}

// B-direct kernels (gemm_bd.hip): k-contiguous operands only, whole 16-column blocks
inline bool bd_ok(int N, bool A_KS, bool B_KS) { return !A_KS && !B_KS && N >= 16 && N % 16 == 0; }

// the tile shape, in afft_set_gemm_variant's numbers
inline int choose_variant(int M, int N, bool A_KS, bool B_KS, const GemmTuning& t) {
  if (t.variant >= 7 && t.variant <= 10) { if (bd_ok(N, A_KS, B_KS)) return t.variant; }
#ifdef AFFT_EXPERIMENT_Q4
  else if (t.variant == 11) { if (!A_KS && !B_KS) return 11; }      // four-quadrant kernel: k-contiguous operands only
#endif
  else if (t.variant != 0) return t.variant;
  // measured (profiles/r01_gemm_variants_bench2.txt): the 256x256 ping-pong kernel (1 workgroup/CU) wins once its
  // grid covers >= ~60 % of the CUs; below that (GPT-2's M = 1024 GEMMs, small weight gradients) two independent
  // 128x128 workgroups per CU win.  The 256x128 3-stage shape (variant 2) never wins and is kept for reference.
  const int64_t t3 = (int64_t)((M + 255) / 256) * ((N + 255) / 256);
  if (t3 < 160) return 1;
  // Both shapes waste the slots of their last, partial round (256 slots of one 256x256 tile, 512 of two 128x128 tiles per
  // CU); per FLOP the big tile is ~1.25x as efficient.  Round 2 (profiles/r02_gemm_ek100_shapes.txt): 5120x4096x1024 is 320
  // big tiles = 1.25 rounds (57 us on 128x128 tiles, 66 us on 256x256), 5120x3072x1024 is 240 = one nearly full round (45
  // vs 38 us); 5120x2048x2048 (160 big tiles) 60 vs 55 us.
  const int64_t t1 = (int64_t)((M + 127) / 128) * ((N + 127) / 128);
  const int ncu = t.ncu;
  const double u3 = (double)t3 / ((double)ncu * ((t3 + ncu - 1) / ncu)), u1 = (double)t1 / (2.0 * ncu * ((t1 + 2 * ncu - 1) / (2 * ncu)));
  return u3 * 1.25 >= u1 ? 3 : 1;
}

// K-slices afft_gemm will use for a fast-path problem (1 = no split-K)
inline int choose_splitk(int variant, int M, int N, int K, const GemmTuning& t) {
  if (!t.splitk_mode) return 1;
  const int nk = K / BK;
  if (variant == 3) return 1;     // 256x256 tiles never split K (stream-K was built, measured slower on this power-limited part and removed: profiles/HISTORY.md)
  // 128x128 tiles (2 workgroups per CU = 512 slots): a grid that leaves slots empty is bound by the LDS fill rate of the CUs
  // that have a workgroup -- more workgroups pulling is the lever.  Cut K so that tiles x slices approaches 512, keeping at
  // least 16 K-steps (K = 1024) per slice: <= 128 tiles -> 2 slices (4 when K >= 6144), and -- round 2, measured on the
  // K = 5120 weight gradients of the d = 1024 and d = 2048 models (profiles/r02_gemm_ek100_shapes.txt: 3072x1024x5120
  // 70 -> 49 us, 4096x1024x5120 74 -> 54 us, 1024x1024x5120 39 -> 30 us) -- <= 256 tiles with K >= 4096 -> 2 slices,
  // <= 64 tiles with K >= 4096 -> 4.
  const int64_t t1 = (int64_t)((M + 127) / 128) * ((N + 127) / 128);
  int s = 1;
  if (t.splitk_mode == 1) {
    if (t1 <= 128 && nk >= 32) s = (nk >= 96 && t1 * 4 <= 512) ? 4 : 2;
    if (t1 <= 64 && nk >= 64) s = 4;
    if (t1 > 128 && t1 <= 256 && nk >= 64) s = 2;
  }
  else if (t1 * t.splitk_mode <= kMaxSplitTiles && nk >= 2 * t.splitk_mode) s = t.splitk_mode;
  while (s > 1 && nk % s != 0) s >>= 1;
  return (s > 1 && t1 <= kMaxSplitTiles) ? s : 1;
}

// bytes of partial tiles (without the counter header) `slices` K-slices of this problem park in the workspace
inline int64_t splitk_bytes(int M, int N, int slices) {
  const int64_t tiles = (int64_t)((M + 127) / 128) * ((N + 127) / 128);
  return tiles * slices * 128 * 128 * (int64_t)sizeof(float);
}

inline GemmPlan plan_gemm(const GemmProblem& p, const GemmTuning& t) {
  GemmPlan plan = {};
  plan.x3 = p.split3 == 4 ? 2 : p.split3;
  plan.K = p.split3 == 3 ? p.K + p.K / 2 : p.split3 == 2 ? 2 * p.K : p.split3 == 1 ? 3 * p.K : p.K;      // in 64-wide K-tiles of 128 B per row
  plan.splitk = 1;
  const int K = plan.K;
  if (!p.a_ks && !p.b_ks && p.b_packed && !p.split3 && t.variant == 0 && bd_packed_wins(p.M, p.N, K, t)) {
    plan.kernel = 10;
    plan.b_from_packed = true;
    return plan;
  }
  const int variant = choose_variant(p.M, p.N, p.a_ks, p.b_ks, t);
  if (p.split3 == 3) {     // fp16 hi pass + fp8 lo pass: NT on the 256x256 kernel (callers ask afft_gemm_lo8_ok first)
    if (p.a_ks || p.b_ks || variant != 3) plan.refusal = "afft_gemm: split3 = 3 needs the NT layout and a problem the 256x256 kernel takes (afft_gemm_lo8_ok)";
    else plan.kernel = pp_kernel(p, 3, K);
    return plan;
  }
  if ((p.split3 == 2 || p.split3 == 4) && p.a_ks) {     // fp16 two-pass / one pass (K = one segment): forward layouts only, same tile choice as bf16x3
    plan.refusal = "afft_gemm: the fp16 two-pass mode (split3 = 2) is built for the forward layouts only (A k-contiguous)";
    return plan;
  }
  if (variant == 3) {     // 256x256 tiles never split K
    plan.kernel = pp_kernel(p, plan.x3, K);
    return plan;
  }
  if (p.split3 == 1) {     // bf16x3: 256x256 tiles once the grid fills the chip, else 128x128; no split-K
    plan.kernel = 1;
    return plan;
  }
  // plain bf16, and the fp16 forward GEMMs on small grids (the predictor's M = B*T rows): split-K -- over the 2K-long loop of the
  // two-pass form: with two slices one workgroup runs the hi pass of a tile and another its lo pass, and the last to arrive adds
  // them (slice order: bitwise repeatable) -- if the workspace offered holds the partial tiles, else: run unsplit
  const int s = variant >= 4 ? 1 : choose_splitk(variant, p.M, p.N, K, t);
  if (s > 1 && p.ws_bytes >= splitk_bytes(p.M, p.N, s) + AFFT_GEMM_WS_HEADER) plan.splitk = s;
  if (p.split3 || variant < 4) plan.kernel = g128_kernel(p, plan.x3, K, plan.splitk);      // the fp16 modes know two tiles: 256x256 and this one
  else plan.kernel = variant;      // 4 (128x128, 4 stages), 7-10 (B-direct), 11 (four quadrants)
  return plan;
}

}  // namespace afft_gemm_detail
