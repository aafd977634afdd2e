// Device helpers shared by the three attention files (attention.hip, attention_mfma.hip, attention_long.hip): the in-register mask
// rule and the swizzled bf16 operand tiles of the MFMA kernels.  One copy: a new mask kind or tile layout is written here.
#pragma once
#include "common.h"

// the reference's masks on a pair (query i, key j) of one sequence; period: AFFT_MASK_BLOCKCAUSAL only (T-SA-Fuser: causal T x T tiled)
__device__ __forceinline__ bool masked(int mask, int period, int i, int j) {
  return (mask == AFFT_MASK_DIAG && i == j) || (mask == AFFT_MASK_CAUSAL && j > i) ||
         (mask == AFFT_MASK_BLOCKCAUSAL && (j % period) > (i % period));
}

// LDS tile [R][hd] bf16; 32-byte unit u of row r is stored at unit u ^ (r & 7): conflict-free transposed reads,
// 2-way (harmless here) ds_read_b128 row reads.
__device__ __forceinline__ int swz(int row, int row_bytes) {   // XOR stays inside the row: rows hold n = row_bytes/32 units, and only the
  const int n = row_bytes >> 5;                                //   bits below n's lowest set bit may flip (n = 6, the 96-channel slices of
  return row & 7 & ((n & -n) - 1);                             //   hd = 384: bit 0 alone; n - 1 = 5 sent units 2, 3 into the next row)
}
__device__ __forceinline__ int tile_off(int row, int chunk16, int row_bytes) {
  return row * row_bytes + ((chunk16 ^ (swz(row, row_bytes) << 1)) << 4);
}

// stages columns [0, hd) of rows row0 .. row0 + R of src (the caller offsets src to the head and head-dimension chunk); rows >=
// rows_valid are staged as zeros, never read
__device__ __forceinline__ void load_tile(const bf16_t* __restrict__ src, int64_t ld, int64_t row0, int rows_valid,
                                          int R, int hd, char* lds) {
  const int cpr = hd >> 3;  // 16-byte chunks per row
  for (int idx = threadIdx.x; idx < R * cpr; idx += 256) {
    const int row = idx / cpr, ch = idx - row * cpr;
    uint4 val = make_uint4(0u, 0u, 0u, 0u);
    if (row < rows_valid) val = *(const uint4*)(src + (row0 + row) * ld + ch * 8);
    *(uint4*)(lds + tile_off(row, ch, hd * 2)) = val;
  }
}

__device__ __forceinline__ bf16x8 row_frag(const char* lds, int row, int chunk16, int row_bytes) {
  return *(const bf16x8*)(lds + tile_off(row, chunk16, row_bytes));
}
// A operand of 16x16x16 for X^T: lane (g, i) gets tile[row0 + 4g + j][16*cb + i], j = 0..3
__device__ __forceinline__ bf16x4 tr_frag(const char* lds, int row0, int cb, int lane, int row_bytes) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int r = row0 + 4 * g + q;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (AFFT_LDS bf16x4*)(lds + r * row_bytes + ((cb ^ swz(r, row_bytes)) << 5) + p * 8));
}
__device__ __forceinline__ void store_o4(bf16_t* dst, const f32x4& a) {
  uint2 u;
  u.x = (unsigned)f2bf(a[0]) | ((unsigned)f2bf(a[1]) << 16);
  u.y = (unsigned)f2bf(a[2]) | ((unsigned)f2bf(a[3]) << 16);
  *(uint2*)dst = u;
}
