"""The short-attention case table (L <= 128: afft_attention_fwd / afft_attention_bwd / afft_attention_fwd_split) shared by
test_attention_short_gpu.py, which runs every case elementwise against float64, and test_attention_coverage_cpu.py, which checks that
every `attn_(fwd|bwd)(_mfma|_sliced)?_kernel<...>` instantiation the library compiles is the kernel of at least one case and that the
dispatch plan (csrc/attn_plan.h) answers, for every case, the kernels the case is written for -- written the way `nm -C` prints them.

entry:   fwd_bwd   afft_attention_fwd, then afft_attention_bwd (storage f32 / bf16)
         split     afft_attention_fwd_split: fp16 planes in and out (storage f16x2: hi + lo planes, PL = 1; f16x1: the hi plane alone,
                   in_lo = 0, PL = 2), no backward
mask:    0 none, 1 diagonal, 2 causal, 3 block-causal with `period` (include/afft_hip.h: AFFT_MASK_*)
drop_p:  0 = no dropout
align:   how the GPU test lays the operands out, every one inside a NaN (inputs) or sentinel (results) frame of two rows above and below
         a16   8 frame columns: every pitch a multiple of 8 elements, every base 16-byte aligned
         a8    inputs as a16; out, dq, dk, dv with 4 frame columns: pitch % 4 == 0 but % 8 != 0, which the column-sliced backward refuses
               (attn_bwd_mfma_kernel runs where the aligned problem would be sliced)
         odd   one frame column on an even width: every pitch odd, no 16-byte load possible -- bf16 falls to the generic kernels
fwd/bwd: the kernels the case is written for
hc, hc_bwd, G: MFMA cases -- the head-dimension chunk staged in LDS (forward, backward; == hd: the whole head) and the number of
         sequences packed into the 16 NT rows of a workgroup
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

NONE, DIAG, CAUSAL, BLOCK = 0, 1, 2, 3
FWD, BWD = 0, 1                                                   # afft_attention_plan_for directions
GENERIC, MFMA_FWD, MFMA_BWD, SLICED_BWD = 1, 2, 3, 4              # its families (csrc/attn_plan.h: AttnFamily)
_CTYPE = {"f32": "float", "bf16": "unsigned short"}               # the element type of the generic kernels as nm -C prints it


@dataclass(frozen=True)
class AttnCase:
    name: str
    entry: str
    storage: str
    nseq: int
    L: int
    H: int
    hd: int
    mask: int
    period: int
    drop_p: float
    align: str
    fwd: str
    bwd: Optional[str]
    hc: int = 0
    hc_bwd: int = 0
    G: int = 0

    @property
    def mfma(self) -> bool:
        return "_mfma_" in self.fwd


def gen(name, storage, LM, nseq, L, H, hd, mask=NONE, period=0, p=0.0, align="a16"):
    """a case of the generic kernels attn_fwd_kernel / attn_bwd_kernel<T, LM>"""
    t = _CTYPE[storage]
    return AttnCase(name, "fwd_bwd", storage, nseq, L, H, hd, mask, period, p, align, f"attn_fwd_kernel<{t}, {LM}>", f"attn_bwd_kernel<{t}, {LM}>")


def mfma(name, NT, bwd, nseq, L, H, hd, G, hc=0, hc_bwd=0, mask=NONE, period=0, p=0.0, align="a16"):
    """a bf16 case of attn_fwd_mfma_kernel<NT, 0> and, bwd = "mfma" / "sliced", attn_bwd_mfma_kernel<NT> / attn_bwd_sliced_kernel<NT>"""
    return AttnCase(name, "fwd_bwd", "bf16", nseq, L, H, hd, mask, period, p, align, f"attn_fwd_mfma_kernel<{NT}, 0>",
                    f"attn_bwd_{bwd}_kernel<{NT}>", hc or hd, hc_bwd or hd, G)


def split(name, PL, NT, nseq, L, H, hd, G, hc=0, mask=NONE, period=0, p=0.0):
    """a case of the fp16x2 forward attn_fwd_mfma_kernel<NT, PL>: PL = 1 two planes an operand, PL = 2 one"""
    return AttnCase(name, "split", "f16x2" if PL == 1 else "f16x1", nseq, L, H, hd, mask, period, p, "a16", f"attn_fwd_mfma_kernel<{NT}, {PL}>",
                    None, hc or hd, 0, G)


P = 0.3

CASES = [
    # ---- generic kernels, fp32: every L at which LM changes (32 | 33, 64 | 65, 128), L = 1, 2 (one key under the diagonal mask), hd = 1, 24,
    # 65 (second 64-lane stride of the score loop), 257 (second pass of the c += 256 loops), 1024 (all NQ = 16 registers of a lane)
    gen("g_f32_L1_odd", "f32", 32, 3, 1, 2, 24, align="odd"),
    gen("g_f32_L2_hd1024", "f32", 32, 2, 2, 1, 1024),
    gen("g_f32_L5_H3_causal_drop", "f32", 32, 3, 5, 3, 65, CAUSAL, p=P),
    gen("g_f32_L31_hd1", "f32", 32, 2, 31, 1, 1),
    gen("g_f32_L32_hd257_bc8", "f32", 32, 1, 32, 2, 257, BLOCK, 8),
    gen("g_f32_L33_diag_drop", "f32", 64, 2, 33, 1, 65, DIAG, p=P),
    gen("g_f32_L64_H3_bc16", "f32", 64, 1, 64, 3, 24, BLOCK, 16),
    gen("g_f32_L65", "f32", 128, 2, 65, 1, 24),
    gen("g_f32_L127_hd1_causal_odd", "f32", 128, 1, 127, 2, 1, CAUSAL, align="odd"),
    gen("g_f32_L128_hd257_bc32_drop", "f32", 128, 1, 128, 2, 257, BLOCK, 32, p=P),
    # ---- generic kernels, bf16: by hd % 64 != 0, by L > 64, and -- odd -- by operands no 16-byte load can take at hd = 64 and 1024
    gen("g_bf16_L1", "bf16", 32, 17, 1, 2, 24),
    gen("g_bf16_L2_hd1024_causal_odd", "bf16", 32, 2, 2, 1, 1024, CAUSAL, align="odd"),
    gen("g_bf16_L5_H3_hd64_odd_drop", "bf16", 32, 4, 5, 3, 64, p=P, align="odd"),
    gen("g_bf16_L31_diag", "bf16", 32, 2, 31, 2, 65, DIAG),
    gen("g_bf16_L32_hd1_bc4", "bf16", 32, 2, 32, 1, 1, BLOCK, 4),
    gen("g_bf16_L33_hd257", "bf16", 64, 1, 33, 2, 257),
    gen("g_bf16_L64_hd64_odd_causal_drop", "bf16", 64, 2, 64, 1, 64, CAUSAL, p=P, align="odd"),
    gen("g_bf16_L65_H3_diag", "bf16", 128, 1, 65, 3, 24, DIAG),
    gen("g_bf16_L127_hd64_causal_drop", "bf16", 128, 2, 127, 1, 64, CAUSAL, p=P),
    gen("g_bf16_L128_bc16", "bf16", 128, 1, 128, 2, 65, BLOCK, 16),
    # ---- MFMA forward (PL = 0) with the two MFMA backward kernels.  NT = 1: sequences packed into one 16-row tile
    mfma("m1_L1_G16_last_group_of_one", 1, "mfma", 17, 1, 2, 64, G=16),
    mfma("m1_L2_diag_hd192", 1, "mfma", 3, 2, 2, 192, G=8, mask=DIAG),
    mfma("m1_L3_H3_causal_drop", 1, "mfma", 7, 3, 3, 64, G=5, mask=CAUSAL, p=P),
    mfma("m1_L5_one_sequence_sliced128", 1, "sliced", 1, 5, 2, 128, G=3),
    mfma("m1_L5_ragged_group_drop", 1, "mfma", 4, 5, 2, 64, G=3, p=P),
    mfma("m1_L5_ragged_sliced512_bcL_drop", 1, "sliced", 4, 5, 2, 512, G=3, mask=BLOCK, period=5, p=P),
    mfma("m1_L8_hd320_bc1_drop", 1, "mfma", 3, 8, 2, 320, G=2, mask=BLOCK, period=1, p=P),
    mfma("m1_L9_dead_rows_hd1024_whole", 1, "mfma", 2, 9, 1, 1024, G=1, mask=CAUSAL),          # backward: 4 tiles of 32 KiB = 128 KiB
    mfma("m1_L16_hd128_a8_bc4", 1, "mfma", 2, 16, 1, 128, G=1, mask=BLOCK, period=4, align="a8"),
    # NT = 2
    mfma("m2_L17_causal_drop", 2, "mfma", 2, 17, 1, 64, G=1, mask=CAUSAL, p=P),
    mfma("m2_L17_sliced384", 2, "sliced", 2, 17, 1, 384, G=1),
    mfma("m2_L31_hd640_lds_160k", 2, "mfma", 1, 31, 2, 640, G=1),                              # backward: 4 * 32 * 640 * 2 = 163840 bytes
    mfma("m2_L31_sliced512_causal_drop", 2, "sliced", 1, 31, 2, 512, G=1, mask=CAUSAL, p=P),
    mfma("m2_L32_hd1024_chunks_diag", 2, "mfma", 1, 32, 2, 1024, G=1, hc=512, hc_bwd=512, mask=DIAG),
    mfma("m2_L32_H3_sliced128_bcL", 2, "sliced", 1, 32, 3, 128, G=1, mask=BLOCK, period=32),
    mfma("m2_L32_hd256_a8_bc8_drop", 2, "mfma", 2, 32, 1, 256, G=1, mask=BLOCK, period=8, p=P, align="a8"),
    # NT = 4
    mfma("m4_L33_causal_drop", 4, "mfma", 2, 33, 1, 64, G=1, mask=CAUSAL, p=P),
    mfma("m4_L33_hd1024_chunks_bc1", 4, "mfma", 1, 33, 2, 1024, G=1, hc=512, hc_bwd=256, mask=BLOCK, period=1),
    mfma("m4_L49_hd320_lds_160k_bc7", 4, "mfma", 1, 49, 2, 320, G=1, mask=BLOCK, period=7),    # backward: 4 * 64 * 320 * 2 = 163840 bytes
    mfma("m4_L64_hd512_chunks", 4, "mfma", 1, 64, 2, 512, G=1, hc=256, hc_bwd=256),
    mfma("m4_L64_hd768_chunks384_diag", 4, "mfma", 2, 64, 1, 768, G=1, hc=384, hc_bwd=384, mask=DIAG),
    mfma("m4_L64_H3_hd192_bcL", 4, "mfma", 1, 64, 3, 192, G=1, mask=BLOCK, period=64),
    # ---- the fp16x2 forward: two planes an operand (PL = 1) and the hi plane alone (PL = 2, in_lo = 0), 48 KiB of LDS
    split("s1_L5_ragged_group_drop", 1, 1, 4, 5, 2, 64, G=3, p=P),
    split("s1_L16_diag", 1, 1, 2, 16, 1, 64, G=1, mask=DIAG),
    split("s1_L17_causal_drop", 1, 2, 1, 17, 2, 64, G=1, mask=CAUSAL, p=P),
    split("s1_L33_bc11", 1, 4, 2, 33, 1, 64, G=1, mask=BLOCK, period=11),
    split("s1_L64_H3_drop", 1, 4, 1, 64, 3, 64, G=1, p=P),
    split("s1_L64_hd128_chunks_causal", 1, 4, 1, 64, 2, 128, G=1, hc=64, mask=CAUSAL),
    split("s2_L5_ragged_group_causal_drop", 2, 1, 4, 5, 2, 64, G=3, mask=CAUSAL, p=P),
    split("s2_L16_H3_bc4", 2, 1, 1, 16, 3, 64, G=1, mask=BLOCK, period=4),
    split("s2_L17_drop", 2, 2, 2, 17, 1, 64, G=1, p=P),
    split("s2_L17_hd512_chunks_diag", 2, 2, 1, 17, 2, 512, G=1, hc=256, mask=DIAG),
    split("s2_L33_diag", 2, 4, 1, 33, 2, 64, G=1, mask=DIAG),
    split("s2_L64_bcL_drop", 2, 4, 2, 64, 1, 64, G=1, mask=BLOCK, period=64, p=P),
]

assert len({c.name for c in CASES}) == len(CASES), "case names must be unique"


def plan_query(c: AttnCase, direction: int, aligned: Optional[bool] = None):
    """the arguments of afft_attention_plan_for(direction, dtype, L, hd, planes, in_lo, pitch_alignment_ok) that describe case c.  The
    query knows aligned rows and rows no 16-byte load can take; an a8 case asks as aligned (what it would run without its gradient pitches).
    `aligned` overrides the case's own mode."""
    from afft_amd import _lib
    dtype = {"f32": _lib.F32, "bf16": _lib.BF16, "f16x2": _lib.F16, "f16x1": _lib.F16}[c.storage]
    ok = (c.align != "odd") if aligned is None else aligned
    return direction, dtype, c.L, c.hd, int(c.entry == "split"), int(c.storage == "f16x2"), int(ok)


def frame_cols(c: AttnCase, result: bool, width: int) -> int:
    """frame columns to the right of an operand (result = False) or of out / dq / dk / dv (True) of `width` columns"""
    if c.align == "odd":
        return 1 if width % 2 == 0 else 2
    return 4 if c.align == "a8" and result else 8
