"""The case table of the kernels of csrc/attention_long.hip -- long_fwd_kernel, long_bwd_q_kernel, long_bwd_kv_kernel and
bias_bwd_ds_kernel, each as <float, false>, <bf16, false> and <bf16, true>, and bias_bwd_reduce_kernel -- shared by
test_attention_long_cases_gpu.py, which runs every case elementwise against float64, and test_attention_long_coverage_cpu.py, which
checks that every instantiation the library compiles is the kernel of at least one case, that the dispatch plan (csrc/attn_plan.h)
answers the family every case is written for, and that the table keeps the shapes listed below.

entry:   fwd_bwd   afft_attention_long_fwd (mask kind and, bias = "table", the additive [L, L] table), then afft_attention_long_bwd; 129 <= L <= 512
         bias      the forward with an additive bias of shape kind `bias` (afft_attention_long_fwd_bias; L <= 128: afft_attention_fwd_bias,
                   a short kernel that only supplies the probabilities), afft_attention_bias_bwd at every L from 1, and, L > 128,
                   afft_attention_long_bwd
storage: f32, bf16
mask:    0 none, 1 diagonal, 2 causal, 3 block-causal with `period` (include/afft_hip.h: AFFT_MASK_*); the bias entry has none
bias:    none | table (L, L) | pad (nseq, 1, 1, L) | head (1, H, L, L) | sample (nseq, 1, L, L) | full (nseq, H, L, L); about 20 % of a
         table or bias is -inf, column 0 stays finite
drop_p:  0 = no dropout
align:   every operand inside a NaN (inputs) or sentinel (results) frame of two rows above and below
         a16   8 frame columns: every pitch a multiple of 8 elements, every base 16-byte aligned
         a4    inputs as a16; out, dq, dk, dv with 4 frame columns: pitches = 4 mod 8, 8-byte stores at 8-byte alignment -- stays on MFMA
         odd   every pitch odd: no 16-byte load possible, bf16 falls to the generic form
family:  the form of the kernels: f32 <float, false>, bf16 <unsigned short, false>, mfma <unsigned short, true>
kernels: the instantiations the case is written for, as `nm -C` prints them
hc, Lp, ntiles: MFMA cases -- the head-dimension chunk staged in LDS (256 / 128 / 64: the largest that divides hd), L rounded up to 64,
         tiles of 32 rows
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from attention_cases import BLOCK, CAUSAL, DIAG, NONE

FWD, BWD, BIAS = 0, 1, 2                                          # afft_attention_plan_for directions
LONG_F32, BIAS_F32 = 5, 8                                         # its families (csrc/attn_plan.h: AttnFamily): + 0 f32, + 1 bf16, + 2 MFMA
FORMS = ("f32", "bf16", "mfma")
_TARGS = {"f32": "float, false", "bf16": "unsigned short, false", "mfma": "unsigned short, true"}
LONG_KERNELS = ("long_fwd_kernel", "long_bwd_q_kernel", "long_bwd_kv_kernel")
REDUCE = "bias_bwd_reduce_kernel"
BIAS_KINDS = ("table", "pad", "head", "sample", "full")
P = 0.3


@dataclass(frozen=True)
class LongCase:
    name: str
    entry: str
    storage: str
    nseq: int
    L: int
    H: int
    hd: int
    mask: int
    period: int
    bias: str
    drop_p: float
    align: str
    family: str
    kernels: Tuple[str, ...]
    hc: int = 0
    Lp: int = 0
    ntiles: int = 0
    key: int = 0x9E3779B9      # the dropout key

    @property
    def mfma(self) -> bool:
        return self.family == "mfma"

    @property
    def long(self) -> bool:
        return self.L > 128

    def bias_shape(self) -> Optional[tuple]:
        n, H, L = self.nseq, self.H, self.L
        return {"none": None, "table": (L, L), "pad": (n, 1, 1, L), "head": (1, H, L, L), "sample": (n, 1, L, L), "full": (n, H, L, L)}[self.bias]

    def reduces(self) -> bool:
        """the bias gradient sums over a dimension the bias broadcasts in (bias_bwd_reduce_kernel runs)"""
        s = self.bias_shape()
        s4 = (1,) * (4 - len(s)) + s
        return any(a == 1 and f > 1 for a, f in zip(s4[:3], (self.nseq, self.H, self.L)))


def _kernels(entry, form, L, reduces):
    ks = []
    if entry == "fwd_bwd" or L > 128:
        ks += [f"{k}<{_TARGS[form]}>" for k in LONG_KERNELS]
    if entry == "bias":
        ks.append(f"bias_bwd_ds_kernel<{_TARGS[form]}>")
        if reduces:
            ks.append(REDUCE)
    return tuple(ks)


def case(name, entry, form, nseq, L, H, hd, mask=NONE, period=0, bias="none", p=0.0, align="a16", hc=0, Lp=0, nt=0, key=0x9E3779B9):
    storage = "f32" if form == "f32" else "bf16"
    c = LongCase(name, entry, storage, nseq, L, H, hd, mask, period, bias, p, align, form, ())
    return LongCase(name, entry, storage, nseq, L, H, hd, mask, period, bias, p, align, form,
                    _kernels(entry, form, L, entry == "bias" and c.reduces()), hc, Lp, nt, key)


def f32(name, *a, **kw):
    return case(name, "fwd_bwd", "f32", *a, **kw)


def b16(name, *a, **kw):
    return case(name, "fwd_bwd", "bf16", *a, **kw)


def mfma(name, nseq, L, H, hd, hc, Lp, nt, **kw):
    return case(name, "fwd_bwd", "mfma", nseq, L, H, hd, hc=hc, Lp=Lp, nt=nt, **kw)


def bias(name, form, kind, nseq, L, H, hd, hc=0, Lp=0, nt=0, **kw):
    return case(name, "bias", form, nseq, L, H, hd, bias=kind, hc=hc, Lp=Lp, nt=nt, **kw)


CASES = [
    # ---- forward and backward, fp32: every column class of matmul_generic (nc = 16, 32, 64, 128, 256 at hd = 1, 17, 33, 65, 129; a second
    # c += 256 pass at 257, four at 1024), L on both sides of every Lp step (192 | 193, 256 | 257, 448 | 449) and one-row last tiles
    f32("f_L129_hd1", 2, 129, 1, 1),
    f32("f_L160_hd17_bc5_drop", 2, 160, 1, 17, BLOCK, 5, p=P),
    f32("f_L192_H3_hd33_causal", 1, 192, 3, 33, CAUSAL),
    f32("f_L193_hd65_diag_drop_odd", 2, 193, 1, 65, DIAG, p=P, align="odd"),
    f32("f_L256_hd129_table", 1, 256, 2, 129, bias="table"),
    f32("f_L257_hd257_bc1", 1, 257, 2, 257, BLOCK, 1),
    f32("f_L320_hd1024_bcL", 1, 320, 2, 1024, BLOCK, 320),
    f32("f_L449_hd65_table_drop", 2, 449, 1, 65, bias="table", p=P),
    f32("f_L511_hd17_diag", 1, 511, 2, 17, DIAG),
    f32("f_L512_hd33_causal_table", 1, 512, 2, 33, CAUSAL, bias="table"),
    # ---- bf16 on the generic form: by hd % 64 != 0 (24, 65) and -- odd -- by operands no 16-byte load can take at hd = 64 and 256
    b16("b_L129_hd24_diag_drop", 2, 129, 1, 24, DIAG, p=P),
    b16("b_L160_hd64_odd_bc5", 2, 160, 1, 64, BLOCK, 5, align="odd"),
    b16("b_L193_hd256_odd_causal", 1, 193, 2, 256, CAUSAL, align="odd"),
    b16("b_L256_H3_hd65_table_drop", 1, 256, 3, 65, bias="table", p=P),
    b16("b_L320_hd24_bcL", 1, 320, 2, 24, BLOCK, 320),
    b16("b_L449_hd65", 2, 449, 1, 65),
    b16("b_L512_hd64_odd_bc1_drop", 1, 512, 2, 64, BLOCK, 1, p=P, align="odd"),
    # ---- bf16 on MFMA: every hc with one chunk (64, 128, 256) and with more (192 = 3 x 64, 320 = 5 x 64, 384 = 3 x 128, 768 = 3 x 256,
    # 1024 = 4 x 256); hd = 1024 at L = 512 is the largest LDS request
    mfma("m_L129_hd64_diag", 2, 129, 1, 64, 64, 192, 5, mask=DIAG),
    mfma("m_L160_hd192_bc5_drop", 1, 160, 2, 192, 64, 192, 5, mask=BLOCK, period=5, p=P),
    mfma("m_L160_hd64_many_tiles_bc40", 18, 160, 3, 64, 64, 192, 5, mask=BLOCK, period=40),      # 54 (sequence, head) pairs x 5 tiles > 256 CUs
    mfma("m_L192_hd384_causal", 1, 192, 2, 384, 128, 192, 6, mask=CAUSAL),
    mfma("m_L193_hd320_drop", 2, 193, 1, 320, 64, 256, 7, p=P),
    mfma("m_L256_H3_hd128_bc1", 1, 256, 3, 128, 128, 256, 8, mask=BLOCK, period=1),
    mfma("m_L257_hd256_a4_table_drop", 1, 257, 2, 256, 256, 320, 9, bias="table", p=P, align="a4"),
    mfma("m_L320_hd768_bcL", 1, 320, 2, 768, 256, 320, 10, mask=BLOCK, period=320),
    mfma("m_L449_hd192_table_diag", 1, 449, 2, 192, 64, 512, 15, mask=DIAG, bias="table"),
    mfma("m_L511_hd64_diag_drop", 2, 511, 1, 64, 64, 512, 16, mask=DIAG, p=P),
    mfma("m_L512_hd1024_table_lds_max", 1, 512, 2, 1024, 256, 512, 16, bias="table"),
    # ---- the bias gradient (every L from 1) behind the forward with that bias: every shape kind with -inf on every form, short and long
    bias("bf_L1_table_hd17", "f32", "table", 3, 1, 2, 17),
    bias("bf_L5_pad_hd1_drop", "f32", "pad", 3, 5, 2, 1, p=P, key=1),      # (the default key drops all five keys of a row)
    bias("bf_L32_head_H3_hd33", "f32", "head", 2, 32, 3, 33),
    bias("bf_L33_sample_hd65_drop_odd", "f32", "sample", 2, 33, 2, 65, p=P, align="odd"),
    bias("bf_L64_full_hd129", "f32", "full", 2, 64, 2, 129),
    bias("bf_L65_table_hd257_drop", "f32", "table", 2, 65, 1, 257, p=P),
    bias("bf_L128_pad_hd1024", "f32", "pad", 2, 128, 1, 1024),
    bias("bf_L129_table_hd65_drop", "f32", "table", 2, 129, 2, 65, p=P),
    bias("bf_L160_full_hd1_drop", "f32", "full", 2, 160, 1, 1, p=P),
    bias("bf_L193_pad_hd17", "f32", "pad", 3, 193, 1, 17),
    bias("bf_L320_head_hd33_drop", "f32", "head", 2, 320, 2, 33, p=P),
    bias("bf_L512_sample_hd129", "f32", "sample", 1, 512, 2, 129),
    bias("bb_L1_pad_hd24", "bf16", "pad", 2, 1, 2, 24),
    bias("bb_L5_table_hd64_odd_drop", "bf16", "table", 2, 5, 1, 64, p=P, align="odd"),
    bias("bb_L32_sample_hd65", "bf16", "sample", 2, 32, 2, 65),
    bias("bb_L64_head_H3_hd24_drop", "bf16", "head", 2, 64, 3, 24, p=P),
    bias("bb_L128_full_hd256_odd", "bf16", "full", 1, 128, 2, 256, align="odd"),
    bias("bb_L129_pad_hd65_drop", "bf16", "pad", 2, 129, 2, 65, p=P),
    bias("bb_L160_full_hd65", "bf16", "full", 2, 160, 1, 65),
    bias("bb_L193_table_hd24", "bf16", "table", 2, 193, 1, 24),
    bias("bb_L320_sample_hd64_odd", "bf16", "sample", 1, 320, 2, 64, align="odd"),
    bias("bb_L512_head_hd24_drop", "bf16", "head", 2, 512, 1, 24, p=P),
    bias("bm_L1_full_hd64", "mfma", "full", 3, 1, 2, 64, 64, 64, 1),
    bias("bm_L5_head_hd192_drop", "mfma", "head", 2, 5, 2, 192, 64, 64, 1, p=P, key=1),
    bias("bm_L33_pad_hd384", "mfma", "pad", 2, 33, 2, 384, 128, 64, 2),
    bias("bm_L64_table_H3_hd128_drop", "mfma", "table", 2, 64, 3, 128, 128, 64, 2, p=P),
    bias("bm_L65_sample_hd320", "mfma", "sample", 2, 65, 2, 320, 64, 128, 3),
    bias("bm_L128_full_hd768", "mfma", "full", 1, 128, 2, 768, 256, 128, 4),
    bias("bm_L129_sample_hd256_drop", "mfma", "sample", 2, 129, 2, 256, 256, 192, 5, p=P),
    bias("bm_L193_full_hd192", "mfma", "full", 2, 193, 1, 192, 64, 256, 7),
    bias("bm_L256_head_hd768", "mfma", "head", 2, 256, 1, 768, 256, 256, 8),
    bias("bm_L320_pad_hd384_drop", "mfma", "pad", 2, 320, 2, 384, 128, 320, 10, p=P),
    bias("bm_L512_table_hd1024", "mfma", "table", 2, 512, 1, 1024, 256, 512, 16),
]

assert len({c.name for c in CASES}) == len(CASES), "case names must be unique"


def make_bias(c: LongCase, seed: int = 5):
    """the additive fp32 table / bias of case c (None: it has none): 0.5 N(0, 1) with about 20 % -inf, never a whole row -- key 0 stays finite"""
    shape = c.bias_shape()
    if shape is None:
        return None
    rng = np.random.RandomState(seed)
    b = (0.5 * rng.standard_normal(shape)).astype(np.float32)
    hide = rng.random_sample(shape) < 0.2
    hide[..., 0] = False
    b[hide] = -np.inf
    return b


def plan_query(c: LongCase, direction: int, aligned: Optional[bool] = None):
    """the arguments of afft_attention_plan_for(direction, dtype, L, hd, planes, in_lo, pitch_alignment_ok) that describe case c.  The
    query knows aligned rows and rows no 16-byte load can take; an a4 case asks as aligned (it stays on MFMA).  `aligned` overrides the
    case's own mode."""
    from afft_amd import _lib
    dtype = _lib.F32 if c.storage == "f32" else _lib.BF16
    ok = (c.align != "odd") if aligned is None else aligned
    return direction, dtype, c.L, c.hd, 0, 0, int(ok)


def frame_cols(c: LongCase, result: bool, width: int) -> int:
    """frame columns to the right of an operand (result = False) or of out / dq / dk / dv (True) of `width` columns"""
    if c.align == "odd":
        return 1 if width % 2 == 0 else 2
    return 4 if c.align == "a4" and result else 8
