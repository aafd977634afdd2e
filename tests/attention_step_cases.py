"""The case table of the kernels of csrc/attention_step.hip -- the cached attention step: causal attention of Lq new rows against a key /
value cache and the append of those rows.  Its 14 instantiations are attn_step_kernel<Dense<float> | Dense<bf16_t>, V, DROP> (8),
attn_step_kernel<Planes, V, false> (2) and attn_step_bwd_kernel<float | bf16_t, V> (4).  Shared by test_attention_step_cases_gpu.py,
which runs every case elementwise against float64 (attention_step_double.py), and test_attention_step_coverage_cpu.py, which checks that
the table reaches every instantiation, every column chunk and every row / key geometry class at least twice.  Plain data: importable
without a device and without the library.

entry:    fwd        afft_attention_step_fwd
          fwd_drop   afft_attention_step_fwd_drop (drop_p = 0: the plan gives DROP = false, and the bits of `fwd`, which the case also runs)
          bwd        the forward (with drop_p > 0: the _drop entry point), then afft_attention_step_bwd on the caches the forward left
          split      afft_attention_step_fwd_split: fp16 planes in and out, fp32 caches
storage:  f32, bf16 (Dense), planes
Lk = past + Lq; cap >= Lk rows per sequence in every cache.
pad_in / pad_c / pad_g: frame columns to the right of the operands and results / of the key and value caches / of the gradient caches.
          Multiples of 8 keep every pitch on the 16-byte grid; with `odd` they are ignored and every pitch is odd (frame_cols()): no
          16-byte access is possible and the plan gives V = false whatever hd is.
xseq / xseq_g: rows between one sequence's `cap` cache rows and the next sequence's: cache_seq = (cap + xseq) * ldc, grad_seq alike.
drop_p, key: attention-probability dropout (0: none).
in_lo / out_lo / probs: split only -- is there a lo plane behind q / k_new / v_new, behind out, and is probs asked for.

A lane owns columns (lane + 64 t) N .. + N with N = 4 (f32) or 8 (bf16, planes) and t < NT = 1024 / (64 N): chunks() lists the t a case
runs, last_chunk() is NT - 1."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

STEP_QT = 4      # query rows of one workgroup (csrc/attn_plan.h)
P = 0.3
KEY = 12345
ENTRIES = ("fwd", "fwd_drop", "bwd", "split")
STORAGES = ("f32", "bf16", "planes")
LK_BOUNDARIES = (1, 63, 64, 65, 127, 128, 129, 512)
# (in_lo given, out_lo given, probs given): the forms of test_attention_step_split_gpu.py
FORMS = ((True, True, True), (False, True, True), (True, False, True), (False, False, True), (True, True, False))


@dataclass(frozen=True)
class StepCase:
    name: str
    entry: str
    storage: str
    nseq: int
    H: int
    hd: int
    Lq: int
    past: int
    cap: int
    pad_in: int = 8
    pad_c: int = 8
    pad_g: int = 8
    xseq: int = 0
    xseq_g: int = 0
    odd: bool = False
    drop_p: float = 0.0
    key: int = KEY
    in_lo: bool = True
    out_lo: bool = True
    probs: bool = True

    @property
    def Lk(self) -> int:
        return self.past + self.Lq

    @property
    def d(self) -> int:
        return self.H * self.hd

    @property
    def vec(self) -> int:
        """elements of one 16-byte access of the storage's operands"""
        return 4 if self.storage == "f32" else 8

    @property
    def V(self) -> bool:
        """the rule test_attention_step_cpu.py::expected states: the pitches allow 16-byte accesses and hd is a multiple of them"""
        return not self.odd and self.hd % self.vec == 0

    @property
    def DROP(self) -> bool:
        return self.drop_p > 0

    @property
    def ntiles(self) -> int:
        return (self.Lq + STEP_QT - 1) // STEP_QT

    def frame_cols(self, pad: int) -> int:
        """frame columns to the right of a buffer of H * hd columns"""
        if self.odd:
            return 1 if self.d % 2 == 0 else 2
        return pad

    def last_chunk(self) -> int:
        return 1024 // (64 * self.vec) - 1

    def chunks(self) -> Tuple[int, ...]:
        """the column chunks t in which some lane has c = (lane + 64 t) N < hd"""
        per = 64 * self.vec
        return tuple(range((self.hd + per - 1) // per))

    def instantiations(self) -> Tuple[Tuple[str, str, bool, bool], ...]:
        """(kernel, storage, V, DROP) of every kernel the case launches: "fwd" attn_step_kernel<Dense<T>, V, DROP>, "planes"
        attn_step_kernel<Planes, V, false>, "bwd" attn_step_bwd_kernel<T, V> (DROP is no template parameter there: False)"""
        if self.entry == "split":
            return (("planes", "planes", self.V, False),)
        ks = [("fwd", self.storage, self.V, self.DROP)]
        if self.entry == "bwd":
            ks.append(("bwd", self.storage, self.V, False))
        return tuple(ks)

    def lds(self, bwd: bool) -> int:
        """plan_attention_step's LDS bytes"""
        rows = min(self.Lq, STEP_QT)
        return 4 * (rows * ((self.Lk + 3) // 4 * 4 + 3 * ((self.hd + 7) // 8 * 8)) + (self.Lq if bwd else 0))


ALL_INSTANTIATIONS = tuple([("fwd", s, v, dr) for s in ("f32", "bf16") for v in (True, False) for dr in (False, True)]
                           + [("planes", "planes", v, False) for v in (True, False)]
                           + [("bwd", s, v, False) for s in ("f32", "bf16") for v in (True, False)])
assert len(ALL_INSTANTIATIONS) == 14


def case(name, entry, storage, nseq, H, hd, Lq, past, cap=None, **kw):
    """cap: None = Lk (the cache is full after the append)"""
    return StepCase(name, entry, storage, nseq, H, hd, Lq, past, past + Lq if cap is None else cap, **kw)


PITCH = dict(pad_in=16, pad_c=24, pad_g=40, xseq=3, xseq_g=5)      # pad columns everywhere, ldg != ldc, grad_seq != cache_seq > cap * ldc

_DENSE = [
    # ---- fp32 (N = 4, 256 columns per chunk, NT = 4).  Vector path: the smallest hd; one lane short of chunk 0 (252); one lane into
    # t = 1 (260); the last lane in t = 2 (520: lane 129); t = 3 full (1024).  Element path: tails inside t = 3 (1021, 1023), hd = 1, an
    # aligned hd on an odd pitch.  Lk walks 1, 63, 64, 65, 127, 128, 129, 512; Lq 1, 3, 5, 9, 4, 6, 7, 16, 8
    case("f_hd4_Lq1_Lk1", "bwd", "f32", 3, 2, 4, 1, 0),
    case("f_hd252_Lq3_Lk63_drop", "bwd", "f32", 2, 2, 252, 3, 60, 70, drop_p=P),
    case("f_hd260_Lq5_Lk64_drop", "bwd", "f32", 2, 2, 260, 5, 59, drop_p=P),
    case("f_hd520_Lq9_Lk65_pitch", "bwd", "f32", 2, 2, 520, 9, 56, 66, **PITCH),
    case("f_hd1024_Lq4_Lk127", "bwd", "f32", 1, 2, 1024, 4, 123, 128),
    case("f_hd1021_Lq6_Lk128", "bwd", "f32", 1, 2, 1021, 6, 122),
    case("f_hd1023_Lq7_Lk129_drop", "bwd", "f32", 1, 2, 1023, 7, 122, 131, drop_p=P),
    case("f_hd1_Lq16_Lk18_drop", "bwd", "f32", 2, 3, 1, 16, 2, 19, drop_p=P),
    case("f_hd64_odd_Lq8_Lk10_pitch", "bwd", "f32", 2, 3, 64, 8, 2, 12, odd=True, xseq=2, xseq_g=1),
    case("f_hd1024_Lq1_Lk512", "bwd", "f32", 1, 1, 1024, 1, 511),
    case("f_hd12_Lq5_prefill_drop0", "fwd_drop", "f32", 2, 2, 12, 5, 0, 7),
    case("f_hd8_Lq13_prefill_drop_pitch", "fwd_drop", "f32", 2, 2, 8, 13, 0, 14, drop_p=P, **PITCH),
    case("f_hd10_Lq37_prefill", "fwd", "f32", 1, 3, 10, 37, 0),
    # ---- bf16 (N = 8, 512 columns per chunk, NT = 2).  Vector path: 8; one lane short of chunk 0 (504); one lane into t = 1 (520); t = 1
    # full (1024).  Element path: 1021, 1023, 1, 64 on an odd pitch.  H * hd = 72 is off every power of two
    case("b_hd8_Lq1_Lk1", "bwd", "bf16", 3, 2, 8, 1, 0, 2),
    case("b_hd504_Lq4_Lk63_drop", "bwd", "bf16", 2, 2, 504, 4, 59, drop_p=P),
    case("b_hd520_Lq3_Lk65_pitch", "bwd", "bf16", 2, 2, 520, 3, 62, 67, **PITCH),
    case("b_hd1024_Lq9_Lk64_drop", "bwd", "bf16", 1, 2, 1024, 9, 55, drop_p=P),
    case("b_hd1021_Lq5_Lk129", "bwd", "bf16", 1, 2, 1021, 5, 124, 130),
    case("b_hd1023_Lq11_Lk127_drop", "bwd", "bf16", 1, 2, 1023, 11, 116, drop_p=P),
    case("b_hd1_Lq10_prefill_drop", "bwd", "bf16", 2, 3, 1, 10, 0, 11, drop_p=P),
    case("b_hd64_odd_Lq6_Lk128_pitch", "bwd", "bf16", 2, 2, 64, 6, 122, 129, odd=True, xseq=1, xseq_g=2),
    case("b_hd24_H3_Lq5_Lk18", "bwd", "bf16", 2, 3, 24, 5, 13, 20),
    case("b_hd1024_Lq3_Lk512", "bwd", "bf16", 1, 1, 1024, 3, 509),
    case("b_hd40_Lq6_prefill_drop0", "fwd_drop", "bf16", 2, 2, 40, 6, 0),
    case("b_hd16_Lq9_Lk12_drop_pitch", "fwd_drop", "bf16", 2, 2, 16, 9, 3, 13, drop_p=P, **PITCH),
    case("b_hd3_Lq4_Lk7", "fwd", "bf16", 2, 3, 3, 4, 3, 9),
]

# ---- planes (N = 8, NT = 2): the five forms on 8, 504 (one lane short of chunk 0), 520 (one lane into t = 1), 1024 and 1021 on an odd
# pitch (the element path's tail inside t = 1); 64 on an odd pitch and hd = 1 in the full form
_WIDTHS = [("p_hd8_Lq1_Lk1", 3, 2, 8, 1, 0, 3, {}),
           ("p_hd504_Lq9_Lk64", 2, 2, 504, 9, 55, 64, {}),
           ("p_hd520_Lq5_Lk65_pitch", 2, 2, 520, 5, 60, 66, dict(pad_in=16, pad_c=24, xseq=3)),
           ("p_hd1024_Lq4_Lk129", 1, 2, 1024, 4, 125, 130, {}),
           ("p_hd1021_odd_Lq6_Lk63", 1, 2, 1021, 6, 57, 63, dict(odd=True, xseq=1))]
_PLANES = [case("%s_in%d_out%d_probs%d" % ((name,) + tuple(map(int, f))), "split", "planes", nseq, H, hd, Lq, past, cap,
                in_lo=f[0], out_lo=f[1], probs=f[2], **kw)
           for name, nseq, H, hd, Lq, past, cap, kw in _WIDTHS for f in FORMS]
_PLANES += [case("p_hd64_odd_Lq7_Lk10", "split", "planes", 2, 3, 64, 7, 3, 12, odd=True),
            case("p_hd1_Lq3_prefill", "split", "planes", 3, 2, 1, 3, 0, 4),
            case("p_hd24_Lq1_Lk512", "split", "planes", 1, 2, 24, 1, 511)]

CASES = _DENSE + _PLANES

assert len({c.name for c in CASES}) == len(CASES), "case names must be unique"
