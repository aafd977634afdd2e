"""CPU: the case table of the cached attention step (tests/attention_step_cases.py), which the GPU suite runs elementwise against float64
(tests/test_attention_step_cases_gpu.py), reaches everything csrc/attention_step.hip compiles: all 14 instantiations, every column
chunk t < NT of every storage on the vector path and the last chunk on the element path, every Lk % 4 and every Lk boundary in each
direction, every row-tile remainder with at least two tiles in forward and backward -- each by AT LEAST TWO cases, so that the loss of
one case leaves the class covered and the loss of the second-to-last fails here, by name.  A case's instantiation comes from the rule
test_attention_step_cpu.py::expected states (V: the pitches allow 16-byte accesses and hd % vec == 0; DROP: drop_p > 0); that rule is
held against afft_attention_step_plan_for / afft_attention_step_split_plan_for wherever those answer (the forward without dropout,
the planes), with the LDS bytes and the tiles.  No case may be refused by the plan.  No compute call is made."""
import ctypes as C
from collections import Counter

import numpy as np

from attention_step_cases import (ALL_INSTANTIATIONS, CASES, ENTRIES, FORMS, LK_BOUNDARIES, STEP_QT, STORAGES, StepCase)
from attention_step_double import step_banned, step_keep_scale
from test_attention_step_cpu import expected

LDS_MAX = 64 * 1024      # what a workgroup of these kernels may ask for: hd 1024 x Lk 512 x 4 rows is 56 KiB + the backward's row terms


def uncovered(cases, at_least=2):
    """the classes fewer than `at_least` cases of `cases` reach, as sorted strings: what the tests below assert to be empty"""
    n = Counter()

    def reach(*cls):
        n[cls] += 1

    want = set()
    for inst in ALL_INSTANTIATIONS:
        want.add(("instantiation",) + inst)
    for direction, storages in (("fwd", STORAGES), ("bwd", ("f32", "bf16"))):
        for s in storages:
            nt = 4 if s == "f32" else 2
            want |= {("vector chunk", direction, s, t) for t in range(nt)}
            want.add(("element path in the last chunk", direction, s))
        want |= {("Lk % 4", direction, r) for r in range(4)} | {("Lk", direction, L) for L in LK_BOUNDARIES}
        want |= {("Lq % 4 with two tiles or more", direction, r) for r in range(4)}
    for s in STORAGES:
        want |= {("more than two row tiles and a past", s), ("cap == Lk", s), ("cap > Lk", s), ("prefill, Lq % 4 != 0", s)}
    for direction in ("fwd", "bwd"):
        want.add(("dense pitch", direction))
        for s in ("f32", "bf16"):
            want |= {("dropout", direction, s, v) for v in (True, False)}
    want |= {("Lq", q) for q in (1, 3, 4, 5, 9, 16)} | {("planes form", f) for f in FORMS}
    want |= {("fwd_drop at p = 0", s) for s in ("f32", "bf16")}

    for c in cases:
        for inst in c.instantiations():
            reach("instantiation", *inst)
        for direction in ("fwd", "bwd") if c.entry == "bwd" else ("fwd",):
            if c.V:
                for t in c.chunks():
                    reach("vector chunk", direction, c.storage, t)
            elif c.chunks()[-1] == c.last_chunk():
                reach("element path in the last chunk", direction, c.storage)
            reach("Lk % 4", direction, c.Lk % 4)
            reach("Lk", direction, c.Lk)
            if c.ntiles >= 2:
                reach("Lq % 4 with two tiles or more", direction, c.Lq % 4)
            if c.storage != "planes":
                if c.pad_in and c.pad_c and c.xseq and (direction == "fwd" or (c.pad_g != c.pad_c and c.xseq_g != c.xseq)) and not c.odd:
                    reach("dense pitch", direction)
                if c.drop_p > 0:
                    reach("dropout", direction, c.storage, c.V)
        if c.ntiles > 2 and c.past > 0:
            reach("more than two row tiles and a past", c.storage)
        reach("cap == Lk" if c.cap == c.Lk else "cap > Lk", c.storage)
        if c.past == 0 and c.Lq % 4:
            reach("prefill, Lq % 4 != 0", c.storage)
        reach("Lq", c.Lq)
        if c.entry == "split":
            reach("planes form", (c.in_lo, c.out_lo, c.probs))
        if c.entry == "fwd_drop" and c.drop_p == 0:
            reach("fwd_drop at p = 0", c.storage)
    at = {cls: (1 if cls[0] in ("Lq", "fwd_drop at p = 0", "prefill, Lq % 4 != 0", "cap == Lk", "cap > Lk",
                                "more than two row tiles and a past") else at_least) for cls in want}
    return sorted(" ".join(map(str, cls)) for cls in want if n[cls] < at[cls])


def test_case_table_is_well_formed():
    for c in CASES:
        assert isinstance(c, StepCase) and c.entry in ENTRIES and c.storage in STORAGES, c.name
        assert (c.entry == "split") == (c.storage == "planes"), c.name
        assert 1 <= c.Lq <= c.Lk <= 512 and c.Lk <= c.cap and 1 <= c.hd <= 1024, c.name
        assert 1 <= c.nseq * c.H <= 6 and c.nseq * c.H * c.hd * c.Lk <= 1024 * 512 * 2, c.name
        assert c.hd * c.Lk < 1024 * 512 or c.nseq * c.H == 1, c.name      # nothing larger than hd 1024 x Lk 512 on one sequence and head
        assert c.drop_p in (0.0, 0.3) and (c.drop_p == 0 or c.entry in ("fwd_drop", "bwd")), c.name
        assert all(p % 8 == 0 for p in (c.pad_in, c.pad_c, c.pad_g)), c.name
        assert not c.odd or all((c.d + c.frame_cols(p)) % 2 == 1 for p in (c.pad_in, c.pad_c, c.pad_g)), c.name
        assert c.entry == "split" or (c.in_lo and c.out_lo and c.probs), c.name
        assert c.lds(c.entry == "bwd") <= LDS_MAX, c.name
    both = [c for c in CASES if c.nseq > 1 and c.H > 1]
    assert 2 * len(both) > len(CASES), "nseq > 1 and H > 1 together in most cases"
    assert sum(1 for c in CASES if c.d & (c.d - 1)) >= 6, "H * hd off any power of two in some"


def test_table_reaches_every_instantiation_and_geometry_class_twice():
    lost = uncovered(CASES)
    assert not lost, "tests/attention_step_cases.py has too few cases left for: " + "; ".join(lost)


def test_coverage_check_notices_the_loss_of_a_second_to_last_case():
    """the check above is not vacuous: without its two bf16 hd = 1024 cases the bf16 backward has one vector case left in chunk t = 1"""
    assert uncovered([c for c in CASES if c.name != "b_hd24_H3_Lq5_Lk18"]) == []      # (a case no class depends on)
    lost = uncovered([c for c in CASES if not c.name.startswith("b_hd1024")])
    assert "vector chunk bwd bf16 1" in lost, lost
    lost = uncovered([c for c in CASES if c.name not in ("f_hd1024_Lq1_Lk512",)])
    assert "Lk bwd 512" in lost and "Lk fwd 512" not in lost, lost
    assert "instantiation fwd f32 False True" in uncovered([c for c in CASES if c.name != "f_hd1023_Lq7_Lk129_drop"])


def _asked(fn, *args):
    from afft_amd import _lib
    o = (C.c_int64 * 2)()
    r = getattr(_lib.lib(), fn)(*args, o)
    assert r >= 0, (fn, args, _lib.lib().afft_last_error())
    return r // 10000, r % 10000 // 10, r % 10, o[0], o[1]


def test_the_plan_refuses_no_case_and_gives_the_stated_instantiation():
    from afft_amd import _lib
    for c in CASES:
        ok = 0 if c.odd else 1
        if c.entry == "split":
            got = _asked("afft_attention_step_split_plan_for", c.Lq, c.Lk, c.hd, int(c.in_lo), int(c.out_lo), ok)
            assert got == (13, int(c.V), 0, c.lds(False), c.ntiles), (c.name, got)
            continue
        dtype = _lib.F32 if c.storage == "f32" else _lib.BF16
        got = _asked("afft_attention_step_plan_for", dtype, c.Lq, c.Lk, c.hd, ok)      # the forward without dropout
        want = expected(dtype, c.Lq, c.Lk, c.hd, ok)
        assert want is not None and got == (want[0], want[1], 0, want[2], want[3]), (c.name, got, want)
        assert (want[1], want[2], want[3]) == (int(c.V), c.lds(False), c.ntiles), (c.name, want)
        assert c.ntiles == (c.Lq + STEP_QT - 1) // STEP_QT


def test_every_dropout_case_keeps_and_drops_visible_pairs_in_every_head():
    for c in CASES:
        if c.drop_p == 0:
            continue
        visible = np.broadcast_to(~step_banned(c.Lq, c.past), (c.nseq, c.H, c.Lq, c.Lk))
        assert int(visible[0, 0].sum()) >= 32, f"{c.name}: fewer than 32 visible (query, key) pairs per head"
        _, keep = step_keep_scale(c.nseq, c.H, c.Lq, c.Lk, c.drop_p, c.key)
        kept, dropped = (visible & keep).sum((-1, -2)), (visible & ~keep).sum((-1, -2))
        assert bool((kept > 0).all()) and bool((dropped > 0).all()), f"{c.name}: a (sequence, head) keeps or drops every visible pair"
