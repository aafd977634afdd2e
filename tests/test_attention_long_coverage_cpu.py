"""CPU: every instantiation of the kernels of csrc/attention_long.hip the library compiles -- long_fwd_kernel, long_bwd_q_kernel,
long_bwd_kv_kernel, bias_bwd_ds_kernel<T, MFMA> and bias_bwd_reduce_kernel -- is the kernel of at least one case of the shared table
(tests/attention_long_cases.py), which the GPU suite runs elementwise against float64 (tests/test_attention_long_cases_gpu.py).  A
kernel added to the launcher without a case fails here, by name; so does a case whose kernel is not built, and a trim of the table that
drops the only case of a listed shape.  The dispatch plan (csrc/attn_plan.h) is host arithmetic: afft_attention_plan_for answers here
which family every case runs, and hc, Lp, ntiles and the LDS bytes are restated and held against the case's fields.  The inputs of the
GPU test (mask, -inf of the bias, dropout mask) are checked here for rows that would lose every key.  No compute call is made."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from attention_cases import BLOCK
from attention_double import banned_pairs, keep_scale
from attention_long_cases import (BIAS, BIAS_F32, BIAS_KINDS, BWD, CASES, FORMS, FWD, LONG_F32, LONG_KERNELS, REDUCE, _TARGS, make_bias,
                                  plan_query)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_KERNEL = re.compile(r"((?:long_(?:fwd|bwd_q|bwd_kv)|bias_bwd_ds)_kernel<[^()]*>|bias_bwd_reduce_kernel)\(")
TEMPLATES = LONG_KERNELS + ("bias_bwd_ds_kernel",)
QT, KB, CUS = 32, 64, 256
LDS_MAX = 115200      # 112.5 KiB: what launch_long asks for


@pytest.fixture(scope="module")
def built_lib():
    from afft_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "afft_amd", "csrc"), "-j4"])
    return _lib


def _instantiations(path):
    out = subprocess.check_output(["nm", "-C", path], text=True)
    return {m.group(1) for line in out.splitlines() for m in _KERNEL.finditer(line)}


def orphans(found, cases):
    """(kernels of `found` without a case, kernels the cases name that are not in `found`)"""
    covered = {k for c in cases for k in c.kernels}
    return sorted(found - covered), sorted(covered - found)


def test_every_long_attention_instantiation_has_a_case(built_lib):
    found = _instantiations(built_lib.LIB_PATH)
    if not found:       # a link that keeps no local symbols: the objects it was linked from
        objdir = os.path.join(ROOT, "afft_amd", "csrc", "build")
        for f in sorted(os.listdir(objdir)) if os.path.isdir(objdir) else []:
            if f.startswith("attention") and f.endswith(".o"):
                found |= _instantiations(os.path.join(objdir, f))
    assert len(found) >= 13, sorted(found)
    assert {s.split("<")[0] for s in found} == set(TEMPLATES) | {REDUCE}, sorted(found)
    missing, stale = orphans(found, CASES)
    assert not missing, "long attention kernels without a case in tests/attention_long_cases.py: " + "; ".join(missing)
    assert not stale, "tests/attention_long_cases.py expects kernels the library does not build: " + "; ".join(stale)


def _of(form, entry=None):
    return [c for c in CASES if c.family == form and entry in (None, c.entry)]


def test_case_table_is_well_formed():
    for c in CASES:
        assert c.entry in ("fwd_bwd", "bias") and c.storage in ("f32", "bf16") and c.align in ("a16", "a4", "odd"), c.name
        assert c.family in FORMS and (c.family == "f32") == (c.storage == "f32"), c.name
        assert (129 if c.entry == "fwd_bwd" else 1) <= c.L <= 512 and 1 <= c.hd <= 1024, c.name
        assert 2 <= c.nseq * c.H <= 6 or "many_tiles" in c.name, c.name
        assert c.mask in (0, 1, 2, 3) and (c.mask == BLOCK) == (c.period > 0) and (c.mask != BLOCK or c.L % c.period == 0), c.name
        assert c.bias in (("none", "table") if c.entry == "fwd_bwd" else BIAS_KINDS) and (c.entry == "fwd_bwd" or c.mask == 0), c.name
        assert c.drop_p in (0.0, 0.3), c.name
        assert c.mfma == (c.storage == "bf16" and c.hd % 64 == 0 and c.align != "odd"), c.name
        assert c.align != "a4" or c.mfma, c.name
        assert c.align != "odd" or (c.H * c.hd + (1 if (c.H * c.hd) % 2 == 0 else 2)) % 2 == 1, c.name
        want = [f"{k}<{_TARGS[c.family]}>" for k in LONG_KERNELS] if c.entry == "fwd_bwd" or c.L > 128 else []
        if c.entry == "bias":
            want += [f"bias_bwd_ds_kernel<{_TARGS[c.family]}>"] + ([REDUCE] if c.reduces() else [])
        assert list(c.kernels) == want, c.name

    def need(values, have, what):
        lost = sorted(set(values) - set(have))
        assert not lost, f"tests/attention_long_cases.py has no case left for {what}: {lost}"

    fb, bi = [c for c in CASES if c.entry == "fwd_bwd"], [c for c in CASES if c.entry == "bias"]
    need((129, 160, 192, 193, 256, 257, 320, 449, 511, 512), {c.L for c in fb}, "fwd_bwd at L")
    need((1, 5, 32, 33, 64, 65, 128, 129, 193, 320, 512), {c.L for c in bi}, "the bias gradient at L")
    mf = (64, 128, 192, 256, 320, 384, 768, 1024)
    need(mf, {c.hd for c in _of("mfma", "fwd_bwd")}, "MFMA forward / backward at hd")
    need(mf, {c.hd for c in _of("mfma", "bias")}, "the MFMA bias gradient at hd")
    for hc in (64, 128, 256):      # every chunk size with one chunk and with more than one, on each of the four MFMA kernels
        for entry in ("fwd_bwd", "bias"):
            need(("one chunk", "several chunks"), {"one chunk" if c.hd == c.hc else "several chunks" for c in _of("mfma", entry) if c.hc == hc},
                 f"{entry} on MFMA with hc = {hc} and")
    assert any(c.L == 512 and c.hd == 1024 for c in _of("mfma", "fwd_bwd")), "the largest LDS request (L = 512, hd = 1024 on MFMA) has no case"
    need((1, 17, 33, 65, 129, 257, 1024), {c.hd for c in _of("f32", "fwd_bwd")}, "generic fp32 at hd")
    need((24, 65), {c.hd for c in _of("bf16", "fwd_bwd") if c.align != "odd"}, "generic bf16 by hd % 64 != 0 at hd")
    need((64, 256), {c.hd for c in _of("bf16", "fwd_bwd") if c.align == "odd"}, "generic bf16 by odd pitches at hd")
    assert any(c.align == "a4" for c in _of("mfma", "fwd_bwd")), "no a4 case (result pitches = 4 mod 8) on MFMA"
    for form in FORMS:
        mine = _of(form, "fwd_bwd")
        need((0, 1, 2, 3), {c.mask for c in mine}, f"{form}: mask kind")
        bc = [c for c in mine if c.mask == BLOCK]
        assert any(c.period == 1 for c in bc) and any(c.period == c.L for c in bc) and any(c.period % 32 and 1 < c.period < c.L for c in bc), \
            f"{form}: block-causal needs period 1, L and one that 32 does not divide"
        assert any(c.bias == "table" for c in mine), f"{form}: no case with an additive table"
        for span, cs in (("long", [c for c in _of(form, "bias") if c.long]), ("short", [c for c in _of(form, "bias") if not c.long])):
            need(BIAS_KINDS, {c.bias for c in cs}, f"{form}, {span} L: bias shape kind")
        assert any(c.H == 3 for c in _of(form)), f"{form}: no case with three heads"
        for k in TEMPLATES:      # dropout on every (kernel, form) pair; the bias cases drop behind a bias
            sym = f"{k}<{_TARGS[form]}>"
            assert any(c.drop_p > 0 for c in CASES if sym in c.kernels), "no dropout case on " + sym
            assert any(c.drop_p > 0 and c.bias != "none" for c in CASES if sym in c.kernels), "no dropout case with a bias on " + sym
    assert any(c.reduces() for c in bi) and any(not c.reduces() for c in bi)
    big = [c for c in CASES if c.nseq * c.H * ((c.L + QT - 1) // QT) > CUS]
    assert big and all(c.hd == 64 and c.L == 160 for c in big), "one cheap case with more workgroups than CUs"


def _ask(_lib, args):
    r = _lib.lib().afft_attention_plan_for(*args)
    assert r >= 0, (args, _lib.lib().afft_last_error())
    assert r % 10000 == 0, (args, r)
    return r // 10000


def test_every_case_dispatches_to_its_family(built_lib):
    """a short bias case asks for the bias gradient alone: its forward is a short kernel (the query has no word for a bias)"""
    assert os.environ.get("AFFT_ATTN_GENERIC", "0") != "1"
    for c in CASES:
        form = FORMS.index(c.family)
        asks = [(FWD, LONG_F32), (BWD, LONG_F32)] if c.entry == "fwd_bwd" or c.long else []
        asks += [(BIAS, BIAS_F32)] if c.entry == "bias" else []
        for direction, base in asks:
            got = _ask(built_lib, plan_query(c, direction))
            assert got == base + form, f"{c.name}: the plan answers family {got} in direction {direction}, the case is written for {base + form}"
            if c.align == "odd" and c.storage == "bf16" and c.hd % 64 == 0:      # misalignment alone keeps it off MFMA
                assert _ask(built_lib, plan_query(c, direction, aligned=True)) == base + 2, c.name


def long_geometry(L, hd, mfma):
    """the long branch of plan_attention restated: (hc, Lp, ntiles, LDS bytes)"""
    hc = 256 if hd % 256 == 0 else 128 if hd % 128 == 0 else 64
    Lp = (L + KB - 1) // KB * KB
    return hc, Lp, (L + QT - 1) // QT, QT * (Lp + 4) * 4 + ((QT + KB) * hc * 2 if mfma else 0)


def test_chunks_tiles_and_lds_of_the_cases():
    worst = 0
    for c in CASES:
        hc, Lp, nt, lds = long_geometry(c.L, c.hd, c.mfma)
        assert lds <= LDS_MAX, c.name
        worst = max(worst, lds)
        if c.mfma:
            assert (hc, Lp, nt) == (c.hc, c.Lp, c.ntiles), f"{c.name}: hc, Lp, ntiles = {(hc, Lp, nt)}, the case says {(c.hc, c.Lp, c.ntiles)}"
            assert c.hd % c.hc == 0 and c.Lp % KB == 0 and c.Lp - KB < c.L <= c.Lp, c.name
        else:
            assert (c.hc, c.Lp, c.ntiles) == (0, 0, 0), c.name
    assert worst == LDS_MAX == QT * (512 + 4) * 4 + (QT + KB) * 256 * 2, worst


def test_inputs_leave_every_row_a_key_and_dropout_keeps_its_share():
    """the mask, the -inf entries of the bias and the dropout mask together leave every query row a key (a condition on the inputs: the
    reference alone is asked); the kept share over unmasked pairs is within 4 standard deviations of the binomial"""
    for c in CASES:
        if c.drop_p == 0 and c.bias == "none":
            continue
        open_ = np.broadcast_to(~banned_pairs(c.L, c.mask, c.period), (c.nseq, c.H, c.L, c.L))
        b = make_bias(c)
        if b is not None:
            open_ = open_ & np.isfinite(b.reshape((1,) * (4 - b.ndim) + b.shape))
        assert open_.any(-1).all(), f"{c.name}: the mask and the bias hide every key of a row"
        if c.drop_p > 0:
            _, keep = keep_scale(c.nseq, c.H, c.L, c.drop_p, c.key)
            assert (open_ & keep).any(-1).all(), f"{c.name}: a row loses every key to mask, bias and dropout"
            valid, p = keep[open_], float(np.float32(c.drop_p))
            assert abs(float(valid.mean()) - (1.0 - p)) <= 4.0 * math.sqrt(p * (1.0 - p) / valid.size), c.name
