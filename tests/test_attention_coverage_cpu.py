"""CPU: every short-attention kernel instantiation the library compiles -- attn_fwd_kernel / attn_bwd_kernel<T, LM>,
attn_fwd_mfma_kernel<NT, PL>, attn_bwd_mfma_kernel<NT>, attn_bwd_sliced_kernel<NT> -- is the kernel of at least one case of the shared
table (tests/attention_cases.py), which the GPU suite runs elementwise against float64 (tests/test_attention_short_gpu.py).  A kernel
added to a launcher without a case fails here, by name; so does a case whose kernel is not built.  The dispatch plan
(csrc/attn_plan.h) is host arithmetic: afft_attention_plan_for answers here which kernel every case runs, and the chunk and packing
factor of plan_short_mfma are restated and held against the case's fields.  No compute call is made."""
import os
import re
import subprocess

import pytest

from attention_cases import BWD, CASES, FWD, GENERIC, MFMA_BWD, MFMA_FWD, SLICED_BWD, plan_query
from test_attention_plan_cpu import lds_fits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_KERNEL = re.compile(r"\b(attn_(?:fwd|bwd)(?:_mfma|_sliced)?_kernel<[^()]*>)\(")
KINDS = {"attn_fwd_kernel", "attn_bwd_kernel", "attn_fwd_mfma_kernel", "attn_bwd_mfma_kernel", "attn_bwd_sliced_kernel"}
LDS_160K = 160 * 1024


@pytest.fixture(scope="module")
def built_lib():
    from afft_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "afft_amd", "csrc"), "-j4"])
    return _lib


def _instantiations(path):
    """the short-attention kernel symbols (host-side launch stubs of the anonymous-namespace kernels, hence local symbols) of one binary"""
    out = subprocess.check_output(["nm", "-C", path], text=True)
    return {m.group(1) for line in out.splitlines() for m in _KERNEL.finditer(line)}


def test_every_attention_instantiation_has_a_case(built_lib):
    found = _instantiations(built_lib.LIB_PATH)
    if not found:       # a link that keeps no local symbols: the objects it was linked from
        objdir = os.path.join(ROOT, "afft_amd", "csrc", "build")
        for f in sorted(os.listdir(objdir)) if os.path.isdir(objdir) else []:
            if f.startswith("attention") and f.endswith(".o"):
                found |= _instantiations(os.path.join(objdir, f))
    assert len(found) >= 26, sorted(found)
    kinds = {s.split("<")[0] for s in found}
    assert kinds == KINDS, kinds
    covered = {k for c in CASES for k in (c.fwd, c.bwd) if k}
    missing = sorted(found - covered)
    assert not missing, "attention kernels without a case in tests/attention_cases.py: " + "; ".join(missing)
    stale = sorted(covered - found)
    assert not stale, "tests/attention_cases.py expects kernels the library does not build: " + "; ".join(stale)


def test_case_table_is_well_formed():
    for c in CASES:
        assert c.entry in ("fwd_bwd", "split") and c.align in ("a16", "a8", "odd"), c.name
        assert c.storage in (("f32", "bf16") if c.entry == "fwd_bwd" else ("f16x2", "f16x1")), c.name
        assert (c.bwd is None) == (c.entry == "split"), c.name
        assert 1 <= c.L <= (128 if c.entry == "fwd_bwd" else 64) and 1 <= c.hd <= 1024, c.name
        assert c.nseq <= 17 and c.H <= 3 and c.nseq * c.H >= 2, c.name
        assert c.mask in (0, 1, 2, 3) and not (c.mask == 1 and c.L == 1), c.name
        assert (c.mask == 3) == (c.period > 0) and (c.mask != 3 or c.L % c.period == 0), c.name
        assert c.drop_p in (0.0, 0.3), c.name
        assert c.align == "a16" or c.entry == "fwd_bwd", c.name      # the planes have no fallback to misalign into
        assert c.align != "a8" or c.bwd.startswith("attn_bwd_mfma_kernel"), c.name
        assert c.align != "odd" or (c.H * c.hd) % 2 == 0, c.name     # width + 1 frame column: an odd pitch
    for kind in KINDS:      # every family: three heads somewhere, dropout on every instantiation of the MFMA families
        mine = [c for c in CASES if kind in (c.fwd.split("<")[0], (c.bwd or "").split("<")[0])]
        assert any(c.H == 3 for c in mine), kind
    for sym in {k for c in CASES for k in (c.fwd, c.bwd) if k and ("_mfma_" in k or "_sliced_" in k)}:
        assert any(c.drop_p > 0 for c in CASES if sym in (c.fwd, c.bwd)), "no dropout case on " + sym
    for t in ("float", "unsigned short"):
        for lm in (32, 64, 128):
            mine = [c for c in CASES if c.fwd == f"attn_fwd_kernel<{t}, {lm}>"]
            assert any(c.drop_p > 0 for c in mine), (t, lm)
    for lm in (32, 64, 128):      # every mask kind at every LM
        assert {c.mask for c in CASES if c.fwd.endswith(f", {lm}>") and not c.mfma} == {0, 1, 2, 3}, lm
    for nt in (1, 2, 4):          # and at every NT of the bf16 MFMA kernels; block-causal with period 1, L and one that 16 does not divide
        assert {c.mask for c in CASES if c.fwd == f"attn_fwd_mfma_kernel<{nt}, 0>"} == {0, 1, 2, 3}, nt
    bc = [c for c in CASES if c.mfma and c.mask == 3]
    assert any(c.period == 1 for c in bc) and any(c.period == c.L for c in bc) and any(c.period % 16 and 1 < c.period < c.L for c in bc)
    packed = [c for c in CASES if c.mfma and c.G > 1 and c.nseq % c.G and c.drop_p > 0]
    assert {3, 5, 8} <= {c.L for c in packed}


def _symbols(c, direction, family, p0, p1):
    """(family, p0, p1) of afft_attention_plan_for -> the kernel symbol"""
    t = {"f32": "float", "bf16": "unsigned short"}.get(c.storage, "?")
    if family == GENERIC:
        return f"attn_{'fwd' if direction == FWD else 'bwd'}_kernel<{t}, {p0}>"
    if family == MFMA_FWD:
        return f"attn_fwd_mfma_kernel<{p0}, {p1}>"
    if family in (MFMA_BWD, SLICED_BWD):
        return f"attn_bwd_{'mfma' if family == MFMA_BWD else 'sliced'}_kernel<{p0}>"
    return f"<family {family}>"


def _ask(_lib, args):
    r = _lib.lib().afft_attention_plan_for(*args)
    assert r >= 0, (args, _lib.lib().afft_last_error())
    return r // 10000, r % 10000 // 10, r % 10


def test_every_case_dispatches_to_its_kernels(built_lib):
    assert os.environ.get("AFFT_ATTN_GENERIC", "0") != "1"
    for c in CASES:
        got = _symbols(c, FWD, *_ask(built_lib, plan_query(c, FWD)))
        assert got == c.fwd, f"{c.name}: the plan picks {got} forward, the case is written for {c.fwd}"
        if c.bwd is None:
            continue
        got = _symbols(c, BWD, *_ask(built_lib, plan_query(c, BWD)))
        if c.align == "a8":      # the query cannot say "8-byte gradient rows": the aligned problem is sliced (the GPU test shows a8 is not)
            nt = c.bwd[c.bwd.index("<"):]
            assert c.bwd == "attn_bwd_mfma_kernel" + nt and got == "attn_bwd_sliced_kernel" + nt, (c.name, got)
        else:
            assert got == c.bwd, f"{c.name}: the plan picks {got} backward, the case is written for {c.bwd}"
        if c.align == "odd" and c.storage == "bf16" and c.hd % 64 == 0 and c.L <= 64:      # misalignment alone keeps it off the MFMA kernels
            assert _ask(built_lib, plan_query(c, FWD, aligned=True))[0] == MFMA_FWD, c.name
            assert _ask(built_lib, plan_query(c, BWD, aligned=True))[0] in (MFMA_BWD, SLICED_BWD), c.name


def short_mfma_geometry(L, hd, planes_per_tile, backward, budget_kib):
    """plan_short_mfma restated: (NT, hc, G, LDS bytes of the [16 NT][hc] tiles) -- the whole head in 3 (forward) / 4 (backward) tiles
    when that fits the budget, else the largest chunk hd / 2, hd / 4, .. that is a multiple of 64, divides hd and fits in one tile fewer"""
    NT = 1 if L <= 16 else 2 if L <= 32 else 4
    tile = planes_per_tile * 16 * NT * 2      # bytes per staged channel
    whole, chunked = (4, 3) if backward else (3, 2)
    if whole * tile * hd <= budget_kib * 1024:
        return NT, hd, 16 * NT // L, whole * tile * hd
    hc = hd // 2
    while hc >= 64:
        if hd % hc == 0 and hc % 64 == 0 and chunked * tile * hc <= budget_kib * 1024:
            return NT, hc, 16 * NT // L, chunked * tile * hc
        hc //= 2
    return NT, None, 16 * NT // L, 0


def test_chunks_packing_and_lds_of_the_mfma_cases():
    exact = set()
    for c in (c for c in CASES if c.mfma):
        nt_sym = int(c.fwd[c.fwd.index("<") + 1])
        np_, budget = (2 if c.storage == "f16x2" else 1), (48 if c.entry == "split" else 160)
        NT, hc, G, lds = short_mfma_geometry(c.L, c.hd, np_, False, budget)
        assert lds_fits(c.hd, NT, np_, False, budget) == (hc is not None), c.name
        assert (NT, hc, G) == (nt_sym, c.hc, c.G), f"{c.name}: forward NT, hc, G = {(NT, hc, G)}, the case says {(nt_sym, c.hc, c.G)}"
        assert lds <= budget * 1024, c.name
        if c.bwd:
            NT, hc, G, lds = short_mfma_geometry(c.L, c.hd, 1, True, 160)
            assert lds_fits(c.hd, NT, 1, True, 160) == (hc is not None), c.name
            assert (NT, hc, G) == (nt_sym, c.hc_bwd, c.G), f"{c.name}: backward NT, hc, G = {(NT, hc, G)}, the case says {(nt_sym, c.hc_bwd, c.G)}"
            if "_mfma_" in c.bwd and lds == LDS_160K:
                exact.add((NT, c.hd))
        if "chunks" in c.name:
            assert c.hc < c.hd or (c.bwd and c.hc_bwd < c.hd), c.name
    # the two whole-head backward requests of exactly the CU's 160 KiB, which the plan accepts with <=
    assert exact == {(2, 640), (4, 320)}, exact
    fwd_chunks = {(int(c.fwd[c.fwd.index("<") + 1]), c.hd, c.hc) for c in CASES if c.mfma and c.entry == "fwd_bwd" and c.hc < c.hd}
    assert fwd_chunks == {(4, 512, 256), (4, 768, 384), (2, 1024, 512), (4, 1024, 512)}, fwd_chunks
    assert any(c.storage == "f16x2" and c.hc < c.hd for c in CASES) and any(c.storage == "f16x1" and c.hc < c.hd for c in CASES)
