"""CPU: the attention dispatch plan (csrc/attn_plan.h) is host arithmetic: afft_attention_plan_for answers without a device.  The rule
is stated here independently (as tests/gemm_cases.py states the GEMM rule) and compared over the whole grid of directions, dtypes,
lengths, head dimensions, plane forms and alignments; the entry points' argument checks run before anything touches a device, so
their error texts are asserted with dummy pointers that are never dereferenced."""
import itertools
import os
import subprocess
import sys

import pytest

from afft_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, BWD, BIAS = 0, 1, 2
HDS = (1, 8, 63, 64, 128, 192, 256, 512, 1024, 1025)
LS = range(1, 514)


def lds_fits(hd, NT, planes_per_tile, backward, budget_kib):
    """the MFMA short kernels stage [16 NT][hc] bf16 tiles: the whole head (3 tiles forward, 4 backward) or, one tile fewer, a chunk hc =
    hd / 2, hd / 4, .. that is a multiple of 64 and divides hd"""
    def size(tiles, hc):
        return tiles * planes_per_tile * 16 * NT * hc * 2
    if size(4 if backward else 3, hd) <= budget_kib * 1024:
        return True
    hc = hd // 2
    while hc >= 64:
        if hd % hc == 0 and hc % 64 == 0 and size(3 if backward else 2, hc) <= budget_kib * 1024:
            return True
        hc //= 2
    return False


def expected(direction, dtype, L, hd, planes, in_lo, ok, generic=False):
    """(family, p0, p1) as include/afft_hip.h numbers them, or None: refused"""
    if not 1 <= L <= 512:
        return None
    NT = 1 if L <= 16 else 2 if L <= 32 else 4
    if planes:      # the fp16x2 forward: MFMA kernels or nothing; AFFT_ATTN_GENERIC does not apply
        if direction != FWD or L > 64 or hd % 64 or hd > 1024 or not ok or not lds_fits(hd, NT, 2 if in_lo else 1, False, 48):
            return None      # (48 KiB: three workgroups per CU; hd = 192 has no chunk)
        return (2, NT, 1 if in_lo else 2)
    if not 1 <= hd <= 1024:
        return None
    mfma = dtype == _lib.BF16 and not generic and ok and hd % 64 == 0
    form = 0 if dtype == _lib.F32 else 2 if mfma else 1
    if direction == BIAS:
        return (8 + form, 0, 0)
    if L > 128:
        return (5 + form, 0, 0)
    if mfma and L <= 64 and lds_fits(hd, NT, 1, direction == BWD, 160):
        if direction == FWD:
            return (2, NT, 0)
        return (4 if NT <= 2 and hd % 128 == 0 and hd <= 512 else 3, NT, 0)
    return (1, 32 if L <= 32 else 64 if L <= 64 else 128, 0)


def asked(direction, dtype, L, hd, planes, in_lo, ok):
    r = _lib.lib().afft_attention_plan_for(direction, dtype, L, hd, planes, in_lo, ok)
    return None if r < 0 else (r // 10000, r % 10000 // 10, r % 10)


def grid(dtypes):
    return itertools.product((FWD, BWD, BIAS), dtypes, LS, HDS, ((0, 0), (1, 0), (1, 1)), (1, 0))


def mismatches(dtypes, generic):
    rows = ((a, asked(*a), expected(*a, generic=generic)) for a in ((d, t, L, hd, pl, lo, ok) for d, t, L, hd, (pl, lo), ok in grid(dtypes)))
    return [r for r in rows if r[1] != r[2]]


def test_plan_matches_the_rule_on_the_full_grid():
    assert os.environ.get("AFFT_ATTN_GENERIC", "0") != "1"
    assert mismatches((_lib.F32, _lib.BF16), False)[:5] == []


def test_plan_with_the_generic_switch_in_a_child_process():
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_attention_plan_cpu as t\nfrom afft_amd import _lib\n"
            "bad = t.mismatches((_lib.BF16,), True)\nassert not bad, bad[:5]\nprint('rows ok')") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, AFFT_ATTN_GENERIC="1"), capture_output=True, text=True)
    assert r.returncode == 0 and "rows ok" in r.stdout, r.stderr[-2000:]


def test_coverage_facts():
    for d, t, L in itertools.product((FWD, BWD), (_lib.F32, _lib.BF16), range(1, 513)):
        assert asked(d, t, L, 64, 0, 0, 1) and asked(d, t, L, 8, 0, 0, 0), (d, t, L)
    for lo in (0, 1):
        assert asked(FWD, _lib.F16, 64, 1024, 1, lo, 1) == (2, 4, 2 - lo)
        for L, hd in ((65, 64), (16, 63), (16, 96), (16, 1088), (16, 2048)):
            assert asked(FWD, _lib.F16, L, hd, 1, lo, 1) is None, (L, hd)
    for a in itertools.product((FWD, BWD, BIAS), (_lib.F32, _lib.BF16), (513,), HDS, (0, 1), (0, 1), (0, 1)):
        assert asked(*a) is None, a


P = 4096      # a null-free, 16-byte aligned dummy pointer


def _fwd(**kw):
    a = dict(q=P, ldq=64, k=P, ldk=64, v=P, ldv=64, dtype=_lib.F32, nseq=1, L=16, H=1, hd=64, scale=0.125, mask=0, period=0, drop_p=0.0,
             key=0, out=P, ldo=64, probs=None, stream=None)
    return dict(a, **kw)


def _with(a, after, drop=(), **new):
    """a's arguments in order, without `drop`, with `new` inserted behind `after`"""
    out = {}
    for k, v in a.items():
        if k not in drop:
            out[k] = v
        if k == after:
            out.update(new)
    return out


def _bwd(**kw):
    a = dict(dout=P, lddo=64, q=P, ldq=64, k=P, ldk=64, v=P, ldv=64, dtype=_lib.F32, probs=P, nseq=1, L=16, H=1, hd=64, scale=0.125,
             drop_p=0.0, key=0, dq=P, lddq=64, dk=P, lddk=64, dv=P, lddv=64, stream=None)
    return dict(a, **kw)


ENTRIES = {
    "attention_fwd": lambda **kw: _fwd(**kw),
    "attention_fwd_table": lambda **kw: dict(_with(_fwd(), "scale", ("mask", "period"), table=P), **kw),
    "attention_fwd_bias": lambda **kw: dict(_with(_fwd(), "scale", ("mask", "period"), bias=P, sb=0, sh=0, si=16), **kw),
    "attention_fwd_split": lambda **kw: dict(_with(_with(_with(_fwd(), "ldv", ("dtype",), in_lo=0), "ldo", out_lo=0, out_bf16=None, ldob=0),
                                                   "probs", out_lo8=None), **kw),
    "attention_bwd": lambda **kw: _bwd(**kw),
    "attention_long_fwd": lambda **kw: dict(_with(_fwd(L=160), "period", table=None), **kw),
    "attention_long_fwd_bias": lambda **kw: dict(_with(_fwd(L=160), "scale", ("mask", "period"), bias=P, sb=0, sh=0, si=160), **kw),
    "attention_long_bwd": lambda **kw: dict(_with(_bwd(L=160), "lddv", row_term=P), **kw),
    "attention_bias_bwd": lambda **kw: dict(dict(dout=P, lddo=64, v=P, ldv=64, dtype=_lib.F32, probs=P, nseq=1, L=16, H=1, hd=64, drop_p=0.0, key=0,
                                                 dbias=P, sb=256, sh=256, si=16, scratch=None, stream=None), **kw),
}
RANGE = {"attention_fwd": "1..128", "attention_fwd_table": "1..128", "attention_fwd_bias": "1..128", "attention_bwd": "1..128",
         "attention_fwd_split": "1..64 (MFMA path only)", "attention_long_fwd": "129..512", "attention_long_fwd_bias": "129..512",
         "attention_long_bwd": "129..512", "attention_bias_bwd": "1..512"}
MASKED = ("attention_fwd", "attention_fwd_split", "attention_long_fwd")
BATCH = ("attention_long_fwd", "attention_long_fwd_bias", "attention_long_bwd", "attention_bias_bwd")


def refused(name, **kw):
    lib = _lib.lib()
    assert getattr(lib, "afft_" + name)(*ENTRIES[name](**kw).values()) == 1, (name, kw)
    return lib.afft_last_error().decode()


@pytest.mark.parametrize("name", list(ENTRIES))
def test_error_texts(name):
    first = "dout" if "bwd" in name else "q"
    assert refused(name, **{first: None}) == name + ": null pointer"
    for L in (0, 513):
        assert refused(name, L=L) == "%s: sequence length %d outside %s" % (name, L, RANGE[name])
    assert refused(name, drop_p=1.0) == name + ": dropout p outside [0,1)"
    if name != "attention_fwd_split":
        assert refused(name, hd=1025) == name + ": head dimension 1025 outside 1..1024"
        assert refused(name, dtype=7) == name + ": bad dtype 7"
    if name in MASKED:
        L = ENTRIES[name]()["L"]
        assert refused(name, mask=4) == name + ": bad mask 4"
        assert refused(name, mask=3, period=7) == "%s: block-causal mask needs a period that divides L (L=%d, period=7)" % (name, L)
        assert refused(name, mask=3, period=0).startswith(name + ": block-causal mask needs a period")
        if name != "attention_long_fwd":
            assert refused(name, mask=1, L=1) == name + ": diagonal mask with L=1 masks every key"
    if name in BATCH:
        assert refused(name, nseq=-1) == name + ": bad nseq -1 / H 1"
        assert refused(name, H=0) == name + ": bad nseq 1 / H 0"
    if "sb" in ENTRIES[name]():
        ptr = "dbias" if name == "attention_bias_bwd" else "bias"
        assert refused(name, sh=-1).startswith("%s: negative bias stride (sb=" % name) and "sh=-1" in _lib.lib().afft_last_error().decode()
        assert refused(name, **{ptr: P + 2}) == "%s: %s pointer 0x1002 is not 4-byte aligned" % (name, ptr)
    if name in ("attention_fwd_table", "attention_fwd_bias", "attention_long_fwd_bias"):
        assert refused(name, **{"table" if "table" in name else "bias": None}) == name + ": null pointer"
    if name == "attention_long_bwd":
        assert refused(name, row_term=None) == name + ": null pointer"
    if name == "attention_bias_bwd":
        assert refused(name, sb=0).startswith(name + ": a broadcast bias needs 4-byte aligned scratch of nseq*H*L*L floats (scratch=")
        assert refused(name, sb=0, scratch=P + 2).startswith(name + ": a broadcast bias needs 4-byte aligned scratch")
    if name == "attention_fwd_split":
        assert refused(name, in_lo=-8) == name + ": in_lo is the distance to the inputs' lo planes (0: one fp16 plane each)"
        assert refused(name, out_lo8=P, out_lo=8) == name + ": out_lo8 excludes out_lo and must be 4-byte aligned"
        assert refused(name, out_lo8=P + 1) == name + ": out_lo8 excludes out_lo and must be 4-byte aligned"
        for kw in (dict(hd=63), dict(hd=2048), dict(ldq=65)):
            assert refused(name, **kw) == ("attention_fwd_split: shape not handled by the MFMA path (hd %d must be a multiple of 64 and <= 1024, "
                                           "16-byte aligned rows)" % kw.get("hd", 64))


def test_nothing_to_do_is_not_an_error():
    lib = _lib.lib()
    for name in ENTRIES:
        assert getattr(lib, "afft_" + name)(*ENTRIES[name](nseq=0).values()) == 0, name
    assert lib.afft_attention_fwd(*ENTRIES["attention_fwd"](nseq=0, dtype=7).values()) == 0      # the short pair looks at dtype after this
    assert lib.afft_attention_bwd(*ENTRIES["attention_bwd"](nseq=0, dtype=7).values()) == 0


def test_python_gates_ask_the_query(monkeypatch):
    """functional.attn_take_ok and the composite gate of AttnSublayer.forward (both through _attn_core_ok) under 'fp16x2'"""
    import torch
    from afft_amd import functional as F_, runtime as rt
    monkeypatch.setattr(rt, "precision", lambda: "fp16x2")
    monkeypatch.setattr(F_, "_composite_ok", lambda *a, **k: True)
    for L, hd in itertools.product(LS, HDS):
        want = asked(FWD, _lib.F16, L, hd, 1, 1, 1) is not None
        assert F_._attn_core_ok(L, hd) == want, (L, hd)
        assert want or not (L <= 16 and hd in (64, 128, 192, 256, 512, 1024))
        x = torch.empty(64 * L, 2 * hd, device="meta")      # shape only
        assert F_.attn_take_ok(x, L, 2) == (want and 1 < L <= 128), (L, hd)
    monkeypatch.setattr(rt, "precision", lambda: "bf16")
    assert F_._attn_core_ok(128, 8)
