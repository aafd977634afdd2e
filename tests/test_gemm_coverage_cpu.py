"""CPU: every GEMM kernel instantiation the library compiles is the expected kernel of at least one case of the shared GEMM case
table (tests/gemm_cases.py), which the GPU suite runs against float64 and checks, through the GEMM trace, that it ran that kernel.
A kernel added without a case fails here, by name.  The dispatch plan (csrc/gemm_plan.h) is host arithmetic: afft_gemm_plan_for
answers here what afft_gemm would launch for every case, and the shape queries are held against it.  No compute call is made (no
GPU in the build container)."""
import ctypes
import os
import re
import subprocess

import pytest

from gemm_cases import CASES, SGD_FAMILIES, _traced_symbol, dispatch_fields, gemm_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_KERNEL = re.compile(r"\b(gemm_[a-z0-9_]+_kernel<[^()]*>)\(")


@pytest.fixture(scope="module")
def built_lib():
    from afft_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "afft_amd", "csrc"), "-j4"])
    return _lib


def _instantiations(path):
    """`gemm_*_kernel<...>` symbols (host-side launch stubs of the anonymous-namespace kernels, hence local symbols) of one binary"""
    out = subprocess.check_output(["nm", "-C", path], text=True)
    return {m.group(1) for line in out.splitlines() for m in _KERNEL.finditer(line)}


def test_every_gemm_instantiation_has_a_case(built_lib):
    found = _instantiations(built_lib.LIB_PATH)
    if not found:       # a link that keeps no local symbols: the objects it was linked from
        objdir = os.path.join(ROOT, "afft_amd", "csrc", "build")
        for f in sorted(os.listdir(objdir)) if os.path.isdir(objdir) else []:
            if f.startswith("gemm") and f.endswith(".o"):
                found |= _instantiations(os.path.join(objdir, f))
    assert len(found) >= 50, sorted(found)
    kinds = {s.split("<")[0] for s in found}
    assert kinds == {"gemm_bf16_kernel", "gemm_bf16_g2_kernel", "gemm_bf16_pp_kernel", "gemm_bf16_pp2_kernel", "gemm_bf16_bd_kernel",
                     "gemm_f32_kernel"}, kinds
    covered = {c.kernel for c in CASES}
    missing = sorted(found - covered)
    assert not missing, "GEMM kernels without a case in tests/gemm_cases.py: " + "; ".join(missing)
    stale = sorted(covered - found)
    assert not stale, "tests/gemm_cases.py expects kernels the library does not build: " + "; ".join(stale)


def test_case_table_is_well_formed():
    modes = {"bf16", "f32", "bf16x3", "fp16x2", "fp16", "fp16_lo8"}
    for c in CASES:
        assert c.layout in ("nt", "nn", "tn", "tt") and c.mode in modes, c.name
        assert c.layout != "tt" or not c.fast, c.name       # (A k-strided, B k-contiguous) has no fast-path kernel
        assert (c.mode == "f32") <= (c.kernel == "gemm_f32_kernel<float>"), c.name
        assert c.variant in (0, 1, 3, 4, 7, 8, 9, 10) and c.splitk in (0, 1, 2, 4), c.name
        assert not (c.epi.get("accumulate") and c.epi.get("out", "f32") != "f32"), c.name
        assert not ((c.epi.get("out_lo") or c.epi.get("out_lo8")) and c.epi.get("out") != "f16"), c.name
        s = c.epi.get("sgd")
        if s is not None:
            assert set(c.epi) == {"sgd"}, c.name      # the fused update takes the plain product: alpha, ldo, col0 live in its dict
            assert set(s) <= {"flags", "images", "ok", "alpha", "ldo", "col0"} and s["flags"] in (0, 1, 2, 3) and s["ok"] in (None, 0, 1), c.name
            assert set(s["images"]) <= {"bf16", "f16", "f8", "pk"} and len(set(s["images"])) == len(s["images"]), c.name
            assert "pk" not in s["images"] or (c.M % 16 == 0 and s.get("ldo", 0) % 32 == 0 and s.get("ldo", 0) >= s.get("col0", 0) + c.N), c.name


def test_every_weight_gradient_kernel_family_carries_the_fused_update():
    """every kernel family a weight gradient can reach ends in the fused SGD update in at least one case, and the cases together
    cover what the update's code branches on"""
    sgd = [c for c in CASES if "sgd" in c.epi]
    carried = {c.kernel for c in sgd}
    for k in SGD_FAMILIES:
        assert k in carried, f"no `sgd` case of tests/gemm_cases.py runs on {k}"
    tn_families = {c.kernel.split("<")[0] for c in CASES if c.layout == "tn"}
    assert tn_families == {k.split("<")[0] for k in SGD_FAMILIES}, tn_families      # a new family with a tn case: add it to SGD_FAMILIES
    assert {c.layout for c in sgd} >= {"tn", "nt", "nn"}
    s = [c.epi["sgd"] for c in sgd]
    assert {x["flags"] for x in s} == {0, 1, 2, 3} and {x["ok"] for x in s} == {None, 0, 1}
    assert {x.get("alpha", 1.0) for x in s} >= {0.5, -2.0, 1.0}
    assert any(c.splitk > 1 and "pk" in c.epi["sgd"]["images"] for c in sgd)
    widths = {(x.get("ldo", 0) % 8, x.get("col0", 0) % 4) for x in s}
    assert {(0, 0), (4, 0), (0, 1)} <= widths, widths


def _plan_for(_lib, fields):
    """afft_gemm_plan_for on a descriptor with these fields -> (return value, trace record)"""
    d, rec = _lib.GemmDesc(), _lib.GemmTraceRec()
    for k, v in fields.items():
        setattr(d, k, v)
    return _lib.lib().afft_gemm_plan_for(ctypes.byref(d), ctypes.byref(rec)), rec


def test_every_case_dispatches_to_its_kernel(built_lib):
    """The kernel the table names for a case is the kernel the dispatch plan picks for the case's operands (the GPU suite checks the same
    through the trace of the launch itself).  The expectations were established on a 256-CU part; without a device the library
    assumes 256 CUs as well."""
    lib = built_lib.lib()
    for c in CASES:
        built_lib.check(lib.afft_set_gemm_variant(c.variant))
        built_lib.check(lib.afft_set_gemm_splitk(c.splitk))
        try:
            rc, rec = _plan_for(built_lib, dispatch_fields(c))
        finally:
            built_lib.check(lib.afft_set_gemm_variant(0))
            built_lib.check(lib.afft_set_gemm_splitk(1))
        if c.fast:
            assert rc == 1, (c.name, rc, lib.afft_last_error())
            assert _traced_symbol(rec) == c.kernel, f"{c.name}: the plan picks {_traced_symbol(rec)}, the case is written for {c.kernel}"
            assert (rec.M, rec.N, rec.K, rec.ms) == (c.M, c.N, c.K, 0.0), c.name
        else:
            assert rc == 0, (c.name, rc, _traced_symbol(rec))


def test_shape_queries_agree_with_the_plan(built_lib):
    """The five shape queries against afft_gemm_plan_for on the row-major problem they describe (unpadded operands, ample workspace),
    for the shapes of the training step's forward and backward GEMMs."""
    from afft_amd import ops
    lib = built_lib.lib()
    shapes = [c for c in CASES if c.name.startswith(("fwd_", "bwd_"))]
    assert len(shapes) >= 20
    for c in shapes:
        M, N, K = c.M, c.N, c.K
        a_t, b_t = c.layout[0] == "t", c.layout[1] == "t"
        a_ks, b_ks = int(a_t), int(not b_t)
        geom = (c.layout, M, N, K, M if a_t else K, K if b_t else N)
        rc, rec = _plan_for(built_lib, gemm_fields(*geom, ws_bytes=ops._WS_BYTES))
        assert rc == 1, c.name
        assert lib.afft_gemm_variant_for(M, N, K, a_ks, b_ks) == {12: 1, 13: 3}.get(rec.variant, rec.variant), c.name
        assert lib.afft_gemm_splitk_for(M, N, K, a_ks, b_ks) == rec.splitk, c.name
        need = lib.afft_gemm_workspace_bytes(M, N, K, a_ks, b_ks)
        assert (need > 0) == (rec.splitk > 1) and need <= ops._WS_BYTES, c.name
        if need:      # exactly that many bytes let the launch split; one fewer and it runs unsplit
            assert _plan_for(built_lib, gemm_fields(*geom, ws_bytes=need))[1].splitk == rec.splitk, c.name
            assert _plan_for(built_lib, gemm_fields(*geom, ws_bytes=need - 1))[1].splitk == 1, c.name
        # the NT problem of this size: with a fragment-packed B, and in the fp16 + fp8 precision
        rc, rec = _plan_for(built_lib, gemm_fields("nt", M, N, K, K, K, packed=True, ws_bytes=ops._WS_BYTES))
        assert rc == 1 and lib.afft_gemm_packed_wanted(M, N, K) == int(rec.variant == 10), c.name
        rc, rec = _plan_for(built_lib, gemm_fields("nt", M, N, K, K, K, split3=3, ld8=K, ws_bytes=ops._WS_BYTES))
        assert K % 128 == 0 and lib.afft_gemm_lo8_ok(M, N, K) == int(rc == 1), (c.name, rc)
        assert rc == 1 or (rc < 0 and b"afft_gemm_lo8_ok" in lib.afft_last_error()), (c.name, rc)
