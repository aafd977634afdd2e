"""CPU: every GEMM kernel instantiation the library compiles is the expected kernel of at least one case of the shared GEMM case
table (tests/gemm_cases.py), which the GPU suite runs against float64 and checks, through the GEMM trace, that it ran that kernel.
A kernel added without a case fails here, by name.  No compute call is made (no GPU in the build container)."""
import os
import re
import subprocess

import pytest

from gemm_cases import CASES

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
