"""ctypes binding of the C-ABI in include/afft_hip.h (libafft_hip.so, built by afft_amd/csrc/Makefile).

The product path fails loudly when the HIP library is missing: there is no CPU or eager-PyTorch
fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AFFT_LIB") or os.path.join(_HERE, "lib", "libafft_hip.so")   # AFFT_LIB: kernel-tuning builds

# Everything below is read from include/afft_hip.h by _cabi: nothing of the ABI is restated here.
globals().update({k[len("AFFT_"):]: v for k, v in _cabi.consts.items()})      # AFFT_X -> X: F32 / BF16 / F16, ACT_*, MASK_*, K_*, SGD_*, ...

_NAMES = {"afft_dropout_t": "Dropout", "afft_sgd_fused_t": "SgdFused", "afft_gemm_t": "GemmDesc", "afft_attn_sublayer_t": "AttnSublayer",
          "afft_mlp_sublayer_t": "MLPSublayer", "afft_cross_attn_sublayer_t": "CrossAttnSublayer", "afft_attn_step_sublayer_t": "AttnStepSublayer",
          "afft_gemm_trace_rec_t": "GemmTraceRec", "afft_kernel_trace_rec_t": "KernelTraceRec"}      # C struct -> its public name here
for _c, _py in _NAMES.items():
    _cabi.structs[_c].__name__ = _cabi.structs[_c].__qualname__ = _py
    globals()[_py] = _cabi.structs[_c]

i32, i64, f32, vp, u32, fp = C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.c_uint32, C.POINTER(C.c_float)
SgdP, DropP = C.POINTER(SgdFused), C.POINTER(Dropout)      # noqa: F821

_SIGS = {name: sig for name, sig in _cabi.protos.items() if name != "afft_last_error"}      # name -> (argtypes, restype)
EXPORTS = sorted(_cabi.protos)

_lib = None


def lib():
    """The loaded shared library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"afft_amd: {LIB_PATH} is missing. Build it with `make -C afft_amd/csrc` "
                f"(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
        beside = os.path.join(os.path.dirname(LIB_PATH), "afft_hip.h")      # the header the library was built from, where the Makefile put it
        if os.path.exists(beside):
            with open(beside, "rb") as f:
                if f.read() != _cabi.TEXT:
                    raise RuntimeError(
                        f"afft_amd: {LIB_PATH} is stale: it was built from a header that differs from {_cabi.HEADER}, which this "
                        f"binding was derived from. Rebuild it with `make -C afft_amd/csrc`.")
        _lib = C.CDLL(LIB_PATH)
        for name, (args, res) in _cabi.protos.items():
            fn = getattr(_lib, name)
            fn.argtypes = args
            fn.restype = res
        if os.environ.get("AFFT_GEMM_SPLITK"):      # 0 off, 1 automatic (default), 2 / 4 forced
            check(_lib.afft_set_gemm_splitk(int(os.environ["AFFT_GEMM_SPLITK"])), "set_gemm_splitk")
        if os.environ.get("AFFT_GEMM_VARIANT"):
            check(_lib.afft_set_gemm_variant(int(os.environ["AFFT_GEMM_VARIANT"])), "set_gemm_variant")
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().afft_last_error().decode(errors="replace")
        raise RuntimeError(f"afft_hip {what} failed (code {rc}): {msg}")
