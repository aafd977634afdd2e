"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/afft_hip.h declares.
No compute call is made here (no GPU in the build container)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    from afft_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "afft_amd", "csrc"), "-j4"])
    return _lib


def test_header_symbols_are_exported(built_lib):
    hdr = open(os.path.join(ROOT, "include", "afft_hip.h")).read()
    declared = sorted(set(re.findall(r"\b(afft_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) >= 15
    lib = ctypes.CDLL(built_lib.LIB_PATH)
    for sym in declared:
        assert hasattr(lib, sym), f"{sym} declared in include/afft_hip.h but not exported"
    assert sorted(built_lib.EXPORTS) == declared, "ctypes signature table and header disagree"


def test_library_loads_and_reports_version(built_lib):
    assert built_lib.lib().afft_version() >= 1


def test_gemm_desc_matches_c_layout(built_lib):
    # offsets computed by the C compiler for afft_gemm_t must equal the ctypes mirror
    src = r'''
#include <stddef.h>
#include <stdio.h>
#include "afft_hip.h"
int main(){ printf("%zu %zu %zu %zu %zu %zu\n", sizeof(afft_gemm_t), offsetof(afft_gemm_t, alpha),
  offsetof(afft_gemm_t, aux), offsetof(afft_gemm_t, rowscale), offsetof(afft_gemm_t, out), offsetof(afft_gemm_t, out2_dtype)); return 0; }
'''
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    G = built_lib.GemmDesc
    want = [ctypes.sizeof(G), G.alpha.offset, G.aux.offset, G.rowscale.offset, G.out.offset, G.out2_dtype.offset]
    assert got == want


def _struct_cases():
    """every struct the reader finds in the header, under the name _lib publishes it by: a ninth struct is covered without an edit"""
    from afft_amd import _cabi, _lib
    return [(cname, _lib._NAMES.get(cname, cname)) for cname in _cabi.structs]


@pytest.mark.parametrize("cname,pyname", _struct_cases())
def test_every_struct_field_matches_c_layout(built_lib, cname, pyname):
    """sizeof and the offset of EVERY field of each derived ctypes structure against what the C compiler lays out for the header."""
    import tempfile
    from afft_amd import _cabi
    S = _cabi.structs[cname]
    assert getattr(built_lib, pyname, S) is S
    names = [f[0] for f in S._fields_]
    body = "".join(f'printf("%zu\\n", offsetof({cname}, {n}));' for n in names)
    src = f'#include <stddef.h>\n#include <stdio.h>\n#include "afft_hip.h"\nint main(){{ printf("%zu\\n", sizeof({cname})); {body} return 0; }}\n'
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got[0] == ctypes.sizeof(S), (got[0], ctypes.sizeof(S))
    for n, off in zip(names, got[1:]):
        assert getattr(S, n).offset == off, (n, getattr(S, n).offset, off)


def test_no_gpu_means_loud_failure(built_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from afft_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.layernorm_fwd(torch.zeros(2, 4), None, None, 1e-6, torch.zeros(2, 4))


# ---------------------------------------------------------------- the binding is derived from the header (afft_amd/_cabi.py)

def _gcc(src, *args, run=False):
    """compile `src` against the header in a temporary directory; returns the -aux-info text, or the program's output with run=True"""
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        c, out = os.path.join(td, "t.c"), os.path.join(td, "t.out")
        open(c, "w").write(src)
        if run:
            subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", out])
            return subprocess.check_output([out]).decode()
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", "-aux-info", out, c])
        return open(out).read()


def test_signatures_match_the_compilers_reading_of_the_header(built_lib):
    """gcc's own canonical list of the header's prototypes (-aux-info) against the derived table: names, argument counts, at every
    position the same scalar C type or a pointer of the same kind, and the result type."""
    from afft_amd import _cabi
    scalars = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float}

    def want(t, ret=False):
        t = " ".join(t.replace("const", " ").split())
        base, stars = t.replace("*", "").strip(), t.count("*")
        if stars == 0:
            return scalars[base]
        if ret and base == "char":
            return ctypes.c_char_p
        if stars == 2:
            return ctypes.POINTER(ctypes.c_void_p)
        return ctypes.POINTER(_cabi.structs[base]) if base in _cabi.structs else ctypes.c_void_p

    seen = {}
    for ret, name, args in re.findall(r"\*/ extern (.*?)\b(afft_\w+) \((.*)\);", _gcc('#include "afft_hip.h"\n')):
        seen[name] = ([] if args == "void" else [want(a) for a in args.split(",")], want(ret, ret=True))
    assert len(seen) >= 77
    assert sorted(seen) == built_lib.EXPORTS
    sigs = dict(built_lib._SIGS, afft_last_error=_cabi.protos["afft_last_error"])
    for name, (args, res) in seen.items():
        have_args, have_res = sigs[name]
        assert len(have_args) == len(args), name
        for i, (h, w) in enumerate(zip(have_args, args)):
            assert h is w, (name, i, h, w)
        assert have_res is res, (name, have_res, res)
    assert any(ctypes.c_int64 in a for a, _ in seen.values()) and ctypes.c_int64 is not ctypes.c_int32      # the comparison can tell widths apart


def test_constants_match_the_compiler(built_lib):
    from afft_amd import _cabi
    names = sorted(_cabi.consts)
    assert len(names) >= 26
    body = "".join(f'printf("%lld\\n", (long long)({n}));' for n in names)
    got = _gcc(f'#include <stdio.h>\n#include "afft_hip.h"\nint main(){{ {body} return 0; }}\n', run=True).split()
    assert [int(v) for v in got] == [_cabi.consts[n] for n in names]
    hdr = open(os.path.join(ROOT, "include", "afft_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    mentioned = set(re.findall(r"\b(AFFT_[A-Z0-9_]+)\s*=", hdr)) | set(re.findall(r"#define\s+(AFFT_[A-Z0-9_]+)[ \t]+\S", hdr))
    assert mentioned == set(names)                       # the reader missed none
    for n in names:
        assert getattr(built_lib, n[len("AFFT_"):]) == _cabi.consts[n]


def test_public_names_keep_their_meaning(built_lib):
    """the names other modules import from _lib, with their values as they were written by hand: a rename in the header cannot
    silently move a Python name"""
    frozen = dict(F32=0, BF16=1, F16=2, GEMM_WS_HEADER=4096, ADAM_DECOUPLED=1,
                  ACT_NONE=0, ACT_GELU_ERF=1, ACT_GELU_TANH=2, ACT_DGELU_ERF=3, ACT_DGELU_TANH=4, ACT_RELU=5, ACT_SIGMOID_GATE=6,
                  MASK_NONE=0, MASK_DIAG=1, MASK_CAUSAL=2, MASK_BLOCKCAUSAL=3, K_ATTN_FWD=1, K_ATTN_BWD=2, K_LN_FWD=3, K_LN_BWD=4,
                  SGD_FIRST_STEP=1, SGD_PLAIN_MOMENTUM=2, F16X2_ONE_PASS_1=4, F16X2_ONE_PASS_2=8, F16X2_ONE_PASS_ATTN=16)
    for name, value in frozen.items():
        assert getattr(built_lib, name) == value, name
    L = built_lib
    assert (L.i32, L.i64, L.f32, L.vp, L.u32) == (ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_uint32)
    assert L.fp is ctypes.POINTER(ctypes.c_float) and L.SgdP is ctypes.POINTER(L.SgdFused) and L.DropP is ctypes.POINTER(L.Dropout)
    for name in ("GemmDesc", "Dropout", "SgdFused", "AttnSublayer", "MLPSublayer", "CrossAttnSublayer", "GemmTraceRec", "KernelTraceRec"):
        assert issubclass(getattr(L, name), ctypes.Structure) and getattr(L, name).__name__ == name
    assert [f[0] for f in L.Dropout._fields_] == ["p", "key", "path_p", "path_key", "path_group"]
    assert dict(L.GemmDesc._fields_)["drop"] is L.Dropout and dict(L.GemmDesc._fields_)["sgd"] is L.SgdP
    assert "afft_last_error" in L.EXPORTS and "afft_last_error" not in L._SIGS and L.EXPORTS == sorted(L.EXPORTS)
    assert callable(L.lib) and callable(L.check) and L.LIB_PATH.endswith(".so")
    from afft_amd import parallel, runtime
    assert runtime.one_pass_flags(False, 1 << 20, "fc1", "fc2") in (0, 4, 8, 12)
    opt = parallel.FusedSGD.__new__(parallel.FusedSGD)
    opt.steps, opt.nesterov = 0, False
    assert opt.flags() == 3
    opt.steps, opt.nesterov = 1, True
    assert opt.flags() == 0


@pytest.mark.parametrize("what,text", [
    ("unknown scalar type", "int afft_f(size_t n, void* stream);"),
    ("function-pointer argument", "int afft_f(void (*cb)(int), void* stream);"),
    ("array field", "typedef struct { float a[4]; } afft_x_t;"),
    ("bit-field", "typedef struct { int32_t a : 3; } afft_x_t;"),
    ("unnamed argument", "int afft_f(int32_t, void* stream);"),
    ("struct by value before its definition", "typedef struct { afft_y_t y; } afft_x_t;"),
    ("pointer to an unknown type", "int afft_f(const afft_y_t* y);"),
    ("computed constant", "enum { AFFT_A = 1 << 2 };"),
    ("macro with arguments", "#define AFFT_M(x) 1"),
    ("stray text", "int afft_f(void* stream); static int x;"),
])
def test_reader_refuses_what_it_does_not_know(what, text):
    from afft_amd import _cabi
    with pytest.raises(_cabi.HeaderError, match=r"afft_hip\.h:3: "):
        _cabi.parse("/* two lines\n   of comment */\n" + text + "\n")


def test_reader_reads_the_grammar_and_nothing_from_comments():
    from afft_amd import _cabi
    consts, structs, protos = _cabi.parse('''
/* int afft_foo(void* p); is only talked about here */      // and afft_bar(int x); here
enum { AFFT_A = 1, AFFT_B = -2 };
#define AFFT_C 7      /* with a comment */
typedef struct { float p; uint32_t key; } afft_in_t;
typedef struct { int64_t a_rs, a_cs; const float* x; afft_in_t in; const struct afft_late* late; const afft_in_t* q, * r; } afft_out_t;
typedef struct afft_late { void* p; } afft_late_t;
const char* afft_name(void);
int64_t afft_f(const afft_out_t* o, const float* const* xs, const uint8_t* keep, int n,
               uint32_t key, void* stream);
''')
    assert consts == {"AFFT_A": 1, "AFFT_B": -2, "AFFT_C": 7}
    assert list(structs) == ["afft_in_t", "afft_out_t", "afft_late_t"]
    In, Out, Late = structs.values()
    assert Out._fields_ == [("a_rs", ctypes.c_int64), ("a_cs", ctypes.c_int64), ("x", ctypes.c_void_p), ("in", In),
                            ("late", ctypes.POINTER(Late)), ("q", ctypes.POINTER(In)), ("r", ctypes.POINTER(In))]
    assert protos == {"afft_name": ([], ctypes.c_char_p),
                      "afft_f": ([ctypes.POINTER(Out), ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32,
                                  ctypes.c_void_p], ctypes.c_int64)}


def test_stale_library_is_refused(built_lib, monkeypatch, tmp_path):
    """a header beside the library that differs from the parsed one: lib() refuses the pair; no header there: it loads as before"""
    so = tmp_path / "libafft_hip.so"
    os.symlink(os.path.abspath(built_lib.LIB_PATH), so)             # the same file: the loader maps it once
    monkeypatch.setattr(built_lib, "LIB_PATH", str(so))
    monkeypatch.setattr(built_lib, "_lib", None)
    assert built_lib.lib().afft_version() >= 1                      # no header beside it (an AFFT_LIB tuning build)
    monkeypatch.setattr(built_lib, "_lib", None)
    hdr = open(os.path.join(ROOT, "include", "afft_hip.h"), "rb").read()
    (tmp_path / "afft_hip.h").write_bytes(hdr)
    assert built_lib.lib().afft_version() >= 1                      # the same header
    monkeypatch.setattr(built_lib, "_lib", None)
    (tmp_path / "afft_hip.h").write_bytes(hdr + b"\n")
    with pytest.raises(RuntimeError, match=r"stale.*make -C afft_amd/csrc"):
        built_lib.lib()


def test_built_library_carries_its_header(built_lib):
    beside = os.path.join(os.path.dirname(built_lib.LIB_PATH), "afft_hip.h")
    if os.environ.get("AFFT_LIB") or not os.path.exists(beside):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "afft_amd", "csrc"), "-j4"])
        beside = os.path.join(ROOT, "afft_amd", "lib", "afft_hip.h")
    assert open(beside, "rb").read() == open(os.path.join(ROOT, "include", "afft_hip.h"), "rb").read()


def test_call_sites_still_convert(built_lib):
    """from_param of the derived argtypes (and assignment to the derived fields) on the kinds of object that ops.py, functional.py and
    parallel.py pass at those positions: None, an int address, byref / pointer of a structure, host arrays, trace-record arrays"""
    L, S = built_lib, built_lib._SIGS
    drop, sgd, gemm = L.Dropout(), L.SgdFused(), L.GemmDesc()
    vps, i64s, f32s, i32s = (ctypes.c_void_p * 3)(), (ctypes.c_int64 * 3)(), (ctypes.c_float * 3)(), (ctypes.c_int32 * 3)()
    sites = [(n, i, [None, 0x7F0000001000]) for n, (args, _) in S.items() for i, a in enumerate(args) if a is ctypes.c_void_p]      # tensors, streams
    sites += [(n, i, [None, ctypes.byref(drop)]) for n, i in (("afft_layernorm_bwd", 14), ("afft_layernorm_bwd_take", 16), ("afft_cast", 10),
                                                           ("afft_act_bwd", 10))]
    sites += [("afft_gemm", 0, [ctypes.byref(gemm)]), ("afft_gemm_plan_for", 0, [ctypes.byref(gemm)]),
              ("afft_gemm_plan_for", 1, [ctypes.byref(L.GemmTraceRec())]),
              ("afft_gemm_trace_end", 0, [(L.GemmTraceRec * 4)()]), ("afft_kernel_trace_end", 0, [(L.KernelTraceRec * 4)()])]
    sites += [(f"afft_{k}_sublayer_{d}", 0, [ctypes.byref(T())]) for k, T in (("attn", L.AttnSublayer), ("mlp", L.MLPSublayer),
                                                                              ("cross_attn", L.CrossAttnSublayer)) for d in ("fwd", "bwd")]
    sites += [(n, i, [vps]) for n, i in (("afft_loss_reduce", 0), ("afft_loss_reduce_bwd", 0), ("afft_loss_reduce_bwd_ok", 0),
                                         ("afft_assemble_tokens", 0), ("afft_gather_frames", 7), ("afft_weighted_sum_fwd", 0),
                                         ("afft_weighted_sum_bwd", 0), ("afft_weighted_sum_bwd", 9))]
    sites += [(n, i, [i64s]) for n, i in (("afft_loss_reduce", 1), ("afft_loss_reduce_bwd", 1), ("afft_loss_reduce_bwd_ok", 1),
                                          ("afft_assemble_tokens", 1), ("afft_gather_frames", 8), ("afft_gather_frames", 9))]
    sites += [(n, 2, [f32s]) for n in ("afft_loss_reduce", "afft_loss_reduce_bwd", "afft_loss_reduce_bwd_ok")]
    sites += [("afft_gather_frames", i, [i32s]) for i in (10, 11, 12)]
    assert len(sites) > 300
    for name, i, objs in sites:
        for o in objs:
            S[name][0][i].from_param(o)
    gemm.sgd, gemm.drop, gemm.A, gemm.bias = ctypes.pointer(sgd), drop, 0x7F0000001000, None          # ops.gemm
    a, m, c = L.AttnSublayer(), L.MLPSublayer(), L.CrossAttnSublayer()
    for s, fields in ((a, ("sgd_w_qkv", "sgd_w_proj")), (m, ("sgd_w1", "sgd_w2")), (c, ("sgd_w_q", "sgd_w_k", "sgd_w_v", "sgd_w_proj"))):
        for f in fields:
            setattr(s, f, ctypes.pointer(sgd))                                                          # functional: the fused optimizer
        s.up_drop, s.out_drop, s.x, s.dx_bf16 = ctypes.pointer(drop), drop, 0x7F0000001000, None
    sgd.p, sgd.p_f16, sgd.ok, sgd.first_step = 0x7F0000001000, 0x7F0000001000 + 2, None, L.SGD_PLAIN_MOMENTUM      # parallel
