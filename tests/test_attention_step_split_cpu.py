"""CPU: the cached attention step in the operand form of the 'fp16x2' forward (afft_attention_step_fwd_split, csrc/attention_step.hip) and
the composite entry around it (afft_attn_step_sublayer_fwd, csrc/sublayer.hip), as far as they go without a device: the exports and their
derived bindings, the plan (csrc/attn_plan.h plan_attention_step, family 13) restated here and compared with
afft_attention_step_split_plan_for, and the argument checks, which run before anything touches a device (dummy pointers, never
dereferenced)."""
import ctypes as C
import itertools

import pytest

from afft_amd import _cabi, _lib

STEP_QT = 4      # query rows of one workgroup


def test_exports_exist_and_parse():
    args, res = _cabi.protos["afft_attention_step_fwd_split"]
    assert res is C.c_int and len(args) == 23
    assert args[:7] == [C.c_void_p, C.c_int64] * 3 + [C.c_int64]                                  # q, k_new, v_new with pitches; in_lo
    assert args[7:11] == [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]                           # the caches
    assert args[11:17] == [C.c_int32] * 6 and args[17] is C.c_float
    assert args[18:] == [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]                # out_hi, ldo, out_lo, probs, stream
    args, res = _cabi.protos["afft_attention_step_split_plan_for"]
    assert res is C.c_int and args == [C.c_int32] * 6 + [C.c_void_p]
    args, res = _cabi.protos["afft_attn_step_sublayer_fwd"]
    assert res is C.c_int and args == [C.POINTER(_cabi.structs["afft_attn_step_sublayer_t"]), C.c_void_p]
    for name in ("afft_attention_step_fwd_split", "afft_attention_step_split_plan_for", "afft_attn_step_sublayer_fwd"):
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib(), name).argtypes == _cabi.protos[name][0]      # the built library carries it
    S = _lib.AttnStepSublayer
    assert S is _cabi.structs["afft_attn_step_sublayer_t"] and S.__name__ == "AttnStepSublayer"
    fields = dict(S._fields_)
    for name in ("rows", "d", "Lq", "Lk", "cap", "H", "conv1d", "f16x2"):
        assert fields[name] is C.c_int32, name
    for name in ("ldw_qkv", "ldw_proj", "ldc", "cache_seq", "gemm_ws_bytes"):
        assert fields[name] is C.c_int64, name
    assert not {"xn_b", "qkv_b", "ao_b", "mean", "rstd", "out_drop", "p_attn"} & set(fields)      # inference: no twins, nothing saved, no dropout


def expected(Lq, Lk, hd, ok):
    """(family, p0, LDS bytes, workgroups per (sequence, head)), or None: refused"""
    if not (1 <= Lq <= Lk <= 512 and 1 <= hd <= 1024):
        return None
    rows = min(Lq, STEP_QT)
    lds = 4 * rows * ((Lk + 3) // 4 * 4 + 3 * ((hd + 7) // 8 * 8))      # the dense step's carve: fp32 scores + 3 waves' partial P V rows
    return (13, 1 if (ok and hd % 8 == 0) else 0, lds, (Lq + STEP_QT - 1) // STEP_QT)


def asked(Lq, Lk, hd, ok, in_lo=1, out_lo=1):
    o = (C.c_int64 * 2)()
    r = _lib.lib().afft_attention_step_split_plan_for(Lq, Lk, hd, in_lo, out_lo, ok, o)
    return None if r < 0 else (r // 10000, r % 10000 // 10, o[0], o[1])


def test_split_plan_is_the_stated_rule():
    grid = itertools.product((1, 4, 5, 16, 37), (1, 17, 37, 128, 512, 513), (20, 24, 64, 512, 1024), (1, 0))
    bad = [(a, asked(*a), expected(*a)) for a in grid if asked(*a) != expected(*a)]
    assert not bad, bad[:5]
    for planes in itertools.product((0, 1), (0, 1)):      # which lo planes there are changes no launch parameter
        assert asked(1, 19, 512, 1, *planes) == expected(1, 19, 512, 1)
    assert asked(1, 19, 1025, 1) is None and asked(1, 19, 0, 1) is None and asked(0, 4, 64, 1) is None and asked(5, 4, 64, 1) is None
    assert asked(3, 19, 20, 1) == expected(3, 19, 20, 1)      # hd off the 16-byte grid: element accesses
    assert asked(1, 512, 64, 1)[2] == 4 * (512 + 3 * 64)


def test_the_dense_plan_query_keeps_its_answers():
    o = (C.c_int64 * 2)()
    lib = _lib.lib()
    assert lib.afft_attention_step_plan_for(_lib.F32, 1, 19, 512, 1, o) == 110010 and lib.afft_attention_step_plan_for(_lib.BF16, 4, 4, 24, 1, o) == 110010
    assert lib.afft_attention_step_plan_for(_lib.F16, 1, 4, 64, 1, o) < 0      # planes have a query of their own


def _call(q=4096, kc=4096, vc=4096, out=4096, Lq=1, Lk=4, cap=8, H=2, hd=64, ldq=384, ldc=128, cache_seq=None, nseq=2, in_lo=0, out_lo=0, ldo=128):
    """afft_attention_step_fwd_split with dummy pointers: only a call that the host check refuses is made (one that passed would launch)"""
    cache_seq = cap * ldc if cache_seq is None else cache_seq
    rc = _lib.lib().afft_attention_step_fwd_split(q, ldq, 4096, 384, 4096, 384, in_lo, kc, vc, ldc, cache_seq, nseq, Lq, Lk, cap, H, hd, 0.125,
                                                  out, ldo, out_lo, None, None)
    return rc, _lib.lib().afft_last_error().decode()


@pytest.mark.parametrize("kw,text", [
    (dict(Lk=513, cap=600), "sequence length 513 outside 1..512"),
    (dict(Lq=5, Lk=4), "5 new rows against 4 keys"),
    (dict(Lq=0, Lk=4), "0 new rows against 4 keys"),
    (dict(hd=0), "head dimension 0 outside 1..1024"),
    (dict(hd=1025, ldc=4096, ldq=8192, ldo=4096), "head dimension 1025 outside 1..1024"),
    (dict(ldq=64), "a row pitch is below H * hd = 128"),
    (dict(ldo=127), "a row pitch is below H * hd = 128"),
    (dict(ldc=64), "a row pitch is below H * hd = 128"),
    (dict(Lk=9, cap=8), "9 keys do not fit a cache of 8 rows"),
    (dict(cache_seq=512), "cache sequence stride 512 does not hold 8 rows of pitch 128"),
    (dict(kc=None), "null pointer"),
    (dict(out=None), "null pointer"),
    (dict(nseq=-1), "bad nseq -1"),
    # the lo offsets (include/afft_hip.h): 0, or behind the last element of the hi plane -- (nseq * Lq - 1) * pitch + H * hd
    (dict(in_lo=-8), "in_lo -8 lies inside the hi plane"),
    (dict(in_lo=128), "in_lo 128 lies inside the hi plane"),                      # the k block of the same rows: inside q's plane
    (dict(in_lo=384 + 127), "in_lo 511 lies inside the hi plane (0: no lo plane, else at least (nseq * Lq - 1) * pitch + H * hd = 512)"),
    (dict(out_lo=-1), "out_lo -1 lies inside the hi plane"),
    (dict(out_lo=128), "out_lo 128 lies inside the hi plane"),                    # the next row of out
    (dict(out_lo=255), "out_lo 255 lies inside the hi plane (0: no lo plane, else at least (nseq * Lq - 1) * pitch + H * hd = 256)"),
    (dict(q=4097), "fp16 planes must be 2-byte aligned"),
    (dict(kc=4098), "the fp32 caches and probs 4-byte aligned"),
])
def test_refused_arguments_are_host_errors(kw, text):
    rc, msg = _call(**kw)
    assert rc != 0 and text in msg, (rc, msg)
    assert msg.startswith("attention_step_split: ")


def test_no_sequences_is_a_no_op():
    assert _call(nseq=0)[0] == 0
    assert _call(nseq=0, in_lo=0, out_lo=0)[0] == 0


def _step(**kw):
    """afft_attn_step_sublayer_fwd with dummy pointers, refused before its first launch"""
    s = _lib.AttnStepSublayer()
    s.rows, s.d, s.Lq, s.Lk, s.cap, s.H, s.conv1d, s.f16x2, s.eps, s.scale = 2, 128, 1, 4, 8, 2, 1, 1, 1e-5, 0.125
    for f in ("x", "w_qkv", "w_proj", "xn", "qkv", "ao", "k_cache", "v_cache", "y"):
        setattr(s, f, 4096)
    s.ldw_qkv, s.ldw_proj, s.ldc, s.cache_seq = 384, 128, 128, 1024
    for k, v in kw.items():
        setattr(s, k, v)
    rc = _lib.lib().afft_attn_step_sublayer_fwd(C.byref(s), None)
    return rc, _lib.lib().afft_last_error().decode()


@pytest.mark.parametrize("kw,text", [
    (dict(k_cache=None), "attn_step_sublayer_fwd: null pointer"),
    (dict(ao=None), "attn_step_sublayer_fwd: null pointer"),
    (dict(d=96), "attn_step_sublayer_fwd: bad geometry"),
    (dict(rows=3, Lq=2), "attn_step_sublayer_fwd: bad geometry"),
    (dict(f16x2=0), "f16x2 must be 1 | AFFT_F16X2_ONE_PASS_*"),
    (dict(f16x2=2), "f16x2 must be 1 | AFFT_F16X2_ONE_PASS_*"),                    # the e4m3 lo planes: refused, as conv1d refuses them
    (dict(f16x2=2 | _lib.F16X2_ONE_PASS_1 | _lib.F16X2_ONE_PASS_2), "f16x2 must be 1 | AFFT_F16X2_ONE_PASS_*"),
])
def test_composite_refuses_before_any_launch(kw, text):
    rc, msg = _step(**kw)
    assert rc != 0 and text in msg, (rc, msg)
