"""CPU: the cached attention step (csrc/attention_step.hip) as far as it goes without a device -- the export and its derived binding,
the step plan (csrc/attn_plan.h plan_attention_step) restated here and compared with afft_attention_step_plan_for, and the argument
checks, which run before anything touches a device (dummy pointers, never dereferenced)."""
import ctypes as C
import itertools

import pytest

from afft_amd import _cabi, _lib

STEP_QT = 4      # query rows of one workgroup


def expected(dtype, Lq, Lk, hd, ok):
    """(family, p0, LDS bytes, workgroups per (sequence, head)), or None: refused"""
    if not (1 <= Lq <= Lk <= 512 and 1 <= hd <= 1024):
        return None
    vec = 4 if dtype == _lib.F32 else 8                       # elements of a 16-byte load
    rows = min(Lq, STEP_QT)
    lds = 4 * rows * ((Lk + 3) // 4 * 4 + 3 * ((hd + 7) // 8 * 8))      # fp32 scores [rows][Lk up to 4] + 3 waves' partial P V rows
    return (11, 1 if (ok and hd % vec == 0) else 0, lds, (Lq + STEP_QT - 1) // STEP_QT)


def asked(dtype, Lq, Lk, hd, ok):
    o = (C.c_int64 * 2)()
    r = _lib.lib().afft_attention_step_plan_for(dtype, Lq, Lk, hd, ok, o)
    return None if r < 0 else (r // 10000, r % 10000 // 10, o[0], o[1])


def test_export_exists_and_parses():
    args, res = _cabi.protos["afft_attention_step_fwd"]
    assert res is C.c_int and len(args) == 22
    assert args[:10] == [C.c_void_p, C.c_int64] * 3 + [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]
    assert args[10:17] == [C.c_int32] * 7 and args[17] is C.c_float and args[-1] is C.c_void_p
    assert "afft_attention_step_fwd" in _lib.EXPORTS and "afft_attention_step_plan_for" in _lib.EXPORTS
    assert _lib.lib().afft_attention_step_fwd.argtypes == args      # the built library carries it


@pytest.mark.parametrize("dtype", [_lib.F32, _lib.BF16])
def test_step_plan_is_the_stated_rule(dtype):
    grid = itertools.product((1, 2, 16, 32), (1, 17, 128, 129, 512, 513), (1, 8, 24, 64, 512, 520, 1021, 1024), (1, 0))
    bad = [(a, asked(dtype, *a), expected(dtype, *a)) for a in grid if asked(dtype, *a) != expected(dtype, *a)]
    assert not bad, bad[:5]
    assert asked(dtype, 1, 19, 1025, 1) is None and asked(dtype, 0, 4, 64, 1) is None
    assert asked(dtype, 3, 19, 30, 1) == expected(dtype, 3, 19, 30, 1)      # hd off the 16-byte grid: element loads
    assert asked(_lib.F16, 1, 4, 64, 1) is None


def test_directions_0_to_2_keep_their_answers():
    """the step has a query of its own: afft_attention_plan_for still knows three directions"""
    assert _lib.lib().afft_attention_plan_for(3, _lib.BF16, 16, 64, 0, 0, 1) < 0
    assert _lib.lib().afft_attention_plan_for(0, _lib.BF16, 16, 64, 0, 0, 1) == 20010


def _call(q=4096, kc=4096, vc=4096, Lq=1, Lk=4, cap=8, H=2, hd=64, dtype=None, ldc=128, cache_seq=None, nseq=2):
    """afft_attention_step_fwd with dummy pointers: only a call that the host check refuses is made (one that passed would launch)"""
    dtype = _lib.BF16 if dtype is None else dtype
    cache_seq = cap * ldc if cache_seq is None else cache_seq
    rc = _lib.lib().afft_attention_step_fwd(q, 384, 4096, 384, 4096, 384, kc, vc, ldc, cache_seq, dtype, nseq, Lq, Lk, cap, H, hd, 0.125,
                                            4096, 128, None, None)
    return rc, _lib.lib().afft_last_error().decode()


@pytest.mark.parametrize("kw,text", [
    (dict(Lq=5, Lk=4), "5 new rows against 4 keys"),
    (dict(Lq=0, Lk=4), "0 new rows against 4 keys"),
    (dict(Lk=9, cap=8), "9 keys do not fit a cache of 8 rows"),
    (dict(Lk=513, cap=600), "sequence length 513 outside 1..512"),
    (dict(kc=None), "null pointer"),
    (dict(vc=None), "null pointer"),
    (dict(q=None), "null pointer"),
    (dict(hd=1025, ldc=4096), "head dimension 1025 outside 1..1024"),
    (dict(dtype=2), "bad dtype 2"),
    (dict(ldc=64), "a row pitch is below H * hd = 128"),
    (dict(cache_seq=512), "cache sequence stride 512 does not hold 8 rows of pitch 128"),
    (dict(nseq=-1), "bad nseq -1"),
])
def test_refused_arguments_are_host_errors(kw, text):
    rc, msg = _call(**kw)
    assert rc != 0 and text in msg, (rc, msg)
    assert msg.startswith("attention_step: ")


def test_no_sequences_is_a_no_op():
    assert _call(nseq=0)[0] == 0
