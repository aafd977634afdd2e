"""CPU: the float64 reference of the cached attention step (tests/attention_step_double.py) is right.  On four small shapes, one with
dropout, the rectangular attention_double.reference() under the step's mask and keep-scale equals float64 torch autograd of
((softmax over the visible keys) o M) V -- the _reference of test_attention_step_bwd_gpu.py -- to 1e-12, and the gradient-cache rule
equals that test's want_new / += arithmetic.  The magnitude sums bound their values and are what the values are on all-positive
inputs.  The keep-scale is drawn on the index attention_step.hip draws on."""
import numpy as np
import pytest
import torch

import kernel_doubles as kd
from attention_double import rows
from attention_step_cases import case
from attention_step_double import cache_rows, case_inputs, case_reference, step_banned, step_keep_scale, step_reference
from test_attention_step_bwd_gpu import _reference as autograd_reference

SMALL = [case("s_Lq1_Lk1", "bwd", "f32", 2, 2, 4, 1, 0, 3),
         case("s_Lq3_Lk7", "bwd", "f32", 2, 3, 16, 3, 4, 9),
         case("s_Lq6_prefill", "bwd", "bf16", 1, 2, 4, 6, 0),
         case("s_Lq5_Lk9_drop", "bwd", "f32", 2, 2, 16, 5, 4, 10, drop_p=0.3)]
TOL = 1e-12      # (hd is 4 or 16: hd ** -0.5 is the same number as a C float and as a double)


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and float(np.abs(a - b).max(initial=0.0)) <= TOL * max(1.0, float(np.abs(b).max(initial=0.0)))


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.name)
def test_reference_equals_float64_autograd_and_the_write_rule(c):
    ins = case_inputs(c)
    ref, keep = case_reference(c, ins)
    shape = (c.nseq, c.H, c.hd, c.Lq, c.Lk, c.cap)
    caches = torch.full((2, c.nseq, c.cap, c.d), float("nan"), dtype=ins["old"].dtype)
    caches[:, :, :c.past] = ins["old"]
    caches[0, :, c.past:c.Lk] = ins["k_new"].reshape(c.nseq, c.Lq, c.d)
    caches[1, :, c.past:c.Lk] = ins["v_new"].reshape(c.nseq, c.Lq, c.d)
    M = None
    if c.drop_p > 0:
        M = torch.from_numpy(np.where(keep, 1.0 / (1.0 - float(np.float32(c.drop_p))), 0.0))
        assert keep.any() and not keep.all()
    p, out, dq, ck, cv = autograd_reference(shape, ins["q"], ins["dout"], caches, M)
    assert _close(ref["probs"][0], p.numpy())
    assert _close(rows(ref["out"][0]), out.numpy()) and _close(rows(ref["dq"][0]), dq.numpy())
    # the gradient-cache rule, as test_attention_step_bwd_gpu.py::_check writes it
    g = ins["g"]
    for i, (cx, new, old) in enumerate(((ck, "dk_new", "gk"), (cv, "dv_new", "gv"))):
        want_new = (g[i, :, c.past:c.Lk].double() + cx[:, c.past:]).reshape(c.nseq * c.Lq, c.d)
        assert _close(rows(ref[new][0]), want_new.numpy())
        assert _close(cache_rows(ref[old][0]), (g[i, :, :c.past].double() + cx[:, :c.past]).numpy())
    for kind, (val, S) in ref.items():
        assert val.shape == S.shape and bool((np.abs(val) <= S * (1 + 1e-12)).all()), kind
    hidden = np.broadcast_to(step_banned(c.Lq, c.past), ref["probs"][0].shape)
    assert float(np.abs(ref["probs"][0][hidden]).sum()) == 0.0 and float(ref["probs"][1][hidden].sum()) == 0.0


def test_magnitude_sums_are_the_values_on_positive_inputs():
    """with every operand positive, no dropout and a zero softmax gradient out of reach, out / dv / dk_new of positive terms ARE their sums"""
    rng = np.random.RandomState(3)
    nseq, H, hd, Lq, past = 2, 2, 5, 3, 4
    q, do = rng.random_sample((2, nseq, H, Lq, hd)) + 0.1
    k, v, gk, gv = rng.random_sample((4, nseq, H, past + Lq, hd)) + 0.1
    r = step_reference(q, k, v, do, hd ** -0.5, past, np.ones((nseq, H, Lq, past + Lq)), gk, gv)
    for kind in ("out", "dv_new", "gv"):
        assert _close(r[kind][0], r[kind][1]), kind
    assert r["dk_new"][0].shape == (nseq, H, Lq, hd) and r["gk"][0].shape == (nseq, H, past, hd)


def test_keep_scale_is_drawn_on_the_steps_index():
    nseq, H, Lq, Lk, p, key = 2, 3, 4, 9, 0.3, 777
    ks, keep = step_keep_scale(nseq, H, Lq, Lk, p, key)
    assert ks.shape == keep.shape == (nseq, H, Lq, Lk)
    for seq, h, i, j in ((0, 0, 0, 0), (1, 2, 3, 8), (1, 0, 2, 5), (0, 2, 1, 7)):
        idx = ((seq * H + h) * Lq + i) * Lk + j
        assert bool(keep[seq, h, i, j]) == bool(kd.drop_keep(key, np.array([idx]), p)[0])
    inv = 1.0 / (1.0 - float(np.float32(p)))
    assert set(np.unique(ks)) == {0.0, inv} and inv != 1.0 / (1.0 - p)      # p is the C float, not the double
    ones, none = step_keep_scale(nseq, H, Lq, Lk, 0.0, key)
    assert none is None and bool((ones == 1.0).all())
