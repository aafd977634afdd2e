"""Every case of tests/attention_step_cases.py -- every instantiation of the kernels of csrc/attention_step.hip: the cached attention
step forward (Dense fp32 / bf16 with and without dropout, the fp16 planes of the 'fp16x2' forward) and its backward with the gradient
caches -- ELEMENTWISE against float64 (attention_step_double.step_reference(), which is attention_double.reference() under the step's
mask and keep-scale plus the write rule of the gradient caches).

Frames.  Every operand (q, k_new, v_new, dout, cache rows < Lk) sits in a NaN frame of its own; cache rows >= Lk, every pad column, the
rows between two sequences and a lo plane the call does not name are NaN.  Every result (out, probs, dq, dk_new, dv_new) sits in a
sentinel frame.  After the call the frames are as they were and every result element is finite and not the sentinel.

Elementwise.  |got - ref| <= c * u * S for every element of out, probs, dq, dk_new, dv_new and of rows < past of both gradient caches, S
the magnitude sum of the reference; u = 2^-24 for every fp32-storage output, every probs and the fp32 gradient-cache rows in both
storages (the inputs are storage-exact and accumulation is fp32), 2^-9 for bf16 out, dq, dk_new, dv_new.  Masked probs are exactly 0.  The
backward runs twice: on the kernel's own probs, and on the float64 probabilities rounded to fp32, both held to the same bars.
Planes, per element, with C the fp32 bar of out (the terms of test_attention_step_split_gpu.py's docstring, taken at the element):
    hi + lo                       within C * 2^-24 * S + 2^-21 |ref| + 2^-24
    hi alone, the hi-only form    within C * 2^-24 * S + 2^-11 |ref| + 2^-24
and the appended cache rows are exactly float(hi) + float(lo).

Exact facts.  The append is bit for bit in Dense; the past rows of the key / value caches are untouched in forward and backward; rows
[past, Lk) of the gradient caches keep their bits; a second run gives equal bits for every output; fwd_drop with p = 0 gives the bits of
fwd.  Dropped entries contribute nothing: the reference multiplies them by 0, and a head whose row lost every visible key must be 0.0.

The relative-L2 bars of test_attention_step_gpu.py, test_attention_step_bwd_gpu.py and test_attention_step_split_gpu.py are kept as a
second assertion.

c: twice the worst |got - ref| / (u S) measured over the table on an MI355X, rounded up to a power of two (MEASURED: the worst per
storage and output kind, gradients over both probs sources).  The kernels are deterministic: the margin is for other seeds and compiler
versions.  Every bar is asserted to stay within a ceiling that is a condition, not a measurement: CEILING["generic_f32"] /
CEILING["generic_bf16"] of test_attention_long_cases_gpu.py (at most 512 keys there as here); dk_new and the key gradient cache take
the dk ceiling, dv_new and the value gradient cache the dv ceiling; what is held to u = 2^-24 (the gradient-cache rows of both storages,
everything of the planes) takes the fp32 ceilings.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from attention_double import (PAD_ROWS, SENTINEL, dev, flat_framed, flat_untouched, frame_untouched, framed, rows, worst_ratio)  # noqa: E402
from attention_step_cases import CASES  # noqa: E402
from attention_step_double import cache_rows, case_inputs, case_reference, step_banned  # noqa: E402
from helpers import rel_l2  # noqa: E402
from test_attention_long_cases_gpu import CEILING as LONG_CEILING  # noqa: E402

pytestmark = pytest.mark.gpu

U32, U16 = 2.0 ** -24, 2.0 ** -9
NAN = float("nan")

# worst |got - ref| / (u S) over the table, MI355X: storage -> kind -> value (gk / gv: rows < past of the gradient caches, u = 2^-24)
MEASURED = {
    "f32": dict(out=5.04, probs=2.11, dq=1.71, dk_new=1.50, dv_new=4.91, gk=0.996, gv=6.17),
    "bf16": dict(out=1.82, probs=2.05, dq=1.11, dk_new=1.94, dv_new=1.99, gk=0.970, gv=7.44),
    "planes": dict(out=1.40, probs=1.40),
}
# The cases that set them.  f32: out f_hd64_odd_Lq8_Lk10_pitch; probs, dq, dk_new f_hd1_Lq16_Lk18_drop (hd = 1: a score is ONE product, its
# whole rounding shows); dv_new f_hd1021_Lq6_Lk128 and gv f_hd1024_Lq4_Lk127, both on the kernel's own probs (1.6 and 2.6 on the float64
# probabilities: P' carries the forward's rounding of p, which the magnitude sum of P'^T dO does not know); gk f_hd1024_Lq1_Lk512.
# bf16: out b_hd40_Lq6_prefill_drop0; probs, dq b_hd1_Lq10_prefill_drop (one bf16 rounding of a one-term result reads as up to 2 in
# units of 2^-9, see test_attention_short_gpu.py); dk_new b_hd1021_Lq5_Lk129; dv_new, gv b_hd1023_Lq11_Lk127_drop (gv on its own probs;
# 3.0 on the float64 ones); gk b_hd1024_Lq3_Lk512.  planes: out p_hd64_odd_Lq7_Lk10 (the larger of hi + lo and hi alone); probs
# p_hd1_Lq3_prefill.  No maximum is set by hd = 1024 as such: the ceilings below stand as they are, unscaled.
C = {s: {kind: 2.0 ** math.ceil(math.log2(2.0 * w)) for kind, w in kinds.items()} for s, kinds in MEASURED.items()}
_F, _B = LONG_CEILING["generic_f32"], LONG_CEILING["generic_bf16"]
CEILING = {"f32": dict(out=_F["out"], probs=_F["probs"], dq=_F["dq"], dk_new=_F["dk"], dv_new=_F["dv"], gk=_F["dk"], gv=_F["dv"]),
           "bf16": dict(out=_B["out"], probs=_B["probs"], dq=_B["dq"], dk_new=_B["dk"], dv_new=_B["dv"], gk=_F["dk"], gv=_F["dv"]),
           "planes": dict(out=_F["out"], probs=_F["probs"])}
assert all(C[s][k] <= CEILING[s][k] for s in C for k in C[s]), (C, CEILING)
# relative L2, as the three step tests hold them; SPLIT_BAR: the fp32 term of the planes' per-tensor bound
L2 = {"f32": dict(out=2e-5, probs=2e-5, grads=3e-5), "bf16": dict(out=1e-2, probs=2e-3, grads=2e-2), "planes": dict(probs=2e-5)}
SPLIT_BAR = 2e-5

_SHARED = {}


def shared(c):
    """inputs and float64 reference of a case: made once per distinct problem, shared (the planes' forms), never modified"""
    key = (c.storage, c.nseq, c.H, c.hd, c.Lq, c.past, c.drop_p, c.key, c.in_lo)
    if key not in _SHARED:
        ins = case_inputs(c)
        _SHARED[key] = (ins, case_reference(c, ins)[0])
    return _SHARED[key]


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()]).cpu()


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def written(*ts):
    """no element is NaN, infinite or still the sentinel"""
    return all(bool(torch.isfinite(t.float()).all()) and not bool((t.float() == SENTINEL).any()) for t in ts)


def cache_framed(c, pad, xseq, dtype):
    """nseq sequences of (cap + xseq) rows of H * hd + pad columns between two more such blocks, all NaN -> (buffer, its [nseq, cap, d] view)"""
    buf = torch.full((c.nseq + 2, c.cap + xseq, c.d + c.frame_cols(pad)), NAN, dtype=dtype, device=dev())
    return buf, buf[1:c.nseq + 1, :c.cap, :c.d]


def cache_frame_is_nan(buf, c):
    """everything but rows < Lk, columns < d of the nseq sequences is NaN, and those are finite"""
    b = buf.float().cpu()
    inner = torch.zeros_like(b, dtype=torch.bool)
    inner[1:c.nseq + 1, :c.Lk, :c.d] = True
    return bool(torch.isnan(b[~inner]).all()) and bool(torch.isfinite(b[inner]).all())


def takes_16_bytes(c, views, pitches, vec):
    """the plan's condition for V on the buffers of a call: 16-byte aligned bases, pitches on the grid"""
    return all(v.data_ptr() % 16 == 0 for v in views) and all(p % vec == 0 for p in pitches)


def run_forward(c, ins, entry):
    """one forward call of case c through `entry` (fwd | fwd_drop | split) on fresh framed buffers -> the buffers and views"""
    from afft_amd import _lib, ops
    R, d, planes = c.nseq * c.Lq, c.d, c.storage == "planes"
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "planes": torch.float16}[c.storage]
    cdt = torch.float32 if planes else tdt
    pi = c.frame_cols(c.pad_in)
    r = {}
    for nm in ("q", "k_new", "v_new"):
        buf, view, dist = framed(R, d, NAN, tdt, pi, planes=2 if planes else 1)
        if planes:
            view.copy_(ins[nm + "_hi"])
            if c.in_lo:
                buf[1, PAD_ROWS:PAD_ROWS + R, :d].copy_(ins[nm + "_lo"])
        else:
            view.copy_(ins[nm])
        r[nm], r["in_lo"] = view, dist
    for i, nm in enumerate(("kc", "vc")):
        r[nm + "_buf"], r[nm] = cache_framed(c, c.pad_c, c.xseq, cdt)
        r[nm][:, :c.past].copy_(ins["old"][i])
    r["out_buf"], r["out"], r["out_lo"] = framed(R, d, SENTINEL, tdt, pi, planes=2 if planes else 1)
    r["probs_buf"], pflat = flat_framed(c.nseq * c.H * c.Lq * c.Lk)
    r["probs"] = pflat.view(c.nseq, c.H, c.Lq, c.Lk) if c.probs else None
    scale = c.hd ** -0.5
    views = [r[k] for k in ("q", "k_new", "v_new", "kc", "vc", "out")]
    pitches = [r[k].stride(0) for k in ("q", "k_new", "v_new", "out")] + ([r["in_lo"], r["out_lo"]] if planes else [])
    ok = takes_16_bytes(c, views, pitches, c.vec) and takes_16_bytes(c, [], [r["kc"].stride(1), r["kc"].stride(0)], 4 if planes else c.vec)
    assert c.hd % c.vec or ok == (not c.odd), (c.name, "the buffers do not have the alignment the case is written for")
    if entry == "split":
        ops.attention_step_split(r["q"], r["k_new"], r["v_new"], r["in_lo"] if c.in_lo else 0, r["kc"], r["vc"], c.nseq, c.Lq, c.Lk, c.H, c.hd,
                                 scale, r["out"], r["out_lo"] if c.out_lo else 0, r["probs"])
    elif entry == "fwd_drop":      # the _drop entry point itself, also at p = 0 (ops.attention_step takes the plain one there)
        rc = _lib.lib().afft_attention_step_fwd_drop(
            r["q"].data_ptr(), r["q"].stride(0), r["k_new"].data_ptr(), r["k_new"].stride(0), r["v_new"].data_ptr(), r["v_new"].stride(0),
            r["kc"].data_ptr(), r["vc"].data_ptr(), r["kc"].stride(1), r["kc"].stride(0), _lib.F32 if c.storage == "f32" else _lib.BF16, c.nseq,
            c.Lq, c.Lk, c.cap, c.H, c.hd, scale, float(c.drop_p), int(c.key), r["out"].data_ptr(), r["out"].stride(0), r["probs"].data_ptr(),
            torch.cuda.current_stream().cuda_stream)
        assert rc == 0, _lib.lib().afft_last_error().decode()
    else:
        ops.attention_step(r["q"], r["k_new"], r["v_new"], r["kc"], r["vc"], c.nseq, c.Lq, c.Lk, c.H, c.hd, scale, r["out"], r["probs"])
    torch.cuda.synchronize()
    r["results"] = [r["out_buf"], r["probs_buf"], r["kc_buf"], r["vc_buf"]]
    return r


def check_forward(c, ins, ref, f, ratios, l2, facts):
    R, d, planes = c.nseq * c.Lq, c.d, c.storage == "planes"
    o_ref, o_S = rows(ref["out"][0]), rows(ref["out"][1])
    ok = frame_untouched(f["out_buf"], R, d) and flat_untouched(f["probs_buf"])
    if planes:
        hi, lo = f["out"], f["out_buf"][1, PAD_ROWS:PAD_ROWS + R, :d]
        joined = hi.double() + lo.double() if c.out_lo else hi.double()
        tail = (2.0 ** -21 if c.out_lo else 2.0 ** -11) * np.abs(o_ref) + 2.0 ** -24
        ratios["out"] = max(worst_ratio(joined, o_ref, o_S, U32, floor=tail),
                            worst_ratio(hi, o_ref, o_S, U32, floor=2.0 ** -11 * np.abs(o_ref) + 2.0 ** -24))
        facts["fwd_written"] = written(hi, lo) if c.out_lo else (written(hi) and bool((f["out_buf"][1] == SENTINEL).all()))
        m = float(np.abs(o_ref).max())      # the per-tensor bound of test_attention_step_split_gpu.py
        l2["out_max"] = float(np.abs(joined.cpu().numpy() - o_ref).max()) / ((SPLIT_BAR + (2.0 ** -21 if c.out_lo else 2.0 ** -11)) * m)
        l2["hi_max"] = float(np.abs(hi.double().cpu().numpy() - o_ref).max()) / ((SPLIT_BAR + 2.0 ** -11) * m)
        new = [(ins[nm + "_hi"].float() + ins[nm + "_lo"].float()) if c.in_lo else ins[nm + "_hi"].float() for nm in ("k_new", "v_new")]
    else:
        ratios["out"] = worst_ratio(f["out"].float(), o_ref, o_S, U32 if c.storage == "f32" else U16)
        facts["fwd_written"] = written(f["out"])
        l2["out"] = rel_l2(f["out"].float().cpu(), torch.from_numpy(o_ref))
        new = [ins["k_new"], ins["v_new"]]
    if c.probs:
        ratios["probs"] = worst_ratio(f["probs"], ref["probs"][0], ref["probs"][1], U32)
        l2["probs"] = rel_l2(f["probs"].cpu(), torch.from_numpy(ref["probs"][0]))
        hidden = torch.from_numpy(np.broadcast_to(step_banned(c.Lq, c.past), ref["probs"][0].shape).copy())
        facts["masked_probs_zero"] = float(f["probs"].cpu()[hidden].abs().sum()) == 0.0
        facts["fwd_written"] = facts["fwd_written"] and written(f["probs"])
    else:
        facts["probs_not_written"] = bool((f["probs_buf"] == SENTINEL).all())
    # the caches: the past as it was, the new rows appended bit for bit (planes: exactly float(hi) + float(lo)), NaN everywhere else
    for i, nm in enumerate(("kc", "vc")):
        ok = ok and cache_frame_is_nan(f[nm + "_buf"], c)
        facts["past_untouched"] = facts.get("past_untouched", True) and torch.equal(bits(f[nm][:, :c.past]), bits(ins["old"][i]))
        facts["append_exact"] = facts.get("append_exact", True) and torch.equal(bits(f[nm][:, c.past:c.Lk]), bits(new[i].reshape(c.nseq, c.Lq, d)))
    facts["fwd_frames"] = ok


def run_backward(c, ins, f, probs):
    """one afft_attention_step_bwd call on the caches forward run `f` left, with `probs` [nseq, H, Lq, Lk] -> the buffers and views"""
    from afft_amd import ops
    R, d = c.nseq * c.Lq, c.d
    tdt = torch.float32 if c.storage == "f32" else torch.bfloat16
    pi = c.frame_cols(c.pad_in)
    r = {}
    _, r["dout"], _ = framed(R, d, NAN, tdt, pi)
    r["dout"].copy_(ins["dout"])
    for i, nm in enumerate(("gk", "gv")):
        r[nm + "_buf"], r[nm] = cache_framed(c, c.pad_g, c.xseq_g, torch.float32)
        r[nm][:, :c.Lk].copy_(ins["g"][i])
    for nm in ("dq", "dk_new", "dv_new"):
        r[nm + "_buf"], r[nm], _ = framed(R, d, SENTINEL, tdt, pi)
    views = [r["dout"], f["q"], f["kc"], f["vc"], r["dq"], r["dk_new"], r["dv_new"], r["gk"], r["gv"]]
    pitches = [v.stride(0) for v in (r["dout"], f["q"], r["dq"], r["dk_new"], r["dv_new"])] + [f["kc"].stride(1), f["kc"].stride(0)]
    ok = takes_16_bytes(c, views, pitches, c.vec) and takes_16_bytes(c, [], [r["gk"].stride(1), r["gk"].stride(0)], 4)
    assert c.hd % c.vec or ok == (not c.odd), (c.name, "the buffers do not have the alignment the case is written for")
    if not c.odd and (c.pad_g != c.pad_c or c.xseq_g != c.xseq):
        assert r["gk"].stride(1) != f["kc"].stride(1) and r["gk"].stride(0) != f["kc"].stride(0), c.name      # ldg != ldc, grad_seq != cache_seq
    ops.attention_step_bwd(r["dout"], f["q"], f["kc"], f["vc"], probs, c.nseq, c.Lq, c.Lk, c.H, c.hd, c.hd ** -0.5, r["dq"], r["dk_new"],
                           r["dv_new"], r["gk"], r["gv"], drop=(c.drop_p, c.key) if c.drop_p > 0 else None)
    torch.cuda.synchronize()
    r["results"] = [r[k + "_buf"] for k in ("dq", "dk_new", "dv_new", "gk", "gv")]
    return r


def check_backward(c, ins, ref, b, tag, ratios, l2, facts):
    R, d = c.nseq * c.Lq, c.d
    u = U32 if c.storage == "f32" else U16
    ok, wr = True, True
    for kind in ("dq", "dk_new", "dv_new"):
        ratios[f"{kind}/{tag}"] = worst_ratio(b[kind].float(), rows(ref[kind][0]), rows(ref[kind][1]), u)
        l2[f"{kind}/{tag}"] = rel_l2(b[kind].float().cpu(), torch.from_numpy(rows(ref[kind][0])))
        ok, wr = ok and frame_untouched(b[kind + "_buf"], R, d), wr and written(b[kind])
    for i, kind in enumerate(("gk", "gv")):
        if c.past:
            ratios[f"{kind}/{tag}"] = worst_ratio(b[kind][:, :c.past], cache_rows(ref[kind][0]), cache_rows(ref[kind][1]), U32)
            l2[f"{kind}/{tag}"] = rel_l2(b[kind][:, :c.past].cpu(), torch.from_numpy(cache_rows(ref[kind][0])))
        ok = ok and cache_frame_is_nan(b[kind + "_buf"], c)
        facts["new_rows_of_gradient_caches_keep_bits/" + tag] = facts.get("new_rows_of_gradient_caches_keep_bits/" + tag, True) and \
            torch.equal(bits(b[kind][:, c.past:c.Lk]), bits(ins["g"][i][:, c.past:]))
    facts["bwd_frames/" + tag], facts["bwd_written/" + tag] = ok, wr


def run_case(c):
    """runs case c -> (ratios {kind: worst |got - ref| / (u S)}, l2 {kind: relative L2, or error / per-tensor bound}, facts {name: bool})"""
    ins, ref = shared(c)
    ratios, l2, facts = {}, {}, {}
    entry = {"fwd": "fwd", "fwd_drop": "fwd_drop", "split": "split", "bwd": "fwd_drop" if c.drop_p > 0 else "fwd"}[c.entry]
    f = run_forward(c, ins, entry)
    check_forward(c, ins, ref, f, ratios, l2, facts)
    facts["fwd_same_bits"] = same_bits(f["results"], run_forward(c, ins, entry)["results"])
    if c.entry == "fwd_drop" and c.drop_p == 0:      # the plan gives DROP = false: the bits of the plain entry point
        facts["drop_p0_is_fwd"] = same_bits(f["results"], run_forward(c, ins, "fwd")["results"])
    if c.entry == "bwd":
        before = [f["kc_buf"].clone(), f["vc_buf"].clone()]
        rbuf, rflat = flat_framed(c.nseq * c.H * c.Lq * c.Lk)
        rflat.copy_(torch.from_numpy(ref["probs"][0]).float().flatten())
        for tag, pr in (("own", f["probs"]), ("ref", rflat.view(c.nseq, c.H, c.Lq, c.Lk))):
            b = run_backward(c, ins, f, pr)
            check_backward(c, ins, ref, b, tag, ratios, l2, facts)
            if tag == "own":
                facts["bwd_same_bits"] = same_bits(b["results"], run_backward(c, ins, f, pr)["results"])
        facts["bwd_leaves_caches_and_probs"] = same_bits(before, [f["kc_buf"], f["vc_buf"]]) and flat_untouched(f["probs_buf"]) and \
            flat_untouched(rbuf)
    return ratios, l2, facts


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_attention_step_case(c):
    ratios, l2, facts = run_case(c)
    print(f"attention_step_case {c.name}: " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + " | L2 "
          + " ".join(f"{k} {v:.2e}" for k, v in l2.items()))
    for kind, r in ratios.items():
        bar = C[c.storage][kind.split("/")[0]]
        assert r <= bar, f"{c.name}: {kind} is off by {r:.3g} u S, the bar is {bar}"
    for kind, e in l2.items():
        k = kind.split("/")[0]
        bar = 1.0 if k in ("out_max", "hi_max") else L2[c.storage]["grads" if k[0] in "dg" else k]
        assert e <= bar if bar == 1.0 else e < bar, (c.name, kind, e)
    assert all(facts.values()), (c.name, facts)
