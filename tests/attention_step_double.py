"""The float64 reference of the cached attention step (csrc/attention_step.hip) on top of attention_double.reference(), which is
rectangular already: Lq query rows against Lk = past + Lq key rows, banned[i, j] = j > past + i, the keep-scale drawn on the index
attention_step.hip draws on.  The softmax and the products are NOT restated here; what this module adds is the step's own:

step_keep_scale()   kernel_doubles.drop_keep at ((seq * H + h) * Lq + i) * Lk + j, scaled by 1 / (1 - p) with p as the C float
step_reference()    reference() plus the write rule of the backward with its magnitude sums: with cK = dk and cV = dv of reference()
                    over the Lq query rows and gk / gv the fp32 gradient caches before the call,
                        dk_new = gk[past:Lk] + cK[past:]     S = |gk| + S_dk      (dv_new alike)
                        gk[:past] += cK[:past]               S = |gk| + S_dk      (gv alike)
case_inputs()       the seeded operands of a case of attention_step_cases.py, rounded to the storage type, and what float64 sees of them
                    (planes: float(hi) + float(lo), or float(hi) alone when the call names no lo plane)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(__file__))
import kernel_doubles as kd  # noqa: E402
from attention_double import heads, reference  # noqa: E402


def step_banned(Lq, past):
    """bool [Lq, Lk]: query row i sits at position past + i and sees keys 0 .. past + i"""
    return np.arange(past + Lq)[None, :] > past + np.arange(Lq)[:, None]


def step_keep_scale(nseq, H, Lq, Lk, p, key):
    """(float64 [nseq, H, Lq, Lk]: 0 or 1 / (1 - p) by the replica mask, the bool mask or None)"""
    if p <= 0:
        return np.ones((nseq, H, Lq, Lk)), None
    idx = np.arange(nseq * H * Lq * Lk, dtype=np.uint64).reshape(nseq, H, Lq, Lk)      # ((seq * H + h) * Lq + i) * Lk + j
    keep = kd.drop_keep(key, idx, p)
    return np.where(keep, 1.0 / (1.0 - float(np.float32(p))), 0.0), keep


def step_reference(q, k, v, do, scale, past, ks, gk=None, gv=None):
    """q, do float64 [nseq, H, Lq, hd]; k, v [nseq, H, Lk, hd] (the past rows of the cache, then the new rows); gk, gv [nseq, H, Lk, hd]:
    the gradient caches before the call -> {kind: (value, magnitude sum S)} with probs, out, dq of reference() and, given gk / gv,
    dk_new, dv_new [nseq, H, Lq, hd] and gk, gv [nseq, H, past, hd] (the rows the backward adds to)"""
    Lq = q.shape[2]
    r = reference(q, k, v, do, scale, step_banned(Lq, past), ks)
    out = {kind: r[kind] for kind in ("probs", "out", "dq")}
    if gk is not None:
        for name, g, (c, S) in (("k", gk, r["dk"]), ("v", gv, r["dv"])):
            tot, mag = g + c, np.abs(g) + S
            out["d%s_new" % name] = (tot[:, :, past:], mag[:, :, past:])
            out["g" + name] = (tot[:, :, :past], mag[:, :, :past])
    return out


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def case_inputs(c):
    """-> dict of torch tensors in the layouts the entry points take (rows [nseq * Lq, H * hd], caches [nseq, rows, H * hd]):
    q, k_new, v_new, dout in the storage type (planes: *_hi / *_lo fp16 and q, k_new, v_new as the float64 the call sees), old [2, nseq,
    past, d] the past rows of the key / value caches in the cache type, g [2, nseq, Lk, d] fp32 rows of the gradient caches"""
    R, d = c.nseq * c.Lq, c.d
    seed = 1000 * c.hd + 10 * c.Lq + c.past
    x = _randn(R, 3 * d, seed=seed)
    old = _randn(2, c.nseq, c.past, d, seed=seed + 1)
    ins = {"dout": _randn(R, d, seed=seed + 2), "g": _randn(2, c.nseq, c.Lk, d, seed=seed + 3)}
    if c.storage == "planes":
        hi = x.half()
        lo = (x - hi.float()).half()
        val = hi.double() + lo.double() if c.in_lo else hi.double()
        for i, nm in enumerate(("q", "k_new", "v_new")):
            ins[nm + "_hi"], ins[nm + "_lo"], ins[nm] = hi[:, i * d:(i + 1) * d], lo[:, i * d:(i + 1) * d], val[:, i * d:(i + 1) * d]
        ins["old"] = old
        return ins
    tdt = torch.float32 if c.storage == "f32" else torch.bfloat16
    for i, nm in enumerate(("q", "k_new", "v_new")):
        ins[nm] = x[:, i * d:(i + 1) * d].to(tdt)
    ins["dout"], ins["old"] = ins["dout"].to(tdt), old.to(tdt)
    return ins


def case_reference(c, ins):
    """step_reference() of a case on the values of case_inputs(); (reference dict, keep mask or None)"""
    hd4 = lambda t, L: heads(t.double().numpy(), c.nseq, L, c.H, c.hd)      # noqa: E731
    q, do = hd4(ins["q"], c.Lq), hd4(ins["dout"], c.Lq)
    k, v = (np.concatenate([hd4(ins["old"][i].reshape(c.nseq * c.past, c.d), c.past), hd4(ins[nm], c.Lq)], axis=2)
            for i, nm in ((0, "k_new"), (1, "v_new")))
    ks, keep = step_keep_scale(c.nseq, c.H, c.Lq, c.Lk, c.drop_p, c.key)
    gk, gv = (hd4(ins["g"][i].reshape(c.nseq * c.Lk, c.d), c.Lk) for i in (0, 1))
    return step_reference(q, k, v, do, float(np.float32(c.hd ** -0.5)), c.past, ks, gk, gv), keep


def cache_rows(x):
    """[nseq, H, L, hd] -> the [nseq, L, H * hd] layout of a cache"""
    n, H, L, hd = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(n, L, H * hd)
