"""The float64 reference of attention and the elementwise comparison shared by test_attention_short_gpu.py (L <= 128) and
test_attention_long_cases_gpu.py (attention_long.hip: 129..512 tokens, and the bias gradient at every L).

reference(): float64 scores, mask, the optional additive bias (added after the score scale, -inf allowed), softmax, the dropout mask of
the integer replica (kernel_doubles.drop_keep at index ((seq * H + h) * L + i) * L + j, scaled by 1 / (1 - p)), P'V, and the backward
products written out.  Beside every output element it forms the magnitude sum S: the same expression with absolute values at every
product and sum (for probs, which is all positive, the first-order image of the score's magnitude sum A = scale * sum |q| |k| + |bias|
through the softmax: S = p * (1 + A_ij + sum_j p_ij A_ij)).  worst_ratio() is max |got - ref| / (u S).

The frame helpers put every operand in a NaN frame and every result in a sentinel frame of its own on the device."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(__file__))
import kernel_doubles as kd  # noqa: E402
from attention_cases import BLOCK, CAUSAL, DIAG  # noqa: E402

PAD_ROWS, PAD_FLAT, SENTINEL, KEY = 2, 64, 512.0, 0x9E3779B9


def dev():
    return torch.device("cuda:0")


def framed(R, C_, fill, dtype, pad_cols, planes=1):
    """[planes] buffers of (R + 2 PAD_ROWS) x (C_ + pad_cols) filled with `fill`; the [R, C_] view of plane 0; elements between planes"""
    buf = torch.full((planes, R + 2 * PAD_ROWS, C_ + pad_cols), fill, dtype=dtype, device=dev())
    return buf, buf[0, PAD_ROWS:PAD_ROWS + R, :C_], (R + 2 * PAD_ROWS) * (C_ + pad_cols)


def frame_untouched(buf, R, C_):
    b = buf.float().cpu()
    edge = torch.cat([b[:, :PAD_ROWS].flatten(), b[:, PAD_ROWS + R:].flatten(), b[:, PAD_ROWS:PAD_ROWS + R, C_:].flatten()])
    return bool((edge == SENTINEL).all())


def flat_framed(n, fill=SENTINEL):
    buf = torch.full((n + 2 * PAD_FLAT,), fill, device=dev())
    return buf, buf[PAD_FLAT:PAD_FLAT + n]


def flat_untouched(buf):
    b = buf.cpu()
    return bool((b[:PAD_FLAT] == SENTINEL).all()) and bool((b[-PAD_FLAT:] == SENTINEL).all())


def banned_pairs(L, mask, period):
    """bool [L, L]: (query i, key j) pairs the mask removes.  Block-causal with period 1 IS no mask and with period L IS the causal mask:
    those two are written that way, not through the modulo rule"""
    i, j = np.arange(L)[:, None], np.arange(L)[None, :]
    if mask == DIAG:
        return i == j
    if mask == CAUSAL or (mask == BLOCK and period == L):
        return j > i
    if mask == BLOCK and period > 1:
        return (j % period) > (i % period)
    return np.zeros((L, L), dtype=bool)


def keep_scale(nseq, H, L, p, key):
    """float64 [nseq, H, L, L]: 0 or 1 / (1 - p) by the replica mask (p as the C float the kernels get)"""
    if p <= 0:
        return np.ones((nseq, H, L, L)), None
    idx = np.arange(nseq * H * L * L, dtype=np.uint64).reshape(nseq, H, L, L)      # ((seq * H + h) * L + i) * L + j
    keep = kd.drop_keep(key, idx, p)
    return np.where(keep, 1.0 / (1.0 - float(np.float32(p))), 0.0), keep


def _sum_like(x, shape4):
    """x [nseq, H, L, L] summed over the dimensions in which a bias of (4-dimensional) shape `shape4` broadcasts"""
    axes = tuple(a for a in range(3) if shape4[a] == 1 and x.shape[a] != 1)
    return x.sum(axis=axes, keepdims=True) if axes else x


def reference(q, k, v, do, scale, banned, ks, bias=None):
    """float64 [nseq, H, L, hd] operands -> {kind: (value, magnitude sum S)}.  bias: float64, 2 to 4 dimensions, broadcastable to
    [nseq, H, L, L], added after the score scale (-inf allowed); with it the result has "dbias", in the bias's own shape: dS / scale =
    p (dP - sum p dP) summed over the dimensions the bias broadcasts in"""
    T = lambda x: np.swapaxes(x, -1, -2)      # noqa: E731
    aq, ak, av, ado = np.abs(q), np.abs(k), np.abs(v), np.abs(do)
    s = np.where(banned, -np.inf, scale * (q @ T(k)))
    A = scale * (aq @ T(ak))
    if bias is not None:
        b4 = bias.reshape((1,) * (4 - bias.ndim) + bias.shape)
        s = s + b4
        A = A + np.where(np.isfinite(b4), np.abs(b4), 0.0)
    e = np.exp(s - s.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    r = {"probs": (p, p * (1.0 + A + (p * A).sum(-1, keepdims=True)))}
    pd = p * ks                                # P': after dropout
    r["out"] = (pd @ v, pd @ av)
    r["dv"] = (T(pd) @ do, T(pd) @ ado)
    dp, dpm = (do @ T(v)) * ks, (ado @ T(av)) * ks
    dot, dotm = (p * dp).sum(-1, keepdims=True), (p * dpm).sum(-1, keepdims=True)
    ds, dsm = p * (dp - dot) * scale, p * (dpm + dotm) * scale
    r["dq"] = (ds @ k, dsm @ ak)
    r["dk"] = (T(ds) @ q, T(dsm) @ aq)
    if bias is not None:
        r["dbias"] = tuple(_sum_like(x, b4.shape).reshape(bias.shape) for x in (p * (dp - dot), p * (dpm + dotm)))
    return r


def rows(x):
    """[nseq, H, L, hd] -> the [nseq * L, H * hd] layout of the operands"""
    n, H, L, hd = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(n * L, H * hd)


def heads(x, nseq, L, H, hd):
    return x.reshape(nseq, L, H, hd).transpose(0, 2, 1, 3)


def worst_ratio(got, ref, S, u, floor=0.0):
    """max (|got - ref| - floor) / (u S); where S is 0 the result must be the reference exactly (to the floor)"""
    got = got.detach().double().cpu().numpy().reshape(ref.shape)
    err = np.maximum(np.abs(got - ref) - floor, 0.0)
    if not np.isfinite(got).all() or bool((err[S == 0] != 0).any()):
        return math.inf
    nz = S > 0
    return float((err[nz] / (u * S[nz])).max()) if nz.any() else 0.0
