"""TEST DOUBLES of the elementwise, loss-reduce and fusion entry points -- test infrastructure, never part of the product.

Plain numpy restatements of the C-ABI contracts in include/afft_hip.h (float64 unless a dtype is asked for), in the way
tests/metrics_double.py restates the metrics kernels: no GPU code, nothing of afft_amd.ops.  tests/test_kernel_doubles_cpu.py keeps them
honest on the CPU (torch float64 autograd, a transcription of Runner._reduce_loss, the binomial bound of the mask);
tests/test_elementwise_gpu.py compares the kernels with them.

The dropout mask is an INTEGER replica of csrc/common.h (mix32 / drop_keep / drop_row_scale / drop_elem_scale / make_drop / with_salt):
the one replica of the repository (tests/test_attention_bias_gpu.py imports mix32 from here).
"""
import math

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH, ACT_RELU, ACT_SIGMOID_GATE = 0, 1, 2, 5, 6      # include/afft_hip.h: AFFT_ACT_*


# ---- dropout: keep(idx) = mix32(mix32(idx) ^ key) >= floor(p * 2^32)
def mix32(x):
    """csrc/common.h mix32 on uint64 arrays that hold 32-bit values"""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & _M32
    return x ^ (x >> np.uint64(16))


def drop_thresh(p):
    """make_drop: the rate is a C float; floor(p * 2^32), saturated"""
    t = float(np.float32(p)) * 4294967296.0
    return 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def device_salt():
    """the device word every kernel XORs into its keys once afft_amd.dropout.enable_device_salt has run (None: off)"""
    from afft_amd import dropout as D_
    return None if D_._salt is None else int(D_._salt.item()) & 0xFFFFFFFF


def salted_key(key, path=False):
    """with_salt: key ^ salt for the element mask, key ^ mix32(salt ^ 0x5bd1e995) for DropPath"""
    key, s = int(key) & 0xFFFFFFFF, device_salt()
    if s is None:
        return key
    return key ^ (int(mix32(np.uint64(s ^ 0x5bd1e995))) if path else s)


def drop_keep(key, idx, p, path=False):
    """bool array: which of the indices `idx` (any integers, taken mod 2^32) the mask of (key, p) keeps"""
    idx = np.asarray(idx).astype(np.uint64) & _M32
    return mix32(mix32(idx) ^ np.uint64(salted_key(key, path))) >= np.uint64(drop_thresh(p))


def drop_scales(desc, rows, cols):
    """float32 [rows, cols]: what a kernel multiplies element [r, c] by under the afft_dropout_t `desc` (fields p, key, path_p, path_key,
    path_group): drop_row_scale(r // path_group) * drop_elem_scale(r * cols + c mod 2^32), each 0 or 1 / (1 - rate) in fp32"""
    one = np.float32(1.0)
    scale = np.ones((rows, cols), dtype=np.float32)
    if desc is None:
        return scale
    if desc.p > 0:
        idx = (np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(cols) + np.arange(cols, dtype=np.uint64)[None, :]) & _M32
        scale = np.where(drop_keep(desc.key, idx, desc.p), one / (one - np.float32(desc.p)), np.float32(0.0)).astype(np.float32)
    if desc.path_p > 0:
        group = desc.path_group if desc.path_group > 0 else 1
        keep = drop_keep(desc.path_key, np.arange(rows) // group, desc.path_p, path=True)
        row = np.where(keep, one / (one - np.float32(desc.path_p)), np.float32(0.0)).astype(np.float32)
        scale = (row[:, None] * scale).astype(np.float32)
    return scale


# ---- afft_act_bwd
_erf = np.vectorize(math.erf, otypes=[np.float64])


def act_bwd(act, dy, saved, aux=None, scale=None):
    """(dpre, daux) of y = drop(act(pre)): dy, saved = pre, aux, scale (the dropout scales, or None) as float64 arrays"""
    g = np.asarray(dy, dtype=np.float64)
    if scale is not None:
        g = g * np.asarray(scale, dtype=np.float64)
    if act == ACT_NONE:
        return g, None
    p = np.asarray(saved, dtype=np.float64)
    if act == ACT_GELU_ERF:
        return g * (0.5 * (1.0 + _erf(p / math.sqrt(2.0))) + p * np.exp(-0.5 * p * p) / math.sqrt(2.0 * math.pi)), None
    if act == ACT_GELU_TANH:
        k = math.sqrt(2.0 / math.pi)
        t = np.tanh(k * (p + 0.044715 * p ** 3))
        return g * (0.5 * (1.0 + t) + 0.5 * p * (1.0 - t * t) * k * (1.0 + 3.0 * 0.044715 * p * p)), None
    if act == ACT_RELU:
        return np.where(p > 0, g, 0.0), None
    if act == ACT_SIGMOID_GATE:
        sg = 1.0 / (1.0 + np.exp(-p))
        return g * np.asarray(aux, dtype=np.float64) * sg * (1.0 - sg), g * sg
    raise ValueError(f"act_bwd: bad activation {act}")


# ---- afft_loss_reduce / afft_loss_reduce_bwd(_ok)
def loss_reduce(vals, weights):
    """(means float64 [nterms], total): the mean of every term (0 for an empty one) and sum_i w[i] * means[i] over the terms whose
    weight is not 0 -- a weight of 0 DROPS the term, so its NaN / inf stays out of the total"""
    means = np.array([float(np.mean(np.asarray(v, dtype=np.float64))) if np.size(v) else 0.0 for v in vals])
    total = 0.0
    for m, w in zip(means, weights):
        if float(np.float32(w)) != 0.0:
            total += float(np.float32(w)) * m
    return means, total


def loss_reduce_bwd(ns, weights, g_total=None, total=None):
    """([fp32 value every element of g[i] takes: float32(go * w[i] / n[i]) in the kernel's fp32 order, None for an empty term], ok)"""
    go = np.float32(1.0 if g_total is None else g_total)
    with np.errstate(all="ignore"):
        vals = [None if n <= 0 else np.float32(np.float32(go * np.float32(w)) / np.float32(n)) for n, w in zip(ns, weights)]
    ok = 1.0 if (total is None or math.isfinite(float(total))) and math.isfinite(float(go)) else 0.0
    return vals, ok


# ---- softmax / score fusion
def softmax_rows(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


softmax_small_fwd = softmax_rows


def softmax_small_bwd(y, dy):
    y, dy = np.asarray(y, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    return y * (dy - (dy * y).sum(axis=1, keepdims=True))


def weighted_sum_fwd(xs, w):
    w = np.asarray(w, dtype=np.float64)
    return sum(w[:, i:i + 1] * np.asarray(x, dtype=np.float64) for i, x in enumerate(xs))


def weighted_sum_bwd(xs, w, dout):
    """([dx_i], dw)"""
    w, dout = np.asarray(w, dtype=np.float64), np.asarray(dout, dtype=np.float64)
    dxs = [w[:, i:i + 1] * dout for i in range(len(xs))]
    dw = np.stack([(dout * np.asarray(x, dtype=np.float64)).sum(axis=1) for x in xs], axis=1)
    return dxs, dw


# ---- frames, MSE, periodic tables
def gather_frames(clips, frames, C, srcs, dtype=np.float64):
    """out[clip, t] = sum over the sources (array [clips, f, C], lo, hi, off), in their order, with lo <= t < hi of src[clip, t + off];
    zeros where none covers t.  dtype float32 repeats the kernel's own additions (0 + first + second ...)."""
    out = np.zeros((clips, frames, C), dtype=dtype)
    for s, lo, hi, off in srcs:
        if hi > lo:
            out[:, lo:hi] = out[:, lo:hi] + np.asarray(s, dtype=dtype)[:, lo + off:hi + off]
    return out


def mse(a, b, g=1.0):
    """(sum (a - b)^2, da = 2 g (a - b), db = -da)"""
    diff = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return float((diff * diff).sum()), 2.0 * g * diff, -2.0 * g * diff


def mse_frames_bwd(a, b, a_lo, b_lo, nt, g=1.0):
    """whole gradients of g * sum((a[:, a_lo:a_lo+nt] - b[:, b_lo:b_lo+nt])^2) for a [B, Ta, C], b [B, Tb, C]: zeros outside the ranges"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    diff = a[:, a_lo:a_lo + nt] - b[:, b_lo:b_lo + nt]
    da, db = np.zeros_like(a), np.zeros_like(b)
    da[:, a_lo:a_lo + nt] = 2.0 * g * diff
    db[:, b_lo:b_lo + nt] = -2.0 * g * diff
    return da, db


def reduce_rows_periodic(src, period):
    """[period, d]: row p = sum of the rows r of src with r % period == p"""
    src = np.asarray(src, dtype=np.float64)
    out = np.zeros((period, src.shape[1]))
    for p in range(period):
        out[p] = src[p::period].sum(axis=0)
    return out


# ---- MixUp prologue
def mixup_plan(sub, B, ignore_cls):
    """(partner int32 [B], ign uint8 [B, T] or None): the samples without an ignored past label are paired in reverse order among
    themselves; everyone else -- and everyone when at most one sample qualifies -- is its own partner.  sub None: all qualify."""
    if sub is None:
        ok, ign = np.ones(B, dtype=bool), None
    else:
        sub = np.asarray(sub).reshape(B, -1)
        ign = (sub == ignore_cls).astype(np.uint8)
        ok = ~ign.any(axis=1)
    partner = np.arange(B, dtype=np.int32)
    sel = np.nonzero(ok)[0]
    if len(sel) > 1:
        partner[sel] = sel[::-1]
    return partner, ign
