"""TEST DOUBLE of afft_amd.ops.attention_step with its `drop` argument and of afft_amd.ops.attention_step_bwd, on top of tests/cpu_ops_step.py
(which stays as it is): plain-torch restatements of the afft_attention_step_fwd_drop / afft_attention_step_bwd contracts of
include/afft_hip.h at p = 0 (the double models no dropout).  `installed()` swaps them in together with every double below them."""
from __future__ import annotations

import contextlib

import torch

import cpu_ops
import cpu_ops_step


@torch.no_grad()
def attention_step(q, k_new, v_new, k_cache, v_cache, nseq, Lq, Lk, H, hd, scale, out, probs, drop=None):
    assert drop is None or drop[0] == 0.0
    return cpu_ops_step.attention_step(q, k_new, v_new, k_cache, v_cache, nseq, Lq, Lk, H, hd, scale, out, probs)


@torch.no_grad()
def attention_step_bwd(dout, q, k_cache, v_cache, probs, nseq, Lq, Lk, H, hd, scale, dq, dk_new, dv_new, gk_cache, gv_cache, drop=None):
    assert drop is None or drop[0] == 0.0
    past, d = Lk - Lq, H * hd
    assert 1 <= Lq <= Lk <= k_cache.shape[1] and Lk <= 512
    assert gk_cache.shape == gv_cache.shape == k_cache.shape == v_cache.shape and gk_cache.dtype == gv_cache.dtype == torch.float32
    qh, doh = (cpu_ops._heads(t, nseq, Lq, H, hd) for t in (q, dout))
    kh, vh = (cpu_ops._heads(c[:, :Lk], nseq, Lk, H, hd) for c in (k_cache, v_cache))
    p = probs.float().reshape(nseq, H, Lq, Lk)
    dp = doh @ vh.transpose(-1, -2)
    ds = p * (dp - (dp * p).sum(-1, keepdim=True)) * scale
    back = lambda t, Ln: t.permute(0, 2, 1, 3).reshape(nseq, Ln, d)   # noqa: E731
    ck, cv = back(ds.transpose(-1, -2) @ qh, Lk), back(p.transpose(-1, -2) @ doh, Lk)
    dq.copy_(back(ds @ kh, Lq).reshape(nseq * Lq, d))
    dk_new.copy_((gk_cache[:, past:Lk] + ck[:, past:]).reshape(nseq * Lq, d))      # rows [past, Lk): read, not written
    dv_new.copy_((gv_cache[:, past:Lk] + cv[:, past:]).reshape(nseq * Lq, d))
    gk_cache[:, :past] += ck[:, :past]
    gv_cache[:, :past] += cv[:, :past]


@contextlib.contextmanager
def installed():
    from afft_amd import ops
    saved = ops.attention_step, ops.attention_step_bwd
    with cpu_ops_step.installed():
        ops.attention_step, ops.attention_step_bwd = attention_step, attention_step_bwd
        try:
            yield
        finally:
            ops.attention_step, ops.attention_step_bwd = saved
