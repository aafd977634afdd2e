"""TEST DOUBLE of afft_amd.ops.attention_step, on top of tests/cpu_ops.py (which stays as it is): a plain-torch restatement of the
afft_attention_step_fwd contract of include/afft_hip.h.  `installed()` swaps it in together with every double of cpu_ops."""
from __future__ import annotations

import contextlib

import torch

import cpu_ops


@torch.no_grad()
def attention_step(q, k_new, v_new, k_cache, v_cache, nseq, Lq, Lk, H, hd, scale, out, probs):
    past, d = Lk - Lq, H * hd
    assert 1 <= Lq <= Lk <= k_cache.shape[1] and Lk <= 512
    assert k_cache.shape == v_cache.shape == (nseq, k_cache.shape[1], d) and k_cache.dtype == v_cache.dtype == q.dtype == out.dtype
    k_cache[:, past:Lk] = k_new.reshape(nseq, Lq, d)
    v_cache[:, past:Lk] = v_new.reshape(nseq, Lq, d)
    qh = cpu_ops._heads(q, nseq, Lq, H, hd)
    kh, vh = (cpu_ops._heads(c[:, :Lk], nseq, Lk, H, hd) for c in (k_cache, v_cache))
    s = qh @ kh.transpose(-1, -2) * scale
    hidden = torch.arange(Lk)[None, :] > past + torch.arange(Lq)[:, None]      # query i sits at position past + i
    p = torch.softmax(s.masked_fill(hidden, float("-inf")), -1)
    if probs is not None:
        probs.copy_(p.reshape(probs.shape))
    out.copy_((p @ vh).permute(0, 2, 1, 3).reshape(nseq * Lq, d))
    return out


@contextlib.contextmanager
def installed():
    from afft_amd import ops
    saved = ops.attention_step
    with cpu_ops.installed():
        ops.attention_step = attention_step
        try:
            yield
        finally:
            ops.attention_step = saved
