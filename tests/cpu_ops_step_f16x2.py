"""TEST DOUBLES of afft_amd.ops.attn_step_sublayer_f16x2 / mlp_step_sublayer_f16x2, the two composite calls of the cached step in the
'fp16x2' precision, on top of tests/cpu_ops_step.py (which supplies every other double): plain-torch restatements of the contracts in
include/afft_hip.h that record what they were handed.  `installed()` swaps them in together with every double below them."""
from __future__ import annotations

import contextlib

import torch

import cpu_ops_step

ONE1, ONE2, ONE_ATTN = 4, 8, 16      # AFFT_F16X2_ONE_PASS_1 / _2 / _ATTN


def _operand(t, one_pass):
    """what a GEMM or the attention core reads of an activation carried as fp16 planes: hi alone, or hi + lo"""
    hi = t.half().float()
    return hi if one_pass else hi + (t - hi).half().float()


class Doubles:
    """the two composite step calls in plain torch, and a record of every call"""

    def __init__(self):
        self.attn, self.mlp = [], []

    @torch.no_grad()
    def attn_step_sublayer_f16x2(self, x, ln_w, ln_b, w_qkv, b_qkv, w_proj, b_proj, flags, Lq, Lk, H_, eps, scale, xn, qkv, ao, k_cache, v_cache,
                                 probs, y):
        rows, d = x.shape
        assert flags & 3 == 1 and w_qkv.dtype == w_proj.dtype == xn.dtype == qkv.dtype == ao.dtype == torch.float16
        assert k_cache.dtype == v_cache.dtype == torch.float32
        self.attn.append(dict(flags=flags, rows=rows, d=d, Lq=Lq, Lk=Lk, xn=xn.numel(), qkv=qkv.numel(), ao=ao.numel(), probs=probs is not None))
        v = torch.nn.functional.layer_norm(x, (d,), ln_w, ln_b, eps)
        q3 = _operand(_operand(v, flags & ONE1) @ w_qkv[:d, :3 * d].float() + b_qkv, flags & ONE_ATTN)
        out = torch.empty(rows, d)
        cpu_ops_step.attention_step(q3[:, :d], q3[:, d:2 * d], q3[:, 2 * d:], k_cache, v_cache, rows // Lq, Lq, Lk, H_, d // H_, scale, out, probs)
        y.copy_(x + _operand(out, flags & ONE2) @ w_proj[:d, :d].float() + b_proj)
        return y

    @torch.no_grad()
    def mlp_step_sublayer_f16x2(self, x, ln_w, ln_b, w1, b1, w2, b2, flags, gelu, eps, xn, h, stats, y):
        from afft_amd import _lib
        rows, d = x.shape
        hidden = w1.shape[1]
        assert flags & 3 == 1 and gelu == _lib.ACT_GELU_TANH and stats.shape == (2, rows)
        self.mlp.append(dict(flags=flags, rows=rows, d=d, hidden=hidden, xn=xn.numel(), h=h.numel()))
        v = torch.nn.functional.layer_norm(x, (d,), ln_w, ln_b, eps)
        u = torch.nn.functional.gelu(_operand(v, flags & ONE1) @ w1[:d, :hidden].float() + b1, approximate="tanh")
        y.copy_(x + _operand(u, flags & ONE2) @ w2[:hidden, :d].float() + b2)
        return y


@contextlib.contextmanager
def installed():
    from afft_amd import ops
    dbl = Doubles()
    with cpu_ops_step.installed():
        saved = ops.attn_step_sublayer_f16x2, ops.mlp_step_sublayer_f16x2
        ops.attn_step_sublayer_f16x2, ops.mlp_step_sublayer_f16x2 = dbl.attn_step_sublayer_f16x2, dbl.mlp_step_sublayer_f16x2
        try:
            yield dbl
        finally:
            ops.attn_step_sublayer_f16x2, ops.mlp_step_sublayer_f16x2 = saved
