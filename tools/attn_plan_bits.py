"""One forward, one backward and, where there is a bias, one bias-gradient call at the smallest shape of every attention plan family
(csrc/attn_plan.h), fixed seed, nseq = 3, H = 2; prints a SHA-256 per output tensor.  Two builds that plan and launch alike print the
same lines on the same device: every one of these kernels is free of atomics.      python tools/attn_plan_bits.py > bits.txt"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from afft_amd import _lib, ops  # noqa: E402

NSEQ, H = 3, 2


def show(tag, **tensors):
    torch.cuda.synchronize()
    for name, t in tensors.items():
        print(tag, name, hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest())


def rnd(g, dtype, *shape):
    return torch.randn(*shape, generator=g).to(dtype).cuda()


def case(tag, dtype, L, hd, p, mask=_lib.MASK_NONE, period=0, table=False, bias_shape=None):
    g = torch.Generator().manual_seed(1234)
    q, k, v, dout = (rnd(g, dtype, NSEQ * L, H * hd) for _ in range(4))
    bias = rnd(g, torch.float32, *bias_shape) if bias_shape else rnd(g, torch.float32, L, L) if table else None
    out, probs = torch.empty_like(q), torch.empty(NSEQ, H, L, L, dtype=torch.float32, device="cuda")
    scale, key, long = hd ** -0.5, 77, L > 128
    if bias_shape:
        (ops.attention_long_fwd_bias if long else ops.attention_fwd_bias)(q, k, v, NSEQ, L, H, hd, scale, bias, out, probs, p, key)
    elif long:
        ops.attention_long_fwd(q, k, v, NSEQ, L, H, hd, scale, mask, out, probs, p, key, period, bias)
    elif table:
        ops.attention_fwd_table(q, k, v, NSEQ, L, H, hd, scale, bias, out, probs, p, key)
    else:
        ops.attention_fwd(q, k, v, NSEQ, L, H, hd, scale, mask, out, probs, p, key, period)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    (ops.attention_long_bwd if long else ops.attention_bwd)(dout, q, k, v, probs, NSEQ, L, H, hd, scale, dq, dk, dv, p, key)
    tag = "%s %s L=%d hd=%d p=%g" % (tag, str(dtype)[6:], L, hd, p)
    show(tag, out=out, probs=probs, dq=dq, dk=dk, dv=dv)
    if bias_shape:
        show(tag, dbias=ops.attention_bias_bwd(dout, v, probs, NSEQ, L, H, hd, torch.empty_like(bias), p, key))


def split_case(L, hd, p, two_planes):
    g = torch.Generator().manual_seed(4321)
    R, d = NSEQ * L, H * hd

    def planes():      # x = hi + lo as fp16 planes, or the hi plane alone
        x = rnd(g, torch.float32, R, d)
        hi = x.half()
        return torch.stack([hi, (x - hi.float()).half()]) if two_planes else hi[None]

    q, k, v = planes(), planes(), planes()
    out, out_b = torch.empty(2, R, d, dtype=torch.float16, device="cuda"), torch.empty(R, d, dtype=torch.bfloat16, device="cuda")
    probs = torch.empty(NSEQ, H, L, L, dtype=torch.float32, device="cuda")
    ops.attention_fwd_split(q[0], k[0], v[0], R * d if two_planes else 0, NSEQ, L, H, hd, hd ** -0.5, _lib.MASK_CAUSAL, out[0], R * d, out_b,
                            probs, p, 77)
    show("split planes=%d L=%d hd=%d p=%g" % (1 + two_planes, L, hd, p), out=out, out_bf16=out_b, probs=probs)


def main():
    f32, bf16 = torch.float32, torch.bfloat16
    for p in (0.0, 0.3):
        for L in (5, 33, 65):
            case("generic-short", f32, L, 8, p, _lib.MASK_DIAG)
        case("generic-short", bf16, 5, 8, p, _lib.MASK_CAUSAL)
        for L in (3, 16, 17, 33, 64):
            case("mfma-short", bf16, L, 64, p, _lib.MASK_CAUSAL)
        case("mfma-short-chunked", bf16, 33, 1024, p)
        for L in (16, 17):
            case("sliced-bwd", bf16, L, 128, p, _lib.MASK_DIAG)
        split_case(16, 64, p, True)
        split_case(16, 64, p, False)
        split_case(33, 128, p, True)
        for dtype, hd, name in ((f32, 8, "long-f32"), (bf16, 64, "long-mfma"), (bf16, 8, "long-bf16")):
            for L in (129, 160, 512):
                case(name, dtype, L, hd, p)
            case(name + " causal", dtype, 129, hd, p, _lib.MASK_CAUSAL)
            case(name + " block-causal", dtype, 129, hd, p, _lib.MASK_BLOCKCAUSAL, 43)
            for L in (5, 129):
                case(name + " table", dtype, L, hd, p, table=True)
                for what, shape in (("batch", (1, H, L, L)), ("heads", (NSEQ, 1, L, L)), ("full", (NSEQ, H, L, L))):
                    case(name + " bias-" + what, dtype, L, hd, p, bias_shape=shape)


if __name__ == "__main__":
    main()
