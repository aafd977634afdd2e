"""Attention over 129..512 tokens (csrc/attention_long.hip) against float64 math (oracle._softmax_attend), written like
test_kernels_gpu.py::test_attention_fwd_bwd and with its bars: relative L2, f32 2e-5 (out, probs) / 3e-5 (gradients), bf16 1e-2 (out) /
2e-3 (probs) / 2e-2 (gradients).  Every operand (q, k, v, dout: each on its own) sits inside a larger NaN-filled buffer and every
result (out, dq, dk, dv, probs) inside a sentinel-filled one."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from helpers import rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu

PAD_ROWS, PAD_COLS, PAD_FLAT, SENTINEL = 2, 8, 64, 512.0


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def bfr(t):
    return t.to(torch.bfloat16).float()


def framed(t, fill):
    """t [R, C] inside a [R + 2 PAD_ROWS, C + PAD_COLS] buffer of `fill` (rows stay 16-byte aligned for bf16 and fp32)"""
    R, C = t.shape
    buf = torch.full((R + 2 * PAD_ROWS, C + PAD_COLS), fill, dtype=t.dtype, device=dev())
    buf[PAD_ROWS:PAD_ROWS + R, :C] = t.to(dev())
    return buf, buf[PAD_ROWS:PAD_ROWS + R, :C]


def frame_untouched(buf, R, C):
    b = buf.float().cpu()
    edge = torch.cat([b[:PAD_ROWS].flatten(), b[PAD_ROWS + R:].flatten(), b[PAD_ROWS:PAD_ROWS + R, C:].flatten()])
    return bool((edge == SENTINEL).all())


def make_table(L, seed):
    """random additive table with some -inf (never a whole row: column 0 stays finite)"""
    t = 0.5 * rnd(L, L, seed=seed)
    hide = torch.rand(L, L, generator=torch.Generator().manual_seed(seed + 1)) < 0.2
    hide[:, 0] = False
    return t.masked_fill(hide, float("-inf"))


def ref_mask(L, mask, period, table):
    from oracle import afft_oracle as O
    if mask == 3:
        m = O.make_mask("causal", period, torch.float64).repeat(L // period, L // period)
    else:
        m = O.make_mask(["none", "diag", "causal"][mask], L, torch.float64)
    if table is not None:
        m = table.double() if m is None else m + table.double()
    return m


# (nseq, L, H, hd, mask kind, block-causal divisor, additive table, storage)
CASES = [
    (2, 129, 2, 64, 0, 0, False, "f32"), (2, 129, 2, 64, 1, 0, False, "bf16"),
    (3, 160, 2, 16, 3, 4, False, "bf16"),                                     # generic bf16 (hd % 64 != 0)
    (3, 160, 2, 64, 3, 5, False, "f32"),
    (40, 160, 16, 64, 3, 4, False, "bf16"),                                   # 640 (sequence, head) pairs x 5 tiles: well above the CU count
    (24, 160, 16, 16, 2, 0, False, "f32"),
    (2, 160, 4, 512, 1, 0, False, "bf16"),
    (2, 256, 2, 128, 2, 0, False, "bf16"), (1, 256, 2, 128, 0, 0, True, "f32"), (1, 256, 1, 512, 3, 4, False, "f32"),
    (1, 320, 1, 64, 3, 5, False, "bf16"), (1, 320, 2, 512, 0, 0, True, "bf16"), (2, 320, 2, 128, 2, 0, True, "f32"),
    (1, 511, 1, 64, 2, 0, False, "bf16"), (1, 511, 2, 16, 2, 0, True, "f32"), (2, 511, 2, 128, 0, 0, True, "bf16"),
    (1, 512, 2, 512, 3, 4, False, "bf16"), (1, 512, 1, 1024, 2, 0, True, "bf16"), (1, 512, 1, 1024, 2, 0, False, "f32"),
    (1, 512, 2, 64, 3, 4, False, "f32"),
]


@pytest.mark.parametrize("nseq,L,H,hd,mask,div,tab,dt", CASES)
def test_attention_long_fwd_bwd(nseq, L, H, hd, mask, div, tab, dt):
    from afft_amd import ops
    from oracle import afft_oracle as O
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    d, R = H * hd, nseq * L
    qkv = rnd(R, 3 * d, seed=1)
    dout = rnd(R, d, seed=2)
    if dt == "bf16":
        qkv, dout = bfr(qkv), bfr(dout)
    # q, k and v each in a NaN frame of its own: a read past H * hd columns or nseq * L rows of any of them meets NaN, not a neighbour
    (_, q), (_, k), (_, v) = (framed(qkv[:, i * d:(i + 1) * d].to(tdt), float("nan")) for i in range(3))
    obuf, out = framed(torch.full((R, d), SENTINEL, dtype=tdt), SENTINEL)
    pflat = torch.full((nseq * H * L * L + 2 * PAD_FLAT,), SENTINEL, device=dev())
    probs = pflat[PAD_FLAT:-PAD_FLAT].view(nseq, H, L, L)
    scale = hd ** -0.5
    period = L // div if mask == 3 else 0
    table = make_table(L, seed=5) if tab else None
    ops.attention_long_fwd(q, k, v, nseq, L, H, hd, scale, mask, out, probs, mask_period=period,
                           table=table.to(dev()) if tab else None)
    qr = qkv.clone().double().requires_grad_(True)
    t = qr.view(nseq, L, 3, H, hd).permute(2, 0, 3, 1, 4)
    m = ref_mask(L, mask, period, table)
    o_ref, p_ref = O._softmax_attend(t[0], t[1], t[2], scale, m)
    e_out, e_p = rel_l2(out.float().cpu(), o_ref.reshape(R, d).float()), rel_l2(probs.cpu(), p_ref.float())
    o_ref.reshape(R, d).backward(dout.double())
    _, do = framed(dout.to(tdt), float("nan"))
    (qbuf, dq), (kbuf, dk), (vbuf, dv) = (framed(torch.full((R, d), SENTINEL, dtype=tdt), SENTINEL) for _ in range(3))
    ops.attention_long_bwd(do, q, k, v, probs, nseq, L, H, hd, scale, dq, dk, dv)
    torch.cuda.synchronize()
    e_g = rel_l2(torch.cat([dq, dk, dv], dim=1).float().cpu(), qr.grad.float())
    print(f"attention_long {dt} nseq={nseq} L={L} H={H} hd={hd} mask={mask} table={tab}: out {e_out:.3e} probs {e_p:.3e} grads {e_g:.3e}")
    assert e_out < (2e-5 if dt == "f32" else 1e-2)
    assert e_p < (2e-5 if dt == "f32" else 2e-3)
    assert e_g < (3e-5 if dt == "f32" else 2e-2)
    if mask or tab:  # masked probabilities are exactly zero
        assert float(probs.cpu()[..., torch.isinf(m)].abs().max()) == 0.0
    # nothing outside nseq * L rows and H * hd columns was written (and nothing outside was read: it is NaN there, and no result is)
    assert all(frame_untouched(b, R, d) for b in (obuf, qbuf, kbuf, vbuf))
    assert bool(torch.isfinite(out.float()).all()) and all(bool(torch.isfinite(t.float()).all()) for t in (dq, dk, dv))
    pf = pflat.cpu()
    assert bool((pf[:PAD_FLAT] == SENTINEL).all()) and bool((pf[-PAD_FLAT:] == SENTINEL).all())


def _run(tdt, qkv, dout, nseq, L, H, hd, mask, period, p, key):
    from afft_amd import ops
    d = H * hd
    g = qkv.to(tdt).to(dev())
    q, k, v = g[:, :d], g[:, d:2 * d], g[:, 2 * d:]
    out = torch.empty(nseq * L, d, dtype=tdt, device=dev())
    probs = torch.empty(nseq, H, L, L, device=dev())
    ops.attention_long_fwd(q, k, v, nseq, L, H, hd, hd ** -0.5, mask, out, probs, drop_p=p, drop_key=key, mask_period=period)
    dg = torch.zeros(nseq * L, 3 * d, dtype=tdt, device=dev())
    ops.attention_long_bwd(dout.to(tdt).to(dev()), q, k, v, probs, nseq, L, H, hd, hd ** -0.5, dg[:, :d], dg[:, d:2 * d],
                           dg[:, 2 * d:], drop_p=p, drop_key=key)
    torch.cuda.synchronize()
    return out.cpu(), probs.cpu(), dg.cpu()


def test_attention_long_dropout_mfma_matches_fp32():
    """one key: the bf16 MFMA form and the fp32 form drop the same elements (bars of test_attention_dropout_mfma_matches_generic)"""
    nseq, L, H, hd = 4, 160, 2, 64
    qkv, dout = bfr(rnd(nseq * L, 3 * H * hd, seed=11)), bfr(rnd(nseq * L, H * hd, seed=12))
    o32, p32, g32 = _run(torch.float32, qkv, dout, nseq, L, H, hd, 3, 40, 0.3, 12345)
    o16, p16, g16 = _run(torch.bfloat16, qkv, dout, nseq, L, H, hd, 3, 40, 0.3, 12345)
    assert rel_l2(p16, p32) < 2e-3
    assert rel_l2(o16.float(), o32) < 1.5e-2
    assert rel_l2(g16.float(), g32) < 3e-2
    o0, _, _ = _run(torch.float32, qkv, dout, nseq, L, H, hd, 3, 40, 0.0, 0)
    assert rel_l2(o0, o32) > 0.1


@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16])
def test_attention_long_run_to_run_bitwise(tdt):
    nseq, L, H, hd = 3, 320, 2, 128
    qkv, dout = bfr(rnd(nseq * L, 3 * H * hd, seed=21)), bfr(rnd(nseq * L, H * hd, seed=22))
    a = _run(tdt, qkv, dout, nseq, L, H, hd, 2, 0, 0.1, 777)
    b = _run(tdt, qkv, dout, nseq, L, H, hd, 2, 0, 0.1, 777)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_attention_long_range():
    from afft_amd import ops
    H, hd = 1, 64
    for L in (128, 513):
        g = torch.zeros(L, 3 * hd, device=dev())
        out, probs = torch.empty(L, hd, device=dev()), torch.empty(1, H, L, L, device=dev())
        with pytest.raises(RuntimeError, match=r"outside 129\.\.512"):
            ops.attention_long_fwd(g[:, :hd], g[:, hd:2 * hd], g[:, 2 * hd:], 1, L, H, hd, 0.125, 0, out, probs)
        with pytest.raises(RuntimeError, match=r"outside 129\.\.512"):
            ops.attention_long_bwd(out, g[:, :hd], g[:, hd:2 * hd], g[:, 2 * hd:], probs, 1, L, H, hd, 0.125, out, out, out)
    L = 129
    g = torch.zeros(L, 3 * hd, device=dev())
    out, probs = torch.empty(L, hd, device=dev()), torch.empty(1, H, L, L, device=dev())
    with pytest.raises(RuntimeError, match=r"outside 1\.\.128"):
        ops.attention_fwd(g[:, :hd], g[:, hd:2 * hd], g[:, 2 * hd:], 1, L, H, hd, 0.125, 0, out, probs)
