"""GPU: afft_attention_step_fwd (csrc/attention_step.hip) -- causal attention of Lq new rows against a key / value cache plus the append
of those rows, in one launch -- against float64 torch math, in both storage dtypes, with the tolerances tests/test_kernels_gpu.py applies
to afft_attention_fwd (relative L2: out 2e-5 fp32 / 1e-2 bf16, probs 2e-5 / 2e-3)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import rel_l2  # noqa: E402

# (nseq, H, hd, Lq, Lk, cap): the smallest shapes at which the kernel can go wrong
SHAPES = [(3, 2, 64, 1, 1, 4),          # the smallest case
          (3, 2, 64, 1, 17, 20),        # the workload's first decode step
          (2, 3, 24, 1, 5, 5),          # hd off the 64 grid, cap == Lk
          (2, 2, 64, 3, 19, 32),        # Lq > 1 with a past
          (2, 2, 64, 4, 4, 8),          # first pass; also compared with ops.attention_fwd(mask = causal)
          (2, 4, 512, 16, 16, 19),      # the workload's first pass (4 tiles of 4 rows)
          (1, 4, 512, 1, 19, 19),       # the workload's last decode step
          (1, 2, 64, 1, 130, 160),      # crosses 128 keys
          (1, 1, 64, 1, 512, 512),      # the limit
          (2, 2, 10, 6, 9, 11)]         # rows no 16-byte load can take (element loads), a ragged last tile
TOL = {"f32": (2e-5, 2e-5), "bf16": (1e-2, 2e-3)}      # (out, probs)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _inputs(shape, dt):
    nseq, H, hd, Lq, Lk, cap = shape
    d, past = H * hd, Lk - Lq
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    g = torch.Generator().manual_seed(11 + Lk)
    new = torch.randn(nseq * Lq, 3 * d, generator=g).to(tdt)
    caches = torch.full((2, nseq, cap, d), float("nan"), dtype=tdt)      # rows the kernel must neither read nor write stay NaN
    caches[:, :, :past] = torch.randn(2, nseq, past, d, generator=g).to(tdt)
    return new, caches


def _run(shape, new, caches):
    from afft_amd import ops
    nseq, H, hd, Lq, Lk, cap = shape
    d = H * hd
    dev = torch.device("cuda:0")
    n, c = new.to(dev), caches.to(dev)
    out = torch.empty(nseq * Lq, d, dtype=new.dtype, device=dev)
    probs = torch.full((nseq, H, Lq, Lk), float("nan"), device=dev)
    ops.attention_step(n[:, :d], n[:, d:2 * d], n[:, 2 * d:], c[0], c[1], nseq, Lq, Lk, H, hd, hd ** -0.5, out, probs)
    torch.cuda.synchronize()
    return out.cpu(), probs.cpu(), c.cpu()


def _reference(shape, new, caches):
    nseq, H, hd, Lq, Lk, cap = shape
    d, past = H * hd, Lk - Lq
    n = new.double().view(nseq, Lq, 3, H, hd)
    q = n[:, :, 0].permute(0, 2, 1, 3)
    k, v = (torch.cat([caches[i, :, :past].double(), n[:, :, 1 + i].reshape(nseq, Lq, d)], 1).view(nseq, Lk, H, hd).permute(0, 2, 1, 3)
            for i in (0, 1))
    hidden = torch.arange(Lk)[None, :] > past + torch.arange(Lq)[:, None]
    p = torch.softmax((q @ k.transpose(-1, -2) * hd ** -0.5).masked_fill(hidden, float("-inf")), -1)
    return (p @ v).permute(0, 2, 1, 3).reshape(nseq * Lq, d), p, hidden


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_step_matches_float64_and_appends(shape, dt):
    nseq, H, hd, Lq, Lk, cap = shape
    d, past = H * hd, Lk - Lq
    new, caches = _inputs(shape, dt)
    out, probs, after = _run(shape, new, caches)
    o_ref, p_ref, hidden = _reference(shape, new, caches)
    e_out, e_p = rel_l2(out.float(), o_ref.float()), rel_l2(probs, p_ref.float())
    print(f"[{shape}/{dt}] out {e_out:.2e} probs {e_p:.2e}")
    assert torch.isfinite(out.float()).all() and torch.isfinite(probs).all()
    assert e_out < TOL[dt][0] and e_p < TOL[dt][1]
    # the cache: the past untouched, the new rows appended bit for bit, nothing written at or beyond Lk
    assert torch.isnan(after[:, :, Lk:].float()).all()
    assert torch.equal(_bits(after[:, :, :past]), _bits(caches[:, :, :past]))
    for i in (0, 1):
        assert torch.equal(_bits(after[i, :, past:Lk]), _bits(new[:, (1 + i) * d:(2 + i) * d].reshape(nseq, Lq, d).contiguous()))
    # the mask: query row i sits at position past + i
    if hidden.any():
        assert float(probs[..., hidden].abs().max()) == 0.0
    # rows sum to 1 within fp32 rounding: the sum the kernel divides by is built from the very terms it stores, so what is left is the
    # rounding of that sum (per lane ceil(Lk / 64) adds, then 6 tree levels), of 1 / sum and of each product -- 2^-24 each, doubled
    assert float((probs.double().sum(-1) - 1).abs().max()) < (8 + Lk / 64) * 2.0 ** -23
    # no atomics, fixed summation order: a second run gives the same bits
    out2, probs2, after2 = _run(shape, new, caches)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(probs), _bits(probs2)) and torch.equal(_bits(after), _bits(after2))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_first_pass_agrees_with_attention_fwd_causal(dt):
    """Lq == Lk fills the cache and is afft_attention_fwd(mask = causal) to rounding: each within the dtype's tolerance of the other"""
    from afft_amd import ops
    from afft_amd._lib import MASK_CAUSAL
    shape = (2, 2, 64, 4, 4, 8)
    nseq, H, hd, Lq, Lk, cap = shape
    d = H * hd
    new, caches = _inputs(shape, dt)
    out, probs, _ = _run(shape, new, caches)
    n = new.cuda()
    out_f = torch.empty_like(n[:, :d].contiguous())
    probs_f = torch.empty(nseq, H, Lk, Lk, device=n.device)
    ops.attention_fwd(n[:, :d], n[:, d:2 * d], n[:, 2 * d:], nseq, Lk, H, hd, hd ** -0.5, MASK_CAUSAL, out_f, probs_f)
    torch.cuda.synchronize()
    assert rel_l2(out.float(), out_f.float().cpu()) < TOL[dt][0] and rel_l2(probs, probs_f.cpu()) < TOL[dt][1]


def test_refused_arguments_raise_without_a_launch():
    """host checks, not faults: the error comes back through ops and the buffers are as they were"""
    from afft_amd import _lib, ops
    dev = torch.device("cuda:0")
    nseq, H, hd, cap = 2, 2, 64, 8
    d = H * hd
    new = torch.randn(nseq * 4, 3 * d, device=dev)
    caches = torch.zeros(2, nseq, cap, d, device=dev)
    out = torch.zeros(nseq * 4, d, device=dev)
    q, k, v = new[:, :d], new[:, d:2 * d], new[:, 2 * d:]
    for Lq, Lk, text in ((4, 3, "4 new rows against 3 keys"), (1, 9, "9 keys do not fit a cache of 8 rows")):
        with pytest.raises(RuntimeError, match=text):
            ops.attention_step(q, k, v, caches[0], caches[1], nseq, Lq, Lk, H, hd, 0.125, out, None)
    big = torch.zeros(2, 1, 520, d, device=dev)
    with pytest.raises(RuntimeError, match="sequence length 513 outside 1..512"):
        ops.attention_step(q[:1], k[:1], v[:1], big[0], big[1], 1, 1, 513, H, hd, 0.125, out[:1], None)
    rc = _lib.lib().afft_attention_step_fwd(q.data_ptr(), 3 * d, k.data_ptr(), 3 * d, v.data_ptr(), 3 * d, None, caches[1].data_ptr(), d, cap * d,
                                            _lib.F32, nseq, 1, 4, cap, H, hd, 0.125, out.data_ptr(), d, None, None)
    assert rc != 0 and "null pointer" in _lib.lib().afft_last_error().decode()
    torch.cuda.synchronize()
    assert float(caches.abs().max()) == 0.0 and float(out.abs().max()) == 0.0 and float(big.abs().max()) == 0.0
