"""GPU: afft_attention_step_bwd and afft_attention_step_fwd_drop (csrc/attention_step.hip) -- the backward of the cached attention step with
its gradient caches, and the step's attention-probability dropout -- against float64 autograd of the arithmetic include/afft_hip.h states,
in both storage dtypes, with the tolerances tests/test_kernels_gpu.py applies to afft_attention_bwd (relative L2: 3e-5 fp32, 2e-2 bf16)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import rel_l2  # noqa: E402

# (nseq, H, hd, Lq, Lk, cap): the shapes of tests/test_attention_step_gpu.py, plus more than two row tiles in the first pass
SHAPES = [(3, 2, 64, 1, 1, 4), (3, 2, 64, 1, 17, 20), (2, 3, 24, 1, 5, 5), (2, 2, 64, 3, 19, 32), (2, 2, 64, 4, 4, 8),
          (2, 4, 512, 16, 16, 19), (1, 4, 512, 1, 19, 19), (1, 2, 64, 1, 130, 160), (1, 1, 64, 1, 512, 512), (2, 2, 10, 6, 9, 11),
          (1, 1, 64, 9, 9, 12)]
TOL = {"f32": 3e-5, "bf16": 2e-2}
P_DROP, KEY = 0.3, 12345


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _tdt(dt):
    return torch.float32 if dt == "f32" else torch.bfloat16


def _inputs(shape, dt, seed=0):
    """q and dout of the new rows, the caches as the forward leaves them (rows < Lk valid, NaN behind), gradient caches with random
    rows < Lk and NaN behind"""
    nseq, H, hd, Lq, Lk, cap = shape
    d = H * hd
    g = torch.Generator().manual_seed(23 + Lk + seed)
    q = torch.randn(nseq * Lq, d, generator=g).to(_tdt(dt))
    dout = torch.randn(nseq * Lq, d, generator=g).to(_tdt(dt))
    caches = torch.full((2, nseq, cap, d), float("nan"), dtype=_tdt(dt))
    caches[:, :, :Lk] = torch.randn(2, nseq, Lk, d, generator=g).to(_tdt(dt))
    gcaches = torch.full((2, nseq, cap, d), float("nan"))
    gcaches[:, :, :Lk] = torch.randn(2, nseq, Lk, d, generator=g)
    return q, dout, caches, gcaches


def _heads(t, nseq, L, H, hd):
    return t.double().reshape(nseq, L, H, hd).permute(0, 2, 1, 3)


def _reference(shape, q, dout, caches, M=None):
    """float64 autograd of out = ((softmax over the visible keys) o M) V: (P, out, dq, cK, cV), rows as [nseq * L, d]"""
    nseq, H, hd, Lq, Lk, cap = shape
    d, past = H * hd, Lk - Lq
    qh = _heads(q, nseq, Lq, H, hd).requires_grad_(True)
    kh = _heads(caches[0, :, :Lk], nseq, Lk, H, hd).requires_grad_(True)
    vh = _heads(caches[1, :, :Lk], nseq, Lk, H, hd).requires_grad_(True)
    hidden = torch.arange(Lk)[None, :] > past + torch.arange(Lq)[:, None]
    p = torch.softmax((qh @ kh.transpose(-1, -2) * hd ** -0.5).masked_fill(hidden, float("-inf")), -1)
    out = (p if M is None else p * M.double()) @ vh
    out.backward(_heads(dout, nseq, Lq, H, hd))
    back = lambda t, L: t.permute(0, 2, 1, 3).reshape(nseq, L, d)   # noqa: E731
    return p.detach(), back(out.detach(), Lq).reshape(nseq * Lq, d), back(qh.grad, Lq).reshape(nseq * Lq, d), back(kh.grad, Lk), back(vh.grad, Lk)


def _run_bwd(shape, q, dout, caches, gcaches, probs, drop=None):
    from afft_amd import ops
    nseq, H, hd, Lq, Lk, cap = shape
    d = H * hd
    dev = torch.device("cuda:0")
    c, gc = caches.to(dev), gcaches.to(dev)
    dqkv = torch.full((nseq * Lq, 3 * d), float("nan"), dtype=q.dtype, device=dev)
    ops.attention_step_bwd(dout.to(dev), q.to(dev), c[0], c[1], probs.to(dev), nseq, Lq, Lk, H, hd, hd ** -0.5, dqkv[:, :d], dqkv[:, d:2 * d],
                           dqkv[:, 2 * d:], gc[0], gc[1], drop=drop)
    torch.cuda.synchronize()
    return dqkv.cpu(), c.cpu(), gc.cpu()


def _check(shape, dt, q, dout, caches, gcaches, probs, ref, drop=None):
    nseq, H, hd, Lq, Lk, cap = shape
    d, past = H * hd, Lk - Lq
    _, _, dq_ref, ck, cv = ref
    dqkv, c_after, g_after = _run_bwd(shape, q, dout, caches, gcaches, probs, drop)
    want_new = [(gcaches[i, :, past:Lk].double() + (ck, cv)[i][:, past:]).reshape(nseq * Lq, d) for i in (0, 1)]
    errs = {"dq": rel_l2(dqkv[:, :d].float(), dq_ref.float()), "dk_new": rel_l2(dqkv[:, d:2 * d].float(), want_new[0].float()),
            "dv_new": rel_l2(dqkv[:, 2 * d:].float(), want_new[1].float())}
    if past:
        for i, nm in ((0, "gk"), (1, "gv")):
            errs[nm] = rel_l2(g_after[i, :, :past], (gcaches[i, :, :past].double() + (ck, cv)[i][:, :past]).float())
    print(f"[{shape}/{dt}{'/drop' if drop else ''}] " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert torch.isfinite(dqkv.float()).all()
    for k, v in errs.items():
        assert v < TOL[dt], (k, v)
    # rows [past, Lk) of the gradient caches are read and keep their bits, rows >= Lk stay NaN, the key / value caches are untouched
    assert torch.equal(_bits(g_after[:, :, past:Lk]), _bits(gcaches[:, :, past:Lk]))
    assert torch.isnan(g_after[:, :, Lk:]).all()
    assert torch.equal(_bits(c_after), _bits(caches))
    return dqkv, g_after


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_step_bwd_matches_float64_and_keeps_the_write_rule(shape, dt):
    q, dout, caches, gcaches = _inputs(shape, dt)
    ref = _reference(shape, q, dout, caches)
    probs = ref[0].float().contiguous()
    dqkv, g_after = _check(shape, dt, q, dout, caches, gcaches, probs, ref)
    # no atomics, fixed summation order: a second run gives the same bits
    dqkv2, _, g_after2 = _run_bwd(shape, q, dout, caches, gcaches, probs)
    assert torch.equal(_bits(dqkv), _bits(dqkv2)) and torch.equal(_bits(g_after), _bits(g_after2))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_first_pass_agrees_with_attention_bwd_causal(dt):
    """Lq == Lk with a zero gradient cache is afft_attention_bwd on the causal probabilities, each within the dtype's tolerance of the other"""
    from afft_amd import ops
    from afft_amd._lib import MASK_CAUSAL
    shape = (2, 2, 64, 4, 4, 8)
    nseq, H, hd, Lq, Lk, cap = shape
    d = H * hd
    q, dout, caches, gcaches = _inputs(shape, dt)
    gcaches[:, :, :Lk] = 0.0
    dev = torch.device("cuda:0")
    qd, dd = q.to(dev), dout.to(dev)
    k, v = (caches[i, :, :Lk].reshape(nseq * Lk, d).contiguous().to(dev) for i in (0, 1))
    out = torch.empty_like(qd)
    probs = torch.empty(nseq, H, Lk, Lk, device=dev)
    ops.attention_fwd(qd, k, v, nseq, Lk, H, hd, hd ** -0.5, MASK_CAUSAL, out, probs)
    dg = torch.empty(nseq * Lk, 3 * d, dtype=q.dtype, device=dev)
    ops.attention_bwd(dd, qd, k, v, probs, nseq, Lk, H, hd, hd ** -0.5, dg[:, :d], dg[:, d:2 * d], dg[:, 2 * d:])
    dqkv, _, _ = _run_bwd(shape, q, dout, caches, gcaches, probs.cpu())
    for i, nm in enumerate(("dq", "dk", "dv")):
        e = rel_l2(dqkv[:, i * d:(i + 1) * d].float(), dg[:, i * d:(i + 1) * d].float().cpu())
        assert e < TOL[dt], (nm, e)


def _fwd(shape, new, caches, drop, want_probs=True):
    """ops.attention_step on new [nseq * Lq, 3 d] (q | k | v) and caches [2, nseq, cap, d]: (out, probs, caches after)"""
    from afft_amd import ops
    nseq, H, hd, Lq, Lk, cap = shape
    d = H * hd
    dev = torch.device("cuda:0")
    n, c = new.to(dev), caches.to(dev)
    out = torch.empty(nseq * Lq, d, dtype=new.dtype, device=dev)
    probs = torch.full((nseq, H, Lq, Lk), float("nan"), device=dev) if want_probs else None
    ops.attention_step(n[:, :d], n[:, d:2 * d], n[:, 2 * d:], c[0], c[1], nseq, Lq, Lk, H, hd, hd ** -0.5, out, probs, drop=drop)
    torch.cuda.synchronize()
    return out.cpu(), probs.cpu() if want_probs else None, c.cpu()


def _mask_off_the_device(shape, new, caches, drop):
    """one forward call whose value rows are the identity (hd >= Lk): out row i of head h is P'_i.  Returns (P, P') [nseq, H, Lq, Lk]"""
    nseq, H, hd, Lq, Lk, cap = shape
    d, past = H * hd, Lk - Lq
    assert hd >= Lk
    eye = torch.eye(Lk, hd).repeat(1, H)                       # key j's value row: e_j in every head
    n, c = new.clone(), caches.clone()
    n[:, 2 * d:] = eye[past:].repeat(nseq, 1)
    c[1, :, :past] = eye[:past]
    out, probs, _ = _fwd(shape, n, c, drop)
    return probs, out.view(nseq, Lq, H, hd).permute(0, 2, 1, 3)[..., :Lk].contiguous()


def _visible(shape):
    nseq, H, hd, Lq, Lk, cap = shape
    return (torch.arange(Lk)[None, :] <= Lk - Lq + torch.arange(Lq)[:, None]).expand(nseq, H, Lq, Lk)


@pytest.mark.parametrize("shape", [(2, 2, 64, 3, 19, 32), (2, 2, 64, 4, 4, 8)], ids=lambda s: "x".join(map(str, s)))
def test_dropout_forward_and_backward_against_float64_with_the_device_mask(shape):
    nseq, H, hd, Lq, Lk, cap = shape
    d, past = H * hd, Lk - Lq
    g = torch.Generator().manual_seed(5 + Lk)
    new = torch.randn(nseq * Lq, 3 * d, generator=g)
    caches = torch.full((2, nseq, cap, d), float("nan"))
    caches[:, :, :past] = torch.randn(2, nseq, past, d, generator=g)
    P, Pd = _mask_off_the_device(shape, new, caches, (P_DROP, KEY))
    vis = _visible(shape)
    M = torch.where(vis, Pd / P.clamp_min(1e-30), torch.zeros(()))
    kept = M > 0.5
    # P' = P M with M in {0, 1 / (1 - p)}; the identity product adds exact zeros, so what is left is the rounding of p * dinv
    assert torch.equal(Pd[~kept], torch.zeros_like(Pd[~kept]))
    assert float((M[kept] * (1 - P_DROP) - 1).abs().max()) < 4 * 2.0 ** -23
    assert 0 < int((vis & ~kept).sum()) < int(vis.sum())
    Mx = torch.where(kept, torch.full((), 1 / (1 - P_DROP), dtype=torch.float64), torch.zeros((), dtype=torch.float64))
    # forward with real values and the same key
    out, probs, after = _fwd(shape, new, caches, (P_DROP, KEY))
    assert torch.equal(probs, P)                               # probs is pre-dropout and does not depend on the values
    gq = torch.Generator().manual_seed(6)
    dout = torch.randn(nseq * Lq, d, generator=gq)
    gcaches = torch.full((2, nseq, cap, d), float("nan"))
    gcaches[:, :, :Lk] = torch.randn(2, nseq, Lk, d, generator=gq)
    ref = _reference(shape, new[:, :d], dout, after, Mx)
    e_p, e_out = rel_l2(probs, ref[0].float()), rel_l2(out, ref[1].float())
    print(f"[{shape}/drop] probs {e_p:.2e} out {e_out:.2e}")
    assert e_p < 2e-5 and e_out < 2e-5                         # tests/test_attention_step_gpu.py's forward tolerances (fp32)
    _check(shape, "f32", new[:, :d].contiguous(), dout, after, gcaches, probs, ref, drop=(P_DROP, KEY))


def test_dropout_keeps_the_stated_fraction():
    shape = (8, 4, 64, 16, 16, 16)
    nseq, H, hd, Lq, Lk, cap = shape
    d = H * hd
    new = torch.randn(nseq * Lq, 3 * d, generator=torch.Generator().manual_seed(9))
    caches = torch.full((2, nseq, cap, d), float("nan"))
    P, Pd = _mask_off_the_device(shape, new, caches, (P_DROP, KEY + 1))
    vis = _visible(shape)
    n = int(vis.sum())
    frac = float(((Pd > 0) & vis).sum()) / n
    sd = (P_DROP * (1 - P_DROP) / n) ** 0.5
    print(f"kept {frac:.4f} of {n} visible elements (1 - p = {1 - P_DROP}, 5 sd = {5 * sd:.4f})")
    assert float(P[vis].min()) > 0 and abs(frac - (1 - P_DROP)) < 5 * sd


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_drop_entry_at_p_0_gives_the_bits_of_the_plain_entry(dt):
    from afft_amd import _lib
    shape = (2, 2, 64, 3, 19, 32)
    nseq, H, hd, Lq, Lk, cap = shape
    d, past = H * hd, Lk - Lq
    g = torch.Generator().manual_seed(3)
    new = torch.randn(nseq * Lq, 3 * d, generator=g).to(_tdt(dt))
    caches = torch.full((2, nseq, cap, d), float("nan"), dtype=_tdt(dt))
    caches[:, :, :past] = torch.randn(2, nseq, past, d, generator=g).to(_tdt(dt))
    out0, probs0, after0 = _fwd(shape, new, caches, None)
    dev = torch.device("cuda:0")
    n, c = new.to(dev), caches.to(dev)
    out = torch.empty(nseq * Lq, d, dtype=new.dtype, device=dev)
    probs = torch.full((nseq, H, Lq, Lk), float("nan"), device=dev)
    es = n.element_size()
    rc = _lib.lib().afft_attention_step_fwd_drop(n.data_ptr(), 3 * d, n.data_ptr() + d * es, 3 * d, n.data_ptr() + 2 * d * es, 3 * d,
                                                 c[0].data_ptr(), c[1].data_ptr(), d, cap * d, _lib.F32 if dt == "f32" else _lib.BF16, nseq, Lq, Lk,
                                                 cap, H, hd, hd ** -0.5, 0.0, KEY, out.data_ptr(), d, probs.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().afft_last_error().decode()
    assert torch.equal(_bits(out.cpu()), _bits(out0)) and torch.equal(_bits(probs.cpu()), _bits(probs0))
    assert torch.equal(_bits(c.cpu()), _bits(after0))


def test_refused_arguments_raise_without_a_launch():
    """host checks, not faults: the error comes back through ops and the buffers are as they were"""
    from afft_amd import _lib, ops
    dev = torch.device("cuda:0")
    nseq, H, hd, cap = 2, 2, 64, 8
    d = H * hd
    q = torch.randn(nseq * 4, d, device=dev)
    dout = torch.randn(nseq * 4, d, device=dev)
    caches = torch.zeros(2, nseq, cap, d, device=dev)
    gcaches = torch.zeros(2, nseq, cap, d, device=dev)
    dqkv = torch.zeros(nseq * 4, 3 * d, device=dev)
    probs = torch.zeros(nseq * H * 4 * 9, device=dev)
    dq, dk, dv = dqkv[:, :d], dqkv[:, d:2 * d], dqkv[:, 2 * d:]
    for Lq, Lk, text in ((4, 3, "4 new rows against 3 keys"), (1, 9, "9 keys do not fit a cache of 8 rows")):
        with pytest.raises(RuntimeError, match=text):
            ops.attention_step_bwd(dout, q, caches[0], caches[1], probs[:nseq * H * Lq * Lk], nseq, Lq, Lk, H, hd, 0.125, dq, dk, dv,
                                   gcaches[0], gcaches[1])
    big, gbig = torch.zeros(2, 1, 520, d, device=dev), torch.zeros(2, 1, 520, d, device=dev)
    with pytest.raises(RuntimeError, match="sequence length 513 outside 1..512"):
        ops.attention_step_bwd(dout[:1], q[:1], big[0], big[1], torch.zeros(H * 513, device=dev), 1, 1, 513, H, hd, 0.125, dq[:1], dk[:1],
                               dv[:1], gbig[0], gbig[1])
    lib = _lib.lib()

    def raw(gk, ldg):
        return lib.afft_attention_step_bwd(dout.data_ptr(), d, q.data_ptr(), d, caches[0].data_ptr(), caches[1].data_ptr(), d, cap * d, _lib.F32,
                                           probs.data_ptr(), nseq, 1, 4, cap, H, hd, 0.125, 0.0, 0, dq.data_ptr(), 3 * d, dk.data_ptr(), 3 * d,
                                           dv.data_ptr(), 3 * d, gk, gcaches[1].data_ptr(), ldg, cap * d, None)
    assert raw(None, d) != 0 and "null pointer" in lib.afft_last_error().decode()
    assert raw(gcaches[0].data_ptr(), d - 4) != 0 and "a row pitch is below H * hd" in lib.afft_last_error().decode()
    torch.cuda.synchronize()
    for t in (caches, gcaches, dqkv, big, gbig):
        assert float(t.abs().max()) == 0.0
