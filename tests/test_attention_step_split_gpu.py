"""GPU: afft_attention_step_fwd_split (csrc/attention_step.hip, the cached step on the operand planes of the 'fp16x2' forward) against
float64 torch math on the joined values hi + lo, and afft_attn_step_sublayer_fwd (csrc/sublayer.hip) against its four pieces called one by
one.

Bars.  probs: relative L2 2e-5, the bar tests/test_attention_step_gpu.py applies to its fp32-storage cases (the arithmetic between load and
store is the same fp32 code).  Appended cache rows: exactly float(hi) + float(lo).  ao, element by element, with m = max |ref|:
  with a lo plane   |hi + lo - ref| <= 2e-5 m + 2^-21 m   (fp16(x) leaves at most 2^-11 |x|, fp16 of that residue at most 2^-22 |x|; fp16
                                                            subnormal residues add at most 2^-25 absolute: 2^-21 m covers both)
  hi plane only     |hi - ref|      <= 2e-5 m + 2^-11 m   (fp16's half ulp)
where 2e-5 m is the fp32 bar above taken at the largest element."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import rel_l2  # noqa: E402

NSEQ, H = 3, 2
BAR = 2e-5
# (hd, Lq, past, odd pitch): the smallest shapes at which each path of the kernel can go wrong
SHAPES = ([(64, Lq, past, False) for Lq in (1, 4, 5) for past in (0, 3, 17)]                       # 16-byte accesses: one row / a tile / a tile + tail
          + [(24, 1, 17, False), (24, 5, 3, False), (24, 4, 0, False)]                             # 16-byte accesses, hd no multiple of the wave's stride
          + [(20, 1, 17, True), (20, 5, 3, True), (20, 4, 0, True)]                                # element accesses (an odd pitch)
          + [(64, 1, 511, False),                                                                  # the corner Lq = 1, Lk = 512
             (64, 37, 0, False), (20, 37, 0, True)])                                               # prefill at a non-multiple of 4
# (in_lo given, out_lo given, probs given)
FORMS = [(True, True, True), (False, True, True), (True, False, True), (False, False, True), (True, True, False)]
_CASES = {}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _case(shape):
    """inputs and float64 references of a shape, for both input forms: made once, shared, never modified"""
    if shape not in _CASES:
        hd, Lq, past, odd = shape
        d, Lk, R = H * hd, past + Lq, NSEQ * Lq
        g = torch.Generator().manual_seed(100 * hd + 10 * Lq + past)
        x = torch.randn(R, 3 * d, generator=g)
        hi = x.half()
        lo = (x - hi.float()).half()
        old = torch.randn(2, NSEQ, past, d, generator=g)
        ref = {}
        for with_lo in (True, False):
            n = (hi.double() + lo.double() if with_lo else hi.double()).view(NSEQ, Lq, 3, H, hd)
            q = n[:, :, 0].permute(0, 2, 1, 3)
            k, v = (torch.cat([old[i].double(), n[:, :, 1 + i].reshape(NSEQ, Lq, d)], 1).view(NSEQ, Lk, H, hd).permute(0, 2, 1, 3) for i in (0, 1))
            hidden = torch.arange(Lk)[None, :] > past + torch.arange(Lq)[:, None]
            p = torch.softmax((q @ k.transpose(-1, -2) * hd ** -0.5).masked_fill(hidden, float("-inf")), -1)
            new32 = hi.float() + lo.float() if with_lo else hi.float()      # what the caches must hold, bit for bit
            ref[with_lo] = ((p @ v).permute(0, 2, 1, 3).reshape(R, d), p, hidden, new32)
        _CASES[shape] = (hi, lo, old, ref)
    return _CASES[shape]


def _run(shape, form):
    """-> out planes [2, R, ldo] fp16 (hi, lo), probs or None, the caches [2, NSEQ, cap, ldc] with their pad columns"""
    from afft_amd import ops
    hd, Lq, past, odd = shape
    in_lo, out_lo, want_probs = form
    hi, lo, old, _ = _case(shape)
    d, Lk, R = H * hd, past + Lq, NSEQ * Lq
    cap = Lk + 2
    dev = torch.device("cuda:0")
    ld, ldo, ldc = (3 * d + 1, d + 1, d + 1) if odd else (3 * d, d + 8, d + 8)
    new = torch.full((2, R, ld), float("nan"), dtype=torch.float16)      # a lo plane the call does not name must not be read: it stays NaN
    new[0, :, :3 * d] = hi
    if in_lo:
        new[1, :, :3 * d] = lo
    caches = torch.full((2, NSEQ, cap, ldc), float("nan"))               # rows and columns the kernel must neither read nor write stay NaN
    caches[:, :, :past, :d] = old
    n, c = new.to(dev), caches.to(dev)
    out = torch.full((2, R, ldo), float("nan"), dtype=torch.float16, device=dev)
    probs = torch.full((NSEQ, H, Lq, Lk), float("nan"), device=dev) if want_probs else None
    ops.attention_step_split(n[0, :, :d], n[0, :, d:2 * d], n[0, :, 2 * d:3 * d], R * ld if in_lo else 0, c[0, :, :, :d], c[1, :, :, :d], NSEQ, Lq, Lk,
                             H, hd, hd ** -0.5, out[0, :, :d], R * ldo if out_lo else 0, probs)
    torch.cuda.synchronize()
    return out.cpu(), None if probs is None else probs.cpu(), c.cpu()


@pytest.mark.parametrize("form", FORMS, ids=lambda f: "in%d-out%d-probs%d" % tuple(map(int, f)))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "hd%d-Lq%d-past%d%s" % (s[0], s[1], s[2], "-odd" if s[3] else ""))
def test_split_step_matches_float64_and_appends(shape, form):
    hd, Lq, past, odd = shape
    in_lo, out_lo, want_probs = form
    d, Lk, R = H * hd, past + Lq, NSEQ * Lq
    from afft_amd import _lib
    assert _lib.lib().afft_attention_step_split_plan_for(Lq, Lk, hd, int(in_lo), int(out_lo), 0 if odd else 1, None) == 130000 + (0 if odd else 10)
    o_ref, p_ref, hidden, new32 = _case(shape)[3][in_lo]
    old = _case(shape)[2]
    out, probs, after = _run(shape, form)
    m = float(o_ref.abs().max())
    joined = out[0, :, :d].double() + (out[1, :, :d].double() if out_lo else 0.0)
    e_out = float((joined - o_ref).abs().max())
    bound = BAR * m + (2.0 ** -21 if out_lo else 2.0 ** -11) * m
    e_p = rel_l2(probs, p_ref.float()) if want_probs else 0.0
    print(f"[{shape}/{form}] max |ao - ref| {e_out:.3e} (bound {bound:.3e}, max |ref| {m:.3f})  probs rel L2 {e_p:.2e}")
    assert torch.isfinite(joined).all()
    assert e_out <= bound
    # the planes follow the producers' rule: hi = fp16(x), lo = fp16(x - hi) -- so hi alone is within fp16's half ulp either way
    assert float((out[0, :, :d].double() - o_ref).abs().max()) <= BAR * m + 2.0 ** -11 * m
    assert torch.isnan(out[0, :, d:].float()).all()                                  # pad columns
    if not out_lo:
        assert torch.isnan(out[1].float()).all()                                     # no lo plane asked for: none written
    else:
        assert torch.isnan(out[1, :, d:].float()).all()
    if want_probs:
        assert torch.isfinite(probs).all() and e_p < BAR
        if hidden.any():
            assert float(probs[..., hidden].abs().max()) == 0.0                      # exact zeros behind the diagonal
        assert float((probs.double().sum(-1) - 1).abs().max()) < (8 + Lk / 64) * 2.0 ** -23      # tests/test_attention_step_gpu.py's argument
    # the caches: the past untouched, the new rows = float(hi) + float(lo) exactly, nothing else written
    assert torch.isnan(after[:, :, Lk:]).all() and torch.isnan(after[:, :, :, d:]).all()
    assert torch.equal(_bits(after[:, :, :past, :d]), _bits(old))
    for i in (0, 1):
        assert torch.equal(_bits(after[i, :, past:Lk, :d]), _bits(new32[:, (1 + i) * d:(2 + i) * d].reshape(NSEQ, Lq, d)))
    # no atomics, fixed summation order: a second run gives the same bits
    out2, probs2, after2 = _run(shape, form)
    keep = ~torch.isnan(out.float())
    assert torch.equal(keep, ~torch.isnan(out2.float())) and torch.equal(_bits(out)[keep], _bits(out2)[keep])
    keep = ~torch.isnan(after)
    assert torch.equal(_bits(after)[keep], _bits(after2)[keep])
    if want_probs:
        assert torch.equal(_bits(probs), _bits(probs2))


def test_one_plane_form_equals_two_planes_with_a_zero_lo():
    """in_lo = 0 is 'the lo plane is zero', bit for bit (float(hi) + 0.0 is float(hi))"""
    from afft_amd import ops
    hd, Lq, past = 64, 5, 3
    d, Lk, R = H * hd, past + Lq, NSEQ * Lq
    hi, _, old, _ = _case((hd, Lq, past, False))
    dev = torch.device("cuda:0")
    res = []
    for with_lo in (False, True):
        n = torch.zeros(2, R, 3 * d, dtype=torch.float16, device=dev)
        n[0] = hi.to(dev)
        c = torch.zeros(2, NSEQ, Lk, d, device=dev)
        c[:, :, :past] = old.to(dev)
        out = torch.zeros(2, R, d, dtype=torch.float16, device=dev)
        probs = torch.zeros(NSEQ, H, Lq, Lk, device=dev)
        ops.attention_step_split(n[0, :, :d], n[0, :, d:2 * d], n[0, :, 2 * d:], R * 3 * d if with_lo else 0, c[0], c[1], NSEQ, Lq, Lk, H, hd, hd ** -0.5,
                                 out[0], R * d, probs)
        torch.cuda.synchronize()
        res.append((out.cpu(), probs.cpu(), c.cpu()))
    for a, b in zip(*res):
        assert torch.equal(_bits(a), _bits(b))


def test_refused_arguments_raise_without_a_launch():
    """host checks, not faults: the error comes back through ops and the buffers are as they were"""
    from afft_amd import ops
    dev = torch.device("cuda:0")
    hd, cap = 64, 8
    d = H * hd
    new = torch.zeros(2, NSEQ * 4, 3 * d, dtype=torch.float16, device=dev)
    caches = torch.zeros(2, NSEQ, cap, d, device=dev)
    out = torch.zeros(2, NSEQ * 4, d, dtype=torch.float16, device=dev)
    q, k, v = new[0, :, :d], new[0, :, d:2 * d], new[0, :, 2 * d:]
    for Lq, Lk, in_lo, out_lo, text in ((4, 3, 0, 0, "4 new rows against 3 keys"), (4, 9, 0, 0, "9 keys do not fit a cache of 8 rows"),
                                        (4, 4, d, 0, "in_lo 128 lies inside the hi plane"), (4, 4, 0, d, "out_lo 128 lies inside the hi plane")):
        with pytest.raises(RuntimeError, match=text):
            ops.attention_step_split(q, k, v, in_lo, caches[0], caches[1], NSEQ, Lq, Lk, H, hd, 0.125, out[0], out_lo, None)
    with pytest.raises(AssertionError):
        ops.attention_step_split(q, k, v, 0, caches[0].half(), caches[1].half(), NSEQ, 4, 4, H, hd, 0.125, out[0], 0, None)      # fp32 caches only
    torch.cuda.synchronize()
    assert float(caches.abs().max()) == 0.0 and float(out.float().abs().max()) == 0.0


# ---------------------------------------------------------------- the composite entry against its four pieces
D, B = 128, 3
FLAGS = {"two-pass": 0, "one-pass-gemms": 4 | 8, "one-pass-all": 4 | 8 | 16}      # AFFT_F16X2_ONE_PASS_1 | _2 (| _ATTN)


def _weights():
    g = torch.Generator().manual_seed(7)
    dev = torch.device("cuda:0")
    r = lambda *s, k=1.0: (k * torch.randn(*s, generator=g))      # noqa: E731
    return dict(ln_w=(1 + 0.1 * r(D)).to(dev), ln_b=(0.1 * r(D)).to(dev), w_qkv=r(D, 3 * D, k=0.05).half().to(dev), b_qkv=(0.1 * r(3 * D)).to(dev),
                w_proj=r(D, D, k=0.05).half().to(dev), b_proj=(0.1 * r(D)).to(dev))


@pytest.mark.parametrize("Lq", [5, 1])
@pytest.mark.parametrize("name", list(FLAGS))
def test_composite_step_equals_its_pieces_bitwise(name, Lq):
    from afft_amd import _lib, ops
    assert (_lib.F16X2_ONE_PASS_1, _lib.F16X2_ONE_PASS_2, _lib.F16X2_ONE_PASS_ATTN) == (4, 8, 16)
    flags = 1 | FLAGS[name]
    one1, one2, one_attn = bool(flags & 4), bool(flags & 8), bool(flags & 16)
    dev = torch.device("cuda:0")
    hd, past, eps = D // H, 3, 1e-5
    Lk, R = past + Lq, B * Lq
    pr = (R + 63) // 64 * 64
    w = _weights()
    g = torch.Generator().manual_seed(20 + Lq)
    x = torch.randn(R, D, generator=g).to(dev)
    old = torch.randn(2, B, past, D, generator=g).to(dev)

    def fresh():
        c = torch.zeros(2, B, Lk + 1, D, device=dev)
        c[:, :, :past] = old
        bufs = [torch.full((2 * pr * width,), float("nan"), dtype=torch.float16, device=dev) for width in (D, 3 * D, D)]
        return c, bufs, torch.empty(B, H, Lq, Lk, device=dev), torch.empty(R, D, device=dev)

    c1, (xn, qkv, ao), p1, y1 = fresh()
    ops.attn_step_sublayer_f16x2(x, w["ln_w"], w["ln_b"], w["w_qkv"], w["b_qkv"], w["w_proj"], w["b_proj"], flags, Lq, Lk, H, eps, hd ** -0.5,
                                 xn, qkv, ao, c1[0], c1[1], p1, y1)
    torch.cuda.synchronize()
    # rows R .. pr - 1 of every plane that is written are zero; a plane the flags leave out is not touched
    for buf, width, has_lo in ((xn, D, not one1), (qkv, 3 * D, not one_attn), (ao, D, not one2)):
        planes = buf.view(2, pr, width).float().cpu()
        assert torch.isfinite(planes[0, :R]).all() and float(planes[0, R:].abs().max()) == 0.0
        if has_lo:
            assert torch.isfinite(planes[1, :R]).all() and float(planes[1, R:].abs().max()) == 0.0
        else:
            assert torch.isnan(planes[1]).all()

    c2, (xn, qkv, ao), p2, y2 = fresh()

    def operand(buf, width, two):
        planes = buf.view(2, pr, width)
        if not two:
            return planes[0, :R]
        s = ops.Split.__new__(ops.Split)
        s.planes, s.rows, s.cols, s.f16 = planes, R, width, True
        return s
    ops.layernorm_fwd_split(x, w["ln_w"], w["ln_b"], eps, xn.view(2, pr, D)[0, :R], 0 if one1 else pr * D)
    q3 = qkv.view(2, pr, 3 * D)[0, :R]
    ops.gemm(operand(xn, D, not one1), w["w_qkv"], q3, bias=w["b_qkv"], out_lo=0 if one_attn else pr * 3 * D)
    ops.attention_step_split(q3[:, :D], q3[:, D:2 * D], q3[:, 2 * D:], 0 if one_attn else pr * 3 * D, c2[0], c2[1], B, Lq, Lk, H, hd, hd ** -0.5,
                             ao.view(2, pr, D)[0, :R], 0 if one2 else pr * D, p2)
    ops.gemm(operand(ao, D, not one2), w["w_proj"], y2, bias=w["b_proj"], residual=x)
    torch.cuda.synchronize()
    assert torch.isfinite(y1).all()
    assert torch.equal(_bits(y1.cpu()), _bits(y2.cpu())) and torch.equal(_bits(p1.cpu()), _bits(p2.cpu())) and torch.equal(_bits(c1.cpu()), _bits(c2.cpu()))
    # and the whole agrees with float64 on the same (fp16-rounded) weights within the precision's bar
    xd = torch.nn.functional.layer_norm(x.double().cpu(), (D,), w["ln_w"].double().cpu(), w["ln_b"].double().cpu(), eps)
    n = (xd @ w["w_qkv"].double().cpu() + w["b_qkv"].double().cpu()).view(B, Lq, 3, H, hd)
    k, v = (torch.cat([old[i].double().cpu(), n[:, :, 1 + i].reshape(B, Lq, D)], 1).view(B, Lk, H, hd).permute(0, 2, 1, 3) for i in (0, 1))
    hidden = torch.arange(Lk)[None, :] > past + torch.arange(Lq)[:, None]
    p = torch.softmax((n[:, :, 0].permute(0, 2, 1, 3) @ k.transpose(-1, -2) * hd ** -0.5).masked_fill(hidden, float("-inf")), -1)
    y = x.double().cpu() + (p @ v).permute(0, 2, 1, 3).reshape(R, D) @ w["w_proj"].double().cpu() + w["b_proj"].double().cpu()
    tol = 1e-3 if name == "two-pass" else 2e-3      # tests/test_model_gpu.py: TOL['fp16x2'], and its bar for one-pass sites on small models
    assert rel_l2(y1.cpu(), y.float()) < tol and rel_l2(p1.cpu(), p.float()) < tol
