"""CPU: the float64 restatement of the momentum-SGD update (tests/sgd_double.py), which the GPU tests hold the update kernels and the
fused GEMM epilogue against, is itself held against torch.optim.SGD in float64, and its fragment-packed index map against the torch
restatement of afft_pack_weight the B-direct GEMM tests use."""
import pytest
import torch

import sgd_double as sd


@pytest.mark.parametrize("flags", sd.FLAG_WORDS)
def test_reference_is_torch_sgd_in_float64(flags):
    """two steps from the state the flag word describes: FIRST_STEP = no momentum buffer yet (torch creates it from the gradient),
    otherwise a buffer that exists; PLAIN_MOMENTUM = nesterov=False.  gscale multiplies the gradient torch is handed."""
    gen = torch.Generator().manual_seed(11 + flags)
    n, lr, mom, wd, gscale = 257, 0.05, 0.9, 1e-3, 0.5
    p0, buf0 = torch.randn(n, generator=gen, dtype=torch.float64), torch.randn(n, generator=gen, dtype=torch.float64)
    grads = [torch.randn(n, generator=gen, dtype=torch.float64) for _ in range(2)]
    w = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([w], lr=lr, momentum=mom, weight_decay=wd, dampening=0.0, nesterov=not flags & sd.PLAIN_MOMENTUM)
    if not flags & sd.FIRST_STEP:
        opt.state[w]["momentum_buffer"] = buf0.clone()
    p, buf = p0, torch.full_like(buf0, float("nan")) if flags & sd.FIRST_STEP else buf0      # a first step must not read buf
    for k, g in enumerate(grads):
        w.grad = gscale * g
        opt.step()
        p, buf = sd.sgd_ref(p, buf, g, lr, mom, wd, gscale, flags if k == 0 else flags & ~sd.FIRST_STEP)
        torch.testing.assert_close(p, w.detach(), rtol=1e-14, atol=1e-15)
        torch.testing.assert_close(buf, opt.state[w]["momentum_buffer"], rtol=1e-14, atol=1e-15)
    assert not torch.equal(p, p0)


def test_stages_and_bound_cover_an_fp32_evaluation():
    """the five-rounding bound holds for the update evaluated step by step in fp32 (each product and sum rounded: at least the
    roundings of the device function), and is tight enough to notice one fp32 ulp of the step on p"""
    gen = torch.Generator().manual_seed(5)
    n = 4096
    p, buf, g = (torch.randn(n, generator=gen) for _ in range(3))
    lr, mom, wd, gs = (sd.f32(x) for x in (0.05, 0.9, 1e-3, 0.5))
    for flags in sd.FLAG_WORDS:
        pr, br = sd.sgd_ref(p, buf, g, lr, mom, wd, gs, flags)
        ep, eb = sd.sgd_bound(p, buf, g, lr, mom, wd, gs, flags)
        # fused multiply-adds as the kernel's: exact product in float64, one rounding of the sum
        fma = lambda a, b, c: (a.double() * b.double() + c.double()).float()      # noqa: E731
        T = lambda x: torch.tensor(x, dtype=torch.float32)      # noqa: E731
        g1 = fma(g, T(gs), (T(wd) * p))
        b = g1 if flags & sd.FIRST_STEP else fma(T(mom), buf, g1)
        s = b if flags & sd.PLAIN_MOMENTUM else fma(T(mom), b, g1)
        pn = fma(T(-lr), s, p)
        assert bool(((pn.double() - pr).abs() <= ep).all()) and bool(((b.double() - br).abs() <= eb).all())
        # a few ulp of the operands, not a tolerance a wrong term hides in
        assert bool((ep <= 4 * sd.U * (p.abs() + lr * (g.abs() + buf.abs()))).all()) and bool((eb <= 4 * sd.U * (g.abs() + buf.abs() + p.abs())).all())


def test_images_round_once_and_saturate():
    p = torch.tensor([0.0, 1.0, 1.00390625, 1.75, 1.7578125, -3.0, 2.0 ** -10, 1.0 + 2.0 ** -9, 0.0048828125])
    im = sd.images(p)
    assert im["bf16"].tolist() == [0.0, 1.0, 1.0, 1.75, 1.7578125, -3.0, 2.0 ** -10, 1.0, 0.0048828125]      # ties to even
    assert im["f16"].float().tolist()[7] == 1.0 + 2.0 ** -9
    # 256 p = 0, 256, 257, 448, 450, -768, 0.25, .., 1.25: e4m3fn codes (bias 7, 3 mantissa bits, 0x7e = 448 the largest)
    assert im["f8"].tolist()[:7] == [0x00, 0x78, 0x78, 0x7E, 0x7E, 0xFE, 0x28]
    assert im["f8"].tolist()[8] == 0x3A


@pytest.mark.parametrize("rows,cols", [(32, 64), (48, 96)])
def test_packed_index_map_is_the_pack_weight_layout(rows, cols):
    from test_kernels_gpu import _pack_ref
    w = torch.arange(rows * cols, dtype=torch.float32).reshape(rows, cols)
    table = sd.packed_frag(rows, cols)
    want = _pack_ref(w)
    got = torch.empty(rows * cols)
    got[table.reshape(-1)] = w.reshape(-1)
    assert torch.equal(got, want)
    assert sorted(table.reshape(-1).tolist()) == list(range(rows * cols))
    wb = torch.randn(rows, cols)
    assert torch.equal(sd.packed_image(wb), _pack_ref(wb.to(torch.bfloat16)))
