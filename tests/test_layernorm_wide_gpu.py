"""GPU: the LayerNorm backward for rows of 2049 to 4096 columns (csrc/norm.hip: 2 row groups x 8 column slices) against
torch.nn.functional.layer_norm in float64 on the CPU, on the same seeded inputs.

Bounds: the ones of test_kernels_gpu.py::test_layernorm_fwd_bwd -- dx, dw, db rel-L2 < 3e-5 (fp32 arithmetic, another summation
order), the bf16 copy < 5e-3 (bf16 output rounding), forward 2e-5 / 5e-3.  The masked copy is compared bit for bit: with element and
path rates of 0.5 every mask value is 0 or 4, so masking a number and rounding it to bf16 is exact on the host too."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import rel_l2  # noqa: E402

EPS = 1e-6


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def bfr(t):
    return t.to(torch.bfloat16).to(torch.float32)


@functools.lru_cache(maxsize=None)
def problem(rows, d, dt, affine=True):
    """seeded inputs of one LayerNorm and its float64 reference, computed once per (rows, d, dy dtype): (x, w, b, dy, y, dx, dw, db)
    with the reference's forward result and gradients as fp32 tensors"""
    x = rnd(rows, d, seed=1, scale=2.0) + 0.3
    w = rnd(d, seed=2) * 0.2 + 1.0 if affine else None
    b = rnd(d, seed=3) * 0.1 if affine else None
    dy = rnd(rows, d, seed=4)
    if dt == "bf16":
        dy = bfr(dy)
    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True) if affine else None
    br = b.double().requires_grad_(True) if affine else None
    yr = torch.nn.functional.layer_norm(xr, (d,), wr, br, EPS)
    yr.backward(dy.double())
    return (x, w, b, dy, yr.detach().float(), xr.grad.float(), wr.grad.float() if affine else None,
            br.grad.float() if affine else None)


def forward(x, w, b, ydt=torch.float32):
    """the library's forward on the GPU: (x on the GPU, y, mean, rstd)"""
    from afft_amd import ops
    rows, d = x.shape
    xg = x.to(dev())
    y = torch.empty(rows, d, dtype=ydt, device=dev())
    mean = torch.empty(rows, device=dev())
    rstd = torch.empty(rows, device=dev())
    ops.layernorm_fwd(xg, w.to(dev()) if w is not None else None, b.to(dev()) if b is not None else None, EPS, y, mean, rstd)
    return xg, y, mean, rstd


WIDE_CASES = [(70, 2052, "f32"),    # the smallest width past 2048: 513 float4 do not divide over the 8 slices
              (33, 3072, "bf16"),
              (130, 4096, "f32"),   # full width, several row steps per workgroup
              (5, 4096, "bf16"),    # fewer rows than row groups x 2
              (9, 2560, "bf16")]


@pytest.mark.parametrize("rows,d,dt", WIDE_CASES)
def test_wide_layernorm_fwd_bwd(rows, d, dt):
    from afft_amd import ops
    ydt = torch.float32 if dt == "f32" else torch.bfloat16
    x, w, b, dy, yr, dxr, dwr, dbr = problem(rows, d, dt)
    xg, y, mean, rstd = forward(x, w, b, ydt)
    assert rel_l2(y.float().cpu(), yr) < (2e-5 if dt == "f32" else 5e-3)
    dx_in = rnd(rows, d, seed=5)
    dx = torch.empty(rows, d, device=dev())
    dxb = torch.empty(rows, d, dtype=torch.bfloat16, device=dev())
    dw = torch.full((d,), 0.5, device=dev())
    db = torch.full((d,), -0.25, device=dev())
    dyg, wg = dy.to(ydt).to(dev()), w.to(dev())
    ops.layernorm_bwd(dyg, xg, wg, mean, rstd, dx, dx_in=dx_in.to(dev()), dx_bf16=dxb, dw=dw, db=db)
    torch.cuda.synchronize()
    assert rel_l2(dx.cpu(), dxr + dx_in) < 3e-5
    assert rel_l2(dxb.float().cpu(), dxr + dx_in) < 5e-3
    assert rel_l2(dw.cpu() - 0.5, dwr) < 3e-5
    assert rel_l2(db.cpu() + 0.25, dbr) < 3e-5
    # accumulate = False overwrites whatever the gradient buffers held
    ops.layernorm_bwd(dyg, xg, wg, mean, rstd, dx, dx_in=dx_in.to(dev()), dw=dw, db=db, accumulate=False)
    assert rel_l2(dw.cpu(), dwr) < 3e-5 and rel_l2(db.cpu(), dbr) < 3e-5


def test_wide_layernorm_without_affine_and_without_incoming_gradient():
    from afft_amd import ops
    rows, d = 9, 2560
    x, _, _, dy, yr, dxr, _, _ = problem(rows, d, "f32", affine=False)
    xg, y, mean, rstd = forward(x, None, None)
    assert rel_l2(y.cpu(), yr) < 2e-5
    dx = torch.empty(rows, d, device=dev())
    ops.layernorm_bwd(dy.to(dev()), xg, None, mean, rstd, dx)
    assert rel_l2(dx.cpu(), dxr) < 3e-5


def replayed_mask(rows, d, drop):
    """what the backward kernel that serves width d multiplies the copy by: the copy of dx = 0 + 1 (dy = 0, dx_in = 1)"""
    from afft_amd import ops
    one = torch.ones(rows, d, device=dev())
    mask = torch.empty(rows, d, dtype=torch.bfloat16, device=dev())
    ops.layernorm_bwd(torch.zeros(rows, d, device=dev()), one, None, torch.zeros(rows, device=dev()), torch.ones(rows, device=dev()),
                      torch.empty(rows, d, device=dev()), dx_in=one, dx_bf16=mask, copy_drop=drop)
    return mask.float()


@pytest.mark.parametrize("rows,d,group", [(66, 2560, 3), (40, 4096, 4)])
def test_wide_layernorm_handover_copy_replays_the_mask(rows, d, group):
    """dx_bf16 and dcol with a dropout + DropPath mask against the unmasked call times the mask on the host; the mask itself is the one
    the d <= 2048 kernel replays for the same element indices (an [rows, d] tensor seen as [2 rows, d / 2]: element index and DropPath
    group of every element are the same with twice the rows per group)"""
    from afft_amd import _lib as L, ops
    x, w, b, dy, _, dxr, _, _ = problem(rows, d, "bf16")
    xg, _, mean, rstd = forward(x, w, b)
    dx_in = rnd(rows, d, seed=5).to(dev())
    dyg, wg = dy.to(torch.bfloat16).to(dev()), w.to(dev())
    drop = L.Dropout(0.5, 0x1234567, 0.5, 0x89abcd, group)
    mask = replayed_mask(rows, d, drop)
    narrow = replayed_mask(2 * rows, d // 2, L.Dropout(0.5, 0x1234567, 0.5, 0x89abcd, 2 * group))
    assert torch.equal(mask.view(2 * rows, d // 2), narrow)
    vals = set(mask.unique().tolist())
    assert vals == {0.0, 4.0}, vals
    dead = (mask == 0).view(rows // group, group * d).all(1)          # DropPath: whole row groups
    assert dead.any() and not dead.all()
    assert (mask.view(rows // group, group * d)[~dead] == 0).any()    # element dropout inside the groups that stay
    dx = torch.empty(rows, d, device=dev())
    dxb = torch.empty(rows, d, dtype=torch.bfloat16, device=dev())
    dcol = torch.full((d,), 2.0, device=dev())
    dw, db = torch.zeros(d, device=dev()), torch.zeros(d, device=dev())
    ops.layernorm_bwd(dyg, xg, wg, mean, rstd, dx, dx_in=dx_in, dx_bf16=dxb, dw=dw, db=db, accumulate=False, copy_drop=drop,
                      dcol=dcol, dcol_accumulate=True)
    dx0 = torch.empty(rows, d, device=dev())
    dxb0 = torch.empty(rows, d, dtype=torch.bfloat16, device=dev())
    dcol0 = torch.empty(d, device=dev())
    ops.layernorm_bwd(dyg, xg, wg, mean, rstd, dx0, dx_in=dx_in, dx_bf16=dxb0, dw=dw, db=db, accumulate=False, copy_drop=None,
                      dcol=dcol0, dcol_accumulate=False)
    torch.cuda.synchronize()
    assert rel_l2(dx0.cpu(), dxr + dx_in.cpu()) < 3e-5
    assert torch.equal(dx, dx0)                                   # the mask touches the copy only
    assert torch.equal(dxb0, dx0.to(torch.bfloat16))
    assert torch.equal(dxb, (dx0 * mask).to(torch.bfloat16))
    assert rel_l2(dcol0.cpu(), dx0.double().sum(0).cpu()) < 3e-5
    assert rel_l2(dcol.cpu() - 2.0, (dx0.double() * mask.double()).sum(0).cpu()) < 3e-5


def test_wide_layernorm_bwd_take():
    """in_take = 5: the incoming gradient [12, d] lands on rows 0, 5, 10, .. only"""
    from afft_amd import ops
    rows, take, d = 60, 5, 3072
    x, w, b, dy, _, dxr, dwr, dbr = problem(rows, d, "bf16")
    xg, _, mean, rstd = forward(x, w, b)
    dx_in = rnd(rows // take, d, seed=6)
    want = dxr.clone()
    want[::take] += dx_in
    dx = torch.empty(rows, d, device=dev())
    dxb = torch.empty(rows, d, dtype=torch.bfloat16, device=dev())
    dw, db = torch.empty(d, device=dev()), torch.empty(d, device=dev())
    ops.layernorm_bwd_take(dy.to(torch.bfloat16).to(dev()), xg, w.to(dev()), mean, rstd, dx, dx_in.to(dev()), take, dx_bf16=dxb,
                           dw=dw, db=db, accumulate=False)
    torch.cuda.synchronize()
    assert rel_l2(dx.cpu(), want) < 3e-5
    assert rel_l2(dx.cpu()[1::take], dxr[1::take]) < 3e-5        # a row between two taken ones receives none
    assert rel_l2(dxb.float().cpu(), want) < 5e-3
    assert rel_l2(dw.cpu(), dwr) < 3e-5 and rel_l2(db.cpu(), dbr) < 3e-5


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_wide_layernorm_bwd_is_bitwise_reproducible(dt):
    from afft_amd import _lib as L, ops
    rows, d = 130, 4096
    ydt = torch.float32 if dt == "f32" else torch.bfloat16
    x, w, b, dy, _, _, _, _ = problem(rows, d, dt)
    xg, _, mean, rstd = forward(x, w, b)
    dx_in = rnd(rows, d, seed=5).to(dev())
    dyg, wg = dy.to(ydt).to(dev()), w.to(dev())
    drop = L.Dropout(0.25, 77, 0.1, 99, 2)
    runs = []
    for _ in range(2):
        dx = torch.empty(rows, d, device=dev())
        dxb = torch.empty(rows, d, dtype=torch.bfloat16, device=dev())
        dw, db, dcol = (torch.empty(d, device=dev()) for _ in range(3))
        ops.layernorm_bwd(dyg, xg, wg, mean, rstd, dx, dx_in=dx_in, dx_bf16=dxb, dw=dw, db=db, accumulate=False, copy_drop=drop,
                          dcol=dcol, dcol_accumulate=False)
        runs.append((dx, dxb, dw, db, dcol))
    torch.cuda.synchronize()
    for a, c, what in zip(runs[0], runs[1], ("dx", "dx_bf16", "dw", "db", "dcol")):
        assert torch.equal(a, c), what
