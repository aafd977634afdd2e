"""GPU: every derived weight image afft_amd.runtime hands out is bit-identical to its fill kernel run directly on the fp32 master
into a fresh zeroed buffer of the same shape -- after construction, after an in-place update and after copies of new values --
for parameters adopted into hand-made flat views and for one that keeps padded images of its own.  The same kernel on the same
input: the comparison is exact."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _direct(p, like, kind):
    from afft_amd import ops
    want = torch.zeros_like(like)
    with torch.no_grad():
        if kind == "packed":
            ops.pack_weight(p.detach(), want)
        elif kind == "e4m3":
            ops.quant_e4m3(p.detach(), 256.0, want)
        else:
            ops.cast(p.detach(), want[:p.shape[0], :p.shape[1]])
    return want


def _adopt(rt, p):
    n = p.numel()
    dev = p.device
    views = dict(bf16=torch.zeros(n, dtype=torch.bfloat16, device=dev).view(p.shape), f16=torch.zeros(n, dtype=torch.float16, device=dev).view(p.shape),
                 e4m3=torch.zeros(n, dtype=torch.uint8, device=dev).view(p.shape), packed=torch.zeros(n, dtype=torch.bfloat16, device=dev))
    for kind in ("bf16", "f16", "e4m3"):       # adopted views are handed over fresh, as parallel.FlatParams derives its flat buffers first
        views[kind].copy_(_direct(p, views[kind], kind))
    rt.adopt_weight_image(p, views["bf16"], packed=views["packed"])
    rt.adopt_weight_f16(p, views["f16"])
    rt.adopt_weight_f8(p, views["e4m3"])
    return views


def test_every_image_equals_its_fill_kernel_on_the_master():
    from afft_amd import _lib, runtime as rt
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(7)
    new = lambda r, c: torch.nn.Parameter(torch.randn(r, c, generator=g).to(dev))      # noqa: E731
    small, big, odd = new(64, 128), new(256, 64), new(70, 100)
    wanted = _lib.lib().afft_gemm_packed_wanted
    # no row count makes the dispatcher want a packed [64, 128] weight (it needs >= 256 output columns); [256, 64] is the smallest
    # weight it accepts, for a row count that fills the B-direct kernel's grid exactly once
    rows = next((r for r in range(160, 160 * 2048, 160) if wanted(r, 256, 64)), None)
    assert rows is not None, "afft_gemm_packed_wanted accepts no row count for a [256, 64] weight"
    views = {id(p): _adopt(rt, p) for p in (small, big)}

    def check(what):
        for p in (small, big, odd):
            got = dict(bf16=rt.weight_images(p), f16=rt.weight_f16(p), e4m3=rt.weight_f8(p))
            pk = rt.weight_packed(p, rows)
            assert (pk is not None) == (p is big) == rt.packed_live(p), (what, tuple(p.shape))
            if pk is not None:
                got["packed"] = pk
            for kind, t in got.items():
                if id(p) in views:
                    assert t is views[id(p)][kind], (what, tuple(p.shape), kind)
                else:
                    assert tuple(t.shape) == (128, 128), (what, kind)
                    assert not t[70:].any() and not t[:, 100:].any(), (what, kind, "padding")
                assert torch.equal(t, _direct(p, t, kind)), (what, tuple(p.shape), kind)

    check("constructed")
    with torch.no_grad():
        for p in (small, big, odd):
            p.mul_(0.5)
    check("p.mul_(0.5)")
    with torch.no_grad():
        for p in (small, big, odd):
            p.copy_(torch.randn(p.shape, generator=g).to(dev))
    check("p.copy_")
    # a write through .data goes behind the version counter: whoever does it says so with invalidate_weight_images(True), and then
    # every image, the adopted and the packed ones included, follows
    for p in (small, big, odd):
        p.data.copy_(torch.randn(p.shape, generator=g).to(dev))
    rt.invalidate_weight_images(True)
    check("p.data.copy_")
