"""GPU: the stand-alone momentum-SGD kernels (afft_sgd_nesterov2: one flat slice; afft_sgd_nesterov_runs2: a table of runs of one set
of flat buffers; csrc/elementwise.hip) elementwise against the float64 restatement tests/sgd_double.py, which test_sgd_double_cpu.py
holds against torch.optim.SGD.  (The third user of the same device function, the fused GEMM epilogue, is a stage of the GEMM case
table: test_kernels_gpu.py::test_gemm_instantiation_exact.)

Two kinds of inputs.  Dyadic: power-of-two hyperparameters, p / buf / g on grids such that every intermediate of the update is an fp32
number (asserted on the reference), so p, buf and every image must equal the reference bit for bit; the new p carries 17 significant
bits, so all three image formats round, and |256 p| passes 448 in some elements, where the byte image saturates.  Normal: randn
inputs and the recipes' hyperparameters, p and buf within the five-rounding bound sgd_double.sgd_bound derives; the images are then the
independent roundings of the kernel's own p.  Every buffer sits between sentinel elements, the images are sentinel-filled: nothing
outside [0, n) (outside the runs) is written, an image that was not asked for does not exist, and ok = 0 leaves every bit."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

import sgd_double as sd  # noqa: E402

PAD = 64      # sentinel elements either side of every buffer (offset 0 stays 16-byte aligned in every dtype)
_INT = {torch.float32: (torch.int32, 0x7FC0DEAD), torch.bfloat16: (torch.int16, 0x7DAD), torch.float16: (torch.int16, 0x7DAD),
        torch.uint8: (torch.uint8, 0xA5)}
_IMG = {"bf16": (torch.bfloat16, sd.bf16_image), "f16": (torch.float16, sd.f16_image), "f8": (torch.uint8, sd.e4m3_image)}
SUBSETS = [s for r in range(4) for s in itertools.combinations(("bf16", "f16", "f8"), r)]
NS = [1, 3, 4, 5, 1023, 1025, 256 * 1024 + 5]      # the last: 256 blocks x 1024 elements is a whole grid stride: second trip + tail


def dev():
    return torch.device("cuda:0")


def _fenced(n, dtype, content=None):
    """(whole buffer, its [PAD, PAD + n) view): sentinel bit pattern everywhere, `content` in the view if given"""
    idt, s = _INT[dtype]
    big = torch.empty(PAD + n + PAD, dtype=dtype, device=dev())
    big.view(idt).fill_(s)
    view = big[PAD:PAD + n]
    if content is not None:
        view.copy_(content)
    return big, view


def _bits(t):
    return t.view(_INT[t.dtype][0])


def _inputs(n, kind, gdtype, flags, seed):
    """p, buf, g (float64, exact in fp32 / in gdtype), hyperparameters (lr, mom, wd, gscale), the value of *gscale_dev"""
    gen = torch.Generator(device=dev()).manual_seed(seed)
    if kind == "dyadic":
        ints = lambda amp, sh: torch.randint(-amp, amp + 1, (n,), generator=gen, device=dev()).double() * 2.0 ** -sh      # noqa: E731
        return ints(30, 4), ints(4096, 9), ints(128, 4), (2.0 ** -4, 0.5, 2.0 ** -6, 0.5), 0.5      # |p| <= 1.875: e4m3(256 p) saturates from 1.75
    p, buf, g = (torch.randn(n, generator=gen, device=dev(), dtype=torch.float64) for _ in range(3))
    return p.float().double(), buf.float().double(), g.to(gdtype).double(), tuple(sd.f32(x) for x in (0.05, 0.9, 1e-3, 0.5)), sd.f32(0.8)


def _reference(p, buf, g, hyper, gsd, flags, kind):
    """(want p, want buf, bound on p, bound on buf) with the gradient scale the kernel forms: fl(gscale * *gscale_dev)"""
    lr, mom, wd, gs = hyper
    gs = gs if gsd is None else sd.f32(gs * gsd)
    st = sd.sgd_stages(p, buf, g, lr, mom, wd, gs, flags)
    if kind == "dyadic":
        for k, v in st.items():
            assert torch.equal(v, v.float().double()), f"{k} is not exact in fp32: the inputs do not make the update exact"
        zero = torch.zeros_like(p)
        return st["p"], st["buf"], zero, zero
    return (st["p"], st["buf"]) + sd.sgd_bound(p, buf, g, lr, mom, wd, gs, flags)


def _check(p, buf, imgs, want_p, want_buf, ep, eb, where, what):
    """p / buf [where] against the reference within the bounds (zero: bitwise), the images [where] = roundings of the kernel's p"""
    for got, want, bound, name in ((p, want_p, ep, "p"), (buf, want_buf, eb, "buf")):
        bad = ~((got[where].double() - want[where]).abs() <= bound[where])
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            raise AssertionError(f"{what}: {int(bad.sum())} elements of {name} off, first [{i}] of the checked ones: "
                                 f"{float(got[where][i])} vs {float(want[where][i])} (bound {float(bound[where][i]):.3g})")
    for k, img in imgs.items():
        want = _IMG[k][1](p)
        assert torch.equal(_bits(img)[where], _bits(want)[where]), f"{what}: the {k} image is not the rounding of p"


@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16], ids=["g_f32", "g_bf16"])
@pytest.mark.parametrize("n", NS)
def test_flat_kernel_matches_float64(n, gdtype):
    """afft_sgd_nesterov2: four flag words x {dyadic, normal} inputs x gscale_dev given or not x ok NULL / 1 / 0 x every subset of images"""
    from afft_amd import ops
    everything = slice(None)
    for flags, kind in itertools.product(sd.FLAG_WORDS, ("dyadic", "normal")):
        p0, b0, g0, hyper, gsd_value = _inputs(n, kind, gdtype, flags, seed=97 * n + flags)
        first = bool(flags & sd.FIRST_STEP)
        g = g0.to(gdtype)
        assert torch.equal(g.double(), g0)
        for use_gsd in (False, True):
            want = _reference(p0, b0, g0, hyper, gsd_value if use_gsd else None, flags, kind)
            gsd = torch.tensor([gsd_value], device=dev()) if use_gsd else None
            if kind == "dyadic" and n > 1000:      # the inputs exercise the byte image's saturation as well as its rounding
                assert 0 < int((want[0].abs() * 256.0 > 448.0).sum()) < n // 2
            for subset, ok in itertools.product(SUBSETS, (None, 1.0, 0.0)):
                what = f"n={n} flags={flags} {kind} gscale_dev={use_gsd} ok={ok} images={subset}"
                pb, p = _fenced(n, torch.float32, p0)
                bb, buf = _fenced(n, torch.float32, torch.full_like(b0, float("nan")) if first else b0)      # a first step must not read it
                imgs = {k: _fenced(n, _IMG[k][0]) for k in subset}
                bufs = [pb, bb] + [big for big, _ in imgs.values()]
                before = [t.clone() for t in bufs]
                ops.sgd_nesterov(p, g, buf, *hyper, flags, gscale_dev=gsd, ok=None if ok is None else torch.tensor([ok], device=dev()),
                                 **{"p_" + k: v for k, (_, v) in imgs.items()})
                torch.cuda.synchronize()
                if ok == 0.0:
                    assert all(torch.equal(_bits(t), _bits(t0)) for t, t0 in zip(bufs, before)), f"{what}: something was written"
                    continue
                for t, t0 in zip(bufs, before):      # nothing outside [0, n)
                    assert torch.equal(_bits(t)[:PAD], _bits(t0)[:PAD]) and torch.equal(_bits(t)[PAD + n:], _bits(t0)[PAD + n:]), what
                assert not torch.isnan(p).any() and not torch.isnan(buf).any(), what
                _check(p, buf, {k: v for k, (_, v) in imgs.items()}, *want, everything, what)


RUN_LENGTHS = [0, 1, 255, 256, 257, 16384]      # one 256-thread block per run: nothing, one lane, one trip less one, exactly one, one more, 64 trips


def _runs():
    """(runs {start, length}, size of the buffers): 7 or 8 untouched elements between the runs and 9 behind the last, no start a
    multiple of 4 (test_sgd_runs_equals_sgd_over_the_same_ranges has those)"""
    runs, pos = [], 3
    for n in RUN_LENGTHS:
        pos += pos % 4 == 0
        runs.append((pos, n))
        pos += n + 7
    assert all(s % 4 for s, _ in runs)
    return runs, pos + 2


@pytest.mark.parametrize("kind", ["dyadic", "normal"])
@pytest.mark.parametrize("flags", sd.FLAG_WORDS)
def test_runs_kernel_matches_float64_and_leaves_the_rest(flags, kind):
    """afft_sgd_nesterov_runs2: the elements of the runs are updated as the reference says, everything between and behind them keeps
    its bits in p, buf and every image; ok = 0 writes nothing"""
    from afft_amd import ops
    runs, n = _runs()
    inside = torch.zeros(n, dtype=torch.bool, device=dev())
    for s, ln in runs:
        inside[s:s + ln] = True
    table = torch.tensor(runs, dtype=torch.int64, device=dev())
    p0, b0, g0, hyper, _ = _inputs(n, kind, torch.float32, flags, seed=500 + flags)
    first = bool(flags & sd.FIRST_STEP)
    want = _reference(p0, b0, g0, hyper, None, flags, kind)
    for subset, ok in itertools.product((("bf16", "f16", "f8"), (), ("f8",)), (None, 1.0, 0.0)):
        what = f"flags={flags} {kind} ok={ok} images={subset}"
        pb, p = _fenced(n, torch.float32, p0)
        bb, buf = _fenced(n, torch.float32, torch.full_like(b0, float("nan")) if first else b0)
        imgs = {k: _fenced(n, _IMG[k][0]) for k in subset}
        bufs = [pb, bb] + [big for big, _ in imgs.values()]
        before = [t.clone() for t in bufs]
        ops.sgd_nesterov_runs(p, g0.float(), buf, table, *hyper, flags, ok=None if ok is None else torch.tensor([ok], device=dev()),
                              **{"p_" + k: v for k, (_, v) in imgs.items()})
        torch.cuda.synchronize()
        if ok == 0.0:
            assert all(torch.equal(_bits(t), _bits(t0)) for t, t0 in zip(bufs, before)), f"{what}: something was written"
            continue
        outside = torch.ones(n + 2 * PAD, dtype=torch.bool, device=dev())
        outside[PAD:PAD + n] = ~inside
        for t, t0 in zip(bufs, before):
            assert torch.equal(_bits(t)[outside], _bits(t0)[outside]), f"{what}: a write outside the runs"
        assert not torch.isnan(p[inside]).any() and not torch.isnan(buf[inside]).any(), what
        _check(p, buf, {k: v for k, (_, v) in imgs.items()}, *want, inside, what)
