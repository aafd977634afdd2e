"""GPU: the weight-averaging kernels (afft_ema, afft_swap_f32; csrc/optim.hip) elementwise against float64 and bit for bit between
their 16-byte and element paths, and afft_amd.optim.WeightEMA on the smallest model that has every kind of parameter: an SA-Fuser with
two modalities (the 24-wide one behind a [64, 24] mapping that keeps a padded cast image), T = 4, d = 64, one block whose 64-multiple
weights own flat images, the predictor (its position table is read as fp32) and the 11-class classifier (padded cast image), 2 clips.

The bar of the kernel is derived (tests/ema_double.py): |got - ref| <= 2 * 2^-24 * (|p| + |ema|), one rounding of the difference and
one of the fused multiply-add.  Over steps it accumulates as err_t <= (1 - w_t) err_(t-1) + 2 * 2^-24 * (|p_t| + |ema_(t-1)|)."""
import ctypes
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from ema_double import U, ema_ref  # noqa: E402
from test_model_gpu import _reference_loop, build  # noqa: E402

NS = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024 * 256 + 3]
WS = [0.0, 2.0 ** -12, 0.1, 1.0]
PAD = 64                      # sentinel elements before and after every buffer (a multiple of 4: offset 0 is 16-byte aligned)
SENTINEL = -12345.678


@functools.lru_cache(maxsize=None)
def _operands(n):
    """(ema, p) on the host: magnitudes 1e-8 .. 1e3 log-uniform, both signs, every fourth element p == ema exactly, and a few pairs
    that differ in the last bit or in sign only"""
    g = torch.Generator().manual_seed(1000 + n)
    mag = lambda: (10.0 ** (torch.rand(n, generator=g) * 11.0 - 8.0)) * (torch.randint(0, 2, (n,), generator=g) * 2.0 - 1.0)      # noqa: E731
    e, p = mag().float(), mag().float()
    i = torch.arange(n)
    p = torch.where(i % 4 == 1, e, p)
    p = torch.where(i % 16 == 2, torch.nextafter(e, torch.zeros_like(e)), p)
    p = torch.where(i % 16 == 6, -e, p)
    return e, p


def _padded(t, off, dev):
    """t on the device at element offset `off` of a sentinel-filled buffer: (whole buffer, view)"""
    big = torch.full((PAD + off + t.numel() + PAD,), SENTINEL, device=dev)
    assert big.data_ptr() % 16 == 0
    view = big[PAD + off:PAD + off + t.numel()]
    view.copy_(t)
    assert t.numel() == 0 or view.data_ptr() % 16 == 4 * off
    return big, view


def _padding_intact(big, off, n):
    return bool((big[:PAD + off] == SENTINEL).all()) and bool((big[PAD + off + n:] == SENTINEL).all())


def _bits(t):
    """the tensor's bytes: comparisons below are of bit patterns (signed zeros and NaN payloads count), whatever the dtype"""
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("n", NS)
def test_ema_kernel_matches_float64_on_both_paths(n, w):
    from afft_amd import ops
    dev = torch.device("cuda:0")
    e, p = _operands(n)
    ref, bar = ema_ref(e, p, w)
    got = {}
    for off in (0, 1):      # 16-byte aligned: the vector body and its tail; one element off: element accesses
        for ok in (None, 1.0, 0.0):
            eb, ev = _padded(e, off, dev)
            pb, pv = _padded(p, off, dev)
            okt = None if ok is None else torch.full((), ok, device=dev)
            ops.ema(ev, pv, w, ok=okt)
            torch.cuda.synchronize()
            assert _padding_intact(eb, off, n) and _padding_intact(pb, off, n), (off, ok)
            assert torch.equal(_bits(pv.cpu()), _bits(p)), (off, ok)
            got[off, ok] = ev.cpu()
    for off in (0, 1):
        out = got[off, None]
        err = (out.double() - ref).abs()
        assert bool((err <= bar).all()), (off, float((err / bar.clamp_min(1e-300)).max()))
        assert torch.equal(_bits(got[off, 1.0]), _bits(out)), off           # ok = 1 is ok = None
        assert torch.equal(_bits(got[off, 0.0]), _bits(e)), off             # ok = 0 writes nothing
        same = p == e
        assert torch.equal(_bits(out[same]), _bits(e[same])), off            # an element equal to its parameter keeps its bits
        if w == 0.0:
            assert torch.equal(_bits(out), _bits(e)), off
        if w == 1.0 and n:
            assert bool(((out.double() - p.double()).abs() <= bar).all())
    assert torch.equal(_bits(got[0, None]), _bits(got[1, None]))             # the two paths give the same bits
    if n > 16 and 0.0 < w:
        assert not torch.equal(got[0, None], e)


def test_ema_kernel_same_inputs_same_bits_and_signed_zeros_and_nan():
    from afft_amd import ops
    dev = torch.device("cuda:0")
    n = NS[-1]
    e, p = _operands(n)
    e, p = e.clone(), p.clone()
    e[:4] = torch.tensor([-0.0, 0.0, -0.0, 1.0])
    p[:4] = torch.tensor([-0.0, -0.0, 0.0, float("nan")])
    outs = []
    for _ in range(2):
        ev, pv = e.to(dev), p.to(dev)
        ops.ema(ev, pv, 0.1)
        outs.append(ev.cpu())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    assert torch.equal(_bits(outs[0][:3]), _bits(e[:3])) and math.isnan(float(outs[0][3]))


@pytest.mark.parametrize("n", NS)
def test_swap_kernel_is_an_exact_exchange_on_both_paths(n):
    from afft_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2000 + n)
    a = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)      # every bit pattern: NaN payloads too
    b = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    special = torch.tensor([0x7fc00001, -0x003ffffe, -2 ** 31, 0, 0x7f800001, 0x7f800000], dtype=torch.int64).to(torch.int32)
    k = min(n, special.numel())
    a[:k] = special[:k]                 # quiet / signalling NaNs with payloads, -0, +0, inf
    b[:k] = special.flip(0)[:k]
    for off in (0, 1):
        ab, av = _padded(torch.zeros(n), off, dev)
        bb, bv = _padded(torch.zeros(n), off, dev)
        av.view(torch.int32).copy_(a)
        bv.view(torch.int32).copy_(b)
        ops.swap_f32(av, bv)
        torch.cuda.synchronize()
        assert torch.equal(av.view(torch.int32).cpu(), b) and torch.equal(bv.view(torch.int32).cpu(), a), off
        assert _padding_intact(ab, off, n) and _padding_intact(bb, off, n), off
        ops.swap_f32(av, bv)
        assert torch.equal(av.view(torch.int32).cpu(), a) and torch.equal(bv.view(torch.int32).cpu(), b), off
    # mixed alignment takes the element path as well
    ab, av = _padded(torch.zeros(n), 0, dev)
    bb, bv = _padded(torch.zeros(n), 1, dev)
    av.view(torch.int32).copy_(a)
    bv.view(torch.int32).copy_(b)
    ops.swap_f32(av, bv)
    assert torch.equal(av.view(torch.int32).cpu(), b) and torch.equal(bv.view(torch.int32).cpu(), a)
    assert _padding_intact(ab, 0, n) and _padding_intact(bb, 1, n)


def test_overlap_and_bad_w_are_refused_through_ops():
    from afft_amd import ops
    dev = torch.device("cuda:0")
    x = torch.zeros(64, device=dev)
    with pytest.raises(RuntimeError, match="overlap"):
        ops.swap_f32(x[:40], x[24:])
    with pytest.raises(RuntimeError, match=r"w must lie in \[0, 1\]"):
        ops.ema(x[:32], x[32:], 1.5)
    assert not x.any()


# ----------------------------------------------------------------------------- WeightEMA on the small model
CASE = dict(fuser="sa", modal_dims={"rgb": 64, "objects": 24}, d=64, D=128, depth=1, num_heads=4, fp_layers=1, fp_heads=2, T=4,
            num_classes=11)
CLIPS = 2


def _inputs(dev):
    g = torch.Generator().manual_seed(11)
    feats = {m: torch.randn(CLIPS, CASE["T"], C, 1, 1, 1, generator=g).to(dev) for m, C in CASE["modal_dims"].items()}
    tgt = torch.randint(0, CASE["num_classes"], (CLIPS,), generator=g).to(dev)
    sub = torch.randint(0, CASE["num_classes"], (CLIPS, CASE["T"], 1), generator=g).to(dev)
    return feats, tgt, sub


def _model(precision, dev, seed=0):
    torch.manual_seed(seed)
    return build(CASE, precision).to(dev).eval()


def _optimizer(kind, model, **kw):
    from afft_amd.common.scheduler import prepare_params
    from afft_amd.optim import SGD, AdamW
    groups = prepare_params(model, None, 1e-2, 1e-4)
    if kind == "SGD":
        return SGD(groups, lr=1e-2, momentum=0.9, nesterov=True, bucket_elems=1 << 14, **kw)
    return AdamW(groups, lr=1e-3, bucket_elems=1 << 14, **kw)


def _forward(model, feats, tgt, sub):
    """every tensor the model returns, flattened: [(key, fp32 clone)]"""
    with torch.no_grad():
        outs, _ = model(feats, mixup_fn=None, target={"action": tgt}, target_subclips={"action": sub}, target_subclips_ignore_index=None)
    flat = []

    def walk(key, v):
        if isinstance(v, dict):
            for k in sorted(v):
                walk(f"{key}/{k}", v[k])
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk(f"{key}/{i}", x)
        elif isinstance(v, torch.Tensor):
            flat.append((key, v.detach().float().clone()))
    walk("", outs)
    assert flat
    return flat


def _same(a, b):
    return len(a) == len(b) and all(ka == kb and torch.equal(_bits(x), _bits(y)) for (ka, x), (kb, y) in zip(a, b))


def _images(flat):
    return {k: getattr(flat, k).clone() for k in ("flat_p", "flat_p16", "flat_h16", "flat_p8", "flat_pk16") if getattr(flat, k) is not None}


@pytest.mark.parametrize("kind,kw", [("SGD", dict(ema_decay=0.9, ema_warmup=False)), ("AdamW", dict(ema_decay=0.9))])
def test_average_equals_the_float64_recurrence_over_the_steps(kind, kw):
    import afft_amd
    dev = torch.device("cuda:0")
    feats, tgt, sub = _inputs(dev)
    try:
        model = _model("bf16", dev)
        has_images = {n: tuple(p.shape) for n, p in model.named_parameters() if p.dim() == 2}
        assert any(s[0] % 64 or s[1] % 64 for s in has_images.values()) and any(not (s[0] % 64 or s[1] % 64) for s in has_images.values())
        opt = _optimizer(kind, model, **kw)
        assert opt.ema.ok is opt.opt.ok and opt.ema.ema.shape == opt.flat.flat_p.shape
        ref = opt.flat.flat_p.double().cpu()
        assert torch.equal(opt.ema.ema.cpu().double(), ref)
        err = torch.zeros_like(ref)
        for t in range(3):
            _reference_loop(model, opt, None, feats, tgt, sub, 1)
            p = opt.flat.flat_p.cpu()
            decay = 0.9 if not kw.get("ema_warmup", True) else min(0.9, (1 + t) / (10 + t))
            w = ctypes.c_float(1.0 - decay).value
            err = (1.0 - w) * err + 2.0 * U * (p.double().abs() + ref.abs() + err)
            ref = ref + w * (p.double() - ref)
        got = opt.ema.ema.cpu().double()
        assert opt.ema.num_updates == 3
        assert bool(((got - ref).abs() <= err).all()), float(((got - ref).abs() / err.clamp_min(1e-300)).max())
        assert not torch.equal(opt.ema.ema, opt.flat.flat_p)
    finally:
        afft_amd.set_precision("bf16")


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16x2"])
def test_applied_computes_with_the_average_and_restores_every_bit(precision):
    import afft_amd
    dev = torch.device("cuda:0")
    feats, tgt, sub = _inputs(dev)
    try:
        model = _model(precision, dev)
        opt = _optimizer("SGD", model, ema_decay=0.9, ema_warmup=False)
        _reference_loop(model, opt, None, feats, tgt, sub, 3)
        flat, avg = opt.flat, opt.ema
        if precision == "fp16x2":
            assert flat.flat_h16 is not None
        before_imgs, before_ema = _images(flat), avg.ema.clone()
        before_out = _forward(model, feats, tgt, sub)
        fresh = _model(precision, dev, seed=1)
        fresh.load_state_dict(avg.averaged_state_dict(model), strict=True)
        fresh_out = _forward(fresh, feats, tgt, sub)
        assert not _same(before_out, fresh_out)
        with avg.applied():
            inside_out = _forward(model, feats, tgt, sub)
            assert torch.equal(_bits(flat.flat_p), _bits(before_ema)) and torch.equal(_bits(avg.ema), _bits(before_imgs["flat_p"]))
            assert torch.equal(flat.flat_p16, flat.flat_p.bfloat16())
            with pytest.raises(RuntimeError, match="applied"):
                avg.update()
            with pytest.raises(RuntimeError, match="applied"):
                opt.zero_grad()
        if precision in ("fp32", "bf16"):
            assert _same(inside_out, fresh_out), [k for (k, x), (_, y) in zip(inside_out, fresh_out) if not torch.equal(x, y)]
        else:
            assert not _same(inside_out, before_out)
        after_imgs = _images(flat)
        assert before_imgs.keys() == after_imgs.keys()
        for k in before_imgs:
            assert torch.equal(_bits(before_imgs[k]), _bits(after_imgs[k])), k
        assert torch.equal(_bits(avg.ema), _bits(before_ema))
        assert _same(_forward(model, feats, tgt, sub), before_out)
    finally:
        afft_amd.set_precision("bf16")


def test_a_twin_that_never_entered_applied_trains_on_to_the_same_bits():
    import afft_amd
    dev = torch.device("cuda:0")
    feats, tgt, sub = _inputs(dev)
    try:
        ends = []
        for enters in (True, False):
            model = _model("bf16", dev)
            opt = _optimizer("SGD", model, ema_decay=0.9, ema_warmup=False)
            _reference_loop(model, opt, None, feats, tgt, sub, 3)
            if enters:
                with opt.ema.applied():
                    _forward(model, feats, tgt, sub)
            _reference_loop(model, opt, None, feats, tgt, sub, 1)
            ends.append((opt.flat.flat_p.clone(), opt.opt.buf.clone(), opt.ema.ema.clone(), opt.flat.flat_p16.clone()))
        for a, b in zip(*ends):
            assert torch.equal(_bits(a), _bits(b))
    finally:
        afft_amd.set_precision("bf16")


def _traced(fn, cap=8192):
    from afft_amd import _lib
    _lib.check(_lib.lib().afft_kernel_trace_begin(cap), "kernel_trace_begin")
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        buf = (_lib.KernelTraceRec * cap)()
        n = _lib.lib().afft_kernel_trace_end(buf, cap)
    assert 0 <= n < cap
    return [(buf[i].kind, buf[i].rows, buf[i].bytes) for i in range(n)]


def test_off_by_default_same_bits_no_buffer_no_launch():
    """ema_decay=None (or not given): parameters and momentum after three steps are those of a run with the average on -- which only
    reads them -- and of one that does not name the argument; no buffer exists and the kernel trace holds no afft_ema record, where
    the run with the average on holds one per step with its 12 B per element"""
    import afft_amd
    from afft_amd import _lib
    dev = torch.device("cuda:0")
    feats, tgt, sub = _inputs(dev)
    try:
        ends, traces = [], []
        for kw in (dict(), dict(ema_decay=None), dict(ema_decay=0.9)):
            model = _model("bf16", dev)
            opt = _optimizer("SGD", model, **kw)
            assert (opt.ema is None) == (kw.get("ema_decay") is None)
            traces.append(_traced(lambda: _reference_loop(model, opt, None, feats, tgt, sub, 3)))
            ends.append((opt.flat.flat_p.clone(), opt.opt.buf.clone()))
        for other in ends[1:]:
            for a, b in zip(ends[0], other):
                assert torch.equal(_bits(a), _bits(b))
        kinds = [[r for r in tr if r[0] in (_lib.K_EMA, _lib.K_SWAP_F32)] for tr in traces]
        assert all(len(tr) > 0 for tr in traces)      # the trace was live: attention / LayerNorm records
        assert kinds[0] == [] and kinds[1] == []
        total = opt.flat.total
        assert kinds[2] == [(_lib.K_EMA, total, 12 * total)] * 3

        def in_and_out():
            with opt.ema.applied():
                pass
        swaps = _traced(in_and_out)
        assert [r for r in swaps if r[0] in (_lib.K_EMA, _lib.K_SWAP_F32)] == [(_lib.K_SWAP_F32, total, 16 * total)] * 2
    finally:
        afft_amd.set_precision("bf16")
