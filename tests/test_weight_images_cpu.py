"""The refresh rule of a parameter's derived weight images (afft_amd.runtime: bf16 / fp16 / e4m3 row-major images and the
fragment-packed bf16 one), pinned as the exact sequence of fill launches each scenario causes.

tests/cpu_ops.py stands in for the kernels; `cast`, `quant_e4m3` and `pack_weight` are wrapped so that every call appends
(name, destination data_ptr, destination shape) to a log, and the afft_gemm_packed_wanted query is answered by the test.  A
log is compared after its pointers have been replaced by the names of the tensors the accessors returned.

The expected logs below are literals.  They were recorded by running these same scenario functions against the runtime as it
was BEFORE the images got one record and one rule (the parent commit of that change), not against the code under test: they
pin which fills are launched, in which order and into which tensors."""
import gc
import types

import pytest
import torch

import cpu_ops


class _Trace:
    def __init__(self):
        self.calls, self.wanted, self.queries = [], True, []

    def wrap(self, name, fn):
        def logged(src, *rest, **kw):
            dst = rest[1] if name == "quant_e4m3" else rest[0]       # cast(src, dst), quant_e4m3(src, scale, dst), pack_weight(w, dst)
            self.calls.append((name, dst.data_ptr(), tuple(dst.shape)))
            return fn(src, *rest, **kw)
        return logged

    def take(self, **named):
        """the calls since the last take(), destination pointers replaced by the keyword whose tensor starts there"""
        names = {t.data_ptr(): k for k, t in named.items()}
        out = [(n, names.get(ptr, hex(ptr)), shape) for n, ptr, shape in self.calls]
        self.calls.clear()
        return out


@pytest.fixture
def traced(monkeypatch):
    from afft_amd import _lib, ops, runtime as rt
    tr = _Trace()

    def wanted(rows, out, in_):
        tr.queries.append((rows, out, in_))
        return 1 if tr.wanted else 0

    with cpu_ops.installed():
        for n in ("cast", "quant_e4m3", "pack_weight"):
            monkeypatch.setattr(ops, n, tr.wrap(n, getattr(ops, n)))
        monkeypatch.setattr(_lib, "lib", lambda: types.SimpleNamespace(afft_gemm_packed_wanted=wanted))
        gc.collect()
        rt.invalidate_weight_images()       # drops the entries of parameters earlier tests left behind
        yield rt, tr
        monkeypatch.undo()                  # before cpu_ops puts the real wrappers back


def _param(rows, cols, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.Parameter(torch.randn(rows, cols, generator=g))


def _adopted(rt, lo8=True):
    """a [64, 128] parameter whose images are views of hand-made flat buffers, as parallel.FlatParams hands them over"""
    p = _param(64, 128, seed=1)
    n = p.numel()
    v = types.SimpleNamespace(p=p, bf16=torch.zeros(n, dtype=torch.bfloat16).view(64, 128), pk=torch.zeros(n, dtype=torch.bfloat16),
                              f16=torch.zeros(n, dtype=torch.float16).view(64, 128), e4m3=torch.zeros(n, dtype=torch.uint8).view(64, 128))
    rt.adopt_weight_image(p, v.bf16, packed=v.pk)
    rt.adopt_weight_f16(p, v.f16)
    if lo8:
        rt.adopt_weight_f8(p, v.e4m3)
    return v


def _views(v):
    return dict(bf16=v.bf16, f16=v.f16, e4m3=v.e4m3, pk=v.pk)


def test_non_adopted_warm_record_refreshes_each_image_once(traced):
    rt, tr = traced
    p = _param(70, 100)
    w = rt.weight_images(p)
    assert rt.weight_images(p) is w and tuple(w.shape) == (128, 128) and w.dtype == torch.bfloat16
    assert tr.take(bf16=w) == [("cast", "bf16", (70, 100))]
    with torch.no_grad():
        p.add_(1.0)
    assert rt.weight_images(p) is w
    assert tr.take(bf16=w) == [("cast", "bf16", (70, 100))]
    h = rt.weight_f16(p)
    e = rt.weight_f8(p)
    assert h.dtype == torch.float16 and e.dtype == torch.uint8 and tuple(h.shape) == tuple(e.shape) == (128, 128)
    assert tr.take(bf16=w, f16=h, e4m3=e) == [("cast", "f16", (70, 100)), ("quant_e4m3", "e4m3", (128, 128))]
    assert rt.weight_f16(p) is h and rt.weight_f8(p) is e and rt.weight_images(p) is w
    assert tr.take() == []
    assert torch.equal(w[:70, :100], p.detach().bfloat16()) and torch.equal(h[:70, :100], p.detach().half())
    for t in (w, h, e):
        assert not t[70:].any() and not t[:, 100:].any()
    assert rt.weight_packed(p, 4096) is None and not rt.packed_live(p) and tr.queries == []


def test_non_adopted_cold_fp16_and_e4m3_refresh_the_bf16_image_first(traced):
    rt, tr = traced
    p = _param(70, 100)
    h = rt.weight_f16(p)
    w = rt.weight_images(p)
    assert tr.take(bf16=w, f16=h) == [("cast", "bf16", (70, 100)), ("cast", "f16", (70, 100))]
    q = _param(70, 100, seed=2)
    e = rt.weight_f8(q)
    w = rt.weight_images(q)
    assert tr.take(bf16=w, e4m3=e) == [("cast", "bf16", (70, 100)), ("quant_e4m3", "e4m3", (128, 128))]
    with torch.no_grad():
        q.mul_(0.5)
    assert rt.weight_f8(q) is e            # stale: bf16 again first, then its own
    assert tr.take(bf16=w, e4m3=e) == [("cast", "bf16", (70, 100)), ("quant_e4m3", "e4m3", (128, 128))]


def test_re_homed_parameter_gets_a_new_record(traced):
    rt, tr = traced
    p = _param(70, 100)
    old = (rt.weight_images(p), rt.weight_f16(p), rt.weight_f8(p))
    tr.take()
    listed = len(rt._wlist)
    p.data = torch.full((70, 100), 3.0)
    w = rt.weight_images(p)
    assert w is not old[0]
    assert tr.take(bf16=w) == [("cast", "bf16", (70, 100))]
    h, e = rt.weight_f16(p), rt.weight_f8(p)
    assert h is not old[1] and e is not old[2]
    assert tr.take(bf16=w, f16=h, e4m3=e) == [("cast", "f16", (70, 100)), ("quant_e4m3", "e4m3", (128, 128))]
    assert torch.equal(h[:70, :100], torch.full((70, 100), 3.0).half())
    assert len(rt._wlist) == listed


def test_adopted_images_are_silent_until_written_from_outside(traced):
    rt, tr = traced
    v = _adopted(rt)
    p = v.p
    assert rt.weight_images(p) is v.bf16 and rt.weight_f16(p) is v.f16 and rt.weight_f8(p) is v.e4m3
    assert tr.take() == []
    with torch.no_grad():
        p.copy_(torch.ones(64, 128))
    assert rt.weight_images(p) is v.bf16
    assert tr.take(**_views(v)) == [("cast", "bf16", (64, 128))]
    assert rt.weight_f16(p) is v.f16
    assert tr.take(**_views(v)) == [("cast", "f16", (64, 128))]
    assert rt.weight_f8(p) is v.e4m3
    assert tr.take(**_views(v)) == [("quant_e4m3", "e4m3", (64, 128))]
    assert torch.equal(v.bf16, torch.ones(64, 128).bfloat16()) and torch.equal(v.f16, torch.ones(64, 128).half())
    with torch.no_grad():
        p.copy_(torch.zeros(64, 128))
    assert rt.weight_f8(p) is v.e4m3       # one call: the bf16 view first, then the byte view; the fp16 view on its own next use
    assert tr.take(**_views(v)) == [("cast", "bf16", (64, 128)), ("quant_e4m3", "e4m3", (64, 128))]
    assert rt.weight_f16(p) is v.f16
    assert tr.take(**_views(v)) == [("cast", "f16", (64, 128))]


def test_adopted_record_without_byte_view_gets_a_padded_one_of_its_own(traced):
    rt, tr = traced
    v = _adopted(rt, lo8=False)
    e = rt.weight_f8(v.p)
    assert e is not v.e4m3 and tuple(e.shape) == (64, 128)
    assert tr.take(own=e, **_views(v)) == [("quant_e4m3", "own", (64, 128))]
    rt.invalidate_weight_images()          # not external: stale again
    assert rt.weight_f8(v.p) is e
    assert tr.take(own=e, **_views(v)) == [("quant_e4m3", "own", (64, 128))]


def test_packed_image_comes_to_life_on_demand(traced):
    rt, tr = traced
    v = _adopted(rt)
    p = v.p
    assert rt.weight_packed(p) is None and not rt.packed_live(p)
    assert tr.queries == [] and tr.take() == []
    tr.wanted = False
    assert rt.weight_packed(p, 4096) is None and not rt.packed_live(p)
    assert tr.queries == [(4096, 64, 128)] and tr.take() == []
    tr.wanted = True
    assert rt.weight_packed(p, 4096) is v.pk and rt.packed_live(p)
    assert tr.take(**_views(v)) == [("pack_weight", "pk", (8192,))]
    del tr.queries[:]
    assert rt.weight_packed(p, 4096) is v.pk and rt.weight_packed(p) is v.pk
    assert tr.queries == [] and tr.take() == []        # live: no more questions, fresh: no more packing
    with torch.no_grad():
        p.mul_(2.0)
    assert rt.weight_packed(p) is v.pk
    assert tr.take(**_views(v)) == [("pack_weight", "pk", (8192,))]
    assert rt.weight_packed(p) is v.pk and tr.take() == []
    # a record adopted without a packed tensor has no packed image, whatever the dispatcher would say
    q = _param(64, 128, seed=3)
    rt.adopt_weight_image(q, torch.zeros(64, 128, dtype=torch.bfloat16))
    assert rt.weight_packed(q, 4096) is None and not rt.packed_live(q) and tr.queries == []


def test_adopting_again_starts_a_fresh_record(traced):
    rt, tr = traced
    v = _adopted(rt)
    assert rt.weight_packed(v.p, 4096) is v.pk
    tr.take()
    rt.adopt_weight_image(v.p, v.bf16, packed=v.pk)
    assert not rt.packed_live(v.p) and rt.weight_packed(v.p) is None
    h = rt.weight_f16(v.p)                  # the fp16 view is gone with the old record: a cast image of its own
    assert h is not v.f16
    assert tr.take(own=h, **_views(v)) == [("cast", "own", (64, 128))]


def test_invalidation_spares_adopted_images_unless_told_otherwise(traced):
    rt, tr = traced
    v = _adopted(rt)
    p, q = v.p, _param(70, 100)
    w, h, e = rt.weight_images(q), rt.weight_f16(q), rt.weight_f8(q)
    assert rt.weight_packed(p, 4096) is v.pk
    tr.take()
    rt.invalidate_weight_images(False)
    rt.weight_images(p), rt.weight_f16(p), rt.weight_f8(p), rt.weight_packed(p)
    assert tr.take() == []
    assert (rt.weight_images(q), rt.weight_f16(q), rt.weight_f8(q)) == (w, h, e)
    assert tr.take(bf16=w, f16=h, e4m3=e) == [("cast", "bf16", (70, 100)), ("cast", "f16", (70, 100)), ("quant_e4m3", "e4m3", (128, 128))]
    rt.invalidate_weight_images(True)
    rt.weight_images(p), rt.weight_f16(p), rt.weight_f8(p), rt.weight_packed(p)
    assert rt.packed_live(p)
    assert tr.take(**_views(v)) == [("cast", "bf16", (64, 128)), ("cast", "f16", (64, 128)), ("quant_e4m3", "e4m3", (64, 128)),
                                    ("pack_weight", "pk", (8192,))]
    rt.weight_images(q), rt.weight_f16(q), rt.weight_f8(q)
    assert tr.take(bf16=w, f16=h, e4m3=e) == [("cast", "bf16", (70, 100)), ("cast", "f16", (70, 100)), ("quant_e4m3", "e4m3", (128, 128))]


def test_invalidation_of_a_packed_image_that_is_not_live_packs_nothing(traced):
    rt, tr = traced
    v = _adopted(rt)
    rt.invalidate_weight_images(True)
    assert rt.weight_packed(v.p) is None and not rt.packed_live(v.p) and tr.take() == []
    assert rt.weight_packed(v.p, 4096) is v.pk
    assert tr.take(**_views(v)) == [("pack_weight", "pk", (8192,))]


def test_dead_parameters_leave_the_registry(traced):
    rt, tr = traced
    before = len(rt._wlist)
    v = _adopted(rt)
    q = _param(70, 100)
    rt.weight_f16(q)
    for _ in range(3):                      # one weak reference per parameter, however often its record is rebuilt
        q.data = q.data.clone()
        rt.weight_images(q)
        rt.adopt_weight_image(v.p, v.bf16, packed=v.pk)
    assert len(rt._wlist) - before == 2
    rt.invalidate_weight_images()
    assert len(rt._wlist) - before == 2
    del v, q
    gc.collect()
    rt.invalidate_weight_images()
    assert len(rt._wlist) == before
