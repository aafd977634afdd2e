"""CPU: weight averaging without a GPU.  The two entry points of the C-ABI (afft_ema, afft_swap_f32; csrc/optim.hip) are exported with
the header's signatures, and each of their host checks returns 1 with its message before any HIP call (dummy pointers, as in
tests/test_ce_host_checks_cpu.py).  The host logic of afft_amd.optim.WeightEMA runs on the torch doubles of tests/ema_double.py:
warm-up schedule, the ema_decay / sharded refusals, state_dict through torch.save, averaged_state_dict, applied() and its guards,
and the wiring into SGD / AdamW / Trainer / evaluate (off by default: no buffer and no call)."""
import ctypes
import io
import os

import pytest
import torch

from ema_double import doubles
from test_optim_cpu import _groups, _loop
from test_parallel_cpu import WTS, _afft_case, _afft_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, PTR2 = 0x1000, 0x9000      # non-null, 16-byte aligned, 32 KiB apart: nothing reads them


@pytest.fixture(scope="module")
def lib():
    from afft_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "afft_amd", "csrc"), "-j4"])
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("afft_ema", "afft_swap_f32"):
        fn = getattr(so, name)
        fn.argtypes, fn.restype = _lib._SIGS[name]
    so.afft_last_error.argtypes, so.afft_last_error.restype = [], ctypes.c_char_p
    return so


def ema(lib, e=PTR, p=PTR2, n=0, w=0.5, ok=None):
    return lib.afft_ema(e, p, n, w, ok, None), lib.afft_last_error().decode()


def swap(lib, a=PTR, b=PTR2, n=0):
    return lib.afft_swap_f32(a, b, n, None), lib.afft_last_error().decode()


def test_both_symbols_are_exported_with_the_header_s_signatures(lib):
    from afft_amd import _lib
    vp, i64, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert _lib._SIGS["afft_ema"] == ([vp, vp, i64, f32, vp, vp], ctypes.c_int)
    assert _lib._SIGS["afft_swap_f32"] == ([vp, vp, i64, vp], ctypes.c_int)
    assert {"afft_ema", "afft_swap_f32"} <= set(_lib.EXPORTS)
    assert (_lib.K_EMA, _lib.K_SWAP_F32) == (5, 6)
    assert lib.afft_ema and lib.afft_swap_f32      # the library has them (the fixture bound them by name)


def test_ema_host_checks(lib):
    """n > 0 throughout: a case that passed a check it should fail would go on to launch on the dummy pointers"""
    assert ema(lib, n=-1) == (1, "ema: negative length")
    for w in (-0.25, 1.5, float("nan"), float("inf")):
        assert ema(lib, n=8, w=w) == (1, "ema: w must lie in [0, 1] (got %g)" % ctypes.c_float(w).value)
    assert ema(lib, e=None, n=8) == (1, "ema: null pointer")
    assert ema(lib, p=None, n=8) == (1, "ema: null pointer")
    assert ema(lib, e=PTR + 2, n=8) == (1, "ema: buffers must be 4-byte aligned")
    assert ema(lib, p=PTR2 + 1, n=8) == (1, "ema: buffers must be 4-byte aligned")
    # nothing to do: no launch, whatever the pointers; the argument checks still come first
    assert ema(lib, n=0)[0] == 0 and ema(lib, e=None, p=None, n=0)[0] == 0
    assert ema(lib, n=8, w=0.0)[0] == 0
    assert ema(lib, n=0, w=2.0)[0] == 1 and ema(lib, e=PTR + 2, n=0)[0] == 1


def test_swap_host_checks(lib):
    assert swap(lib, n=-1) == (1, "swap_f32: negative length")
    assert swap(lib, a=None, n=8) == (1, "swap_f32: null pointer")
    assert swap(lib, b=None, n=8) == (1, "swap_f32: null pointer")
    assert swap(lib, a=PTR + 2, n=8) == (1, "swap_f32: buffers must be 4-byte aligned")
    assert swap(lib, b=PTR2 + 3, n=8) == (1, "swap_f32: buffers must be 4-byte aligned")
    over = "swap_f32: the buffers overlap"
    assert swap(lib, a=PTR, b=PTR, n=1) == (1, over)
    assert swap(lib, a=PTR, b=PTR + 4 * 7, n=8) == (1, over)
    assert swap(lib, a=PTR + 4 * 7, b=PTR, n=8) == (1, over)
    assert swap(lib, n=0)[0] == 0 and swap(lib, a=None, b=None, n=0)[0] == 0 and swap(lib, a=PTR, b=PTR, n=0)[0] == 0


# ----------------------------------------------------------------------------- WeightEMA on the doubles
def _sgd(model, **kw):
    from afft_amd.optim import SGD
    return SGD(_groups(model), lr=1e-2, momentum=0.9, nesterov=True, bucket_elems=8192, **kw)


def test_warmup_schedule_is_the_closed_form_and_reaches_the_kernel_as_fp32_of_one_minus_decay():
    from afft_amd import ops
    from afft_amd.optim import WeightEMA
    c, state, *_ = _afft_case()
    with doubles():
        model = _afft_model(c, state, "fp32")
        opt = _sgd(model)
        seen = []
        real = ops.ema
        ops.ema = lambda e, p, w, ok=None: seen.append((w, ok))
        try:
            for decay, warm in ((0.9998, True), (0.9, True), (0.9998, False)):
                avg = WeightEMA(opt, decay, warmup=warm)
                assert avg.ok is opt.opt.ok
                for t in (0, 1, 9, 10 ** 4):
                    want = min(decay, (1 + t) / (10 + t)) if warm else decay
                    assert avg.decay_at(t) == want
                    avg.num_updates = t
                    avg.update()
                    assert avg.num_updates == t + 1
                    w, ok = seen[-1]
                    assert w == ctypes.c_float(1.0 - want).value and ok is opt.opt.ok, (decay, warm, t)
        finally:
            ops.ema = real
    assert min(0.9998, 10001 / 10010) == 10001 / 10010 and min(0.9, 10 / 19) == 10 / 19      # the cases above sit on both branches


@pytest.mark.parametrize("bad", [0.0, 1.0, -0.1, 1.5, float("nan"), "0.99"])
def test_a_bad_ema_decay_is_a_value_error_at_construction(bad):
    from afft_amd.optim import SGD, AdamW, WeightEMA
    from afft_amd.parallel import FlatParams, Trainer
    c, state, *_ = _afft_case()
    with doubles():
        model = _afft_model(c, state, "fp32")
        before = [p.data_ptr() for p in model.parameters()]
        with pytest.raises(ValueError, match="ema_decay"):
            SGD(_groups(model), lr=1e-2, momentum=0.9, ema_decay=bad)
        with pytest.raises(ValueError, match="ema_decay"):
            AdamW(_groups(model), lr=1e-3, ema_decay=bad)
        with pytest.raises(ValueError, match="ema_decay"):
            Trainer(model, WTS, ema_decay=bad)
        assert before == [p.data_ptr() for p in model.parameters()]      # refused before anything was re-homed
        with pytest.raises(ValueError, match="ema_decay"):
            WeightEMA(FlatParams(model), bad)


def test_sharded_update_on_more_than_one_rank_is_refused():
    from afft_amd.optim import WeightEMA
    c, state, *_ = _afft_case()
    with doubles():
        model = _afft_model(c, state, "fp32")
        opt = _sgd(model, comm_algo="sharded", ema_decay=0.99)      # one rank: every slice is this rank's, nothing is stale
        assert opt.ema is not None and opt.reducer.world == 1
        opt.reducer.world = 2
        with pytest.raises(NotImplementedError, match="sharded"):
            WeightEMA(opt, 0.99)
        opt.reducer.comm_algo = "allreduce"      # replicas are bitwise equal: nothing to refuse
        WeightEMA(opt, 0.99)


def test_off_by_default_no_buffer_no_call():
    from afft_amd import ops
    from afft_amd.parallel import Trainer
    c, state, data, tgt, sub = _afft_case()
    with doubles():
        calls = []
        ops.ema = lambda *a, **k: calls.append(a)
        m1, m2 = _afft_model(c, state, "fp32"), _afft_model(c, state, "fp32")
        opt = _sgd(m1)
        _loop(m1, opt, None, data, tgt, sub, 2)
        tr = Trainer(m2, WTS, lr=1e-2, momentum=0.9, weight_decay=1e-4, bucket_elems=8192)
        tr.step(data, {"action": tgt}, {"action": sub})
        assert opt.ema is None and tr.ema is None and not calls


@pytest.mark.parametrize("kind", ["SGD", "AdamW", "Trainer"])
def test_average_follows_the_recurrence_once_per_step(kind):
    """the flat parameters after every step, then the recurrence over them in float64: the update runs once per step, after it"""
    from afft_amd.optim import AdamW
    from afft_amd.parallel import Trainer
    c, state, data, tgt, sub = _afft_case()
    with doubles():
        model = _afft_model(c, state, "fp32")
        if kind == "Trainer":
            own = Trainer(model, WTS, lr=1e-2, momentum=0.9, weight_decay=1e-4, bucket_elems=8192, ema_decay=0.9, ema_warmup=False)
            step = lambda: own.step(data, {"action": tgt}, {"action": sub})      # noqa: E731
        else:
            own = _sgd(model, ema_decay=0.9) if kind == "SGD" else AdamW(_groups(model), lr=1e-3, bucket_elems=8192, ema_decay=0.9)
            step = lambda: _loop(model, own, None, data, tgt, sub, 1)            # noqa: E731
        ref = own.flat.flat_p.double().clone()
        assert torch.equal(own.ema.ema, own.flat.flat_p) and own.ema.ema.data_ptr() != own.flat.flat_p.data_ptr()
        for t in range(3):
            step()
            d = own.ema.decay_at(t)
            assert d == (0.9 if kind == "Trainer" else min(0.9, (1 + t) / (10 + t)))
            ref += ctypes.c_float(1.0 - d).value * (own.flat.flat_p.double() - ref)
        assert own.ema.num_updates == 3
        assert float((own.ema.ema.double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
        assert not torch.equal(own.ema.ema, own.flat.flat_p)
        # a step the optimizer skipped leaves the average; the host counter advances all the same
        own.opt.ok.zero_()
        snap = own.ema.ema.clone()
        own.ema.update()
        assert torch.equal(own.ema.ema, snap) and own.ema.num_updates == 4


def test_state_dict_round_trips_through_torch_save_and_stays_beside_the_optimizer_s():
    from afft_amd.optim import WeightEMA
    c, state, data, tgt, sub = _afft_case()
    with doubles():
        m1, m2 = _afft_model(c, state, "fp32"), _afft_model(c, state, "fp32")
        o1 = _sgd(m1, ema_decay=0.95, ema_warmup=False)
        _loop(m1, o1, None, data, tgt, sub, 2)
        sd = o1.ema.state_dict()
        assert set(sd) == {"decay", "warmup", "num_updates", "ema"} and (sd["decay"], sd["warmup"], sd["num_updates"]) == (0.95, False, 2)
        assert set(sd["ema"]) == {g["name"] for g in o1.param_groups} == {n for n, _ in m1.named_parameters()}
        for n, p in m1.named_parameters():
            assert sd["ema"][n].shape == p.shape
        assert "ema" not in o1.state_dict() and set(o1.state_dict()) == {"state", "param_groups"}
        f = io.BytesIO()
        torch.save(sd, f)
        f.seek(0)
        back = torch.load(f)
        o2 = _sgd(m2)
        avg = WeightEMA(o2)
        assert (avg.decay, avg.warmup, avg.num_updates) == (0.9998, True, 0) and not torch.equal(avg.ema, o1.ema.ema)
        avg.load_state_dict(back)
        assert (avg.decay, avg.warmup, avg.num_updates) == (0.95, False, 2) and torch.equal(avg.ema, o1.ema.ema)
        del back["ema"][next(iter(back["ema"]))]
        with pytest.raises(ValueError, match="names differ"):
            avg.load_state_dict(back)


def test_averaged_state_dict_has_the_module_s_keys_and_loads_into_a_fresh_model():
    c, state, data, tgt, sub = _afft_case()
    with doubles():
        model = _afft_model(c, state, "fp32")
        model.register_buffer("extra_counter", torch.arange(3.0))
        opt = _sgd(model, ema_decay=0.5, ema_warmup=False)
        _loop(model, opt, None, data, tgt, sub, 2)
        asd = opt.ema.averaged_state_dict(model)
        msd = model.state_dict()
        assert list(asd) == list(msd) and "extra_counter" in asd
        ix = opt.flat.index_of()
        for k, t in model.state_dict(keep_vars=True).items():
            assert asd[k].shape == t.shape and asd[k].data_ptr() != t.data_ptr()
            if id(t) in ix:
                o = opt.flat.offsets[ix[id(t)]]
                assert torch.equal(asd[k].reshape(-1), opt.ema.ema[o:o + t.numel()]) and not torch.equal(asd[k], t.detach()), k
            else:
                assert torch.equal(asd[k], t.detach()), k
        fresh = _afft_model(c, state, "fp32")
        fresh.register_buffer("extra_counter", torch.zeros(3))
        fresh.load_state_dict(asd, strict=True)
        assert torch.equal(fresh.extra_counter, torch.arange(3.0))


def test_applied_exchanges_refreshes_restores_and_guards():
    from afft_amd import evaluate as ev
    c, state, data, tgt, sub = _afft_case()
    with doubles():
        model = _afft_model(c, state, "fp32")
        opt = _sgd(model, ema_decay=0.5, ema_warmup=False)
        _loop(model, opt, None, data, tgt, sub, 2)
        flat, avg = opt.flat, opt.ema
        p0, e0 = flat.flat_p.clone(), avg.ema.clone()
        refreshed = []
        real = flat.refresh_images
        flat.refresh_images = lambda: (refreshed.append(flat.flat_p.clone()), real())[1]
        with avg.applied() as inside:
            assert inside is avg and flat.averaged
            assert torch.equal(flat.flat_p, e0) and torch.equal(avg.ema, p0)
            assert torch.equal(next(model.parameters()).detach().reshape(-1), e0[:next(model.parameters()).numel()])
            for call in (avg.update, opt.zero_grad, opt.step, avg.state_dict, lambda: avg.averaged_state_dict(model),
                         lambda: avg.applied().__enter__()):
                with pytest.raises(RuntimeError, match="applied"):
                    call()
        assert not flat.averaged and torch.equal(flat.flat_p, p0) and torch.equal(avg.ema, e0)
        assert len(refreshed) == 2 and torch.equal(refreshed[0], e0) and torch.equal(refreshed[1], p0)      # after each exchange
        # an exception inside still restores
        with pytest.raises(KeyError):
            with avg.applied():
                raise KeyError("x")
        assert not flat.averaged and torch.equal(flat.flat_p, p0) and torch.equal(avg.ema, e0)
        _loop(model, opt, None, data, tgt, sub, 1)      # and training goes on
        # evaluate(..., ema=) runs the whole evaluation inside applied()
        seen = {}

        def fake_collect(model_, loader, device, precision=None):
            seen["averaged"] = flat.averaged
            raise StopIteration
        real_collect, ev.collect_logits = ev.collect_logits, fake_collect
        try:
            with pytest.raises(StopIteration):
                ev.evaluate(model, None, [], torch.device("cpu"), ema=avg)
        finally:
            ev.collect_logits = real_collect
        assert seen == {"averaged": True} and not flat.averaged
    import afft_amd
    afft_amd.set_precision("bf16")
