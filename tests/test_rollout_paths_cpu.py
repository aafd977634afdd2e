"""Build-container test that PINS what each roll-out path of BaseFuturePredictor hands to afft_amd.ops, on CPU tensors with the doubles of
tests/cpu_ops_step.py, cpu_ops_step_train.py and cpu_ops_step_f16x2.py: every public callable of afft_amd.ops is wrapped with a recorder,
and the ordered list of calls -- with the output shape of every GEMM, (Lq, Lk) and whether `probs` / `drop` were passed for the attention
step, and whether the LayerNorm was asked for its statistics -- is compared with the lists written out below.  The lists say what the code
did before the three cached roll-outs were folded into one path; a reshaping of the host code leaves them as they are.  Also here: the
rule that selects the path (recompute, cached evaluation, cached training), as one case list."""
import contextlib

import pytest
import torch

import cpu_ops_step
import cpu_ops_step_f16x2
import cpu_ops_step_train

B, T, D, H, LAYERS, OUT = 3, 4, 64, 2, 2, 3      # D = 64: the fp16x2 composite step is in play; B = 3: the one-row steps pad 3 rows to 64


def _ops_names():
    from afft_amd import ops
    return [n for n, v in vars(ops).items() if not n.startswith("_") and callable(v) and getattr(v, "__module__", None) == ops.__name__]


@contextlib.contextmanager
def _recording(log, names):
    """every public callable of afft_amd.ops (`names`, taken before the doubles went in; what is wrapped is what is installed now) behind a
    wrapper that appends one line per call to `log`"""
    from afft_amd import ops
    saved = {n: getattr(ops, n) for n in names}

    def wrap(name, fn):
        def rec(*a, **k):
            if name == "gemm":
                log.append("gemm %dx%d" % tuple(a[2].shape))
            elif name in ("attention_step", "attention_step_bwd"):
                probs = a[12] if name == "attention_step" else a[4]
                log.append("%s %d/%d%s%s" % (name, a[6], a[7], " probs" if probs is not None else "", " drop" if "drop" in k else ""))
            elif name == "attn_step_sublayer_f16x2":
                log.append("%s %d/%d%s" % (name, a[8], a[9], " probs" if a[18] is not None else ""))
            elif name == "layernorm_fwd":
                log.append(name + (" stats" if len(a) > 5 or "mean" in k else ""))
            else:
                log.append(name)
            return fn(*a, **k)
        return rec
    for n, f in saved.items():
        setattr(ops, n, wrap(n, f))
    try:
        yield
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)


@pytest.fixture()
def rt_state():
    import afft_amd
    from afft_amd import runtime as rt
    saved = rt.kv_cache(), rt.kv_cache_train(), rt.kv_cache_fp16x2(), rt.grad_mode()
    rt.set_grad_mode("autograd")
    yield rt
    afft_amd.set_precision("bf16")
    rt.set_kv_cache(saved[0])
    rt.set_kv_cache_train(saved[1])
    rt.set_kv_cache_fp16x2(saved[2])
    rt.set_grad_mode(saved[3])


def _predictor(output_attentions=True):
    from afft_amd.models.future_prediction import BaseFuturePredictor
    torch.manual_seed(0)
    return BaseFuturePredictor(D, inter_dim=D, n_layer=LAYERS, n_head=H, embd_pdrop=0.0, resid_pdrop=0.0, attn_pdrop=0.0,
                               output_attentions=output_attentions)


def _run(rt, precision, path, output_attentions=True):
    """(calls of the forward, calls of the backward) of one fresh predictor on `path`: 'recompute', 'eval' or 'train'"""
    import afft_amd
    afft_amd.set_precision(precision)
    rt.set_kv_cache(path != "recompute")
    rt.set_kv_cache_train(path == "train")
    rt.set_kv_cache_fp16x2(precision == "fp16x2")
    train = path == "train"
    m = _predictor(output_attentions).train(train)
    x = torch.randn(B, T, D, requires_grad=train)
    doubles = cpu_ops_step_f16x2 if precision == "fp16x2" else cpu_ops_step_train if train else cpu_ops_step
    log, names = [], _ops_names()
    with doubles.installed(), _recording(log, names), torch.set_grad_enabled(train):
        out, att = m(x, OUT)
        n_fwd = len(log)
        if train:
            out.sum().backward()
    assert out.shape == (B, T + OUT - 1, D) and (sorted(att) == [f"gpt2_att_{i}" for i in range(OUT)] if output_attentions else att == {})
    return log[:n_fwd], log[n_fwd:]


# ---------------------------------------------------------------- the pinned sequences
def _block(R, core, before_gemm=()):
    """one GPT-2 block call by call on R rows: LN, QKV, core, projection; LN, fc1, fc2"""
    g = lambda n: list(before_gemm) + [f"gemm {R}x{n}"]      # noqa: E731
    ln = ["layernorm_fwd stats"]
    return ln + g(3 * D) + [core] + g(D) + ln + g(4 * D) + g(D)


def _pass(R, core, before_gemm=(), stats=" stats"):
    """positions, the blocks, ln_f (stats: through LayerNormRows, which keeps mean and rstd for its backward; "": the bare evaluation call)"""
    return ["add_rows_periodic"] + _block(R, core, before_gemm) * LAYERS + ["layernorm_fwd" + stats]


def _cached(core, first=(), later=(), stats="", tail=""):
    """the T observed frames once, then one row per clip and predicted frame; first / later: what precedes every GEMM of the first pass
    (fresh weight images) and of the later ones"""
    return (_pass(B * T, f"{core} {T}/{T} probs{tail}", first, stats) + _pass(B, f"{core} 1/{T + 1} probs{tail}", later, stats)
            + _pass(B, f"{core} 1/{T + 2} probs{tail}", later, stats))


def _f16x2_pass(Lq, Lk, images=()):
    half = lambda name: list(images) + [name]      # noqa: E731
    return (["add_rows_periodic"] + (half(f"attn_step_sublayer_f16x2 {Lq}/{Lk} probs") + half("mlp_step_sublayer_f16x2")) * LAYERS
            + ["layernorm_fwd"])


FORWARD = {
    ("fp32", "recompute"): _pass(B * T, "attention_fwd") + _pass(B * (T + 1), "attention_fwd") + _pass(B * (T + 2), "attention_fwd"),
    ("fp32", "eval"): _cached("attention_step"),
    ("bf16", "eval"): _cached("attention_step", first=["cast"]),                       # the bf16 image of each weight, once
    ("bf16x3", "eval"): _cached("attention_step", first=["Split", "Split"], later=["Split"]),      # activation planes (+ the weight's, once)
    ("fp16x2", "eval"): _f16x2_pass(T, T, images=["cast"] * 4) + _f16x2_pass(1, T + 1) + _f16x2_pass(1, T + 2),
    ("fp32", "train"): _cached("attention_step", stats=" stats", tail=" drop"),
    ("bf16", "train"): _cached("attention_step", first=["cast"], stats=" stats", tail=" drop"),
}


def _bwd_block(R, core, handed_mlp, handed_attn):
    """one block's backward on R rows.  handed: dy came with the sub-layer downstream's hand-over (bf16 only) -- no cast of dy, and the
    output bias's gradient with it (no colsum)"""
    mlp = ([] if handed_mlp is not False else ["cast"]) + [f"gemm {4 * D}x{D}"] + ([] if handed_mlp else ["colsum"]) + [
        f"gemm {R}x{4 * D}", f"gemm {D}x{4 * D}", "colsum", f"gemm {R}x{D}", "layernorm_bwd"]
    attn = [f"gemm {D}x{D}"] + ([] if handed_attn else ["colsum"]) + [f"gemm {R}x{D}", core, f"gemm {D}x{3 * D}", "colsum", f"gemm {R}x{D}",
                                                                     "layernorm_bwd"]
    return mlp + attn


def _bwd_pass(R, Lq, Lk, bf16):
    core = f"attention_step_bwd {Lq}/{Lk} probs drop"
    if bf16:      # the last block's MLP takes dy from ln_f (no hand-over: a cast); everything upstream of it is handed its dy
        blocks = _bwd_block(R, core, False, True) + _bwd_block(R, core, True, True) * (LAYERS - 1)
    else:         # fp32: dy is used in place (None: no cast), every bias gradient is a colsum
        blocks = _bwd_block(R, core, None, False) * LAYERS
    return ["layernorm_bwd"] + blocks + ["reduce_rows_periodic"]


BACKWARD = {prec: _bwd_pass(B, 1, T + 2, prec == "bf16") + _bwd_pass(B, 1, T + 1, prec == "bf16") + _bwd_pass(B * T, T, T, prec == "bf16")
            for prec in ("fp32", "bf16")}


@pytest.mark.parametrize("precision,path", sorted(FORWARD))
def test_ops_call_sequence(rt_state, precision, path):
    fwd, bwd = _run(rt_state, precision, path)
    assert fwd == FORWARD[precision, path]
    assert bwd == (BACKWARD[precision] if path == "train" else [])


def test_recorder_wraps_every_public_callable_of_ops():
    names = _ops_names()
    assert {"gemm", "Split", "layernorm_fwd", "attention_step", "attention_step_bwd", "attn_step_sublayer_f16x2", "mlp_step_sublayer_f16x2",
            "attention_fwd", "attention_bwd", "add_rows_periodic", "cast", "colsum"} <= set(names)
    assert not any(n in names for n in ("Tensor", "Optional", "torch"))


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3", "fp16x2"])
def test_no_probs_reach_the_step_without_output_attentions(rt_state, precision):
    fwd, _ = _run(rt_state, precision, "eval", output_attentions=False)
    steps = [c for c in fwd if c.startswith(("attention_step", "attn_step_sublayer_f16x2"))]
    assert len(steps) == LAYERS * OUT and not any("probs" in c for c in steps)


# ---------------------------------------------------------------- which path a call takes
# (output_len, grad enabled, training mode, kv_cache, kv_cache_train, kv_cache_fp16x2, precision) -> the GPT2Model method the roll-out runs
PATHS = [
    (1, False, False, True, True, True, "bf16", "forward_rows"),            # output_len == 1: nothing to roll out
    (1, True, True, True, True, True, "bf16", "forward_rows"),
    (3, False, False, True, False, False, "bf16", "forward_step"),          # evaluation: the cache, by default
    (3, False, False, True, False, False, "fp32", "forward_step"),
    (3, False, False, True, False, False, "bf16x3", "forward_step"),
    (3, False, False, True, True, False, "bf16", "forward_step"),           # (the training switch does not touch evaluation)
    (3, False, False, True, False, False, "fp16x2", "forward_rows"),        # fp16x2 evaluates through it only with its own switch
    (3, False, False, True, True, False, "fp16x2", "forward_rows"),
    (3, False, False, True, False, True, "fp16x2", "forward_step"),
    (3, False, False, True, False, True, "bf16", "forward_step"),           # (that switch changes nothing elsewhere)
    (3, True, False, True, False, False, "bf16", "forward_rows"),           # grad enabled or training mode: the recompute, by default
    (3, False, True, True, False, False, "bf16", "forward_rows"),
    (3, True, True, True, False, True, "fp32", "forward_rows"),
    (3, True, False, True, True, False, "bf16", "forward_step_train"),      # ... and the cache with the training switch
    (3, False, True, True, True, False, "bf16", "forward_step_train"),
    (3, True, True, True, True, False, "fp32", "forward_step_train"),
    (3, True, True, True, True, False, "bf16x3", "forward_step_train"),
    (2, True, False, True, True, True, "bf16", "forward_step_train"),
    (3, True, False, True, True, False, "fp16x2", "forward_rows"),          # fp16x2 never trains through the cache
    (3, False, True, True, True, True, "fp16x2", "forward_rows"),
    (3, True, True, True, True, True, "fp16x2", "forward_rows"),
    (3, False, False, False, False, False, "bf16", "forward_rows"),         # AFFT_KV_CACHE=0 wins over everything
    (3, False, False, False, True, True, "fp16x2", "forward_rows"),
    (3, False, False, False, True, True, "fp32", "forward_rows"),
    (3, True, True, False, True, True, "bf16", "forward_rows"),
    (3, True, False, False, True, False, "bf16x3", "forward_rows"),
]


class _Taken(Exception):
    pass


@pytest.mark.parametrize("output_len,grad,training,kv,kv_train,kv_f16x2,precision,want", PATHS)
def test_path_selection(rt_state, output_len, grad, training, kv, kv_train, kv_f16x2, precision, want):
    import afft_amd
    afft_amd.set_precision(precision)
    rt_state.set_kv_cache(kv)
    rt_state.set_kv_cache_train(kv_train)
    rt_state.set_kv_cache_fp16x2(kv_f16x2)
    m = _predictor().train(training)

    def stop(name):
        def f(*a, **k):
            raise _Taken(name)
        return f
    for name in ("forward_rows", "forward_step", "forward_step_train"):
        setattr(m.gpt_model, name, stop(name))
    with torch.set_grad_enabled(grad), pytest.raises(_Taken) as e:
        m(torch.randn(B, T, D), output_len)
    assert str(e.value) == want
