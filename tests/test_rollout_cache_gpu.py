"""GPU: the roll-out of the future predictor over a key / value cache (BaseFuturePredictor.forward with output_len > 1 in evaluation,
GPT2Model.forward_step, afft_attention_step_fwd) at model level: against the reference's golden of the tiny roll-out configuration
(t2_roll, fp_output_len = 3) within the bars of tests/test_model_gpu.py (fp32 1e-3 relative L2 and 3e-3 max-relative, bf16 2e-2 / 6e-2),
with the switch off, with grad enabled (the cached path must not engage: bitwise the recompute), at output_len == 1, and once at the
real head size.  The golden holds no temporal attention maps (the reference's fixture was made with output_attentions off), so gpt2_att_*
is compared with the CPU oracle on the same weights, which tests/test_oracle_golden.py pins to that golden."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cases import oracle_cfg  # noqa: E402
from helpers import case_tensors, flatten_outputs, load_golden, max_rel, rel_l2  # noqa: E402

TOL = {"fp32": 1e-3, "bf16": 2e-2}      # tests/test_model_gpu.py TOL
NAME = "t2_roll"
_REF = {}


def _reference():
    """the golden, the case's tensors and the oracle's temporal attention maps: made once, shared, never modified"""
    if not _REF:
        from oracle import afft_oracle as O
        z, _ = load_golden(NAME)
        c, state, data, tgt, sub = case_tensors(NAME)
        with torch.no_grad():
            oout = O.base_model_forward({k: v.clone() for k, v in state.items()}, data, dict(oracle_cfg(c), output_attentions=True))
        _REF.update(z=z, c=c, state=state, data=data, tgt=tgt, sub=sub, att=oout["attentions"]["all-fused"]["temporal_attns"])
    return _REF


class _count_steps:
    """how many times ops.attention_step ran inside the block"""

    def __enter__(self):
        from afft_amd import ops
        self.ops, self.real, self.n = ops, ops.attention_step, 0

        def counted(*a, **k):
            self.n += 1
            return self.real(*a, **k)
        ops.attention_step = counted
        return self

    def __exit__(self, *exc):
        self.ops.attention_step = self.real


def _model(precision):
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.config import make_model_cfg
    from afft_amd.models.base_model import BaseModel
    r = _reference()
    c = r["c"]
    afft_amd.set_precision(precision)
    rt.set_grad_mode("sink")
    cfg = make_model_cfg(c["modal_dims"], c["d"], c["D"], fuser=c["fuser"], depth=c["depth"], num_heads=c["num_heads"],
                         fp_layers=c["fp_layers"], fp_heads=c["fp_heads"], fp_output_len=c["fp_output_len"], T=c["T"],
                         fp_output_attentions=True)
    model = BaseModel(cfg, num_classes={"action": c["num_classes"]}, class_mappings={})
    model.load_state_dict(r["state"], strict=True)
    return model.cuda().eval()


def _forward(model, grad):
    r = _reference()
    dev = torch.device("cuda:0")
    from afft_amd import runtime as rt
    rt.SINK.begin_step()
    with torch.set_grad_enabled(grad), _count_steps() as steps:
        out, _ = model({m: d.to(dev) for m, d in r["data"].items()}, mixup_fn=None, target={"action": r["tgt"].to(dev)},
                       target_subclips={"action": r["sub"].to(dev)}, target_subclips_ignore_index=None)
    torch.cuda.synchronize()
    flat = {k: v.detach().float().cpu() for k, v in flatten_outputs(out).items()}
    att = {k: v.detach().float().cpu() for k, v in out["attentions"]["all-fused"]["temporal_attns"].items()}
    return flat, att, steps.n


@pytest.fixture()
def switch():
    import afft_amd
    from afft_amd import runtime as rt
    saved = rt.kv_cache()
    yield rt
    rt.set_kv_cache(saved)
    afft_amd.set_precision("bf16")


@pytest.mark.parametrize("cache", [True, False], ids=["cached", "recompute"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_rollout_matches_reference_golden(precision, cache, switch):
    r = _reference()
    c, z, tol = r["c"], r["z"], TOL[precision]
    switch.set_kv_cache(cache)
    flat, att, steps = _forward(_model(precision), grad=False)
    assert steps == (c["fp_layers"] * c["fp_output_len"] if cache else 0)      # the path under test is the one that ran
    worst, checked = 0.0, 0
    for k in z.files:
        if not k.startswith("out:"):
            continue
        ref = torch.from_numpy(z[k])
        got = flat[k[4:]]
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        e, em = rel_l2(got, ref), max_rel(got, ref)
        worst = max(worst, e, em)
        assert e < tol and em < tol * 3, (k, e, em)
        checked += 1
    assert checked >= 6
    T, B, H, layers = c["T"], c["B"], c["fp_heads"], c["fp_layers"]
    assert sorted(att) == [f"gpt2_att_{i}" for i in range(c["fp_output_len"])]
    for i in range(c["fp_output_len"]):
        got, ref = att[f"gpt2_att_{i}"], r["att"][f"gpt2_att_{i}"]
        assert got.shape == ref.shape == ((B, layers, H, T, T) if i == 0 else (B, layers, H, 1, T + i))
        e, em = rel_l2(got, ref), max_rel(got, ref)
        worst = max(worst, e, em)
        assert e < tol and em < tol * 3, (i, e, em)
    print(f"[{NAME}/{precision}/{'cached' if cache else 'recompute'}] worst output / attention error {worst:.2e}")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_grad_enabled_keeps_the_recompute_bitwise(precision, switch):
    """with grad enabled the cached path must not engage: the switch changes no bit"""
    model = _model(precision)
    runs = {}
    for on in (True, False):
        switch.set_kv_cache(on)
        flat, att, steps = _forward(model, grad=True)
        assert steps == 0
        runs[on] = dict(flat, **att)
    for k, v in runs[True].items():
        assert torch.equal(v, runs[False][k]), k


def _predictor(D, H, layers, seed):
    from afft_amd.models.future_prediction import BaseFuturePredictor
    torch.manual_seed(seed)
    return BaseFuturePredictor(D, inter_dim=D, n_layer=layers, n_head=H, embd_pdrop=0.0, resid_pdrop=0.0, attn_pdrop=0.0,
                               output_attentions=True).eval()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_output_len_1_is_untouched_bitwise(precision, switch):
    import afft_amd
    afft_amd.set_precision(precision)
    pred = _predictor(64, 2, 2, seed=3).cuda()
    feats = torch.randn(3, 5, 64, generator=torch.Generator().manual_seed(4)).cuda()
    runs = {}
    for on in (True, False):
        switch.set_kv_cache(on)
        with torch.no_grad(), _count_steps() as steps:
            out, att = pred(feats, 1)
        assert steps.n == 0
        runs[on] = (out.cpu(), att["gpt2_att_0"].cpu())
    assert torch.equal(runs[True][0], runs[False][0]) and torch.equal(runs[True][1], runs[False][1])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_real_head_size_cached_against_recompute(precision, switch):
    """D = 2048, H = 4 (head dimension 512), 1 layer, B = 2, T = 16, output_len = 3: cached against recompute.
    fp32: relative L2 of the difference at most 10 x the measured error of the RECOMPUTE against the float64 oracle on the same weights,
    computed here for this very case (both are fp32-grade; the step kernel sums in another order than the generic kernel and the
    GEMMs see other row counts).  bf16: the mode's output tolerance, 2e-2.
    Measured on an MI355X (the test prints the figures of its run; profiles/rollout_cache.txt):
      fp32: recompute vs oracle 1.17e-06, cached vs oracle 1.18e-06, cached vs recompute 5.98e-07 (bound 1.17e-05), attention maps 9.18e-07
      bf16: recompute vs oracle 2.45e-03, cached vs oracle 2.42e-03, cached vs recompute 1.61e-03 (bound 2e-2), attention maps 3.57e-03"""
    import afft_amd
    from oracle import afft_oracle as O
    D, H, B, T, n_out = 2048, 4, 2, 16, 3
    afft_amd.set_precision(precision)
    pred = _predictor(D, H, 1, seed=5)
    feats = torch.randn(B, T, D, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        o_ref, a_ref = O.future_predictor({k: v.double() for k, v in pred.state_dict().items()}, "", feats.double(), 1, H, n_out, True)
    pred, x = pred.cuda(), feats.cuda()
    runs = {}
    for on in (True, False):
        switch.set_kv_cache(on)
        with torch.no_grad(), _count_steps() as steps:
            out, att = pred(x, n_out)
        assert steps.n == (n_out if on else 0)
        runs[on] = (out.float().cpu(), {k: v.float().cpu() for k, v in att.items()})
    assert runs[True][0].shape == (B, T + n_out - 1, D)
    recompute_vs_oracle = rel_l2(runs[False][0], o_ref)
    cached_vs_oracle = rel_l2(runs[True][0], o_ref)
    cached_vs_recompute = rel_l2(runs[True][0], runs[False][0])
    att_diff = max(rel_l2(runs[True][1][k], runs[False][1][k]) for k in a_ref)
    print(f"[real head size/{precision}] recompute vs oracle {recompute_vs_oracle:.2e}  cached vs oracle {cached_vs_oracle:.2e}  "
          f"cached vs recompute {cached_vs_recompute:.2e}  attention maps cached vs recompute {att_diff:.2e}")
    bound = 10 * recompute_vs_oracle if precision == "fp32" else TOL["bf16"]
    assert cached_vs_recompute < bound and att_diff < bound, (cached_vs_recompute, att_diff, bound)
    for k in a_ref:
        assert runs[True][1][k].shape == a_ref[k].shape
