"""GPU: the cached roll-out in the 'fp16x2' precision (runtime.kv_cache_fp16x2: GPT2Block.forward_step -> functional.attn_step /
mlp_step -> afft_attn_step_sublayer_fwd / afft_mlp_sublayer_fwd) at model level: against the reference's golden of the tiny roll-out
configuration (t2_roll, fp_output_len = 3) within the 1e-3 tests/test_model_gpu.py applies to this precision (2e-3 with every one-pass
site forced on, as its test_fp16x2_one_pass_sites_on_the_small_goldens), switch on against switch off, once at the full predictor width
with the GEMM trace read as test_fp16x2_forward_full_size reads it, and through evaluate.collect_logits.  The golden holds no temporal
attention maps, so gpt2_att_* is compared with the CPU oracle on the same weights (tests/test_rollout_cache_gpu.py does the same)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cases import oracle_cfg  # noqa: E402
from helpers import case_tensors, flatten_outputs, load_golden, rel_l2  # noqa: E402

TOL = 1e-3               # tests/test_model_gpu.py TOL["fp16x2"]
TOL_ALL_ONE_PASS = 2e-3  # tests/test_model_gpu.py test_fp16x2_one_pass_sites_on_the_small_goldens
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


class _count:
    """how many times the composite step and the call-by-call step ran inside the block"""

    def __enter__(self):
        from afft_amd import ops
        self.ops, self.real, self.composite, self.cbc = ops, (ops.attn_step_sublayer_f16x2, ops.attention_step), [], 0

        def composite(*a, **k):
            self.composite.append((a[8], a[9]))      # (Lq, Lk)
            return self.real[0](*a, **k)

        def cbc(*a, **k):
            self.cbc += 1
            return self.real[1](*a, **k)
        ops.attn_step_sublayer_f16x2, ops.attention_step = composite, cbc
        return self

    def __exit__(self, *exc):
        self.ops.attn_step_sublayer_f16x2, self.ops.attention_step = self.real


@pytest.fixture()
def switch():
    import afft_amd
    from afft_amd import runtime as rt
    saved = rt.kv_cache(), rt.kv_cache_fp16x2(), rt.one_pass_sites()
    min_dim = rt.set_one_pass_min_dim(0)
    rt.set_one_pass_min_dim(min_dim)
    yield rt
    rt.set_kv_cache(saved[0])
    rt.set_kv_cache_fp16x2(saved[1])
    rt.set_one_pass_sites(saved[2])
    rt.set_one_pass_min_dim(min_dim)
    afft_amd.set_precision("bf16")


def _model(fp_output_len=None, precision="fp16x2"):
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.config import make_model_cfg
    from afft_amd.models.base_model import BaseModel
    r = _reference()
    c = r["c"]
    afft_amd.set_precision(precision)
    rt.set_grad_mode("sink")
    cfg = make_model_cfg(c["modal_dims"], c["d"], c["D"], fuser=c["fuser"], depth=c["depth"], num_heads=c["num_heads"],
                         fp_layers=c["fp_layers"], fp_heads=c["fp_heads"], fp_output_len=fp_output_len or c["fp_output_len"], T=c["T"],
                         fp_output_attentions=True)
    model = BaseModel(cfg, num_classes={"action": c["num_classes"]}, class_mappings={})
    model.load_state_dict(r["state"], strict=True)
    return model.cuda().eval()


def _forward(model):
    r = _reference()
    dev = torch.device("cuda:0")
    from afft_amd import runtime as rt
    rt.SINK.begin_step()
    with torch.no_grad(), _count() as n:
        out, _ = model({m: d.to(dev) for m, d in r["data"].items()}, mixup_fn=None, target={"action": r["tgt"].to(dev)},
                       target_subclips={"action": r["sub"].to(dev)}, target_subclips_ignore_index=None)
    torch.cuda.synchronize()
    flat = {k: v.detach().float().cpu() for k, v in flatten_outputs(out).items()}
    att = {k: v.detach().float().cpu() for k, v in out["attentions"]["all-fused"]["temporal_attns"].items()}
    return flat, att, n


@pytest.mark.parametrize("sites", ["default", "every-site-one-pass"])
def test_cached_rollout_matches_reference_golden(sites, switch):
    r = _reference()
    c, z = r["c"], r["z"]
    tol = TOL
    if sites != "default":
        switch.set_one_pass_sites("linear,conv1d")
        switch.set_one_pass_min_dim(0)
        tol = TOL_ALL_ONE_PASS
    switch.set_kv_cache_fp16x2(True)
    flat, att, n = _forward(_model())
    T, B, H, layers, n_out = c["T"], c["B"], c["fp_heads"], c["fp_layers"], c["fp_output_len"]
    assert n.cbc == 0 and n.composite == [(T, T)] * layers + [(1, T + 1)] * layers + [(1, T + 2)] * layers      # the path under test ran
    worst, checked = 0.0, 0
    for k in z.files:
        if not k.startswith("out:"):
            continue
        ref = torch.from_numpy(z[k])
        got = flat[k[4:]]
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        e = rel_l2(got, ref)
        worst = max(worst, e)
        assert e < tol, (k, e)
        checked += 1
    assert checked >= 6
    assert sorted(att) == [f"gpt2_att_{i}" for i in range(n_out)]
    for i in range(n_out):
        got, ref = att[f"gpt2_att_{i}"], r["att"][f"gpt2_att_{i}"]
        assert got.shape == ref.shape == ((B, layers, H, T, T) if i == 0 else (B, layers, H, 1, T + i))
        e = rel_l2(got, ref)
        worst = max(worst, e)
        assert e < tol, (i, e)
    print(f"[{NAME}/fp16x2/cached/{sites}] worst output / attention error {worst:.2e}")


def _predictor(D, H, layers, seed):
    from afft_amd.models.future_prediction import BaseFuturePredictor
    torch.manual_seed(seed)
    return BaseFuturePredictor(D, inter_dim=D, n_layer=layers, n_head=H, embd_pdrop=0.0, resid_pdrop=0.0, attn_pdrop=0.0,
                               output_attentions=True).eval()


@pytest.mark.parametrize("n_out", [2, 4])
def test_switch_on_against_switch_off(n_out, switch):
    """two results that are each within 1e-3 of exact: relative L2 below 2e-3 (not bit equality: the step's attention is fp32 arithmetic on
    joined planes, the recompute's is the plane attention)"""
    import afft_amd
    afft_amd.set_precision("fp16x2")
    layers = 2
    pred = _predictor(64, 2, layers, seed=3).cuda()
    feats = torch.randn(3, 5, 64, generator=torch.Generator().manual_seed(4)).cuda()
    runs = {}
    for on in (True, False):
        switch.set_kv_cache_fp16x2(on)
        with torch.no_grad(), _count() as n:
            out, att = pred(feats, n_out)
        torch.cuda.synchronize()
        assert n.cbc == 0 and len(n.composite) == (layers * n_out if on else 0)
        runs[on] = (out.float().cpu(), {k: v.float().cpu() for k, v in att.items()})
    assert runs[True][0].shape == runs[False][0].shape == (3, 5 + n_out - 1, 64)
    e = rel_l2(runs[True][0], runs[False][0])
    e_att = max(rel_l2(runs[True][1][k], runs[False][1][k]) for k in runs[False][1])
    print(f"[fp16x2 switch on vs off, output_len {n_out}] outputs {e:.2e}  attention maps {e_att:.2e}")
    assert e < 2e-3 and e_att < 2e-3
    for k, v in runs[False][1].items():
        assert runs[True][1][k].shape == v.shape


def test_output_len_1_is_untouched_bitwise(switch):
    import afft_amd
    afft_amd.set_precision("fp16x2")
    pred = _predictor(64, 2, 2, seed=3).cuda()
    feats = torch.randn(3, 5, 64, generator=torch.Generator().manual_seed(4)).cuda()
    runs = {}
    for on in (True, False):
        switch.set_kv_cache_fp16x2(on)
        with torch.no_grad(), _count() as n:
            out, att = pred(feats, 1)
        assert n.cbc == 0 and n.composite == []
        runs[on] = (out.cpu(), att["gpt2_att_0"].cpu())
    assert torch.equal(runs[True][0], runs[False][0]) and torch.equal(runs[True][1], runs[False][1])


def _traced_rollout(switch, pred, x, n_out, sites):
    """fp16x2 with the switch on: (output, split3 of every GEMM launch over M = B rows -- the one-row steps')"""
    import afft_amd
    from afft_amd import _lib
    B, layers = x.shape[0], len(pred.gpt_model.h)
    if sites is not None:
        switch.set_one_pass_sites(sites)
    switch.set_kv_cache_fp16x2(True)
    afft_amd.set_precision("fp16x2")
    _lib.check(_lib.lib().afft_gemm_trace_begin(1024))
    with torch.no_grad(), _count() as n:
        out, _ = pred(x, n_out)
    torch.cuda.synchronize()
    buf = (_lib.GemmTraceRec * 1024)()
    nrec = _lib.lib().afft_gemm_trace_end(buf, 1024)
    assert len(n.composite) == layers * n_out and n.cbc == 0
    return out.float().cpu(), [buf[i].split3 for i in range(nrec) if buf[i].M == B]


def test_full_width_against_fp32(switch):
    """inter_dim = 2048, 4 heads, 2 layers, B = 8, T = 16, output_len = 4, random weights: fp16x2 over the cache against the same model in the
    fp32 precision, within the bars of tests/test_model_gpu.py test_fp16x2_forward_full_size (9e-4 with the default one-pass sites, 8e-4
    with every site on two passes); every predictor GEMM of the one-row steps runs one fp16 pass by default (4 x layers x 3 launches),
    none with the sites off, and the error with the sites off is not larger"""
    import afft_amd
    D, H, layers, B, T, n_out = 2048, 4, 2, 8, 16, 4
    pred = _predictor(D, H, layers, seed=5).cuda()
    x = torch.randn(B, T, D, generator=torch.Generator().manual_seed(6)).cuda()
    try:
        afft_amd.set_precision("fp32")
        with torch.no_grad():
            ref, _ = pred(x, n_out)
        ref = ref.float().cpu()
        assert ref.shape == (B, T + n_out - 1, D)
        out, one_row = _traced_rollout(switch, pred, x, n_out, None)
        e_default = rel_l2(out, ref)
        assert len(one_row) == 4 * layers * (n_out - 1) and all(s == 4 for s in one_row), one_row
        out2, one_row2 = _traced_rollout(switch, pred, x, n_out, "")
        e_two = rel_l2(out2, ref)
        print(f"[full width/fp16x2/cached] vs fp32: default sites {e_default:.2e}, every site two passes {e_two:.2e}")
        assert len(one_row2) == 4 * layers * (n_out - 1) and all(s == 2 for s in one_row2), one_row2
        assert e_default < 9e-4 and e_two < 8e-4 and e_two <= e_default
    finally:
        del pred
        torch.cuda.empty_cache()


def test_collect_logits_in_fp16x2_with_and_without_the_switch(switch):
    """evaluate.collect_logits(..., precision='fp16x2') on a two-batch loader with fp_output_len = 2: the same logits within 2e-3 with the
    switch on and off (each within 1e-3 of exact), and the training precision is back afterwards"""
    import afft_amd
    from afft_amd import evaluate as E
    r = _reference()
    model = _model(fp_output_len=2, precision="bf16")
    dev = torch.device("cuda:0")
    loader = [({"data_dict": {m: d[i:i + 1] for m, d in r["data"].items()}}, {}) for i in range(r["c"]["B"])]
    assert len(loader) == 2
    got = {}
    for on in (False, True):
        switch.set_kv_cache_fp16x2(on)
        with _count() as n:
            key, lg = E.collect_logits(model, loader, dev, precision="fp16x2")
        torch.cuda.synchronize()
        assert afft_amd.runtime.precision() == "bf16"
        assert n.cbc == 0 and len(n.composite) == (len(loader) * r["c"]["fp_layers"] * 2 if on else 0)
        got[on] = lg.float().cpu()
    assert key == "logits/action_all-fused" and got[True].shape == (2, r["c"]["num_classes"])
    e = rel_l2(got[True], got[False])
    print(f"[collect_logits/fp16x2] switch on vs off {e:.2e}")
    assert e < 2e-3
