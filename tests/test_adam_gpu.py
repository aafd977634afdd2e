"""GPU: the Adam / AdamW kernels (afft_adam, afft_adam_runs) against a float64 restatement, and afft_amd.optim.AdamW in the reference's
loop against torch.optim.AdamW through the gradient sink, in every forward precision, plus the non-finite-step skip and two ranks."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import case_tensors, rel_l2  # noqa: E402
from test_adam_cpu import LR_WD, comparable  # noqa: E402
from test_model_gpu import _reference_loop, build  # noqa: E402

B1, B2, EPS = 0.9, 0.999, 1e-8
B1F, B2F = (float(torch.tensor(b, dtype=torch.float32)) for b in (B1, B2))     # the fp32 betas the kernel receives


def _restate(p, g, m, v, lr, wd, gscale, t_prev, decoupled):
    """afft_adam in float64 from the kernel's inputs: its fp32 betas (1 - beta is taken of those, as in torch's fused kernels)
    and its fp32 product gscale * g"""
    g = g.float() * torch.tensor(gscale, dtype=torch.float32)      # the kernel's first rounding: g' = fp32(gscale * g)
    p, g, m, v = (x.double() for x in (p, g, m, v))
    t = t_prev + 1.0
    if decoupled:
        p = p * (1.0 - lr * wd)
    else:
        g = g + wd * p
    g_terms = g.abs() + (0.0 if decoupled else (wd * p).abs())      # the size of g + wd p before it cancels (Adam)
    m_terms = (B1F * m).abs() + (1 - B1F) * g_terms
    v_terms = B2F * v + (1 - B2F) * g_terms * g_terms
    m = B1F * m + (1 - B1F) * g
    v = B2F * v + (1 - B2F) * g * g
    p = p - (lr / (1 - B1F ** t)) * m / (v.sqrt() / math.sqrt(1 - B2F ** t) + EPS)
    return p, m, v, m_terms, v_terms


def _e4m3_of(p):
    """the e4m3 image of p by the rounding rule itself (tests/sgd_double.py): (256 p) clamped to +-448, rounded once; no kernel"""
    from sgd_double import e4m3_image
    return e4m3_image(p)


@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("decoupled", [False, True])
def test_adam_kernel_matches_float64(gdtype, decoupled):
    from afft_amd import ops
    dev = torch.device("cuda:0")
    n, lr, wd, gscale = 1_000_003, 1e-3, 1e-2, 0.5          # n % 4 != 0: the tail runs
    gen = torch.Generator(device=dev).manual_seed(3)
    p = 0.05 * torch.randn(n, device=dev, generator=gen)
    m = torch.zeros(n, device=dev)
    v = torch.zeros(n, device=dev)
    p16 = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    h16 = torch.zeros(n, dtype=torch.float16, device=dev)
    p8 = torch.zeros(n, dtype=torch.uint8, device=dev)
    step = torch.zeros((), device=dev)
    ok = torch.ones((), device=dev)
    coef = torch.tensor([0.8], device=dev)
    for k in range(3):
        g = (torch.randn(n, device=dev, generator=gen) * (1.0 + k)).to(gdtype)
        p0, m0, v0 = p.clone(), m.clone(), v.clone()
        ops.adam(p, g, m, v, lr, B1, B2, EPS, wd, gscale, step, decoupled, p_bf16=p16, gscale_dev=coef, p_f16=h16, p_f8=p8, ok=ok)
        step.add_(ok)
        torch.cuda.synchronize()
        gs = float(torch.tensor(gscale, dtype=torch.float32) * coef.cpu()[0])     # the kernel's gscale * *gscale_dev, in fp32
        rp, rm, rv, m_terms, v_terms = _restate(p0, g.float(), m0, v0, lr, wd, gs, float(k), decoupled)
        a = p.abs()
        ulp = (torch.nextafter(a, torch.full_like(a, math.inf)) - a).double()
        assert bool(((p.double() - rp).abs() <= ulp + 1e-5 * lr).all()), float((p.double() - rp).abs().max())
        assert bool(((m.double() - rm).abs() <= 1e-6 * m_terms + 1e-30).all()), float(((m.double() - rm).abs() / (m_terms + 1e-30)).max())
        assert bool(((v.double() - rv).abs() <= 1e-6 * v_terms + 1e-30).all()), float(((v.double() - rv).abs() / (v_terms + 1e-30)).max())
        assert torch.equal(p16, p.bfloat16()) and torch.equal(h16, p.half())
        assert torch.equal(p8, _e4m3_of(p))
    assert float(step) == 3.0


def test_adam_runs_kernel_equals_flat_kernel_bitwise_and_ok_zero_writes_nothing():
    from afft_amd import ops
    dev = torch.device("cuda:0")
    n = 1_000_003
    gen = torch.Generator(device=dev).manual_seed(5)
    base = [0.05 * torch.randn(n, device=dev, generator=gen), 0.01 * torch.randn(n, device=dev, generator=gen),
            1e-4 * torch.rand(n, device=dev, generator=gen)]
    g = torch.randn(n, device=dev, generator=gen)
    step = torch.full((), 4.0, device=dev)
    starts = list(range(0, n, 16384))
    runs = torch.tensor([(s, min(16384, n - s)) for s in starts], dtype=torch.int64, device=dev)
    outs = []
    for kind in ("flat", "runs"):
        p, m, v = (t.clone() for t in base)
        imgs = (torch.zeros(n, dtype=torch.bfloat16, device=dev), torch.zeros(n, dtype=torch.float16, device=dev),
                torch.zeros(n, dtype=torch.uint8, device=dev))
        for decoupled in (True, False):
            if kind == "flat":
                ops.adam(p, g, m, v, 2e-3, B1, B2, EPS, 0.05, 0.7, step, decoupled, p_bf16=imgs[0], p_f16=imgs[1], p_f8=imgs[2])
            else:
                ops.adam_runs(p, g, m, v, runs, 2e-3, B1, B2, EPS, 0.05, 0.7, step, decoupled, p_bf16=imgs[0], p_f16=imgs[1], p_f8=imgs[2])
        outs.append((p, m, v) + imgs)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # ok = 0: neither kernel writes anything, and the host's step_t.add_(ok) leaves the counter
    ok = torch.zeros((), device=dev)
    state = outs[0]
    snap = [t.clone() for t in state] + [step.clone()]
    p, m, v, b16, f16, e8 = state
    ops.adam(p, g, m, v, 1e-3, B1, B2, EPS, 0.01, 1.0, step, True, p_bf16=b16, p_f16=f16, p_f8=e8, ok=ok)
    ops.adam_runs(p, g, m, v, runs, 1e-3, B1, B2, EPS, 0.01, 1.0, step, True, p_bf16=b16, p_f16=f16, p_f8=e8, ok=ok)
    step.add_(ok)
    torch.cuda.synchronize()
    for a, b in zip(snap, list(state) + [step]):
        assert torch.equal(a, b)


def _feeds(c, data, tgt, sub, dev):
    return {m: d.to(dev) for m, d in data.items()}, tgt.to(dev), sub.to(dev)


def _model(c, state, precision, dev):
    model = build(c, precision)
    model.load_state_dict(state)
    return model.to(dev).eval()


def _eval_logits(model, feats, tgt, sub):
    with torch.no_grad():
        outs, _ = model(feats, mixup_fn=None, target={"action": tgt}, target_subclips={"action": sub}, target_subclips_ignore_index=None)
    return outs["logits/action"]["all-fused"].float().clone()


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16x2"])
@pytest.mark.parametrize("in_backward", [True, False])
def test_adamw_in_the_reference_loop_matches_torch_adamw(precision, in_backward):
    """afft AdamW vs torch.optim.AdamW over the same per-parameter groups (two lr / wd classes), both through the gradient sink:
    after step 1 the gradients are the same bits and the parameters agree to 1e-6; after 5 steps to 1e-6 (fp32) / 3e-4 (16-bit
    modes), the noise-only key bias aside (test_adam_cpu.comparable).  Then the images the optimizer kept are fresh: a forward on
    them equals one after every image is re-derived from the fp32 masters, bit for bit."""
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.common.scheduler import prepare_params
    from afft_amd.optim import AdamW
    c, state, data, tgt, sub = case_tensors("t0_sa")
    dev = torch.device("cuda:0")
    feats, tgt, sub = _feeds(c, data, tgt, sub, dev)
    try:
        ma, mt = _model(c, state, precision, dev), _model(c, state, precision, dev)
        ga, gt = prepare_params(ma, LR_WD, 1e-3, 1e-2), prepare_params(mt, LR_WD, 1e-3, 1e-2)
        opt = AdamW(ga, lr=1e-3, bucket_elems=1 << 15, in_backward=in_backward)
        assert opt.in_backward == in_backward and not opt._can_fuse()
        ref = torch.optim.AdamW(gt, lr=1e-3)
        names = [n for n, _ in ma.named_parameters()]
        for k in range(5):
            _reference_loop(ma, opt, None, feats, tgt, sub, 1)
            _reference_loop(mt, ref, None, feats, tgt, sub, 1)
            torch.cuda.synchronize()
            if k == 0:
                for n, p, q in zip(names, ma.parameters(), mt.parameters()):
                    assert torch.equal(p.grad, q.grad), n
                a = torch.cat([p.detach().reshape(-1) for p in ma.parameters()])
                b = torch.cat([q.detach().reshape(-1) for q in mt.parameters()])
                assert rel_l2(a, b) < 1e-6, rel_l2(a, b)
        a = torch.cat([comparable(n, p) for n, p in ma.named_parameters()])
        b = torch.cat([comparable(n, q) for n, q in mt.named_parameters()])
        # 16-bit modes: an image that rounds the other way changes a gradient, and Adam's normalised step carries it on (measured
        # 1.0e-4 .. 1.25e-4 after 5 steps on this case)
        tol = 1e-6 if precision == "fp32" else 3e-4
        assert rel_l2(a, b) < tol, rel_l2(a, b)
        assert float(opt.state_dict()["state"][0]["step"]) == 5.0
        before = _eval_logits(ma, feats, tgt, sub)
        rt.invalidate_weight_images(include_external=True)
        opt.flat.refresh_images()
        after = _eval_logits(ma, feats, tgt, sub)
        assert torch.equal(before, after)
    finally:
        afft_amd.set_precision("bf16")


@pytest.mark.parametrize("precision", ["bf16", "fp16x2"])
def test_a_non_finite_loss_step_leaves_adam_state_untouched(precision):
    import afft_amd
    from afft_amd.common.scheduler import prepare_params
    from afft_amd.optim import AdamW
    c, state, data, tgt, sub = case_tensors("t0_sa")
    dev = torch.device("cuda:0")
    feats, tgt, sub = _feeds(c, data, tgt, sub, dev)
    bad = {m: f.clone() for m, f in feats.items()}
    next(iter(bad.values()))[0, 0, 0] = float("nan")
    try:
        model = _model(c, state, precision, dev)
        opt = AdamW(prepare_params(model, LR_WD, 1e-3, 1e-2), lr=1e-3, bucket_elems=1 << 15)
        _reference_loop(model, opt, None, feats, tgt, sub, 2)
        torch.cuda.synchronize()
        f = opt.flat
        snap = lambda: [t.clone() for t in (f.flat_p, opt.opt.exp_avg, opt.opt.exp_avg_sq, f.flat_p16, f.flat_h16, f.flat_p8, f.flat_pk16)  # noqa: E731
                        if t is not None]
        before = snap()
        step0 = float(opt.state_dict()["state"][0]["step"])
        loss = _reference_loop(model, opt, None, bad, tgt, sub, 1, async_metrics=None)      # lazy metrics: the NaN error comes later
        torch.cuda.synchronize()
        assert float(loss) != float(loss) and float(opt.opt.ok) == 0.0
        for a, b in zip(before, snap()):
            assert torch.equal(a, b)
        assert float(opt.state_dict()["state"][0]["step"]) == step0 == 2.0
        loss = _reference_loop(model, opt, None, feats, tgt, sub, 1)
        torch.cuda.synchronize()
        assert float(loss) == float(loss) and float(opt.opt.ok) == 1.0
        assert not torch.equal(before[0], f.flat_p) and bool(torch.isfinite(f.flat_p).all())
        assert float(opt.state_dict()["state"][0]["step"]) == 3.0
    finally:
        afft_amd.set_precision("bf16")


def _run_two_rank(tmp_path, precision, algo, steps=3):
    """tests/scripts/two_rank_adam_gpu.py: two gloo ranks on cuda:0 (algo 'allreduce' | 'sharded') or one process (algo 'none')"""
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "tests", "scripts", "two_rank_adam_gpu.py")
    out = str(tmp_path / f"adam_{precision}_{algo}.pt")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "LOCAL_WORLD_SIZE", "GROUP_RANK"):
        env.pop(k, None)
    tail = [script, precision, algo, str(steps), out]
    if algo == "none":
        cmd = [sys.executable] + tail
    else:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", str(port)] + tail
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(out)


def test_two_ranks_on_one_gpu_adamw(tmp_path):
    """two gloo ranks on cuda:0 with afft AdamW in the reference's loop: replicas bitwise equal; 'allreduce' and 'sharded' bitwise equal
    (parameters, both moments, bf16 images); both equal one process on the whole batch to 1e-6 in fp32 (the noise-only key bias aside)"""
    one = _run_two_rank(tmp_path, "fp32", "none")
    runs = {a: _run_two_rank(tmp_path, "fp32", a) for a in ("allreduce", "sharded")}
    for a, r in runs.items():
        assert r["info"]["replicas_bitwise_equal"], a
        assert r["info"]["step"] == 3.0
        ref = torch.cat([comparable(k, one["params"][k]) for k in sorted(one["params"])])
        got = torch.cat([comparable(k, r["params"][k]) for k in sorted(one["params"])])
        assert rel_l2(got, ref) < 1e-6, (a, rel_l2(got, ref))
    a, b = runs["allreduce"], runs["sharded"]
    assert b["info"]["stale_before_sync"] and not b["info"]["stale_after_sync"]
    for grp in ("params", "exp_avg", "exp_avg_sq", "images"):
        assert a[grp].keys() == b[grp].keys()
        for k in a[grp]:
            assert torch.equal(a[grp][k], b[grp][k]), (grp, k)
