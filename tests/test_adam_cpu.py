"""Host logic of afft_amd.optim.Adam / AdamW in the build container: the kernels are replaced by torch test doubles (tests/cpu_ops.py,
and the Adam double below), everything else is the product code.

  * the reference's loop shape (train.py:228-265) with afft AdamW, Adam and Adam(decoupled_weight_decay=True) == torch's class over
    the same per-parameter groups (two lr / weight-decay classes, Warmup(CosineLR)), to rounding; clipping by the loop and by grad_clip=;
  * state_dict interchange with torch.optim.AdamW in both directions;
  * world size 2 over gloo with parallel.DistributedDataParallel == one process on the full batch; 'sharded' == 'allreduce';
  * the options the kernels do not have raise.
"""
import contextlib
import copy
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_optim_cpu import _groups, _loop
from test_parallel_cpu import _afft_case, _afft_model

LR_WD = [[["future_predictor.future_predictor"], 3e-3, 0.0]]     # a second (lr, weight_decay) class beside the default one


@torch.no_grad()
def adam_double(p, g, m, v, lr, beta1, beta2, eps, wd, gscale, step, decoupled, p_bf16=None, gscale_dev=None, p_f16=None, p_f8=None,
                ok=None):
    """torch restatement of afft_adam (include/afft_hip.h)"""
    if ok is not None and float(ok) == 0.0:
        return
    if gscale_dev is not None:
        gscale = gscale * float(gscale_dev)
    t = float(step) + 1.0
    gg = g.float() * gscale
    if decoupled:
        p.mul_(1.0 - lr * wd)
    else:
        gg = gg + wd * p
    m.mul_(beta1).add_((1.0 - beta1) * gg)
    v.mul_(beta2).add_((1.0 - beta2) * gg * gg)
    denom = v.sqrt() / math.sqrt(1.0 - beta2 ** t) + eps
    p.sub_((lr / (1.0 - beta1 ** t)) * m / denom)
    for img in (p_bf16, p_f16):
        if img is not None:
            img.copy_(p)


@torch.no_grad()
def adam_runs_double(p, g, m, v, runs, lr, beta1, beta2, eps, wd, gscale, step, decoupled, p_bf16=None, p_f16=None, p_f8=None, ok=None):
    if ok is not None and float(ok) == 0.0:
        return
    for a, n in runs.tolist():
        adam_double(p[a:a + n], g[a:a + n], m[a:a + n], v[a:a + n], lr, beta1, beta2, eps, wd, gscale, step, decoupled,
                    p_bf16=None if p_bf16 is None else p_bf16[a:a + n], p_f16=None if p_f16 is None else p_f16[a:a + n])


@contextlib.contextmanager
def doubles():
    """cpu_ops.installed() plus the Adam doubles"""
    import cpu_ops
    from afft_amd import ops
    saved = ops.adam, ops.adam_runs
    with cpu_ops.installed():
        ops.adam, ops.adam_runs = adam_double, adam_runs_double
        try:
            yield
        finally:
            ops.adam, ops.adam_runs = saved


def comparable(name, t):
    """`t` without what Adam makes of pure rounding noise: the key third of a fused q / k / v bias (GPT-2 c_attn.bias) has a gradient
    that is zero in exact arithmetic (softmax is invariant to a constant added to every score of a query), so the computed one is
    rounding residue, and Adam turns any residue into a full +-lr step.  Two implementations that round one step apart move it
    apart by lr; everything else stays within rounding."""
    t = t.detach().reshape(-1)
    if name.endswith("c_attn.bias"):
        d = t.numel() // 3
        t = torch.cat([t[:d], t[2 * d:]])
    return t


def _flat(model):
    return torch.cat([comparable(n, p) for n, p in model.named_parameters()])


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-12))


def _sched(opt):
    from afft_amd.common.scheduler import CosineLR, Warmup
    return Warmup(opt, CosineLR(opt, num_epochs=3, iters_per_epoch=2, world_size=1, eta_min=1e-6), init_lr_ratio=0.1, num_epochs=1,
                  iters_per_epoch=2, world_size=1)


def _make(kind, groups, **kw):
    from afft_amd import optim
    if kind == "AdamW":
        return optim.AdamW(groups, lr=1e-3, weight_decay=1e-2, **kw), torch.optim.AdamW
    if kind == "Adam":
        return optim.Adam(groups, lr=1e-3, weight_decay=1e-2, **kw), torch.optim.Adam
    return optim.Adam(groups, lr=1e-3, weight_decay=1e-2, decoupled_weight_decay=True, **kw), \
        (lambda g, **k: torch.optim.Adam(g, decoupled_weight_decay=True, **k))


@pytest.mark.parametrize("kind,in_backward,clip", [("AdamW", True, None), ("Adam", False, None), ("Adam_decoupled", True, None),
                                                   ("AdamW", False, "loop"), ("AdamW", False, "grad_clip")])
def test_reference_loop_matches_torch(kind, in_backward, clip):
    """the reference's loop with afft Adam / AdamW == torch's class over the same per-parameter groups (two lr / wd classes, a
    Warmup(CosineLR) scheduler), to rounding; the Adam state is published the way torch's is"""
    c, state, data, tgt, sub = _afft_case()
    CLIP = 0.05
    with doubles():
        m1, m2 = _afft_model(c, state, "fp32"), _afft_model(c, state, "fp32")
        g1, g2 = _groups(m1, lr=1e-3, wd=1e-2, lr_wd=LR_WD), _groups(m2, lr=1e-3, wd=1e-2, lr_wd=LR_WD)
        assert len({(g["lr"], g["weight_decay"]) for g in g1}) == 2
        opt, torch_cls = _make(kind, g1, bucket_elems=8192, in_backward=in_backward,
                               grad_clip=CLIP if clip == "grad_clip" else None)
        ref = torch_cls(g2, lr=1e-3, weight_decay=1e-2)
        norms1, norms2 = [], []
        _loop(m1, opt, _sched(opt), data, tgt, sub, 4, clip=CLIP if clip == "loop" else None, norms=norms1)
        _loop(m2, ref, _sched(ref), data, tgt, sub, 4, clip=CLIP if clip else None, norms=norms2)
        assert opt.opt.hyper is not None and isinstance(opt.opt.step_t, torch.Tensor) and float(opt.opt.step_t) == 4.0
        assert opt.opt.decoupled == (kind != "Adam")
        for (n, p), q in zip(m1.named_parameters(), m2.parameters()):
            assert _rel(comparable(n, p), comparable(n, q)) < 1e-6, n
        assert _rel(_flat(m1), _flat(m2)) < 1e-6
        if clip:
            assert all(x > 2 * CLIP for x in norms2), norms2        # the clip really bit
        if clip == "grad_clip":
            assert abs(float(opt.opt.last_grad_norm) - norms2[-1]) < 1e-5 * norms2[-1]
        sd = opt.state_dict()
        for (n, p), q in zip(m1.named_parameters(), m2.parameters()):
            for k in ("exp_avg", "exp_avg_sq"):
                assert _rel(comparable(n, opt.state[p][k]), comparable(n, ref.state[q][k])) < 1e-5, (n, k)
        st = next(iter(sd["state"].values()))
        assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and float(st["step"]) == 4.0


@pytest.mark.parametrize("direction", ["afft_to_torch", "torch_to_afft"])
def test_state_dict_interchange_with_torch(direction):
    """a checkpoint of one side loads into the other; both then continue 3 steps and stay equal"""
    from afft_amd.optim import AdamW
    c, state, data, tgt, sub = _afft_case()
    with doubles():
        m1 = _afft_model(c, state, "fp32")
        g1 = _groups(m1, lr=1e-3, wd=1e-2, lr_wd=LR_WD)
        o1 = AdamW(g1, lr=1e-3, bucket_elems=8192) if direction == "afft_to_torch" else torch.optim.AdamW(g1, lr=1e-3)
        _loop(m1, o1, None, data, tgt, sub, 2)
        sd_model = {k: v.clone() for k, v in m1.state_dict().items()}
        sd_opt = copy.deepcopy(o1.state_dict())         # state_dict() hands out references, as torch's does (torch.save copies)
        m2 = _afft_model(c, state, "fp32")
        m2.load_state_dict(sd_model)
        g2 = _groups(m2, lr=1e-3, wd=1e-2, lr_wd=LR_WD)
        o2 = torch.optim.AdamW(g2, lr=1e-3) if direction == "afft_to_torch" else AdamW(g2, lr=1e-3, bucket_elems=8192)
        o2.load_state_dict(sd_opt)
        afft = o1 if direction == "afft_to_torch" else o2
        assert float(afft.opt.step_t) == 2.0 and afft.opt.steps == 2
        _loop(m1, o1, None, data, tgt, sub, 3)
        _loop(m2, o2, None, data, tgt, sub, 3)
        assert _rel(_flat(m2), _flat(m1)) < 1e-6
        for p, q in zip(m1.parameters(), m2.parameters()):
            assert float(o1.state[p]["step"]) == float(o2.state[q]["step"]) == 5.0


def test_load_state_dict_refuses_sgd_and_unequal_steps():
    from afft_amd.optim import SGD, AdamW
    c, state, data, tgt, sub = _afft_case()
    with doubles():
        m = _afft_model(c, state, "fp32")
        sgd = SGD(_groups(m), lr=1e-2, momentum=0.9, nesterov=True, bucket_elems=8192)
        _loop(m, sgd, None, data, tgt, sub, 1)
        sd_sgd = copy.deepcopy(sgd.state_dict())
        m2 = _afft_model(c, state, "fp32")
        tw = torch.optim.AdamW(_groups(m2), lr=1e-3)
        _loop(m2, tw, None, data, tgt, sub, 1)
        sd_w = copy.deepcopy(tw.state_dict())
        m3 = _afft_model(c, state, "fp32")
        opt = AdamW(_groups(m3), lr=1e-3, bucket_elems=8192)
        with pytest.raises(ValueError, match="not an Adam"):
            opt.load_state_dict(sd_sgd)
        first = next(iter(sd_w["state"]))
        sd_w["state"][first]["step"] = torch.tensor(7.0)
        with pytest.raises(ValueError, match="different numbers of steps"):
            opt.load_state_dict(sd_w)


def test_unsupported_arguments_raise():
    from afft_amd.optim import Adam, AdamW
    c, state, _, _, _ = _afft_case()
    with doubles():
        m = _afft_model(c, state, "fp32")
        for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True), dict(lr=torch.tensor(1e-3))):
            with pytest.raises(NotImplementedError):
                AdamW(_groups(m), **kw)
        groups = _groups(m)
        groups[1]["betas"] = (0.8, 0.999)
        with pytest.raises(NotImplementedError, match="betas"):
            Adam(groups)
        groups = _groups(m)
        groups[2]["eps"] = 1e-6
        with pytest.raises(NotImplementedError, match="eps"):
            AdamW(groups)
        with pytest.raises(TypeError):
            AdamW(_groups(m), decoupled_weight_decay=False)
        # torch's defaults
        a, w = Adam(_groups(m)), AdamW(_groups(m))
        assert a.defaults["weight_decay"] == 0.0 and w.defaults["weight_decay"] == 1e-2
        assert a.defaults["betas"] == w.defaults["betas"] == (0.9, 0.999) and a.defaults["eps"] == 1e-8 and a.defaults["lr"] == 1e-3
        assert not a.opt.decoupled and w.opt.decoupled and a.opt.runs is None
        assert not a._can_fuse() and not w._can_fuse()


# ----------------------------------------------------------------------------- world size 2 over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ddp_worker(rank, world, port, out, algo):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.join(here, "golden"), os.path.dirname(here)):
        if p not in sys.path:
            sys.path.insert(0, p)
    from afft_amd.optim import AdamW
    from afft_amd.parallel import DistributedDataParallel
    c, state, data, tgt, sub = _afft_case()
    with doubles():
        model = _afft_model(c, state, "fp32")
        if rank == 1:        # the construction-time broadcast must overwrite these
            with torch.no_grad():
                for p in model.parameters():
                    p.add_(0.05)
        opt = AdamW(_groups(model, lr=1e-3, wd=1e-2, lr_wd=LR_WD), lr=1e-3, bucket_elems=8192, comm_algo=algo)
        ddp = DistributedDataParallel(model)
        assert ddp._own is None and ddp._engines == [opt]
        h = data[next(iter(data))].shape[0] // world
        _loop(ddp, opt, None, data, tgt, sub, 3, sl=slice(rank * h, (rank + 1) * h))
        info = {}
        if algo == "sharded":
            info["stale"] = bool(opt.reducer.masters_stale)
            assert isinstance(opt.reducer.opt_buf, tuple) and len(opt.reducer.opt_buf) == 2
            opt.sync_masters()       # every rank: both moments and the masters of the other rank's slices
        sd = opt.state_dict()
    named = list(model.named_parameters())
    ix = opt.flat.index_of()
    off = {k: opt.flat.offsets[ix[id(p)]] for k, p in named}
    res = {"params": {k: p.detach().clone() for k, p in named},
           "exp_avg": {k: opt.opt.exp_avg[off[k]:off[k] + p.numel()].clone() for k, p in named},
           "exp_avg_sq": {k: opt.opt.exp_avg_sq[off[k]:off[k] + p.numel()].clone() for k, p in named},
           "step": float(next(iter(sd["state"].values()))["step"]), "info": info}
    both = [None] * world
    dist.all_gather_object(both, res)
    if rank == 0:
        res["info"]["replicas_equal"] = all(torch.equal(both[0][g][k], both[1][g][k]) for g in ("params", "exp_avg", "exp_avg_sq")
                                            for k in both[0][g])
        torch.save(res, out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_with_ddp_wrapper_match_single_process_and_sharded_equals_allreduce(tmp_path):
    res = {}
    for algo in ("allreduce", "sharded"):
        out = str(tmp_path / f"adam_{algo}.pt")
        mp.spawn(_ddp_worker, args=(2, _free_port(), out, algo), nprocs=2, join=True)
        res[algo] = torch.load(out)
        assert res[algo]["info"]["replicas_equal"], algo
        assert res[algo]["step"] == 3.0
    assert res["sharded"]["info"]["stale"]
    a, b = res["allreduce"], res["sharded"]
    for grp in ("params", "exp_avg", "exp_avg_sq"):
        for k in a[grp]:
            assert torch.equal(a[grp][k], b[grp][k]), (grp, k)
    from afft_amd.optim import AdamW
    c, state, data, tgt, sub = _afft_case()
    with doubles():
        model = _afft_model(c, state, "fp32")
        opt = AdamW(_groups(model, lr=1e-3, wd=1e-2, lr_wd=LR_WD), lr=1e-3, bucket_elems=8192)
        _loop(model, opt, None, data, tgt, sub, 3)
    ref = _flat(model)
    got = torch.cat([comparable(k, a["params"][k]) for k, _ in model.named_parameters()])
    assert _rel(got, ref) < 1e-6
    import afft_amd
    afft_amd.set_precision("bf16")
