"""Worker of tests/test_adam_gpu.py::test_two_ranks_on_one_gpu_adamw: one data-parallel rank of afft_amd.optim.AdamW in the reference's
loop (Runner -> zero_grad -> backward -> step) on the HIP path, or -- world size 1 -- the single process on the whole batch.

    python -m torch.distributed.run --nproc-per-node 2 ... two_rank_adam_gpu.py <precision> <comm_algo> <steps> <out.pt>
    python two_rank_adam_gpu.py <precision> none <steps> <out.pt>

Both ranks sit on cuda:0 and exchange through gloo.  Rank 1 starts from perturbed weights (the construction-time broadcast must
overwrite them).  After the steps every rank calls sync_masters(); rank 0 saves parameters, both moments and bf16 images by name,
after checking that rank 1 holds the same bits."""
import os
import sys
from datetime import timedelta

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.join(TESTS, "golden"), os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)

WTS = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
LR_WD = [[["future_predictor.future_predictor"], 3e-3, 0.0]]


def batch(c, B=4):
    """labels without ignored frames: the mean losses of two half-batches then average to the full-batch mean"""
    g = torch.Generator().manual_seed(7)
    data = {m: torch.randn(B, c["T"], C, 1, 1, 1, generator=g) for m, C in c["modal_dims"].items()}
    tgt = torch.randint(0, c["num_classes"], (B,), generator=g)
    sub = torch.randint(0, c["num_classes"], (B, c["T"], 1), generator=g)
    return data, tgt, sub


def main():
    precision, algo, steps, out = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if world > 1:
        dist.init_process_group("gloo", timeout=timedelta(seconds=120))
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.common.runner import Runner
    from afft_amd.common.scheduler import prepare_params
    from afft_amd.config import make_model_cfg
    from afft_amd.models.base_model import BaseModel
    from afft_amd.optim import AdamW
    from helpers import case_tensors
    afft_amd.set_precision(precision)
    rt.set_grad_mode("sink")
    c, state, _, _, _ = case_tensors("t0_sa")
    cfg = make_model_cfg(c["modal_dims"], c["d"], c["D"], fuser=c["fuser"], depth=c["depth"], num_heads=c["num_heads"],
                         fp_layers=c["fp_layers"], fp_heads=c["fp_heads"], T=c["T"], drop=0.0)
    model = BaseModel(cfg, num_classes={"action": c["num_classes"]}, class_mappings={})
    model.load_state_dict(state)
    model = model.to(dev).eval()
    if rank == 1:
        with torch.no_grad():
            for p in model.parameters():
                p.add_(0.05)
    opt = AdamW(prepare_params(model, LR_WD, 1e-3, 1e-2), lr=1e-3, bucket_elems=8192,
                comm_algo=("allreduce" if algo == "none" else algo))
    data, tgt, sub = batch(c)
    h = tgt.shape[0] // world
    sl = slice(rank * h, (rank + 1) * h)
    mine = ({"data_dict": {m: d[sl].to(dev) for m, d in data.items()}, "target": {"action": tgt[sl].to(dev)},
             "target_subclips": {"action": sub[sl].to(dev)}}, {})
    runner = Runner(model, dev, WTS, compute_metrics=False)
    for _ in range(steps):
        loss, _ = runner(mine, None, True)
        opt.zero_grad()
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    info = {"stale_before_sync": bool(opt.reducer.masters_stale)}
    opt.sync_masters()         # every rank: masters and both moments of the other rank's slices
    info["stale_after_sync"] = bool(opt.reducer.masters_stale)
    info["step"] = float(opt.state_dict()["state"][0]["step"])
    torch.cuda.synchronize()
    ix = opt.flat.index_of()
    named = list(model.named_parameters())
    off = {k: opt.flat.offsets[ix[id(p)]] for k, p in named}
    res = {"params": {k: p.detach().float().cpu().clone() for k, p in named},
           "exp_avg": {k: opt.opt.exp_avg[off[k]:off[k] + p.numel()].cpu().clone() for k, p in named},
           "exp_avg_sq": {k: opt.opt.exp_avg_sq[off[k]:off[k] + p.numel()].cpu().clone() for k, p in named},
           "images": {k: opt.flat.flat_p16[off[k]:off[k] + p.numel()].cpu().clone() for k, p in named if opt.flat.owns_image(p)},
           "info": info}
    if world > 1:
        both = [None] * world
        dist.all_gather_object(both, res)
        if rank == 0:
            a, b = both[0], both[1]
            res["info"]["replicas_bitwise_equal"] = all(torch.equal(a[g][k], b[g][k]) for g in ("params", "exp_avg", "exp_avg_sq", "images")
                                                        for k in a[g])
    if rank == 0:
        torch.save(res, out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
