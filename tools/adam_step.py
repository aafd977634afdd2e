"""Cost of the Adam / AdamW update at cfg2 (about 614 M parameters), in one process, variants alternated round by round.

(a) the update alone over whole flat buffers: afft_adam (AdamW, bf16 image), afft_sgd_nesterov2 (bf16 image) and torch.optim.AdamW over
    the model's parameter shapes (fused=True where this build has it, otherwise foreach) -- ms, bytes moved, GB/s, fraction of the
    6.29 TB/s copy rate;
(b) the reference-loop step at B = 64, bf16 (Runner -> zero_grad -> backward -> step): afft SGD, afft SGD without the GEMM-epilogue
    fusion (runtime.set_fused_sgd(False), the AFFT_FUSED_SGD=0 shape), afft AdamW, torch.optim.AdamW through the gradient sink.

usage: python tools/adam_step.py [--rounds 5] [--out FILE]"""
import argparse
import gc
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as B  # noqa: E402
import afft_amd  # noqa: E402
from afft_amd import ops, runtime as rt  # noqa: E402
from afft_amd.common.runner import Runner  # noqa: E402
from afft_amd.common.scheduler import prepare_params  # noqa: E402
from afft_amd.optim import SGD, AdamW  # noqa: E402

COPY_TBS = 6.29
dev = torch.device("cuda:0")
WTS = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def torch_adamw(params, lr=1e-3):
    try:
        return torch.optim.AdamW(params, lr=lr, fused=True), "fused"
    except (RuntimeError, ValueError):
        return torch.optim.AdamW(params, lr=lr, foreach=True), "foreach"


def part_a(rounds):
    afft_amd.set_precision("bf16")
    model, _ = B.build_model("cfg2", dev)
    shapes = [p.shape for p in model.parameters() if p.requires_grad]
    del model
    torch.cuda.empty_cache()
    n = sum((s.numel() + 63) // 64 * 64 for s in shapes)
    g = torch.randn(n, device=dev) * 1e-3
    p = torch.randn(n, device=dev) * 0.02
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    p16 = torch.empty(n, dtype=torch.bfloat16, device=dev)
    step = torch.zeros((), device=dev)
    tp = [torch.nn.Parameter(torch.randn(s, device=dev) * 0.02) for s in shapes]
    for t in tp:
        t.grad = torch.randn_like(t) * 1e-3
    topt, tkind = torch_adamw(tp)
    variants = {
        "afft_adam (AdamW, bf16 image)": (lambda: ops.adam(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, step, True, p_bf16=p16), 30),
        "afft_sgd_nesterov2 (bf16 image)": (lambda: ops.sgd_nesterov(p, g, m, 1e-3, 0.9, 1e-6, 1.0, 0, p_bf16=p16), 22),
        f"torch.optim.AdamW ({tkind})": (topt.step, 28),
    }
    for f, _ in variants.values():      # warm up (torch: state allocation)
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    gc.collect()
    gc.freeze()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (f, _) in variants.items():
            ms[k].append(timed(f, 10))
    say(f"(a) update alone, {n / 1e6:.1f} M parameters (flat, 64-aligned), median of {rounds} alternated rounds of 10 launches")
    say(f"{'variant':36} {'ms':>8} {'B/param':>8} {'GB':>7} {'GB/s':>8} {'of 6.29 TB/s':>13}")
    gbs = {}
    for k, (_, bpp) in variants.items():
        t = statistics.median(ms[k])
        gb = n * bpp / 1e9
        gbs[k] = gb / t * 1e3
        say(f"{k:36} {t:8.3f} {bpp:8d} {gb:7.2f} {gbs[k]:8.0f} {gbs[k] / (COPY_TBS * 1e3):13.2f}")
    ka, ks = list(variants)[:2]
    say(f"afft AdamW / afft SGD effective bandwidth: {gbs[ka] / gbs[ks]:.2f}")
    say("(torch.optim.AdamW: 28 B/param counts its own update only; its GEMM images are re-cast on next use, +6 B/param)")
    gc.unfreeze()
    del p, g, m, v, p16, tp, topt
    torch.cuda.empty_cache()


def part_b(rounds, steps=10):
    afft_amd.set_precision("bf16")
    rt.set_grad_mode("sink")
    runs = {}
    for kind in ("afft SGD", "afft SGD, AFFT_FUSED_SGD=0", "afft AdamW", "torch.optim.AdamW (sink)"):
        model, c = B.build_model("cfg2", dev)
        model.train()
        feats, tgt, sub = B.make_inputs(c, 64, c["T"], 0, dev)
        batch = ({"data_dict": feats, "target": tgt, "target_subclips": sub}, {})
        groups = prepare_params(model, None, 1e-3, 1e-2 if "AdamW" in kind else 1e-6)
        if kind.startswith("afft SGD"):
            opt = SGD(groups, lr=1e-3, momentum=0.9, nesterov=True)
        elif kind == "afft AdamW":
            opt = AdamW(groups, lr=1e-3)
        else:
            opt, tk = torch_adamw(groups)
            kind = f"torch.optim.AdamW ({tk}, sink)"
        runner = Runner(model, dev, WTS, compute_metrics=False)
        fused = "FUSED_SGD=0" not in kind

        def step(runner=runner, opt=opt, batch=batch, fused=fused):
            rt.set_fused_sgd(fused)
            loss, _ = runner(batch, None, True)
            opt.zero_grad()
            loss.backward()
            opt.step()
        runs[kind] = step
    for f in runs.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    gc.collect()
    gc.freeze()
    ms = {k: [] for k in runs}
    for _ in range(rounds):
        for k, f in runs.items():
            f()          # the switch between variants settles outside the timed window
            ms[k].append(timed(f, steps))
    rt.set_fused_sgd(True)
    say()
    say(f"(b) reference-loop step, cfg2, B = 64, bf16: median of {rounds} alternated rounds of {steps} steps (min .. max)")
    for k, v in ms.items():
        say(f"{k:36} {statistics.median(v):8.3f} ms/step   ({min(v):.3f} .. {max(v):.3f})")
    say("arithmetic, not measured: AdamW's extra 8 B/param over unfused SGD is about 5 GB per step, about 1 ms at 5 TB/s")
    gc.unfreeze()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    part_a(args.rounds)
    part_b(args.rounds)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
