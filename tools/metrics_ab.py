"""Cost of the metric half of the training step at cfg2, 64 and 16 clips, with MixUp, in the reference's loop shape
(runner(...) -> zero_grad -> backward -> step -> tracker.update), device_metrics off and on alternated in one process.

  off  Runner's default metric path (the parent commit's): topk / clone / index_put on the (B, 3806) logits, a pinned host copy of
       them, np.argsort over every row in the tracker -- the baseline;
  on   Runner(device_metrics=True): one ops.label_rank call, one ops.recall_accumulate launch in the tracker.

Recorded per batch size: ms per step, host time inside runner(...) + tracker.update(...), and the number of kernel launches between
the first loss kernel of a step and the first backward kernel, counted in a rocprofv3 --kernel-trace --stats run of its own (a child
process per leg: `--trace-leg off|on`; the parent parses the trace).

usage: python tools/metrics_ab.py [--rounds 5] [--steps 10] [--no-trace] [--out profiles/metrics_step.txt]"""
import argparse
import csv
import gc
import glob
import os
import socket
import statistics
import subprocess
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as B  # noqa: E402
import afft_amd  # noqa: E402
from afft_amd import runtime as rt  # noqa: E402
from afft_amd.common.metric_tracking import MetricTracker  # noqa: E402
from afft_amd.common.mixup import MixUp  # noqa: E402
from afft_amd.common.runner import Runner  # noqa: E402
from afft_amd.common.scheduler import prepare_params  # noqa: E402
from afft_amd.optim import SGD  # noqa: E402

dev = torch.device("cuda:0")
WTS = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
NCLS = 3806
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def make_leg(model, opt, c, clips, on):
    feats, tgt, sub = B.make_inputs(c, clips, c["T"], 0, dev)
    batch = ({"data_dict": feats, "target": tgt, "target_subclips": sub}, {})
    mix = MixUp(alpha=0.1, label_smoothing={"action": 0.4}, num_classes={"action": NCLS})
    runner = Runner(model, dev, WTS, device_metrics=on)
    tracker = MetricTracker({"action": NCLS})
    host = [0.0]

    def step():
        t0 = time.perf_counter()
        loss, metrics = runner(batch, mix, True)
        t1 = time.perf_counter()
        opt.zero_grad()
        loss.backward()
        opt.step()
        t2 = time.perf_counter()
        tracker.update(metrics, clips, True)
        host[0] += (t1 - t0) + (time.perf_counter() - t2)
    return step, host, tracker


def setup():
    afft_amd.set_precision("bf16")
    rt.set_grad_mode("sink")
    model, c = B.build_model("cfg2", dev)
    model.train()
    opt = SGD(prepare_params(model, None, 1e-3, 1e-6), lr=1e-3, momentum=0.9, nesterov=True)
    return model, opt, c


def measure(rounds, steps):
    model, opt, c = setup()
    for clips in (64, 16):
        legs = {name: make_leg(model, opt, c, clips, on) for name, on in (("off", False), ("on", True))}
        for step, _, _ in legs.values():
            for _ in range(5):
                step()
        torch.cuda.synchronize()
        gc.collect()
        gc.freeze()
        ms = {k: [] for k in legs}
        host_ms = {k: [] for k in legs}
        for _ in range(rounds):
            for k, (step, host, tracker) in legs.items():
                step()          # the switch between legs settles outside the timed window
                torch.cuda.synchronize()
                host[0] = 0.0
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(steps):
                    step()
                b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b) / steps)
                host_ms[k].append(host[0] * 1e3 / steps)
        gc.unfreeze()
        say(f"cfg2, {clips} clips, bf16, MixUp, reference loop: median of {rounds} alternated rounds of {steps} steps (min .. max)")
        for k in legs:
            say(f"  device_metrics {k:3}  {statistics.median(ms[k]):8.3f} ms/step ({min(ms[k]):.3f} .. {max(ms[k]):.3f})   host in runner + "
                f"tracker.update {statistics.median(host_ms[k]):7.3f} ms/step ({min(host_ms[k]):.3f} .. {max(host_ms[k]):.3f})")
        vals = {k: legs[k][2].get_all_data(True) for k in legs}
        key = next(k for k in vals["off"] if "mt5r" in k)
        say(f"  mt5r of the epoch so far: off {vals['off'][key]}, on {vals['on'][key]}")


def trace_leg(on, clips, steps=4):
    """child process under rocprofv3: a few steps of one leg"""
    model, opt, c = setup()
    step, _, _ = make_leg(model, opt, c, clips, on)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()


def launches_between_loss_and_backward(trace_csv):
    """per step: kernels after the step's first softmax_ce_kernel up to (not including) its loss_reduce_bwd_kernel, the first kernel
    of the backward pass; the last step of the trace"""
    with open(trace_csv, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    ends = [i for i, n in enumerate(names) if "loss_reduce_bwd_kernel" in n]
    if not ends:
        return None
    end = ends[-1]
    prev = ends[-2] if len(ends) > 1 else -1
    first = next(i for i in range(prev + 1, end) if "softmax_ce_kernel" in names[i])
    return end - first - 1, names[first + 1:end]


def trace(out_lines):
    exe = "rocprofv3"
    for clips in (64, 16):
        counts = {}
        for leg in ("off", "on"):
            with tempfile.TemporaryDirectory() as d:
                cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "trace", "--",
                       sys.executable, os.path.abspath(__file__), "--trace-leg", leg, "--clips", str(clips)]
                subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
                found = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
                counts[leg] = launches_between_loss_and_backward(found[0]) if found else None
        for leg, res in counts.items():
            if res is None:
                say(f"  {clips} clips, device_metrics {leg}: no kernel trace")
                continue
            n, names = res
            short = [x.split("(")[0].split("<")[0][-40:] for x in names]
            say(f"  {clips} clips, device_metrics {leg:3}: {n} launches between the first loss kernel and the first backward kernel: {short}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-leg", choices=("off", "on"), default=None)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace_leg:
        trace_leg(args.trace_leg == "on", args.clips)
        sys.exit(0)
    say(f"box: {socket.gethostname()}; device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    measure(args.rounds, args.steps)
    torch.cuda.synchronize()
    if not args.no_trace:
        say("kernel launches (rocprofv3 --kernel-trace --stats, one child process per leg):")
        trace(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
