#!/usr/bin/env python
"""Time the weighted / label-smoothed cross-entropy launch (afft_softmax_ce_w with class weights and smoothing 0.1: the general
instantiation of softmax_ce_kernel) against the plain launch (afft_softmax_ce) on the same logits: rows = 1024, C = 3806, hard labels
and soft targets, the forward launch (row_loss) and the gradient launch (dlogits fp32, row_g), one process.

    python tools/ce_weighted_bench.py [--out profiles/ce_weighted.txt] [--rows 1024] [--C 3806] [--reps 5] [--launches 200]

A timed window is `launches` back-to-back launches between two device events (one launch is a few microseconds: a window of one would
time the event pair); per-launch time = window / launches; the two variants alternate, window by window, and the median of `reps`
windows of each is reported with its ratio.  Every window is warmed up first.  The logits (15.6 MB) stay in the 256 MB last-level
cache between launches, so these are cache-resident times for both variants alike.  The extra traffic of the general kernel is the
weight vector (C floats per row, from cache) read once per column loop."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--C", type=int, default=3806)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    import torch
    from afft_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("ce_weighted_bench: no GPU visible (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rows, C = a.rows, a.C
    x = (torch.randn(rows, C, generator=g) * 3).to(dev)
    labels = torch.randint(0, C, (rows,), generator=g).to(dev)
    soft = torch.softmax(torch.randn(rows, C, generator=g), 1).to(dev)
    w = (torch.rand(C, generator=g) + 0.5).to(dev)
    row_g = torch.rand(rows, generator=g).to(dev)
    rl = torch.empty(rows, device=dev)
    d = torch.empty(rows, C, device=dev)
    opts = dict(weight=w, smoothing=0.1)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.launches      # microseconds per launch

    lines = [f"ce_weighted_bench: rows={rows} C={C} launches/window={a.launches} windows={a.reps} device={torch.cuda.get_device_name(0)}",
             f"{'target':6s} {'launch':9s} {'plain us':>10s} {'weighted us':>12s} {'ratio':>7s}"]
    for tname, tkw in (("hard", dict(labels=labels)), ("soft", dict(soft=soft))):
        for lname, lkw in (("forward", dict(row_loss=rl)), ("gradient", dict(dlogits=d, row_g=row_g))):
            plain = lambda: ops.softmax_ce(x, C, **tkw, **lkw)                  # noqa: E731
            wtd = lambda: ops.softmax_ce_w(x, C, **tkw, **lkw, **opts)          # noqa: E731
            window(plain), window(wtd)
            tp, tw = [], []
            for _ in range(a.reps):
                tp.append(window(plain))
                tw.append(window(wtd))
            mp, mw = statistics.median(tp), statistics.median(tw)
            lines.append(f"{tname:6s} {lname:9s} {mp:10.2f} {mw:12.2f} {mw / mp:7.3f}   (windows: plain {min(tp):.2f}..{max(tp):.2f}, "
                         f"weighted {min(tw):.2f}..{max(tw):.2f})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
