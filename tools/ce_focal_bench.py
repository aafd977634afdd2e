#!/usr/bin/env python
"""Time the focal / logit-adjusted cross-entropy launch (afft_softmax_ce_focal: softmax_ce_focal_kernel) against the weighted launch
(afft_softmax_ce_w) on the same logits, class weights and smoothing: rows = 1024, C = 3806, the forward launch (row_loss) and the
gradient launch (dlogits fp32, row_g), one process.  Hard labels run with smoothing 0 (one non-zero coefficient per row: the kernel's
one-term path) and with smoothing 0.1; soft targets with smoothing 0.1.  Variants: gamma 0 with an adjustment, gamma 2, gamma 2 with an
adjustment.

    python tools/ce_focal_bench.py [--out profiles/ce_focal.txt] [--rows 1024] [--C 3806] [--reps 5] [--launches 200]

A timed window is `launches` back-to-back launches between two device events; per-launch time = window / launches; the baseline and
the three variants alternate, window by window, and the median of `reps` windows of each is reported with its ratio to the baseline.
Every window is warmed up first.  The logits (15.6 MB) stay in the 256 MB last-level cache between launches, so these are
cache-resident times for all variants alike."""
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
        raise SystemExit("ce_focal_bench: no GPU visible (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rows, C = a.rows, a.C
    x = (torch.randn(rows, C, generator=g) * 3).to(dev)
    labels = torch.randint(0, C, (rows,), generator=g).to(dev)
    soft = torch.softmax(torch.randn(rows, C, generator=g), 1).to(dev)
    w = (torch.rand(C, generator=g) + 0.5).to(dev)
    b = (-8.0 * torch.rand(C, generator=g)).to(dev)
    row_g = torch.rand(rows, generator=g).to(dev)
    rl = torch.empty(rows, device=dev)
    d = torch.empty(rows, C, device=dev)
    variants = (("g0+adj", dict(adjust=b, gamma=0.0)), ("g2", dict(adjust=None, gamma=2.0)), ("g2+adj", dict(adjust=b, gamma=2.0)))

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.launches      # microseconds per launch

    lines = [f"ce_focal_bench: rows={rows} C={C} launches/window={a.launches} windows={a.reps} device={torch.cuda.get_device_name(0)}",
             "us per launch, median of the windows (ratio to afft_softmax_ce_w on the same inputs; min..max of the windows)",
             f"{'target':10s} {'launch':9s} {'weighted':>10s} " + " ".join(f"{n:>28s}" for n, _ in variants)]
    targets = (("hard e=0", dict(labels=labels), 0.0), ("hard e=.1", dict(labels=labels), 0.1), ("soft e=.1", dict(soft=soft), 0.1))
    for tname, tkw, eps in targets:
        for lname, lkw in (("forward", dict(row_loss=rl)), ("gradient", dict(dlogits=d, row_g=row_g))):
            fns = [lambda: ops.softmax_ce_w(x, C, **tkw, **lkw, weight=w, smoothing=eps)]
            for _, fkw in variants:
                fns.append(lambda fkw=fkw: ops.softmax_ce_focal(x, C, **tkw, **lkw, weight=w, smoothing=eps, **fkw))
            for fn in fns:
                window(fn)
            times = [[] for _ in fns]
            for _ in range(a.reps):
                for t, fn in zip(times, fns):
                    t.append(window(fn))
            med = [statistics.median(t) for t in times]
            cells = " ".join(f"{m:8.2f} ({m / med[0]:5.3f}x {min(t):6.2f}..{max(t):6.2f})" for m, t in zip(med[1:], times[1:]))
            lines.append(f"{tname:10s} {lname:9s} {med[0]:10.2f} {cells}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
