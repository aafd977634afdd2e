#!/usr/bin/env python
"""Time the marginal cross-entropy launch (afft_softmax_ce_groups: softmax_ce_groups_kernel, loss and fp32 gradient in ONE launch)
beside the weighted action term's gradient launch (afft_softmax_ce_w, class weights, smoothing 0.1) on the same logits, one process:
rows = 1088, C = 3806, hard labels, G = 97 (the verbs of EPIC-KITCHENS-100) and G = 300 (its nouns), a random class -> group map in
which every group has a member.

    python tools/ce_groups_bench.py [--out profiles/ce_groups.txt] [--rows 1088] [--C 3806] [--reps 7] [--launches 400]

A timed window is `launches` back-to-back launches between two device events; per-launch time = window / launches; the baseline and
the two group launches alternate, window by window, and the median of `reps` windows of each is reported.  Every window is warmed up
first.  The logits (16.6 MB) stay in the 256 MB last-level cache between launches: cache-resident times for all alike.
Requested bytes of a group launch, from the shapes (what the kernel asks of the memory system, not what reaches HBM): three passes
over the row (max, sum, gradient), group_of once, the target group's members twice with their index, and the gradient written once:
rows * (4 * 4 C + 4 C + 2 * 8 * mean group size)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--rows", type=int, default=1088)
    ap.add_argument("--C", type=int, default=3806)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=400)
    a = ap.parse_args()
    import torch
    from afft_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("ce_groups_bench: no GPU visible (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rows, C = a.rows, a.C
    x = (torch.randn(rows, C, generator=g) * 3).to(dev)
    labels = torch.randint(0, C, (rows,), generator=g)
    w = (torch.rand(C, generator=g) + 0.5).to(dev)
    row_g = torch.rand(rows, generator=g).to(dev)
    rl = torch.empty(rows, device=dev)
    d = torch.empty(rows, C, device=dev)
    d2 = torch.empty(rows, C, device=dev)
    lab_d = labels.to(dev)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.launches      # microseconds per launch

    names, fns, nbytes = ["softmax_ce_w"], [lambda: ops.softmax_ce_w(x, C, labels=lab_d, dlogits=d, row_g=row_g, weight=w, smoothing=0.1)], [None]
    for G in (97, 300):
        perm = torch.randperm(C, generator=g)
        go = torch.randint(0, G, (C,), generator=g)
        go[perm[:G]] = torch.arange(G)
        groups = ops.group_csr(go, G, device=dev)
        gl = go[labels].to(dev)
        names.append(f"groups G={G}")
        fns.append(lambda groups=groups, gl=gl: ops.softmax_ce_groups(x, C, groups, glabels=gl, dlogits=d2, row_g=row_g, row_loss=rl))
        nbytes.append(rows * (16 * C + 4 * C + 16 * C / G))
    for fn in fns:
        window(fn)
    times = [[] for _ in fns]
    for _ in range(a.reps):
        for t, fn in zip(times, fns):
            t.append(window(fn))
    med = [statistics.median(t) for t in times]
    lines = [f"ce_groups_bench: rows={rows} C={C} launches/window={a.launches} windows={a.reps} device={torch.cuda.get_device_name(0)}",
             "hard labels, fp32 gradient; us per launch, median of the windows (min..max), ratio to afft_softmax_ce_w's gradient launch "
             "on the same logits, requested bytes / time",
             "the group launch writes row_loss AND dlogits; the baseline is the gradient launch alone (its forward launch is a second one)"]
    for n, m, t, b in zip(names, med, times, nbytes):
        rate = "" if b is None else f"  requested {b / 1e6:7.2f} MB -> {b / m / 1e3:7.1f} GB/s"
        lines.append(f"{n:14s} {m:8.2f} ({min(t):6.2f}..{max(t):6.2f})  {m / med[0]:5.3f}x{rate}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
