#!/usr/bin/env python
"""Time the late-fusion weight search (afft_amd.challenge.device_sweep) at EPIC-KITCHENS-100 validation size against the two paths a
sweep had before it: N = 9668 segments, R = 3 runs, 64 weight sets, for the action (C = 3806), noun (300) and verb (97) spaces.

    python tools/fuse_sweep_bench.py [--out profiles/late_fuse_sweep.txt] [--sets 64] [--reps 5] [--no-host-loop]

Per space it reports, as time per weight set:
  sweep       device_sweep over all sets (scores already on the device): fused_label_rank + rank_counts_sets + the copy of the counters;
  kernel      afft_fused_label_rank alone (device events), with the bytes it requests -- one pass over the R matrices per tile of 8
              sets -- over that time, set against the 3.9 TB/s of the HBM.  The tiles re-read the same R matrices, which the 256 MiB
              Infinity Cache can hold in part or whole: this is a request rate, not HBM traffic, and may exceed the HBM's;
  per-set     what the parent commit offers for one set: weighted_sum_fwd into a materialised [N, C] combination, then device_accuracy
              on it (label_rank, recall_accumulate, the copy of the counters);
and once, for all three spaces together:
  late_fuse   one iteration of get_epic_marginalize_late_fuse's loop over weight combinations (combine on the device, copy back, rebuild
              the {uid: row} dicts, compute_accuracies_epic in numpy), taken as the difference between a call with two combinations
              and a call with one, runs served from memory.
Every timed window ends in a device synchronise and is warmed up first; medians over --reps.  The sweep's numbers are checked against
the per-set path's before anything is timed.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

HBM_BYTES_PER_S = 3.9e12
WT = 8


def _median_ms(fn, reps, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--N", type=int, default=9668)
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host-loop", action="store_true", help="skip the get_epic_marginalize_late_fuse iteration (tens of seconds)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from afft_amd import challenge, ops
    if not torch.cuda.is_available():
        raise SystemExit("fuse_sweep_bench: no GPU visible (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    N, R = a.N, a.runs
    spaces = (("action", 3806), ("noun", 300), ("verb", 97))
    weights = (torch.rand(a.sets, R, generator=gen) * 2).numpy().astype(np.float32)
    lines = [f"late-fusion weight search: N = {N} segments, R = {R} runs, {a.sets} weight sets; medians of {a.reps} windows, each ended by a "
             f"device synchronise", f"device: {torch.cuda.get_device_name(0)}", ""]
    host = {}
    for name, C in spaces:
        xs = [torch.randn(N, C, generator=gen).to(dev) for _ in range(R)]
        labels = torch.randint(0, C, (N,), generator=gen).to(dev)
        host[name] = ([x.cpu().numpy() for x in xs], labels.cpu().numpy())
        w_dev = torch.from_numpy(weights).to(dev)
        out = torch.empty(N, C, device=dev)

        def per_set(j):
            ops.weighted_sum_fwd(xs, w_dev[j:j + 1].expand(N, R), out)
            return challenge.device_accuracy(out, labels)

        sweep = challenge.device_sweep(xs, labels, weights)
        for j in (0, a.sets - 1):                               # the same integer counts; device_accuracy rounds its accuracies to fp32
            want = per_set(j)
            assert abs(sweep[0][j] - want[0]) < 1e-4 and abs(sweep[1][j] - want[1]) < 1e-4 and abs(sweep[2][j] - want[2]) < 1e-9, (j, want)
        t_sweep = _median_ms(lambda: challenge.device_sweep(xs, labels, weights), a.reps)
        t_set = _median_ms(lambda: [per_set(j) for j in range(a.sets)], a.reps)
        rank = torch.empty(a.sets, N, dtype=torch.int32, device=dev)
        ev = []
        for _ in range(2 + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.fused_label_rank(xs, w_dev, labels, rank=rank)
            e1.record()
            torch.cuda.synchronize()
            ev.append(e0.elapsed_time(e1))
        t_kernel = statistics.median(ev[2:])
        tiles = (a.sets + WT - 1) // WT
        nbytes = tiles * R * N * C * 4
        rate = nbytes / (t_kernel * 1e-3)
        lines += [f"{name} (C = {C}):",
                  f"  sweep    {t_sweep / a.sets:9.4f} ms per set   ({t_sweep:.3f} ms for {a.sets} sets: device_sweep, counters copied back)",
                  f"  kernel   {t_kernel / a.sets:9.4f} ms per set   ({t_kernel:.3f} ms for {tiles} tiles of {WT}; {nbytes / 1e6:.1f} MB requested, "
                  f"{rate / 1e12:.3f} TB/s = {100 * rate / HBM_BYTES_PER_S:.1f} % of the HBM's 3.9 TB/s; cache hits included)",
                  f"  per-set  {t_set / a.sets:9.4f} ms per set   ({t_set:.3f} ms for {a.sets} sets: weighted_sum_fwd + device_accuracy each)",
                  f"  per-set / sweep = {t_set / t_sweep:.1f}", ""]
        print("\n".join(lines[-6:]), flush=True)
    if not a.no_host_loop:
        import pandas as pd

        class _DS:
            df = pd.DataFrame(dict(narration_id=[f"s{i}" for i in range(N)], verb_class=host["verb"][1], noun_class=host["noun"][1],
                                   action_class=host["action"][1]))
            classes_manyshot = {}
        served = {f"run{i}": [host[s][0][i] for s in ("verb", "noun", "action")] for i in range(R)}
        challenge.get_epic_marginalize_verb_noun = lambda resdir, dataset=None: ({}, served[resdir])
        challenge.print_accuracies_epic = lambda *args, **kw: None
        took = []
        for n in (1, 2):
            t0 = time.perf_counter()
            challenge.get_epic_marginalize_late_fuse(list(served), [list(map(float, w)) for w in weights[:n]], dataset=_DS)
            torch.cuda.synchronize()
            took.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        challenge.late_fuse_sweep(list(served), [list(map(float, w)) for w in weights], dataset=_DS)
        t_all = time.perf_counter() - t0
        lines += ["all three spaces, runs served from memory as {uid: row} dicts (one window each, not a median):",
                  f"  late_fuse  {1e3 * (took[1] - took[0]):10.1f} ms per weight combination   (get_epic_marginalize_late_fuse: {took[0]:.2f} s with "
                  f"one combination, {took[1]:.2f} s with two)",
                  f"  late_fuse_sweep  {1e3 * t_all:10.1f} ms for all {a.sets} combinations, reading and stacking the runs included", ""]
        print("\n".join(lines[-4:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
