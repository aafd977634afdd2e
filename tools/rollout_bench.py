#!/usr/bin/env python
"""Time the evaluation forward of the future predictor alone (BaseFuturePredictor: eval mode, no grad) over output_len = 1, 2, 4, 8 --
or, with --train, one training pass of it (training mode with the reference's drop rates, forward + backward of sum(out * w) in sink
mode) over output_len = 2, 4, 8.

    python tools/rollout_bench.py [--tree DIR] [--cache 0|1] [--label NAME] [--out FILE]      one run: one JSON line per output_len
    python tools/rollout_bench.py --train [--cache-train 0|1] ...                             the same for a training pass
    python tools/rollout_bench.py --table FILE [FILE ...]                                     the table of several runs

Defaults are the cfg2 widths of bench.py: B = 64 clips, T = 16 frames, D = 2048, 6 layers, 4 heads, precision bf16.  --tree imports
afft_amd from another checkout (a build of the parent commit, to compare against); --cache sets runtime.set_kv_cache where the tree has
it, --cache-train sets runtime.set_kv_cache_train where the tree has it (0, or a tree without it: the recompute).  --precision fp16x2
--cache-fp16x2 0|1: the evaluation forward in that precision with runtime.set_kv_cache_fp16x2 off (the recompute: the parent's behaviour)
or on (the cached roll-out through the composite step), where the tree has the switch.  Every pass is bracketed by a device event pair and followed by a synchronise; every output_len is warmed up before its timed
window; a run reports the median and the 10th / 90th percentile of its window.  Run-to-run spread: repeat the command (alternating the
trees) and give the files to --table, which prints every run's median and their range per label.
"""
import argparse
import json
import os
import statistics
import sys


def run(a):
    tree = os.path.abspath(a.tree or os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    sys.path.insert(0, tree)
    import torch
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.models.future_prediction import BaseFuturePredictor
    assert os.path.abspath(afft_amd.__file__).startswith(tree), (afft_amd.__file__, tree)
    if not torch.cuda.is_available():
        raise SystemExit("rollout_bench: no GPU visible (there is nothing to time without one)")
    afft_amd.set_precision(a.precision)
    has_switch = hasattr(rt, "set_kv_cache")
    if has_switch:
        rt.set_kv_cache(bool(a.cache))
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    has_train = hasattr(rt, "set_kv_cache_train")
    if has_train:
        rt.set_kv_cache_train(bool(a.cache_train))
    has_f16 = hasattr(rt, "set_kv_cache_fp16x2")
    if has_f16:
        rt.set_kv_cache_fp16x2(bool(a.cache_fp16x2))
    pred = BaseFuturePredictor(a.D, inter_dim=a.D, n_layer=a.layers, n_head=a.heads).to(dev)
    pred = pred.train() if a.train else pred.eval()
    feats = torch.randn(a.B, a.T, a.D, device=dev)
    lines = []
    if a.train:
        rt.set_grad_mode("sink")
        params = list(pred.parameters())

        def once(n_out, w):
            rt.SINK.begin_step()
            out, _ = pred(feats, n_out)
            (out * w).sum().backward()
            rt.SINK.finish_step(params)
            return out
    else:
        def once(n_out, w):
            return pred(feats, n_out)[0]
    with torch.set_grad_enabled(bool(a.train)):
        for n_out in a.output_len or ([2, 4, 8] if a.train else [1, 2, 4, 8]):
            w = torch.randn(a.B, a.T + n_out - 1, a.D, device=dev) if a.train else None
            for _ in range(a.warmup):
                once(n_out, w)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = once(n_out, w)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            ms.sort()
            rec = dict(label=a.label, kv_cache=bool(a.cache) if has_switch else None, train=bool(a.train),
                       kv_cache_train=bool(a.cache_train) if has_train else None,
                       kv_cache_fp16x2=bool(a.cache_fp16x2) if has_f16 else None, precision=a.precision, B=a.B, T=a.T, D=a.D, layers=a.layers,
                       output_len=n_out, reps=a.reps, median_ms=round(statistics.median(ms), 4), p10_ms=round(ms[len(ms) // 10], 4),
                       p90_ms=round(ms[(len(ms) * 9) // 10], 4), checksum=float(out.detach().float().abs().mean()))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def table(files):
    runs = {}      # (label, output_len) -> [median of each run]
    for fn in files:
        with open(fn) as f:
            for line in f:
                if line.strip():
                    r = json.loads(line)
                    runs.setdefault((r["label"], r["output_len"]), []).append(r["median_ms"])
    labels = sorted({k[0] for k in runs})
    print(f"{'output_len':>10}  " + "  ".join(f"{lb + ' median ms of each run (min..max)':<58}" for lb in labels))
    for n_out in sorted({k[1] for k in runs}):
        cells = []
        for lb in labels:
            m = runs.get((lb, n_out), [])
            cells.append(f"{' '.join(f'{x:.3f}' for x in m)} ({min(m):.3f}..{max(m):.3f})" if m else "-")
        print(f"{n_out:>10}  " + "  ".join(f"{c:<58}" for c in cells))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--table", nargs="+")
    ap.add_argument("--tree")
    ap.add_argument("--cache", type=int, default=1)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--out")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--cache-train", type=int, default=1)
    ap.add_argument("--cache-fp16x2", type=int, default=0)
    ap.add_argument("--output-len", type=int, nargs="+", default=None)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=16)
    ap.add_argument("--D", type=int, default=2048)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    a = ap.parse_args()
    if a.table:
        table(a.table)
    else:
        run(a)


if __name__ == "__main__":
    main()
