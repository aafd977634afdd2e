#!/usr/bin/env python
"""Time the weight-average update (afft_ema: 12 B per parameter) against the AdamW update (afft_adam with its bf16 image: 30 B per
parameter) on buffers of the cfg2 flat size, one process, the two alternated window by window; afft_swap_f32 (16 B per element, twice
per evaluation) is timed beside them.

    python tools/ema_bench.py [--out profiles/ema_step.txt] [--n ELEMENTS] [--reps 7] [--launches 20]

A timed window is `launches` back-to-back launches between two device events; per-launch time = window / launches; the median of
`reps` windows of each kernel is reported with its algorithmic bytes per second (every operand read once, every result written once).
Every kernel is warmed up first.  The buffers are far larger than the 256 MB last-level cache, so these are HBM times.  The bar for
afft_ema is relative to this run's own afft_adam: at least 90 % of its bytes per second (the shorter kernel spends a larger share of
its time between launches); the last line says whether it was met."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

BAR = 0.90


def cfg2_flat_size(dev):
    """elements of parallel.FlatParams' buffers for the cfg2 model: every trainable parameter, 64-aligned"""
    import bench as B
    model, _ = B.build_model("cfg2", dev)
    n = sum((p.numel() + 63) // 64 * 64 for p in model.parameters() if p.requires_grad)
    del model
    return n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--n", type=int, default=0, help="elements per buffer (default: the cfg2 flat size)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    import torch
    from afft_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench: no GPU visible (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    n = a.n or cfg2_flat_size(dev)
    torch.cuda.empty_cache()
    p = torch.randn(n, device=dev) * 0.02
    g = torch.randn(n, device=dev) * 1e-3
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    p16 = torch.empty(n, dtype=torch.bfloat16, device=dev)
    avg = p.clone()
    step = torch.zeros((), device=dev)
    ok = torch.ones((), device=dev)
    kernels = {      # name: (launch, bytes per element)
        "afft_adam (AdamW, bf16 image)": (lambda: ops.adam(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, step, True, p_bf16=p16, ok=ok), 30),
        "afft_ema (w = 2e-4, ok flag)": (lambda: ops.ema(avg, p, 2e-4, ok=ok), 12),
        "afft_swap_f32": (lambda: ops.swap_f32(avg, m), 16),
    }

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.launches      # milliseconds per launch

    for fn, _ in kernels.values():
        window(fn)
    ms = {k: [] for k in kernels}
    for _ in range(a.reps):
        for k, (fn, _) in kernels.items():
            ms[k].append(window(fn))
    lines = [f"ema_bench: n={n} ({n / 1e6:.1f} M elements per buffer) launches/window={a.launches} windows={a.reps} "
             f"device={torch.cuda.get_device_name(0)} torch={torch.__version__}",
             f"{'kernel':32s} {'ms':>8s} {'B/elem':>7s} {'GB':>7s} {'GB/s':>8s}   windows (min .. max ms)"]
    gbs = {}
    for k, (_, bpe) in kernels.items():
        t = statistics.median(ms[k])
        gbs[k] = n * bpe / 1e9 / (t * 1e-3)
        lines.append(f"{k:32s} {t:8.3f} {bpe:7d} {n * bpe / 1e9:7.2f} {gbs[k]:8.0f}   {min(ms[k]):.3f} .. {max(ms[k]):.3f}")
    adam, ema = list(kernels)[:2]
    ratio = gbs[ema] / gbs[adam]
    lines.append(f"afft_ema / afft_adam bytes per second: {ratio:.3f} (bar {BAR:.2f}): {'met' if ratio >= BAR else 'NOT met'}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
