"""Time of the LayerNorm backward kernel (csrc/norm.hip) alone at rows = 5120: the wide arrangement at d = 4096 (2 row groups x 8 column
slices) beside the d = 2048 kernel (4 x 4), bf16 dy, with the incoming dx and the bf16 copy, without dw / db (so that the column
reduction kernel is not launched: the event window holds ln_bwd_kernel only).  Device events over windows of >= 0.3 s after warm-up, the
two widths alternating in one process, three rounds.  GB/s over the bytes the library's kernel trace counts for the call:
rows * d * (2 dy + 4 x + 4 dx_in + 4 dx_out + 2 dx_bf16) + 8 rows.

Two figures per width.  "resident": one set of buffers launched back to back -- 168 MB at d = 2048 stay in the 256 MiB last-level cache from
one launch to the next, 336 MB at d = 4096 only in part, so the two are not comparable.  "streamed": successive launches walk through
enough sets of buffers (>= 1.3 GB in all) that every launch finds its operands in HBM: the figure that says what the kernel does in a
training step, and the one to compare across widths.

usage: python tools/ln_bwd_wide.py [--out FILE]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS = 5120


def setup(d, sets=1):
    """a launch closure; sets > 1: successive launches take successive sets of buffers"""
    if sets > 1:
        fns = [setup(d) for _ in range(sets)]
        state = {"i": 0}

        def rotate():
            fns[state["i"] % sets]()
            state["i"] += 1
        return rotate
    import torch
    from afft_amd import ops
    dev = torch.device("cuda:0")
    x = torch.randn(ROWS, d, device=dev) * 2.0 + 0.3
    w = torch.randn(d, device=dev) * 0.2 + 1.0
    y = torch.empty(ROWS, d, device=dev)
    mean, rstd = torch.empty(ROWS, device=dev), torch.empty(ROWS, device=dev)
    ops.layernorm_fwd(x, w, None, 1e-6, y, mean, rstd)
    dy = torch.randn(ROWS, d, device=dev).to(torch.bfloat16)
    dx_in = torch.randn(ROWS, d, device=dev)
    dx = torch.empty(ROWS, d, device=dev)
    dxb = torch.empty(ROWS, d, dtype=torch.bfloat16, device=dev)
    return lambda: ops.layernorm_bwd(dy, x, w, mean, rstd, dx, dx_in=dx_in, dx_bf16=dxb)


def timed(fn):
    import torch
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 200
    while True:
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= 300.0 or reps >= 100000:
            return ms / reps
        reps = int(reps * max(2.0, 400.0 / max(ms, 1e-3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for mode, sets in (("resident", {2048: 1, 4096: 1}), ("streamed", {2048: 8, 4096: 4})):
        fns = {d: setup(d, n) for d, n in sets.items()}
        best = {}
        for rnd in range(3):
            for d, fn in fns.items():
                ms = timed(fn)
                nbytes = ROWS * d * 16 + ROWS * 8
                gbs = nbytes / ms * 1e-6
                best[d] = max(best.get(d, 0.0), gbs)
                lines.append(f"{mode} round {rnd}: rows {ROWS} d {d}: {ms * 1e3:8.1f} us  {gbs:8.1f} GB/s")
                print(lines[-1], flush=True)
        lines.append(f"{mode}, best of 3: d 2048 {best[2048]:.1f} GB/s, d 4096 {best[4096]:.1f} GB/s, ratio 4096 / 2048 = {best[4096] / best[2048]:.3f}")
        print(lines[-1], flush=True)
        del fns
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
