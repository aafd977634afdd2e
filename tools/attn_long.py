"""Forward and backward time of the long-sequence attention kernels (csrc/attention_long.hip) alone, bf16 storage, every shape as the
MFMA form and as the generic form.  AFFT_ATTN_GENERIC is read once per process, so every (shape, form) runs in a fresh child process
(one GPU process at a time).  Per setting: device-event time over a window of >= 0.3 s after warm-up, TF/s over the four / eight
L^2 hd products the algorithm needs (forward 4 nseq H L^2 hd, backward 8 nseq H L^2 hd; the backward kernels execute 10), GB/s
over the bytes that have to move (q, k, v, out (+ dout, dq, dk, dv) once, probs once).

Then one configuration nobody has timed before: the five cfg5 streams at T = 32 through the T-SA-Fuser (160 tokens), 16 clips, one bf16
training step of the Trainer (train mode, eager, optimizer included): host clock around steps that end in a synchronise, and, from one
more step under the library's kernel trace (afft_kernel_trace_begin / _end), the summed event time of the attention calls over the step.

usage: python tools/attn_long.py [--out FILE]          (children: --one nseq L H hd | --step)"""
import argparse
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(64, 160, 4, 512), (64, 320, 4, 512), (16, 512, 4, 512), (64, 160, 4, 256)]


def one(nseq, L, H, hd):
    import torch
    from afft_amd import ops
    dev = torch.device("cuda:0")
    d, R = H * hd, nseq * L
    g = torch.randn(R, 3 * d, device=dev).to(torch.bfloat16)
    q, k, v = g[:, :d], g[:, d:2 * d], g[:, 2 * d:]
    out = torch.empty(R, d, dtype=torch.bfloat16, device=dev)
    dout = torch.randn(R, d, device=dev).to(torch.bfloat16)
    dg = torch.empty(R, 3 * d, dtype=torch.bfloat16, device=dev)
    probs = torch.empty(nseq, H, L, L, device=dev)
    scale, period = hd ** -0.5, L // 4

    def fwd():
        ops.attention_long_fwd(q, k, v, nseq, L, H, hd, scale, 3, out, probs, mask_period=period)

    def bwd():
        ops.attention_long_bwd(dout, q, k, v, probs, nseq, L, H, hd, scale, dg[:, :d], dg[:, d:2 * d], dg[:, 2 * d:])

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps, ms = 10, 0.0
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

    pairs = nseq * H * L * L
    rw = nseq * L * H * hd * 2
    for name, fn, flops, nbytes in (("fwd", fwd, 4 * pairs * hd, 4 * rw + 4 * pairs), ("bwd", bwd, 8 * pairs * hd, 7 * rw + 4 * pairs)):
        ms = timed(fn)
        form = "generic" if os.environ.get("AFFT_ATTN_GENERIC") == "1" else "mfma"
        print(f"({nseq:3d}, {L:3d}, {H}, {hd:4d}) {form:7s} {name}: {ms * 1e3:9.1f} us  {flops / ms * 1e-9:7.2f} TF/s  {nbytes / ms * 1e-6:8.1f} GB/s",
              flush=True)


def step(B=16, T=32, warm=6, n=20):
    import time
    import torch
    from afft_amd import _lib
    from afft_amd.config import BASELINE_CONFIGS, make_model_cfg
    from afft_amd.models.base_model import BaseModel
    from afft_amd.parallel import Trainer
    dev = torch.device("cuda:0")
    c = BASELINE_CONFIGS["cfg5"]
    torch.manual_seed(42)
    cfg = make_model_cfg(c["modal_dims"], c["common_dim"], c["fp_inter_dim"], fuser="tsa", T=T, modal_encoding=True)
    model = BaseModel(cfg, num_classes={"action": 3806}, class_mappings={}).to(dev).train()
    g = torch.Generator().manual_seed(1234)
    feats = {m: torch.randn(B, T, C, 1, 1, 1, generator=g).to(dev) for m, C in c["modal_dims"].items()}
    tgt = {"action": torch.randint(0, 3806, (B,), generator=g).to(dev)}
    sub = {"action": torch.randint(0, 3806, (B, T, 1), generator=g).to(dev)}
    tr = Trainer(model, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0})
    for _ in range(warm):
        tr.step(feats, tgt, sub)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        tr.step(feats, tgt, sub)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / n * 1e3
    cap = 4096
    _lib.check(_lib.lib().afft_kernel_trace_begin(cap), "kernel_trace_begin")
    loss = tr.step(feats, tgt, sub)[0]
    torch.cuda.synchronize()
    buf = (_lib.KernelTraceRec * cap)()
    nrec = _lib.lib().afft_kernel_trace_end(buf, cap)
    if nrec < 0:
        raise RuntimeError("afft_kernel_trace_end failed: " + _lib.lib().afft_last_error().decode())
    form = "generic" if os.environ.get("AFFT_ATTN_GENERIC") == "1" else "mfma"
    print(f"cfg5 streams, tsa fuser, T = {T} ({len(c['modal_dims']) * T} tokens), {B} clips, bf16 train step, {form}: {ms:.2f} ms / step "
          f"({n} steps after {warm}), loss {float(loss):.4f}")
    attn = 0.0
    for kind, name in ((_lib.K_ATTN_FWD, "attn_fwd"), (_lib.K_ATTN_BWD, "attn_bwd")):
        rows = {}
        for r in (buf[i] for i in range(nrec)):
            if r.kind == kind:
                e = rows.setdefault(r.rows, [0, 0.0])
                e[0] += 1
                e[1] += r.ms
        for nr, (cnt, t) in sorted(rows.items()):
            attn += t
            print(f"  {name} rows {nr:6d}: {cnt:2d} calls, {t * 1e3:8.1f} us in the traced step")
    print(f"  attention calls: {attn:.3f} ms = {100.0 * attn / ms:.1f} % of the step time", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=4, type=int)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.one:
        return one(*a.one)
    if a.step:
        return step()
    lines = []
    for shape in SHAPES:
        for generic in ("0", "1"):
            env = dict(os.environ, AFFT_ATTN_GENERIC=generic)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one"] + [str(x) for x in shape], env=env,
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:        # a child that died: report and start nothing more on the GPU
                print(r.stdout + r.stderr)
                sys.exit(f"attn_long: child for {shape} generic={generic} ended with {r.returncode}")
            print(r.stdout, end="", flush=True)
            lines.append(r.stdout)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        print(r.stdout + r.stderr)
        sys.exit(f"attn_long: the training-step child ended with {r.returncode}")
    print(r.stdout, end="", flush=True)
    lines.append(r.stdout)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/attn_long.py: (nseq, L, H, hd), bf16, block-causal period L/4, no dropout; one process per line pair\n")
            f.write("".join(lines))


if __name__ == "__main__":
    main()
