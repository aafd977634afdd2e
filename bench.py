#!/usr/bin/env python3
"""bench.py -- clips/sec (fwd+bwd) of the AFFT hot path on MI355X, BASELINE.json's metric.

    python bench.py [--gpus N] [--steps K] [--warmup W]          (N > 1 without a launcher: starts its own ranks, below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1] / SURVEY.md 8d "cfg2"): SA-Fuser, 4 modalities (rgb, objects, audio, flow)
x T=16 frames x d = D = 2048, depth 6 + 6 GPT-2 layers, 3806 classes, 64 clips per GPU, synthetic fp32 features
resident in HBM, train mode with the reference's dropout rates (0.1, classifier 0.2, DropPath linspace(0,0.1)).
One step = forward + 3-term loss + backward (+ bucketed gradient all-reduce for N > 1) + fused Nesterov-SGD update.
Weak scaling: per-GPU batch fixed.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up (--warmup W steps), times --steps K steps and prints the headline line (`value`, `ms_per_step` ...).
--full adds every side measurement (roofline, power, forward latency, parity precisions, other widths and batches, reference loop,
CPU baseline; for N > 1 the sharded leg and the communication report).  --dump-outputs DIR writes what the last timed step computed
as DIR/<name>.npy.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

GRAPH_AUTO: tuple = ()      # configurations replayed as a captured hipGraph under --graph auto (filled from measurements)
PEAK_BF16_TFLOPS = 2500.0   # dense bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="cfg2", help="cfg2 (default) | ek100 | cfg1 | cfg4 | cfg5 | cfg2_cm | cfg2_tsa")
    ap.add_argument("--batch", type=int, default=64, help="clips per GPU")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32", "bf16x3", "fp16x2"])
    ap.add_argument("--comm-dtype", default=None, choices=["bf16", "fp32"],
                    help="gradient all-reduce payload; default: bf16 beside --precision bf16 (whose gradients carry bf16 operand rounding anyway), fp32 "
                         "-- what the reference's DDP exchanges, train.py:364-368 -- beside every other precision")
    ap.add_argument("--comm-algo", default="allreduce", choices=["allreduce", "rs_ag", "sharded"],
                    help="gradient exchange per bucket of the HEADLINE step: one all-reduce + replicated update (default: what the north star and "
                         "train.py:364-368 name), reduce-scatter + all-gather of the gradient + replicated update, or 'sharded' (reduce-scatter, "
                         "update of the rank's 1 / N slice, all-gather of the 16-bit weight images).  With the default, N > 1 also times the "
                         "sharded step in the same job as `comm.sharded` (--no-sharded-leg skips it)")
    ap.add_argument("--no-sharded-leg", action="store_true", help="N > 1: do not time the sharded update beside the all-reduce headline")
    ap.add_argument("--side-leg-budget", type=float, default=None,
                    help="N > 1: seconds a side measurement (sharded leg, communication report, instrumented step) may take before rank 0 prints "
                         "the headline line as it stands and every rank exits (default 100: below --collective-timeout, whose watchdog would abort "
                         "the process; 1500 in a gloo / shared-GPU rehearsal, where buckets travel through the host)")
    ap.add_argument("--fallback-note", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--no-comm-report", action="store_true", help="N > 1: skip the RCCL / exposed-communication / payload side measurements")
    ap.add_argument("--no-optimizer", action="store_true", help="time fwd+loss+bwd(+all-reduce) only")
    ap.add_argument("--eval-drop", action="store_true", help="disable dropout (eval-mode layers) in the timed steps")
    ap.add_argument("--graph", default="auto", choices=["auto", "on", "off", "single"],
                    help="replay the step as one captured hipGraph (Trainer.capture); single GPU with the optimizer only; "
                         "auto = on for the configurations whose eager step is bound by the host's enqueue rate")
    ap.add_argument("--bucket-melems", type=int, default=32, help="gradient bucket size (Mi elements) of the all-reduce / SGD pipeline")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--cpu-batch", type=int, default=16, help="clips per CPU-baseline step on the bench workload (SURVEY.md 8d: 16)")
    ap.add_argument("--no-parity-mode", action="store_true", help="skip the fp16x2 / bf16x3 (1e-3-accurate) throughput / error side measurements")
    ap.add_argument("--full-rows", action="store_true",
                    help="run the SA-Fuser's last block on every token row as the reference does (default: its MLP half on token 0 only, "
                         "the only rows that reach an output; runtime.skip_dead_rows)")
    ap.add_argument("--launch-timeout", type=float, default=1500.0,
                    help="N > 1 started by bench.py itself: seconds after which the ranks are terminated and an error line is printed")
    ap.add_argument("--collective-timeout", type=float, default=120.0,
                    help="torch.distributed timeout (s): a rank that waits longer in a collective raises instead of hanging")
    ap.add_argument("--no-reference-loop", action="store_true",
                    help="skip the side measurement of the reference's own loop (Runner + MixUp + optimizer over 151 groups + lr scheduler)")
    ap.add_argument("--no-power", action="store_true", help="skip the package power / clock poll")
    ap.add_argument("--no-ek100", action="store_true", help="skip the side measurement at the EK100 widths of expts/01 (d = 1024)")
    ap.add_argument("--no-separate-update", action="store_true", help="N = 1: skip the leg with the per-bucket update kernel (profiling runs: one kernel mix)")
    ap.add_argument("--no-small-batch", action="store_true", help="skip the side measurement at the reference's per-GPU batch of 16 clips")
    ap.add_argument("--full", action="store_true",
                    help="run every side measurement after the headline (N = 1: separate-update leg, reference row set, instrumented step "
                         "and roofline, power, forward latency, parity precisions, EK100 widths, small batch, reference loop, CPU baseline; "
                         "N > 1: sharded leg, communication report, instrumented step); the --no-* switches above apply within it.  "
                         "Without it a run sets up, warms up, times --steps steps and prints the headline line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed to DIR/<name>.npy: its loss and loss terms "
                         "(float64) and a fixed, seeded sample of the parameters and momentum it left (float32; under --no-optimizer the "
                         "gradient averaged over the ranks instead of the momentum), so that two builds can be compared output for output")
    args = ap.parse_args()
    if args.comm_dtype is None:
        args.comm_dtype = "bf16" if args.precision == "bf16" else "fp32"
    return args


def _token_rows(args) -> bool:
    """does the step project only the token-0 rows in the SA-Fuser's last block (functional.attn_take_ok: composite path, frames % 64 == 0)"""
    from afft_amd.config import BASELINE_CONFIGS
    import afft_amd
    T = BASELINE_CONFIGS[args.config]["T"] if args.config in BASELINE_CONFIGS else 16
    return (afft_amd.runtime.skip_dead_rows() and afft_amd.runtime.composite() and args.precision in ("bf16", "fp16x2")
            and (args.batch * T) % 64 == 0)


def make_inputs(cfg, B, T, rank, device, ncls=3806):
    g = torch.Generator().manual_seed(1234 + rank)
    feats = {m: torch.randn(B, T, C, 1, 1, 1, generator=g).to(device) for m, C in cfg["modal_dims"].items()}
    tgt = torch.randint(0, ncls, (B,), generator=g)
    sub = torch.randint(0, ncls, (B, T, 1), generator=g)
    drop = torch.rand(B, T, 1, generator=g) < 0.10
    sub[drop] = -1
    return feats, {"action": tgt.to(device)}, {"action": sub.to(device)}


def build_model(name, device, drop=0.1):
    from afft_amd.config import BASELINE_CONFIGS, make_model_cfg
    from afft_amd.models.base_model import BaseModel
    c = BASELINE_CONFIGS[name]
    torch.manual_seed(42)   # conf/config.yaml:4
    cfg = make_model_cfg(c["modal_dims"], c["common_dim"], c["fp_inter_dim"], fuser=c["fuser"], T=c["T"], drop=drop,
                         modal_encoding=(c["fuser"] == "tsa"))
    model = BaseModel(cfg, num_classes={"action": 3806}, class_mappings={})
    return model.to(device), c


# ----------------------------------------------------------------------------- roofline of the dominant kernel
class GemmTimer:
    """The library's own measurement hook (afft_gemm_trace_begin / _end, include/afft_hip.h) around ONE instrumented step: a HIP
    event pair on the launch stream around every bf16 GEMM launch, whichever entry point it comes from (the composite
    sub-layer calls included), so the average launch duration of the dominant kernel and its algorithmic FLOPs per launch are
    measured live, on the same workload and the same kernel sequence as the timed region."""
    CAP = 4096

    def __enter__(self):
        from afft_amd import _lib
        self.lib = _lib
        _lib.check(_lib.lib().afft_gemm_trace_begin(self.CAP), "gemm_trace_begin")
        self.records = None
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        buf = (self.lib.GemmTraceRec * self.CAP)()
        n = self.lib.lib().afft_gemm_trace_end(buf, self.CAP)
        if n < 0:
            raise RuntimeError("afft_gemm_trace_end failed: " + self.lib.lib().afft_last_error().decode())
        self.records = [buf[i] for i in range(n)]

    @staticmethod
    def symbol(r) -> str:
        b = lambda x: "true" if x else "false"    # noqa: E731
        x3 = 2 if int(r.split3) == 4 else int(r.split3)      # one fp16 pass (split3 = 4) runs the two-pass instantiation over one segment
        if r.variant == 3:
            return f"gemm_bf16_pp_kernel<{b(r.a_kstrided)}, {b(r.b_kstrided)}, {x3}>"
        if r.variant == 13:      # round 6: the steady-state 256x256 kernel (whole tiles, even K-tile count, plain bf16)
            return f"gemm_bf16_pp2_kernel<{b(r.a_kstrided)}, {b(r.b_kstrided)}, {x3}>"
        if r.variant in (7, 8, 9, 10):       # B-direct kernels (csrc/gemm_bd.hip): <16-row blocks per tile, A look-ahead, B look-ahead, packed B>
            return f"gemm_bf16_bd_kernel<{10 if r.variant in (8, 10) else 16}, 3, {2 if r.variant in (8, 10) else 1}, {b(r.variant >= 9)}>"
        return f"gemm_bf16_kernel<2, 2, 2, {b(r.a_kstrided)}, {b(r.b_kstrided)}, {b(r.splitk > 1)}, {x3}>"

    def summary(self):
        out = {}
        for r in self.records:
            d = out.setdefault(self.symbol(r), {"launches": 0, "flops": 0.0, "ms": 0.0, "fused_update_launches": 0, "bytes": 0.0})
            d["launches"] += 1
            d["flops"] += 2.0 * r.M * r.N * r.K
            # algorithmic HBM bytes: both bf16 operands once + the output -- bf16 activations (2 B), an fp32 weight gradient
            # (4 B), or, with the optimizer in the epilogue, parameter and momentum read and written plus the bf16 image (18 B)
            wgrad = r.a_kstrided and r.b_kstrided
            d["bytes"] += 2.0 * r.K * (r.M + r.N) + r.M * r.N * (18.0 if r.fused_update else 4.0 if wgrad else 2.0)
            d["ms"] += r.ms
            d["fused_update_launches"] += r.fused_update
        return out


def by_k_class(records, symbol, mfma_peak_tflops, hbm_peak_gbs=8000.0):
    """The launches of one kernel symbol split by their reduction length K: the weight-gradient symbol holds the fuser's K = B*T*S
    = 5120-row reductions (MFMA-bound) and the predictor's K = B*T = 1024-row ones, whose 18-20 B / parameter optimizer epilogue
    moves more bytes than their MFMA work hides (arithmetic intensity below the ridge peak_flops / peak_bytes: HBM-bound).  Each
    class is priced against the roof that bounds IT: frac = achieved / peak of `bound`."""
    ridge = mfma_peak_tflops * 1e12 / (hbm_peak_gbs * 1e9)      # FLOP per byte
    cls = {}
    for r in records:
        if GemmTimer.symbol(r) != symbol:
            continue
        d = cls.setdefault(int(r.K), {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0, "shapes": {}})
        wgrad = r.a_kstrided and r.b_kstrided
        d["launches"] += 1
        d["ms"] += r.ms
        d["flops"] += 2.0 * r.M * r.N * r.K
        d["bytes"] += 2.0 * r.K * (r.M + r.N) + r.M * r.N * (18.0 if r.fused_update else 4.0 if wgrad else 2.0)
        key = f"{r.M}x{r.N}"
        d["shapes"][key] = d["shapes"].get(key, 0) + 1
    out = {}
    for K, d in sorted(cls.items()):
        if d["ms"] <= 0:
            continue
        tf, gbs, ai = d["flops"] / (d["ms"] * 1e-3) / 1e12, d["bytes"] / (d["ms"] * 1e-3) / 1e9, d["flops"] / d["bytes"]
        hbm = ai < ridge
        out[f"K={K}"] = {"launches": d["launches"], "avg_us": round(d["ms"] / d["launches"] * 1e3, 1), "shapes_MxN": d["shapes"],
                         "flop_per_byte": round(ai, 1), "bound": "hbm" if hbm else "mfma",
                         "achieved": round(gbs if hbm else tf, 1), "peak": hbm_peak_gbs if hbm else mfma_peak_tflops,
                         "unit": "GB/s" if hbm else "TFLOP/s", "frac": round((gbs / hbm_peak_gbs) if hbm else (tf / mfma_peak_tflops), 4),
                         "tflops": round(tf, 1), "algorithmic_gbs": round(gbs, 1)}
    return {"ridge_flop_per_byte": round(ridge, 1), "classes": out,
            "note": "bytes = both 16-bit operands once + the result (18 B per parameter with the optimizer in the epilogue: p and momentum read and written, "
                    "the bf16 image written; +2 B where a packed or FP16 image is kept), from the same HIP-event records as `achieved`"}


class KernelTimer:
    """The same hook for the HBM-bound kernels (afft_kernel_trace_begin / _end): attention and LayerNorm calls of one
    instrumented step, each bracketed by a HIP event pair on its stream, with the call's algorithmic bytes and FLOPs."""
    CAP = 4096
    NAMES = {1: "attn_fwd", 2: "attn_bwd", 3: "ln_fwd", 4: "ln_bwd"}

    def __enter__(self):
        from afft_amd import _lib
        self.lib = _lib
        _lib.check(_lib.lib().afft_kernel_trace_begin(self.CAP), "kernel_trace_begin")
        self.records = None
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        buf = (self.lib.KernelTraceRec * self.CAP)()
        n = self.lib.lib().afft_kernel_trace_end(buf, self.CAP)
        if n < 0:
            raise RuntimeError("afft_kernel_trace_end failed: " + self.lib.lib().afft_last_error().decode())
        self.records = [buf[i] for i in range(n)]

    def summary(self):
        out = {}
        for r in self.records:
            d = out.setdefault(self.NAMES.get(r.kind, str(r.kind)), {"launches": 0, "ms": 0.0, "bytes": 0.0, "flops": 0.0, "by_rows": {}})
            d["launches"] += 1
            d["ms"] += r.ms
            d["bytes"] += r.bytes
            d["flops"] += r.flops
            e = d["by_rows"].setdefault(r.rows, [0, 0.0])
            e[0] += 1
            e[1] += r.ms
        return out


def hbm_kernel_report(in_step, alone):
    """achieved HBM GB/s of the attention / LayerNorm kernels (algorithmic bytes / HIP-event time of the call), inside the
    two-stream step and with every kernel alone on the chip, against the 8 TB/s peak of the guide"""
    rep = {}
    for name, d in in_step.items():
        a = (alone or {}).get(name)
        gbs = d["bytes"] / (d["ms"] * 1e-3) / 1e9 if d["ms"] > 0 else None
        rep[name] = {"launches_per_step": d["launches"], "avg_us_in_step": round(d["ms"] / d["launches"] * 1e3, 1),
                     "gbs_in_step": round(gbs, 0) if gbs else None, "frac_of_hbm_peak_in_step": round(gbs / PEAK_HBM_GBS, 3) if gbs else None,
                     "avg_us_alone": round(a["ms"] / a["launches"] * 1e3, 1) if a and a["launches"] else None,
                     "gbs_alone": round(a["bytes"] / (a["ms"] * 1e-3) / 1e9, 0) if a and a["ms"] > 0 else None,
                     "algorithmic_mb_per_launch": round(d["bytes"] / d["launches"] / 1e6, 1)}
        if d["flops"]:
            rep[name]["tflops_in_step"] = round(d["flops"] / (d["ms"] * 1e-3) / 1e12, 1)
    return rep


def sublayer_report(gemm_records, kern, c, B):
    """The north-star's "fused-attention kernel" is a REGION here -- LN -> QKV GEMM -> packed-frame attention -> projection +
    bias + dropout + residual, one composite C-ABI call, 4 kernels -- so its MFMA utilisation is reported for the region:
    FLOPs of its GEMMs and of the attention MFMAs over the summed HIP-event durations of its kernels inside the instrumented
    step, forward and backward (data-gradient chain; the weight gradients run on the auxiliary stream and are listed apart),
    for the fuser's full-row blocks (R = B * T * S rows).  Same for the MLP sub-layer."""
    T, d = c["T"], c["common_dim"]
    S = len(c["modal_dims"]) + 1
    R = B * T * S

    def gemm(layout, M, N, K):
        a_ks, b_ks = {"nt": (0, 0), "nn": (0, 1), "tn": (1, 1)}[layout]
        rs = [r for r in gemm_records if (r.M, r.N, r.K, r.a_kstrided, r.b_kstrided) == (M, N, K, a_ks, b_ks)]
        if not rs:
            return None
        return sum(r.ms for r in rs) / len(rs), 2.0 * M * N * K, len(rs)

    def kern_avg(name, rows):
        e = kern.get(name, {}).get("by_rows", {}).get(rows)
        if not e:
            return None
        fl = kern[name]["flops"] / kern[name]["launches"] if kern[name]["launches"] else 0.0
        return e[1] / e[0], fl, e[0]

    def region(parts):
        if any(p is None for p in parts):
            return None
        ms, fl = sum(p[0] for p in parts), sum(p[1] for p in parts)
        return {"us": round(ms * 1e3, 1), "gflop": round(fl / 1e9, 1), "tflops": round(fl / (ms * 1e-3) / 1e12, 1),
                "frac_of_mfma_peak": round(fl / (ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4)}

    rep = {"rows": R, "d": d,
           "attention_fwd": region([kern_avg("ln_fwd", R), gemm("nt", R, 3 * d, d), kern_avg("attn_fwd", R), gemm("nt", R, d, d)]),
           "attention_bwd_chain": region([gemm("nn", R, d, d), kern_avg("attn_bwd", R), gemm("nn", R, d, 3 * d), kern_avg("ln_bwd", R)]),
           "attention_wgrads_aux_stream": region([gemm("tn", d, d, R), gemm("tn", 3 * d, d, R)]),
           "mlp_fwd": region([kern_avg("ln_fwd", R), gemm("nt", R, 4 * d, d), gemm("nt", R, d, 4 * d)]),
           "mlp_bwd_chain": region([gemm("nn", R, 4 * d, d), gemm("nn", R, d, 4 * d), kern_avg("ln_bwd", R)]),
           "mlp_wgrads_aux_stream": region([gemm("tn", d, 4 * d, R), gemm("tn", 4 * d, d, R)]),
           "note": "kernel-time based (sum of HIP-event durations of the region's launches inside the instrumented two-stream step); "
                   "LN rows = the region's own LayerNorm; backward chains exclude the weight-gradient GEMMs, which overlap them on the "
                   "auxiliary stream with the optimizer in their epilogues"}
    return rep


def _cpu_steps(name, B, steps):
    """seconds per fwd + loss + bwd step of the oracle on cfg `name` at batch B: 1 warm-up + `steps` timed, median"""
    from oracle import afft_oracle as O
    from afft_amd.config import BASELINE_CONFIGS
    c = BASELINE_CONFIGS[name]
    model, _ = build_model(name, "cpu", drop=0.0)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    del model
    feats, tgt, sub = make_inputs(c, B, c["T"], 0, "cpu")
    ocfg = dict(fuser=c["fuser"], depth=6, num_heads=4, fp_layers=6, fp_heads=4, fp_output_len=1,
                num_classes={"action": 3806})
    times = []
    for i in range(steps + 1):
        for p in P.values():
            p.grad = None
        t0 = time.perf_counter()
        out = O.base_model_forward(P, feats, ocfg)
        total, _ = O.loss(out, tgt["action"], sub["action"])
        total.backward()
        times.append(time.perf_counter() - t0)
    times = sorted(times[1:])
    return times[len(times) // 2]


def cpu_baseline(name, B, steps=3):
    """The oracle (CPU restatement, proven equal to the reference: tests/test_oracle_golden.py) timed on this host's cores
    on a bounded sample of the same workload: fwd + loss + bwd, eval-mode math, cfg1 (B = 4) and the bench
    configuration (B = 16), 1 warm-up + >= 3 timed steps, at the best intra-op thread count of a short sweep on cfg1."""
    ncpu = os.cpu_count() or 1
    # measured on the GPU box (2 x 64 cores, 256 threads): 16 intra-op threads are the best (13.7 clips/s on cfg1), 64 lose 2.6x
    # and oversubscribing all 256 logical cores is 700x slower -- so the sweep stays at or below 64
    cands = sorted({t for t in (8, 16, 32, 64) if 1 <= t <= ncpu}) or [1]
    sweep = {}
    for t in cands:
        torch.set_num_threads(t)
        sweep[t] = round(4 / _cpu_steps("cfg1", 4, 2), 2)
    best = max(sweep, key=sweep.get)
    torch.set_num_threads(best)
    cfg1 = 4 / _cpu_steps("cfg1", 4, steps)
    t = _cpu_steps(name, B, steps)
    return {"value": round(B / t, 3), "unit": "clips/s", "cores": best, "kind": "port",
            "sample": f"{name} B={B}: 1 warm-up + {steps} timed fwd+loss+bwd steps of oracle/afft_oracle.py (torch fp32 CPU, "
                      f"{best} intra-op threads of {ncpu} logical cores, the best of the sweep), median",
            "cfg1_B4_clips_s": round(cfg1, 3), "thread_sweep_cfg1_clips_s": {str(k): v for k, v in sweep.items()}}


def _power_probe():
    """A function () -> (package power in W, graphics clock in MHz) of THE GPU THIS PROCESS USES, read IN PROCESS -- sysfs (amdgpu
    hwmon), else the amdsmi Python binding -- or None.  No child process: `rocm-smi` is a `#!/usr/bin/env python3` script, i.e. two
    exec hops from a process that has initialised the GPU (and, under rocprofv3, inherited the profiler's preloaded library) -- what
    this pool forbids -- and 20 forks per second pollute a profiled run.  The device is matched by its PCI address: a box shows
    every card of the node in sysfs, the process sees one."""
    import glob
    try:
        pr = torch.cuda.get_device_properties(torch.cuda.current_device())
        bdf = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
    except Exception:  # noqa: BLE001
        return None, None
    for card in sorted(glob.glob("/sys/class/drm/card[0-9]*")):
        devdir = os.path.join(card, "device")
        if os.path.basename(os.path.realpath(devdir)).lower() != bdf:
            continue
        for hw in sorted(glob.glob(os.path.join(devdir, "hwmon", "hwmon*"))):
            pw = next((os.path.join(hw, f) for f in ("power1_average", "power1_input") if os.path.exists(os.path.join(hw, f))), None)
            fq = os.path.join(hw, "freq1_input")
            if pw is None or not os.path.exists(fq):
                continue

            def read(pw=pw, fq=fq):
                return float(open(pw).read()) / 1e6, int(open(fq).read()) // 1_000_000
            try:
                read()
                return read, f"sysfs hwmon of {bdf} (power1_average / freq1_input)"
            except Exception:  # noqa: BLE001
                continue
    try:
        import amdsmi
        amdsmi.amdsmi_init()
        h = next(x for x in amdsmi.amdsmi_get_processor_handles() if str(amdsmi.amdsmi_get_gpu_device_bdf(x)).lower() == bdf)

        def read():
            p = amdsmi.amdsmi_get_power_info(h)
            w = p.get("current_socket_power", p.get("average_socket_power"))
            c = amdsmi.amdsmi_get_clock_info(h, amdsmi.AmdSmiClkType.GFX)
            return float(w), int(c.get("clk", c.get("cur_clk")))
        read()
        return read, f"amdsmi Python binding, {bdf}"
    except Exception:  # noqa: BLE001
        return None, None


def power_report(step_fn, seconds=2.5):
    """Package power and graphics clock while the training step loops (polled in process from a thread, after the timed region:
    the timing above is not perturbed).  The GEMM loops of this path run at the package power limit (profiles/r04_power.txt), so
    the line says at which clock and power the number above was made.  An error entry when neither source is there."""
    import threading
    smi, source = _power_probe()
    if smi is None:
        return {"error": "no in-process power source (amdgpu hwmon in sysfs, amdsmi binding)"}
    stop, samples = threading.Event(), []

    def poll():
        while not stop.is_set():
            try:
                samples.append(smi())
            except Exception:  # noqa: BLE001
                pass
            time.sleep(0.05)
    th = threading.Thread(target=poll)
    th.start()
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        step_fn()
        n += 1
        if n % 4 == 0:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    stop.set()
    th.join()
    pw = sorted(s[0] for s in samples if s[0] is not None)
    ck = sorted(s[1] for s in samples if s[1] is not None)
    if not pw or not ck:
        return {"error": "no samples"}
    return {"samples": len(pw), "package_power_w_avg": round(sum(pw) / len(pw), 1), "package_power_w_max": pw[-1],
            "sclk_mhz_median": ck[len(ck) // 2], "sclk_mhz_max_of_part": 2400, "ms_per_step_while_polled": round(dt * 1e3, 3),
            "source": source,
            "note": "polled every 50 ms over a separate loop of the same step; GEMM loops alone sit at ~1375 W (profiles/r04_power.txt)"}


def parity_side_measurements(args, device, feats, tgt, sub, c):
    """What the precision of the headline number costs, on the record: throughput of the 1e-3-accurate mode
    (bf16x3: fp32-grade GEMMs from three bf16 MFMA passes) on the same workload and step definition, and the relative L2
    error of each mode's logits against the exact-fp32 mode (itself within 1e-6 of the oracle: tests/test_model_gpu.py) on
    8 clips of the same synthetic input, eval mode."""
    import afft_amd
    from afft_amd.parallel import Trainer
    wts = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
    out = {}
    small = {m: f[:8].contiguous() for m, f in feats.items()}
    ts, ss = {"action": tgt["action"][:8].contiguous()}, {"action": sub["action"][:8].contiguous()}
    logits = {}
    fwd_ms = {}
    for mode in ("fp32", "bf16x3", "fp16x2", "bf16"):
        afft_amd.set_precision(mode)
        model, _ = build_model(args.config, device)
        model.eval()
        with torch.no_grad():
            o, _ = model(small, mixup_fn=None, target=ts, target_subclips=ss, target_subclips_ignore_index=None)
            logits[mode] = o["logits/action"]["all-fused"].double()
            if mode != "fp32":       # the evaluation forward of the full batch: what a parity-grade test / validation pass costs
                for _ in range(2):
                    model(feats, mixup_fn=None, target=tgt, target_subclips=sub, target_subclips_ignore_index=None)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(5):
                    model(feats, mixup_fn=None, target=tgt, target_subclips=sub, target_subclips_ignore_index=None)
                torch.cuda.synchronize()
                fwd_ms[mode] = round((time.perf_counter() - t0) / 5 * 1e3, 2)
        del o
        if mode in ("bf16x3", "fp16x2"):
            model.train(not args.eval_drop)
            tr = Trainer(model, wts, bucket_elems=args.bucket_melems * 1024 * 1024)
            for _ in range(3):
                tr.step(feats, tgt, sub)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 10
            for _ in range(n):
                tr.step(feats, tgt, sub)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / n
            last_loss = float(tr.step(feats, tgt, sub)[0])
            with GemmTimer() as gt:       # the MFMA passes this step really runs, from the library's own launch records
                tr.step(feats, tgt, sub)
            w = {0: 1.0, 1: 3.0, 2: 2.0, 3: 1.5, 4: 1.0}      # split3: bf16 | bf16x3 | two fp16 passes | fp16 + fp8 (twice the rate) | one fp16 pass
            traced_passes = sum(2.0 * r.M * r.N * r.K * w[int(r.split3)] for r in gt.records) / max(1.0, sum(2.0 * r.M * r.N * r.K for r in gt.records))
            from afft_amd.config import gflop_per_clip
            useful = args.batch / dt * gflop_per_clip(args.config, fwd_bwd=True, executed=afft_amd.runtime.skip_dead_rows(), token_row_projection=_token_rows(args)) / 1e3   # TFLOP/s executed
            if mode == "bf16x3":
                # three bf16 MFMA passes per product, forward and backward: fp32-grade gradients too (1.4e-5 / 2.8e-5)
                passes, note = 3.0, "bf16x3: hi*hi + lo*hi + hi*lo on the bf16 MFMAs in every GEMM of the step"
            else:
                # forward two fp16 MFMA passes (activation hi + lo, weight rounded once), backward one bf16 pass: the step's GEMM work
                # is (2 + 2) / 3 of the algorithmic FLOPs (backward = 2 x forward)
                sites = sorted(afft_amd.runtime.one_pass_sites())
                passes, note = traced_passes, ("fp16x2: forward A_hi W + A_lo W (fp16 MFMA; the lo pass on the block-scaled fp8 MFMA at twice the rate where the "
                                               "256x256 kernel runs) with the operand planes written by the producing kernels; ONE fp16 pass at the sites "
                                               f"{', '.join(sites) or '(none)'} (runtime.one_pass_sites, tools/lo_pass_sweep.py); backward = the bf16 mode's on "
                                               "bf16 copies (gradients inside the bf16 bound).  passes = bf16-rate MFMA passes per algorithmic FLOP, from "
                                               "the GEMM launch records of one step")
            rec = {"precision": mode, "clips_per_s": round(args.batch / dt, 1), "ms_per_step": round(dt * 1e3, 2), "steps": n,
                   "final_loss": round(last_loss, 4) if last_loss == last_loss else "nan: MEASUREMENT VOID (updates skipped)",
                   "roofline": {"bound": "mfma", "achieved": round(useful, 1), "peak": round(PEAK_BF16_TFLOPS / passes, 1),
                                "unit": "TFLOP/s (algorithmic, whole step)", "frac": round(useful * passes / PEAK_BF16_TFLOPS, 4),
                                "executed_tflops": round(passes * useful, 1), "passes": round(passes, 3)},
                   "note": note}
            # the mode whose LOGITS meet the north-star 1e-3 at the highest training rate is the parity mode of the line
            if mode == "fp16x2":
                rec["one_pass_sites"] = sorted(afft_amd.runtime.one_pass_sites())
            out["parity_mode" if mode == "fp16x2" else "parity_mode_bf16x3"] = rec
            del tr
        del model
        torch.cuda.empty_cache()
    ref = logits["fp32"]
    out["logits_rel_l2_vs_exact_fp32_mode"] = {m: float(((logits[m] - ref).norm() / ref.norm()).cpu()) for m in ("bf16", "bf16x3", "fp16x2")}
    if "parity_mode" in out:
        out["parity_mode"]["logits_rel_l2_vs_exact_fp32_mode"] = out["logits_rel_l2_vs_exact_fp32_mode"]["fp16x2"]
    out["eval_forward_ms"] = {"batch": args.batch, **fwd_ms}
    afft_amd.set_precision(args.precision)
    return out


def ek100_side_measurement(args, device):
    """The metric's namesake at its own widths (expts/01_SA-Fuser_ek100_train.txt: rgb / audio / flow 1024, objects 352, d = 1024,
    D = 2048 -- config 'ek100'), same batch, step definition and precision as the headline: clips/s, ms/step and the whole-step
    fraction of the dense MFMA peak.  (The headline workload is BASELINE configs[1], every width 2048.)"""
    import afft_amd
    from afft_amd.config import gflop_per_clip
    from afft_amd.parallel import Trainer
    model, c = build_model("ek100", device)
    B, T = args.batch, c["T"]
    feats, tgt, sub = make_inputs(c, B, T, 0, device)
    tr = Trainer(model, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, bucket_elems=args.bucket_melems * 1024 * 1024)
    model.train(not args.eval_drop)
    for _ in range(5):
        tr.step(feats, tgt, sub)
    torch.cuda.synchronize()
    n = 20
    t0 = time.perf_counter()
    for _ in range(n):
        tr.step(feats, tgt, sub)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    last_loss = float(tr.step(feats, tgt, sub)[0])
    gf = gflop_per_clip("ek100", fwd_bwd=True, executed=afft_amd.runtime.skip_dead_rows(), token_row_projection=_token_rows(args))
    tf = B / dt * gf / 1e3
    del tr, model
    torch.cuda.empty_cache()
    return {"clips_per_s": round(B / dt, 1), "ms_per_step": round(dt * 1e3, 3), "steps": n, "batch": B, "precision": args.precision,
            "final_loss": round(last_loss, 4) if last_loss == last_loss else "nan: MEASUREMENT VOID (updates skipped)",
            "gflop_per_clip_executed": round(gf, 2), "tflops": round(tf, 1), "frac_of_mfma_peak": round(tf / PEAK_BF16_TFLOPS, 4),
            "workload": "ek100: SA-Fuser 4-modality T=16 d=1024 (objects 352) D=2048 depth 6+6, 3806 classes, train mode, eager"}


def small_batch_measurement(args, device, B=16):
    """The bench workload at the reference's own per-GPU batch (expts/01_SA-Fuser_ek100_train.txt:7 trains with 16 clips per GPU): the
    step is then bound by streaming the 614 M parameters, not by MFMA work -- per parameter and step 2 B (bf16 image, forward) + 2 B (data
    gradient) + 18 B (optimizer inside the weight-gradient epilogue: parameter and momentum read and written, image written) -- so it is
    priced against the HBM roof.  (Activations add < 3 % at this batch and are left out of the algorithmic bytes.)"""
    import afft_amd
    from afft_amd.parallel import Trainer
    model, c = build_model(args.config, device)
    feats, tgt, sub = make_inputs(c, B, c["T"], 0, device)
    tr = Trainer(model, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, bucket_elems=args.bucket_melems * 1024 * 1024)
    model.train(not args.eval_drop)
    for _ in range(6):
        tr.step(feats, tgt, sub)
    torch.cuda.synchronize()
    n = 20
    t0 = time.perf_counter()
    for _ in range(n):
        tr.step(feats, tgt, sub)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    host = []
    for _ in range(8):      # the host's enqueue time per step (nothing waits for the GPU inside a step): what bounds the step from the other side
        h0 = time.perf_counter()
        tr.step(feats, tgt, sub)
        host.append((time.perf_counter() - h0) * 1e3)
    torch.cuda.synchronize()
    last_loss = float(tr.step(feats, tgt, sub)[0])
    params = tr.flat.total
    nbytes = params * 22.0
    del tr, model
    torch.cuda.empty_cache()
    return {"batch": B, "clips_per_s": round(B / dt, 1), "ms_per_step": round(dt * 1e3, 3), "steps": n,
            "host_enqueue_ms_p50": round(sorted(host)[len(host) // 2], 2),
            "final_loss": round(last_loss, 4) if last_loss == last_loss else "nan: MEASUREMENT VOID (updates skipped)",
            "roofline": {"bound": "hbm", "achieved": round(nbytes / dt / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                         "frac": round(nbytes / dt / 1e9 / PEAK_HBM_GBS, 4), "algorithmic_bytes_per_step": int(nbytes),
                         "note": "22 B per parameter and step (2 forward image + 2 data gradient + 18 optimizer epilogue) x %d parameters" % params},
            "workload": f"{args.config} at the reference's per-GPU batch of {B} clips (expts/01_SA-Fuser_ek100_train.txt:7), train mode, eager"}


def reference_loop_measurements(args, device, feats, tgt, sub, c, trainer_ms):
    """What a user of the reference's UNCHANGED loop gets, on the bench workload, beside the headline number --
    train.py:228-265 with the recipe of expts/01 (train.use_mixup=true, mixup_backbone=true, mixup_alpha 0.1, label smoothing
    0.4, SGD momentum 0.9 nesterov over the 151 per-parameter groups of prepare_params, Warmup(CosineLR) stepped per iteration):

        loss, metrics = Runner(model, device, wts)(batch, mixup_fn, True)       # host syncs as the reference has them
        optimizer.zero_grad(); loss.backward(); optimizer.step(); lr_scheduler.step()

    with (a) torch.optim.SGD and gradients through autograd (AFFT_GRAD_MODE=autograd: what works below torch's own DDP),
    (b) torch.optim.SGD on the default gradient sink, (c) afft_amd.optim.SGD (Hydra: opt.optimizer._target_=afft_amd.optim.SGD)
    with the reference's synchronous Runner and (d) the same with Runner(async_metrics=True); and Trainer.step with MixUp."""
    import afft_amd
    from afft_amd import dropout as D_
    from afft_amd.common.mixup import MixUp
    from afft_amd.common.runner import Runner
    from afft_amd.common.scheduler import CosineLR, Warmup, prepare_params
    from afft_amd.optim import SGD as AfftSGD
    from afft_amd.parallel import Trainer
    wts = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
    B = args.batch
    batch = ({"data_dict": feats, "target": tgt, "target_subclips": sub}, {})
    n_warm, n_timed = 4, 10
    out = {"steps": n_timed, "recipe": "expts/01: MixUp(alpha 0.1, label smoothing 0.4, mixup_backbone) + SGD(momentum 0.9, nesterov, lr 1e-3, "
                                       "wd 1e-6) over prepare_params' per-parameter groups + Warmup(CosineLR) per iteration"}

    def run(kind):
        D_.manual_seed(42)
        afft_amd.set_grad_mode("autograd" if kind == "torch_sgd_autograd" else "sink")
        model, _ = build_model(args.config, device)
        model.train(not args.eval_drop)
        mix = MixUp(alpha=0.1, label_smoothing={"action": 0.4}, num_classes={"action": 3806})
        if kind == "trainer_mixup":
            tr = Trainer(model, wts, bucket_elems=args.bucket_melems * 1024 * 1024)
            step = lambda: tr.step(feats, tgt, sub, mixup_fn=mix)      # noqa: E731
            info = {}
        else:
            groups = prepare_params(model, None, 1e-3, 1e-6)
            if kind.startswith("torch_sgd"):
                opt = torch.optim.SGD(groups, lr=1e-3, momentum=0.9, nesterov=True)
            else:
                opt = AfftSGD(groups, lr=1e-3, momentum=0.9, nesterov=True, bucket_elems=args.bucket_melems * 1024 * 1024)
            sched = Warmup(opt, CosineLR(opt, num_epochs=30, iters_per_epoch=1000, world_size=1, eta_min=1e-6), init_lr_ratio=0.01,
                           num_epochs=20, iters_per_epoch=1000, world_size=1)
            # torch_sgd_*: the reference's blocking fetches inside the runner call; afft_sgd: our Runner's default (lazy host values:
            # the same keys, waited for at their first use); afft_sgd_async: one PendingScalars object
            runner = Runner(model, device, wts, async_metrics=(True if kind == "afft_sgd_async" else False if kind.startswith("torch_sgd") else None))
            info = {"param_groups": len(opt.param_groups)}

            def step():
                loss, metrics = runner(batch, mix, True)
                opt.zero_grad()
                loss.backward()
                opt.step()
                sched.step()
                # train.py:278 metric_tracker.update(metrics, ...): every value is consumed on the host at the end of the iteration
                for k, v in metrics.items():
                    if isinstance(v, dict):
                        for a in v.values():
                            float(__import__("numpy").asarray(a).reshape(-1)[0])
                    elif hasattr(v, "result"):
                        v.result()
                    elif not isinstance(v, torch.Tensor):      # accuracies stay device tensors in the reference's meters too (val * n, +=)
                        float(v)
                return loss, metrics
        for _ in range(n_warm):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_timed):
            r = step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n_timed
        info.update({"clips_per_s": round(B / dt, 1), "ms_per_step": round(dt * 1e3, 3)})
        if kind.startswith("afft_sgd"):
            info["optimizer_path"] = "fused-epilogue" if opt._fused else "separate"
            info["lr_seen_by_kernels"] = opt.opt.lr if opt.opt.hyper is None else "per-parameter"
        del r
        return info

    try:
        for kind in ("torch_sgd_autograd", "torch_sgd_sink", "afft_sgd", "afft_sgd_async", "trainer_mixup"):
            try:
                out[kind] = run(kind)
            except Exception as ex:  # noqa: BLE001
                out[kind] = {"error": repr(ex)}
            torch.cuda.empty_cache()
    finally:
        afft_amd.set_grad_mode("sink")
    if "ms_per_step" in out.get("afft_sgd", {}):
        out["afft_sgd_vs_trainer_step"] = round(out["afft_sgd"]["ms_per_step"] / trainer_ms, 4)
    return out


def comm_report(args, trainer, feats, tgt, sub, world, rank, device, ms_with_comm, rccl_log, sync_all, n_noexch=10, n_payload=20):
    """N > 1 side measurements, every rank takes part (collectives inside): what the gradient exchange costs and what the
    library does for it.  (a) exposed communication = ms/step with the exchange - ms/step of the same ranks stepping without
    it (buckets handed straight to the optimizer); (b) loss after 20 steps from the same start with fp32 and with bf16
    gradient payloads (the reference all-reduces fp32, train.py:364-368); (c) RCCL's own words on topology / algorithm /
    protocol, from its debug file."""
    from afft_amd.parallel import Trainer
    import afft_amd
    rep = {"world_size": dist.get_world_size(), "backend": dist.get_backend(), "buckets": len(trainer.reducer.buckets),
           "bucket_mib": round(4 * max(e - s for s, e in trainer.reducer.buckets) / 2 ** 20, 1),
           "payload_gb_per_step": round(trainer.flat.total * (2 if args.comm_dtype == "bf16" else 4) / 1e9, 3)}
    # (a) the same ranks without the exchange (replicas diverge from here on: this runs after the timed region)
    was = trainer.reducer.comm
    fused_was = afft_amd.runtime.fused_sgd()
    afft_amd.runtime.set_fused_sgd(False)     # same kernels as the step with the exchange (the fused update is single-GPU only)
    trainer.reducer.comm = False
    for _ in range(3):
        trainer.step(feats, tgt, sub)
    sync_all()
    t0 = time.perf_counter()
    n = n_noexch
    for _ in range(n):
        trainer.step(feats, tgt, sub)
    sync_all()
    t = torch.tensor([(time.perf_counter() - t0) / n * 1e3], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    trainer.reducer.comm = was
    afft_amd.runtime.set_fused_sgd(fused_was)
    rep["ms_per_step_without_exchange"] = round(float(t), 3)
    rep["exposed_comm_ms"] = round(ms_with_comm - float(t), 3)
    # (b) payload precision: two fresh replicas of the model, 20 steps each
    wts = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
    losses = {}
    for cd in ("fp32", "bf16"):
        from afft_amd import dropout as D_
        D_.manual_seed(42 + rank)
        m, _ = build_model(args.config, device)
        m.train(not args.eval_drop)
        tr = Trainer(m, wts, comm_dtype=cd, bucket_elems=args.bucket_melems * 1024 * 1024, comm_algo=args.comm_algo)
        for _ in range(n_payload):
            loss, _ = tr.step(feats, tgt, sub)
        lt = loss.detach().double().reshape(1).clone()
        dist.all_reduce(lt)
        losses[cd] = float(lt) / world
        del tr, m
        torch.cuda.empty_cache()
    rep["loss_after_%d_steps" % n_payload] = {k: round(v, 5) for k, v in losses.items()}
    rep["loss_delta_bf16_vs_fp32_payload"] = round(losses["bf16"] - losses["fp32"], 6)
    # (b2) what the exchange itself achieves: every bucket's collective alone, in the payload dtype, 5 timed repeats each --
    # algorithm bandwidth = bytes / time, bus bandwidth = 2 (n - 1) / n of it (what a ring moves per link; xGMI: 7 links x ~153 GB/s)
    try:
        pay = torch.bfloat16 if args.comm_dtype == "bf16" else torch.float32
        per_bucket = []
        for (s0, e0) in trainer.reducer.buckets:
            buf = torch.zeros(e0 - s0, dtype=pay, device=device)
            for _ in range(2):
                trainer.reducer._reduce(buf)
            sync_all()
            t1 = time.perf_counter()
            for _ in range(5):
                trainer.reducer._reduce(buf)
            sync_all()
            dt = torch.tensor([(time.perf_counter() - t1) / 5], dtype=torch.float64, device=device)
            dist.all_reduce(dt, op=dist.ReduceOp.MAX)
            gb = buf.numel() * buf.element_size() / 1e9
            per_bucket.append({"mib": round(gb * 1e9 / 2 ** 20, 1), "ms": round(float(dt) * 1e3, 3), "algbw_gbs": round(gb / float(dt), 1),
                               "busbw_gbs": round(gb / float(dt) * 2 * (world - 1) / world, 1)})
            del buf
        rep["allreduce_per_bucket"] = per_bucket
        tot_gb = sum(b["mib"] for b in per_bucket) * 2 ** 20 / 1e9
        tot_s = sum(b["ms"] for b in per_bucket) / 1e3
        rep["allreduce_alone_ms_per_step"] = round(tot_s * 1e3, 3)
        rep["allreduce_busbw_gbs"] = round(tot_gb / tot_s * 2 * (world - 1) / world, 1) if tot_s > 0 else None
    except Exception as ex:  # noqa: BLE001
        rep["allreduce_per_bucket"] = {"error": repr(ex)}
    # (c) RCCL debug lines
    if rank == 0 and rccl_log:
        try:
            import glob
            import re
            txt = "".join(open(f).read() for f in glob.glob(rccl_log + "*"))
            pick = lambda pat: sorted(set(re.findall(pat, txt)))[:8]    # noqa: E731
            rep["rccl"] = {"version": pick(r"(?:RCCL|NCCL) version ([^\n]+)"),
                           "algo_proto_env": {k: os.environ.get(k) for k in ("NCCL_ALGO", "NCCL_PROTO", "NCCL_MIN_NCHANNELS", "NCCL_MAX_NCHANNELS")},
                           "channels": pick(r"(\d+ coll channels[^\n]*)"),
                           "rings_trees": pick(r"(?:Ring|Trees?) \d+ :[^\n]{0,80}")[:4],
                           "tuning": pick(r"(AllReduce[^\n]*(?:algo|Algo)[^\n]*|ReduceScatter[^\n]*(?:algo|Algo)[^\n]*|AllGather[^\n]*(?:algo|Algo)[^\n]*)"),
                           "xgmi": pick(r"([^\n]*XGMI[^\n]{0,100})")[:4],
                           "log_bytes": len(txt)}
        except Exception as ex:  # noqa: BLE001
            rep["rccl"] = {"error": repr(ex)}
    return rep


def _run_launcher(cmd, env, timeout, n):
    """one `python -m torch.distributed.run` child in its own process group; (rc, error text or None, its stdout).  stdout is held back
    so that the caller decides which child's JSON line becomes THE line of the run (stderr passes through)"""
    import signal
    import subprocess
    proc = subprocess.Popen(cmd, env=env, start_new_session=True, stdout=subprocess.PIPE, text=True)      # own process group: the ranks can be ended together
    err, out = None, ""
    try:
        out, _ = proc.communicate(timeout=timeout)
        rc = proc.returncode
        if rc != 0:
            err = f"the launcher exited with code {rc} (a rank failed; its traceback is on stderr above)"
    except subprocess.TimeoutExpired:
        err = f"no result within {timeout:.0f} s: ranks terminated (hung collective or rendezvous?)"
        rc = 124
    if err is not None:
        for sig in (signal.SIGTERM, signal.SIGKILL):
            try:
                os.killpg(proc.pid, sig)      # the exact group this function started, nothing matched by name
            except ProcessLookupError:
                break
            try:
                more, _ = proc.communicate(timeout=10)
                out = (out or "") + (more or "")
                break
            except subprocess.TimeoutExpired:
                continue
    return rc, err, out or ""


def _has_result_line(out: str) -> bool:
    for ln in out.splitlines():
        if ln.startswith("{") and '"metric"' in ln and '"value"' in ln:
            return True
    return False


def launch_ranks(n: int, script: str = None, argv: list = None, timeout: float = None, fallback_argv: list = None) -> int:
    """`python bench.py --gpus N` with N > 1 and no launcher around it: start the ranks ourselves, as the reference does
    (run.py:34-51 calls `torchrun --nproc_per_node=N` through subprocess).  The launcher is a CHILD process (never an exec: this
    process must not be replaced, and nothing here has touched the GPU yet); its stdout -- rank 0's JSON line -- is ours, and
    so is its return code.  A run that fails or does not finish within `timeout` seconds (--launch-timeout) cannot hang the
    caller silently: the child's whole process group is terminated.  With `fallback_argv` (bench.py's own N > 1 run) a FRESH child
    then runs the plain all-reduce step alone (no sharded leg, no side reports) and its JSON line carries the first failure's text
    (`fallback_after`); if that fails too -- or without a fallback -- ONE JSON line {"error": ..., "rc": ...} is printed and the
    return code is non-zero (VERDICT r3 #6, r5 #3b; the reference's launcher has no such guard, common/utils.py:187-190)."""
    import socket

    def command(extra):
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
                "--master-port", str(port), script or os.path.abspath(__file__)] + list(extra)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")    # dmabuf IPC: RCCL across processes needs it on this pool
    env.setdefault("OMP_NUM_THREADS", "8")
    t0 = time.perf_counter()
    first = sys.argv[1:] if argv is None else list(argv)
    rc, err, out = _run_launcher(command(first), env, timeout, n)
    if err is None or _has_result_line(out):      # a child that printed its headline line and died afterwards (a side leg) still measured
        sys.stdout.write(out)
        sys.stdout.flush()
        return 0
    sys.stderr.write(out)
    if fallback_argv is not None:
        print(f"bench.py: {err}; starting a fresh child for the all-reduce step alone", file=sys.stderr, flush=True)
        rc2, err2, out2 = _run_launcher(command(list(fallback_argv) + ["--fallback-note", err]), env, timeout, n)
        if err2 is None or _has_result_line(out2):
            sys.stdout.write(out2)
            sys.stdout.flush()
            return 0
        sys.stderr.write(out2)
        err = f"{err}; the all-reduce-only fallback failed too: {err2}"
        rc = rc2
    print(json.dumps({"error": err, "rc": rc, "n_gpus": n, "elapsed_s": round(time.perf_counter() - t0, 1)}), flush=True)
    return rc if rc != 0 else 1


def fallback_args(argv: list) -> list:
    """the argument list of the all-reduce-only child: the caller's own arguments, minus any --comm-algo, plus the switches that
    drop every optional leg"""
    out, skip = [], False
    for a in argv:
        if skip:
            skip = False
            continue
        if a == "--comm-algo":
            skip = True
            continue
        if a.startswith("--comm-algo=") or a in ("--no-sharded-leg", "--no-comm-report", "--no-roofline"):
            continue
        out.append(a)
    return out + ["--comm-algo", "allreduce", "--no-sharded-leg", "--no-comm-report", "--no-roofline"]


class SideLegGuard:
    """N > 1: everything after the timed region (sharded leg, communication report, instrumented step) is optional, full of
    collectives and running on hardware this code has never met -- it must not cost the headline line.  arm(name) snapshots the
    JSON line as it stands; if the leg is still running after `budget` seconds (kept below the process group's collective timeout,
    whose watchdog would abort the process), or a SIGTERM arrives (torchrun ending the ranks because one of them died), rank 0
    prints the snapshot -- with the leg's name under `side_leg_cut` -- and the process exits 0.  disarm() when the leg returned."""

    def __init__(self, result: dict, rank: int, budget: float):
        import signal
        import threading
        self.result, self.rank, self.budget = result, rank, budget
        self._lock = threading.Lock()
        self._timer = None
        self._snap = None
        self._printed = False
        try:
            signal.signal(signal.SIGTERM, lambda *_: self._fire("SIGTERM (a rank died?)"))
        except ValueError:      # not the main thread (tests)
            pass

    def arm(self, name: str):
        import threading
        self.disarm()
        snap = dict(self.result)
        snap["side_leg_cut"] = name
        self._snap = json.dumps(snap, default=str)
        self._timer = threading.Timer(self.budget, self._fire, args=(f"no return within {self.budget:.0f} s",))
        self._timer.daemon = True
        self._timer.start()

    def disarm(self):
        if self._timer is not None:
            self._timer.cancel()
            self._timer = None
        self._snap = None

    def _fire(self, why: str):
        with self._lock:
            if self._printed:
                return
            self._printed = True
            if self.rank == 0 and self._snap is not None:
                d = json.loads(self._snap)
                d["side_leg_cut"] = f"{d['side_leg_cut']}: {why}"
                print(json.dumps(d), flush=True)
        os._exit(0 if self._snap is not None else 1)

    def final(self, line: str):
        """the one regular exit: print the full line unless the snapshot went out already"""
        with self._lock:
            if self._printed:
                return
            self._printed = True
            self.disarm()
            print(line, flush=True)


DUMP_SAMPLE = 16384     # elements per parameter tensor in --dump-outputs (all of a smaller one): <= 147 tensors in every config, < 20 MB


def dump_outputs(out_dir: str, trainer, loss, parts, optimized: bool):
    """--dump-outputs: the last timed step's loss and loss terms (what Trainer.step returns) and the state it left -- parameters and
    momentum (without the optimizer: the rank-averaged gradient) -- as a sample of each parameter tensor, in module order, whose indices are seeded
    by the parameter's name: the same arguments give the same file contents up to the kernels' own rounding."""
    import re
    import zlib
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"), np.array([float(loss)], dtype=np.float64))
    for k, v in parts.items():
        np.save(os.path.join(out_dir, "loss_" + re.sub(r"[^\w.-]", "_", k) + ".npy"), np.array([float(v)], dtype=np.float64))
    flat = trainer.flat
    # without the optimizer: the gradient it would apply -- summed over the ranks (the bf16 payload has a buffer of its own), times 1 / N
    state, scale = (trainer.opt.buf, 1.0) if optimized else trainer.reducer.grad_for_optimizer()
    offset = {id(p): o for p, o in zip(flat.params, flat.offsets)}
    ps, ss = [], []
    with torch.no_grad():
        for name, p in trainer.model.named_parameters():
            if id(p) not in offset:
                continue
            n = p.numel()
            idx = np.arange(n) if n <= DUMP_SAMPLE else np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(n, DUMP_SAMPLE, replace=False))
            ix = torch.from_numpy(idx).to(p.device)
            ps.append(p.detach().reshape(-1)[ix].float().cpu())
            ss.append(state[offset[id(p)]:offset[id(p)] + n][ix].float().cpu() * scale)
    np.save(os.path.join(out_dir, "params_sample.npy"), torch.cat(ps).numpy())
    np.save(os.path.join(out_dir, "momentum_sample.npy" if optimized else "grads_sample.npy"), torch.cat(ss).numpy())


def timed_steps(trainer, feats, tgt, sub, sync_all, warm: int, n: int, device, world: int) -> float:
    """ms per step (max over ranks) of `n` steps after `warm` untimed ones"""
    for _ in range(warm):
        trainer.step(feats, tgt, sub)
    sync_all()
    t0 = time.perf_counter()
    for _ in range(n):
        trainer.step(feats, tgt, sub)
    sync_all()
    dt = (time.perf_counter() - t0) / n * 1e3
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t)
    return dt


def sharded_leg(args, feats, tgt, sub, world, rank, device, sync_all, n: int = 10):
    """N > 1, in the same job as the all-reduce headline: the same step with the SHARDED update (reduce-scatter of each weight
    bucket's gradient, update of this rank's 1 / N slice, all-gather of the 16-bit weight images; parallel.GradReducer) on a
    fresh replica of the model -- what it is worth against the all-reduce form on this fabric."""
    from afft_amd import dropout as D_
    from afft_amd.parallel import Trainer
    if os.environ.get("AFFT_BENCH_FAIL_LEG") == "sharded":      # test hook: the leg raises on every rank
        raise RuntimeError("AFFT_BENCH_FAIL_LEG=sharded")
    if os.environ.get("AFFT_BENCH_FAIL_LEG") == "sharded_hang":  # test hook: the leg never returns
        time.sleep(3600)
    D_.manual_seed(42 + rank)
    model, c = build_model(args.config, device)
    model.train(not args.eval_drop)
    tr = Trainer(model, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, comm_dtype=args.comm_dtype,
                 bucket_elems=args.bucket_melems * 1024 * 1024, comm_algo="sharded")
    ms = timed_steps(tr, feats, tgt, sub, sync_all, 3, n, device, world)
    nsh = sum(tr.reducer.sharded_bucket(b) for b in range(len(tr.reducer.buckets)))
    loss, _ = tr.step(feats, tgt, sub)
    rep = {"ms_per_step": round(ms, 3), "clips_per_s": round(world * args.batch / ms * 1e3, 1), "steps": n,
           "sharded_buckets": nsh, "buckets": len(tr.reducer.buckets), "replicated_elems": tr.flat.total - tr.flat.split,
           "optimizer_path": "sharded" if tr.overlap_optimizer else "separate", "loss": round(float(loss), 4)}
    tr.sync_masters()
    del tr, model
    torch.cuda.empty_cache()
    return rep


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        fb = None if (args.fallback_note or os.environ.get("AFFT_BENCH_NO_FALLBACK") == "1") else fallback_args(sys.argv[1:])
        sys.exit(launch_ranks(args.gpus, timeout=args.launch_timeout, fallback_argv=fb))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    # Rehearsal of the N > 1 path on a ONE-GPU box (tests/test_model_gpu.py): AFFT_BENCH_SHARE_GPU=1 puts every rank on the
    # GPUs that exist, AFFT_BENCH_BACKEND=gloo exchanges through the host (RCCL refuses two ranks on one device).  The line such
    # a run prints says so ("rehearsal") and is not a measurement.
    backend = os.environ.get("AFFT_BENCH_BACKEND", "nccl")
    share = os.environ.get("AFFT_BENCH_SHARE_GPU") == "1"
    dev_index = local_rank % torch.cuda.device_count() if share else local_rank
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    rccl_log = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        from datetime import timedelta
        pg_timeout = timedelta(seconds=args.collective_timeout)
        if backend != "nccl":
            dist.init_process_group(backend=backend, timeout=pg_timeout)
        elif args.full and not args.no_comm_report:
            # which algorithm / protocol RCCL picks for the bucket sizes is decided inside the library: have it say so, into a
            # per-process file (INIT + TUNING lines only) that rank 0 summarises after the timed region
            rccl_log = f"/tmp/afft_rccl_{os.getpid()}.log"
            os.environ.setdefault("NCCL_DEBUG", "INFO")
            os.environ.setdefault("NCCL_DEBUG_SUBSYS", "INIT,TUNING")
            os.environ.setdefault("NCCL_DEBUG_FILE", rccl_log)
        if backend == "nccl":
            # a bounded timeout + asynchronous error handling: a rank that dies leaves the others an exception, not a hang
            os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "1")
            dist.init_process_group(backend="nccl", device_id=device, timeout=pg_timeout)   # "nccl" == RCCL on ROCm
    assert world == args.gpus or world == 1 and args.gpus == 1, f"--gpus {args.gpus} but WORLD_SIZE={world}"

    import afft_amd
    from afft_amd import dropout as D_
    from afft_amd.config import gflop_per_clip
    from afft_amd.parallel import Trainer
    afft_amd.set_precision(args.precision)
    afft_amd.set_grad_mode("sink")
    afft_amd.runtime.set_skip_dead_rows(not args.full_rows)
    D_.manual_seed(42 + rank)

    model, c = build_model(args.config, device)
    B, T = args.batch, c["T"]
    feats, tgt, sub = make_inputs(c, B, T, rank, device)
    wts = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
    if os.environ.get("AFFT_BENCH_FAIL_LEG") == "headline_sharded" and args.comm_algo == "sharded":      # test hook (launcher fallback)
        raise RuntimeError("AFFT_BENCH_FAIL_LEG=headline_sharded")
    trainer = Trainer(model, wts, comm_dtype=args.comm_dtype, bucket_elems=args.bucket_melems * 1024 * 1024,
                      comm_algo=args.comm_algo)
    model.train(not args.eval_drop)

    def sync_all():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # Python's cyclic collector: ~20 steps into a process it runs its first full (generation-2) collection over the ~200 k objects that
    # importing torch / building the model left behind -- 50-65 ms on the enqueueing thread (tools/gc_probe.py, profiles/r06_gc_stall.txt).
    # A training loop absorbs that in the host's lead over the GPU (~150 ms of queued launches); a 20-step timed region that starts right
    # after a synchronisation does not (+2.7 ms/step).  Set-up objects are moved out of the collector's sight; the collector stays on.
    import gc
    gc.collect()
    gc.freeze()

    captured = False
    if world == 1 and not args.no_optimizer and args.graph != "off":
        if args.graph in ("on", "single") or args.config in GRAPH_AUTO:
            trainer.capture(feats, tgt, sub, warmup=2, single_stream=(args.graph == "single"))
            captured = True
    for _ in range(args.warmup):
        trainer.step(feats, tgt, sub, optimize=not args.no_optimizer)
    sync_all()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss, parts = trainer.step(feats, tgt, sub, optimize=not args.no_optimizer)
    sync_all()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t)
    loss_val = float(loss)
    if loss_val != loss_val or abs(loss_val) == float("inf"):
        # A non-finite loss voids the timing: every update kernel of such a step leaves parameters and momentum untouched (FusedSGD.ok), i.e.
        # the step does less work (round 6: a race in a new GEMM kernel produced NaN losses in half of the processes -- and "faster" steps)
        if rank == 0:
            print(json.dumps({"error": "the loss of the timed region is not finite: measurement void", "final_loss": repr(loss_val), "n_gpus": world,
                              "ms_per_step_void": round(elapsed / args.steps * 1e3, 3)}), flush=True)
        raise SystemExit(3)
    if args.dump_outputs:
        trainer.sync_masters()      # sharded update: whole masters and momentum on every rank (a collective; else a no-op)
        if rank == 0:
            dump_outputs(args.dump_outputs, trainer, loss, parts, not args.no_optimizer)
    if captured:
        trainer.release_graph()
    ms_per_step = elapsed / args.steps * 1e3
    clips_s = world * B * args.steps / elapsed
    gf_ref = gflop_per_clip(args.config, fwd_bwd=True)             # what the reference executes per clip
    gf = gflop_per_clip(args.config, fwd_bwd=True, executed=afft_amd.runtime.skip_dead_rows(), token_row_projection=_token_rows(args))    # what THIS step executes

    result = {
        "metric": "clips/sec (fwd+bwd) EK100 SA-Fuser 4-mod T=16", "value": round(clips_s, 2), "unit": "clips/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.precision,
        "data": "synthetic" if backend == "nccl" and not share else
                f"synthetic -- REHEARSAL, not a measurement: backend {backend}, ranks share {torch.cuda.device_count()} GPU(s)",
        "config": {"workload": f"{args.config}: {c['fuser'].upper()}-Fuser {len(c['modal_dims'])}-modality T={T} "
                               f"d={c['common_dim']} D={c['fp_inter_dim']} depth 6+6, 3806 classes, train mode "
                               f"(dropout {'off' if args.eval_drop else 'on'}), step = fwd+loss+bwd"
                               f"{'+allreduce' if world > 1 else ''}{'' if args.no_optimizer else '+nesterov-sgd'}",
                   "per_gpu_batch": B, "global_batch": B * world, "seq_len": T,
                   "parallelism": f"dp{world}", "grad_comm_dtype": args.comm_dtype if world > 1 else None,
                   "grad_comm_algo": args.comm_algo if world > 1 else None,
                   "step_launch": ("hipGraph replay" + (", one stream" if args.graph == "single" else "")) if captured else "eager, 3 streams"},
        # FLOP accounting: utilisation figures use the FLOPs this step EXECUTES.  The reference runs the last SA-Fuser block's MLP on
        # all M + 1 tokens of a frame although only token 0 reaches an output (models/fusion.py:362-365); here those dead rows are
        # not computed (same outputs, same gradients: tests/test_model_gpu.py), 7.4 % of the reference's FLOPs on this workload
        "algorithmic_gflop_per_clip": round(gf_ref, 2),
        "executed_gflop_per_clip": round(gf, 2),
        "dead_rows_skipped": bool(afft_amd.runtime.skip_dead_rows()) and c["fuser"] == "sa",
        "model_tflops": round(clips_s * gf / 1e3, 1),
        "mfma_frac_whole_step": round(clips_s * gf / 1e3 / (PEAK_BF16_TFLOPS * world), 4),
        "final_loss": round(loss_val, 4),
        # N = 1 updates the sub-layer weights inside their weight-gradient GEMM epilogues; with a gradient exchange the summed
        # gradient has to exist first, so N > 1 runs the per-bucket update kernel (about +0.5 ms/step on cfg2): the N = 1 point
        # of a scaling curve and the ranks of its N > 1 points differ by that, by construction
        "optimizer_path": ("none" if args.no_optimizer else "fused-epilogue" if trainer._fused else
                           "sharded" if (world > 1 and args.comm_algo == "sharded" and trainer.overlap_optimizer) else "separate"),
    }
    if args.fallback_note:
        result["fallback_after"] = args.fallback_note      # this line comes from the all-reduce-only child started after that failure
    if not args.full:
        finish(result, rank, world, None)
        return
    # (a rehearsal over gloo moves the buckets through the host: minutes, and gloo raises on a timeout instead of aborting the process)
    budget = args.side_leg_budget if args.side_leg_budget is not None else (100.0 if (backend == "nccl" and not share) else 1500.0)
    guard = SideLegGuard(result, rank, budget) if world > 1 else None

    # N = 1: the same step with the SEPARATE per-bucket update kernel -- the kernels every rank of an N > 1 run executes (there the
    # summed gradient has to exist before the update), so that a scaling curve has an N = 1 anchor on the same code
    if world == 1 and not captured and not args.no_optimizer and trainer._fused and not args.no_separate_update:
        try:
            afft_amd.runtime.set_fused_sgd(False)
            ms_sep = timed_steps(trainer, feats, tgt, sub, sync_all, 3, 10, device, 1)
            result["separate_update"] = {"ms_per_step": round(ms_sep, 3), "clips_per_s": round(B / ms_sep * 1e3, 1), "steps": 10,
                                         "note": "optimizer as one kernel per gradient bucket behind the backward pass (gradients go to HBM): "
                                                 "the N > 1 ranks' code path; the headline N = 1 step updates inside the weight-gradient epilogues"}
        finally:
            afft_amd.runtime.set_fused_sgd(True)
            for _ in range(2):
                trainer.step(feats, tgt, sub)

    if world > 1:
        result["comm"] = {}
    if world > 1 and not args.no_sharded_leg and args.comm_algo != "sharded" and not args.no_optimizer:
        guard.arm("sharded leg")
        try:
            result["comm"]["sharded"] = sharded_leg(args, feats, tgt, sub, world, rank, device, sync_all)
            result["comm"]["sharded"]["vs_allreduce_step"] = round(result["comm"]["sharded"]["ms_per_step"] / ms_per_step, 4)
        except Exception as ex:  # noqa: BLE001
            result["comm"]["sharded"] = {"error": repr(ex)[:400]}
        guard.disarm()

    # the same workload with the reference's full row set (the last SA-Fuser block's MLP on all M + 1 tokens of a frame), in the same
    # process: what the dead-row elimination is worth, on the record beside the headline number
    if world == 1 and not captured and afft_amd.runtime.skip_dead_rows() and c["fuser"] == "sa" and not args.no_parity_mode:
        try:
            afft_amd.runtime.set_skip_dead_rows(False)
            for _ in range(3):
                trainer.step(feats, tgt, sub, optimize=not args.no_optimizer)
            sync_all()
            t1 = time.perf_counter()
            for _ in range(10):
                trainer.step(feats, tgt, sub, optimize=not args.no_optimizer)
            sync_all()
            dt = (time.perf_counter() - t1) / 10
            result["reference_row_set"] = {"clips_per_s": round(B / dt, 1), "ms_per_step": round(dt * 1e3, 3), "steps": 10,
                                           "gflop_per_clip": round(gf_ref, 2),
                                           "mfma_frac_whole_step": round(B / dt * gf_ref / 1e3 / PEAK_BF16_TFLOPS, 4)}
        finally:
            afft_amd.runtime.set_skip_dead_rows(True)

    if world > 1 and not args.no_comm_report:
        guard.arm("communication report")
        try:     # deterministic on every rank (same code path), so a failure cannot leave a collective half-entered
            result["comm"].update(comm_report(args, trainer, feats, tgt, sub, world, rank, device, ms_per_step, rccl_log, sync_all))
        except Exception as ex:  # noqa: BLE001
            result["comm"]["error"] = repr(ex)
        guard.disarm()

    # the instrumented step for the roofline object runs on EVERY rank (its gradient all-reduce is a collective);
    # only rank 0 keeps the timings
    summ = summ_alone = None
    ksumm = ksumm_alone = gemm_recs = None
    if not args.no_roofline:
        if guard is not None:
            guard.arm("instrumented step")
        with GemmTimer() as gt, KernelTimer() as kt:      # the same kernel sequence as a timed step (fused optimizer epilogues included)
            trainer.step(feats, tgt, sub, optimize=not args.no_optimizer)
        summ = gt.summary()
        ksumm, gemm_recs = kt.summary(), gt.records
        if guard is not None:
            sync_all()
            guard.disarm()
        # the same launches with NOTHING beside them (weight gradients on the main stream for one more instrumented step): what the
        # dominant kernel does alone, to set beside what it does inside the two-stream step (kernel quality vs schedule)
        summ_alone = None
        if world == 1 and not captured and afft_amd.runtime.overlap_wgrad():
            try:
                afft_amd.runtime.set_overlap_wgrad(False)
                trainer.step(feats, tgt, sub, optimize=not args.no_optimizer)
                with GemmTimer() as gt2, KernelTimer() as kt2:
                    trainer.step(feats, tgt, sub, optimize=not args.no_optimizer)
                summ_alone = gt2.summary()
                ksumm_alone = kt2.summary()
            finally:
                afft_amd.runtime.set_overlap_wgrad(True)

    if rank == 0 and world == 1 and not captured and not args.no_roofline and not args.no_power:
        try:
            result["power"] = power_report(lambda: trainer.step(feats, tgt, sub, optimize=not args.no_optimizer))
        except Exception as ex:  # noqa: BLE001
            result["power"] = {"error": repr(ex)[:120]}

    if rank == 0:
        # forward latency, eval mode (BASELINE.json: "fwd p50 ms")
        model.eval()
        lat = []
        with torch.no_grad():
            for i in range(110):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                model(feats, mixup_fn=None, target=tgt, target_subclips=sub, target_subclips_ignore_index=None)
                e.record()
                torch.cuda.synchronize()
                if i >= 10:
                    lat.append(s.elapsed_time(e))
        lat.sort()
        result["fwd_p50_ms"] = round(lat[len(lat) // 2], 3)
        result["fwd_p50_samples"] = len(lat)
        gff = gflop_per_clip(args.config, fwd_bwd=False, executed=afft_amd.runtime.skip_dead_rows(), token_row_projection=_token_rows(args))
        fwd_tf = B * gff / (result["fwd_p50_ms"] * 1e-3) / 1e3
        passes = {"fp16x2": 2.0, "bf16x3": 3.0}.get(args.precision, 1.0)      # MFMA passes per product of the forward GEMMs
        peak_f = 157.3 if args.precision == "fp32" else PEAK_BF16_TFLOPS
        result["fwd_p50_roofline"] = {"bound": "mfma", "achieved": round(fwd_tf, 1), "peak": round(peak_f / passes, 1),
                                      "unit": "TFLOP/s (algorithmic, whole evaluation forward of the batch)",
                                      "frac": round(fwd_tf * passes / peak_f, 4), "gflop_per_clip_forward": round(gff, 2)}
        model.train(not args.eval_drop)

        if summ is not None:
            # dominant kernel symbol = largest total duration in this instrumented step; the rocprofv3 --stats summary
            # of the same command (profiles/) ranks the symbols the same way.  Weight-gradient (TN) and nn.Linear
            # dgrad (NN) launches share the chip with each other (two streams), so their per-launch durations are
            # longer than the same launches alone (tools/gemm_bench.py); they are reported as measured.
            dom = max(summ, key=lambda k: summ[k]["ms"])
            d = summ[dom]
            avg_ms = d["ms"] / d["launches"]
            avg_fl = d["flops"] / d["launches"]
            ach = avg_fl / (avg_ms * 1e-3) / 1e12
            dtype_peak = 157.3 if args.precision == "fp32" else PEAK_BF16_TFLOPS      # bf16 / fp16 dense MFMA peak; exact-fp32 MFMA peak
            # HBM-side bytes per launch from separate rocprofv3 --pmc passes (tools/profile_round.sh + tools/traffic_summary.py, committed
            # under profiles/).  A profile belongs to ONE workload: its "_workload" entry (config, per-GPU batch, precision, GPUs) must
            # match this run, else `traffic` is null -- a kernel symbol alone says nothing about the bytes of another shape set
            traffic, traffic_src = None, None
            me = {"config": args.config, "batch": args.batch, "precision": args.precision, "gpus": world}
            import glob as _glob
            for fn in sorted(_glob.glob(os.path.join(ROOT, "profiles", "r*_gemm_hbm_traffic_pmc.json")), reverse=True):
                try:
                    tj = json.load(open(fn))
                    wl = tj.get("_workload", {"config": "cfg2", "batch": 64, "precision": "bf16", "gpus": 1})     # rounds 1-5 profiled the default run only
                    if any(wl.get(k) != v for k, v in me.items()) or args.no_optimizer or args.full_rows:
                        continue
                    hit = [v for k, v in tj.items() if isinstance(v, dict) and k != "_workload" and (k == dom or dom.startswith(k.rstrip(">")))]
                    if hit:
                        traffic, traffic_src = hit[0].get("hbm_bytes_per_launch"), os.path.basename(fn)
                        break
                except Exception:  # noqa: BLE001
                    pass
            result["roofline"] = {
                "kernel": dom + " (bf16 MFMA GEMM, v_mfma_f32_16x16x32_bf16; template <A k-strided, B k-strided[, operand planes (0 = plain bf16, 1 = bf16x3, 2 = fp16x2)]>: "
                          "A,B = false,false NT forward / false,true NN data gradient / true,true TN weight gradient; pp2 = the round-6 steady-state loop)",
                "bound": "mfma", "achieved": round(ach, 1), "peak": dtype_peak, "unit": "TFLOP/s",
                "frac": round(ach / dtype_peak, 4), "traffic": traffic,
                "algorithmic_bytes_per_launch": int(d["bytes"] / d["launches"]),
                "traffic_note": "no committed --pmc profile of this workload (config, batch, precision, GPUs): null" if traffic is None else
                                f"bytes/launch = (2*FETCH_SIZE + WRITE_SIZE)*1024 from separate --pmc passes of this command "
                                f"(profiles/{traffic_src}); fabric-side: includes Infinity-Cache hits, which the L2's counters cannot tell from HBM "
                                f"reads (profiles/r03_l2_hit_pmc.txt: 70-79 % L2 hits, ~2 TB/s of fabric reads while the kernel runs: not time-relevant); read from the committed profile of this command, not measured in this run",
                "fused_optimizer_epilogue": bool(d.get("fused_update_launches")),
                # the same kernel symbol in a step whose weight gradients run on the main stream: every launch alone on the chip
                "alone": (lambda a: {"achieved": round(a["flops"] / (a["ms"] * 1e-3) / 1e12, 1),
                                     "frac": round(a["flops"] / (a["ms"] * 1e-3) / 1e12 / dtype_peak, 4),
                                     "avg_launch_ms": round(a["ms"] / a["launches"], 4), "launches": a["launches"]})(summ_alone[dom])
                         if summ_alone and dom in summ_alone and summ_alone[dom]["ms"] > 0 else None,
                "launches_per_step": d["launches"], "avg_launch_ms": round(avg_ms, 4),
                "avg_algorithmic_gflop_per_launch": round(avg_fl / 1e9, 2),
                "by_k_class": by_k_class(gemm_recs, dom, dtype_peak),
                "by_kernel": {k: {"launches": v["launches"], "ms": round(v["ms"], 3),
                                  "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) if v["ms"] > 0 else None}
                              for k, v in summ.items()},
            }
            try:
                result["roofline"]["sublayers"] = sublayer_report(gemm_recs, ksumm, c, B)
                result["hbm_kernels"] = hbm_kernel_report(ksumm, ksumm_alone)
            except Exception as ex:  # noqa: BLE001
                result["hbm_kernels"] = {"error": repr(ex)}
        if not args.no_parity_mode and world == 1 and args.precision == "bf16":
            try:
                result.update(parity_side_measurements(args, device, feats, tgt, sub, c))
            except Exception as ex:  # noqa: BLE001
                result["parity_mode"] = {"error": repr(ex)}
        if not args.no_ek100 and world == 1 and args.config == "cfg2" and not args.no_optimizer:
            try:
                result["ek100"] = ek100_side_measurement(args, device)
            except Exception as ex:  # noqa: BLE001
                result["ek100"] = {"error": repr(ex)}
        if not args.no_small_batch and world == 1 and args.batch != 16 and not args.no_optimizer and not args.no_parity_mode:
            try:
                result["small_batch"] = small_batch_measurement(args, device)
            except Exception as ex:  # noqa: BLE001
                result["small_batch"] = {"error": repr(ex)}
        if "parity_mode" in result and "clips_per_s" in result.get("parity_mode", {}):
            # the training step whose LOGITS meet the north star's 1e-3 (fp16x2), at the top level beside `value`
            result["value_parity"] = result["parity_mode"]["clips_per_s"]
            result["ms_per_step_parity"] = result["parity_mode"]["ms_per_step"]
            result["parity_logits_rel_l2"] = result["parity_mode"].get("logits_rel_l2_vs_exact_fp32_mode")
        if not args.no_reference_loop and world == 1 and args.precision == "bf16" and not args.no_optimizer:
            try:
                result["reference_loop"] = reference_loop_measurements(args, device, feats, tgt, sub, c, ms_per_step)
            except Exception as ex:  # noqa: BLE001
                result["reference_loop"] = {"error": repr(ex)}
        if not args.no_cpu_baseline and world == 1:
            try:
                result["cpu_baseline"] = cpu_baseline(args.config, args.cpu_batch)
            except Exception as ex:  # noqa: BLE001
                result["cpu_baseline"] = {"value": None, "error": repr(ex)}

    finish(result, rank, world, guard)


def finish(result: dict, rank: int, world: int, guard):
    """rank 0 prints THE line; N > 1 leaves the process group"""
    if rank == 0:
        if guard is not None:
            guard.final(json.dumps(result))
        else:
            print(json.dumps(result), flush=True)
    if world > 1:
        try:
            dist.destroy_process_group()
        except Exception:  # noqa: BLE001
            pass


if __name__ == "__main__":
    main()
