"""Call trace of the call-by-call sub-layer path on the torch test double (no GPU): one line per ops.* call, readiness notification,
side-stream scope and join, with every argument, then a hash of every output and gradient of the step.  Two checkouts whose host code
enqueues the same kernels with the same arguments in the same order write byte-identical files:

    python tools/cbc_trace.py trace.txt                      # this checkout
    python tools/cbc_trace.py trace_parent.txt --root DIR    # afft_amd of another checkout (AFFT_LIB may point it at this one's library)
    cmp trace.txt trace_parent.txt

Configurations: the nine HOST_CASES goldens of tests/test_host_logic_cpu.py x {fp32, bf16, bf16x3, fp16x2} x {sink, autograd} x hand-over
{on, off}, and every cell of tests/test_sublayer_cbc.py at fp32 and bf16.  A tensor is written as shape, stride, dtype, storage offset and
the index of its storage's first appearance in the configuration's trace (never an address).  The tests are always this checkout's."""
import argparse
import contextlib
import hashlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Recorder:
    def __init__(self, out):
        self.out, self.events, self.seen, self.keep = out, 0, {}, []

    def new_config(self, title):
        self.seen, self.keep = {}, []
        self.out.write(f"== {title}\n")

    def arg(self, a):
        from afft_amd import _lib
        if isinstance(a, torch.Tensor):
            key = a.untyped_storage().data_ptr() if a.numel() else 0
            if key not in self.seen:
                self.seen[key] = len(self.seen)
                self.keep.append(a)      # an address must not come back for another storage while the configuration runs
            return f"T{self.seen[key]}{tuple(a.shape)}{a.stride()}{str(a.dtype)[6:]}@{a.storage_offset()}"
        if isinstance(a, _lib.Dropout):
            return f"Drop({a.p!r},{a.key},{a.path_p!r},{a.path_key},{a.path_group})"
        if hasattr(a, "planes") and hasattr(a, "f16"):
            return f"Split({self.arg(a.planes)},{a.rows},{a.cols},{a.f16})"
        if isinstance(a, (list, tuple)):
            return "[" + ",".join(self.arg(x) for x in a) + "]"
        if a is None or isinstance(a, (bool, int, float, str)):
            return repr(a)
        return type(a).__name__

    def event(self, name, args=(), kwargs=None):
        kw = "".join(f" {k}={self.arg(v)}" for k, v in sorted((kwargs or {}).items()))
        self.out.write(name + "".join(" " + self.arg(a) for a in args) + kw + "\n")
        self.events += 1

    def wrap(self, name, fn):
        def traced(*args, **kwargs):
            self.event(name, args, kwargs)
            return fn(*args, **kwargs)
        return traced

    def result(self, name, t):
        h = "None" if t is None else hashlib.sha256(t.detach().float().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]
        self.out.write(f"  = {name} {h}\n")


@contextlib.contextmanager
def recording(rec, extra_ops):
    """the installed double (plus extra_ops: name -> function) and functional's ordering points, traced"""
    import cpu_ops
    from afft_amd import functional as F_, ops
    with cpu_ops.installed():
        saved_ops = {n: getattr(ops, n) for n in list(cpu_ops._NAMES) + list(extra_ops)}
        saved_f = {n: getattr(F_, n) for n in ("_ready", "join_side")}
        enter, leave = F_._Side.__enter__, F_._Side.__exit__
        try:
            for n, f in saved_ops.items():
                setattr(ops, n, rec.wrap("ops." + n, extra_ops.get(n, f)))
            F_._ready = rec.wrap("_ready", saved_f["_ready"])
            F_.join_side = rec.wrap("join_side", saved_f["join_side"])
            F_._Side.__enter__ = lambda self: (rec.event("_Side.enter"), enter(self))[1]
            F_._Side.__exit__ = lambda self, *exc: (rec.event("_Side.exit"), leave(self, *exc))[1]
            yield
        finally:
            for n, f in saved_ops.items():
                setattr(ops, n, f)
            for n, f in saved_f.items():
                setattr(F_, n, f)
            F_._Side.__enter__, F_._Side.__exit__ = enter, leave


def golden_configs(rec):
    import afft_amd
    from afft_amd import runtime as rt
    from helpers import case_tensors, flatten_outputs
    from test_host_logic_cpu import HOST_CASES, _build, _step
    n = 0
    for name in HOST_CASES:
        c, state, data, tgt, sub = case_tensors(name)
        for precision in ("fp32", "bf16", "bf16x3", "fp16x2"):
            for gm in ("sink", "autograd"):
                for handover in (True, False):
                    rec.new_config(f"golden {name} {precision} {gm} handover={handover}")
                    n += 1
                    try:
                        with recording(rec, {}):
                            model = _build(c, precision)
                            model.load_state_dict(state, strict=True)
                            model.eval()
                            rt.set_grad_mode(gm)
                            rt.set_handover(handover)
                            out, total = _step(model, data, tgt, sub)
                        rec.result("loss", total)
                        for k, v in sorted(flatten_outputs(out).items()):
                            rec.result("out:" + k, v)
                        for k, p in model.named_parameters():
                            rec.result("grad:" + k, p.grad)
                    except Exception as e:      # noqa: BLE001  -- a configuration the double does not serve: the same text on both sides
                        rec.out.write(f"  ! {type(e).__name__}: {str(e)[:200]}\n")
                    finally:
                        rt.set_grad_mode("sink")
                        rt.set_handover(True)
                        afft_amd.set_precision("bf16")
    return n


def matrix_configs(rec):
    import afft_amd
    import test_sublayer_cbc as M
    n = 0
    for precision in ("fp32", "bf16"):
        for cell in M.CELLS:
            rec.new_config(f"cell {M.cell_id(cell)} {precision}")
            n += 1
            afft_amd.set_precision(precision)
            try:
                with recording(rec, {"attention_fwd_bias": M._bias_fwd, "attention_bias_bwd": M._bias_bwd}):
                    got = M.run_cell(cell, torch.device("cpu"))
                for k, v in sorted(got.items()):
                    rec.result(k, v)
            finally:
                afft_amd.set_precision("bf16")
    return n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out")
    ap.add_argument("--root", default=HERE, help="checkout whose afft_amd package is traced")
    a = ap.parse_args()
    sys.path[:0] = [os.path.abspath(a.root), os.path.join(HERE, "tests"), os.path.join(HERE, "tests", "golden"), HERE]
    with open(a.out, "w") as f:
        rec = Recorder(f)
        n = golden_configs(rec) + matrix_configs(rec)
        f.write(f"== {n} configurations, {rec.events} events\n")
    import afft_amd
    print(f"{os.path.dirname(afft_amd.__file__)}: {n} configurations, {rec.events} events -> {a.out}")


if __name__ == "__main__":
    main()
