"""Restatements of afft_ema / afft_swap_f32 (include/afft_hip.h): the float64 reference with its derived error bar for the GPU
tests, and torch doubles of ops.ema / ops.swap_f32 for the host-logic tests (installed beside tests/cpu_ops.py)."""
import contextlib

import torch

U = 2.0 ** -24      # fp32 unit roundoff


def ema_ref(ema, p, w):
    """(float64 result, bar) of ema + w * (p - ema) for fp32 inputs and the fp32 w the kernel receives.
    The kernel rounds twice: d = fl(p - e), |d - (p - e)| <= u (|p| + |e|); r = fl(e + w d), |r - (e + w d)| <= u |e + w d|
    <= u (|p| + |e|) (a convex combination of e and p, up to the first error).  With w <= 1: |r - ref| <= 2 u (|p| + |e|)."""
    e64, p64 = ema.double(), p.double()
    w64 = float(torch.tensor(w, dtype=torch.float32))
    return e64 + w64 * (p64 - e64), 2.0 * U * (p64.abs() + e64.abs())


@torch.no_grad()
def ema_double(ema_, p, w, ok=None):
    if (ok is not None and float(ok) == 0.0) or w == 0.0:
        return
    w32 = float(torch.tensor(w, dtype=torch.float32))
    d = p - ema_
    r = (ema_.double() + w32 * d.double()).float()      # the fp32 x fp32 product is exact in double
    ema_.copy_(torch.where(d == 0, ema_, r))


@torch.no_grad()
def swap_double(a, b):
    t = a.clone()
    a.copy_(b)
    b.copy_(t)


@contextlib.contextmanager
def doubles():
    """cpu_ops.installed() plus the Adam doubles of test_adam_cpu plus the two above"""
    from afft_amd import ops
    from test_adam_cpu import doubles as adam_doubles
    saved = ops.ema, ops.swap_f32
    with adam_doubles():
        ops.ema, ops.swap_f32 = ema_double, swap_double
        try:
            yield
        finally:
            ops.ema, ops.swap_f32 = saved
