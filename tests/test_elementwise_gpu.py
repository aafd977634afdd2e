"""The small kernels of csrc/elementwise.hip and the loss reductions of csrc/loss.hip, one parametrized test per entry point, against the
float64 / integer doubles of tests/kernel_doubles.py at the shapes where such kernels go wrong: one element, odd sizes, sizes around the
256-thread / 1024-float loop steps, the second workgroup, the grid clamps, leading dimensions wider than the row.

Conventions: every output is a view inside a larger buffer filled with a sentinel (Box / Flat), whose border must come back untouched;
every input that takes a stride is a view inside a NaN-filled buffer, so that a read outside the logical matrix poisons the result.
Bars: copies, casts, adds, broadcasts and the loss_reduce_bwd values are bit-equal to torch; a computed 16-bit output is within one ulp
of the float64 value rounded to the type; reductions and transcendentals take the bar of the nearest existing test (cited where used);
where there is none (loss_reduce means, softmax_rows at the new widths) the bar is max(4 x the worst error measured on an MI355X,
n 2^-24 for an n-term fp32 sum), the measured value beside it.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import kernel_doubles as kd  # noqa: E402
from helpers import rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 512.0
NAN = float("nan")
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
K_ELEM, K_OTHER, K_PATH = 4321, 0x9E3779B9, 77
EPS = 2.0 ** -24


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def up(n, m):
    return (n + m - 1) // m * m


class Box:
    """a [rows, cols] view with a border on every side: one row above and below, c0 columns to the left, at least 4 to the right; the
    leading dimension is a multiple of 8 elements, so c0 = 8 keeps rows 16-byte aligned and c0 = 1 makes every row unaligned"""

    def __init__(self, rows, cols, dtype=torch.float32, fill=SENT, c0=8, src=None):
        self.rows, self.cols, self.c0, self.fill = rows, cols, c0, fill
        self.buf = torch.full((rows + 2, up(c0 + cols + 4, 8)), fill, dtype=dtype, device=dev())
        self.v = self.buf[1:rows + 1, c0:c0 + cols]
        if src is not None:
            self.v.copy_(src.to(dtype))

    def border_ok(self):
        t = self.buf.clone()
        t[1:self.rows + 1, self.c0:self.c0 + self.cols] = self.fill
        return bool((t == self.fill).all())


def nanbox(t, dtype=torch.float32, c0=8):
    """the CPU matrix t on the device as a strided view inside a NaN-filled buffer"""
    return Box(t.shape[0], t.shape[1], dtype, NAN, c0, t).v


class Flat:
    """n contiguous elements with `pad` sentinel elements on either side"""

    def __init__(self, n, dtype=torch.float32, fill=SENT, pad=8):
        self.n, self.pad, self.fill = n, pad, fill
        self.buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev())
        self.v = self.buf[pad:pad + n]

    def border_ok(self):
        return bool((self.buf[:self.pad] == self.fill).all()) and bool((self.buf[self.pad + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def ulps16(a, b):
    """largest distance, in units in the last place, between two bf16 / fp16 tensors (+0 and -0 coincide)"""
    def key(t):
        bits = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(bits < 0, -(bits & 0x7FFF), bits)
    return int((key(a.cpu()) - key(b.cpu())).abs().max()) if a.numel() else 0


def check_computed(got, ref64, bar, what):
    """fp32 output: relative L2 against the double below `bar`; 16-bit output: at most one ulp from the double rounded to the type"""
    ref = torch.from_numpy(np.ascontiguousarray(ref64))
    if got.dtype == torch.float32:
        e = rel_l2(got, ref)
        print(f"{what}: rel L2 {e:.3e} (bar {bar:.1e})")
        assert e < bar, (what, e)
    else:
        u = ulps16(got, ref.to(got.dtype))
        print(f"{what}: {u} ulp")
        assert u <= 1, (what, u)


def drop_desc(kind):
    from afft_amd import _lib as L
    return L.Dropout(*{"elem": (0.3, K_ELEM, 0.0, 0, 1), "path1": (0.0, 0, 0.5, K_PATH, 1), "path3": (0.0, 0, 0.5, K_PATH, 3),
                       "both": (0.3, K_OTHER, 0.5, K_PATH, 3)}[kind])


# ----------------------------------------------------------------------------- afft_cast
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("mode", ["dst", "dst_t", "both", "pad"])
@pytest.mark.parametrize("rows,cols", [(1, 1), (63, 65), (64, 64), (70, 24), (129, 130)])
def test_cast_tile_kernel(rows, cols, mode, dt):
    """cast_kernel (64x64 tile through LDS): the source rows are unaligned (a column-offset view), which keeps the call off the
    4-wide kernel.  pad: dst and dst_t with zero_pad, ld = cols rounded up to 64."""
    from afft_amd import ops
    tdt = TORCH[dt]
    src = rnd(rows, cols, seed=rows * 131 + cols)
    s = nanbox(src, c0=1)
    ref = src.to(tdt)
    dst = Box(rows, cols, tdt) if mode in ("dst", "both") else None
    dst_t = Box(cols, rows, tdt) if mode != "dst" else None
    if mode == "pad":
        ld = up(cols, 64)
        pbuf = torch.full((rows + 2, ld), SENT, dtype=tdt, device=dev())
        ops.cast(s, pbuf[1:rows + 1, :cols], dst_t.v, zero_pad=True)
        assert torch.equal(pbuf[1:rows + 1, :cols].cpu(), ref)
        assert bool((pbuf[1:rows + 1, cols:] == 0).all())
        assert bool((pbuf[0] == SENT).all()) and bool((pbuf[-1] == SENT).all())
    else:
        ops.cast(s, dst.v if dst else None, dst_t.v if dst_t else None)
    if dst is not None:
        assert torch.equal(dst.v.cpu(), ref) and dst.border_ok()
    if dst_t is not None:
        assert torch.equal(dst_t.v.cpu(), ref.t()) and dst_t.border_ok()


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("rows,cols", [(5, 8), (37, 1028)])
def test_cast_rows4_kernel(rows, cols, dt):
    """cast_rows4_kernel: dst only, cols % 4 == 0, 16-byte aligned rows with ld % 4 == 0 and ld > cols on both sides"""
    from afft_amd import ops
    src = rnd(rows, cols, seed=rows + cols)
    dst = Box(rows, cols, TORCH[dt])
    ops.cast(nanbox(src), dst.v)
    assert torch.equal(dst.v.cpu(), src.to(TORCH[dt])) and dst.border_ok()


def test_cast_rows4_kernel_grid_stride():
    """rows * cols / 4 > 8192 * 256: every thread of the clamped grid takes a second quad"""
    from afft_amd import ops
    rows, cols, ld = 2052, 4100, 4104
    assert rows * cols // 4 > 8192 * 256
    sb = ((torch.arange(rows * ld, device=dev()) % 1021).float() - 510.0) * 0.37
    s = sb.view(rows, ld)[:, :cols]
    db = torch.full((rows + 1, ld), SENT, dtype=torch.bfloat16, device=dev())
    ops.cast(s, db[:rows, :cols])
    assert torch.equal(db[:rows, :cols], s.to(torch.bfloat16))
    assert bool((db[:rows, cols:] == SENT).all()) and bool((db[rows] == SENT).all())


@pytest.mark.parametrize("N", [40, 42])
@pytest.mark.parametrize("kind", ["elem", "path1", "path3", "both"])
def test_cast_dropout_replays_the_replica_mask(kind, N):
    """One descriptor over one logical [37, N] matrix: the tile kernel (unaligned view), the 4-wide kernel (aligned view, N % 4 == 0) and
    the GEMM epilogue (N % 8 == 0 vectorized, N = 42 with a scalar tail) all draw the mask of the integer replica, index r * N + c and
    row group r // path_group (37 rows: the last group is short); the two cast kernels agree bit for bit."""
    from afft_amd import ops
    rows = 37
    desc = drop_desc(kind)
    scale = torch.from_numpy(kd.drop_scales(desc, rows, N))
    assert 0 < int((scale == 0).sum()) < scale.numel()
    src = rnd(rows, N, seed=N) + 3.0
    ref = src * scale
    tile = Box(rows, N)
    ops.cast(nanbox(src, c0=1), tile.v, drop=desc)
    assert torch.equal(tile.v.cpu(), ref) and tile.border_ok()
    if N % 4 == 0:
        r4 = Box(rows, N)
        ops.cast(nanbox(src), r4.v, drop=desc)
        assert torch.equal(r4.v.cpu(), ref) and r4.border_ok()
        assert torch.equal(r4.v, tile.v)
    out = Box(rows, N)
    a, b = rnd(rows, 8, seed=1).to(dev()), (rnd(8, N, seed=2) * 0.1).to(dev())
    ops.gemm(a, b, out.v, bias=torch.full((N,), 1e3, device=dev()), drop=desc)      # bias 1e3: no kept output is 0
    assert torch.equal(out.v.cpu() == 0, scale == 0) and out.border_ok()


# ----------------------------------------------------------------------------- afft_act_bwd
ACTS = {"none": (kd.ACT_NONE, False), "gelu_erf": (kd.ACT_GELU_ERF, False), "gelu_tanh": (kd.ACT_GELU_TANH, False),
        "relu": (kd.ACT_RELU, False), "gate": (kd.ACT_SIGMOID_GATE, False), "gate_daux": (kd.ACT_SIGMOID_GATE, True)}
ACT_BAR = 3e-5      # test_linear_act_forward_backward


def _act_inputs(rows, cols, sdt, spread=3.0):
    saved = rnd(rows, cols, seed=rows * 7 + cols, scale=spread)
    flat = saved.view(-1)
    flat[0] = 0.0
    if flat.numel() >= 3:
        flat[1], flat[2] = 30.0, -30.0
    saved = saved.to(TORCH[sdt]).float()      # the reference sees the values the kernel loads
    return rnd(rows, cols, seed=5), saved, rnd(rows, cols, seed=6)


@pytest.mark.parametrize("pdt", ["f32", "bf16"])
@pytest.mark.parametrize("sdt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("rows,cols", [(1, 1), (37, 40), (3, 1027)])
@pytest.mark.parametrize("act", list(ACTS))
def test_act_bwd(act, rows, cols, sdt, pdt):
    from afft_amd import ops
    code, with_daux = ACTS[act]
    # The one-ulp bar of a bf16 dpre is RELATIVE: it can hold only where the fp32 formulas keep relative accuracy.  In the far tails of the
    # GELU derivatives (|pre| > 5) 1 + erf / 1 + tanh round to 0 and leave an ABSOLUTE error of ~1e-9 on values of ~1e-8 (7 ulp of bf16
    # measured at spread 3) -- fp32-grade, and covered by the relative-L2 bar of the fp32 cases, which keep the spread of 3.  0 and +-30 are
    # in every case.
    dy, saved, aux = _act_inputs(rows, cols, sdt, 3.0 if pdt == "f32" else 1.0)
    dpre = Box(rows, cols, TORCH[pdt])
    daux = Box(rows, cols) if with_daux else None
    ops.act_bwd(code, nanbox(dy), nanbox(saved, TORCH[sdt]), dpre.v, aux=nanbox(aux) if code == kd.ACT_SIGMOID_GATE else None,
                daux=daux.v if daux else None)
    r_pre, r_aux = kd.act_bwd(code, dy.numpy(), saved.numpy(), aux.numpy())
    check_computed(dpre.v.cpu(), r_pre, ACT_BAR, f"act_bwd {act} dpre")
    assert dpre.border_ok()
    if daux is not None:
        check_computed(daux.v.cpu(), r_aux, ACT_BAR, "act_bwd daux")
        assert daux.border_ok()
    if code in (kd.ACT_NONE, kd.ACT_RELU) and pdt == "f32":      # no arithmetic: the bits of dy, or 0
        assert torch.equal(dpre.v.cpu(), torch.from_numpy(r_pre).float())


@pytest.mark.parametrize("kind", ["elem", "path3", "both"])
def test_act_bwd_dropout_replays_the_replica_mask(kind):
    from afft_amd import ops
    rows, cols = 37, 40
    desc = drop_desc(kind)
    scale = kd.drop_scales(desc, rows, cols)
    dy, saved, _ = _act_inputs(rows, cols, "f32")
    plain, gelu = Box(rows, cols), Box(rows, cols)
    ops.act_bwd(kd.ACT_NONE, nanbox(dy), None, plain.v, drop=desc)
    ops.act_bwd(kd.ACT_GELU_ERF, nanbox(dy), nanbox(saved), gelu.v, drop=desc)
    assert torch.equal(plain.v.cpu(), dy * torch.from_numpy(scale)) and plain.border_ok()
    check_computed(gelu.v.cpu(), kd.act_bwd(kd.ACT_GELU_ERF, dy.numpy(), saved.numpy(), scale=scale)[0], ACT_BAR, "act_bwd gelu + dropout")
    assert torch.equal((gelu.v.cpu() == 0) | (saved <= -9.0), torch.from_numpy(scale == 0) | (saved <= -9.0)) and gelu.border_ok()


def test_act_bwd_grid_stride():
    """more than 8192 * 256 elements, RELU, all operands strided: a thread's second element"""
    from afft_amd import ops
    rows, cols, ld = 1030, 2051, 2056
    assert rows * cols > 8192 * 256
    i = torch.arange(rows * ld, device=dev())
    dy = (((i % 1013).float() - 506.0) * 0.01).view(rows, ld)[:, :cols]
    saved = ((((i * 7) % 1019).float() - 509.0) * 0.1).view(rows, ld)[:, :cols]
    db = torch.full((rows + 1, ld), SENT, device=dev())
    ops.act_bwd(kd.ACT_RELU, dy, saved, db[:rows, :cols])
    assert torch.equal(db[:rows, :cols], torch.where(saved > 0, dy, torch.zeros_like(dy)))
    assert bool((db[:rows, cols:] == SENT).all()) and bool((db[rows] == SENT).all())


# ----------------------------------------------------------------------------- afft_loss_reduce / afft_loss_reduce_bwd(_ok)
# no existing test supplies a bar for the means: measured worst |mean - double| / mean(|x|) on an MI355X = LOSS_MEAN_MEASURED,
# bar = max(4 x that, n 2^-24)
LOSS_MEAN_MEASURED = 2.3e-8      # worst of the three tables (n = 5000)
TERM_TABLES = {
    "one": ([5000], [0.7], {}),
    "three": ([257, 256, 1], [1.0, 0.0, 2.5], {1: NAN}),
    "eight": ([0, 1, 255, 256, 257, 5000, 256, 255], [1.0, 0.5, 0.25, 2.0, 1.5, 0.125, 0.0, 0.0], {6: float("inf"), 7: NAN}),
    "clamp": ([20000, 300, 7], [1.0, 0.3, 0.0], {}),      # 20000 > 64 * 256: the backward's grid clamp
}


def _terms(name):
    ns, ws, bad = TERM_TABLES[name]
    vals = [rnd(n, seed=11 + i) + 0.5 for i, n in enumerate(ns)]
    for i, v in bad.items():
        vals[i][ns[i] // 2] = v
    return ns, ws, bad, vals


@pytest.mark.parametrize("with_means", [True, False])
@pytest.mark.parametrize("name", ["one", "three", "eight"])
def test_loss_reduce(name, with_means):
    from afft_amd import ops
    ns, ws, bad, vals = _terms(name)
    means = Flat(len(ns)) if with_means else None
    total = Flat(1)
    ops.loss_reduce([v.to(dev()) for v in vals], ws, means.v if means else None, total.v)
    r_means, r_total = kd.loss_reduce([v.numpy() for v in vals], ws)
    tot = float(total.v)
    assert math.isfinite(tot) and total.border_ok()      # a weight of 0 drops the term: its NaN / inf stays out
    if means is None:
        # the double's total: every mean within its bar (below), every product and addition one fp32 rounding
        slack = sum(abs(w) * max(4 * LOSS_MEAN_MEASURED, n * EPS) * float(v.abs().mean()) for n, w, v in zip(ns, ws, vals) if w and n)
        assert abs(tot - r_total) <= slack + 2 * len(ns) * EPS * sum(abs(w * m) for w, m in zip(ws, r_means) if w)
        return
    m = means.v.cpu().double().numpy()
    worst = 0.0
    for i, n in enumerate(ns):
        if i in bad:
            assert (math.isnan(m[i]) and math.isnan(r_means[i])) or m[i] == r_means[i]      # the mean still reports the NaN / inf
        elif n == 0:
            assert m[i] == 0.0
        else:
            e = abs(m[i] - r_means[i]) / float(vals[i].abs().double().mean())
            worst = max(worst, e)
            assert e <= max(4 * LOSS_MEAN_MEASURED, n * EPS), (i, n, e)
    print(f"loss_reduce {name}: worst mean error {worst:.3e} relative to mean |x|")
    # the total from the kernel's own means: one fp32 rounding per product and per addition
    kept = [(w, m[i]) for i, w in enumerate(ws) if w != 0]
    assert abs(tot - sum(w * x for w, x in kept)) <= 2 * len(ns) * EPS * sum(abs(w * x) for w, x in kept)
    assert means.border_ok()


@pytest.mark.parametrize("go", [None, 0.5])
@pytest.mark.parametrize("name", list(TERM_TABLES))
def test_loss_reduce_bwd(name, go):
    """g[i][:] = float32(go * w[i] / n[i]) bit for bit; a NULL g[i] and an empty term are skipped; ok = 1 for a finite total"""
    from afft_amd import ops
    ns, ws, _, _ = _terms(name)
    skip = 1 if len(ns) > 1 else -1
    grads = [Flat(n) for n in ns]
    ok = Flat(1)
    ops.loss_reduce_bwd([None if i == skip else g.v for i, g in enumerate(grads)], ws,
                        None if go is None else torch.tensor([go], device=dev()), torch.tensor([1.25], device=dev()), ok.v)
    vals, r_ok = kd.loss_reduce_bwd(ns, ws, go, 1.25)
    for i, g in enumerate(grads):
        if i == skip or ns[i] == 0:
            assert g.untouched()
        else:
            assert torch.equal(g.v.cpu(), torch.full((ns[i],), float(vals[i]))) and g.border_ok(), i
    assert float(ok.v) == r_ok == 1.0 and ok.border_ok()


@pytest.mark.parametrize("total,go,want", [(NAN, None, 0.0), (float("inf"), None, 0.0), (1.0, float("inf"), 0.0), (1.0, float("-inf"), 0.0),
                                           (1.0, None, 1.0), (None, 0.5, 1.0)])
def test_loss_reduce_bwd_ok_flag(total, go, want):
    from afft_amd import ops
    g, ok = Flat(300), Flat(1)
    ops.loss_reduce_bwd([g.v], [1.0], None if go is None else torch.tensor([go], device=dev()),
                        None if total is None else torch.tensor([total], device=dev()), ok.v)
    assert float(ok.v) == want == kd.loss_reduce_bwd([300], [1.0], go, total)[1] and ok.border_ok() and g.border_ok()


def test_loss_reduce_bwd_without_ok():
    from afft_amd import ops
    g = Flat(257)
    ops.loss_reduce_bwd([g.v], [0.3], None)
    assert torch.equal(g.v.cpu(), torch.full((257,), float(kd.loss_reduce_bwd([257], [0.3])[0][0]))) and g.border_ok()


# ----------------------------------------------------------------------------- afft_mse / afft_mse_frames_bwd
@pytest.mark.parametrize("rows,d", [(1, 1), (45, 64), (515, 1028)])
def test_mse_with_gradients(rows, d):
    """(515, 1028) passes the 2048-workgroup clamp: every thread takes several elements.  a, b, da, db strided; da / db prefilled (+= / -=);
    the upstream gradient on the device; the loss sum accumulates over two calls."""
    from afft_amd import ops
    a, b = rnd(rows, d, seed=1), rnd(rows, d, seed=2)
    A, B = nanbox(a), nanbox(b)
    da, db = Box(rows, d), Box(rows, d)
    da.v.fill_(0.25)
    db.v.fill_(-0.5)
    ls = Flat(1, fill=0.0)
    ops.mse(A, B, 0.5, ls.v, da.v, db.v, g_dev=torch.tensor([0.5], device=dev()))
    ops.mse(A, B, 0.5, ls.v, None, None)
    s, r_da, r_db = kd.mse(a.numpy(), b.numpy(), g=0.25)
    e = abs(float(ls.v) - 2 * s) / (2 * s)
    print(f"mse [{rows}, {d}]: loss {e:.3e}")
    assert e < 2e-6      # test_mse_loss_scalar_is_bit_stable
    for got, pre, ref in ((da, 0.25, r_da), (db, -0.5, r_db)):
        # 1e-5 (test_mse_and_elementwise's db bar) on the gradient, plus the fp32 rounding of prefill + gradient
        err = float(np.linalg.norm(got.v.cpu().double().numpy() - pre - ref))
        assert err <= 1e-5 * float(np.linalg.norm(ref)) + 2 * EPS * float(np.linalg.norm(pre + ref)), err
        assert got.border_ok()


@pytest.mark.parametrize("which", ["both", "da", "db"])
def test_mse_frames_bwd_long_span(which):
    """a span above 64 * 1024 floats: the grid-stride loop; either gradient alone.  2 * gscale * g_dev is a power of two, so the
    gradient has the bits of the fp32 difference scaled."""
    from afft_amd import ops
    B, Ta, Tb, C, a_lo, b_lo, nt = 2, 5, 4, 16384, 1, 0, 3
    assert Ta * C > 64 * 1024
    a, b = rnd(B, Ta, C, seed=3), rnd(B, Tb, C, seed=4)
    ab = torch.full((B, Ta + 1, C), NAN, device=dev())
    bb = torch.full((B, Tb + 2, C), NAN, device=dev())
    ab[:, :Ta], bb[:, :Tb] = a.to(dev()), b.to(dev())
    da = Flat(B * Ta * C) if which != "db" else None
    db = Flat(B * Tb * C) if which != "da" else None
    ops.mse_frames_bwd(ab[:, :Ta], bb[:, :Tb], a_lo, b_lo, nt, 0.25, torch.tensor([0.5], device=dev()),
                       da.v.view(B, Ta, C) if da else None, db.v.view(B, Tb, C) if db else None)
    r_da, r_db = kd.mse_frames_bwd(a.numpy(), b.numpy(), a_lo, b_lo, nt, g=0.125)
    for got, ref in ((da, r_da), (db, r_db)):
        if got is not None:
            assert torch.equal(got.v.cpu(), torch.from_numpy(ref).float().reshape(-1)) and got.border_ok()


# ----------------------------------------------------------------------------- afft_assemble_tokens / afft_add_rows_periodic
@pytest.mark.parametrize("d,n_mod,tok", [(d, n, t) for d in (4, 1024, 1028, 2052) for n in (1, 8) for t in ("universal", "per_t", "per_t_padded")]
                         + [(64, 4, "per_t")])
def test_assemble_tokens(d, n_mod, tok):
    """d > 1024: the second trip of the c += 1024 loop; feature rows with ldf > d; token stride 0, d and d + 4"""
    from afft_amd import ops
    B, T = 2, 3
    BT, S = B * T, n_mod + 1
    feats = [rnd(BT, d, seed=10 + i) for i in range(n_mod)]
    token, emb = rnd(T, d, seed=20), rnd(S, d, seed=21)
    if tok == "universal":
        tv, stride, rows0 = token[:1].contiguous().to(dev()), 0, token[:1].expand(BT, d)
    else:
        tb = torch.full((T, d + 4), NAN, device=dev())
        tb[:, :d] = token.to(dev())
        tv, stride = (tb[:, :d], d + 4) if tok == "per_t_padded" else (token.to(dev()), d)
        rows0 = token.repeat(B, 1)
    fv = [nanbox(f) for f in feats]
    ref = torch.stack([rows0] + feats, dim=1)
    for e in (emb, None):
        X = Flat(BT * S * d)
        ops.assemble_tokens(fv, tv, stride, e.to(dev()) if e is not None else None, BT, T, d, X.v.view(BT, S, d))
        assert torch.equal(X.v.cpu().view(BT, S, d), ref + e if e is not None else ref) and X.border_ok()


@pytest.mark.parametrize("period", [1, 3])
@pytest.mark.parametrize("d", [4, 1024, 1028, 2052])
def test_add_rows_periodic(d, period):
    from afft_amd import ops
    rows = 7      # rows % 3 != 0
    x, table = rnd(rows, d, seed=31), rnd(period, d, seed=32)
    y = Box(rows, d)
    ops.add_rows_periodic(nanbox(x), nanbox(table), period, y.v)
    assert torch.equal(y.v.cpu(), x + table[torch.arange(rows) % period]) and y.border_ok()


# ----------------------------------------------------------------------------- afft_reduce_rows_periodic
@pytest.mark.parametrize("d", [4, 130, 260, 1028])
@pytest.mark.parametrize("branch", ["period1", "dense", "generic"])
def test_reduce_rows_periodic(branch, d):
    """period1: a plain column sum at any row stride; dense (lds = ldo = d, rows % period == 0): the column sums of the
    [rows / period, period * d] view; generic: ragged rows, lds > d, ldo > d, d not a multiple of 4.  out is added to."""
    from afft_amd import ops
    rows, period = {"period1": (11, 1), "dense": (12, 4), "generic": (11, 4)}[branch]
    src = rnd(rows, d, seed=33 + d)
    if branch == "dense":
        out = Flat(period * d)
        out.v.fill_(1.0)
        ops.reduce_rows_periodic(src.to(dev()), period, out.v.view(period, d))
        got = out.v.cpu().view(period, d)
    else:
        out = Box(period, d)
        out.v.fill_(1.0)
        ops.reduce_rows_periodic(nanbox(src), period, out.v)
        got = out.v.cpu()
    e = rel_l2(got - 1.0, torch.from_numpy(kd.reduce_rows_periodic(src.numpy(), period)))
    print(f"reduce_rows_periodic {branch} d={d}: {e:.3e}")
    assert e < 1e-5 and out.border_ok()      # test_mse_and_elementwise (reduce_rows_periodic), test_colsum_is_exact_enough...


# ----------------------------------------------------------------------------- afft_group_sum / afft_group_bcast
@pytest.mark.parametrize("W,S,G", [(W, S, G) for W in (4, 1024, 1028, 4100) for S in (1, 5) for G in (1, 6)] + [(72, 5, 6)])
def test_group_sum_and_bcast(W, S, G):
    from afft_amd import ops
    x = rnd(G, S, W, seed=34)
    y = Flat(G * W)
    ops.group_sum(x.to(dev()), G, S, W, 1.0 / S, y.v.view(G, W))
    assert rel_l2(y.v.cpu().view(G, W), x.double().sum(1) * float(np.float32(1.0 / S))) < 1e-6 and y.border_ok()      # test_mse_and_elementwise
    dy = rnd(G, W, seed=35)
    dx = Flat(G * S * W)
    ops.group_bcast(dy.to(dev()), G, S, W, 0.2, dx.v.view(G * S, W))
    assert torch.equal(dx.v.cpu().view(G, S, W), (dy * np.float32(0.2))[:, None, :].expand(G, S, W)) and dx.border_ok()


# ----------------------------------------------------------------------------- afft_gather_frames
GATHER = {      # clips, frames, C, [(source frames, lo, hi, off)]
    "no_source": (2, 3, 8, []),
    "negative_off": (3, 5, 8, [(4, 2, 5, -2)]),
    "four_overlapping": (2, 6, 12, [(6, 0, 6, 0), (3, 1, 4, -1), (5, 2, 2, 0), (7, 3, 6, 1)]),      # the third: lo == hi
    "grid_clamp": (5, 7, 60004, [(8, 0, 7, 1)]),      # 7 * 15001 quads: 411 workgroups wanted, 410 allowed
}


@pytest.mark.parametrize("name", list(GATHER))
def test_gather_frames(name):
    from afft_amd import ops
    clips, frames, C, spec = GATHER[name]
    srcs, host = [], []
    for k, (f, lo, hi, off) in enumerate(spec):
        h = rnd(clips, f, C, seed=40 + k)
        b = torch.full((clips, f + 1, C + 4), NAN, device=dev())
        b[:, :f, :C] = h.to(dev())
        srcs.append((b[:, :f, :C], lo, hi, off))
        host.append((h.numpy(), lo, hi, off))
    ob = torch.full((clips + 1, frames + 1, C + 4), SENT, device=dev())
    ops.gather_frames(ob[:clips, :frames, :C], srcs)
    ref = kd.gather_frames(clips, frames, C, host, dtype=np.float32)      # the kernel's own additions, in source order
    assert torch.equal(ob[:clips, :frames, :C].cpu(), torch.from_numpy(ref))
    assert np.allclose(ref, kd.gather_frames(clips, frames, C, host), rtol=0, atol=1e-5)
    ob[:clips, :frames, :C] = SENT
    assert bool((ob == SENT).all())


# ----------------------------------------------------------------------------- afft_softmax_rows
# C = 3806: 2e-5 (test_marginalize_verb_noun_scores).  The other widths have no bar: measured worst relative L2 on an MI355X =
# SOFTMAX_ROWS_MEASURED, bar = max(4 x that, C 2^-24)
SOFTMAX_ROWS_MEASURED = 1.4e-7      # worst over the eight widths (C = 64)


def _softmax_bar(C):
    return 2e-5 if C == 3806 else max(4 * SOFTMAX_ROWS_MEASURED, C * EPS)


@pytest.mark.parametrize("C", [1, 63, 64, 65, 255, 256, 257, 3806])
def test_softmax_rows(C):
    """rows: plain, -inf entries (never a whole row), shifted by +80 and -80, large equal values, wide spread"""
    from afft_amd import ops
    x = rnd(6, C, seed=C)
    x[1, 1::3] = float("-inf")
    x[2] += 80.0
    x[3] -= 80.0
    x[4] = 1e4
    x[5] *= 10.0
    y = Box(6, C)
    ops.softmax_rows(nanbox(x), y.v)
    got, ref = y.v.cpu().double(), torch.from_numpy(kd.softmax_rows(x.numpy()))
    e = max(float((got[r] - ref[r]).norm() / ref[r].norm()) for r in range(6))
    s = float((got.sum(1) - 1.0).abs().max())
    print(f"softmax_rows C={C}: worst row rel L2 {e:.3e}, worst |row sum - 1| {s:.3e} (bar {_softmax_bar(C):.2e})")
    assert e <= _softmax_bar(C) and s <= _softmax_bar(C)
    assert bool((got[1, 1::3] == 0).all()) and y.border_ok()


# ----------------------------------------------------------------------------- afft_softmax_small_fwd / _bwd
@pytest.mark.parametrize("rows", [1, 255, 256, 257])
@pytest.mark.parametrize("n", [1, 2, 31, 32])
def test_softmax_small(n, rows):
    from afft_amd import ops
    x, dy = rnd(rows, n, seed=61, scale=2.0), rnd(rows, n, seed=62)
    y = Box(rows, n)
    ops.softmax_small_fwd(nanbox(x), y.v)
    r_y = kd.softmax_small_fwd(x.numpy())
    assert rel_l2(y.v.cpu(), torch.from_numpy(r_y)) < 1e-6 and y.border_ok()      # test_softmax_small_and_weighted_sum
    y32 = torch.from_numpy(r_y).float()
    dx = Box(rows, n)
    ops.softmax_small_bwd(nanbox(y32), nanbox(dy), dx.v)
    r_dx = kd.softmax_small_bwd(y32.numpy(), dy.numpy())
    if n == 1:      # y = 1: the gradient is 0 up to the rounding of dy - dy * y
        assert float(dx.v.abs().max()) <= 2 * EPS * float(dy.abs().max())
    else:
        assert rel_l2(dx.v.cpu(), torch.from_numpy(r_dx)) < 2e-5      # test_softmax_small_and_weighted_sum (logit gradients)
    assert dx.border_ok()


# ----------------------------------------------------------------------------- afft_weighted_sum_fwd / _bwd
@pytest.mark.parametrize("cols", [1, 63, 256, 257, 3806])
@pytest.mark.parametrize("n", [1, 5, 8])
def test_weighted_sum(n, cols):
    """dw sums over the whole row: a lost wave partial shows at cols 63 (one wave, partly filled) and 257 (a second trip of wave 0)"""
    from afft_amd import ops
    rows = 3
    xs = [rnd(rows, cols, seed=70 + i) for i in range(n)]
    w, dout = rnd(rows, n, seed=80), rnd(rows, cols, seed=81)
    xv, wv = [nanbox(x) for x in xs], nanbox(w)
    out = Box(rows, cols)
    ops.weighted_sum_fwd(xv, wv, out.v)
    assert rel_l2(out.v.cpu(), torch.from_numpy(kd.weighted_sum_fwd([x.numpy() for x in xs], w.numpy()))) < 1e-6 and out.border_ok()
    dxs, dw = [Box(rows, cols) for _ in range(n)], Box(rows, n)
    ops.weighted_sum_bwd(xv, wv, nanbox(dout), [b.v for b in dxs], dw.v)
    r_dxs, r_dw = kd.weighted_sum_bwd([x.numpy() for x in xs], w.numpy(), dout.numpy())
    for got, ref in zip(dxs, r_dxs):
        assert rel_l2(got.v.cpu(), torch.from_numpy(ref)) < 1e-6 and got.border_ok()      # test_softmax_small_and_weighted_sum
    e = rel_l2(dw.v.cpu(), torch.from_numpy(r_dw))
    print(f"weighted_sum dw n={n} cols={cols}: {e:.3e}")
    assert e < 1e-5 and dw.border_ok()      # an fp32 sum over the row: test_colsum_is_exact_enough...


# ----------------------------------------------------------------------------- afft_mixup_plan / _rows / _labels
@pytest.mark.parametrize("scen", ["no_sub", "mixed", "all_ignored", "one_left"])
@pytest.mark.parametrize("B", [1, 2, 256, 257, 4096])
def test_mixup_plan(B, scen):
    from afft_amd import ops
    T = 3
    g = torch.Generator().manual_seed(B)
    sub = torch.randint(0, 9, (B, T), generator=g)
    if scen == "mixed":
        sub[torch.rand(B, T, generator=g) < 0.2] = -1
    elif scen in ("all_ignored", "one_left"):
        sub[torch.arange(B), torch.arange(B) % T] = -1
        if scen == "one_left":
            sub[B // 2] = 5
    partner, ign = Flat(B, torch.int32, fill=-7), Flat(B * T, torch.uint8, fill=7)
    ops.mixup_plan(None if scen == "no_sub" else sub.to(dev()), B, -1, partner.v, ign.v)
    r_partner, r_ign = kd.mixup_plan(None if scen == "no_sub" else sub.numpy(), B, -1)
    assert np.array_equal(partner.v.cpu().numpy(), r_partner) and partner.border_ok()
    if r_ign is None:
        assert ign.untouched()
    else:
        assert np.array_equal(ign.v.cpu().numpy().reshape(B, T), r_ign) and ign.border_ok()


@pytest.mark.parametrize("W", [1, 255, 16384 + 260])
def test_mixup_rows(W):
    """W > 64 * 256: the clamp of the grid's x dimension"""
    from afft_amd import ops
    B, lam = 3, float(np.float32(0.3))
    oml = float(np.float32(1.0) - np.float32(0.3))
    x = rnd(B, W, seed=90)
    y = Flat(B * W)
    ops.mixup_rows(x.to(dev()), torch.tensor([2, 1, 0], dtype=torch.int32, device=dev()), 0.3, y.v.view(B, W))
    got = y.v.cpu().view(B, W)
    ref = torch.stack([lam * x[0].double() + oml * x[2].double(), x[1].double(), lam * x[2].double() + oml * x[0].double()])
    assert rel_l2(got, ref) < 1e-6 and torch.equal(got[1], x[1]) and y.border_ok()      # test_mixup_prologue_matches_oracle


@pytest.mark.parametrize("K", [1, 255, 257])
def test_mixup_labels(K):
    """ignored labels count as class 0"""
    from afft_amd import ops
    B, rps, ls, ignore = 3, 2, 0.4, -1
    lam, oml = float(np.float32(0.3)), float(np.float32(1.0) - np.float32(0.3))
    labels = torch.randint(0, K, (B, rps), generator=torch.Generator().manual_seed(K))
    labels[0, 1] = ignore
    labels[2, 0] = K - 1
    partner = [2, 1, 0]
    out = Flat(B * rps * K)
    ops.mixup_labels(labels.to(dev()), B, K, ls, ignore, torch.tensor(partner, dtype=torch.int32, device=dev()), 0.3, out.v.view(B * rps, K))
    off = float(np.float32(ls) / np.float32(K))
    on = float(np.float32(1.0) - np.float32(ls) + np.float32(off))
    lab = labels.clone()
    lab[lab == ignore] = 0
    hot = torch.full((B, rps, K), off, dtype=torch.float64).scatter_(2, lab[..., None], on)
    ref = torch.stack([hot[b] if partner[b] == b else lam * hot[b] + oml * hot[partner[b]] for b in range(B)])
    assert rel_l2(out.v.cpu().view(B, rps, K), ref) < 1e-6 and out.border_ok()      # test_mixup_prologue_matches_oracle


# ----------------------------------------------------------------------------- afft_zero_mask_frames / afft_zero
@pytest.mark.parametrize("C", [1, 255, 257])
@pytest.mark.parametrize("k", [0, 3, 8])
def test_zero_mask_frames(k, C):
    from afft_amd import ops
    B, T = 5, 8
    x = torch.rand(B, T, C, generator=torch.Generator().manual_seed(C)) + 1.0
    y = Flat(B * T * C)
    y.v.copy_(x.reshape(-1))
    ops.zero_mask_frames(y.v.view(B, T, C), k, K_ELEM)
    got = y.v.cpu().view(B, T, C)
    zero = (got == 0).all(-1)
    assert torch.equal(zero.sum(1), torch.full((B,), k)) and torch.equal(got[~zero], x[~zero]) and y.border_ok()
    if k == 3:
        assert len({tuple(r.tolist()) for r in zero}) > 1      # clips draw different subsets


@pytest.mark.parametrize("nbytes", [16, 2048 * 256 * 16 + 80])
def test_zero(nbytes):
    from afft_amd import _lib as L, ops
    buf = torch.full((nbytes + 512,), 0x5A, dtype=torch.uint8, device=dev())
    L.check(L.lib().afft_zero(buf.data_ptr() + 256, nbytes, ops._stream()), "zero")
    assert bool((buf[256:256 + nbytes] == 0).all())
    assert bool((buf[:256] == 0x5A).all()) and bool((buf[256 + nbytes:] == 0x5A).all())


# ----------------------------------------------------------------------------- afft_split_bf16 / afft_split_f16 / afft_quant_e4m3
def _e4m3_decode(b):
    """uint8 tensor of OCP e4m3fn codes -> float32 values"""
    b = b.to(torch.int32)
    s, e, m = b >> 7, (b >> 3) & 15, b & 7
    v = torch.where(e == 0, m.float() / 8.0 * 2.0 ** -6, (1.0 + m.float() / 8.0) * torch.pow(2.0, (e - 7).float()))
    return torch.where(s == 1, -v, v)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("cols", [1, 7, 8, 9, 70])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_split_planes(kind, cols, aligned):
    """rows_pad > rows, ldd > cols, 16-byte aligned (src_vec = 1) and unaligned (src_vec = 0) source rows"""
    from afft_amd import _lib as L, ops
    rows, rows_pad, ldd = 5, 8, up(cols, 8) + 8
    tdt = torch.bfloat16 if kind == "bf16" else torch.float16
    x = rnd(rows, cols, seed=cols, scale=3.0)
    s = nanbox(x, c0=8 if aligned else 1)
    n, ps = rows_pad * ldd, rows_pad * ldd + 16
    buf = torch.full((8 + ps + n + 8,), SENT, dtype=tdt, device=dev())
    fn = L.lib().afft_split_bf16 if kind == "bf16" else L.lib().afft_split_f16
    L.check(fn(s.data_ptr(), s.stride(0), rows, cols, buf.data_ptr() + 16, ldd, rows_pad, ps, ops._stream()), "split")
    b = buf.cpu()
    hi, lo = b[8:8 + n].view(rows_pad, ldd).float(), b[8 + ps:8 + ps + n].view(rows_pad, ldd).float()
    r_hi = x.to(tdt).float()
    assert torch.equal(hi[:rows, :cols], r_hi) and torch.equal(lo[:rows, :cols], (x - r_hi).to(tdt).float())
    assert float((hi + lo)[:rows, :cols].double().sub(x.double()).abs().max()) <= float(x.abs().max()) * 2.0 ** -16      # test_split_bf16_planes
    for p in (hi, lo):
        assert float(p[rows:].abs().max()) == 0 and float(p[:, cols:].abs().max()) == 0
    assert bool((b[:8] == SENT).all()) and bool((b[8 + n:8 + ps] == SENT).all()) and bool((b[8 + ps + n:] == SENT).all())


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("cols", [1, 7, 8, 9, 70])
@pytest.mark.parametrize("with_hi", [False, True])
def test_quant_e4m3(with_hi, cols, aligned):
    """e4m3 has 3 mantissa bits: a normal value is off by at most 2^-4 of itself, a subnormal one (below 2^-6) by at most 2^-10"""
    from afft_amd import _lib as L, ops
    rows, rows_pad, ldd = 5, 8, up(cols, 8) + 8
    scale = 2048.0 if with_hi else 16.0
    x = rnd(rows, cols, seed=cols, scale=3.0)
    s = nanbox(x, c0=8 if aligned else 1)
    n = rows_pad * ldd
    buf = torch.full((16 + n + 16,), 0xA5, dtype=torch.uint8, device=dev())
    hib = torch.full((8 + n + 8,), SENT, dtype=torch.float16, device=dev()) if with_hi else None
    L.check(L.lib().afft_quant_e4m3(s.data_ptr(), s.stride(0), rows, cols, scale, buf.data_ptr() + 16, ldd, rows_pad,
                                    hib.data_ptr() + 16 if with_hi else None, ops._stream()), "quant_e4m3")
    b = buf.cpu()
    q = b[16:16 + n].view(rows_pad, ldd)
    want = x * scale
    if with_hi:
        h = hib.cpu()
        hi = h[8:8 + n].view(rows_pad, ldd)
        assert torch.equal(hi[:rows, :cols], x.half()) and float(hi[rows:].float().abs().max()) == 0 and float(hi[:, cols:].float().abs().max()) == 0
        assert bool((h[:8] == SENT).all()) and bool((h[8 + n:] == SENT).all())
        want = (x - x.half().float()) * scale
    assert float(want.abs().max()) < 448.0
    dec = _e4m3_decode(q[:rows, :cols])
    assert bool(((dec - want).abs() <= want.abs() * 2.0 ** -4 + 2.0 ** -10).all())
    if cols == 70:
        assert rel_l2(dec, want) < 0.05      # test_gemm_fp16_hi_pass_plus_fp8_lo_pass
    assert int(q[rows:].max()) == 0 and int(q[:, cols:].max()) == 0
    assert bool((b[:16] == 0xA5).all()) and bool((b[16 + n:] == 0xA5).all())


def test_split_bf16_grid_stride():
    """rows_pad * ldd / 8 > 16384 * 256: the clamped grid's second trip, compared on the device"""
    from afft_amd import _lib as L, ops
    rows, cols, rows_pad, ldd = 4099, 8190, 4100, 8192
    assert rows_pad * ldd // 8 > 16384 * 256
    src = (((torch.arange(rows * ldd, device=dev()) % 4093).float() - 2046.0) * 0.0137).view(rows, ldd)[:, :cols]
    n = rows_pad * ldd
    buf = torch.full((8 + 2 * n + 8,), SENT, dtype=torch.bfloat16, device=dev())
    L.check(L.lib().afft_split_bf16(src.data_ptr(), src.stride(0), rows, cols, buf.data_ptr() + 16, ldd, rows_pad, n, ops._stream()), "split")
    hi, lo = buf[8:8 + n].view(rows_pad, ldd), buf[8 + n:8 + 2 * n].view(rows_pad, ldd)
    r_hi = src.to(torch.bfloat16)
    assert torch.equal(hi[:rows, :cols], r_hi) and torch.equal(lo[:rows, :cols], (src - r_hi.float()).to(torch.bfloat16))
    for p in (hi, lo):
        assert bool((p[rows:] == 0).all()) and bool((p[:, cols:] == 0).all())
    assert bool((buf[:8] == SENT).all()) and bool((buf[8 + 2 * n:] == SENT).all())


# ----------------------------------------------------------------------------- afft_clip_coef
@pytest.mark.parametrize("with_norm", [False, True])
@pytest.mark.parametrize("sumsq", [0.0, 1e-30, 1.0, 3.9999, 1e8])
def test_clip_coef(sumsq, with_norm):
    """coef = min(1, max_norm / (sqrt(sumsq) + 1e-6)): 0 and tiny sums and every norm below max_norm give exactly 1"""
    from afft_amd import ops
    max_norm = 2.0
    coef, norm = Flat(1), Flat(1) if with_norm else None
    ops.clip_coef(torch.tensor([sumsq], device=dev()), max_norm, coef.v, norm.v if norm else None)
    r_norm = math.sqrt(float(np.float32(sumsq)))
    r_coef = min(1.0, max_norm / (r_norm + 1e-6))
    if r_coef == 1.0:
        assert float(coef.v) == 1.0
    assert abs(float(coef.v) - r_coef) <= 1e-6 * r_coef and coef.border_ok()      # tighter than test_mse_and_elementwise's 1e-5
    if norm is not None:
        assert abs(float(norm.v) - r_norm) <= 1e-6 * r_norm and norm.border_ok()
