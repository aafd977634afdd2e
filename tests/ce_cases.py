"""What the tests of the cross-entropy family share (test_ce_weighted_*.py, test_ce_focal_*.py): the inputs of one case, the launch of
a wrapper of afft_amd.ops into sentinel-framed buffers, the error ratios against a float64 double, and a recording stand-in for the
six wrappers on a machine without a GPU."""
import torch

import ce_double
import cpu_ops
import focal_double

U = 2.0 ** -24
SENT = 512.0


def dev():
    return torch.device("cuda:0")


def up(n, m):
    return (n + m - 1) // m * m


def make_inputs(rows, C, kind, wmode, seed, adj=False):
    """CPU tensors of one case: x, labels, soft, keep, weight, adjustment (None where the case has none).  Hard: every fourth row is
    ignored.  zeros: every third class (and class 0) has weight 0; row 1's label (hard) or whole support (soft) lies in that set, so
    with smoothing 0 its A is 0.  The generator is drawn from in this order: x, weights, adjustment, targets."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) * 3.0
    w = None
    if wmode != "none":
        w = torch.rand(C, generator=g) * 2.0 + 0.1
        if wmode == "zeros":
            w[::3] = 0.0
    b = -8.0 * torch.rand(C, generator=g) if adj else None
    labels = soft = keep = None
    if kind == "hard":
        labels = torch.randint(0, C, (rows,), generator=g)
        labels[2::4] = -1
        if rows > 1:
            labels[1] = 0
    else:
        soft = torch.softmax(torch.randn(rows, C, generator=g), 1) * (torch.rand(rows, C, generator=g) < 0.6)
        soft = soft / soft.sum(1, keepdim=True).clamp(min=1e-3)
        if rows > 1:
            soft[1] = 0.0
            soft[1, 0] = 1.0
        if kind == "soft_keep":
            keep = (torch.rand(rows, generator=g) < 0.7).to(torch.uint8)
            if rows > 1:
                keep[1] = 1
    return x, labels, soft, keep, w, b


def framed(t, ld, fill=float("nan")):
    """the CPU matrix t on the device as the first columns of a [rows, ld] buffer (the rest: fill)"""
    buf = torch.full((t.shape[0], ld), fill, dtype=torch.float32, device=dev())
    buf[:, :t.shape[1]] = t.to(dev())
    return buf[:, :t.shape[1]]


def to_dev(t):
    return None if t is None else t.to(dev())


def launch(fn, x, C, labels, soft, keep, ld, bf16, gscale, row_g, **opts):
    """forward (row_loss) and gradient launches of `fn` (a row-form wrapper of afft_amd.ops).  Returns loss [rows], the [rows, ld]
    gradient block and whether the sentinel rows around it survived."""
    rows = x.shape[0]
    xd = framed(x, ld)
    kw = dict(labels=to_dev(labels), soft=to_dev(soft), keep=to_dev(keep), **opts)
    rl = torch.full((rows,), SENT, device=dev())
    fn(xd, C, row_loss=rl, **kw)
    dbuf = torch.full((rows + 2, ld), SENT, dtype=torch.bfloat16 if bf16 else torch.float32, device=dev())
    fn(xd, C, dlogits=dbuf[1:rows + 1], gscale=gscale, row_g=to_dev(row_g), **kw)
    border = bool((dbuf[0] == SENT).all()) and bool((dbuf[-1] == SENT).all())
    return rl.cpu(), dbuf[1:rows + 1].float().cpu(), border


def ratios(loss, dblock, ref, C, bf16):
    """worst |got - ref| / (u S) of the loss and of the gradient over the rows where S > 0; asserts the exact properties: rows of
    S == 0 (ignored, or A == 0) are exactly 0, the pad columns are exactly 0, nothing is NaN"""
    zero = (ref["s_loss"] == 0) | ~ref["kept"]
    assert bool((loss[zero] == 0).all()) and bool((dblock[zero] == 0).all()), "a row that is ignored or whose A is 0 must be exactly 0"
    assert bool((dblock[:, C:] == 0).all()), "pad columns"
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dblock).all())
    live = ~zero
    if not bool(live.any()):
        return 0.0, 0.0
    r_loss = float(((loss.double() - ref["loss"]).abs()[live] / (U * ref["s_loss"][live])).max())
    err = (dblock[:, :C].double() - ref["grad"]).abs()
    if bf16:
        err = (err - 2.0 ** -8 * ref["grad"].abs()).clamp(min=0)
    g_live = ref["s_grad"] > 0
    assert bool((err[~g_live] == 0).all())
    r_grad = float((err[g_live] / (U * ref["s_grad"][g_live, None])).max()) if bool(g_live.any()) else 0.0
    return r_loss, r_grad


class Recorder:
    """stands in for the six cross-entropy wrappers of afft_amd.ops: notes every call as (name, (logits, C), keywords); the plain ones
    compute by tests/cpu_ops.py, the _w ones by the float64 double of ce_double.py, the _focal ones by that of focal_double.py"""
    NAMES = ("softmax_ce", "softmax_ce_frames", "softmax_ce_w", "softmax_ce_frames_w", "softmax_ce_focal", "softmax_ce_frames_focal")

    def __init__(self, monkeypatch):
        from afft_amd import ops
        self.calls = []
        for name in self.NAMES:
            monkeypatch.setattr(ops, name, self._stub(name))

    def _stub(self, name):
        def call(logits, C_, **kw):
            self.calls.append((name, (logits, C_), kw))
            if not name.endswith(("_w", "_focal")):
                return getattr(cpu_ops, name)(logits, C_, **kw)
            with torch.no_grad():
                d = kw.get("dlogits3" if "frames" in name else "dlogits")
                d2 = None if d is None else torch.zeros(d.numel() // d.shape[-1], d.shape[-1])
                self._double(name, logits.reshape(-1, logits.shape[-1]), C_, kw, d2)
                if d is not None:
                    d.copy_(d2.view(d.shape))
        return call

    @staticmethod
    def _double(name, x2, C_, kw, d2):
        common = dict(labels=kw.get("labels"), soft=kw.get("soft"), keep=kw.get("keep"), weight=kw.get("weight"),
                      eps=kw.get("smoothing", 0.0), gscale=kw.get("gscale", 1.0), row_g=kw.get("row_g"))
        if name.endswith("_focal"):
            got = focal_double.focal(x2[:, :C_], adjust=kw.get("adjust"), gamma=kw.get("gamma", 0.0), **common)
        else:
            got = ce_double.ce(x2[:, :C_], **common)
        if kw.get("row_loss") is not None:
            kw["row_loss"].copy_(got["loss"])
        if kw.get("loss_sum") is not None:
            kw["loss_sum"] += got["loss"].sum()
        if d2 is not None:
            d2[:, :C_].copy_(got["grad"])
