"""GPU: afft_topk_rows (afft_amd/csrc/metrics.hip) against tests/topk_double.py, the float64 / int64 numpy restatement of the ORDER
that include/afft_hip.h defines (value descending with -0.0 == +0.0, the lower class first among equal values, NaN last).

Every comparison is exact: the indices are integers, and the values are gathered, never computed, so they are compared bit for bit
(view(int32): the sign of a zero and the payload of a NaN included).  Every output buffer lies between sentinels, and the columns
>= k of a wider buffer must still hold theirs.

Shapes (rows, C, k): the smallest at which each part can go wrong -- one class; C around the wave (63 / 64 / 65) and the workgroup
(255 / 256 / 257: the power-of-two padding is empty, or almost all of the second half); k = C; EK100's 3806; both sides of 4096;
the limit 8192 (64 KiB of LDS, the raised dynamic-LDS attribute); more rows than CUs."""
import numpy as np
import pytest
import torch

import topk_double

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1, 1), (3, 2, 2), (2, 63, 5), (2, 64, 64), (2, 65, 1), (3, 255, 100), (3, 256, 100), (3, 257, 257), (2, 100, 100),
          (2, 3806, 100), (1, 4096, 4096), (1, 4097, 100), (1, 8192, 8192), (300, 211, 5)]
KINDS = ["tie_free", "seven_values", "constant", "specials", "nans"]
FORMS = ["plain", "pitch3", "offset1", "middle", "wide_out"]
GUARD = 64
VAL_SENTINEL, IDX_SENTINEL = -12345.5, -7


def make_values(kind, rows, C, seed):
    g = np.random.default_rng(seed)
    if kind == "tie_free":
        return (np.stack([g.permutation(C) for _ in range(rows)]).astype(np.float32) - np.float32(C // 2)) * np.float32(0.37)
    if kind == "seven_values":
        return g.choice(np.asarray([-2.5, -1.0, 0.0, 0.25, 1.0, 3.0, 7.5], np.float32), size=(rows, C))
    if kind == "constant":
        return np.full((rows, C), 1.5, np.float32)
    if kind == "specials":         # both infinities, the two zeros side by side, denormals of both signs, the largest finite numbers
        pool = np.asarray([np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.17549435e-38, 1.0, -1.0, 3.4028235e38, -3.4028235e38],
                          np.float32)
        x = g.choice(pool, size=(rows, C))
        x[:, 0:C:5] = np.float32(-0.0)
        x[:, 1:C:5] = np.float32(0.0)
        return x
    if kind == "nans":             # per row: NaNs at the front / at the back / throughout / everywhere; two payloads and both signs
        x = g.standard_normal((rows, C)).astype(np.float32)
        x[:, C // 2:] = np.round(x[:, C // 2:])                  # ties among the numbers as well
        nans = np.asarray([0x7FC00000, 0xFFC00000, 0x7FC00001, 0x7F800001], np.uint32).view(np.float32)
        for r in range(rows):
            pat = (r + (2 if rows == 1 else 0)) % 4
            where = [slice(0, max(C // 3, 1)), slice(C - max(C // 3, 1), C), slice(0, C, 2), slice(0, C)][pat]
            n = len(range(*where.indices(C)))
            x[r, where] = nans[np.arange(n) % 4]
        return x
    raise ValueError(kind)


def place(x, form):
    """the rows of x on the device in memory form `form`; returns the [rows, C] view the kernel is given"""
    rows, C = x.shape
    xd = torch.tensor(x, device=DEV)        # a copy: the shared reference arrays are read-only
    if form in ("plain", "wide_out"):
        return xd
    if form == "pitch3":           # ldx = C + 3: rows 2.. are not 16-byte aligned -> scalar loads
        buf = torch.full((rows, C + 3), float("nan"), device=DEV)
        view = buf[:, :C]
    elif form == "offset1":        # base off by one float
        flat = torch.full((rows * C + 1,), float("nan"), device=DEV)
        view = flat[1:].view(rows, C)
    elif form == "middle":         # [:, 0, :] of a (rows, 2, pitch) tensor, pitch a multiple of 4: 16-byte loads on a strided view
        pitch = (C + 3) // 4 * 4 + 4
        buf = torch.full((rows, 2, pitch), float("nan"), device=DEV)
        view = buf[:, 0, :C]
        assert view.stride(0) == 2 * pitch or rows == 1
    else:
        raise ValueError(form)
    view.copy_(xd)
    return view


def guarded(rows, ld, dtype, fill):
    flat = torch.full((2 * GUARD + rows * ld,), fill, dtype=dtype, device=DEV)
    return flat, flat[GUARD:GUARD + rows * ld].view(rows, ld)


def run(view, k, extra=0):
    """ops.topk_rows into guarded buffers of k + extra columns; checks the sentinels; returns numpy (vals [rows, k], idx [rows, k])"""
    from afft_amd import ops
    rows = view.shape[0]
    vflat, vals = guarded(rows, k + extra, torch.float32, VAL_SENTINEL)
    iflat, idx = guarded(rows, k + extra, torch.int32, IDX_SENTINEL)
    got = ops.topk_rows(view, k, vals=vals, idx=idx)
    assert got[0] is vals and got[1] is idx
    v, i = vflat.cpu().numpy(), iflat.cpu().numpy()
    for flat, fill in ((v, VAL_SENTINEL), (i, IDX_SENTINEL)):
        assert (flat[:GUARD] == fill).all() and (flat[-GUARD:] == fill).all(), "wrote outside its buffer"
        assert (flat[GUARD:-GUARD].reshape(rows, k + extra)[:, k:] == fill).all(), "wrote a column >= k"
    return v[GUARD:-GUARD].reshape(rows, k + extra)[:, :k], i[GUARD:-GUARD].reshape(rows, k + extra)[:, :k]


_REFERENCE = {}


def reference(kind, shape):
    """(x, vals, idx) of one (kind, shape), computed once and shared, never written to"""
    key = (kind, shape)
    if key not in _REFERENCE:
        rows, C, k = shape
        x = make_values(kind, rows, C, seed=1000 * C + 10 * rows + KINDS.index(kind))
        vals, idx = topk_double.topk(x, k)
        for a in (x, vals, idx):
            a.setflags(write=False)
        _REFERENCE[key] = (x, vals, idx)
    return _REFERENCE[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matches_the_restatement_in_every_memory_form(shape, kind):
    rows, C, k = shape
    x, want_vals, want_idx = reference(kind, shape)
    for form in FORMS:
        vals, idx = run(place(x, form), k, extra=3 if form == "wide_out" else 0)
        assert np.array_equal(idx.astype(np.int64), want_idx), (form, np.argwhere(idx != want_idx)[:4])
        assert np.array_equal(vals.view(np.int32), want_vals.view(np.int32)), form
    if kind == "constant":
        assert np.array_equal(want_idx, np.tile(np.arange(k), (rows, 1)))
    if kind == "nans" and rows >= 4:
        assert np.array_equal(want_idx[3], np.arange(k))        # the all-NaN row: class order


def test_the_restatement_orders_by_hand():
    """the double against the header's rules on a row small enough to order by hand (no kernel involved beyond the comparison)"""
    x = np.asarray([[0.0, np.nan, -np.inf, 2.0, -0.0, np.inf, 2.0, 1e-45, np.nan, -1e-45]], np.float32)
    want = [5, 3, 6, 7, 0, 4, 9, 2, 1, 8]
    assert topk_double.order(x[0]).tolist() == want
    vals, idx = run(torch.from_numpy(x).to(DEV), 10)
    assert idx[0].tolist() == want and np.array_equal(vals.view(np.int32), x[:, want].view(np.int32))


def test_two_runs_are_bitwise_equal():
    for shape, kind in (((2, 3806, 100), "tie_free"), ((300, 211, 5), "seven_values"), ((1, 8192, 8192), "nans")):
        x = reference(kind, shape)[0]
        view = place(x, "plain")
        a, b = run(view, shape[2]), run(view, shape[2])
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_agrees_with_label_rank_on_tied_rows():
    """the same total order as afft_label_rank: where rank < k, the label sits at position rank"""
    from afft_amd import ops
    shape = (300, 211, 5)
    rows, C, k = shape
    x = reference("seven_values", shape)[0]
    labels = np.random.default_rng(5).integers(0, C, rows).astype(np.int64)
    best = reference("seven_values", shape)[2]
    labels[:2 * k] = best[np.arange(2 * k), np.arange(2 * k) % k]         # labels that are hits at every position 0 .. k - 1
    xd = torch.tensor(x, device=DEV)
    rank = torch.empty(rows, dtype=torch.int32, device=DEV)
    lab = torch.empty(rows, dtype=torch.int64, device=DEV)
    ops.label_rank(xd, C, labels=torch.from_numpy(labels).to(DEV), k=k, rank=rank, label_out=lab)
    _, idx = run(xd, k)
    rank = rank.cpu().numpy()
    hit = rank < k
    assert hit[:2 * k].all() and rank[:2 * k].tolist() == (np.arange(2 * k) % k).tolist() and (~hit).any()
    assert np.array_equal(idx[np.flatnonzero(hit), rank[hit]], labels[hit])
    for r in np.flatnonzero(~hit):
        assert labels[r] not in idx[r]


def test_refusals():
    from afft_amd import _lib as L
    from afft_amd import ops
    x = torch.zeros(4, 5, device=DEV)
    with pytest.raises(RuntimeError, match=r"1 <= k <= C <= 8192 \(got k = 0, C = 5\)"):
        ops.topk_rows(x, 0)
    with pytest.raises(RuntimeError, match=r"1 <= k <= C <= 8192 \(got k = 6, C = 5\)"):
        ops.topk_rows(x, 6)
    with pytest.raises(RuntimeError, match=r"1 <= k <= C <= 8192 \(got k = 1, C = 8193\)"):
        ops.topk_rows(torch.zeros(1, 8193, device=DEV), 1)
    vals = torch.full((4, 2), VAL_SENTINEL, device=DEV)
    idx = torch.full((4, 3), IDX_SENTINEL, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="ldv 2 < k = 3"):
        ops.topk_rows(x, 3, vals=vals, idx=idx)
    with pytest.raises(RuntimeError, match="ldi 2 < k = 3"):
        ops.topk_rows(x, 3, vals=torch.zeros(4, 3, device=DEV), idx=torch.zeros(4, 2, dtype=torch.int32, device=DEV))
    s = torch.cuda.current_stream().cuda_stream
    rc = L.lib().afft_topk_rows(x.data_ptr(), 4, 4, 5, 1, vals.data_ptr(), 2, idx.data_ptr(), 3, s)
    assert rc != 0 and b"ldx 4 < C = 5" in L.lib().afft_last_error()
    rc = L.lib().afft_topk_rows(x.data_ptr(), 5, 0, 5, 1, vals.data_ptr(), 2, idx.data_ptr(), 3, s)
    assert rc != 0 and b"rows >= 1" in L.lib().afft_last_error()
    rc = L.lib().afft_topk_rows(x.data_ptr(), 5, 4, 5, 1, None, 2, idx.data_ptr(), 3, s)
    assert rc != 0 and b"null" in L.lib().afft_last_error()
    # the wrapper's own errors: not fp32, columns not contiguous
    with pytest.raises(TypeError, match="fp32"):
        ops.topk_rows(x.to(torch.bfloat16), 1)
    with pytest.raises(TypeError, match="fp32"):
        ops.topk_rows(x.double(), 1)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.topk_rows(torch.zeros(5, 4, device=DEV).t(), 1)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.topk_rows(torch.zeros(4, 10, device=DEV)[:, ::2], 1)
    torch.cuda.synchronize()
    assert (vals == VAL_SENTINEL).all() and (idx == IDX_SENTINEL).all()          # nothing was launched
