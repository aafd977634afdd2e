"""CPU: the host checks of the six cross-entropy entry points of the C-ABI (afft_softmax_ce, _frames, _w, _frames_w, _focal,
_frames_focal; csrc/loss.hip).  Every check returns before the first HIP call, so no GPU is needed and nothing is dereferenced: the
pointers are dummy integers.  Each case gives one bad argument and pins the return code 1 and the WHOLE last-error string -- the name
in front of a message is that of the narrowest entry that serves the options (a focal call with gamma 0 and no adjustment reports as
softmax_ce_w, and as softmax_ce when weight is null and smoothing 0 as well), except for the gamma check, which comes first and
carries the focal entry's name; the smoothing check comes before the null-logits check.  An empty problem returns 0."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 7
PTR = 0x1000      # a non-null pointer that nothing reads
ENTRIES = ["softmax_ce", "softmax_ce_frames", "softmax_ce_w", "softmax_ce_frames_w", "softmax_ce_focal", "softmax_ce_frames_focal"]
W_ENTRIES, FOCAL_ENTRIES = ENTRIES[2:], ENTRIES[4:]
ROW_ENTRIES, FRAME_ENTRIES = ENTRIES[0::2], ENTRIES[1::2]
ONE_OF = "give exactly one of labels / soft targets"
LOSS_SUM = "loss_sum is the ordered sum of row_loss: give row_loss as well"


@pytest.fixture(scope="module")
def lib():
    from afft_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "afft_amd", "csrc"), "-j4"])
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        fn = getattr(so, "afft_" + name)
        fn.argtypes, fn.restype = _lib._SIGS["afft_" + name]
    so.afft_last_error.argtypes, so.afft_last_error.restype = [], ctypes.c_char_p
    return so


def call(lib, name, **over):
    """the entry `name` with valid arguments for C classes and a gradient, and the options that select its own kernel (smoothing 0.1
    for the _w entries; gamma 2 as well for the focal ones), but for `over`.  The problem is EMPTY (0 rows; 0 clips of 3 frames): the
    checks come before the empty-problem exit, so a case that passes a check it should fail still launches nothing on the dummy
    pointers.  Returns (return code, last error)."""
    a = dict(logits=PTR, clip_stride=3 * C, ldl=C, rows=0, clips=0, frames=3, C=C, labels=PTR, soft=None, lds=0, keep=None, gscale=1.0,
             row_g=None, loss_sum=None, dlogits=PTR, d_clip_stride=3 * C, ldd=C, d_dtype=0, row_loss=PTR, weight=None, smoothing=0.1,
             adjust=None, gamma=2.0)
    assert set(over) <= set(a), over
    a.update(over)
    if "frames" in name:
        args = [a[k] for k in ("logits", "clip_stride", "ldl", "clips", "frames", "C", "labels", "soft", "lds", "keep", "gscale", "row_g",
                               "dlogits", "d_clip_stride", "ldd", "d_dtype", "row_loss")]
    else:
        args = [a[k] for k in ("logits", "ldl", "rows", "C", "labels", "soft", "lds", "keep", "gscale", "row_g", "loss_sum", "dlogits",
                               "ldd", "d_dtype", "row_loss")]
    if name in W_ENTRIES:
        args += [a["weight"], a["smoothing"]]
    if name in FOCAL_ENTRIES:
        args += [a["adjust"], a["gamma"]]
    rc = getattr(lib, "afft_" + name)(*args, None)
    return rc, lib.afft_last_error().decode()


def g(v):
    """C's %g of the float the library receives"""
    return "%g" % ctypes.c_float(v).value


@pytest.mark.parametrize("name", ENTRIES)
def test_one_bad_argument_gives_code_1_and_the_entry_s_message(lib, name):
    bad = [(dict(logits=None), "null logits"),
           (dict(soft=PTR, lds=C), ONE_OF),
           (dict(labels=None), ONE_OF),
           (dict(ldl=C - 1), "bad sizes"),
           (dict(ldd=C - 1), "bad sizes"),
           (dict(C=0), "bad sizes")]
    if name in ROW_ENTRIES:
        bad.append((dict(loss_sum=PTR, row_loss=None), LOSS_SUM))
    else:
        bad.append((dict(frames=0), "bad sizes"))
    for over, text in bad:
        assert call(lib, name, **over) == (1, f"{name}: {text}"), over
    assert call(lib, name, ldd=C - 1, dlogits=None)[0] == 0      # ldd is looked at only with a gradient


@pytest.mark.parametrize("name", W_ENTRIES)
@pytest.mark.parametrize("eps", [-0.1, 1.5, float("nan")])
def test_smoothing_outside_0_1(lib, name, eps):
    want = (1, f"{name}: smoothing must lie in [0, 1] (got {g(eps)})")
    assert call(lib, name, smoothing=eps) == want
    assert call(lib, name, smoothing=eps, weight=PTR) == want
    assert call(lib, name, smoothing=eps, logits=None, ldl=0) == want      # before the null-logits check
    if name in FOCAL_ENTRIES:      # gamma 0, no adjustment: the _w entry's check, under its name
        assert call(lib, name, smoothing=eps, gamma=0.0) == (1, f"{name[:-6]}_w: smoothing must lie in [0, 1] (got {g(eps)})")


@pytest.mark.parametrize("name", FOCAL_ENTRIES)
@pytest.mark.parametrize("gamma", [-1.0, float("inf"), float("nan")])
def test_gamma_not_finite_or_negative(lib, name, gamma):
    want = (1, f"{name}: gamma must be finite and >= 0 (got {g(gamma)})")
    assert call(lib, name, gamma=gamma) == want
    assert call(lib, name, gamma=gamma, adjust=PTR) == want
    assert call(lib, name, gamma=gamma, smoothing=1.5, logits=None) == want      # the first check of all
    assert call(lib, name, gamma=gamma, smoothing=0.0) == want                   # whatever the other options


@pytest.mark.parametrize("form", ["softmax_ce", "softmax_ce_frames"])
def test_the_name_printed_is_that_of_the_narrowest_entry_that_serves_the_options(lib, form):
    """gamma 0 and no adjustment is the _w call; no weight and smoothing 0 is the plain call"""
    for over, text in ((dict(ldl=C - 1), "bad sizes"), (dict(logits=None), "null logits"), (dict(labels=None), ONE_OF)):
        assert call(lib, form + "_focal", gamma=0.0, **over) == (1, f"{form}_w: {text}")
        assert call(lib, form + "_focal", gamma=0.0, smoothing=0.0, weight=PTR, **over) == (1, f"{form}_w: {text}")
        assert call(lib, form + "_focal", gamma=0.0, smoothing=0.0, **over) == (1, f"{form}: {text}")
        assert call(lib, form + "_w", smoothing=0.0, **over) == (1, f"{form}: {text}")
        # an adjustment alone, or a weight alone, keeps the entry's own name
        assert call(lib, form + "_focal", gamma=0.0, smoothing=0.0, adjust=PTR, **over) == (1, f"{form}_focal: {text}")
        assert call(lib, form + "_w", smoothing=0.0, weight=PTR, **over) == (1, f"{form}_w: {text}")
    if form == "softmax_ce":
        assert call(lib, form + "_focal", gamma=0.0, smoothing=0.0, loss_sum=PTR, row_loss=None) == (1, f"{form}: {LOSS_SUM}")
        assert call(lib, form + "_focal", gamma=0.0, loss_sum=PTR, row_loss=None) == (1, f"{form}_w: {LOSS_SUM}")
    else:
        assert call(lib, form + "_focal", gamma=0.0, smoothing=0.0, frames=0) == (1, f"{form}: bad sizes")
        assert call(lib, form + "_focal", gamma=0.0, frames=0) == (1, f"{form}_w: bad sizes")


@pytest.mark.parametrize("name", ENTRIES)
def test_an_empty_problem_returns_0(lib, name):
    """rows == 0 / clips == 0 with otherwise valid arguments, in every forwarding case: nothing is launched"""
    for over in (dict(), dict(smoothing=0.0), dict(gamma=0.0), dict(gamma=0.0, smoothing=0.0), dict(weight=PTR, adjust=PTR),
                 dict(loss_sum=PTR), dict(dlogits=None, ldd=0)):
        assert call(lib, name, **over)[0] == 0, over
