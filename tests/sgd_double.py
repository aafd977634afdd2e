"""Restatement of the momentum-SGD update (include/afft_hip.h: afft_sgd_fused_t, afft_sgd_nesterov2; torch.optim.SGD with dampening 0)
in plain torch float64, with the weight images the update kernels keep beside the fp32 parameters, for the GPU tests of the flat
kernel, the runs kernel and the fused GEMM epilogue.  Nothing here calls the library.

    g'  = gscale * g + wd * p
    buf = g'                         on the first step (AFFT_SGD_FIRST_STEP), else  mom * buf + g'
    p  -= lr * buf                   with plain momentum (AFFT_SGD_PLAIN_MOMENTUM), else  p -= lr * (g' + mom * buf)

Images of the fp32 p: bf16 and fp16 = p rounded once; e4m3 = (256 p) clamped to +-448, rounded once to float8_e4m3fn; packed = the
bf16 image in the fragment order of afft_pack_weight."""
import torch

FIRST_STEP, PLAIN_MOMENTUM = 1, 2
FLAG_WORDS = (0, FIRST_STEP, PLAIN_MOMENTUM, FIRST_STEP | PLAIN_MOMENTUM)
U = 2.0 ** -24      # fp32 unit roundoff


def f32(x):
    """the fp32 number a float hyperparameter becomes on its way into the kernel, as a Python float"""
    return float(torch.tensor(x, dtype=torch.float32))


def sgd_stages(p, buf, g, lr, mom, wd, gscale, flags):
    """float64 intermediates of one update, in the order the device function forms them: {wdp, g1 (= g'), buf, step (what lr
    multiplies), p}.  p, buf, g: tensors of any float dtype (taken as they are, in float64); on a first step buf is not read"""
    p, g = p.double(), g.double()
    wdp = wd * p
    g1 = gscale * g + wdp
    nbuf = g1 if flags & FIRST_STEP else mom * buf.double() + g1
    step = nbuf if flags & PLAIN_MOMENTUM else g1 + mom * nbuf
    return dict(wdp=wdp, g1=g1, buf=nbuf, step=step, p=p - lr * step)


def sgd_ref(p, buf, g, lr, mom, wd, gscale, flags):
    """(new p, new buf) in float64"""
    s = sgd_stages(p, buf, g, lr, mom, wd, gscale, flags)
    return s["p"], s["buf"]


def sgd_bound(p, buf, g, lr, mom, wd, gscale, flags, dg=None):
    """(bound on |p_kernel - p_ref|, bound on |buf_kernel - buf_ref|), elementwise, for fp32 inputs and fp32 hyperparameters.
    sgd_update rounds five times (four with plain momentum, fewer on a first step); each rounding errs by at most u times the
    magnitude of its exact result, and u times the float64 magnitude (1 + 5u, absorbed by the factor 1.001) bounds that:
        t = fl(wd p)                 e_t <= u |wd p|
        g' = fl(gscale g + t)        e_g <= e_t + u |g'|                                  (+ gscale dg: an error dg of the gradient itself)
        b = fl(mom buf + g')         e_b <= e_g + u |b|            (first step: b = g', e_b = e_g)
        s = fl(mom b + g')           e_s <= mom e_b + e_g + u |s|  (plain momentum: s = b, e_s = e_b)
        p = fl(p - lr s)             e_p <= lr e_s + u |p_new|
    so a gradient error reaches buf times gscale and p times lr gscale (1 + mom) (Nesterov) or lr gscale (plain momentum)."""
    s = sgd_stages(p, buf, g, lr, mom, wd, gscale, flags)
    e_t = U * s["wdp"].abs()
    e_g = e_t + U * s["g1"].abs() + (0.0 if dg is None else abs(gscale) * dg)
    e_b = e_g if flags & FIRST_STEP else e_g + U * s["buf"].abs()
    e_s = e_b if flags & PLAIN_MOMENTUM else abs(mom) * e_b + e_g + U * s["step"].abs()
    e_p = abs(lr) * e_s + U * s["p"].abs()
    return 1.001 * e_p, 1.001 * e_b


def bf16_image(p32):
    return p32.float().to(torch.bfloat16)


def f16_image(p32):
    return p32.float().to(torch.float16)


def e4m3_image(p32):
    """bytes of e4m3(2^8 p): the scaling is exact, values beyond the format's 448 saturate, one rounding to nearest even"""
    q = (p32.float().cpu() * 256.0).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    return q.to(p32.device)


def images(p32):
    """{bf16, f16, f8}: the three row-major images of the fp32 parameters p32, same shape"""
    return dict(bf16=bf16_image(p32), f16=f16_image(p32), f8=e4m3_image(p32))


def packed_frag(rows, cols, device="cpu"):
    """int64 [rows, cols]: the element of the fragment-packed image (afft_pack_weight, include/afft_hip.h) that holds W[m][n], from the
    documented layout  dst[((rb * (cols / 32) + ks) * 64 + lane) * 8 + j] = W[16 rb + (lane & 15)][32 ks + 8 (lane >> 4) + j]:
    every dst index is enumerated with its source element and the table is filled from that list"""
    assert rows % 16 == 0 and cols % 32 == 0
    dst = torch.arange(rows * cols, device=device)
    j, lane, blk = dst % 8, (dst // 8) % 64, dst // 512
    ks, rb = blk % (cols // 32), blk // (cols // 32)
    m, n = 16 * rb + (lane & 15), 32 * ks + 8 * (lane >> 4) + j
    table = torch.full((rows, cols), -1, dtype=torch.int64, device=device)
    table[m, n] = dst
    assert int(table.min()) == 0      # a permutation: every element has its place
    return table


def packed_image(p32):
    """the fragment-packed bf16 image of p32 [rows, cols], flat"""
    out = torch.empty(p32.numel(), dtype=torch.bfloat16, device=p32.device)
    out[packed_frag(*p32.shape, device=p32.device).reshape(-1)] = bf16_image(p32).reshape(-1)
    return out
