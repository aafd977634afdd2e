"""The GEMM case table shared by the kernel-vs-float64 GEMM section of test_kernels_gpu.py and the coverage and dispatch checks of
test_gemm_coverage_cpu.py: for every case the layout, shape, precision mode, forced dispatch, epilogue -- and the kernel
instantiation the dispatcher must run for it, written the way `nm -C` prints the symbol.  Every `gemm_*_kernel<...>`
instantiation the library compiles is the expected kernel of at least one case (test_gemm_coverage_cpu.py).  Below the table: the
operand geometry of a case (pitches, plane offsets: what dispatch depends on), shared by the GPU test, which allocates such operands,
and the CPU test, which asks afft_gemm_plan_for about a descriptor of them.

layout: nt (A[M][K], B[N][K]), nn (A[M][K], B[K][N]), tn (A[K][M], B[K][N]), tt (A[K][M], B[N][K]: exact-fp32 kernel only).
mode:   bf16           plain bf16 operands (the fast path, or the exact-fp32 kernel where the fast path refuses the problem)
        f32            fp32 operands: the exact-fp32 kernel
        bf16x3         two-plane bf16 splits of both operands (afft_gemm_t.split3 = 1)
        fp16x2         two-plane fp16 split of A, fp16 B (split3 = 2)
        fp16           one fp16 pass (split3 = 4)
        fp16_lo8       fp16 hi pass + e4m3 lo pass (split3 = 3)
variant / splitk: afft_set_gemm_variant / afft_set_gemm_splitk for the launch (0 / 1 = automatic).
epi:    alpha (float), bias, rowscale, residual, accumulate (bools), act (AFFT_ACT_* code), pre / out2 ("f32" / "bf16" / "f16"),
        out ("f32", "bf16" or "f16"; default f32), out_lo / out_lo8 (bools: fp16 plane outputs), packed (B also as the
        fragment-packed image: afft_gemm_t.b_packed), ldo (row pitch of every output-shaped view), col0 (element offset of those
        views inside their rows: 0 -> 16-byte aligned), a_off (A's base one element off 16-byte alignment).
        sgd: the product is the gradient of a weight and is consumed by the fused momentum-SGD update (afft_gemm_t.sgd) instead of
        being stored; no other stage beside it.  A dict: flags (AFFT_SGD_* word), images (which of the weight's images the update
        keeps: bf16, f16, f8 row-major, pk fragment-packed: M % 16 == 0 and ldo % 32 == 0), ok (None: no flag, 1 / 0: the device flag
        that lets the update happen / makes it a no-op) and optionally alpha, ldo, col0 with the meaning above: p, buf and the
        row-major images all have the output's geometry.
ld:     leading dimension of both k-strided operands (0 = a small padding past the logical width): the 32-bit walk cases.
amp, sh: operand values are integers in [-amp, amp] times 2^-sh (exact in every operand format; see the GPU test)."""
from __future__ import annotations

from dataclasses import dataclass, field

GELU_ERF, GELU_TANH, DGELU_ERF, DGELU_TANH, RELU, SIGMOID_GATE = 1, 2, 3, 4, 5, 6


@dataclass
class GemmCase:
    name: str
    layout: str
    M: int
    N: int
    K: int
    kernel: str
    mode: str = "bf16"
    variant: int = 0
    splitk: int = 1
    epi: dict = field(default_factory=dict)
    ld: int = 0
    amp: int = 2
    sh: int = 0

    @property
    def fast(self) -> bool:
        """runs on a bf16 / fp16 MFMA kernel (one trace record) rather than the exact-fp32 kernel (none)"""
        return not self.kernel.startswith("gemm_f32_kernel")


def _c(name, layout, M, N, K, kernel, **kw):
    return GemmCase(name, layout, M, N, K, kernel, **kw)


# kernel symbols as `nm -C` prints them
def _b(x):
    return "true" if x else "false"


def gen(a_ks, b_ks, splitk=False, x3=0, stages=2):
    return f"gemm_bf16_kernel<2, 2, {stages}, {_b(a_ks)}, {_b(b_ks)}, {_b(splitk)}, {x3}>"


def g2(a_ks, b_ks, splitk=False, f16=False):
    return f"gemm_bf16_g2_kernel<{_b(a_ks)}, {_b(b_ks)}, {_b(splitk)}, {_b(f16)}>"


def pp(a_ks, b_ks, x3=0):
    return f"gemm_bf16_pp_kernel<{_b(a_ks)}, {_b(b_ks)}, {x3}>"


def pp2(a_ks, b_ks, x3=0):
    return f"gemm_bf16_pp2_kernel<{_b(a_ks)}, {_b(b_ks)}, {x3}>"


def bd(rows160, packed):
    return f"gemm_bf16_bd_kernel<{10 if rows160 else 16}, 3, {2 if rows160 else 1}, {_b(packed)}>"


F32_FLOAT = "gemm_f32_kernel<float>"
F32_BF16 = "gemm_f32_kernel<unsigned short>"

NT, NN, TN = (False, False), (False, True), (True, True)

# AFFT_SGD_* flag words (include/afft_hip.h)
NESTEROV, FIRST, PLAIN = 0, 1, 2


def _sgd(flags, images, ok=None, **geometry):
    """the epilogue of a case whose product is consumed by the fused optimizer update: see `sgd` in the module docstring"""
    return dict(sgd=dict(flags=flags, images=tuple(images.split()), ok=ok, **geometry))


# the kernel families a weight gradient can reach: each is the expected kernel of at least one `sgd` case (test_gemm_coverage_cpu.py)
SGD_FAMILIES = [gen(*TN), gen(*TN, splitk=True), g2(*TN), g2(*TN, splitk=True), pp(*TN), pp2(*TN), gen(*TN, x3=1), pp(*TN, 1), pp2(*TN, 1),
                gen(*TN, stages=4), F32_FLOAT, F32_BF16]

# plane-output operands: values with more significant bits than fp16 holds, so that the lo plane is not zero
_LO = dict(amp=16, sh=3)

CASES = [
    # ---- the cfg2 step's forward GEMMs (profiles/r06_gemm_forward_by_shape.txt), bf16, automatic dispatch
    _c("fwd_fc1", "nt", 5120, 8192, 2048, pp2(*NT), epi=dict(bias=True, act=GELU_ERF, pre="bf16", out="bf16")),
    _c("fwd_fc2", "nt", 5120, 2048, 8192, pp2(*NT), epi=dict(bias=True, residual=True)),
    _c("fwd_fc2_packed", "nt", 5120, 2048, 8192, bd(True, True), epi=dict(bias=True, residual=True, packed=True)),
    _c("fwd_qkv", "nt", 5120, 6144, 2048, pp2(*NT), epi=dict(out="bf16")),
    _c("fwd_proj_packed", "nt", 5120, 2048, 2048, bd(True, True), epi=dict(bias=True, residual=True, rowscale=True, packed=True)),
    _c("fwd_pred_fc2_nn", "nn", 1024, 2048, 8192, g2(*NN, splitk=True), epi=dict(bias=True, residual=True)),
    _c("fwd_pred_fc1_nn", "nn", 1024, 8192, 2048, g2(*NN), epi=dict(bias=True, out="bf16")),
    _c("fwd_pred_qkv_nn", "nn", 1024, 6144, 2048, g2(*NN)),
    _c("fwd_pred_proj_nn", "nn", 1024, 2048, 2048, g2(*NN, splitk=True), epi=dict(bias=True, residual=True)),
    _c("fwd_pred_fc2_nt", "nt", 1024, 2048, 8192, g2(*NT, splitk=True)),
    _c("fwd_classifier", "nt", 1088, 3806, 2048, gen(*NT), epi=dict(bias=True, ldo=3840)),
    _c("fwd_pred_fc1_nt", "nt", 1024, 8192, 2048, g2(*NT), epi=dict(out="bf16")),
    _c("fwd_pred_proj_nt", "nt", 1024, 2048, 2048, g2(*NT, splitk=True), epi=dict(bias=True)),
    # ---- the same forward GEMMs in the fp16x2 precision (split3 as the profile lists them)
    _c("f16_fwd_fc1_lo8", "nt", 5120, 8192, 2048, pp2(*NT, 3), mode="fp16_lo8", sh=6, epi=dict(bias=True, out="f16", out_lo8=True)),
    _c("f16_fwd_fc2_one_pass", "nt", 5120, 2048, 8192, pp2(*NT, 2), mode="fp16", epi=dict(bias=True, residual=True)),
    _c("f16_fwd_qkv_lo8", "nt", 5120, 6144, 2048, pp2(*NT, 3), mode="fp16_lo8", sh=6),
    _c("f16_fwd_proj_lo8", "nt", 5120, 2048, 2048, pp2(*NT, 3), mode="fp16_lo8", sh=6, epi=dict(bias=True, residual=True)),
    _c("f16_fwd_qkv_two_pass", "nt", 5120, 6144, 2048, pp2(*NT, 2), mode="fp16x2"),
    _c("f16_fwd_pred_fc2_nn", "nn", 1024, 2048, 8192, g2(*NN, splitk=True, f16=True), mode="fp16", epi=dict(bias=True, residual=True)),
    _c("f16_fwd_pred_fc1_nn", "nn", 1024, 8192, 2048, g2(*NN, f16=True), mode="fp16", epi=dict(bias=True)),
    _c("f16_fwd_pred_proj_nn", "nn", 1024, 2048, 2048, g2(*NN, splitk=True, f16=True), mode="fp16"),
    _c("f16_fwd_pred_fc1_nt_two_pass", "nt", 1024, 8192, 2048, gen(*NT, x3=2), mode="fp16x2", epi=dict(bias=True)),
    _c("f16_fwd_classifier_two_pass", "nt", 1088, 3806, 2048, gen(*NT, x3=2), mode="fp16x2", epi=dict(bias=True, ldo=3840)),
    _c("f16_fwd_pred_fc2_nt", "nt", 1024, 2048, 8192, g2(*NT, splitk=True, f16=True), mode="fp16"),
    _c("f16_fwd_pred_proj_nt_two_pass", "nt", 1024, 2048, 2048, gen(*NT, splitk=True, x3=2), mode="fp16x2"),
    _c("f16_fwd_pred_fc1_nt", "nt", 1024, 8192, 2048, g2(*NT, f16=True), mode="fp16"),
    # ---- their data gradients (nn) and weight gradients (tn), bf16
    _c("bwd_fc1_dgrad", "nn", 5120, 2048, 8192, pp2(*NN), epi=dict(act=DGELU_ERF, out="bf16")),
    _c("bwd_fc1_wgrad", "tn", 8192, 2048, 5120, pp2(*TN)),
    _c("bwd_fc2_dgrad", "nn", 5120, 8192, 2048, pp2(*NN), epi=dict(out="bf16")),
    _c("bwd_qkv_wgrad", "tn", 6144, 2048, 5120, pp2(*TN)),
    _c("bwd_proj_dgrad", "nn", 5120, 2048, 2048, pp2(*NN), epi=dict(accumulate=True)),
    _c("bwd_proj_wgrad", "tn", 2048, 2048, 5120, g2(*TN, splitk=True)),
    _c("bwd_pred_fc1_dgrad", "nt", 1024, 8192, 2048, g2(*NT), epi=dict(act=DGELU_TANH)),
    _c("bwd_pred_fc1_wgrad", "tn", 8192, 2048, 1024, pp2(*TN)),
    _c("bwd_pred_proj_wgrad", "tn", 2048, 2048, 1024, g2(*TN)),
    _c("bwd_small_wgrad_splitk4", "tn", 512, 512, 4096, g2(*TN, splitk=True), epi=dict(accumulate=True)),
    # ---- K edges
    _c("k_one_tile", "nt", 256, 256, 64, gen(*NT), epi=dict(bias=True)),
    _c("k_one_tile_tn", "tn", 256, 256, 64, gen(*TN)),
    _c("k_two_tiles_g2", "nt", 256, 256, 128, g2(*NT)),
    _c("k_two_tiles_pp", "nn", 256, 256, 128, pp(*NN), variant=3),
    _c("k_odd_general", "nn", 256, 256, 192, gen(*NN)),
    _c("k_odd_pp", "nt", 512, 512, 192, pp(*NT), variant=3),
    _c("k_odd5_pp_tn", "tn", 512, 512, 320, pp(*TN), variant=3),
    _c("k_shortest_pp2", "nt", 512, 512, 256, pp2(*NT), variant=3),
    _c("k_shortest_pp2_nn", "nn", 256, 256, 256, pp2(*NN), variant=3),
    _c("k_shortest_pp2_tn", "tn", 256, 512, 256, pp2(*TN), variant=3),
    _c("splitk2_odd_slices", "nn", 1024, 2048, 384, gen(*NN, splitk=True), splitk=2),
    _c("splitk2_even_slices", "nn", 1024, 2048, 512, g2(*NN, splitk=True), splitk=2),
    _c("splitk4_odd_slices_tn", "tn", 256, 256, 768, gen(*TN, splitk=True), splitk=4, epi=dict(accumulate=True)),
    _c("splitk4_even_slices_tn", "tn", 256, 256, 512, g2(*TN, splitk=True), splitk=4),
    _c("splitk4_pred_k2048", "nn", 1024, 2048, 2048, g2(*NN, splitk=True), splitk=4),
    _c("splitk2_ragged_nt", "nt", 200, 384, 2048, gen(*NT, splitk=True), epi=dict(bias=True, rowscale=True)),
    _c("splitk4_ragged_nn", "nn", 200, 256, 8192, gen(*NN, splitk=True)),
    _c("splitk4_ragged_tn", "tn", 200, 130, 6144, gen(*TN, splitk=True), epi=dict(accumulate=True)),
    _c("lo8_k256_pp2", "nt", 512, 512, 256, pp2(*NT, 3), mode="fp16_lo8", variant=3, sh=6),
    _c("lo8_k384_general", "nt", 512, 512, 384, pp(*NT, 3), mode="fp16_lo8", variant=3, sh=6, epi=dict(out="f16", out_lo8=True)),
    # ---- M and N edges, every layout (general 128x128 kernel; a few on the general 256x256 one)
    *[_c(f"edge_{lay}_{m}x{n}", lay, m, n, k, gen(lay == "tn", lay != "nt"))
      for lay, k in (("nt", 128), ("nn", 192), ("tn", 64))
      for m, n in ((1, 257), (15, 129), (16, 255), (17, 16), (129, 1), (255, 15), (257, 17))],
    _c("edge_pp_nt", "nt", 257, 255, 256, pp(*NT), variant=3, epi=dict(out="bf16")),
    _c("edge_pp_nn", "nn", 300, 520, 192, pp(*NN), variant=3, epi=dict(bias=True, act=GELU_TANH, out2="bf16")),
    _c("edge_pp_tn", "tn", 129, 257, 256, pp(*TN), variant=3),
    # ---- B-direct kernels (NT, N % 16 == 0)
    _c("bd160_min_n16", "nt", 160, 16, 128, bd(True, False), variant=8, epi=dict(bias=True)),
    _c("bd160_tails", "nt", 333, 272, 320, bd(True, False), variant=8, epi=dict(alpha=0.5, residual=True)),
    _c("bd256_tails", "nt", 300, 512, 192, bd(False, False), variant=7, epi=dict(out="bf16", pre="bf16", act=GELU_ERF)),
    _c("bd256_packed_forced", "nt", 512, 256, 256, bd(False, True), variant=9, epi=dict(bias=True)),
    _c("bd_refuses_n_not_16", "nt", 160, 200, 128, gen(*NT), variant=8),
    # ---- epilogue stages and store paths
    _c("epi_alpha_half", "nt", 256, 256, 128, g2(*NT), epi=dict(alpha=0.5, bias=True)),
    _c("epi_alpha_minus2_bf16", "nn", 130, 200, 192, gen(*NN), epi=dict(alpha=-2.0, out="bf16")),
    _c("epi_everything_aligned", "nt", 256, 256, 256, g2(*NT),
       epi=dict(alpha=0.5, bias=True, rowscale=True, residual=True, accumulate=True, pre="f32", out2="bf16")),
    _c("epi_everything_ld4", "nt", 130, 260, 128, gen(*NT),
       epi=dict(alpha=-2.0, bias=True, rowscale=True, residual=True, accumulate=True, pre="bf16", out2="f32", ldo=268)),
    _c("epi_everything_scalar", "tn", 130, 259, 192, gen(*TN),
       epi=dict(alpha=0.5, bias=True, rowscale=True, residual=True, pre="f32", out2="bf16", out="bf16", col0=1)),
    _c("epi_pp2_everything", "nn", 512, 512, 256, pp2(*NN), variant=3,
       epi=dict(alpha=-2.0, bias=True, rowscale=True, residual=True, accumulate=True, pre="bf16", out2="bf16")),
    _c("epi_pp2_scalar", "nt", 256, 256, 256, pp2(*NT), variant=3, epi=dict(bias=True, pre="bf16", out="bf16", col0=3)),
    _c("epi_splitk_everything", "nn", 256, 384, 2048, g2(*NN, splitk=True),
       epi=dict(alpha=0.5, bias=True, rowscale=True, residual=True, pre="bf16", out2="bf16", out="bf16")),
    _c("epi_gelu_erf", "nt", 130, 512, 192, gen(*NT), epi=dict(bias=True, act=GELU_ERF, pre="bf16")),
    _c("epi_gelu_tanh", "nt", 256, 256, 128, g2(*NT), epi=dict(bias=True, act=GELU_TANH, pre="f32", rowscale=True)),
    _c("epi_dgelu_erf", "nn", 256, 256, 256, pp2(*NN), variant=3, epi=dict(act=DGELU_ERF)),
    _c("epi_dgelu_tanh_scalar", "nt", 64, 130, 64, gen(*NT), epi=dict(act=DGELU_TANH, out2="bf16", col0=1)),
    _c("epi_relu", "nt", 300, 520, 192, pp(*NT), variant=3, epi=dict(bias=True, act=RELU, pre="bf16", residual=True)),
    _c("epi_sigmoid_gate", "nn", 200, 136, 128, gen(*NN), epi=dict(act=SIGMOID_GATE, bias=True)),
    _c("epi_out_lo_general", "nt", 130, 256, 128, gen(*NT, x3=2), mode="fp16x2", **_LO,
       epi=dict(bias=True, out="f16", out_lo=True, pre="bf16", out2="bf16")),
    _c("epi_out_lo_pp2", "nt", 512, 768, 256, pp2(*NT, 2), mode="fp16x2", variant=3, **_LO, epi=dict(bias=True, out="f16", out_lo=True)),
    _c("epi_out_lo_scalar", "nn", 130, 260, 320, gen(*NN, x3=2), mode="fp16x2", **_LO, epi=dict(out="f16", out_lo=True, ldo=268)),
    _c("epi_out_lo_bf16_g2", "nt", 256, 256, 128, g2(*NT), **_LO, epi=dict(out="f16", out_lo=True, residual=True)),
    _c("epi_out_lo8_pp2", "nt", 512, 512, 512, pp2(*NT, 3), mode="fp16_lo8", variant=3, sh=6, epi=dict(bias=True, out="f16", out_lo8=True)),
    # ---- the 32-bit running K offset: both k-strided operands with a pitch where the walk just fits, and one where it just does not
    _c("walk_fits_pp2", "tn", 256, 256, 2048, pp2(*TN), variant=3, ld=1044488),
    _c("walk_fails_pp", "tn", 256, 256, 2048, pp(*TN), variant=3, ld=1044496),
    _c("walk_fits_g2", "tn", 256, 256, 2048, g2(*TN, splitk=True), variant=1, ld=1044488),
    _c("walk_fails_general", "tn", 256, 256, 2048, gen(*TN, splitk=True), variant=1, ld=1044496),
    # ---- bf16x3 (split3 = 1): 128x128, general 256x256, steady-state 256x256, every layout
    _c("x3_nt_general", "nt", 300, 520, 256, gen(*NT, x3=1), mode="bf16x3", epi=dict(bias=True, act=GELU_ERF, pre="f32")),
    _c("x3_nn_general", "nn", 130, 256, 320, gen(*NN, x3=1), mode="bf16x3", epi=dict(bias=True, residual=True)),
    _c("x3_tn_general", "tn", 256, 130, 512, gen(*TN, x3=1), mode="bf16x3", epi=dict(accumulate=True)),
    _c("x3_nt_pp", "nt", 300, 520, 192, pp(*NT, 1), mode="bf16x3", variant=3),
    _c("x3_nn_pp", "nn", 512, 300, 320, pp(*NN, 1), mode="bf16x3", variant=3, epi=dict(residual=True)),
    _c("x3_tn_pp", "tn", 512, 264, 704, pp(*TN, 1), mode="bf16x3", variant=3, epi=dict(accumulate=True)),
    _c("x3_nt_pp2", "nt", 512, 768, 256, pp2(*NT, 1), mode="bf16x3", variant=3, epi=dict(bias=True)),
    _c("x3_nt_pp2_two_ktiles", "nt", 256, 256, 128, pp2(*NT, 1), mode="bf16x3", variant=3),
    _c("x3_nn_pp2", "nn", 512, 512, 384, pp2(*NN, 1), mode="bf16x3", variant=3),
    _c("x3_tn_pp2", "tn", 512, 256, 640, pp2(*TN, 1), mode="bf16x3", variant=3, epi=dict(accumulate=True)),
    # ---- fp16 two-pass (split3 = 2) and one pass (split3 = 4): forward layouts
    _c("f16x2_nn_general", "nn", 130, 256, 320, gen(*NN, x3=2), mode="fp16x2", epi=dict(bias=True, residual=True)),
    _c("f16x2_nn_splitk", "nn", 1024, 2048, 2048, gen(*NN, splitk=True, x3=2), mode="fp16x2"),
    _c("f16x2_nt_pp", "nt", 300, 520, 192, pp(*NT, 2), mode="fp16x2", variant=3, epi=dict(bias=True)),
    _c("f16x2_nn_pp", "nn", 512, 300, 320, pp(*NN, 2), mode="fp16x2", variant=3, epi=dict(residual=True)),
    _c("f16x2_nn_pp2", "nn", 256, 512, 384, pp2(*NN, 2), mode="fp16x2", variant=3),
    _c("f16_nt_pp2_shortest", "nt", 512, 768, 256, pp2(*NT, 2), mode="fp16", variant=3),
    _c("f16_nn_pp2", "nn", 256, 512, 384, pp2(*NN, 2), mode="fp16", variant=3, epi=dict(residual=True)),
    _c("f16_nt_pp_two_ktiles", "nt", 512, 512, 128, pp(*NT, 2), mode="fp16", variant=3),
    _c("f16_nn_general_tail", "nn", 130, 256, 320, gen(*NN, x3=2), mode="fp16", variant=1, epi=dict(bias=True)),
    # ---- the test-hook-only 4-stage 128x128 kernel
    _c("v4_nt", "nt", 200, 300, 320, gen(*NT, stages=4), variant=4, epi=dict(bias=True)),
    _c("v4_nn", "nn", 256, 256, 2048, gen(*NN, stages=4), variant=4),
    _c("v4_tn", "tn", 130, 257, 192, gen(*TN, stages=4), variant=4, epi=dict(accumulate=True)),
    # ---- the exact-fp32 kernel: fp32 operands in every layout with K tails, bf16 problems the fast path refuses
    _c("f32_nt_k1", "nt", 70, 50, 1, F32_FLOAT, mode="f32", epi=dict(bias=True)),
    _c("f32_nn_k17", "nn", 96, 200, 17, F32_FLOAT, mode="f32", epi=dict(residual=True, alpha=0.5)),
    _c("f32_tn_k63", "tn", 66, 70, 63, F32_FLOAT, mode="f32", epi=dict(accumulate=True)),
    _c("f32_tt_k65", "tt", 33, 65, 65, F32_FLOAT, mode="f32", epi=dict(alpha=-2.0)),
    _c("f32_nt_k100", "nt", 150, 130, 100, F32_FLOAT, mode="f32", epi=dict(bias=True, act=GELU_ERF, pre="f32")),
    _c("f32_nn_k64", "nn", 129, 1, 64, F32_FLOAT, mode="f32", epi=dict(out="bf16")),
    _c("bf16_fallback_k24", "nt", 70, 50, 24, F32_BF16, epi=dict(bias=True)),
    _c("bf16_fallback_k100_tn", "tn", 65, 33, 100, F32_BF16, epi=dict(accumulate=True)),
    _c("bf16_fallback_tt", "tt", 33, 65, 128, F32_BF16),
    _c("bf16_fallback_a_off", "nn", 130, 200, 128, F32_BF16, epi=dict(a_off=1, out="bf16")),
    # ---- the fused momentum-SGD update as the epilogue (afft_gemm_t.sgd) of every kernel family a weight gradient can reach: the four
    #      flag words, alpha, ok, the 8-wide / 4-wide / scalar accesses, every image; a first step enters with a NaN momentum buffer
    _c("sgd_gen_tn", "tn", 256, 256, 64, gen(*TN), epi=_sgd(NESTEROV, "bf16 f16 f8 pk", ldo=288)),
    _c("sgd_gen_tn_n254_pk", "tn", 256, 254, 64, gen(*TN), epi=_sgd(PLAIN, "bf16 f16 f8 pk", ok=1, alpha=-2.0, ldo=256)),      # a row ends 8-wide, 4-wide, scalar
    _c("sgd_gen_tn_n250_col4_pk", "tn", 256, 250, 64, gen(*TN), epi=_sgd(NESTEROV, "bf16 pk", alpha=0.5, ldo=256, col0=4)),    # 4-wide pieces at n % 8 == 4
    _c("sgd_gen_tn_splitk4_pk", "tn", 256, 254, 768, gen(*TN, splitk=True), splitk=4, epi=_sgd(FIRST, "bf16 f8 pk", alpha=0.5, ldo=256)),
    _c("sgd_g2_tn", "tn", 256, 256, 128, g2(*TN), epi=_sgd(FIRST | PLAIN, "f16 f8", ok=1, alpha=0.5)),
    _c("sgd_g2_tn_splitk4", "tn", 256, 256, 512, g2(*TN, splitk=True), splitk=4, epi=_sgd(NESTEROV, "bf16 pk", alpha=-2.0, ldo=288)),
    _c("sgd_g2_tn_splitk4_ok0", "tn", 256, 256, 512, g2(*TN, splitk=True), splitk=4, epi=_sgd(NESTEROV, "bf16 f16 f8 pk", ok=0, ldo=288)),
    _c("sgd_pp_tn_tails_ld4", "tn", 129, 257, 256, pp(*TN), variant=3, epi=_sgd(PLAIN, "bf16 f16 f8", ldo=260)),
    _c("sgd_pp2_tn", "tn", 256, 512, 256, pp2(*TN), variant=3, epi=_sgd(FIRST, "bf16 f16 f8 pk", alpha=-2.0, ldo=544)),
    _c("sgd_x3_tn_general", "tn", 256, 130, 512, gen(*TN, x3=1), mode="bf16x3", epi=_sgd(NESTEROV, "bf16 f8 pk", ok=1, ldo=160)),
    _c("sgd_x3_tn_pp", "tn", 512, 264, 704, pp(*TN, 1), mode="bf16x3", variant=3, epi=_sgd(FIRST | PLAIN, "f16", alpha=0.5)),
    _c("sgd_x3_tn_pp2", "tn", 512, 256, 640, pp2(*TN, 1), mode="bf16x3", variant=3, epi=_sgd(PLAIN, "bf16 f8")),
    _c("sgd_v4_tn_scalar", "tn", 130, 257, 192, gen(*TN, stages=4), variant=4, epi=_sgd(NESTEROV, "bf16 f16 f8", ok=1, alpha=-2.0, col0=1)),
    _c("sgd_v4_tn_scalar_ok0", "tn", 130, 257, 192, gen(*TN, stages=4), variant=4, epi=_sgd(PLAIN, "bf16 f16 f8", ok=0, col0=1)),
    _c("sgd_f32_tn_k63", "tn", 66, 70, 63, F32_FLOAT, mode="f32", epi=_sgd(FIRST, "bf16 f16 f8", alpha=0.5)),
    _c("sgd_f32_tn_k63_ok0", "tn", 66, 70, 63, F32_FLOAT, mode="f32", epi=_sgd(NESTEROV, "bf16 f16 f8", ok=0)),
    _c("sgd_bf16_fallback_k100_tn", "tn", 65, 33, 100, F32_BF16, epi=_sgd(PLAIN, "bf16 f16 f8", ok=1, alpha=-2.0)),
    _c("sgd_g2_nt_f8_col4", "nt", 256, 256, 128, g2(*NT), epi=_sgd(NESTEROV, "f8", ldo=264, col0=4)),      # p / buf 16-byte aligned, the byte image 4
    _c("sgd_gen_nn", "nn", 256, 256, 192, gen(*NN), epi=_sgd(FIRST | PLAIN, "bf16 f16 f8 pk", ldo=256)),
]

assert len({c.name for c in CASES}) == len(CASES), "case names must be unique"


def _traced_symbol(r):
    """afft_gemm_trace_rec_t -> the kernel symbol (as nm -C prints it) that the launcher recorded"""
    b = lambda x: "true" if x else "false"    # noqa: E731
    a, bb, sk = b(r.a_kstrided), b(r.b_kstrided), b(r.splitk > 1)
    x3 = 2 if r.split3 == 4 else int(r.split3)      # one fp16 pass runs the two-pass instantiation over one segment
    if r.variant in (1, 4):
        return f"gemm_bf16_kernel<2, 2, {2 if r.variant == 1 else 4}, {a}, {bb}, {sk}, {x3}>"
    if r.variant == 12:
        return f"gemm_bf16_g2_kernel<{a}, {bb}, {sk}, {b(x3 == 2)}>"
    if r.variant in (3, 13):
        return f"gemm_bf16_{'pp' if r.variant == 3 else 'pp2'}_kernel<{a}, {bb}, {x3}>"
    if r.variant in (7, 8, 9, 10):
        rows160 = r.variant in (8, 10)
        return f"gemm_bf16_bd_kernel<{10 if rows160 else 16}, 3, {2 if rows160 else 1}, {b(r.variant >= 9)}>"
    return f"<trace variant {r.variant}>"


# ---- operand geometry
def padded_pitch(cols, col0=0, al=8):
    """row pitch of a NaN-padded operand view of `cols` columns starting at column col0 of its buffer: a little wider than the view,
    a multiple of `al` elements (8: 16-bit operands, 16: e4m3 byte planes)"""
    return col0 + cols + al + (-(col0 + cols)) % al


def plane_shape(rows, cols):
    """[rows, cols] of one plane of an ops.Split: both padded to 64"""
    return (rows + 63) // 64 * 64, (cols + 63) // 64 * 64


def pitches(c):
    """{lda, ldb, ld8}: element pitches of the stored operands of case c (A [K, M] if transposed else [M, K]; B [N, K] if transposed
    else [K, N]) and the byte pitch of the e4m3 planes (fp16_lo8)"""
    a_t, b_t = c.layout[0] == "t", c.layout[1] == "t"
    a_cols, b_cols = (c.M if a_t else c.K), (c.K if b_t else c.N)
    if c.mode == "bf16x3":
        lda, ldb = plane_shape(1, a_cols)[1], plane_shape(1, b_cols)[1]
    else:
        lda = (c.ld if a_t else 0) or padded_pitch(a_cols, c.epi.get("a_off", 0))
        ldb = (c.ld if not b_t else 0) or padded_pitch(b_cols)
        if c.mode == "fp16x2":
            lda = plane_shape(1, a_cols)[1]
        if c.variant == 9 or c.epi.get("packed"):      # the packed image / the weight beside it: unpadded (the B-direct path wants b_cs == K)
            ldb = c.K
    return dict(lda=lda, ldb=ldb, ld8=padded_pitch(c.K, 0, 16))


def gemm_fields(layout, M, N, K, lda, ldb, *, split3=0, f32=False, a_off=0, a_lo=0, b_lo=0, ld8=0, packed=False, ws_bytes=0):
    """afft_gemm_t fields (name -> value) that validation and dispatch read, for operands of the given geometry at synthetic 16-byte
    aligned addresses (nothing dereferences them on the way to the plan)"""
    a_t, b_t = layout[0] == "t", layout[1] == "t"
    f = dict(M=M, N=N, K=K, dtype=0 if f32 else 1, split3=split3, a_lo=a_lo, b_lo=b_lo,
             A=(1 << 32) + a_off * (4 if f32 else 2), B=2 << 32, out=3 << 32, ldo=padded_pitch(N), alpha=1.0)
    f["a_rs"], f["a_cs"] = (1, lda) if a_t else (lda, 1)
    f["b_rs"], f["b_cs"] = (1, ldb) if b_t else (ldb, 1)
    if split3 == 3:
        f.update(a8=4 << 32, b8=5 << 32, a8_ld=ld8, b8_ld=ld8)
    if packed:
        f["b_packed"] = 6 << 32
    if ws_bytes:
        f.update(workspace=7 << 32, workspace_bytes=ws_bytes)
    return f


def dispatch_fields(c):
    """gemm_fields of case c as the GPU test's operands make them: strides and pitches of its NaN-padded views and Split planes, plane
    offsets, the e4m3 planes' pitch, the packed flag, A one element off alignment (a_off), the workspace ops.gemm hands over"""
    from afft_amd import ops
    a_t, b_t = c.layout[0] == "t", c.layout[1] == "t"
    p = pitches(c)
    split3 = {"bf16": 0, "f32": 0, "bf16x3": 1, "fp16x2": 2, "fp16_lo8": 3, "fp16": 4}[c.mode]
    a_plane = plane_shape(*((c.K, c.M) if a_t else (c.M, c.K)))
    b_plane = plane_shape(*((c.N, c.K) if b_t else (c.K, c.N)))
    return gemm_fields(c.layout, c.M, c.N, c.K, p["lda"], p["ldb"], split3=split3, f32=c.mode == "f32", a_off=c.epi.get("a_off", 0),
                       a_lo=a_plane[0] * a_plane[1] if split3 in (1, 2) else 0, b_lo=b_plane[0] * b_plane[1] if split3 == 1 else 0,
                       ld8=p["ld8"], packed=bool(c.epi.get("packed")),
                       ws_bytes=ops._WS_BYTES if c.mode != "f32" and split3 != 1 else 0)
