"""GPU: the whole Augmented CycleGAN step at grid sizes that are not powers of two, against the fp32 oracle.

The fast paths are chosen per layer by grid-size predicates (csrc/conv_api.hip: acg_conv2d_s16_supported, dgrad_unpad_ok,
acg_conv2d_bwd_data_sums_supported, acg_conv2d_fwd_stats_supported), and the host hand-off protocols
(ops.ConvStats, SkipGrad, NormSums, the S16 plan) fall back when the producer did not take the fused path.  At these sizes some
fast paths engage while their neighbours fall back, which no power-of-two size exercises.  Full widths (ngf 32, ndf 64, nef 32,
nlatent 16), 3 resblocks, batch 3 (the latent BatchNorms need at least 3 samples), both arithmetics at the oracle tolerances of
configs[1] (conv_cases.ORACLE_TOL; one measured exception, F32_GNORM_TOL).  In bf16x3 each case asserts the exact
ops.FUSED counts and the set of convolution kernels that ran (parenthesised launch details dropped), so a path that silently
stops engaging — or starts engaging where its predicate says it cannot — fails here.

What ran (FUSED / KERNELS below), against DESIGN.md's predicate table:

* S = 192 (3 channels, trunk 96x96): the S16 trunk runs (conv_fwd_s16, wgrad_s16, igemm_conv_x3_pre).  The un-padded trunk
  data gradient is off (trunk W % 128 != 0): dgrad_s16_plain and dgrad_s16_relu_src replace dgrad_s16_norm_sums /
  dgrad_s16_relu_bitmask, so the trunk norms take their backward sums from a pass of their own.  Row pipeline and four-phase
  tile are off (no conv_rows_x3, no igemm_conv_ph4); of the four full-resolution norms of a generator pass only the head's
  takes its sums from a data gradient (conv_thinrow_x3<SUMS=1>: dgrad_f32_norm_sums 4 = 1 x 4 passes).  Statistics
  epilogues and the stem's 8x16 tiles are on.
* S = 384 (3 channels, trunk 192x192): as 192 in the trunk; at full resolution the row pipeline runs (conv_rows_x3, the
  row-patch tile igemm_conv_bf16<...,RP=1>) while the four-phase tile stays off (stride-2 output width 192 % 128 != 0):
  3 of the 4 full-resolution norms take their sums from a data gradient (dgrad_f32_norm_sums 12), the one in front of the
  stride-2 layer does not.
* S = 324 (1 channel, the Livneh 321x321 fields rounded up to a multiple of 4; trunk 162x162): every S16 path, the un-padded
  data gradients, the row pipeline, the four-phase tile and the stem's 8x16 statistics tiles are off (162 % 32, 324 % 8 and
  324 * 324 % 128 are all non-zero): the trunk runs the generic kernels (igemm_conv_x3_ws) with the plain hand-offs
  (dgrad_skip_addend, dgrad_relu_link).  One statistics epilogue does engage, which the generator-grid table does not
  predict: acg_conv2d_fwd_stats_supported is decided per layer (Ho * Wo % 128), and D_B's third convolution (k4, stride 1,
  on the 81x81 map) has an 80x80 = 50 x 128 output — igemm_conv_x3_ws<STATS=1>, 3 = the three D_B forwards of a step.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conv_cases import _run_cfg, _oracle_step, _matches_oracle  # noqa: E402

WIDTHS = dict(ngf=32, nef=32, ndf=64, nlatent=16, n_blocks=3)
CASES = {192: 3, 384: 3, 324: 1}   # grid size -> image channels
NB = 3
# gnorm_G_A_B (G_A_B's CondInstanceNorm scales start near zero: its gradient norm is the smallest of the step by three orders of
# magnitude) is not pinned to 1e-3 by any fp32 arithmetic at these sizes.  Measured at S = 384 with the oracle alone on the
# host: fp32 0.0373096, the same step in fp64 0.0372886 (fp32 is 5.6e-4 off), and fp32 with every weight perturbed by 1e-6
# relative 0.0372481 (1.65e-3 from the unperturbed fp32 value).  The exact-fp32 HIP step lands at 0.0372484, 1.64e-3 from the
# fp32 oracle and 1.1e-3 from fp64.  In f32 that one gradient norm is held to the bf16x3 bar, 3e-3; every other quantity keeps
# conv_cases.ORACLE_TOL.
F32_GNORM_TOL = {"gnorm_G_A_B": 3e-3}

# bf16x3, one step: ops.FUSED and the convolution kernels that ran (observed on an MI355X; see the module docstring)
FUSED = {
    192: {"conv_fwd_tile_stats": 22, "norm_stats_from_conv_epilogue": 44, "conv_fwd_s16": 24,
          "packed_weights_multi": 33, "dgrad_f32_norm_sums": 4, "norm_bwd_sums_from_dgrad": 4,
          "norm_bwd_sign_bitmask": 12, "dgrad_s16_plain": 18, "wgrad_s16": 24, "dgrad_s16_lazy_skip": 12,
          "dgrad_s16_relu_src": 6},
    384: {"conv_fwd_tile_stats": 25, "norm_stats_from_conv_epilogue": 47, "conv_fwd_s16": 24,
          "packed_weights_multi": 33, "dgrad_f32_norm_sums": 12, "norm_bwd_sums_from_dgrad": 12,
          "norm_bwd_sign_bitmask": 12, "dgrad_s16_plain": 18, "wgrad_s16": 24, "dgrad_s16_lazy_skip": 12,
          "dgrad_s16_relu_src": 6},
    324: {"conv_fwd_tile_stats": 3, "norm_stats_from_conv_epilogue": 3, "packed_weights_multi": 32,
          "norm_bwd_sign_bitmask": 12, "dgrad_skip_addend": 12, "dgrad_relu_link": 6},
}
KERNELS = {
    192: {"conv_patchn_x3<REFLECT=0>", "conv_thinrow_x3<REFLECT=0,SUMS=1>", "conv_thinrow_x3<REFLECT=1>",
          "igemm_conv_bf16<128,128,KC=16,REFLECT=0,SPLIT=1>", "igemm_conv_bf16<128,32,KC=16,REFLECT=0,SPLIT=1>",
          "igemm_conv_bf16<128,32,KC=32,REFLECT=0,SPLIT=1>", "igemm_conv_bf16<128,64,KC=32,REFLECT=0,SPLIT=1>",
          "igemm_conv_f32<128,128,KC=32,REFLECT=0,THIN=1,X3=1>",
          "igemm_conv_f32<128,32,KC=32,REFLECT=0,THIN=1,X3=1>", "igemm_conv_f32<128,64,KC=32,REFLECT=0,THIN=1,X3=1>",
          "igemm_conv_x3_pre<REFLECT=0,STATS=0>", "igemm_conv_x3_pre<REFLECT=1,STATS=0>",
          "igemm_conv_x3_pre<REFLECT=1,STATS=1>", "igemm_conv_x3_ws<REFLECT=0,STATS=0,ROWP=0>",
          "igemm_conv_x3_ws<REFLECT=0,STATS=0,ROWP=1>", "igemm_conv_x3_ws<REFLECT=0,STATS=1,ROWP=0>",
          "wgrad_bf16<128,128,SPLIT=1,NT=1>", "wgrad_bf16<32,32,SPLIT=1,NT=1>", "wgrad_bf16<32,64,SPLIT=1,NT=1>",
          "wgrad_bf16<64,32,SPLIT=1,NT=1>", "wgrad_f32", "wgrad_thin_patch_x3<K=7,flip=0>",
          "wgrad_thin_patch_x3<K=7,flip=1>", "wgrad_x3_krow_s16", "wgrad_x3_krowg<NT=3,IS=2,BCI=64>",
          "wgrad_x3_krowg<NT=4,IS=2,BCI=64>"},
    384: {"conv_patchn_x3<REFLECT=0>", "conv_rows_x3<32,64>", "conv_thinrow_x3<REFLECT=0,SUMS=1>",
          "conv_thinrow_x3<REFLECT=1>", "igemm_conv_bf16<128,128,KC=16,REFLECT=0,SPLIT=1>",
          "igemm_conv_bf16<128,32,KC=16,REFLECT=0,SPLIT=1>", "igemm_conv_bf16<128,32,KC=32,REFLECT=0,SPLIT=1,RP=1>",
          "igemm_conv_bf16<128,32,KC=32,REFLECT=0,SPLIT=1>", "igemm_conv_bf16<128,64,KC=32,REFLECT=0,SPLIT=1>",
          "igemm_conv_f32<128,128,KC=32,REFLECT=0,THIN=1,X3=1>",
          "igemm_conv_f32<128,32,KC=32,REFLECT=0,THIN=1,X3=1>", "igemm_conv_f32<128,64,KC=32,REFLECT=0,THIN=1,X3=1>",
          "igemm_conv_x3_pre<REFLECT=0,STATS=0>", "igemm_conv_x3_pre<REFLECT=1,STATS=0>",
          "igemm_conv_x3_pre<REFLECT=1,STATS=1>", "igemm_conv_x3_ws<REFLECT=0,STATS=0,ROWP=0>",
          "igemm_conv_x3_ws<REFLECT=0,STATS=0,ROWP=1>", "igemm_conv_x3_ws<REFLECT=0,STATS=1,ROWP=0>",
          "wgrad_bf16<128,128,SPLIT=1,NT=1>", "wgrad_bf16<32,32,SPLIT=1,NT=1>", "wgrad_bf16<32,64,SPLIT=1,NT=1>",
          "wgrad_f32", "wgrad_thin_patch_x3<K=7,flip=0>", "wgrad_thin_patch_x3<K=7,flip=1>", "wgrad_x3_krow_s16",
          "wgrad_x3_krow_s<32,64>", "wgrad_x3_krow_s<64,32>", "wgrad_x3_krowg<NT=3,IS=2,BCI=64>",
          "wgrad_x3_krowg<NT=4,IS=1,BCI=128>", "wgrad_x3_krowg<NT=4,IS=2,BCI=64>"},
    324: {"conv_patchn_x3<REFLECT=0>", "conv_thinrow_x3<REFLECT=0>", "conv_thinrow_x3<REFLECT=1>",
          "igemm_conv_bf16<128,128,KC=16,REFLECT=0,SPLIT=1>", "igemm_conv_bf16<128,32,KC=32,REFLECT=0,SPLIT=1>",
          "igemm_conv_bf16<128,64,KC=32,REFLECT=0,SPLIT=1>", "igemm_conv_f32<128,128,KC=32,REFLECT=0,THIN=1,X3=1>",
          "igemm_conv_f32<128,32,KC=32,REFLECT=0,THIN=1,X3=1>", "igemm_conv_f32<128,64,KC=32,REFLECT=0,THIN=1,X3=1>",
          "igemm_conv_x3_ws<REFLECT=0,STATS=0,ROWP=0>", "igemm_conv_x3_ws<REFLECT=0,STATS=0,ROWP=1>",
          "igemm_conv_x3_ws<REFLECT=0,STATS=1,ROWP=1>", "igemm_conv_x3_ws<REFLECT=1,STATS=0,ROWP=1>",
          "wgrad_bf16<128,128,SPLIT=1,NT=1>", "wgrad_bf16<32,32,SPLIT=1,NT=1>", "wgrad_bf16<32,64,SPLIT=1,NT=1>",
          "wgrad_bf16<64,128,SPLIT=1,NT=3>", "wgrad_bf16<64,32,SPLIT=1,NT=1>", "wgrad_f32",
          "wgrad_thin_patch_x3<K=7,flip=0>", "wgrad_thin_patch_x3<K=7,flip=1>", "wgrad_x3_krowg<NT=4,IS=1,BCI=128>",
          "wgrad_x3_krowg<NT=4,IS=2,BCI=64>"},
}


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("S", sorted(CASES))
def test_offgrid_step_matches_oracle(S, prec):
    from hip_util import Spy
    from dtgan_amd import ops
    kw = dict(input_nc=CASES[S], output_nc=CASES[S], **WIDTHS)
    ops.FUSED.clear()
    with Spy() as spy:
        got, = _run_cfg(kw, S, NB, prec, seed=0, in_seed=110 + S)
    fused, kernels = dict(ops.FUSED), set(k.split(" (")[0] for k in spy.kernels())
    if prec == "bf16x3":
        print("fused case=s%d %r" % (S, fused))
        print("kernels case=s%d %r" % (S, sorted(kernels)))
    assert got[1]["fake_B"].shape == (NB, CASES[S], S, S)
    _matches_oracle(got, _oracle_step(kw, S, NB, 0, 110 + S), prec, "s%d" % S, gnorm_tol=F32_GNORM_TOL if prec == "f32" else None)
    if prec == "bf16x3":
        assert fused == FUSED[S], fused
        assert kernels == KERNELS[S], sorted(kernels)
