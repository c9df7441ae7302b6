"""Case table and runner of the NON-Winograd forms of the conv interpreter (conv_form() in csrc/fvp_conv.hip: Direct on
k_conv / k_conv_dma, KSplit, K7, Pair7, TPair and the unpaired transposed conv, Reg, k_pool2, and the refusals), one op per
case, shared by tests/test_conv_forms_emu.py (CPU emulation, child processes: tests/conv_form_child.py) and
tests/test_conv_forms_gpu.py (MI355X).  Not a test module.

Every row names the form and the kernel instantiation it must reach (``expect``, as the emulator's launch log names it,
demangled by instantiations()).  For every row that runs, run_row() checks
  (a) the fp64 bound of tests/common.py (conv_gamma: (cinp * taps + 3) * eps32, + 3 for split K) for every op of the row's stack
      against its own stored inputs; the max-pool bit for bit; a fused 1x1 head through the propagated chain bound;
  (b) a plane's bits do not depend on the plane count it is computed in (``alt``: a count on the other side of the form's
      pixel / tile thresholds where it has one);
  (c) person masks (plane_valid, valid_div 1 / 2 / 3 by row, alternating groups, so multi-plane tiles are split) leave the
      valid planes bit-identical and the masked planes unwritten;
  (d) guards intact, valid outputs finite, and on the emulator no fenced read;
  (e) emulator: the launch log holds the instantiation the row names.

Bit-equality between forms is asserted only where the source claims it (tests/test_conv_forms_emu.py):
  * k_conv_reg = k_conv_dma: "k_conv_reg and k_conv_dma produce the same bits, so the choice may depend on the amount of
    work" (csrc/fvp_conv.hip, above reg_takes()): every Reg row, both children;
  * the 1x1 head fused into a transposed conv = the separate launch: "ONE fma chain over the 32 channels in channel order -
    what the standalone 1x1 kernel's MFMA sequence (and a plain fp32 dot product) computes, so the fused form is
    bit-identical to the two-kernel form" (conv_epilogue_tpair, FUSE2): tp_head15 under the default switches against the
    child with only FVP_CONV_NO_HEAD_FUSE=1; and with the claim above, k_conv_reg's fused MFMA head (reg_64_2_2, MODE 2)
    against k_conv_reg's and k_conv_dma's separate launches;
  * the max-pool behind a conv: exact in every form (a maximum rounds nothing), compared bit for bit with the maximum of
    the stored conv output.

Measured worst error / bound per form: the docstrings of tests/test_conv_forms_emu.py (emulator) and
tests/test_conv_forms_gpu.py (MI355X)."""
import collections
import re

import torch

import common as CM

Row = collections.namedtuple("Row", "name form expect kind cin cout hw planes alt opts sets gpu_planes gpu_alt")

EINVAL, ELIMIT = 10001, 10002


def _r(name, form, expect, kind, cin, cout, hw, planes=2, alt=1, sets=("default",), gpu_planes=None, gpu_alt=None, **opts):
    return Row(name, form, expect, kind, cin, cout, hw, planes, alt, opts, sets, gpu_planes, gpu_alt)


def dma(kh, kw, cb, pb, pair=0, tpair=0, ks=0):
    return f"k_conv_dma<{kh},{kw},{cb},{pb},{pair},{tpair},{ks}>"


def stg(kh, kw, cb, pb):
    return f"k_conv<{kh},{kw},{cb},{pb}>"


SW = ("default", "switch")      # rows that also run under every switch set (small)
REG = ("reg",)                  # rows of the FVP_CONV_REG_MIN_TILES=1 child (the emulated k_conv_reg)
BOTH = ("default", "reg")       # the same row through k_conv_dma (default) and k_conv_reg: the bit-equality claim

ROWS = [
    # ---- Direct, LDS-DMA staging (k_conv_dma; rows of whole quads) ------------------------------------------------------
    _r("dma3_12x12", "Direct", dma(3, 3, 1, 1), "conv", 6, 32, (12, 12), k=3, res=True, bn=True, sets=SW),
    _r("dma3_5x20", "Direct", dma(3, 3, 1, 1), "conv", 3, 16, (5, 20), planes=3, k=3),
    _r("dma3_3x36", "Direct", dma(3, 3, 1, 1), "conv", 4, 32, (3, 36), k=3, res=True, res_after=True),
    _r("dma3_1x8", "Direct", dma(3, 3, 1, 1), "conv", 2, 8, (1, 8), planes=5, k=3, relu=False),
    _r("dma1_c1", "Direct", dma(1, 1, 1, 1), "conv", 4, 1, (8, 8), planes=3, relu=False),
    _r("dma1_c2", "Direct", dma(1, 1, 1, 1), "conv", 4, 2, (8, 8), planes=3, bn=True),
    _r("dma1_c15", "Direct", dma(1, 1, 1, 1), "conv", 4, 15, (8, 8), planes=3, res=True),
    _r("dma1_c17", "Direct", dma(1, 1, 1, 1), "conv", 4, 17, (8, 8), planes=3, res=True, bn=True, sets=SW),
    _r("dma1_c32", "Direct", dma(1, 1, 1, 1), "conv", 4, 32, (8, 8), planes=3),
    _r("dma1_c128", "Direct", dma(1, 1, 1, 1), "conv", 4, 128, (8, 8), planes=3, bn=True),
    _r("dma3_15_16", "Direct", dma(3, 3, 1, 1), "conv", 15, 16, (12, 12), k=3, bn=True),
    _r("dma3_17_1", "Direct", dma(3, 3, 1, 1), "conv", 17, 1, (12, 12), k=3, relu=False),
    _r("dma3_32_2", "Direct", dma(3, 3, 1, 1), "conv", 32, 2, (12, 12), k=3),
    _r("dma3_66_64", "Direct", dma(3, 3, 1, 1), "conv", 66, 64, (12, 12), k=3, res=True, bn=True),
    _r("dma3_128_128", "Direct", dma(3, 3, 1, 1), "conv", 128, 128, (12, 12), k=3, res=True, sets=SW),
    _r("dma1_pb2", "Direct", dma(1, 1, 1, 2), "conv", 4, 32, (64, 64), planes=32, alt=2),
    _r("dma1_pb4", "Direct", dma(1, 1, 1, 4), "conv", 4, 32, (64, 64), planes=64, alt=3, res=True),
    _r("dma1_cb2pb2", "Direct", dma(1, 1, 2, 2), "conv", 4, 64, (64, 64), planes=32, alt=2, bn=True),
    _r("dma1_cb4", "Direct", dma(1, 1, 4, 1), "conv", 4, 128, (64, 64), planes=16, alt=2, bn=True),
    _r("dma3_pb4", "Direct", dma(3, 3, 1, 4), "conv", 2, 16, (64, 64), planes=64, alt=2, k=3),
    _r("dma3_cb2pb2", "Direct", dma(3, 3, 2, 2), "conv", 2, 48, (64, 64), planes=32, alt=2, k=3),
    _r("dma3_cb4", "Direct", dma(3, 3, 4, 1), "conv", 2, 100, (64, 64), planes=16, alt=2, k=3),
    _r("dma3_pb2", "Direct", dma(3, 3, 1, 2), "conv", 2, 16, (64, 64), planes=32, alt=2, k=3),
    _r("dma3_tn_4x12", "Direct", dma(3, 3, 1, 1), "conv", 4, 16, (4, 12), planes=7, alt=2, k=3, bn=True, sets=SW),
    _r("dma3_bands_36x36", "Direct", dma(3, 3, 1, 1), "conv", 4, 16, (36, 36), k=3, res=True),
    _r("dma3_rows_4x100", "Direct", dma(3, 3, 1, 1), "conv", 4, 16, (4, 100), k=3),
    _r("dma7_big_cout", "Direct", dma(7, 7, 1, 1), "conv", 2, 20, (12, 12), k=7, sets=SW),
    # 1-D instances (H = 1)
    _r("dma13_L20", "Direct", dma(1, 3, 1, 1), "conv", 6, 32, (1, 20), planes=5, dim=1, k=3, res=True, bn=True, sets=SW),
    _r("dma17_L24", "Direct", dma(1, 7, 1, 1), "conv", 15, 16, (1, 24), planes=5, dim=1, k=7, bn=True, sets=SW),
    _r("stg13_L10", "Direct", stg(1, 3, 1, 1), "conv", 6, 64, (1, 10), planes=5, dim=1, k=3, res=True, sets=SW),
    _r("stg17_L5", "Direct", stg(1, 7, 1, 1), "conv", 17, 16, (1, 5), planes=5, dim=1, k=7, sets=SW),
    _r("up1d_L12", "Direct", dma(1, 1, 1, 1), "up", 64, 32, (1, 12), planes=5, dim=1, bn=True, sets=SW),
    _r("up1d_L5", "Direct", stg(1, 1, 1, 1), "up", 128, 64, (1, 5), planes=3, dim=1),
    # the (2,2) and (4,1) tiles of the 1-D and 7x7 instances: pixel counts alone select them, so long rows with one or two
    # channels; their (1,2) and (1,4) tiles are reached at small shapes under FVP_CONV_PB = 2 / 4 (the switch sets)
    _r("dma13_cb2pb2", "Direct", dma(1, 3, 2, 2), "conv", 2, 64, (1, 256), planes=512, alt=2, dim=1, k=3, bn=True),
    _r("dma13_cb4", "Direct", dma(1, 3, 4, 1), "conv", 2, 128, (1, 128), planes=512, alt=2, dim=1, k=3, bn=True),
    _r("dma17_cb2pb2", "Direct", dma(1, 7, 2, 2), "conv", 2, 64, (1, 256), planes=512, alt=2, dim=1, k=7, bn=True),
    _r("dma17_cb4", "Direct", dma(1, 7, 4, 1), "conv", 2, 128, (1, 128), planes=512, alt=2, dim=1, k=7, bn=True),
    _r("dma7_cb2pb2", "Direct", dma(7, 7, 2, 2), "conv", 1, 48, (64, 64), planes=32, alt=2, k=7),
    # ---- Direct, register staging (k_conv: W % 4 != 0, or pieces of a row) ----------------------------------------------
    _r("stg3_10x10", "Direct", stg(3, 3, 1, 1), "conv", 6, 32, (10, 10), k=3, res=True, bn=True, sets=SW),
    _r("stg3_7x9", "Direct", stg(3, 3, 1, 1), "conv", 3, 16, (7, 9), planes=3, k=3),
    _r("stg3_9x9", "Direct", stg(3, 3, 1, 1), "conv", 17, 33, (9, 9), k=3, res=True, res_after=True),
    _r("stg3_2x260", "Direct", stg(3, 3, 1, 1), "conv", 4, 16, (2, 260), k=3, bn=True),
    _r("stg1_7x9", "Direct", stg(1, 1, 1, 1), "conv", 5, 17, (7, 9), planes=3, res=True, sets=SW),
    _r("stg7_10x10", "Direct", stg(7, 7, 1, 1), "conv", 3, 16, (10, 10), k=7, bn=True, sets=SW),
    _r("stg1_pb2", "Direct", stg(1, 1, 1, 2), "conv", 4, 32, (62, 66), planes=33, alt=2),
    _r("stg1_pb4", "Direct", stg(1, 1, 1, 4), "conv", 4, 32, (62, 66), planes=65, alt=3, res=True),
    _r("stg1_cb2pb2", "Direct", stg(1, 1, 2, 2), "conv", 4, 64, (62, 66), planes=33, alt=2, bn=True),
    _r("stg1_cb4", "Direct", stg(1, 1, 4, 1), "conv", 4, 128, (62, 66), planes=17, alt=2, bn=True),
    _r("stg3_pb4", "Direct", stg(3, 3, 1, 4), "conv", 2, 16, (62, 66), planes=65, alt=2, k=3),
    _r("stg3_cb4", "Direct", stg(3, 3, 4, 1), "conv", 2, 100, (62, 66), planes=17, alt=2, k=3),
    _r("stg3_pb2", "Direct", stg(3, 3, 1, 2), "conv", 2, 16, (62, 66), planes=33, alt=2, k=3),
    _r("stg3_cb2pb2", "Direct", stg(3, 3, 2, 2), "conv", 2, 48, (62, 66), planes=33, alt=2, k=3),
    _r("stg13_cb2pb2", "Direct", stg(1, 3, 2, 2), "conv", 2, 64, (1, 254), planes=517, alt=2, dim=1, k=3, bn=True),
    _r("stg13_cb4", "Direct", stg(1, 3, 4, 1), "conv", 2, 128, (1, 126), planes=521, alt=2, dim=1, k=3, bn=True),
    _r("stg17_cb2pb2", "Direct", stg(1, 7, 2, 2), "conv", 2, 64, (1, 254), planes=517, alt=2, dim=1, k=7, bn=True),
    _r("stg17_cb4", "Direct", stg(1, 7, 4, 1), "conv", 2, 128, (1, 126), planes=521, alt=2, dim=1, k=7, bn=True),
    _r("stg7_cb2pb2", "Direct", stg(7, 7, 2, 2), "conv", 1, 48, (62, 66), planes=33, alt=2, k=7),
    _r("stg7_cb4", "Direct", stg(7, 7, 4, 1), "conv", 1, 100, (62, 66), planes=17, alt=2, k=7),
    # ---- KSplit (3x3, >= 64 channels in whole groups of 8, rows of whole quads <= 32, 256 .. 576 pixels) ------------------
    _r("ks_64x4", "KSplit", dma(3, 3, 1, 1, ks=1), "conv", 64, 64, (64, 4), k=3, res=True, bn=True, sets=SW),
    _r("ks_144x4", "KSplit", dma(3, 3, 1, 1, ks=1), "conv", 72, 17, (144, 4), k=3, bn=True),
    _r("ks_21x24", "KSplit", dma(3, 3, 1, 1, ks=1), "conv", 128, 128, (21, 24), planes=1, alt=2, k=3, res=True),
    _r("ks_23x12", "KSplit", dma(3, 3, 1, 1, ks=1), "conv", 64, 1, (23, 12), planes=3, k=3, relu=False),
    _r("ks_20x28", "KSplit", dma(3, 3, 1, 1, ks=1), "conv", 72, 64, (20, 28), k=3, res=True, res_after=True),
    _r("ks_not_66ch", "Direct", dma(3, 3, 1, 1), "conv", 66, 32, (16, 20), k=3),
    _r("ks_not_608px", "Direct", dma(3, 3, 1, 1), "conv", 64, 32, (19, 32), k=3),
    _r("ks_not_252px", "Direct", dma(3, 3, 1, 1), "conv", 64, 32, (63, 4), k=3),
    _r("ks_not_580px", "Direct", dma(3, 3, 1, 1), "conv", 64, 32, (145, 4), k=3),
    _r("ks_not_255px", "Direct", stg(3, 3, 1, 1), "conv", 64, 32, (15, 17), k=3),
    _r("ks_not_577px", "Direct", stg(3, 3, 1, 1), "conv", 64, 32, (1, 577), planes=1, alt=2, k=3),
    # ---- K7 (k_conv7: 7x7, cout <= 16, no residual, W 64 / 128, cin <= 20, H >= 4) ------------------------------------
    _r("k7_c1_h4", "K7", "k_conv7<64,4,4>", "conv", 1, 16, (4, 64), k=7),
    _r("k7_c3_h5_w128", "K7", "k_conv7<128,4,4>", "conv", 3, 8, (5, 128), k=7, bn=True),
    _r("k7_c15_h6", "K7", "k_conv7<64,4,4>", "conv", 15, 16, (6, 64), planes=3, k=7, bn=True, sets=SW),
    _r("k7_c16_h7", "K7", "k_conv7<64,4,4>", "conv", 16, 8, (7, 64), k=7, relu=False),
    _r("k7_c17_h9", "K7", "k_conv7<64,5,4>", "conv", 17, 16, (9, 64), k=7, bn=True),
    _r("k7_c20_h4_w128", "K7", "k_conv7<128,5,4>", "conv", 20, 16, (4, 128), k=7),
    _r("k7_not_c21", "Pair7", dma(7, 7, 1, 1, pair=1), "conv", 21, 16, (4, 64), k=7),
    _r("k7_not_h3", "Pair7", dma(7, 7, 1, 1, pair=1), "conv", 15, 16, (3, 64), k=7),
    # ---- Pair7 (7x7, cout <= 16, rows of whole quads) ------------------------------------------------------------------
    _r("p7_80x80", "Pair7", dma(7, 7, 1, 1, pair=1), "conv", 15, 16, (80, 80), planes=1, alt=2, k=7, bn=True),
    _r("p7_20x20", "Pair7", dma(7, 7, 1, 1, pair=1), "conv", 17, 16, (20, 20), k=7, res=True, bn=True, sets=SW),
    _r("p7_12x12", "Pair7", dma(7, 7, 1, 1, pair=1), "conv", 2, 1, (12, 12), planes=3, k=7, relu=False),
    _r("p7_3x8", "Pair7", dma(7, 7, 1, 1, pair=1), "conv", 1, 16, (3, 8), planes=5, k=7, res=True, res_after=True),
    _r("p7_pb2", "Pair7", dma(7, 7, 1, 2, pair=1), "conv", 2, 16, (80, 80), planes=41, alt=2, k=7),
    _r("p7_pb4", "Pair7", dma(7, 7, 1, 4, pair=1), "conv", 1, 16, (80, 80), planes=82, alt=2, k=7),
    # ---- TPair and the unpaired transposed conv --------------------------------------------------------------------------
    _r("tp_128_64_8x8", "TPair", dma(1, 1, 4, 1, tpair=1), "up", 128, 64, (8, 8), bn=True, sets=SW),
    _r("tp_64_32_10x12", "TPair", dma(1, 1, 2, 2, tpair=1), "up", 64, 32, (10, 12), planes=3, bn=True),
    _r("tp_16_32_20x20", "TPair", dma(1, 1, 2, 2, tpair=1), "up", 16, 32, (20, 20)),
    _r("tp_30_20_8x8", "TPair", dma(1, 1, 2, 2, tpair=1), "up", 30, 20, (8, 8), planes=5, bn=True),
    _r("tp_head15", "TPair", dma(1, 1, 2, 2, tpair=1), "up", 64, 32, (8, 8), planes=3, head=15, head_fused=True, sets=SW + ("head",)),
    _r("tp_head17", "TPair", dma(1, 1, 2, 2, tpair=1), "up", 64, 32, (8, 8), planes=3, head=17, head_fused=False, sets=SW),
    _r("up_128_128", "Direct", dma(1, 1, 1, 1), "up", 128, 128, (8, 8), bn=True, sets=SW),
    _r("up_5x5", "Direct", stg(1, 1, 1, 1), "up", 64, 32, (5, 5), planes=3, bn=True),
    _r("up_3x7", "Direct", stg(1, 1, 1, 1), "up", 16, 64, (3, 7), planes=3),
    # ---- Reg (k_conv_reg<K, NB, MODE, HAS_RES>: the seven FVP_REG_INSTANCES; FVP_CONV_REG_MIN_TILES=1 on the emulator) -----
    _r("reg_16_1_0", "Reg", "k_conv_reg<16,1,0,0>", "conv", 16, 32, (8, 8), planes=5, sets=BOTH, bn=True, gpu_planes=520, gpu_alt=5),
    _r("reg_32_1_0", "Reg", "k_conv_reg<32,1,0,1>", "conv", 32, 32, (8, 8), planes=5, sets=BOTH, res=True, gpu_planes=520, gpu_alt=5),
    _r("reg_32_1_0_c15", "Reg", "k_conv_reg<32,1,0,0>", "conv", 32, 15, (8, 8), planes=5, sets=BOTH, relu=False, gpu_planes=520, gpu_alt=5),
    _r("reg_32_2_0", "Reg", "k_conv_reg<32,2,0,1>", "conv", 32, 64, (16, 16), planes=3, sets=BOTH, res=True, bn=True, gpu_planes=130, gpu_alt=3),
    _r("reg_64_4_0", "Reg", "k_conv_reg<64,4,0,0>", "conv", 64, 128, (8, 8), planes=5, sets=BOTH, bn=True, gpu_planes=520, gpu_alt=5),
    _r("reg_128_4_1", "Reg", "k_conv_reg<128,4,1,1>", "up", 128, 64, (8, 8), planes=5, sets=BOTH, bn=True, gpu_planes=101, gpu_alt=5),
    _r("reg_64_2_1", "Reg", "k_conv_reg<64,2,1,1>", "up", 64, 32, (8, 8), planes=5, sets=BOTH, bn=True, gpu_planes=101, gpu_alt=5),
    _r("reg_64_2_2", "Reg", "k_conv_reg<64,2,2,1>", "up", 64, 32, (8, 8), planes=5, sets=REG + ("head",), head=17, head_fused=True, gpu_planes=101, gpu_alt=120),
    _r("reg_16_1_0_res", "Reg", "k_conv_reg<16,1,0,1>", "conv", 16, 32, (8, 8), planes=5, sets=BOTH, res=True, gpu_planes=520, gpu_alt=5),
    _r("reg_64_4_0_res", "Reg", "k_conv_reg<64,4,0,1>", "conv", 64, 128, (8, 8), planes=5, sets=BOTH, res=True, res_after=True, gpu_planes=520, gpu_alt=5),
    _r("reg_not_res_c20", "Direct", dma(1, 1, 1, 1), "conv", 32, 20, (8, 8), planes=5, sets=REG, res=True),
    # ---- 3x3 layers the Winograd kernel takes by default: FVP_CONV_NO_WINO puts them on k_conv_dma ----------------------------
    _r("nowino_16x16", "Direct", dma(3, 3, 1, 1), "conv", 8, 32, (16, 16), planes=3, k=3, res=True, bn=True, sets=("no_wino",)),
    _r("nowino_pool_8x32", "Direct", dma(3, 3, 1, 1), "conv", 16, 64, (8, 32), k=3, bn=True, pool=True, sets=("no_wino",)),
    # ---- Pool -----------------------------------------------------------------------------------------------------------
    _r("pool_8x8", "Pool", "k_pool2", "pool", 5, 5, (8, 8), planes=3, sets=SW),
    _r("pool_20x20", "Pool", "k_pool2", "pool", 3, 3, (20, 20), planes=5),
    _r("pool_L20", "Pool", "k_pool2", "pool", 7, 7, (1, 20), planes=5, dim=1),
    _r("pool_L24", "Pool", "k_pool2", "pool", 33, 33, (1, 24), planes=3, dim=1),
    _r("pool_behind_dma3", "Direct", "k_pool2", "conv", 6, 32, (12, 12), planes=3, k=3, bn=True, pool=True),
    _r("pool_behind_stg1", "Direct", "k_pool2", "conv", 5, 17, (6, 10), planes=3, pool=True),
    # ---- k_conv_dma<7,7,4,1>: two pipeline stages of two channels' weights need ~110 KB, more than the default 64 KB chunk budget
    # (REFUSALS: conv7_coutp128_65536px); reached under FVP_CONV_LDS_KB=128 (emulator only: set 'lds128')
    _r("dma7_cb4_lds128", "Direct", dma(7, 7, 4, 1), "conv", 1, 100, (64, 64), planes=16, alt=2, k=7, sets=("lds128",)),
]

# ---- refusals: (name, kind, cin, cout, hw, opts, error code) - nothing may be written ------------------------------------
REFUSALS = [
    ("pool_7x8", "pool", 3, 3, (7, 8), dict(), EINVAL),
    ("pool_8x7", "pool", 3, 3, (8, 7), dict(), EINVAL),
    ("pool_L5", "pool", 3, 3, (1, 5), dict(dim=1), EINVAL),
    ("conv3_coutp96", "conv", 4, 96, (10, 10), dict(k=3), ELIMIT),
    ("conv1_coutp96", "conv", 4, 70, (8, 8), dict(k=1), ELIMIT),
    ("up_coutp96", "up", 8, 96, (4, 4), dict(), ELIMIT),
    # k_conv_dma<7,7,4,1>: the weights of two channels in two pipeline stages (2 x 2 x 49 x 128 floats = 98 KB) exceed the 64 KB
    # chunk budget, so from 65536 pixels on (where all four cout blocks go to one workgroup) a 7x7 conv to more than 64
    # couts on rows of whole quads is refused; with fewer pixels (one block per workgroup) and on k_conv it runs
    ("conv7_coutp128_65536px", "conv", 1, 100, (64, 64), dict(k=7, planes=16), ELIMIT),
]

# instantiations of ALL_INSTANTIATIONS that no shape reaches under any switch set, with the reason (none: k_conv_dma<7,7,4,1>,
# which plan_tiles() refuses under the default 64 KB chunk budget, runs under FVP_CONV_LDS_KB=128)
UNREACHABLE = {}

# every instantiation of the non-Winograd conv kernels the library can launch, written out: dispatch_tile() x
# dispatch_conv() on both stagings, the KSplit / Pair7 / TPair instances, the four k_conv7, the seven FVP_REG_INSTANCES
# (with and without a residual where both can occur: a transposed conv always has its skip) and k_pool2
ALL_INSTANTIATIONS = sorted(
    [f(kh, kw, cb, pb) for f in (dma, stg) for kh, kw in ((7, 7), (3, 3), (1, 1), (1, 7), (1, 3))
     for cb, pb in ((1, 1), (1, 2), (1, 4), (2, 2), (4, 1))] +
    [dma(3, 3, 1, 1, ks=1), dma(7, 7, 1, 1, pair=1), dma(7, 7, 1, 2, pair=1), dma(7, 7, 1, 4, pair=1),
     dma(1, 1, 2, 2, tpair=1), dma(1, 1, 4, 1, tpair=1),
     "k_conv7<64,4,4>", "k_conv7<128,4,4>", "k_conv7<64,5,4>", "k_conv7<128,5,4>",
     "k_conv_reg<16,1,0,0>", "k_conv_reg<16,1,0,1>", "k_conv_reg<32,1,0,0>", "k_conv_reg<32,1,0,1>", "k_conv_reg<32,2,0,0>",
     "k_conv_reg<32,2,0,1>", "k_conv_reg<64,4,0,0>", "k_conv_reg<64,4,0,1>", "k_conv_reg<128,4,1,1>", "k_conv_reg<64,2,1,1>",
     "k_conv_reg<64,2,2,1>", "k_pool2"])


# Switch sets of the diagnostics build (read once when the library loads: one process each): environment, and the sets
# whose rows run under it ((a) - (e); the default and the reg set are the table proper).  FVP_CONV_NO_DMA leaves the pixel-pair 7x7 form out: it has no register-staged instance, the
# interpreter refuses those layers under that switch.
SWITCH_SETS = {
    "default": ({}, ("default",)),
    "reg": ({"FVP_CONV_REG_MIN_TILES": "1"}, ("reg",)),
    "no_dma": ({"FVP_CONV_NO_DMA": "1"}, ("switch",)),
    "no_pair": ({"FVP_CONV_NO_PAIR": "1"}, ("switch",)),
    "no_k7": ({"FVP_CONV_NO_K7": "1"}, ("switch",)),
    "no_ksplit": ({"FVP_CONV_NO_KSPLIT": "1"}, ("switch",)),
    "no_reg": ({"FVP_CONV_NO_REG": "1", "FVP_CONV_REG_MIN_TILES": "1"}, ("switch", "reg")),
    "no_wino": ({"FVP_CONV_NO_WINO": "1"}, ("switch", "no_wino")),
    "no_fuse": ({"FVP_CONV_NO_HEAD_FUSE": "1", "FVP_CONV_NO_POOL_FUSE": "1", "FVP_CONV_REG_MIN_TILES": "1"}, ("switch", "reg")),
    "no_head_fuse": ({"FVP_CONV_NO_HEAD_FUSE": "1"}, ("head",)),      # only this switch: the bit-equality of the fused head
    "lds16": ({"FVP_CONV_LDS_KB": "16"}, ("switch",)),
    "lds128": ({"FVP_CONV_LDS_KB": "128"}, ("lds128",)),
    "pb1": ({"FVP_CONV_PB": "1"}, ("switch",)),
    "pb2": ({"FVP_CONV_PB": "2"}, ("switch",)),
    "pb4": ({"FVP_CONV_PB": "4"}, ("switch",)),
}
SWITCH_VARS = ("FVP_WINO_GENERIC", "FVP_CONV_REG_MIN_TILES", "FVP_CONV_NO_DMA", "FVP_CONV_NO_PAIR", "FVP_CONV_NO_K7",
               "FVP_CONV_NO_KSPLIT", "FVP_CONV_NO_REG", "FVP_CONV_NO_WINO", "FVP_CONV_NO_HEAD_FUSE", "FVP_CONV_NO_POOL_FUSE",
               "FVP_CONV_NO_SKIP_FUSE", "FVP_CONV_LDS_KB", "FVP_CONV_PB", "FVP_CONV_ABLATE", "FVP_CONV_REG_WGS", "FVP_K7_LDS_KB")


EMU_ONLY_SETS = ("lds128",)      # (k_conv_dma has no opt-in for more than 64 KB of LDS: a diagnostics budget for the emulator)


def head_unfused(env, row):
    """Whether the switches in ``env`` keep a row's 1x1 head out of the transposed conv's epilogue (fused_head())."""
    return (env.get("FVP_CONV_NO_HEAD_FUSE", "0") not in ("", "0") or env.get("FVP_CONV_NO_PAIR", "0") not in ("", "0")
            or (env.get("FVP_CONV_NO_REG", "0") not in ("", "0") and row.form == "Reg" and row.opts.get("head", 0) > 16))


def rows_of(set_name):
    """(index, row) of the rows that run under switch set ``set_name``."""
    sets = SWITCH_SETS[set_name][1]
    rows = [(i, r) for i, r in enumerate(ROWS) if any(s in r.sets for s in sets)]
    if set_name == "no_dma":
        rows = [(i, r) for i, r in rows if r.form != "Pair7"]
    if set_name == "lds16":     # two pipeline stages of one channel pair of a 7x7 conv, or of KSplit's eight channels, exceed 16 KB
        rows = [(i, r) for i, r in rows if r.opts.get("k", 1) != 7 and r.form != "KSplit"]
    return rows


def child_env(set_name, base):
    """The environment of the child process of a switch set: every conv switch removed, then the set's own."""
    e = {k: v for k, v in base.items() if k not in SWITCH_VARS}
    e.update(SWITCH_SETS[set_name][0])
    return e


# ---- launch log ------------------------------------------------------------------------------------------------------
_SYM = re.compile(r"^_ZN3fvp(\d+)(.*)$")
_ARG = re.compile(r"L[ib](\d+)E")


def instantiations(log):
    """Launches of the conv / pool kernels in an emulator launch log as 'name<template arguments>' (the packing kernels
    are left out)."""
    out = []
    for line in log.split():
        m = _SYM.match(line)
        if not m:
            continue
        n = int(m.group(1))
        name, rest = m.group(2)[:n], m.group(2)[n:]
        if not (name.startswith("k_conv") or name == "k_pool2"):
            continue
        if rest.startswith("I"):
            args, pos = [], 1
            while True:
                a = _ARG.match(rest, pos)
                if not a:
                    break
                args.append(a.group(1))
                pos = a.end()
            name += "<" + ",".join(args) + ">"
        out.append(name)
    return out


def load_lib(gpu=False):
    """The emulated library (or the diagnostics build of the HIP library) under the FVP_* switches of the environment."""
    import ctypes as C
    import os

    from faster_voxelpose_amd import _capi as capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if gpu:
        lib = capi.bind(C.CDLL(os.path.join(root, "tests", "diag", "libfvp_hip_diag.so")))
        assert lib.fvp_diag_build() == 1
        return lib
    lib = capi.bind(C.CDLL(os.path.join(root, "tests", "hipemu", "libfvp_emu.so")))
    lib.hipemu_launch_log.restype = C.c_char_p
    lib.hipemu_launch_log.argtypes = []
    lib.hipemu_launch_log_reset.argtypes = []
    return lib


def _mask(row_index, planes):
    """(plane_valid, valid_div, per-plane validity): alternating groups, the first group masked on odd rows; from the
    seventh group on only the last one is valid (the rows with hundreds of planes need them for the pixel count alone)."""
    vd = 1 + row_index % 3
    ng = -(-planes // vd)
    pv = torch.tensor([(g + row_index) % 2 if g < 6 else int(g == ng - 1) for g in range(ng)], dtype=torch.uint8)
    if ng == 1:
        pv[0] = 1
    return pv, vd, pv.bool()[torch.arange(planes) // vd]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_ops(row, spec, w, ids, blob, bufs, sel, split):
    """(a) on the planes ``sel``: worst error / bound over every op of the stack (the max-pool: exact)."""
    unstored = (ids["out"],) if row.opts.get("head_fused", False) else ()
    return CM.conv_stack_ratio(spec, w, blob, bufs, sel, split=split, unstored=unstored)


def run_row(lib, device, row, index, gpu=False, sample=None, head_fused=None, full=True):
    """Checks (a) - (d) of one row (assertions), returns dict(ratio, insts, out: the first two planes of the op's output (the
    head's for a head row), planes).  ``gpu``: plane counts gpu_planes / gpu_alt where the row has them (the shipped
    library's thresholds).  ``sample``: check (a) on at most that many planes (first, middle, last)."""
    if head_fused is not None and "head_fused" in row.opts:      # a switch that keeps the head from being fused
        row = row._replace(opts=dict(row.opts, head_fused=head_fused))
    planes = row.gpu_planes if (gpu and row.gpu_planes) else row.planes
    alt = row.gpu_alt if (gpu and row.gpu_alt) else row.alt
    opts = {k: v for k, v in row.opts.items() if k != "head_fused"}
    spec, w, ids = CM.conv_layer(row.kind, row.cin, row.cout, row.hw, seed=index, **opts)
    g = torch.Generator().manual_seed(1000 + index)
    nmax = max(planes, alt)
    x = torch.randn((nmax,) + spec.bufs[0], generator=g).to(device)
    emu = device == "cpu"
    unwritten = (ids["out"],) if row.opts.get("head_fused", False) else ()
    watch = ids["head"] if ids["head"] is not None else ids["out"]
    split = row.form == "KSplit"

    def run(n, pv=None, vd=1):
        info = {}
        if emu:
            lib.hipemu_launch_log_reset()
        bufs, check = CM.run_custom_conv_stack(lib, device, spec, w, x[:n], plane_valid=pv, valid_div=vd, poison=True, info=info)
        insts = instantiations(lib.hipemu_launch_log().decode()) if emu else []
        check(unwritten=unwritten)                                                            # (d)
        return bufs, info["blob"], insts

    bufs, blob, insts = run(planes)
    sel = list(range(planes)) if not sample or planes <= sample else sorted({0, planes // 2, planes - 1})
    ratio = _check_ops(row, spec, w, ids, blob, bufs, sel, split)                            # (a)
    assert ratio <= 1.0, f"{row.name}: error / bound {ratio:.3g}"
    if not full:
        return dict(ratio=ratio, insts=insts, alt_insts=[], out=bufs[watch][:2].cpu().clone(), planes=planes)
    full = [b.cpu() for b in bufs]
    # (b) the other plane count: the common planes keep their bits, in every buffer
    ab, _, alt_insts = run(alt)
    m = min(alt, planes)
    for i in range(1, len(bufs)):
        assert torch.equal(_bits(ab[i][:m].cpu()), _bits(full[i][:m])), f"{row.name}: buffer {i} differs between {planes} and {alt} planes"
    # (c) person masks
    pv, vd, valid = _mask(index, planes)
    mb, _, _ = run(planes, pv, vd)
    for i in range(1, len(bufs)):
        got = mb[i].cpu()
        assert torch.equal(_bits(got[valid]), _bits(full[i][valid])), f"{row.name}: buffer {i}: valid planes differ under the mask (valid_div {vd})"
        if i not in unwritten:
            assert bool((_bits(got[~valid]) == CM.POISON_BITS).all()), f"{row.name}: buffer {i}: masked planes were written"
    return dict(ratio=ratio, insts=insts, alt_insts=alt_insts, out=full[watch][:2].clone(), planes=planes)


def run_refusal(lib, device, case):
    """A stack the interpreter refuses: the error code, and nothing written (every buffer keeps its poison, guards intact)."""
    name, kind, cin, cout, hw, opts, code = case
    opts = dict(opts)
    planes = opts.pop("planes", 2)
    spec, w, ids = CM.conv_layer(kind, cin, cout, hw, seed=7, **opts)
    x = torch.randn((planes,) + spec.bufs[0], generator=torch.Generator().manual_seed(3)).to(device)
    info = {}
    bufs, check = CM.run_custom_conv_stack(lib, device, spec, w, x, poison=True, info=info, allow_rc=(code,))
    assert info["rc"] == code, f"{name}: returned {info['rc']}, expected {code}"
    first_refused = ids["op"]
    # ops before the refused one (the prelude of an 'up' row) ran; the refused op's output and everything after it did not
    untouched = tuple(spec.op_array[i].dst for i in range(first_refused, len(spec.ops)))
    check(unwritten=untouched)
    return info["rc"]
