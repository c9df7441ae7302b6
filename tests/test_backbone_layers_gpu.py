"""The bf16 Pose-ResNet backbone layer by layer on the MI355X: the case functions of tests/backbone_cases.py (every op alone
against float64 with the derived interval, every kernel form, the non-default cfg.RESNET.* configurations) on cuda:0.  Every
test launches on the current stream and synchronises once before it reads; nothing is retried."""
import numpy as np
import pytest
import torch

import backbone_cases as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWITCHES = ("FVP_BB_NO_BIG", "FVP_BB_DMA_BN", "FVP_BB_NO_FUSE_FINAL", "FVP_BB_NO_FUSE_STEM", "FVP_BB_NO_FUSE_BLOCK")


@pytest.fixture()
def no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _build(lib, **cfg):
    m, sd = B.build(lib, DEV, **cfg)
    m.autotune = False
    return m, sd


# ---- the shipped library ---------------------------------------------------------------------------------------------------
# 3 x 160 x 224: ragged 256-pixel tiles, two tile columns in the fused kernels, more workgroups than one round at layer1
@pytest.mark.parametrize("shape", [(2, 64, 96), (3, 160, 224)], ids=["2x64x96", "3x160x224"])
@pytest.mark.parametrize("name", ["r50", "r18", "r50_bias_f256_128_64_j17"])
def test_every_op_alone_vs_fp64(no_switches, name, shape):
    m, sd = _build(None, **B.CONFIGS[name])
    stats = B.per_op_pass(m, sd, *shape, DEV)
    assert len(stats) == len(m._convs)
    print(name, shape, B.summary(stats))


@pytest.mark.parametrize("filters", [(256, 64, 32), (16,), ()])
def test_narrow_deconv_heads_vs_fp64(no_switches, filters):
    """Deconv heads of 32 / 16 stored channels (masked channel groups, K below one k chunk in the heatmap layer) and no
    deconv at all: every op behind layer4 alone against fp64."""
    m, sd = _build(None, deconv_filters=filters)
    stats = B.per_op_pass(m, sd, 2, 64, 96, DEV, only=lambda o, op: not o.get("key", "layer").startswith("layer")
                          and not o.get("stem"))
    assert len(stats) == len(filters) + 2


def test_every_tile_configuration_of_every_tunable_op(no_switches):
    """Extends test_backbone_tile_configurations_are_bit_identical_per_op with the reference check: configurations 1, 2, 3
    per tunable op at 3 x 64 x 96 (partial pixel tiles, partial XCD groups), bit-equal and within the interval."""
    m, sd = _build(None, **B.CONFIGS["r50"])
    stats = B.per_op_pass(m, sd, 3, 64, 96, DEV, all_cfgs=True)
    assert len(stats) >= 40
    print("tile configurations", B.summary(stats))


# ---- the diagnostics build: kernel forms behind the switches ---------------------------------------------------------------
def test_every_op_alone_register_staged_kernel(no_switches, diag_lib):
    no_switches.setenv("FVP_BB_NO_BIG", "1")
    m, sd = _build(diag_lib, **B.CONFIGS["r50"])
    stats = B.per_op_pass(m, sd, 2, 64, 96, DEV)
    assert len(stats) == len(m._convs)
    print("FVP_BB_NO_BIG", B.summary(stats))


@pytest.mark.parametrize("N,H,W", [(1, 64, 64), (3, 128, 128), (2, 32, 256)])
def test_fused_stem_and_bottlenecks_equal_the_separate_launches(no_switches, diag_lib, N, H, W):
    m, _ = _build(diag_lib, seed=5, **B.CONFIGS["r50"])
    B.stage1_forms(m, N, H, W, DEV, no_switches.setenv)


@pytest.mark.parametrize("shape", [(3, 32, 32), (2, 160, 224)], ids=["3x32x32", "2x160x224"])
@pytest.mark.parametrize("J", [1, 15, 17, 20, 32, 33])
def test_heatmap_layer_fused_and_separate(no_switches, diag_lib, J, shape):
    m, sd = _build(diag_lib, joints=J)
    stats = B.heat_matrix(m, sd, *shape, DEV, no_switches.setenv, no_switches.delenv)
    print("J", J, shape, B.summary(stats))


@pytest.mark.parametrize("shape", [(3, 32, 32), (2, 160, 224)], ids=["3x32x32", "2x160x224"])
def test_heatmap_layer_behind_a_64_filter_deconv(no_switches, diag_lib, shape):
    m, sd = _build(diag_lib, **B.CONFIGS["r50_bias_f256_128_64_j17"])
    B.heat_matrix(m, sd, *shape, DEV, no_switches.setenv, no_switches.delenv)


# ---- whole network, non-default configurations -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["r18", "r50_bias_f256_128_64_j17"])
def test_whole_network_non_default_configurations(no_switches, name):
    cfg = B.CONFIGS[name]
    m, sd = B.build(None, DEV, seed=3, **cfg)
    x = torch.from_numpy(np.random.default_rng(0).random((2, 3, 96, 128), dtype=np.float32))
    B.whole_network(m, sd, x, cfg.get("layers", 50), len(cfg.get("deconv_filters", (1, 2, 3))))
