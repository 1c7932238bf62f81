"""SCSEBlock (models/blocks.py:52-65) at the drop-in boundary, without a GPU: the reference's import path, its state_dict keys,
shapes and seeded default init (fixture written by tools/gen_golden_scse.py from the reference class), the refusal to compute on
the CPU, and the host-side workspace query."""
import numpy as np
import pytest
import torch

from tests.util import load_golden

# NHWC activations of the three StyleUp stages at 256x256 images, batch 32 (models/network_Style_GAN.py:54-59): (B, HW, C, hidden)
STYLEGAN_SHAPES = ((32, 32 * 32, 256, 64), (32, 64 * 64, 128, 32), (32, 128 * 128, 64, 16))


def test_reference_import_path_resolves_to_the_hip_class():
    from models.blocks import SCSEBlock as alias
    from vae_play_amd.blocks import SCSEBlock as impl
    import models.blocks
    assert alias is impl
    assert "SCSEBlock" in models.blocks.__all__


def test_seeded_state_dict_equals_the_reference():
    from vae_play_amd.blocks import SCSEBlock
    g = load_golden("blocks_scse_c32_r4")
    ref = {k[len("state/"):]: v for k, v in g.items() if k.startswith("state/")}
    assert len(ref) == 6
    torch.manual_seed(0)
    sd = SCSEBlock(32, reduction=4).state_dict()
    assert list(sd.keys()) == ["cSE.1.weight", "cSE.1.bias", "cSE.3.weight", "cSE.3.bias", "sSE.0.weight", "sSE.0.bias"]
    assert set(sd.keys()) == set(ref.keys())
    shapes = {"cSE.1.weight": (8, 32, 1, 1), "cSE.1.bias": (8,), "cSE.3.weight": (32, 8, 1, 1), "cSE.3.bias": (32,),
              "sSE.0.weight": (1, 32, 1, 1), "sSE.0.bias": (1,)}
    for k, v in sd.items():
        assert tuple(v.shape) == shapes[k] == ref[k].shape, k
        assert np.array_equal(v.numpy(), ref[k]), f"{k}: seeded default init differs from the reference's"


def test_default_reduction_and_empty_hidden_layer():
    from vae_play_amd.blocks import SCSEBlock
    assert SCSEBlock(64).state_dict()["cSE.1.weight"].shape == (4, 64, 1, 1)      # reduction=16 like the reference
    with pytest.raises(ValueError):
        SCSEBlock(8, reduction=16)


def test_no_cpu_path():
    from vae_play_amd import functional as F_hip
    from vae_play_amd._lib import VaePlayHipError
    from vae_play_amd.blocks import SCSEBlock
    blk = SCSEBlock(32, reduction=4)
    x = torch.randn(2, 32, 5, 7)
    with pytest.raises(VaePlayHipError):
        blk(x)
    p = [blk.cSE[1].weight, blk.cSE[1].bias, blk.cSE[3].weight, blk.cSE[3].bias, blk.sSE[0].weight, blk.sSE[0].bias]
    with pytest.raises(VaePlayHipError):
        F_hip.scse(x, *p)
    with pytest.raises(VaePlayHipError):
        F_hip.scse(x, *p, relu=True)


def test_workspace_query_runs_on_the_host():
    from vae_play_amd import _lib, ops
    lib = _lib.load()
    for B, HW, C, hidden in STYLEGAN_SHAPES:
        n = lib.vp_scse_workspace_bytes(B, HW, C, hidden)
        assert n > 0 and n == ops.scse_workspace_bytes(B, HW, C, hidden)
        assert n < B * HW * C * 4 // 10, "the partials are a small fraction of the activation"
    # shapes the entry points refuse have no workspace
    assert lib.vp_scse_workspace_bytes(2, 35, 8, 0) == 0
    assert lib.vp_scse_workspace_bytes(0, 35, 8, 2) == 0
