"""The Style-GAN StyleEncoder's and Discriminator's drop-in boundary without a GPU (models/network_Style_GAN.py:12-43, :201-229 of
the reference): keys, their order, shapes and seeded init against the fixtures written by tools/gen_golden_stylegan_nets.py; the
fp64 restatement of tests/stylegan_nets_ref.py against the same fixtures (so that the GPU tests may use it as their reference),
outputs and every gradient within 1e-5 of the tensor's max; the rule by which the Discriminator selects its fused output stage;
the ``models.network_Style_GAN`` alias; and the new entry points in header, ctypes table and library."""
import numpy as np
import pytest
import torch

from tests import stylegan_nets_ref as R
from tests.util import rel_err, t

TOL = 1e-5


def _build(which):
    from vae_play_amd import network_Style_GAN as N
    torch.manual_seed(int(R.fixture(which)["seed"]))
    return N.StyleEncoder(8, 16, max_channels=32) if which == "encoder" else N.Discriminator(16, 3, max_channels=32)


ENCODER_KEYS = ([f"convs.0.conv.0.{n}" for n in ("weight", "bias")] + [f"convs.{i}.conv.0.weight" for i in (1, 2)]
                + [f"convs.{i}.conv.0.{n}" for i in (3, 4) for n in ("weight", "bias")]
                + [f"fc_{h}.fc.0.{n}" for h in ("mu", "logvar") for n in ("weight", "bias")])
DISC_KEYS = ([f"convs.0.conv.0.{n}" for n in ("weight", "bias")] + [f"convs.{i}.conv.0.weight" for i in (1, 2)]
             + [f"{h}_convs.{i}.conv.0.{n}" for h in ("adv", "aux") for i in (0, 1) for n in ("weight", "bias")])


@pytest.mark.parametrize("which,keys,floats", [("encoder", ENCODER_KEYS, 51536), ("disc", DISC_KEYS, 56964)])
def test_keys_order_shapes_and_seeded_init_equal_the_reference(which, keys, floats):
    g, sd = R.fixture(which), _build(which).state_dict()
    assert list(sd) == keys == [str(k) for k in g["keys"]]
    assert sum(v.numel() for v in sd.values()) == floats
    for k, v in sd.items():
        assert tuple(v.shape) == g[f"param/{k}"].shape, k
        assert np.array_equal(g[f"param/{k}"], v.numpy()), k
    assert list(sd) == [k for k, _ in _build(which).named_parameters()]          # no buffers: every key is a parameter


@pytest.mark.parametrize("which", ["encoder", "disc"])
def test_fp64_restatement_reproduces_the_fixture(which):
    g = R.fixture(which)
    _, _, _, _, n_out, n_din = R.FIXTURES[which]
    outs, dins, grads = R.reference(which)
    for name, got in list(zip(n_out, outs)) + list(zip(n_din, dins)):
        assert rel_err(got, t(g[name])) <= TOL, name
    assert sorted(grads) == sorted(str(k) for k in g["keys"])
    for k, got in grads.items():
        assert rel_err(got, t(g[f"grad/{k}"])) <= TOL, k


def test_discriminator_head_selection(monkeypatch):
    """fused: the switch on, a 4 x 4 trunk output, K and C in the kernel's range, fp32 (decided before anything touches a GPU)"""
    from vae_play_amd import network_Style_GAN as N
    assert N._HEAD_FUSED is True
    x16, x24 = torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 24, 24)
    assert N.Discriminator(16, 3, max_channels=32).uses_fused_head(x16, x16)
    assert not N.Discriminator(24, 3, max_channels=32).uses_fused_head(x24, x24)      # 24 -> 12 -> 6: the heads see 6 -> 3 -> 2
    assert not N.Discriminator(16, 3, max_channels=32).uses_fused_head(x16.double(), x16.double())
    assert not N.Discriminator(16, 3, max_channels=32).double().uses_fused_head(x16, x16)
    assert not N.Discriminator(16, 65, max_channels=32).uses_fused_head(x16, x16)     # K above the kernel's 64
    with torch.device("meta"):
        big = N.Discriminator(256, 2)                                                  # the training script's
        assert big.head_channels == 256 and big.uses_fused_head(torch.zeros(1, 3, 256, 256), torch.zeros(1, 3, 256, 256))
    monkeypatch.setattr(N, "_HEAD_FUSED", False)
    assert not N.Discriminator(16, 3, max_channels=32).uses_fused_head(x16, x16)


def test_alias_names_the_same_classes():
    import models.network_Style_GAN as A
    import vae_play_amd.network_Style_GAN as N
    assert A.StyleEncoder is N.StyleEncoder and A.Discriminator is N.Discriminator
    assert "StyleEncoder" in A.__all__ and "Discriminator" in A.__all__


def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    from tests.test_abi import header_functions
    from vae_play_amd import _lib
    lib = _lib.load()
    for n in ("vp_twin_head_fwd_f32", "vp_twin_head_bwd_f32"):
        assert n in header_functions() and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert len(_lib.SIGNATURES["vp_twin_head_fwd_f32"][1]) == 12 and len(_lib.SIGNATURES["vp_twin_head_bwd_f32"][1]) == 18


@pytest.mark.parametrize("which", ["encoder", "disc"])
def test_networks_refuse_to_run_without_a_gpu(which):
    """no fall-back: the CPU forward raises instead of computing with torch"""
    from vae_play_amd import _lib
    g, mod = R.fixture(which), _build(which)
    args = (t(g["x"]),) if which == "encoder" else (t(g["x"]), t(g["x_content"]), None)
    with pytest.raises(_lib.VaePlayHipError):
        mod(*args)
