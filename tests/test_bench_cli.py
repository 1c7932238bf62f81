"""bench.py's command line and its --dump-outputs writer, on the host: no GPU is touched (the snapshot is taken of a stand-in for
the fused plan that holds CPU tensors of the same names and shapes)."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests.util import ROOT

import bench  # noqa: E402


@pytest.mark.parametrize("argv", [["--tags-out", "t.json"], ["--steps", "0"]])
def test_refused_arguments(argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 2 and "error" in r.stderr, r.stderr[-2000:]


def _stand_in(S, z, B, C=3):
    import vae_play_amd as V
    torch.manual_seed(0)
    vae = V.VAE(S, z, C, init_rule=True)
    g = torch.Generator().manual_seed(7)
    return types.SimpleNamespace(vae=vae, x_tilde=torch.rand(B, S, S, C, generator=g).permute(0, 3, 1, 2),
                                 mu=torch.randn(B, z, generator=g), logvar=torch.randn(B, z, generator=g))


def test_dump_outputs_names_dtypes_and_budget(tmp_path):
    f = _stand_in(128, 128, 32)      # the default workload
    snap = bench.output_snapshot(f)
    out = snap(torch.tensor(1.5), torch.tensor([2.0]), torch.tensor(3.0))
    bench.write_outputs(out, str(tmp_path))
    names = {p[:-4] for p in os.listdir(tmp_path)}
    params = dict(f.vae.named_parameters())
    assert names == ({"loss", "recon", "kl", "x_tilde", "mu", "logvar"} | {"param." + k for k in params}
                     | {"buffer." + k for k, b in f.vae.named_buffers() if b.is_floating_point()})
    total = 0
    for n in names:
        a = np.load(tmp_path / (n + ".npy"))
        assert a.dtype == np.float32
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "recon.npy").shape == () and float(np.load(tmp_path / "recon.npy")) == 2.0
    np.testing.assert_array_equal(np.load(tmp_path / "x_tilde.npy"), f.x_tilde.numpy())      # whole, logical NCHW
    small = min(params, key=lambda k: params[k].numel())
    np.testing.assert_array_equal(np.load(tmp_path / f"param.{small}.npy"), params[small].detach().numpy())
    big = np.load(tmp_path / "param.encoder.fc.0.weight.npy")      # 33.5 M elements: a seeded sample of them
    assert big.shape == (bench.DUMP_CAP_PARAM,)
    again = snap(torch.tensor(1.5), torch.tensor([2.0]), torch.tensor(3.0))
    np.testing.assert_array_equal(again["param.encoder.fc.0.weight"], big)       # the same positions from run to run


def test_dump_outputs_stays_within_budget_at_a_large_workload(tmp_path):
    out = bench.output_snapshot(_stand_in(256, 128, 256))(torch.tensor(1.0), torch.tensor(1.0), torch.tensor(1.0))
    assert out["x_tilde"].shape == (bench.DUMP_CAP_OUTPUT,)
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
