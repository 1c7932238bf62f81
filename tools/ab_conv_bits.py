"""Two builds of libvaeplay_hip.so: every convolution entry point of csrc/conv*.hip over the case list of
tests/test_gpu_launch_plan_branches.py (BRANCHES + VARIANTS) and the weight re-pack entry points, on guarded buffers (NaN-prefilled,
64 sentinels each side, exact-size workspaces), and every output compared bit for bit: the convolution outputs, split planes, dW, mean,
rstd, the running statistics and the packed weights.  Each library runs the list once, in a fresh child process under its own time
limit (selected through VAEPLAY_HIP_LIB); this process never opens the GPU.  Split-K here is two addends onto zero, so every case is
expected to reproduce: run a build against itself first.
usage: python tools/ab_conv_bits.py --ref-lib <the other build's libvaeplay_hip.so> [--lib <this build's>]
Exit status 0 when nothing differs."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT = 600      # seconds per library


def pack_digests():
    """vp_pack_w5_batch (fp32, bf16-pair and fp16-pair jobs, the split ones padded), vp_pack_w_split at 3 x 3 and
    vp_pack_w5_p1_split_padded: 3 small and 72 big channels (two 64-wide tiles, the second one partial), padded to 8"""
    import torch
    from tests.guarded import Guards
    from vae_play_amd import _lib, ops
    Cs, Cb, pad = 3, 72, 8
    gen = torch.Generator(device="cuda").manual_seed(5)
    w5 = torch.randn(Cs, Cb, 5, 5, device="cuda", generator=gen)
    w3 = torch.randn(Cs, Cb, 3, 3, device="cuda", generator=gen)
    g, out = Guards("cuda"), {}
    out["batch f32 p0"], out["batch f32 p1"] = g.out("f0", Cs * 25 * Cb), g.out("f1", Cb * 25 * Cs)
    jobs = [_lib.PackJob(w5.data_ptr(), out["batch f32 p0"].data_ptr(), out["batch f32 p1"].data_ptr(), Cs, Cb, Cs, 0)]
    for split, tag in ((1, "bf16"), (2, "f16")):
        p0, p1 = g.planes(f"{tag}0", Cs * 25 * Cb), g.planes(f"{tag}1", Cb * 25 * pad)
        out[f"batch {tag} p0"], out[f"batch {tag} p1 padded"] = p0, p1
        jobs.append(_lib.PackJob(w5.data_ptr(), p0.data_ptr(), p1.data_ptr(), Cs, Cb, pad, split))
    _lib.call("vp_pack_w5_batch", (_lib.PackJob * len(jobs))(*jobs), len(jobs), ops._stream())
    out["k3 split p0"], out["k3 split p1"] = g.planes("k0", Cs * 9 * Cb), g.planes("k1", Cb * 9 * Cs)
    _lib.call("vp_pack_w_split", ops._p(w3), ops._pv(out["k3 split p0"]), ops._pv(out["k3 split p1"]), Cs, Cb, 3, ops._stream())
    out["p1 split padded"] = g.planes("pp", Cb * 25 * pad)
    _lib.call("vp_pack_w5_p1_split_padded", ops._p(w5), ops._pv(out["p1 split padded"]), Cs, Cb, pad, ops._stream())
    g.check()
    return {f"pack.{k}": hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest() for k, t in out.items()}


def emit():
    from tests import test_gpu_launch_plan_branches as T
    d = T.digests({**T.BRANCHES, **T.VARIANTS})
    d.update(pack_digests())
    print("DIGESTS " + json.dumps(d))


def run(lib):
    env = dict(os.environ, VAEPLAY_HIP_LIB=os.path.abspath(lib))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--emit"], env=env, cwd=ROOT, timeout=LIMIT, capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGESTS ")]
    if r.returncode or not lines:
        sys.exit(f"ab_conv_bits: the run of {lib} ended with status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(lines[-1][len("DIGESTS "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-lib")
    ap.add_argument("--lib", default=os.path.join(ROOT, "vae_play_amd", "libvaeplay_hip.so"))
    ap.add_argument("--emit", action="store_true", help="(child) run the case list on VAEPLAY_HIP_LIB and print the digests")
    a = ap.parse_args()
    if a.emit:
        return emit()
    if not a.ref_lib:
        ap.error("--ref-lib is required")
    got, want = run(a.lib), run(a.ref_lib)      # a fault ends this process before anything else is started
    assert got.keys() == want.keys()
    bad = sorted(k for k in got if got[k] != want[k])
    for k in bad:
        print(f"DIFFERENT {k}")
    print(f"ab_conv_bits: {len(got)} outputs of {len({k.split('.')[0] for k in got})} cases compared, {len(bad)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
