"""Two builds of libvaeplay_hip.so, one process: every entry point of csrc/elementwise.hip, optim.hip, score.hip and project.hip over
the case list of tests/small_cases.py, on guarded buffers with exact-size workspaces, and every output, workspace query and updated
state compared bit for bit.
usage: python tools/ab_small_bits.py --ref-lib <the other build's libvaeplay_hip.so> [--lib <this build's>]
Exit status 0 when nothing differs."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from ab_norm_bits import differences  # noqa: E402
from tests import small_cases as S  # noqa: E402
from tests.norm_cases import Lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-lib", required=True)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    from vae_play_amd import _lib
    new, ref = Lib(os.path.abspath(a.lib or _lib.LIB_PATH)), Lib(os.path.abspath(a.ref_lib))
    outputs = failures = 0
    for fn, args, _ in S.CASES:
        got, want = fn(new, *args), fn(ref, *args)
        bad = differences(got, want)
        outputs += sum(t is not None for t in got.values())
        if bad:
            failures += 1
            print(f"DIFFERENT {fn.__name__}{args}: {bad}")
    print(f"ab_small_bits: {len(S.CASES)} cases, {outputs} outputs compared, {failures} cases differ")
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
