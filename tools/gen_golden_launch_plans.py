"""Record the host-side launch queries of a built library over the shape grid of tests/test_launch_plan.py (no GPU needed: the
queries are host code) into tests/golden/conv_launch_plans.json.  Run it on the tree whose answers are the baseline -- the parent of
a planner change -- never on the tree under test.

usage: python tools/gen_golden_launch_plans.py [--lib vae_play_amd/libvaeplay_hip.so] [--out tests/golden/conv_launch_plans.json]
       [--launches recorded.json]   merge per-shape launch records (kernel name, grid, workgroup, memset) taken on a GPU

Each answer is stored as a small code from which decode() restores it exactly (encode() asserts that): the row tile of a statistics
slab, the slab count of a weight-gradient workspace, the flag of the affine query.  The codes are listed in the nested order of the
query's axes (last axis fastest) and run-length encoded as a string of "code*count" tokens."""
import argparse
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = [1, 2, 4, 16, 32, 128]
SIDE = [4, 8, 16, 32, 64, 128]                       # Hs = Ws
CHAN = [1, 2, 3, 8, 16, 32, 40, 64, 128, 256, 512]   # both sides: the pairs of this list (1, 2, 3: what the padded layers start from)
STRIDE = [1, 2]
KS = [1, 3, 4, 5]
I = ctypes.c_int

# query -> (C entry point, axes in nested order: the order that gives each query the longest runs)
QUERIES = {
    "stats_bf16x3": ("vp_conv5_stats_workspace_bytes", ("family", "Cbig", "Csmall", "stride", "S", "B")),
    "stats_f16": ("vp_conv5_stats_f16_workspace_bytes", ("family", "S", "Cbig", "Csmall", "B", "stride")),
    "stats_f32": ("vp_conv5_stats_f32_workspace_bytes", ("family", "S", "Cbig", "Csmall", "B", "stride")),
    "affine": ("vp_conv5_affine_supported", ("family", "precision", "Cbig", "Csmall", "stride", "S", "B")),
    "wgrad_bf16x3": ("vp_conv_wgrad_bf16x3_workspace_bytes", ("B", "S", "Cbig", "ks", "Csmall", "stride")),
    "wgrad_f32": ("vp_conv_wgrad_workspace_bytes", ("B", "S", "Cbig", "ks", "Csmall", "stride")),
}
AXES = {"family": [0, 1], "precision": [0, 1], "B": BATCH, "S": SIDE, "Cbig": CHAN, "Csmall": CHAN, "stride": STRIDE, "ks": KS}


def big_side(S, ks, stride):
    """the big side that a k x k, padding (ks - 1) // 2 layer of this stride maps onto a small side of S (even for stride 2)"""
    return (S + 1 if ks == 4 else S) if stride == 1 else 2 * S


def points(query):
    axes = QUERIES[query][1]
    for v in itertools.product(*(AXES[a] for a in axes)):
        yield dict(zip(axes, v))


def call_args(query, p):
    """the C arguments of one grid point"""
    if query.startswith("stats"):
        return (p["family"], p["B"], p["S"], p["S"], p["Cbig"], p["Csmall"], p["stride"])
    if query == "affine":
        return (p["family"], p["precision"], p["B"], p["S"], p["S"], p["Cbig"], p["Csmall"], p["stride"])
    Hb = big_side(p["S"], p["ks"], p["stride"])
    return (p["B"], p["S"], p["S"], Hb, Hb, p["Cbig"], p["Csmall"], p["ks"], p["stride"])


def decode(query, p, code):
    """the query's answer (floats, or the affine flag) at grid point p from its stored code"""
    if query == "affine":
        return code
    if query.startswith("stats"):        # code: 0 = no statistics, else the row tile bm: 3 * N * ceil(M / bm) * phases floats
        if not code:
            return 0
        N, phases = (p["Csmall"], 1) if p["family"] == 0 else (p["Cbig"], p["stride"] ** 2)
        return 3 * N * -(-p["B"] * p["S"] * p["S"] // code) * phases
    return code * p["ks"] ** 2 * p["Cbig"] * p["Csmall"]          # code: slabs of [taps][Csmall][Cbig] floats


def encode(query, p, value):
    codes = [c for c in ((256, 128, 64, 0) if query.startswith("stats") else (value // (p["ks"] ** 2 * p["Cbig"] * p["Csmall"]),)
                         if query != "affine" else (value,)) if decode(query, p, c) == value]
    assert codes, f"{query} {p}: {value} has no code"
    return codes[0]


def rle(values):
    out = []
    for v in values:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return " ".join(f"{v}*{n}" if n > 1 else str(v) for v, n in out)


def unrle(text):
    return [int(t.split("*")[0]) for t in text.split() for _ in range(int(t.split("*")[1]) if "*" in t else 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "vae_play_amd", "libvaeplay_hip.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "conv_launch_plans.json"))
    ap.add_argument("--launches", default=None)
    a = ap.parse_args()
    lib = ctypes.CDLL(a.lib)
    doc = {"axes": AXES, "queries": {}}
    for q, (entry, axes) in QUERIES.items():
        f = getattr(lib, entry)
        f.restype = I if q == "affine" else ctypes.c_size_t
        nargs = len(call_args(q, next(points(q))))
        f.argtypes = [I] * nargs
        vals = []
        for p in points(q):
            v = f(*call_args(q, p))
            assert q == "affine" or v % 4 == 0
            vals.append(encode(q, p, v if q == "affine" else v // 4))
        doc["queries"][q] = {"entry": entry, "axes": list(axes), "rle": rle(vals)}
        print(q, len(vals), "values,", len(doc["queries"][q]["rle"]), "characters", file=sys.stderr)
    if a.launches:
        with open(a.launches) as fh:
            doc["launches"] = json.load(fh)
    elif os.path.exists(a.out):
        with open(a.out) as fh:
            old = json.load(fh)
        if "launches" in old:
            doc["launches"] = old["launches"]
    with open(a.out, "w") as fh:
        fh.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in doc.items()) + "\n}\n")


if __name__ == "__main__":
    main()
