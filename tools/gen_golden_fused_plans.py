"""Record the launch lists of the three fused plans (engine.FusedVAEStep, engine_gan.FusedVAEGANStep, infer.FusedVAEInference) into
tests/golden/fused_plans.json.gz (JSON with one launch per line, gzip-compressed: it is 400 KB of text otherwise).  No GPU is needed:
every case is built with ``_plan_only=True`` over host tensors and never run; the workspace / support queries it asks the library
are host code.  tests/test_fused_plan_lists.py rebuilds every case and requires the
same lists: a refactor of the plan-building code (plan.py, sections.py, the three ``_build`` methods) must not move, drop or re-aim a
launch.

usage: python tools/gen_golden_fused_plans.py [--root DIR] [--out tests/golden/fused_plans.json.gz] [--diff] [--show]
  --root  the tree whose ``vae_play_amd`` package (with a built library) is recorded; default: this tree.  Point it at a checkout of
          the PARENT commit: the fixture is the baseline a change is held against, so it is never generated from the tree under test.
  --diff  write nothing: print the unified diff, launch by launch, between the committed fixture and the recording of --root
  --show  write nothing, record nothing: print the committed fixture as text

Regenerating the fixture is legitimate only for a deliberate change of a plan (a launch added, removed, moved or given other
arguments) or of the library's planner answers (a workspace size, a fused-epilogue decision): regenerate from the tree that
carries that change alone and review ``--diff`` launch by launch.  A refactor never regenerates it.

What is recorded per case: its environment switches, the total bytes of ``step._bufs``, a few attributes the steps expose, the
buffers that tests and tools read by name, and every plan of the step as a list of
    [plan, entry point or pseudo-call, arguments, flops, tag, side slot, side_args]
with the stream slot left out.  Floats are written as ``float.hex()``.  A pointer is written as [kind, id, byte offset], resolved
against the address ranges the step may legitimately launch on:
    "buf"    step._bufs; id = ordinal of the buffer's first appearance in the dump (buffer NAMES may change, the wiring may not)
    "param"  the model's named parameters          "mbuf"  its named buffers (BatchNorm running statistics)
    "grad"   a parameter's slice of its optimiser's gradient arena
    "shadow" FusedVAEGANStep._dec_shadow            "sat"   FusedVAEStep._f16_sat
Anything else is ["?", 0, 0]: memory nobody the step knows owns -- a tensor that was freed when the builder returned.  The test
refuses those after a garbage collection.  ``PackJob`` arrays are expanded field by field through the same mapping."""
import argparse
import bisect
import contextlib
import ctypes
import difflib
import gzip
import json
import os
import re
import sys
from ctypes import c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fused_plans.json.gz")

# (C, S, z, B) of the FusedVAEStep cases: L = 1 (the pack wait behind the loop) | fp32 stem packed ``first``, padded-halo final input
# gradient | 16-bit stem with the first pack on the main stream, generic final conv | > 64 rows: three-launch dense BatchNorm |
# L = 4 with the enc_tail hook
VAE_SHAPES = [(1, 16, 8, 2), (2, 32, 16, 2), (8, 32, 16, 2), (3, 64, 32, 66), (3, 128, 128, 4)]
INFER_SHAPES = [(1, 16, 8, 2), (2, 32, 16, 2), (3, 64, 64, 4), (3, 128, 128, 32)]


def _case(kind, name, env=None, **kw):
    return dict(kind=kind, name=name, env=env or {}, **kw)


CASES = (
    [_case("vae", f"vae-{p}-c{C}-s{S}-z{z}-b{B}", precision=p, C=C, S=S, z=z, B=B)
     for p in ("f32", "bf16x3", "f16x2") for (C, S, z, B) in VAE_SHAPES]
    + [_case("vae", "vae-bf16x3-c3-s128-z128-b4-nofuse", {"VP_FUSE_BN_STATS": "0"}, precision="bf16x3", C=3, S=128, z=128, B=4)]
    + [_case("vaegan", f"vaegan-s{S}-z{z}-b{B}", S=S, z=z, B=B) for (S, z, B) in ((16, 8, 2), (32, 16, 4), (64, 32, 2))]
    + [_case("vaegan", "vaegan-s32-z16-b4-mainwgrad", {"VP_SIDE_WGRAD": "0"}, S=32, z=16, B=4),
       _case("vaegan", "vaegan-s32-z16-b4-nofuse", {"VP_FUSE_BN_STATS": "0"}, S=32, z=16, B=4)]
    + [_case("infer", f"infer-{p}-c{C}-s{S}-z{z}-b{B}", precision=p, C=C, S=S, z=z, B=B)
       for p in ("bf16x3", "f32") for (C, S, z, B) in INFER_SHAPES]
    + [_case("infer", "infer-vaegan-halves-s32-z16-b4", precision="bf16x3", C=1, S=32, z=16, B=4, halves=True)]
)
CASE_NAMES = [c["name"] for c in CASES]

# the plan-shaping switches: a case runs with exactly its own, whatever the caller's environment holds
SWITCHES = ("VP_FUSE_BN_STATS", "VP_SIDE_WGRAD", "VP_WGRAD_MAIN_CUS", "VP_WGRAD_SIDE_CUS")
# buffers that tests, tools and bench.py read from ``_bufs`` by name
KEPT_NAMES = re.compile(r"(enc\.hb|decp?\.db|disc\.hb|disc0\.y|(enc|disc)\d+\.as?|decp?\d+\.us?)$")

_MODELS = {}


def _model(kind, C, S, z):
    """one model (and its flat-arena optimisers) per shape, shared by the cases over it: construction dominates a case's time"""
    import torch
    import vae_play_amd as V
    from vae_play_amd import optim
    key = (kind, C, S, z)
    if key not in _MODELS:
        torch.manual_seed(0)
        if kind == "vaegan":
            net = V.VaeGan(S, z).train()
            opts = [optim.RMSprop(m.parameters(), lr=1e-4) for m in (net.encoder, net.decoder, net.discriminator, net.param_encoder)]
        else:
            net = V.VAE(S, z, C).train()
            opts = optim.Adam(net.parameters(), lr=1e-4)
        _MODELS[key] = (net, opts)
    return _MODELS[key]


@contextlib.contextmanager
def _switches(env):
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def build_case(case):
    """-> (step, [(plan name, _Plan)], [(prefix, module)], {kind: extra tensor}, attributes)"""
    import vae_play_amd as V
    from vae_play_amd.engine import FusedVAEStep
    from vae_play_amd.engine_gan import FusedVAEGANStep
    c = case
    with _switches(c["env"]):
        if c["kind"] == "vae":
            vae, opt = _model("vae", c["C"], c["S"], c["z"])
            st = FusedVAEStep(vae, opt, c["B"], c["S"], c["C"], precision=c["precision"], _plan_only=True)
            attrs = {"n_side_events": st._n_side_events, "bwd_b_enc_tail": st._bwd_b_enc_tail, "enc_tail_first": st._enc_tail_first}
            return st, [("fwd", st._fwd), ("bwd", st._bwd)], [("", vae)], {"sat": st._f16_sat}, attrs
        if c["kind"] == "vaegan":
            net, opts = _model("vaegan", 1, c["S"], c["z"])
            st = FusedVAEGANStep(net, opts, c["B"], c["S"], _plan_only=True)
            attrs = {"n_side_events": st._n_side_events, "c_disc": float(st.c_disc).hex(), "c_mse": float(st.c_mse).hex()}
            return st, [("fwd", st._fwd), ("fwd_disc", st._fwd_disc), ("bwd", st._bwd)], [("", net)], {"shadow": st._dec_shadow}, attrs
        if c.get("halves"):
            net, _ = _model("vaegan", 1, c["S"], c["z"])
            st = V.FusedVAEInference.from_modules(net.encoder, net.decoder, c["B"], c["S"], 1, precision=c["precision"], _plan_only=True)
            mods = [("encoder.", net.encoder), ("decoder.", net.decoder)]
        else:
            vae, _ = _model("vae", c["C"], c["S"], c["z"])
            st = V.FusedVAEInference(vae, c["B"], c["S"], c["C"], precision=c["precision"], _plan_only=True)
            mods = [("", vae)]
        attrs = {"n_side_events": st._n_side_events, "fused_layers": list(st.fused_layers), "unfused_layers": list(st.unfused_layers)}
        # each plan once, under every name it runs by
        plans, seen = [("prep", st._prep)], {}
        for which, ps in st._plans.items():
            for p in ps:
                seen.setdefault(id(p), (p, []))[1].append(which)
        plans += [("+".join(names), p) for p, names in seen.values()]
        return st, plans, mods, {}, attrs


def _ranges(step, modules, extra):
    """sorted (lo, hi, kind, id) of everything a launch may point into"""
    reg = []

    def add(t, kind, name):
        reg.append((t.data_ptr(), t.data_ptr() + max(1, t.numel()) * t.element_size(), kind, name))
    for n, t in step._bufs.items():
        add(t, "buf", n)
    for prefix, m in modules:
        for n, p in m.named_parameters():
            add(p, "param", prefix + n)
            arena = getattr(p, "_vp_arena", None)
            if arena is not None:
                add(arena.grad_view(p), "grad", prefix + n)
        for n, t in m.named_buffers():
            add(t, "mbuf", prefix + n)
    for kind, t in extra.items():
        add(t, kind, "")
    reg.sort(key=lambda r: r[0])
    return reg


def canonical(step, plans, modules, extra):
    """-> (calls, number of unresolved pointers, {kept buffer name: [ordinal, bytes]})"""
    reg = _ranges(step, modules, extra)
    los = [r[0] for r in reg]
    order, unknown = {}, [0]

    def ptr(v):
        if not v:
            return None
        i = bisect.bisect_right(los, v) - 1
        if i >= 0 and v < reg[i][1]:
            lo, _, kind, name = reg[i]
            return [kind, order.setdefault(name, len(order)) if kind == "buf" else name, v - lo]
        unknown[0] += 1
        return ["?", 0, 0]

    def arg(x):
        if isinstance(x, c_void_p):
            return ptr(x.value)
        if isinstance(x, ctypes.Array):       # PackJob[]
            return [[ptr(j.w), ptr(j.p0), ptr(j.p1), j.Csmall, j.Cbig, j.Csmall_pad, j.split] for j in x]
        if isinstance(x, float):
            return float(x).hex()
        assert x is None or isinstance(x, (int, str, bool)), type(x)
        return x

    calls = []
    for pname, plan in plans:
        for name, fn, a, slot, flops, tag, side, sargs in plan.calls:
            args = [arg(x) for i, x in enumerate(a) if fn is None or i != slot]
            calls.append([pname, name, args, float(flops).hex(), tag, side,
                          {str(k): [arg(v) for v in vs] for k, vs in sorted(sargs.items())} if sargs else None])
    kept = {n: [order.get(n), t.numel() * t.element_size()] for n, t in step._bufs.items() if KEPT_NAMES.match(n)}
    return calls, unknown[0], kept


def record_case(case, collect=None):
    """the fixture's record of one case; ``collect`` (the test: gc.collect) runs between building and resolving"""
    step, plans, modules, extra, attrs = build_case(case)
    if collect is not None:
        collect()
    calls, unknown, kept = canonical(step, plans, modules, extra)
    return {"env": dict(case["env"]), "bufs_bytes": sum(t.numel() * t.element_size() for t in step._bufs.values()),
            "attrs": attrs, "kept": kept, "unresolved": unknown, "calls": calls}


def dumps(doc):
    """one launch per line: a reviewable diff"""
    out = []
    for name, rec in doc.items():
        head = {k: v for k, v in rec.items() if k != "calls"}
        lines = ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in rec["calls"])
        out.append(f"{json.dumps(name)}: {json.dumps(head, separators=(',', ':'))[:-1]},\"calls\":[\n{lines}\n]}}")
    return "{\n" + ",\n".join(out) + "\n}\n"


def read_golden(path=GOLDEN) -> str:
    with gzip.open(path, "rt") as f:
        return f.read()


def write_golden(text: str, path=GOLDEN):
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:     # (the same bytes every time)
        f.write(text.encode())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--diff", action="store_true")
    ap.add_argument("--show", action="store_true")
    a = ap.parse_args()
    if a.show:
        sys.stdout.write(read_golden())
        return
    sys.path.insert(0, os.path.abspath(a.root))
    import vae_play_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(vae_play_amd.__file__))) == os.path.abspath(a.root), vae_play_amd.__file__
    doc = {}
    for c in CASES:
        doc[c["name"]] = rec = record_case(c)
        assert rec["unresolved"] == 0, (c["name"], rec["unresolved"])
        print(c["name"], len(rec["calls"]), "calls,", rec["bufs_bytes"], "bytes of buffers", file=sys.stderr)
    text = dumps(doc)
    assert json.loads(text) == json.loads(json.dumps(doc))
    if a.diff:
        sys.stdout.writelines(difflib.unified_diff(read_golden().splitlines(True), text.splitlines(True), "committed", a.root, n=1))
        return
    write_golden(text, a.out)
    print(f"{len(doc)} cases, {len(text)} bytes -> {a.out}", file=sys.stderr)


if __name__ == "__main__":
    main()
