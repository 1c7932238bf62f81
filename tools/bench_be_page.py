"""Page compositing (test_BE_manga.py's main_annotation path below the backbone): one 1654 x 1170 page with 16 bubble crops through
``networks_BE.ComposeNet`` at feat 128 x 128 (logit planes 512 x 512), to the page's (H, W, 3) label map on the device, as
  host     ``FusedBEInference.segment``, the logits copied to the host, the serial restatement there (tests/be_page_ref.py: what the
           reference does, numpy in place of CPU torch), the page copied back,
  torch    ``segment``, then the same per-bubble procedure with torch ops on the device (full-page tensors per bubble,
           F.interpolate(mode="nearest"), a 13 x 13 max-pool for the dilation),
  fused    ``FusedBEInference.segment_page``,
  kernel   the compose launch alone on logits that lie on the device (``be_page.launch``; the table is uploaded outside the window),
in ONE process on one captured plan, the rows alternated over ``--rounds`` windows; a window is as many calls as fill ``--window``
seconds and ends in a device synchronise.  Reported per row: the median window's time per call and the spread (min, max).  The kernel
row also gets its achieved GB/s over the bytes it must move: the page once (H W 3) plus, for every bubble read from the logits, the
distinct texels of both planes its box samples (overlaps between bubbles are not subtracted).
usage: python tools/bench_be_page.py [--page 1654x1170] [--crops 16] [--feat 128x128] [--out profiles/r10_be_page.json]
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def calls_for(fn, seconds):
    for _ in range(2):
        fn()
    t = window(fn, 2)
    return max(2, int(seconds / max(t, 1e-6)))


def synthetic_page(H, W, b, seed=0):
    """b bubbles as load_manga_from_annotaion lays them out: the box is the annotated boundary plus 50 pixels clipped to the page, the
    crop square its larger side with the box centred in it; every fifth bubble has label 3"""
    rng = np.random.default_rng(seed)
    info, boxes, oboxes, labels = [], [], [], []
    for i in range(b):
        ow, oh = int(rng.integers(120, 420)), int(rng.integers(120, 420))
        ox, oy = int(rng.integers(0, W - ow)), int(rng.integers(0, H - oh))
        box = (max(ox - 50, 0), max(oy - 50, 0), min(ox + ow + 50, W), min(oy + oh + 50, H))
        w, h = box[2] - box[0], box[3] - box[1]
        size = max(w, h)
        info.append((0, (w - h) // 2, size) if w > h else ((h - w) // 2, 0, size))
        boxes.append(box)
        oboxes.append((ox, oy, ox + ow, oy + oh))
        labels.append(3 if i % 5 == 4 else 1 + i % 4 if 1 + i % 4 != 3 else 4)
    return torch.tensor(info), torch.tensor(boxes), torch.tensor(labels), torch.tensor(oboxes)


def torch_page(edges, masks, info, boxes, labels, oboxes, hw, thr):
    """paset_result_on_manga's procedure with device tensors (metadata as Python integers: no synchronisation)"""
    H, W = hw
    dev = edges.device
    result = torch.zeros((3, H, W), dtype=torch.uint8, device=dev)
    check = torch.zeros((H, W), dtype=torch.bool, device=dev)
    for i, ((ax, ay, size), (xmin, ymin, xmax, ymax), label, obox) in enumerate(zip(info, boxes, labels, oboxes)):
        w, h = xmax - xmin, ymax - ymin
        E = torch.zeros((H, W), dtype=torch.bool, device=dev)
        M = torch.zeros((H, W), dtype=torch.bool, device=dev)
        if label != 3:
            e = F.interpolate(edges[i][None], size=(size, size), mode="nearest")[0, 0]
            m = F.interpolate(masks[i][None], size=(size, size), mode="nearest")[0, 0]
            E[ymin:ymax, xmin:xmax] = ~(e[ay:ay + h, ax:ax + w] < thr)
            M[ymin:ymax, xmin:xmax] = ~(m[ay:ay + h, ax:ax + w] < thr)
        else:
            sq = torch.zeros((1, 1, size, size), device=dev)
            sq[..., ay + obox[1] - ymin:ay + obox[3] - ymin, ax + obox[0] - xmin:ax + obox[2] - xmin] = 1.0
            dil = F.max_pool2d(sq, 13, 1, 6)
            E[ymin:ymax, xmin:xmax] = dil[0, 0, ay:ay + h, ax:ax + w] > 0
            M[ymin:ymax, xmin:xmax] = sq[0, 0, ay:ay + h, ax:ax + w] > 0
        E &= ~M
        E &= ~check
        M &= ~check
        total = E | M
        check |= total
        result += torch.stack([E.to(torch.uint8) * 255, total.to(torch.uint8) * label, M.to(torch.uint8) * 255])
    result[:, ~check] = 255
    return result.permute(1, 2, 0).contiguous()


def must_move_bytes(info, boxes, labels, hw, S):
    from tests.be_page_ref import nearest_index
    total = hw[0] * hw[1] * 3
    for (ax, ay, size), (xmin, ymin, xmax, ymax), label in zip(info, boxes, labels):
        if label != 3:
            idx = nearest_index(size, S)
            total += 2 * 4 * len(np.unique(idx[ay:ay + ymax - ymin])) * len(np.unique(idx[ax:ax + xmax - xmin]))
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--page", default="1654x1170", help="H x W")
    ap.add_argument("--crops", type=int, default=16)
    ap.add_argument("--feat", default="128x128")
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_be_page.py measures on the GPU; none is visible")
    import vae_play_amd as V
    from ctypes import c_void_p
    from tests import be_page_ref as R
    from vae_play_amd import be_page, networks_BE
    H, W = (int(v) for v in a.page.split("x"))
    h, w = (int(v) for v in a.feat.split("x"))
    assert h == w, "square crops"
    S, b = 4 * h, a.crops
    torch.manual_seed(0)
    net = networks_BE.ComposeNet(networks_BE.FeatureNet(None, a.channels, 32)).to("cuda").eval()
    x = torch.randn((b, a.channels, h, w), generator=torch.Generator().manual_seed(1)).to("cuda").contiguous(memory_format=torch.channels_last)
    info, boxes, labels, oboxes = synthetic_page(H, W, b)
    inf = V.FusedBEInference(net, b, h, w)
    inf.capture()
    seg = inf.segment(x)
    # an untrained net's logits sit where they like: the page's threshold is their median, so that both bits occur
    thr = float(torch.cat([seg["edges"].flatten(), seg["masks"].flatten()]).median())
    meta = (info.tolist(), boxes.tolist(), labels.tolist(), oboxes.tolist())
    table = be_page.page_descriptors(info, boxes, labels, (H, W), (S, S), oboxes).to("cuda")
    page_k = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    e_dev, m_dev = seg["edges"], seg["masks"]

    def host():
        s = inf.segment(x)
        e, m = s["edges"].cpu().numpy(), s["masks"].cpu().numpy()
        return torch.from_numpy(R.compose(e, m, *meta[:3], (H, W), original_boxes=meta[3], threshold=thr)).to("cuda")

    def torch_dev():
        s = inf.segment(x)
        return torch_page(s["edges"], s["masks"], *meta, (H, W), thr)

    def fused():
        return inf.segment_page(x, info, boxes, labels, (H, W), original_boxes=oboxes, threshold=thr)

    def kernel():
        be_page.launch(c_void_p(e_dev.data_ptr()), S * S, c_void_p(m_dev.data_ptr()), S * S, table, b, None, page_k, (S, S), thr, True)
        return page_k

    fns = {"host": host, "torch": torch_dev, "fused": fused, "kernel": kernel}
    ref = host()
    same = {k: bool(torch.equal(fns[k](), ref)) for k in ("torch", "fused", "kernel")}
    n = {k: calls_for(f, a.window) for k, f in fns.items()}
    times = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():                # alternated: every round times each row once
            times[k].append(window(f, n[k]))
    seg_ms = statistics.median(window(lambda: inf.segment(x), max(5, n["fused"])) for _ in range(a.rounds)) * 1e3
    row = {"page": f"{H}x{W}", "crops": b, "logits": f"{S}x{S}", "threshold": thr, "claimed_fraction": round(float((ref != 255).any(dim=2).float().mean()), 4),
           "equal_to_host_row": same, "segment_alone_ms": round(seg_ms, 4)}
    for k in fns:
        ms = [t * 1e3 for t in times[k]]
        row[k] = {"ms_per_call": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "calls_per_window": n[k],
                  "windows": a.rounds}
    moved = must_move_bytes(*meta[:3], (H, W), S)
    row["kernel"]["bytes_it_must_move"] = moved
    row["kernel"]["achieved_GBps"] = round(moved / (row["kernel"]["ms_per_call"] * 1e-3) / 1e9, 2)
    row["host_over_fused"] = round(row["host"]["ms_per_call"] / row["fused"]["ms_per_call"], 3)
    row["torch_over_fused"] = round(row["torch"]["ms_per_call"] / row["fused"]["ms_per_call"], 3)
    out = {"metric": "ms per page (networks_BE.ComposeNet below the backbone, crops to the page label map on the device)", "unit": "ms",
           "device": torch.cuda.get_device_name(0), "rows": [row],
           "method": "one process, one captured plan, rows alternated per round, host clock around a window of calls that ends in a device "
                     "synchronise; median window, spread = min / max over the windows"}
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
