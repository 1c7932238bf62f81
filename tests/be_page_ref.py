"""A plain serial restatement of the reference's two paste functions (test_BE_manga.py:63-147 ``paset_result_on_manga`` and :160-225
``paset_edge_result_on_manga``): numpy on the CPU, one bubble after the other, every step spelled out.  It is the oracle of
tests/test_gpu_be_page.py; tests/test_be_page_cpu.py holds it to the arrays the reference itself produced (tests/golden/be_page_*.npz,
written by tools/gen_golden_be_page.py)."""
import numpy as np

RING = 6                     # (13 - 1) // 2, the reference's dilation kernel (:81-84)
NO_FRAME = 3                 # the label whose bubbles are not read from the net (:98)


def nearest_index(n_out, n_in):
    """source index of each of n_out samples of an n_in-long axis: torch's ``nearest`` in fp32"""
    scale = np.float32(n_in) / np.float32(n_out)
    j = np.arange(n_out, dtype=np.float32)
    return np.minimum(np.floor(j * scale).astype(np.int64), n_in - 1)


def resize_bits(plane, size, threshold):
    """a logit plane (SH, SW) -> its bits on the size x size crop square; a bit is set unless logit < threshold (a NaN is set)"""
    bits = ~(plane < np.float32(threshold))
    return bits[nearest_index(size, plane.shape[0])][:, nearest_index(size, plane.shape[1])]


def dilate(bits):
    """OR over the 13 x 13 window, zeros outside the array (a convolution with a kernel of ones, zero padding, clamped to 1)"""
    h, w = bits.shape
    padded = np.zeros((h + 2 * RING, w + 2 * RING), dtype=bool)
    padded[RING:RING + h, RING:RING + w] = bits
    out = np.zeros((h, w), dtype=bool)
    for dy in range(2 * RING + 1):
        for dx in range(2 * RING + 1):
            out |= padded[dy:dy + h, dx:dx + w]
    return out


def compose(edges, masks, recon_info, boxes, labels, page_hw, original_boxes=None, page_masks=None, variant="result", threshold=0.5,
            page=None):
    """(H, W, 3) uint8.  edges / masks: (b, 1, SH, SW) float32 arrays (masks unused for variant "edge"); page_masks (b, H, W), non-zero =
    set.  ``page``: a page to continue (only its white pixels are written), else a new one."""
    H, W = page_hw
    result = np.full((H, W, 3), 255, dtype=np.uint8) if page is None else page.copy()
    taken = (result != 255).any(axis=2)
    for i in range(len(labels)):
        ax, ay, size = (int(v) for v in recon_info[i])
        xmin, ymin, xmax, ymax = (int(v) for v in boxes[i])
        w, h = xmax - xmin, ymax - ymin
        label = int(labels[i])
        E = np.zeros((H, W), dtype=bool)
        M = np.zeros((H, W), dtype=bool)
        if label != NO_FRAME:
            E[ymin:ymax, xmin:xmax] = resize_bits(np.asarray(edges[i][0]), size, threshold)[ay:ay + h, ax:ax + w]
            if variant == "edge":
                M[ymin:ymax, xmin:xmax] = np.asarray(page_masks[i])[ymin:ymax, xmin:xmax] != 0
            else:
                M[ymin:ymax, xmin:xmax] = resize_bits(np.asarray(masks[i][0]), size, threshold)[ay:ay + h, ax:ax + w]
        elif original_boxes is None or variant == "edge":
            crop = np.asarray(page_masks[i])[ymin:ymax, xmin:xmax] != 0
            E[ymin:ymax, xmin:xmax] = dilate(crop)
            M[ymin:ymax, xmin:xmax] = crop
        else:
            oxmin, oymin, oxmax, oymax = (int(v) for v in original_boxes[i])
            square = np.zeros((size, size), dtype=bool)
            square[ay + oymin - ymin:ay + oymax - ymin, ax + oxmin - xmin:ax + oxmax - xmin] = True
            E[ymin:ymax, xmin:xmax] = dilate(square)[ay:ay + h, ax:ax + w]
            M[ymin:ymax, xmin:xmax] = square[ay:ay + h, ax:ax + w]
        E &= ~M
        E &= ~taken
        M &= ~taken
        taken |= E | M
        result[E] = (255, label, 0)
        result[M] = (0, label, 255)
    return result


# ---- the cases of tests/test_gpu_be_page.py (the fixtures' pages: golden_pages) ------------------------------------------------------
KINDS = {"annot": ("result", "original_boxes"), "mask": ("result", "page_masks"), "edge": ("edge", "page_masks")}
PAGES = [(33, 47, 8), (64, 65, 16), (96, 131, 20)]      # (H, W, S): W odd; the largest page is more than one workgroup's pixels


def golden_pages(kind):
    """the pages of tests/golden/be_page_<kind>.npz as dicts of arrays (inputs and "page", the reference's output)"""
    from tests.util import load_golden
    g = load_golden(f"be_page_{kind}")
    return [{k.split("/", 1)[1]: v for k, v in g.items() if k.startswith(f"p{i}/")} for i in range(int(g["n"]))]


def logits(rng, b, SH, SW, threshold=0.5):
    """a (b, 1, SH, SW) plane stack around the threshold: one value in twenty equals it exactly, one per stack is a NaN"""
    v = (threshold + 0.6 * rng.standard_normal((b, 1, SH, SW))).astype(np.float32)
    v[rng.random(v.shape) < 0.05] = np.float32(threshold)
    v[b // 2, 0, SH // 2, SW // 2] = np.nan
    return v


def blobs(rng, boxes, H, W):
    """page masks (b, H, W): random rectangles anywhere, one just above each box (within the 13 x 13 window's reach of its first rows:
    it must not dilate in), one inside along the box's right border, one astride its bottom border"""
    pm = np.zeros((len(boxes), H, W), dtype=np.uint8)
    for i, (xmin, ymin, xmax, ymax) in enumerate(boxes):
        for _ in range(3):
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            pm[i, y:y + int(rng.integers(1, 9)), x:x + int(rng.integers(1, 9))] = 1 + int(rng.integers(0, 255))      # (non-zero = set)
        pm[i, max(ymin - 4, 0):max(ymin - 1, 0), xmin + 2:xmin + 6] = 1
        pm[i, ymin + 3:ymin + 5, max(xmax - 2, xmin):xmax] = 1
        pm[i, ymax - 1:min(ymax + 3, H), xmin:xmin + 3] = 1
    return pm


def standard_case(kind, H, W, S, seed=0):
    """Six hand-placed bubbles on an H x W page (H >= 33, W >= 47) with S x S logits -- what each is there for:
      0  flush with the top and left borders, wider than high with the anchor in y, size == S, label 0
      1  flush with the bottom and right borders, higher than wide with the anchor in x (and one in y), size > S, label 255
      2  inside bubble 0, size < S
      3  label 3 over bubbles 0 and 2 (three bubbles share pixels, the order decides); its rectangle lies 3 pixels from the box's left
         side, which is also the crop square's (anchor_x = 0): the ring is clipped by the square there, and 2 pixels from the box's top,
         which is 2 rows inside the square (anchor_y = 2): the ring is clipped by the box there
      4  label 3 with an empty rectangle (it claims nothing)
      5  over bubble 4's box, flush with the right border
    For the page-mask kinds the same bubbles with ``blobs``."""
    rng = np.random.default_rng(seed + 100 * S + H)
    rows = [((0, 1, S), (0, 0, S, S - 2), 0, (0, 0, 0, 0)),
            ((4, 1, 24), (W - 15, H - 22, W, H), 255, (0, 0, 0, 0)),
            ((0, 0, S - 3), (3, 2, S, S - 2), 1, (0, 0, 0, 0)),
            ((0, 2, 30), (2, 1, 30, 28), 3, (5, 3, 17, 13)),
            ((0, 2, 18), (W - 20, 0, W - 2, 14), 3, (W - 15, 5, W - 15, 9)),
            ((0, 3, 22), (W - 22, 1, W, 16), 2, (0, 0, 0, 0))]
    return _case(rng, kind, H, W, S, S, rows)


def random_case(kind, H, W, S, b, seed=0, max_side=12):
    """b small random bubbles (every third with label 3), a third of them flush with a page border"""
    rng = np.random.default_rng(seed + b)
    rows = []
    for i in range(b):
        w, h = int(rng.integers(2, min(W, max_side) + 1)), int(rng.integers(2, min(H, max_side) + 1))
        xmin = int(rng.choice([0, W - w, rng.integers(0, W - w + 1), rng.integers(0, W - w + 1)]))
        ymin = int(rng.choice([0, H - h, rng.integers(0, H - h + 1), rng.integers(0, H - h + 1)]))
        size = max(w, h) + int(rng.choice([0, 1, 4]))
        ax, ay = int(rng.integers(0, size - w + 1)), int(rng.integers(0, size - h + 1))
        ox0, oy0 = xmin + int(rng.integers(0, w)), ymin + int(rng.integers(0, h))
        obox = (ox0, oy0, int(rng.integers(ox0, xmin + w + 1)), int(rng.integers(oy0, ymin + h + 1)))
        rows.append(((ax, ay, size), (xmin, ymin, xmin + w, ymin + h), 3 if i % 3 == 0 else int(rng.choice([0, 1, 2, 4, 255])), obox))
    return _case(rng, kind, H, W, S, S, rows)


def column_case(kind, H, seed=0):
    """a page one pixel wide (every flat group of four pixels spans four rows): three 1 x h bubbles, the second over the first"""
    rng = np.random.default_rng(seed + H)
    rows = [((2, 0, 9), (0, 0, 1, 9), 1, (0, 0, 0, 0)), ((0, 1, 8), (0, 5, 1, 12), 3 if kind == "annot" else 2, (0, 6, 1, 9)),
            ((0, 0, 5), (0, H - 5, 1, H), 255, (0, 0, 0, 0))]
    return _case(rng, kind, H, 1, 8, 8, rows)


def _case(rng, kind, H, W, SH, SW, rows):
    variant, source = KINDS[kind]
    b = len(rows)
    case = dict(variant=variant, page_hw=(H, W), recon_info=np.array([r[0] for r in rows], dtype=np.int64).reshape(b, 3),
                boxes=np.array([r[1] for r in rows], dtype=np.int64).reshape(b, 4), labels=np.array([r[2] for r in rows], dtype=np.int64),
                edges=logits(rng, b, SH, SW), masks=logits(rng, b, SH, SW), original_boxes=None, page_masks=None)
    if source == "original_boxes":
        case["original_boxes"] = np.array([r[3] for r in rows], dtype=np.int64).reshape(b, 4)
    else:
        case["page_masks"] = blobs(rng, case["boxes"], H, W)
    return case


def expected(case, threshold=0.5, page=None, rows=None):
    """the restatement on a case (``rows``: a slice of its bubbles)"""
    s = rows or slice(None)
    cut = lambda v: None if v is None else v[s]      # noqa: E731
    return compose(case["edges"][s], cut(case["masks"]), case["recon_info"][s], case["boxes"][s], case["labels"][s], case["page_hw"],
                   cut(case["original_boxes"]), cut(case["page_masks"]), case["variant"], threshold, page)
