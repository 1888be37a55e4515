"""Single-field edits of a chain image (include/pgbart_image.h) that no writer produces and every loader must refuse:
the table shared by tests/test_chain_image.py (the oracle) and tests/test_steady_state_gpu.py (the HIP library refuses
what the oracle refuses, with the same words, before any kernel sees the record)."""
import ctypes as C

import numpy as np

from pymc_bart_amd.image import ChainImage, ImageHeader

EDIT_CASES = ["ragged_1025", "linear_response", "categorical_k3_mix", "nan_onehot_prior"]
ORPHAN = 255


def _writable(blob):
    """(header offsets aside) the sections of a private copy of the image as writable views."""
    raw = bytearray(blob)
    return raw, ChainImage.parse(raw)


def _header_double(raw, field, index, value):
    off = getattr(ImageHeader, field).offset + 8 * index
    raw[off: off + 8] = np.float64(value).tobytes()


def _header_int64(raw, offset, value):
    raw[offset: offset + 8] = np.int64(value).tobytes()


def image_edits(blob):
    """[(name, edited image, the text pgb_image_check must answer with)] for one good image.  An edit whose
    precondition the image does not meet (no orphan rows, a single leaf ...) raises: the test cases are chosen so
    that every edit applies to at least one of them, and `skipped` names the ones that did not apply here."""
    img0 = ChainImage.parse(blob)
    n, K, p = int(img0.header.s.n), int(img0.header.s.n_outputs), int(img0.header.s.p)
    noff = np.array(img0.node_off)
    sizes = np.diff(noff)
    big = int(np.argmax(sizes))                       # the bushiest tree
    base = int(noff[big])
    var = np.array(img0.var[base: base + sizes[big]])
    left = np.array(img0.left[base: base + sizes[big]])
    right = np.array(img0.right[base: base + sizes[big]])
    inner = np.flatnonzero(var >= 0)
    leaves = np.flatnonzero(var < 0)
    assert inner.size >= 2 and leaves.size >= 3, "the image's bushiest tree is too small for the edit table"
    leaf, leaf2 = base + int(leaves[0]), base + int(leaves[1])
    node = base + int(inner[0])                       # the root of that tree
    deep = int(inner[-1])                             # an inner node whose children are both leaves' ancestors-free
    out, skipped = [], []

    def edit(name, text, fn):
        raw, img = _writable(blob)
        try:
            fn(raw, img)
        except LookupError as e:
            skipped.append((name, str(e)))
            return
        out.append((name, bytes(raw), text))

    def put(field, idx, value):
        def fn(raw, img):
            a = getattr(img, field)
            a.reshape(-1)[idx] = value
        return fn

    edit("count[leaf] = -5", "row count", put("count", leaf, -5))
    edit("count[leaf] = n + 1", "row count", put("count", leaf, n + 1))
    edit("count[root] = 2^33", "row count", put("count", node, 2 ** 33))
    edit("count[leaf] off by one", "leaf count differs", put("count", leaf, int(img0.count[leaf]) + (1 if img0.count[leaf] < n else -1)))
    edit("depth[leaf] = 200", "depth", put("depth", leaf, 200))
    edit("depth[leaf] + 1", "depth", put("depth", leaf, int(img0.depth[leaf]) + 1))
    edit("depth[root] = 1", "root depth", put("depth", node, 1))
    edit("a leaf with another leaf's label", "label used twice", put("label", leaf2, int(img0.label[leaf])))

    def lid_of_a_leaf_row(value):
        def fn(raw, img):
            rows = np.flatnonzero(img.lid[big] == img0.label[leaf])
            if rows.size == 0:
                raise LookupError("the leaf holds no row")
            img.lid[big, rows[0]] = value
        return fn

    edit("lid byte 250 on a leaf's row", "leaf count differs", lid_of_a_leaf_row(250))
    edit("a leaf's row made an orphan", "leaf count differs", lid_of_a_leaf_row(ORPHAN))

    def lid_of_an_orphan(raw, img):
        t, rows = np.nonzero(np.asarray(img.lid) == ORPHAN)
        if rows.size == 0:
            raise LookupError("no orphan rows")
        free = sorted(set(range(250)) - set(int(x) for x in img0.label[noff[t[0]]: noff[t[0] + 1]][img0.var[noff[t[0]]: noff[t[0] + 1]] < 0]))
        img.lid[t[0], rows[0]] = free[-1]

    edit("an orphan row with a label no leaf has", "row label of no leaf", lid_of_an_orphan)
    edit("value[leaf] = NaN", "leaf values", put("value", leaf * K + K - 1, np.nan))
    edit("slope[leaf] = inf", "leaf values", put("slope", leaf * K, np.inf))
    edit("xbar[leaf] = NaN", "leaf values", put("xbar", leaf, np.nan))
    edit("sum_trees[0] = inf", "sum_trees", put("sum_trees", 0, np.inf))
    edit("sum_trees[last] = NaN", "sum_trees", put("sum_trees", K * n - 1, np.nan))
    edit("rs_mean = NaN", "running sd", put("rs_mean", n // 2, np.nan))
    edit("rs_m2 = -inf", "running sd", put("rs_m2", K * n - 1, -np.inf))
    edit("alpha[0] = -1", "negative split weight", put("alpha", 0, -1))
    edit("cdf[0] = -1", "split weight sums decrease", put("cdf", 0, -1))
    edit("cdf[p-1] < cdf[p-2]", "split weight sums decrease", put("cdf", p - 1, int(img0.cdf[p - 2]) - 1))
    edit("split[inner] = NaN", "split value", put("split", node, np.nan))
    edit("left == right", "children", put("right", node, int(img0.left[node])))

    def inner_to_leaf(raw, img):
        img.var[base + deep] = -1
        img.left[base + deep] = -1
        img.right[base + deep] = -1

    edit("an inner node made a leaf (its children orphaned)", r"label used twice|leaf count differs|without a parent", inner_to_leaf)

    def two_parents(raw, img):
        # an inner node's right child becomes a node of the right depth that already has another parent
        depth = np.array(img0.depth[base: base + var.size])
        for a in inner:
            for j in range(int(a) + 1, var.size):
                if j not in (int(left[a]), int(right[a])) and depth[j] == depth[a] + 1:
                    img.right[base + int(a)] = j
                    return
        raise LookupError("no two inner nodes at the same depth")

    edit("a node with two parents, another with none", "without a parent, or with two", two_parents)
    edit("leaf_sd[0] = 0", "leaf_sd", lambda raw, img: _header_double(raw, "leaf_sd", 0, 0.0))
    edit("leaf_sd[0] = -1", "leaf_sd", lambda raw, img: _header_double(raw, "leaf_sd", 0, -1.0))
    edit("leaf_sd[K-1] = NaN", "leaf_sd", lambda raw, img: _header_double(raw, "leaf_sd", K - 1, np.nan))
    edit("leaf_sd[K-1] = inf", "leaf_sd", lambda raw, img: _header_double(raw, "leaf_sd", K - 1, np.inf))
    edit("lik_param[0] = inf", "likelihood parameters", lambda raw, img: _header_double(raw, "lik_param", 0, np.inf))
    edit("lik_param[1] = NaN", "likelihood parameters", lambda raw, img: _header_double(raw, "lik_param", 1, np.nan))
    hd = img0.header
    edit("rs_count = iter + 1", "cursor", lambda raw, img: _header_int64(raw, ImageHeader.rs_count.offset, hd.iter + 1))
    edit("iter = 2^63 - 1", "cursor", lambda raw, img: _header_int64(raw, ImageHeader.iter.offset, 2 ** 63 - 1))
    edit("ctr.rounds = -1", "counters", lambda raw, img: _header_int64(raw, ImageHeader.ctr.offset + type(hd.ctr).rounds.offset, -1))
    edit("ctr.slots = 2^63 - 1", "counters",
         lambda raw, img: _header_int64(raw, ImageHeader.ctr.offset + type(hd.ctr).slots.offset, 2 ** 63 - 1))
    edit("alpha[p-1] = 2^63 - 1", "split weights beyond", put("alpha", p - 1, 2 ** 63 - 1))
    assert C.sizeof(ImageHeader) == img0.header.header_bytes
    return out, skipped
