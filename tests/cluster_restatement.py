"""An independent restatement of the connected clusters (include/gdyn_cluster.h) for the tests of csrc/gdyn_cluster.hip,
cluster.py and gd_clusters.  numpy, fp64 in exactly the header's operation order (numpy rounds every elementwise operation on its
own); it shares no code with the package.  Two routes from the same edge list to the canonical roots: a plain sequential
union-find (components) and scipy.sparse.csgraph.connected_components canonicalised by np.minimum.at (components_scipy)."""
import numpy as np

MAX_LABELS = 8


def n_classes(K):
    return K * (K + 1) // 2


def class_index(a, b, K):
    """The class of an unordered pair with labels a and b (arrays or scalars): p = lo K - lo (lo - 1) / 2 + (hi - lo), lo <= hi."""
    lo, hi = np.minimum(a, b).astype(np.int64), np.maximum(a, b).astype(np.int64)
    return lo * K - lo * (lo - 1) // 2 + (hi - lo)


def link_mask(links, K):
    """"all", "same" or [(a, b), ...] as the 64-bit mask."""
    if isinstance(links, (int, np.integer)):
        return int(links)
    if links == "all":
        return (1 << n_classes(K)) - 1
    pairs = [(a, a) for a in range(K)] if links == "same" else links
    mask = 0
    for a, b in pairs:
        mask |= 1 << int(class_index(np.int64(a), np.int64(b), K))
    return mask


def frames_of(F, first=0, count=0, stride=1):
    if count:
        return [first + k * stride for k in range(count)]
    return list(range(first, F, stride))


def _selection(N, label, K):
    if label is None:
        return np.arange(N), np.zeros(N, np.int64), 1
    label = np.asarray(label, np.int64)
    return np.flatnonzero(label >= 0), label, K


def _kept(p, lab, K, i, j, box, distance, mask):
    """Of the candidate pairs (i, j) (index arrays into the selected beads, each unordered pair at most once), those that are edges."""
    r = p[i] - p[j]
    if box is not None:
        b = np.broadcast_to(np.asarray(box, np.float64), (3,))
        r = r - b * np.rint(r / b)
    r2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    keep = r2 < distance * distance
    cls = class_index(lab[i], lab[j], K)
    keep &= ((np.uint64(mask) >> cls.astype(np.uint64)) & np.uint64(1)).astype(bool)
    return i[keep], j[keep]


def edges(x_frame, distance, box=None, label=None, K=1, links="all", candidates=None, chunk=256):
    """(sel, i, j): the selected beads (ascending bead indices) and the edges of one frame as indices into sel, each once.
    candidates: a function (positions of the selected beads) -> (i, j) candidate pairs that replaces the walk over all pairs."""
    sel, label, K = _selection(len(x_frame), label, K)
    mask = link_mask(links, K)
    p, lab = np.asarray(x_frame).astype(np.float64)[sel], label[sel]
    if candidates is not None:
        i, j = candidates(p)
        i, j = _kept(p, lab, K, np.asarray(i, np.int64), np.asarray(j, np.int64), box, distance, mask)
        return sel, i, j
    ei, ej = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for i0 in range(0, len(p), chunk):
        i, j = np.meshgrid(np.arange(i0, min(i0 + chunk, len(p))), np.arange(len(p)), indexing="ij")
        first_of = i < j
        a, b = _kept(p, lab, K, i[first_of], j[first_of], box, distance, mask)
        ei.append(a)
        ej.append(b)
    return sel, np.concatenate(ei), np.concatenate(ej)


def roots_union_find(N, sel, i, j):
    """root (N) int32 by a sequential union-find with the smaller index as the root; -1 for a bead that is not selected."""
    parent = list(range(len(sel)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in zip(i.tolist(), j.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    root = np.full(N, -1, np.int32)
    for k in range(len(sel)):
        root[sel[k]] = sel[find(k)]      # sel ascends: the smallest selected index is the smallest bead index
    return root


def roots_scipy(N, sel, i, j):
    """The same by scipy.sparse.csgraph.connected_components, canonicalised: the smallest bead index of every component."""
    import scipy.sparse
    import scipy.sparse.csgraph
    n = len(sel)
    root = np.full(N, -1, np.int32)
    if n == 0:
        return root
    graph = scipy.sparse.coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n, n))
    count, comp = scipy.sparse.csgraph.connected_components(graph, directed=False)
    smallest = np.full(count, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(smallest, comp, sel.astype(np.int64))
    root[sel] = smallest[comp]
    return root


def tables(root, n_size_bins):
    """summary (4) uint64 and hist (n_size_bins) uint64 of one frame's roots."""
    taken = root[root >= 0]
    sizes = np.bincount(taken, minlength=1)
    sizes = sizes[sizes > 0].astype(np.uint64)
    summary = np.zeros(4, np.uint64)
    hist = np.zeros(n_size_bins, np.uint64)
    if len(taken):
        summary[:] = [len(taken), len(sizes), sizes.max(), int((sizes.astype(object) ** 2).sum())]
        np.add.at(hist, (np.minimum(sizes, np.uint64(n_size_bins)) - np.uint64(1)).astype(np.int64), np.uint64(1))
    return summary, hist


def components(x, distance, box=None, label=None, K=1, links="all", n_size_bins=64, first=0, count=0, stride=1, candidates=None, route=roots_union_find):
    """(root (F, N) int32, summary (F, 4) uint64, hist (F, n_size_bins) uint64) of the frames first + k stride."""
    x = np.asarray(x)
    if x.ndim == 2:
        x = x[None]
    fr = frames_of(len(x), first, count, stride)
    N = x.shape[1]
    root, summary, hist = np.zeros((len(fr), N), np.int32), np.zeros((len(fr), 4), np.uint64), np.zeros((len(fr), n_size_bins), np.uint64)
    for o, f in enumerate(fr):
        sel, i, j = edges(x[f], distance, box, label, K, links, candidates)
        root[o] = route(N, sel, i, j)
        summary[o], hist[o] = tables(root[o], n_size_bins)
    return root, summary, hist


def components_scipy(*args, **kw):
    return components(*args, route=roots_scipy, **kw)


def kdtree_candidates(distance, box=None):
    """candidates= for sizes where the walk over all pairs is too slow: cKDTree.query_pairs a little beyond the distance, in a periodic
    box on the wrapped coordinates (the edge test itself stays _kept's, on the coordinates as given)."""
    import scipy.spatial

    def fn(p):
        if box is None:
            return scipy.spatial.cKDTree(p).query_pairs(distance * (1 + 1e-6) + 1e-9, output_type="ndarray").T
        b = np.broadcast_to(np.asarray(box, np.float64), (3,))
        w = np.mod(p, b)
        w[w >= b] = 0.0
        return scipy.spatial.cKDTree(w, boxsize=b).query_pairs(distance * (1 + 1e-6) + 1e-6, output_type="ndarray").T
    return fn


def known_cases():
    """[(name, x (N, 3) float64 exactly representable in float32, distance, box, label, K, links, root)]"""
    up = float(np.nextafter(np.float32(3.0), np.float32(4.0)))
    cases = [
        ("exactly the distance apart", [[0, 0, 0], [3, 0, 0], [10, 0, 0], [10, 4, 0], [10, 4, 12]], 3.0, None, None, 1, "all", [0, 1, 2, 3, 4]),
        ("the next float above the distance", [[0, 0, 0], [3, 0, 0], [10, 0, 0], [10, 4, 0]], up, None, None, 1, "all", [0, 0, 2, 3]),
        ("a bead that takes no part does not bridge", [[0, 0, 0], [0.75, 0, 0], [1.5, 0, 0]], 1.0, None, [0, -1, 0], 1, "all", [0, -1, 2]),
        ("the same three, all taking part", [[0, 0, 0], [0.75, 0, 0], [1.5, 0, 0]], 1.0, None, [0, 0, 0], 1, "all", [0, 0, 0]),
        ("an A-B contact under same", [[0, 0, 0], [0.5, 0, 0], [0.5, 0.5, 0], [5, 5, 5]], 1.0, None, [0, 1, 1, 0], 2, "same", [0, 1, 1, 3]),
        ("the A-B contact alone", [[0, 0, 0], [0.5, 0, 0], [0.5, 0.5, 0], [5, 5, 5]], 1.0, None, [0, 1, 1, 0], 2, [(1, 0)], [0, 0, 0, 3]),
        ("three beads across a periodic boundary", [[0.25, 5, 5], [9.75, 5, 5], [9.25, 5, 5], [5, 5, 5]], 0.75, (10.0, 10.0, 10.0), None, 1, "all",
         [0, 0, 0, 3]),
        ("the same three in an open box", [[0.25, 5, 5], [9.75, 5, 5], [9.25, 5, 5], [5, 5, 5]], 0.75, None, None, 1, "all", [0, 1, 1, 3]),
        ("coincident beads", [[1, 2, 3], [7, 7, 7], [1, 2, 3], [1, 2, 3], [7, 7, 7]], 0.125, None, None, 1, "all", [0, 1, 0, 0, 1]),
    ]
    return [(n, np.array(x, np.float64), d, box, None if lab is None else np.array(lab), K, links, np.array(root, np.int32))
            for n, x, d, box, lab, K, links, root in cases]
