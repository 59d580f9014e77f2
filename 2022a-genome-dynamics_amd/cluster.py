"""Connected clusters of a history on the device: ctypes binding of ``include/gdyn_cluster.h`` (exported by ``csrc/libgdyn.so``).
Per frame, the connected components of the graph whose edges are the pairs of selected beads closer than a distance: which beads
form one domain, how many domains there are, how large the largest is and how their sizes are distributed.  The reference has no
such analysis: this is a capability beyond it.  The header states the definitions; every output is an integer that depends on
the graph alone, so the results are bit-identical from run to run and for every ``max_frames_per_launch``.

    c = Clusters(device=0)
    c.set_history(frames)                       # (F, N, 3) float32 or float64, kept in its precision
    c.set_history_from(recorder, replica)       # the same from frames a live.History recorded on the device
    c.set_labels(types, n_labels=2)             # label[i] in [-1, K), K <= 8; -1: takes no part; None: one label of all beads
    c.set_links("same")                         # "all" (default), "same" (a-a only) or [(a, b), ...]: the label pairs that may link
    r = c.components(0.35, box=(10, 10, 10))    # .root (F, N) int32, .selected .clusters .largest .sum_s2 (F) uint64, .histogram (F, bins)
    weight_average(r)                           # (F) float64: sum_s2 / selected
    sizes_of(r.root[0])                         # (N) the size of every bead's cluster
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from ._binding import GdynError, HistoryHandle, box3, load_history_library

CLUSTER_ABI_VERSION = 1      # GD_CLUSTER_ABI_VERSION of the include/gdyn_cluster.h this binding mirrors
CLUSTER_SYMBOLS = ["gd_cluster_abi_version", "gd_cluster_create", "gd_cluster_destroy", "gd_cluster_set_history", "gd_cluster_set_history_live",
                   "gd_cluster_set_labels", "gd_cluster_set_links", "gd_cluster_classes", "gd_cluster_frames", "gd_cluster_components"]
MAX_LABELS = 8               # GD_CLUSTER_MAX_LABELS
MAX_SIZE_BINS = 1 << 20      # GD_CLUSTER_MAX_SIZE_BINS

Components = namedtuple("Components", "root selected clusters largest sum_s2 histogram")


class _ClusterDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_frames_per_launch", C.c_uint32)]


def load_cluster_library(path=None):
    """Loads libgdyn and checks the gd_cluster_* symbols and their ABI version."""
    d = load_history_library("cluster", CLUSTER_SYMBOLS, CLUSTER_ABI_VERSION, path)
    d.gd_cluster_create.argtypes = [C.POINTER(_ClusterDesc), C.POINTER(C.c_void_p)]
    d.gd_cluster_destroy.argtypes = [C.c_void_p]
    d.gd_cluster_set_labels.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    d.gd_cluster_set_links.argtypes = [C.c_void_p, C.c_uint64]
    d.gd_cluster_classes.argtypes = [C.c_void_p]
    d.gd_cluster_classes.restype = C.c_uint32
    d.gd_cluster_frames.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    d.gd_cluster_frames.restype = C.c_uint32
    d.gd_cluster_components.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_double, C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
    return d


# ---- pure Python: the definitions of the header that a caller needs without a device

def n_classes(n_labels):
    """P: the unordered label pairs."""
    return n_labels * (n_labels + 1) // 2


def class_index(a, b, n_labels):
    """The class of a pair with labels a and b: lo K - lo (lo - 1) / 2 + (hi - lo)."""
    lo, hi = min(int(a), int(b)), max(int(a), int(b))
    if lo < 0 or hi >= n_labels:
        raise ValueError(f"labels ({a}, {b}) are not in [0, {n_labels})")
    return lo * n_labels - lo * (lo - 1) // 2 + (hi - lo)


def link_mask(pairs, n_labels):
    """The 64-bit mask of "all", "same" or a list of label pairs [(a, b), ...]: bit class_index(a, b) set for every pair."""
    if n_labels < 1 or n_labels > MAX_LABELS:
        raise ValueError(f"{n_labels} labels (1 to {MAX_LABELS})")
    if isinstance(pairs, str):
        if pairs == "all":
            return (1 << n_classes(n_labels)) - 1
        if pairs != "same":
            raise ValueError(f'links must be "all", "same" or a list of label pairs, got {pairs!r}')
        pairs = [(a, a) for a in range(n_labels)]
    mask = 0
    for a, b in pairs:
        mask |= 1 << class_index(a, b, n_labels)
    if not mask:
        raise ValueError("an empty list of label pairs links nothing")
    return mask


def sizes_of(root):
    """The size of every bead's cluster from its root array (..., N): 0 for a bead that takes no part (root -1)."""
    root = np.asarray(root)
    flat = root.reshape(-1, root.shape[-1])
    out = np.zeros(flat.shape, np.int64)
    for r, o in zip(flat, out):
        taken = r >= 0
        o[taken] = np.bincount(r[taken], minlength=len(r))[r[taken]]
    return out.reshape(root.shape)


def weight_average(components):
    """The weight-average cluster size of every frame, sum of s^2 over the number of selected beads; NaN where no bead is selected."""
    total, n = np.asarray(components.sum_s2, np.float64), np.asarray(components.selected, np.float64)
    out = np.full(total.shape, np.nan)
    np.divide(total, n, out=out, where=n > 0)
    return out


class Clusters(HistoryHandle):
    """One device-side history with its bead labels and link mask.  max_frames_per_launch: 0 = automatic (no result depends on it)."""

    _prefix = "cluster"
    _destroy = "gd_cluster_destroy"

    def __init__(self, device=0, max_frames_per_launch=0, path=None):
        super().__init__(load_cluster_library(path))
        self._check(self.dll.gd_cluster_create(C.byref(_ClusterDesc(device, max_frames_per_launch)), C.byref(self._h)))
        self.n_labels = 1

    def _beads_changed(self, n_beads):      # the library drops labels and mask of another N
        self.n_labels = 1

    def set_labels(self, label, n_labels=None):
        """label: (N,) integers in [-1, n_labels), -1 for a bead that takes no part; None: one label of all beads.
        n_labels=None: the largest label + 1.  The link mask becomes "all"."""
        self.n_labels, _ = self._set_labels(label, n_labels)

    def set_links(self, links):
        """Which label pairs may link: "all", "same" (a with a only), a list [(a, b), ...], or the 64-bit mask itself."""
        mask = int(links) if isinstance(links, (int, np.integer)) else link_mask(links, self.n_labels)
        if mask < 0 or mask >= 1 << 64:
            raise ValueError("the link mask has 64 bits")
        self._check(self.dll.gd_cluster_set_links(self._h, mask))

    @property
    def n_classes(self):
        return int(self.dll.gd_cluster_classes(self._h))

    def components(self, distance, box=None, size_bins=64, roots=True, first_frame=0, n_frames=0, frame_stride=1):
        """Components(root (F, N) int32 or None, selected, clusters, largest, sum_s2 (F) uint64, histogram (F, size_bins) uint64) of the
        frames first_frame + k frame_stride (n_frames 0: all that fit).  box: a period or three, None: open.  root[f, i]: the
        smallest bead index of bead i's cluster, -1 for a bead that takes no part.  histogram[f, b]: clusters of size b + 1, the last
        bin those of size_bins and more."""
        box_at, _keep = box3(box)
        F = int(self.dll.gd_cluster_frames(self._h, int(first_frame), int(n_frames), int(frame_stride)))
        N = self.shape[1] if self.shape is not None else 0
        nb = int(size_bins)
        if nb < 0 or nb >= 1 << 32:
            raise ValueError(f"size_bins {size_bins}")
        keep = 0 < nb <= MAX_SIZE_BINS
        root = np.full((F, N), -1, np.int32) if roots else None
        summary, hist = np.zeros((F, 4), np.uint64), np.zeros((F, nb if keep else 1), np.uint64)
        self._check(self.dll.gd_cluster_components(self._h, int(first_frame), int(n_frames), int(frame_stride), box_at,
                                                   float(distance), nb, root.ctypes.data if roots else None, summary.ctypes.data, hist.ctypes.data))
        return Components(root, summary[:, 0].copy(), summary[:, 1].copy(), summary[:, 2].copy(), summary[:, 3].copy(), hist)
