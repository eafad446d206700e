"""The reference's record formats on either side of the hot path,
backed by csrc/formats.cpp through the C-ABI (host code; no device needed).

* ``MapperDataset_github`` / ``read_dataset`` -- the dataset text -> points
  (MapperDataset_github.java:12-20): ``s.split(" ")`` + ``Double.parseDouble``, one point per
  line, numbered in file order.  ``strict=False`` is deviation D1: runs of
  blanks/tabs separate fields and the first ``d`` columns are kept (Skin_NonSkin.txt is
  TAB-separated with a trailing label column).
* ``format_local_mst`` -- CreateLocalMST's local-MST text (CreateLocalMST.java:110-123):
  ``"v1 v2 w f1 f2 node"`` lines joined by ``\\n``, ``w`` via ``Double.toString``.
* ``parse_local_mst`` -- UnionFindReducer.call's parse of those records
  (UnionFindReducer.java:22-45).
* ``double_to_string`` -- ``Double.toString`` (Java layout, shortest round-trip digits).

Malformed fields raise ``NumberFormatException`` and short lines
``ArrayIndexOutOfBoundsException``, as the Java does.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._capi import check, lib, ptr


def double_to_string(v: float) -> str:
    """Double.toString(v)."""
    buf = C.create_string_buffer(40)
    n = lib().hdb_format_double(float(v), buf, 40)
    if n < 0:
        check(n, "hdb_format_double")
    return buf.value.decode()


def _as_bytes(text_or_path) -> bytes:
    if isinstance(text_or_path, (bytes, bytearray)):
        return bytes(text_or_path)
    if isinstance(text_or_path, str) and "\n" not in text_or_path and os.path.exists(text_or_path):
        with open(text_or_path, "rb") as fh:
            return fh.read()
    return str(text_or_path).encode()


def read_dataset(text_or_path, d: int = 0, strict: bool = False) -> np.ndarray:
    """The whole dataset as an ``n x d`` FP64 array in file order (the ids the reference's
    ``count`` assigns).  ``d = 0``: the first line's field count."""
    raw = _as_bytes(text_or_path)
    n, dd = C.c_int64(), C.c_int32()
    L = lib()
    check(L.hdb_parse_points(raw, len(raw), int(d), int(strict), None, 0, C.byref(n), C.byref(dd)),
          "hdb_parse_points")
    X = np.empty((n.value, dd.value), dtype=np.float64)
    check(L.hdb_parse_points(raw, len(raw), int(d), int(strict), ptr(X), n.value, C.byref(n), C.byref(dd)),
          "hdb_parse_points")
    return X


class MapperDataset_github:
    """PairFunction<String, Integer, Tuple2<Integer, double[]>> (MapperDataset_github.java:6-21):
    ``call(line)`` returns ``(0, (count, point))`` with a running ``count`` from 0."""

    def __init__(self, d: int = 0, strict: bool = True):
        self.count = -1
        self.d = d
        self.strict = strict

    def call(self, s: str):
        X = read_dataset(s.encode(), self.d, self.strict)
        if X.shape[0] != 1:
            raise ValueError("call() takes one line")
        self.count += 1
        return 0, (self.count, X[0])


def format_local_mst(va, vb, w, fake1=None, fake2=None, node=None) -> str:
    """CreateLocalMST.java:110-123 text for one local MST (edges in the given order)."""
    va = np.ascontiguousarray(np.asarray(va), dtype=np.int32)
    vb = np.ascontiguousarray(np.asarray(vb), dtype=np.int32)
    w = np.ascontiguousarray(np.asarray(w), dtype=np.float64)
    ne = va.shape[0]
    if vb.shape[0] != ne or w.shape[0] != ne:
        raise ValueError("va, vb, w must have the same length")
    extra = [None if a is None else np.ascontiguousarray(np.asarray(a), dtype=np.int32) for a in (fake1, fake2, node)]
    for a in extra:
        if a is not None and a.shape[0] != ne:
            raise ValueError("fake1/fake2/node must match the edge count")
    L = lib()
    n = C.c_int64()
    args = [ptr(va), ptr(vb), ptr(w), *[ptr(a) for a in extra], ne]
    check(L.hdb_format_mst_records(*args, None, 0, C.byref(n)), "hdb_format_mst_records")
    buf = C.create_string_buffer(n.value + 1)
    check(L.hdb_format_mst_records(*args, buf, n.value + 1, C.byref(n)), "hdb_format_mst_records")
    return buf.raw[: n.value].decode()


def format_outlier_scores(scores, ids) -> str:
    """The outlier-score file's text (HDBSCANStar.calculateOutlierScores :680-682 with its ","
    delimiter): one line ``Double.toString(score) + "," + id + "\\n"`` per entry, in the order
    given -- pass ``scores[p], p`` with ``p = outlier_ranking(scores, core)`` for the file the
    reference writes."""
    s = np.asarray(scores.detach().cpu().numpy() if hasattr(scores, "detach") else scores, dtype=np.float64)
    i = np.asarray(ids.detach().cpu().numpy() if hasattr(ids, "detach") else ids, dtype=np.int64)
    if s.shape != i.shape or s.ndim != 1:
        raise ValueError("scores and ids must be one-dimensional and of the same length")
    return "".join(f"{double_to_string(v)},{int(k)}\n" for v, k in zip(s, i))


def hierarchy_levels(tree, compact: bool = True) -> np.ndarray:
    """The levels the reference's hierarchy file has a row for, descending.  Every level
    computeHierarchyAndClusterTree processes is the level of a reached node: the distinct values
    of ``point_level`` together with ``birth[1:]``.  ``compact`` keeps the first level, every
    birth level and every level whose predecessor in that list is a birth level -- the
    ``!compactHierarchy || nextLevelSignificant || !newClusters.isEmpty()`` rule of
    HDBSCANStar.java:394."""
    t = tree.host()
    births = np.asarray(t.birth[1:], dtype=np.float64) + 0.0
    births = births[~np.isnan(births)]
    allv = np.unique(np.concatenate([np.asarray(t.point_level, dtype=np.float64) + 0.0, births]))[::-1]
    if not compact or allv.shape[0] == 0:
        return np.ascontiguousarray(allv)
    is_birth = np.isin(allv, births)
    keep = is_birth.copy()
    keep[0] = True
    keep[1:] |= is_birth[:-1]
    return np.ascontiguousarray(allv[keep])


def format_hierarchy(tree, levels=None, compact: bool = True, ctx=None):
    """The hierarchy file's text (HDBSCANStar.java:393-414, 436-442) and the cluster offsets
    (``setFileOffset``, :419-421): one row ``level,l0,...,l(n-1)\\n`` per level (default:
    ``hierarchy_levels(tree, compact)``) with the tree labels of ``labels_at_levels``, then the
    closing row of n + 1 zeros.  Levels are written as ``Double.toString`` writes them.  Returns
    ``(text, offsets)``: ``offsets[i]`` = the number of characters written through the row of
    tree label i + 1's birth level (0 for the root, and for a birth level that has no row)."""
    from .hdbscanstar import labels_at_levels
    t = tree.host()
    lv = hierarchy_levels(t, compact) if levels is None else np.ascontiguousarray(levels, dtype=np.float64)
    rows = labels_at_levels(tree, lv, ctx=ctx)
    rows = rows.detach().cpu().numpy() if hasattr(rows, "detach") else np.asarray(rows)
    parts, written, through = [], 0, {}
    for k in range(lv.shape[0]):
        line = double_to_string(lv[k]) + "".join(f",{v}" for v in rows[k].tolist()) + "\n"
        parts.append(line)
        written += len(line)
        through.setdefault(float(lv[k]) + 0.0, written)
    parts.append(",".join(["0"] * (t.n + 1)) + "\n")
    offsets = np.zeros(t.n_tree, dtype=np.int64)
    for i in range(1, t.n_tree):
        offsets[i] = through.get(float(t.birth[i]) + 0.0, 0)
    return "".join(parts), offsets


def format_cluster_tree(tree, offsets=None, constrained=None) -> str:
    """The cluster-tree file's text (HDBSCANStar.java:449-468): one line
    ``label,birth,death,stability,0,0,offset,parentLabel\\n`` per cluster in label order (the two
    zeros are the constraint counts of a run without constraints); doubles as ``Double.toString``
    writes them (``NaN`` for the root's birth and stability).  ``offsets``: the second result of
    format_hierarchy (default: zeros).  ``constrained``: the record of constrained_flat_labels; the
    two columns are then ``0.5 * num_sat / m`` and ``0.5 * prop_sat / m`` as doubles (``NaN`` for
    m == 0, Java's 0.0 / 0)."""
    t = tree.host()
    off = np.zeros(t.n_tree, dtype=np.int64) if offsets is None else np.asarray(offsets, dtype=np.int64)
    if off.shape[0] != t.n_tree:
        raise ValueError("offsets must have one entry per cluster")
    d = double_to_string
    if constrained is None:
        cols = ["0,0"] * t.n_tree
    else:
        host = lambda x: np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64)
        num, prop = host(constrained.num_sat), host(constrained.prop_sat)
        if num.shape[0] != t.n_tree or prop.shape[0] != t.n_tree:
            raise ValueError("constrained must have one entry per cluster")
        with np.errstate(invalid="ignore", divide="ignore"):
            m = np.float64(constrained.m)
            cols = [f"{d(0.5 * a / m)},{d(0.5 * b / m)}" for a, b in zip(num, prop)]
    return "".join(f"{i + 1},{d(t.birth[i])},{d(t.death[i])},{d(t.stability[i])},{cols[i]},{int(off[i])},{int(t.parent[i])}\n"
                   for i in range(t.n_tree))


def parse_constraints(text):
    """The constraints file (Main.java:49 ``constraints=<file>``): one constraint per line,
    ``a,b,ml`` (must-link) or ``a,b,cl`` (cannot-link), a and b point ids.  Returns
    ``(ca, cb, ctype)`` as int32 arrays (ctype 0 = must-link, 1 = cannot-link).  A trailing
    newline is allowed; anything else -- a blank line, another field count, a negative or
    non-decimal id, another type -- raises ValueError naming the line."""
    if isinstance(text, (bytes, bytearray)):
        text = bytes(text).decode()
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    ca, cb, ct = [], [], []
    for no, line in enumerate(lines, 1):
        f = line.rstrip("\r").split(",")
        if len(f) != 3 or f[2] not in ("ml", "cl") or not (f[0].isascii() and f[0].isdigit()) \
                or not (f[1].isascii() and f[1].isdigit()) or int(f[0]) > 2 ** 31 - 1 or int(f[1]) > 2 ** 31 - 1:
            raise ValueError(f"constraints line {no}: expected 'a,b,ml' or 'a,b,cl', got {line!r}")
        ca.append(int(f[0])), cb.append(int(f[1])), ct.append(0 if f[2] == "ml" else 1)
    return np.array(ca, np.int32), np.array(cb, np.int32), np.array(ct, np.int32)


def parse_local_mst(text):
    """UnionFindReducer.java:22-45: the records of one text value as arrays
    ``(va, vb, w, fake1, fake2, node)``."""
    raw = text.encode() if isinstance(text, str) else bytes(text)
    L = lib()
    n = C.c_int64()
    check(L.hdb_parse_mst_records(raw, len(raw), None, None, None, None, None, None, 0, C.byref(n)),
          "hdb_parse_mst_records")
    ne = n.value
    va, vb, f1, f2, nd = (np.empty(ne, np.int32) for _ in range(5))
    w = np.empty(ne, np.float64)
    check(L.hdb_parse_mst_records(raw, len(raw), ptr(va), ptr(vb), ptr(w), ptr(f1), ptr(f2), ptr(nd), ne,
                                  C.byref(n)), "hdb_parse_mst_records")
    return va, vb, w, f1, f2, nd
