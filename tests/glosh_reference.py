"""Test-side reference for the GLOSH outlier scores: a plain top-down restatement.

Definitions (Campello et al., "Hierarchical density estimates for data clustering,
visualization, and outlier detection", and the project's canonical tie rules, DESIGN.md
"flat labels" / "outlier scores"):

* the hierarchy is read off the spanning tree by removing its edges in descending weight, all
  edges of one weight (a tie group) at once;
* when a cluster's component falls apart, a part with >= minClSize points is *valid*; with two
  or more valid parts the cluster ends and each valid part starts a child cluster, with exactly
  one the cluster lives on in it; the points of every other part become noise at that level:
  eps(x) = the level, last(x) = the cluster they leave;
* a cluster's death level is the level at which its last points leave it; eps_max(C) is the
  lowest death level among C and its descendants -- except for the root, which takes its
  descendants only and starts from the largest finite double when it has none;
* score(x) = 0 if eps(x) == 0 else 1 - eps_max(last(x)) / eps(x).

O(levels x n): for n of about 2,000 or less.
"""
import sys

import numpy as np

DBL_MAX = sys.float_info.max


def glosh_reference(va, vb, w, n, min_cl_size):
    """Returns (scores[n], eps[n]) as float64 arrays."""
    va, vb = np.asarray(va, np.int64), np.asarray(vb, np.int64)
    w = np.asarray(w, np.float64)
    eps = np.zeros(n, np.float64)
    last = np.zeros(n, np.int64)
    adj = [set() for _ in range(n)]
    by_level = {}
    for a, b, x in zip(va.tolist(), vb.tolist(), w.tolist()):
        if a == b:
            continue
        adj[a].add(b)
        adj[b].add(a)
        by_level.setdefault(x + 0.0, []).append((a, b))  # -0.0 and 0.0 are one level
    cluster_of = [0] * n           # -1 once a point is noise
    parent = [-1]                  # cluster tree; cluster 0 is the root holding every point
    death = [0.0]
    for level in sorted(by_level, reverse=True):
        touched = {}               # cluster -> endpoints of its removed edges
        for a, b in by_level[level]:
            adj[a].discard(b)
            adj[b].discard(a)
            c = cluster_of[a]
            if c >= 0:
                touched.setdefault(c, []).extend((a, b))
        for c, ends in touched.items():
            seen, parts = set(), []
            for s in ends:         # every part of the broken component holds such an endpoint
                if s in seen:
                    continue
                seen.add(s)
                part, i = [s], 0
                while i < len(part):
                    for y in adj[part[i]]:
                        if y not in seen:
                            seen.add(y)
                            part.append(y)
                    i += 1
                parts.append(part)
            valid = [p for p in parts if len(p) >= min_cl_size]
            for p in parts:
                if len(p) < min_cl_size:
                    for x in p:
                        eps[x] = level
                        last[x] = c
                        cluster_of[x] = -1
            if len(valid) >= 2:
                for p in valid:
                    parent.append(c)
                    death.append(0.0)
                    for x in p:
                        cluster_of[x] = len(parent) - 1
            if len(valid) != 1:
                death[c] = level   # no point is left in c
    eps_max = list(death)
    eps_max[0] = DBL_MAX
    for c in range(len(parent) - 1, 0, -1):  # children were numbered after their parents
        eps_max[parent[c]] = min(eps_max[parent[c]], eps_max[c])
    scores = np.zeros(n, np.float64)
    with np.errstate(over="ignore"):
        for x in range(n):
            if eps[x] != 0.0:
                scores[x] = np.float64(1.0) - np.float64(eps_max[last[x]]) / np.float64(eps[x])
    return scores, eps
