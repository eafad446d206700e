"""Device scratch reused on ONE context across sizes that grow, shrink and grow again (csrc/common.hpp
Carver and carve(), csrc/sort.hpp with_tmp): every arena is sized by a probing pass of the layout
that then assigns its pointers, and an arena only grows, so a call after a larger one runs in a
buffer sized for another n, and a call after a smaller one must grow it first.  A probe that sized
too little would show here as a wrong tree or wrong labels.

The exact leaf (csrc/spatial.hip), the flat labels (csrc/flat.hip) and the constrained labels
(csrc/constraints.hip) run for n = 4097, 257, 20000, 2 at d = 3, minPts 4: the prim_leaf and tile
edges, more than one 512-point group and several BVH levels, and the degenerate 2.  With count_evals
off and on (the diagnostic array changes the Boruvka layout) and ssort 1 and 0 (0 takes the radix
sorts and their temp buffers).  Checked as the tests of these calls check them: sorted MST weights
against the oracle Prim's, labels against the host algorithms (csrc/flat.cpp, csrc/constraints.cpp)."""
import functools

import numpy as np
import pytest
import torch

from conftest import blobs
from constraints_reference import random_constraints
from path_helpers import bits_eq, options, spanning_tree
from test_constraints import same_result
from test_flat_labels import lib_flat
from test_gpu_constraints import Host, cuda, dev_tree

pytestmark = pytest.mark.gpu

SIZES = (4097, 257, 20000, 2)
MIN_PTS, MCS, EXCL_SELF = 4, 4, 2


def top(w):
    """sorted weights; the reference Prim leaves Double.MAX_VALUE where the exact leaf reports +inf
    (n = 2 below minPts: as test_gpu_list_bound reads them)"""
    w = np.asarray(w, np.float64)
    return np.sort(np.where(w == np.finfo(np.float64).max, np.inf, w))


@functools.lru_cache(maxsize=None)
def reference(n):
    """(X, oracle core distances, the oracle Prim's sorted weights), once per size"""
    from oracle import oracle as O
    O.lib()
    X = np.ascontiguousarray(blobs(n, 3, 4, n), np.float64)
    core = O.core_distances(X, MIN_PTS, semantics=EXCL_SELF)
    _, _, pw = O.prim_mst(X, core, self_edges=False)
    pw = top(pw)
    for a in (X, core, pw):
        a.setflags(write=False)
    return X, core, pw


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.Context(0)  # one context of this module's own: its arenas start empty


@pytest.mark.parametrize("ssort", [1, 0])
@pytest.mark.parametrize("count_evals", [0, 1])
def test_grow_shrink_grow_on_one_context(pkg, ctx, count_evals, ssort):
    star = pkg.HDBSCANStar(ctx)
    with options(ctx, count_evals=count_evals, ssort=ssort):
        for n in SIZES:
            where = (n, count_evals, ssort)
            X, ref_core, ref_w = reference(n)
            core, g = star.exactMST(X, MIN_PTS, None, EXCL_SELF, selfEdges=False)
            va, vb, w = g.getVerticeA(), g.getVericeB(), g.getEges()
            assert bits_eq(core, ref_core), where
            assert spanning_tree(va, vb, n) and bits_eq(top(w), ref_w), where
            lab, k = pkg.flat_labels(cuda(va), cuda(vb), cuda(w, np.float64), n, MCS, ctx=ctx)
            want, kw = lib_flat(pkg, va, vb, w, n, MCS)
            assert k == kw and np.array_equal(lab.cpu().numpy(), want), where
            tree = pkg.cluster_tree(np.asarray(va, np.int32), np.asarray(vb, np.int32), np.asarray(w, np.float64), n, MCS)
            for m in (0, 7, 300):
                c = random_constraints(n, m, n + m)
                r = pkg.constrained_flat_labels(dev_tree(pkg, tree), *[cuda(x) for x in c], ctx=ctx)
                assert torch.is_tensor(r.labels) and r.labels.is_cuda
                same_result(Host(r), pkg.constrained_flat_labels(tree, *c), where + (m,))
