"""The alpha-edge contraction of K6 (csrc/flat.hip section 2; kruskal_contract_reference.py is its
plain Python restatement) against sequential Kruskal: parent, |C(e)| and the smallest id of C(e)
per edge, on seeded trees of 2 to 400 points -- random, hub, path and caterpillar shapes under
random, monotone and V-shaped rank orders."""
import random

import pytest

from kruskal_contract_reference import contract, kruskal

SHAPES = ("random", "hub", "path", "caterpillar")
ORDERS = ("random", "monotone", "vshape")


def tree(shape, n, rng):
    """n - 1 edges (u, v) in construction order: vertex i + 1 attaches to an earlier one"""
    if shape == "random":
        par = [rng.randrange(i + 1) for i in range(n - 1)]
    elif shape == "hub":
        par = [0 if rng.random() < 0.3 else rng.randrange(i + 1) for i in range(n - 1)]
    elif shape == "path":
        par = list(range(n - 1))
    else:  # a spine over the first half, every other vertex a leaf of a random spine vertex
        spine = max(1, n // 2)
        par = [i if i + 1 < spine else rng.randrange(spine) for i in range(n - 1)]
    return [(par[i], i + 1) for i in range(n - 1)]


def ranked(edges, order, rng):
    """the edges in rank order, the points renamed by a random permutation"""
    m = len(edges)
    if order == "random":
        idx = list(range(m))
        rng.shuffle(idx)
    elif order == "monotone":
        idx = list(range(m)) if rng.random() < 0.5 else list(range(m - 1, -1, -1))
    else:  # lightest in the middle of the construction order, rising toward both ends
        mid = m // 2
        idx = sorted(range(m), key=lambda i: (abs(i - mid), i))
    perm = list(range(m + 1))
    rng.shuffle(perm)
    return [(perm[edges[i][0]], perm[edges[i][1]]) for i in idx]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("order", ORDERS)
def test_contraction_equals_sequential_kruskal(shape, order):
    rng = random.Random(f"{shape}/{order}")
    sizes = list(range(2, 41)) * 5 + [rng.randrange(41, 401) for _ in range(60)]
    for n in sizes:  # 255 trees per (shape, order): 3060 in all
        edges = ranked(tree(shape, n, rng), order, rng)
        ref = kruskal(n, edges)
        parent, esize, eminid, ma = contract(n, edges)
        assert (parent, esize, eminid) == ref, (shape, order, n, edges)
        assert 2 * ma < n - 1 or n == 2


def test_alpha_counts_of_known_shapes():
    # a monotone path has no alpha edge; a comb's spine edges (heavier than every tooth) all are
    path = [(i, i + 1) for i in range(50)]
    assert contract(51, path)[3] == 0
    teeth, tooth = 20, 5
    comb = [(t * tooth, t * tooth + j) for t in range(teeth) for j in range(1, tooth)]
    comb += [(t * tooth, (t + 1) * tooth) for t in range(teeth - 1)]
    got = contract(teeth * tooth, comb)
    assert got[3] == teeth - 1 and got[:3] == kruskal(teeth * tooth, comb)
