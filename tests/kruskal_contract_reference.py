"""Plain Python restatement of the K6 alpha-edge contraction (csrc/flat.hip, section 2).

Edges are given in rank order (rank = position, ascending weight, ties already broken), points
are 0..n-1.  ``kruskal`` is the sequential process the device must equal; ``contract`` builds the
same three arrays (parent, |C(e)|, smallest id of C(e)) the way the device does:

1. m(p) = the lightest edge at point p.  Edge e is non-alpha iff it is m() of an endpoint;
   c(e) counts those endpoints, cmin(e) is the smallest of them.  Alpha edges are numbered in
   rank order; apos(e) = alpha edges below rank e.
2. A non-alpha edge with c = 1 points to m() of its other endpoint (a lighter non-alpha edge),
   one with c = 2 is a root: the forest's trees are the super-vertices, numbered by the rank of
   their root edge.  a0(V) = the smallest alpha index at V.
3. Kruskal on the alpha edges over the super-vertices gives parent_alpha.
4. A non-alpha edge e of V with apos(e) <= a0(V) (or no alpha edge at V) is keyed V; otherwise
   it is keyed n_alpha + b, b = the last ancestor-or-self of a0(V) with index < apos(e).
5. A stable sort by key keeps the rank order inside a key; an inclusive scan of (sum c, min cmin)
   over each run gives pre / premin and the run totals.
6. Kruskal on the alpha edges again with weights: vertex V = its bottom run's totals, the
   component under alpha edge R = (size, min) of R combined with the totals of run n_alpha + R.
7. The arrays in rank space.

Steps 3 and 6 are sequential here.  The device runs them as a rank divide and conquer, where an
edge is the root of its component at several depths; there every edge adds the totals of the
run above it to its component, which this restatement cannot exercise:
tests/test_gpu_flat_contract.py does.
"""

NONE = 2**31 - 1


def kruskal(n, edges):
    """Sequential Kruskal over edges in rank order: parent, size and smallest id per edge."""
    m = len(edges)
    uf = list(range(n))
    root_edge = [-1] * n
    size = [1] * n
    mn = list(range(n))
    parent = [NONE] * m
    esize = [0] * m
    eminid = [0] * m

    def find(x):
        while uf[x] != x:
            uf[x] = uf[uf[x]]
            x = uf[x]
        return x

    for e, (u, v) in enumerate(edges):
        a, b = find(u), find(v)
        assert a != b, "cycle"
        for r in (a, b):
            if root_edge[r] >= 0:
                parent[root_edge[r]] = e
        if size[a] < size[b]:
            a, b = b, a
        uf[b] = a
        size[a] += size[b]
        mn[a] = min(mn[a], mn[b])
        root_edge[a] = e
        esize[e] = size[a]
        eminid[e] = mn[a]
    return parent, esize, eminid


def _weighted_kruskal(nv, edges, wv, mv, wl=None, ml=None):
    """Kruskal over super-vertices: vertex V weighs (wv, mv); the component under edge R gains
    (wl[R], ml[R]) once R is complete (its chain), before a heavier edge consumes it."""
    m = len(edges)
    uf = list(range(nv))
    root_edge = [-1] * nv
    size = list(wv)
    mn = list(mv)
    parent = [NONE] * m
    esize = [0] * m
    eminid = [0] * m

    def find(x):
        while uf[x] != x:
            uf[x] = uf[uf[x]]
            x = uf[x]
        return x

    for e, (u, v) in enumerate(edges):
        a, b = find(u), find(v)
        assert a != b, "cycle"
        for r in (a, b):
            R = root_edge[r]
            if R >= 0:
                parent[R] = e
                if wl is not None:
                    size[r] += wl[R]
                    mn[r] = min(mn[r], ml[R])
        if size[a] < size[b]:
            a, b = b, a
        uf[b] = a
        size[a] += size[b]
        mn[a] = min(mn[a], mn[b])
        root_edge[a] = e
        esize[e] = size[a]
        eminid[e] = mn[a]
    return parent, esize, eminid


def contract(n, edges):
    """The contraction path; returns (parent, esize, eminid, n_alpha_edges)."""
    m = len(edges)
    # 1. classify
    mp = [NONE] * n
    for e, (u, v) in enumerate(edges):
        mp[u] = min(mp[u], e)
        mp[v] = min(mp[v], e)
    c = [0] * m
    cmin = [NONE] * m
    up = [0] * m
    for e, (u, v) in enumerate(edges):
        cu, cv = mp[u] == e, mp[v] == e
        c[e] = cu + cv
        if cu:
            cmin[e] = min(cmin[e], u)
        if cv:
            cmin[e] = min(cmin[e], v)
        up[e] = e if c[e] != 1 else (mp[v] if cu else mp[u])
    apos, vpos = [0] * m, [0] * m
    ma = nv = 0
    for e in range(m):
        apos[e], vpos[e] = ma, nv
        ma += c[e] == 0
        nv += c[e] == 2
    assert ma == nv - 1 and 2 * ma < max(m, 1)
    # 2. super-vertices
    ev = [NONE] * m
    for e in range(m):
        if c[e]:
            r = e
            while up[r] != r:
                r = up[r]
            ev[e] = vpos[r]
    arank = [e for e in range(m) if c[e] == 0]
    aedges = [(ev[mp[edges[e][0]]], ev[mp[edges[e][1]]]) for e in arank]
    a0 = [NONE] * nv
    for a, (x, y) in enumerate(aedges):
        a0[x] = min(a0[x], a)
        a0[y] = min(a0[y], a)
    # 3. alpha tree, pass 1
    par_a, _, _ = _weighted_kruskal(nv, aedges, [1] * nv, list(range(nv)))
    # 4. keys (the climb is a binary-lifting search on the device)
    ALPHA_KEY = 2 * ma + 1
    key = [ALPHA_KEY] * m
    for e in range(m):
        if not c[e]:
            continue
        V = ev[e]
        if a0[V] == NONE or apos[e] <= a0[V]:
            key[e] = V
        else:
            b = a0[V]
            while par_a[b] != NONE and par_a[b] < apos[e]:
                b = par_a[b]
            key[e] = nv + b
    # 5. chains
    order = sorted((e for e in range(m) if c[e]), key=lambda e: key[e])  # stable
    pre, premin = [0] * m, [NONE] * m
    wv, mv = [0] * nv, [NONE] * nv
    wl, ml = [0] * ma, [NONE] * ma
    first = [NONE] * ma
    nxt = [NONE] * m  # next edge of the chain
    for i, e in enumerate(order):
        head = i == 0 or key[order[i - 1]] != key[e]
        pre[e] = c[e] + (0 if head else pre[order[i - 1]])
        premin[e] = min(cmin[e], NONE if head else premin[order[i - 1]])
        if not head:
            nxt[order[i - 1]] = e
        elif key[e] >= nv:
            first[key[e] - nv] = e
        if i + 1 == len(order) or key[order[i + 1]] != key[e]:
            if key[e] < nv:
                wv[key[e]], mv[key[e]] = pre[e], premin[e]
            else:
                wl[key[e] - nv], ml[key[e] - nv] = pre[e], premin[e]
    # 6. alpha tree, pass 2
    par_2, es_a, em_a = _weighted_kruskal(nv, aedges, wv, mv, wl, ml)
    assert par_2 == par_a
    # 7. rank space
    parent, esize, eminid = [NONE] * m, [0] * m, [0] * m
    up_rank = lambda a: NONE if a == NONE else arank[a]
    for a, e in enumerate(arank):
        esize[e], eminid[e] = es_a[a], em_a[a]
        parent[e] = first[a] if first[a] != NONE else up_rank(par_a[a])
    for e in range(m):
        if not c[e]:
            continue
        k = key[e]
        if k < nv:
            base, basemin, last = 0, NONE, up_rank(a0[k])
        else:
            base, basemin, last = es_a[k - nv], em_a[k - nv], up_rank(par_a[k - nv])
        esize[e] = base + pre[e]
        eminid[e] = min(basemin, premin[e])
        parent[e] = nxt[e] if nxt[e] != NONE else last
    return parent, esize, eminid, ma
