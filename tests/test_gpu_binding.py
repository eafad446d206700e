"""The context rule of the Python wrappers (_capi.context_for) on the six hierarchy functions:
called with device tensors and no ctx, on a thread whose context has made no call yet and under
a non-default torch stream, each gives the host path's result bit for bit and leaves this
thread's context on that stream (so the call was ordered with the torch work around it).  Input:
300 blobs in 2-d, oracle core distances, the Kruskal reference MST, minClSize 5."""
import threading

import numpy as np
import pytest
import torch

from conftest import blobs
from constraints_reference import random_constraints
from path_helpers import kruskal_mst
from test_cluster_tree import DOUBLES, INTS, same_tree
from test_hierarchy_weights import same_constrained
from test_outlier_scores import bits

pytestmark = pytest.mark.gpu

N, MCS = 300, 5


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.fixture(scope="module")
def case(pkg, oracle):
    """host inputs and the host path's results, computed once"""
    X = np.round(blobs(N, 2, 3, 5), 1)
    lo, hi, w = kruskal_mst(X, oracle.core_distances(X, 4, semantics=2))
    order = np.argsort(-w, kind="stable")  # merged order: descending weight
    va, vb, w = lo[order], hi[order], w[order]
    tree = pkg.cluster_tree(va, vb, w, N, MCS)
    assert tree.n_clusters >= 2 and tree.n_tree >= 3
    levels = np.concatenate([np.unique(w)[::7], [0.0, np.inf]])
    rng = np.random.default_rng(1)
    nearest = rng.integers(-1, N, 64).astype(np.int32)
    level = rng.choice(w, 64) * rng.choice([0.5, 1.0, 2.0], 64)
    ca, cb, ct = random_constraints(N, 40, 2)
    return dict(va=va, vb=vb, w=w, tree=tree, levels=levels, nearest=nearest, level=level, ca=ca, cb=cb, ct=ct,
                flat_labels=pkg.flat_labels(va, vb, w, N, MCS),
                outlier_scores=pkg.outlier_scores(va, vb, w, N, MCS, with_labels=True),
                labels_at_levels=pkg.labels_at_levels(tree, levels),
                predict_labels=pkg.predict_labels(tree, nearest, level),
                constrained_flat_labels=pkg.constrained_flat_labels(tree, ca, cb, ct))


def host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else x


def run(pkg, c, name):
    """the call on device tensors without a ctx, compared with the host result"""
    va, vb, w = cuda(c["va"]), cuda(c["vb"]), cuda(c["w"])
    t = c["tree"]
    dev_tree = pkg.ClusterTree(*[cuda(getattr(t, k)) for k in pkg.ClusterTree.FIELDS], t.n_clusters)
    want = c.get(name)
    if name == "flat_labels":
        labels, k = pkg.flat_labels(va, vb, w, N, MCS)
        assert labels.is_cuda and k == want[1] and np.array_equal(host(labels), want[0])
    elif name == "outlier_scores":
        s, e, labels, k = pkg.outlier_scores(va, vb, w, N, MCS, with_labels=True)
        assert s.is_cuda and k == want[3] and np.array_equal(host(labels), want[2])
        assert np.array_equal(bits(host(s)), bits(want[0])) and np.array_equal(bits(host(e)), bits(want[1]))
    elif name == "cluster_tree":
        got = pkg.cluster_tree(va, vb, w, N, MCS)
        assert got.parent.is_cuda and got.point_level.is_cuda
        same_tree(got.host(), t, name)
    elif name == "labels_at_levels":
        rows = pkg.labels_at_levels(dev_tree, cuda(c["levels"]))
        assert rows.is_cuda and np.array_equal(host(rows), want)
    elif name == "predict_labels":
        tl, lab, sc = pkg.predict_labels(dev_tree, cuda(c["nearest"]), cuda(c["level"]))
        assert tl.is_cuda and np.array_equal(host(tl), want[0]) and np.array_equal(host(lab), want[1])
        assert np.array_equal(bits(host(sc)), bits(want[2]))
    else:
        got = pkg.constrained_flat_labels(dev_tree, cuda(c["ca"]), cuda(c["cb"]), cuda(c["ct"]))
        assert got.labels.is_cuda
        for k in ("num_sat", "prop_sat", "flat_label", "labels", "prop_stability"):
            setattr(got, k, host(getattr(got, k)))
        same_constrained(got, want, name)


@pytest.mark.parametrize("name", ["flat_labels", "outlier_scores", "cluster_tree", "labels_at_levels",
                                  "predict_labels", "constrained_flat_labels"])
def test_tree_function_adopts_the_torch_stream(pkg, case, name):
    assert set(INTS) | set(DOUBLES) == set(pkg.ClusterTree.FIELDS)
    out = {}

    def body():
        try:
            s = torch.cuda.Stream()
            assert s.cuda_stream != 0 and s.cuda_stream != torch.cuda.default_stream().cuda_stream
            with torch.cuda.stream(s):
                run(pkg, case, name)
                out["stream"] = pkg.Context.get(torch.cuda.current_device())._stream
            out["want"] = s.cuda_stream
        except BaseException as e:  # reported on the test's thread
            out["error"] = e

    th = threading.Thread(target=body)  # a new thread: its context has made no call yet
    th.start()
    th.join()
    if "error" in out:
        raise out["error"]
    assert out["stream"] == out["want"]
