"""Multi-GPU driver on the GPU box: 2 ranks (gloo process group, both on the
box's one MI355X -- RCCL refuses two ranks on one device) run the sharded MR-HDBSCAN* loop
(leaves by LPT, point-chunked nearest sample, local models by LPT, seq-ordered merge) and must
return exactly what one device returns: the same levels, bubble labels, merged edge list
(order included) and flat labels, on a C1-prefix (Skin, zero-weight ties) and a C3-shaped
(d = 16, recursive sampling with an explicit per-subset sample count) input.

The library's own RCCL communicator (hdb_comm_* / hdb_merge_edges, the C-ABI a Java driver
binds) is exercised at world size 1 under an nccl process group: seq-ordered placement +
stable descending sort must equal the reference merge of the canonical concatenation."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import driver_cases
from conftest import blobs, check_driver_structure, golden, load_skin

pytestmark = pytest.mark.gpu

def _c5s_case():
    """the scaled-C5 oracle fixture (tests/golden/make_c5s.py) with reference-Prim leaves"""
    G = golden("c5s")
    n, d, centers, seed = (int(x) for x in G["shape"])
    mp_, mcl, pu, sps, s2 = (int(x) for x in G["args"])
    return dict(data=lambda: blobs(n, d, centers, seed, spread=100.0), processing_units=pu,
                samples_per_subset=sps, seed=s2, exact_prim_leaves=True, minPts=mp_, minClSize=mcl, bubble_slices=1)


CASES = {
    "skin_prefix": dict(data=lambda: load_skin(12000), processing_units=1500, k=0.05),
    "c3_shaped": dict(data=lambda: blobs(24000, 16, 12, 3, spread=50.0), processing_units=3000,
                      samples_per_subset=256),
    # two well-separated blobs: level 0's one local model splits them into two leaves, so at
    # world 4 two ranks get no leaf and three no local model
    "few_leaves": dict(data=lambda: blobs(6000, 3, 2, 9), processing_units=4000, samples_per_subset=300),
    # tests/driver_cases.py: levels with several big subsets under a non-Euclidean metric (the keyed
    # generic nearest-sample scan in point chunks, the metric's local models dealt by LPT), minPts 8
    "ang5_cosine": dict(data=lambda: np.array(driver_cases.input_of("ang5")), processing_units=300, k=0.1,
                        distanceFunction="cosine"),
    "d7r_manhattan": dict(data=lambda: np.array(driver_cases.input_of("d7r")), processing_units=300, k=0.1,
                          distanceFunction="manhattan", minPts=8, minClSize=8, bubble_slices=8),
}
LAZY = {"c5s": _c5s_case}


def _case(name):
    return CASES[name] if name in CASES else LAZY[name]()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(pkg, X, case, raw=None):
    kw = {"minPts": 4, "minClSize": 4} | {k: v for k, v in case.items() if k != "data"}
    r = pkg.MRHDBSCANStar(**kw).run(X)
    if raw is not None:
        raw.append(r)
    lev = [(L["iteration"], sorted(L["leaves"].items()), sorted(L["big"].items()),
            {k: np.asarray(v).tolist() for k, v in L["labels"].items()}, L["new_keys"], L.get("model_errors"))
           for L in r["levels"]]
    return dict(edges=[x.cpu().numpy() for x in r["edges"]], labels=r["labels"].cpu().numpy(),
                n_clusters=r["n_clusters"], leaf_of=r["leaf_of"].cpu().numpy(), levels=lev, iterations=r["iterations"])


def _worker(rank, world, port, name, out_dir):
    import importlib
    import sys

    import torch
    import torch.distributed as dist

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = importlib.import_module("232-hierarchical-density-based-clustering-using-mapreduce_amd")
    case = _case(name)
    res = _run(pkg, case["data"](), case)
    np.save(os.path.join(out_dir, f"r{rank}.npy"), np.array([res], dtype=object), allow_pickle=True)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("name,world", [("skin_prefix", 2), ("c3_shaped", 2), ("c3_shaped", 3), ("few_leaves", 4),
                                        ("c5s", 3), ("c5s", 4), ("ang5_cosine", 2), ("d7r_manhattan", 2)])
def test_sharded_driver_equals_single_device(pkg, name, world, tmp_path):
    """world 3 / 4 on the scaled-C5 fixture: every rank's merged list equals the oracle's
    MR-HDBSCAN* bit for bit (reference-Prim leaves), levels and bubble labels included.  The
    other cases run the driver default, D11's 8 bubble slices: at world 2 / 3 / 4 the ranks fold
    4 / 3-2-3 / 2 slices each and merge the gathered partials (test_gpu_driver.py pins the
    one-device run to the oracle with the same slices)"""
    case = _case(name)
    raw = []
    ref = _run(pkg, case["data"](), case, raw)
    if name == "c5s":
        G = golden("c5s")
        check_driver_structure(G, raw[0])
        assert _digest(*ref["edges"]) == str(G["digest"])
    if name == "few_leaves":
        assert sum(len(L["leaves"]) for L in raw[0]["levels"]) < world  # some ranks get no leaf
    del raw
    mp.spawn(_worker, args=(world, _free_port(), name, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        got = np.load(os.path.join(tmp_path, f"r{r}.npy"), allow_pickle=True)[0]  # written by this test
        assert got["iterations"] == ref["iterations"] and got["levels"] == ref["levels"], r
        assert np.array_equal(got["leaf_of"], ref["leaf_of"])
        for a, b in zip(got["edges"], ref["edges"]):
            assert np.array_equal(a, b), r
        assert got["n_clusters"] == ref["n_clusters"] and np.array_equal(got["labels"], ref["labels"])


def _digest(va, vb, w):
    import hashlib
    h = hashlib.sha256()
    for a, t in ((va, np.int32), (vb, np.int32), (w, np.float64)):
        h.update(np.ascontiguousarray(a.astype(t)).tobytes())
    return h.hexdigest()


def _comm_worker(rank, world, port, out_dir):
    import importlib
    import sys

    import torch
    import torch.distributed as dist

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    pkg = importlib.import_module("232-hierarchical-density-based-clustering-using-mapreduce_amd")
    P = importlib.import_module("232-hierarchical-density-based-clustering-using-mapreduce_amd.parallel")
    ctx = pkg.Context.get(0)
    ctx.use_torch_stream()
    comm = P.HdbComm(ctx)
    rng = np.random.default_rng(5)
    E = 5000
    va = rng.integers(0, 10**6, E).astype(np.int32)
    vb = rng.integers(0, 10**6, E).astype(np.int32)
    w = np.round(rng.uniform(0, 4, E), 1)  # heavy ties: order matters
    seq = rng.permutation(E).astype(np.int64)
    t = lambda x: torch.from_numpy(x).cuda()
    a, b, ww = P.merge_local_msts(t(va), t(vb), t(w), seq=t(seq), comm=comm)
    a2, b2, w2 = P.merge_local_msts(t(va), t(vb), t(w), comm=comm)
    np.savez(os.path.join(out_dir, "comm.npz"), va=va, vb=vb, w=w, seq=seq, a=a.cpu().numpy(), b=b.cpu().numpy(),
             ww=ww.cpu().numpy(), a2=a2.cpu().numpy(), b2=b2.cpu().numpy(), w2=w2.cpu().numpy())
    bad = False
    try:
        P.merge_local_msts(t(va), t(vb), t(w), seq=t(np.zeros(E, np.int64)), comm=comm)
    except pkg.HdbError:
        bad = True
    assert bad, "a non-permutation seq must be rejected"
    # a rank with no local edges passes an empty seq (data_ptr() == 0): accepted
    e0 = P.merge_local_msts(t(va[:0]), t(vb[:0]), t(w[:0]), seq=t(seq[:0]), comm=comm)
    assert all(x.shape[0] == 0 for x in e0)
    comm.close()
    dist.destroy_process_group()


def test_hdb_merge_edges_rccl_world1(oracle, tmp_path):
    mp.spawn(_comm_worker, args=(1, _free_port(), str(tmp_path)), nprocs=1, join=True)
    z = np.load(os.path.join(tmp_path, "comm.npz"))
    inv = np.empty_like(z["seq"])
    inv[z["seq"]] = np.arange(z["seq"].shape[0])
    canon = [(z["va"][inv], z["vb"][inv], z["w"][inv])]
    ref = oracle.merge_edges(canon)
    assert np.array_equal(z["a"], ref[0]) and np.array_equal(z["b"], ref[1]) and np.array_equal(z["ww"], ref[2])
    ref2 = oracle.merge_edges([(z["va"], z["vb"], z["w"])])
    assert np.array_equal(z["a2"], ref2[0]) and np.array_equal(z["b2"], ref2[1]) and np.array_equal(z["w2"], ref2[2])


def test_gather_sorted_msts_merges_on_device(oracle):
    """gather_sorted_msts with HIP tensors (2 and 3 ranks on the box's one device, gloo carries
    the blocks): rank 0 merges the presorted runs with hdb_merge_sorted_runs -> the oracle's
    SortMST order of the rank-major concatenation, ragged and empty blocks included"""
    from test_distributed import _check_gather
    for world in (2, 3):
        _check_gather(oracle, world, "cuda")
