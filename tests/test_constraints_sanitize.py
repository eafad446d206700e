"""ASan/UBSan on the host constraint-aware flat extraction (csrc/constraints.cpp,
constrained_flat_labels_host): the stand-alone driver tests/sanitize/host_constraints.cpp (its
own main: the hand-worked vector bit for bit, 300 seeded random trees against a linear-walk
restatement, the error paths) is compiled together with csrc/constraints.cpp and csrc/flat.cpp
(the trees) for the host only, with the flags of test_cluster_tree_sanitize.py, and run.  A
sanitizer report or a mismatch makes it exit non-zero.  No GPU, nothing loaded into python,
nothing preloaded."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "232-hierarchical-density-based-clustering-using-mapreduce_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]


def test_host_constraints_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "host_constraints")
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "--cuda-host-only", "-x", "hip", *SAN,
           f"-I{CSRC}", "-o", exe, os.path.join(HERE, "sanitize", "host_constraints.cpp"),
           os.path.join(CSRC, "constraints.cpp"), os.path.join(CSRC, "flat.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "host constraints ok" in r.stdout, r.stdout + r.stderr[-4000:]
