"""CPU: the lock-free union-find of the duplicate clusters (csrc/unionfind.h, the code the kernels of clusters.hip run) as
host code: tests/native/unionfind_host_check.cpp applies chains, stars, a dense clique, duplicate edges, self-pairs and random
edges from 8 threads at once, under AddressSanitizer + UBSan, and compares every vertex's root with a sequential union-find
(`make unionfind_check`).  A loop that would never end on the device ends here at its trip limit, as an error."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "revers-o_amd", "csrc")


def test_concurrent_unions_equal_a_sequential_union_find():
    subprocess.run(["make", "-C", CSRC, "unionfind_check"], check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "asan", "unionfind_host_check")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "FAILED" not in r.stdout
    for case in ("chain ascending", "chain permuted", "stars", "clique + duplicates + self", "random sparse", "two vertices"):
        assert case in r.stdout
