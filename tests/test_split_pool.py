"""The allocator behind the tickets and the workspace of the in-launch split finish (sige_amd/csrc/split_pool.hpp: a ring for eager
launches, a bump region for captured ones) as a host program: tests/split_pool_check.cpp, built with the address and
undefined-behaviour sanitizers and run as a child process.  (CPU only; the header makes no HIP call.)"""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for cand in (os.environ.get("CXX"), "/opt/rocm/llvm/bin/clang++", "g++", "clang++"):
        path = cand and shutil.which(cand)
        if path:
            return path
    raise AssertionError("no host C++ compiler")


def test_ring_and_graph_region_bookkeeping(tmp_path):
    exe = str(tmp_path / "split_pool_check")
    cmd = [_host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(REPO, "sige_amd", "csrc"), os.path.join(REPO, "tests", "split_pool_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "split_pool ok", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
