"""The host-only part of the calls that take a window of result rows (spaghettisearch_amd/csrc/hit_window_plan.hpp: the paging check,
the overlap test of hits and hits_out, the search for a host count outside the window, and copy_written, which brings back exactly the
entries a kernel wrote) on its own, without a GPU: tests/hit_window_plan_harness.cpp is compiled with the host C++ compiler, no device
header on the include path, and AddressSanitizer + UBSan (a stand-alone program: the only place a sanitizer build belongs).  The
harness checks every property itself; this file builds and runs it."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("hit_window_plan") / "hit_window_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "hit_window_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def test_plan_harness(harness):
    r = subprocess.run([harness], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    # 4 element sizes x 3 inner widths x (whole entries, per-query widths)
    assert lines[:4] == ["ok paging", "ok overlap", "ok bad_count", "ok copy_written 24"], r.stdout
    with open(os.path.join(ROOT, "include", "spaghetti_rank.h")) as f:
        max_topk = int(re.search(r"#define SS_MAX_TOPK (\d+)", f.read()).group(1))
    assert lines[4] == f"max_topk {max_topk}"                             # (the harness checks the edges of the ABI's limit)


def test_plan_header_is_host_only():
    with open(os.path.join(CSRC, "hit_window_plan.hpp")) as f:
        text = f.read()
    assert "#include <hip" not in text and "#include \"" not in text
