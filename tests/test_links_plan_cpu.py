"""The host-only part of the links calls (spaghettisearch_amd/csrc/links_plan.hpp: option ranges and the sizes of the temporaries) on
its own, without a GPU: tests/links_plan_harness.cpp is compiled with the host C++ compiler, no device header on the include path,
and AddressSanitizer + UBSan (a stand-alone program: the only place a sanitizer build belongs).  The harness checks the properties
the kernels rely on; the figures are compared with the same arithmetic in Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")

CASES = [  # n_rows, m, max_degree, wave_max, chunk
    (1, 1, 0, 1024, 1024), (4, 5, 7, 128, 64), (51200, 5, 200000, 1024, 1024), (51200, 64, 200000, 128, 64), (10, 64, 129, 128, 64),
    (10, 64, 128, 128, 64), (3, 5, 5000, 1, 1), (3, 5, 5000, 1 << 40, -5), (3, 5, 100, 64, 4096), ((1 << 31) - 1, 1, (1 << 32) - 1, 32, 32),
    (33554431, 64, (1 << 32) - 1, 32, 32), (1 << 40, 64, (1 << 32) - 1, 32, 32),
]


def model(n_rows, m, max_degree, wave_max, chunk):
    clamp = lambda v: min(max(v, 32), 4096)                               # noqa: E731
    w, c = clamp(wave_max), clamp(chunk)
    per_row = 0 if max_degree == 0 else 1 if max_degree <= w else -(-max_degree // c)
    per_row = max(per_row, 1)
    too_large = n_rows > 0 and per_row * m > (1 << 60) // n_rows
    return [w, c, max(w, c), per_row, 0 if too_large else n_rows * per_row, int(too_large)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("links_plan") / "links_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "links_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def test_plan_harness(harness):
    text = "".join(" ".join(str(x) for x in case) + "\n" for case in CASES)
    r = subprocess.run([harness], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == f"ok {len(CASES)} lines"
    for case, line in zip(CASES, lines):
        assert [int(x) for x in line.split()] == model(*case), case
    assert model(*CASES[-1])[-1] == 1                                      # (more rows than the ABI admits: the one case that cannot be held)
