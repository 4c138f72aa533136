"""The term lexicon's host-only part (spaghettisearch_amd/csrc/lexicon_plan.hpp) on its own, without a GPU: tests/lexicon_plan_harness.cpp
is compiled with the host C++ compiler, no device header on the include path, and AddressSanitizer + UBSan (a stand-alone program: the
only place a sanitizer build belongs).  The harness checks the pointer validation, the sort order, the grouped layout and the chunk
ranges itself; its order is compared with the Python model here."""
import os
import shutil
import subprocess

import pytest

from tests import lexicon_model as lm
from tests.test_lexicon_cpu import random_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("lexicon_plan") / "lexicon_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "lexicon_plan_harness.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("words", [[], [b""], [b"solo"], [b"same"] * 9,
                                   random_words(600, seed=31) + [b"x" * 64, b"x" * 65, b"\xff" * 3, b"\x00", b"\x00\x00", b"ab\x80", b"ab\x7f"]],
                         ids=["none", "one-empty", "one", "all-equal", "random"])
def test_plan_harness(harness, words):
    text = "".join(w.hex() + "\n" for w in words)
    r = subprocess.run([harness], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == f"ok {len(words)} words"
    assert [int(x) for x in lines[0].split()[1:]] == lm.order(words).tolist()
    starts = [int(x) for x in lines[1].split()[1:]]
    assert starts == [sum(len(w) < L for w in words if len(w) <= 64) for L in range(65)] + [sum(len(w) <= 64 for w in words)]
