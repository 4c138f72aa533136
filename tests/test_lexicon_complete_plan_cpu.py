"""The completions' plan arithmetic (spaghettisearch_amd/csrc/lexicon_plan.hpp: complete_parts, complete_part) on its own, without a
GPU: tests/lexicon_complete_plan_harness.cpp is compiled with the host C++ compiler, no device header on the include path, and
AddressSanitizer + UBSan (a stand-alone program: the only place a sanitizer build belongs), and run directly.  The harness checks that
the parts of a range tile it exactly once and in order for lengths 0, 1, P - 1, P, P + 1 and 2^32 - 1 at P = 1, 2, 7, 256, and that P
stays within 1 .. 256 for 1, 1024 and 2^20 prefixes."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")


def test_complete_plan_harness(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "lexicon_complete_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "lexicon_complete_plan_harness.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines()[-1].startswith("ok ")
