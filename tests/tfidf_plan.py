"""Builds and runs tests/tfidf_plan_harness.cpp: spaghettisearch_amd/csrc/tfidf_plan.hpp compiled alone with the host C++ compiler, no
device header on the include path, and AddressSanitizer + UBSan (a stand-alone program: the only place a sanitizer build belongs).
Shared by tests/test_tfidf_plan_cpu.py and tests/test_tfidf_cases_cpu.py."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spaghettisearch_amd", "csrc")
FIELDS = ("bucketed", "shift", "shift_forced", "nb", "per", "nblk", "head_thr", "bpt", "nbt", "bpt_inst", "scatter_lds_bytes",
          "bucket_lds_bytes", "too_many_buckets")
OPTIONS = ("tfidf.blocks", "tfidf.bucket_shift", "tfidf.head_min_run", "tfidf.bucket_min")      # in the order of an input line


def build(out_dir):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(out_dir), "tfidf_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "tfidf_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def run(exe, inputs=()):
    """inputs: (n_docs, n_post, blocks, bucket_shift, head_min_run, bucket_min) each
    -> (constants: dict, default options: dict, plans: one dict of FIELDS per input).  The harness checks its invariants on every line."""
    text = "".join("%d %d %d %d %d %d\n" % tuple(x) for x in inputs)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    head, dflt = lines[0].split(), lines[1].split()
    assert head[0] == "const" and dflt[0] == "default" and lines[-1] == f"ok {len(inputs)}", (lines[:2], lines[-1:])
    consts = {k: int(v) for k, v in zip(head[1::2], head[2::2])}
    defaults = {"tfidf." + k: int(v) for k, v in zip(dflt[1::2], dflt[2::2])}
    plans = [dict(zip(FIELDS, map(int, ln.split()))) for ln in lines[2:-1]]
    assert len(plans) == len(inputs) and all(len(p) == len(FIELDS) for p in plans)
    return consts, defaults, plans
