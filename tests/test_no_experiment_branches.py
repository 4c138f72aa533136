"""The product kernels carry no wrong-results experiment branches: no preprocessor conditional under csrc names an
`_EXP_` macro or one of the retired A/B switches, and the Makefile defines none.  Plain text matching on macro names."""
import pathlib
import re

CSRC = pathlib.Path(__file__).resolve().parent.parent / "spaghettisearch_amd" / "csrc"
RETIRED = ("SS_SC_NO_NT", "SS_SC_W_PLAIN_STORE", "SS_PR_NO_NT", "SS_UNCACHED_STREAMS")
CONDITIONAL = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif)\b(.*)$")


def _logical_lines(text):
    """(first line number, line) with backslash continuations joined"""
    out, buf, start = [], "", 0
    for no, line in enumerate(text.splitlines(), 1):
        if not buf:
            start = no
        if line.endswith("\\"):
            buf += line[:-1] + " "
            continue
        out.append((start, buf + line))
        buf = ""
    if buf:
        out.append((start, buf))
    return out


def test_no_experiment_macro_in_a_preprocessor_conditional():
    sources = sorted(list(CSRC.glob("*.hip")) + list(CSRC.glob("*.hpp")))
    assert len(sources) >= 10, sources          # the glob found the kernel files
    bad = []
    for path in sources:
        for no, line in _logical_lines(path.read_text()):
            m = CONDITIONAL.match(line)
            if not m:
                continue
            for name in re.findall(r"[A-Za-z_]\w*", m.group(2)):
                if "_EXP_" in name or name in RETIRED:
                    bad.append(f"{path.name}:{no}: {name}")
    assert not bad, bad


def test_retired_switches_are_not_mentioned_at_all():
    # they selected code, so any remaining mention (a #define, a comment) would be stale
    bad = [f"{path.name}: {name}" for path in sorted(CSRC.iterdir()) if path.suffix in (".hip", ".hpp")
           for name in RETIRED if name in path.read_text()]
    assert not bad, bad


def test_makefile_defines_no_experiment_macro():
    text = (CSRC / "Makefile").read_text().replace("\\\n", " ")
    flags = [line for line in text.splitlines() if re.match(r"^\s*CXXFLAGS\s*[+:?]?=", line)]
    assert flags, "no CXXFLAGS line found"
    bad = [d for line in flags for d in re.findall(r"-D\s*(SS\w*_EXP\w*)", line)]
    assert not bad, bad
