"""The engine's VMR_* environment switches: read in one place (read_opts, once per handle), each one documented in the
INTEGRATION.md table.  Reads the sources only; no GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vimure_amd", "csrc")


def _sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert paths
    return {os.path.basename(p): open(p).read() for p in paths}


def _read_opts_body(src):
    """The text of read_opts' body, from its opening brace to the matching closing one."""
    m = re.search(r"^static void read_opts\(VmrOpts& o\) \{", src, re.M)
    assert m, "read_opts not found"
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(src[i], 0)
        i += 1
    return m.start(), i


def test_getenv_only_in_read_opts():
    srcs = _sources()
    hits = [(name, src.count("getenv(")) for name, src in srcs.items() if "getenv(" in src]
    assert [name for name, _ in hits] == ["create.hip"], hits
    src = srcs["create.hip"]
    a, b = _read_opts_body(src)
    assert "getenv(" not in src[:a] + src[b:]


def test_every_switch_has_a_row_in_the_integration_table():
    src = _sources()["create.hip"]
    a, b = _read_opts_body(src)
    names = set(re.findall(r'"(VMR_[A-Z0-9_]+)"', src[a:b]))
    assert len(names) >= 20, names
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rows = set()
    for line in doc.splitlines():
        if line.startswith("| `VMR_"):
            rows.update(re.findall(r"`(VMR_[A-Z0-9_]+)`", line.split("|")[1]))
    assert names <= rows, sorted(names - rows)
