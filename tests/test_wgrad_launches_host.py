"""No GPU: what every row of tests/wgrad_cases.py really launches.  tests/wgrad_launch_recorder.cpp links the release library, defines the
HIP runtime calls of the weight-gradient host path itself (so nothing reaches a device) and prints, per row, the return code and every
launch -- kernel name, grid, block, LDS bytes, argument bytes.  Here: the main kernels of a row are exactly its "reaches" column, in
order, and a row that must refuse its pointers returns DF_EALIGN and launches nothing."""
import os
import re
import subprocess

import pytest

import wgrad_cases as wc
from deep_fluids_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")      # as deep_fluids_amd/csrc/Makefile
EALIGN = -3
HELPERS = re.compile(r"^(?:df::zero_words_kernel|pad_rows_kernel|wgrad_\w*reduce_kernel)\(")


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    """{row id: (return code, [kernel name without blanks, ...] in launch order)} of one recorder run over ALL_ROWS"""
    tmp = tmp_path_factory.mktemp("wgrad_launches")
    exe, syms, rows = str(tmp / "recorder"), str(tmp / "symbols.txt"), str(tmp / "rows.txt")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-I", os.path.join(os.path.dirname(HERE), "include"),
                           os.path.join(HERE, "wgrad_launch_recorder.cpp"), "-x", "none", "-o", exe, "-rdynamic", _lib.LIB_PATH, "-ldl",
                           "-Wl,-rpath," + libdir])
    with open(syms, "w") as f:
        for line in subprocess.check_output(["nm", "-C", "--defined-only", _lib.LIB_PATH]).decode().splitlines():
            parts = line.split(" ", 2)
            if len(parts) == 3:
                f.write("%s %s\n" % (parts[0], parts[2]))
    with open(rows, "w") as f:
        for r in wc.ALL_ROWS:
            rid, entry, (B, D, H, W), cin, cout, kz, algo, bias, xoff, goff = r[:10]
            f.write("%s %s %d %d %d %d %d %d %d %d %d %d %d\n" % (rid, entry, B, D, H, W, cin, cout, kz, -1 if algo is None else algo, int(bias),
                                                                  xoff, goff))
    out = subprocess.check_output([exe, syms, rows]).decode()
    print(out)
    got, cur = {}, None
    for line in out.splitlines():
        w = line.split()
        if w[0] == "row":
            cur = []
        elif w[0] == "launch":
            name = line.split(" launch ", 1)[1].split(" grid ")[0].replace("(anonymous namespace)::", "")
            assert not name.startswith("?"), line      # every launch maps to a symbol of the library
            cur.append(name)
        elif w[0] == "end":
            got[w[1]] = (int(w[3]), cur)
    return got


@pytest.mark.parametrize("row", wc.ALL_ROWS, ids=[r[0] for r in wc.ALL_ROWS])
def test_row_launches_what_it_claims(record, row):
    rc, launches = record[row[0]]
    if row[11] == "EALIGN":
        assert rc == EALIGN and launches == [], (row[0], rc, launches)
        return
    main = [re.sub(r"\s+", "", n.split("(")[0]) for n in launches if not HELPERS.match(n)]
    assert rc == 0 and main == row[11], (row[0], rc, main, row[11])
