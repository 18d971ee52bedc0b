"""No GPU: the case table of the direct conv edge tests (tests/conv_cases.py) against the host side of csrc/conv.hip, csrc/conv_small.hip
and csrc/conv_bf16.hip.  tests/wgrad_launch_recorder.cpp links the release library, answers the HIP runtime calls itself and prints, per
row, the return code and every launch; here: a row launches exactly the instantiations it claims, in order; an error row returns its code
and launches nothing; every instantiation of these kernel families in the library's symbol table is named by a row (or listed as
unreachable with a reason); df_conv_s2_dgrad_form answers what the row says; the packed-size queries follow the header's rule."""
import ctypes
import os
import re
import subprocess

import pytest

import conv_cases as cc
from deep_fluids_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")      # as deep_fluids_amd/csrc/Makefile
IDS = [r["id"] for r in cc.ROWS]


def present(r):
    """bit mask over cc.SLOTS of the operands the call passes (the others are NULL)"""
    fl, e = r["flags"], r["entry"]
    have = {"x": True, "wp": True, "y": True, "bias": bool(fl & cc.BIAS) and "dgrad" not in e,
            "residual": bool(fl & cc.RESIDUAL) and e in ("fwd", "fwd_bf16x3"), "mask_src": bool(fl & cc.MASK) and e in ("fwd", "fwd_bf16x3")}
    return sum(1 << i for i, s in enumerate(cc.SLOTS) if have[s] and s not in r["null"])


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    """{row id: (return code, [kernel name without blanks, ...] in launch order)} of one recorder run over the table"""
    tmp = tmp_path_factory.mktemp("conv_launches")
    exe, syms, rows = str(tmp / "recorder"), str(tmp / "symbols.txt"), str(tmp / "rows.txt")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-I", os.path.join(os.path.dirname(HERE), "include"),
                           os.path.join(HERE, "wgrad_launch_recorder.cpp"), "-x", "none", "-o", exe, "-rdynamic", _lib.LIB_PATH, "-ldl",
                           "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH)])
    with open(syms, "w") as f:
        for line in subprocess.check_output(["nm", "-C", "--defined-only", _lib.LIB_PATH]).decode().splitlines():
            parts = line.split(" ", 2)
            if len(parts) == 3:
                f.write("%s %s\n" % (parts[0], parts[2]))
    with open(rows, "w") as f:
        for r in cc.ROWS:
            f.write("%s dc_%s %d %d %d %d %d %d %d %d %d %s\n" % ((r["id"], r["entry"]) + r["shape"] + (r["cin"], r["cout"], r["kz"], r["flags"], present(r),
                                                                                                     " ".join(str(r["off"][s]) for s in cc.SLOTS))))
    got, cur = {}, None
    for line in subprocess.check_output([exe, syms, rows]).decode().splitlines():
        w = line.split()
        if w[0] == "row":
            cur = []
        elif w[0] == "launch":
            m = re.match(r"\s+launch (.*) grid (\d+) (\d+) (\d+) block (\d+) lds (\d+) args ([0-9a-f.?]+)$", line)
            assert m, line
            name = m.group(1).replace("dfconv::", "").replace("(anonymous namespace)::", "")
            assert not name.startswith("?") and m.group(7) != "?", line      # a symbol of the library, with a known argument layout
            assert int(m.group(5)) == 256 and all(int(m.group(i)) >= 1 for i in (2, 3, 4)), line
            cur.append(re.sub(r"\s+", "", name.split("(")[0]))
        elif w[0] == "funcattr":
            assert int(w[-1]) > 64 * 1024 and "conv_thin_k_mfma_kernel" in line, line      # the LDS opt-in, only above the default 64 KB
        elif w[0] == "end":
            got[w[1]] = (int(w[3]), cur)
    return got


def test_table_is_consistent():
    assert len(IDS) == len(set(IDS))
    for r in cc.ROWS:
        assert r["kz"] == 3 or r["shape"][1] == 1 or isinstance(r["reaches"], int), r["id"]
        if r["twin"]:
            t = cc.by_id(r["twin"][0])
            assert all(t[k] == r[k] for k in ("entry", "shape", "cin", "cout", "kz", "mode")) and r["twin"][1] in ("bits", "tol"), r["id"]
            assert t["flags"] == r["flags"] & ~cc.VALU_ONLY and not any(t["off"].values()), r["id"]
            if r["twin"][1] == "bits":      # claimed only for the VEC = false twin of the same kernel on the same chunk length
                assert [n.replace("false", "true", 1) for n in r["names"]] == t["names"] and r["names"] != t["names"], r["id"]
    for rid in cc.NARROWED + cc.TINY_BATCH:
        assert cc.by_id(rid)["shape"][0] > 1
    assert len(cc.NARROWED) >= 30


@pytest.mark.parametrize("rid", IDS)
def test_row_launches_what_it_claims(record, rid):
    r = cc.by_id(rid)
    rc, launches = record[rid]
    if isinstance(r["reaches"], int):
        assert rc == r["reaches"] and launches == [], (rid, rc, launches)
    else:
        assert rc == 0 and launches == r["names"], (rid, rc, launches, r["names"])


def test_every_instantiation_has_a_row():
    out = subprocess.check_output(["nm", "-C", _lib.LIB_PATH]).decode()
    have = set()
    for fam in cc.FAMILIES:
        if fam.endswith("("):      # not a template: one kernel
            have |= set(re.findall(r"::(%s)\(" % re.escape(fam[:-1]), out))
        else:
            have |= set(re.sub(r"\s+", "", m) for m in re.findall(r"::(%s[^>]*>)" % re.escape(fam), out))
    named = set(n for r in cc.OK_ROWS for n in r["names"]) | set(cc.PACKS[r["entry"]] for r in cc.OK_ROWS)
    assert len(have) > 180, len(have)      # the patterns still find the kernels
    assert not (set(cc.UNREACHABLE) & named), "a row reaches an instantiation listed as unreachable"
    assert not (set(cc.UNREACHABLE) - have), "UNREACHABLE names an instantiation the library no longer holds"
    named |= set(cc.UNREACHABLE)
    assert have - named == set(), "instantiations without a row in tests/conv_cases.py: %s" % sorted(have - named)
    assert named - have == set(), "rows that name a kernel the library does not hold: %s" % sorted(named - have)


S2DG = [r["id"] for r in cc.OK_ROWS if r["entry"] == "s2_dgrad"]


@pytest.mark.parametrize("rid", S2DG)
def test_s2_dgrad_form_answers_what_the_row_claims(rid):
    r = cc.by_id(rid)
    fn = _lib.lib().df_conv_s2_dgrad_form
    got = fn(ctypes.c_void_p((1 << 44) + 4 * r["off"]["x"]), r["cin"], r["cout"])      # host-only: the pointer is looked at, never followed
    assert got == r["form"] and (got == 1) == (r["reaches"] == ("s2d",)), (rid, got)


def packed_query(r):
    """(query name, its arguments, taps (x classes), K, N, K chunk) of the row's packed operand"""
    e, kz, cin, cout = r["entry"], r["kz"], r["cin"], r["cout"]
    bf = "_bf16x3" if e.endswith("bf16x3") else ""
    if e in ("fwd", "fwd_bf16x3"):      # mode 1: the layer's weights are [taps, Cout, Cin] of this call, so K = its cout = this Cin either way
        w_cin, w_cout = (cin, cout) if r["mode"] == 0 else (cout, cin)
        return "df_conv_packed_elems" + bf, (9 * kz, w_cin, w_cout, r["mode"]), 9 * kz, cin, cout, 32 if bf else 16
    if e == "s2_fwd":
        return "df_conv_packed_elems", (9 * kz, cin, cout, 0), 9 * kz, cin, cout, 16
    nct = 64 if kz == 3 else 16
    if e.startswith("up_fwd"):
        return "df_upconv_packed_elems" + bf, (cin, cout, kz, 0), nct, cin, cout, 32 if bf else 16
    return "df_upconv_packed_elems" + bf, (cin, cout, kz, 2 if e == "s2_dgrad" else 1), nct, cout, cin, 32 if bf else 16


@pytest.mark.parametrize("rid", [r["id"] for r in cc.OK_ROWS])
def test_packed_size_query_follows_the_header_rule(rid):
    """taps x K rounded up to the chunk (16; bf16x3: 32) x N rounded up to its N tile (32 up to 32, 64 up to 64, else 128)"""
    name, args, taps, K, N, ck = packed_query(cc.by_id(rid))
    got = _lib.query(name, *args)
    nt = 128 if N > 64 else 64 if N > 32 else 32
    assert got > 0 and got % 4 == 0 and got == taps * (-(-K // ck) * ck) * (-(-N // nt) * nt), (rid, name, args, got)
