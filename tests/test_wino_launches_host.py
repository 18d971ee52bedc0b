"""No GPU: what the seven df_wino_* entry points and df_wino43_conv accept, reject and launch.  tests/wgrad_launch_recorder.cpp links the
release library, defines the HIP runtime calls itself and prints every launch; the expected values -- return code, instantiation, grid,
block, LDS bytes, argument bytes -- are tests/golden/wino_launches.json, recorded with this recorder from the last commit whose
conv_wino.hip still held one argument fill per entry point (2f63d5b); the cout-slices rows, which the parent of their commit answered with
an empty grid, from the commit that added the limit.  `python tests/test_wino_launches_host.py <library> <json>`
records such a file from any build of the library."""
import json
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")      # as deep_fluids_amd/csrc/Makefile
GOLDEN = os.path.join(HERE, "golden", "wino_launches.json")
X, WP, BIAS, RES, MSRC, MBITS, Y, Y2, SBITS = (1 << i for i in range(9))      # operand slots of the recorder
SLOT_NAMES = dict(zip((X, WP, BIAS, RES, MSRC, MBITS, Y, Y2, SBITS), "x wp bias res msrc mbits y y2 sbits".split()))
LRELU, RESIDUAL, MASK, FBIAS, ADDUP = 1, 2, 4, 8, 16                            # DF_CONV_*

# Per entry point: the flags and operands of a call it accepts; the operands whose 16-byte alignment it checks and those it does not;
# whether its extents are the COARSE ones (the kernel runs on twice each); the form of its 2 GiB bound.
ENTRIES = {
    "wino_fwd": dict(flags=9, ops=X | WP | BIAS | Y, need=X | WP | Y, aligned=X | WP | Y, loose=BIAS | RES | MSRC),
    "wino_fwd_bits": dict(flags=9, ops=X | WP | BIAS | Y | SBITS, need=X | WP | Y, aligned=X | WP | Y | SBITS | MBITS, loose=BIAS),
    "wino_fwd_addup": dict(flags=0, ops=X | WP | BIAS | RES | Y | Y2, need=X | WP | BIAS | RES | Y | Y2, aligned=X | WP, loose=BIAS | RES | Y | Y2,
                           even=True),
    "wino_fwd_addup_bits": dict(flags=0, ops=X | WP | BIAS | RES | Y2 | SBITS, need=X | WP | BIAS | RES | Y2 | SBITS, aligned=X | WP | SBITS,
                                loose=BIAS | RES | Y2, even=True),
    "wino_upconv_fwd": dict(flags=9, ops=X | WP | BIAS | Y, need=X | WP | BIAS | Y, aligned=X | WP | Y, loose=BIAS, vol="upfwd"),
    "wino_upconv_fwd_bits": dict(flags=0, ops=X | WP | BIAS | Y | SBITS, need=X | WP | BIAS | Y | SBITS, aligned=X | WP | Y | SBITS, loose=BIAS,
                                 vol="upfwd"),
    "wino_upconv_dgrad": dict(flags=0, ops=X | WP | Y, need=X | WP | Y, aligned=X | WP, loose=Y, vol="updgrad"),
    "wino43": dict(flags=9, ops=X | WP | BIAS | Y, need=X | WP | Y, aligned=X | WP | Y | Y2 | MBITS | SBITS, loose=BIAS | RES | MSRC),
}


def _rows():
    rows = []

    def add(rid, entry, dims, cin, cout, flags=None, ops=None, mis=0):
        e = ENTRIES[entry]
        rows.append((entry + "-" + rid, entry, dims, cin, cout, e["flags"] if flags is None else flags, e["ops"] if ops is None else ops, mis))

    small = (2, 6, 10, 12)      # even extents, ragged tile blocks (4 x 8 x 8 outputs each)
    # ---- every instantiation by name, and the run-time-flags fallback of df_wino_conv_fwd ----
    add("fl0", "wino_fwd", small, 32, 64, 0, X | WP | Y)
    add("fl2", "wino_fwd", small, 32, 64, RESIDUAL, X | WP | RES | Y)
    add("fl4", "wino_fwd", small, 32, 64, MASK, X | WP | MSRC | Y)
    add("fl9", "wino_fwd", small, 32, 64)
    add("fallback-bias", "wino_fwd", small, 32, 64, FBIAS)
    add("fallback-all", "wino_fwd", small, 32, 64, 15, X | WP | BIAS | RES | MSRC | Y)
    add("fl73", "wino_fwd_bits", small, 32, 64)
    add("fl132", "wino_fwd_bits", small, 32, 64, MASK, X | WP | MBITS | Y)
    add("fl25", "wino_fwd_addup", small, 32, 64)
    add("fl345", "wino_fwd_addup_bits", small, 32, 64)
    add("fl9m3", "wino_upconv_fwd", small, 32, 64)
    add("fl73m3", "wino_upconv_fwd_bits", small, 32, 64)
    add("fl0m2", "wino_upconv_dgrad", small, 32, 64)
    add("fl0m2-swap", "wino_upconv_dgrad", small, 96, 32)      # the kernel's Cin is the entry point's Cout
    add("fl9", "wino43", small, 32, 64)
    add("fl73", "wino43", small, 32, 64, 9, X | WP | BIAS | Y | SBITS)
    add("fl132", "wino43", small, 32, 64, MASK, X | WP | MBITS | Y)
    add("fl4", "wino43", small, 32, 64, MASK, X | WP | MSRC | Y)
    add("fl2", "wino43", small, 32, 64, RESIDUAL, X | WP | RES | Y)
    add("fl0", "wino43", small, 32, 64, 0, X | WP | Y)
    add("fl25", "wino43", small, 32, 64, 25, X | WP | BIAS | RES | Y | Y2)
    add("fl345", "wino43", small, 32, 64, 25, X | WP | BIAS | RES | Y2 | SBITS)
    add("fallback-bias", "wino43", small, 32, 64, FBIAS)
    add("fallback-all", "wino43", small, 32, 64, 15, X | WP | BIAS | RES | MSRC | Y)
    # ---- flags without their operands, operands without their flags ----
    add("bias-without", "wino_fwd", small, 32, 64, 9, X | WP | Y)
    add("residual-without", "wino_fwd", small, 32, 64, RESIDUAL, X | WP | Y)
    add("mask-without", "wino_fwd", small, 32, 64, MASK, X | WP | Y)
    add("addup-flag", "wino_fwd", small, 32, 64, 25, X | WP | BIAS | RES | Y)
    add("fwd-without-bits", "wino_fwd_bits", small, 32, 64, 9, X | WP | BIAS | Y)
    add("fwd-without-bias", "wino_fwd_bits", small, 32, 64, 9, X | WP | Y | SBITS)
    add("fwd-with-mask-bits", "wino_fwd_bits", small, 32, 64, 9, X | WP | BIAS | MBITS | Y | SBITS)
    add("mask-without-bits", "wino_fwd_bits", small, 32, 64, MASK, X | WP | Y)
    add("mask-with-sign-bits", "wino_fwd_bits", small, 32, 64, MASK, X | WP | MBITS | Y | SBITS)
    add("other-flags", "wino_fwd_bits", small, 32, 64, FBIAS)
    for fl in (0, LRELU, FBIAS, 11, 25):
        add("badflags%d" % fl, "wino_upconv_fwd", small, 32, 64, fl)
    add("unknown-flag", "wino43", small, 32, 64, 9 | 32)
    add("bias-without", "wino43", small, 32, 64, 9, X | WP | Y)
    add("residual-without", "wino43", small, 32, 64, RESIDUAL, X | WP | Y)
    add("addup-without-coarse", "wino43", small, 32, 64, 25, X | WP | BIAS | Y | Y2)
    add("residual-and-addup", "wino43", small, 32, 64, 27, X | WP | BIAS | RES | Y | Y2)
    add("addup-without-y2", "wino43", small, 32, 64, 25, X | WP | BIAS | RES | Y)
    add("mask-without", "wino43", small, 32, 64, MASK, X | WP | Y)
    add("mask-both", "wino43", small, 32, 64, MASK, X | WP | MSRC | MBITS | Y)
    add("no-y-no-addup", "wino43", small, 32, 64, 9, X | WP | BIAS | Y2 | SBITS)
    add("no-y-no-bits", "wino43", small, 32, 64, 25, X | WP | BIAS | RES | Y2)
    add("fallback-with-bits", "wino43", small, 32, 64, FBIAS, X | WP | BIAS | Y | SBITS)
    add("addup-odd-d", "wino43", (2, 7, 10, 12), 32, 64, 25, X | WP | BIAS | RES | Y | Y2)
    # ---- misaligned operands that the accepted call of the loop below does not have ----
    add("misaligned-res", "wino_fwd", small, 32, 64, RESIDUAL, X | WP | RES | Y, RES)
    add("misaligned-msrc", "wino_fwd", small, 32, 64, MASK, X | WP | MSRC | Y, MSRC)
    add("misaligned-mbits", "wino_fwd_bits", small, 32, 64, MASK, X | WP | MBITS | Y, MBITS)
    add("misaligned-res", "wino43", small, 32, 64, RESIDUAL, X | WP | RES | Y, RES)
    add("misaligned-msrc", "wino43", small, 32, 64, MASK, X | WP | MSRC | Y, MSRC)
    add("misaligned-mbits", "wino43", small, 32, 64, MASK, X | WP | MBITS | Y, MBITS)
    add("misaligned-sbits", "wino43", small, 32, 64, 9, X | WP | BIAS | Y | SBITS, SBITS)
    add("misaligned-y2", "wino43", small, 32, 64, 25, X | WP | BIAS | RES | Y | Y2, Y2)
    add("misaligned-coarse", "wino43", small, 32, 64, 25, X | WP | BIAS | RES | Y | Y2, RES)
    for entry, e in ENTRIES.items():
        up = "vol" in e
        # ---- null operands, one at a time; extents; channel counts ----
        for s, n in SLOT_NAMES.items():
            if e["need"] & s:
                add("null-" + n, entry, small, 32, 64, ops=e["ops"] & ~s)
        for i in range(4):
            add("zero-extent%d" % i, entry, tuple(0 if j == i else v for j, v in enumerate(small)), 32, 64)
        add("negative-extent", entry, (2, 6, -10, 12), 32, 64)
        for cin, cout in ((48, 64), (32, 80), (0, 64), (32, 0), (-32, 64)):
            add("channels-%d-%d" % (cin, cout), entry, small, cin, cout)
        for i in (1, 2, 3):      # odd extents: refused by the add-up forms only
            add("odd-extent%d" % i, entry, tuple(v + 1 if j == i else v for j, v in enumerate(small)), 32, 64)
        # ---- one misaligned operand at a time ----
        for s, n in SLOT_NAMES.items():
            if e["ops"] & s:
                add("misaligned-" + n, entry, small, 32, 64, mis=s)
        # ---- the 2 GiB bound of one batch volume in this entry point's own form, at the limit and one step over it ----
        if e.get("vol") == "upfwd":
            vols = (("out", (1, 128, 128, 128), 32, 32), ("in", (1, 64, 128, 128), 512, 32))      # 8 v Cout = 2^29 | v Cin = 2^29
        elif up:
            vols = (("in", (1, 128, 128, 128), 32, 32), ("out", (1, 128, 128, 64), 32, 64))       # 8 v max(Cin, Cout) = 2^29
        else:
            vols = (("in", (1, 256, 256, 128), 64, 32), ("out", (1, 256, 256, 256), 32, 32))      # D H W max(Cin, Cout) = 2^29
        for n, dims, cin, cout in vols:
            add("volume-%s-at" % n, entry, dims, cin, cout)
            add("volume-%s-over" % n, entry, dims[:3] + (dims[3] + 2,), cin, cout)
        cc = 2048 if entry == "wino43" else 4096      # Cin Cout <= 2^22 | 2^24
        add("cincout-at", entry, small, cc, cc)
        add("cincout-over", entry, small, cc, cc + 32)
        # ---- at most 256 cout slices: beyond them the persistent grid would be empty (the dgrad's slices are the entry point's Cin) ----
        dg = entry == "wino_upconv_dgrad"
        add("cout-slices-at", entry, small, 8192 if dg else 32, 32 if dg else 8192)
        add("cout-slices-over", entry, small, 8224 if dg else 32, 32 if dg else 8224)
        # ---- tile blocks x cout slices < 2^31 ----
        add("workgroups-at", entry, ((1 << 31) - 1, 2 if up else 4, 4, 4), 32, 32)      # one tile block per batch entry, one slice
        add("workgroups-over", entry, (1 << 31, 2 if up else 4, 4, 4), 32, 32)
    # ---- grids: cout slices x (few | ragged | saturating) tile blocks ----
    for ncs in (1, 2, 3, 4, 8, 16):
        for n, dims in (("1", (1, 4, 8, 8)), ("3", (3, 4, 8, 8)), ("12", (1, 5, 9, 17)), ("37", (37, 3, 8, 8)), ("100", (25, 4, 16, 16)),
                        ("257", (257, 4, 8, 8)), ("512", (4, 16, 32, 32))):
            add("grid-ncs%d-ntb%s" % (ncs, n), "wino_fwd", dims, 32, 32 * ncs)
            add("grid-ncs%d-ntb%s" % (ncs, n), "wino43", dims, 32, 32 * ncs)
        add("grid-ncs%d" % ncs, "wino_upconv_dgrad", (3, 2, 4, 4), 32 * ncs, 64)
        add("grid-ncs%d" % ncs, "wino_upconv_fwd_bits", (3, 2, 4, 4), 32, 32 * ncs)
    assert len({r[0] for r in rows}) == len(rows)
    return rows


ROWS = _rows()


def _instantiation(name):
    """(family, FL, MODE) of a kernel symbol, whether or not it still carries the experiment template arguments <DBG, FL, MODE, PREC, XS>
    (3-D F(2,3)^3) / <FL, DBG> (F(2,2,4)), which then must all be 0"""
    m = re.search(r"(wino3d|wino43)_kernel<([-0-9, ]+)>", name)
    assert m, name
    v = [int(t) for t in m.group(2).split(",")]
    if m.group(1) == "wino43":
        assert len(v) == 1 or (len(v) == 2 and v[1] == 0), name
        return ["wino43", v[0], 0]
    if len(v) == 5:
        assert v[0] == 0 and v[3] == 0 and v[4] == 0, name
        v = v[1:3]
    assert len(v) == 2, name
    return ["wino3d", v[0], v[1]]


def run_recorder(lib_path, tmp):
    """{row id: {"rc": return code, "launches": [{"kernel": [family, FL, MODE], "grid", "block", "lds", "args"}, ...]}} of the ROWS"""
    exe, syms, rows = os.path.join(tmp, "recorder"), os.path.join(tmp, "symbols.txt"), os.path.join(tmp, "rows.txt")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-I", os.path.join(os.path.dirname(HERE), "include"),
                           os.path.join(HERE, "wgrad_launch_recorder.cpp"), "-x", "none", "-o", exe, "-rdynamic", lib_path, "-ldl",
                           "-Wl,-rpath," + os.path.dirname(lib_path)])
    with open(syms, "w") as f:
        for line in subprocess.check_output(["nm", "-C", "--defined-only", lib_path]).decode().splitlines():
            parts = line.split(" ", 2)
            if len(parts) == 3:
                f.write("%s %s\n" % (parts[0], parts[2]))
    with open(rows, "w") as f:
        for rid, entry, dims, cin, cout, flags, ops, mis in ROWS:
            f.write("%s %s %d %d %d %d %d %d %d %d %d\n" % ((rid, entry) + tuple(dims) + (cin, cout, flags, ops, mis)))
    got, cur = {}, None
    for line in subprocess.check_output([exe, syms, rows]).decode().splitlines():
        w = line.split()
        if w[0] == "row":
            cur = []
        elif w[0] == "launch":
            m = re.match(r"\s+launch (.*) grid (\d+) (\d+) (\d+) block (\d+) lds (\d+) args (\w+)$", line)
            assert m, line
            cur.append({"kernel": _instantiation(m.group(1)), "grid": [int(m.group(i)) for i in (2, 3, 4)], "block": int(m.group(5)),
                        "lds": int(m.group(6)), "args": m.group(7)})
        elif w[0] == "end":
            got[w[1]] = {"rc": int(w[3]), "launches": cur}
    return got


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    from deep_fluids_amd import _lib
    return run_recorder(_lib.LIB_PATH, str(tmp_path_factory.mktemp("wino_launches")))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("rid", [r[0] for r in ROWS])
def test_call_returns_and_launches_what_the_fixture_holds(record, golden, rid):
    print(record[rid])
    assert record[rid] == golden[rid], (rid, record[rid], golden[rid])


def test_fixture_holds_exactly_the_table_and_reaches_every_instantiation(golden):
    assert sorted(golden) == sorted(r[0] for r in ROWS)
    reached = {tuple(l["kernel"]) for g in golden.values() for l in g["launches"]}
    want = {("wino3d", f, 0) for f in (-1, 0, 2, 4, 9, 25, 73, 132, 345)} | {("wino3d", 0, 2), ("wino3d", 9, 3), ("wino3d", 73, 3)}
    want |= {("wino43", f, 0) for f in (-1, 0, 2, 4, 9, 25, 73, 132, 345)}
    assert reached == want, sorted(reached ^ want)
    for g in golden.values():      # a refused call launches nothing; an accepted one exactly one 512-thread kernel without dynamic LDS
        assert (g["rc"] == 0 and len(g["launches"]) == 1 and g["launches"][0]["block"] == 512 and g["launches"][0]["lds"] == 0) or \
               (g["rc"] in (-1, -2, -3) and g["launches"] == []), g


def test_fixture_refuses_and_accepts_the_classes_the_table_names(golden):
    """the recorded return codes themselves: DF_EINVAL -1 (null, extents, flags), DF_ESHAPE -2 (channels, bounds), DF_EALIGN -3"""
    for rid, entry, dims, cin, cout, flags, ops, mis in ROWS:
        e, rc, tag = ENTRIES[entry], golden[rid]["rc"], rid[len(entry) + 1:]
        if tag.startswith(("null-", "zero-extent", "negative-extent")):
            assert rc == -1, rid
        elif tag.startswith("channels-") or tag.endswith("-over"):
            assert rc == -2, rid
        elif tag.endswith("-at") or tag.startswith(("fl", "fallback-bias", "fallback-all", "grid-")):
            assert rc == 0, rid
        elif tag.startswith("odd-extent"):
            assert rc == (-1 if e.get("even") else 0), rid
        elif tag.startswith("misaligned-"):
            assert rc == (-3 if e["aligned"] & mis else 0), rid
        else:      # the flag / operand rows
            assert rc == -1, rid


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp_dir:
        rec = run_recorder(os.path.abspath(sys.argv[1]), tmp_dir)
    with open(sys.argv[2], "w") as out:
        json.dump(rec, out, indent=0, sort_keys=True)
        out.write("\n")
