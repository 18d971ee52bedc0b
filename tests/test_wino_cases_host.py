"""No GPU: the case table of the Winograd edge tests (tests/wino_cases.py) and the ten 2-D Winograd entry points against the host side of
csrc/conv_wino.hip, csrc/conv_wino43.hip, csrc/conv_wino2d.hip and csrc/conv_wino2d43.hip.  tests/wgrad_launch_recorder.cpp links the
release library, answers the HIP runtime calls itself and prints, per row, the return code and every launch.  Here:
  * every row of the table returns the code, or launches the one instantiation, it claims;
  * the table reaches every instantiation of the four kernel families (and the two backward tails) in the library's symbol table, and no other;
  * what the 2-D entry points accept, refuse and launch -- return code, instantiation, grid, block, LDS bytes, argument bytes -- equals
    tests/golden/wino2d_launches.json, the twin of wino_launches.json, recorded with this recorder from the parent commit's library (efc0617),
    except for the rows CHANGED names;
  * df_wino2d43_signbits_bytes and the two *_packed_elems queries follow the closed forms of the header.
`python tests/test_wino_cases_host.py <library> <json>` records the golden file from any build of the library."""
import json
import os
import re
import subprocess
import sys

import pytest

import wino_cases as wc
from wino_cases import FBIAS, MBITS, MSRC, RES, SBITS, WP, X, Y, Y2

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")      # as deep_fluids_amd/csrc/Makefile
GOLDEN = os.path.join(HERE, "golden", "wino2d_launches.json")

# ---- the rows of the golden file: the classes of tests/test_wino_launches_host.py for the 2-D entry points --------------------------------------
PACK = {"w2_pack": dict(ops=X | WP, need=X | WP, aligned=0), "w2_43_pack": dict(ops=X | WP, need=X | WP, aligned=0)}
QUERIES = ("w2_packed_elems", "w2_43_packed_elems", "w2_43_signbits_bytes")
E2 = dict((n, e) for n, e in wc.ENTRIES.items() if e["nd"] == 2)


def _golden_rows():
    rows = []

    def add(rid, entry, dims, cin, cout, flags=None, ops=None, mis=0):
        e = E2.get(entry) or PACK.get(entry) or dict(flags=0, ops=0)
        rows.append(("g-" + entry + "-" + rid, entry, tuple(dims), cin, cout, e.get("flags", 0) if flags is None else flags,
                     e["ops"] if ops is None else ops, mis))

    small = (2, 10, 12)      # even extents, a ragged tile block
    # ---- every instantiation by name, and the run-time-flags fallbacks ----
    for entry in ("w2_fwd", "w2_43"):
        for fl in (0, 2, 4, 8, 9, 15):
            add("fl%d" % fl, entry, small, 32, 64, fl, wc.ops_of(entry, fl))
    add("fl73", "w2_43_bits", small, 32, 64)
    add("fl132", "w2_43_bits", small, 32, 64, 4, X | WP | MBITS | Y)
    for entry in ("w2_up_fwd", "w2_up_dgrad", "w2_43_addup_bits", "w2_words_bwd"):
        add("base", entry, small, 32, 64)
    add("swap", "w2_up_dgrad", small, 96, 32)      # the kernel's Cin is the entry point's Cout
    # ---- flags without their operands, operands without their flags ----
    for entry in ("w2_fwd", "w2_43"):
        add("bias-without", entry, small, 32, 64, 9, X | WP | Y)
        add("residual-without", entry, small, 32, 64, 2, X | WP | Y)
        add("mask-without", entry, small, 32, 64, 4, X | WP | Y)
        add("addup-flag", entry, small, 32, 64, 25, X | WP | FBIAS | RES | Y)      # (df_wino2d_conv_fwd does not look at unknown bits)
        add("misaligned-res", entry, small, 32, 64, 2, X | WP | RES | Y, RES)
        add("misaligned-msrc", entry, small, 32, 64, 4, X | WP | MSRC | Y, MSRC)
    add("unknown-flag", "w2_43", small, 32, 64, 9 | 32)
    add("fwd-without-bits", "w2_43_bits", small, 32, 64, 9, X | WP | FBIAS | Y)
    add("fwd-without-bias", "w2_43_bits", small, 32, 64, 9, X | WP | Y | SBITS)
    add("both-words", "w2_43_bits", small, 32, 64, 9, X | WP | FBIAS | MBITS | Y | SBITS)
    add("mask-without-bits", "w2_43_bits", small, 32, 64, 4, X | WP | Y)
    add("mask-with-sign-bits", "w2_43_bits", small, 32, 64, 4, X | WP | Y | SBITS)
    add("other-flags", "w2_43_bits", small, 32, 64, 8)
    add("misaligned-mbits", "w2_43_bits", small, 32, 64, 4, X | WP | MBITS | Y, MBITS)
    for fl in (0, 1, 8, 11, 25):
        add("badflags%d" % fl, "w2_up_fwd", small, 32, 64, fl)
    for entry, e in list(E2.items()) + list(PACK.items()):
        pack, tail = entry in PACK, entry == "w2_words_bwd"
        up = pack is False and e["form"] in ("up_fwd", "up_dgrad", "tail")
        # ---- null operands, one at a time; extents; channel counts; odd extents; one misaligned operand at a time ----
        for i, n in enumerate(wc.SLOTS):
            if e["need"] & (1 << i):
                add("null-" + n, entry, small, 32, 64, ops=e["ops"] & ~(1 << i))
            if e["ops"] & (1 << i):
                add("misaligned-" + n, entry, small, 32, 64, mis=1 << i)
        for cin, cout in ((48, 64), (32, 80), (0, 64), (32, 0), (-32, 64)):
            add("channels-%d-%d" % (cin, cout), entry, small, cin, cout)
        if pack:
            for mode in (1, 2, -1):
                add("mode%d" % mode, entry, small, 32, 64, mode)
            continue
        for i in range(3):
            add("zero-extent%d" % i, entry, tuple(0 if j == i else v for j, v in enumerate(small)), 32, 64)
            if i:
                add("odd-extent%d" % i, entry, tuple(v + 1 if j == i else v for j, v in enumerate(small)), 32, 64)
        add("negative-extent", entry, (2, -10, 12), 32, 64)
        # ---- the 2 GiB bound of one image in this entry point's own form, at the limit and one step over it ----
        if tail:    # 4 Hc Wc C = 2^29
            vols = (("in", (1, 2048, 2048), 32, 32),)
        elif up:    # 4 Hc Wc max(Cin, Cout) = 2^29
            vols = (("in", (1, 2048, 2048), 32, 32), ("out", (1, 2048, 1024), 32, 64))
        else:       # H W max(Cin, Cout) = 2^29
            vols = (("in", (1, 4096, 2048), 64, 32), ("out", (1, 4096, 4096), 32, 32))
        for n, dims, cin, cout in vols:
            add("volume-%s-at" % n, entry, dims, cin, cout)
            add("volume-%s-over" % n, entry, dims[:2] + (dims[2] + 2,), cin, cout)
        # ---- tile blocks x cout slices < 2^31: one tile block per image, one slice ----
        add("workgroups-at", entry, ((1 << 31) - 1, 8 if up else 16, 16 if up else 32), 32, 32)
        add("workgroups-over", entry, (1 << 31, 8 if up else 16, 16 if up else 32), 32, 32)
        if tail:
            continue
        add("cincout-at", entry, small, 4096, 4096)      # Cin Cout <= 2^24
        add("cincout-over", entry, small, 4096, 4128)
        # ---- at most 256 cout slices (the dgrad's are the entry point's Cin) ----
        dg = e["form"] == "up_dgrad"
        add("cout-slices-at", entry, small, 8192 if dg else 32, 32 if dg else 8192)
        add("cout-slices-over", entry, small, 8224 if dg else 32, 32 if dg else 8224)
    # ---- grids: cout slices x (few | ragged | saturating) tile blocks ----
    for ncs in (1, 2, 3, 4, 8, 16):
        for n, dims in (("1", (1, 16, 32)), ("3", (3, 16, 32)), ("12", (1, 17, 161)), ("37", (37, 15, 32)), ("100", (25, 32, 64)), ("257", (257, 16, 32)),
                        ("512", (16, 64, 256))):
            add("grid-ncs%d-ntb%s" % (ncs, n), "w2_fwd", dims, 32, 32 * ncs)
            add("grid-ncs%d-ntb%s" % (ncs, n), "w2_43", dims, 32, 32 * ncs)
        add("grid-ncs%d" % ncs, "w2_up_dgrad", (3, 4, 8), 32 * ncs, 64)
        add("grid-ncs%d" % ncs, "w2_up_fwd", (3, 4, 8), 32, 32 * ncs)
        add("grid-ncs%d" % ncs, "w2_43_addup_bits", (3, 8, 16), 32, 32 * ncs)
        add("grid-ncs%d" % ncs, "w2_words_bwd", (3, 4, 8), 32 * ncs, 32 * ncs)
    # ---- the queries: answers and refusals ----
    for cin, cout in ((32, 32), (96, 160), (4096, 4096)):
        for mode in (0, 1):
            add("c%d-%d-m%d" % (cin, cout, mode), "w2_packed_elems", (1, 1, 1), cin, cout, mode)
            add("c%d-%d-m%d" % (cin, cout, mode), "w2_43_packed_elems", (1, 1, 1), cin, cout, mode)
    for dims, c in (((1, 1, 1), 32), ((2, 16, 32), 32), ((3, 17, 33), 96), ((1, 10, 12), 256), ((2, 16, 32), 48), ((2, 16, 32), 0), ((2, 16, 32), -32),
                    ((0, 16, 32), 32), ((2, 0, 32), 32), ((2, 16, 0), 32), ((2, -16, 32), 32), (((1 << 20), 4096, 4096), 256)):
        add("%s-c%d" % ("x".join(str(v) for v in dims), c), "w2_43_signbits_bytes", dims, c, c)
    assert len({r[0] for r in rows}) == len(rows)
    return rows


GOLDEN_ROWS = _golden_rows()
# Rows whose recorded (parent) behaviour this commit changes on purpose, with the reason
CHANGED = dict((r[0], "more than 256 cout slices: the parent launched an EMPTY grid ((256 // ncs) * ncs = 0 workgroups: a raw HIP error on a device); "
                      "now refused with DF_ESHAPE before any launch") for r in GOLDEN_ROWS if r[0].endswith("-cout-slices-over"))


def _instantiation(name):
    """[family, FL, MODE] of a kernel symbol; a kernel that is no template: [its name, 0, 0]"""
    m = re.search(r"(wino3d|wino43|wino2d43|wino2d)_kernel<([-0-9, ]+)>", name)
    if not m:
        return [re.sub(r"\(.*", "", name.replace("(anonymous namespace)::", "")).split("::")[-1], 0, 0]
    v = [int(t) for t in m.group(2).split(",")]
    assert len(v) in (1, 2), name
    return [m.group(1), v[0], v[1] if len(v) == 2 else 0]


def _line(rid, entry, dims, cin, cout, flags, ops, mis):
    return "%s %s %s %d %d %d %d %d\n" % (rid, entry, " ".join(str(v) for v in dims), cin, cout, flags, ops, mis)


def run_recorder(lib_path, tmp, lines):
    """{row id: {"rc", "value" (a query's answer), "launches": [{"kernel": [family, FL, MODE], "grid", "block", "lds", "args"}, ...]}}"""
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
        f.writelines(lines)
    got, cur = {}, None
    for line in subprocess.check_output([exe, syms, rows]).decode().splitlines():
        w = line.split()
        if w[0] == "row":
            cur = []
        elif w[0] == "launch":
            m = re.match(r"\s+launch (.*) grid (\d+) (\d+) (\d+) block (\d+) lds (\d+) args ([0-9a-f.]+)$", line)
            assert m, line      # a symbol of the library, with a known argument layout
            cur.append({"kernel": _instantiation(m.group(1)), "grid": [int(m.group(i)) for i in (2, 3, 4)], "block": int(m.group(5)),
                        "lds": int(m.group(6)), "args": m.group(7)})
        elif w[0] == "end":
            got[w[1]] = {"rc": int(w[3]), "value": int(w[5]), "launches": cur}
    return got


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    """one recorder run over the table and the golden rows"""
    from deep_fluids_amd import _lib
    lines = [_line(r["id"], r["entry"], r["shape"], r["cin"], r["cout"], r["flags"], r["ops"], r["mis"]) for r in wc.ROWS]
    lines += [_line(*r) for r in GOLDEN_ROWS]
    return run_recorder(_lib.LIB_PATH, str(tmp_path_factory.mktemp("wino_cases")), lines)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------
def test_table_is_consistent():
    for r in wc.ROWS:
        e = wc.ENTRIES[r["entry"]]
        assert set(r["off"].values()) <= {0, 1} and sum(r["off"].values()) <= 1, r["id"]
        if r["twin"]:
            t = wc.by_id(r["twin"])
            assert all(t[k] == r[k] for k in ("shape", "cin", "cout", "mode")) and not t["mis"] and not isinstance(t["reaches"], int), r["id"]
            assert wc.ENTRIES[t["entry"]]["fam"] == e["fam"], r["id"]
        if r["passes"]:      # ntb from the shape; more than one pass of the grid, not a whole number of passes
            ntb, per = r["passes"]
            blk = (16, 32) if e["nd"] == 2 else (4, 8, 8)
            n = r["shape"][0]
            for v, b in zip(r["shape"][1:], blk):
                n *= -(-v // b)
            ncs = r["cout"] // 32
            assert n == ntb and per == (256 // ncs if 8 % ncs else {1: 256, 2: 128, 4: 64, 8: 32}[ncs]) and per < ntb < 2 * per, r["id"]
            out = r["cout"]
            for v in r["shape"]:
                out *= v
            assert out <= 2.2e6, (r["id"], out)      # the largest output of the table
    # every operand the host leaves unchecked has its offset-1 row on a ragged and on a full block; every checked one its DF_EALIGN row
    for entry, e in wc.ENTRIES.items():
        for i, s in enumerate(wc.SLOTS):
            if e["loose"] & (1 << i):
                assert len([r for r in wc.OK_ROWS if r["entry"] == entry and r["mis"] == 1 << i and r["twin"]]) >= 2, (entry, s)
            if e["aligned"] & (1 << i):
                assert [r for r in wc.ERR_ROWS if r["entry"] == entry and r["mis"] == 1 << i and r["reaches"] == wc.EALIGN], (entry, s)
    assert len(set(wc.by_id(i)["cout"] // 32 for i in wc.MULTIPASS if wc.by_id(i)["entry"] == "wino43")) == 4


@pytest.mark.parametrize("rid", [r["id"] for r in wc.ROWS])
def test_row_returns_or_launches_what_it_claims(record, rid):
    r, got = wc.by_id(rid), record[rid]
    if isinstance(r["reaches"], int):
        assert got["rc"] == r["reaches"] and got["launches"] == [], (rid, got)
        return
    fam, fl, mode = r["reaches"]
    want = [wc.TAILS[fam], 0, 0] if fam in wc.TAILS else [fam, fl, mode]
    assert got["rc"] == 0 and [l["kernel"] for l in got["launches"]] == [want], (rid, got, want)
    la = got["launches"][0]
    assert la["grid"][0] >= 1 and la["grid"][1:] == [1, 1] and la["lds"] == 0 and la["block"] == (256 if fam == "bits_bwd" else 512), (rid, la)
    if fam not in wc.TAILS:      # the persistent grid: at most one workgroup per CU, a multiple of the slice count or of the 8 XCDs
        ncs = (r["cin"] if wc.ENTRIES[r["entry"]]["form"] == "up_dgrad" else r["cout"]) // 32
        assert la["grid"][0] <= 256 and la["grid"][0] % (8 if 8 % ncs == 0 else ncs) == 0, (rid, la)


def test_table_reaches_every_instantiation_and_no_other():
    """fails when a kernel variant is added to one of the four files without a row (or a row outlives its variant)"""
    from deep_fluids_amd import _lib
    out = subprocess.check_output(["nm", "-C", "--defined-only", _lib.LIB_PATH]).decode()
    have = set()
    for fam, pat in wc.FAMILIES.items():
        for m in re.findall(r"::(%s[-0-9, ]+>)" % re.escape(pat), out):
            have.add(tuple(_instantiation(m)))
    for fam, name in wc.TAILS.items():
        if re.search(r"::%s\(" % name, out):
            have.add((fam, 0, 0))
    assert len(have) == 12 + 9 + 6 + 7 + 2, sorted(have)      # the patterns still find the kernels (conv_wino | 43 | 2d | 2d43 | tails)
    named = set(r["reaches"] for r in wc.OK_ROWS)
    assert have - named == set(), "instantiations without a row in tests/wino_cases.py: %s" % sorted(have - named)
    assert named - have == set(), "rows that name a kernel the library does not hold: %s" % sorted(named - have)


# ---- the golden file of the 2-D entry points ------------------------------------------------------------------------------------------------------
def _strip(g):
    return {"rc": g["rc"], "value": g["value"], "launches": g["launches"]}


@pytest.mark.parametrize("rid", [r[0] for r in GOLDEN_ROWS])
def test_call_returns_and_launches_what_the_fixture_holds(record, golden, rid):
    if rid in CHANGED:
        assert golden[rid]["rc"] == 0 and [l["grid"] for l in golden[rid]["launches"]] == [[0, 1, 1]], (rid, golden[rid])      # the defect, as recorded
        assert record[rid] == {"rc": wc.ESHAPE, "value": 0, "launches": []}, (rid, record[rid])
        return
    assert record[rid] == golden[rid], (rid, record[rid], golden[rid])


def test_fixture_holds_exactly_the_rows_and_every_2d_instantiation(golden):
    assert sorted(golden) == sorted(r[0] for r in GOLDEN_ROWS)
    reached = {tuple(l["kernel"]) for g in golden.values() for l in g["launches"]}
    want = {("wino2d", f, 0) for f in (-1, 2, 4, 9)} | {("wino2d", 9, 1), ("wino2d", 0, 2)} | {("wino2d43", f, 0) for f in (-1, 2, 4, 9, 73, 132, 345)}
    want |= {("lrelu_words2d_bwd_pool_kernel", 0, 0), ("wino2d_pack_kernel", 0, 0), ("wino2d43_pack_kernel", 0, 0)}
    assert reached == want, sorted(reached ^ want)
    for rid, g in golden.items():      # a refused call launches nothing; an accepted one exactly one kernel without dynamic LDS
        assert (g["rc"] == 0 and len(g["launches"]) == (0 if rid.split("-")[1] in QUERIES else 1) and all(l["lds"] == 0 for l in g["launches"])) or \
               (g["rc"] in (-1, -2, -3) and g["launches"] == []), (rid, g)


def test_fixture_refuses_and_accepts_the_classes_the_rows_name(golden):
    """the recorded return codes themselves: DF_EINVAL -1 (null, extents, flags), DF_ESHAPE -2 (channels, bounds), DF_EALIGN -3"""
    for rid, entry, dims, cin, cout, flags, ops, mis in GOLDEN_ROWS:
        if entry in QUERIES:
            continue
        e, rc, tag = E2.get(entry) or PACK[entry], golden[rid]["rc"], rid[len(entry) + 3:]
        if tag.startswith(("null-", "zero-extent", "negative-extent")):
            assert rc == -1, rid
        elif tag.startswith("channels-"):
            assert rc == (0 if entry == "w2_words_bwd" and cin == 32 else -2), rid      # (the tail has one channel count, C = cin)
        elif tag.endswith("-over") and rid not in CHANGED:
            assert rc == -2, rid
        elif tag.endswith("-at") or tag.startswith(("fl", "base", "swap", "grid-")) or rid in CHANGED:
            assert rc == 0, rid
        elif tag.startswith("odd-extent"):
            assert rc == (-1 if e["form"] == "addup" else 0), rid
        elif tag.startswith("misaligned-"):
            assert rc == (-3 if e["aligned"] & mis else 0), rid
        elif tag.startswith("mode"):
            assert rc == (0 if flags == 1 else -2), rid
        elif tag == "addup-flag" and entry == "w2_fwd":
            assert rc == 0 and golden[rid]["launches"][0]["kernel"] == ["wino2d", -1, 0], rid      # ADDUP is no bit this kernel tests
        else:      # the flag / operand rows
            assert rc == -1, rid


def test_size_queries_follow_the_closed_forms_of_the_header(record):
    n = 0
    for rid, entry, dims, cin, cout, flags, ops, mis in GOLDEN_ROWS:
        if entry not in QUERIES:
            continue
        got = record[rid]
        if entry == "w2_43_signbits_bytes":      # one 32-bit word per (tile block of 16 x 32 pixels, 32-channel slice, thread of 512); refusals: 0
            B, H, W = dims
            ok = B > 0 and H > 0 and W > 0 and cin > 0 and cin % 32 == 0
            want = B * -(-H // 16) * -(-W // 32) * (cin // 32) * 512 * 4 if ok else 0
        else:                                    # 4 x 4 | 4 x 6 transform points per (cin, cout) filter, either mode
            want = (16 if entry == "w2_packed_elems" else 24) * cin * cout
        assert got["rc"] == 0 and got["launches"] == [] and got["value"] == want, (rid, got, want)
        n += 1
    assert n == 24


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp_dir:
        rec = run_recorder(os.path.abspath(sys.argv[1]), tmp_dir, [_line(*r) for r in GOLDEN_ROWS])
    with open(sys.argv[2], "w") as out:
        json.dump(rec, out, indent=0, sort_keys=True)
        out.write("\n")
