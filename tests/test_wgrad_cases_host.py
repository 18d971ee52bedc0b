"""No GPU: the case table of the weight-gradient edge tests (tests/wgrad_cases.py) against the host side of csrc/conv_wgrad.hip -- the form
queries, the workspace queries, and the symbol table of the release library.  The table's "reaches" column is observed by
tests/test_wgrad_launches_host.py; what keeps it complete here is that it must name EVERY weight-gradient kernel instantiation the library
holds, and nothing else: a new instantiation without a row fails test_every_instantiation_has_a_row."""
import re
import subprocess

import pytest

import wgrad_cases as wc
from deep_fluids_amd import _lib

FP32_ROWS = [r for r in wc.ALL_ROWS if r[1] in ("conv", "up", "conv_bf16x3", "up_bf16x3")]
# kernel family -> what the form query calls it
CONV_FORM = {"wgrad_kernel": 0, "wgrad_wx_kernel": 1, "wgrad_wxy_kernel": 2, "wgrad_wxyz_fused_kernel": 3, "wgrad_wxyz_staged_kernel": 3,
             "wgrad_thin_mfma_kernel": 10, "wgrad_small_n_kernel": 11}
UP_FORM = {"wgrad_wxyz_up_fused_kernel": 3, "wgrad_up2_kernel": 0, "wgrad_kernel": 0}


def _ws_query(row, B=None):
    _, entry, (b, D, H, W), cin, cout, kz = row[:6]
    name = {"conv": "df_conv_wgrad_workspace_bytes", "conv_bf16x3": "df_conv_wgrad_workspace_bytes", "up": "df_upconv_wgrad_workspace_bytes",
            "up_bf16x3": "df_upconv_wgrad_workspace_bytes", "s2": "df_conv_s2_wgrad_workspace_bytes"}[entry]
    return _lib.query(name, b if B is None else B, D, H, W, cin, cout, kz)


def test_row_ids_are_unique_and_twins_exist():
    ids = [r[0] for r in wc.ALL_ROWS]
    assert len(ids) == len(set(ids))
    for r in wc.ALL_ROWS:
        assert len(r) == 13 and (r[5] == 3 or r[2][1] == 1), r[0]
        if r[12] is not None:
            twin = wc._row(r[12][0])
            assert twin[1:8] == r[1:8] and twin[8:10] == (0, 0) and r[12][1] in ("bits", "tol"), r[0]
            if r[11] != "EALIGN" and r[12][1] == "bits":      # "bits" is claimed only for the same kernel, or staged -> register-ring
                assert r[11] == twin[11] or (twin[11][0].startswith("wgrad_wxyz_staged") and r[11][0].startswith("wgrad_wxyz_fused")), r[0]
    for rid in wc.BATCH_ROWS + [p[0] for p in wc.PADDED]:
        assert wc._row(rid)[8:10] == (0, 0)


@pytest.mark.parametrize("row", FP32_ROWS, ids=[r[0] for r in FP32_ROWS])
def test_form_query_answers_what_the_row_claims(row):
    rid, entry, (B, D, H, W), cin, cout, kz, algo = row[:7]
    q = "df_upconv_wgrad_form" if entry.startswith("up") else "df_conv_wgrad_form"
    got = _lib.query(q, B, D, H, W, cin, cout, kz, algo or 0)
    assert got == row[10], (rid, got, row[10])
    # aligned fp32 rows: the kernel the row names belongs to the family the query reports
    if entry in ("conv", "up") and row[8:10] == (0, 0):
        fam = row[11][0].split("<")[0]
        assert (UP_FORM if entry == "up" else CONV_FORM)[fam] == got, (rid, fam, got)


def test_every_instantiation_has_a_row():
    out = subprocess.check_output(["nm", "-C", _lib.LIB_PATH]).decode()
    pat = r"\b(?:%s)[^>]*>" % "|".join(re.escape(f) for f in wc.FAMILIES)
    have = set(re.sub(r"\s+", "", m) for m in re.findall(pat, out))
    named = set(k for r in wc.ALL_ROWS if r[11] != "EALIGN" for k in r[11])
    assert len(have) > 60, sorted(have)      # the pattern still finds the kernels
    assert not (set(wc.UNREACHABLE) & named), "a row reaches an instantiation listed as unreachable"
    assert not (set(wc.UNREACHABLE) - have), "UNREACHABLE names an instantiation the library no longer holds"
    named |= set(wc.UNREACHABLE)
    assert have - named == set(), "instantiations without a row in tests/wgrad_cases.py: %s" % sorted(have - named)
    assert named - have == set(), "rows that name a kernel the library does not hold: %s" % sorted(named - have)


@pytest.mark.parametrize("row", wc.ROWS, ids=[r[0] for r in wc.ROWS])
def test_workspace_query_is_positive_whole_floats_and_monotone_in_batch(row):
    sizes = [_ws_query(row, B) for B in (1, 2, 3, 4, 8, 64)]
    own = _ws_query(row)
    print(row[0], own, sizes)
    assert own > 0 and own % 4 == 0
    assert all(s > 0 and s % 4 == 0 for s in sizes)
    assert all(b >= a for a, b in zip(sizes, sizes[1:])), sizes
