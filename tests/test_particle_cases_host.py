"""No GPU: the case table of the particle and liquid edge tests (tests/particle_cases.py).
  * Completeness: the df_* names the public header declares in its particle, FLIP, ghost-fluid level-set and resampling blocks that are
    defined in csrc/particles.hip or csrc/liquid.hip -- taken from the header as deep_fluids_amd._lib parses it for its binding -- are
    exactly the entry points the table names.
  * Block counts: the cell-per-thread kernels that take their block from xcd_block(bid, nblk, 0) are reached at 1, 7, 8, 9 and 17
    workgroups (remainder 1, 7, 0, 1, 1 and quotient 0, 0, 1, 1, 2), the particle-per-thread kernels at B*N = 1, 255, 256, 257 and 771.
  * Reference run: the NumPy restatements run on every row in fp64 and in their fp32 twin; e32 is printed per row.
  * Hostile rows: the restatement alone is finite where the header says so, selects the documented edge cell or particle and writes no
    row at or beyond the capacity; hostile indices stay within 5 elements of their array.
  * The one-call restatements of the resampling added for these tests agree with liquid_resample_ref.resample on its own state."""
import os
import re

import numpy as np
import pytest

import liquid_resample_ref as rref
import particle_cases as pc
import particles_ref as pref
from deep_fluids_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deep_fluids_amd", "csrc")
FAMILY = re.compile(r"df_(particles_|particle_levelset_|levelset_|liquid_|mac_extrapolate|flip_update|resample_)")


def _defined():
    names = set()
    for f in ("particles.hip", "liquid.hip"):
        with open(os.path.join(CSRC, f)) as fh:
            names |= set(re.findall(r"^int (df_\w+)\(", fh.read(), re.M))
    return names


def test_table_is_complete():
    declared = set(n for n in _lib.SIGNATURES if FAMILY.match(n))
    defined = _defined()
    assert declared == defined, sorted(declared ^ defined)
    assert len(declared) == 35
    named = set(pc.entry_point(r) for r in pc.ROWS)
    assert named == declared, sorted(named ^ declared)
    for r in pc.ROWS:                                        # the argument count the harness will pass is the header's
        ops = pc.OPS[r["op"]]
        ptrs = set(n for n, _ in ops[1]) | set(n for n, _ in ops[2])
        if not r["ragged"]:
            ptrs.discard("es")
        sig = _lib.SIGNATURES[pc.entry_point(r)][1]
        assert sum(1 for a in sig if a is _lib.P) == len(ptrs) + 1, r["name"]          # + the stream


def test_block_counts():
    for op in pc.REMAPPED_OPS:
        got = sorted(pc.block_count(r) for r in pc.rows(op, axes="blocks"))
        assert got == [1, 7, 8, 9, 17], (op, got)
        assert sorted((n % 8, n // 8) for n in got) == sorted([(1, 0), (7, 0), (0, 1), (1, 1), (1, 2)])
    for nblk, (B, shape) in pc.GRIDS.items():
        assert -(-B * int(np.prod(shape)) // pc.THREADS) == nblk
    for op in pc.PARTICLE_THREAD_OPS:
        for d in (2, 3):
            got = sorted(r["B"] * r["N"] for r in pc.rows(op, axes="counts") if len(r["shape"]) == d)
            assert got == [1, 255, 256, 257, 771], (op, got)
    assert 771 > 512 and set(r["B"] for r in pc.rows(axes="odd,B2")) == {2}
    for r in pc.rows(axes="odd,B2"):
        assert all(n % 2 for n in r["shape"]) and (r["B"] * int(np.prod(r["shape"]))) % pc.THREADS and int(np.prod(r["shape"])) % pc.THREADS


def test_axes_are_present():
    """the axes of the issue that are not a count: every op has a loose twin in 2-D and 3-D, the windows, the ragged forms, N = 0"""
    for op in pc.OPS:
        for d in (2, 3):
            loose = [r for r in pc.rows(op, off=1) if len(r["shape"]) == d]
            assert loose and all(pc.BY_NAME[r["twin"]]["off"] == 0 for r in loose), (op, d)
    for op in ("union", "averaged"):
        assert set(r["rf"] for r in pc.rows(op)) >= set(pc.RADIUS_FACTORS)
        assert set(r["shape"][0] for r in pc.rows(op, rf=2.0, axes="window") if len(set(r["shape"])) == 1) >= {2, 3, 4}
        assert pc.rows(op, N=0)
    assert set((r["mode"], r["band"]) for r in pc.rows("smooth")) >= set((m, b) for m in (0, 1, 2) for b in (0, 1, 7))
    assert all(7 >= max(s) / 2.0 for s in pc.MID.values())
    for op in ("extrap", "layer"):
        assert set(r["layer"] for r in pc.rows(op)) >= ({1, 2, 254} if op == "extrap" else {2, 254})
    for op in ("trace", "keys", "flip"):
        assert set(r["ragged"] for r in pc.rows(op)) >= {None, "dense", "empty_first", "empty_last", "unused", "nonmono"}
    for r in pc.ROWS:
        if isinstance(r["place"], tuple):
            i = pc.inputs(r)
            cells = np.diff(pref.clamp_ranges(i["cs"], len(i["sp"]))) if "cs" in i else np.bincount(rref.keys(i["pos"], i["es"] if r["ragged"] else np.arange(r["B"] + 1) * r["N"], r["shape"]))
            assert cells.max() >= 300, r["name"]


def _e32(r):
    a, b = pc.expected(r, np.float32), pc.expected(r, np.float64)
    worst = 0.0
    for name in a:
        x, y = np.asarray(a[name][0], np.float64), np.asarray(b[name][0], np.float64)
        assert x.shape == y.shape, (r["name"], name)
        with np.errstate(invalid="ignore"):
            both = np.isfinite(x) & np.isfinite(y)
        if both.any():
            worst = max(worst, float(np.abs(x[both] - y[both]).max()))
    return worst


@pytest.mark.parametrize("op", sorted(pc.OPS))
def test_reference_runs(op):
    for r in pc.rows(op):
        e = _e32(r)
        print("%-34s %-40s blocks %3d  e32 %.3e" % (r["name"], pc.entry_point(r), pc.block_count(r), e))
        out = pc.expected(r, np.float32)
        assert set(out) == set(n for n, _ in pc.OPS[op][2])
        if r["twin"]:                                        # a loose row computes what its twin computes
            tw = pc.expected(pc.BY_NAME[r["twin"]], np.float32)
            for name in out:
                np.testing.assert_array_equal(out[name][0], tw[name][0])


def _written(pair):
    a, w = pair
    return a if w is None else a[w]


HOSTILE = [r["name"] for r in pc.ROWS if r["hostile"]]


@pytest.mark.parametrize("name", HOSTILE)
def test_hostile_rows(name):
    r = pc.BY_NAME[name]
    i = pc.inputs(r)
    shape, B, N = r["shape"], r["B"], r["N"]
    D, P = len(shape), B * N
    ncell = int(np.prod(shape))
    for dtype in (np.float32, np.float64):
        out = pc.expected(r, dtype)
        # ---- the planted values are there, and within 5 elements of their array ----
        if "pos" in r["hostile"]:
            p = i["pos"] if "pos" in i else i["sp"]
            assert np.isnan(p[:i.get("live", P)]).any() and np.isposinf(p).any() and np.isneginf(p).any() and (p == -1).any() and (p == 1e30).any()
            assert any((p[:, a] == shape[::-1][a]).any() for a in range(D))
        if "vel" in r["hostile"]:
            assert np.isnan(i["vel"]).any() and np.isposinf(i["vel"]).any() and np.isneginf(i["vel"]).any()
        if "order" in r["hostile"]:
            assert set(i["order"][(i["order"] < 0) | (i["order"] >= P)]) == {-1, P, P + 3}
        if "cell_start" in r["hostile"]:
            cs = i["cs"].astype(np.int64)
            assert cs.min() == -3 and cs.max() == P + 5 and (np.diff(cs) < 0).any()
            assert r["op"] == "scatter" or set(range(P + 1, P + 6)) <= set(cs)
            if r["op"] == "scatter":
                # behind row B*N lie 5 finite decoys; with the upper clamp gone the last cell would copy them (the keep bytes there are
                # the non-zero guard fill) into rows behind the wanted total, which must keep the fill: emulate that with the
                # restatement on the padded arrays, whose capacity then lets the hostile end through
                for n in ("sp", "spvel"):
                    padded, lead = i["padded"][n]
                    assert lead == 0 and len(padded) == P + 5 and np.isfinite(padded[P:]).all()
                    assert (padded[:P].view(np.int32) == i[n].view(np.int32)).all()
                assert cs[-1] == P + 5 and i["wanted"] + 5 <= P
                keep = np.concatenate([i["keep"], np.full(5, 0xA5, np.uint8)])
                po, _, w = rref.resample_scatter(i["padded"]["sp"][0], i["padded"]["spvel"][0], cs, keep, i["seeds"], i["new_start"], i["vel"],
                                                 r["minp"], pc.SEED, pc.STEP, dtype)
                extra = np.flatnonzero(w[i["wanted"]:P])
                assert len(extra) == 5 and (po[i["wanted"]:i["wanted"] + 5] == pc.decoy_position(D)).all()
            if r["op"] == "union":                              # the hostile ends land on the decoys, none on the guard
                padded, lead = i["padded"]["sp"]
                assert lead == 3 * D and len(padded) == P + 3 + 5 and (padded[3:3 + P].view(np.int32) == i["sp"].view(np.int32)).all()
                assert (padded[:3] == pc.decoy_position(D)).all() and (padded[3 + P:] == pc.decoy_position(D)).all()
        if "entry_start" in r["hostile"]:
            assert (np.diff(i["es"]) < 0).any() and i["es"].min() >= 0 and i["es"].max() <= P
        if "new_start" in r["hostile"]:
            ns = i["new_start"].astype(np.int64)
            assert ns.min() == -3 and P < ns.max() <= P + 5
        if "seeds" in r["hostile"]:
            assert i["seeds"].min() == -2 and i["seeds"].max() == r["minp"] + 3
        if "overflow" in r["hostile"]:
            assert P < i["wanted"] <= P + 5
        # ---- finite where the header says so; the documented edge cell or particle; nothing at or beyond the capacity ----
        if r["op"] == "trace":
            got = _written(out["pos_out"]).reshape(-1, D)
            lo, hi = pref.clamp_bounds(shape, r["bnd"], dtype)
            assert np.isfinite(got).all() and (got >= lo).all() and (got <= hi).all()       # pushed back into the domain, NaN -> bnd
            if "pos" in r["hostile"]:
                assert (got[np.isnan(i["pos"]).all(axis=1)] == lo).all()
        elif r["op"] == "keys":
            k = out["keys"][0]
            assert k.min() >= 0 and k.max() <= B * ncell
            if "pos" in r["hostile"]:
                p = i["pos"]
                ext = shape[::-1]
                e = rref.entries(np.arange(B + 1) * N, P)
                np.testing.assert_array_equal(k[np.isnan(p).all(axis=1)] - e[np.isnan(p).all(axis=1)] * ncell, 0)          # NaN -> cell 0
                np.testing.assert_array_equal(k[np.isneginf(p).all(axis=1)] - e[np.isneginf(p).all(axis=1)] * ncell, 0)
                for big in (np.isposinf(p).all(axis=1), (p == 1e30).all(axis=1), (p == np.array(ext, np.float32)).all(axis=1)):
                    assert big.any()
                    np.testing.assert_array_equal(k[big] - e[big] * ncell, ncell - 1)                                       # -> the last cell
            else:
                e = rref.entries(i["es"], P)
                np.testing.assert_array_equal(k[e < 0], B * ncell)
                assert ((k[e >= 0] // ncell) == e[e >= 0]).all() and e.max() <= B - 1
        elif r["op"] == "gather":
            o = i["order"]
            g = out["pos_sorted"][0]
            np.testing.assert_array_equal(g[o < 0], np.broadcast_to(i["pos"][0].astype(dtype), g[o < 0].shape))             # the first row
            np.testing.assert_array_equal(g[o >= P], np.broadcast_to(i["pos"][P - 1].astype(dtype), g[o >= P].shape))       # the last row
        elif r["op"] == "union":
            phi = out["phi"][0]
            assert np.isfinite(phi).all() and (phi <= pref.radius_of(D, r["rf"], dtype)).all()
            if "cell_start" in r["hostile"]:
                # what the clamps keep out: a decoy sits on the centre of cell (1, 0[, 0]) of entry 0, whose thread reads cell_start[0] = -3
                # as a start and cell_start[4] = B*N + 3 as an end; walking one would give sqrt(0) - radius there
                cs, X, w = i["cs"], shape[-1], pref.window_of(r["rf"])
                assert max(1 - w, 0) == 0 and min(1 + w, X - 1) + 1 == 4 and cs[0] == -3 and cs[4] == P + 3
                # by a margin far above the GPU test's bound of 3 * e32 + 1e-7, whatever the seed puts next to the decoy
                assert phi[(0,) * D + (1,)] + pref.radius_of(D, r["rf"], dtype) > 1e-3
        elif r["op"] == "averaged":
            phi, wacc, _ = pc.gref.levelset_raw(i["sp"].reshape(B, N, D), i["cs"], shape, r["rf"], dtype, parts=True)
            assert (np.isnan(phi) == np.isnan(out["phi"][0])).all()
            if "pos" in r["hostile"]:
                # 0 * NaN and 0 * inf enter pacc: a cell is NaN exactly where a particle with a non-finite coordinate lies in its window
                # and the weights of the window sum to more than 1e-6; every other cell is finite
                rad = int(pref.radius_of(D, r["rf"], dtype)) + 1
                sp = i["sp"]
                bad = np.flatnonzero(~np.isfinite(sp).all(axis=1))
                ext = shape[::-1]
                poisoned = np.zeros((B,) + shape, bool)
                for row in bad:
                    at = [int(pref._cell_of(sp[row, a:a + 1], ext[a])[0]) for a in range(D)]
                    win = tuple(slice(max(at[a] - rad, 0), at[a] + rad + 1) for a in reversed(range(D)))
                    poisoned[(row // N,) + win] = True
                assert len(bad) and poisoned.any() and not poisoned.all()
                assert (np.isnan(phi) == (poisoned & (wacc > dtype(1e-6)))).all()
                assert np.isfinite(phi[~np.isnan(phi)]).all() and np.isnan(phi).any()
            else:
                # the clamps select edge particles: the result is that of the ranges cut to 0 .. B*N by hand, and finite
                assert np.isfinite(phi).all()
                cut = np.clip(i["cs"].astype(np.int64), 0, P)
                np.testing.assert_array_equal(phi, pc.gref.levelset_raw(i["sp"].reshape(B, N, D), cut, shape, r["rf"], dtype))
        elif r["op"] == "p2g":
            for name in ("vel", "weight"):
                assert np.isfinite(out[name][0]).all(), name                                # positions only select cells; pvel is finite
            assert (out["weight"][0] >= 0).all()
        elif r["op"] == "flip":
            got = _written(out["pvel_out"])
            if "vel" not in r["hostile"]:
                assert np.isfinite(got).all()
        elif r["op"] == "flags":
            assert (out["flags"][0] < 128).all() and set(np.unique(out["touch"][0])) <= {0, 1}
            inter = np.broadcast_to(pc.interior_mask(shape, r["bnd"])[None], out["flags"][0].shape)
            assert not (out["flags"][0][~inter] & 1).any()
        elif r["op"] == "forces":
            assert np.isfinite(out["out"][0]).all()
        elif r["op"] == "count":
            keep, w = out["keep"]
            assert set(np.unique(keep[w])) <= {0, 1} and (out["kept"][0] >= 0).all() and (out["seeds"][0] >= 0).all()
            assert (out["seeds"][0] <= r["minp"]).all() and out["kept"][0].max() <= P
        elif r["op"] == "scatter":
            po, w = out["pos_out"]
            assert po.shape == (P, D) and np.isfinite(po[w]).all()
            rows = w.all(axis=1)
            if "overflow" in r["hostile"]:
                assert rows.all()                                                           # full to the last row, the tail left out
            else:
                assert not rows[i["wanted"]:].any() and rows[:i["wanted"]].all()


@pytest.mark.parametrize("shape", rref.SHAPES)
def test_one_call_restatements_agree_with_resample(shape):
    """resample_count and resample_scatter (one call each, with the header's clamps and a capacity) against rref.resample"""
    s = rref.resample_state(shape)
    f, _ = pc.lref.flags_of(s["liquid"])
    for dtype in (np.float32, np.float64):
        want = rref.resample(s["pos"], s["pvel"], s["cell_start"], s["phi"], s["liquid"], s["vel"], rref.MIN_P, dtype=dtype)
        keep, kept, seeds = rref.resample_count(s["pos"], s["cell_start"], s["phi"], f, rref.BND, rref.MIN_P, 2 * rref.MIN_P, 1.0, dtype)
        np.testing.assert_array_equal(np.where(keep == 255, 0, keep), want["keep"])
        np.testing.assert_array_equal(kept, want["kept"])
        np.testing.assert_array_equal(seeds, want["seeds"])
        po, pv, written = rref.resample_scatter(s["pos"], s["pvel"], s["cell_start"], want["keep"], seeds, want["cell_start"], s["vel"],
                                                rref.MIN_P, 123, 0, dtype)
        t = want["total"]
        assert written[:t].all() and not written[t:].any()
        np.testing.assert_array_equal(po[:t], want["pos"])
        np.testing.assert_array_equal(pv[:t], want["pvel"])


def test_bisection_is_searchsorted_on_monotone_starts():
    rng = np.random.RandomState(0)
    for _ in range(50):
        B, P = rng.randint(1, 6), rng.randint(1, 40)
        es = np.sort(rng.randint(0, P + 1, size=B + 1))
        e = np.searchsorted(es, np.arange(P), side="right") - 1
        np.testing.assert_array_equal(rref.entries(es, P), np.where(e == B, -1, e))
