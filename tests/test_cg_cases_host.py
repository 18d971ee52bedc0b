"""No GPU: the conditions on the rows of tests/cg_cases.py that tests/test_gpu_cg_edges.py relies on, each from the fp32 twin alone --
the workgroup counts the table must cover, a non-zero residual past workgroup 255 on every row with more than 256, the iteration counts
the rows state for the entry at rest and the early-freezing entry, and the told-apart condition: the twin with a wrong reduction (partials
256.. lost, partial t + 256 added by thread t + 1, NumPy's order, the lanes of a wave in ascending order) differs from the true twin in
the bits of x after the row's iterations.  Also cg_ref itself against a scalar loop, and that the restatements' default reductions are
still NumPy's.  Mutants run on entry 0 alone (an entry's result does not depend on the rest of the batch: asserted once)."""
import numpy as np
import pytest

import cg_cases as cc
import cg_ref

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


# ---- cg_ref against a thread-by-thread loop ------------------------------------------------------------------------------------------------
def _scalar_block(v):
    """one workgroup, lane by lane: the xor butterfly on all 64 lanes, lane 0's value, then the four waves ascending"""
    waves = []
    for w in range(4):
        lanes = [F32(x) for x in v[64 * w:64 * w + 64]]
        m = 32
        while m >= 1:
            lanes = [F32(lanes[l] + lanes[l ^ m]) for l in range(64)]
            m >>= 1
        assert len(set(float(x) for x in lanes)) == 1            # every lane ends with the same bits
        waves.append(lanes[0])
    return F32(F32(F32(waves[0] + waves[1]) + waves[2]) + waves[3])


def _scalar_sum(v):
    n = v.size
    nblk = -(-n // 256)
    p = np.zeros(nblk * 256, F32)
    p[:n] = v
    part = [_scalar_block(p[256 * j:256 * j + 256]) for j in range(nblk)]
    acc = []
    for t in range(256):
        a = F32(0)
        for j in range(t, nblk, 256):
            a = F32(a + part[j])
        acc.append(a)
    return _scalar_block(np.array(acc, F32)), np.array(part, F32)


@pytest.mark.parametrize("n", (1, 63, 256, 323, 256 * 257 + 5))
def test_ordered_sum_is_the_scalar_loop(n):
    rng = np.random.RandomState(n)
    v = (rng.standard_normal((2, n)) * 10.0 ** rng.uniform(-3, 3, (2, n))).astype(F32)
    part = cg_ref.block_partials(v, F32)
    tot = cg_ref.entry_sum(part, F32)
    assert part.dtype == F32 and tot.dtype == F32 and part.shape == (2, -(-n // 256))
    for e in range(2 if n < 1000 else 1):
        s, p = _scalar_sum(v[e])
        assert (_bits(part[e]) == _bits(p)).all() and _bits(tot[e]) == _bits(s)
    assert (_bits(cg_ref.ordered_dot(v, v)) == _bits(cg_ref.entry_sum(cg_ref.block_partials(v * v, F32), F32))).all()
    assert (cg_ref.ordered_amax(v) == np.abs(v).max(axis=1)).all() and cg_ref.ordered_amax(v).dtype == F32
    with pytest.raises(AssertionError):
        cg_ref.block_partials(v.astype(np.float64), F32)          # every intermediate keeps the dtype


def test_defaults_are_numpys_reductions():
    """no value of an earlier test moves: without dot= / amax= every restatement reduces as before"""
    for name in ("closed-17x19-b1", "obstacle-17x19-b1", "open-17x19-b2", "liquid-17x19-b1", "gf-17x19-b1", "diffuse-17x19-b1", "mg-17x19-b1"):
        for dt in (F32, np.float64):
            a = cc.run(name, 3, dtype=dt, dot=cg_ref.numpy_dot, amax=cg_ref.numpy_amax)
            i = cc.inputs(name)
            r = cc.BY_NAME[name]
            import diffuse_ref, liquid_gf_ref, liquid_ref, smoke_mg_ref, smoke_obs_ref, smoke_open_ref, smoke_ref
            x = {"closed": lambda: smoke_ref.cg(i["vel"], r["bnd"], 0.0, 3, dt)[0],
                 "obstacle": lambda: smoke_obs_ref.cg(i["vel"], i["obstacle"], r["bnd"], 0.0, 3, dt)[0],
                 "open": lambda: smoke_open_ref.cg(i["vel"], i["obstacle"], i["bits"], r["bnd"], 0.0, 3, dt)[0],
                 "liquid": lambda: liquid_ref.cg(i["vel"], i["liquid"], r["bnd"], 0.0, 3, dt)[0],
                 "gf": lambda: liquid_gf_ref.pcg(i["vel"], i["liquid"], i["phi"], r["bnd"], 0.0, 3, cc.GF_CLAMP, dt)[0],
                 "diffuse": lambda: diffuse_ref.cg(i["vel"], i["alpha"], r["bnd"], 0.0, 3, dt)[3],
                 "mg": lambda: smoke_mg_ref.pcg(i["vel"], i["obstacle"], i["bits"], r["bnd"], 0.0, 3, dt)[0]}[r["variant"]]()
            assert x.dtype == dt and np.array_equal(x, a["x"])


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
def test_table_covers_every_variant_and_workgroup_count():
    assert set(r["variant"] for r in cc.ROWS) == set(cc.VARIANTS)
    for nd in (2, 3):
        counts = sorted(set(cc.nblk(r) for r in cc.ROWS if len(r["shape"]) == nd))
        assert 1 in counts and 2 in counts and 256 in counts, counts
        assert any(256 < c < 512 for c in counts) and any(c > 512 for c in counts), counts
    for v in cc.VARIANTS:
        rows = [r for r in cc.ROWS if r["variant"] == v]
        assert any(cc.nblk(r) > 256 for r in rows) and any(cc.nblk(r) <= 2 for r in rows), v
        assert set(len(r["shape"]) for r in rows) == {2, 3}, v
    assert set(r["bnd"] for r in cc.ROWS) == {1, 2}
    for fam in ("closed", "obstacle", "open", "obsopen", "liquid", "gf", "diffuse", "mg"):
        assert sum(r["solve"] for r in cc.ROWS if r["variant"] == fam) >= 1, fam
    for r in cc.ROWS:
        n = int(np.prod(r["shape"]))
        assert r["B"] == 3 and (r["shape"][-1] % 4 != 0) and 1 <= min(r["ks"]) and max(r["ks"]) <= 4
        assert n <= 136000 and (n % 256 != 0 or cc.nblk(r) == 1), r["name"]       # the last workgroup is ragged
        assert not r["solve"] or cc.nblk(r) <= 2                                   # no solve to convergence at a large shape
        grid = cc.systems(r) * cc.nblk(r)
        if cc.nblk(r) % 8:                                                         # 256 workgroups: B * 256 is a multiple of 8 for every B
            assert grid % 8 != 0, r["name"]
        if cc.nblk(r) > 8:                                                         # an entry begins inside an XCD's chunk of the remap
            q, rem = grid >> 3, grid & 7
            starts = set((x * (q + 1) if x < rem else rem * (q + 1) + (x - rem) * q) for x in range(8))
            assert any(e * cc.nblk(r) not in starts for e in range(1, cc.systems(r))), r["name"]


def test_entry_points_match_the_header():
    from deep_fluids_amd import _lib
    for r in cc.ROWS:
        for kind, (name, args) in cc.entry_points(r).items():
            res, types = _lib.SIGNATURES[name]
            assert len(types) == len(args), (name, len(types), args)
            for a, t in zip(args, types):
                assert (t is _lib.P) == (a in cc.POINTERS or a == "stream"), (name, a)
                if a in ("acc", "gf_clamp", "mg_alpha"):
                    assert t is _lib.F32, (name, a)


@pytest.mark.parametrize("name", cc.names(large=True))
def test_a_workgroup_past_255_holds_a_residual(name):
    r = cc.BY_NAME[name]
    live = cc.residual_by_workgroup(name)
    assert live.shape == (cc.systems(r), cc.nblk(r))
    per = len(r["shape"]) if r["variant"] == "diffuse" else 1
    assert live[:per, 256:].any(axis=1).all(), "entry 0 of %s has no residual past workgroup 255" % name
    assert not live[per:2 * per].any()                                            # entry 1 is at rest


@pytest.mark.parametrize("name", cc.names())
def test_iteration_counts_are_the_rows(name):
    r = cc.BY_NAME[name]
    for K in r["ks"]:
        t = cc.twin(name, K)
        assert np.array_equal(t["iters"], cc.expected_iters(r, K)), (name, K, t["iters"].tolist())
        assert t["x"].dtype == F32 and t["out"].dtype == F32 and np.isfinite(t["x"]).all()
    it2 = np.max(r["it2"])
    assert 0 < it2 < max(r["ks"])
    one = cc.run(name, max(r["ks"]), entries=slice(0, 1))                           # an entry alone gives its bits in the batch
    per = len(r["shape"]) if r["variant"] == "diffuse" else 1
    assert (_bits(one["x"]) == _bits(cc.twin(name, max(r["ks"]))["x"][:per])).all()


@pytest.mark.parametrize("name", cc.names())
def test_wrong_orders_are_told_apart(name):
    r = cc.BY_NAME[name]
    K = max(r["ks"])
    per = len(r["shape"]) if r["variant"] == "diffuse" else 1
    true = _bits(cc.twin(name, K)["x"][:per])
    for mutant, dot in sorted(cc.MUTANTS.items()):
        x = _bits(cc.run(name, K, dot=dot, entries=slice(0, 1))["x"])
        if mutant in cc.LARGE_ONLY and cc.nblk(r) <= 256:
            assert (x == true).all(), (name, mutant)                                # the same sum by construction
        else:
            assert (x != true).any(), "%s cannot tell %s from the header's order" % (name, mutant)


@pytest.mark.parametrize("name", cc.names(solve=True))
def test_solve_rows_converge_with_entry_2_first(name):
    r = cc.BY_NAME[name]
    t = cc.twin(name, None, solve=True)
    it = t["iters"].reshape(r["B"], -1)
    assert (it[1] == 0).all() and (it[2] > 0).all() and (it[2] < it[0]).all() and it.max() < 400, it.tolist()
