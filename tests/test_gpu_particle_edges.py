"""-m gpu: the particle and liquid entry points -- df_particles_advect* / _cell_keys* (dense and ragged), df_particles_gather,
df_particle_levelset_union* / _averaged*, df_levelset_smooth*, df_liquid_p2g*, df_mac_extrapolate*, df_liquid_flags* / _forces*,
df_flip_update* (dense and ragged), df_levelset_extrapolate_marks* / _layer*, df_resample_count* / _scatter* -- through the raw C ABI, one
row of tests/particle_cases.py per branch of the host code and the kernels of csrc/particles.hip and csrc/liquid.hip
(tests/test_particle_cases_host.py keeps the table complete against the header and runs the restatements on every row without a GPU).  The
tests through ops.* (test_gpu_particles.py, test_gpu_liquid.py, test_gpu_liquid_gf.py, test_gpu_liquid_resample.py) run on fresh
256-byte aligned tensors and on well-formed inputs.  They do not see a record at a 4-byte aligned address, a write one record outside a
buffer, the remainder branch of the block remap (their grids give 1, 2 or 24 workgroups), or what the header promises for non-finite
positions and velocities and for out-of-range entries of order, cell_start, entry_start, new_start and seeds.

Harness: every operand and every output is a guarded buffer (gpu_util.Guarded, GuardedBytes, GuardedInts, GuardedLongs) at the row's payload
offset; outputs hold the fill pattern before the call.  After the call: return code 0, all guards intact, no fill left in any element the
header says is written and the fill intact in every element it says is not (unused ragged rows, rows at or beyond the capacity, keep bytes
of rows no cell holds), the inputs unchanged bit for bit, and a second call gives the same bits.  Hostile indices are off by at most 5
elements, inside the guard zones: nothing here relies on the device faulting.

Reference, no tolerance of its own: bit for bit the fp32 twin of the NumPy restatement for keys, gather, p2g, extrapolate, flags, forces,
flip update, marks and layer, smooth, resample count and scatter (a NaN must be a NaN; its payload is the hardware's); for the trace and
both level sets the suite's standing rule, distance to the fp64 restatement <= 3 * e32 + 1e-7 with e32 measured from the twin in the same
test.  profiles/particle_edge_tests.md holds the measured maxima.

Relations, all exact: a loose row gives the bits of its aligned twin; ragged with entry_start[b] = b*N gives the dense bits; in place gives
the bits of out of place (trace, flip update, forces, smooth mode 0); entry 0 of a B = 2 call gives the bits of entry 0 alone;
df_levelset_smooth* mode 0 with band 0 is a bit copy; keys -> torch's stable sort -> gather gives the restatement's sorted particles."""
import numpy as np
import pytest
import torch

import liquid_resample_ref as rref
import particle_cases as pc
from gpu_util import NAN_BITS, Guarded, GuardedBytes, GuardedInts, GuardedLongs, host

pytestmark = pytest.mark.gpu
KIND = {"f32": Guarded, "i32": GuardedInts, "i64": GuardedLongs, "u8": GuardedBytes}
NP = {"f32": np.float32, "i32": np.int32, "i64": np.int64, "u8": np.uint8}
# per op: its pointer arguments in the header's order; whether N follows B
ARGS = {"trace": ("pos pos_out vel es", True), "keys": ("pos keys es", True), "gather": ("pos order pos_sorted", None),
        "union": ("sp cs phi", True), "averaged": ("sp cs phi", True), "smooth": ("phi_in phi", False),
        "p2g": ("sp spvel cs vel weight known", True), "extrap": ("vel mark vel_out mark_out", False), "flags": ("cs flags touch", True),
        "forces": ("vel flags out", False), "flip": ("pos pvel pvel_out vel vel_old es", True), "marks": ("phi mark", False),
        "layer": ("phi mark", False), "count": ("sp cs phi flags keep kept seeds", True),
        "scatter": ("sp spvel cs keep seeds new_start vel pos_out pvel_out", True)}
IN_PLACE = {"trace": ("pos_out", "pos"), "flip": ("pvel_out", "pvel"), "forces": ("out", "vel"), "smooth": ("phi", "phi_in")}


@pytest.fixture(scope="module")
def k():
    """(library handle, stream)"""
    from deep_fluids_amd import _lib
    from deep_fluids_amd.ops import _stream
    return _lib.lib(), _stream()


def out_shape(r, name):
    """the extent of an output by what its elements belong to (pc.EXTENT)"""
    D, P, grid = len(r["shape"]), r["B"] * r["N"], (r["B"],) + r["shape"]
    if pc.EXTENT[name] == "row":
        return (P,) if name in ("keys", "keep") else (P, D)
    if pc.EXTENT[name] == "cell":
        return (r["B"] * int(np.prod(r["shape"])),)
    return grid if name in ("phi", "flags", "mark") else grid + (D,)


def _bits(buf):
    """the payload as the host sees it, fill included: float buffers as their int32 words"""
    return host(buf.bits[buf.lo:buf.lo + buf.n]).reshape(buf.shape)


class Call(object):
    """The guarded buffers of one row with operands ``i`` and the argument list of its entry point.  An operand of ``i["padded"]`` is
    (array, lead): the array goes into the payload and the pointer passed is ``lead`` elements into it."""

    def __init__(self, k, r, i):
        self.lib, stream = k
        self.r = r
        _, ins, outs = pc.OPS[r["op"]]
        self.kinds = dict(ins + outs)
        self.outs = [n for n, _ in outs]
        self.data, self.bufs, lead = {}, {}, {}
        for name, kind in ins:                                         # inputs, the arrays of an in-place entry point among them
            if name == "es" and not r["ragged"]:
                continue
            data, lead[name] = i.get("padded", {}).get(name, (i.get(name), 0))
            if data is None or data.size == 0:
                self.bufs[name] = None
                continue
            self.data[name] = np.ascontiguousarray(data, NP[kind])
            self.bufs[name] = KIND[kind](data.shape, self.data[name], 0 if kind == "i64" else r["off"])
        for name, kind in outs:
            if name in self.bufs:
                continue
            if name in r["null"] or int(np.prod(out_shape(r, name))) == 0:
                self.bufs[name] = None
            elif r["inplace"] and IN_PLACE[r["op"]][0] == name:
                self.bufs[name] = self.bufs[IN_PLACE[r["op"]][1]]
            else:
                self.bufs[name] = KIND[kind](out_shape(r, name), None, r["off"])
        names, has_n = ARGS[r["op"]]
        ptrs = [None if self.bufs[n] is None else self.bufs[n].ptr + lead.get(n, 0) * self.bufs[n].bits.element_size()
                for n in names.split() if n in self.bufs]
        ext = (r["B"] * r["N"], len(r["shape"])) if r["op"] == "gather" else (r["B"],) + ((r["N"],) if has_n else ()) + r["shape"]
        self.args = ptrs + list(ext) + list(pc.scalars(r)) + [stream]
        targets = set(id(self.bufs[n]) for n in self.outs)
        self.pure_inputs = [n for n in self.data if id(self.bufs[n]) not in targets]

    def reset(self):
        """every buffer as it was before the first call: inputs hold their data, outputs the fill"""
        for n, b in self.bufs.items():
            if b is None:
                continue
            if n in self.data:
                b.payload().copy_(torch.from_numpy(self.data[n].reshape(-1)).cuda())
            elif not self.r["inplace"] or IN_PLACE[self.r["op"]][0] != n:
                b.refill()

    def run(self):
        """the call; return code 0, guards intact, inputs unchanged -> {output: payload}, float outputs as int32 words, the fill still in them"""
        name = self.r["name"]
        rc = getattr(self.lib, pc.entry_point(self.r))(*self.args)
        assert rc == 0, (name, rc, self.lib.df_last_error())
        torch.cuda.synchronize()
        for n, b in self.bufs.items():
            if b is not None:
                b.check_guards("%s %s" % (name, n))
        for n in self.pure_inputs:
            want = self.data[n].view(np.int32) if self.kinds[n] == "f32" else self.data[n]
            assert (_bits(self.bufs[n]) == want).all(), "%s: the input %s was changed" % (name, n)
        return dict((n, _bits(self.bufs[n]).copy()) for n in self.outs if self.bufs[n] is not None)


def _call(k, r, i):
    """one row on the device, twice from the same state: the second call must repeat the first.  Returns the outputs of the first."""
    c = Call(k, r, i)
    first = c.run()
    c.reset()
    second = c.run()
    for n in first:
        assert (first[n] == second[n]).all(), "%s: the second call changed %s" % (r["name"], n)
    return first


_RESULTS = {}


def _run(k, r):
    if r["name"] not in _RESULTS:
        _RESULTS[r["name"]] = _call(k, r, pc.inputs(r))
    return _RESULTS[r["name"]]


def _fill_of(kind):
    return NAN_BITS if kind == "f32" else KIND[kind].fill


def _check_written(r, name, kind, got, mask, fresh):
    """no fill where the header says an element is written; the fill intact where it says it is not (``fresh``: the buffer held the fill)"""
    fill = _fill_of(kind)
    if not fresh:
        return
    left = (got == fill)
    if mask is None:
        assert not left.any(), "%s: %d of %d elements of %s were never written" % (r["name"], int(left.sum()), left.size, name)
    else:
        assert not left[mask].any(), "%s: %d elements of %s were never written" % (r["name"], int(left[mask].sum()), name)
        assert left[~mask].all(), "%s: %d elements of %s that must stay as they were have been written" % (r["name"], int((~left[~mask]).sum()), name)


def _same_bits(r, name, got_words, want, mask):
    """bit for bit on the written elements; where the twin holds a NaN the kernel must hold one (the payload is the hardware's)"""
    want = np.ascontiguousarray(want, np.float32)
    got = got_words.view(np.float32)
    sel = np.ones(want.shape, bool) if mask is None else mask
    nan = np.isnan(want)
    bad = sel & np.where(nan, ~np.isnan(got), got_words != want.view(np.int32))
    if bad.any():
        at = np.unravel_index(int(np.argmax(bad)), bad.shape)
        raise AssertionError("%s %s: %d of %d elements differ, first at %s: got %r, want %r" % (r["name"], name, int(bad.sum()), bad.size, at,
                                                                                                got[at], want[at]))


def _within_rule(r, name, got_words, w32, w64, mask):
    """the suite's standing rule: distance to the fp64 restatement <= 3 * e32 + 1e-7, e32 the twin's; non-finite values must agree exactly"""
    got = got_words.view(np.float32).astype(np.float64)
    w32, w64 = np.asarray(w32, np.float64), np.asarray(w64, np.float64)
    sel = np.ones(w64.shape, bool) if mask is None else mask
    fin = sel & np.isfinite(w64)
    odd = sel & ~np.isfinite(w64)
    assert (np.isnan(got[odd]) == np.isnan(w64[odd])).all() and (got[odd][~np.isnan(w64[odd])] == w64[odd][~np.isnan(w64[odd])]).all(), \
        "%s %s: a non-finite value of the restatement is another one on the device" % (r["name"], name)
    assert np.isfinite(got[fin]).all(), "%s %s: non-finite where the restatement is finite" % (r["name"], name)
    e32 = float(np.abs(w32[fin] - w64[fin]).max()) if fin.any() and np.isfinite(w32[fin]).all() else 0.0
    d = float(np.abs(got[fin] - w64[fin]).max()) if fin.any() else 0.0
    print("%-34s %-10s e32 %.3e  gpu-f64 %.3e  bound %.3e" % (r["name"], name, e32, d, 3 * e32 + 1e-7))
    assert d <= 3 * e32 + 1e-7, (r["name"], name, d, e32)


def _check_row(k, r):
    got = _run(k, r)
    e32 = pc.expected(r, np.float32)
    kinds = dict(pc.OPS[r["op"]][2])
    ins = set(n for n, _ in pc.OPS[r["op"]][1])
    for name, words in got.items():
        want, mask = e32[name]
        assert words.shape == tuple(np.shape(want)), (r["name"], name, words.shape, np.shape(want))
        fresh = name not in ins and not (r["inplace"] and IN_PLACE[r["op"]][0] == name)
        _check_written(r, name, kinds[name], words, mask, fresh)
        if kinds[name] != "f32":
            sel = np.ones(words.shape, bool) if mask is None else mask
            bad = sel & (words != np.asarray(want).astype(words.dtype))
            assert not bad.any(), "%s %s: %d of %d elements differ, first at %s" % (r["name"], name, int(bad.sum()), bad.size,
                                                                                   np.unravel_index(int(np.argmax(bad)), bad.shape))
        elif r["op"] in pc.TOLERANCE_OPS and r["N"] > 0:          # N = 0: phi is the radius bit for bit
            _within_rule(r, name, words, want, pc.expected(r, np.float64)[name][0], mask)
        else:
            _same_bits(r, name, words, want, mask)
    for name in r["null"]:
        assert name not in got
    return got


def _equal(a, b, what):
    assert set(a) == set(b), what
    for n in a:
        assert a[n].shape == b[n].shape and (a[n] == b[n]).all(), "%s: %s differs in %d elements" % (what, n, int((a[n] != b[n]).sum()))


@pytest.mark.parametrize("name", pc.names())
def test_row(k, name):
    r = pc.BY_NAME[name]
    got = _check_row(k, r)
    if r["twin"]:                                              # a loose row gives the bits of its aligned twin
        _equal(got, _run(k, pc.BY_NAME[r["twin"]]), "%s against %s" % (name, r["twin"]))
    if r["inplace"]:                                           # in place gives the bits of out of place
        other = dict(r, name=name + "/apart", inplace=False, twin=name)
        _equal(got, _call(k, other, pc.inputs(r)), "%s against out of place" % name)
    if r["ragged"] == "dense":                                 # entry_start[b] = b*N gives the dense bits
        i = dict(pc.inputs(r), es=None)
        _equal(got, _call(k, dict(r, name=name + "/dense", ragged=None), i), "%s against the dense entry point" % name)
    if r["op"] == "smooth" and r["mode"] == 0 and r["band"] == 0:
        assert (got["phi"] == pc.inputs(r)["phi_in"].view(np.int32)).all(), "%s: mode 0 with band 0 is a bit copy" % name


def _entry0(name, a, N, ncell):
    """the part of an operand that belongs to entry 0, by what its elements belong to"""
    return {"row": a[:N], "entry": a[:1], "cell": a[:ncell], "range": a[:ncell + 1], None: None}[pc.EXTENT[name]]


@pytest.mark.parametrize("name", [n for n in pc.names(axes="odd,B2") if pc.BY_NAME[n]["op"] != "gather"])
def test_entry0_alone(k, name):
    """entry 0 of a B = 2 call gives the bits of entry 0 alone (the header: the result of a batch entry does not depend on the rest)"""
    r = pc.BY_NAME[name]
    i, N, ncell = pc.inputs(r), r["N"], int(np.prod(r["shape"]))
    one = dict((n, _entry0(n, v, N, ncell)) for n, v in i.items() if n in pc.EXTENT and isinstance(v, np.ndarray))
    # the rows of entry 0 that a resampling call touches: its live rows (count), its resampled rows (scatter); both fit its own capacity
    rows = {"count": lambda: int(i["cs"][ncell]), "scatter": lambda: int(i["new_start"][ncell])}.get(r["op"], lambda: N)()
    assert rows <= N
    both = _run(k, r)
    alone = _call(k, dict(r, name=name + "/entry0", B=1), one)
    for n, a in alone.items():
        b = _entry0(n, both[n], N, ncell)
        if pc.EXTENT[n] == "row":
            a, b = a[:rows], b[:rows]
        assert a.shape == b.shape and (a == b).all(), "%s: %s of entry 0 depends on entry 1 (%d elements)" % (name, n, int((a != b).sum()))


@pytest.mark.parametrize("dim", (2, 3))
def test_keys_sort_gather_chain(k, dim):
    """the caller's part between keys and gather, as the library's own driver does it: torch's stable sort of the kernel's keys, the kernel's
    gather with that order, searchsorted ranges -- against the restatement's sorted particles and ranges"""
    r = pc.BY_NAME["keys-%dd-hostile-pos" % dim]
    i = pc.inputs(r)
    P, D = i["pos"].shape
    keys = torch.from_numpy(_run(k, r)["keys"].astype(np.int32)).cuda()
    skeys, order = torch.sort(keys, stable=True)
    g = dict(r, name=r["name"] + "/gather", op="gather", B=1, N=P)
    out = _call(k, g, dict(pos=i["pos"], order=host(order)))["pos_sorted"]
    es = (np.arange(r["B"] + 1) * r["N"]).astype(np.int32)
    sp, _, cs, ref_order = rref.sort(i["pos"], None, es, r["shape"])
    assert (host(order) == ref_order).all()
    assert (out == sp.view(np.int32)).all()
    ncell = r["B"] * int(np.prod(r["shape"]))
    got_cs = torch.searchsorted(skeys, torch.arange(ncell + 1, dtype=torch.int32, device="cuda"))
    assert (host(got_cs) == cs).all()
