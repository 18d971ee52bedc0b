"""The case table of tests/test_gpu_wino_edges.py (GPU) and tests/test_wino_cases_host.py (no GPU): one row per branch of the host code and
of the epilogues of csrc/conv_wino.hip, csrc/conv_wino43.hip, csrc/conv_wino2d.hip and csrc/conv_wino2d43.hip.  Data only; imports nothing.

Tile geometry the rows rest on: a tile block is 16 x 32 pixels (2-D) or 4 x 8 x 8 voxels (3-D), a cout slice 32 channels, a cin chunk 16
channels; tiles are 2 x 2, 2 x 4, 2 x 2 x 2 or 2 x 2 x 4 outputs.  The kernels are persistent: a grid of at most 256 workgroups walks the
(tile block, cout slice) items in one of three worker mappings -- XCD-pinned with one slice per XCD (1 slice), XCD-pinned with two (2, 4, 8
slices), generic (3, 5, 6, 7, more than 8 slices) -- and one pass of the grid covers 256 / 128 / 64 / 32 tile blocks for 1 / 2 / 4 / 8 slices,
256 // ncs for the generic mapping.

A row is a dict:
  id, entry   entry = the recorder's name of the entry point (ENTRIES[entry]["fn"] is the C name)
  shape       (B, H, W) | (B, D, H, W) as the entry point takes them: the COARSE grid of the up-sampling forms and of the backward tails
  cin, cout   as the entry point takes them (the tails: cin = C)
  flags       as the entry point takes them (0 where it has no flags argument)
  mode        the pack mode of wp (1: the call is a dgrad; the layer's weights are [taps, cout, cin] of this call)
  ops         bit mask over SLOTS of the operands the call passes; every other one is NULL
  off         payload offset in floats per slot: 0 = 16-byte aligned, 1 = 4-byte aligned only
  reaches     (kernel family, FL, MODE) of the one instantiation the call launches, or the negative DF_E* code it must return without
              launching anything.  OBSERVED without a GPU: tests/test_wino_cases_host.py runs every row through tests/wgrad_launch_recorder.cpp
  twin        id of the row with the same arguments and data whose outputs must have the same bits (a loose operand against all aligned;
              mask words against the fp32 activation they were taken from; an entry point that does not write y against the one that does)
  passes      multi-pass rows: (ntb, tile blocks per pass of the grid): the first ntb - per_pass workers of the first pass run two
              iterations, all others one"""

LRELU, RESIDUAL, MASK, BIAS, ADDUP = 1, 2, 4, 8, 16
EINVAL, ESHAPE, EALIGN = -1, -2, -3
SLOTS = ("x", "wp", "bias", "res", "msrc", "mbits", "y", "y2", "sbits")      # res: the fine residual, or the coarse xc of the add-up forms
X, WP, FBIAS, RES, MSRC, MBITS, Y, Y2, SBITS = (1 << i for i in range(9))       # (the tails: x = gy, y = gx, y2 = gpool)
KSIGN, KMASK, KNOY = 64, 128, 256      # the internal epilogue flags of the kernels (sign words out, mask words in, y not written)

# Per entry point: C name, dimensionality, kernel family, form (conv | addup | up_fwd | up_dgrad | tail), the flags and operands of a call it
# accepts, the operands it needs, those whose 16-byte alignment it checks and those it does not (read / written with scalar accesses)
ENTRIES = {
    "wino_fwd": dict(fn="df_wino_conv_fwd", nd=3, fam="wino3d", form="conv", flags=9, ops=X | WP | FBIAS | Y, need=X | WP | Y, aligned=X | WP | Y,
                     loose=FBIAS | RES | MSRC),
    "wino_fwd_bits": dict(fn="df_wino_conv_fwd_bits", nd=3, fam="wino3d", form="conv", flags=9, ops=X | WP | FBIAS | Y | SBITS, need=X | WP | Y,
                          aligned=X | WP | Y | SBITS | MBITS, loose=FBIAS),
    "wino_fwd_addup": dict(fn="df_wino_conv_fwd_addup", nd=3, fam="wino3d", form="addup", flags=0, ops=X | WP | FBIAS | RES | Y | Y2,
                           need=X | WP | FBIAS | RES | Y | Y2, aligned=X | WP, loose=FBIAS | RES | Y | Y2),
    "wino_fwd_addup_bits": dict(fn="df_wino_conv_fwd_addup_bits", nd=3, fam="wino3d", form="addup", flags=0, ops=X | WP | FBIAS | RES | Y2 | SBITS,
                                need=X | WP | FBIAS | RES | Y2 | SBITS, aligned=X | WP | SBITS, loose=FBIAS | RES | Y2),
    "wino_upconv_fwd": dict(fn="df_wino_upconv_fwd", nd=3, fam="wino3d", form="up_fwd", flags=9, ops=X | WP | FBIAS | Y, need=X | WP | FBIAS | Y,
                            aligned=X | WP | Y, loose=FBIAS),
    "wino_upconv_fwd_bits": dict(fn="df_wino_upconv_fwd_bits", nd=3, fam="wino3d", form="up_fwd", flags=0, ops=X | WP | FBIAS | Y | SBITS,
                                 need=X | WP | FBIAS | Y | SBITS, aligned=X | WP | Y | SBITS, loose=FBIAS),
    "wino_upconv_dgrad": dict(fn="df_wino_upconv_dgrad", nd=3, fam="wino3d", form="up_dgrad", flags=0, ops=X | WP | Y, need=X | WP | Y, aligned=X | WP,
                              loose=Y),
    "wino43": dict(fn="df_wino43_conv", nd=3, fam="wino43", form="conv", flags=9, ops=X | WP | FBIAS | Y, need=X | WP | Y,
                   aligned=X | WP | Y | Y2 | MBITS | SBITS, loose=FBIAS | RES | MSRC),
    "w2_fwd": dict(fn="df_wino2d_conv_fwd", nd=2, fam="wino2d", form="conv", flags=9, ops=X | WP | FBIAS | Y, need=X | WP | Y, aligned=X | WP,
                   loose=FBIAS | RES | MSRC | Y),
    "w2_up_fwd": dict(fn="df_wino2d_upconv_fwd", nd=2, fam="wino2d", form="up_fwd", flags=9, ops=X | WP | FBIAS | Y, need=X | WP | FBIAS | Y,
                      aligned=X | WP, loose=FBIAS | Y),
    "w2_up_dgrad": dict(fn="df_wino2d_upconv_dgrad", nd=2, fam="wino2d", form="up_dgrad", flags=0, ops=X | WP | Y, need=X | WP | Y, aligned=X | WP,
                        loose=Y),
    "w2_43": dict(fn="df_wino2d43_conv", nd=2, fam="wino2d43", form="conv", flags=9, ops=X | WP | FBIAS | Y, need=X | WP | Y,
                  aligned=X | WP | RES | MSRC | Y, loose=FBIAS),
    "w2_43_bits": dict(fn="df_wino2d43_conv_bits", nd=2, fam="wino2d43", form="conv", flags=9, ops=X | WP | FBIAS | Y | SBITS, need=X | WP | Y,
                       aligned=X | WP | Y | MBITS | SBITS, loose=FBIAS),
    "w2_43_addup_bits": dict(fn="df_wino2d43_conv_addup_bits", nd=2, fam="wino2d43", form="addup", flags=0, ops=X | WP | FBIAS | RES | Y2 | SBITS,
                             need=X | WP | FBIAS | RES | Y2 | SBITS, aligned=X | WP | RES | Y2 | SBITS, loose=FBIAS),
    "wino_bits_bwd": dict(fn="df_lrelu_bits_bwd_pool2x", nd=3, fam="bits_bwd", form="tail", flags=0, ops=X | MBITS | Y | Y2, need=X | MBITS | Y | Y2,
                          aligned=X | MBITS | Y | Y2, loose=0),
    "w2_words_bwd": dict(fn="df_lrelu_words2d_bwd_pool2x", nd=2, fam="words2d_bwd", form="tail", flags=0, ops=X | MBITS | Y | Y2,
                         need=X | MBITS | Y | Y2, aligned=X | MBITS | Y | Y2, loose=0),
}
CONVS = [e for e in ENTRIES if ENTRIES[e]["form"] != "tail"]
# the kernel families of the four files as `nm -C` prints their templates; tests/test_wino_cases_host.py lists the library's instantiations
FAMILIES = {"wino3d": "wino3d_kernel<", "wino43": "wino43_kernel<", "wino2d": "wino2d_kernel<", "wino2d43": "wino2d43_kernel<"}
TAILS = {"bits_bwd": "lrelu_bits_bwd_pool_kernel", "words2d_bwd": "lrelu_words2d_bwd_pool_kernel"}


def kernel(entry, flags, ops):
    """the instantiation an ACCEPTED call reaches: the host dispatch of the four files restated"""
    e = ENTRIES[entry]
    fam = e["fam"]
    if e["form"] == "tail":
        return (fam, 0, 0)
    if entry in ("wino_fwd", "w2_fwd", "w2_43"):
        own = (9, 4, 2, 0) if entry == "wino_fwd" else (9, 4, 2)
        return (fam, flags if flags in own else -1, 0)
    if entry in ("wino_fwd_bits", "w2_43_bits"):
        return (fam, 9 | KSIGN if ops & SBITS else 4 | KMASK, 0)
    if entry == "wino_fwd_addup":
        return (fam, 25, 0)
    if entry in ("wino_fwd_addup_bits", "w2_43_addup_bits"):
        return (fam, 25 | KSIGN | KNOY, 0)
    if entry in ("wino_upconv_fwd", "wino_upconv_fwd_bits"):
        return (fam, 9 | (KSIGN if ops & SBITS else 0), 3)
    if entry == "w2_up_fwd":
        return (fam, 9, 1)
    if entry in ("wino_upconv_dgrad", "w2_up_dgrad"):
        return (fam, 0, 2)
    assert entry == "wino43", entry
    f = flags | (KSIGN if ops & SBITS else 0) | (KMASK if ops & MBITS else 0) | (0 if ops & Y else KNOY)
    return (fam, f if f in (9, 73, 132, 4, 2, 0, 25, 345) else -1, 0)


ROWS = []


def row(rid, entry, shape, cin, cout, flags=None, ops=None, mis=0, reaches=None, mode=0, twin=None, passes=None):
    e = ENTRIES[entry]
    flags = e["flags"] if flags is None else flags
    ops = e["ops"] if ops is None else ops
    assert len(shape) == e["nd"] + 1 and not (mis & ~ops), rid
    r = dict(id=rid, entry=entry, shape=tuple(shape), cin=cin, cout=cout, flags=flags, ops=ops, mis=mis, mode=mode, twin=twin, passes=passes,
             off=dict((s, (mis >> i) & 1) for i, s in enumerate(SLOTS)), reaches=kernel(entry, flags, ops) if reaches is None else reaches)
    ROWS.append(r)
    return r


def ops_of(entry, flags, bits=None):
    """the operands of an accepted call with these flags: bits = "s" sign words out, "m" mask words in, "noy" add-up without y"""
    o = X | WP | Y
    if flags & BIAS:
        o |= FBIAS
    if flags & (RESIDUAL | ADDUP):
        o |= RES
    if flags & MASK:
        o |= MBITS if bits == "m" else MSRC
    if flags & ADDUP:
        o |= Y2
    if bits in ("s", "noy"):
        o |= SBITS
    if bits == "noy":
        o &= ~Y
    return o


def coarse(shape):
    """the coarse extents of an up-sampling form whose fine grid covers `shape`: halved, rounded up where odd"""
    return (shape[0],) + tuple((v + 1) // 2 for v in shape[1:])


# the extents every family runs: smaller than one tile, exactly one tile block, one row / column past every block edge, two ragged images, odd
EXT = {2: [(1, 1, 1), (1, 16, 32), (1, 17, 33), (2, 15, 31), (1, 10, 12)],
       3: [(1, 1, 1, 1), (1, 4, 8, 8), (1, 5, 9, 9), (2, 3, 7, 7), (1, 5, 7, 9)]}
EXT_ADDUP = {2: [(1, 2, 2), (1, 16, 32), (1, 18, 34), (2, 14, 30)], 3: [(1, 2, 2, 2), (1, 4, 8, 8), (1, 6, 10, 10), (2, 2, 6, 6)]}      # even
RAGGED = {2: (1, 17, 33), 3: (1, 5, 9, 9)}
FULL = {2: (1, 16, 32), 3: (1, 4, 8, 8)}
RAGGED_EVEN = {2: (1, 18, 34), 3: (1, 6, 10, 10)}
CHANNELS = [(32, 32), (96, 32), (32, 96), (160, 64), (64, 256), (128, 128)]      # 6 chunks, Cin != Cout | generic mapping | 10 chunks | 8 slices


def _tag(shape):
    return "x".join(str(v) for v in shape)


# ---- every instantiation, at a ragged and at a full tile block (the epilogues have one branch for each) ----------------------------------------
# (entry, tag, flags, ops, mode); the -1 instantiations run with every flag the kernel tests at run time: 0 (2-D), BIAS, all four, and for
# df_wino43_conv ADDUP alone, with BIAS, with BIAS | LRELU | MASK
VARIANTS = [
    ("wino_fwd", "fl0", 0, None, 0), ("wino_fwd", "fl2", 2, None, 0), ("wino_fwd", "fl4", 4, None, 1), ("wino_fwd", "fl9", 9, None, 0),
    ("wino_fwd", "rt8", 8, None, 0), ("wino_fwd", "rt15", 15, None, 0),
    ("wino_fwd_bits", "fl73", 9, "s", 0), ("wino_fwd_bits", "fl132", 4, "m", 1),
    ("wino43", "fl0", 0, None, 0), ("wino43", "fl2", 2, None, 0), ("wino43", "fl4", 4, None, 1), ("wino43", "fl9", 9, None, 0),
    ("wino43", "fl73", 9, "s", 0), ("wino43", "fl132", 4, "m", 1), ("wino43", "rt8", 8, None, 0), ("wino43", "rt15", 15, None, 0),
    ("w2_fwd", "fl2", 2, None, 0), ("w2_fwd", "fl4", 4, None, 1), ("w2_fwd", "fl9", 9, None, 0),
    ("w2_fwd", "rt0", 0, None, 0), ("w2_fwd", "rt8", 8, None, 0), ("w2_fwd", "rt15", 15, None, 0),
    ("w2_43", "fl2", 2, None, 0), ("w2_43", "fl4", 4, None, 1), ("w2_43", "fl9", 9, None, 0),
    ("w2_43", "rt0", 0, None, 0), ("w2_43", "rt8", 8, None, 0), ("w2_43", "rt15", 15, None, 0),
    ("w2_43_bits", "fl73", 9, "s", 0), ("w2_43_bits", "fl132", 4, "m", 1),
]
MASK_TWIN = {"wino_fwd_bits": "wino_fwd", "wino43": "wino43", "w2_43_bits": "w2_43"}      # the fp32-mask call of a mask-words call
for entry, tag, fl, bits, mode in VARIANTS:
    nd = ENTRIES[entry]["nd"]
    for where, shape in (("ragged", RAGGED[nd]), ("full", FULL[nd])):
        twin = "%s-fl4-%s" % (MASK_TWIN[entry], where) if bits == "m" else None
        row("%s-%s-%s" % (entry, tag, where), entry, shape, 32, 32, fl, ops_of(entry, fl, bits), mode=mode, twin=twin)
# the add-up forms (even extents): the run-time-flags instantiation of df_wino43_conv with ADDUP in both branches
ADDUP_VARIANTS = [("wino_fwd_addup", "fl25", 0, None), ("wino_fwd_addup_bits", "fl345", 0, None), ("wino43", "fl25", 25, None), ("wino43", "fl345", 25, "noy"),
                  ("wino43", "rt16", 16, None), ("wino43", "rt24", 24, None), ("wino43", "rt29", 29, None), ("w2_43_addup_bits", "fl345", 0, None)]
NOY_TWIN = {"wino_fwd_addup_bits": "wino_fwd_addup-fl25", "wino43": "wino43-fl25", "w2_43_addup_bits": None}      # (2-D: no entry point writes y and y2)
for entry, tag, fl, bits in ADDUP_VARIANTS:
    nd = ENTRIES[entry]["nd"]
    for where, shape in (("ragged", RAGGED_EVEN[nd]), ("full", FULL[nd])):
        noy = tag == "fl345"
        ops = ops_of(entry, fl, bits) if entry == "wino43" else None
        row("%s-%s-%s" % (entry, tag, where), entry, shape, 32, 32, fl, ops, twin="%s-%s" % (NOY_TWIN[entry], where) if noy and NOY_TWIN[entry] else None)
for entry in ("wino_upconv_fwd", "wino_upconv_fwd_bits", "wino_upconv_dgrad", "w2_up_fwd", "w2_up_dgrad"):
    nd = ENTRIES[entry]["nd"]
    for where, shape in (("ragged", RAGGED[nd]), ("full", FULL[nd])):
        row("%s-%s" % (entry, where), entry, coarse(shape), 32, 32)

# ---- extents: every family's plain call, its masked dgrad and the up-sampling forms at every extent; the add-up forms at the even ones --------
EPI = (9, 0, 15, 2, 8)
for nd in (2, 3):
    for i, shape in enumerate(EXT[nd]):
        if shape in (RAGGED[nd], FULL[nd]):      # (run above with every variant)
            continue
        for entry in ("w2_fwd", "w2_43") if nd == 2 else ("wino_fwd", "wino43"):
            fl = EPI[i]
            row("%s-ext-%s" % (entry, _tag(shape)), entry, shape, 32, 32, fl, ops_of(entry, fl))
            row("%s-ext-%s-dgrad" % (entry, _tag(shape)), entry, shape, 32, 32, 4, ops_of(entry, 4), mode=1)
        for entry in ("w2_43_bits",) if nd == 2 else ("wino_fwd_bits",):
            row("%s-ext-%s" % (entry, _tag(shape)), entry, shape, 32, 32)
    for shape in sorted(set(coarse(s) for s in EXT[nd])):
        if shape in (coarse(RAGGED[nd]), coarse(FULL[nd])):
            continue
        for entry in ("w2_up_fwd", "w2_up_dgrad") if nd == 2 else ("wino_upconv_fwd", "wino_upconv_fwd_bits", "wino_upconv_dgrad"):
            row("%s-ext-%s" % (entry, _tag(shape)), entry, shape, 32, 32)
    for shape in EXT_ADDUP[nd]:
        if shape in (RAGGED_EVEN[nd], FULL[nd]):
            continue
        for entry, tag, fl, bits in ADDUP_VARIANTS:
            if ENTRIES[entry]["nd"] == nd and tag in ("fl25", "fl345", "rt29"):
                row("%s-%s-ext-%s" % (entry, tag, _tag(shape)), entry, shape, 32, 32, fl, ops_of(entry, fl, bits) if entry == "wino43" else None,
                    twin="%s-ext-%s" % (NOY_TWIN[entry], _tag(shape)) if tag == "fl345" and NOY_TWIN[entry] else None)

# ---- channels: chunk counts 2 .. 10, every worker mapping by its slice count; the dgrads swap Cin and Cout ------------------------------------
for cin, cout in CHANNELS[1:]:
    for nd in (2, 3):
        shape = (2, 15, 31) if nd == 2 else (2, 3, 7, 7)
        for entry in ("w2_fwd", "w2_43") if nd == 2 else ("wino_fwd", "wino43"):
            row("%s-c%d-%d" % (entry, cin, cout), entry, shape, cin, cout)
        up = (("w2_up_fwd", "w2_up_dgrad") if nd == 2 else ("wino_upconv_fwd", "wino_upconv_dgrad")) if (cin, cout) in ((96, 32), (32, 96)) else ()
        for entry in up:
            row("%s-c%d-%d" % (entry, cin, cout), entry, coarse(shape), cin, cout)
# a masked dgrad whose own channel count (96 in, 32 out) differs from ... and equals (the mask has the call's Cout channels) the masked tensor's
for entry, bits, twin in (("wino_fwd", None, None), ("wino_fwd_bits", "m", "wino_fwd"), ("wino43", None, None), ("wino43", "m", "wino43"),
                          ("w2_fwd", None, None), ("w2_43", None, None), ("w2_43_bits", "m", "w2_43")):
    nd = ENTRIES[entry]["nd"]
    for cin, cout in ((96, 32), (32, 96)):
        row("%s-dgrad%s-c%d-%d" % (entry, "-words" if bits else "", cin, cout), entry, (2, 15, 31) if nd == 2 else (2, 3, 7, 7), cin, cout, 4,
            ops_of(entry, 4, bits), mode=1, twin="%s-dgrad-c%d-%d" % (twin, cin, cout) if twin else None)

# ---- multi-pass: a worker walks more than one tile block, and not every worker equally many -------------------------------------------------------
# a small ragged image of two tile blocks (3 x 33 | 3 x 5 x 9), the batch chosen so that ntb is just over one pass of the grid; 8 slices: the
# 12-block images 17 x 161 | 5 x 9 x 17.            (cout, batch, ntb, tile blocks per pass)
MULTI = {2: ((3, 33), (17, 161)), 3: ((3, 5, 9), (5, 9, 17))}
for nd in (2, 3):
    two, twelve = MULTI[nd]
    for cout, img, B, ntb, per in ((32, two, 129, 258, 256), (64, two, 65, 130, 128), (256, twelve, 3, 36, 32), (96, two, 43, 86, 85)):
        for entry in ("w2_fwd", "w2_43") if nd == 2 else ("wino_fwd", "wino43"):
            row("%s-multipass-ncs%d" % (entry, cout // 32), entry, (B,) + img, 32, cout, passes=(ntb, per))
MULTIPASS = [r["id"] for r in ROWS if r["passes"]]

# ---- loose operands: every operand whose alignment the host does not check, one at a time at offset 1, on a ragged and on a full block --------
LOOSE = [("w2_fwd", 15, None, FBIAS | RES | MSRC | Y), ("w2_up_fwd", 9, None, FBIAS | Y), ("w2_up_dgrad", 0, None, Y),
         ("wino_fwd", 15, None, FBIAS | RES | MSRC), ("wino_fwd_addup", 0, None, FBIAS | RES | Y | Y2), ("wino_fwd_addup_bits", 0, None, FBIAS | RES | Y2),
         ("wino_upconv_dgrad", 0, None, Y), ("wino43", 15, None, FBIAS | RES | MSRC), ("wino43", 25, None, FBIAS | RES),
         ("wino_fwd_bits", 9, "s", FBIAS), ("wino_upconv_fwd", 9, None, FBIAS), ("wino_upconv_fwd_bits", 0, None, FBIAS), ("w2_43", 9, None, FBIAS),
         ("w2_43_bits", 9, "s", FBIAS), ("w2_43_addup_bits", 0, None, FBIAS)]
for entry, fl, bits, slots in LOOSE:
    e = ENTRIES[entry]
    nd, form = e["nd"], e["form"]
    assert not (slots & e["aligned"]) and not (slots & ~e["loose"]), entry
    addup = form == "addup" or bool(fl & ADDUP)
    for where, shape in (("ragged", RAGGED_EVEN[nd] if addup else RAGGED[nd]), ("full", FULL[nd])):
        if form in ("up_fwd", "up_dgrad"):
            shape = coarse(shape)
        ops = ops_of(entry, fl, bits) if entry in ("wino_fwd", "wino_fwd_bits", "wino43", "w2_fwd", "w2_43", "w2_43_bits") else None
        base = "%s-loose%d-%s" % (entry, fl, where)
        row(base, entry, shape, 32, 64, fl, ops)
        for i, s in enumerate(SLOTS):
            if slots & (1 << i):
                row("%s-%s1" % (base, s), entry, shape, 32, 64, fl, ops, mis=1 << i, twin=base)

# ---- the backward tails: ragged fine extents (coarse extents given), a coarse 1 x 1 (x 1), 1 and 3 cout slices --------------------------------
for shape, c in (((1, 1, 1), 32), ((2, 5, 9), 96), ((1, 8, 16), 32), ((1, 9, 17), 64)):
    row("w2_words_bwd-%s-c%d" % (_tag(shape), c), "w2_words_bwd", shape, c, c)
for shape, c in (((1, 1, 1, 1), 32), ((2, 3, 5, 5), 96), ((1, 2, 4, 4), 32), ((1, 3, 2, 5), 64)):
    row("wino_bits_bwd-%s-c%d" % (_tag(shape), c), "wino_bits_bwd", shape, c, c)

OK_ROWS = list(ROWS)

# ---- error rows: a code, no launch, every output untouched --------------------------------------------------------------------------------------
for entry, e in ENTRIES.items():
    nd, tail = e["nd"], e["form"] == "tail"
    small = (2, 10, 12) if nd == 2 else (2, 6, 10, 12)
    for i, s in enumerate(SLOTS):
        if e["need"] & (1 << i):
            row("err-%s-null-%s" % (entry, s), entry, small, 32, 64, ops=e["ops"] & ~(1 << i), reaches=EINVAL)
        if e["ops"] & e["aligned"] & (1 << i):
            row("err-%s-misaligned-%s" % (entry, s), entry, small, 32, 64, mis=1 << i, reaches=EALIGN)
    for i in range(nd + 1):
        row("err-%s-zero-extent%d" % (entry, i), entry, tuple(0 if j == i else v for j, v in enumerate(small)), 32, 64, reaches=EINVAL)
    row("err-%s-negative-extent" % entry, entry, small[:-2] + (-10, 12), 32, 64, reaches=EINVAL)
    for cin, cout in ((48, 64), (0, 64), (-32, 64)) + (() if tail else ((32, 80), (32, 0))):
        row("err-%s-channels-%d-%d" % (entry, cin, cout), entry, small, cin, cout, reaches=ESHAPE)
    if e["form"] == "addup":
        for i in range(1, nd + 1):
            row("err-%s-odd-extent%d" % (entry, i), entry, tuple(v + 1 if j == i else v for j, v in enumerate(small)), 32, 64, reaches=EINVAL)
    if not tail:      # more than 256 cout slices: no worker of the 256-workgroup grid is left for some (the dgrads' slices are the entry point's Cin)
        cc = (8224, 32) if e["form"] == "up_dgrad" else (32, 8224)
        row("err-%s-cout-slices-over" % entry, entry, small, cc[0], cc[1], reaches=ESHAPE)
# operands the alignment check of an entry point reaches only with other flags than its base call's
row("err-wino_fwd_bits-misaligned-mbits", "wino_fwd_bits", (2, 6, 10, 12), 32, 64, 4, X | WP | MBITS | Y, mis=MBITS, reaches=EALIGN)
for s, fl, ops in ((MBITS, 4, X | WP | MBITS | Y), (SBITS, 9, X | WP | FBIAS | Y | SBITS), (Y2, 25, X | WP | FBIAS | RES | Y | Y2)):
    row("err-wino43-misaligned-%s" % SLOTS[s.bit_length() - 1], "wino43", (2, 6, 10, 12), 32, 64, fl, ops, mis=s, reaches=EALIGN)
for s, fl in ((RES, 2), (MSRC, 4)):
    row("err-w2_43-misaligned-%s" % SLOTS[s.bit_length() - 1], "w2_43", (2, 10, 12), 32, 64, fl, ops_of("w2_43", fl), mis=s, reaches=EALIGN)
row("err-w2_43_bits-misaligned-mbits", "w2_43_bits", (2, 10, 12), 32, 64, 4, X | WP | MBITS | Y, mis=MBITS, reaches=EALIGN)
# flags without their operands, operands without their flags, flags an entry point does not take
for entry in ("wino_fwd", "wino43", "w2_fwd", "w2_43"):
    small = (2, 10, 12) if ENTRIES[entry]["nd"] == 2 else (2, 6, 10, 12)
    row("err-%s-bias-without" % entry, entry, small, 32, 64, 9, X | WP | Y, reaches=EINVAL)
    row("err-%s-residual-without" % entry, entry, small, 32, 64, 2, X | WP | Y, reaches=EINVAL)
    row("err-%s-mask-without" % entry, entry, small, 32, 64, 4, X | WP | Y, reaches=EINVAL)
row("err-wino_fwd-addup-flag", "wino_fwd", (2, 6, 10, 12), 32, 64, 25, X | WP | FBIAS | RES | Y, reaches=EINVAL)
row("err-w2_43-addup-flag", "w2_43", (2, 10, 12), 32, 64, 25, X | WP | FBIAS | RES | Y, reaches=EINVAL)
row("err-w2_43-unknown-flag", "w2_43", (2, 10, 12), 32, 64, 9 | 32, reaches=EINVAL)
row("err-wino43-unknown-flag", "wino43", (2, 6, 10, 12), 32, 64, 9 | 32, reaches=EINVAL)
row("err-wino43-addup-without-coarse", "wino43", (2, 6, 10, 12), 32, 64, 25, X | WP | FBIAS | Y | Y2, reaches=EINVAL)
row("err-wino43-residual-and-addup", "wino43", (2, 6, 10, 12), 32, 64, 27, X | WP | FBIAS | RES | Y | Y2, reaches=EINVAL)
row("err-wino43-addup-without-y2", "wino43", (2, 6, 10, 12), 32, 64, 25, X | WP | FBIAS | RES | Y, reaches=EINVAL)
row("err-wino43-addup-odd-d", "wino43", (2, 7, 10, 12), 32, 64, 25, X | WP | FBIAS | RES | Y | Y2, reaches=EINVAL)
row("err-wino43-mask-both", "wino43", (2, 6, 10, 12), 32, 64, 4, X | WP | MSRC | MBITS | Y, reaches=EINVAL)
row("err-wino43-no-y-no-addup", "wino43", (2, 6, 10, 12), 32, 64, 9, X | WP | FBIAS | Y2 | SBITS, reaches=EINVAL)
row("err-wino43-no-y-no-bits", "wino43", (2, 6, 10, 12), 32, 64, 25, X | WP | FBIAS | RES | Y2, reaches=EINVAL)
row("err-wino43-runtime-flags-with-bits", "wino43", (2, 6, 10, 12), 32, 64, 8, X | WP | FBIAS | Y | SBITS, reaches=EINVAL)
row("err-wino43-addup-bits-with-y", "wino43", (2, 6, 10, 12), 32, 64, 25, X | WP | FBIAS | RES | Y | Y2 | SBITS, reaches=EINVAL)
for entry in ("wino_fwd_bits", "w2_43_bits"):
    small = (2, 10, 12) if ENTRIES[entry]["nd"] == 2 else (2, 6, 10, 12)
    row("err-%s-fwd-without-bits" % entry, entry, small, 32, 64, 9, X | WP | FBIAS | Y, reaches=EINVAL)
    row("err-%s-fwd-without-bias" % entry, entry, small, 32, 64, 9, X | WP | Y | SBITS, reaches=EINVAL)
    row("err-%s-both-words" % entry, entry, small, 32, 64, 9, X | WP | FBIAS | MBITS | Y | SBITS, reaches=EINVAL)
    row("err-%s-mask-without-bits" % entry, entry, small, 32, 64, 4, X | WP | Y, reaches=EINVAL)
    row("err-%s-mask-with-sign-bits" % entry, entry, small, 32, 64, 4, X | WP | Y | SBITS, reaches=EINVAL)
    row("err-%s-other-flags" % entry, entry, small, 32, 64, 8, reaches=EINVAL)
for entry in ("wino_upconv_fwd", "w2_up_fwd"):
    small = (2, 10, 12) if ENTRIES[entry]["nd"] == 2 else (2, 6, 10, 12)
    for fl in (0, 1, 8, 11, 25):
        row("err-%s-badflags%d" % (entry, fl), entry, small, 32, 64, fl, reaches=EINVAL)
ERR_ROWS = [r for r in ROWS if isinstance(r["reaches"], int)]
assert len(OK_ROWS) + len(ERR_ROWS) == len(ROWS) and len({r["id"] for r in ROWS}) == len(ROWS)
assert not [r["id"] for r in OK_ROWS if isinstance(r["reaches"], int)]


def by_id(rid):
    return [r for r in ROWS if r["id"] == rid][0]
