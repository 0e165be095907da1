"""Inputs for the tests of mean_attributes (dsa_encode_mean_sequential_batch; synth.merge_means, synth.encode_merged(mean_attributes=)):
point clouds of mergecases.along_z -- integer positions on z_grid(bits), a multiplicity per cell, shuffled rows -- with attribute
values designed per cell, and the contract restated in Python integers.

    by_cell(case, fn)               an array with the rows of cell j set to fn(j, k) (k rows of values), whatever the shuffle
    cases()                         [Case]: ties, signed element types, saturated bytes, sums beyond 32 bits, 1 - 4 components, a
                                    masked attribute beside an unmasked one, every run shape of mergecases.boundary_runs
    pin(case)                       per attribute of the stream the (m, nc) integers entry j must carry: q from the oracle's decode of
                                    the plain ordered stream of all n rows (the CPU coder's, no merge), the mean per cell by the rule
                                    floor((2 S + cnt) / (2 cnt)) in Python integers for a masked attribute, q[kept[j]] otherwise
    cpu_args(case) / cloud(case)    the arguments of the synth twins / the PointCloudData of the device call"""
import collections
import functools

import numpy as np

import mergecases as mc
import oracle
import draco_sharp_amd.synth as synth

TILE = mc.TILE
BITS = 14               # every case on one position grid: the cases are one batch
# extras: a list of (values, quantization_bits, grid) with grid None or (origin, range); mask: bits over the attributes of the stream;
# expect: {attribute of the stream: (m, nc) means known by construction}
Case = collections.namedtuple("Case", "name pos bits grid normals uvs generic extras mask expect")


def make(base, normals=None, uvs=None, generic=None, extras=(), mask=0, expect=None):
    return Case(base.name, base.pos, base.bits, base.grid, normals, uvs, generic, list(extras), mask, expect or {})


def cell_of(case):
    return case.pos[:, 2].astype(np.int64)


def by_cell(case, fn, dtype, nc=1):
    """rows of cell j = fn(j, k), an array (k, nc) or (k,) for the k rows of the cell, handed out in row order"""
    cell = cell_of(case)
    out = np.zeros((len(cell), nc), dtype)
    for j, k in enumerate(mc.runs_of(case)):
        out[np.flatnonzero(cell == j)] = np.asarray(fn(j, int(k))).reshape(k, nc)
    return out


def ties():
    """{0,1} -> 1, {-1,0} -> 0, {-2,-1} -> -1, {1,2,2} -> 2, {1,1,2} -> 1: the exact mean, halves toward +infinity"""
    sets = [[0, 1], [-1, 0], [-2, -1], [1, 2, 2], [1, 1, 2], [7], [-128, 127]]
    base = mc.along_z("ties", [len(s) for s in sets], BITS, 901)
    want = np.array([[1], [0], [-1], [2], [1], [7], [0]], np.int32)
    vals = lambda dt: by_cell(base, lambda j, k: sets[j], dt)          # noqa: E731
    return make(base, extras=[(vals(np.int8), 0, None), (vals(np.int16), 0, None), (vals(np.int32), 0, None)], mask=0b1110, expect={1: want, 2: want, 3: want})


def signed():
    """int8 x 1, int16 x 2, int32 x 3 with negative values and a uint8 x 4 generic attribute, over cells of 1 .. 5 rows; normals and
    the int16 attribute are NOT masked: they carry row kept[j]"""
    rng = np.random.default_rng(902)
    base = mc.along_z("signed", rng.integers(1, 6, 300), BITS, 902)
    n = len(base.pos)
    return make(base, normals=rng.normal(size=(n, 3)).astype(np.float32), generic=rng.integers(0, 256, (n, 4)).astype(np.uint8),
                extras=[(rng.integers(-128, 128, (n, 1)).astype(np.int8), 0, None), (rng.integers(-32768, 32768, (n, 2)).astype(np.int16), 0, None),
                        (rng.integers(-2**27, 2**27 + 1, (n, 3)).astype(np.int32), 0, None)],
                mask=(1 << 2) | (1 << 3) | (1 << 5))        # the stream: 0 positions, 1 normals, 2 generic uint8 x 4, 3 int8, 4 int16 (not masked), 5 int32


def saturated():
    """uint8 at 255 throughout (a byte-wide accumulator or mean would wrap), uint16 at 65 535 over a run of 3 000 rows"""
    base = mc.along_z("saturated", [60, 8, 3000, 1, 64, 5], BITS, 903)
    n = len(base.pos)
    full16 = by_cell(base, lambda j, k: [65535] * k if j == 2 else [j] * k, np.uint16)
    m = 6
    return make(base, generic=np.full((n, 3), 255, np.uint8), extras=[(full16, 0, None)], mask=0b110,
                expect={1: np.full((m, 3), 255, np.int32), 2: np.array([[0], [1], [65535], [3], [4], [5]], np.int32)})


def wide_sums():
    """int32 at +2^27 and at -2^27 over runs of 2 049 rows: |S| = 2^38 and a bit, a 32-bit accumulator fails; a float attribute at 20
    quantisation bits near the top of its grid over 4 097 rows: S > 2^32"""
    base = mc.along_z("wide-sums", [2049, 3, 2049, 4097, 2], BITS, 904)
    top = 2**27
    ints = by_cell(base, lambda j, k: {0: [top] * k, 2: [-top] * k}.get(j, [5 - j] * k), np.int32)
    rng = np.random.default_rng(904)
    # the grid of the floats: 0 in cells 1 and 4, 1 - 2^-12 .. 1 in the long run of cell 3, so that its integers lie within 256 of 2^20 - 1
    floats = by_cell(base, lambda j, k: (1.0 - rng.random(k) / 4096.0) if j == 3 else (np.linspace(0.0, 1.0, k) if j == 4 else rng.random(k) * 0.5), np.float32)
    return make(base, extras=[(ints, 0, None), (floats, 20, None)], mask=0b110, expect={1: np.array([[top], [4], [-top], [2], [1]], np.int32)})


def components_and_uv():
    """texture coordinates (quantised, built in) and float attributes of 1, 3 and 4 components on own bounds and on an explicit grid"""
    rng = np.random.default_rng(905)
    base = mc.along_z("components", rng.integers(1, 9, 150), BITS, 905)
    n = len(base.pos)
    return make(base, uvs=rng.random((n, 2)).astype(np.float32),
                extras=[(rng.random((n, 1)).astype(np.float32), 12, None), (rng.random((n, 3)).astype(np.float32) * 2 - 1, 9, ([-1.5, -1.0, -1.25], 3.0)),
                        (rng.random((n, 4)).astype(np.float32), 0, None), (rng.integers(0, 256, (n, 4)).astype(np.uint8), 0, None)], mask=0b111110)


def run_shapes():
    """a uint8 x 4 colour and one float attribute, both masked, over every run shape: multiplicity 1 throughout, the runs of
    mergecases.boundary_runs (ending at / beginning at / straddling a 64-entry step and a 1024-entry tile), one run of 2 TILE + 1"""
    out = []
    bases = [mc.along_z("distinct-65", np.ones(65, np.int64), BITS, 906), mc.along_z("distinct-%d" % (TILE + 1), np.ones(TILE + 1, np.int64), BITS, 907)]
    bases += mc.boundary_runs(BITS) + [mc.along_z("identical-%d" % (2 * TILE + 1), [2 * TILE + 1], BITS, 908), mc.along_z("one-point", [1], BITS, 909)]
    for k, base in enumerate(bases):
        rng = np.random.default_rng(910 + k)
        n = len(base.pos)
        out.append(make(base, extras=[(rng.integers(0, 256, (n, 4)).astype(np.uint8), 0, None), (rng.normal(size=(n, 1)).astype(np.float32), 16, None)], mask=0b110))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return tuple([ties(), signed(), saturated(), wide_sums(), components_and_uv()] + run_shapes())


def attributes(case):
    """the stream's attributes beyond the positions: (index of the stream, kind, values) with kind "normals" / "uvs" / "generic" / k"""
    out, a = [], 1
    for kind in ("normals", "uvs", "generic"):
        if getattr(case, kind) is not None:
            out.append((a, kind, getattr(case, kind)))
            a += 1
    for k, (values, _, _) in enumerate(case.extras):
        out.append((a + k, k, values))
    return out


def cpu_args(case, rows=None):
    """the arguments of synth.encode_merged / encode_cell_parts / encode_lod_parts / encode_ordered for the case (rows: a shuffle)"""
    take = (lambda a: a) if rows is None else (lambda a: None if a is None else np.ascontiguousarray(a[rows]))
    extra = [synth.Extra(take(v), quantization_bits=b, grid=None if g is None else synth.grid(g[0], g[1])) for v, b, g in case.extras] or None
    opt = synth.options(pos_bits=case.bits, generic_components=case.generic.shape[1] if case.generic is not None else 1)
    return dict(pos=take(case.pos), normals=take(case.normals), uvs=take(case.uvs), generic=take(case.generic), extra=extra, opt=opt,
                pos_grid=None if case.grid is None else synth.grid(case.grid[0], case.grid[1]))


def cloud(case, rows=None):
    """the PointCloudData of the device call (rows: a shuffle of the input rows)"""
    import draco_sharp_amd as dsa
    take = (lambda a: a) if rows is None else (lambda a: None if a is None else np.ascontiguousarray(a[rows]))
    atts = [dsa.Attribute(take(v), quantization_bits=b, grid=None if g is None else dsa.Grid(g[0], float(g[1]))) for v, b, g in case.extras]
    return dsa.PointCloudData(take(case.pos), normals=take(case.normals), texcoords=take(case.uvs), generic=take(case.generic), attributes=atts,
                              position_grid=None if case.grid is None else dsa.Grid(case.grid[0], float(case.grid[1])))


def mean(values):
    """the rule in Python integers: floor((2 S + cnt) / (2 cnt))"""
    s, cnt = sum(int(v) for v in values), len(values)
    return (2 * s + cnt) // (2 * cnt)


@functools.lru_cache(maxsize=None)
def _pin(name):
    case = next(c for c in cases() if c.name == name)
    kept, cells, _ = mc.pin(case.pos, case.bits, case.grid)
    data, perm = synth.encode_ordered(geometry=0, **cpu_args(case))
    dec = oracle.decode(data)
    assert dec.num_points == len(case.pos) and len(dec.attributes) == 1 + len(attributes(case))
    order = np.argsort(cells, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(np.bincount(cells, minlength=len(kept)))])
    out = {}
    for a, _, _ in attributes(case):
        q = np.zeros(dec.attributes[a].portable.shape, np.int64)
        q[perm] = dec.attributes[a].portable
        if not (case.mask >> a) & 1:
            out[a] = q[kept]
            continue
        out[a] = np.array([[mean(q[order[bounds[j]:bounds[j + 1]], c]) for c in range(q.shape[1])] for j in range(len(kept))], np.int64)
    return kept, cells, out


def pin(case):
    """(kept, row_entries, {attribute of the stream: (m, nc) integers entry j carries})"""
    return _pin(case.name)


def decoded(streams):
    """per attribute beyond the positions the integers of the streams' entries joined, through the oracle"""
    decs = [oracle.decode(s) for s in streams]
    return {a: np.concatenate([d.attributes[a].portable for d in decs]).astype(np.int64) for a in range(1, len(decs[0].attributes))}
