"""Designed floats for the quantisers at the front of the encoder -- the bounds (k_enc_bounds), the quantised floats and the
octahedral normals (k_enc_quantize) and the dequantisation on the way back (k_finalize, k_predict_wrap) -- and their reference
in numpy, derived from the source arrays alone.  No GPU here: tests/test_quantise_designs_cpu.py holds every case to the
condition it was built for and the host coder to this reference; tests/test_gpu_encode_quantise.py holds the device to both.

The rules (AttributeQuantizationTransform.cs:66-108,136-177, Core/Quantizer.cs, OctahedronToolBox.cs:28-119):
  minimum of a component  the value of the FIRST row that attains it (a serial strict compare): the sign of a zero is that row's
  range                   the largest float32(max - min) over the components, 1 if that is 0
  q                       floor(float32(float32(v - min) * float32(max_q / range)) + 0.5f), every step rounded to float32
  back                    float32(float32(q) * float32(range / max_q)) + min, every step rounded to float32
A value that is not finite refuses the mesh ("<slot>: row R is not finite", the smallest such row); else a range that is not
finite, or so small that max_q / range is not, does (range_refusal)."""
import collections
import functools

import numpy as np

import meshutil
import oracle

F = np.float32

# One point cloud: positions (n, 3) always, the other arrays where the design has them.  `extras`: float32 arrays (n, 1..4), each
# quantised to extra_bits.  `refusal`: the text both coders refuse the cloud with (None: it is coded).  `family` groups the cases.
Case = collections.namedtuple("Case", "name family pos pos_bits uvs uv_bits normals normal_bits extras extra_bits refusal")


def case(name, family, pos, pos_bits=11, uvs=None, uv_bits=11, normals=None, normal_bits=8, extras=(), extra_bits=12, refusal=None):
    f = lambda a: None if a is None else np.ascontiguousarray(a, F)          # noqa: E731
    return Case(name, family, f(pos), pos_bits, f(uvs), uv_bits, f(normals), normal_bits, tuple(f(e).reshape(len(pos), -1) for e in extras), extra_bits, refusal)


# ---- the reference
def own_bounds(values):
    """(qmin float32[nc], qrange float32) by the serial rule."""
    v = np.asarray(values, F).reshape(len(values), -1)
    qmin = np.array([col[np.flatnonzero(col == col.min())[0]] for col in v.T], F)
    with np.errstate(over="ignore"):
        ext = (v.max(axis=0).astype(F) - qmin).astype(F)
    qrange = F(ext.max())
    return qmin, (F(1.0) if qrange == 0 else qrange)


def quantised(values, bits):
    v = np.asarray(values, F).reshape(len(values), -1)
    qmin, qrange = own_bounds(v)
    return meshutil.quantize(v, qmin, qrange, bits)


def dequantised(q, qmin, qrange, bits):
    delta = F(F(qrange) / F((1 << bits) - 1))
    return (np.asarray(q).astype(F) * delta).astype(F) + np.asarray(qmin, F)


def bits_of(a):
    """float32 values as their bit patterns (-0.0 is not +0.0)"""
    return np.ascontiguousarray(a, F).view(np.uint32)


def row_refusal(slot, row):
    return "%s: row %d is not finite" % (slot, row)


def range_refusal(slot, qrange, bits):
    return "%s: the range %g of its values cannot carry %d quantisation bits (the range and (2^bits - 1) / range must be finite)" % (slot, float(qrange), bits)


def range_carries(qrange, bits):
    with np.errstate(over="ignore", divide="ignore"):
        return bool(np.isfinite(qrange) and np.isfinite(F(F((1 << bits) - 1) / F(qrange))))


def quantised_slots(c):
    """(slot name as the messages call it, values, bits) of every quantised attribute of case c, in stream order"""
    out = [("positions", c.pos, c.pos_bits)]
    if c.uvs is not None:
        out.append(("texcoords", c.uvs, c.uv_bits))
    return out + [("attribute %d" % k, e, c.extra_bits) for k, e in enumerate(c.extras)]


def expected_refusal(c):
    """the refusal the rules give case c from its arrays alone (None: coded): the first slot in stream order that has one"""
    for slot, v, bits in quantised_slots(c):
        bad = np.flatnonzero(~np.isfinite(v).all(axis=1))
        if len(bad):
            return row_refusal(slot, bad[0])
        qrange = own_bounds(v)[1]
        if not range_carries(qrange, bits):
            return range_refusal(slot, qrange, bits)
    return None


# ---- the cases
def _spread(cols, n):
    """pos / uvs / extras (1 and 4 components) of n rows whose ten columns cycle through `cols`"""
    take = lambda lo, hi: np.stack([np.asarray(cols[i % len(cols)], F) for i in range(lo, hi)], axis=1)          # noqa: E731
    assert all(len(col) == n for col in cols)
    return dict(pos=take(0, 3), uvs=take(3, 5), extras=(take(5, 6), take(6, 10)))


SIZES = (1, 2, 255, 256, 257, 513, 1025)


def extreme_rows(n):
    """the rows a minimum or maximum is put in: the first, the last, and the two around the block's 256 threads"""
    return sorted({r for r in (0, n - 1, 255, 256) if r < n})


@functools.lru_cache(None)
def sizes():
    """every n around the 256 threads of the reduction; column j has its minimum in row place[j][0] and its maximum in row
    place[j][1], over the ordered pairs of extreme_rows(n) -- different rows in different columns"""
    out = []
    for n in SIZES:
        rng = np.random.default_rng(1000 + n)
        rows = sorted(set(extreme_rows(n)))
        pairs = [(a, b) for a in rows for b in rows if a != b] or [(0, 0)]
        cols, place = [], []
        for j in range(10):
            lo, hi = pairs[j % len(pairs)]
            col = rng.uniform(-1, 1, n).astype(F)
            if n > 1:
                col[hi] = F(3 + j)
            col[lo] = F(-2 - j) if n > 1 else F(0.25 * j - 1)
            cols.append(col)
            place.append((lo, hi))
        out.append((case("sizes-%d" % n, "sizes", **_spread(cols, n)), place))
    return out


PZ, NZ = F(0.0), F(-0.0)
ZERO_ORDERS = ((5, NZ, PZ, None), (5, PZ, NZ, None), (None, NZ, PZ, 5), (None, PZ, NZ, 5))      # (head, first zero, second zero, tail)


def _zero_column(order, gap, rng):
    """5 in front of or behind two zeros that lie `gap` rows apart, positive values between"""
    head, z1, z2, tail = order
    n = gap + 2
    col = rng.uniform(1, 4, n).astype(F)
    at = 1 if head is not None else 0
    col[at], col[at + gap] = z1, z2
    col[0 if head is not None else n - 1] = F(5)
    return col


@functools.lru_cache(None)
def zeros():
    out = []
    for gap in (1, 256, 257):           # side by side; in the rows of one thread; in the rows of neighbouring threads
        rng = np.random.default_rng(2000 + gap)
        cols = [_zero_column(o, gap, rng) for o in ZERO_ORDERS]
        out.append(case("zeros-gap-%d" % gap, "zeros", **_spread(cols, gap + 2)))
    neg = lambda z: np.array([-3, -1, z, -2], F)          # noqa: E731
    cols = [np.full(4, NZ, F), neg(NZ), neg(PZ), np.array([PZ, PZ, PZ, NZ], F)]
    out.append(case("zeros-flat-and-maxima", "zeros", **_spread(cols, 4)))
    return out


TIE_BITS = (1, 2, 11, 16, 20)


def tie_values(bits, ks):
    """0, max_q and around every k + 0.5 the float32 below, the tie and the float32 above"""
    max_q = (1 << bits) - 1
    v = [F(0), F(max_q)]
    for k in ks:
        t = F(k + 0.5)
        v += [np.nextafter(t, F(0)), t, np.nextafter(t, F(np.inf))]
    return np.array(v, F)


@functools.lru_cache(None)
def ties():
    """range exactly max_q and minimum 0: inv_delta is 1, and the integer is floor(float32(v + 0.5))"""
    out = []
    for bits in TIE_BITS:
        max_q = (1 << bits) - 1
        rng = np.random.default_rng(3000 + bits)
        cols = []
        for j in range(4):
            ks = sorted({0, min(1, max_q - 1), max_q // 2, max_q - 1} | set(int(k) for k in rng.integers(0, max_q, 40)))
            col = tie_values(bits, ks)
            cols.append(col)
        n = max(len(col) for col in cols)
        cols = [np.concatenate([col, np.full(n - len(col), col[-1], F)]) for col in cols]          # (a repeat changes no bound)
        cols = [np.roll(col, j) for j, col in enumerate(cols)]
        out.append(case("ties-%d-bits" % bits, "ties", pos_bits=bits, uv_bits=bits, extra_bits=bits, **_spread(cols, n)))
    return out


@functools.lru_cache(None)
def subnormal():
    """600 points in [0, 8e-36], 200 of them below 1e-38: at 11 bits inv_delta = 2047 / 8e-36 is finite, and of the differences
    v - qmin hundreds are subnormal with an integer above 0 -- a flush to zero anywhere changes those integers"""
    rng = np.random.default_rng(4000)
    pos = (rng.random((600, 3)) * 8e-36).astype(F)
    small = rng.permutation(600)[:200]
    pos[small] = (rng.random((200, 3)) * 1e-38).astype(F)
    lo, hi = [r for r in range(600) if r not in set(small)][:2]
    pos[lo], pos[hi] = F(0), F(8e-36)
    return [case("subnormal-differences", "subnormal", pos, uvs=pos[:, :2][::-1].copy())]


@functools.lru_cache(None)
def magnitudes():
    rng = np.random.default_rng(5000)
    p = rng.random((1000, 3)).astype(F)
    out = [case("magnitudes-1e6-at-20-bits", "magnitudes", (p * F(1e6) - F(3e5)).astype(F), pos_bits=20, uvs=(p[:, :2] * F(1e6) - F(3e5)).astype(F), uv_bits=20,
                extras=[(p[:, :1] * F(1e6)).astype(F)], extra_bits=20)]
    big = rng.uniform(-1e30, 1e30, (700, 3)).astype(F)
    out.append(case("magnitudes-1e30", "magnitudes", big, uvs=big[:, 1:], extras=[big[:, :1], np.concatenate([big, big[:, :1]], axis=1)]))
    flat = np.tile(F([7.25, -3, 0.1]), (300, 1))
    out.append(case("magnitudes-flat", "magnitudes", flat, uvs=flat[:, :2], extras=[flat[:, 2:]]))
    thin = np.stack([rng.uniform(0, 1000, 900), 5 + rng.uniform(0, 1e-4, 900), np.full(900, 41.5)], axis=1).astype(F)
    out.append(case("magnitudes-thin-component", "magnitudes", thin, uvs=thin[:, :2], extras=[np.concatenate([thin, thin[:, 1:2]], axis=1)]))
    return out


NORMAL_BITS = (2, 3, 4, 8, 11)
NORMAL_SAMPLE = 4000
SMALL_NORMALS = ((1e-7, 0, 0), (3e-7, 4e-7, 3e-7), (4e-7, 3e-7, 4e-7))          # L1 norm under, at and over the 1e-6 cut
AXES = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))


def oct_center(bits):
    return ((1 << bits) - 2) // 2


def lattice(bits):
    """every integer point with |a| + |b| + |c| = center, both signs of c (one row where c is 0); more than NORMAL_SAMPLE of them:
    that many by a fixed permutation"""
    center = oct_center(bits)
    r = np.arange(-center, center + 1, dtype=np.int32)
    a, b = [x.ravel() for x in np.meshgrid(r, r, indexing="ij")]
    keep = np.abs(a) + np.abs(b) <= center
    a, b = a[keep], b[keep]
    c = center - np.abs(a) - np.abs(b)
    pts = np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, b, -c], axis=1)[c > 0]])
    if len(pts) > NORMAL_SAMPLE:
        pts = pts[np.random.default_rng(6000 + bits).permutation(len(pts))[:NORMAL_SAMPLE]]
    return pts.astype(F)


@functools.lru_cache(None)
def normals():
    out = []
    for bits in NORMAL_BITS:
        pts = lattice(bits)
        rows = np.concatenate([pts, (pts * F(0.37)).astype(F), (pts + F([0.5, -0.5, 0])).astype(F), np.zeros((1, 3), F), np.array(SMALL_NORMALS, F),
                               np.array(AXES, F), np.array([[NZ, 0, 1]], F)])
        n = len(rows)
        pos = np.stack([np.arange(n) / n, np.zeros(n), np.ones(n)], axis=1)
        out.append(case("normals-%d-bits" % bits, "normals", pos, normals=rows, normal_bits=bits))
    return out


@functools.lru_cache(None)
def refused():
    rng = np.random.default_rng(7000)
    cloud = lambda n: rng.random((n, 3)).astype(F)          # noqa: E731
    out = []

    def add(name, pos, **kw):
        c = case(name, "refused", pos, **kw)
        out.append(c._replace(refusal=expected_refusal(c)))

    p = cloud(800)
    p[417, 2] = np.nan
    add("refused-nan-row-417", p)
    p = cloud(300)
    p[17, 0] = -np.inf
    add("refused-inf-row-17", p)
    p = cloud(300)
    p[0, 1] = np.nan
    p[299, 0] = np.inf
    add("refused-nan-row-0", p)
    w = rng.random((500, 4)).astype(F)
    w[40, 3] = np.nan
    add("refused-nan-in-an-extra", cloud(500), extras=[rng.random((500, 1)).astype(F), w])
    add("refused-range-too-small", (cloud(400) * F(1e-39)).astype(F))
    add("refused-range-infinite", np.where(rng.random((400, 3)) < 0.5, F(-3e38), F(3e38)).astype(F))
    p = (cloud(400) * F(1e-39)).astype(F)
    p[5, 0] = np.nan
    add("refused-nan-before-range", p)
    add("refused-small-range-in-texcoords", cloud(400), uvs=(rng.random((400, 2)) * 1e-39).astype(F))
    return out


def coded():
    """every case that both coders code"""
    return [c for c, _ in sizes()] + zeros() + ties() + subnormal() + magnitudes() + normals()


def families(names=None):
    """the coded cases by family, in the order above"""
    out = collections.OrderedDict()
    for c in coded():
        if names is None or c.family in names:
            out.setdefault(c.family, []).append(c)
    return out


def grouped_by_bits(cases):
    """cases that one Config can take together: [((pos_bits, uv_bits, normal_bits), [cases])]"""
    out = collections.OrderedDict()
    for c in cases:
        out.setdefault((c.pos_bits, c.uv_bits, c.normal_bits), []).append(c)
    return list(out.items())


def as_mesh(c):
    """Case c on the vertices of the smallest two-row GRID mesh that holds its rows: (the case with its arrays at the mesh's vertex
    count, faces).  Vertex v carries row v; the one vertex an odd row count leaves over repeats the last row, which moves no
    bound and no first row that attains one."""
    import draco_sharp_amd.synth as synth
    n = len(c.pos)
    _, _, _, faces = synth.make_mesh(synth.GRID, max(1, (n + 1) // 2 - 1), 1, 1)
    nv = int(faces.max()) + 1
    assert n <= nv <= max(4, n + 1)
    pad = lambda a: None if a is None else np.concatenate([a, np.repeat(a[-1:], nv - n, axis=0)])          # noqa: E731
    return c._replace(pos=pad(c.pos), uvs=pad(c.uvs), normals=pad(c.normals), extras=tuple(pad(e) for e in c.extras)), faces


def check_stream(c, stream, in_row_order):
    """header floats as bits and the integers of every attribute of the oracle's decode against the reference; in row order also
    the oracle's values bit for bit"""
    d = oracle.decode(stream)
    slots = quantised_slots(c)
    want_types = [0] + ([1] if c.normals is not None else []) + ([3] if c.uvs is not None else []) + [4] * len(c.extras)
    assert [a.att_type for a in d.attributes] == want_types
    k = 0
    for a in d.attributes:
        assert not in_row_order or len(a.point_map) == 0 or np.array_equal(a.point_map, np.arange(len(c.pos)))
        if a.att_type == 1:
            want = meshutil.oct_quantize(c.normals, c.normal_bits)
            assert a.oct_bits == c.normal_bits
            if in_row_order:
                assert np.array_equal(a.portable, want), (c.name, "normals")
            else:
                assert sorted(map(tuple, a.portable.tolist())) == sorted(map(tuple, want.tolist())), (c.name, "normals")
            continue
        slot, v, bits = slots[k]
        k += 1
        nc = v.shape[1]
        qmin, qrange = own_bounds(v)
        assert a.q_bits == bits and a.num_components == nc
        assert bits_of(F(a.q_min[:nc])).tolist() == bits_of(qmin).tolist(), (c.name, slot, "minimum")
        assert bits_of(F(a.q_range)).item() == bits_of(qrange).item(), (c.name, slot, "range")
        want = quantised(v, bits)
        if in_row_order:
            assert np.array_equal(a.portable, want), (c.name, slot, "integers")
            assert a.values.tobytes() == dequantised(want, qmin, qrange, bits).tobytes(), (c.name, slot, "values")
        else:
            assert sorted(map(tuple, a.portable.tolist())) == sorted(map(tuple, want.tolist())), (c.name, slot, "integers")
            assert a.values.tobytes() == dequantised(a.portable, qmin, qrange, bits).tobytes(), (c.name, slot, "values")
    assert k == len(slots)
