"""The designed floats of tests/quantcases.py, without a GPU: every case meets the condition it was built for, and the host
coder (draco-sharp_amd/csrc/dsa_encode_host.h quantize, Octa) equals the numpy reference through the oracle -- header floats
as bit patterns, portable integers, and the oracle's dequantised values bit for bit -- or refuses with the text the rules give."""
import numpy as np
import pytest

import meshutil
import quantcases as qc
import draco_sharp_amd.synth as synth

F = np.float32
SUBNORMAL = F(2.0 ** -126)


def opt_of(c):
    return synth.options(pos_bits=c.pos_bits, uv_bits=c.uv_bits, normal_bits=c.normal_bits)


def extras_of(c):
    return [synth.Extra(e, quantization_bits=c.extra_bits) for e in c.extras] or None


def columns(c):
    """every column of every quantised attribute of the case"""
    return [v[:, j] for _, v, _ in qc.quantised_slots(c) for j in range(v.shape[1])]


def first_row_of_minimum(col):
    m = col[0]
    row = 0
    for r, x in enumerate(col):          # the serial strict compare, as the reference takes it
        if x < m:
            m, row = x, r
    return row


# ---- the designs
def test_sizes_put_minima_and_maxima_in_the_first_the_last_and_the_rows_around_256():
    assert [len(c.pos) for c, _ in qc.sizes()] == list(qc.SIZES)
    held_min, held_max = set(), set()
    for c, place in qc.sizes():
        n = len(c.pos)
        assert [v.shape[1] for _, v, _ in qc.quantised_slots(c)] == [3, 2, 1, 4] and (c.pos_bits, c.extra_bits) == (11, 12)
        cols = columns(c)
        assert len(cols) == len(place) == 10
        for col, (lo, hi) in zip(cols, place):
            assert first_row_of_minimum(col) == lo == int(np.argmin(col)) and int(np.argmax(col)) == hi
            assert (lo != hi or n == 1) and np.count_nonzero(col == col.min()) == 1 and np.count_nonzero(col == col.max()) == 1
            held_min.add((n, lo))
            held_max.add((n, hi))
        assert len({p for p in place}) == min(10, len(qc.extreme_rows(n)) * (len(qc.extreme_rows(n)) - 1)) or n == 1
    for n in qc.SIZES:
        for r in qc.extreme_rows(n):
            assert (n, r) in held_min and (n, r) in held_max
    assert qc.extreme_rows(1025) == [0, 255, 256, 1024] and qc.extreme_rows(256) == [0, 255] and qc.extreme_rows(257) == [0, 255, 256]


def test_zeros_give_the_sign_of_the_first_zero():
    by = {c.name: c for c in qc.zeros()}
    for gap in (1, 256, 257):
        c = by["zeros-gap-%d" % gap]
        assert len(c.pos) == gap + 2
        for j, col in enumerate(columns(c)):
            head, z1, z2, tail = qc.ZERO_ORDERS[j % 4]
            z = np.flatnonzero(col == 0)
            assert len(z) == 2 and z[1] - z[0] == gap and col.min() == 0 and col.max() == 5
            assert qc.bits_of(col[z]).tolist() == [qc.bits_of(z1).item(), qc.bits_of(z2).item()] and qc.bits_of(z1) != qc.bits_of(z2)
            assert z[0] == (1 if head is not None else 0) and int(np.argmax(col)) == (0 if head is not None else gap + 1)
            assert qc.bits_of(qc.own_bounds(col)[0]).item() == qc.bits_of(z1).item()
        # both zeros in the rows of one thread of 256 (gap 256), and of neighbouring threads (gap 257)
        assert gap != 256 or all((np.flatnonzero(col == 0) % 256).tolist() in ([0, 0], [1, 1]) for col in columns(c))
    # [5, -0, +0] is the issue's example: 0x80000000 in the header
    assert qc.bits_of(qc.own_bounds(F([5.0, -0.0, 0.0]))[0]).item() == 0x80000000 and qc.bits_of(qc.own_bounds(F([5.0, 0.0, -0.0]))[0]).item() == 0
    c = by["zeros-flat-and-maxima"]
    cols = columns(c)
    assert all(qc.bits_of(x) == 0x80000000 for x in cols[0]) and qc.bits_of(qc.own_bounds(cols[0])[0]).item() == 0x80000000
    assert cols[1].max() == 0 and cols[2].max() == 0 and cols[1].min() == cols[2].min() == -3
    assert qc.bits_of(cols[1].max()).item() == 0x80000000 and qc.bits_of(cols[2].max()).item() == 0
    assert qc.bits_of(qc.own_bounds(cols[3])[0]).item() == 0 and qc.bits_of(cols[3][-1]).item() == 0x80000000
    assert qc.own_bounds(np.stack([cols[0], cols[3]], axis=1))[1] == 1          # all zeros: the range is 1


def test_ties_pin_the_float32_rounding_of_every_step():
    assert [c.pos_bits for c in qc.ties()] == list(qc.TIE_BITS) == [1, 2, 11, 16, 20]
    for c in qc.ties():
        bits = c.pos_bits
        max_q = (1 << bits) - 1
        assert c.uv_bits == c.extra_bits == bits
        rounded_up = 0
        for _, v, b in qc.quantised_slots(c):
            qmin, qrange = qc.own_bounds(v)
            assert not qmin.any() and qrange == max_q and F(F(max_q) / qrange) == 1          # inv_delta == 1
            q = qc.quantised(v, b)
            assert q.min() == 0 and q.max() == max_q
            exact = np.floor(v.astype(np.float64) + 0.5).astype(np.int64)                 # what an unrounded sum would give
            frac = v - np.floor(v)
            assert np.count_nonzero(frac == 0.5) >= 1 and np.count_nonzero((frac > 0) & (frac < 0.5)) >= 1 and np.count_nonzero(frac > 0.5) >= 1
            rounded_up += np.count_nonzero(q != exact)
            below = np.nextafter(F(0.5), F(0))
            assert (v == below).any() and (q[v == below] == 1).all() and (exact[v == below] == 0).all()      # float32 rounds 0.5- + 0.5 up to 1
            assert (q[v == F(0.5)] == 1).all()
        assert rounded_up >= 4


def test_subnormal_differences_carry_integers():
    (c,) = qc.subnormal()
    assert len(c.pos) == 600 and c.pos_bits == 11
    qmin, qrange = qc.own_bounds(c.pos)
    inv = F(F(2047) / qrange)
    assert not qmin.any() and qrange == F(8e-36) and np.isfinite(inv)
    assert np.count_nonzero((c.pos < 1e-38).all(axis=1)) >= 200
    d = (c.pos - qmin).astype(F)
    q = qc.quantised(c.pos, 11)
    hit = (d > 0) & (d < SUBNORMAL) & (q > 0)
    print("subnormal differences with an integer above 0:", np.count_nonzero(hit))
    assert np.count_nonzero(hit) >= 300
    flushed = meshutil.quantize(np.where(d < SUBNORMAL, F(0), c.pos), qmin, qrange, 11)      # what a flush of the difference would give
    assert np.count_nonzero(flushed != q) == np.count_nonzero(hit)
    assert F(qrange / F(2047)) < SUBNORMAL          # and the dequantiser's delta is subnormal itself


def test_magnitudes():
    by = {c.name: c for c in qc.magnitudes()}
    c = by["magnitudes-1e6-at-20-bits"]
    assert c.pos_bits == 20 and c.pos.min() < -2.9e5 and c.pos.max() > 6.9e5
    c = by["magnitudes-1e30"]
    assert np.abs(c.pos).max() > 9e29 and np.isfinite(qc.own_bounds(c.pos)[1]) and qc.own_bounds(c.pos)[1] > 1.9e30
    c = by["magnitudes-flat"]
    assert all(qc.own_bounds(v)[1] == 1 and not qc.quantised(v, b).any() for _, v, b in qc.quantised_slots(c))
    c = by["magnitudes-thin-component"]
    qmin, qrange = qc.own_bounds(c.pos)
    q = qc.quantised(c.pos, 11)
    assert np.ptp(c.pos[:, 1]) > 0 and np.ptp(c.pos[:, 1]) < 1e-6 * qrange and not q[:, 1:].any() and q[:, 0].max() == 2047


def test_normals_reach_the_rules_every_edge_and_the_ties():
    assert [c.normal_bits for c in qc.normals()] == list(qc.NORMAL_BITS) == [2, 3, 4, 8, 11]
    for c in qc.normals():
        bits = c.normal_bits
        center, max_value = qc.oct_center(bits), (1 << bits) - 2
        pts = qc.lattice(bits)
        full = 4 * center * center + 2
        assert len(pts) == min(full, qc.NORMAL_SAMPLE) and (np.abs(pts).sum(axis=1) == center).all() and len({tuple(p) for p in pts.tolist()}) == len(pts)
        assert len(c.normals) == 3 * len(pts) + 11 <= 12011
        st, rule, raw = meshutil.oct_quantize_rules(c.normals, bits)
        # Which rules a float vector can reach.  The integers (i0, i1, i2) always end with |i0| + |i1| + |i2| = center, and the
        # full lattice (bits 2 to 4 hold all of it) is every such triple, so what it reaches is all there is: rule 2 (s == 0, t
        # above the centre) and rule 5 (t == 0, s above the centre) from 3 bits on, nothing at 2 bits (center 1: i0 < 0 leaves
        # i1 = i2 = 0), and never the corners nor the rules of s == max_value / t == max_value -- with i0 < 0 an s of max_value
        # needs i2 == 0 and i1 >= 0, which puts t at max_value - i1 >= center.  Those three serve integers from elsewhere.
        assert set(rule.tolist()) == ({0} if bits == 2 else {0, 2, 5}), (bits, sorted(set(rule.tolist())))
        if full <= qc.NORMAL_SAMPLE:
            assert len(pts) == full and np.array_equal(meshutil.oct_quantize_rules(pts, bits)[1] != 0, rule[:len(pts)] != 0)
        for axis in (0, 1):
            for edge in (0, max_value):
                assert (raw[:, axis] == edge).any(), (bits, axis, edge)
        assert st.min() >= 0 and st.max() <= max_value
        # the shifted lattice: both scaled coordinates times the centre end in .5, so floor(x + 0.5) sits on a tie
        shifted = c.normals[2 * len(pts):3 * len(pts)].astype(np.float64)
        s = shifted / np.abs(shifted).sum(axis=1, keepdims=True) * center
        on_tie = np.abs(s[:, :2] - np.floor(s[:, :2]) - 0.5) < 1e-9
        print("normals at %d bits: %d of %d shifted rows on a tie" % (bits, np.count_nonzero(on_tie.all(axis=1)), len(pts)))
        assert np.count_nonzero(on_tie.any(axis=1)) >= len(pts) // 8
        # the lattice itself maps to itself: x and y come back exactly
        got = meshutil.oct_quantize(pts, bits)
        assert len(got) == len(pts)
        # the rows behind: zero, under / at / over the 1e-6 cut, the axes, -0.0
        tail = c.normals[3 * len(pts):]
        assert not tail[0].any() and np.array_equal(tail[1:4], F(qc.SMALL_NORMALS)) and np.array_equal(tail[4:10], F(qc.AXES)) and qc.bits_of(tail[10][0]) == 0x80000000
        l1 = np.abs(tail[1:4].astype(np.float64)).sum(axis=1)
        assert l1[0] < 1e-6 and l1[2] > 1e-6 and abs(l1[1] - 1e-6) < 1e-12
        x_axis = meshutil.oct_quantize(F([[1, 0, 0]]), bits)[0]
        t = meshutil.oct_quantize(tail, bits)
        assert np.array_equal(t[0], x_axis) and np.array_equal(t[1], x_axis) and np.array_equal(t[4], x_axis)      # below the cut: (1, 0, 0)
        assert not np.array_equal(t[3], x_axis) or center < 3
        assert np.array_equal(t[2], x_axis) == (l1[1] <= 1e-6)
        assert np.array_equal(t[10], t[8])                                         # (-0.0, 0, 1) is (0, 0, 1)


def test_refused_cases_are_the_rules_refusals():
    by = {c.name: c for c in qc.refused()}
    assert by["refused-nan-row-417"].refusal == "positions: row 417 is not finite" and len(by["refused-nan-row-417"].pos) == 800
    assert by["refused-inf-row-17"].refusal == "positions: row 17 is not finite" and by["refused-inf-row-17"].pos[17, 0] == -np.inf
    assert by["refused-nan-row-0"].refusal == "positions: row 0 is not finite"
    assert by["refused-nan-in-an-extra"].refusal == "attribute 1: row 40 is not finite"
    c = by["refused-range-too-small"]
    qrange = qc.own_bounds(c.pos)[1]
    assert c.pos_bits == 11 and np.isfinite(c.pos).all() and 0 < qrange < 1.1e-39 and not qc.range_carries(qrange, 11)
    assert c.refusal == qc.range_refusal("positions", qrange, 11) and c.refusal.startswith("positions: the range 9.9") and " 11 quantisation bits" in c.refusal
    c = by["refused-range-infinite"]
    assert np.isfinite(c.pos).all() and np.isinf(qc.own_bounds(c.pos)[1]) and c.refusal.startswith("positions: the range inf ")
    assert by["refused-nan-before-range"].refusal == "positions: row 5 is not finite" and not qc.range_carries(qc.own_bounds(np.nan_to_num(by["refused-nan-before-range"].pos))[1], 11)
    assert by["refused-small-range-in-texcoords"].refusal.startswith("texcoords: the range ")
    assert all(c.refusal for c in qc.refused()) and all(c.refusal is None and qc.expected_refusal(c) is None for c in qc.coded())
    assert all(len(c.pos) <= 12011 for c in qc.coded() + qc.refused())


# ---- the host coder against the reference
@pytest.mark.parametrize("name", [c.name for c in qc.coded()])
def test_host_coder_equals_the_reference_on_clouds(name):
    c = {c.name: c for c in qc.coded()}[name]
    stream = synth.encode_point_cloud_attributes(c.pos, c.normals, c.uvs, None, opt_of(c), extras_of(c))
    qc.check_stream(c, stream, True)


@pytest.mark.parametrize("name", [c.name for cs in qc.families(("zeros", "ties", "subnormal")).values() for c in cs])
def test_host_coder_equals_the_reference_on_meshes(name):
    c, faces = qc.as_mesh({c.name: c for c in qc.coded()}[name])
    stream = synth.encode_mesh(c.pos, faces, c.normals, c.uvs, None, opt_of(c), extras_of(c))
    qc.check_stream(c, stream, False)


@pytest.mark.parametrize("name", [c.name for c in qc.refused()])
def test_host_coder_refuses(name):
    c = {c.name: c for c in qc.refused()}[name]
    with pytest.raises(RuntimeError) as e:
        synth.encode_point_cloud_attributes(c.pos, c.normals, c.uvs, None, opt_of(c), extras_of(c))
    assert str(e.value) == c.refusal
    faces = synth.make_mesh(synth.GRID, len(c.pos) // 2 - 1, 1, 1)[3]
    assert int(faces.max()) + 1 == len(c.pos)
    with pytest.raises(RuntimeError) as e:
        synth.encode_mesh(c.pos, faces, None, c.uvs, None, opt_of(c), extras_of(c))
    assert str(e.value) == c.refusal
