"""Inputs and pins for the rows a coded stream carries (dsa_encode_rows_batch with track_rows, dsa_encoded_entry_rows,
synth.entry_rows; dsa_batch_source_rows behind a decode).  A case is one mesh in the form an encode call takes it, with the options
that shape its stream; the pins say, from the values passed and a decode of the stream alone, what

    rows[a][p] = entry_rows[a][point_map[a][p]]

must be for every attribute a of the stream and point p of the decoded mesh -- never by running an encoder's own bookkeeping again:

  (a) a uint32 attribute arange(V) per vertex decodes at p to the row of every attribute given per vertex; an int32 attribute
      arange(R) with the ids of an attribute given per corner over R rows decodes to that attribute's rows and to its own;
  (b) values[a][rows[a][p]] is what was decoded at p: integers bit for bit; quantised floats through the numpy quantisation of
      tests/meshutil.py with the stream's own (min, range, bits); normals through meshutil.oct_quantize;
  (c) with normals drawn from the 14 axis and diagonal directions (54 degrees apart at least, 8-bit octahedral error under 2) the
      normal decoded at p has a dot product above 0.99 with normals[rows[n][p]].
numpy only; deterministic."""
import collections

import numpy as np

import cornerattrcases
import defects
import draco_sharp_amd.synth as synth
import irregular
import meshutil
import seamdefects
import weldcases

Case = collections.namedtuple("Case", "name form pos faces nrm nid uv uid generic extras opt weld_attributes geometry")
Case.__doc__ = """form 1: the arguments of synth.encode_mesh_corners (ids None: per vertex); 2: one row per point (weld_points); 0: a
sequential stream (geometry 1) or a point cloud (0).  extras: synth.Extra list; opt: synth.options fields."""


def case(name, form, pos, faces, nrm=None, nid=None, uv=None, uid=None, generic=None, extras=(), opt=None, weld_attributes=False, geometry=1):
    u32 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint32).reshape(-1, 3)      # noqa: E731
    return Case(name, form, np.ascontiguousarray(pos, np.float32), u32(faces), nrm, u32(nid), uv, u32(uid), generic, list(extras), dict(opt or {}), weld_attributes, geometry)


DIRECTIONS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]] + [[x, y, z] for x in (1, -1) for y in (1, -1) for z in (1, -1)], np.float64)
DIRECTIONS = (DIRECTIONS / np.linalg.norm(DIRECTIONS, axis=1, keepdims=True)).astype(np.float32)


def directions_like(nrm):
    """One of the 14 directions per row, a function of the row's bytes: rows that were equal stay equal."""
    key = np.ascontiguousarray(nrm, np.float32).view(np.uint32).reshape(len(nrm), -1).astype(np.uint64)
    key = (key * np.array([2654435761, 40503, 2246822519], np.uint64)[None, :key.shape[1]]).sum(axis=1)
    return np.ascontiguousarray(DIRECTIONS[((key >> np.uint64(5)) % np.uint64(14)).astype(np.int64)])


def with_directions(c):
    return c._replace(name=c.name + "/14-directions", nrm=directions_like(c.nrm))


# ------------------------------------------------------------------------------------------------------------------ a case's calls
def values(c):
    """The value arrays of the case in the order of the stream's attributes."""
    out = [c.pos]
    if c.nrm is not None:
        out.append(np.asarray(c.nrm, np.float32))
    if c.uv is not None:
        out.append(np.asarray(c.uv, np.float32))
    if c.generic is not None:
        g = np.asarray(c.generic)
        out.append(g.reshape(len(g), -1))
    return out + [e.values for e in c.extras]


def per_vertex(c):
    """Per attribute of the stream: is it given per vertex (form 1; else None)."""
    if c.form != 1:
        return None
    out = [True]
    if c.nrm is not None:
        out.append(c.nid is None)
    if c.uv is not None:
        out.append(c.uid is None)
    if c.generic is not None:
        out.append(True)
    return out + [e.corners is None for e in c.extras]


def _args(c):
    return dict(pos=c.pos, faces=c.faces, normals=c.nrm, uvs=c.uv, generic=c.generic, extra=c.extras, opt=synth.options(**c.opt), form=c.form,
                normal_corners=c.nid, uv_corners=c.uid, geometry=c.geometry, weld_attributes=c.weld_attributes)


def twin(c):
    """The host coder's entry rows."""
    return synth.entry_rows(**_args(c))


def encode(c):
    """The host coder's stream."""
    return synth.encode_grid(**_args(c))


def mesh_data(c):
    """(dsa.MeshData or PointCloudData, dsa.Config fields) for the device encoder."""
    import draco_sharp_amd as dsa
    atts = [dsa.Attribute(e.values, attribute_type=e.attribute_type, normalized=bool(e.normalized), quantization_bits=e.quantization_bits, corners=e.corners) for e in c.extras]
    o = dict(c.opt)
    cfg = dict(weld_points=c.form == 2, weld_attributes=c.weld_attributes, repair_topology=o.pop("repair_topology", 0) != 0, repair_seams=c.opt.get("repair_topology", 0) == 2,
               traversal_method=o.pop("traversal_method", 0), position_prediction=1, texcoord_prediction=1)
    mp = o.pop("pos_prediction", 1)
    if mp in (2, 4):
        cfg["multi_parallelogram"] = mp
    else:
        cfg["position_prediction"] = mp
    up = o.pop("uv_prediction", 1)
    assert (up == mp) if (mp in (2, 4) or up in (2, 4)) else True, "multi_parallelogram replaces Parallelogram for the positions and the first UV set alike"
    cfg["texcoord_prediction"] = 1 if up in (2, 4) else up
    if o.pop("predictive_connectivity", 0) == 2:
        cfg["edgebreaker_method"] = 2
    cfg["normal_prediction"] = o.pop("normal_prediction", 0)
    cfg["single_connectivity"] = bool(o.pop("single_connectivity", 0))
    assert not o, o
    if c.form == 0:
        cfg = dict(encoding_method=0)
        if c.geometry == 0:
            return dsa.PointCloudData(c.pos, c.nrm, c.uv, c.generic, attributes=atts), cfg
    return dsa.MeshData(c.pos, c.faces, c.nrm, c.uv, c.generic, c.nid, c.uid, attributes=atts), cfg


# ------------------------------------------------------------------------------------------------------------------------ the pins
Decoded = collections.namedtuple("Decoded", "values portable point_map seq_type q_min q_range q_bits oct_bits")


def from_oracle(ref):
    return [Decoded(a.values, a.portable, a.point_map, a.seq_type, a.q_min, a.q_range, a.q_bits, a.oct_bits) for a in ref.attributes], ref.num_points


def from_device(mesh):
    """A decoder.Mesh / PointCloud of the device decode."""
    out = []
    for a in mesh.Attributes:
        out.append(Decoded(a.Values, a.PortableValues, a.PointMap, a.DecoderType, list(a.MinValues) + [0.0] * 4, a.Range, a.QuantizationBits, a.QuantizationBits))
    return out, mesh.PointsCount


def rows_by_point(entry_rows, decoded, num_points):
    """rows[a][p] = entry_rows[a][map[a][p]], the identity map where none is stored; an entry past the tracked ones: 0xFFFFFFFF."""
    out = []
    for r, d in zip(entry_rows, decoded):
        m = np.asarray(d.point_map, np.int64) if len(d.point_map) else np.arange(num_points, dtype=np.int64)
        r = np.asarray(r, np.uint32)
        out.append(np.where(m < len(r), r[np.minimum(m, max(len(r) - 1, 0))] if len(r) else 0, 0xFFFFFFFF).astype(np.uint32))
    return out


def at_points(d, what, num_points):
    m = np.asarray(d.point_map, np.int64) if len(d.point_map) else np.arange(num_points, dtype=np.int64)
    return np.asarray(what)[m]


def check_bytes(c, decoded, num_points, rows):
    """Pin (b) for every attribute of the stream."""
    vals = values(c)
    assert len(vals) == len(decoded) == len(rows), (c.name, len(vals), len(decoded), len(rows))
    for a, (v, d, r) in enumerate(zip(vals, decoded, rows)):
        assert len(r) == num_points and (len(r) == 0 or int(r.max()) < len(v)), (c.name, a)
        src = v[r.astype(np.int64)]
        if d.seq_type == 1:
            assert at_points(d, d.values, num_points).tobytes() == np.ascontiguousarray(src).tobytes(), (c.name, a)
        elif d.seq_type == 3:
            assert np.array_equal(at_points(d, d.portable, num_points), meshutil.oct_quantize(src, d.oct_bits)), (c.name, a)
        else:
            nc = src.shape[1]
            want = meshutil.quantize(src, np.asarray(d.q_min[:nc], np.float32), np.float32(d.q_range), d.q_bits)
            assert np.array_equal(at_points(d, d.portable, num_points), want), (c.name, a)


def with_counters(c):
    """Pin (a), form 1: the case with a uint32 arange(V) per vertex and, per attribute given per corner, an int32 arange(R) with
    its ids, behind its own attributes (ids are taken up to index 7 of the stream: the counters of the first attributes that fit)."""
    assert c.form == 1
    extras = list(c.extras)
    base = 1 + (c.nrm is not None) + (c.uv is not None) + (c.generic is not None)
    given = [(1, c.nid, c.nrm)] if c.nrm is not None and c.nid is not None else []
    given += [(1 + (c.nrm is not None), c.uid, c.uv)] if c.uv is not None and c.uid is not None else []
    given += [(base + k, e.corners, e.values) for k, e in enumerate(c.extras) if e.corners is not None]
    mirrors = []
    for index, ids, rows in given:
        if base + len(extras) > 7:
            break
        mirrors.append((index, base + len(extras)))
        extras.append(synth.Extra(np.arange(len(rows), dtype=np.int32), corners=ids))
    extras.append(synth.Extra(np.arange(len(c.pos), dtype=np.uint32)))
    return c._replace(extras=extras), base + len(extras) - 1, mirrors


def check_counters(c, counter, mirrors, decoded, num_points, rows):
    """Pin (a) on a case of with_counters: `counter` the index of arange(V) in the stream, mirrors [(attribute, its arange(R))]."""
    v = at_points(decoded[counter], decoded[counter].values, num_points).reshape(-1).astype(np.uint32)
    for a, pv in enumerate(per_vertex(c)):
        if pv:
            assert np.array_equal(rows[a], v), (c.name, a)
    for a, m in mirrors:
        own = at_points(decoded[m], decoded[m].values, num_points).reshape(-1).astype(np.uint32)
        assert np.array_equal(rows[m], own), (c.name, m)
        assert np.array_equal(rows[a], own), (c.name, a)


def check_normals(c, decoded, num_points, rows):
    """Pin (c): the case's normals are of the 14 directions."""
    n = 1
    got = at_points(decoded[n], decoded[n].values, num_points).astype(np.float64)
    want = np.asarray(c.nrm, np.float64)[rows[n].astype(np.int64)]
    dots = (got * want).sum(axis=1) / np.linalg.norm(got, axis=1)
    assert len(dots) == num_points and (num_points == 0 or dots.min() > 0.99), (c.name, float(dots.min()))


# ----------------------------------------------------------------------------------------------------------------------- the cases
GRIDS = [("grid5x4", synth.GRID, 4, 3), ("grid17x13", synth.GRID, 16, 12), ("holes16x12", synth.HOLES, 16, 12), ("torus9x7", synth.TORUS, 9, 7),
         ("sphere8x6", synth.SPHERE, 8, 6), ("two-parts10x7", synth.TWO_PARTS, 10, 7)]
DIALECTS = [dict(), dict(predictive_connectivity=2), dict(traversal_method=1), dict(traversal_method=2, pos_prediction=4, uv_prediction=4), dict(pos_prediction=0, single_connectivity=1)]

_cases = None


def cases():
    """Every kind of input the issue names, small: {group: [Case]}."""
    global _cases
    if _cases is not None:
        return _cases
    out = collections.OrderedDict()
    grids = []
    for k, (name, kind, nx, ny) in enumerate(GRIDS):
        pos, nrm, uv, faces = synth.make_mesh(kind, nx, ny, 3 + k)
        gen = (np.arange(2 * len(pos)) * 7 % 251).astype(np.uint8).reshape(-1, 2) if k % 2 else None
        for j, d in enumerate(DIALECTS):
            if (j + k) % 2 == 0 or j == 0:
                grids.append(case("%s/%d" % (name, j), 1, pos, faces, nrm, None, uv, None, gen, opt=d))
    out["grids"] = grids
    seamed = []
    for k, (name, kind, nx, ny) in enumerate(GRIDS[:5]):
        charts = seamdefects.CHARTS[k % len(seamdefects.CHARTS)]
        m = seamdefects.seamed_source(synth, name, kind, nx, ny, charts, 5 + k)
        for j, d in enumerate(DIALECTS[:4]):
            if (j + k) % 2 == 0:
                seamed.append(case("%s/%d" % (m.name, j), 1, m.pos, m.faces, m.nrm, m.nid, m.uv, m.uid, opt=d))
    for k, (name, charts, args) in enumerate(irregular.seamed_small()):
        pos, faces, nrm, nid, uv, uid = args
        seamed.append(case("irregular/%s" % name, 1, pos, faces, nrm, nid, uv, uid, opt=DIALECTS[k % 4]))
    out["seamed"] = seamed
    listed = []
    for k, kc in enumerate(cornerattrcases.CASES[:9] + cornerattrcases.IRREGULAR[::3]):
        b = cornerattrcases.build(kc)
        listed.append(case("listed/%s" % b.name, 1, b.pos, b.faces, b.nrm, b.nid, b.uv, b.uid, extras=b.extras, opt=DIALECTS[k % 4]))
    out["listed"] = listed
    repaired = []
    for k, dfc in enumerate(defects.named() + defects.placed() + defects.injected_small()[::2]):
        pos, nrm, uv, gen, extra = defects.attributes(dfc.nv, k)
        repaired.append(case("repaired/%s" % dfc.name, 1, pos, dfc.faces, nrm, None, uv, None, gen, [synth.Extra(extra)], opt=dict(DIALECTS[k % 4], repair_topology=1)))
    for k, dfc in enumerate(defects.named()[:6] + defects.placed()[:3]):
        m = seamdefects.with_ids(dfc, seamdefects.ID_KINDS[k % 3], k)
        repaired.append(case("repaired-ids/%s" % m.name, 1, m.pos, m.faces, m.nrm, m.nid, m.uv, m.uid, opt=dict(seamdefects.OPTIONS[k % 2 * 2], repair_topology=2)))
    clean = seamdefects.seamed_source(synth, "grid", synth.GRID, 6, 5, (None, "stripes"), 6)
    for kind in ("double", "pinch", "degenerate"):
        m = seamdefects.inject(clean, kind, 2, np.random.default_rng(12))
        repaired.append(case("repaired-ids/%s" % m.name, 1, m.pos, m.faces, m.nrm, m.nid, m.uv, m.uid, opt=dict(repair_topology=2)))
    out["repaired"] = repaired
    welded = []
    for k, wc in enumerate(weldcases.small_cases()):
        if wc.refused or wc.weld_only or len(wc.pos) < 3:
            continue
        if k % 3 and len(wc.pos) > 60:
            continue
        extras = weldcases.extras_of(wc)
        welded.append(case("weld/%s" % wc.name, 2, wc.pos, wc.faces, wc.normals, None, wc.uvs, None, wc.generic, extras, opt=dict(DIALECTS[k % 4], repair_topology=2 if k % 2 else 0)))
    for k, kc in enumerate([kc for kc in cornerattrcases.CASES if any(cut is not None for _, cut in kc.attrs)][:10:2]):
        b = cornerattrcases.build(kc)
        pos, faces, nrm, uv, arrays = cornerattrcases.unweld(b, np.random.default_rng(3 + k))
        extras = cornerattrcases.point_extras(b, arrays)
        welded.append(case("weld-attributes/%s" % b.name, 2, pos, faces, nrm, None, uv, None, None, extras, opt=dict(repair_topology=2), weld_attributes=True))
        welded.append(case("weld-in-key/%s" % b.name, 2, pos, faces, nrm, None, uv, None, None, extras, opt=dict(repair_topology=2)))
    out["welded"] = welded
    linear = []
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 6, 4, 2)
    linear.append(case("sequential", 0, pos, faces, nrm, None, uv, None, None, [synth.Extra(np.arange(len(pos), dtype=np.uint16))]))
    linear.append(case("point-cloud", 0, pos, np.zeros((0, 3), np.uint32), nrm, None, uv, geometry=0))
    out["linear"] = linear
    seen = collections.Counter()
    for group in out.values():                                # (the generators reuse names across chart patterns)
        for k, c in enumerate(group):
            seen[c.name] += 1
            if seen[c.name] > 1:
                group[k] = c._replace(name="%s#%d" % (c.name, seen[c.name]))
    _cases = out
    return out


def all_cases():
    return [c for group in cases().values() for c in group]
