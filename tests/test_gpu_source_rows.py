"""The rows a coded stream carries, on the device: dsa_encode_rows_batch with track_rows = 1 keeps per stream and attribute the row
of the caller's arrays every entry carries (k_enc_entry_rows, dsa_encoded_entry_rows).  Held exactly to the host coder's twin
(synth.entry_rows) on both connectivity and both weld paths (the switches of tests/test_gpu_encode_corner_attributes.py), with the
streams byte for byte what they are without the option and through the older entry points; and held, through the device's own
decode of the same streams, to the pins of tests/rowcases.py, which know nothing of either coder's bookkeeping.  A crowded batch
over chunks of 37 with refused meshes in between gives every mesh its own rows or its own status.
dsa_batch_source_rows (k_source_rows behind the decode, Batch.source_rows) gathers rows[a][p] = entry_rows[a][map[a][p]] on the
device: against the same gather on the host and against the pins; streams named through a permutation, a stream that is not the
one named failing alone, the request queued before the wait, the device-only form, a second decode invalidating the arrays, the
identity of sequential streams and point clouds, the general decode path (traversal_method 1 and 2, seams, valence)."""
import collections

import numpy as np
import pytest

import rowcases as R
import draco_sharp_amd as dsa
from draco_sharp_amd import native
from draco_sharp_amd.encoder import _entry_rows

pytestmark = pytest.mark.gpu

PATHS = pytest.mark.parametrize("weld_host,conn_host", [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")])
GROUPS = R.cases()
EDGEBREAKER = [c for name, group in GROUPS.items() if name != "linear" for c in group]


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


def force_paths(monkeypatch, weld_host, conn_host):
    for name, value in (("DSA_ENC_HOST_WELD", weld_host), ("DSA_ENC_HOST_CONN", conn_host), ("DSA_ENC_HOST_PLAN", conn_host)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    monkeypatch.delenv("DSA_ENC_CHUNK", raising=False)


def batches(cases):
    """The cases by the Config that codes them: [(config fields, [case], [MeshData])]."""
    out = collections.OrderedDict()
    for c in cases:
        m, cfg = R.mesh_data(c)
        slot = out.setdefault(tuple(sorted(cfg.items())), (cfg, [], []))
        slot[1].append(c)
        slot[2].append(m)
    return list(out.values())


@pytest.fixture(scope="module")
def cpu():
    """Per case name the host coder's stream and entry rows, computed once."""
    return {c.name: (R.encode(c), R.twin(c)) for c in R.all_cases()}


def same_rows(got, want):
    return len(got) == len(want) and all(g.dtype == np.uint32 and np.array_equal(g, w) for g, w in zip(got, want))


@PATHS
def test_entry_rows_equal_the_host_coder(ctx, monkeypatch, cpu, weld_host, conn_host):
    force_paths(monkeypatch, weld_host, conn_host)
    enc = dsa.DracoEncoder(ctx)
    for cfg, cases, meshes in batches(EDGEBREAKER):
        if weld_host == "1" and not cfg["weld_points"]:
            continue                                          # (the weld switch moves nothing of a batch that is not welded)
        got = enc.EncodeBatch(meshes, dsa.Config(track_rows=True, **cfg))
        for i, c in enumerate(cases):
            assert got[i] == cpu[c.name][0], (c.name, cfg)
            assert same_rows(got.entry_rows(i), cpu[c.name][1]), (c.name, cfg)
        got.close()


def test_the_option_changes_no_byte(ctx, monkeypatch):
    """Config(track_rows=True) against Config(): the new call with tracking on against the entry point a batch took before
    (the new call with tracking off: test_the_new_call_with_tracking_off_is_the_old_call)."""
    force_paths(monkeypatch, None, None)
    enc = dsa.DracoEncoder(ctx)
    L = native.lib()
    for cfg, cases, meshes in batches(EDGEBREAKER):
        on = enc.EncodeBatch(meshes, dsa.Config(track_rows=True, **cfg))
        off = enc.EncodeBatch(meshes, dsa.Config(**cfg))      # dsa_encode_seam_repair_batch / dsa_encode_corner_attributes_batch
        assert on == off, cfg
        # a handle without tracking: refused, and the message says what to set
        count = native.C.c_uint32(7)
        assert L.dsa_encoded_entry_rows(off._h, 0, 0, None, 0, native.C.byref(count)) == native.DSA_ERR_INVALID_ARGUMENT and count.value == 0
        assert "track_rows" in ctx.error()
        with pytest.raises(ValueError, match="track_rows"):
            off.entry_rows(0)
        on.close()
        off.close()


def answers(ctx, h, n):
    """Per mesh of an encoded handle (status, the stream's bytes or the refusal's message)."""
    L, C = native.lib(), native.C
    out, p, ln = [], C.c_void_p(), C.c_size_t()
    for i in range(n):
        st = L.dsa_encoded_stream(h, i, C.byref(p), C.byref(ln))
        out.append((st, C.string_at(p, ln.value) if st == 0 else ctx.error()))
    return out


def test_the_new_call_with_tracking_off_is_the_old_call(ctx, monkeypatch):
    """dsa_encode_rows_batch with track_rows = 0 against the entry point a batch took before (dsa_encode_seam_repair_batch, or
    dsa_encode_corner_attributes_batch where there are listed ids or weld_attributes) and against track_rows = 1: the same meshes,
    a refused one among them -- the same bytes, statuses and messages three ways; and the handle of the new call with tracking off
    refuses its rows and names track_rows."""
    from draco_sharp_amd.encoder import _fill_attribute_corners, _native_meshes
    force_paths(monkeypatch, None, None)
    L, C = native.lib(), native.C
    enc = dsa.DracoEncoder(ctx)
    for cfg, cases, meshes in batches(EDGEBREAKER):
        bad, _ = R.mesh_data(cases[0])
        bad.faces = bad.faces + np.uint32(len(bad.positions))          # every index out of range: refused alone
        meshes = meshes[:1] + [bad] + meshes[1:]
        n = len(meshes)
        config = dsa.Config(**cfg)
        _, old, _ = enc.EncodeBatch(meshes, config, handle=True)
        arr, grids, keep = _native_meshes(meshes)
        corners = (native.MeshAttributeCorners * n)()
        for i, m in enumerate(meshes):
            _fill_attribute_corners(corners[i], m, keep)
        handles = [old]
        try:
            for track in (0, 1):
                o = native.EncodeRowsOptions()
                L.dsa_encode_default_rows_options(C.byref(o))
                o.corner_attributes.seam_repair.grid.repair = config._native_repair()
                o.corner_attributes.seam_repair.grid.weld_points = int(config.weld_points)
                o.corner_attributes.seam_repair.corner_repair = int(config.repair_seams)
                o.corner_attributes.weld_attributes = int(config.weld_attributes)
                o.track_rows = track
                h = C.c_void_p()
                assert L.dsa_encode_rows_batch(ctx._h, n, arr, grids, corners, C.byref(o), C.byref(h)) == 0, ctx.error()
                handles.append(h)
            want = answers(ctx, old, n)
            assert want[1][0] == native.DSA_ERR_INVALID_DATA and "face index out of range" in want[1][1] and all(st == 0 for k, (st, _) in enumerate(want) if k != 1), cfg
            assert answers(ctx, handles[1], n) == want, cfg          # tracking off
            assert answers(ctx, handles[2], n) == want, cfg          # tracking on
            count = C.c_uint32(7)
            for h in handles[:2]:                                     # neither kept rows: refused, and the message says what to set
                assert L.dsa_encoded_entry_rows(h, 0, 0, None, 0, C.byref(count)) == native.DSA_ERR_INVALID_ARGUMENT and count.value == 0 and "track_rows" in ctx.error()
                assert L.dsa_encoded_attributes(h, 0, C.byref(count)) == native.DSA_ERR_INVALID_ARGUMENT and "track_rows" in ctx.error()
            assert L.dsa_encoded_attributes(handles[2], 0, C.byref(count)) == 0 and count.value == len(R.values(cases[0]))
            assert L.dsa_encoded_attributes(handles[2], 1, C.byref(count)) == native.DSA_ERR_INVALID_DATA and count.value == 0      # the refused mesh: its own status
        finally:
            for h in handles:
                L.dsa_encoded_free(h)


def test_the_accessor_answers_as_the_header_says(ctx, monkeypatch):
    force_paths(monkeypatch, None, None)
    L, C = native.lib(), native.C
    c = GROUPS["seamed"][0]
    m, cfg = R.mesh_data(c)
    bad = dsa.MeshData(c.pos, c.faces + np.uint32(len(c.pos)), c.nrm, c.uv, None, c.nid, c.uid)      # every index out of range
    _, h, n = dsa.DracoEncoder(ctx).EncodeBatch([m, bad], dsa.Config(track_rows=True, **cfg), handle=True)
    try:
        count = C.c_uint32()
        assert L.dsa_encoded_entry_rows(h, 0, 0, None, 0, C.byref(count)) == 0 and count.value == len(R.twin(c)[0])
        small = np.full(count.value, 0xABABABAB, np.uint32)
        assert L.dsa_encoded_entry_rows(h, 0, 0, small.ctypes.data, count.value - 1, C.byref(count)) == native.DSA_ERR_INVALID_ARGUMENT
        assert count.value == len(small) and (small == 0xABABABAB).all()          # too little room: nothing written, the count said
        assert L.dsa_encoded_entry_rows(h, 0, 3, None, 0, C.byref(count)) == native.DSA_ERR_INVALID_ARGUMENT      # positions, normals, texcoords: 0 .. 2
        assert L.dsa_encoded_entry_rows(h, 1, 0, None, 0, C.byref(count)) == native.DSA_ERR_INVALID_DATA and "face index out of range" in ctx.error()
        assert L.dsa_encoded_entry_rows(h, 2, 0, None, 0, C.byref(count)) == native.DSA_ERR_INVALID_ARGUMENT      # no such mesh
    finally:
        L.dsa_encoded_free(h)


@pytest.mark.parametrize("c", GROUPS["linear"], ids=lambda c: c.name)
def test_sequential_handles_answer_with_the_identity(ctx, cpu, c):
    m, cfg = R.mesh_data(c)
    got = dsa.DracoEncoder(ctx).EncodeBatch([m], dsa.Config(**cfg))
    assert got[0] == cpu[c.name][0]
    assert same_rows(got.entry_rows(0), cpu[c.name][1]) and len(cpu[c.name][1]) == len(R.values(c))
    got.close()


PATHS_SEEN = collections.Counter()


def decode_rows(ctx, encoded, cases):
    """The device's decode of the streams and its source rows: per case (decoded attributes, points, rows by point)."""
    b = dsa.Batch(ctx, list(encoded))
    b.decode()
    got = b.source_rows(encoded)
    out = []
    for i, c in enumerate(cases):
        assert b.status(i) == 0, c.name
        PATHS_SEEN[b.mesh_info(i).decode_path] += 1
        decoded, num_points = R.from_device(b.result(i).ConnectedData)
        want = R.rows_by_point(encoded.entry_rows(i), decoded, num_points)          # the same gather on the host
        assert not isinstance(got[i], Exception), (c.name, got[i])
        assert same_rows(got[i], want), c.name
        out.append((decoded, num_points, [np.array(r) for r in got[i]]))
    b.close()
    return out


def test_counters_bytes_and_normals_through_the_device_decode(ctx, monkeypatch):
    """Pins (a), (b), (c) of tests/rowcases.py with the entry rows of the device encoder and the point maps of the device decoder."""
    force_paths(monkeypatch, "0", "0")
    enc = dsa.DracoEncoder(ctx)
    indexed = [R.with_counters(c) for c in GROUPS["grids"][::2] + GROUPS["seamed"][::2] + GROUPS["listed"][::2] + GROUPS["repaired"][::2]]
    for cfg, cases, meshes in batches([cc for cc, _, _ in indexed]):
        extra = {cc.name: (counter, mirrors) for cc, counter, mirrors in indexed}
        got = enc.EncodeBatch(meshes, dsa.Config(track_rows=True, **cfg))
        for c, (decoded, num_points, rows) in zip(cases, decode_rows(ctx, got, cases)):
            R.check_counters(c, *extra[c.name], decoded, num_points, rows)
            R.check_bytes(c, decoded, num_points, rows)
        got.close()
    directed = [R.with_directions(c) for c in GROUPS["welded"] + GROUPS["seamed"][1::4] if c.nrm is not None]
    for cfg, cases, meshes in batches(directed):
        got = enc.EncodeBatch(meshes, dsa.Config(track_rows=True, **cfg))
        for c, (decoded, num_points, rows) in zip(cases, decode_rows(ctx, got, cases)):
            R.check_bytes(c, decoded, num_points, rows)
            R.check_normals(c, decoded, num_points, rows)
        got.close()
    # traversal_method 1 / 2, seams and valence symbols leave the wave-per-mesh kernels (decode_path 1); decode_path 2, the retry
    # batch, is taken by none of the suite's small streams
    assert PATHS_SEEN[0] > 0 and PATHS_SEEN[1] > 0, dict(PATHS_SEEN)
    print("decode paths of the meshes whose source rows were checked:", dict(PATHS_SEEN))


def test_streams_named_through_a_permutation_and_one_that_is_not_the_one_named(ctx, monkeypatch):
    force_paths(monkeypatch, "0", "0")
    cfg, cases, meshes = max(batches(GROUPS["seamed"] + GROUPS["listed"]), key=lambda x: len(x[1]))
    n = len(cases)
    assert n >= 4
    encoded = dsa.DracoEncoder(ctx).EncodeBatch(meshes, dsa.Config(track_rows=True, **cfg))
    perm = np.random.default_rng(4).permutation(n).astype(np.uint32)
    b = dsa.Batch(ctx, [encoded[int(k)] for k in perm])
    b.decode(wait=False)
    assert b.source_rows(encoded, encoded_mesh=perm, wait=False) is None          # queued behind the kernels; the wait covers it
    b.wait()
    for i in range(n):
        decoded, num_points = R.from_device(b.result(i).ConnectedData)
        assert same_rows(b.source_row_views(i), R.rows_by_point(encoded.entry_rows(int(perm[i])), decoded, num_points)), cases[int(perm[i])].name
    # one mesh held against another's stream: it fails alone, with the argument's status, the others have their arrays
    sizes = encoded.sizes
    wrong = perm.copy()
    other = next(k for k in range(n) if sizes[k] != sizes[int(perm[0])])
    wrong[0] = other
    got = b.source_rows(encoded, encoded_mesh=wrong)
    assert isinstance(got[0], ValueError) and "not stream %d" % other in str(got[0])
    for i in range(1, n):
        decoded, num_points = R.from_device(b.result(i).ConnectedData)
        assert same_rows(got[i], R.rows_by_point(encoded.entry_rows(int(perm[i])), decoded, num_points))
    with pytest.raises(ValueError):
        b.source_rows(encoded, encoded_mesh=perm[:-1])
    # the device-only form: the same numbers, nothing on the host
    want = [[np.array(r) for r in rows] for rows in b.source_rows(encoded, encoded_mesh=perm)]
    dev = b.source_rows(encoded, encoded_mesh=perm, device_only=True)
    with pytest.raises(RuntimeError):
        b.source_row_views(0)
    for rows, tensors in zip(want, dev):
        assert all(np.array_equal(r.view(np.int32), t.cpu().numpy()) for r, t in zip(rows, tensors))
    # a second decode invalidates the arrays
    b.decode()
    with pytest.raises(ValueError, match="no source rows were requested since the batch was decoded"):
        b.source_row_views(0)
    # a handle without rows: the call fails and says what to set
    plain = dsa.DracoEncoder(ctx).EncodeBatch(meshes, dsa.Config(**cfg))
    with pytest.raises(ValueError, match="track_rows"):
        b.source_rows(plain)
    plain.close()
    b.close()
    encoded.close()


def test_a_stream_of_the_same_length_with_other_entry_counts_fails_alone(ctx, monkeypatch):
    """What the host cannot tell at the request: mesh 1 of the batch is the small mesh's stream filled up to the large one's
    length (a decoder reads no further than the stream's end), named as the large one's.  Lengths and attribute counts agree, the
    entry counts do not: nothing is gathered for it, the layout call says so, and its neighbours have their rows."""
    force_paths(monkeypatch, None, None)
    small, large = GROUPS["grids"][0], next(c for c in GROUPS["grids"] if len(c.pos) > 150 and not c.opt and c.generic is None)
    assert len(R.values(small)) == len(R.values(large))
    meshes = [R.mesh_data(small)[0], R.mesh_data(large)[0]]
    encoded = dsa.DracoEncoder(ctx).EncodeBatch(meshes, dsa.Config(track_rows=True))
    assert len(encoded[0]) < len(encoded[1])
    padded = encoded[0] + bytes(len(encoded[1]) - len(encoded[0]))
    b = dsa.Batch(ctx, [encoded[0], padded, encoded[1]])
    b.decode()
    assert [b.status(i) for i in range(3)] == [0, 0, 0]
    got = b.source_rows(encoded, encoded_mesh=[0, 1, 1])
    assert isinstance(got[1], ValueError) and "entries decoded" in str(got[1]) and "tracked" in str(got[1])
    for i, k in ((0, 0), (2, 1)):
        decoded, num_points = R.from_device(b.result(i).ConnectedData)
        assert same_rows(got[i], R.rows_by_point(encoded.entry_rows(k), decoded, num_points))
    lay = native.MeshSourceRows()
    assert native.lib().dsa_batch_source_rows_layout(b._h, 1, native.C.byref(lay)) == native.DSA_ERR_INVALID_ARGUMENT
    b.close()
    encoded.close()


def test_sequential_streams_and_point_clouds_carry_their_own_rows(ctx):
    for c in GROUPS["linear"]:
        m, cfg = R.mesh_data(c)
        encoded = dsa.DracoEncoder(ctx).EncodeBatch([m, m], dsa.Config(**cfg))
        for decoded, num_points, rows in decode_rows(ctx, encoded, [c, c]):
            assert num_points == len(c.pos) and all(np.array_equal(r, np.arange(num_points, dtype=np.uint32)) for r in rows)
            R.check_bytes(c, decoded, num_points, rows)
        encoded.close()


def test_call_level_refusals_name_the_field(ctx):
    L, C = native.lib(), native.C
    h = C.c_void_p()
    o = native.EncodeRowsOptions()
    for field, edit in (("track_rows 2", lambda o: setattr(o, "track_rows", 2)), ("dsa_encode_rows_options.reserved[5]", lambda o: o.reserved.__setitem__(5, 1)),
                        ("dsa_encode_corner_attributes_options.reserved[0]", lambda o: o.corner_attributes.reserved.__setitem__(0, 9))):
        L.dsa_encode_default_rows_options(C.byref(o))
        edit(o)
        assert L.dsa_encode_rows_batch(ctx._h, 0, None, None, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT
        assert field in ctx.error(), (field, ctx.error())
    L.dsa_encode_default_rows_options(C.byref(o))
    o.track_rows = 1
    assert L.dsa_encode_rows_batch(ctx._h, 0, None, None, None, C.byref(o), C.byref(h)) == 0 and L.dsa_encoded_size(h) == 0
    L.dsa_encoded_free(h)


@pytest.mark.parametrize("weld", [False, True], ids=["indexed", "per-point"])
def test_crowded_batch_with_refused_meshes(ctx, monkeypatch, weld):
    """300 meshes over chunks of 37 on the device paths (a batch of 256 and more), every seventh mesh refused, the meshes that
    need the repair coded in its second pass: every mesh has its own rows, exactly the host coder's, or its own status."""
    force_paths(monkeypatch, None, None)
    monkeypatch.setenv("DSA_ENC_CHUNK", "37")
    opt = dict(repair_topology=2)
    if weld:
        pool = [c._replace(opt=opt) for c in GROUPS["welded"] if c.weld_attributes]
    else:
        pool = [c._replace(opt=opt) for name in ("grids", "seamed", "listed", "repaired") for c in GROUPS[name] if not c.opt.get("single_connectivity")]
    want = {c.name: (R.encode(c), R.twin(c)) for c in pool}
    cases = [pool[(11 * k) % len(pool)] for k in range(300)]
    meshes, cfg = [], None
    for k, c in enumerate(cases):
        m, cfg = R.mesh_data(c)
        if k % 7 == 3:
            m.faces = m.faces + np.uint32(len(m.positions))      # (every index out of range: refused before anything reads through it)
        meshes.append(m)
    _, h, n = dsa.DracoEncoder(ctx).EncodeBatch(meshes, dsa.Config(track_rows=True, **cfg), handle=True)
    L, C = native.lib(), native.C
    try:
        p, ln, count = C.c_void_p(), C.c_size_t(), C.c_uint32()
        for k, c in enumerate(cases):
            st = L.dsa_encoded_stream(h, k, C.byref(p), C.byref(ln))
            if k % 7 == 3:
                assert st == native.DSA_ERR_INVALID_DATA and "face index out of range" in ctx.error(), (k, c.name)
                assert L.dsa_encoded_entry_rows(h, k, 0, None, 0, C.byref(count)) == native.DSA_ERR_INVALID_DATA and count.value == 0
                continue
            assert st == 0 and C.string_at(p, ln.value) == want[c.name][0], (k, c.name)
            assert same_rows(_entry_rows(ctx, h, k), want[c.name][1]), (k, c.name)
    finally:
        L.dsa_encoded_free(h)
