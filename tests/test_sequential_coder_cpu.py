"""The CPU coder of sequential streams (draco-sharp_amd/csrc/dsa_encode_host.h: write_sequential_stream, encode_sequential; through
synth.encode_sequential / synth.encode_point_cloud_attributes) against the oracle: the statement of what
dsa_encode_sequential_batch must write.  Decoded faces equal the input array element for element, point i is input vertex i, and
the values equal the numpy quantisation of the input (tests/seqcases.py check_decoded) -- not the coder's own arithmetic.  CPU only."""
import itertools

import numpy as np
import pytest

import draco_sharp_amd.synth as synth
import irregular
import oracle
import seqcases

SUBSETS = list(itertools.product((False, True), repeat=3))          # normals, texture coordinates, generic


def attributes(pos, nrm, uv, subset, components=3, seed=0):
    n, u, g = subset
    return (nrm if n else None, uv if u else None, seqcases.generic_of(len(pos), components, seed) if g else None)


@pytest.mark.parametrize("compressed", [False, True])
@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("subset", SUBSETS)
def test_mesh_with_each_attribute_subset(subset, scheme, compressed):
    pos, nrm, uv, faces = synth.make_mesh(synth.TORUS, 17, 23, 7)
    n, u, g = attributes(pos, nrm, uv, subset, components=1 + sum(subset))
    data = synth.encode_sequential(pos, faces, n, u, g, compressed=compressed, opt=synth.options(force_scheme=scheme))
    seqcases.check_decoded(oracle.decode(data), pos, faces, n, u, g)
    if not subset[2]:          # the entry point of before keeps its bytes
        assert data == synth.encode_mesh_sequential(pos, faces, n, u, compressed, synth.options(force_scheme=scheme))


@pytest.mark.parametrize("compressed", [False, True])
@pytest.mark.parametrize("points", sorted(seqcases.WIDTH_GRIDS))
def test_index_width_boundaries(points, compressed):
    pos, nrm, uv, faces = seqcases.grid(points)
    faces = faces.copy()
    faces[-1, 2] = points - 1                                       # the largest index occurs
    gen = seqcases.generic_of(points, 4)
    data = synth.encode_sequential(pos, faces, nrm, uv, gen, compressed=compressed)
    seqcases.check_decoded(oracle.decode(data), pos, faces, nrm, uv, gen)
    if not compressed:          # header 11, face and point count, connectivity method, then the indices at the width of `points`
        head = 11 + len(synth_varint(len(faces))) + len(synth_varint(points)) + 1
        if points < 65536:      # u8 below 256 points, u16 below 65 536
            raw = np.frombuffer(data, np.uint8 if points < 256 else "<u2", 3 * len(faces), head)
            assert np.array_equal(raw, faces.ravel())
        else:                   # varints from 65 536 points on: the indices of this mesh take one to three bytes
            want = b"".join(synth_varint(int(v)) for v in faces.ravel())
            assert data[head:head + len(want)] == want


def synth_varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


@pytest.mark.parametrize("compressed", [False, True])
def test_varint_indices_above_65536_points(compressed):
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 300, 250, 3)      # 75 551 points
    data = synth.encode_sequential(pos, faces, nrm, uv, None, compressed=compressed)
    seqcases.check_decoded(oracle.decode(data), pos, faces, nrm, uv)
    # stream sizes of this mesh are counts, not timings: what the issue of this feature records
    assert len(data) == (357578 if compressed else 1464503)


@pytest.mark.parametrize("subset", SUBSETS)
@pytest.mark.parametrize("points", [1, 777, 100000])
def test_point_cloud_with_each_attribute_subset(points, subset):
    rng = np.random.default_rng(points)
    pos = np.cumsum(rng.normal(size=(points, 3)), axis=0).astype(np.float32)
    nrm = rng.normal(size=(points, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    uv = rng.random((points, 2)).astype(np.float32)
    n, u, g = attributes(pos, nrm, uv, subset, components=2, seed=points)
    data = synth.encode_point_cloud_attributes(pos, n, u, g)
    seqcases.check_decoded(oracle.decode(data), pos, None, n, u, g)
    if subset == (False, False, False):
        assert data == synth.encode_point_cloud(pos)                # byte for byte


@pytest.mark.parametrize("scheme", [-1, 0, 1])
def test_positions_only_cloud_equals_the_old_writer(scheme):
    pos, _, _, _ = synth.make_mesh(synth.SPHERE, 30, 31, 2)
    for bits in (4, 11, 18):
        opt = synth.options(pos_bits=bits, force_scheme=scheme)
        assert synth.encode_point_cloud_attributes(pos, opt=opt) == synth.encode_point_cloud(pos, opt)


@pytest.mark.parametrize("compressed", [False, True])
def test_meshes_edgebreaker_refuses(compressed):
    for name, pos, nrm, uv, faces in seqcases.refused_by_edgebreaker():
        with pytest.raises(RuntimeError, match="non-manifold|degenerate|isolated"):
            synth.encode_mesh(pos, faces, nrm, uv)
        gen = seqcases.generic_of(len(pos), 1)
        data = synth.encode_sequential(pos, faces, nrm, uv, gen, compressed=compressed)
        seqcases.check_decoded(oracle.decode(data), pos, faces, nrm, uv, gen)


@pytest.mark.parametrize("case", irregular.CASES, ids=lambda c: c.name)
def test_irregular_cases(case):
    pos, nrm, uv, faces = irregular.mesh(case)
    for compressed in (False, True):
        data = synth.encode_sequential(pos, faces, nrm, uv, None, compressed=compressed)
        seqcases.check_decoded(oracle.decode(data), pos, faces, nrm, uv)


@pytest.mark.parametrize("bits", [(4, 4, 4), (14, 10, 12), (18, 18, 18)])
def test_quantisation_bits(bits):
    pos, nrm, uv, faces = synth.make_mesh(synth.HOLES, 20, 16, 9)
    opt = synth.options(pos_bits=bits[0], normal_bits=bits[1], uv_bits=bits[2])
    data = synth.encode_sequential(pos, faces, nrm, uv, None, compressed=True, opt=opt)
    seqcases.check_decoded(oracle.decode(data), pos, faces, nrm, uv, bits=bits)


def test_argument_checks_of_the_cpu_entry_point():
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 4, 4, 1)
    bad = faces.copy()
    bad[3, 1] = len(pos)
    with pytest.raises(RuntimeError, match="out of range"):
        synth.encode_sequential(pos, bad)
    with pytest.raises(ValueError, match="generic"):
        synth.encode_sequential(pos, faces, generic=np.zeros((len(pos), 5), np.uint8))
    with pytest.raises(RuntimeError, match="needs faces"):
        synth.encode_sequential(pos, faces[:0])
