"""Inputs and pins shared by the sequential-encoder tests (test_sequential_coder_cpu.py, test_gpu_encode_sequential.py,
test_hostcheck_encseq.py): meshes at the boundaries of the index widths, inputs Edgebreaker refuses, and the expected decode of a
sequential stream derived from the INPUT arrays with the numpy restatements of tests/meshutil.py -- the independent pin of
test_independent_pin.py restated for linear order: faces equal the input array element for element, point i is input vertex i,
and the portable values are the numpy quantisation of row i."""
import numpy as np

import draco_sharp_amd.synth as synth
from meshutil import oct_quantize, source_quantization

# (nx, ny) of a GRID with exactly that many vertices: the four widths of raw indices change at 256, 65 536 and 2^21 points
WIDTH_GRIDS = {255: (14, 16), 256: (15, 15), 65535: (254, 256), 65536: (255, 255)}


def generic_of(n, components, seed=0):
    """A uint8 attribute of `components` per point: smooth in the point index with some noise, like vertex colours."""
    rng = np.random.default_rng(1000 + seed)
    base = (np.arange(n)[:, None] * (np.arange(components)[None, :] + 1) // 3) % 251
    return ((base + rng.integers(0, 4, (n, components))) % 256).astype(np.uint8)


def grid(points, seed=5):
    nx, ny = WIDTH_GRIDS[points]
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, nx, ny, seed)
    assert len(pos) == points
    return pos, nrm, uv, faces


def refused_by_edgebreaker():
    """[(name, pos, nrm, uv, faces)]: legal sequential meshes that the Edgebreaker coder refuses."""
    out = []
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 9, 7, 11)
    out.append(("duplicated-and-flipped-face", pos, nrm, uv, np.concatenate([faces, faces[5:6], faces[9:10, ::-1]])))
    extra = np.concatenate([pos, pos[:1] + 2.0]), np.concatenate([nrm, nrm[:1]]), np.concatenate([uv, uv[:1]])
    out.append(("isolated-vertex-and-degenerate-face", *extra, np.concatenate([faces, np.array([[3, 3, 4]], np.uint32)])))
    bow = np.array([[0, 1, 2], [0, 3, 4], [1, 2, 5], [2, 1, 6], [1, 2, 7]], np.uint32)      # a bow-tie vertex and an edge with four faces
    p = np.random.default_rng(3).normal(size=(8, 3)).astype(np.float32)
    out.append(("non-manifold-edge-and-vertex", p, p / np.linalg.norm(p, axis=1, keepdims=True), p[:, :2].copy(), bow))
    return [(n, np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32), np.ascontiguousarray(c, np.float32),
             np.ascontiguousarray(f, np.uint32)) for n, a, b, c, f in out]


def check_decoded(m, pos, faces=None, nrm=None, uv=None, gen=None, bits=(11, 8, 10), kind="mesh"):
    """`m`: a decode by the oracle (tests/oracle.py OracleMesh).  faces None: a point cloud."""
    pos_bits, normal_bits, uv_bits = bits
    assert m.encoder_type == (0 if faces is None else 1) and m.encoder_method == 0
    assert m.num_points == len(pos)
    if faces is None:
        assert m.num_faces == 0
    else:
        assert np.array_equal(np.asarray(m.faces, np.int64), np.asarray(faces, np.int64).reshape(-1, 3))        # element for element
    want = [(0, 3)] + ([(1, 2)] if nrm is not None else []) + ([(3, 2)] if uv is not None else []) + ([(4, None)] if gen is not None else [])
    assert [a.att_type for a in m.attributes] == [t for t, _ in want]
    assert len(m.decoders) == 1
    for a in m.attributes:
        assert len(a.point_map) == 0 or np.array_equal(a.point_map, np.arange(len(pos)))       # point i is entry i
        assert a.pred_method == 0
        if a.att_type == 0:
            mn, rng, q = source_quantization(pos, pos_bits)
            assert a.q_bits == pos_bits and np.array_equal(np.asarray(a.q_min[:3], np.float32), mn) and np.float32(a.q_range) == rng
            assert np.array_equal(np.asarray(a.portable, np.int64), q)
        elif a.att_type == 1:
            assert a.oct_bits == normal_bits and np.array_equal(np.asarray(a.portable, np.int64), oct_quantize(nrm, normal_bits))
        elif a.att_type == 3:
            mn, rng, q = source_quantization(uv, uv_bits)
            assert a.q_bits == uv_bits and np.array_equal(np.asarray(a.q_min[:2], np.float32), mn) and np.float32(a.q_range) == rng
            assert np.array_equal(np.asarray(a.portable, np.int64), q)
        else:
            g = np.asarray(gen, np.uint8).reshape(len(pos), -1)
            assert a.num_components == g.shape[1] and a.data_type == 2
            assert np.array_equal(np.asarray(a.values, np.uint8).reshape(g.shape), g)


def check_decoded_gpu(d, pos, faces=None, nrm=None, uv=None, gen=None, bits=(11, 8, 10)):
    """check_decoded for a decode by the GPU path (dsa.Batch.result(i).ConnectedData)."""
    pos_bits, normal_bits, uv_bits = bits
    assert d.PointsCount == len(pos)
    if faces is None:
        assert not hasattr(d, "Faces") or len(d.Faces) == 0
    else:
        assert np.array_equal(np.asarray(d.Faces, np.int64), np.asarray(faces, np.int64).reshape(-1, 3))
    want = [0] + ([1] if nrm is not None else []) + ([3] if uv is not None else []) + ([4] if gen is not None else [])
    assert [a.AttributeType for a in d.Attributes] == want
    for a in d.Attributes:
        assert np.array_equal(np.asarray(a.PointMap, np.int64), np.arange(len(pos)))
        if a.AttributeType == 0:
            mn, rng, q = source_quantization(pos, pos_bits)
            assert a.QuantizationBits == pos_bits and np.array_equal(np.asarray(a.MinValues, np.float32), mn) and np.float32(a.Range) == rng
            assert np.array_equal(np.asarray(a.PortableValues, np.int64), q)
        elif a.AttributeType == 1:
            assert np.array_equal(np.asarray(a.PortableValues, np.int64), oct_quantize(nrm, normal_bits))
        elif a.AttributeType == 3:
            mn, rng, q = source_quantization(uv, uv_bits)
            assert a.QuantizationBits == uv_bits and np.array_equal(np.asarray(a.MinValues, np.float32), mn) and np.float32(a.Range) == rng
            assert np.array_equal(np.asarray(a.PortableValues, np.int64), q)
        else:
            g = np.asarray(gen, np.uint8).reshape(len(pos), -1)
            assert a.NumComponents == g.shape[1]
            assert np.array_equal(np.asarray(a.Values).reshape(g.shape).astype(np.int64), g.astype(np.int64))
