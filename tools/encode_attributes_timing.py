"""Encode direction, the attribute list (dsa_encode_attributes_batch): N bench meshes (GRID 128 x 256, positions + normals + UVs)
encoded three ways, each as one warm call after a call of the same shape:
  (a) through dsa_encode_batch_ex;
  (b) through dsa_encode_attributes_batch with no extras -- the same work as (a): read (b) against (a) of the same run, a gap is
      overhead of the new entry point's plumbing;
  (c) through dsa_encode_attributes_batch with a skinned-vertex set: uint16 x 4 joints, float32 x 4 weights at 8 bits, uint8 x 4
      normalised colour.
The native calls alone are timed (the argument arrays are built before).  Prints meshes/s and checks the first stream of each
against the CPU coder.  usage: python tools/encode_attributes_timing.py [meshes]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import draco_sharp_amd as dsa  # noqa: E402
import draco_sharp_amd.synth as synth  # noqa: E402
from draco_sharp_amd import native  # noqa: E402
from draco_sharp_amd.encoder import _native_meshes  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
ctx = dsa.Context(0)
L = native.lib()
plain = [synth.make_mesh(synth.GRID, 128, 256, 1000 + i) for i in range(16)]


def skinned(i):
    nv = len(plain[i][0])
    rng = np.random.default_rng(i)
    joints = np.sort(rng.integers(0, 64, (nv, 4)), axis=1).astype(np.uint16)
    w = rng.random((nv, 4)).astype(np.float32)
    weights = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    colour = rng.integers(0, 256, (nv, 4)).astype(np.uint8)
    return [dsa.Attribute(joints, attribute_type=4), dsa.Attribute(weights, attribute_type=4, quantization_bits=8),
            dsa.Attribute(colour, attribute_type=2, normalized=True)]


extras = [skinned(i) for i in range(16)]
bare = [dsa.MeshData(p, f, nr, u) for p, nr, u, f in plain]
listed = [dsa.MeshData(p, f, nr, u, attributes=extras[i]) for i, (p, nr, u, f) in enumerate(plain)]
keep = []


def arrays(meshes, with_list):
    arr, _, alive = _native_meshes([meshes[i % 16] for i in range(n)], native.MeshAttrInput if with_list else native.MeshCornerInput)
    keep.append(alive)
    return arr


opt = dsa.Config()._native_ex()
RUNS = [("(a) dsa_encode_batch_ex", L.dsa_encode_batch_ex, arrays(bare, False), bare, []),
        ("(b) dsa_encode_attributes_batch, no extras", L.dsa_encode_attributes_batch, arrays(bare, True), bare, []),
        ("(c) dsa_encode_attributes_batch, joints + weights + colour", L.dsa_encode_attributes_batch, arrays(listed, True), listed, extras)]


def call(entry, arr):
    h = C.c_void_p()
    t0 = time.perf_counter()
    st = entry(ctx._h, n, arr, C.byref(opt), C.byref(h))
    dt = time.perf_counter() - t0
    if st != 0:
        raise RuntimeError(ctx.error())
    p, ln = C.c_void_p(), C.c_size_t()
    if L.dsa_encoded_stream(h, 0, C.byref(p), C.byref(ln)) != 0:
        raise RuntimeError(ctx.error())
    first = C.string_at(p, ln.value)
    L.dsa_encoded_free(h)
    return dt, first


for name, entry, arr, meshes, ex in RUNS:
    call(entry, arr)                                   # a call of the same shape first
    dt, first = call(entry, arr)
    m = meshes[0]
    cpu = synth.encode_mesh(m.positions, m.faces, m.normals, m.texcoords,
                            extra=[synth.Extra(a.values, a.attribute_type, a.normalized, a.unique_id, a.quantization_bits) for a in m.attributes])
    print("%d meshes  %-60s %8.1f ms %8.0f meshes/s   first stream equals the CPU coder's: %s" % (n, name + ":", dt * 1e3, n / dt, first == cpu), flush=True)
