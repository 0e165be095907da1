"""Parity + time on awkward topologies (thousands of components, one huge vertex fan, long thin strip; the meshes of
tests/irregular.py, which tests/test_gpu_irregular.py decodes as well).  usage: python tools/odd_mesh_check.py"""
import sys; sys.path.insert(0,'.'); sys.path.insert(0,'tests')
import numpy as np, time, oracle, draco_sharp_amd as dsa, draco_sharp_amd.synth as synth
import test_gpu_parity as T
import irregular
# 20000 disjoint quads; a centre vertex with 60000 triangles around it (closed disc); a strip of 2 x 100000 vertices
meshes = {"components": irregular.components(20000), "fan": irregular.fan(60000, closed=True), "strip": irregular.strip(100000)}
meshes = {name: (m[0], m[3]) for name, m in meshes.items()}
ctx = dsa.Context(0); ctx.set_profiling(True)
for name, (pos, faces) in meshes.items():
    s = synth.encode_mesh(pos, faces)
    b = dsa.Batch(ctx, [s]); b.decode(); t0 = time.time(); b.decode(); dt = time.time() - t0
    assert b.status(0) == 0, (name, b.status(0), b.mesh_info(0).detail)
    T.assert_same(b.result(0), oracle.decode(s), b, 0)
    print(name, len(faces), "faces,", len(s), "bytes: decode %.3f s" % dt, {k: round(v, 1) for k, v in b.stage_times().items()})
    b.close()
