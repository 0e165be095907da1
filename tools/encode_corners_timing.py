"""Encode direction, attributes given per corner: N bench-size seamed meshes (GRID 128 x 256; UV charts 'stripes', then UV +
normal charts 'checker') through dsa_encode_batch_corners with the connectivity on the device and on the host cores
(DSA_ENC_HOST_CONN, read per call), and the per-vertex batch of the same meshes through dsa_encode_batch in the same process.
Prints meshes/s and whether the first streams equal the CPU coder's.  usage: python tools/encode_corners_timing.py [meshes ...]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import draco_sharp_amd as dsa  # noqa: E402
import draco_sharp_amd.synth as synth  # noqa: E402
from meshutil import seamed_mesh  # noqa: E402

counts = [int(x) for x in sys.argv[1:]] or [512]
ctx = dsa.Context(0)
enc = dsa.DracoEncoder(ctx)
uv_only = [seamed_mesh(synth, synth.GRID, 128, 256, 1000 + i, normal_charts=None, uv_charts="stripes") for i in range(16)]
both = [seamed_mesh(synth, synth.GRID, 128, 256, 1000 + i, normal_charts="checker", uv_charts="stripes") for i in range(16)]
plain = [synth.make_mesh(synth.GRID, 128, 256, 1000 + i) for i in range(16)]


def timed(meshes, cpu, host_conn=None):
    if host_conn is None:
        os.environ.pop("DSA_ENC_HOST_CONN", None)
    else:
        os.environ["DSA_ENC_HOST_CONN"] = host_conn
    enc.EncodeBatch(meshes[:2])
    t0 = time.perf_counter()
    out = enc.EncodeBatch(meshes)
    dt = time.perf_counter() - t0
    os.environ.pop("DSA_ENC_HOST_CONN", None)
    return dt, all(out[i] == cpu(i) for i in range(2))


for n in counts:
    rows = []
    pv = [dsa.MeshData(plain[i % 16][0], plain[i % 16][3], plain[i % 16][1], plain[i % 16][2]) for i in range(n)]
    rows.append(("per vertex, device connectivity", timed(pv, lambda i: synth.encode_mesh(pv[i].positions, pv[i].faces, pv[i].normals, pv[i].texcoords))))
    for name, base in (("UV per corner", uv_only), ("UV + normals per corner", both)):
        ms = [base[i % 16] for i in range(n)]
        md = [dsa.MeshData(p, f, nr, u, normal_corners=ni, texcoord_corners=ui) for p, f, nr, ni, u, ui in ms]
        cpu = lambda i, ms=ms: synth.encode_mesh_corners(*ms[i])  # noqa: E731
        rows.append((name + ", device connectivity", timed(md, cpu)))
        rows.append((name + ", host connectivity", timed(md, cpu, "1")))
    for name, (dt, same) in rows:
        print("%d meshes, %-42s %8.1f ms %8.0f meshes/s  first streams equal the CPU coder's: %s" % (n, name + ":", dt * 1e3, n / dt, same), flush=True)
