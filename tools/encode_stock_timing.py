"""Encode direction, the stock default schemes (valence Edgebreaker, TexCoordsPortable, GeometricNormal; dsa_encode_batch_ex):
N bench meshes (GRID 128 x 256, positions + normals + UVs) encoded, after a warm-up, in alternating passes of the speed-5 default,
the stock default per vertex, the stock default with UV seams, and the stock default per vertex on the host connectivity + plan path
(DSA_ENC_HOST_CONN = DSA_ENC_HOST_PLAN = 1, read per call).  Prints meshes/s per pass and whether sampled streams equal the CPU
coder's.  usage: python tools/encode_stock_timing.py [meshes [rounds]]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import draco_sharp_amd as dsa  # noqa: E402
import draco_sharp_amd.synth as synth  # noqa: E402
from meshutil import seamed_mesh  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
ctx = dsa.Context(0)
enc = dsa.DracoEncoder(ctx)
plain = [synth.make_mesh(synth.GRID, 128, 256, 1000 + i) for i in range(16)]
seamed = [seamed_mesh(synth, synth.GRID, 128, 256, 1000 + i, normal_charts=None, uv_charts="stripes") for i in range(16)]
pv = [dsa.MeshData(plain[i % 16][0], plain[i % 16][3], plain[i % 16][1], plain[i % 16][2]) for i in range(n)]
sm = [dsa.MeshData(p, f, nr, u, normal_corners=ni, texcoord_corners=ui) for p, f, nr, ni, u, ui in (seamed[i % 16] for i in range(n))]
speed5 = dsa.Config()
stock = dsa.Config(edgebreaker_method=2, texcoord_prediction=5, normal_prediction=6)
opt_stock = synth.options(predictive_connectivity=2, uv_prediction=5, normal_prediction=6)


def cpu_pv(i, opt=None):
    m = pv[i]
    return synth.encode_mesh(m.positions, m.faces, m.normals, m.texcoords, opt=opt)


def cpu_sm(i):
    return synth.encode_mesh_corners(*seamed[i % 16], opt=opt_stock)


PASSES = [
    ("speed-5 default", pv, speed5, None, lambda i: cpu_pv(i)),
    ("stock default, per vertex", pv, stock, None, lambda i: cpu_pv(i, opt_stock)),
    ("stock default, UV seams", sm, stock, None, cpu_sm),
    ("stock default, per vertex, host path", pv, stock, "1", lambda i: cpu_pv(i, opt_stock)),
]


def run(meshes, cfg, host):
    for k in ("DSA_ENC_HOST_CONN", "DSA_ENC_HOST_PLAN"):
        if host is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = host
    t0 = time.perf_counter()
    out = enc.EncodeBatch(meshes, cfg)
    return time.perf_counter() - t0, out


for name, meshes, cfg, host, cpu in PASSES:           # warm-up, and the byte check of a sample
    _, out = run(meshes, cfg, host)
    same = all(out[i] == cpu(i) for i in (0, 1, n - 1))
    print("%-40s warm-up; sampled streams equal the CPU coder's: %s" % (name + ":", same), flush=True)
    out.close()
rates = {p[0]: [] for p in PASSES}
for r in range(rounds):
    for name, meshes, cfg, host, _ in PASSES:
        dt, out = run(meshes, cfg, host)
        out.close()
        rates[name].append(n / dt)
        print("round %d  %-40s %8.1f ms %8.0f meshes/s" % (r, name + ":", dt * 1e3, n / dt), flush=True)
for name, _, _, _, _ in PASSES:
    v = rates[name]
    print("%d meshes  %-40s median %8.0f meshes/s  (min %.0f, max %.0f)" % (n, name + ":", statistics.median(v), min(v), max(v)), flush=True)
