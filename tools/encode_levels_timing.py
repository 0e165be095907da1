"""Encode direction, the levels above the default (dsa_encode_level_batch): N bench meshes (GRID 128 x 256, positions + normals +
UVs) encoded in one process, after a warm-up batch of every setting, in alternating passes of the default options,
multi_parallelogram=4, traversal_method=1, and both.  Prints meshes/s per pass beside the default-options rate of the same run and
whether sampled streams equal the CPU coder's.  usage: python tools/encode_levels_timing.py [meshes [rounds]]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import draco_sharp_amd as dsa  # noqa: E402
import draco_sharp_amd.synth as synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
ctx = dsa.Context(0)
enc = dsa.DracoEncoder(ctx)
plain = [synth.make_mesh(synth.GRID, 128, 256, 1000 + i) for i in range(16)]
pv = [dsa.MeshData(plain[i % 16][0], plain[i % 16][3], plain[i % 16][1], plain[i % 16][2]) for i in range(n)]
PASSES = [
    ("default options", dsa.Config(), synth.options()),
    ("multi_parallelogram=4", dsa.Config(multi_parallelogram=4), synth.options(pos_prediction=4, uv_prediction=4)),
    ("traversal_method=1", dsa.Config(traversal_method=1), synth.options(traversal_method=1)),
    ("multi_parallelogram=4, traversal_method=1", dsa.Config(multi_parallelogram=4, traversal_method=1), synth.options(pos_prediction=4, uv_prediction=4, traversal_method=1)),
]


def run(cfg):
    t0 = time.perf_counter()
    out = enc.EncodeBatch(pv, cfg)
    return time.perf_counter() - t0, out


for name, cfg, opt in PASSES:           # warm-up, and the byte check of a sample
    _, out = run(cfg)
    same = all(out[i] == synth.encode_mesh(pv[i].positions, pv[i].faces, pv[i].normals, pv[i].texcoords, opt=opt) for i in (0, 1, n - 1))
    print("%-44s warm-up; sampled streams equal the CPU coder's: %s; %d bytes a stream" % (name + ":", same, len(out[0])), flush=True)
    out.close()
rates = {p[0]: [] for p in PASSES}
for r in range(rounds):
    for name, cfg, _ in PASSES:
        dt, out = run(cfg)
        out.close()
        rates[name].append(n / dt)
        print("round %d  %-44s %8.1f ms %8.0f meshes/s" % (r, name + ":", dt * 1e3, n / dt), flush=True)
base = statistics.median(rates[PASSES[0][0]])
for name, _, _ in PASSES:
    v = rates[name]
    print("%d meshes  %-44s median %8.0f meshes/s  (min %.0f, max %.0f)  %.2f of the default options' rate" %
          (n, name + ":", statistics.median(v), min(v), max(v), statistics.median(v) / base), flush=True)
