"""Encode direction, sequential streams beside Edgebreaker: N bench meshes (GRID 128 x 256, positions + normals + texture
coordinates) from host arrays to .drc bytes, in one process, a warm-up call per mode, then the modes alternating for a number of
timed repetitions:
    edgebreaker   dsa_encode_batch, the defaults: the yardstick of the same build on the same box
    seq-raw       dsa_encode_sequential_batch, raw indices
    seq-comp      dsa_encode_sequential_batch, compressed indices
    cloud         dsa_encode_sequential_batch, the same vertices as point clouds
Prints meshes/s per mode (median, and the spread of the repetitions) and the bytes per stream.
usage: python tools/encode_sequential_timing.py [--meshes 4096] [--reps 5] [--only MODE] [--once]
--only / --once: one mode, one warm batch after the warm-up (what a kernel trace is taken of)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import draco_sharp_amd as dsa                                       # noqa: E402
import draco_sharp_amd.synth as synth                               # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--meshes", type=int, default=4096)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only", default=None)
ap.add_argument("--once", action="store_true")
args = ap.parse_args()

ctx = dsa.Context(0)
enc = dsa.DracoEncoder(ctx)
base = [synth.make_mesh(synth.GRID, 128, 256, 1000 + i) for i in range(16)]
meshes = [dsa.MeshData(base[i % 16][0], base[i % 16][3], base[i % 16][1], base[i % 16][2]) for i in range(args.meshes)]
clouds = [dsa.PointCloudData(m.positions, m.normals, m.texcoords) for m in meshes[:16]]
clouds = [clouds[i % 16] for i in range(args.meshes)]
MODES = {
    "edgebreaker": (meshes, dsa.Config()),
    "seq-raw": (meshes, dsa.Config(encoding_method=0)),
    "seq-comp": (meshes, dsa.Config(encoding_method=0, compress_connectivity=True)),
    "cloud": (clouds, dsa.Config(encoding_method=0)),
}
if args.only:
    MODES = {args.only: MODES[args.only]}
sizes, times = {}, {k: [] for k in MODES}
for name, (items, cfg) in MODES.items():                            # warm-up: lanes, staging buffers, device memory
    out = enc.EncodeBatch(items, cfg)
    sizes[name] = out.sizes[0]
    out.close()
for rep in range(1 if args.once else max(5, args.reps)):
    for name, (items, cfg) in MODES.items():
        t0 = time.perf_counter()
        out = enc.EncodeBatch(items, cfg)
        times[name].append(time.perf_counter() - t0)
        out.close()
m0 = meshes[0]
checks = {
    "edgebreaker": lambda: synth.encode_mesh(m0.positions, m0.faces, m0.normals, m0.texcoords),
    "seq-raw": lambda: synth.encode_sequential(m0.positions, m0.faces, m0.normals, m0.texcoords),
    "seq-comp": lambda: synth.encode_sequential(m0.positions, m0.faces, m0.normals, m0.texcoords, compressed=True),
    "cloud": lambda: synth.encode_point_cloud_attributes(m0.positions, m0.normals, m0.texcoords),
}
for name, (items, cfg) in MODES.items():
    rates = sorted(args.meshes / t for t in times[name])
    same = enc.EncodeBatch(items[:1], cfg)[0] == checks[name]()
    print("%-12s %6d meshes: median %7.0f meshes/s (min %7.0f, max %7.0f over %d repetitions), %8d bytes per stream, equals the CPU coder's: %s"
          % (name, args.meshes, statistics.median(rates), rates[0], rates[-1], len(rates), sizes[name], same), flush=True)
ctx.close()
