"""Encode direction, per-point meshes whose attribute list holds a lightmap-style TEXCOORD_1 with a chart layout of its own
(dsa_encode_corner_attributes_batch, weld_attributes): what welding the listed attributes alone costs and saves.

  --sizes   (no device) the CPU coder on the bench grid (GRID 128 x 256, `stripes` UV0 charts, `checker` TEXCOORD_1 charts, unwelded
            into one shuffled row per point): bytes per mesh and vertices in the stream with the attribute in the vertex key
            (weld_attributes 0: its seams cut the positions) against welded alone (weld_attributes 1).
  default   N such meshes encoded in one process, after a warm-up of every leg, in alternating passes of
              (a) dsa_encode_points_batch -- the attribute in the vertex key, what the library did before the option existed,
              (b) dsa_encode_corner_attributes_batch with weld_attributes = 1,
            meshes/s per pass, the spread of (a) against itself, (b) against (a), whether a sample of (b) equals the CPU coder.
            Before the device is touched a child process runs leg (b) once with DSA_ENC_TIMING=1 and the share of its chunks' wall
            time spent in the weld stage is read off the library's stage clocks.
The TEXCOORD_1 charts are `island` (one closed seam loop: with the attribute in the key the cut positions are still a table the
strict coder takes, so both legs code every mesh) or, with --checker, `checker` (seams that cross: in the key they leave vertices
the strict coder refuses, and the size of leg (a) is that of the repaired table).
At 4096 meshes the library's default chunks (1024 meshes on each of four lanes) do not fit the device's memory in leg (b): the
stream then has two attributes with ids (UV0 and TEXCOORD_1), each sized for 3 F entries and its seam tables, about 45 MB per mesh
in all; the call fails as a whole with DSA_ERR_OUT_OF_MEMORY.  Run both legs with DSA_ENC_CHUNK=512 in the environment.
usage: [DSA_ENC_CHUNK=512] python tools/encode_corner_attributes_timing.py [--sizes] [--checker] [meshes [rounds]]"""
import ctypes as C
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cornerattrcases as K  # noqa: E402
import draco_sharp_amd.synth as synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 4096
rounds = int(args[1]) if len(args) > 1 else 3
stages_only = "--stages" in sys.argv
DISTINCT = 16
CHARTS = "checker" if "--checker" in sys.argv else "island"


def bench_points(i):
    """(pos, faces, normals, uvs, [TEXCOORD_1]) of bench mesh i, one shuffled row per point"""
    case = K.Case("bench-%s-%d" % (CHARTS, i), lambda: synth.make_mesh(synth.GRID, 128, 256, 1000 + i), (None, "stripes"), [("uv1", CHARTS)])
    return K.unweld(K.build(case), np.random.default_rng(i))


if "--sizes" in sys.argv:
    pos, faces, nrm, uv, arrays = bench_points(0)
    extra = [synth.Extra(arrays[0], attribute_type=3)]
    rows = []
    for weld_attributes in (False, True):
        opt = synth.options()
        try:
            s = synth.encode_mesh_points(pos, faces, nrm, uv, extra=extra, opt=opt, weld_attributes=weld_attributes)
            how = "strict"
        except RuntimeError as e:                             # (the cut positions are a table the strict coder refuses)
            s = synth.encode_mesh_points(pos, faces, nrm, uv, extra=extra, opt=synth.options(repair_topology=2), weld_attributes=weld_attributes)
            how = "repair_topology 2 (strict: %s)" % e
        w = synth.weld_points(pos, faces, nrm, uv, extra=extra, weld_attributes=weld_attributes)
        rows.append((len(s), w.num_vertices))
        print("TEXCOORD_1 charts %s, weld_attributes %d: %7d bytes, %6d vertices in the stream (%d points, %d faces; %s)" % (CHARTS, weld_attributes, len(s), w.num_vertices, len(pos), len(faces), how), flush=True)
    print("welded alone: %.1f %% of the bytes, %.1f %% of the vertices" % (100.0 * rows[1][0] / rows[0][0], 100.0 * rows[1][1] / rows[0][1]), flush=True)
    sys.exit(0)

if not stages_only:
    # the stage clocks are read once per process, so they get a process of their own -- started before this one opens the device
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(n), "1", "--stages"] + (["--checker"] if CHARTS == "checker" else []), env=dict(os.environ, DSA_ENC_TIMING="1"),
                       capture_output=True, text=True)
    measured = r.stderr.split("== measured call ==")[-1]
    weld_ms = sum(float(x) for x in re.findall(r" weld\s+([0-9.]+) ms", measured))
    chunk_ms = sum(float(x) for x in re.findall(r"chunk \d+ \(\d+ meshes\) returned after\s+([0-9.]+) ms", measured))
    call = re.search(r"leg \(b\) call ([0-9.]+) ms", r.stdout)
    if r.returncode != 0 or not call or chunk_ms == 0:
        print("stage clocks: the child run failed\n" + r.stdout[-2000:] + r.stderr[-2000:], flush=True)
    else:
        print("stage clocks of leg (b), one call of %.1f ms: weld stage %.1f ms of %.1f ms summed over the chunks: %.1f %%"
              % (float(call.group(1)), weld_ms, chunk_ms, 100.0 * weld_ms / chunk_ms), flush=True)

import draco_sharp_amd as dsa  # noqa: E402
import encodecall  # noqa: E402
from draco_sharp_amd import native  # noqa: E402

ctx = dsa.Context(0)
L = native.lib()
points = []
for i in range(DISTINCT):
    pos, faces, nrm, uv, arrays = bench_points(i)
    points.append(dsa.MeshData(pos, faces, nrm, uv, attributes=[dsa.Attribute(arrays[0], attribute_type=3)]))
arr, _, keep = encodecall.arrays([points[i % DISTINCT] for i in range(n)])
cfg = dsa.Config()
points_opt = cfg._native_repair()
wide = native.EncodeCornerAttributesOptions()
L.dsa_encode_default_corner_attributes_options(C.byref(wide))
wide.seam_repair.grid.repair = cfg._native_repair()
wide.seam_repair.grid.weld_points = 1
wide.weld_attributes = 1


def leg_a(h):
    return L.dsa_encode_points_batch(ctx._h, n, arr, C.byref(points_opt), C.byref(h))


def leg_b(h):
    return L.dsa_encode_corner_attributes_batch(ctx._h, n, arr, None, None, C.byref(wide), C.byref(h))


LEGS = [("(a) dsa_encode_points_batch, attribute in the key", leg_a), ("(b) weld_attributes = 1", leg_b)]


def run(leg, sample=()):
    h = C.c_void_p()
    t0 = time.perf_counter()
    st = leg(h)
    dt = time.perf_counter() - t0
    if st != 0:
        raise RuntimeError(ctx.error())
    out, failed, total = {}, 0, 0
    p, ln = C.c_void_p(), C.c_size_t()
    for i in range(n):
        if L.dsa_encoded_stream(h, i, C.byref(p), C.byref(ln)) != 0:
            failed += 1
            if failed == 1:
                print("    mesh %d refused: %s" % (i, ctx.error()), flush=True)
        else:
            total += ln.value
            if i in sample:
                out[i] = C.string_at(p, ln.value)
    L.dsa_encoded_free(h)
    return dt, failed, out, total


sample = (0, 1)
for name, leg in LEGS:                          # warm-up; the sizes, and for (b) the byte check of a sample of the streams
    dt, failed, out, total = run(leg, sample)
    print("%-52s warm-up %8.1f ms; meshes refused: %d; %.0f bytes per coded mesh" % (name + ":", dt * 1e3, failed, total / max(1, n - failed)), flush=True)
    if leg is leg_b:
        m = points[0]
        want = synth.encode_mesh_points(m.positions, m.faces, m.normals, m.texcoords, extra=[synth.Extra(m.attributes[0].values, attribute_type=3)], weld_attributes=True)
        print("stream 0 of (b) equals the CPU coder's: %s" % (out.get(0) == want), flush=True)
if stages_only:
    print("== measured call ==", file=sys.stderr, flush=True)
    dt, _, _, _ = run(leg_b)
    print("leg (b) call %.1f ms" % (dt * 1e3), flush=True)
    sys.exit(0)
rates = {name: [] for name, _ in LEGS}
for r in range(rounds):
    for name, leg in LEGS:
        dt, _, _, _ = run(leg)
        rates[name].append(n / dt)
        print("round %d  %-52s %8.1f ms %8.0f meshes/s" % (r, name + ":", dt * 1e3, n / dt), flush=True)
base = rates[LEGS[0][0]]
print("%d meshes; spread of (a) against itself: %.1f %% (min %.0f, max %.0f meshes/s)" %
      (n, 100.0 * (max(base) - min(base)) / statistics.median(base), min(base), max(base)), flush=True)
for name, _ in LEGS:
    v = rates[name]
    print("%-52s median %8.0f meshes/s (%.3f x (a))" % (name + ":", statistics.median(v), statistics.median(v) / statistics.median(base)), flush=True)
ctx.close()
