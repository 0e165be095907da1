"""Encode direction, meshes given as one row per point (dsa_encode_points_batch): N bench-size seamed meshes (GRID 128 x 256,
`stripes` UV charts, unwelded into one shuffled row per point) encoded in one process, after a warm-up of every leg, in alternating
passes of
  (a) dsa_encode_batch_ex on the same meshes welded beforehand, outside the clock (what a caller has to do without the call, and
      a lower bound for it),
  (b) dsa_encode_points_batch on the per-point meshes.
Prints meshes/s per pass, the spread of (a) against itself, (b) against (a), whether the streams of both legs are the same bytes,
and the bytes the weld stage moves over the link.  Before the device is touched a child process runs leg (b) once with
DSA_ENC_TIMING=1 and the share of its chunks' wall time spent in the weld stage is read off the library's stage clocks.
usage: python tools/encode_weld_timing.py [meshes [rounds]]"""
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

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 1024
rounds = int(args[1]) if len(args) > 1 else 3
stages_only = "--stages" in sys.argv

if not stages_only:
    # the stage clocks are read once per process, so they get a process of their own -- started before this one opens the device
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(n), "1", "--stages"], env=dict(os.environ, DSA_ENC_TIMING="1"),
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
import draco_sharp_amd.synth as synth  # noqa: E402
import irregular  # noqa: E402
import weldcases  # noqa: E402
from draco_sharp_amd import native  # noqa: E402

ctx = dsa.Context(0)
L = native.lib()
points, welded = [], []
for i in range(16):
    m = synth.make_mesh(synth.GRID, 128, 256, 1000 + i)
    p, f, nr, uv = weldcases.unweld(*irregular.with_seams(*m, None, "stripes", seed=i), np.random.default_rng(i))
    points.append(dsa.MeshData(p, f, nr, uv))
    w = synth.weld_points(p, f, nr, uv)
    welded.append(dsa.MeshData(w.pos, w.faces, w.normals, w.uvs, normal_corners=w.normal_corners, texcoord_corners=w.uv_corners))
up = sum(m.positions.nbytes + m.faces.nbytes + m.normals.nbytes + m.texcoords.nbytes for m in points) / 16.0
down = sum(4 * len(p.positions) * 3 + 4 * (len(w.positions) + len(w.positions) + len(w.texcoords)) + w.faces.nbytes + w.texcoord_corners.nbytes +
           w.positions.nbytes + w.normals.nbytes + w.texcoords.nbytes for p, w in zip(points, welded)) / 16.0
print("per mesh: %d points -> %d vertices, %d uv rows; the weld stage moves %.0f KiB up (point arrays) and %.0f KiB down (maps, faces, ids, welded rows); "
      "the welded rows then go up again with the ordinary uploads" % (len(points[0].positions), len(welded[0].positions), len(welded[0].texcoords), up / 1024, down / 1024), flush=True)


def inputs(meshes, form=None):
    return encodecall.arrays([meshes[i % 16] for i in range(n)], form)[0]


def corner_inputs(meshes):
    return inputs(meshes, native.MeshCornerInput)


cfg = dsa.Config()
LEGS = [("(a) dsa_encode_batch_ex, welded beforehand", L.dsa_encode_batch_ex, cfg._native_ex(), corner_inputs(welded)),
        ("(b) dsa_encode_points_batch, per point", L.dsa_encode_points_batch, cfg._native_repair(), inputs(points))]


def run(entry, opt, arr, sample=()):
    h = C.c_void_p()
    t0 = time.perf_counter()
    st = entry(ctx._h, n, arr, C.byref(opt), C.byref(h))
    dt = time.perf_counter() - t0
    if st != 0:
        raise RuntimeError(ctx.error())
    out, failed = {}, 0
    p, ln = C.c_void_p(), C.c_size_t()
    for i in range(n):
        if L.dsa_encoded_stream(h, i, C.byref(p), C.byref(ln)) != 0:
            failed += 1
        elif i in sample:
            out[i] = C.string_at(p, ln.value)
    L.dsa_encoded_free(h)
    return dt, failed, out


sample = tuple(range(min(n, 16)))
first = {}
for name, entry, opt, arr in LEGS:              # warm-up; the byte check of a sample of the streams
    dt, failed, out = run(entry, opt, arr, sample)
    first[name] = out
    print("%-46s warm-up %8.1f ms; meshes refused: %d" % (name + ":", dt * 1e3, failed), flush=True)
print("sampled streams of (b) equal those of (a): %s (%d bytes for mesh 0)" % (first[LEGS[0][0]] == first[LEGS[1][0]], len(first[LEGS[1][0]].get(0, b""))), flush=True)
if stages_only:
    print("== measured call ==", file=sys.stderr, flush=True)
    dt, _, _ = run(*LEGS[1][1:])
    print("leg (b) call %.1f ms" % (dt * 1e3), flush=True)
    sys.exit(0)
rates = {leg[0]: [] for leg in LEGS}
for r in range(rounds):
    for name, entry, opt, arr in LEGS:
        dt, _, _ = run(entry, opt, arr)
        rates[name].append(n / dt)
        print("round %d  %-46s %8.1f ms %8.0f meshes/s" % (r, name + ":", dt * 1e3, n / dt), flush=True)
base = rates[LEGS[0][0]]
print("%d meshes; spread of (a) against itself: %.1f %% (min %.0f, max %.0f meshes/s)" %
      (n, 100.0 * (max(base) - min(base)) / statistics.median(base), min(base), max(base)), flush=True)
for name, _, _, _ in LEGS:
    v = rates[name]
    print("%-46s median %8.0f meshes/s  (min %.0f, max %.0f)  %.3f of (a)" % (name + ":", statistics.median(v), min(v), max(v), statistics.median(v) / statistics.median(base)), flush=True)
