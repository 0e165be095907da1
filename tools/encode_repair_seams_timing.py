"""Encode direction, attributes given per corner over meshes whose topology needs the repair (dsa_encode_seam_repair_batch,
corner_repair = 1): N bench-size seamed meshes given as one row per point (GRID 128 x 256, `stripes` UV charts, unwelded into one
shuffled row per point), encoded in one process, after a warm-up of every leg, in alternating passes of
  (a) dsa_encode_points_batch on the meshes as they are: clean, one pass (the capability before this call, and its ceiling),
  (b) dsa_encode_seam_repair_batch (topology 1, weld_points 1, corner_repair 1) on the same meshes with 50 injected defects each
      (doubled faces, fins, flips, slivers with a repeated index, pinches): every mesh is refused by the strict pass, welded again
      and coded on the repaired table with its UV seams.
Prints meshes/s per pass, the spread of (a) against itself, (b) against (a), and whether a sample of (b)'s streams equals the CPU
coder's with repair_topology = 2.  Before the device is touched a child process runs leg (b) once with DSA_ENC_TIMING=1 and the
share of its chunks' wall time spent in the repair stage (the repair kernels, the face scan and the id compaction, from_repaired on
the host) is read off the library's stage clocks.
usage: python tools/encode_repair_seams_timing.py [meshes [rounds]]"""
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
    repair_ms = sum(float(x) for x in re.findall(r" topology repair\s+([0-9.]+) ms", measured))
    weld_ms = sum(float(x) for x in re.findall(r" weld\s+([0-9.]+) ms", measured))
    chunk_ms = sum(float(x) for x in re.findall(r"chunk \d+ \(\d+ meshes\) returned after\s+([0-9.]+) ms", measured))
    call = re.search(r"leg \(b\) call ([0-9.]+) ms", r.stdout)
    if r.returncode != 0 or not call or chunk_ms == 0:
        print("stage clocks: the child run failed\n" + r.stdout[-2000:] + r.stderr[-2000:], flush=True)
    else:
        print("stage clocks of leg (b), one call of %.1f ms: repair stage %.1f ms, weld stage %.1f ms of %.1f ms summed over the chunks of both passes: %.1f %% and %.1f %%"
              % (float(call.group(1)), repair_ms, weld_ms, chunk_ms, 100.0 * repair_ms / chunk_ms, 100.0 * weld_ms / chunk_ms), flush=True)

import defects  # noqa: E402
import encodecall  # noqa: E402
import draco_sharp_amd as dsa  # noqa: E402
import draco_sharp_amd.synth as synth  # noqa: E402
import irregular  # noqa: E402
import seamdefects as sd  # noqa: E402
import weldcases  # noqa: E402
from draco_sharp_amd import native  # noqa: E402

ctx = dsa.Context(0)
L = native.lib()
clean, broken = [], []
for i in range(16):
    m = synth.make_mesh(synth.GRID, 128, 256, 1000 + i)
    pos, faces, nrm, nid, uv, uid = irregular.with_seams(*m, None, "stripes", seed=i)
    p, f, nr, u = weldcases.unweld(pos, faces, nrm, nid, uv, uid, np.random.default_rng(i))
    clean.append(dsa.MeshData(p, f, nr, u))
    s = sd.Seamed("bench-%d" % i, pos, np.asarray(faces, np.uint32).reshape(-1, 3), nrm, None if nid is None else np.asarray(nid, np.uint32).reshape(-1, 3),
                  uv, None if uid is None else np.asarray(uid, np.uint32).reshape(-1, 3))
    rng = np.random.default_rng(500 + i)
    for kind in ("double", "fin", "flip", "degenerate", "pinch"):      # 50 in all
        s = sd.inject(s, kind, 10, rng)
    p, f, nr, u = weldcases.unweld(s.pos, s.faces, s.nrm, s.nid, s.uv, s.uid, np.random.default_rng(i))
    broken.append(dsa.MeshData(p, f, nr, u))
print("per mesh: %d points, %d faces clean; %d points, %d faces with 50 defects" % (len(clean[0].positions), len(clean[0].faces), len(broken[0].positions), len(broken[0].faces)), flush=True)


def inputs(meshes):
    return encodecall.arrays([meshes[i % 16] for i in range(n)])[0]


cfg = dsa.Config(repair_topology=True, repair_seams=True, weld_points=True)
so = native.EncodeSeamRepairOptions()
L.dsa_encode_default_seam_repair_options(C.byref(so))
so.grid.repair = cfg._native_repair()
so.grid.weld_points = 1
so.corner_repair = 1


def points_call(h, arr, opt):
    return L.dsa_encode_points_batch(ctx._h, n, arr, C.byref(opt), C.byref(h))


def seams_call(h, arr, opt):
    return L.dsa_encode_seam_repair_batch(ctx._h, n, arr, None, C.byref(opt), C.byref(h))


LEGS = [("(a) dsa_encode_points_batch, clean", points_call, dsa.Config(weld_points=True)._native_repair(), inputs(clean)),
        ("(b) dsa_encode_seam_repair_batch, 50 defects", seams_call, so, inputs(broken))]


def run(entry, opt, arr, sample=()):
    h = C.c_void_p()
    t0 = time.perf_counter()
    st = entry(h, arr, opt)
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


sample = tuple(range(min(n, 2)))
for k, (name, entry, opt, arr) in enumerate(LEGS):      # warm-up; the byte check of a sample of leg (b)'s streams
    dt, failed, out = run(entry, opt, arr, sample)
    print("%-48s warm-up %8.1f ms; meshes refused: %d" % (name + ":", dt * 1e3, failed), flush=True)
    if k == 1:
        want = {i: synth.encode_mesh_points(broken[i].positions, broken[i].faces, broken[i].normals, broken[i].texcoords, opt=synth.options(repair_topology=2)) for i in sample}
        print("sampled streams of (b) equal the CPU coder's (repair_topology = 2): %s (%d bytes for mesh 0)" % (out == want, len(out.get(0, b""))), flush=True)
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
        print("round %d  %-48s %8.1f ms %8.0f meshes/s" % (r, name + ":", dt * 1e3, n / dt), flush=True)
base = rates[LEGS[0][0]]
print("%d meshes; spread of (a) against itself: %.1f %% (min %.0f, max %.0f meshes/s)" %
      (n, 100.0 * (max(base) - min(base)) / statistics.median(base), min(base), max(base)), flush=True)
for name, _, _, _ in LEGS:
    v = rates[name]
    print("%-48s median %8.0f meshes/s  (min %.0f, max %.0f)  %.3f of (a)" % (name + ":", statistics.median(v), min(v), max(v), statistics.median(v) / statistics.median(base)), flush=True)
