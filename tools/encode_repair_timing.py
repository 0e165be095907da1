"""Encode direction, meshes that are not clean (dsa_encode_repair_batch): N bench meshes (GRID 128 x 256, positions + normals + UVs)
encoded in one process, after a warm-up batch of every leg, in alternating passes of
  (a) dsa_encode_level_batch,
  (b) dsa_encode_repair_batch with topology = 1 on the same clean meshes,
  (c) the same batch with one mesh in 16 carrying 1 - 8 defects (a face twice, a fin, a face turned over, a degenerate face, an
      isolated vertex, two vertices pinched into one).
Prints meshes/s per pass, the spread of (a) against itself, (b) and (c) against (a), and whether sampled repaired streams equal the
CPU coder's.  Before the device is touched a child process runs leg (c) once with DSA_ENC_TIMING=1 and the share of its chunks'
wall time spent in the repair stage is read off the library's stage clocks.
usage: python tools/encode_repair_timing.py [meshes [rounds]]"""
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
n = int(args[0]) if len(args) > 0 else 4096
rounds = int(args[1]) if len(args) > 1 else 3
stages_only = "--stages" in sys.argv

if not stages_only:
    # the stage clocks are read once per process, so they get a process of their own -- started before this one opens the device
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(n), "1", "--stages"], env=dict(os.environ, DSA_ENC_TIMING="1"),
                       capture_output=True, text=True)
    measured = r.stderr.split("== measured call ==")[-1]
    repair_ms = sum(float(x) for x in re.findall(r"topology repair\s+([0-9.]+) ms", measured))
    chunk_ms = sum(float(x) for x in re.findall(r"chunk \d+ \(\d+ meshes\) returned after\s+([0-9.]+) ms", measured))
    call = re.search(r"leg \(c\) call ([0-9.]+) ms", r.stdout)
    if r.returncode != 0 or not call or chunk_ms == 0:
        print("stage clocks: the child run failed\n" + r.stdout[-2000:] + r.stderr[-2000:], flush=True)
    else:
        print("stage clocks of leg (c), one call of %.1f ms: repair stage %.1f ms of %.1f ms summed over the chunks of both passes: %.1f %%"
              % (float(call.group(1)), repair_ms, chunk_ms, 100.0 * repair_ms / chunk_ms), flush=True)

import defects  # noqa: E402
import encodecall  # noqa: E402
import draco_sharp_amd as dsa  # noqa: E402
import draco_sharp_amd.synth as synth  # noqa: E402
from draco_sharp_amd import native  # noqa: E402

ctx = dsa.Context(0)
L = native.lib()
plain = [synth.make_mesh(synth.GRID, 128, 256, 1000 + i) for i in range(16)]
clean = [dsa.MeshData(plain[i % 16][0], plain[i % 16][3], plain[i % 16][1], plain[i % 16][2]) for i in range(n)]
rng = np.random.default_rng(4)
damaged, which = list(clean), []
for i in range(5, n, 16):
    pos, nrm, uv, faces = plain[i % 16]
    nv, f = defects.inject(len(pos), faces, defects.KINDS[(i // 16) % len(defects.KINDS)], 1 + (i // 16) % 8, rng)
    pad = nv - len(pos)                          # rows for vertices the injection added
    damaged[i] = dsa.MeshData(np.concatenate([pos, pos[:pad]]), f, np.concatenate([nrm, nrm[:pad]]), np.concatenate([uv, uv[:pad]]))
    which.append(i)


def inputs(meshes):
    return encodecall.arrays(meshes)[0]


cfg = dsa.Config()
level_opt, repair_opt = cfg._native_level(), dsa.Config(repair_topology=True)._native_repair()
in_clean, in_damaged = inputs(clean), inputs(damaged)
LEGS = [("(a) dsa_encode_level_batch", L.dsa_encode_level_batch, level_opt, in_clean),
        ("(b) dsa_encode_repair_batch, clean", L.dsa_encode_repair_batch, repair_opt, in_clean),
        ("(c) dsa_encode_repair_batch, 1 in 16 damaged", L.dsa_encode_repair_batch, repair_opt, in_damaged)]


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


for name, entry, opt, arr in LEGS:              # warm-up; the byte check of a sample of the repaired streams
    sample = which[:2] if arr is in_damaged else ()
    dt, failed, out = run(entry, opt, arr, sample)
    same = all(out[i] == synth.encode_mesh(damaged[i].positions, damaged[i].faces, damaged[i].normals, damaged[i].texcoords, opt=synth.options(repair_topology=1)) for i in sample)
    print("%-46s warm-up %8.1f ms; meshes refused: %d%s" % (name + ":", dt * 1e3, failed, "; sampled repaired streams equal the CPU coder's: %s" % same if sample else ""), flush=True)
if stages_only:
    print("== measured call ==", file=sys.stderr, flush=True)
    dt, _, _ = run(*LEGS[2][1:])
    print("leg (c) call %.1f ms" % (dt * 1e3), flush=True)
    sys.exit(0)
rates = {leg[0]: [] for leg in LEGS}
for r in range(rounds):
    for name, entry, opt, arr in LEGS:
        dt, _, _ = run(entry, opt, arr)
        rates[name].append(n / dt)
        print("round %d  %-46s %8.1f ms %8.0f meshes/s" % (r, name + ":", dt * 1e3, n / dt), flush=True)
base = rates[LEGS[0][0]]
print("%d meshes, %d of them damaged in (c); spread of (a) against itself: %.1f %% (min %.0f, max %.0f meshes/s)" %
      (n, len(which), 100.0 * (max(base) - min(base)) / statistics.median(base), min(base), max(base)), flush=True)
for name, _, _, _ in LEGS:
    v = rates[name]
    print("%-46s median %8.0f meshes/s  (min %.0f, max %.0f)  %.3f of (a)" % (name + ":", statistics.median(v), min(v), max(v), statistics.median(v) / statistics.median(base)), flush=True)
