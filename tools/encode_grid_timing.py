"""Encode direction, quantisation grids (dsa_encode_grid_batch): N bench meshes (GRID 128 x 256, positions + normals + UVs) encoded
in one process, after a warm-up batch of every leg, in alternating passes of
  (a) dsa_encode_level_batch,
  (b) dsa_encode_grid_batch with every grid at mode 0 (it must be the call of (a): nothing of the grids is touched),
  (c) dsa_encode_grid_batch with explicit grids (mode 1) for positions and texture coordinates,
  (d) dsa_encode_grid_batch with shared grids (mode 2) in groups of 16: the pre-pass in front of the chunks, which uploads the
      positions and texture coordinates once more, reduces them and folds the groups.
Prints meshes/s per pass, the spread of every leg, (b), (c) and (d) against (a), and whether sampled streams of (c) and (d) equal
the CPU coder's.  DSA_ENC_TIMING=1 adds the library's stage clocks.
usage: python tools/encode_grid_timing.py [meshes [rounds]]"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 4096
rounds = int(args[1]) if len(args) > 1 else 3

import draco_sharp_amd as dsa  # noqa: E402
import draco_sharp_amd.synth as synth  # noqa: E402
import encodecall  # noqa: E402
from draco_sharp_amd import native  # noqa: E402

ctx = dsa.Context(0)
L = native.lib()
plain = [synth.make_mesh(synth.GRID, 128, 256, 1000 + i) for i in range(16)]
meshes = [dsa.MeshData(plain[i % 16][0], plain[i % 16][3], plain[i % 16][1], plain[i % 16][2]) for i in range(n)]
arr = encodecall.arrays(meshes)[0]


def bounds(arrays):
    v = np.concatenate(arrays)
    mn = v.min(axis=0).astype(np.float32)
    return mn, np.float32((v.max(axis=0).astype(np.float32) - mn).max())


pos_grid, uv_grid = bounds([p[0] for p in plain]), bounds([p[2] for p in plain])      # (every group of 16 holds the 16 distinct meshes)
zero, explicit, shared = (native.MeshGrids * n)(), (native.MeshGrids * n)(), (native.MeshGrids * n)()
for i in range(n):
    for g, (origin, rng) in ((explicit[i].position, pos_grid), (explicit[i].texcoord, uv_grid)):
        for c, x in enumerate(origin):
            g.origin[c] = x
        g.range, g.mode = rng, 1
    shared[i].position.mode = shared[i].texcoord.mode = 2
    shared[i].group = i // 16
level_opt = dsa.Config()._native_level()
grid_opt = native.EncodeGridOptions()
L.dsa_encode_default_grid_options(C.byref(grid_opt))
grid_opt.repair.level = level_opt
LEGS = [("(a) dsa_encode_level_batch", None), ("(b) dsa_encode_grid_batch, every mode 0", zero),
        ("(c) dsa_encode_grid_batch, mode 1", explicit), ("(d) dsa_encode_grid_batch, mode 2 in groups of 16", shared)]


def run(grids, sample=()):
    h = C.c_void_p()
    t0 = time.perf_counter()
    if grids is None:
        st = L.dsa_encode_level_batch(ctx._h, n, arr, C.byref(level_opt), C.byref(h))
    else:
        st = L.dsa_encode_grid_batch(ctx._h, n, arr, grids, C.byref(grid_opt), C.byref(h))
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


def cpu(i, gridded):
    m = meshes[i]
    kw = dict(pos_grid=synth.grid(*pos_grid), uv_grid=synth.grid(*uv_grid)) if gridded else {}
    return synth.encode_grid(m.positions, m.faces, m.normals, m.texcoords, **kw)


sample = sorted({0, min(n - 1, 17), n - 1})
first = None
for name, grids in LEGS:                        # warm-up; the byte check of a sample
    dt, failed, out = run(grids, sample)
    if first is None:
        first = out
    same = all(out[i] == cpu(i, grids is explicit or grids is shared) for i in sample) and (grids is not zero or out == first)
    print("%-52s warm-up %8.1f ms; meshes refused: %d; sampled streams equal the CPU coder's: %s" % (name + ":", dt * 1e3, failed, same), flush=True)
rates = {name: [] for name, _ in LEGS}
for r in range(rounds):
    for name, grids in LEGS:
        dt, _, _ = run(grids)
        rates[name].append(n / dt)
        print("round %d  %-52s %8.1f ms %8.0f meshes/s" % (r, name + ":", dt * 1e3, n / dt), flush=True)
base = statistics.median(rates[LEGS[0][0]])
upload = sum(m.positions.nbytes + m.texcoords.nbytes for m in meshes) / sum(m.positions.nbytes + m.texcoords.nbytes + m.normals.nbytes + m.faces.nbytes for m in meshes)
print("%d meshes; the pre-pass of (d) uploads %.1f %% of a call's input bytes once more" % (n, 100.0 * upload), flush=True)
for name, _ in LEGS:
    v = rates[name]
    print("%-52s median %8.0f meshes/s  (min %.0f, max %.0f, spread %.1f %%)  %.3f of (a)" %
          (name + ":", statistics.median(v), min(v), max(v), 100.0 * (max(v) - min(v)) / statistics.median(v), statistics.median(v) / base), flush=True)
