"""What keeping the rows costs (dsa_encode_rows_batch with track_rows, dsa_batch_source_rows): the encode batch of bench.py -- N (default 1024)
64k-triangle grids cycling through 32 distinct meshes, positions + normals + UVs per vertex -- encoded in one process, after a
warm-up of both legs, in alternating passes of
    (a) Config()                  dsa_encode_seam_repair_batch, what the bench leg calls,
    (b) Config(track_rows=True)   dsa_encode_rows_batch with track_rows = 1,
meshes/s per pass, the spread of (a) against itself and (b) against (a); whether the streams of (b) are those of (a) and a sample of
its entry rows the host coder's; then the streams decoded and `rounds` calls of Batch.source_rows on the decoded batch, wall time
per call (queued behind a finished decode: the upload of the entry rows, k_source_rows, the transfer of the arrays, the wait) and
with device_only (no transfer down), and the bytes that move.
usage: python tools/source_rows_timing.py [meshes [rounds]]"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import draco_sharp_amd as dsa  # noqa: E402
import draco_sharp_amd.synth as synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 1024      # (the rows of 4096 bench meshes are 1.6 GB in the handle, and as much again in each block of source_rows)
rounds = int(args[1]) if len(args) > 1 else 3

distinct = [synth.make_mesh(synth.GRID, 128, 256, 1000 + i) for i in range(min(32, n))]
meshes = [dsa.MeshData(pos, faces, nrm, uv) for pos, nrm, uv, faces in (distinct[i % len(distinct)] for i in range(n))]
ctx = dsa.Context(0)
enc = dsa.DracoEncoder(ctx)
legs = {"a": dsa.Config(), "b": dsa.Config(track_rows=True)}
for cfg in legs.values():                                     # untimed: the lanes pin their staging and size their device memory once
    enc.EncodeBatch(meshes, cfg).close()
rates = {"a": [], "b": []}
kept = None
for r in range(rounds):
    for leg in ("a", "b", "a") if r == 0 else ("b", "a"):
        t0 = time.perf_counter()
        out = enc.EncodeBatch(meshes, legs[leg])
        dt = time.perf_counter() - t0
        rates[leg].append(n / dt)
        print("pass %d leg (%s): %8.1f ms, %8.1f meshes/s" % (r, leg, dt * 1e3, n / dt), flush=True)
        if leg == "b" and kept is None:
            kept = out
        else:
            if leg == "a" and r == 0 and kept is not None:
                print("streams of (b) equal those of (a): %s" % (kept == out), flush=True)
            out.close()
ma, mb = statistics.median(rates["a"]), statistics.median(rates["b"])
print("(a) median %.1f meshes/s (min %.1f, max %.1f); (b) median %.1f meshes/s (min %.1f, max %.1f): (b) / (a) = %.3f"
      % (ma, min(rates["a"]), max(rates["a"]), mb, min(rates["b"]), max(rates["b"]), mb / ma), flush=True)
same = True
for k in range(min(4, len(distinct))):
    pos, nrm, uv, faces = distinct[k]
    want = synth.entry_rows(pos, faces, nrm, uv)
    got = kept.entry_rows(k)
    same = same and len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
entries = sum(len(r) for r in kept.entry_rows(0))
print("entry rows of %d sample meshes equal the host coder's: %s; %d entries per mesh in 3 attributes: %.1f KB per mesh, %.1f MB in the handle"
      % (min(4, len(distinct)), same, entries, 4 * entries / 1e3, 4.0 * entries * n / 1e6), flush=True)

batch = dsa.Batch(ctx, kept)
batch.decode()
for device_only in (False, True):
    batch.source_rows(kept, device_only=device_only)          # untimed: the block and the mirror are made once
    ms = []
    for r in range(max(rounds, 3)):
        t0 = time.perf_counter()
        batch.source_rows(kept, wait=False, device_only=device_only)
        batch.wait()
        ms.append((time.perf_counter() - t0) * 1e3)
    if not device_only:
        per_mesh = sum(4 * len(a) for a in batch.source_row_views(0))
    print("Batch.source_rows%s: median %.2f ms per batch of %d meshes (min %.2f, max %.2f); %.1f MB of arrays, %.1f MB of entry rows up"
          % (" (device_only)" if device_only else "", statistics.median(ms), n, min(ms), max(ms), per_mesh * n / 1e6, 4.0 * entries * n / 1e6), flush=True)
rows = batch.source_rows(kept)
r0 = dsa.Batch.result(batch, 0).ConnectedData
pos = distinct[0][0]
a = r0.Attributes[0]
back = a.Values[a.PointMap]
err = float(np.abs(back - pos[rows[0][0]]).max())
print("positions decoded at the points against the input rows the source rows name: max |difference| %.3g (quantisation step %.3g)"
      % (err, float(a.Range) / ((1 << a.QuantizationBits) - 1)), flush=True)
batch.close()
kept.close()
ctx.close()
