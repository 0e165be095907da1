"""Encode direction, the Morton point order of sequential streams (dsa_encode_ordered_sequential_batch): point clouds of shuffled
height-field points encoded in one process, after a warm-up batch of every leg, in alternating passes of
  (a) N clouds of 65 536 points, point_order 0        (b) the same, point_order 1
  (c) 16 N clouds of 4 096 points, point_order 0      (d) the same, point_order 1       (the crowded case: many small segments)
Prints clouds/s per pass, the spread of every leg, bytes per stream, (b) against (a) and (d) against (c), and whether a sampled
stream of (b) and (d) equals the CPU coder's.  Then one more pass of (b) and (d) on one lane with the library's stage clocks
(DSA_ENC_TIMING, DSA_ENC_LANES=1, DSA_ENC_HOST_PLAN=0: every kernel of a chunk in one stage), whose laps give the share of a chunk's
device time spent in the order kernels.
usage: python tools/encode_order_timing.py [N [rounds]]"""
import ctypes as C
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 64
rounds = int(args[1]) if len(args) > 1 else 3

import draco_sharp_amd as dsa  # noqa: E402
import draco_sharp_amd.synth as synth  # noqa: E402
import encodecall  # noqa: E402
import ordercases  # noqa: E402
from draco_sharp_amd import native  # noqa: E402

ctx = dsa.Context(0)
L = native.lib()
large = [ordercases.height_field(256, 256, 500 + i) for i in range(min(n, 8))]
small = [ordercases.height_field(64, 64, 600 + i) for i in range(min(16 * n, 32))]
SETS = {"large": [dsa.PointCloudData(large[i % len(large)]) for i in range(n)], "small": [dsa.PointCloudData(small[i % len(small)]) for i in range(16 * n)]}
ARRAYS = {k: encodecall.arrays(v)[0] for k, v in SETS.items()}
LEGS = [("(a) %d clouds of 65 536 points, point_order 0" % n, "large", 0), ("(b) %d clouds of 65 536 points, point_order 1" % n, "large", 1),
        ("(c) %d clouds of 4 096 points, point_order 0" % (16 * n), "small", 0), ("(d) %d clouds of 4 096 points, point_order 1" % (16 * n), "small", 1)]


def run(which, order, sample=()):
    o = native.EncodeOrderOptions()
    L.dsa_encode_default_order_options(C.byref(o))
    o.sequential.geometry, o.point_order = 0, order
    count = len(SETS[which])
    h = C.c_void_p()
    t0 = time.perf_counter()
    st = L.dsa_encode_ordered_sequential_batch(ctx._h, count, ARRAYS[which], None, C.byref(o), C.byref(h))
    dt = time.perf_counter() - t0
    if st != 0:
        raise RuntimeError(ctx.error())
    out, failed, total = {}, 0, 0
    p, ln = C.c_void_p(), C.c_size_t()
    for i in range(count):
        if L.dsa_encoded_stream(h, i, C.byref(p), C.byref(ln)) != 0:
            failed += 1
            continue
        total += ln.value
        if i in sample:
            out[i] = C.string_at(p, ln.value)
    L.dsa_encoded_free(h)
    return dt, failed, out, total / max(1, count - failed)


size = {}
for name, which, order in LEGS:                 # warm-up; the byte check of a sample
    count = len(SETS[which])
    dt, failed, out, size[name] = run(which, order, (count - 1,))
    pos = SETS[which][count - 1].positions
    want = synth.encode_ordered(pos, geometry=0)[0] if order else synth.encode_point_cloud(pos)
    print("%-52s warm-up %8.1f ms; clouds refused: %d; %9.0f bytes per stream; the sampled stream equals the CPU coder's: %s" %
          (name + ":", dt * 1e3, failed, size[name], out[count - 1] == want), flush=True)
rates = {name: [] for name, _, _ in LEGS}
for r in range(rounds):
    for name, which, order in LEGS:
        dt = run(which, order)[0]
        rates[name].append(len(SETS[which]) / dt)
        print("round %d  %-52s %8.1f ms %8.0f clouds/s" % (r, name + ":", dt * 1e3, len(SETS[which]) / dt), flush=True)
for k, (name, _, _) in enumerate(LEGS):
    v, base = rates[name], statistics.median(rates[LEGS[k - k % 2][0]])
    print("%-52s median %8.0f clouds/s  (min %.0f, max %.0f, spread %.1f %%)  %.3f of its order-0 leg; %.3f of its bytes" %
          (name + ":", statistics.median(v), min(v), max(v), 100.0 * (max(v) - min(v)) / statistics.median(v), statistics.median(v) / base,
           size[name] / size[LEGS[k - k % 2][0]]), flush=True)

# the share of the order kernels: one pass of each ordered leg with the stage clocks, the library's stderr into a file
os.environ.update(DSA_ENC_TIMING="1", DSA_ENC_LANES="1", DSA_ENC_HOST_PLAN="0")
for name, which, order in LEGS:
    if not order:
        continue
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            run(which, order)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode(errors="replace")
    laps = {}
    for what, ms in re.findall(r"ms: (.*?)\s+([0-9.]+) ms\n", text):
        laps[what] = laps.get(what, 0.0) + float(ms)
    stage = sum(laps.get(k, 0.0) for k in ("uploads + quantisers", "point order", "gather to entropy coding"))
    print("%-52s uploads + quantisers %.2f ms, point order %.2f ms, gather to entropy coding %.2f ms: the order kernels are %.1f %% of the chunks' device stage" %
          (name + ":", laps.get("uploads + quantisers", 0.0), laps.get("point order", 0.0), laps.get("gather to entropy coding", 0.0),
           100.0 * laps.get("point order", 0.0) / stage if stage else float("nan")), flush=True)
