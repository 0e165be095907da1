"""Encode direction, one point per quantisation cell of Morton-ordered point clouds (dsa_encode_merged_sequential_batch): point
clouds of shuffled height-field points of which a stated share repeat the position of another point, encoded in one process, after
a warm-up batch of every leg, in alternating passes of
  (a) N clouds of 65 536 points, ordered (merge_points 0)        (b) the same, merged (merge_points 1)
  (c) 16 N clouds of 4 096 points, ordered                       (d) the same, merged       (the crowded case: many small segments)
once per share (by default 0.5 and 0: with no duplicates the merge can only cost).  Prints clouds/s per pass, the spread of every
leg, bytes and points per stream, the merged leg against the ordered leg of the same run, and whether a sampled stream of every leg
equals the CPU coder's.  Then one more pass of the merged legs on one lane with the library's stage clocks (DSA_ENC_TIMING,
DSA_ENC_LANES=1, DSA_ENC_HOST_PLAN=0: every kernel of a chunk in one stage), whose laps give the share of a chunk's device time
spent in the merge kernels, beside that of the order kernels.
usage: python tools/encode_merge_timing.py [N [rounds [share ...]]]"""
import ctypes as C
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 64
rounds = int(args[1]) if len(args) > 1 else 3
shares = [float(a) for a in args[2:]] or [0.5, 0.0]

import draco_sharp_amd as dsa  # noqa: E402
import draco_sharp_amd.synth as synth  # noqa: E402
import encodecall  # noqa: E402
import ordercases  # noqa: E402
from draco_sharp_amd import native  # noqa: E402

ctx = dsa.Context(0)
L = native.lib()


def duplicated(pos, share, seed):
    """pos with the last `share` of its rows replaced by copies of earlier rows, shuffled: that share of the points lies in the cell
    of another point, whatever the grid"""
    rng = np.random.default_rng(seed)
    keep = len(pos) - int(round(share * len(pos)))
    out = np.concatenate([pos[:keep], pos[rng.integers(0, keep, len(pos) - keep)]])
    return np.ascontiguousarray(out[rng.permutation(len(out))])


def run(which, merge, sample=()):
    o = native.EncodeMergeOptions()
    L.dsa_encode_default_merge_options(C.byref(o))
    o.order.sequential.geometry, o.order.point_order, o.merge_points = 0, 1, merge
    count = len(SETS[which])
    h = C.c_void_p()
    t0 = time.perf_counter()
    st = L.dsa_encode_merged_sequential_batch(ctx._h, count, ARRAYS[which], None, C.byref(o), C.byref(h))
    dt = time.perf_counter() - t0
    if st != 0:
        raise RuntimeError(ctx.error())
    out, failed, total, points = {}, 0, 0, 0
    p, ln, entries = C.c_void_p(), C.c_size_t(), C.c_uint32()
    for i in range(count):
        if L.dsa_encoded_stream(h, i, C.byref(p), C.byref(ln)) != 0:
            failed += 1
            continue
        total += ln.value
        L.dsa_encoded_entry_rows(h, i, 0, None, 0, C.byref(entries))
        points += entries.value
        if i in sample:
            out[i] = C.string_at(p, ln.value)
    L.dsa_encoded_free(h)
    return dt, failed, out, total / max(1, count - failed), points / max(1, count - failed)


for share in shares:
    print("---- %.0f %% of the points of every cloud repeat the position of another" % (100 * share), flush=True)
    large = [duplicated(ordercases.height_field(256, 256, 500 + i), share, 700 + i) for i in range(min(n, 8))]
    small = [duplicated(ordercases.height_field(64, 64, 600 + i), share, 800 + i) for i in range(min(16 * n, 32))]
    SETS = {"large": [dsa.PointCloudData(large[i % len(large)]) for i in range(n)], "small": [dsa.PointCloudData(small[i % len(small)]) for i in range(16 * n)]}
    ARRAYS = {k: encodecall.arrays(v)[0] for k, v in SETS.items()}
    LEGS = [("(a) %d clouds of 65 536 points, ordered" % n, "large", 0), ("(b) %d clouds of 65 536 points, merged" % n, "large", 1),
            ("(c) %d clouds of 4 096 points, ordered" % (16 * n), "small", 0), ("(d) %d clouds of 4 096 points, merged" % (16 * n), "small", 1)]
    for k in ("DSA_ENC_TIMING", "DSA_ENC_LANES", "DSA_ENC_HOST_PLAN"):
        os.environ.pop(k, None)
    size, points = {}, {}
    for name, which, merge in LEGS:                 # warm-up; the byte check of a sample
        count = len(SETS[which])
        dt, failed, out, size[name], points[name] = run(which, merge, (count - 1,))
        pos = SETS[which][count - 1].positions
        want = synth.encode_merged(pos)[0] if merge else synth.encode_ordered(pos, geometry=0)[0]
        print("%-46s warm-up %8.1f ms; clouds refused: %d; %9.0f bytes, %7.0f points per stream; the sampled stream equals the CPU coder's: %s" %
              (name + ":", dt * 1e3, failed, size[name], points[name], out[count - 1] == want), flush=True)
    rates = {name: [] for name, _, _ in LEGS}
    for r in range(rounds):
        for name, which, merge in LEGS:
            dt = run(which, merge)[0]
            rates[name].append(len(SETS[which]) / dt)
            print("round %d  %-46s %8.1f ms %8.0f clouds/s" % (r, name + ":", dt * 1e3, len(SETS[which]) / dt), flush=True)
    for k, (name, _, _) in enumerate(LEGS):
        v, base = rates[name], statistics.median(rates[LEGS[k - k % 2][0]])
        print("%-46s median %8.0f clouds/s  (min %.0f, max %.0f, spread %.1f %%)  %.3f of its ordered leg; %.3f of its bytes, %.3f of its points" %
              (name + ":", statistics.median(v), min(v), max(v), 100.0 * (max(v) - min(v)) / statistics.median(v), statistics.median(v) / base,
               size[name] / size[LEGS[k - k % 2][0]], points[name] / points[LEGS[k - k % 2][0]]), flush=True)

    # the share of the merge kernels: one pass of each merged leg with the stage clocks, the library's stderr into a file
    os.environ.update(DSA_ENC_TIMING="1", DSA_ENC_LANES="1", DSA_ENC_HOST_PLAN="0")
    for name, which, merge in LEGS:
        if not merge:
            continue
        with tempfile.TemporaryFile() as f:
            sys.stderr.flush()
            saved = os.dup(2)
            os.dup2(f.fileno(), 2)
            try:
                run(which, merge)
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            f.seek(0)
            text = f.read().decode(errors="replace")
        laps = {}
        for what, ms in re.findall(r"ms: (.*?)\s+([0-9.]+) ms\n", text):
            laps[what] = laps.get(what, 0.0) + float(ms)
        names = ("uploads + quantisers", "point order", "point merge", "gather to entropy coding")
        stage = sum(laps.get(k, 0.0) for k in names)
        print("%-46s %s: the merge kernels are %.1f %%, the order kernels %.1f %% of the chunks' device stage" %
              (name + ":", ", ".join("%s %.2f ms" % (k, laps.get(k, 0.0)) for k in names),
               100.0 * laps.get("point merge", 0.0) / stage if stage else float("nan"), 100.0 * laps.get("point order", 0.0) / stage if stage else float("nan")), flush=True)
