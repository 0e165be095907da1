"""Encode direction, one point per quantisation cell AND parts of bounded size (dsa_encode_cell_parts_sequential_batch): ONE cloud of
a few million shuffled height-field points in which every position occurs `multiplicity` times (m about n / multiplicity kept
points), at 11 and at 14 position bits, encoded in one process
    merged       as the merged single stream (merge_points alone: the reference point, "of 0"),
    part_cells   in 16, 256 and 4096 parts sized on the device (part_cells = ceil(m / parts)),
    round trip   the way without the new call: the merged call, kept downloaded, rows[kept] gathered on the host, then the split call
                 (part_points) on explicit grids equal to the bounds of all rows -- for 256 parts; its streams must be the new call's,
and every result decoded as one Batch.  Per leg: the parts, the encode time, the total bytes, the decode time.  One warm-up pass of
every leg, then `rounds` alternating passes; the medians are reported.
usage: python tools/encode_cell_parts_timing.py [millions of points [rounds [multiplicity]]]
       python tools/encode_cell_parts_timing.py --calls [millions [rounds]]    the merged call and the split call (256 parts) alone,
              seven passes each behind a warm-up, median and spread: run once per library build (DSA_LIB) to hold two builds against
              each other on one box -- neither call is new, so a build without the new entry point runs this leg too"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import draco_sharp_amd as dsa  # noqa: E402
import ordercases  # noqa: E402

PARTS = [16, 256, 4096]
BITS = [11, 14]


def scan(points, multiplicity, seed):
    """a height field of points / multiplicity positions, every one `multiplicity` times, shuffled"""
    side = int(np.sqrt(points // multiplicity))
    base = ordercases.height_field(side, side, seed)
    pos = np.repeat(base, multiplicity, axis=0)
    return np.ascontiguousarray(pos[np.random.default_rng(seed + 1).permutation(len(pos))])


def bounds(values):
    v = np.asarray(values, np.float32).reshape(len(values), -1)
    mn = v.min(axis=0)
    rng = np.float32((v.max(axis=0) - mn).astype(np.float32).max())
    return dsa.Grid(mn, float(rng) if rng != 0 else 1.0)


def decode_ms(ctx, streams, what):
    b = dsa.Batch(ctx, streams)
    t0 = time.perf_counter()
    b.decode()
    t1 = time.perf_counter()
    bad = [s for s in range(len(streams)) if b.status(s) != 0]
    b.close()
    if bad:
        raise RuntimeError("%s: streams %s did not decode" % (what, bad[:4]))
    return (t1 - t0) * 1e3


def merged_config(bits, **kw):
    return dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS, position_bits=bits, **kw)


def gpu_table(millions, rounds, multiplicity):
    ctx = dsa.Context(0)
    enc = dsa.DracoEncoder(ctx)
    pos = scan(int(millions * (1 << 20)), multiplicity, 47)
    cloud = [dsa.PointCloudData(pos)]
    grid = bounds(pos)
    print("one cloud of %d points (%.2f Mi), every position %d times, %d rounds behind a warm-up" % (len(pos), len(pos) / (1 << 20), multiplicity, rounds), flush=True)
    for bits in BITS:
        got = enc.EncodeBatch(cloud, merged_config(bits))
        m = len(got.entry_rows(0)[0])
        got.close()
        size_of = {P: -(-m // P) for P in PARTS}
        legs = [("merged", 0)] + [("part_cells", P) for P in PARTS] + [("round trip", 256)]
        enc_ms, dec_ms, size, parts = ({leg: [] for leg in legs} for _ in range(4))
        streams_of = {}
        for r in range(rounds + 1):
            for leg in legs:
                kind, P = leg
                t0 = time.perf_counter()
                if kind == "merged":
                    got = enc.EncodeBatch(cloud, merged_config(bits))
                elif kind == "part_cells":
                    got = enc.EncodeBatch(cloud, merged_config(bits, part_cells=size_of[P]))
                else:
                    first = enc.EncodeBatch(cloud, merged_config(bits))
                    kept = first.entry_rows(0)[0]
                    first.close()
                    got = enc.EncodeBatch([dsa.PointCloudData(np.ascontiguousarray(pos[kept]), position_grid=grid)],
                                          dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, position_bits=bits, part_points=size_of[P]))
                t1 = time.perf_counter()
                streams = list(got)
                got.close()
                d = decode_ms(ctx, streams, "%s %d" % leg)
                size[leg], parts[leg], streams_of[leg] = sum(len(s) for s in streams), len(streams), streams
                if r:
                    enc_ms[leg].append((t1 - t0) * 1e3)
                    dec_ms[leg].append(d)
                print("%2d bits  pass %d  %-10s  %4d parts  encode %9.1f ms  decode %9.1f ms" % (bits, r, kind, parts[leg], (t1 - t0) * 1e3, d), flush=True)
        same = streams_of[("round trip", 256)] == streams_of[("part_cells", 256)]
        e0, d0, s0 = statistics.median(enc_ms[legs[0]]), statistics.median(dec_ms[legs[0]]), size[legs[0]]
        for leg in legs:
            e, d = statistics.median(enc_ms[leg]), statistics.median(dec_ms[leg])
            print("MI355X  %2d bits  n %d  m %d  %-10s  %4d parts  encode %9.1f ms (%.3f of the merged stream's)  %9d bytes (%.4f)  decode %9.1f ms (%.4f)" %
                  (bits, len(pos), m, leg[0], parts[leg], e, e / e0, size[leg], size[leg] / s0, d, d / d0), flush=True)
        e_new, e_old = statistics.median(enc_ms[("part_cells", 256)]), statistics.median(enc_ms[("round trip", 256)])
        print("MI355X  %2d bits  256 parts: part_cells %.1f ms, the round trip through the host %.1f ms (%.2f x); the same streams: %s" % (bits, e_new, e_old, e_old / e_new, same), flush=True)
    ctx.close()


def calls_table(millions, rounds):
    ctx = dsa.Context(0)
    enc = dsa.DracoEncoder(ctx)
    pos = scan(int(millions * (1 << 20)), 4, 47)
    cloud = [dsa.PointCloudData(pos)]
    print("library %s; one cloud of %d points, %d passes behind a warm-up" % (os.environ.get("DSA_LIB", "in tree"), len(pos), rounds), flush=True)
    for name, cfg in (("merged call", merged_config(11)),
                      ("split call, 256 parts", dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, position_bits=11, part_points=len(pos) // 256))):
        ms = []
        for r in range(rounds + 1):
            t0 = time.perf_counter()
            got = enc.EncodeBatch(cloud, cfg)
            t1 = time.perf_counter()
            total = sum(got.sizes)
            got.close()
            if r:
                ms.append((t1 - t0) * 1e3)
        print("MI355X  %-22s  %9d bytes  encode median %9.2f ms  min %9.2f  max %9.2f  (spread %.1f %% of the median)" %
              (name, total, statistics.median(ms), min(ms), max(ms), 100.0 * (max(ms) - min(ms)) / statistics.median(ms)), flush=True)
    ctx.close()


args = [a for a in sys.argv[1:] if not a.startswith("--")]
if "--calls" in sys.argv[1:]:
    calls_table(float(args[0]) if len(args) > 0 else 4.0, int(args[1]) if len(args) > 1 else 7)
else:
    gpu_table(float(args[0]) if len(args) > 0 else 4.0, int(args[1]) if len(args) > 1 else 2, int(args[2]) if len(args) > 2 else 4)
