"""Encode direction, the Morton order of a point cloud in parts of bounded size (dsa_encode_split_sequential_batch): ONE cloud of a
few million shuffled height-field points, at 11 and at 14 position bits, encoded in one process at part_points 0 (one stream: the
call as it was, byte for byte), 1 Mi, 256 Ki, 64 Ki and 16 Ki, and every result decoded as one Batch.  Per leg: the parts, the
encode time, the total bytes against the single stream's (what a header and a set of tables per part cost), the decode time of all
parts in one Batch against the single stream's, and whether part 0 equals the CPU coder's.  One warm-up pass of every leg, then
`rounds` alternating passes; the medians are reported.
usage: python tools/encode_split_timing.py [millions of points [rounds]]
       python tools/encode_split_timing.py --cpu      the byte cost alone, from the CPU coder (synth.encode_split), for a 1 Mi-point
                                                      height field and a 1 Mi-point random cloud: needs no device"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import draco_sharp_amd as dsa  # noqa: E402
import draco_sharp_amd.synth as synth  # noqa: E402
import ordercases  # noqa: E402

PART_POINTS = [0, 1 << 20, 1 << 18, 1 << 16, 1 << 14]
BITS = [11, 14]


def field(points, seed):
    side = int(np.sqrt(points))
    return ordercases.height_field(side, side, seed)


def cpu_table():
    clouds = [("height field", field(1 << 20, 41)), ("random cloud", ordercases.random_cloud(1 << 20, 42))]
    for name, pos in clouds:
        for bits in BITS:
            opt = synth.options(pos_bits=bits)
            base = None
            for N in PART_POINTS:
                parts = synth.encode_split(pos, opt=opt, part_points=N)
                total = sum(len(p[0]) for p in parts)
                base = base or total
                print("CPU coder  %-12s %7d points  %2d bits  part_points %8d  %4d parts  %9d bytes  %.4f of the single stream  (%+.1f bytes per part)" %
                      (name, len(pos), bits, N, len(parts), total, total / base, (total - base) / max(1, len(parts) - 1) if len(parts) > 1 else 0.0), flush=True)


def gpu_table(millions, rounds):
    ctx = dsa.Context(0)
    enc = dsa.DracoEncoder(ctx)
    pos = field(int(millions * (1 << 20)), 43)
    cloud = [dsa.PointCloudData(pos)]
    print("one cloud of %d points (%.2f Mi), %d rounds behind a warm-up" % (len(pos), len(pos) / (1 << 20), rounds), flush=True)
    for bits in BITS:
        legs = [(N, dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, position_bits=bits, part_points=N)) for N in PART_POINTS]
        enc_ms, dec_ms, size, parts, same = ({N: [] for N in PART_POINTS} for _ in range(5))
        twin0 = {}
        for N in PART_POINTS:                       # part 0 of every leg by the CPU coder
            kw = synth.split_arguments(pos, opt=synth.options(pos_bits=bits), part_points=N)[0][3]
            twin0[N] = synth.encode_grid(kw.pop("pos"), None, form=0, geometry=0, **kw)
        for r in range(rounds + 1):
            for N, cfg in legs:
                t0 = time.perf_counter()
                got = enc.EncodeBatch(cloud, cfg)
                t1 = time.perf_counter()
                streams = list(got)
                b = dsa.Batch(ctx, streams)
                t2 = time.perf_counter()
                b.decode()
                t3 = time.perf_counter()
                bad = [s for s in range(len(streams)) if b.status(s) != 0]
                b.close()
                got.close()
                if bad:
                    raise RuntimeError("part_points %d: streams %s did not decode" % (N, bad[:4]))
                size[N], parts[N] = sum(len(s) for s in streams), len(streams)
                same[N] = streams[0] == twin0[N]
                if r:
                    enc_ms[N].append((t1 - t0) * 1e3)
                    dec_ms[N].append((t3 - t2) * 1e3)
                print("%2d bits  pass %d  part_points %8d  %4d parts  encode %9.1f ms  decode %9.1f ms" % (bits, r, N, parts[N], (t1 - t0) * 1e3, (t3 - t2) * 1e3), flush=True)
        e0, d0 = statistics.median(enc_ms[0]), statistics.median(dec_ms[0])
        for N in PART_POINTS:
            e, d = statistics.median(enc_ms[N]), statistics.median(dec_ms[N])
            print("MI355X  %2d bits  part_points %8d  %4d parts  encode %9.1f ms (%.3f of the single stream's)  %9d bytes (%.4f)  decode %9.1f ms (%.3f)  part 0 equals the CPU coder's: %s" %
                  (bits, N, parts[N], e, e / e0, size[N], size[N] / size[0], d, d / d0, same[N]), flush=True)
    ctx.close()


if "--cpu" in sys.argv[1:]:
    cpu_table()
else:
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    gpu_table(float(args[0]) if len(args) > 0 else 4.0, int(args[1]) if len(args) > 1 else 2)
