"""Encode direction, additive levels of detail of merged point clouds (dsa_encode_lod_sequential_batch): ONE cloud of a few million
shuffled height-field points in which every position occurs `multiplicity` times, at 11 and at 14 position bits, parts of at most
4 096 kept points, encoded in one process
    cell parts   the kept order in parts (part_cells alone: the reference point),
    lod D        the levels with lod_base_bits = B - 4 and B - 8, every level in parts,
and every result decoded as one Batch.  Per leg: the streams, the encode time, the total bytes, the decode time, and per level its
points, streams and bytes.  One warm-up pass of every leg, then `rounds` alternating passes; the medians are reported.
usage: python tools/encode_lod_timing.py [millions of points [rounds [multiplicity]]]
       python tools/encode_lod_timing.py --cpu [millions [multiplicity]]      the byte table alone, from the CPU coder: no device
       python tools/encode_lod_timing.py --laps [millions [bits [D [passes]]]]     lod encodes (11 bits, D = 7, one pass) with DSA_ENC_TIMING
              set, and a cell-parts encode behind each: the laps of the chunk's device stage on stderr, "levels" the kernels of this call
       python tools/encode_lod_timing.py --calls [millions [rounds]]          the merged call and the cell-parts call (256 parts) alone,
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

import ordercases  # noqa: E402

BITS = [11, 14]
PART_CELLS = 4096


def scan(points, multiplicity, seed):
    """a height field of points / multiplicity positions, every one `multiplicity` times, shuffled"""
    side = int(np.sqrt(points // multiplicity))
    base = ordercases.height_field(side, side, seed)
    pos = np.repeat(base, multiplicity, axis=0)
    return np.ascontiguousarray(pos[np.random.default_rng(seed + 1).permutation(len(pos))])


def legs_of(bits):
    return [("cell parts", 0), ("lod", bits - 4), ("lod", bits - 8)]


def level_table(bits, D, level, points, sizes):
    """per level of a lod leg: cell bits, points, streams, bytes and bytes per point"""
    for l in sorted(set(level)):
        pick = [k for k, x in enumerate(level) if x == l]
        n, b = sum(points[k] for k in pick), sum(sizes[k] for k in pick)
        print("        %2d bits  D %2d  level %d (%2d bits a cell)  %8d points  %4d streams  %9d bytes  %6.2f bytes a point" % (bits, D, l, D + l, n, len(pick), b, b / n), flush=True)


def cpu_table(millions, multiplicity):
    import draco_sharp_amd.synth as synth
    pos = scan(int(millions * (1 << 20)), multiplicity, 47)
    print("CPU coder; one cloud of %d points (%.2f Mi), every position %d times, parts of at most %d kept points" % (len(pos), len(pos) / (1 << 20), multiplicity, PART_CELLS), flush=True)
    for bits in BITS:
        base = None
        for kind, D in legs_of(bits):
            got = synth.encode_lod_parts(pos, opt=synth.options(pos_bits=bits), part_cells=PART_CELLS, lod_base_bits=D)
            sizes = [len(s) for s in got.streams]
            base = base or sum(sizes)
            print("CPU  %2d bits  n %d  m %d  %-10s D %2d  %4d streams  %9d bytes (%.4f of cell parts)" % (bits, len(pos), len(got.kept), kind, D, len(sizes), sum(sizes), sum(sizes) / base), flush=True)
            if D:
                level_table(bits, D, got.level.tolist(), (got.ranges[:, 1].astype(np.int64) - got.ranges[:, 0]).tolist(), sizes)


def config(dsa, bits, D=0, **kw):
    return dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS, position_bits=bits, lod_base_bits=D, **kw)


def decode_ms(dsa, ctx, streams, what):
    b = dsa.Batch(ctx, streams)
    t0 = time.perf_counter()
    b.decode()
    t1 = time.perf_counter()
    bad = [s for s in range(len(streams)) if b.status(s) != 0]
    b.close()
    if bad:
        raise RuntimeError("%s: streams %s did not decode" % (what, bad[:4]))
    return (t1 - t0) * 1e3


def gpu_table(millions, rounds, multiplicity):
    import draco_sharp_amd as dsa
    ctx = dsa.Context(0)
    enc = dsa.DracoEncoder(ctx)
    pos = scan(int(millions * (1 << 20)), multiplicity, 47)
    cloud = [dsa.PointCloudData(pos)]
    print("one cloud of %d points (%.2f Mi), every position %d times, parts of at most %d kept points, %d rounds behind a warm-up" %
          (len(pos), len(pos) / (1 << 20), multiplicity, PART_CELLS, rounds), flush=True)
    for bits in BITS:
        legs = legs_of(bits)
        enc_ms, dec_ms = ({leg: [] for leg in legs} for _ in range(2))
        said = {}
        for r in range(rounds + 1):
            for leg in legs:
                kind, D = leg
                t0 = time.perf_counter()
                got = enc.EncodeBatch(cloud, config(dsa, bits, D, part_cells=PART_CELLS))
                t1 = time.perf_counter()
                streams = list(got)
                if leg not in said:
                    info = [got.part_info(s) for s in range(len(streams))]
                    said[leg] = ([got.lod_info(s).level for s in range(len(streams))] if D else None, [p.num_points for p in info], [len(s) for s in streams])
                got.close()
                d = decode_ms(dsa, ctx, streams, "%s %d" % leg)
                if r:
                    enc_ms[leg].append((t1 - t0) * 1e3)
                    dec_ms[leg].append(d)
                print("%2d bits  pass %d  %-10s D %2d  %4d streams  encode %9.1f ms  decode %9.1f ms" % (bits, r, kind, D, len(streams), (t1 - t0) * 1e3, d), flush=True)
        e0, d0, s0 = statistics.median(enc_ms[legs[0]]), statistics.median(dec_ms[legs[0]]), sum(said[legs[0]][2])
        for leg in legs:
            e, d = statistics.median(enc_ms[leg]), statistics.median(dec_ms[leg])
            level, points, sizes = said[leg]
            print("MI355X  %2d bits  n %d  m %d  %-10s D %2d  %4d streams  encode %9.1f ms (%.3f of cell parts)  %9d bytes (%.4f)  decode %9.2f ms (%.3f)" %
                  (bits, len(pos), sum(points), leg[0], leg[1], len(sizes), e, e / e0, sum(sizes), sum(sizes) / s0, d, d / d0), flush=True)
            if level:
                level_table(bits, leg[1], level, points, sizes)
    ctx.close()


def laps(millions, bits, base_bits, passes):
    import draco_sharp_amd as dsa
    ctx = dsa.Context(0)
    enc = dsa.DracoEncoder(ctx)
    cloud = [dsa.PointCloudData(scan(int(millions * (1 << 20)), 4, 47))]
    enc.EncodeBatch(cloud, config(dsa, bits, base_bits, part_cells=PART_CELLS)).close()         # warm-up
    os.environ["DSA_ENC_TIMING"] = "1"
    for r in range(passes):
        for D in (base_bits, 0):
            t0 = time.perf_counter()
            enc.EncodeBatch(cloud, config(dsa, bits, D, part_cells=PART_CELLS)).close()
            print("%d bits, lod_base_bits %d, pass %d: the call took %.1f ms" % (bits, D, r, (time.perf_counter() - t0) * 1e3), file=sys.stderr, flush=True)
    ctx.close()


def calls_table(millions, rounds):
    import draco_sharp_amd as dsa
    ctx = dsa.Context(0)
    enc = dsa.DracoEncoder(ctx)
    pos = scan(int(millions * (1 << 20)), 4, 47)
    cloud = [dsa.PointCloudData(pos)]
    print("library %s; one cloud of %d points, %d passes behind a warm-up" % (os.environ.get("DSA_LIB", "in tree"), len(pos), rounds), flush=True)
    merged = dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS, position_bits=11)
    got = enc.EncodeBatch(cloud, merged)
    m = len(got.entry_rows(0)[0])
    got.close()
    parts = dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS, position_bits=11, part_cells=-(-m // 256))
    for name, cfg in (("merged call", merged), ("cell-parts call, 256 parts", parts)):
        ms = []
        for r in range(rounds + 1):
            t0 = time.perf_counter()
            got = enc.EncodeBatch(cloud, cfg)
            t1 = time.perf_counter()
            total, streams = sum(got.sizes), len(got)
            got.close()
            if r:
                ms.append((t1 - t0) * 1e3)
        print("MI355X  %-27s  %4d streams  %9d bytes  encode median %9.2f ms  min %9.2f  max %9.2f  (spread %.1f %% of the median)" %
              (name, streams, total, statistics.median(ms), min(ms), max(ms), 100.0 * (max(ms) - min(ms)) / statistics.median(ms)), flush=True)
    ctx.close()


args = [a for a in sys.argv[1:] if not a.startswith("--")]
if "--cpu" in sys.argv[1:]:
    cpu_table(float(args[0]) if len(args) > 0 else 4.0, int(args[1]) if len(args) > 1 else 4)
elif "--laps" in sys.argv[1:]:
    laps(float(args[0]) if len(args) > 0 else 4.0, int(args[1]) if len(args) > 1 else 11, int(args[2]) if len(args) > 2 else 7, int(args[3]) if len(args) > 3 else 1)
elif "--calls" in sys.argv[1:]:
    calls_table(float(args[0]) if len(args) > 0 else 4.0, int(args[1]) if len(args) > 1 else 7)
else:
    gpu_table(float(args[0]) if len(args) > 0 else 4.0, int(args[1]) if len(args) > 1 else 2, int(args[2]) if len(args) > 2 else 4)
