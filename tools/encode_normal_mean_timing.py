"""Encode direction, the mean normal of every cell (dsa_encode_normal_mean_sequential_batch): ONE cloud of a few million shuffled
height-field points in which every position occurs `multiplicity` times (the scan of tools/encode_mean_timing.py), with normals that
follow the surface with noise, at 11 position bits and 10 normal bits, cut into 256 parts sized on the device (part_cells = ceil(m /
256)), encoded in one process
    (a) mean normals  the call with mean_normals: the extra time beside the bytes the zeroing and the two launches move,
    (b) cell parts    the same call with mean_normals off (the normal of a kept point is the one of whichever row came first): the reference,
    (c) host          the way without the new call: the cell-parts call, row_entries downloaded, the rows' normals normalised and summed
                      per cell with numpy, new arrays of the kept rows built and encoded again (the split call on the explicit grid
                      equal to the bounds of all rows).
One warm-up pass of every leg, then `rounds` passes with the legs alternating; medians, minima, maxima and spreads are reported.
usage: python tools/encode_normal_mean_timing.py [millions of points [rounds [multiplicity]]]
       python tools/encode_normal_mean_timing.py --laps [millions [rounds]]    the call without and with mean_normals, under
              DSA_ENC_TIMING: the library drains the stream around the groups of kernels of a chunk's device stage and prints a lap
              for each on stderr ("cell normals": the memset, k_enc_normal_sum and k_enc_normal_store), each pass behind a line
              naming its leg
       python tools/encode_normal_mean_timing.py --once [millions]             a warm-up and one call with mean_normals, nothing else:
              the process to put behind `rocprofv3 --kernel-trace --stats --`, whose statistics give the time of each of the two kernels"""
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

BITS, NORMAL_BITS, PARTS = 11, 10, 256


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


def config(**kw):
    return dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS, position_bits=BITS, normal_bits=NORMAL_BITS, **kw)


def inputs(millions, multiplicity=4):
    pos = scan(int(millions * (1 << 20)), multiplicity, 47)
    rng = np.random.default_rng(48)
    nrm = np.float32([0.2, 0.3, 1.0]) + rng.normal(size=(len(pos), 3)).astype(np.float32) * np.float32(0.25)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return pos, np.ascontiguousarray(nrm, np.float32)


def cell_normals(nrm, cells, m):
    """the host's mean normal per cell: the rows normalised, summed and normalised again, in float64"""
    v = np.asarray(nrm, np.float64)
    v = v / np.linalg.norm(v, axis=1)[:, None]
    total = np.stack([np.bincount(cells, weights=v[:, c], minlength=m) for c in range(3)], axis=1)
    length = np.linalg.norm(total, axis=1)
    return np.where(length[:, None] > 0, total / np.where(length > 0, length, 1.0)[:, None], [1.0, 0.0, 0.0]).astype(np.float32)


def part_cells(enc, cloud):
    got = enc.EncodeBatch(cloud, config())
    m = len(got.entry_rows(0)[0])
    got.close()
    return m, -(-m // PARTS)


def main(millions, rounds, multiplicity):
    ctx = dsa.Context(0)
    enc = dsa.DracoEncoder(ctx)
    pos, nrm = inputs(millions, multiplicity)
    n = len(pos)
    cloud = [dsa.PointCloudData(pos, normals=nrm)]
    pos_grid = bounds(pos)
    m, N = part_cells(enc, cloud)
    print("one cloud of %d points (%.2f Mi), every position %d times, m = %d kept points, part_cells %d, %d rounds behind a warm-up" % (n, n / (1 << 20), multiplicity, m, N, rounds), flush=True)
    legs = ["(b) cell parts", "(a) mean normals", "(c) host"]
    ms, size, parts = {leg: [] for leg in legs}, {}, {}
    for r in range(rounds + 1):
        for leg in legs:
            t0 = time.perf_counter()
            if leg == "(b) cell parts":
                got = enc.EncodeBatch(cloud, config(part_cells=N))
            elif leg == "(a) mean normals":
                got = enc.EncodeBatch(cloud, config(part_cells=N, mean_normals=True))
            else:
                first = enc.EncodeBatch(cloud, config(part_cells=N))
                kept = np.concatenate([first.entry_rows(s)[0] for s in first.parts(0)])
                cells = first.row_entries(0)
                first.close()
                again = dsa.PointCloudData(np.ascontiguousarray(pos[kept]), normals=cell_normals(nrm, cells, len(kept)), position_grid=pos_grid)
                got = enc.EncodeBatch([again], dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, position_bits=BITS, normal_bits=NORMAL_BITS, part_points=N))
            t1 = time.perf_counter()
            size[leg], parts[leg] = sum(len(s) for s in got), len(got)
            got.close()
            if r:
                ms[leg].append((t1 - t0) * 1e3)
            print("pass %d  %-16s  %4d parts  encode %9.2f ms" % (r, leg, parts[leg], (t1 - t0) * 1e3), flush=True)
    med = {leg: statistics.median(ms[leg]) for leg in legs}
    for leg in legs:
        print("MI355X  n %d  m %d  %-16s  %4d parts  %9d bytes  encode median %9.2f ms  min %9.2f  max %9.2f  (spread %.1f %% of the median)" %
              (n, m, leg, parts[leg], size[leg], med[leg], min(ms[leg]), max(ms[leg]), 100.0 * (max(ms[leg]) - min(ms[leg])) / med[leg]), flush=True)
    # what the zeroing and the two launches move: sums and counts zeroed (24 n + 4 n), the sorted keys, rows, row entries and codes of
    # every input row (n (8 + 4 + 4 + 8)), per kept point the kept row, its count, its three sums and the stored code
    moved = 28 * n + 24 * n + m * (4 + 4 + 24 + 8)
    a, b = med["(a) mean normals"], med["(b) cell parts"]
    print("MI355X  (a) the normals averaged: %.2f ms, %+.2f ms against (b) the call without them (whose passes ran %.2f .. %.2f ms), %d bytes against %d; the zeroing and the two launches move %.1f MB (their own time: --laps)" %
          (a, a - b, min(ms["(b) cell parts"]), max(ms["(b) cell parts"]), size["(a) mean normals"], size["(b) cell parts"], moved / 1e6), flush=True)
    print("MI355X  (c) the route through the host: %.2f ms, %.2f x the call with mean_normals" % (med["(c) host"], med["(c) host"] / a), flush=True)
    ctx.close()


def laps(millions, rounds):
    ctx = dsa.Context(0)
    enc = dsa.DracoEncoder(ctx)
    pos, nrm = inputs(millions)
    cloud = [dsa.PointCloudData(pos, normals=nrm)]
    _, N = part_cells(enc, cloud)
    for r in range(rounds + 1):
        for leg, cfg in (("(b) cell parts", config(part_cells=N)), ("(a) mean normals", config(part_cells=N, mean_normals=True))):
            print("---- pass %d  %s" % (r, leg), file=sys.stderr, flush=True)
            enc.EncodeBatch(cloud, cfg).close()
    ctx.close()


def once(millions):
    ctx = dsa.Context(0)
    enc = dsa.DracoEncoder(ctx)
    pos, nrm = inputs(millions)
    cloud = [dsa.PointCloudData(pos, normals=nrm)]
    _, N = part_cells(enc, cloud)
    for _ in range(2):
        enc.EncodeBatch(cloud, config(part_cells=N, mean_normals=True)).close()
    ctx.close()


args = [a for a in sys.argv[1:] if not a.startswith("--")]
if "--laps" in sys.argv[1:]:
    os.environ["DSA_ENC_TIMING"] = "1"
    laps(float(args[0]) if len(args) > 0 else 4.0, int(args[1]) if len(args) > 1 else 3)
    sys.exit(0)
if "--once" in sys.argv[1:]:
    once(float(args[0]) if len(args) > 0 else 4.0)
    sys.exit(0)
main(float(args[0]) if len(args) > 0 else 4.0, int(args[1]) if len(args) > 1 else 7, int(args[2]) if len(args) > 2 else 4)
