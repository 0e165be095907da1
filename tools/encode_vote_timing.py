"""Encode direction, the most frequent value of every cell in a label attribute (dsa_encode_vote_sequential_batch): ONE cloud of a few
million shuffled height-field points in which every position occurs `multiplicity` times, with a uint8 label out of eight classes and
a uint8 x 4 colour, at 11 position bits, cut into 256 parts sized on the device (part_cells = ceil(m / 256)), encoded in one process
    cell parts   the same call without the mask (the label of a kept point is the one of whichever row came first): the reference,
    (a) vote     the label voted: the extra time beside the bytes the zeroing and the four launches move,
    (b) host     the way without the new call: the cell-parts call, row_entries downloaded, the mode of every cell taken with numpy
                 (the smallest label among the most frequent), new arrays of the kept rows built and encoded again (the split call on
                 the explicit grid equal to the bounds of all rows),
    (c) one label  (a) on a cloud whose every label is the same: every run is one insert a step, every cell one slot -- the case in
                 which the adds of a long run would meet on one address, were they not gathered inside the wave.
One warm-up pass of every leg, then `rounds` passes with the legs alternating; medians, minima, maxima and spreads are reported.
usage: python tools/encode_vote_timing.py [millions of points [rounds [multiplicity]]]
       python tools/encode_vote_timing.py --laps [millions [rounds]]    the call without and with the vote alone, under DSA_ENC_TIMING:
              the library drains the stream around the groups of kernels of a chunk's device stage and prints a lap for each on stderr
              ("cell votes": the memset, k_enc_vote_count, k_enc_vote_best twice and k_enc_vote_store), each pass behind a line naming
              its leg
       python tools/encode_vote_timing.py --once [millions]             a warm-up and one call with the vote, nothing else: the
              process to put behind `rocprofv3 --kernel-trace --stats --`, whose statistics give the time of every k_enc_vote_* kernel"""
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

BITS, PARTS, VOTE, CLASSES = 11, 256, 0b010, 8


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
    return dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS, position_bits=BITS, **kw)


def cell_modes(label, cells):
    """the host's vote per cell: the most frequent label, the smallest of those that come equally often"""
    pair, count = np.unique(cells.astype(np.int64) * 256 + label.reshape(-1), return_counts=True)
    cell, value = pair >> 8, pair & 255
    order = np.lexsort((value, -count, cell))
    cell = cell[order]
    first = np.concatenate([[True], cell[1:] != cell[:-1]])
    return value[order][first].astype(np.uint8).reshape(-1, 1)


def inputs(millions, multiplicity=4):
    pos = scan(int(millions * (1 << 20)), multiplicity, 47)
    n = len(pos)
    rng = np.random.default_rng(48)
    label, colour = rng.integers(0, CLASSES, (n, 1)).astype(np.uint8), rng.integers(0, 256, (n, 4)).astype(np.uint8)
    return pos, label, colour


def clouds_of(pos, label, colour):
    return [dsa.PointCloudData(pos, attributes=[dsa.Attribute(label), dsa.Attribute(colour, attribute_type=2)])]


def part_cells(enc, cloud):
    got = enc.EncodeBatch(cloud, config())
    m = len(got.entry_rows(0)[0])
    got.close()
    return m, -(-m // PARTS)


def main(millions, rounds, multiplicity):
    ctx = dsa.Context(0)
    enc = dsa.DracoEncoder(ctx)
    pos, label, colour = inputs(millions, multiplicity)
    n = len(pos)
    cloud, same = clouds_of(pos, label, colour), clouds_of(pos, np.full_like(label, 5), colour)
    pos_grid = bounds(pos)
    m, N = part_cells(enc, cloud)
    print("one cloud of %d points (%.2f Mi), every position %d times, m = %d kept points, part_cells %d, %d rounds behind a warm-up" % (n, n / (1 << 20), multiplicity, m, N, rounds), flush=True)
    legs = ["cell parts", "(a) vote", "(b) host", "(c) one label"]
    ms, size, parts = {leg: [] for leg in legs}, {}, {}
    for r in range(rounds + 1):
        for leg in legs:
            t0 = time.perf_counter()
            if leg == "cell parts":
                got = enc.EncodeBatch(cloud, config(part_cells=N))
            elif leg == "(a) vote":
                got = enc.EncodeBatch(cloud, config(part_cells=N, vote_attributes=VOTE))
            elif leg == "(c) one label":
                got = enc.EncodeBatch(same, config(part_cells=N, vote_attributes=VOTE))
            else:
                first = enc.EncodeBatch(cloud, config(part_cells=N))
                kept = np.concatenate([first.entry_rows(s)[0] for s in first.parts(0)])
                cells = first.row_entries(0)
                first.close()
                again = dsa.PointCloudData(np.ascontiguousarray(pos[kept]), position_grid=pos_grid,
                                           attributes=[dsa.Attribute(cell_modes(label, cells)), dsa.Attribute(np.ascontiguousarray(colour[kept]), attribute_type=2)])
                got = enc.EncodeBatch([again], dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, position_bits=BITS, part_points=N))
            t1 = time.perf_counter()
            size[leg], parts[leg] = sum(len(s) for s in got), len(got)
            got.close()
            if r:
                ms[leg].append((t1 - t0) * 1e3)
            print("pass %d  %-13s  %4d parts  encode %9.2f ms" % (r, leg, parts[leg], (t1 - t0) * 1e3), flush=True)
    med = {leg: statistics.median(ms[leg]) for leg in legs}
    for leg in legs:
        print("MI355X  n %d  m %d  %-13s  %4d parts  %9d bytes  encode median %9.2f ms  min %9.2f  max %9.2f  (spread %.1f %% of the median)" %
              (n, m, leg, parts[leg], size[leg], med[leg], min(ms[leg]), max(ms[leg]), 100.0 * (max(ms[leg]) - min(ms[leg])) / med[leg]), flush=True)
    # what the zeroing and the four launches move for one voted stream of one component: table, counts and values zeroed (16 n + 4 n +
    # 8 n), the sorted keys, rows, row entries and integers of every input row (n (8 + 4 + 4 + 4)) and a slot of the table (8), the
    # table read twice (2 x 16 n), per kept point the kept row, its count, its value and the stored integer
    moved = 28 * n + 28 * n + 32 * n + m * (4 + 4 + 8 + 4)
    print("MI355X  (a) the label voted: %.2f ms, %+.2f ms against the call without the mask (whose passes ran %.2f .. %.2f ms), %d bytes against %d; the zeroing and the four launches move %.1f MB (their own time: --laps)" %
          (med["(a) vote"], med["(a) vote"] - med["cell parts"], min(ms["cell parts"]), max(ms["cell parts"]), size["(a) vote"], size["cell parts"], moved / 1e6), flush=True)
    print("MI355X  (b) the route through the host: %.2f ms, %.2f x the call with the vote; as many bytes: %s" % (med["(b) host"], med["(b) host"] / med["(a) vote"], size["(b) host"] == size["(a) vote"]), flush=True)
    print("MI355X  (c) every label the same: %.2f ms, %+.2f ms against (a)" % (med["(c) one label"], med["(c) one label"] - med["(a) vote"]), flush=True)
    ctx.close()


def laps(millions, rounds):
    ctx = dsa.Context(0)
    enc = dsa.DracoEncoder(ctx)
    pos, label, colour = inputs(millions)
    cloud, same = clouds_of(pos, label, colour), clouds_of(pos, np.full_like(label, 5), colour)
    _, N = part_cells(enc, cloud)
    for r in range(rounds + 1):
        for leg, which, cfg in (("cell parts", cloud, config(part_cells=N)), ("(a) vote", cloud, config(part_cells=N, vote_attributes=VOTE)),
                                ("(c) one label", same, config(part_cells=N, vote_attributes=VOTE))):
            print("---- pass %d  %s" % (r, leg), file=sys.stderr, flush=True)
            enc.EncodeBatch(which, cfg).close()
    ctx.close()


def once(millions):
    ctx = dsa.Context(0)
    enc = dsa.DracoEncoder(ctx)
    cloud = clouds_of(*inputs(millions))
    _, N = part_cells(enc, cloud)
    for _ in range(2):
        enc.EncodeBatch(cloud, config(part_cells=N, vote_attributes=VOTE)).close()
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
