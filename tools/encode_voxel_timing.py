"""Encode direction, voxels coarser than the position grid (dsa_encode_voxel_sequential_batch): ONE cloud of a few million shuffled
height-field points in which every position occurs `multiplicity` times (the scan of tools/encode_mean_timing.py) with a colour to
average, stored at 14 position bits and kept one point per cell of the grid with 11 bits per axis (voxel_bits = 11), cut into 256
parts sized on the device (part_cells = ceil(m / 256)), encoded in one process
    (c) centroid      the call with voxel_point = VOXEL_POINT_CENTROID,
    (n) nearest       the call with voxel_point = VOXEL_POINT_NEAREST,
    (a) 11 bits       the closest request without the option: the same call at position_bits = 11, voxel_bits = 0 -- the same
                      voxels, every kept point on the lattice of the 11-bit grid,
    (b) host          the way without the new call: the cell-parts call at 14 bits, kept rows, row entries and cell counts
                      downloaded, the voxel of every kept cell, its centroid (weighted by the cell's rows) or its nearest cell and
                      its mean colour with numpy, the chosen points encoded again (the split call on the explicit grid equal to
                      the bounds of all rows).
One warm-up pass of every leg, then `rounds` passes with the legs alternating; medians, minima, maxima and spreads are reported.
usage: python tools/encode_voxel_timing.py [millions of points [rounds [multiplicity]]]
       python tools/encode_voxel_timing.py --plain [millions [rounds]]     leg (a) alone, `rounds` passes behind a warm-up: the call with
              voxel_bits = 0, to run once with this library and once with another build named by DSA_LIB
       python tools/encode_voxel_timing.py --laps [millions [rounds]]      legs (a), (c) and (n) under DSA_ENC_TIMING: the library drains
              the stream around the groups of kernels of a chunk's device stage and prints a lap for each on stderr ("voxel
              nearest": the memset, the two phases of k_enc_voxel_near and k_enc_voxel_pick; "cell means": the memset, k_enc_mean_sum
              and k_enc_mean_store with the positions among their streams), each pass behind a line naming its leg
       python tools/encode_voxel_timing.py --once [millions]               a warm-up and one call of (c) and of (n), nothing else: the
              process to put behind `rocprofv3 --kernel-trace --stats --`, whose statistics give the time of each kernel"""
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

BITS, VOXEL_BITS, PARTS = 14, 11, 256


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
    return mn, (rng if rng != 0 else np.float32(1.0))


def config(bits=BITS, **kw):
    return dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS, position_bits=bits, **kw)


def inputs(millions, multiplicity=4):
    pos = scan(int(millions * (1 << 20)), multiplicity, 47)
    colour = np.random.default_rng(48).integers(0, 256, (len(pos), 3)).astype(np.uint8)
    return pos, colour


def part_cells(enc, cloud):
    got = enc.EncodeBatch(cloud, config(voxel_bits=VOXEL_BITS))
    m = len(got.entry_rows(0)[0])
    got.close()
    return m, -(-m // PARTS)


LEGS = {"(c) centroid": dict(voxel_bits=VOXEL_BITS, voxel_point=dsa.VOXEL_POINT_CENTROID), "(n) nearest": dict(voxel_bits=VOXEL_BITS, voxel_point=dsa.VOXEL_POINT_NEAREST)}


def through_the_host(enc, cloud, pos, colour, origin, rng, N, nearest):
    """leg (b): the 14-bit cells from the device, the voxels with numpy, a second encode"""
    first = enc.EncodeBatch(cloud, config(part_cells=N))
    kept = np.concatenate([first.entry_rows(s)[0] for s in first.parts(0)])
    cells, counts = first.row_entries(0), first.cell_counts(0)
    first.close()
    scale = np.float32(np.float32((1 << BITS) - 1) / rng)
    q = np.floor(((pos[kept] - origin).astype(np.float32) * scale).astype(np.float32) + np.float32(0.5)).astype(np.int64)
    s = BITS - VOXEL_BITS
    v = q >> s
    ids = (v[:, 0] << (2 * VOXEL_BITS)) | (v[:, 1] << VOXEL_BITS) | v[:, 2]
    _, voxel = np.unique(ids, return_inverse=True)
    voxel = np.asarray(voxel).ravel()
    m = int(voxel.max()) + 1
    rows = np.bincount(voxel, weights=counts, minlength=m)
    if nearest:
        d = 2 * (q & ((1 << s) - 1)) - ((1 << s) - 1)
        order = np.lexsort((kept, (d * d).sum(axis=1), voxel))
        pick = order[np.r_[True, voxel[order][1:] != voxel[order][:-1]]]
        out = pos[kept[pick]]
    else:
        mean = np.stack([np.bincount(voxel, weights=q[:, c] * counts, minlength=m) for c in range(3)], axis=1)
        p = np.floor((2 * mean + rows[:, None]) / (2 * rows[:, None]))
        out = ((p.astype(np.float32) * np.float32(rng / np.float32((1 << BITS) - 1))).astype(np.float32) + origin).astype(np.float32)
    of_row = voxel[cells]
    col = np.stack([np.bincount(of_row, weights=colour[:, c], minlength=m) for c in range(3)], axis=1)
    col = np.floor((2 * col + rows[:, None]) / (2 * rows[:, None])).astype(np.uint8)
    again = dsa.PointCloudData(np.ascontiguousarray(out, np.float32), attributes=[dsa.Attribute(np.ascontiguousarray(col))], position_grid=dsa.Grid(origin, float(rng)))
    return enc.EncodeBatch([again], dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, position_bits=BITS, part_points=-(-m // PARTS)))


def main(millions, rounds, multiplicity):
    ctx = dsa.Context(0)
    enc = dsa.DracoEncoder(ctx)
    pos, colour = inputs(millions, multiplicity)
    n = len(pos)
    cloud = [dsa.PointCloudData(pos, attributes=[dsa.Attribute(colour)])]
    origin, rng = bounds(pos)
    m, N = part_cells(enc, cloud)
    first = enc.EncodeBatch(cloud, config())
    m14 = len(first.entry_rows(0)[0])
    first.close()
    N14 = -(-m14 // PARTS)
    print("one cloud of %d points (%.2f Mi), every position %d times, %d cells at %d bits, m = %d voxels at %d bits, part_cells %d, %d rounds behind a warm-up" %
          (n, n / (1 << 20), multiplicity, m14, BITS, m, VOXEL_BITS, N, rounds), flush=True)
    legs = ["(a) 11 bits", "(c) centroid", "(n) nearest", "(b) host centroid", "(b) host nearest"]
    ms, size, parts = {leg: [] for leg in legs}, {}, {}
    for r in range(rounds + 1):
        for leg in legs:
            t0 = time.perf_counter()
            if leg == "(a) 11 bits":
                got = enc.EncodeBatch(cloud, config(VOXEL_BITS, part_cells=N, mean_attributes=[1]))
            elif leg in LEGS:
                got = enc.EncodeBatch(cloud, config(part_cells=N, mean_attributes=[1], **LEGS[leg]))
            else:
                got = through_the_host(enc, cloud, pos, colour, origin, rng, N14, leg.endswith("nearest"))
            t1 = time.perf_counter()
            size[leg], parts[leg] = sum(len(s) for s in got), len(got)
            got.close()
            if r:
                ms[leg].append((t1 - t0) * 1e3)
            print("pass %d  %-18s  %4d parts  encode %9.2f ms" % (r, leg, parts[leg], (t1 - t0) * 1e3), flush=True)
    med = {leg: statistics.median(ms[leg]) for leg in legs}
    for leg in legs:
        print("MI355X  n %d  m %d  %-18s  %4d parts  %9d bytes  encode median %9.2f ms  min %9.2f  max %9.2f  (spread %.1f %% of the median)" %
              (n, m, leg, parts[leg], size[leg], med[leg], min(ms[leg]), max(ms[leg]), 100.0 * (max(ms[leg]) - min(ms[leg])) / med[leg]), flush=True)
    a = med["(a) 11 bits"]
    for leg, host in (("(c) centroid", "(b) host centroid"), ("(n) nearest", "(b) host nearest")):
        print("MI355X  %s: %.2f ms, %+.2f ms against (a) the same voxels at 11 position bits (whose passes ran %.2f .. %.2f ms), %d bytes against %d; %s: %.2f ms, %.2f x" %
              (leg, med[leg], med[leg] - a, min(ms["(a) 11 bits"]), max(ms["(a) 11 bits"]), size[leg], size["(a) 11 bits"], host, med[host], med[host] / med[leg]), flush=True)
    ctx.close()


def plain(millions, rounds):
    ctx = dsa.Context(0)
    enc = dsa.DracoEncoder(ctx)
    pos, colour = inputs(millions)
    cloud = [dsa.PointCloudData(pos, attributes=[dsa.Attribute(colour)])]
    got = enc.EncodeBatch(cloud, config(VOXEL_BITS))
    N = -(-len(got.entry_rows(0)[0]) // PARTS)
    got.close()
    ms = []
    for r in range(rounds + 1):
        t0 = time.perf_counter()
        got = enc.EncodeBatch(cloud, config(VOXEL_BITS, part_cells=N, mean_attributes=[1]))
        t1 = time.perf_counter()
        size = sum(len(s) for s in got)
        got.close()
        if r:
            ms.append((t1 - t0) * 1e3)
    print("MI355X  library %s  n %d  (a) 11 bits, voxel_bits 0  %d bytes  encode median %.2f ms  min %.2f  max %.2f  over %d passes" %
          (os.environ.get("DSA_LIB") or "of the tree", len(pos), size, statistics.median(ms), min(ms), max(ms), rounds), flush=True)
    ctx.close()


def laps(millions, rounds):
    ctx = dsa.Context(0)
    enc = dsa.DracoEncoder(ctx)
    pos, colour = inputs(millions)
    cloud = [dsa.PointCloudData(pos, attributes=[dsa.Attribute(colour)])]
    _, N = part_cells(enc, cloud)
    for r in range(rounds + 1):
        for leg, cfg in [("(a) 11 bits", config(VOXEL_BITS, part_cells=N, mean_attributes=[1]))] + [(leg, config(part_cells=N, mean_attributes=[1], **kw)) for leg, kw in LEGS.items()]:
            print("---- pass %d  %s" % (r, leg), file=sys.stderr, flush=True)
            enc.EncodeBatch(cloud, cfg).close()
    ctx.close()


def once(millions):
    ctx = dsa.Context(0)
    enc = dsa.DracoEncoder(ctx)
    pos, colour = inputs(millions)
    cloud = [dsa.PointCloudData(pos, attributes=[dsa.Attribute(colour)])]
    _, N = part_cells(enc, cloud)
    for _ in range(2):
        for kw in LEGS.values():
            enc.EncodeBatch(cloud, config(part_cells=N, mean_attributes=[1], **kw)).close()
    ctx.close()


args = [a for a in sys.argv[1:] if not a.startswith("--")]
if "--plain" in sys.argv[1:]:
    plain(float(args[0]) if len(args) > 0 else 4.0, int(args[1]) if len(args) > 1 else 7)
    sys.exit(0)
if "--laps" in sys.argv[1:]:
    os.environ["DSA_ENC_TIMING"] = "1"
    laps(float(args[0]) if len(args) > 0 else 4.0, int(args[1]) if len(args) > 1 else 3)
    sys.exit(0)
if "--once" in sys.argv[1:]:
    once(float(args[0]) if len(args) > 0 else 4.0)
    sys.exit(0)
main(float(args[0]) if len(args) > 0 else 4.0, int(args[1]) if len(args) > 1 else 7, int(args[2]) if len(args) > 2 else 4)
