"""Encode direction, the mean of every cell in chosen attributes (dsa_encode_mean_sequential_batch): ONE cloud of a few million
shuffled height-field points in which every position occurs `multiplicity` times, with a uint8 x 4 colour and one float attribute (16
bits), at 11 position bits, cut into 256 parts sized on the device (part_cells = ceil(m / 256)), encoded in one process
    cell parts   dsa_encode_cell_parts_sequential_batch, the call as it was before mean_attributes: the reference,
    (a) mask 0   dsa_encode_mean_sequential_batch with mean_attributes = 0: the same request through the new entry -- no kernel of
                 it is new, so its median must lie within the run-to-run spread of the reference that this run itself reports,
    (b) means    both attributes masked: the extra time beside the bytes the zeroing and the two passes move,
    (c) host     the way without the new call: the cell-parts call, row_entries downloaded, the mean of every cell taken with numpy,
                 new arrays of the kept rows built and encoded again (the split call on explicit grids equal to the bounds of all rows).
One warm-up pass of every leg, then `rounds` passes with the legs alternating; medians, minima, maxima and spreads are reported.
usage: python tools/encode_mean_timing.py [millions of points [rounds [multiplicity]]]
       python tools/encode_mean_timing.py --laps [millions [rounds]]    the cell-parts call and the call with the means alone, under
              DSA_ENC_TIMING: the library drains the stream around the groups of kernels of a chunk's device stage and prints a lap
              for each on stderr ("cell means": the memset, k_enc_mean_sum and k_enc_mean_store), each pass behind a line naming its leg"""
import ctypes as C
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
from draco_sharp_amd import native  # noqa: E402
from draco_sharp_amd.encoder import EncodedStreams, _native_meshes  # noqa: E402

BITS, PARTS, MASK = 11, 256, 0b110


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


def new_entry(ctx, clouds, cfg, mask):
    """the new entry point itself, whatever the mask (EncodeBatch takes it only with a mask)"""
    arr, grids, keep = _native_meshes(clouds)
    o = cfg._native_mean(0, clouds)
    o.mean_attributes = mask
    h = C.c_void_p()
    st = native.lib().dsa_encode_mean_sequential_batch(ctx._h, len(clouds), arr, grids, C.byref(o), C.byref(h))
    if st != 0:
        raise RuntimeError(ctx.error())
    return EncodedStreams(ctx, h, native.lib().dsa_encoded_size(h))


def cell_means(values, cells, m):
    """the host's mean per cell and component, in float64"""
    v = np.asarray(values, np.float64).reshape(len(values), -1)
    count = np.bincount(cells, minlength=m)
    return np.stack([np.bincount(cells, weights=v[:, c], minlength=m) / count for c in range(v.shape[1])], axis=1)


def main(millions, rounds, multiplicity):
    ctx = dsa.Context(0)
    enc = dsa.DracoEncoder(ctx)
    pos = scan(int(millions * (1 << 20)), multiplicity, 47)
    n = len(pos)
    rng = np.random.default_rng(48)
    colour, scalar = rng.integers(0, 256, (n, 4)).astype(np.uint8), rng.normal(size=(n, 1)).astype(np.float32)
    cloud = [dsa.PointCloudData(pos, attributes=[dsa.Attribute(colour, attribute_type=2), dsa.Attribute(scalar, quantization_bits=16)])]
    pos_grid, scalar_grid = bounds(pos), bounds(scalar)
    got = enc.EncodeBatch(cloud, config())
    m = len(got.entry_rows(0)[0])
    got.close()
    N = -(-m // PARTS)
    print("one cloud of %d points (%.2f Mi), every position %d times, m = %d kept points, part_cells %d, %d rounds behind a warm-up" % (n, n / (1 << 20), multiplicity, m, N, rounds), flush=True)
    legs = ["cell parts", "(a) mask 0", "(b) means", "(c) host"]
    ms, size, parts, streams_of = {leg: [] for leg in legs}, {}, {}, {}
    for r in range(rounds + 1):
        for leg in legs:
            t0 = time.perf_counter()
            if leg == "cell parts":
                got = enc.EncodeBatch(cloud, config(part_cells=N))
            elif leg == "(a) mask 0":
                got = new_entry(ctx, cloud, config(part_cells=N), 0)
            elif leg == "(b) means":
                got = enc.EncodeBatch(cloud, config(part_cells=N, mean_attributes=MASK))
            else:
                first = enc.EncodeBatch(cloud, config(part_cells=N))
                kept = np.concatenate([first.entry_rows(s)[0] for s in first.parts(0)])
                cells = first.row_entries(0)
                first.close()
                mean_colour = np.clip(np.floor(cell_means(colour, cells, len(kept)) + 0.5), 0, 255).astype(np.uint8)
                mean_scalar = cell_means(scalar, cells, len(kept)).astype(np.float32)
                again = dsa.PointCloudData(np.ascontiguousarray(pos[kept]), position_grid=pos_grid,
                                           attributes=[dsa.Attribute(mean_colour, attribute_type=2), dsa.Attribute(mean_scalar, quantization_bits=16, grid=scalar_grid)])
                got = enc.EncodeBatch([again], dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, position_bits=BITS, part_points=N))
            t1 = time.perf_counter()
            streams_of[leg] = list(got)
            size[leg], parts[leg] = sum(len(s) for s in streams_of[leg]), len(got)
            got.close()
            if r:
                ms[leg].append((t1 - t0) * 1e3)
            print("pass %d  %-11s  %4d parts  encode %9.2f ms" % (r, leg, parts[leg], (t1 - t0) * 1e3), flush=True)
    med = {leg: statistics.median(ms[leg]) for leg in legs}
    for leg in legs:
        print("MI355X  n %d  m %d  %-11s  %4d parts  %9d bytes  encode median %9.2f ms  min %9.2f  max %9.2f  (spread %.1f %% of the median)" %
              (n, m, leg, parts[leg], size[leg], med[leg], min(ms[leg]), max(ms[leg]), 100.0 * (max(ms[leg]) - min(ms[leg])) / med[leg]), flush=True)
    ref = ms["cell parts"]
    inside = min(ref) <= med["(a) mask 0"] <= max(ref)
    print("MI355X  (a) mask 0 through the new entry: median %.2f ms against %.2f ms of the cell-parts call, whose passes ran %.2f .. %.2f ms: %s its spread; the same streams: %s" %
          (med["(a) mask 0"], med["cell parts"], min(ref), max(ref), "inside" if inside else "OUTSIDE", streams_of["(a) mask 0"] == streams_of["cell parts"]), flush=True)
    # what the zeroing and the two passes move: per masked stream of nc components the sums (8 n nc zeroed; read and written at m nc),
    # the sorted keys, rows and row entries of every input row and its integers (n (8 + 4 + 4 + 4 nc)), per kept point the kept row
    # and the stored integers; per cloud the counts (4 n zeroed, read at m per masked stream)
    moved = sum(8 * n * nc + n * (16 + 4 * nc) + m * (8 * nc + 4 + 4 + 4 * nc) for nc in (4, 1)) + 4 * n
    extra = med["(b) means"] - med["cell parts"]
    # (the call as a whole can come out faster with the means than without: averaged attributes code to fewer bytes, and the entropy
    # coders behind the gather run for as long as their corrections are large; --laps times the two passes themselves)
    print("MI355X  (b) both attributes masked: %.2f ms, %+.2f ms against the cell-parts call, %d bytes against %d; the zeroing and the two passes move %.1f MB (their own time: --laps)" %
          (med["(b) means"], extra, size["(b) means"], size["cell parts"], moved / 1e6), flush=True)
    print("MI355X  (c) the route through the host: %.2f ms, %.2f x the call with the means" % (med["(c) host"], med["(c) host"] / med["(b) means"]), flush=True)
    ctx.close()


def laps(millions, rounds):
    ctx = dsa.Context(0)
    enc = dsa.DracoEncoder(ctx)
    pos = scan(int(millions * (1 << 20)), 4, 47)
    n = len(pos)
    rng = np.random.default_rng(48)
    colour, scalar = rng.integers(0, 256, (n, 4)).astype(np.uint8), rng.normal(size=(n, 1)).astype(np.float32)
    cloud = [dsa.PointCloudData(pos, attributes=[dsa.Attribute(colour, attribute_type=2), dsa.Attribute(scalar, quantization_bits=16)])]
    got = enc.EncodeBatch(cloud, config())
    N = -(-len(got.entry_rows(0)[0]) // PARTS)
    got.close()
    for r in range(rounds + 1):
        for leg, cfg in (("cell parts", config(part_cells=N)), ("(b) means", config(part_cells=N, mean_attributes=MASK))):
            print("---- pass %d  %s" % (r, leg), file=sys.stderr, flush=True)
            enc.EncodeBatch(cloud, cfg).close()
    ctx.close()


args = [a for a in sys.argv[1:] if not a.startswith("--")]
if "--laps" in sys.argv[1:]:
    os.environ["DSA_ENC_TIMING"] = "1"
    laps(float(args[0]) if len(args) > 0 else 4.0, int(args[1]) if len(args) > 1 else 3)
    sys.exit(0)
main(float(args[0]) if len(args) > 0 else 4.0, int(args[1]) if len(args) > 1 else 7, int(args[2]) if len(args) > 2 else 4)
