"""What putting the parts of a cloud back together costs, with and without dsa_batch_joined_arrays: the height-field scan of
tools/encode_split_timing.py (4 Mi points, with a uint8 x 3 colour) cut into 256 parts (Config(part_points=n / 256)), decoded as one
Batch, and then, every request queued behind the finished decode, wall time per call of
    device:  vertex_arrays(device_only) + one torch.cat per attribute      against  joined_arrays(device_only), stream and input order
    host:    vertex_arrays() + np.concatenate per attribute + the inverse permutation (out[perm] = rows)
                                                                            against  joined_arrays(), stream and input order (one download)
One untimed call of every leg (blocks and mirrors are made once), then `--calls` warm calls each, the legs taking turns; all
times are reported, not a best-of.  Prints one JSON line; no test asserts a time.

    python tools/joined_arrays_timing.py [--millions 4] [--parts 256] [--calls 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch                                 # noqa: E402
import draco_sharp_amd as dsa                # noqa: E402
from draco_sharp_amd import encoder          # noqa: E402
import ordercases                            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--millions", type=float, default=4.0)
    ap.add_argument("--parts", type=int, default=256)
    ap.add_argument("--calls", type=int, default=3)
    args = ap.parse_args()
    torch.cuda.init()
    side = int(np.sqrt(args.millions * (1 << 20)))
    pos = ordercases.height_field(side, side, 43)
    n = len(pos)
    colour = np.random.default_rng(44).integers(0, 256, (n, 3)).astype(np.uint8)
    ctx = dsa.Context(0)
    cloud = dsa.PointCloudData(pos, attributes=[dsa.Attribute(colour, attribute_type=2)])
    h = dsa.DracoEncoder(ctx).EncodeBatch([cloud], dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, part_points=-(-n // args.parts)))
    streams, groups, em = encoder.join_plan(h)
    perm = np.concatenate([h.entry_rows(s)[0] for s in h.parts(0)]).astype(np.int64)
    b = dsa.Batch(ctx, streams)
    b.decode()
    members = range(len(streams))

    def cat_device():
        b.vertex_arrays("values", device_only=True)
        views = [b.device_vertex_views(i) for i in members]
        out = [torch.cat([v["attributes"][a]["values"] for v in views]) for a in range(2)]
        torch.cuda.synchronize()
        return out

    def cat_host():
        b.vertex_arrays("values")
        views = [b.vertex_views(i) for i in members]
        out = []
        for a in range(2):
            rows = np.concatenate([v["attributes"][a]["values"] for v in views])
            back = np.empty_like(rows)
            back[perm] = rows
            out.append(back)
        return out

    legs = {
        "device_vertex_arrays_torch_cat": cat_device,
        "device_joined_stream": lambda: b.joined_arrays(groups, "values", device_only=True),
        "device_joined_input": lambda: b.joined_arrays(groups, "values", order="input", encoded=h, encoded_mesh=em, device_only=True),
        "host_vertex_arrays_concatenate_permute": cat_host,
        "host_joined_stream": lambda: b.joined_arrays(groups, "values"),
        "host_joined_input": lambda: b.joined_arrays(groups, "values", order="input", encoded=h, encoded_mesh=em),
    }
    ms = {k: [] for k in legs}
    for r in range(args.calls + 1):
        for k, f in legs.items():
            t0 = time.perf_counter()
            got = f()
            dt = (time.perf_counter() - t0) * 1e3
            if r:
                ms[k].append(round(dt, 3))
            elif k == "host_joined_input":                      # the join gives back the caller's own colours
                same = bool(np.array_equal(got[0]["attributes"][1]["values"], colour))
    out = {"points": n, "parts": len(streams), "attributes": 2, "joined_bytes": b.joined_arrays_bytes(groups, "values"),
           "vertex_arrays_bytes": b.vertex_arrays_bytes("values"), "input_order_equals_the_input_colours": same, "calls": args.calls,
           "ms": ms, "device": torch.cuda.get_device_name(0)}
    b.close()
    h.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
