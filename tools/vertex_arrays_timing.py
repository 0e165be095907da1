"""Host bytes -> host arrays on the bench batch, four ways to take the results, in one process on one GPU:
full download, compact download, vertex arrays as values, vertex arrays quantised (dsa_batch_vertex_arrays).  Warm, `--in-flight`
batches queued at a time as the end_to_end leg of bench.py runs them (upload k+1 beside kernels k beside download k-1); the forms
take turns inside every pass, so that a drift of the box lands on all of them.  Also the device time of k_pack_output and
k_vertex_arrays from their event pairs (profiling on, a batch of its own each).  Prints one JSON line; no test asserts a time.

    python tools/vertex_arrays_timing.py [--meshes 4096] [--grid 128 256] [--batches 6] [--passes 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import draco_sharp_amd as dsa                # noqa: E402
import draco_sharp_amd.synth as synth        # noqa: E402

FORMS = ("full", "compact", "vertex_values", "vertex_quantized")


def queue(b, form):
    if form == "full":
        b.download(wait=False, compact=False)
    elif form == "compact":
        b.download(wait=False, compact=True)
    else:
        b.vertex_arrays("values" if form == "vertex_values" else "quantized", wait=False)


def host_bytes(b, form):
    return {"full": lambda: b.output_bytes, "compact": lambda: b.compact_bytes, "vertex_values": lambda: b.vertex_arrays_bytes("values"),
            "vertex_quantized": lambda: b.vertex_arrays_bytes("quantized")}[form]()


def touch(b, form, n):
    """Reads one element at either end of the host copy: the arrays are on the host."""
    if form in ("full", "compact"):
        v0, v1 = b.host_views(0), b.host_views(n - 1)
        return int(v0["faces"][0, 0]) + int(v1["faces"][-1, -1]) + int(v1["attributes"][-1]["values"][-1, -1] != 0)
    v0, v1 = b.vertex_views(0), b.vertex_views(n - 1)
    return int(v0["indices"][0, 0]) + int(v1["indices"][-1, -1]) + int(v1["attributes"][-1]["values"][-1, -1] != 0)


def one_pass(ctx, blob, offsets, form, batches, in_flight):
    n = len(offsets) - 1
    live, tags = [], 0

    def finish(b):
        b.wait()
        t = touch(b, form, n)
        b.close()
        return t

    t0 = time.perf_counter()
    for _ in range(batches):
        b = dsa.Batch(ctx, blob=blob, offsets=offsets)
        b.decode(wait=False)
        queue(b, form)
        live.append(b)
        if len(live) == in_flight:
            tags += finish(live.pop(0))
    while live:
        tags += finish(live.pop(0))
    return time.perf_counter() - t0


def kernel_times(ctx, blob, offsets):
    """k_pack_output and k_vertex_arrays alone behind a finished decode: their event pairs on the download stream."""
    out = {}
    ctx.set_profiling(True)
    try:
        for form in ("compact", "vertex_values", "vertex_quantized"):
            b = dsa.Batch(ctx, blob=blob, offsets=offsets)
            best = None
            for _ in range(3):
                b.decode(wait=True)               # the kernel then has the device to itself
                queue(b, form)
                b.wait()
                kt = b.kernel_times()
                ms = kt.get("k_pack_output" if form == "compact" else "k_vertex_arrays")
                best = ms if best is None else min(best, ms)
            out["k_pack_output" if form == "compact" else "k_vertex_arrays[%s]" % form[7:]] = best
            b.close()
    finally:
        ctx.set_profiling(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=4096)
    ap.add_argument("--grid", type=int, nargs=2, default=[128, 256])
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--in-flight", type=int, default=2)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16")))
    args = ap.parse_args()
    nx, ny = args.grid
    blob, offsets = synth.make_batch(synth.GRID, nx, ny, 1000, args.meshes, normals=True, uvs=True, threads=args.threads)
    ctx = dsa.Context(0)
    n = args.meshes
    b = dsa.Batch(ctx, blob=blob, offsets=offsets)
    sizes = {form: host_bytes(b, form) for form in FORMS}
    b.close()
    for form in FORMS:                         # warm-up: arenas, blocks, pinned mirrors of every form into the context's caches
        one_pass(ctx, blob, offsets, form, args.in_flight + 1, args.in_flight)
    seconds = {form: [] for form in FORMS}
    for _ in range(args.passes):
        for form in FORMS:
            seconds[form].append(one_pass(ctx, blob, offsets, form, args.batches, args.in_flight))
    kt = kernel_times(ctx, blob, offsets)
    ctx.close()
    out = {"meshes_per_batch": n, "triangles_per_mesh": 2 * nx * ny, "batches_per_pass": args.batches, "in_flight": args.in_flight, "passes": args.passes,
           "forms": {form: {"meshes_per_s": args.batches * n / min(seconds[form]), "meshes_per_s_median": args.batches * n / sorted(seconds[form])[len(seconds[form]) // 2],
                            "seconds_passes": [round(s, 4) for s in seconds[form]], "host_bytes_per_batch": sizes[form], "host_bytes_per_mesh": sizes[form] / n,
                            "gb_per_s_out": args.batches * sizes[form] / min(seconds[form]) / 1e9} for form in FORMS},
           "kernels_ms": kt}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
