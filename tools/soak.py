"""Randomised differential run: N synthetic meshes with random encoder options (topology, size, bit depths, symbol
scheme, prediction schemes, attribute order, Edgebreaker symbol coding, single / per-attribute connectivity, element type and value
pattern of the generic attribute) decoded in one batch and compared with the oracle; integer attributes also with their input
(tools/typedvalues.py: the pin).  usage: python tools/soak.py [count] [seed]"""
import sys
import os; ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import oracle
import draco_sharp_amd as dsa, draco_sharp_amd.synth as synth


def typed_generic(typ, opt, points, gc):
    """The generic attribute of a case from the generator of the typed draw: element type (int8 ... uint32) and value pattern of
    tools/typedvalues.py, within what the case's other options can carry -- uncompressed integers of 1 / 2 bytes take types no wider
    than that, the raw symbol scheme takes 32-bit values only where their corrections stay below 2^18."""
    import typedvalues
    raw = opt.get("raw_integers", 0)
    dtypes = [d for d in typedvalues.DTYPES if raw not in (1, 2) or d.itemsize <= raw]
    dtype = dtypes[int(typ.integers(0, len(dtypes)))]
    patterns = [p for p in typedvalues.PATTERNS if not (dtype.itemsize == 4 and opt["force_scheme"] == 1 and p in ("random", "extremes"))]
    if raw in (1, 2) and dtype.itemsize == raw:
        patterns = ["ramp", "sentinel"] if raw == 2 else ["random"]          # (an 8-bit wrap keeps every correction within a byte)
    pattern = patterns[int(typ.integers(0, len(patterns)))]
    return typedvalues.values(dtype, pattern, points, gc, seed=int(typ.integers(0, 1 << 30)))


def random_case(rng, irr=None, typ=None):
    """irr: the generator of the irregular draw (tests/irregular.py: roughen), apart from `rng` so that the options of a seed stay
    what they were; None: grids only.  typ: the generator of the typed draw (element type and pattern of the generic attribute),
    apart from both for the same reason; None: uint8 noise.  Returns (stream, description, pin input or None)."""
    kind = int(rng.choice([synth.GRID, synth.TORUS, synth.SPHERE, synth.HOLES, synth.TWO_PARTS]))
    nx, ny = int(rng.integers(4, 48)), int(rng.integers(4, 40))
    if kind == synth.HOLES:
        nx, ny = max(nx, 12), max(ny, 12)
    opt = dict(pos_bits=int(rng.integers(4, 21)), uv_bits=int(rng.integers(4, 17)), normal_bits=int(rng.integers(3, 15)),
               single_connectivity=int(rng.integers(0, 2)), force_scheme=int(rng.integers(-1, 2)),
               compression_level=int(rng.integers(0, 11)), pos_prediction=int(rng.choice([0, 1, 2, 4])),
               uv_prediction=int(rng.choice([0, 1, 2, 4, 5])), normal_prediction=int(rng.choice([0, 6])),
               traversal_method=int(rng.integers(0, 3)), predictive_connectivity=int(rng.integers(0, 3)))
    # decoder branches no stock setting reaches (one case in three): the non-canonicalised octahedral transform, uncompressed
    # integers (the width must hold the zig-zagged corrections), prediction method -2
    if rng.integers(0, 3) == 0:
        opt["normal_transform"] = int(rng.choice([2, 3]))
        opt["no_prediction"] = int(rng.integers(0, 8))
        raw = int(rng.choice([0, 1, 2, 4]))
        if raw == 1:
            opt.update(pos_bits=min(opt["pos_bits"], 6), uv_bits=min(opt["uv_bits"], 6), normal_bits=min(opt["normal_bits"], 6))
        elif raw == 2:
            opt.update(pos_bits=min(opt["pos_bits"], 14), uv_bits=min(opt["uv_bits"], 14))
        opt["raw_integers"] = raw
    mesh_seed = int(rng.integers(0, 1 << 30))
    pos, nrm, uv, faces = synth.make_mesh(kind, nx, ny, mesh_seed)
    grid_vertices = len(pos)
    # one case in three on irregular connectivity: flips, 1->3 splits, a shuffle of ids and faces, sometimes a thickened surface
    rough = irr is not None and irr.integers(0, 3) == 0
    if rough:
        import irregular
        pos, nrm, uv, faces = irregular.roughen(pos, nrm, uv, faces, irr)
    with_n, with_uv = bool(rng.integers(0, 4)), bool(rng.integers(0, 4))
    # one case in three gives its attributes per corner (attribute seams, corner attributes); they need a connectivity of their own
    if rng.integers(0, 3) == 0 and (with_n or with_uv):
        import irregular
        patterns = ["stripes", "island", "checker", "random", "single", "none", None]
        charts = (str(rng.choice(patterns[:6])) if with_n and rng.integers(0, 2) else None, str(rng.choice(patterns[:6])) if with_uv and rng.integers(0, 2) else None)
        opt["single_connectivity"] = 0
        # half of these stay on the wave-per-mesh kernels whatever else was drawn (depth-first order, no predictive symbols), and a
        # third of those put tagged symbols into the corner attributes: the walk of the stream then stops in front of them and what
        # follows is located behind the seam tables
        if rng.integers(0, 2):
            opt.update(traversal_method=0, predictive_connectivity=int(rng.choice([0, 2])), pos_prediction=int(rng.choice([0, 1, 4])), uv_prediction=int(rng.choice([0, 1, 5])))
            if rng.integers(0, 3) == 0 and not opt.get("raw_integers"):
                opt["force_scheme"] = 0
        pos, faces, nrm, nid, uv, uid = irregular.with_seams(pos, nrm, uv, faces, *charts, seed=mesh_seed)       # (meshutil.seamed_mesh on a grid)
        return synth.encode_mesh_corners(pos, faces, nrm if with_n else None, nid if with_n else None, uv if with_uv else None, uid if with_uv else None,
                                         opt=synth.options(**opt)), (kind, nx, ny, opt, with_n, with_uv, charts, rough), None
    # one per-vertex case in four carries a generic attribute of 1 - 4 components (vertex colours, joint indices, feature ids)
    gen = None
    if rng.integers(0, 4) == 0:
        gc = int(rng.integers(1, 5))
        opt["generic_components"] = gc
        gen = rng.integers(0, 256, (grid_vertices, gc)).astype(np.uint8)
        if len(pos) != grid_vertices:
            gen = np.concatenate([gen, irr.integers(0, 256, (len(pos) - grid_vertices, gc)).astype(np.uint8)])
        if typ is not None:
            gen = typed_generic(typ, opt, len(pos), gc)
    what = (kind, nx, ny, opt, with_n, with_uv, rough) + ((gen.dtype.name,) if gen is not None else ())
    return (synth.encode_mesh(pos, faces, nrm if with_n else None, uv if with_uv else None, generic=gen, opt=synth.options(**opt)), what,
            None if gen is None else (pos, faces, gen, opt["pos_bits"]))


def run(count, seed, ctx=None):
    rng = np.random.default_rng(seed)
    irr = np.random.default_rng([seed, 0x1226])          # the irregular draw: seeded from the run's seed, apart from the options
    typ = np.random.default_rng([seed, 0x7E9D])           # the typed draw, likewise
    cases = [random_case(rng, irr, typ) for _ in range(count)]
    import typedvalues
    own = ctx is None
    ctx = ctx or dsa.Context(0)
    b = dsa.Batch(ctx, [c[0] for c in cases])
    b.decode()
    bad = []
    for i, (data, what, pin_input) in enumerate(cases):
        try:
            ref = oracle.decode(data)
        except oracle.OracleError as e:          # a stream the reference refuses (its own limits): the device must refuse it too
            if b.status(i) == 0:
                bad.append((i, what, "oracle refuses (%s), device decodes" % e))
            continue
        if b.status(i) != 0:
            bad.append((i, what, "status %d site %d" % (b.status(i), b.mesh_info(i).detail)))
            continue
        m = b.result(i).ConnectedData
        ok = np.array_equal(m.Faces, ref.faces) and len(m.Attributes) == len(ref.attributes)
        for a, r in zip(m.Attributes, ref.attributes):
            ok = ok and np.array_equal(a.PortableValues, r.portable) and np.array_equal(a.PointMap, r.point_map) and a.Values.tobytes() == r.values.tobytes()
        if not ok:
            bad.append((i, what, "differs from the oracle"))
        elif pin_input is not None:              # integer attributes are lossless: the decoded mesh against the input itself
            pos, faces, gen, pos_bits = pin_input
            if m.Attributes[-1].Values.dtype != gen.dtype or not typedvalues.same_multiset(typedvalues.device_multiset(m), typedvalues.pin(pos, faces, gen, pos_bits)):
                bad.append((i, what, "differs from the input"))
    b.close()
    if own:
        ctx.close()
    return bad


if __name__ == "__main__":
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    bad = run(count, seed)
    print("%d cases, %d bad" % (count, len(bad)))
    for x in bad[:10]:
        print(x)
    sys.exit(1 if bad else 0)
