"""The host side of the pruned decode schedule, without a GPU: the needs walk of draco-sharp_amd/csrc/dsa_host_parse.h (which
kernel groups of dsa_batch_decode have work for a stream), the need bits of dsa_needs.h and the "needs covered by launched"
function k_seal refuses meshes by -- compiled from the library's own headers into a stand-alone program
(tests/hostcheck/needs_host.cpp) under ASan / UBSan.  The library itself needs a GPU to make a batch, so the walk is reached
through the program."""
import subprocess

import pytest

import prunecases as pc

B = pc.need_bits()
ALL = B["ALL"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    # always built from the sources of this checkout
    out = str(tmp_path_factory.mktemp("hostcheck") / "needs_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", out, pc.NEEDS_HOST_SRC], check=True)
    return out


def masks(exe, tmp_path, data):
    """(status, walk_ok, mask without OS_FLAG, mask with OS_FLAG, offsets) of one stream."""
    f = tmp_path / "s.drc"
    f.write_bytes(data)
    r = subprocess.run([exe, "mask", str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    w = r.stdout.split()
    return int(w[0]), int(w[1]), int(w[2], 16), int(w[3], 16), w[4:]


def test_need_bits_are_disjoint_and_all_covers_them():
    single = [B["TAGS"], B["GEOMETRIC"], B["TEXCOORDS"], B["PREDICT_EARLY"], B["PREDICT_LATE"], B["WRAP_EARLY"], B["FINALIZE_LATE"]]
    fields = [pc.group(n, g) for g in ("early", "late", "corner") for n in ("TIER0", "TIER1", "TIER2", "WIDE")]
    bits = single + fields
    assert all(b and b & (b - 1) == 0 for b in bits) and len(set(bits)) == len(bits)
    assert sum(bits) == ALL


def test_the_bench_dialect_needs_no_pruned_kernel(exe, tmp_path):
    """Raw 12-bit streams that k_symbols_reg takes, wrap prediction fused with the dequantisation: of the prunable groups only the
    early k_predict has work (the octahedral delta of the normals), and none once that goes to k_predict_oct_streams."""
    for seed in (1, 2):
        st, ok, plain, crowded, _ = masks(exe, tmp_path, pc.bench(seed))
        assert (st, ok) == (0, 1)
        assert plain == B["PREDICT_EARLY"] and crowded == 0


def test_small_meshes_fall_into_the_tiers(exe, tmp_path):
    """8 x 8 cells: 81 vertices, no room for the tables of k_symbols_reg in any output region (the out_cap rule)."""
    st, ok, plain, crowded, _ = masks(exe, tmp_path, pc.grid(8, 8, 5, (("force_scheme", 1),)))
    assert (st, ok) == (0, 1)
    assert plain & pc.tiers("early") and plain & pc.tiers("late") and not plain & pc.tiers("corner")
    assert not plain & (B["TAGS"] | B["GEOMETRIC"] | B["TEXCOORDS"])
    assert crowded & pc.tiers("early") and crowded & pc.tiers("late")
    # the encoder's own choice for so small a mesh is the tagged scheme: the host sees no further
    st, ok, plain, crowded, _ = masks(exe, tmp_path, pc.grid(8, 8, 5))
    assert (st, ok, plain, crowded) == (0, 0, ALL, ALL)


def test_dialects_ask_for_their_kernels(exe, tmp_path):
    cases = {
        "tagged": (pc.grid(80, 80, 6, (("force_scheme", 0),)), ALL),
        "14-bit positions": (pc.grid(80, 80, 7, (("pos_bits", 14),)), B["PREDICT_EARLY"] | pc.group("WIDE", "late")),
        "GeometricNormal + TexCoordsPortable": (pc.grid(80, 80, 8, pc.STOCK), B["GEOMETRIC"] | B["TEXCOORDS"] | B["FINALIZE_LATE"]),
        "difference": (pc.grid(80, 80, 9, (("pos_prediction", 0), ("uv_prediction", 0))), B["PREDICT_EARLY"] | B["WRAP_EARLY"]),
        "corner attribute": (pc.seamed(), ALL),
        "sequential mesh": (pc.sequential(), ALL),
        "point cloud": (pc.point_cloud(), ALL),
    }
    for name, (data, want) in cases.items():
        st, ok, plain, crowded, _ = masks(exe, tmp_path, data)
        assert st == 0, name
        assert plain == want, (name, hex(plain), hex(want))
        assert crowded in (want, want & ~B["PREDICT_EARLY"]), (name, hex(crowded))


def test_golden_streams_walk_clean(exe, tmp_path):
    for name, data in pc.golden_streams():
        st, ok, plain, crowded, _ = masks(exe, tmp_path, data)
        assert st == 0, name
        assert ok == 1 or (plain == ALL and crowded == ALL), name
        print("%-40s walk %d  0x%05x  0x%05x" % (name, ok, plain, crowded))


def test_needs_covered_on_a_table_of_masks(exe):
    t, g, p = B["TAGS"], B["GEOMETRIC"], B["PREDICT_EARLY"]
    e0, l2 = pc.group("TIER0", "early"), pc.group("TIER2", "late")
    table = [(0, 0, 1), (0, ALL, 1), (ALL, ALL, 1), (ALL, 0, 0), (t, 0, 0), (t, t, 1), (t, ALL & ~t, 0), (g | p, g, 0), (g | p, g | p, 1),
             (e0, l2, 0), (e0, pc.group("TIER0", "late"), 0), (e0 | l2, e0 | l2 | t, 1), (p, ALL & ~p, 0), (ALL & ~p, ALL & ~p, 1),
             (B["FINALIZE_LATE"], ALL >> 1, 0)]
    args = [str(x) for n, l, _ in table for x in (n, l)]
    r = subprocess.run([exe, "cover"] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [int(x) for x in r.stdout.split()] == [c for _, _, c in table]


@pytest.mark.parametrize("which", ["bench", "stock", "wide", "house_04", "level9"])
def test_the_walk_reads_no_byte_outside_a_corrupt_stream(exe, tmp_path, which):
    """Every truncation of the stream and one flipped bit per byte, each copy in a heap block of exactly its length, under ASan /
    UBSan: the walk must end inside the block, and a parse that failed must ask for every kernel."""
    gold = dict(pc.golden_streams())
    data = {"bench": lambda: pc.bench(1), "stock": lambda: pc.grid(80, 80, 8, pc.STOCK), "wide": lambda: pc.grid(80, 80, 7, (("pos_bits", 14),)),
            "house_04": lambda: gold["house_04"],
            "level9": lambda: pc.grid(24, 20, 3, (("pos_prediction", 4), ("normal_prediction", 6), ("uv_prediction", 5), ("predictive_connectivity", 2)))}[which]()
    f = tmp_path / "s.drc"
    f.write_bytes(data)
    r = subprocess.run([exe, "corrupt", str(f), "7"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    print(which, r.stdout.strip())
