"""The prediction arithmetic on designed geometry, without a GPU: tests/predictcases.py's Python-integer reference of the encoder's
side of every prediction scheme against the symbols the oracle decoded from the CPU coder's streams, the oracle's integers against
the numpy pin of the quantised INPUT (a reader and a writer that agree on a wrong value still fail), and the conditions the designs
have to meet -- checked with the reference alone, so that the GPU tests of the same designs are known to walk the paths they are
written for (tests/test_gpu_predict_designs.py, tests/test_gpu_encode_predict_designs.py)."""
import collections
import math

import numpy as np
import pytest

import oracle
import predictcases as P
from meshutil import face_multiset_fast

# every branch the designs have to reach, at least 8 times over all designs and option sets
REACHED = [
    "tc:geometric", "tc:pn_norm2<2^32", "tc:pn_norm2>=2^32", "tc:root-argument-wraps", "tc:|sx|>=4e15", "tc:foot-dividend<2^52",
    "tc:foot-dividend>=2^52", "tc:foot-negative-with-remainder", "tc:negative-dividend-with-remainder", "tc:exact-division", "tc:equal-uv",
    "tc:pn_norm2==0", "tc:fallback-next", "tc:fallback-entry-before", "tc:fallback-zero", "tc:orientation-0", "tc:orientation-1",
    "tc:operand-1-back", "tc:operand-2..7-back", "tc:operand-8..11-back", "tc:operand-12-or-more-back", "tc:quotient-beyond-31-bits",
    "gn:small", "gn:scaled", "gn:s3==0", "gn:left-half", "gn:fold-s-0", "gn:fold-t-0", "gn:flipped", "gn:not-flipped", "gn:open-fan",
    "gn:closed-fan", "gn:negative-dividend-with-remainder",
    "oct:prediction-outside-diamond", "oct:rotation-1", "oct:rotation-2", "oct:rotation-3",
    "wrap:clamp-above", "wrap:clamp-below", "wrap:correction-wraps-up", "wrap:correction-wraps-down", "para:parallelogram", "para:difference",
]
# branches one design owns: (branch, design, entries in its stock stream at the least)
OWNED = [
    ("tc:quotient-beyond-31-bits", "needle-20b", 8),
    ("gn:fold-s-0", "fold-exact-n4b", 5), ("gn:fold-s-0", "fold-exact-n8b", 5), ("gn:fold-s-0", "fold-exact-n10b", 5), ("gn:fold-s-0", "fold-exact-n14b", 5),
    ("gn:s3==0", "collinear-18b", 49), ("gn:s3==0", "collapsed-14b", 25),
    ("tc:pn_norm2==0", "collapsed-14b", 8),
    ("gn:fold-t-0", "box-fold-zx-n4b", 8), ("gn:fold-t-0", "box-fold-zx-n14b", 8),
    ("wrap:clamp-above", "wall-hugger-20b", 8), ("wrap:clamp-below", "wall-hugger-20b", 8),
]
# what the reference counts but no coder-written stream of 1 - 20 bits reaches (see test_the_designs_reach_every_branch)
NEVER = ["gn:corner", "gn:fold-s-max", "gn:fold-t-max", "gn:sum-wraps-2^63", "gn:scale-dividend>=2^52", "tc:sum-wraps-2^63"]

CASES = [(d, o) for d in P.DESIGNS for o in P.OPTION_SETS]

_references = {}


def reference_of(d, o):
    if (d.name, o) not in _references:
        _references[(d.name, o)] = P.reference(P.decoded(d, o))
    return _references[(d.name, o)]


def test_the_designs_are_what_the_issue_lists():
    names = [d.name for d in P.DESIGNS]
    assert len(set(names)) == len(names)
    for n in (7, 13):
        assert [d.bits[:2] for d in P.DESIGNS if d.name.startswith("rough-n%d-" % n) and d.seams is None] == [(b, b) for b in (8, 14, 17, 18, 19, 20)]
    assert sorted(len(P.design("strip-%d-18b" % n).pos) for n in P.STRIP_ENTRIES) == [3, 4, 5, 12, 13, 24, 25, 80]
    assert len(P.design("strip-3-18b").faces) == 1
    assert sorted({d.bits[2] for d in P.DESIGNS if d.name.startswith("box-fold") and d.seams is None}) == [4, 8, 10, 14]
    assert len(P.SEAMED) == 4 and all(3 <= len(d.pos) <= 169 for d in P.DESIGNS)
    assert all(1 <= b <= 20 for d in P.DESIGNS for b in d.bits)
    assert {(d.name.rsplit("-", 1)[0], d.bits[0]) for d in P.MULTI_DESIGNS} >= {(n, b) for n in ("rough-n7", "rough-n13", "wall-hugger") for b in (8, 14, 20)} | {("lattice", 8), ("lattice", 20)}


@pytest.mark.parametrize("d,o", CASES, ids=["%s-%s" % (d.name, o) for d, o in CASES])
def test_reference_symbols_equal_the_oracles(d, o):
    """Every entry of every attribute, and the decoded integers against the quantised input."""
    ref = P.decoded(d, o)
    r = reference_of(d, o)
    methods = {"stock": (1, 6, 5), "stock-valence": (1, 6, 5), "default": (1, 0, 1), "difference": (0, 0, 0)}[o]
    assert tuple(a.pred_method for a in ref.attributes) == methods and sorted(r.symbols) == [0, 1, 2]
    assert (ref.attributes[0].q_bits, ref.attributes[2].q_bits, ref.attributes[1].oct_bits) == d.bits
    for a, want in r.symbols.items():
        got = ref.attributes[a].symbols.astype(np.int64)
        wrong = np.argwhere(got != want)
        assert len(wrong) == 0, (d.name, o, a, len(wrong), wrong[:4].tolist(), got[wrong[0][0]].tolist(), want[wrong[0][0]].tolist())
    ident = np.arange(ref.num_points, dtype=np.uint32)
    keys = np.concatenate([np.asarray(a.portable, np.int64)[a.point_map if len(a.point_map) else ident] for a in ref.attributes], axis=1)
    got, want = face_multiset_fast(ref.faces, keys), P.pin(d)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_the_designs_reach_every_branch():
    """Conditions on the INPUTS, from the reference's counters alone.  Every branch of REACHED at least 8 times over all designs; the
    branches of OWNED in the design that is there for them; every rough design of 17 - 19 bits (and the hole, the two components and
    the seamed one at 18) at least 5 geometric entries on either side of pn_norm2 = 2^32.

    Not reachable from a stream a coder of 1 - 20 bits writes, and counted as 0 here (NEVER):
      the octahedron's corners (0,0), (0,max), (max,0) and the folds s == max with t < center, t == max with s < center: on the left
        half (x < 0) s == max needs y >= 0 and z == 0, and a z of 0 is not negative, so t = max - |y| >= center; t == max needs
        y == 0, which is not negative either, so s = max - |z| >= center; on the right half s, t == 0 or max put the other
        coordinate at center.  The folds s == 0 and t == 0 are reached (fold-exact, box-fold-zx);
      a sum beyond 2^63 in TexCoordsPortable: |n_uv d| and |(cn . pn) pn_uv| stay below 3 * 2^60 each at 20 bits, the offset below
        2^52.  (The product under the root does wrap; the reference reduces it.);
      a cross-product sum beyond 2^63 or a dividend beyond 2^52 in GeometricNormal's scaling: a fan of f faces stays below f * 2^41;
      the root's clamp at 2^32 - 1: it needs a wrapped product of at least (2^32 - 1)^2, one 64-bit value in 2^31.
    Reached against the expectation of the issue: a quotient beyond 31 bits (needle-20b: an edge one quantum long, a tip and texture
    coordinates a box away; 40 bits, of which the low 32 are the prediction)."""
    total, stock = collections.Counter(), {}
    for d, o in CASES:
        c = reference_of(d, o).branches
        total += c
        if o == "stock":
            stock[d.name] = c
    print({k: total[k] for k in sorted(total)})
    assert not [k for k in REACHED if total[k] < 8], [(k, total[k]) for k in REACHED if total[k] < 8]
    assert not [k for k in NEVER if total[k]], [(k, total[k]) for k in NEVER if total[k]]
    assert not set(total) - set(REACHED) - set(NEVER), sorted(set(total) - set(REACHED) - set(NEVER))
    for branch, name, least in OWNED:
        assert stock[name][branch] >= least, (branch, name, stock[name][branch])
    mixed = [d.name for d in P.DESIGNS if d.name.startswith("rough-") and d.bits[0] in P.MIXED_BITS] + ["hole-18b", "two-parts-19b"]
    assert len(mixed) == 9
    for name in mixed:
        assert stock[name]["tc:pn_norm2<2^32"] >= 5 and stock[name]["tc:pn_norm2>=2^32"] >= 5, (name, stock[name])
    # 8 - 14 bits stay on the fast side throughout, 20 bits leave it: the two ends the mixed designs lie between
    for name in ("rough-n7-8b", "rough-n13-14b"):
        assert stock[name]["tc:pn_norm2>=2^32"] == 0 and stock[name]["gn:scaled"] == 0
    assert stock["rough-n7-20b"]["gn:small"] == 0 and stock["rough-n7-20b"]["tc:root-argument-wraps"] >= 40
    # orientation bits in three words, strips around the chain's groups of 12
    assert stock["strip-80-18b"]["tc:geometric"] > 64
    assert [stock["strip-%d-18b" % n]["tc:geometric"] for n in (3, 4, 5, 12, 13, 24, 25)] == [1, 2, 3, 10, 11, 22, 23]
    # boundary fans beside closed ones, seams that end the fans
    for name in ("hole-18b", "two-parts-19b"):
        assert stock[name]["gn:open-fan"] >= 8 and stock[name]["gn:closed-fan"] >= 8, (name, stock[name])
    for name in ("rough-n7-seamed-18b", "rough-n7-seamed-20b"):         # 24 boundary vertices; every further open fan ends at a seam
        assert stock[name]["gn:open-fan"] >= 24 + 8 and stock[name]["gn:open-fan"] + stock[name]["gn:closed-fan"] > 49, (name, stock[name])


def test_multi_parallelogram_designs_average_negative_sums():
    """ConstrainedMultiParallelogram has no reference here (its crease flags are the coder's choice); its designs have to hold entries
    whose summed parallelograms are negative and leave a remainder by 2, 3 and 4 -- where truncation toward zero and a floor differ."""
    total = collections.Counter()
    for d in P.MULTI_DESIGNS:
        ref = P.decoded(d, "multi")
        assert (ref.attributes[0].pred_method, ref.attributes[2].pred_method) == (4, 4)
        total += P.multi_parallelogram_branches(ref)
    print(dict(total))
    for k in (2, 3, 4):
        assert total["mp:negative-sum-with-remainder-by-%d" % k] >= 8, dict(total)


def square_neighbours():
    out = [0, 1, (1 << 64) - 1]
    for centre in (1 << 16, 1 << 26, (1 << 32) - 1):
        for k in range(centre - 2, centre + 3):
            if k < 1 << 32:
                out += [k * k - 1, k * k, k * k + 1]
    return [v for v in out if 0 <= v < 1 << 64]


def test_oracle_int_sqrt_is_the_floor_root():
    L = oracle.lib()
    roots = [v for d, o in CASES if o.startswith("stock") for v in reference_of(d, o).roots]
    assert len(roots) > 2000 and sum(v >= 1 << 63 for v in roots) > 50
    for v in square_neighbours() + roots:
        assert L.orc_int_sqrt(v) == math.isqrt(v), v
