// tests/hostcheck/encsplit_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The encoder's part kernel (draco-sharp_amd/csrc/dsa_encode_order.h: k_enc_part_bounds) compiled for the host with
// AddressSanitizer + UBSan and run thread by thread behind the product's sort, by the product's launch sequence (enc_order_stage),
// in the arena the product's layout hands out for a split chunk (enc_layout_sequential with EncRequest::point_order and part_points:
// stream records, order records, part records, both tile lists and every region are the library's own; encorder_common.h has the
// harness) -- once forwards, once backwards -- against the host coder (dsa_encode_host.h: synth::split_parts, synth::part_boxes) on
// the same points: the same ranges in the part records and in nv / e2v of every part's stream records, the same boxes, the same rows
// in the slice of the sorted buffer every stream of a part reads as its entry -> row map, and not one access outside a region (the
// arena's gaps are poisoned).  The accesses of k_enc_gather are made in its place, in the product's regions, and what lands in d is
// held to the order.  Every cloud carries normals, so that a part has two streams on two sets of shared integers.  The clouds of one
// position_bits and part_points are one chunk.  Nothing here is linked into the product.
//
//   encsplit_host <cases.bin>   file: u32 count, then per case u32 n, bits, has_grid, part_points; f32 pos[3 n]; with a grid f32 origin[3], range
#include "encorder_common.h"

#define FAIL(...) do { fprintf(stderr, "bits %u, part_points %u, %s: ", bits, part_points, backwards ? "backwards" : "forwards"); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

// the cases `which` as one chunk of a request of point clouds
static int run(const std::vector<const In *> &which, uint32_t bits, uint32_t part_points, bool backwards, uint64_t &points, uint64_t &parts_seen) {
  Run R;
  Ask ask;
  ask.bits = bits; ask.part_points = part_points; ask.normals = true;
  if (!R.begin(which, ask)) FAIL("%s", R.why.c_str());
  const EncLayout &L = R.L();
  const EncChunk &ck = *R.ck;
  const uint32_t n = R.n;
  uint8_t *arena = R.arena;
  if (!R.rq.split()) FAIL("the request is not a split one");
  if (!ck.E->split || ck.E->parts.size() != n || ck.parts.size() != n) FAIL("the chunk's handle keeps no parts");
  if (!L.split || L.merge || L.ord_of_mesh.size() != n || L.part_of_mesh.size() != n) FAIL("%zu order records for %u clouds, %u passes", L.ord.size(), n, L.ord_passes);
  if (!R.sized(L.parts_at, sizeof(dsa::EncPart) * L.parts.size()) || !R.sized(L.part_tiles_at, sizeof(dsa::EncPartTile) * L.part_tiles.size())) FAIL("the part records are not among the uploads");
  std::vector<std::vector<uint32_t>> want_perm(n);
  std::vector<std::vector<std::pair<uint32_t, uint32_t>>> want_ranges(n);
  std::vector<std::vector<int32_t>> want_min(n), want_max(n);
  size_t tile_at = 0, part_at = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    const dsa::EncOrder &O = L.ord[i];
    const uint32_t s0 = L.first_stream[i];
    synth::part_boxes(c.pos.data(), c.n, (int)bits, R.grid(i), part_points, want_perm[i], want_ranges[i], want_min[i], want_max[i]);
    const uint32_t np = (uint32_t)want_ranges[i].size();
    if (L.ord_of_mesh[i] != i || O.n != c.n || O.merge != 0 || O.rank != 0 || O.count != 0 || O.cells != 0) FAIL("case %u: order record", i);
    if (ck.num_parts(i) != np || L.part_of_mesh[i] != part_at || L.first_stream[i + 1] != s0 + 2 * np) FAIL("case %u: %u parts laid out, the host coder cuts %u", i, ck.num_parts(i), np);
    if (!R.sized(O.key[0], 8ull * c.n) || !R.sized(O.key[1], 8ull * c.n) || !R.sized(O.row[0], 4ull * c.n) || !R.sized(O.row[1], 4ull * c.n) || !R.sized(O.hist, 4ull * O.tiles))
      FAIL("case %u: order regions too small", i);
    for (uint32_t p = 0; p < np; ++p, ++part_at) {
      const dsa::EncPart &P = L.parts[part_at];
      const uint32_t lo = want_ranges[i][p].first, cnt = want_ranges[i][p].second - lo;
      if (P.cloud != i || P.lo != lo || P.n != cnt || cnt == 0 || cnt > part_points) FAIL("case %u part %u: record says %u + %u, the host coder %u + %u", i, p, P.lo, P.n, lo, cnt);
      for (int k = 0; k < 3; ++k) if (P.qmin[k] != INT32_MAX || P.qmax[k] != INT32_MIN) FAIL("case %u part %u: the box does not start empty", i, p);
      for (uint32_t t = 0; t < (cnt + ORD_TILE - 1) / ORD_TILE; ++t, ++tile_at)
        if (tile_at >= L.part_tiles.size() || L.part_tiles[tile_at].part != part_at || L.part_tiles[tile_at].tile != t) FAIL("case %u part %u: tile %u is not in the list", i, p, t);
      for (uint32_t k = 0; k < 2; ++k) {
        const dsa::EncStream &S = L.streams[s0 + 2 * p + k], &first = L.streams[s0 + k];
        if (S.linear != 0 || S.nv != cnt || S.rows != c.n || S.e2v != dsa::ord_sorted(O).row + 4ull * lo || S.e2v != dsa::ord_part_rows(O) + 4ull * lo || S.vals != first.vals || S.src != first.src || S.part != (p ? 1u : 0u))
          FAIL("case %u part %u: stream %u does not read its slice of the cloud's rows and values", i, p, k);
        if (p && (S.grid_mode != 0 || S.d == first.d || S.syms == first.syms || S.hist_raw == first.hist_raw || S.out_rans == first.out_rans)) FAIL("case %u part %u: stream %u shares a region of the first part's", i, p, k);
        if (S.d == S.vals || !R.sized(S.d, 4ull * S.nc * cnt) || !R.sized(S.syms, 4ull * S.nc * cnt) || !R.sized(S.bl, cnt) || !R.sized(first.vals, 4ull * S.nc * c.n) || S.out_cap < 4u * cnt * S.nc + 16u ||
            !R.sized(S.out_rans, S.out_cap) || !R.sized(S.out_bits, S.out_cap))
          FAIL("case %u part %u: regions of stream %u too small", i, p, k);
      }
    }
    if (O.vals != L.streams[s0].vals) FAIL("case %u: the sort does not read the positions' integers", i);
    R.write_positions(i);
    int32_t *nv = (int32_t *)(arena + L.streams[s0 + 1].vals);       // the normals' two integers per row: the row, told apart per component
    for (uint32_t r = 0; r < c.n; ++r) { nv[2 * r] = (int32_t)r; nv[2 * r + 1] = ~(int32_t)r; }
  }
  if (tile_at != L.part_tiles.size() || part_at != L.parts.size()) FAIL("%zu part tiles and %zu parts laid out, %zu and %zu expected", L.part_tiles.size(), L.parts.size(), tile_at, part_at);
  R.poison();
  if (!R.stage(backwards)) FAIL("%s", R.why.c_str());
  R.gather();
  const dsa::EncOrder *clouds = R.clouds();
  const dsa::EncPart *parts = R.parts();
  part_at = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    const uint32_t s0 = L.first_stream[i];
    const uint32_t *perm = (const uint32_t *)(arena + dsa::ord_sorted(clouds[i]).row);
    for (uint32_t e = 0; e < c.n; ++e) if (perm[e] != want_perm[i][e]) FAIL("case %u (%u points): entry %u carries row %u, the host coder says %u", i, c.n, e, perm[e], want_perm[i][e]);
    const int32_t *q = (const int32_t *)(arena + clouds[i].vals);
    for (uint32_t p = 0; p < want_ranges[i].size(); ++p, ++part_at) {
      const dsa::EncPart &P = parts[part_at], &laid = L.parts[part_at];
      if (P.cloud != laid.cloud || P.lo != laid.lo || P.n != laid.n || P.pad != 0) FAIL("case %u part %u: the record changed beyond its box", i, p);
      for (int k = 0; k < 3; ++k)
        if (P.qmin[k] != want_min[i][3 * p + k] || P.qmax[k] != want_max[i][3 * p + k])
          FAIL("case %u (%u points) part %u component %d: box %d .. %d, the host coder %d .. %d", i, c.n, p, k, P.qmin[k], P.qmax[k], want_min[i][3 * p + k], want_max[i][3 * p + k]);
      const int32_t *dp = (const int32_t *)(arena + L.streams[s0 + 2 * p].d), *dn = (const int32_t *)(arena + L.streams[s0 + 2 * p + 1].d);
      for (uint32_t e = 0; e < P.n; ++e) {
        const uint32_t r = want_perm[i][P.lo + e];
        if (memcmp(dp + 3 * (size_t)e, q + 3 * (size_t)r, 12) != 0 || dn[2 * e] != (int32_t)r || dn[2 * e + 1] != ~(int32_t)r) FAIL("case %u part %u: entry %u does not carry row %u", i, p, e, r);
      }
      ++parts_seen;
    }
    points += c.n;
  }
  R.unpoison();
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: encsplit_host <cases.bin>\n"); return 2; }
  std::vector<In> cases;
  if (!read_cases(argv[1], 4, false, cases)) return 2;
  for (const In &c : cases) if (c.more[0] == 0 || c.more[0] > 0x7FFFFFFFu) return 2;
  uint32_t chunks = 0;
  uint64_t points = 0, parts = 0;
  std::map<std::pair<uint32_t, uint32_t>, std::vector<const In *>> groups;      // (bits, part_points): one request
  for (const In &c : cases) groups[{c.bits, c.more[0]}].push_back(&c);
  for (const auto &g : groups) {
    for (int backwards = 0; backwards < 2; ++backwards) if (run(g.second, g.first.first, g.first.second, backwards != 0, points, parts) != 0) return 1;
    ++chunks;
  }
  printf("encsplit: %u cases in %u chunks cut as the host coder cuts them, forwards and backwards (%llu points, %llu parts)\n", (uint32_t)cases.size(), chunks,
         (unsigned long long)points, (unsigned long long)parts);
  return 0;
}
