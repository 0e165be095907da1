// tests/hostcheck/enclod_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The encoder's level-of-detail steps (draco-sharp_amd/csrc/dsa_encode_order.h: k_enc_lod_levels, k_enc_lod_scan, k_enc_lod_scatter,
// k_enc_lod_cells, and k_enc_part_cells over the level table) compiled for the host with AddressSanitizer + UBSan and run thread by
// thread by the product's launch sequence for a chunk with lod_base_bits >= 1 (enc_order_stage: the sort, the merge, the levels, the
// part sizes, the part boxes) in the arena the product's layout hands out for such a chunk (enc_layout_sequential with
// EncRequest::point_order, merge_points, part_cells and lod_base_bits: stream records, order records, ceil(n / N) + L - 1 part
// slots, both tile lists, the level table and every region are the library's own; encorder_common.h has the harness) -- once
// forwards, once backwards -- against the host coder (dsa_encode_host.h: synth::lod_parts) on the same points: the same lod rows and
// row_entries, the same level table, the same ranges and levels in the slot records and in nv / e2v of every slot's stream records,
// slots behind the last part with n = nv = 0, the same boxes, and not one access outside a region (the arena's gaps are poisoned).
// The regions of a slot that the host coder says stays empty are poisoned as well before the first launch: no kernel touches them.
// The accesses of k_enc_gather are made in its place for every stream record it does not pass by (kind 3, which k_enc_part_cells
// gives the records of an empty slot), in the product's regions, and what lands in d is held to lod.  Every cloud carries normals,
// so that a slot has two streams on two sets of shared integers.  The clouds of one position_bits, part_cells and lod_base_bits are
// one chunk.  Nothing here is linked into the product.
//
//   enclod_host <cases.bin>   file: u32 count, then per case u32 n, bits, has_grid, part_cells, lod_base_bits; f32 pos[3 n]; with a grid f32 origin[3], range
#include "encorder_common.h"

#define FAIL(...) do { fprintf(stderr, "bits %u, part_cells %u, lod_base_bits %u, %s: ", bits, part_cells, lod_bits, backwards ? "backwards" : "forwards"); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

// the cases `which` as one chunk of a request of point clouds
static int run(const std::vector<const In *> &which, uint32_t bits, uint32_t part_cells, uint32_t lod_bits, bool backwards, uint64_t &points, uint64_t &parts_seen, uint64_t &empty_seen) {
  Run R;
  Ask ask;
  ask.bits = bits; ask.merge = true; ask.part_cells = part_cells; ask.lod_base_bits = lod_bits; ask.normals = true;
  if (!R.begin(which, ask)) FAIL("%s", R.why.c_str());
  const EncLayout &L = R.L();
  EncChunk &ck = *R.ck;
  const uint32_t n = R.n, levels = bits - lod_bits + 1;
  uint8_t *arena = R.arena;
  if (!R.rq.lod() || !R.rq.cell_parts() || !R.rq.split() || !R.rq.merged() || R.rq.part_size() != part_cells || R.rq.lod_levels() != levels) FAIL("the request is not one with levels");
  if (!ck.E->split || !ck.E->merged || ck.E->parts.size() != n || ck.E->cells.size() != n || ck.parts.size() != n) FAIL("the chunk's handle keeps no parts and cells");
  if (!L.split || !L.merge || !L.cell_parts || !L.lod || L.ord_of_mesh.size() != n || L.part_of_mesh.size() != n) FAIL("%zu order records for %u clouds, %u passes", L.ord.size(), n, L.ord_passes);
  if (!R.sized(L.parts_at, sizeof(dsa::EncPart) * L.parts.size()) || !R.sized(L.part_tiles_at, sizeof(dsa::EncPartTile) * L.part_tiles.size())) FAIL("the part records are not among the uploads");
  std::vector<std::vector<uint32_t>> want_levels(n);
  std::vector<std::vector<uint32_t>> want_kept(n), want_cells(n);
  std::vector<Run::Ranges> want_ranges(n);
  std::vector<std::vector<int32_t>> want_min(n), want_max(n);
  std::vector<std::pair<uint64_t, uint64_t>> empty_regions;       // of the slots that stay empty: poisoned below
  size_t tile_at = 0, part_at = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    const dsa::EncOrder &O = L.ord[i];
    const uint32_t s0 = L.first_stream[i];
    synth::lod_parts(c.pos.data(), c.n, (int)bits, R.grid(i), part_cells, (int)lod_bits, want_kept[i], want_cells[i], want_ranges[i], want_levels[i], want_min[i], want_max[i]);      // (want_kept: the rows in lod order)
    const uint32_t slots = (uint32_t)(((uint64_t)c.n + part_cells - 1) / part_cells) + levels - 1u, cap = std::min(part_cells, c.n);
    if (L.ord_of_mesh[i] != i || O.n != c.n || O.merge != 1 || O.rank != 0 || O.count != 0 || O.cells == 0 || O.stream0 != s0 || O.streams != 2 || O.lod_bits != lod_bits ||
        O.lod_rows != O.key[O.last ^ 1u] || O.lod_rows == dsa::ord_sorted(O).key || dsa::ord_part_rows(O) != O.lod_rows || !R.sized(O.lod_table, sizeof(dsa::EncLodTable)))
      FAIL("case %u: order record", i);
    if (!R.sized(O.key[0], 8ull * c.n) || !R.sized(O.key[1], 8ull * c.n) || !R.sized(O.row[0], 4ull * c.n) || !R.sized(O.row[1], 4ull * c.n) || !R.sized(O.hist, 4ull * levels * O.tiles) || !R.sized(O.cells, 4ull * c.n))
      FAIL("case %u: order regions too small", i);
    if ((uint64_t)slots * cap >= (uint64_t)c.n + (uint64_t)part_cells * levels) FAIL("case %u: %u slots of %u points for %u rows", i, slots, cap, c.n);
    if (!R.slots_laid(i, (uint32_t)want_ranges[i].size(), slots, part_at, tile_at, empty_regions)) FAIL("%s", R.why.c_str());
    if (O.vals != L.streams[s0].vals) FAIL("case %u: the sort does not read the positions' integers", i);
    R.write_positions(i);
    int32_t *nv = (int32_t *)(arena + L.streams[s0 + 1].vals);       // the normals' two integers per row: the row, told apart per component
    for (uint32_t r = 0; r < c.n; ++r) { nv[2 * r] = (int32_t)r; nv[2 * r + 1] = ~(int32_t)r; }
  }
  if (tile_at != L.part_tiles.size() || part_at != L.parts.size()) FAIL("%zu part tiles and %zu slots laid out, %zu and %zu expected", L.part_tiles.size(), L.parts.size(), tile_at, part_at);
  R.poison(empty_regions);
  if (!R.stage(backwards)) FAIL("%s", R.why.c_str());
  R.gather();
  ck.L.streams = R.records;                                   // what the product's host reads: the records that came back
  const dsa::EncOrder *clouds = R.clouds();
  part_at = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    const uint32_t s0 = L.first_stream[i], m = (uint32_t)want_kept[i].size(), live = (uint32_t)want_ranges[i].size();
    if (clouds[i].m != m) FAIL("case %u (%u points): %u cells, the host coder says %u", i, c.n, clouds[i].m, m);
    const uint32_t *kept = (const uint32_t *)(arena + clouds[i].lod_rows), *cells = (const uint32_t *)(arena + clouds[i].cells);
    for (uint32_t e = 0; e < m; ++e) if (kept[e] != want_kept[i][e]) FAIL("case %u (%u points): lod entry %u is row %u, the host coder says %u", i, c.n, e, kept[e], want_kept[i][e]);
    for (uint32_t r = 0; r < c.n; ++r) if (cells[r] != want_cells[i][r]) FAIL("case %u (%u points): row %u lies in cell %u, the host coder says %u", i, c.n, r, cells[r], want_cells[i][r]);
    const int32_t *q = (const int32_t *)(arena + clouds[i].vals);
    // the level table: points and first lod entry of every level, zero from L on
    const dsa::EncLodTable &table = *(const dsa::EncLodTable *)(arena + clouds[i].lod_table);
    std::vector<uint32_t> level_points(ORD_LOD_LEVELS, 0);
    for (uint32_t p = 0; p < live; ++p) level_points[want_levels[i][p]] += want_ranges[i][p].second - want_ranges[i][p].first;
    for (uint32_t l = 0, at = 0; l < ORD_LOD_LEVELS; at += level_points[l], ++l)
      if (table.count[l] != level_points[l] || table.base[l] != (l < levels ? at : 0u)) FAIL("case %u level %u: the table says %u points from %u, the host coder %u from %u", i, l, table.count[l], table.base[l], level_points[l], at);
    // the live parts and their points as the product's host counts them
    uint32_t back_points = 0;
    if (ck.live_parts(i, &back_points) != live || back_points != m) FAIL("case %u: %u parts of %u points came back, %u of %u expected", i, ck.live_parts(i), back_points, live, m);
    auto entry = [&](uint32_t p, uint32_t e, uint32_t r) {
      const int32_t *dp = (const int32_t *)(arena + R.laid[s0 + 2 * p].d), *dn = (const int32_t *)(arena + R.laid[s0 + 2 * p + 1].d);
      return memcmp(dp + 3 * (size_t)e, q + 3 * (size_t)r, 12) == 0 && dn[2 * e] == (int32_t)r && dn[2 * e + 1] == ~(int32_t)r;
    };
    if (!R.slots_sized(i, want_ranges[i], &want_levels[i], want_kept[i], want_min[i], want_max[i], part_at, parts_seen, empty_seen, entry)) FAIL("%s", R.why.c_str());
    points += c.n;
  }
  R.unpoison();
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: enclod_host <cases.bin>\n"); return 2; }
  std::vector<In> cases;
  if (!read_cases(argv[1], 5, false, cases)) return 2;
  for (const In &c : cases) if (c.more[0] == 0 || c.more[0] > 0x7FFFFFFFu || c.more[1] < 1 || c.more[1] > c.bits) return 2;
  uint32_t chunks = 0;
  uint64_t points = 0, parts = 0, empty = 0;
  std::map<std::pair<std::pair<uint32_t, uint32_t>, uint32_t>, std::vector<const In *>> groups;      // (bits, part_cells, lod_base_bits): one request
  for (const In &c : cases) groups[{{c.bits, c.more[0]}, c.more[1]}].push_back(&c);
  for (const auto &g : groups) {
    for (int backwards = 0; backwards < 2; ++backwards) if (run(g.second, g.first.first.first, g.first.first.second, g.first.second, backwards != 0, points, parts, empty) != 0) return 1;
    ++chunks;
  }
  printf("enclod: %u cases in %u chunks cut as the host coder cuts them, forwards and backwards (%llu points, %llu parts, %llu empty slots untouched)\n", (uint32_t)cases.size(), chunks,
         (unsigned long long)points, (unsigned long long)parts, (unsigned long long)empty);
  return 0;
}
