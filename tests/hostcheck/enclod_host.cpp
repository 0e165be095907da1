// tests/hostcheck/enclod_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The encoder's level-of-detail steps (draco-sharp_amd/csrc/dsa_encode_order.h: k_enc_lod_levels, k_enc_lod_scan, k_enc_lod_scatter,
// k_enc_lod_cells, k_enc_lod_parts) compiled for the host with AddressSanitizer + UBSan and run thread by thread in the product's
// launch sequence for a chunk with lod_base_bits >= 1 -- the sort (enc_order_launch), the merge (enc_merge_launch), the levels
// (enc_lod_launch), the part boxes (enc_part_launch) -- in the arena the product's layout hands out for such a chunk
// (enc_layout_sequential with EncRequest::point_order, merge_points, part_cells and lod_base_bits: stream records, order records,
// ceil(n / N) + L - 1 part slots, both tile lists, the level table and every region are the library's own) -- once forwards, once
// backwards -- against the host coder (dsa_encode_host.h: synth::lod_parts) on the same points: the same lod rows and row_entries,
// the same level table, the same ranges and levels in the slot records and in nv / e2v of every slot's stream records, slots behind
// the last part with n = nv = 0, the same boxes, and not one access outside a region (the arena's gaps are poisoned).
// The regions of a slot that the host coder says stays empty are poisoned as well before the first launch: no kernel touches them.
// k_enc_gather itself lives in dsa_encode.h, which needs HIP: its accesses -- e2v[e], vals[nc e2v[e] + c], d[nc e + c] for e < nv of
// every stream record it does not pass by (kind 3, which k_enc_lod_parts gives the records of an empty slot) -- are made here in its
// place, in the product's regions, and what lands in d is held to lod.  Every cloud carries normals, so that a slot has two streams
// on two sets of shared integers.  The clouds of one position_bits, part_cells and lod_base_bits are one chunk.  Nothing here is
// linked into the product.
//
//   enclod_host <cases.bin>   file: u32 count, then per case u32 n, bits, has_grid, part_cells, lod_base_bits; f32 pos[3 n]; with a grid f32 origin[3], range
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../draco-sharp_amd/csrc/dsa_common.h"
#include "../../draco-sharp_amd/csrc/dsa_types.h"

#include "hip_on_host.h"

#include "../../draco-sharp_amd/csrc/dsa_encode_layout.h"

struct In {
  uint32_t n = 0, bits = 0, has_grid = 0, part_cells = 0, lod_bits = 0;
  std::vector<float> pos;
  float grid[4] = {0, 0, 0, 0};
};

#define FAIL(...) do { fprintf(stderr, "bits %u, part_cells %u, lod_base_bits %u, %s: ", bits, part_cells, lod_bits, backwards ? "backwards" : "forwards"); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

// the cases `which` as one chunk of a request of point clouds
static int run(const std::vector<const In *> &which, uint32_t bits, uint32_t part_cells, uint32_t lod_bits, bool backwards, uint64_t &points, uint64_t &parts_seen, uint64_t &empty_seen) {
  const uint32_t n = (uint32_t)which.size();
  std::vector<dsa_mesh_attr_input> meshes(n);
  std::vector<EncMeshGrids> grids(n);
  memset(meshes.data(), 0, sizeof(dsa_mesh_attr_input) * n);
  bool any_grid = false;
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    dsa_mesh_input &m = meshes[i].mesh.mesh;
    m.num_vertices = c.n; m.positions = c.pos.data(); m.normals = c.pos.data();
    if (c.has_grid) { synth::Grid &g = grids[i].slot[0]; memcpy(g.origin, c.grid, 12); g.range = c.grid[3]; g.mode = 1; any_grid = true; }
  }
  EncRequest rq;
  rq.n = n; rq.meshes = meshes.data(); rq.sequential = true; rq.point_order = true; rq.merge_points = true; rq.part_cells = part_cells; rq.lod_base_bits = lod_bits;
  if (any_grid) rq.grids = grids.data();
  memset(&rq.seq, 0, sizeof(rq.seq));
  synth::Options d;
  dsa_encode_options &o = rq.seq.base;
  o.position_bits = (int32_t)bits; o.texcoord_bits = d.uv_bits; o.normal_bits = d.normal_bits; o.symbol_scheme = d.force_scheme; o.compression_level = d.compression_level;
  rq.seq.geometry = 0; rq.seq.compress_connectivity = 0;
  const uint32_t levels = bits - lod_bits + 1;
  if (!rq.lod() || !rq.cell_parts() || !rq.split() || !rq.merged() || rq.part_size() != part_cells || rq.lod_levels() != levels) FAIL("the request is not one with levels");
  EncChunk ck(rq, 0, n, n);
  if (!ck.E->split || !ck.E->merged || ck.E->parts.size() != n || ck.E->cells.size() != n || ck.parts.size() != n) FAIL("the chunk's handle keeps no parts and cells");
  std::vector<std::pair<uint64_t, uint64_t>> log;
  ck.region_log = &log;
  for (uint32_t i = 0; i < n; ++i) { enc_check_sequential_mesh(ck, i); if (!ck.good(i)) FAIL("case %u refused: %s", i, ck.E->messages[i].c_str()); }
  enc_layout_sequential(ck);
  const EncLayout &L = ck.L;
  if (!L.split || !L.merge || !L.cell_parts || !L.lod || L.ord.size() != n || L.ord_of_mesh.size() != n || L.part_of_mesh.size() != n || L.ord_passes != (3 * bits + 7) / 8)
    FAIL("%zu order records for %u clouds, %u passes", L.ord.size(), n, L.ord_passes);
  // the arena: the uploads as enc_upload copies them, everything behind them zero, every gap between two regions poisoned
  std::vector<uint8_t> store(L.total_bytes + 256, 0);
  uint8_t *arena = store.data();
  for (const EncUpload &u : L.uploads) {
    if (u.off >= L.input_bytes || u.off + u.bytes > L.input_bytes || u.narrow) FAIL("an upload outside the inputs");
    if (u.bytes) memcpy(arena + u.off, u.src, u.bytes);
  }
  std::map<uint64_t, uint64_t> region;
  for (const auto &r : log) { if (r.first + r.second > L.total_bytes) FAIL("a region outside the arena"); region[r.first] = std::max(region[r.first], r.second); }
  auto sized = [&](uint64_t off, uint64_t bytes) { auto it = region.find(off); return it != region.end() && it->second >= bytes; };
  if (!sized(L.parts_at, sizeof(dsa::EncPart) * L.parts.size()) || !sized(L.part_tiles_at, sizeof(dsa::EncPartTile) * L.part_tiles.size())) FAIL("the part records are not among the uploads");
  const uint32_t kept_buffer = (L.ord_passes + 1) & 1;
  std::vector<std::vector<uint32_t>> want_levels(n);
  std::vector<std::vector<uint32_t>> want_kept(n), want_cells(n);
  std::vector<std::vector<std::pair<uint32_t, uint32_t>>> want_ranges(n);
  std::vector<std::vector<int32_t>> want_min(n), want_max(n);
  std::vector<std::pair<uint64_t, uint64_t>> empty_regions;       // of the slots that stay empty: poisoned below
  size_t tile_at = 0, part_at = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    const dsa::EncOrder &O = L.ord[i];
    const uint32_t s0 = L.first_stream[i];
    const synth::Grid *grid = c.has_grid ? &grids[i].slot[0] : nullptr;
    synth::lod_parts(c.pos.data(), c.n, (int)bits, grid, part_cells, (int)lod_bits, want_kept[i], want_cells[i], want_ranges[i], want_levels[i], want_min[i], want_max[i]);      // (want_kept: the rows in lod order)
    const uint32_t live = (uint32_t)want_ranges[i].size(), slots = (uint32_t)(((uint64_t)c.n + part_cells - 1) / part_cells) + levels - 1u, cap = std::min(part_cells, c.n);
    if (L.ord_of_mesh[i] != i || O.n != c.n || O.merge != 1 || O.rank != 0 || O.count != 0 || O.cells == 0 || O.stream0 != s0 || O.streams != 2 || O.part_cells != part_cells || O.part0 != part_at ||
        O.part_slots != slots || O.lod_bits != lod_bits || O.lod_rows != O.key[kept_buffer] || !sized(O.lod_table, sizeof(dsa::EncLodTable)))
      FAIL("case %u: order record", i);
    if (live == 0 || live > slots || ck.num_parts(i) != slots || L.part_of_mesh[i] != part_at || L.first_stream[i + 1] != s0 + 2 * slots) FAIL("case %u: %u slots laid out, %u expected for %u parts", i, ck.num_parts(i), slots, live);
    if (!sized(O.key[0], 8ull * c.n) || !sized(O.key[1], 8ull * c.n) || !sized(O.row[0], 4ull * c.n) || !sized(O.row[1], 4ull * c.n) || !sized(O.hist, 4ull * levels * O.tiles) || !sized(O.cells, 4ull * c.n))
      FAIL("case %u: order regions too small", i);
    if ((uint64_t)slots * cap >= (uint64_t)c.n + (uint64_t)part_cells * levels) FAIL("case %u: %u slots of %u points for %u rows", i, slots, cap, c.n);
    for (uint32_t p = 0; p < slots; ++p, ++part_at) {
      const dsa::EncPart &P = L.parts[part_at];
      if (P.cloud != i || P.lo != 0 || P.n != 0 || P.pad != 0) FAIL("case %u slot %u: the record does not start empty", i, p);
      for (int k = 0; k < 3; ++k) if (P.qmin[k] != INT32_MAX || P.qmax[k] != INT32_MIN) FAIL("case %u slot %u: the box does not start empty", i, p);
      for (uint32_t t = 0; t < (cap + ORD_TILE - 1) / ORD_TILE; ++t, ++tile_at)
        if (tile_at >= L.part_tiles.size() || L.part_tiles[tile_at].part != part_at || L.part_tiles[tile_at].tile != t) FAIL("case %u slot %u: tile %u is not in the list", i, p, t);
      for (uint32_t k = 0; k < 2; ++k) {
        const dsa::EncStream &S = L.streams[s0 + 2 * p + k], &first = L.streams[s0 + k];
        if (S.linear != 0 || S.rows != c.n || S.vals == 0 || S.vals != first.vals || S.src != first.src || S.part != (p ? (dsa::ENC_PART_BEHIND | dsa::ENC_PART_SIZED) : 0u) || (p && S.nv != 0))
          FAIL("case %u slot %u: stream %u is not a slot on the cloud's values", i, p, k);
        if (p && (S.grid_mode != 0 || S.d == first.d || S.syms == first.syms || S.hist_raw == first.hist_raw || S.out_rans == first.out_rans)) FAIL("case %u slot %u: stream %u shares a region of the first slot's", i, p, k);
        if (S.d == S.vals || !sized(S.d, 4ull * S.nc * cap) || !sized(S.syms, 4ull * S.nc * cap) || !sized(S.bl, cap) || !sized(first.vals, 4ull * S.nc * c.n) || S.out_cap < 4u * cap * S.nc + 16u ||
            !sized(S.out_rans, S.out_cap) || !sized(S.out_bits, S.out_cap) || !sized(S.hist_raw, 4ull * S.hist_cap) || !sized(S.prob, 4ull * 64) || !sized(S.cum, 4ull * 64) || !sized(S.plan_order, 4ull * 64) ||
            !sized(S.plan_tmp, 4ull * 64))
          FAIL("case %u slot %u: regions of stream %u too small", i, p, k);
        if (p >= live)
          for (uint64_t off : {S.d, S.syms, S.bl, S.hist_raw, S.out_rans, S.out_bits, S.prob, S.cum, S.plan_order, S.plan_tmp}) empty_regions.push_back({off, region[off]});
      }
    }
    if (O.vals != L.streams[s0].vals) FAIL("case %u: the sort does not read the positions' integers", i);
    synth::PortableAttr a;
    a.att_type = 0; a.nc = a.nc_out = 3; a.seq_type = 2; a.grid = grid;
    synth::quantize(c.pos.data(), c.n, 3, (int)bits, a);
    memcpy(arena + O.vals, a.vals.data(), 12ull * c.n);
    int32_t *nv = (int32_t *)(arena + L.streams[s0 + 1].vals);       // the normals' two integers per row: the row, told apart per component
    for (uint32_t r = 0; r < c.n; ++r) { nv[2 * r] = (int32_t)r; nv[2 * r + 1] = ~(int32_t)r; }
  }
  if (tile_at != L.part_tiles.size() || part_at != L.parts.size()) FAIL("%zu part tiles and %zu slots laid out, %zu and %zu expected", L.part_tiles.size(), L.parts.size(), tile_at, part_at);
  dsa::EncOrder *clouds = (dsa::EncOrder *)(arena + L.ord_at);
  const dsa::EncOrderTile *tiles = (const dsa::EncOrderTile *)(arena + L.ord_tiles_at);
  dsa::EncPart *parts = (dsa::EncPart *)(arena + L.parts_at);
  const dsa::EncPartTile *part_tiles = (const dsa::EncPartTile *)(arena + L.part_tiles_at);
  std::vector<dsa::EncStream> records = L.streams;            // the device's records: k_enc_merge_scan and k_enc_lod_parts write nv and e2v in them
  const std::vector<dsa::EncStream> laid_streams = L.streams;
  ASAN_POISON_MEMORY_REGION(arena, store.size());
  for (const auto &r : region) ASAN_UNPOISON_MEMORY_REGION(arena + r.first, r.second);
  for (const auto &r : empty_regions) ASAN_POISON_MEMORY_REGION(arena + r.first, r.second);
  auto go = [backwards](auto kernel, uint32_t grid_x, uint32_t grid_y, uint32_t block, auto... args) { launch(kernel, grid_x, grid_y, block, backwards, args...); };
  dsa::enc_order_launch(go, arena, (const dsa::EncOrder *)clouds, n, tiles, (uint32_t)L.ord_tiles.size(), L.ord_passes, false, 0u);
  dsa::enc_merge_launch(go, arena, clouds, n, tiles, (uint32_t)L.ord_tiles.size(), L.ord_passes, records.data(), (uint32_t)records.size());
  dsa::enc_lod_launch(go, arena, (const dsa::EncOrder *)clouds, n, tiles, (uint32_t)L.ord_tiles.size(), L.ord_passes, parts, (uint32_t)L.parts.size(), records.data(), (uint32_t)records.size());
  dsa::enc_part_launch(go, arena, (const dsa::EncOrder *)clouds, n, parts, (uint32_t)L.parts.size(), part_tiles, (uint32_t)L.part_tiles.size(), L.ord_passes);
  // the gather's accesses, stream record by stream record, but for the records the product's kernels pass by
  for (const dsa::EncStream &S : records) {
    if (S.kind == 3) continue;
    const int32_t *vals = (const int32_t *)(arena + S.vals);
    const uint32_t *e2v = (const uint32_t *)(arena + S.e2v);
    int32_t *dst = (int32_t *)(arena + S.d);
    for (uint32_t e = 0; e < S.nv; ++e)
      for (uint32_t k = 0; k < S.nc; ++k) dst[(size_t)e * S.nc + k] = vals[(size_t)e2v[e] * S.nc + k];
  }
  ck.L.streams = records;                                     // what the product's host reads: the records that came back
  part_at = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    const uint32_t s0 = L.first_stream[i], m = (uint32_t)want_kept[i].size(), live = (uint32_t)want_ranges[i].size(), slots = ck.num_parts(i);
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
    for (uint32_t p = 0; p < slots; ++p, ++part_at) {
      const dsa::EncPart &P = parts[part_at], &laid = L.parts[part_at];
      const uint32_t lo = p < live ? want_ranges[i][p].first : 0u, cnt = p < live ? want_ranges[i][p].second - lo : 0u;
      if (P.cloud != laid.cloud || P.pad != (p < live ? want_levels[i][p] : 0u)) FAIL("case %u slot %u: the record changed beyond its range and box", i, p);
      if (P.lo != lo || P.n != cnt || (p < live && (cnt == 0 || cnt > part_cells))) FAIL("case %u slot %u: record says %u + %u, the host coder %u + %u", i, p, P.lo, P.n, lo, cnt);
      for (uint32_t k = 0; k < 2; ++k) {
        dsa::EncStream a = records[s0 + 2 * p + k], b = laid_streams[s0 + 2 * p + k];
        if (a.nv != cnt || a.e2v != clouds[i].lod_rows + 4ull * lo) FAIL("case %u slot %u: stream %u has nv %u and reads from %llu", i, p, k, a.nv, (unsigned long long)a.e2v);
        if (a.kind != (p < live ? b.kind : 3u) || (a.part & dsa::ENC_PART_SIZED) != (p ? dsa::ENC_PART_SIZED : 0u)) FAIL("case %u slot %u: stream %u is of kind %u", i, p, k, a.kind);
        a.nv = b.nv; a.e2v = b.e2v; a.kind = b.kind;
        if (memcmp(&a, &b, sizeof(a)) != 0) FAIL("case %u slot %u: the record of stream %u changed beyond nv, e2v and the kind of an empty slot", i, p, k);
      }
      if (p >= live) {
        for (int k = 0; k < 3; ++k) if (P.qmin[k] != INT32_MAX || P.qmax[k] != INT32_MIN) FAIL("case %u slot %u: an empty slot has a box", i, p);
        ++empty_seen;
        continue;
      }
      for (int k = 0; k < 3; ++k)
        if (P.qmin[k] != want_min[i][3 * p + k] || P.qmax[k] != want_max[i][3 * p + k])
          FAIL("case %u (%u points) part %u component %d: box %d .. %d, the host coder %d .. %d", i, c.n, p, k, P.qmin[k], P.qmax[k], want_min[i][3 * p + k], want_max[i][3 * p + k]);
      const int32_t *dp = (const int32_t *)(arena + laid_streams[s0 + 2 * p].d), *dn = (const int32_t *)(arena + laid_streams[s0 + 2 * p + 1].d);
      for (uint32_t e = 0; e < P.n; ++e) {
        const uint32_t r = want_kept[i][P.lo + e];
        if (memcmp(dp + 3 * (size_t)e, q + 3 * (size_t)r, 12) != 0 || dn[2 * e] != (int32_t)r || dn[2 * e + 1] != ~(int32_t)r) FAIL("case %u part %u: entry %u does not carry row %u", i, p, e, r);
      }
      ++parts_seen;
    }
    points += c.n;
  }
  ASAN_UNPOISON_MEMORY_REGION(arena, store.size());
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: enclod_host <cases.bin>\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  std::vector<In> cases(count);
  for (auto &c : cases) {
    uint32_t head[5];
    if (fread(head, 4, 5, f) != 5) return 2;
    c.n = head[0]; c.bits = head[1]; c.has_grid = head[2]; c.part_cells = head[3]; c.lod_bits = head[4];
    if (c.n == 0 || c.bits < 1 || c.bits > 20 || c.part_cells == 0 || c.part_cells > 0x7FFFFFFFu || c.lod_bits < 1 || c.lod_bits > c.bits) return 2;
    c.pos.resize((size_t)3 * c.n);
    if (fread(c.pos.data(), 4, c.pos.size(), f) != c.pos.size()) return 2;
    if (c.has_grid && fread(c.grid, 4, 4, f) != 4) return 2;
  }
  fclose(f);
  uint32_t chunks = 0;
  uint64_t points = 0, parts = 0, empty = 0;
  std::map<std::pair<std::pair<uint32_t, uint32_t>, uint32_t>, std::vector<const In *>> groups;      // (bits, part_cells, lod_base_bits): one request
  for (const In &c : cases) groups[{{c.bits, c.part_cells}, c.lod_bits}].push_back(&c);
  for (const auto &g : groups) {
    for (int backwards = 0; backwards < 2; ++backwards) if (run(g.second, g.first.first.first, g.first.first.second, g.first.second, backwards != 0, points, parts, empty) != 0) return 1;
    ++chunks;
  }
  printf("enclod: %u cases in %u chunks cut as the host coder cuts them, forwards and backwards (%llu points, %llu parts, %llu empty slots untouched)\n", count, chunks,
         (unsigned long long)points, (unsigned long long)parts, (unsigned long long)empty);
  return 0;
}
