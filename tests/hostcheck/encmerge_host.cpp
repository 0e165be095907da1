// tests/hostcheck/encmerge_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The encoder's merge kernels (draco-sharp_amd/csrc/dsa_encode_order.h: k_enc_merge_heads, k_enc_merge_scan, k_enc_merge_compact)
// compiled for the host with AddressSanitizer + UBSan and run thread by thread behind the product's sort (enc_order_launch, then
// enc_merge_launch) in the arena the product's layout hands out (enc_layout_sequential with EncRequest::point_order and
// merge_points: records, tile list and every region are the library's own) -- once forwards, once backwards -- against the host
// coder (dsa_encode_host.h: synth::merge_points) on the same points: the same kept rows in the region every stream of the cloud
// reads as its entry -> row map, the same row_entries, m in the cloud's record and in nv of every stream record of the cloud, and
// not one access outside a region (the arena's gaps are poisoned).  The clouds of one position_bits are one chunk.  Every cloud
// carries normals, so that a cloud has two streams whose nv must fall.  Nothing here is linked into the product.
//
//   encmerge_host <cases.bin>   file: u32 count, then per case u32 n, bits, has_grid, 0; f32 pos[3 n]; with a grid f32 origin[3], range
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
  uint32_t n = 0, bits = 0, has_grid = 0;
  std::vector<float> pos;
  float grid[4] = {0, 0, 0, 0};
};

#define FAIL(...) do { fprintf(stderr, "bits %u, %s: ", bits, backwards ? "backwards" : "forwards"); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

// the cases `which` as one chunk of a request of point clouds
static int run(const std::vector<const In *> &which, uint32_t bits, bool backwards, uint64_t &points, uint64_t &cells) {
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
  rq.n = n; rq.meshes = meshes.data(); rq.sequential = true; rq.point_order = true; rq.merge_points = true;
  if (any_grid) rq.grids = grids.data();
  memset(&rq.seq, 0, sizeof(rq.seq));
  synth::Options d;
  dsa_encode_options &o = rq.seq.base;
  o.position_bits = (int32_t)bits; o.texcoord_bits = d.uv_bits; o.normal_bits = d.normal_bits; o.symbol_scheme = d.force_scheme; o.compression_level = d.compression_level;
  rq.seq.geometry = 0; rq.seq.compress_connectivity = 0;
  EncChunk ck(rq, 0, n, n);
  if (!ck.E->merged || ck.E->cells.size() != n) FAIL("the chunk's handle keeps no row entries");
  std::vector<std::pair<uint64_t, uint64_t>> log;
  ck.region_log = &log;
  for (uint32_t i = 0; i < n; ++i) { enc_check_sequential_mesh(ck, i); if (!ck.good(i)) FAIL("case %u refused: %s", i, ck.E->messages[i].c_str()); }
  enc_layout_sequential(ck);
  const EncLayout &L = ck.L;
  if (!L.merge || L.ord.size() != n || L.ord_of_mesh.size() != n || L.ord_passes != (3 * bits + 7) / 8) FAIL("%zu order records for %u clouds, %u passes", L.ord.size(), n, L.ord_passes);
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
  std::vector<std::vector<uint32_t>> want_kept(n), want_cells(n);
  const uint32_t kept_buffer = (L.ord_passes + 1) & 1;
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    const dsa::EncOrder &O = L.ord[i];
    const uint32_t s0 = L.first_stream[i];
    if (L.ord_of_mesh[i] != i || O.n != c.n || O.merge != 1 || O.stream0 != s0 || O.streams != 2 || L.first_stream[i + 1] != s0 + 2 || O.rank != 0 || O.count != 0) FAIL("case %u: order record", i);
    if (!sized(O.key[0], 8ull * c.n) || !sized(O.key[1], 8ull * c.n) || !sized(O.row[0], 4ull * c.n) || !sized(O.row[1], 4ull * c.n) || !sized(O.hist, 4ull * O.tiles) ||
        !sized(O.cells, 4ull * c.n)) FAIL("case %u: order regions too small", i);
    for (uint32_t k = 0; k < 2; ++k) {
      const dsa::EncStream &S = L.streams[s0 + k];
      if (S.linear != 0 || S.nv != c.n || S.e2v != O.row[kept_buffer] || S.d == S.vals || !sized(S.d, 4ull * S.nc * c.n)) FAIL("case %u: stream %u does not read the kept rows", i, k);
    }
    synth::PortableAttr a;
    a.att_type = 0; a.nc = a.nc_out = 3; a.seq_type = 2; a.grid = c.has_grid ? &grids[i].slot[0] : nullptr;
    synth::quantize(c.pos.data(), c.n, 3, (int)bits, a);
    memcpy(arena + O.vals, a.vals.data(), 12ull * c.n);
    synth::merge_points(c.pos.data(), c.n, (int)bits, a.grid, want_kept[i], want_cells[i]);
  }
  std::vector<dsa::EncStream> records = L.streams;            // the device's records: k_enc_merge_scan lowers nv in them
  dsa::EncOrder *clouds = (dsa::EncOrder *)(arena + L.ord_at);
  const dsa::EncOrderTile *tiles = (const dsa::EncOrderTile *)(arena + L.ord_tiles_at);
  ASAN_POISON_MEMORY_REGION(arena, store.size());
  for (const auto &r : region) ASAN_UNPOISON_MEMORY_REGION(arena + r.first, r.second);
  auto go = [backwards](auto kernel, uint32_t grid_x, uint32_t grid_y, uint32_t block, auto... args) { launch(kernel, grid_x, grid_y, block, backwards, args...); };
  dsa::enc_order_launch(go, arena, (const dsa::EncOrder *)clouds, n, tiles, (uint32_t)L.ord_tiles.size(), L.ord_passes, false, 0u);
  dsa::enc_merge_launch(go, arena, clouds, n, tiles, (uint32_t)L.ord_tiles.size(), L.ord_passes, records.data(), (uint32_t)records.size());
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    const uint32_t s0 = L.first_stream[i], m = (uint32_t)want_kept[i].size();
    if (clouds[i].m != m) FAIL("case %u (%u points): the record has %u cells, the host coder %u", i, c.n, clouds[i].m, m);
    for (uint32_t k = 0; k < 2; ++k) if (records[s0 + k].nv != m) FAIL("case %u: nv of stream %u is %u, %u cells", i, k, records[s0 + k].nv, m);
    const uint32_t *kept = (const uint32_t *)(arena + records[s0].e2v), *row_entries = (const uint32_t *)(arena + clouds[i].cells);
    for (uint32_t j = 0; j < m; ++j) if (kept[j] != want_kept[i][j]) FAIL("case %u (%u points): entry %u carries row %u, the host coder keeps %u", i, c.n, j, kept[j], want_kept[i][j]);
    for (uint32_t r = 0; r < c.n; ++r) if (row_entries[r] != want_cells[i][r]) FAIL("case %u (%u points): row %u lies in entry %u, the host coder says %u", i, c.n, r, row_entries[r], want_cells[i][r]);
    points += c.n; cells += m;
  }
  for (size_t s = 0; s < records.size(); ++s) {                // nothing else of a record moved
    dsa::EncStream a = records[s], b = L.streams[s];
    a.nv = b.nv = 0;
    if (memcmp(&a, &b, sizeof(a)) != 0) FAIL("stream record %zu changed beyond nv", s);
  }
  ASAN_UNPOISON_MEMORY_REGION(arena, store.size());
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: encmerge_host <cases.bin>\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  std::vector<In> cases(count);
  for (auto &c : cases) {
    uint32_t head[4];
    if (fread(head, 4, 4, f) != 4) return 2;
    c.n = head[0]; c.bits = head[1]; c.has_grid = head[2];
    if (c.n == 0 || c.bits < 1 || c.bits > 20 || head[3] != 0) return 2;
    c.pos.resize((size_t)3 * c.n);
    if (fread(c.pos.data(), 4, c.pos.size(), f) != c.pos.size()) return 2;
    if (c.has_grid && fread(c.grid, 4, 4, f) != 4) return 2;
  }
  fclose(f);
  uint32_t chunks = 0;
  uint64_t points = 0, cells = 0;
  for (uint32_t bits = 1; bits <= 20; ++bits) {
    std::vector<const In *> which;
    for (const In &c : cases) if (c.bits == bits) which.push_back(&c);
    if (which.empty()) continue;
    for (int backwards = 0; backwards < 2; ++backwards) if (run(which, bits, backwards != 0, points, cells) != 0) return 1;
    ++chunks;
  }
  printf("encmerge: %u cases in %u chunks merged as the host coder merges them, forwards and backwards (%llu points, %llu cells)\n", count, chunks,
         (unsigned long long)points, (unsigned long long)cells);
  return 0;
}
