// tests/hostcheck/encorder_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The encoder's point-order kernels (draco-sharp_amd/csrc/dsa_encode_order.h: keys, the segmented radix sort's histogram, scan and
// scatter, rank, the faces through rank) compiled for the host with AddressSanitizer + UBSan and run thread by thread under the
// product's launch sequence (enc_order_launch) in the arena the product's layout hands out (enc_layout_sequential with
// EncRequest::point_order: records, tile list and every region are the library's own) -- once forwards, once backwards -- against
// the host coder's order (dsa_encode_host.h: synth::point_order) on the same points: the same permutation in the region every
// stream of the cloud reads as its entry -> row map, its inverse, the same remapped faces, and not one access outside a region
// (the arena's gaps are poisoned).  The clouds of one position_bits are one chunk, so that the segmented passes meet every size
// side by side.  Nothing here is linked into the product.
//
//   encorder_host <cases.bin>   file: u32 count, then per case u32 n, bits, has_grid, F; f32 pos[3 n]; with a grid f32 origin[3],
//                               range; u32 faces[3 F]
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
  uint32_t n = 0, bits = 0, has_grid = 0, F = 0;
  std::vector<float> pos;
  float grid[4] = {0, 0, 0, 0};
  std::vector<uint32_t> faces;
};

#define FAIL(...) do { fprintf(stderr, "bits %u, %s, %s: ", bits, compressed ? "compressed" : (is_mesh ? "raw" : "cloud"), backwards ? "backwards" : "forwards"); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

// the cases `which` as one chunk of a request: point clouds, or meshes with raw / compressed indices
static int run(const std::vector<const In *> &which, uint32_t bits, bool is_mesh, bool compressed, bool backwards) {
  const uint32_t n = (uint32_t)which.size();
  std::vector<dsa_mesh_attr_input> meshes(n);
  std::vector<EncMeshGrids> grids(n);
  memset(meshes.data(), 0, sizeof(dsa_mesh_attr_input) * n);
  bool any_grid = false;
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    dsa_mesh_input &m = meshes[i].mesh.mesh;
    m.num_vertices = c.n; m.positions = c.pos.data();
    if (is_mesh) { m.num_faces = c.F; m.faces = c.faces.data(); }
    if (c.has_grid) { synth::Grid &g = grids[i].slot[0]; memcpy(g.origin, c.grid, 12); g.range = c.grid[3]; g.mode = 1; any_grid = true; }
  }
  EncRequest rq;
  rq.n = n; rq.meshes = meshes.data(); rq.sequential = true; rq.point_order = true;
  if (any_grid) rq.grids = grids.data();
  memset(&rq.seq, 0, sizeof(rq.seq));
  synth::Options d;
  dsa_encode_options &o = rq.seq.base;
  o.position_bits = (int32_t)bits; o.texcoord_bits = d.uv_bits; o.normal_bits = d.normal_bits; o.symbol_scheme = d.force_scheme; o.compression_level = d.compression_level;
  rq.seq.geometry = is_mesh ? 1 : 0; rq.seq.compress_connectivity = compressed ? 1 : 0;
  EncChunk ck(rq, 0, n, n);
  std::vector<std::pair<uint64_t, uint64_t>> log;
  ck.region_log = &log;
  for (uint32_t i = 0; i < n; ++i) { enc_check_sequential_mesh(ck, i); if (!ck.good(i)) FAIL("case %u refused: %s", i, ck.E->messages[i].c_str()); }
  enc_layout_sequential(ck);
  const EncLayout &L = ck.L;
  if (L.ord.size() != n || L.ord_passes != (3 * bits + 7) / 8) FAIL("%zu order records for %u clouds, %u passes", L.ord.size(), n, L.ord_passes);
  uint64_t tiles = 0;
  for (const dsa::EncOrder &O : L.ord) tiles += O.tiles;
  if (L.ord_tiles.size() != tiles) FAIL("%zu tiles listed, %llu in the records", L.ord_tiles.size(), (unsigned long long)tiles);
  // the arena: the uploads as enc_upload copies them, everything behind them zero, every gap between two regions poisoned
  std::vector<uint8_t> store(L.total_bytes + 256, 0);
  uint8_t *arena = store.data();
  for (const EncUpload &u : L.uploads) {
    if (u.off >= L.input_bytes || u.off + u.bytes > L.input_bytes) FAIL("an upload outside the inputs");
    if (!u.narrow) { if (u.bytes) memcpy(arena + u.off, u.src, u.bytes); continue; }
    for (size_t e = 0; e < u.bytes / 2; ++e) ((uint16_t *)(arena + u.off))[e] = (uint16_t)((const uint32_t *)u.src)[e];
  }
  std::map<uint64_t, uint64_t> region;
  for (const auto &r : log) { if (r.first + r.second > L.total_bytes) FAIL("a region outside the arena"); region[r.first] = std::max(region[r.first], r.second); }
  auto sized = [&](uint64_t off, uint64_t bytes) { auto it = region.find(off); return it != region.end() && it->second >= bytes; };
  // the position integers, where k_enc_quantize / k_enc_grid_quantize leave them
  std::vector<std::vector<uint32_t>> want(n);
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    const dsa::EncOrder &O = L.ord[i];
    const dsa::EncStream &S = L.streams[L.first_stream[i]];
    if (O.n != c.n || O.bits != bits || O.tiles != (c.n + ORD_TILE - 1) / ORD_TILE || O.vals != S.vals) FAIL("case %u: order record", i);
    if (!sized(O.vals, 12ull * c.n) || !sized(O.key[0], 8ull * c.n) || !sized(O.key[1], 8ull * c.n) || !sized(O.row[0], 4ull * c.n) || !sized(O.row[1], 4ull * c.n) ||
        !sized(O.hist, 1024ull * O.tiles) || (is_mesh && !sized(O.rank, 4ull * c.n)) || (!is_mesh && O.rank != 0)) FAIL("case %u: order regions too small", i);
    if (S.linear != 0 || S.e2v != O.row[L.ord_passes & 1] || S.d == S.vals || !sized(S.d, 12ull * c.n)) FAIL("case %u: the streams do not read the order", i);
    if (compressed != (O.count != 0) || (compressed && (O.count != 3 * c.F || O.faces >= L.input_bytes || !sized(O.faces, (O.narrow ? 2ull : 4ull) * O.count)))) FAIL("case %u: faces of the order record", i);
    synth::PortableAttr a;
    a.att_type = 0; a.nc = a.nc_out = 3; a.seq_type = 2; a.grid = c.has_grid ? &grids[i].slot[0] : nullptr;
    synth::quantize(c.pos.data(), c.n, 3, (int)bits, a);
    memcpy(arena + O.vals, a.vals.data(), 12ull * c.n);
    synth::point_order(c.pos.data(), c.n, (int)bits, a.grid, want[i]);
  }
  ASAN_POISON_MEMORY_REGION(arena, store.size());
  for (const auto &r : region) ASAN_UNPOISON_MEMORY_REGION(arena + r.first, r.second);
  const uint32_t gf = L.max_count ? std::max(1u, std::min(4u, (L.max_count + 1023u) / 1024u)) : 0u;
  dsa::enc_order_launch([backwards](auto kernel, uint32_t grid_x, uint32_t grid_y, uint32_t block, auto... args) { launch(kernel, grid_x, grid_y, block, backwards, args...); },
                        arena, (const dsa::EncOrder *)(arena + L.ord_at), n, (const dsa::EncOrderTile *)(arena + L.ord_tiles_at), (uint32_t)L.ord_tiles.size(),
                        L.ord_passes, is_mesh, gf);
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    const dsa::EncOrder &O = L.ord[i];
    const uint32_t *perm = (const uint32_t *)(arena + L.streams[L.first_stream[i]].e2v);
    for (uint32_t e = 0; e < c.n; ++e) if (perm[e] != want[i][e]) FAIL("case %u (%u points): entry %u carries row %u, the host coder's order has %u", i, c.n, e, perm[e], want[i][e]);
    if (!is_mesh) continue;
    const uint32_t *rank = (const uint32_t *)(arena + O.rank);
    for (uint32_t e = 0; e < c.n; ++e) if (rank[want[i][e]] != e) FAIL("case %u: rank of row %u", i, want[i][e]);
    for (uint32_t k = 0; compressed && k < 3 * c.F; ++k) {
      const uint32_t got = O.narrow ? (uint32_t)((const uint16_t *)(arena + O.faces))[k] : ((const uint32_t *)(arena + O.faces))[k];
      if (got != rank[c.faces[k]]) FAIL("case %u: corner %u is %u, rank[%u] = %u", i, k, got, c.faces[k], rank[c.faces[k]]);
    }
  }
  ASAN_UNPOISON_MEMORY_REGION(arena, store.size());
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: encorder_host <cases.bin>\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  std::vector<In> cases(count);
  for (auto &c : cases) {
    uint32_t head[4];
    if (fread(head, 4, 4, f) != 4) return 2;
    c.n = head[0]; c.bits = head[1]; c.has_grid = head[2]; c.F = head[3];
    if (c.n == 0 || c.bits < 1 || c.bits > 20) return 2;
    c.pos.resize((size_t)3 * c.n);
    if (fread(c.pos.data(), 4, c.pos.size(), f) != c.pos.size()) return 2;
    if (c.has_grid && fread(c.grid, 4, 4, f) != 4) return 2;
    c.faces.resize((size_t)3 * c.F);
    if (c.F && fread(c.faces.data(), 4, c.faces.size(), f) != c.faces.size()) return 2;
    for (uint32_t x : c.faces) if (x >= c.n) { fprintf(stderr, "index out of range in the input file\n"); return 2; }
  }
  fclose(f);
  uint32_t chunks = 0;
  for (uint32_t bits = 1; bits <= 20; ++bits)
    for (int kind = 0; kind < 3; ++kind) {                     // point clouds; meshes with raw indices; with compressed indices
      std::vector<const In *> which;
      for (const In &c : cases) if (c.bits == bits && (kind == 0 || c.F > 0)) which.push_back(&c);
      if (which.empty()) continue;
      for (int backwards = 0; backwards < 2; ++backwards) if (run(which, bits, kind != 0, kind == 2, backwards != 0) != 0) return 1;
      ++chunks;
    }
  printf("encorder: %u cases in %u chunks ordered as the host coder orders them, forwards and backwards\n", count, chunks);
  return 0;
}
