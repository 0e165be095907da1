// tests/hostcheck/encmeans_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The encoder's mean steps (draco-sharp_amd/csrc/dsa_encode_order.h: k_enc_mean_sum in its serial form, k_enc_mean_store as it
// stands) compiled for the host with AddressSanitizer + UBSan and run thread by thread in the product's launch sequence for a chunk
// with mean_attributes != 0 -- the sort (enc_order_launch), the merge (enc_merge_launch), the zeroing of the sums and counts, the
// means (enc_mean_launch) -- in the arena the product's layout hands out for such a chunk (enc_layout_sequential with
// EncRequest::point_order, merge_points and mean_attributes: stream records, order records, the EncMean / EncMeanCloud records, the
// tile list and every region are the library's own) -- once forwards, once backwards -- against the host coder (dsa_encode_host.h:
// synth::merge_points, synth::merge_means) on the same points and integers: at every kept row of a masked stream the mean of its
// cell, every other integer of every stream as it was, and not one access outside a region (the arena's gaps are poisoned).  The
// sums and counts are filled with a pattern and poisoned until the product's one memset range is zeroed, as the product zeroes it.
// k_enc_gather itself lives in dsa_encode.h, which needs HIP: its accesses -- e2v[e], vals[nc e2v[e] + c], d[nc e + c] for e < nv --
// are made here in its place, and what lands in d is held to the means (masked) or to row kept[j] (not masked).
// Every cloud carries texture coordinates (stream 1, two components, integers over +-2^30 so that a sum leaves 32 bits) and a generic
// attribute (stream 2, three bytes); the chunk runs with mask 0b010 (one record per cloud, stream 2 not masked) and with mask 0b110
// (two records per cloud: blockIdx.y = 1).  The clouds of one position_bits are one chunk.  Nothing here is linked into the product.
//
//   encmeans_host <cases.bin>   file: u32 count, then per case u32 n, bits, has_grid, 0; f32 pos[3 n]; with a grid f32 origin[3], range
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

#define FAIL(...) do { fprintf(stderr, "bits %u, mask 0x%x, %s: ", bits, mask, backwards ? "backwards" : "forwards"); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

static uint32_t mix(uint32_t x) { x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16; return x; }
// the integer of row r, component c of stream k of cloud i: stream 1 over +-2^30, stream 2 a byte
static int32_t designed(uint32_t i, uint32_t k, uint32_t r, uint32_t c) {
  const uint32_t h = mix(r * 8u + c + 0x9E3779B9u * (i + 1u) + 77u * k);
  return k == 1 ? (int32_t)h / 2 : (int32_t)(h & 255u);
}

// the cases `which` as one chunk of a request of point clouds
static int run(const std::vector<const In *> &which, uint32_t bits, uint32_t mask, bool backwards, uint64_t &points, uint64_t &cells, uint64_t &wide) {
  const uint32_t n = (uint32_t)which.size();
  std::vector<dsa_mesh_attr_input> meshes(n);
  std::vector<EncMeshGrids> grids(n);
  memset(meshes.data(), 0, sizeof(dsa_mesh_attr_input) * n);
  bool any_grid = false;
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    dsa_mesh_input &m = meshes[i].mesh.mesh;
    // (texcoords: 2 n floats, generic: 3 n bytes -- both inside the 3 n floats of the positions; their values are not read here)
    m.num_vertices = c.n; m.positions = c.pos.data(); m.texcoords = c.pos.data(); m.generic = (const uint8_t *)c.pos.data(); m.generic_components = 3;
    if (c.has_grid) { synth::Grid &g = grids[i].slot[0]; memcpy(g.origin, c.grid, 12); g.range = c.grid[3]; g.mode = 1; any_grid = true; }
  }
  EncRequest rq;
  rq.n = n; rq.meshes = meshes.data(); rq.sequential = true; rq.point_order = true; rq.merge_points = true; rq.mean_attributes = mask;
  if (any_grid) rq.grids = grids.data();
  memset(&rq.seq, 0, sizeof(rq.seq));
  synth::Options d;
  dsa_encode_options &o = rq.seq.base;
  o.position_bits = (int32_t)bits; o.texcoord_bits = d.uv_bits; o.normal_bits = d.normal_bits; o.symbol_scheme = d.force_scheme; o.compression_level = d.compression_level;
  rq.seq.geometry = 0; rq.seq.compress_connectivity = 0;
  if (!rq.merged() || !rq.means()) FAIL("the request is not one with means");
  EncChunk ck(rq, 0, n, n);
  if (!ck.E->merged || ck.E->cells.size() != n) FAIL("the chunk's handle keeps no row entries");
  std::vector<std::pair<uint64_t, uint64_t>> log;
  ck.region_log = &log;
  for (uint32_t i = 0; i < n; ++i) { enc_check_sequential_mesh(ck, i); if (!ck.good(i)) FAIL("case %u refused: %s", i, ck.E->messages[i].c_str()); }
  enc_layout_sequential(ck);
  const EncLayout &L = ck.L;
  const uint32_t per_cloud = (mask >> 1 & 1u) + (mask >> 2 & 1u);
  if (!L.merge || L.ord.size() != n || L.ord_passes != (3 * bits + 7) / 8) FAIL("%zu order records for %u clouds, %u passes", L.ord.size(), n, L.ord_passes);
  if (L.mean_clouds.size() != n || L.means.size() != (size_t)per_cloud * n || L.mean_stream.size() != L.means.size() || L.mean_most != per_cloud) FAIL("%zu mean records for %u clouds", L.means.size(), n);
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
  if (!sized(L.mean_clouds_at, sizeof(dsa::EncMeanCloud) * n) || !sized(L.means_at, sizeof(dsa::EncMean) * L.means.size())) FAIL("the mean records are not among the uploads");
  if (L.mean_zero_at < L.input_bytes || L.mean_zero_at + L.mean_zero_bytes != L.total_bytes) FAIL("the sums and counts are not the end of the arena");
  std::vector<std::vector<uint32_t>> want_kept(n), want_cells(n);
  std::vector<std::vector<int32_t>> given[3];                 // per stream and cloud: the integers before the means
  for (auto &g : given) g.resize(n);
  const uint32_t kept_buffer = (L.ord_passes + 1) & 1;
  for (uint32_t i = 0, rec = 0; i < n; ++i) {
    const In &c = *which[i];
    const dsa::EncOrder &O = L.ord[i];
    const dsa::EncMeanCloud &MC = L.mean_clouds[i];
    const uint32_t s0 = L.first_stream[i];
    if (O.n != c.n || O.merge != 1 || O.stream0 != s0 || O.streams != 3 || L.first_stream[i + 1] != s0 + 3 || O.cells == 0) FAIL("case %u: order record", i);
    if (MC.first != rec || MC.count != per_cloud || !sized(MC.cnt, 4ull * c.n) || MC.cnt < L.mean_zero_at) FAIL("case %u: mean record of the cloud", i);
    for (uint32_t k = 1; k < 3; ++k) {
      const dsa::EncStream &S = L.streams[s0 + k];
      if (S.nc != k + 1 || S.e2v != O.row[kept_buffer] || S.d == S.vals || !sized(S.vals, 4ull * S.nc * c.n) || !sized(S.d, 4ull * S.nc * c.n)) FAIL("case %u: stream %u", i, k);
      if (!((mask >> k) & 1u)) continue;
      const dsa::EncMean &M = L.means[rec];
      if (L.mean_stream[rec] != s0 + k || M.vals != S.vals || M.nc != S.nc || !sized(M.acc, 8ull * S.nc * c.n) || M.acc < L.mean_zero_at) FAIL("case %u: mean record of stream %u", i, k);
      ++rec;
    }
    synth::PortableAttr a;
    a.att_type = 0; a.nc = a.nc_out = 3; a.seq_type = 2; a.grid = c.has_grid ? &grids[i].slot[0] : nullptr;
    synth::quantize(c.pos.data(), c.n, 3, (int)bits, a);
    memcpy(arena + O.vals, a.vals.data(), 12ull * c.n);
    given[0][i] = a.vals;
    for (uint32_t k = 1; k < 3; ++k) {
      const uint32_t nc = k + 1;
      given[k][i].resize((size_t)nc * c.n);
      for (uint32_t r = 0; r < c.n; ++r) for (uint32_t q = 0; q < nc; ++q) given[k][i][(size_t)nc * r + q] = designed(i, k, r, q);
      memcpy(arena + L.streams[s0 + k].vals, given[k][i].data(), 4ull * nc * c.n);
    }
    synth::merge_points(c.pos.data(), c.n, (int)bits, a.grid, want_kept[i], want_cells[i]);
  }
  std::vector<dsa::EncStream> records = L.streams;            // the device's records: k_enc_merge_scan lowers nv in them
  dsa::EncOrder *clouds = (dsa::EncOrder *)(arena + L.ord_at);
  const dsa::EncOrderTile *tiles = (const dsa::EncOrderTile *)(arena + L.ord_tiles_at);
  memset(arena + L.mean_zero_at, 0xAB, L.mean_zero_bytes);    // what an arena used before leaves there
  ASAN_POISON_MEMORY_REGION(arena, store.size());
  for (const auto &r : region) ASAN_UNPOISON_MEMORY_REGION(arena + r.first, r.second);
  ASAN_POISON_MEMORY_REGION(arena + L.mean_zero_at, L.mean_zero_bytes);       // nothing in front of the means touches the sums and counts
  auto go = [backwards](auto kernel, uint32_t grid_x, uint32_t grid_y, uint32_t block, auto... args) { launch(kernel, grid_x, grid_y, block, backwards, args...); };
  dsa::enc_order_launch(go, arena, (const dsa::EncOrder *)clouds, n, tiles, (uint32_t)L.ord_tiles.size(), L.ord_passes, false, 0u);
  dsa::enc_merge_launch(go, arena, clouds, n, tiles, (uint32_t)L.ord_tiles.size(), L.ord_passes, records.data(), (uint32_t)records.size());
  // the product's memset: the one range, gaps between its regions included
  ASAN_UNPOISON_MEMORY_REGION(arena + L.mean_zero_at, L.mean_zero_bytes);
  memset(arena + L.mean_zero_at, 0, L.mean_zero_bytes);
  ASAN_POISON_MEMORY_REGION(arena + L.mean_zero_at, L.mean_zero_bytes);
  for (const auto &r : region) if (r.first >= L.mean_zero_at) ASAN_UNPOISON_MEMORY_REGION(arena + r.first, r.second);
  dsa::enc_mean_launch(go, arena, (const dsa::EncOrder *)clouds, n, tiles, (uint32_t)L.ord_tiles.size(), L.ord_passes, (const dsa::EncMeanCloud *)(arena + L.mean_clouds_at),
                       (const dsa::EncMean *)(arena + L.means_at), (uint32_t)L.means.size(), L.mean_most);
  // the gather's accesses, stream record by stream record
  for (const dsa::EncStream &S : records) {
    const int32_t *vals = (const int32_t *)(arena + S.vals);
    const uint32_t *e2v = (const uint32_t *)(arena + S.e2v);
    int32_t *dst = (int32_t *)(arena + S.d);
    for (uint32_t e = 0; e < S.nv; ++e)
      for (uint32_t k = 0; k < S.nc; ++k) dst[(size_t)e * S.nc + k] = vals[(size_t)e2v[e] * S.nc + k];
  }
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    const uint32_t s0 = L.first_stream[i], m = (uint32_t)want_kept[i].size();
    if (clouds[i].m != m) FAIL("case %u (%u points): the record has %u cells, the host coder %u", i, c.n, clouds[i].m, m);
    const uint32_t *kept = (const uint32_t *)(arena + records[s0].e2v), *row_entries = (const uint32_t *)(arena + clouds[i].cells);
    for (uint32_t j = 0; j < m; ++j) if (kept[j] != want_kept[i][j]) FAIL("case %u (%u points): entry %u carries row %u, the host coder keeps %u", i, c.n, j, kept[j], want_kept[i][j]);
    for (uint32_t r = 0; r < c.n; ++r) if (row_entries[r] != want_cells[i][r]) FAIL("case %u (%u points): row %u lies in entry %u, the host coder says %u", i, c.n, r, row_entries[r], want_cells[i][r]);
    std::vector<uint32_t> rows(m, 0);
    for (uint32_t r = 0; r < c.n; ++r) ++rows[want_cells[i][r]];
    if (per_cloud) { const uint32_t *cnt = (const uint32_t *)(arena + L.mean_clouds[i].cnt); for (uint32_t j = 0; j < m; ++j) if (cnt[j] != rows[j]) FAIL("case %u: cell %u counted %u rows, it has %u", i, j, cnt[j], rows[j]); }
    for (uint32_t k = 0; k < 3; ++k) {
      const dsa::EncStream &S = records[s0 + k];
      const uint32_t nc = S.nc;
      if (S.nv != m) FAIL("case %u: nv of stream %u is %u, %u cells", i, k, S.nv, m);
      std::vector<int32_t> want = given[k][i];                // the integers behind the means: the mean at every kept row of a masked stream
      if (k && ((mask >> k) & 1u)) {
        std::vector<int32_t> means;
        synth::merge_means(given[k][i].data(), c.n, (int)nc, want_cells[i], m, means);
        std::vector<int64_t> sum((size_t)m * nc, 0);
        for (uint32_t r = 0; r < c.n; ++r) for (uint32_t q = 0; q < nc; ++q) sum[(size_t)nc * want_cells[i][r] + q] += given[k][i][(size_t)nc * r + q];
        for (int64_t s : sum) if (s > INT32_MAX || s < INT32_MIN) ++wide;
        for (uint32_t j = 0; j < m; ++j) for (uint32_t q = 0; q < nc; ++q) want[(size_t)nc * kept[j] + q] = means[(size_t)nc * j + q];
      }
      const int32_t *vals = (const int32_t *)(arena + S.vals), *dst = (const int32_t *)(arena + S.d);
      for (size_t x = 0; x < want.size(); ++x) if (vals[x] != want[x]) FAIL("case %u stream %u: integer %zu of row %zu is %d, the host coder says %d", i, k, x % nc, x / nc, vals[x], want[x]);
      for (uint32_t j = 0; j < m; ++j) for (uint32_t q = 0; q < nc; ++q)
        if (dst[(size_t)nc * j + q] != want[(size_t)nc * kept[j] + q]) FAIL("case %u stream %u: entry %u does not carry what row %u holds", i, k, j, kept[j]);
    }
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
  if (argc < 2) { fprintf(stderr, "usage: encmeans_host <cases.bin>\n"); return 2; }
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
  uint64_t points = 0, cells = 0, wide = 0;
  for (uint32_t bits = 1; bits <= 20; ++bits) {
    std::vector<const In *> which;
    for (const In &c : cases) if (c.bits == bits) which.push_back(&c);
    if (which.empty()) continue;
    for (uint32_t mask : {2u, 6u})
      for (int backwards = 0; backwards < 2; ++backwards) if (run(which, bits, mask, backwards != 0, points, cells, wide) != 0) return 1;
    ++chunks;
  }
  printf("encmeans: %u cases in %u chunks averaged as the host coder averages them, two masks, forwards and backwards (%llu points, %llu cells, %llu sums beyond 32 bits)\n", count, chunks,
         (unsigned long long)points, (unsigned long long)cells, (unsigned long long)wide);
  return 0;
}
