// tests/hostcheck/encvoxel_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The encoder's voxel steps (draco-sharp_amd/csrc/dsa_encode_order.h: the head predicate with its shift in k_enc_merge_heads,
// k_enc_merge_compact and the three cell passes, the positions as a record of k_enc_mean_sum / k_enc_mean_store, k_enc_voxel_near in
// its serial form and k_enc_voxel_pick as it stands, the level count of k_enc_lod_* and k_enc_part_cells) compiled for the host with
// AddressSanitizer + UBSan and run thread by thread by the product's launch sequence for a chunk with voxel_bits (enc_order_stage: the
// sort, the merge, the zeroing of every pass's range, the nearest pick, the means with the centroids among them, the votes, the mean
// normals, and with part_cells and lod_base_bits the levels, the part sizes and the part boxes) in the arena the product's layout
// hands out for such a chunk (enc_layout_sequential; encorder_common.h has the harness) -- once forwards, once backwards -- against
// the host coder (dsa_encode_host.h: synth::merge_points with voxel_bits and voxel_point, a serial pass over the voxels' rows that
// shares nothing with the kernels, and behind it synth::merge_means / merge_votes / merge_mean_normals / lod_parts) on the same points:
// the kept rows, the row entries, at every kept row the integers the host coder codes, every other integer as it was, every count
// region added to once, and not one access outside a region (the arena's gaps are poisoned; what the passes accumulate in is filled
// with a pattern and poisoned until the product's memset of its range).
// Every cloud carries normals (stream 1), texture coordinates (stream 2), a generic attribute of three bytes (stream 3) and a listed
// label (stream 4).  A chunk runs with each of the three rules alone, and with stream 3 averaged, stream 4 voted and the normals
// averaged over the voxels beside it.  Nothing here is linked into the product.
//
//   encvoxel_host <cases.bin>   file: u32 count, then per case u32 n, bits, has_grid, part_cells, lod_base_bits | voxel_bits << 8 (part_cells
//                               and lod_base_bits both 0: neither); f32 pos[3 n]; with a grid f32 origin[3], range
#include "encorder_common.h"

#define FAIL(...) do { fprintf(stderr, "bits %u, voxel_bits %u, voxel_point %u, part_cells %u, lod_base_bits %u, %s, %s: ", bits, voxel_bits, point, part_cells, lod_bits, beside ? "a mean, a vote and normals beside" : "alone", backwards ? "backwards" : "forwards"); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

static const uint32_t STREAMS = 5u, MEAN_MASK = 1u << 3, VOTE_MASK = 1u << 4;
static const uint32_t NC[STREAMS] = {3u, 2u, 2u, 3u, 1u};

static uint32_t mix(uint32_t x) { x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16; return x; }
// the integer of row r, component c of stream k of cloud i: stream 2 over +-2^30, stream 3 a byte, stream 4 one of four labels
static int32_t designed(uint32_t i, uint32_t k, uint32_t r, uint32_t c) {
  const uint32_t h = mix(r * 8u + c + 0x9E3779B9u * (i + 1u) + 77u * k);
  return k == 2 ? (int32_t)h / 2 : k == 4 ? (int32_t)(h % 4u) + 250 : (int32_t)(h & 255u);
}
static void designed_code(const synth::Octa &o, uint32_t i, uint32_t r, int32_t out[2]) {
  const uint32_t h = mix(r + 0x9E3779B9u * (i + 1u)), g = mix(h + 1u);
  int s = (int)(h % (uint32_t)(o.max_value + 1)), t = (int)(g % (uint32_t)(o.max_value + 1));
  o.canonicalize(s, t);
  out[0] = s; out[1] = t;
}
static void pattern(uint8_t *arena, uint64_t at, uint64_t bytes) {
  if (!bytes) return;
  ASAN_UNPOISON_MEMORY_REGION(arena + at, bytes);
  memset(arena + at, 0xAB, bytes);
  ASAN_POISON_MEMORY_REGION(arena + at, bytes);
}

// the cases `which` as one chunk of a request of point clouds
static int run(const std::vector<const In *> &which, uint32_t bits, uint32_t voxel_bits, uint32_t point, uint32_t part_cells, uint32_t lod_bits, bool beside, bool backwards,
               uint64_t &points, uint64_t &voxels, uint64_t &moved) {
  Run R;
  Ask ask;
  ask.bits = bits; ask.merge = true; ask.normals = ask.listed = ask.label = true; ask.part_cells = part_cells; ask.lod_base_bits = lod_bits;
  ask.mean_mask = beside ? MEAN_MASK : 0u; ask.vote_mask = beside ? VOTE_MASK : 0u;
  R.rq.mean_normals = beside; R.rq.voxel_bits = voxel_bits; R.rq.voxel_point = point;      // (Run::begin sets the fields of the request it knows and leaves the others)
  if (!R.begin(which, ask)) FAIL("%s", R.why.c_str());
  const EncLayout &L = R.L();
  const bool coarser = voxel_bits < bits, centroid = coarser && point == DSA_VOXEL_POINT_CENTROID, nearest = coarser && point == DSA_VOXEL_POINT_NEAREST;
  const uint32_t n = R.n, levels = part_cells ? voxel_bits - lod_bits + 1 : 0;
  uint8_t *arena = R.arena;
  const synth::Octa octa((int)R.rq.seq.base.normal_bits);
  if (!R.rq.merged() || R.rq.voxel_shift() != bits - voxel_bits || R.rq.centroids() != centroid || R.rq.nearest() != nearest || R.rq.means() != (beside || centroid) || R.rq.votes() != beside ||
      R.rq.normal_means() != beside || R.rq.lod() != (part_cells != 0) || R.rq.lod_levels() != (part_cells ? levels : 1u)) FAIL("the request is not the one asked for");
  const uint32_t per_cloud = (centroid ? 1u : 0u) + (beside ? 1u : 0u);
  if (L.means.size() != (size_t)per_cloud * n || L.mean_pass.most != per_cloud || L.votes.size() != (beside ? n : 0u) || L.normals.size() != (beside ? n : 0u)) FAIL("%zu mean, %zu vote and %zu normal records for %u clouds", L.means.size(), L.votes.size(), L.normals.size(), n);
  if (L.voxels.size() != (nearest ? n : 0u) || L.near_pass.stream.size() != L.voxels.size() || L.near_pass.most != (nearest ? 1u : 0u)) FAIL("%zu nearest records for %u clouds", L.voxels.size(), n);
  if (nearest) {
    if (!R.sized(L.near_pass.clouds_at, sizeof(dsa::EncCellStreams) * n) || !R.sized(L.near_pass.records_at, sizeof(dsa::EncVoxel) * n)) FAIL("the nearest records are not among the uploads");
    if (L.near_zero_at < L.input_bytes || L.near_zero_at + L.near_zero_bytes != L.total_bytes) FAIL("the best distances and rows are not the end of the arena");
    if (beside && (L.near_zero_at < L.normal_zero_at + L.normal_zero_bytes || L.normal_zero_at < L.vote_zero_at + L.vote_zero_bytes || L.vote_zero_at < L.mean_zero_at + L.mean_zero_bytes)) FAIL("the four ranges do not lie one behind the other");
  } else if (L.near_zero_bytes != 0 || L.near_pass.records_at != 0) FAIL("a range of a pass the chunk does not have");
  if (!beside && !centroid && L.mean_zero_bytes != 0) FAIL("a range of the means without a mean");
  std::vector<std::vector<uint32_t>> want_kept(n), want_cells(n), want_lod(n), want_lod_cells(n), want_levels(n);
  std::vector<std::vector<int32_t>> coded(n);
  std::vector<Run::Ranges> want_ranges(n);
  std::vector<std::vector<int32_t>> want_min(n), want_max(n);
  std::vector<std::vector<int32_t>> given[STREAMS];           // per stream and cloud: the integers as they come in
  for (auto &g : given) g.resize(n);
  std::vector<std::pair<uint64_t, uint64_t>> empty_regions;       // of the slots that stay empty: poisoned below
  size_t tile_at = 0, part_at = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    const dsa::EncOrder &O = L.ord[i];
    const uint32_t s0 = L.first_stream[i];
    if (O.n != c.n || O.merge != 1 || O.stream0 != s0 || O.streams != STREAMS || O.cells == 0 || O.voxel_shift != bits - voxel_bits || O.voxel_point != (coarser ? point : 0u)) FAIL("case %u: order record", i);
    if (per_cloud) {
      const dsa::EncCellStreams &MC = L.mean_pass.clouds[i];
      if (MC.first != per_cloud * i || MC.count != per_cloud) FAIL("case %u: the cloud's mean records", i);
      if (centroid) {                                          // the positions: the cloud's first record, the one that counts
        const dsa::EncMean &M = L.means[MC.first];
        if (L.mean_pass.stream[MC.first] != s0 || M.vals != O.vals || M.vals != L.streams[s0].vals || M.nc != 3u || !R.sized(M.acc, 24ull * c.n) || !R.sized(M.cnt, 4ull * c.n) || M.acc < L.mean_zero_at || M.cnt < L.mean_zero_at) FAIL("case %u: the mean record of the positions", i);
      }
      for (uint32_t k = MC.first; k < MC.first + MC.count; ++k) if (L.means[k].cnt != L.means[MC.first].cnt) FAIL("case %u: two count regions of the means", i);
    }
    if (nearest) {
      const dsa::EncCellStreams &XC = L.near_pass.clouds[i];
      const dsa::EncVoxel &X = L.voxels[i];
      if (XC.first != i || XC.count != 1u || L.near_pass.stream[i] != s0 || !R.sized(X.best_dist, 8ull * c.n) || !R.sized(X.best_row, 4ull * c.n) || X.best_dist < L.near_zero_at || X.best_row < L.near_zero_at) FAIL("case %u: the nearest record of the cloud", i);
    }
    R.write_positions(i);
    given[0][i].assign((const int32_t *)(arena + O.vals), (const int32_t *)(arena + O.vals) + 3ull * c.n);
    for (uint32_t k = 1; k < STREAMS; ++k) {
      const uint32_t nc = NC[k];
      if (L.streams[s0 + k].nc != nc) FAIL("case %u: stream %u has %u components", i, k, L.streams[s0 + k].nc);
      given[k][i].resize((size_t)nc * c.n);
      for (uint32_t r = 0; r < c.n; ++r) {
        if (k == 1) designed_code(octa, i, r, &given[k][i][2ull * r]);
        else for (uint32_t q = 0; q < nc; ++q) given[k][i][(size_t)nc * r + q] = designed(i, k, r, q);
      }
      memcpy(arena + L.streams[s0 + k].vals, given[k][i].data(), 4ull * nc * c.n);
    }
    synth::merge_points(c.pos.data(), c.n, (int)bits, R.grid(i), want_kept[i], want_cells[i], (int)voxel_bits, (int)point, &coded[i]);
    if (!part_cells) continue;
    synth::lod_parts(c.pos.data(), c.n, (int)bits, R.grid(i), part_cells, (int)lod_bits, want_lod[i], want_lod_cells[i], want_ranges[i], want_levels[i], want_min[i], want_max[i], (int)voxel_bits, (int)point);
    if (!R.slots_laid(i, (uint32_t)want_ranges[i].size(), (uint32_t)(((uint64_t)c.n + part_cells - 1) / part_cells) + levels - 1u, part_at, tile_at, empty_regions)) FAIL("%s", R.why.c_str());
  }
  R.poison(empty_regions);
  // the normals' and the nearest pass's ranges as the harness leaves the means' and the votes': what an arena used before holds, poisoned until the stage zeroes them
  pattern(arena, L.normal_zero_at, L.normal_zero_bytes);
  pattern(arena, L.near_zero_at, L.near_zero_bytes);
  if (!R.stage(backwards)) FAIL("%s", R.why.c_str());
  R.gather();
  const dsa::EncOrder *clouds = R.clouds();
  part_at = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    const uint32_t s0 = L.first_stream[i], m = (uint32_t)want_kept[i].size();
    if (clouds[i].m != m) FAIL("case %u (%u points): the record has %u voxels, the host coder %u", i, c.n, clouds[i].m, m);
    const uint32_t *kept = (const uint32_t *)(arena + dsa::ord_kept(clouds[i])), *row_entries = (const uint32_t *)(arena + clouds[i].cells);
    const std::vector<uint32_t> &entries = part_cells ? want_lod_cells[i] : want_cells[i];       // (the levels turn row_entries into lod order)
    for (uint32_t j = 0; j < m; ++j) if (kept[j] != want_kept[i][j]) FAIL("case %u (%u points): entry %u carries row %u, the host coder keeps %u", i, c.n, j, kept[j], want_kept[i][j]);
    for (uint32_t r = 0; r < c.n; ++r) if (row_entries[r] != entries[r]) FAIL("case %u (%u points): row %u lies in entry %u, the host coder says %u", i, c.n, r, row_entries[r], entries[r]);
    std::vector<uint32_t> rows(m, 0);
    for (uint32_t r = 0; r < c.n; ++r) ++rows[want_cells[i][r]];
    // every count region holds the rows of every voxel, once
    if (per_cloud) { const uint32_t *mc = (const uint32_t *)(arena + L.means[L.mean_pass.clouds[i].first].cnt); for (uint32_t j = 0; j < m; ++j) if (mc[j] != rows[j]) FAIL("case %u: the means counted %u rows of voxel %u, it has %u", i, mc[j], j, rows[j]); }
    if (beside) { const uint32_t *cnt = (const uint32_t *)(arena + L.normals[i].cnt); for (uint32_t j = 0; j < m; ++j) if (cnt[j] != rows[j]) FAIL("case %u: the normals counted %u rows of voxel %u, it has %u", i, cnt[j], j, rows[j]); }
    std::vector<int32_t> want[STREAMS];                         // the integers behind the stage
    for (uint32_t k = 0; k < STREAMS; ++k) {
      const dsa::EncStream &S = R.records[s0 + k];
      const uint32_t nc = S.nc;
      want[k] = k == 0 ? coded[i] : given[k][i];
      if (k == 0) for (size_t x = 0; x < want[k].size(); ++x) if (want[k][x] != given[k][i][x]) ++moved;
      std::vector<int32_t> cell;
      if (k == 1 && beside) synth::merge_mean_normals(given[k][i].data(), c.n, octa.q, want_cells[i], m, cell);
      if (k == 3 && beside) synth::merge_means(given[k][i].data(), c.n, (int)nc, want_cells[i], m, cell);
      if (k == 4 && beside) synth::merge_votes(given[k][i].data(), c.n, (int)nc, want_cells[i], m, cell);
      for (uint32_t j = 0; !cell.empty() && j < m; ++j) for (uint32_t q = 0; q < nc; ++q) want[k][(size_t)nc * kept[j] + q] = cell[(size_t)nc * j + q];
      const int32_t *vals = (const int32_t *)(arena + S.vals), *dst = (const int32_t *)(arena + S.d);
      for (size_t x = 0; x < want[k].size(); ++x) if (vals[x] != want[k][x]) FAIL("case %u stream %u: integer %zu of row %zu is %d, the host coder says %d", i, k, x % nc, x / nc, vals[x], want[k][x]);
      if (!part_cells && S.nv != m) FAIL("case %u: nv of stream %u is %u, %u voxels", i, k, S.nv, m);
      for (uint32_t j = 0; !part_cells && j < m; ++j) for (uint32_t q = 0; q < nc; ++q)
        if (dst[(size_t)nc * j + q] != want[k][(size_t)nc * kept[j] + q]) FAIL("case %u stream %u: entry %u does not carry what row %u holds", i, k, j, kept[j]);
    }
    if (part_cells) {                                          // the slots of the levels: lod rows, ranges, levels and boxes, and in d of every slot what its rows hold behind the passes
      const uint32_t *lod = (const uint32_t *)(arena + clouds[i].lod_rows);
      for (uint32_t j = 0; j < m; ++j) if (lod[j] != want_lod[i][j]) FAIL("case %u (%u points): lod entry %u is row %u, the host coder says %u", i, c.n, j, lod[j], want_lod[i][j]);
      for (uint32_t l : want_levels[i]) if (l >= levels) FAIL("case %u: a level %u of %u", i, l, levels);
      uint64_t parts_seen = 0, empty_seen = 0;
      auto entry = [&](uint32_t p, uint32_t e, uint32_t r) {
        for (uint32_t k = 0; k < STREAMS; ++k) {
          const dsa::EncStream &S = R.laid[s0 + STREAMS * p + k];
          if (memcmp((const int32_t *)(arena + S.d) + (size_t)S.nc * e, want[k].data() + (size_t)S.nc * r, 4ull * S.nc) != 0) return false;
        }
        return true;
      };
      if (!R.slots_sized(i, want_ranges[i], &want_levels[i], want_lod[i], want_min[i], want_max[i], part_at, parts_seen, empty_seen, entry)) FAIL("%s", R.why.c_str());
      if (parts_seen == 0) FAIL("case %u: no part seen", i);
    }
    points += c.n; voxels += m;
  }
  for (size_t s = 0; !part_cells && s < R.records.size(); ++s) if (!R.same_beyond(s, false)) FAIL("stream record %zu changed beyond nv", s);
  R.unpoison();
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: encvoxel_host <cases.bin>\n"); return 2; }
  std::vector<In> cases;
  if (!read_cases(argv[1], 5, false, cases)) return 2;
  for (const In &c : cases) {
    const uint32_t lod = c.more[1] & 255u, vb = c.more[1] >> 8;
    if (c.more[0] > 0x7FFFFFFFu || (c.more[0] == 0) != (lod == 0) || vb < 1 || vb > c.bits || lod > vb) return 2;
  }
  uint32_t chunks = 0;
  uint64_t points = 0, voxels = 0, moved = 0;
  std::map<std::pair<std::pair<uint32_t, uint32_t>, uint32_t>, std::vector<const In *>> groups;      // (bits, part_cells, lod_base_bits | voxel_bits << 8): one request
  for (const In &c : cases) groups[{{c.bits, c.more[0]}, c.more[1]}].push_back(&c);
  for (const auto &g : groups) {
    for (uint32_t point = 0; point < 3; ++point)
      for (int beside = 0; beside < 2; ++beside)
        for (int backwards = 0; backwards < 2; ++backwards)
          if (run(g.second, g.first.first.first, g.first.second >> 8, point, g.first.first.second, g.first.second & 255u, beside != 0, backwards != 0, points, voxels, moved) != 0) return 1;
    ++chunks;
  }
  printf("encvoxel: %u cases in %u chunks kept as the host coder keeps them, the three rules alone and beside a mean, a vote and normals, forwards and backwards (%llu points, %llu voxels, %llu position integers moved)\n",
         (uint32_t)cases.size(), chunks, (unsigned long long)points, (unsigned long long)voxels, (unsigned long long)moved);
  return 0;
}
