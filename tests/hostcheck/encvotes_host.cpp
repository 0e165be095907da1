// tests/hostcheck/encvotes_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The encoder's vote steps (draco-sharp_amd/csrc/dsa_encode_order.h: k_enc_vote_count in its serial form, k_enc_vote_best and
// k_enc_vote_store as they stand) compiled for the host with AddressSanitizer + UBSan and run thread by thread by the product's launch
// sequence for a chunk with vote_attributes != 0 (enc_order_stage: the sort, the merge, the means where the request has them, the
// zeroing of the tables, counts and values, the votes, and whatever the product runs behind them for the request -- with part_cells
// and lod_base_bits the levels, which turn row_entries into lod order, the part sizes and the part boxes) in the arena the product's
// layout hands out for such a chunk (enc_layout_sequential: stream records, order records, the EncVote / EncCellStreams records, the
// tile list and every region are the library's own; encorder_common.h has the harness) -- once forwards, once backwards, so that the
// tiles arrive at the tables in another order and the slots are placed differently -- against the host coder (dsa_encode_host.h:
// synth::merge_points, synth::merge_votes, synth::merge_means), with which the kernels share nothing: at every kept row of the voted
// stream the winner of its cell, every other integer as it was, and not one access outside a region (the arena's gaps are poisoned).
// Tables, counts and values are filled with a pattern and poisoned until the product's one memset range is zeroed.  The slots must
// count every row once and hold one slot per distinct (cell, tuple).  The accesses of k_enc_gather are made in its place.
// Every cloud carries texture coordinates (stream 1, two components, out of fifteen signed pairs so that ties are common: voted), a
// generic attribute (stream 2, three bytes: not voted -- three components -- and in every second run averaged, the two masks side
// by side) and a listed uint8 label (stream 3, one component out of four values: voted, the cloud's second record, blockIdx.y = 1).
// Here only, one more run gives the first table of one cloud deliberately too few slots: EncVote::full must be set for it and for
// no other, and no slot beyond the few may be written.  Nothing here is linked into the product.
//
//   encvotes_host <cases.bin>   file: u32 count, then per case u32 n, bits, has_grid, part_cells, lod_base_bits (both 0: neither);
//                               f32 pos[3 n]; with a grid f32 origin[3], range
#include <set>
#include <tuple>

#include "encorder_common.h"

#define FAIL(...) do { fprintf(stderr, "bits %u, part_cells %u, lod_base_bits %u, mean mask 0x%x, %s%s: ", bits, part_cells, lod_bits, mean_mask, backwards ? "backwards" : "forwards", starve ? ", a starved table" : ""); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

static const uint32_t VOTE_MASK = 0xAu, STARVED_SLOTS = 3u, STREAMS = 4u;
static const uint32_t VOTED[2] = {1u, 3u};                     // the voted streams of a cloud, in the order of its records
static const uint32_t NC[STREAMS] = {3u, 2u, 3u, 1u};

static uint32_t mix(uint32_t x) { x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16; return x; }
// the integer of row r, component c of stream k of cloud i: stream 1 one of 5 x 3 signed pairs, stream 2 a byte, stream 3 one of four labels
static int32_t designed(uint32_t i, uint32_t k, uint32_t r, uint32_t c) {
  const uint32_t h = mix(r * 8u + c + 0x9E3779B9u * (i + 1u) + 77u * k);
  return k == 1 ? (c == 0 ? (int32_t)(h % 5u) - 2 : (int32_t)(h % 3u) - 1) : k == 3 ? (int32_t)(h % 4u) + 250 : (int32_t)(h & 255u);
}
typedef std::set<std::tuple<uint32_t, int32_t, int32_t>> Pairs;
// the distinct (cell, tuple) pairs of a stream of nc <= 2 components
static Pairs pairs_of(const std::vector<uint32_t> &cells, const std::vector<int32_t> &q, uint32_t nc) {
  Pairs out;
  for (size_t r = 0; r < cells.size(); ++r) out.insert(std::make_tuple(cells[r], q[nc * r], nc == 2 ? q[nc * r + 1] : 0));
  return out;
}
// the cases `which` as one chunk of a request of point clouds; starve: the first cloud with more than STARVED_SLOTS (cell, tuple)
// pairs gets a table of STARVED_SLOTS slots
static int run(const std::vector<const In *> &which, uint32_t bits, uint32_t part_cells, uint32_t lod_bits, uint32_t mean_mask, bool backwards, bool starve, uint64_t &points, uint64_t &cells, uint64_t &ties) {
  Run R;
  Ask ask;
  ask.bits = bits; ask.merge = true; ask.mean_mask = mean_mask; ask.vote_mask = VOTE_MASK; ask.listed = ask.label = true; ask.part_cells = part_cells; ask.lod_base_bits = lod_bits;
  if (!R.begin(which, ask)) FAIL("%s", R.why.c_str());
  const EncLayout &L = R.L();
  const uint32_t n = R.n;
  uint8_t *arena = R.arena;
  if (!R.rq.merged() || !R.rq.votes() || R.rq.means() != (mean_mask != 0) || R.rq.lod() != (part_cells != 0)) FAIL("the request is not one with votes");
  if (L.vote_pass.clouds.size() != n || L.votes.size() != 2ull * n || L.vote_pass.stream.size() != 2ull * n || L.vote_pass.most != 2u) FAIL("%zu vote records for %u clouds", L.votes.size(), n);
  if (!R.sized(L.vote_pass.clouds_at, sizeof(dsa::EncCellStreams) * n) || !R.sized(L.vote_pass.records_at, sizeof(dsa::EncVote) * 2ull * n)) FAIL("the vote records are not among the uploads");
  if (L.vote_zero_at < L.input_bytes || L.vote_zero_at + L.vote_zero_bytes != L.total_bytes || L.vote_zero_at < L.mean_zero_at + L.mean_zero_bytes) FAIL("tables, counts and values are not the end of the arena, behind the means'");
  std::vector<std::vector<uint32_t>> want_kept(n), want_cells(n);
  std::vector<std::vector<int32_t>> given[STREAMS];           // per stream and cloud: the integers as they come in
  for (auto &g : given) g.resize(n);
  uint32_t starved = DSA_INVALID;
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    const dsa::EncOrder &O = L.ord[i];
    const dsa::EncCellStreams &VC = L.vote_pass.clouds[i];
    const uint32_t s0 = L.first_stream[i];
    if (O.n != c.n || O.merge != 1 || O.stream0 != s0 || O.streams != STREAMS || O.cells == 0) FAIL("case %u: order record", i);
    if (VC.first != 2u * i || VC.count != 2u) FAIL("case %u: vote record of the cloud", i);
    for (uint32_t v = 0; v < 2u; ++v) {
      const dsa::EncVote &V = L.votes[2u * i + v];
      const dsa::EncStream &S = L.streams[s0 + VOTED[v]];
      if (L.vote_pass.stream[2u * i + v] != s0 + VOTED[v] || S.nc != NC[VOTED[v]] || V.nc != S.nc || V.vals != S.vals || V.cap < 2u * c.n || V.full != 0u || !R.sized(S.vals, 4ull * S.nc * c.n)) FAIL("case %u: vote record of stream %u", i, VOTED[v]);
      if (!R.sized(V.table, 8ull * V.cap) || !R.sized(V.best_cnt, 4ull * c.n) || !R.sized(V.best_val, 8ull * c.n) || V.table < L.vote_zero_at || V.best_cnt < L.vote_zero_at || V.best_val < L.vote_zero_at) FAIL("case %u: the regions of the vote of stream %u", i, VOTED[v]);
      if (V.cap > 2u * c.n + 64u) FAIL("case %u: %u slots for %u points: a small cloud pays for a tile", i, V.cap, c.n);
    }
    R.write_positions(i);
    given[0][i].assign((const int32_t *)(arena + O.vals), (const int32_t *)(arena + O.vals) + 3ull * c.n);
    for (uint32_t k = 1; k < STREAMS; ++k) {
      const uint32_t nc = NC[k];
      if (L.streams[s0 + k].nc != nc) FAIL("case %u: stream %u has %u components", i, k, L.streams[s0 + k].nc);
      given[k][i].resize((size_t)nc * c.n);
      for (uint32_t r = 0; r < c.n; ++r) for (uint32_t q = 0; q < nc; ++q) given[k][i][(size_t)nc * r + q] = designed(i, k, r, q);
      memcpy(arena + L.streams[s0 + k].vals, given[k][i].data(), 4ull * nc * c.n);
    }
    synth::merge_points(c.pos.data(), c.n, (int)bits, R.grid(i), want_kept[i], want_cells[i]);
    if (starve && starved == DSA_INVALID && pairs_of(want_cells[i], given[1][i], 2u).size() > STARVED_SLOTS) { starved = i; ((dsa::EncVote *)(arena + L.vote_pass.records_at))[2u * i].cap = STARVED_SLOTS; }
  }
  if (starve && starved == DSA_INVALID) FAIL("no cloud to starve");
  R.poison();
  if (!R.stage(backwards)) FAIL("%s", R.why.c_str());
  R.gather();
  const dsa::EncOrder *clouds = R.clouds();
  const dsa::EncVote *votes = (const dsa::EncVote *)(arena + L.vote_pass.records_at);
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    const uint32_t s0 = L.first_stream[i], m = (uint32_t)want_kept[i].size();
    if (clouds[i].m != m) FAIL("case %u (%u points): the record has %u cells, the host coder %u", i, c.n, clouds[i].m, m);
    const uint32_t *kept = (const uint32_t *)(arena + dsa::ord_kept(clouds[i]));
    for (uint32_t j = 0; j < m; ++j) if (kept[j] != want_kept[i][j]) FAIL("case %u (%u points): entry %u carries row %u, the host coder keeps %u", i, c.n, j, kept[j], want_kept[i][j]);
    if (i == starved) {                                        // the flag, and nothing written beyond the few slots
      const uint32_t *table = (const uint32_t *)(arena + votes[2u * i].table);
      if (votes[2u * i].full == 0u) FAIL("case %u: a table of %u slots was not found full", i, STARVED_SLOTS);
      if (votes[2u * i + 1u].full != 0u) FAIL("case %u: the table of the cloud's other stream was found full", i);
      for (uint64_t x = 2ull * STARVED_SLOTS; x < 2ull * L.votes[2u * i].cap; ++x) if (table[x] != 0u) FAIL("case %u: word %llu beyond the %u slots of the table was written", i, (unsigned long long)x, STARVED_SLOTS);
      continue;
    }
    for (uint32_t v = 0; v < 2u; ++v) {                        // the slots: every row counted once, one slot per distinct (cell, tuple), each holding a row of its own pair
      const dsa::EncVote &V = votes[2u * i + v];
      const uint32_t *table = (const uint32_t *)(arena + V.table);
      const std::vector<int32_t> &q = given[VOTED[v]][i];
      if (V.full != 0u) FAIL("case %u: the table of %u slots for %u points was found full", i, V.cap, c.n);
      const Pairs pairs = pairs_of(want_cells[i], q, V.nc);
      Pairs seen;
      uint64_t rows = 0;
      for (uint32_t s = 0; s < V.cap; ++s) {
        const uint32_t rep = table[2ull * s], count = table[2ull * s + 1u];
        if (rep == 0u) { if (count != 0u) FAIL("case %u: slot %u is empty and counts %u rows", i, s, count); continue; }
        if (rep - 1u >= c.n || count == 0u) FAIL("case %u: slot %u holds row %u and %u rows", i, s, rep - 1u, count);
        if (!seen.insert(std::make_tuple(want_cells[i][rep - 1u], q[(size_t)V.nc * (rep - 1u)], V.nc == 2u ? q[2ull * (rep - 1u) + 1] : 0)).second) FAIL("case %u: slot %u holds a pair a slot before it holds", i, s);
        rows += count;
      }
      if (rows != c.n || seen != pairs) FAIL("case %u stream %u: %llu rows counted in %zu slots, the cloud has %u rows and %zu pairs", i, VOTED[v], (unsigned long long)rows, seen.size(), c.n, pairs.size());
      ties += pairs.size() - m;
    }
    std::vector<int32_t> want[STREAMS];                             // the integers behind the stage: the winner (the mean) at every kept row of the voted (the averaged) stream
    for (uint32_t k = 0; k < STREAMS; ++k) {
      const dsa::EncStream &S = R.records[s0 + k];
      const uint32_t nc = S.nc;
      want[k] = given[k][i];
      std::vector<int32_t> cell;
      if (k == 1 || k == 3) synth::merge_votes(given[k][i].data(), c.n, (int)nc, want_cells[i], m, cell);
      if (k == 2 && mean_mask) synth::merge_means(given[k][i].data(), c.n, (int)nc, want_cells[i], m, cell);
      for (uint32_t j = 0; !cell.empty() && j < m; ++j) for (uint32_t q = 0; q < nc; ++q) want[k][(size_t)nc * kept[j] + q] = cell[(size_t)nc * j + q];
      const int32_t *vals = (const int32_t *)(arena + S.vals), *dst = (const int32_t *)(arena + S.d);
      for (size_t x = 0; x < want[k].size(); ++x) if (vals[x] != want[k][x]) FAIL("case %u stream %u: integer %zu of row %zu is %d, the host coder says %d", i, k, x % nc, x / nc, vals[x], want[k][x]);
      if (!part_cells && S.nv != m) FAIL("case %u: nv of stream %u is %u, %u cells", i, k, S.nv, m);
      for (uint32_t j = 0; !part_cells && j < m; ++j) for (uint32_t q = 0; q < nc; ++q)
        if (dst[(size_t)nc * j + q] != want[k][(size_t)nc * kept[j] + q]) FAIL("case %u stream %u: entry %u does not carry what row %u holds", i, k, j, kept[j]);
    }
    points += c.n; cells += m;
  }
  for (size_t s = 0; !part_cells && s < R.records.size(); ++s) if (!R.same_beyond(s, false)) FAIL("stream record %zu changed beyond nv", s);
  R.unpoison();
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: encvotes_host <cases.bin>\n"); return 2; }
  std::vector<In> cases;
  if (!read_cases(argv[1], 5, false, cases)) return 2;
  for (const In &c : cases) if (c.more[0] > 0x7FFFFFFFu || (c.more[0] == 0) != (c.more[1] == 0) || c.more[1] > c.bits) return 2;
  uint32_t chunks = 0;
  uint64_t points = 0, cells = 0, ties = 0, none = 0;
  std::map<std::pair<std::pair<uint32_t, uint32_t>, uint32_t>, std::vector<const In *>> groups;      // (bits, part_cells, lod_base_bits): one request
  for (const In &c : cases) groups[{{c.bits, c.more[0]}, c.more[1]}].push_back(&c);
  bool starved = false;
  for (const auto &g : groups) {
    for (uint32_t mean_mask : {0u, 4u})
      for (int backwards = 0; backwards < 2; ++backwards) if (run(g.second, g.first.first.first, g.first.first.second, g.first.second, mean_mask, backwards != 0, false, points, cells, ties) != 0) return 1;
    uint64_t total = 0;
    for (const In *c : g.second) total += c->n;
    if (!starved && total > 64) { if (run(g.second, g.first.first.first, g.first.first.second, g.first.second, 0u, false, true, none, none, none) != 0) return 1; starved = true; }
    ++chunks;
  }
  if (!starved) { fprintf(stderr, "no chunk with a cloud to starve\n"); return 1; }
  printf("encvotes: %u cases in %u chunks voted as the host coder votes, with and without a mean beside, forwards and backwards (%llu points, %llu cells, %llu pairs beyond one a cell), one table starved\n",
         (uint32_t)cases.size(), chunks, (unsigned long long)points, (unsigned long long)cells, (unsigned long long)ties);
  return 0;
}
