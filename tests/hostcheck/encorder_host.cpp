// tests/hostcheck/encorder_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The encoder's point-order kernels (draco-sharp_amd/csrc/dsa_encode_order.h: keys, the segmented radix sort's histogram, scan and
// scatter, rank, the faces through rank) compiled for the host with AddressSanitizer + UBSan and run thread by thread by the
// product's launch sequence (enc_order_stage) in the arena the product's layout hands out (enc_layout_sequential with
// EncRequest::point_order: records, tile list and every region are the library's own; encorder_common.h has the harness) -- once
// forwards, once backwards -- against the host coder's order (dsa_encode_host.h: synth::point_order) on the same points: the same
// permutation in the region every stream of the cloud reads as its entry -> row map, its inverse, the same remapped faces, and not
// one access outside a region (the arena's gaps are poisoned).  The clouds of one position_bits are one chunk, so that the segmented
// passes meet every size side by side.  Nothing here is linked into the product.
//
//   encorder_host <cases.bin>   file: u32 count, then per case u32 n, bits, has_grid, F; f32 pos[3 n]; with a grid f32 origin[3],
//                               range; u32 faces[3 F]
#include "encorder_common.h"

#define FAIL(...) do { fprintf(stderr, "bits %u, %s, %s: ", bits, compressed ? "compressed" : (is_mesh ? "raw" : "cloud"), backwards ? "backwards" : "forwards"); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

// the cases `which` as one chunk of a request: point clouds, or meshes with raw / compressed indices
static int run(const std::vector<const In *> &which, uint32_t bits, bool is_mesh, bool compressed, bool backwards) {
  Run R;
  Ask ask;
  ask.bits = bits; ask.is_mesh = is_mesh; ask.compressed = compressed;
  if (!R.begin(which, ask)) FAIL("%s", R.why.c_str());
  const EncLayout &L = R.L();
  const uint32_t n = R.n;
  uint64_t tiles = 0;
  for (const dsa::EncOrder &O : L.ord) tiles += O.tiles;
  if (L.ord_tiles.size() != tiles) FAIL("%zu tiles listed, %llu in the records", L.ord_tiles.size(), (unsigned long long)tiles);
  std::vector<std::vector<uint32_t>> want(n);
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    const dsa::EncOrder &O = L.ord[i];
    const dsa::EncStream &S = L.streams[L.first_stream[i]];
    const uint32_t F = (uint32_t)(c.faces.size() / 3);
    if (O.n != c.n || O.bits != bits || O.tiles != (c.n + ORD_TILE - 1) / ORD_TILE || O.vals != S.vals || O.last != (L.ord_passes & 1)) FAIL("case %u: order record", i);
    if (!R.sized(O.vals, 12ull * c.n) || !R.sized(O.key[0], 8ull * c.n) || !R.sized(O.key[1], 8ull * c.n) || !R.sized(O.row[0], 4ull * c.n) || !R.sized(O.row[1], 4ull * c.n) ||
        !R.sized(O.hist, 1024ull * O.tiles) || (is_mesh && !R.sized(O.rank, 4ull * c.n)) || (!is_mesh && O.rank != 0)) FAIL("case %u: order regions too small", i);
    if (S.linear != 0 || S.e2v != dsa::ord_sorted(O).row || S.d == S.vals || !R.sized(S.d, 12ull * c.n)) FAIL("case %u: the streams do not read the order", i);
    if (compressed != (O.count != 0) || (compressed && (O.count != 3 * F || O.faces >= L.input_bytes || !R.sized(O.faces, (O.narrow ? 2ull : 4ull) * O.count)))) FAIL("case %u: faces of the order record", i);
    R.write_positions(i);
    synth::point_order(c.pos.data(), c.n, (int)bits, R.grid(i), want[i]);
  }
  R.poison();
  if (!R.stage(backwards, L.max_count ? std::max(1u, std::min(4u, (L.max_count + 1023u) / 1024u)) : 0u)) FAIL("%s", R.why.c_str());
  for (uint32_t i = 0; i < n; ++i) {
    const In &c = *which[i];
    const dsa::EncOrder &O = L.ord[i];
    const uint32_t *perm = (const uint32_t *)(R.arena + L.streams[L.first_stream[i]].e2v);
    for (uint32_t e = 0; e < c.n; ++e) if (perm[e] != want[i][e]) FAIL("case %u (%u points): entry %u carries row %u, the host coder's order has %u", i, c.n, e, perm[e], want[i][e]);
    if (!is_mesh) continue;
    const uint32_t *rank = (const uint32_t *)(R.arena + O.rank);
    for (uint32_t e = 0; e < c.n; ++e) if (rank[want[i][e]] != e) FAIL("case %u: rank of row %u", i, want[i][e]);
    for (uint32_t k = 0; compressed && k < c.faces.size(); ++k) {
      const uint32_t got = O.narrow ? (uint32_t)((const uint16_t *)(R.arena + O.faces))[k] : ((const uint32_t *)(R.arena + O.faces))[k];
      if (got != rank[c.faces[k]]) FAIL("case %u: corner %u is %u, rank[%u] = %u", i, k, got, c.faces[k], rank[c.faces[k]]);
    }
  }
  R.unpoison();
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: encorder_host <cases.bin>\n"); return 2; }
  std::vector<In> cases;
  if (!read_cases(argv[1], 4, true, cases)) return 2;
  uint32_t chunks = 0;
  for (uint32_t bits = 1; bits <= 20; ++bits)
    for (int kind = 0; kind < 3; ++kind) {                     // point clouds; meshes with raw indices; with compressed indices
      std::vector<const In *> which;
      for (const In &c : cases) if (c.bits == bits && (kind == 0 || !c.faces.empty())) which.push_back(&c);
      if (which.empty()) continue;
      for (int backwards = 0; backwards < 2; ++backwards) if (run(which, bits, kind != 0, kind == 2, backwards != 0) != 0) return 1;
      ++chunks;
    }
  printf("encorder: %u cases in %u chunks ordered as the host coder orders them, forwards and backwards\n", (uint32_t)cases.size(), chunks);
  return 0;
}
