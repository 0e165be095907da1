// tests/hostcheck/needs_host.cpp
// The host side of the pruned decode schedule as a stand-alone program (tests/test_needs_cpu.py builds it with
// -fsanitize=address,undefined): the needs walk of draco-sharp_amd/csrc/dsa_host_parse.h, the need bits of dsa_needs.h and the
// "needs covered by launched" function k_seal uses -- the library's own headers, no HIP.
//   needs_host mask FILE...          one line per stream: status, walk_ok, the mask without / with OS_FLAG, section offsets
//   needs_host cover N L [N L ...]   needs_covered(N, L) for every pair, one 0 / 1 per line
//   needs_host corrupt FILE SEED     every truncation of the stream and one flipped bit per byte (each copy in a heap block of
//                                    exactly its length, so that a read past its end is an ASan report) through the walk
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../draco-sharp_amd/csrc/dsa_host_parse.h"

static const uint32_t kFlags = PW_FLAG | SYM_WIDE;      // the product schedule's launch flags (dsa_api.hip: kPruneFlags)

static std::vector<uint8_t> read_file(const char *path) {
  std::vector<uint8_t> d;
  FILE *f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  uint8_t buf[65536];
  size_t k;
  while ((k = fread(buf, 1, sizeof(buf), f)) > 0) d.insert(d.end(), buf, buf + k);
  fclose(f);
  return d;
}

// parse + placement + masks of one stream held in a heap block of exactly `len` bytes
struct Verdict { int status; bool walk_ok; uint32_t needs[2]; HostMesh h; };
static Verdict walk(const uint8_t *src, size_t len) {
  uint8_t *exact = (uint8_t *)malloc(len ? len : 1);
  if (len) memcpy(exact, src, len);
  Verdict v;
  host_parse(exact, len, v.h);
  free(exact);
  v.status = v.h.status;
  v.walk_ok = v.h.walk_ok;
  if (v.h.status != 0) { v.h.faces = 0; v.h.enc_vertices = 0; v.h.split_symbols = 0; v.h.splits = 0; v.h.atts.clear(); v.h.general = false; }   // as build_batch does
  MeshLayout L;
  memset(&L, 0, sizeof(L));
  L.stream_len = (uint32_t)len;
  (void)layout_mesh(v.h, len, L, 0, 16);
  for (int k = 0; k < 2; ++k) v.needs[k] = host_mesh_needs(v.h, L, kFlags | (k ? OS_FLAG : 0u));
  return v;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  if (mode == "mask") {
    for (int i = 2; i < argc; ++i) {
      const std::vector<uint8_t> d = read_file(argv[i]);
      const Verdict v = walk(d.data(), d.size());
      printf("%d %d 0x%05x 0x%05x %u", v.status, v.walk_ok ? 1 : 0, v.needs[0], v.needs[1], v.h.off_attributes);
      for (const AttrDesc &a : v.h.walk) printf(" %u:%u:%u", a.off_table, a.off_rans, a.size_rans);
      printf("\n");
    }
    return 0;
  }
  if (mode == "cover") {
    for (int i = 2; i + 1 < argc; i += 2)
      printf("%d\n", dsa::needs_covered((uint32_t)strtoul(argv[i], nullptr, 0), (uint32_t)strtoul(argv[i + 1], nullptr, 0)) ? 1 : 0);
    return 0;
  }
  if (mode == "corrupt" && argc >= 4) {
    const std::vector<uint8_t> d = read_file(argv[2]);
    uint64_t rng = strtoull(argv[3], nullptr, 0) * 6364136223846793005ull + 1442695040888963407ull;
    const Verdict whole = walk(d.data(), d.size());
    // a cut or a flip the parse cannot see (inside a payload it steps over) leaves the mask as it was; one it can see may only
    // fail the parse, end the walk (every bit) or change what a table says -- never read outside the block
    size_t failed = 0, all_bits = 0, same = 0, other = 0;
    auto tally = [&](const Verdict &v) {
      if (v.status != 0) ++failed;
      else if (v.needs[0] == NEED_ALL) ++all_bits;
      else if (v.needs[0] == whole.needs[0]) ++same;
      else ++other;
      if (v.status != 0 && v.needs[0] != NEED_ALL) { fprintf(stderr, "a failed parse must ask for every kernel\n"); exit(1); }
    };
    const size_t step = d.size() > (64u << 10) ? d.size() / (64u << 10) + 1 : 1;
    for (size_t len = 0; len < d.size(); len += step) tally(walk(d.data(), len));
    std::vector<uint8_t> c = d;
    for (size_t at = 0; at < d.size(); at += step) {
      rng = rng * 6364136223846793005ull + 1442695040888963407ull;
      const uint8_t bit = (uint8_t)(1u << ((rng >> 33) & 7));
      c[at] ^= bit;
      tally(walk(c.data(), c.size()));
      c[at] ^= bit;
    }
    printf("%zu bytes: failed %zu, every-bit %zu, same-mask %zu, other-mask %zu\n", d.size(), failed, all_bits, same, other);
    return 0;
  }
  return 2;
}
