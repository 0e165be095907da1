// tests/hostcheck/encseq_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The index kernel of the sequential encoder (draco-sharp_amd/csrc/dsa_encode_seqidx.h: the three phases of k_enc_seq_indices)
// compiled for the host with AddressSanitizer + UBSan and run thread by thread, block by block, against the host coder
// (dsa_encode_host.h: sequential_index_symbols + symbol_stats with nc = 1) on the same faces: symbols, bit lengths, maximum, both
// histograms and the sum of the bit lengths, and not one access outside a mesh's arrays (the arena's gaps are poisoned).  Every
// mesh is run with its faces as 32-bit indices and, when every index fits, again as the 16-bit upload.  Nothing here is linked
// into the product.
//
//   encseq_host <meshes.bin> <blocks>    file: u32 count, then per mesh u32 nv, u32 nf, u32 faces[3 nf]
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../draco-sharp_amd/csrc/dsa_common.h"
#include "../../draco-sharp_amd/csrc/dsa_encode_host.h"

#include "hip_on_host.h"

#include "../../draco-sharp_amd/csrc/dsa_encode_seqidx.h"

struct IdxStream {                 // what the phases read and write of an EncStream
  uint64_t syms, bl, hist_raw;
  uint32_t hist_cap, max_value, overflow;
  unsigned long long total_bl;
  uint32_t hist_tag[33];
};

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: encseq_host <meshes.bin> <blocks>\n"); return 2; }
  const uint32_t blocks = (uint32_t)atoi(argv[2]);
  if (blocks < 1) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  struct In { uint32_t nv, nf; std::vector<uint32_t> faces; };
  std::vector<In> meshes(count);
  for (auto &m : meshes) {
    if (fread(&m.nv, 4, 1, f) != 1 || fread(&m.nf, 4, 1, f) != 1) return 2;
    m.faces.resize((size_t)3 * m.nf);
    if (m.nf && fread(m.faces.data(), 4, m.faces.size(), f) != m.faces.size()) return 2;
    for (uint32_t x : m.faces) if (x >= m.nv) { fprintf(stderr, "index out of range in the input file\n"); return 2; }
  }
  fclose(f);
  // ---- the arena, laid out like dsa_encode_sequential.h lays a chunk out, every gap poisoned: each mesh once per upload width
  struct Run { uint32_t mesh; dsa::EncSeqIdx X; };
  std::vector<Run> runs;
  std::vector<IdxStream> streams;
  uint64_t cur = 0;
  std::vector<std::pair<uint64_t, uint64_t>> regions;
  auto take = [&](uint64_t bytes) { cur = (cur + 255) & ~255ull; cur += 64; const uint64_t at = cur; regions.push_back({at, bytes}); cur += bytes + 64; return at; };
  for (uint32_t i = 0; i < count; ++i)
    for (int narrow = 0; narrow < 2; ++narrow) {
      if (narrow && meshes[i].nv > 65536) continue;
      const uint32_t n = 3u * meshes[i].nf;
      Run r;
      memset(&r.X, 0, sizeof(r.X));
      r.mesh = i; r.X.count = n; r.X.narrow = (uint32_t)narrow; r.X.stream = (uint32_t)streams.size();
      r.X.faces = take((narrow ? 2ull : 4ull) * n);
      IdxStream S;
      memset(&S, 0, sizeof(S));
      S.hist_cap = 2u * meshes[i].nv;
      S.hist_raw = take(4ull * S.hist_cap); S.syms = take(4ull * n); S.bl = take(n);
      runs.push_back(r);
      streams.push_back(S);
    }
  std::vector<uint8_t> arena_store(cur + 256, 0);
  uint8_t *arena = arena_store.data();
  for (const Run &r : runs) {
    const In &m = meshes[r.mesh];
    if (r.X.narrow) { uint16_t *d = (uint16_t *)(arena + r.X.faces); for (size_t k = 0; k < m.faces.size(); ++k) d[k] = (uint16_t)m.faces[k]; }
    else if (!m.faces.empty()) memcpy(arena + r.X.faces, m.faces.data(), 4 * m.faces.size());
  }
  ASAN_POISON_MEMORY_REGION(arena, arena_store.size());
  for (auto &rg : regions) ASAN_UNPOISON_MEMORY_REGION(arena + rg.first, rg.second);
  // ---- the kernel: per (block, mesh) clear | count | flush, a barrier between them
  static dsa::SeqIdxShared sh;
  for (const Run &r : runs)
    for (uint32_t b = 0; b < blocks; ++b) {
      if (b * SEQ_BLOCK >= r.X.count) continue;
      IdxStream &S = streams[r.X.stream];
      for (uint32_t t = 0; t < SEQ_BLOCK; ++t) dsa::seq_idx_clear(sh, t);
      for (uint32_t t = 0; t < SEQ_BLOCK; ++t) dsa::seq_idx_count(sh, arena, r.X, S, b, blocks, t);
      for (uint32_t t = 0; t < SEQ_BLOCK; ++t) dsa::seq_idx_flush(sh, arena, S, t);
    }
  // ---- against the host coder
  uint32_t narrow_runs = 0, lds_only = 0, beyond_lds = 0, ragged = 0;
  for (const Run &r : runs) {
    const In &m = meshes[r.mesh];
    const IdxStream &S = streams[r.X.stream];
    std::vector<uint32_t> want, want_bl;
    synth::sequential_index_symbols(m.faces.data(), m.faces.size(), want);
    synth::SymbolStats st;
    synth::symbol_stats(want, 1, st, &want_bl);
    const uint32_t *syms = (const uint32_t *)(arena + S.syms), *hist = (const uint32_t *)(arena + S.hist_raw);
    const uint8_t *bl = arena + S.bl;
    auto bad = [&](const char *what) { fprintf(stderr, "mesh %u (%s faces): %s differs\n", r.mesh, r.X.narrow ? "16-bit" : "32-bit", what); return 1; };
    if (S.overflow) return bad("overflow flag");
    for (size_t k = 0; k < want.size(); ++k) { if (syms[k] != want[k]) return bad("symbol"); if (bl[k] != want_bl[k]) return bad("bit length"); }
    if (S.max_value != st.max_value) return bad("maximum");
    if (S.total_bl != st.total_bl) return bad("total_bl");
    for (uint32_t b = 0; b < 33; ++b) if (S.hist_tag[b] != st.tag_freq[b]) return bad("bit-length histogram");
    for (uint32_t v = 0; v < S.hist_cap; ++v) if ((uint64_t)hist[v] != (v < st.raw_freq.size() ? st.raw_freq[v] : 0)) return bad("raw histogram");
    narrow_runs += r.X.narrow;
    if (S.hist_cap <= SEQ_LDS_BINS) ++lds_only; else if (st.max_value >= SEQ_LDS_BINS) ++beyond_lds;
    if (r.X.count % SEQ_BLOCK) ++ragged;
  }
  printf("encseq: %zu runs of %u meshes alike (%u as 16-bit uploads, %u within the LDS histogram, %u with symbols beyond it, %u not a multiple of the block)\n",
         runs.size(), count, narrow_runs, lds_only, beyond_lds, ragged);
  return 0;
}
