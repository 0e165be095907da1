// tests/hostcheck/encrepair_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The encoder's topology-repair kernels of the product (draco-sharp_amd/csrc/dsa_encode_repair.h: marks, corners by vertex, the
// per-edge matching, the break pass and the fan pass one lane per mesh) compiled for the host with AddressSanitizer + UBSan and run
// thread by thread, against the host coder's repair (dsa_encode_host.h: CornerTable::repair, the literal transcription of the
// reference's three passes) on the same faces: the same c2v', opposites, parents and counts, and not one access outside a mesh's
// arrays (the arena's gaps are poisoned).  GPU sanitizers are not available on the pool; a pass that leaves its arrays on the
// device can take the machine down.  Nothing here is linked into the product.
//
//   encrepair_host <meshes.bin> [counts]   file: u32 count, then per mesh u32 nv, u32 nf, u32 faces[3 nf]
//                                          counts: one line per mesh "i: V' isolated degenerate breaks"
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../draco-sharp_amd/csrc/dsa_common.h"
#include "../../draco-sharp_amd/csrc/dsa_types.h"
#include "../../draco-sharp_amd/csrc/dsa_encode_host.h"

#include "hip_on_host.h"

#include "../../draco-sharp_amd/csrc/dsa_encode_conn.h"
#include "../../draco-sharp_amd/csrc/dsa_encode_repair.h"

// (launch backwards: the lists of a vertex come out of the atomic counter in any order on the device)
int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: encrepair_host <meshes.bin> [counts]\n"); return 2; }
  const bool print_counts = argc > 2 && std::string(argv[2]) == "counts";
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
    for (uint32_t x : m.faces) if (x >= m.nv) { fprintf(stderr, "index out of range in the input file\n"); return 2; }      // (the library's host checks keep such a mesh from the device)
  }
  fclose(f);
  // ---- the arena, laid out like enc_stage_repair lays it out, every gap poisoned
  const uint32_t n = count;
  std::vector<dsa::EncRepair> recs(n);
  uint64_t cur = 0;
  std::vector<std::pair<uint64_t, uint64_t>> regions;
  auto take = [&](uint64_t bytes) { cur = (cur + 255) & ~255ull; cur += 64; const uint64_t at = cur; regions.push_back({at, bytes}); cur += bytes + 64; return at; };
  uint32_t maxf = 1;
  for (uint32_t i = 0; i < n; ++i) {
    dsa::EncRepair &R = recs[i];
    memset(&R, 0, sizeof(R));
    const uint64_t F = meshes[i].nf, V = meshes[i].nv;
    R.F = (uint32_t)F; R.V = (uint32_t)V;
    R.faces = take(12 * F); R.c2v = take(12 * F); R.opp = take(12 * F); R.parent = take(12 * F);
    R.voff = take(4 * (V + 1)); R.vcur = take(4 * V); R.vlist = take(12 * F);
    R.pend = take(3 * F); R.bvis = take(3 * F); R.cvis = take(3 * F); R.vvis = take(V); R.stamp = take(12 * V);
    maxf = std::max(maxf, meshes[i].nf);
  }
  std::vector<uint8_t> arena_store(cur + 256, 0);
  uint8_t *arena = arena_store.data();
  for (uint32_t i = 0; i < n; ++i) if (meshes[i].nf) memcpy(arena + recs[i].faces, meshes[i].faces.data(), 12ull * meshes[i].nf);
  ASAN_POISON_MEMORY_REGION(arena, arena_store.size());
  for (auto &rg : regions) ASAN_UNPOISON_MEMORY_REGION(arena + rg.first, rg.second);
  const uint32_t gx = std::max(1u, std::min(4u, (3u * maxf + 1023u) / 1024u));
  dsa::EncRepair *reps = recs.data();
  launch(dsa::k_enc_repair_mark, gx, n, 256, false, arena, reps, n);
  launch(dsa::k_enc_repair_offsets, n, 1, WAVE, false, arena, reps, n);
  launch(dsa::k_enc_repair_lists, gx, n, 256, true, arena, reps, n);           // (the lists in another order than the corners')
  launch(dsa::k_enc_repair_opposites, gx, n, 256, true, arena, reps, n);
  const uint32_t lanes = 5;                    // meshes to a wave
  launch(dsa::k_enc_repair_fans, (n + lanes - 1) / lanes, 1, WAVE, false, arena, reps, n, lanes);
  // ---- against the host coder's repair
  uint32_t alike = 0, bound = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const In &m = meshes[i];
    const dsa::EncRepair &R = recs[i];
    synth::CornerTable::Repaired want;
    synth::CornerTable::repair(m.faces.data(), m.nf, m.nv, want);
    if (print_counts) printf("%u: %u %u %u %u\n", i, want.num_vertices, want.isolated, want.degenerate, want.breaks);
    if (R.status == dsa::ENC_REPAIR_BOUND) { ++bound; continue; }                // (a face listed over and over: the device gives the mesh up, it never answers differently)
#define SAME(cond, what) do { if (!(cond)) { fprintf(stderr, "mesh %u: %s differ\n", i, what); return 1; } } while (0)
    SAME(R.status == dsa::ENC_REPAIR_OK, "status");
    SAME(R.num_vertices == want.num_vertices && R.isolated == want.isolated && R.degenerate == want.degenerate && R.breaks == want.breaks, "counts");
    SAME(m.nf == 0 || memcmp(arena + R.c2v, want.c2v.data(), 12ull * m.nf) == 0, "c2v'");
    SAME(m.nf == 0 || memcmp(arena + R.opp, want.opp.data(), 12ull * m.nf) == 0, "opposites");
    SAME(want.parent.size() == R.num_vertices - R.V && (want.parent.empty() || memcmp(arena + R.parent, want.parent.data(), 4ull * want.parent.size()) == 0), "parents");
    ++alike;
  }
  // ---- the repaired tables through the connectivity kernels, as the library lays them out: compacted faces, the opposites given
  // (k_enc_table_opposites is not launched), the walks, the operand entries, then the rows -- against the host coder's plan of the
  // same mesh in repair mode
  uint32_t walked = 0;
  {
    std::vector<dsa::EncConn> hc;
    std::vector<dsa::EncRepairRows> rows;
    std::vector<synth::CornerTable> tables(n);
    std::vector<uint32_t> mesh_of;
    std::vector<std::pair<uint64_t, uint64_t>> regions2;
    uint64_t cur2 = 0;
    auto take2 = [&](uint64_t bytes) { cur2 = (cur2 + 255) & ~255ull; cur2 += 64; const uint64_t at = cur2; regions2.push_back({at, bytes}); cur2 += bytes + 64; return at; };
    uint32_t maxf2 = 1;
    for (uint32_t i = 0; i < n; ++i) {
      const In &m = meshes[i];
      const dsa::EncRepair &R = recs[i];
      if (R.status != dsa::ENC_REPAIR_OK || R.degenerate >= m.nf || m.nv < 3) continue;
      synth::CornerTable::Repaired r;
      r.c2v.assign((const uint32_t *)(arena + R.c2v), (const uint32_t *)(arena + R.c2v) + 3ull * m.nf);
      r.opp.assign((const uint32_t *)(arena + R.opp), (const uint32_t *)(arena + R.opp) + 3ull * m.nf);
      r.parent.assign((const uint32_t *)(arena + R.parent), (const uint32_t *)(arena + R.parent) + (R.num_vertices - R.V));
      r.num_vertices = R.num_vertices; r.isolated = R.isolated; r.degenerate = R.degenerate; r.breaks = R.breaks;
      tables[i].from_repaired(r, m.faces.data(), m.nf, m.nv);
      const uint64_t F = tables[i].nf(), V = tables[i].nv();
      dsa::EncConn C;
      memset(&C, 0, sizeof(C));
      C.F = (uint32_t)F; C.V = (uint32_t)V; C.split_cap = (uint32_t)F; C.fail_key = 0xFFFFFFFFu;
      C.faces = take2(12 * F); C.opp = take2(12 * F); C.voff = take2(4 * (V + 1)); C.vcur = take2(4 * V); C.vlist = take2(12 * F); C.vcorner = take2(4 * V);
      C.vvis = take2(V); C.frec = take2(32 * F);
      C.stack = take2(4 * F); C.processed = take2(4 * F); C.init_corners = take2(4 * F);
      C.symbols = take2(F); C.start_bits = take2(F); C.splits = take2(12ull * C.split_cap);
      C.d2c = take2(4 * V); C.v2d = take2(4 * V); C.e2v = take2(4 * V); C.ops = take2(12 * V);
      dsa::EncRepairRows RR;
      memset(&RR, 0, sizeof(RR));
      RR.e2v = C.e2v; RR.row = take2(4 * V); RR.count = (uint32_t)V;
      hc.push_back(C); rows.push_back(RR); mesh_of.push_back(i);
      maxf2 = std::max(maxf2, C.F);
    }
    const uint32_t n2 = (uint32_t)hc.size();
    std::vector<uint8_t> store2(cur2 + 256, 0);
    uint8_t *arena2 = store2.data();
    for (uint32_t k = 0; k < n2; ++k) {
      const synth::CornerTable &t = tables[mesh_of[k]];
      memcpy(arena2 + hc[k].faces, t.c2v.data(), 4ull * t.c2v.size());
      memcpy(arena2 + hc[k].opp, t.opp.data(), 4ull * t.opp.size());
      memcpy(arena2 + rows[k].row, t.row.data(), 4ull * t.row.size());
    }
    ASAN_POISON_MEMORY_REGION(arena2, store2.size());
    for (auto &rg : regions2) ASAN_UNPOISON_MEMORY_REGION(arena2 + rg.first, rg.second);
    const uint32_t gx2 = std::max(1u, std::min(4u, (3u * maxf2 + 1023u) / 1024u));
    dsa::EncConn *conns = hc.data();
    if (n2) {
      launch(dsa::k_enc_table_clear, gx2, n2, 256, false, arena2, conns, n2);
      launch(dsa::k_enc_table_count, gx2, n2, 256, false, arena2, conns, n2);
      launch(dsa::k_enc_table_offsets, n2, 1, WAVE, false, arena2, conns, n2);
      launch(dsa::k_enc_table_lists, gx2, n2, 256, false, arena2, conns, n2);
      launch(dsa::k_enc_table_corners, gx2, n2, 256, false, arena2, conns, n2);
      launch(dsa::k_enc_repair_scan, gx2, n2, 256, false, arena2, conns, n2);      // (first-pass kernel: a repaired table has no such pair left, it must stay silent)
      launch(dsa::k_enc_connectivity, (n2 + lanes - 1) / lanes, 1, WAVE, false, arena2, conns, n2, lanes);
      launch(dsa::k_enc_operands, gx2, n2, 256, false, arena2, conns, n2);
      launch(dsa::k_enc_repair_rows, gx2, n2, 256, false, arena2, (const dsa::EncRepairRows *)rows.data(), n2);
    }
    for (uint32_t k = 0; k < n2; ++k) {
      const uint32_t i = mesh_of[k];
      const In &m = meshes[i];
      const dsa::EncConn &C = hc[k];
      std::vector<float> pos((size_t)3 * m.nv, 0.0f);
      synth::MeshIn in;
      in.pos = pos.data(); in.nv = m.nv; in.faces = m.faces.data(); in.nf = m.nf; in.normals = nullptr; in.uvs = nullptr; in.generic = nullptr;
      synth::MeshPlan pl;
      synth::Options opt;
      opt.repair_topology = 1;
      try { synth::plan_mesh(in, opt, pl); } catch (const std::exception &e) { fprintf(stderr, "mesh %u: the host coder refuses the repaired mesh: %s\n", i, e.what()); return 1; }
      SAME(C.status == dsa::ENC_OK, "status of the walk over the repaired table");
      const uint32_t V2 = pl.ct.nv();
      SAME(C.V == V2 && C.F == pl.ct.nf(), "compacted sizes");
      SAME(C.num_symbols == pl.eb.symbols.size() && memcmp(arena2 + C.symbols, pl.eb.symbols.data(), C.num_symbols) == 0, "symbols");
      SAME(C.num_start_bits == pl.eb.start_face_bits.size() && memcmp(arena2 + C.start_bits, pl.eb.start_face_bits.data(), C.num_start_bits) == 0, "start-face bits");
      SAME(C.num_split_symbols == pl.eb.num_split_symbols && C.num_splits == pl.eb.splits.size(), "split counts");
      const uint32_t *sp = (const uint32_t *)(arena2 + C.splits);
      for (uint32_t q = 0; q < C.num_splits; ++q) SAME(sp[3 * q] == pl.eb.splits[q].source && sp[3 * q + 1] == pl.eb.splits[q].split && sp[3 * q + 2] == pl.eb.splits[q].edge, "split events");
      SAME(C.num_entries == V2 && memcmp(arena2 + C.d2c, pl.seq.data_to_corner.data(), 4ull * V2) == 0, "traversal order");
      const uint32_t *e2v = (const uint32_t *)(arena2 + C.e2v);
      const int32_t *ops = (const int32_t *)(arena2 + C.ops);
      for (uint32_t p = 0; p < V2; ++p) {
        const uint32_t ci = pl.seq.data_to_corner[p];
        int32_t want[3] = {-1, -1, -1};
        if (p > 0) {
          const uint32_t oci = pl.ct.opposite(ci);
          if (oci != synth::kInvalid) {
            const int32_t vo = pl.seq.vertex_to_data[pl.ct.vertex(oci)], vn = pl.seq.vertex_to_data[pl.ct.vertex(synth::CornerTable::next(oci))], vp = pl.seq.vertex_to_data[pl.ct.vertex(synth::CornerTable::prev(oci))];
            if (vo < (int32_t)p && vn < (int32_t)p && vp < (int32_t)p) { want[0] = vn; want[1] = vp; want[2] = vo; }
          }
        }
        SAME(e2v[p] == pl.ct.row_of(pl.ct.vertex(ci)) && e2v[p] < m.nv && ops[3 * p] == want[0] && ops[3 * p + 1] == want[1] && ops[3 * p + 2] == want[2], "value rows and operand entries");
      }
      ++walked;
    }
  }
  printf("encrepair: %u meshes, %u repaired alike, %u given up at the step bound, %u walked alike\n", n, alike, bound, walked);
  return 0;
}
