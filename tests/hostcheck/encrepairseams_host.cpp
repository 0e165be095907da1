// tests/hostcheck/encrepairseams_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// Attributes given per corner over a mesh whose topology needs the repair (dsa_encode_seam_repair_batch, corner_repair = 1), the
// device's side of it compiled for the host with AddressSanitizer + UBSan and run thread by thread:
//   1. the repair kernels and, in front of the break pass, k_enc_repair_face_scan and k_enc_repair_ids (dsa_encode_repair.h), over
//      an arena laid out like enc_stage_repair lays it out, every gap poisoned;
//   2. CornerTable::from_repaired on what they left, as the library's host side does;
//   3. the table kernels (opposites given), the connectivity walk and the seam kernels (dsa_encode_seams.h: edges, fans, offsets,
//      assign, records, walk, operands, rank, count, scan, bits) over a second arena laid out like enc_layout lays the repaired
//      chunk out, the ids region filled from the first arena as enc_stage_uploads fills it.
// Held against the host coder with repair_topology = 2 (dsa_encode_host.h plan_mesh) on the same faces and ids: the cmap-compacted
// ids, AttrConn (edge_seam, vert_seam, c2v, v2lm), seq_att, value rows and operand entries, seam bits; an id out of range fails
// the mesh with the host coder's words.  Nothing here is linked into the product.
//
//   encrepairseams_host <meshes.bin>   file: u32 count, then per mesh u32 nv, u32 nf, u32 faces[3 nf], u32 mask (bit 0 normal ids,
//                                      bit 1 uv ids), per set bit: u32 rows, u32 ids[3 nf]
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
#include "../../draco-sharp_amd/csrc/dsa_encode_seams.h"

struct StreamStub { uint32_t nv; uint64_t ops; };       // the fields of dsa_encode.h's EncStream that k_enc_seam_operands sets

struct In { uint32_t nv, nf, mask; std::vector<uint32_t> faces; uint32_t rows[2]; std::vector<uint32_t> ids[2]; };

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: encrepairseams_host <meshes.bin>\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  std::vector<In> meshes(count);
  for (auto &m : meshes) {
    if (fread(&m.nv, 4, 1, f) != 1 || fread(&m.nf, 4, 1, f) != 1) return 2;
    m.faces.resize((size_t)3 * m.nf);
    if (m.nf && fread(m.faces.data(), 4, m.faces.size(), f) != m.faces.size()) return 2;
    for (uint32_t x : m.faces) if (x >= m.nv) { fprintf(stderr, "index out of range in the input file\n"); return 2; }      // (the library's host checks keep such a mesh from the device)
    if (fread(&m.mask, 4, 1, f) != 1) return 2;
    for (int a = 0; a < 2; ++a) {
      m.rows[a] = 0;
      if (!(m.mask >> a & 1)) continue;
      if (fread(&m.rows[a], 4, 1, f) != 1) return 2;
      m.ids[a].resize((size_t)3 * m.nf);
      if (m.nf && fread(m.ids[a].data(), 4, m.ids[a].size(), f) != m.ids[a].size()) return 2;
    }
  }
  fclose(f);
  const uint32_t n = count;
#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

  // ---- 1. the repair arena, laid out like enc_stage_repair lays it out, every gap poisoned
  std::vector<dsa::EncRepair> recs(n);
  std::vector<dsa::EncRepairIds> id_recs;
  std::vector<int> id_att;
  std::vector<int> first_id(n, -1);
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
    for (int a = 0; a < 2; ++a) {
      if (!(meshes[i].mask >> a & 1)) continue;
      if (!R.fmap) { R.fmap = take(4 * F); first_id[i] = (int)id_recs.size(); }
      dsa::EncRepairIds I;
      memset(&I, 0, sizeof(I));
      I.rep = i; I.rows = meshes[i].rows[a]; I.narrow = I.rows <= 65536 ? 1u : 0u; I.att_type = a == 0 ? 1u : 3u;
      I.src = take(12 * F); I.dst = take((I.narrow ? 6 : 12) * F);
      id_recs.push_back(I); id_att.push_back(a);
    }
    maxf = std::max(maxf, meshes[i].nf);
  }
  const uint32_t ni = (uint32_t)id_recs.size();
  std::vector<uint8_t> arena_store(cur + 256, 0);
  uint8_t *arena = arena_store.data();
  for (uint32_t i = 0; i < n; ++i) if (meshes[i].nf) memcpy(arena + recs[i].faces, meshes[i].faces.data(), 12ull * meshes[i].nf);
  for (uint32_t q = 0; q < ni; ++q) { const In &m = meshes[id_recs[q].rep]; if (m.nf) memcpy(arena + id_recs[q].src, m.ids[id_att[q]].data(), 12ull * m.nf); }
  ASAN_POISON_MEMORY_REGION(arena, arena_store.size());
  for (auto &rg : regions) ASAN_UNPOISON_MEMORY_REGION(arena + rg.first, rg.second);
  const uint32_t gx = std::max(1u, std::min(4u, (3u * maxf + 1023u) / 1024u));
  const uint32_t lanes = 5;                    // meshes to a wave
  dsa::EncRepair *reps = recs.data();
  launch(dsa::k_enc_repair_mark, gx, n, 256, false, arena, reps, n);
  if (ni) {
    launch(dsa::k_enc_repair_face_scan, n, 1, WAVE, false, arena, reps, n);
    launch(dsa::k_enc_repair_ids, gx, ni, 256, true, arena, (const dsa::EncRepair *)reps, id_recs.data(), ni);
  }
  launch(dsa::k_enc_repair_offsets, n, 1, WAVE, false, arena, reps, n);
  launch(dsa::k_enc_repair_lists, gx, n, 256, true, arena, reps, n);
  launch(dsa::k_enc_repair_opposites, gx, n, 256, true, arena, reps, n);
  launch(dsa::k_enc_repair_fans, (n + lanes - 1) / lanes, 1, WAVE, false, arena, reps, n, lanes);

  // ---- 2. + 3. the host coder's plan (value 2) of every mesh, from_repaired on the kernels' tables, the second arena
  std::vector<synth::MeshPlan> plans(n);
  std::vector<std::vector<float>> vals(3 * (size_t)n);
  std::vector<synth::MeshIn> ins(n);
  std::vector<std::string> host_why(n);
  std::vector<synth::CornerTable> tables(n);
  std::vector<dsa::EncConn> hc;
  std::vector<dsa::EncSeam> hz;
  std::vector<StreamStub> streams;
  std::vector<uint32_t> mesh_of, z_id;           // per EncConn its mesh; per EncSeam its EncRepairIds
  std::vector<std::pair<uint64_t, uint64_t>> regions2;
  uint64_t cur2 = 0;
  auto take2 = [&](uint64_t bytes) { cur2 = (cur2 + 255) & ~255ull; cur2 += 64; const uint64_t at = cur2; regions2.push_back({at, bytes}); cur2 += bytes + 64; return at; };
  uint32_t bound = 0, refused = 0, bad_ids = 0, maxf2 = 1;
  for (uint32_t i = 0; i < n; ++i) {
    const In &m = meshes[i];
    const dsa::EncRepair &R = recs[i];
    vals[3 * i].assign((size_t)3 * std::max(m.nv, 1u), 0.0f); vals[3 * i + 1].assign((size_t)3 * std::max(m.rows[0], m.nv), 0.0f); vals[3 * i + 2].assign((size_t)2 * std::max(m.rows[1], m.nv), 0.0f);
    synth::MeshIn &in = ins[i];
    in.pos = vals[3 * i].data(); in.nv = m.nv; in.faces = m.faces.data(); in.nf = m.nf; in.generic = nullptr;
    in.normals = vals[3 * i + 1].data(); in.uvs = vals[3 * i + 2].data();
    in.normal_corners = (m.mask & 1) ? m.ids[0].data() : nullptr; in.nn = m.rows[0];
    in.uv_corners = (m.mask & 2) ? m.ids[1].data() : nullptr; in.nu = m.rows[1];
    synth::Options opt;
    opt.repair_topology = 2;
    try {
      synth::check(m.nv >= 3 && m.nf >= 1, "mesh needs positions and faces");
      for (uint32_t x : m.ids[0]) synth::check(x < m.rows[0], "normal id out of range");
      for (uint32_t x : m.ids[1]) synth::check(x < m.rows[1], "texture coordinate id out of range");
      synth::plan_mesh(in, opt, plans[i]);
    } catch (const std::exception &e) { host_why[i] = e.what(); }
    if (R.status == dsa::ENC_REPAIR_BOUND) { ++bound; continue; }
    if (R.status != dsa::ENC_REPAIR_OK) FAIL("mesh %u: repair status %u", i, R.status);
    // an id out of range: the kernel's verdict is the host coder's, in its words
    std::string dev_why;
    for (int q = first_id[i]; q >= 0 && q < (int)ni && id_recs[q].rep == i; ++q) if (id_recs[q].bad && dev_why.empty()) dev_why = id_recs[q].att_type == 1 ? "normal id out of range" : "texture coordinate id out of range";
    const bool host_bad = host_why[i] == "normal id out of range" || host_why[i] == "texture coordinate id out of range";
    if (host_bad || !dev_why.empty()) {
      if (host_why[i] != dev_why) FAIL("mesh %u: host coder says '%s', k_enc_repair_ids '%s'", i, host_why[i].c_str(), dev_why.c_str());
      ++bad_ids;
      continue;
    }
    if (m.nv < 3 || m.nf < 1 || R.degenerate >= m.nf) {
      if (host_why[i].empty()) FAIL("mesh %u: the host coder codes a mesh without a face that is not degenerate", i);
      ++refused;
      continue;
    }
    if (!host_why[i].empty()) FAIL("mesh %u: the host coder refuses: %s", i, host_why[i].c_str());
    synth::CornerTable::Repaired r;
    r.c2v.assign((const uint32_t *)(arena + R.c2v), (const uint32_t *)(arena + R.c2v) + 3ull * m.nf);
    r.opp.assign((const uint32_t *)(arena + R.opp), (const uint32_t *)(arena + R.opp) + 3ull * m.nf);
    r.parent.assign((const uint32_t *)(arena + R.parent), (const uint32_t *)(arena + R.parent) + (R.num_vertices - R.V));
    r.num_vertices = R.num_vertices; r.isolated = R.isolated; r.degenerate = R.degenerate; r.breaks = R.breaks;
    synth::CornerTable &t = tables[i];
    t.from_repaired(r, m.faces.data(), m.nf, m.nv);
    if (R.fmap && R.coded_faces != t.nf()) FAIL("mesh %u: the scan kept %u faces, from_repaired %u", i, R.coded_faces, t.nf());
    // the scan against cmap, the compacted ids against the host coder's
    if (R.fmap) {
      const uint32_t *fmap = (const uint32_t *)(arena + R.fmap);
      for (uint32_t ff = 0; ff < m.nf; ++ff) {
        const uint32_t want = t.cmap[3 * ff] == synth::kInvalid ? DSA_INVALID : t.cmap[3 * ff] / 3;
        if (fmap[ff] != want) FAIL("mesh %u: face %u goes to %u, cmap says %u", i, ff, fmap[ff], want);
      }
    }
    const uint64_t F = t.nf(), V = t.nv();
    dsa::EncConn C;
    memset(&C, 0, sizeof(C));
    C.F = (uint32_t)F; C.V = (uint32_t)V; C.split_cap = (uint32_t)F; C.fail_key = 0xFFFFFFFFu;
    C.faces = take2(12 * F); C.opp = take2(12 * F); C.voff = take2(4 * (V + 1)); C.vcur = take2(4 * V); C.vlist = take2(12 * F); C.vcorner = take2(4 * V);
    C.vvis = take2(V); C.frec = take2(32 * F);
    C.stack = take2(4 * F); C.processed = take2(4 * F); C.init_corners = take2(4 * F);
    C.symbols = take2(F); C.start_bits = take2(F); C.splits = take2(12ull * C.split_cap);
    C.d2c = take2(4 * V); C.v2d = take2(4 * V); C.e2v = take2(4 * V); C.ops = take2(12 * V);
    for (int q = first_id[i]; q >= 0 && q < (int)ni && id_recs[q].rep == i; ++q) {
      const dsa::EncRepairIds &I = id_recs[q];
      const size_t pa = id_att[q] == 0 ? 1 : 2;        // plan attribute: normals first, then texture coordinates (both present, per vertex without ids)
      const uint32_t *want = plans[i].atts[pa].corner_value;          // (the cmap-compacted ids where the mesh needed the repair, else the caller's own)
      if (plans[i].ct.needed_repair && (plans[i].coded_ids.size() <= pa || plans[i].coded_ids[pa].size() != 3 * F || want != plans[i].coded_ids[pa].data()))
        FAIL("mesh %u attribute %d: the host coder did not compact the ids over %llu faces", i, id_att[q], (unsigned long long)F);
      for (size_t c = 0; c < 3 * F; ++c) {
        const uint32_t got = I.narrow ? (uint32_t)((const uint16_t *)(arena + I.dst))[c] : ((const uint32_t *)(arena + I.dst))[c];
        if (got != want[c]) FAIL("mesh %u attribute %d: compacted id %zu is %u, the host coder's %u", i, id_att[q], c, got, want[c]);
      }
      dsa::EncSeam Z;
      memset(&Z, 0, sizeof(Z));
      Z.mesh = (uint32_t)hc.size(); Z.stream = (uint32_t)streams.size(); Z.rows = I.rows; Z.ids_narrow = I.narrow;      // (the layout's rule)
      Z.ids = take2((Z.ids_narrow ? 6 : 12) * F);                                                                   // 3 F' entries: the coded face count
      Z.edge_seam = take2(3 * F); Z.vert_seam = take2(V); Z.afirst = take2(4 * V); Z.aoff = take2(4 * (V + 1));
      Z.c2av = take2(12 * F); Z.opp2 = take2(12 * F); Z.v2lm = take2(12 * F); Z.avis = take2(3 * F); Z.frec = take2(32 * F);
      Z.stack = take2(4 * F); Z.d2c = take2(12 * F); Z.v2d = take2(12 * F); Z.e2v = take2(12 * F); Z.ops = take2(36 * F);
      Z.rank = take2(4 * F); Z.rcorner = take2(4 * F); Z.eoff = take2(4 * (F + 1)); Z.bits = take2(4 * ((3 * F + 31) / 32));
      hz.push_back(Z); z_id.push_back((uint32_t)q);
      streams.push_back({(uint32_t)V, 0});
    }
    hc.push_back(C); mesh_of.push_back(i);
    maxf2 = std::max(maxf2, C.F);
  }
  const uint32_t n2 = (uint32_t)hc.size(), nz = (uint32_t)hz.size();
  std::vector<uint8_t> store2(cur2 + 256, 0);
  uint8_t *arena2 = store2.data();
  for (uint32_t k = 0; k < n2; ++k) {
    const synth::CornerTable &t = tables[mesh_of[k]];
    memcpy(arena2 + hc[k].faces, t.c2v.data(), 4ull * t.c2v.size());
    memcpy(arena2 + hc[k].opp, t.opp.data(), 4ull * t.opp.size());
  }
  for (uint32_t z = 0; z < nz; ++z)            // enc_stage_uploads: the ids of the coded faces, from the repair arena
    memcpy(arena2 + hz[z].ids, arena + id_recs[z_id[z]].dst, (hz[z].ids_narrow ? 6ull : 12ull) * hc[hz[z].mesh].F);
  ASAN_POISON_MEMORY_REGION(arena2, store2.size());
  for (auto &rg : regions2) ASAN_UNPOISON_MEMORY_REGION(arena2 + rg.first, rg.second);
  const uint32_t gx2 = std::max(1u, std::min(4u, (3u * maxf2 + 1023u) / 1024u));
  dsa::EncConn *conns = hc.data();
  dsa::EncSeam *seams = hz.data();
  if (n2) {
    launch(dsa::k_enc_table_clear, gx2, n2, 256, false, arena2, conns, n2);
    launch(dsa::k_enc_table_count, gx2, n2, 256, false, arena2, conns, n2);
    launch(dsa::k_enc_table_offsets, n2, 1, WAVE, false, arena2, conns, n2);
    launch(dsa::k_enc_table_lists, gx2, n2, 256, true, arena2, conns, n2);
    launch(dsa::k_enc_table_corners, gx2, n2, 256, false, arena2, conns, n2);      // (the opposites are given: k_enc_table_opposites is not launched)
    launch(dsa::k_enc_connectivity, (n2 + lanes - 1) / lanes, 1, WAVE, false, arena2, conns, n2, lanes);
  }
  if (nz) {
    launch(dsa::k_enc_seam_edges, gx2, nz, 256, false, arena2, (const dsa::EncConn *)conns, seams, nz);
    launch(dsa::k_enc_seam_fans, gx2, nz, 256, false, arena2, (const dsa::EncConn *)conns, seams, nz);
    launch(dsa::k_enc_seam_offsets, nz, 1, WAVE, false, arena2, (const dsa::EncConn *)conns, seams, nz);
    launch(dsa::k_enc_seam_assign, gx2, nz, 256, true, arena2, (const dsa::EncConn *)conns, seams, nz);
    launch(dsa::k_enc_seam_records, gx2, nz, 256, false, arena2, (const dsa::EncConn *)conns, seams, nz);
    launch(dsa::k_enc_seam_walk, (nz + lanes - 1) / lanes, 1, WAVE, false, arena2, (const dsa::EncConn *)conns, seams, nz, lanes);
  }
  if (n2) launch(dsa::k_enc_operands, gx2, n2, 256, false, arena2, conns, n2);
  if (nz) {
    launch(dsa::k_enc_seam_operands<StreamStub>, gx2, nz, 256, false, arena2, (const dsa::EncConn *)conns, seams, nz, streams.data());
    launch(dsa::k_enc_seam_rank, gx2, nz, 256, false, arena2, (const dsa::EncConn *)conns, seams, nz);
    launch(dsa::k_enc_seam_count, gx2, nz, 256, false, arena2, (const dsa::EncConn *)conns, seams, nz);
    launch(dsa::k_enc_seam_scan, nz, 1, WAVE, false, arena2, (const dsa::EncConn *)conns, seams, nz);
    launch(dsa::k_enc_seam_bits, gx2, nz, 256, true, arena2, (const dsa::EncConn *)conns, seams, nz);
  }

  // ---- against the host coder's plan
  uint32_t coded = 0, seamed = 0, repaired = 0, wide = 0;
  size_t zi = 0;
  for (uint32_t k = 0; k < n2; ++k) {
    const uint32_t i = mesh_of[k];
    const In &m = meshes[i];
    const dsa::EncConn &C = hc[k];
    const synth::MeshPlan &pl = plans[i];
    int att = -1;
#define SAME(cond, what) do { if (!(cond)) { fprintf(stderr, "mesh %u attribute %d: %s differ\n", i, att, what); return 1; } } while (0)
    SAME(C.status == dsa::ENC_OK && C.fail_key == 0xFFFFFFFFu, "status of the walk over the repaired table");
    SAME(C.V == pl.ct.nv() && C.F == pl.ct.nf(), "compacted sizes");
    SAME(C.num_symbols == pl.eb.symbols.size() && memcmp(arena2 + C.symbols, pl.eb.symbols.data(), C.num_symbols) == 0, "symbols");
    SAME(C.num_entries == C.V && memcmp(arena2 + C.d2c, pl.seq.data_to_corner.data(), 4ull * C.V) == 0, "traversal order");
    repaired += pl.ct.needed_repair ? 1 : 0;
    // decoder face order of the host coder's seam loop
    std::vector<uint8_t> vis(C.F, 0);
    std::vector<uint32_t> edge_corner;
    for (uint32_t c : pl.eb.processed_corners) {
      const uint32_t cs[3] = {c, synth::CornerTable::next(c), synth::CornerTable::prev(c)};
      vis[c / 3] = 1;
      for (int e = 0; e < 3; ++e) { const uint32_t o = pl.ct.opposite(cs[e]); if (o != synth::kInvalid && !vis[o / 3]) edge_corner.push_back(cs[e]); }
    }
    const uint32_t NC = 3 * C.F;
    for (; zi < nz && hz[zi].mesh == k; ++zi) {
      const dsa::EncSeam &Z = hz[zi];
      att = id_att[z_id[zi]];
      const size_t pa = att == 0 ? 1 : 2;
      const synth::AttrConn &A = pl.conns[pa];
      const uint32_t *ids = pl.atts[pa].corner_value;             // (the compacted ids where the mesh needed repair, else the caller's)
      wide += Z.ids_narrow ? 0 : 1;
      SAME(Z.status == dsa::ENC_SEAM_OK, "seam status");
      SAME(memcmp(arena2 + Z.edge_seam, A.edge_seam.data(), NC) == 0, "seam edge marks");
      SAME(memcmp(arena2 + Z.vert_seam, A.vert_seam.data(), C.V) == 0, "seam vertex marks");
      SAME((Z.interior_seams == 0) == A.no_interior_seams, "interior seam flags");
      SAME(Z.num_av == A.nv() && memcmp(arena2 + Z.c2av, A.c2v.data(), 4ull * NC) == 0 && memcmp(arena2 + Z.v2lm, A.v2lm.data(), 4ull * A.nv()) == 0, "attribute vertices");
      const uint32_t *e2v = (const uint32_t *)(arena2 + Z.e2v);
      if (A.no_interior_seams) {
        SAME(streams[Z.stream].nv == C.V && streams[Z.stream].ops == C.ops, "stream entries");
        for (uint32_t p = 0; p < C.V; ++p) SAME(e2v[p] == ids[pl.seq.data_to_corner[p]] && e2v[p] < Z.rows, "value rows");
        continue;
      }
      ++seamed;
      const synth::Sequence &sq = pl.seq_att[pa];
      const uint32_t entries = (uint32_t)sq.data_to_corner.size();
      SAME(Z.num_entries == entries && streams[Z.stream].nv == entries && streams[Z.stream].ops == Z.ops, "stream entries");
      SAME(memcmp(arena2 + Z.d2c, sq.data_to_corner.data(), 4ull * entries) == 0, "attribute traversal order");
      const int32_t *ops = (const int32_t *)(arena2 + Z.ops);
      for (uint32_t p = 0; p < entries; ++p) {
        const uint32_t ci = sq.data_to_corner[p];
        int32_t want[3] = {-1, -1, -1};
        if (p > 0) {
          const uint32_t oci = A.opposite(ci);
          if (oci != synth::kInvalid) {
            const int32_t vo = sq.vertex_to_data[A.vertex(oci)], vn = sq.vertex_to_data[A.vertex(synth::CornerTable::next(oci))], vp = sq.vertex_to_data[A.vertex(synth::CornerTable::prev(oci))];
            if (vo < (int32_t)p && vn < (int32_t)p && vp < (int32_t)p) { want[0] = vn; want[1] = vp; want[2] = vo; }
          }
        }
        SAME(e2v[p] == ids[ci] && e2v[p] < Z.rows && ops[3 * p] == want[0] && ops[3 * p + 1] == want[1] && ops[3 * p + 2] == want[2], "value rows and operand entries");
      }
      SAME(edge_corner.size() == C.interior_edges, "interior edge counts");
      const uint32_t *bits = (const uint32_t *)(arena2 + Z.bits);
      for (size_t e = 0; e < edge_corner.size(); ++e) SAME(((bits[e >> 5] >> (e & 31)) & 1u) == A.edge_seam[edge_corner[e]], "seam bits");
    }
    ++coded;
  }
  printf("encrepairseams: %u meshes, %u coded alike (%u needed the repair), %u seamed attributes, %u wide id arrays, %u refused alike, %u with an id out of range, %u given up at the step bound\n",
         n, coded, repaired, seamed, wide, refused, bad_ids, bound);
  return 0;
}
