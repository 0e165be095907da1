// tests/hostcheck/encseams_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The encoder's seam kernels of the product (draco-sharp_amd/csrc/dsa_encode_seams.h: seam edges, attribute vertices, the
// attribute walk one lane per (mesh, attribute), operand entries, seam bits) behind the connectivity kernels
// (dsa_encode_conn.h), compiled for the host with AddressSanitizer + UBSan and run thread by thread, against the host coder
// (dsa_encode_host.h: AttrConn, dfs_sequence, write_stream's seam loop) on the same faces and corner ids: the same seam marks,
// attribute vertex ids, traversal order, value rows, operand entries and seam bits on meshes both accept, the same verdict on the
// others, and not one access outside a mesh's arrays (the arena's gaps are poisoned).  Nothing here is linked into the product.
//
//   encseams_host <meshes.bin>   file: u32 count, then per mesh u32 nv, u32 nf, u32 faces[3 nf], u32 mask (bit 0 normal ids,
//                                bit 1 uv ids), per set bit: u32 rows, u32 ids[3 nf]
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
#include "../../draco-sharp_amd/csrc/dsa_encode_seams.h"

struct StreamStub { uint32_t nv; uint64_t ops; };       // the fields of dsa_encode.h's EncStream that k_enc_seam_operands sets

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: encseams_host <meshes.bin>\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  struct In { uint32_t nv, nf, mask; std::vector<uint32_t> faces; uint32_t rows[2]; std::vector<uint32_t> ids[2]; };
  std::vector<In> meshes(count);
  for (auto &m : meshes) {
    if (fread(&m.nv, 4, 1, f) != 1 || fread(&m.nf, 4, 1, f) != 1) return 2;
    m.faces.resize((size_t)3 * m.nf);
    if (m.nf && fread(m.faces.data(), 4, m.faces.size(), f) != m.faces.size()) return 2;
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
  // ---- the arena, laid out like dsa_encode.h lays a chunk out, every gap poisoned
  const uint32_t n = count;
  std::vector<dsa::EncConn> hc(n);
  std::vector<dsa::EncSeam> hz;
  std::vector<StreamStub> streams;
  std::vector<int> zatt;                         // per record: 0 normal ids, 1 uv ids
  uint64_t cur = 0;
  std::vector<std::pair<uint64_t, uint64_t>> regions;
  auto take = [&](uint64_t bytes) { cur = (cur + 255) & ~255ull; cur += 64; const uint64_t at = cur; regions.push_back({at, bytes}); cur += bytes + 64; return at; };
  std::vector<bool> host_checked(n, true);
  for (uint32_t i = 0; i < n; ++i) {
    dsa::EncConn &C = hc[i];
    memset(&C, 0, sizeof(C));
    const uint64_t F = meshes[i].nf, V = meshes[i].nv;
    C.F = (uint32_t)F; C.V = (uint32_t)V; C.split_cap = (uint32_t)F; C.fail_key = 0xFFFFFFFFu;
    C.faces = take(12 * F);
    C.opp = take(12 * F); C.voff = take(4 * (V + 1)); C.vcur = take(4 * V); C.vlist = take(12 * F); C.vcorner = take(4 * V);
    C.vvis = take(V); C.frec = take(32 * F);
    C.stack = take(4 * F); C.processed = take(4 * F); C.init_corners = take(4 * F);
    C.symbols = take(F); C.start_bits = take(F); C.splits = take(12ull * C.split_cap);
    C.d2c = take(4 * V); C.v2d = take(4 * V); C.e2v = take(4 * V); C.ops = take(12 * V);
    bool in_range = true;                       // (the library's host checks: an index out of range never reaches the device)
    for (uint32_t x : meshes[i].faces) in_range = in_range && x < V;
    for (int a = 0; a < 2; ++a) for (uint32_t x : meshes[i].ids[a]) in_range = in_range && x < meshes[i].rows[a];
    if (!in_range || F == 0 || V < 3) { C.status = dsa::ENC_ISOLATED; host_checked[i] = false; continue; }
    for (int a = 0; a < 2; ++a) {
      if (!(meshes[i].mask >> a & 1)) continue;
      dsa::EncSeam Z;
      memset(&Z, 0, sizeof(Z));
      Z.mesh = i; Z.stream = (uint32_t)streams.size(); Z.rows = meshes[i].rows[a]; Z.ids_narrow = (i + a) % 2 == 0 && Z.rows <= 65536;
      Z.ids = take((Z.ids_narrow ? 6 : 12) * F);
      Z.edge_seam = take(3 * F); Z.vert_seam = take(V); Z.afirst = take(4 * V); Z.aoff = take(4 * (V + 1));
      Z.c2av = take(12 * F); Z.opp2 = take(12 * F); Z.v2lm = take(12 * F); Z.avis = take(3 * F); Z.frec = take(32 * F);
      Z.stack = take(4 * F); Z.d2c = take(12 * F); Z.v2d = take(12 * F); Z.e2v = take(12 * F); Z.ops = take(36 * F);
      Z.rank = take(4 * F); Z.rcorner = take(4 * F); Z.eoff = take(4 * (F + 1)); Z.bits = take(4 * ((3 * F + 31) / 32));
      hz.push_back(Z);
      zatt.push_back(a);
      streams.push_back({(uint32_t)V, 0});
    }
  }
  std::vector<uint8_t> arena_store(cur + 256, 0);
  uint8_t *arena = arena_store.data();
  for (uint32_t i = 0; i < n; ++i) if (meshes[i].nf) memcpy(arena + hc[i].faces, meshes[i].faces.data(), 12ull * meshes[i].nf);
  for (auto &Z : hz) {
    const In &m = meshes[Z.mesh];
    const std::vector<uint32_t> &ids = m.ids[zatt[&Z - hz.data()]];
    if (!Z.ids_narrow) { memcpy(arena + Z.ids, ids.data(), 4 * ids.size()); continue; }
    uint16_t *narrow = (uint16_t *)(arena + Z.ids);
    for (size_t e = 0; e < ids.size(); ++e) narrow[e] = (uint16_t)ids[e];
  }
  ASAN_POISON_MEMORY_REGION(arena, arena_store.size());
  for (auto &rg : regions) ASAN_UNPOISON_MEMORY_REGION(arena + rg.first, rg.second);
  uint32_t maxf = 1;
  for (auto &m : meshes) maxf = std::max(maxf, m.nf);
  const uint32_t gx = std::max(1u, std::min(4u, (3u * maxf + 1023u) / 1024u));
  const uint32_t nz = (uint32_t)hz.size();
  dsa::EncConn *conns = hc.data();
  dsa::EncSeam *seams = hz.data();
  launch(dsa::k_enc_table_clear, gx, n, 256, arena, conns, n);
  launch(dsa::k_enc_table_count, gx, n, 256, arena, conns, n);
  launch(dsa::k_enc_table_offsets, n, 1, WAVE, arena, conns, n);
  launch(dsa::k_enc_table_lists, gx, n, 256, arena, conns, n);
  launch(dsa::k_enc_table_opposites, gx, n, 256, arena, conns, n);
  launch(dsa::k_enc_table_corners, gx, n, 256, arena, conns, n);
  const uint32_t lanes = 5;                    // meshes to a wave
  launch(dsa::k_enc_connectivity, (n + lanes - 1) / lanes, 1, WAVE, arena, conns, n, lanes);
  if (nz) {
    launch(dsa::k_enc_seam_edges, gx, nz, 256, arena, (const dsa::EncConn *)conns, seams, nz);
    launch(dsa::k_enc_seam_fans, gx, nz, 256, arena, (const dsa::EncConn *)conns, seams, nz);
    launch(dsa::k_enc_seam_offsets, nz, 1, WAVE, arena, (const dsa::EncConn *)conns, seams, nz);
    launch(dsa::k_enc_seam_assign, gx, nz, 256, arena, (const dsa::EncConn *)conns, seams, nz);
    launch(dsa::k_enc_seam_records, gx, nz, 256, arena, (const dsa::EncConn *)conns, seams, nz);
    launch(dsa::k_enc_seam_walk, (nz + lanes - 1) / lanes, 1, WAVE, arena, (const dsa::EncConn *)conns, seams, nz, lanes);
  }
  launch(dsa::k_enc_operands, gx, n, 256, arena, conns, n);
  if (nz) {
    launch(dsa::k_enc_seam_operands<StreamStub>, gx, nz, 256, arena, (const dsa::EncConn *)conns, seams, nz, streams.data());
    launch(dsa::k_enc_seam_rank, gx, nz, 256, arena, (const dsa::EncConn *)conns, seams, nz);
    launch(dsa::k_enc_seam_count, gx, nz, 256, arena, (const dsa::EncConn *)conns, seams, nz);
    launch(dsa::k_enc_seam_scan, nz, 1, WAVE, arena, (const dsa::EncConn *)conns, seams, nz);
    launch(dsa::k_enc_seam_bits, gx, nz, 256, arena, (const dsa::EncConn *)conns, seams, nz);
  }
  // ---- against the host coder
  uint32_t coded = 0, refused = 0, seamed = 0;
  size_t zi = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const In &m = meshes[i];
    const dsa::EncConn &C = hc[i];
    std::vector<float> pos((size_t)3 * std::max(m.nv, 1u), 0.0f), nrm((size_t)3 * std::max(m.rows[0], 1u), 0.0f), uv((size_t)2 * std::max(m.rows[1], 1u), 0.0f);
    synth::MeshIn in;
    in.pos = pos.data(); in.nv = m.nv; in.faces = m.faces.data(); in.nf = m.nf; in.generic = nullptr;
    in.normals = (m.mask & 1) ? nrm.data() : nullptr; in.uvs = (m.mask & 2) ? uv.data() : nullptr;
    in.normal_corners = (m.mask & 1) ? m.ids[0].data() : nullptr; in.nn = m.rows[0];
    in.uv_corners = (m.mask & 2) ? m.ids[1].data() : nullptr; in.nu = m.rows[1];
    synth::MeshPlan pl;
    synth::Options opt;
    bool host_ok = true;
    std::string why;
    try {
      synth::check(m.nv >= 3 && m.nf >= 1, "mesh needs positions and faces");
      for (uint32_t x : m.faces) synth::check(x < m.nv, "face index out of range");
      for (int a = 0; a < 2; ++a) for (uint32_t x : m.ids[a]) synth::check(x < m.rows[a], "id out of range");
      synth::plan_mesh(in, opt, pl);
    } catch (const std::exception &e) { host_ok = false; why = e.what(); }
    const size_t z0 = zi;
    if (host_checked[i]) zi += __builtin_popcount(m.mask);
    uint32_t seam_status = 0;
    for (size_t z = z0; z < zi; ++z) if (!seam_status) seam_status = hz[z].status;
    const bool dev_ok = C.status == dsa::ENC_OK && seam_status == 0;
    const char *dev_why = C.status != dsa::ENC_OK ? dsa::enc_conn_message(C.status) : dsa::enc_seam_message(seam_status);
    if (host_ok != dev_ok) { fprintf(stderr, "mesh %u: host coder %s (%s), device source %s\n", i, host_ok ? "codes" : "refuses", why.c_str(), dev_ok ? "codes" : dev_why); return 1; }
    if (!host_ok) {
      if (host_checked[i] && why != dev_why) { fprintf(stderr, "mesh %u: host coder says '%s', device source '%s'\n", i, why.c_str(), dev_why); return 1; }
      ++refused;
      continue;
    }
    ++coded;
#define SAME(cond, what) do { if (!(cond)) { fprintf(stderr, "mesh %u attribute %d: %s differ\n", i, att, what); return 1; } } while (0)
    // decoder face order of the host coder's seam loop
    std::vector<uint8_t> vis(m.nf, 0);
    std::vector<uint32_t> edge_corner;
    for (uint32_t c : pl.eb.processed_corners) {
      const uint32_t cs[3] = {c, synth::CornerTable::next(c), synth::CornerTable::prev(c)};
      vis[c / 3] = 1;
      for (int k = 0; k < 3; ++k) { const uint32_t o = pl.ct.opposite(cs[k]); if (o != synth::kInvalid && !vis[o / 3]) edge_corner.push_back(cs[k]); }
    }
    int att = 0;
    for (size_t z = z0; z < zi; ++z) {
      const dsa::EncSeam &Z = hz[z];
      att = zatt[z];
      const size_t pa = (att == 0 || !(m.mask & 1)) ? 1 : 2;        // plan attribute: normals first, then texture coordinates
      const synth::AttrConn &A = pl.conns[pa];
      const uint32_t NC = 3 * m.nf;
      SAME(memcmp(arena + Z.edge_seam, A.edge_seam.data(), NC) == 0, "seam edge marks");
      SAME(memcmp(arena + Z.vert_seam, A.vert_seam.data(), m.nv) == 0, "seam vertex marks");
      SAME((Z.interior_seams == 0) == A.no_interior_seams, "interior seam flags");
      SAME(Z.num_av == A.nv() && memcmp(arena + Z.c2av, A.c2v.data(), 4ull * NC) == 0 && memcmp(arena + Z.v2lm, A.v2lm.data(), 4ull * A.nv()) == 0, "attribute vertices");
      const uint32_t *e2v = (const uint32_t *)(arena + Z.e2v);
      const uint32_t *ids = m.ids[att].data();
      if (A.no_interior_seams) {
        SAME(streams[Z.stream].nv == m.nv && streams[Z.stream].ops == C.ops, "stream entries");
        for (uint32_t p = 0; p < m.nv; ++p) SAME(e2v[p] == ids[pl.seq.data_to_corner[p]], "value rows");
        continue;
      }
      ++seamed;
      const synth::Sequence &sq = pl.seq_att[pa];
      const uint32_t entries = (uint32_t)sq.data_to_corner.size();
      SAME(Z.num_entries == entries && streams[Z.stream].nv == entries && streams[Z.stream].ops == Z.ops, "stream entries");
      SAME(memcmp(arena + Z.d2c, sq.data_to_corner.data(), 4ull * entries) == 0, "attribute traversal order");
      const int32_t *ops = (const int32_t *)(arena + Z.ops);
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
        SAME(e2v[p] == ids[ci] && ops[3 * p] == want[0] && ops[3 * p + 1] == want[1] && ops[3 * p + 2] == want[2], "operand entries");
      }
      SAME(edge_corner.size() == C.interior_edges, "interior edge counts");
      const uint32_t *bits = (const uint32_t *)(arena + Z.bits);
      for (size_t e = 0; e < edge_corner.size(); ++e) SAME(((bits[e >> 5] >> (e & 31)) & 1u) == A.edge_seam[edge_corner[e]], "seam bits");
    }
  }
  printf("encseams: %u meshes, %u coded alike, %u refused alike, %u seamed attributes\n", n, coded, refused, seamed);
  return 0;
}
