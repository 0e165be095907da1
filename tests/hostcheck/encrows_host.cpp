// tests/hostcheck/encrows_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The two kernels of draco-sharp_amd/csrc/dsa_encode_rows.h compiled for the host with AddressSanitizer + UBSan and run thread by
// thread, forwards and backwards, over arenas whose gaps are poisoned:
//   k_enc_entry_rows   over the chunk the product's own layout makes for every mesh of the input file with track_rows set
//                      (dsa_encode_layout.h: enc_plan_mesh with host connectivity, enc_layout; for per-point input the host weld and
//                      enc_weld_view in front, as enc_stage_weld does) -- the records, the uploads and the regions are the
//                      library's.  The rows must be the host coder's (synth::plan_entry_rows on a plan of its own; through
//                      synth::weld_row_points for a welded mesh).
//   k_source_rows      over point maps made here from those rows: every entry once in a scrambled order, entries twice, an entry
//                      index at and beyond the tracked count (0xFFFFFFFF), the identity map, the identity rows of a sequential
//                      stream, a mesh that failed to decode and one whose entry count is not the tracked one (nothing written), an empty mesh.
// Nothing here is linked into the product.
//
//   encrows_host <meshes.bin>   file: u32 count, then per mesh u32 form (1 indexed, 2 one row per point), nv, nf, normals (0 / 1),
//                               texcoords (0 / 1), nn, nu (rows of normals / texcoords given per corner; 0: per vertex), generic
//                               components (0: none), repair (0 / 1 / 2), traversal_method, weld_attributes, extras;
//                               u32 faces[3 nf]; f32 pos[3 nv]; normals f32[3 (nn or nv)], u32 ids[3 nf] when nn; texcoords f32[2 (nu
//                               or nv)], ids when nu; generic u8[components nv]; per extra u32 data type, components, rows (0: per
//                               vertex), its rows packed, u32 ids[3 nf] when rows
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../draco-sharp_amd/csrc/dsa_common.h"
#include "../../draco-sharp_amd/csrc/dsa_types.h"

#include "hip_on_host.h"

#include "../../draco-sharp_amd/csrc/dsa_encode_layout.h"

struct Extra { uint32_t data_type = 0, nc = 0, rows = 0; std::vector<uint8_t> values; std::vector<uint32_t> ids; };
struct In {
  uint32_t form = 1, nv = 0, nf = 0, normals = 0, texcoords = 0, nn = 0, nu = 0, generic = 0, repair = 0, traversal = 0, weld_attributes = 0;
  std::vector<uint32_t> faces, nid, uid;
  std::vector<float> pos, nrm, uv;
  std::vector<uint8_t> gen;
  std::vector<Extra> extras;
};

#define FAIL(...) do { fprintf(stderr, "mesh %u (%s): ", index, backwards ? "backwards" : "forwards"); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return false; } while (0)

// the decoder's record of a mesh as k_source_rows reads it
struct Desc { uint32_t status, num_points, num_attributes; struct { uint32_t num_entries; } att[SRC_ROWS_MAX_ATT]; };

static bool source_rows(uint32_t index, bool backwards, const std::vector<std::vector<uint32_t>> &entry_rows) {
  // meshes: 0 scrambled maps over the tracked rows, 1 the identity map and identity rows, 2 failed to decode, 3 decoded to one entry
  // more than was tracked in its last attribute (not the stream the rows were kept for: nothing written), 4 empty
  const uint32_t na = (uint32_t)std::min<size_t>(entry_rows.size(), SRC_ROWS_MAX_ATT);
  uint32_t most = 0;
  for (uint32_t a = 0; a < na; ++a) most = std::max(most, (uint32_t)entry_rows[a].size());
  const uint32_t points = most + most / 2 + 3, cap_points = points + 5;
  std::vector<std::vector<uint32_t>> maps(na);
  for (uint32_t a = 0; a < na; ++a) {
    const uint32_t ne = (uint32_t)entry_rows[a].size();
    maps[a].resize(cap_points, 0xDDDDDDDDu);
    for (uint32_t p = 0; p < points; ++p) maps[a][p] = ne ? (uint32_t)(((uint64_t)p * 2654435761ull + a) % ne) : 0u;
    maps[a][points - 1] = ne; maps[a][points - 2] = ne + 77u; maps[a][points / 2] = 0xFFFFFFFFu;      // at and beyond the tracked count
  }
  uint64_t acur = 0, bcur = 0;
  std::vector<std::pair<uint64_t, uint64_t>> aregions, bregions;
  auto take = [](uint64_t &cur, std::vector<std::pair<uint64_t, uint64_t>> &regions, uint64_t bytes) { cur = (cur + 63) & ~63ull; cur += 64; const uint64_t at = cur; regions.push_back({at, bytes}); cur += bytes + 64; return at; };
  std::vector<dsa::SrcRowsMesh> table(5);
  memset(table.data(), 0, sizeof(dsa::SrcRowsMesh) * 5);
  const uint64_t table_at = 0;
  bcur = sizeof(dsa::SrcRowsMesh) * 5;
  bregions.push_back({table_at, bcur});
  for (uint32_t m = 0; m < 4; ++m) {
    dsa::SrcRowsMesh &T = table[m];
    T.num_attributes = na; T.cap_points = cap_points;
    for (uint32_t a = 0; a < na; ++a) {
      dsa::SrcRowsAttr &A = T.att[a];
      A.num_rows = (uint32_t)entry_rows[a].size();
      A.map = m == 1 ? dsa::SRC_ROWS_IDENTITY : take(acur, aregions, 4ull * cap_points);
      A.rows = m == 1 ? dsa::SRC_ROWS_IDENTITY : take(bcur, bregions, 4ull * A.num_rows);
      A.out = take(bcur, bregions, 4ull * cap_points);
    }
  }
  std::vector<uint8_t> astore(acur + 128, 0), bstore(bcur + 128, 0xCD);
  uint8_t *arena = astore.data(), *block = bstore.data();
  memcpy(block, table.data(), sizeof(dsa::SrcRowsMesh) * 5);
  for (uint32_t m = 0; m < 4; m += (m == 0 ? 2 : 1))
    for (uint32_t a = 0; a < na; ++a) {
      memcpy(arena + table[m].att[a].map, maps[a].data(), 4ull * cap_points);
      if (!entry_rows[a].empty()) memcpy(block + table[m].att[a].rows, entry_rows[a].data(), 4ull * entry_rows[a].size());
    }
  Desc descs[5];
  memset(descs, 0, sizeof(descs));
  for (uint32_t m = 0; m < 4; ++m) {
    descs[m].status = m == 2 ? 2u : 0u; descs[m].num_points = points; descs[m].num_attributes = na;
    for (uint32_t a = 0; a < na; ++a) descs[m].att[a].num_entries = (uint32_t)entry_rows[a].size() + (m == 3 && a + 1 == na ? 1u : 0u);
  }
  ASAN_POISON_MEMORY_REGION(arena, astore.size());
  for (auto &rg : aregions) ASAN_UNPOISON_MEMORY_REGION(arena + rg.first, rg.second);
  ASAN_POISON_MEMORY_REGION(block, bstore.size());
  for (auto &rg : bregions) ASAN_UNPOISON_MEMORY_REGION(block + rg.first, rg.second);
  launch(dsa::k_source_rows<Desc>, 3, 6, 256, backwards, (const uint8_t *)arena, (const Desc *)descs, 5u, (const dsa::SrcRowsMesh *)block, block);
  for (uint32_t m = 0; m < 4; ++m)
    for (uint32_t a = 0; a < na; ++a) {
      const uint32_t *out = (const uint32_t *)(block + table[m].att[a].out);
      const uint32_t ne = (uint32_t)entry_rows[a].size();
      for (uint32_t p = 0; p < cap_points; ++p) {
        uint32_t want = 0xCDCDCDCDu;                           // untouched: behind the points, and all of a mesh that failed or is not the tracked stream
        if (m == 0 && p < points) want = maps[a][p] < ne ? entry_rows[a][maps[a][p]] : 0xFFFFFFFFu;
        if (m == 1 && p < points) want = p < ne ? p : 0xFFFFFFFFu;
        if (out[p] != want) FAIL("source rows of mesh %u, attribute %u, point %u: %u, expected %u", m, a, p, out[p], want);
      }
    }
  return true;
}

static bool run(uint32_t index, const In &m, bool backwards) {
  // the request of dsa_encode_rows_batch for this mesh alone
  std::vector<dsa_attribute_input> atts(m.extras.size());
  std::vector<dsa_attribute_corners> corners(m.extras.size());
  if (!atts.empty()) { memset(atts.data(), 0, sizeof(dsa_attribute_input) * atts.size()); memset(corners.data(), 0, sizeof(dsa_attribute_corners) * corners.size()); }
  bool any_ids = false;
  for (size_t k = 0; k < m.extras.size(); ++k) {
    const Extra &x = m.extras[k];
    atts[k].attribute_type = x.data_type == 9 ? 3 : 4; atts[k].data_type = (int32_t)x.data_type; atts[k].num_components = x.nc;
    atts[k].unique_id = DSA_UNIQUE_ID_DEFAULT; atts[k].values = x.values.data();
    if (x.rows) { corners[k].corners = x.ids.data(); corners[k].num_rows = x.rows; any_ids = true; }
  }
  dsa_mesh_attr_input am;
  memset(&am, 0, sizeof(am));
  dsa_mesh_input &mi = am.mesh.mesh;
  mi.num_vertices = m.nv; mi.num_faces = m.nf; mi.positions = m.pos.data(); mi.faces = m.faces.data();
  mi.normals = m.normals ? m.nrm.data() : nullptr; mi.texcoords = m.texcoords ? m.uv.data() : nullptr;
  mi.generic = m.generic ? m.gen.data() : nullptr; mi.generic_components = m.generic;
  if (m.nn) { am.mesh.normal_corners = m.nid.data(); am.mesh.num_normals = m.nn; }
  if (m.nu) { am.mesh.texcoord_corners = m.uid.data(); am.mesh.num_texcoords = m.nu; }
  am.attributes = atts.empty() ? nullptr : atts.data(); am.num_attributes = (uint32_t)atts.size();
  dsa_mesh_attribute_corners mc;
  memset(&mc, 0, sizeof(mc));
  mc.attributes = corners.data();
  EncRequest rq;
  rq.n = 1; rq.meshes = &am;
  memset(&rq.level, 0, sizeof(rq.level));
  {
    synth::Options d;
    dsa_encode_options &o = rq.level.ex.base;
    o.position_bits = d.pos_bits; o.texcoord_bits = d.uv_bits; o.normal_bits = d.normal_bits;
    o.single_connectivity = d.single_connectivity; o.symbol_scheme = d.force_scheme; o.compression_level = d.compression_level;
    o.position_prediction = d.pos_prediction; o.texcoord_prediction = d.uv_prediction;
  }
  rq.level.traversal_method = (int32_t)m.traversal;
  rq.repair = m.repair != 0; rq.corner_repair = m.repair == 2;
  rq.weld = m.form == 2; rq.weld_attributes = m.weld_attributes != 0;
  rq.att_corners = any_ids ? &mc : nullptr;
  rq.track_rows = true;
  EncChunk ck(rq, 0, 1, 1);
  std::vector<std::pair<uint64_t, uint64_t>> log;
  ck.region_log = &log;
  if (rq.weld) {                                             // enc_stage_weld, the host's path
    ck.weld.assign(1, synth::Welded()); ck.weld_attrs.assign(1, {}); ck.weld_corners.assign(1, {});
    std::vector<synth::WeldSeg> key, listed;
    if (!enc_weld_check(ck, 0, key, &listed)) FAIL("the weld refuses it: %s", ck.E->messages[0].c_str());
    synth::weld_points(m.nv, m.faces.data(), m.nf, key, mi.normals, mi.texcoords, ck.weld[0], listed);
    ck.welded.resize(1);
    enc_weld_view(ck, 0);
  }
  enc_begin_plans(ck, true, true);
  enc_plan_mesh(ck, 0);
  if (!ck.good(0)) FAIL("refused: %s", ck.E->messages[0].c_str());
  enc_layout(ck);
  const EncLayout &L = ck.L;
  const uint32_t na = (uint32_t)ck.plans[0].atts.size();
  if (L.rows.size() != na || L.rows_of_stream.size() != L.streams.size()) FAIL("%zu row records for %u attributes", L.rows.size(), na);
  // what the host coder says, on a plan of its own
  std::vector<std::vector<uint32_t>> want;
  {
    synth::MeshPlan pl;
    synth::Options mo = ck.opt;
    mo.generic_components = ck.ins[0].generic ? (int32_t)ck.mesh(0).generic_components : 1;
    synth::plan_mesh(ck.ins[0], mo, pl);
    synth::plan_entry_rows(pl, want);
    if (rq.weld)
      for (size_t k = 0; k < want.size(); ++k) {
        const std::vector<uint32_t> &point = synth::weld_row_points(ck.weld[0], pl.atts[k]);
        for (uint32_t &r : want[k]) { if (r >= point.size()) FAIL("row %u outside the weld's %zu classes", r, point.size()); r = point[r]; }
      }
  }
  if (want.size() != na) FAIL("%zu attributes planned, %u laid out", want.size(), na);
  // the arena as the chunk's uploads fill it, everything outside its regions poisoned
  std::vector<uint8_t> store(L.total_bytes + 256, 0);
  uint8_t *arena = store.data();
  if (!L.uploads_a.empty()) FAIL("host connectivity has no phase A");
  for (const EncUpload &u : L.uploads) { if (u.narrow) FAIL("a narrowed upload with host connectivity"); if (u.bytes) memcpy(arena + u.off, u.src, u.bytes); }
  ASAN_POISON_MEMORY_REGION(arena, store.size());
  for (auto &rg : log) ASAN_UNPOISON_MEMORY_REGION(arena + rg.first, rg.second);
  launch(dsa::k_enc_entry_rows<dsa::EncStream>, 2, (uint32_t)L.rows.size() + 1, 256, backwards, arena, L.rows.data(), (uint32_t)L.rows.size(), L.streams.data());
  for (uint32_t k = 0; k < na; ++k) {
    const dsa::EncRows &R = L.rows[L.rows_of_stream[L.first_stream[0] + k]];
    const dsa::EncStream &S = L.streams[R.stream];
    if (R.stream != L.first_stream[0] + k || S.nv != want[k].size() || R.cap < S.nv) FAIL("attribute %u: %u entries laid out (room for %u), %zu coded", k, S.nv, R.cap, want[k].size());
    if (rq.weld != (R.num_points != 0)) FAIL("attribute %u: %u representative points", k, R.num_points);
    const uint32_t *got = (const uint32_t *)(arena + R.out);
    for (uint32_t e = 0; e < S.nv; ++e) if (got[e] != want[k][e]) FAIL("attribute %u, entry %u: row %u, the host coder says %u", k, e, got[e], want[k][e]);
  }
  ASAN_UNPOISON_MEMORY_REGION(arena, store.size());
  return source_rows(index, backwards, want);
}

template <class T>
static bool get(FILE *f, std::vector<T> &v, size_t count) { v.resize(count); return count == 0 || fread(v.data(), sizeof(T), count, f) == count; }

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: encrows_host <meshes.bin>\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  std::vector<In> meshes(count);
  for (auto &m : meshes) {
    uint32_t head[12];
    if (fread(head, 4, 12, f) != 12) return 2;
    m.form = head[0]; m.nv = head[1]; m.nf = head[2]; m.normals = head[3]; m.texcoords = head[4]; m.nn = head[5]; m.nu = head[6];
    m.generic = head[7]; m.repair = head[8]; m.traversal = head[9]; m.weld_attributes = head[10];
    if (head[11] > 16 || m.generic > 4) return 2;
    if (!get(f, m.faces, 3ull * m.nf) || !get(f, m.pos, 3ull * m.nv)) return 2;
    if (m.normals && (!get(f, m.nrm, 3ull * (m.nn ? m.nn : m.nv)) || (m.nn && !get(f, m.nid, 3ull * m.nf)))) return 2;
    if (m.texcoords && (!get(f, m.uv, 2ull * (m.nu ? m.nu : m.nv)) || (m.nu && !get(f, m.uid, 3ull * m.nf)))) return 2;
    if (m.generic && !get(f, m.gen, (size_t)m.generic * m.nv)) return 2;
    m.extras.resize(head[11]);
    for (Extra &x : m.extras) {
      uint32_t h3[3];
      if (fread(h3, 4, 3, f) != 3) return 2;
      x.data_type = h3[0]; x.nc = h3[1]; x.rows = h3[2];
      if (x.nc < 1 || x.nc > 4) return 2;
      if (!get(f, x.values, synth::data_type_size((int)x.data_type) * (size_t)x.nc * (x.rows ? x.rows : m.nv))) return 2;
      if (x.rows && !get(f, x.ids, 3ull * m.nf)) return 2;
    }
  }
  fclose(f);
  for (uint32_t i = 0; i < count; ++i)
    for (int backwards = 0; backwards < 2; ++backwards)
      if (!run(i, meshes[i], backwards != 0)) return 1;
  printf("encrows: %u meshes, entry rows and source rows as the host coder has them, forwards and backwards\n", count);
  return 0;
}
