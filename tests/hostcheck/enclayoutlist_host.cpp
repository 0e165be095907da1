// tests/hostcheck/enclayoutlist_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The encoder's arena layout of the product (draco-sharp_amd/csrc/dsa_encode_layout.h) for attributes of the list given per corner
// (dsa_encode_corner_attributes_batch), compiled for the host with AddressSanitizer + UBSan: enc_take_extras with a
// dsa_attribute_corners array, the id checks of enc_plan_mesh, enc_extra_caps over the rows the ids index, EncChunk::rows_of /
// att_corners, enc_layout -- and the weld view (enc_weld_check, enc_weld_view over synth::weld_points with listed attributes) in
// front of them.  Every array of the caller's is a heap block of exactly the size the structs state, so a read past a row count is
// an error of the sanitizer.  For every chunk the region assertions of enclayout_host.cpp (aligned, inside the arena, uploads
// exactly the regions below input_bytes, no overlap, every offset of a record a region handed out and large enough), and for every
// listed attribute with ids: its stream has the attribute's row count, its source region that many rows, its id region the narrow
// or the wide form by that count, 3 F entries on the device path, an integer attribute's histogram the span of its R rows.
// A mesh with an id at its row count and one with a reserved word set fail alone with their messages, the rest is laid out around
// them.  Nothing here is linked into the product.
//
//   enclayoutlist_host <meshes.bin>   file: u32 count, then per mesh u32 nv, nf, per_point; f32 pos[3 nv]; u32 faces[3 nf]; u32 mask
//                                 (bit 0 normal ids, bit 1 uv ids; 0 for a per-point mesh), per set bit: u32 rows, u32 ids[3 nf];
//                                 u32 extras, per extra u32 attribute_type, data_type, nc, has_ids, rows; u32 ids[3 nf] if has_ids;
//                                 rows * nc elements
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

// the defaults of the library's option structs (dsa_encode.h, which needs HIP)
static void default_options(EncRequest &rq) {
  memset(&rq.level, 0, sizeof(rq.level));
  memset(&rq.seq, 0, sizeof(rq.seq));
  synth::Options d;
  dsa_encode_options &o = rq.level.ex.base;
  o.position_bits = d.pos_bits; o.texcoord_bits = d.uv_bits; o.normal_bits = d.normal_bits;
  o.single_connectivity = d.single_connectivity; o.symbol_scheme = d.force_scheme; o.compression_level = d.compression_level;
  o.position_prediction = d.pos_prediction; o.texcoord_prediction = d.uv_prediction;
  rq.seq.base = o;
  rq.seq.geometry = 1;
}

static std::string g_case;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s: ", g_case.c_str()); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return false; } } while (0)

typedef std::vector<std::pair<uint64_t, uint64_t>> Log;

static bool check_layout(const EncChunk &ck, const Log &log, int bad_mesh, int bad_mesh2 = -1) {
  const EncLayout &L = ck.L;
  auto al = [](uint64_t b) { return (b + 255) & ~255ull; };
  std::map<uint64_t, uint64_t> region;          // offset -> bytes (a region of no bytes shares its offset with the next: the larger counts)
  for (const auto &r : log) {
    CHECK(r.first % 256 == 0, "region at %llu is not 256-byte aligned", (unsigned long long)r.first);
    CHECK(r.first + r.second <= L.total_bytes, "region at %llu + %llu lies outside the arena of %llu", (unsigned long long)r.first, (unsigned long long)r.second, (unsigned long long)L.total_bytes);
    uint64_t &b = region[r.first];
    CHECK(b == 0 || r.second == 0, "two regions at %llu", (unsigned long long)r.first);
    b = std::max(b, r.second);
  }
  uint64_t end = 0;
  for (const auto &r : region) { CHECK(r.first >= end, "regions overlap at %llu", (unsigned long long)r.first); end = r.first + r.second; }
  // the uploads: the regions below input_bytes, one for one and in order
  std::vector<EncUpload> ups = L.uploads_a;
  ups.insert(ups.end(), L.uploads.begin(), L.uploads.end());
  CHECK(ck.host_conn || ck.rq.sequential || L.uploads_a.size() > 0 || L.streams.empty(), "no phase A on the device path");
  CHECK(!(ck.host_conn || ck.rq.sequential) || L.uploads_a.empty(), "phase A without device connectivity");
  uint64_t at = 0;
  for (size_t u = 0; u < ups.size(); ++u) {
    CHECK(ups[u].off == at, "upload %zu at %llu, expected %llu (ascending, one behind the other)", u, (unsigned long long)ups[u].off, (unsigned long long)at);
    CHECK(ups[u].off + ups[u].bytes <= L.input_bytes, "upload %zu ends behind input_bytes", u);
    CHECK(ups[u].src != nullptr || ups[u].bytes == 0, "upload %zu has no source", u);
    CHECK(u < log.size() && log[u].first == ups[u].off && log[u].second == ups[u].bytes, "upload %zu is not the %zu-th region handed out", u, u);
    at = al(ups[u].off + ups[u].bytes);
  }
  CHECK(at == L.input_bytes, "input_bytes %llu is not the end of the last upload's region %llu", (unsigned long long)L.input_bytes, (unsigned long long)at);
  for (size_t r = ups.size(); r < log.size(); ++r)
    CHECK(log[r].first >= L.input_bytes, "a region of the kernels at %llu lies among the inputs (input_bytes %llu)", (unsigned long long)log[r].first, (unsigned long long)L.input_bytes);
  // the records point at regions handed out
  auto handed = [&](uint64_t off) { return off == 0 || region.count(off) != 0; };
  auto sized = [&](uint64_t off, uint64_t bytes) { auto it = region.find(off); return it != region.end() && it->second >= bytes; };
#define FIELD(rec, f) CHECK(handed((rec).f), #rec "." #f " = %llu is no region handed out", (unsigned long long)(rec).f)
  CHECK(L.first_stream.size() == ck.n + 1 && L.first_stream[ck.n] == L.streams.size(), "first_stream does not cover the streams");
  for (uint32_t i = 0; i < ck.n; ++i) {
    if ((int)i == bad_mesh || (int)i == bad_mesh2) {
      CHECK(!ck.good(i) && L.first_stream[i] == L.first_stream[i + 1], "the mesh that fails its checks has streams");
      if (!L.conns.empty()) CHECK(L.conns[i].F == 0 && L.conns[i].status == dsa::ENC_ISOLATED && L.conns[i].faces == 0 && L.conns[i].opp == 0, "the mesh that fails its checks has arrays");
      continue;
    }
    CHECK(ck.good(i), "mesh %u refused: %s", i, ck.E->messages[i].c_str());
    const size_t na = ck.plans[i].atts.size();
    const bool valence = ck.valence_of(i);
    const bool compressed = ck.rq.sequential && ck.rq.seq.geometry == 1 && ck.rq.seq.compress_connectivity == 1;
    CHECK(L.first_stream[i + 1] - L.first_stream[i] == na + (valence ? 6 : 0) + (compressed ? 1 : 0), "mesh %u has %u streams", i, L.first_stream[i + 1] - L.first_stream[i]);
    for (uint32_t s = L.first_stream[i]; s < L.first_stream[i + 1]; ++s) {
      const dsa::EncStream &S = L.streams[s];
      FIELD(S, src); FIELD(S, e2v); FIELD(S, ops); FIELD(S, vals); FIELD(S, d); FIELD(S, syms); FIELD(S, bl); FIELD(S, hist_raw); FIELD(S, out_rans); FIELD(S, out_bits);
      FIELD(S, prob); FIELD(S, cum); FIELD(S, plan_order); FIELD(S, plan_tmp); FIELD(S, pos_vals); FIELD(S, t_c2p); FIELD(S, t_c2a); FIELD(S, t_opp); FIELD(S, t_d2c); FIELD(S, t_v2d);
      FIELD(S, ori); FIELD(S, flags);
      const uint64_t table = 4ull * std::max<uint32_t>(S.hist_cap, 64);
      CHECK(S.hist_cap > 0 && sized(S.hist_raw, 4ull * S.hist_cap) && sized(S.prob, table) && sized(S.cum, table) && sized(S.plan_order, table) && sized(S.plan_tmp, table), "stream %u: histogram or tables too small", s);
      if (S.kind != 3) {
        const uint64_t elem = S.kind == 2 ? synth::data_type_size((int)S.elem) : 4;
        CHECK(S.src < L.input_bytes && sized(S.src, elem * S.rows * S.nc_out), "stream %u: source values", s);
        CHECK(sized(S.vals, 4ull * S.rows * S.nc) && sized(S.d, 4ull * S.nv * S.nc) && sized(S.syms, 4ull * S.nv * S.nc) && sized(S.bl, S.nv), "stream %u: value regions too small", s);
        CHECK((S.linear != 0) == (S.vals == S.d) && (S.linear != 0) == ck.rq.sequential, "stream %u: linear", s);
        CHECK(S.out_cap >= 4u * S.nv * S.nc + 16u && sized(S.out_rans, S.out_cap) && sized(S.out_bits, S.out_cap), "stream %u: output regions too small", s);
        if (!ck.rq.sequential) CHECK(sized(S.e2v, 4ull * S.nv) && sized(S.ops, 12ull * S.nv), "stream %u: entry maps too small", s);
        const synth::PortableAttr &a = ck.plans[i].atts[s - L.first_stream[i]];
        if (!ck.rq.sequential && enc_topo_scheme(a)) CHECK(S.t_c2a != 0 && S.t_opp != 0 && S.t_d2c != 0 && S.t_v2d != 0 && S.t_nc3 == 3 * ck.mesh(i).num_faces, "stream %u: no topology view", s);
        if (!ck.rq.sequential && enc_topo_scheme(a) && !enc_multi_scheme(a)) CHECK(S.pos_vals == L.streams[L.first_stream[i]].vals && S.flags != 0, "stream %u: positions or flags of its scheme", s);
        if (!ck.rq.sequential && a.prediction == 4 && a.seq_type != 3) CHECK(S.ori != 0 && sized(S.flags, 4ull * (S.cr_at[3] + 1)), "stream %u: crease lists", s);
      } else if (S.nv) {
        CHECK(sized(S.syms, 4ull * S.nv) && sized(S.bl, S.nv) && sized(S.out_rans, S.out_cap) && sized(S.out_bits, S.out_cap) && S.out_cap >= 4u * S.nv + 16u, "stream %u: list regions too small", s);
        CHECK((S.syms < L.input_bytes) == ck.host_conn, "stream %u: list symbols on the wrong side of input_bytes", s);
      }
    }
    if (L.conns.empty()) continue;
    const dsa::EncConn &C = L.conns[i];
    const uint64_t F = C.F, V = C.V;
    CHECK(F == ck.mesh(i).num_faces && V == ck.mesh(i).num_vertices && C.status == dsa::ENC_OK, "mesh %u: connectivity record", i);
    FIELD(C, faces); FIELD(C, faces16); FIELD(C, opp); FIELD(C, voff); FIELD(C, vcur); FIELD(C, vlist); FIELD(C, vcorner); FIELD(C, vvis); FIELD(C, frec); FIELD(C, stack); FIELD(C, processed);
    FIELD(C, init_corners); FIELD(C, symbols); FIELD(C, start_bits); FIELD(C, splits); FIELD(C, d2c); FIELD(C, v2d); FIELD(C, e2v); FIELD(C, ops);
    FIELD(C, init_time); FIELD(C, vtime); FIELD(C, vval); FIELD(C, vc2v); FIELD(C, vctx); FIELD(C, vsyms); FIELD(C, vbl); FIELD(C, vrans); FIELD(C, vbits);
    FIELD(C, pd_d2c); FIELD(C, pd_v2d); FIELD(C, pd_e2v); FIELD(C, pd_ops); FIELD(C, pd_next); FIELD(C, pd_degree); FIELD(C, pd_fvis);
    CHECK(sized(C.faces, 12 * F) && sized(C.opp, 12 * F) && sized(C.frec, 32 * F) && sized(C.e2v, 4 * V) && sized(C.ops, 12 * V) && sized(C.voff, 4 * (V + 1)), "mesh %u: connectivity regions too small", i);
    CHECK(C.faces_narrow ? (C.faces16 < L.input_bytes && C.faces >= L.input_bytes) : C.faces < L.input_bytes, "mesh %u: faces on the wrong side of input_bytes", i);
    CHECK((C.pd_e2v != 0) == ck.want_pd && (C.vsyms != 0) == valence && (C.vstream != DSA_INVALID) == valence, "mesh %u: regions of the order / the valence lists", i);
    if (valence) CHECK(C.vstream == L.first_stream[i] + na, "mesh %u: vstream", i);
  }
  for (const dsa::EncSeam &Z : L.seams) {
    FIELD(Z, ids); FIELD(Z, edge_seam); FIELD(Z, vert_seam); FIELD(Z, afirst); FIELD(Z, aoff); FIELD(Z, c2av); FIELD(Z, opp2); FIELD(Z, v2lm); FIELD(Z, avis); FIELD(Z, frec); FIELD(Z, stack);
    FIELD(Z, d2c); FIELD(Z, v2d); FIELD(Z, e2v); FIELD(Z, ops); FIELD(Z, rank); FIELD(Z, rcorner); FIELD(Z, eoff); FIELD(Z, bits);
    const uint64_t F = L.conns[Z.mesh].F;
    CHECK(Z.ids < L.input_bytes && sized(Z.ids, (Z.ids_narrow ? 6 : 12) * F) && sized(Z.ops, 36 * F) && sized(Z.e2v, 12 * F), "seam record of mesh %u: regions too small", Z.mesh);
    const dsa::EncStream &S = L.streams[Z.stream];
    CHECK(Z.stream >= L.first_stream[Z.mesh] && Z.stream < L.first_stream[Z.mesh + 1] && S.e2v == Z.e2v && S.ops == Z.ops && S.rows == Z.rows, "seam record of mesh %u: not its stream's", Z.mesh);
  }
  for (const dsa::EncSeqIdx &X : L.idx) {
    FIELD(X, faces);
    CHECK(X.faces < L.input_bytes && sized(X.faces, (X.narrow ? 2ull : 4ull) * X.count) && L.streams[X.stream].kind == 3 && L.streams[X.stream].nv == X.count, "index record");
  }
  return true;
}

struct Extra { uint32_t att_type, data_type, nc, has_ids, rows; std::vector<uint32_t> ids; std::vector<uint8_t> values; };
struct In { uint32_t nv, nf, per_point, mask; std::vector<float> pos; std::vector<uint32_t> faces; uint32_t rows[2]; std::vector<uint32_t> ids[2]; std::vector<Extra> extras; };

// the mesh of `m` in the C structs; `keep` owns the arrays of exactly the sizes stated
struct Native {
  std::vector<float> nrm, uv;
  std::vector<dsa_attribute_input> list;
  std::vector<dsa_attribute_corners> ids;
};
static void native_of(const In &m, Native &k, dsa_mesh_attr_input &am, dsa_mesh_attribute_corners &mc) {
  memset(&am, 0, sizeof(am)); memset(&mc, 0, sizeof(mc));
  dsa_mesh_input &mi = am.mesh.mesh;
  mi.num_vertices = m.nv; mi.num_faces = m.nf; mi.positions = m.pos.data(); mi.faces = m.faces.data();
  if (!m.per_point) {
    const uint32_t rn = (m.mask & 1) ? m.rows[0] : m.nv, ru = (m.mask & 2) ? m.rows[1] : m.nv;
    k.nrm.assign((size_t)3 * rn, 0.0f); k.uv.assign((size_t)2 * ru, 0.25f);
    mi.normals = k.nrm.data(); mi.texcoords = k.uv.data();
    if (m.mask & 1) { am.mesh.normal_corners = m.ids[0].data(); am.mesh.num_normals = rn; }
    if (m.mask & 2) { am.mesh.texcoord_corners = m.ids[1].data(); am.mesh.num_texcoords = ru; }
  }
  k.list.resize(m.extras.size()); k.ids.resize(m.extras.size());
  if (!k.list.empty()) { memset(k.list.data(), 0, k.list.size() * sizeof(dsa_attribute_input)); memset(k.ids.data(), 0, k.ids.size() * sizeof(dsa_attribute_corners)); }
  bool any = false;
  for (size_t e = 0; e < m.extras.size(); ++e) {
    const Extra &x = m.extras[e];
    k.list[e].attribute_type = (int32_t)x.att_type; k.list[e].data_type = (int32_t)x.data_type; k.list[e].num_components = x.nc;
    k.list[e].unique_id = 0xFFFFFFFFu; k.list[e].values = x.values.data();
    if (x.has_ids) { k.ids[e].corners = x.ids.data(); k.ids[e].num_rows = x.rows; any = true; }
  }
  am.attributes = k.list.empty() ? nullptr : k.list.data(); am.num_attributes = (uint32_t)k.list.size();
  if (any) mc.attributes = k.ids.data();
}

static int32_t element(const Extra &x, size_t k) {
  const uint8_t *p = x.values.data();
  switch (x.data_type) {
    case 1: return ((const int8_t *)p)[k]; case 2: return p[k];
    case 3: return ((const int16_t *)p)[k]; case 4: return ((const uint16_t *)p)[k];
    default: return ((const int32_t *)p)[k];
  }
}

// what the layout must say of the listed attributes of good mesh i of a chunk
static bool check_listed(const EncChunk &ck, uint32_t i, const In &m, const std::vector<uint32_t> &rows, const std::vector<bool> &has_ids) {
  const EncLayout &L = ck.L;
  const size_t na = ck.plans[i].atts.size(), first = na - m.extras.size();
  const uint64_t F = ck.mesh(i).num_faces, V = ck.mesh(i).num_vertices;
  for (size_t e = 0; e < m.extras.size(); ++e) {
    const Extra &x = m.extras[e];
    const synth::PortableAttr &a = ck.plans[i].atts[first + e];
    const dsa::EncStream &S = L.streams[L.first_stream[i] + first + e];
    const uint32_t R = has_ids[e] ? rows[e] : (uint32_t)V;
    CHECK((a.corner_value != nullptr) == (bool)has_ids[e] && ck.rows_of(i, a) == R && S.rows == R, "mesh %u attribute %zu: %u rows, the attribute has %u", i, e, S.rows, R);
    CHECK(ck.ids_narrow(i, a) == (R <= 65536), "mesh %u attribute %zu: id width", i, e);
    CHECK(S.nc == x.nc && S.kind == (x.data_type == 9 ? 0u : 2u), "mesh %u attribute %zu: stream kind", i, e);
    if (x.data_type != 9) {
      uint32_t want = 258;
      if (synth::data_type_size((int)x.data_type) > 1) {
        int32_t lo = element(x, 0), hi = lo;
        for (size_t k = 1; k < (size_t)R * x.nc; ++k) { const int32_t v = element(x, k); lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
        want = dsa::enc_integer_hist_cap(lo, hi);
      }
      CHECK(S.hist_cap == want, "mesh %u attribute %zu: hist_cap %u, the values of its %u rows span %u", i, e, S.hist_cap, R, want);
    }
    if (!has_ids[e]) continue;
    if (ck.host_conn) { CHECK(S.nv == ck.att_e2v[i][first + e].size(), "mesh %u attribute %zu: entries", i, e); continue; }
    bool found = false;
    for (const dsa::EncSeam &Z : L.seams) {
      if (Z.mesh != i || Z.stream != L.first_stream[i] + first + e) continue;
      found = true;
      CHECK(Z.rows == R && (Z.ids_narrow != 0) == (R <= 65536), "mesh %u attribute %zu: seam record", i, e);
    }
    CHECK(found, "mesh %u attribute %zu: no seam record", i, e);
    CHECK(S.out_cap >= 4u * 3u * (uint32_t)F * S.nc + 16u, "mesh %u attribute %zu: not sized for 3 F entries", i, e);
  }
  return true;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: enclayoutlist_host <meshes.bin>\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  std::vector<In> meshes(count);
  for (auto &m : meshes) {
    uint32_t h[3];
    if (fread(h, 4, 3, f) != 3) return 2;
    m.nv = h[0]; m.nf = h[1]; m.per_point = h[2];
    m.pos.resize((size_t)3 * m.nv); m.faces.resize((size_t)3 * m.nf);
    if (fread(m.pos.data(), 4, m.pos.size(), f) != m.pos.size() || fread(m.faces.data(), 4, m.faces.size(), f) != m.faces.size()) return 2;
    if (fread(&m.mask, 4, 1, f) != 1) return 2;
    for (int a = 0; a < 2; ++a) {
      m.rows[a] = 0;
      if (!(m.mask >> a & 1)) continue;
      if (fread(&m.rows[a], 4, 1, f) != 1) return 2;
      m.ids[a].resize((size_t)3 * m.nf);
      if (fread(m.ids[a].data(), 4, m.ids[a].size(), f) != m.ids[a].size()) return 2;
    }
    uint32_t ne = 0;
    if (fread(&ne, 4, 1, f) != 1 || ne > 12) return 2;
    m.extras.resize(ne);
    for (Extra &x : m.extras) {
      uint32_t d[5];
      if (fread(d, 4, 5, f) != 5) return 2;
      x.att_type = d[0]; x.data_type = d[1]; x.nc = d[2]; x.has_ids = d[3]; x.rows = d[4];
      if (x.has_ids) { x.ids.resize((size_t)3 * m.nf); if (fread(x.ids.data(), 4, x.ids.size(), f) != x.ids.size()) return 2; }
      x.values.resize((size_t)x.rows * x.nc * synth::data_type_size((int)x.data_type));
      if (!x.values.empty() && fread(x.values.data(), 1, x.values.size(), f) != x.values.size()) return 2;
    }
  }
  fclose(f);
  uint32_t chunks = 0, regions = 0, with_ids = 0, views_with = 0, views_without = 0;
  // ---- explicit ids: the meshes that are not per point, and in the middle two copies of the first mesh with ids that must fail
  // alone -- an id at the row count (on its last corner), a reserved word of dsa_attribute_corners
  {
    std::vector<In> batch;
    for (const In &m : meshes) if (!m.per_point) batch.push_back(m);
    int first_ids = -1;
    for (size_t i = 0; i < batch.size() && first_ids < 0; ++i) for (const Extra &x : batch[i].extras) if (x.has_ids) first_ids = (int)i;
    if (first_ids < 0) { fprintf(stderr, "no mesh with ids on a listed attribute\n"); return 2; }
    const uint32_t bad = (uint32_t)batch.size() / 2;
    size_t bad_extra = 0;
    {
      In b = batch[first_ids];
      while (!b.extras[bad_extra].has_ids) ++bad_extra;
      In r = b;
      b.extras[bad_extra].ids.back() = b.extras[bad_extra].rows;
      batch.insert(batch.begin() + bad, r);              // bad + 1: the reserved word (set below)
      batch.insert(batch.begin() + bad, b);              // bad: the id
    }
    const uint32_t n = (uint32_t)batch.size();
    std::vector<Native> keep(n);
    std::vector<dsa_mesh_attr_input> in(n);
    std::vector<dsa_mesh_attribute_corners> cor(n);
    for (uint32_t i = 0; i < n; ++i) native_of(batch[i], keep[i], in[i], cor[i]);
    keep[bad + 1].ids[bad_extra].reserved = 1;
    char id_message[64], reserved_message[96];
    snprintf(id_message, sizeof(id_message), "attribute %zu id out of range", bad_extra);
    snprintf(reserved_message, sizeof(reserved_message), "attribute %zu: dsa_attribute_corners.reserved is not zero", bad_extra);
    for (int host_conn = 0; host_conn < 2; ++host_conn)
      for (int traversal = 0; traversal < 3; traversal += 2)
        for (int scheme = 0; scheme < 2; ++scheme)
          for (int valence = 0; valence < 2; ++valence) {
            EncRequest rq;
            default_options(rq);
            rq.n = n; rq.meshes = in.data(); rq.att_corners = cor.data();
            rq.level.multi_parallelogram = scheme ? 4 : 0;
            rq.level.ex.edgebreaker_method = valence ? 2 : 0;
            rq.level.traversal_method = traversal;
            char name[160];
            snprintf(name, sizeof(name), "ids: host_conn %d traversal %d scheme %d valence %d", host_conn, traversal, scheme, valence);
            g_case = name;
            for (uint32_t base = 0; base < n; base += (n + 1) / 2) {      // a chunk that starts in the middle of the request
              const uint32_t cnt = std::min(n - base, (n + 1) / 2);
              EncChunk ck(rq, base, cnt, n);
              Log log;
              ck.region_log = &log;
              enc_begin_plans(ck, host_conn != 0, true);
              for (uint32_t i = 0; i < cnt; ++i) enc_plan_mesh(ck, i);
              int here[2] = {-1, -1};
              for (uint32_t b = bad; b <= bad + 1; ++b) {
                if (b < base || b >= base + cnt) continue;
                here[b - bad] = (int)(b - base);
                const char *want = b == bad ? id_message : reserved_message;
                const int32_t status = b == bad ? DSA_ERR_INVALID_DATA : DSA_ERR_INVALID_ARGUMENT;
                if (ck.good(b - base) || ck.E->status[b - base] != status || ck.E->messages[b - base] != want) {
                  fprintf(stderr, "%s: bad mesh %u: status %d '%s'\n", name, b, (int)ck.E->status[b - base], ck.E->messages[b - base].c_str());
                  return 1;
                }
              }
              enc_layout(ck);
              if (!check_layout(ck, log, here[0], here[1])) return 1;
              for (uint32_t i = 0; i < cnt; ++i) {
                if ((int)i == here[0] || (int)i == here[1]) continue;
                const In &m = batch[base + i];
                std::vector<uint32_t> rows;
                std::vector<bool> ids;
                for (const Extra &x : m.extras) { rows.push_back(x.rows); ids.push_back(x.has_ids != 0); with_ids += x.has_ids ? 1u : 0u; }
                if (!check_listed(ck, i, m, rows, ids)) return 1;
              }
              ++chunks; regions += (uint32_t)log.size();
            }
          }
  }
  // ---- the weld view: the per-point meshes welded by the host coder, with the listed attributes in the vertex key and alone
  {
    std::vector<In> batch;
    for (const In &m : meshes) if (m.per_point) batch.push_back(m);
    const uint32_t n = (uint32_t)batch.size();
    std::vector<Native> keep(n);
    std::vector<dsa_mesh_attr_input> in(n);
    std::vector<dsa_mesh_attribute_corners> cor(n);
    for (uint32_t i = 0; i < n; ++i) native_of(batch[i], keep[i], in[i], cor[i]);
    for (int weld_attributes = 0; weld_attributes < 2 && n; ++weld_attributes)
      for (int host_conn = 0; host_conn < 2; ++host_conn) {
        EncRequest rq;
        default_options(rq);
        rq.n = n; rq.meshes = in.data(); rq.weld = true; rq.weld_attributes = weld_attributes != 0;
        rq.level.ex.edgebreaker_method = host_conn ? 2 : 0;
        char name[160];
        snprintf(name, sizeof(name), "weld view: weld_attributes %d host_conn %d", weld_attributes, host_conn);
        g_case = name;
        EncChunk ck(rq, 0, n, n);
        Log log;
        ck.region_log = &log;
        ck.weld.assign(n, synth::Welded()); ck.weld_attrs.assign(n, {}); ck.weld_corners.assign(n, {});
        for (uint32_t i = 0; i < n; ++i) {                      // (the host path of enc_stage_weld)
          std::vector<synth::WeldSeg> key, listed;
          if (!enc_weld_check(ck, i, key, &listed)) { fprintf(stderr, "%s: mesh %u: %s\n", name, i, ck.E->messages[i].c_str()); return 1; }
          const dsa_mesh_input &m = rq.mesh(i);
          synth::weld_points(m.num_vertices, m.faces, m.num_faces, key, m.normals, m.texcoords, ck.weld[i], listed);
        }
        ck.welded.resize(n);
        for (uint32_t i = 0; i < n; ++i) enc_weld_view(ck, i);
        enc_begin_plans(ck, host_conn != 0, true);
        for (uint32_t i = 0; i < n; ++i) enc_plan_mesh(ck, i);
        enc_layout(ck);
        if (!check_layout(ck, log, -1)) return 1;
        for (uint32_t i = 0; i < n; ++i) {
          const synth::Welded &w = ck.weld[i];
          const dsa_attribute_corners *ac = ck.att_corners(i);
          std::vector<uint32_t> rows;
          std::vector<bool> ids;
          bool any = false;
          for (size_t e = 0; e < batch[i].extras.size(); ++e) {
            const bool alone = e < w.listed.size() && !w.listed[e].per_vertex;
            rows.push_back(alone ? w.listed[e].keys.count : w.vertex.count);
            ids.push_back(alone);
            any = any || alone;
            if (alone && (!ac || ac[e].corners != w.listed[e].corners.data() || ac[e].num_rows != w.listed[e].keys.count || ck.attr(i).attributes[e].values != w.listed[e].rows.data())) {
              fprintf(stderr, "%s: mesh %u attribute %zu: the view does not point at the weld\n", name, i, e);
              return 1;
            }
            if (!alone && ac && ac[e].corners) { fprintf(stderr, "%s: mesh %u attribute %zu: ids no weld made\n", name, i, e); return 1; }
          }
          if ((ac != nullptr) != any || (!weld_attributes && any)) { fprintf(stderr, "%s: mesh %u: att_corners\n", name, i); return 1; }
          (any ? views_with : views_without) += 1;
          // the extras as the welded mesh carries them: heap blocks of the weld, exactly rows * row bytes
          In view = batch[i];
          for (size_t e = 0; e < view.extras.size(); ++e) {
            const std::vector<uint8_t> &src = e < w.listed.size() ? w.listed[e].rows : w.vertex_rows[1 + (e - w.listed.size())];
            view.extras[e].values = src;
            if (src.size() != (size_t)rows[e] * view.extras[e].nc * synth::data_type_size((int)view.extras[e].data_type)) { fprintf(stderr, "%s: mesh %u attribute %zu: welded row count\n", name, i, e); return 1; }
          }
          if (!check_listed(ck, i, view, rows, ids)) return 1;
        }
        ++chunks; regions += (uint32_t)log.size();
      }
  }
  printf("enclayoutlist: %u chunks laid out, %u regions checked, %u listed attributes with ids, weld views with ids %u, without %u\n", chunks, regions, with_ids, views_with, views_without);
  return 0;
}
