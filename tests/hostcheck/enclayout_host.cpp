// tests/hostcheck/enclayout_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The encoder's arena layout of the product (draco-sharp_amd/csrc/dsa_encode_layout.h: enc_plan_mesh + enc_layout for Edgebreaker
// streams, enc_check_sequential_mesh + enc_layout_sequential for sequential ones) compiled for the host with AddressSanitizer +
// UBSan and run on plans the host coder makes for the meshes of the input file, one chunk per setting.  For every chunk:
//   - every region handed out is 256-byte aligned and lies inside [0, total_bytes);
//   - the uploads are exactly the regions below input_bytes, in ascending order, phase A in front of phase B, and input_bytes is
//     the end of the last upload's region; every other region lies at or behind input_bytes;
//   - no two regions handed out overlap (the allocator's log; the intended aliases -- a mesh's shared e2v / ops, the topology
//     views, pos_vals, vals == d of a linear stream -- are one region each);
//   - every offset in an EncStream / EncConn / EncSeam / EncSeqIdx record is 0 or a region handed out, and the regions whose
//     sizes the record states (src, hist_raw, out_rans, out_bits, the tables) have them;
//   - a mesh that fails its checks has no streams and no arrays, and the others are laid out around it.
// Outside the counted chunks: the per-vertex and the corner form, widened by the library (enc_widen), lay a batch without ids out
// exactly like the widest form without its attribute list; and what each form answers to a generic attribute of 5 components.
// Nothing here is linked into the product.
//
//   enclayout_host <meshes.bin>   file: u32 count, then per mesh u32 nv, u32 nf, u32 faces[3 nf], u32 mask (bit 0 normal ids,
//                                 bit 1 uv ids), per set bit: u32 rows, u32 ids[3 nf]
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

static bool check_layout(const EncChunk &ck, const Log &log, int bad_mesh) {
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
    if ((int)i == bad_mesh) {
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

struct In { uint32_t nv, nf, mask; std::vector<uint32_t> faces; uint32_t rows[2]; std::vector<uint32_t> ids[2]; };

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: enclayout_host <meshes.bin>\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
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
  // the batch: the file's meshes with normals and texture coordinates, a generic attribute on every second one, one uint16 and one
  // float32 extra each; in the middle a copy of the first with a face index out of range
  const uint32_t n = count + 1, bad = count / 2;
  std::vector<In> batch;
  for (uint32_t i = 0; i < count; ++i) {
    if (i == bad) { In b = meshes[0]; b.faces[4] = b.nv + 7; batch.push_back(b); }
    batch.push_back(meshes[i]);
  }
  std::vector<dsa_mesh_attr_input> listed(n);
  std::vector<dsa_mesh_corner_input> corners(n);            // forms 1 and 0, which the library widens (enc_widen): no attribute list
  std::vector<dsa_mesh_input> vertex(n);
  std::vector<std::vector<float>> pos(n), nrm(n), uv(n), weights(n);
  std::vector<std::vector<uint8_t>> generic(n);
  std::vector<std::vector<uint16_t>> joints(n);
  std::vector<std::vector<dsa_attribute_input>> extra(n);
  for (uint32_t i = 0; i < n; ++i) {
    const In &m = batch[i];
    const uint32_t rn = (m.mask & 1) ? m.rows[0] : m.nv, ru = (m.mask & 2) ? m.rows[1] : m.nv;
    pos[i].assign((size_t)3 * m.nv, 0.5f); nrm[i].assign((size_t)3 * rn, 0.0f); uv[i].assign((size_t)2 * ru, 0.25f);
    generic[i].assign((size_t)2 * m.nv, 3); joints[i].resize((size_t)4 * m.nv); weights[i].assign((size_t)4 * m.nv, 0.25f);
    for (size_t k = 0; k < joints[i].size(); ++k) joints[i][k] = (uint16_t)((k * 37) % 900);
    dsa_mesh_attr_input &am = listed[i];
    memset(&am, 0, sizeof(am));
    dsa_mesh_input &mi = am.mesh.mesh;
    mi.num_vertices = m.nv; mi.num_faces = m.nf; mi.positions = pos[i].data(); mi.faces = m.faces.data(); mi.normals = nrm[i].data(); mi.texcoords = uv[i].data();
    if (i % 2) { mi.generic = generic[i].data(); mi.generic_components = 2; }
    if (m.mask & 1) { am.mesh.normal_corners = m.ids[0].data(); am.mesh.num_normals = rn; }
    if (m.mask & 2) { am.mesh.texcoord_corners = m.ids[1].data(); am.mesh.num_texcoords = ru; }
    extra[i].resize(2);
    memset(extra[i].data(), 0, 2 * sizeof(dsa_attribute_input));
    extra[i][0].attribute_type = 4; extra[i][0].data_type = 4; extra[i][0].num_components = 4; extra[i][0].unique_id = 0xFFFFFFFFu; extra[i][0].values = joints[i].data();
    extra[i][1].attribute_type = 4; extra[i][1].data_type = 9; extra[i][1].num_components = 4; extra[i][1].unique_id = 0xFFFFFFFFu; extra[i][1].quantization_bits = 10; extra[i][1].values = weights[i].data();
    am.attributes = extra[i].data(); am.num_attributes = 2;
    corners[i] = am.mesh;
    vertex[i] = am.mesh.mesh;            // (per-vertex form: only the batch without ids is run through it)
  }
  bool any_ids = false;
  for (const In &m : batch) any_ids = any_ids || m.mask != 0;
  uint32_t chunks = 0, regions = 0;
  // ---- Edgebreaker streams: the three forms x host / device connectivity x both orders x the prediction schemes x valence
  for (int form = 0; form < 3; ++form)
    for (int host_conn = 0; host_conn < 2; ++host_conn)
      for (int traversal = 0; traversal < 3; traversal += 2)
        for (int scheme = 0; scheme < 4; ++scheme)            // 0: parallelogram (1); 1: constrained multi-parallelogram (4); 2: + TexCoordsPortable (5) + GeometricNormal (6); 3: 4 + 5 + 6
          for (int valence = 0; valence < 2; ++valence) {
            if (form == 0 && any_ids) continue;
            EncRequest rq;
            default_options(rq);
            rq.n = n;
            const std::vector<dsa_mesh_attr_input> wide = form == 0 ? enc_widen(vertex.data(), n) : (form == 1 ? enc_widen(corners.data(), n) : listed);
            rq.meshes = wide.data();
            rq.level.multi_parallelogram = (scheme & 1) ? 4 : 0;
            if (scheme & 2) { rq.level.ex.base.texcoord_prediction = 5; rq.level.ex.normal_prediction = 6; }
            rq.level.ex.edgebreaker_method = valence ? 2 : 0;
            rq.level.traversal_method = traversal;
            char name[160];
            snprintf(name, sizeof(name), "form %d host_conn %d traversal %d scheme %d valence %d", form, host_conn, traversal, scheme, valence);
            g_case = name;
            // two chunks of the batch, so that a chunk starts in the middle of the request
            for (uint32_t base = 0; base < n; base += (n + 1) / 2) {
              const uint32_t cnt = std::min(n - base, (n + 1) / 2);
              EncChunk ck(rq, base, cnt, n);
              Log log;
              ck.region_log = &log;
              enc_begin_plans(ck, host_conn != 0, true);
              for (uint32_t i = 0; i < cnt; ++i) enc_plan_mesh(ck, i);
              enc_layout(ck);
              const int bad_here = bad >= base && bad < base + cnt ? (int)(bad - base) : -1;
              if (bad_here >= 0 && ck.E->messages[bad_here] != "face index out of range") { fprintf(stderr, "%s: the bad mesh says '%s'\n", name, ck.E->messages[bad_here].c_str()); return 1; }
              if (!check_layout(ck, log, bad_here)) return 1;
              bool multi = false, crease = false;
              for (uint32_t i = 0; i < cnt; ++i) for (const auto &a : ck.plans[i].atts) { multi = multi || (ck.good(i) && enc_multi_scheme(a)); crease = crease || (ck.good(i) && enc_multi_scheme(a) && a.prediction == 4); }
              if (ck.L.any_multi != multi || ck.L.any_crease != crease || ck.L.any_valence != (valence != 0)) { fprintf(stderr, "%s: the chunk's flags\n", name); return 1; }
              ++chunks; regions += (uint32_t)log.size();
            }
          }
  // ---- sequential streams: raw indices, compressed indices, point clouds; with the attribute list and without
  for (int form = 0; form < 3; form += 2)
    for (int mode = 0; mode < 3; ++mode) {
      EncRequest rq;
      default_options(rq);
      rq.n = n; rq.sequential = true;
      rq.seq.geometry = mode == 2 ? 0 : 1; rq.seq.compress_connectivity = mode == 1 ? 1 : 0;
      std::vector<dsa_mesh_attr_input> lst = listed;
      std::vector<dsa_mesh_input> vtx = vertex;
      for (uint32_t i = 0; i < n; ++i) {                       // one value per point: no ids, as many rows as points; a point cloud has no faces
        lst[i].mesh.normal_corners = lst[i].mesh.texcoord_corners = nullptr;
        nrm[i].assign((size_t)3 * batch[i].nv, 0.0f); uv[i].assign((size_t)2 * batch[i].nv, 0.25f);
        lst[i].mesh.mesh.normals = vtx[i].normals = nrm[i].data(); lst[i].mesh.mesh.texcoords = vtx[i].texcoords = uv[i].data();
        if (mode == 2) lst[i].mesh.mesh.num_faces = vtx[i].num_faces = 0;
      }
      const std::vector<dsa_mesh_attr_input> wide = form == 0 ? enc_widen(vtx.data(), n) : lst;
      rq.meshes = wide.data();
      char name[160];
      snprintf(name, sizeof(name), "sequential form %d mode %d", form, mode);
      g_case = name;
      EncChunk ck(rq, 0, n, n);
      Log log;
      ck.region_log = &log;
      for (uint32_t i = 0; i < n; ++i) enc_check_sequential_mesh(ck, i);
      enc_layout_sequential(ck);
      if (!check_layout(ck, log, mode == 2 ? -1 : (int)bad)) return 1;          // (a point cloud has no faces to be out of range)
      if (ck.L.idx.size() != (mode == 1 ? n - 1 : 0)) { fprintf(stderr, "%s: %zu index records\n", name, ck.L.idx.size()); return 1; }
      ++chunks; regions += (uint32_t)log.size();
    }
  // ---- widening changes nothing in the layout: without ids, forms 0 and 1 against form 2 without its extras, region for region
  // and record for record (Edgebreaker on both connectivity paths and sequential; a chunk that starts inside the request)
  if (!any_ids) {
    std::vector<dsa_mesh_attr_input> bare = listed;
    for (dsa_mesh_attr_input &am : bare) { am.attributes = nullptr; am.num_attributes = 0; }
    for (int path = 0; path < 3; ++path) {                     // 0 / 1: Edgebreaker, device / host connectivity; 2: sequential
      Log want_log;
      std::vector<dsa::EncStream> want;
      for (int form = 2; form >= 0; --form) {
        char name[96];
        snprintf(name, sizeof(name), "widened form %d against form 2, path %d", form, path);
        g_case = name;
        EncRequest rq;
        default_options(rq);
        rq.n = n; rq.sequential = path == 2;
        const std::vector<dsa_mesh_attr_input> wide = form == 0 ? enc_widen(vertex.data(), n) : (form == 1 ? enc_widen(corners.data(), n) : bare);
        rq.meshes = wide.data();
        EncChunk ck(rq, 1, n - 1, n);
        Log log;
        ck.region_log = &log;
        if (path == 2) { for (uint32_t i = 0; i < n - 1; ++i) enc_check_sequential_mesh(ck, i); enc_layout_sequential(ck); }
        else { enc_begin_plans(ck, path == 1, true); for (uint32_t i = 0; i < n - 1; ++i) enc_plan_mesh(ck, i); enc_layout(ck); }
        if (form == 2) { want_log = log; want = ck.L.streams; continue; }
        if (log != want_log) { fprintf(stderr, "%s: the regions differ\n", name); return 1; }
        if (ck.L.streams.size() != want.size() || (!want.empty() && memcmp(ck.L.streams.data(), want.data(), sizeof(dsa::EncStream) * want.size()) != 0)) { fprintf(stderr, "%s: the stream records differ\n", name); return 1; }
      }
    }
  }
  // ---- a generic attribute of 5 components, on one mesh: dsa_encode_batch's request (EncRequest::drop_generic_outside_1_4) plans
  // the mesh as if `generic` were NULL, every other Edgebreaker request and every sequential one refuses it
  {
    const char *refusal = "generic attribute needs 1 - 4 components";
    dsa_mesh_input with5 = vertex[0], without = vertex[0];
    with5.generic = generic[0].data(); with5.generic_components = 5;
    without.generic = nullptr; without.generic_components = 0;
    dsa_mesh_corner_input with5c = corners[0];
    with5c.mesh = with5;
    dsa_mesh_attr_input with5l = listed[0];
    with5l.mesh.mesh = with5;
    size_t atts_without = 0;
    for (int c = 0; c < 5; ++c) {                              // 0: without the attribute; 1: dsa_encode_batch's request; 2 - 4: forms 0 - 2 of every other entry
      char name[96];
      snprintf(name, sizeof(name), "generic_components 5, case %d", c);
      g_case = name;
      for (int path = 0; path < 3; ++path) {                   // as above
        EncRequest rq;
        default_options(rq);
        rq.n = 1; rq.sequential = path == 2;
        rq.drop_generic_outside_1_4 = c == 1;
        const std::vector<dsa_mesh_attr_input> wide = c == 0 ? enc_widen(&without, 1) : (c <= 2 ? enc_widen(&with5, 1) : (c == 3 ? enc_widen(&with5c, 1) : std::vector<dsa_mesh_attr_input>(1, with5l)));
        rq.meshes = wide.data();
        EncChunk ck(rq, 0, 1, 1);
        Log log;
        ck.region_log = &log;
        if (path == 2) { enc_check_sequential_mesh(ck, 0); enc_layout_sequential(ck); }
        else { enc_begin_plans(ck, path == 1, true); enc_plan_mesh(ck, 0); enc_layout(ck); }
        if (c == 0 || (c == 1 && path != 2)) {
          if (!check_layout(ck, log, -1)) return 1;
          if (c == 0 && path == 0) atts_without = ck.plans[0].atts.size();
          if (path != 2 && ck.plans[0].atts.size() != atts_without) { fprintf(stderr, "%s: %zu attributes, %zu without the generic one\n", name, ck.plans[0].atts.size(), atts_without); return 1; }
        } else if (ck.good(0) || ck.E->status[0] != DSA_ERR_INVALID_ARGUMENT || ck.E->messages[0] != refusal) {
          fprintf(stderr, "%s path %d: status %d '%s'\n", name, path, (int)ck.E->status[0], ck.E->messages[0].c_str());
          return 1;
        }
      }
    }
  }
  printf("enclayout: %u meshes, %u chunks laid out, %u regions checked\n", n, chunks, regions);
  return 0;
}
