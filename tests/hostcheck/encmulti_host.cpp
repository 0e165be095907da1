// tests/hostcheck/encmulti_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The encoder's level kernels of the product (draco-sharp_amd/csrc/dsa_encode_multi.h: k_enc_pd_walk one lane per mesh behind the
// connectivity kernels of dsa_encode_conn.h, k_enc_pd_operands, k_enc_multi one thread per entry, k_enc_crease) compiled for the
// host with AddressSanitizer + UBSan and run thread by thread, against the host coder (dsa_encode_host.h:
// prediction_degree_sequence, write_attribute_values with prediction 2 / 4) on the same faces and values:
//   - d2c / v2d of the prediction-degree order, entry -> vertex and operand entries;
//   - for three components of integers per vertex, methods 2 and 4, in depth-first and in prediction-degree order: the symbols and
//     the four crease lists, held against the host coder through the bytes it writes for them (scheme, tables, coded symbols, the
//     four lists rABS-coded, the wrap bounds: a symbol or a flag that differs changes them);
//   - the same for an attribute given per corner with seams, on its own table (AttrConn) and order;
// and not one access outside a mesh's arrays (the arena's gaps are poisoned).  Nothing here is linked into the product.
//
//   encmulti_host <meshes.bin>    file: u32 count, then per mesh u32 nv, u32 nf, u32 faces[3 nf], u32 rows (0: no ids), u32 ids[3 nf]
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
#include "../../draco-sharp_amd/csrc/dsa_encode_schemes.h"
#include "../../draco-sharp_amd/csrc/dsa_encode_multi.h"

struct MultiStream {               // what k_enc_multi / k_enc_crease read and write of an EncStream
  uint64_t d, syms, bl, hist_raw, t_c2a, t_opp, t_d2c, t_v2d, ori, flags;
  uint32_t nv, nc, kind, prediction, hist_cap, t_nc3, overflow, max_value;
  int32_t wrap_mn, wrap_mx;
  unsigned long long total_bl;
  uint32_t hist_tag[33];
  uint32_t cr_at[4], cr_n[4];
};

struct In { uint32_t nv, nf, rows; std::vector<uint32_t> faces, ids; };
static const int NC = 3;
// values that a parallelogram predicts well but not exactly, some of them far off (creases pay there), a few negative
static int32_t value_of(uint32_t row, int c, uint32_t salt) {
  const uint32_t h = (row * 2654435761u + (uint32_t)c * 40503u + salt * 97u) >> 7;
  return (int32_t)(row * (3 + c)) % 211 + (int32_t)(h % 7) - 3 + ((h >> 8) % 29 == 0 ? 150 : 0) - (c == 2 ? 40 : 0);
}

// One stream's regions in an arena of its own, gaps poisoned; runs k_enc_multi (+ k_enc_crease) and holds the result against
// write_attribute_values of the host coder.  Returns "" or what differs.
template <class CT>
static std::string check_stream(const CT &ct, const synth::CornerTable &pos_ct, const synth::Sequence &seq, const uint32_t *ids, uint32_t rows,
                                const std::vector<uint32_t> &c2a, const std::vector<uint32_t> &opp, int method, uint32_t salt, uint32_t *creases_seen) {
  const uint32_t entries = (uint32_t)seq.data_to_corner.size(), nc3 = (uint32_t)c2a.size();
  synth::PortableAttr a;
  a.att_type = 4; a.nc = a.nc_out = NC; a.seq_type = 1; a.data_type = 5; a.prediction = method; a.corner_value = ids;
  a.vals.resize((size_t)rows * NC);
  for (uint32_t r = 0; r < rows; ++r) for (int c = 0; c < NC; ++c) a.vals[(size_t)r * NC + c] = value_of(r, c, salt);
  synth::Options opt;
  synth::ByteWriter want;
  synth::write_attribute_values(want, a, ct, pos_ct, seq, opt);
  // ---- the device source
  uint64_t cur = 0;
  std::vector<std::pair<uint64_t, uint64_t>> regions;
  auto take = [&](uint64_t bytes) { cur = (cur + 255) & ~255ull; cur += 64; const uint64_t at = cur; regions.push_back({at, bytes}); cur += bytes + 64; return at; };
  MultiStream S;
  memset(&S, 0, sizeof(S));
  S.nv = entries; S.nc = NC; S.kind = 2; S.prediction = (uint32_t)method; S.t_nc3 = nc3;
  S.d = take(4ull * entries * NC); S.syms = take(4ull * entries * NC); S.bl = take(entries);
  S.hist_cap = 1024; S.hist_raw = take(4ull * S.hist_cap);
  S.t_c2a = take(4ull * nc3); S.t_opp = take(4ull * nc3); S.t_d2c = take(4ull * entries); S.t_v2d = take(4ull * seq.vertex_to_data.size());
  if (method == 4) { S.ori = take(entries); S.flags = take(4ull * dsa::em_crease_words(entries, S.cr_at)); }
  std::vector<uint8_t> store(cur + 256, 0);
  uint8_t *arena = store.data();
  int32_t *d = (int32_t *)(arena + S.d);
  int32_t mn = 0x7FFFFFFF, mx = (int32_t)0x80000000;
  for (uint32_t e = 0; e < entries; ++e) {
    const uint32_t corner = seq.data_to_corner[e], row = ids ? ids[corner] : pos_ct.vertex(corner);
    for (int c = 0; c < NC; ++c) { const int32_t x = a.vals[(size_t)row * NC + c]; d[(size_t)e * NC + c] = x; mn = x < mn ? x : mn; mx = x > mx ? x : mx; }
  }
  S.wrap_mn = mn; S.wrap_mx = mx;
  memcpy(arena + S.t_c2a, c2a.data(), 4ull * nc3); memcpy(arena + S.t_opp, opp.data(), 4ull * nc3);
  memcpy(arena + S.t_d2c, seq.data_to_corner.data(), 4ull * entries);
  memcpy(arena + S.t_v2d, seq.vertex_to_data.data(), 4ull * seq.vertex_to_data.size());
  ASAN_POISON_MEMORY_REGION(arena, store.size());
  for (auto &rg : regions) ASAN_UNPOISON_MEMORY_REGION(arena + rg.first, rg.second);
  launch(dsa::k_enc_multi<MultiStream>, 2, 1, 256, arena, &S, 1u);
  launch(dsa::k_enc_crease<MultiStream>, 1, 1, WAVE, arena, &S, 1u);
  ASAN_UNPOISON_MEMORY_REGION(arena, store.size());
  if (S.overflow) return "the device source gave the stream up";
  // ---- the bytes the host coder writes for the device's symbols and lists
  const uint32_t *sy = (const uint32_t *)(arena + S.syms);
  std::vector<uint32_t> symbols(sy, sy + (size_t)entries * NC);
  synth::ByteWriter got;
  got.i8((int8_t)method); got.i8(1); got.u8(1);
  synth::encode_symbols(got, symbols, NC, opt.force_scheme, opt.compression_level);
  if (method == 4)
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t *words = (const uint32_t *)(arena + S.flags) + S.cr_at[j];
      std::vector<uint8_t> bits(S.cr_n[j]);
      for (uint32_t e = 0; e < S.cr_n[j]; ++e) { bits[e] = (uint8_t)((words[e >> 5] >> (e & 31u)) & 1u); creases_seen[j] += 1; }
      got.varint(bits.size());
      if (!bits.empty()) synth::write_rabs(got, bits);
    }
  got.i32(mn); got.i32(mx);
  // statistics as k_enc_corr leaves them: what symbol_stats of the host coder counts
  synth::SymbolStats st;
  synth::symbol_stats(symbols, NC, st);
  if (st.max_value != S.max_value || st.total_bl != S.total_bl) return "max_value / total_bl differ from symbol_stats";
  const uint32_t *hist = (const uint32_t *)(arena + S.hist_raw);
  for (size_t v = 0; v < st.raw_freq.size(); ++v) if (st.raw_freq[v] != hist[v]) return "histogram differs from symbol_stats";
  for (size_t b = 0; b < st.tag_freq.size() && b < 33; ++b) if (st.tag_freq[b] != S.hist_tag[b]) return "bit-length histogram differs from symbol_stats";
  if (got.d != want.d) return "symbols or crease lists differ from the host coder's";
  return "";
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: encmulti_host <meshes.bin>\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  std::vector<In> meshes(count);
  for (auto &m : meshes) {
    if (fread(&m.nv, 4, 1, f) != 1 || fread(&m.nf, 4, 1, f) != 1) return 2;
    m.faces.resize((size_t)3 * m.nf);
    if (m.nf && fread(m.faces.data(), 4, m.faces.size(), f) != m.faces.size()) return 2;
    if (fread(&m.rows, 4, 1, f) != 1) return 2;
    if (m.rows) { m.ids.resize((size_t)3 * m.nf); if (fread(m.ids.data(), 4, m.ids.size(), f) != m.ids.size()) return 2; }
  }
  fclose(f);
  // ---- the connectivity arena, laid out like dsa_encode.h lays a chunk out, every gap poisoned; every fourth mesh without the
  // second order (no regions) in the same launches
  const uint32_t n = count;
  std::vector<dsa::EncConn> hc(n);
  uint64_t cur = 0;
  std::vector<std::pair<uint64_t, uint64_t>> regions;
  auto take = [&](uint64_t bytes) { cur = (cur + 255) & ~255ull; cur += 64; const uint64_t at = cur; regions.push_back({at, bytes}); cur += bytes + 64; return at; };
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
    C.vstream = DSA_INVALID;
    if (i % 4 != 3) {
      C.pd_d2c = take(4 * V); C.pd_v2d = take(4 * V); C.pd_e2v = take(4 * V); C.pd_ops = take(12 * V);
      C.pd_next = take(12 * F); C.pd_degree = take(4 * V); C.pd_fvis = take(F);
    }
    bool in_range = true;
    for (uint32_t x : meshes[i].faces) in_range = in_range && x < V;
    if (!in_range || F == 0 || V < 3) C.status = dsa::ENC_ISOLATED;
  }
  std::vector<uint8_t> arena_store(cur + 256, 0);
  uint8_t *arena = arena_store.data();
  for (uint32_t i = 0; i < n; ++i) if (meshes[i].nf) memcpy(arena + hc[i].faces, meshes[i].faces.data(), 12ull * meshes[i].nf);
  ASAN_POISON_MEMORY_REGION(arena, arena_store.size());
  for (auto &rg : regions) ASAN_UNPOISON_MEMORY_REGION(arena + rg.first, rg.second);
  uint32_t maxf = 1;
  for (auto &m : meshes) maxf = std::max(maxf, m.nf);
  const uint32_t gx = std::max(1u, std::min(4u, (3u * maxf + 1023u) / 1024u));
  dsa::EncConn *conns = hc.data();
  launch(dsa::k_enc_table_clear, gx, n, 256, arena, conns, n);
  launch(dsa::k_enc_table_count, gx, n, 256, arena, conns, n);
  launch(dsa::k_enc_table_offsets, n, 1, WAVE, arena, conns, n);
  launch(dsa::k_enc_table_lists, gx, n, 256, arena, conns, n);
  launch(dsa::k_enc_table_opposites, gx, n, 256, arena, conns, n);
  launch(dsa::k_enc_table_corners, gx, n, 256, arena, conns, n);
  const uint32_t lanes = 5;                    // meshes to a wave
  launch(dsa::k_enc_connectivity, (n + lanes - 1) / lanes, 1, WAVE, arena, conns, n, lanes);
  launch(dsa::k_enc_pd_walk, (n + lanes - 1) / lanes, 1, WAVE, arena, conns, n, lanes);
  launch(dsa::k_enc_operands, gx, n, 256, arena, conns, n);
  launch(dsa::k_enc_pd_operands, gx, n, 256, arena, conns, n);
  // ---- against the host coder
  uint32_t ordered = 0, plain = 0, refused = 0, split_meshes = 0, streams = 0, seamed = 0, creases[4] = {0, 0, 0, 0};
  for (uint32_t i = 0; i < n; ++i) {
    const In &m = meshes[i];
    const dsa::EncConn &C = hc[i];
    std::vector<float> pos((size_t)3 * std::max(m.nv, 1u), 0.0f);
    synth::MeshIn in;
    in.pos = pos.data(); in.nv = m.nv; in.faces = m.faces.data(); in.nf = m.nf; in.normals = nullptr; in.uvs = nullptr; in.generic = nullptr;
    synth::MeshPlan pl;
    synth::Options opt;
    opt.traversal_method = 1;
    bool host_ok = true;
    try {
      synth::check(m.nv >= 3 && m.nf >= 1, "mesh needs positions and faces");
      for (uint32_t x : m.faces) synth::check(x < m.nv, "face index out of range");
      synth::plan_mesh(in, opt, pl);
    } catch (const std::exception &) { host_ok = false; }
    const bool dev_ok = C.status == dsa::ENC_OK;
    if (host_ok != dev_ok) { fprintf(stderr, "mesh %u: host coder %s, device source status %u\n", i, host_ok ? "codes" : "refuses", C.status); return 1; }
    if (!host_ok) { ++refused; continue; }
    if (pl.eb.num_split_symbols) ++split_meshes;
    if (C.pd_d2c) {
      ++ordered;
      const uint32_t *d2c = (const uint32_t *)(arena + C.pd_d2c), *e2v = (const uint32_t *)(arena + C.pd_e2v);
      const int32_t *v2d = (const int32_t *)(arena + C.pd_v2d), *ops = (const int32_t *)(arena + C.pd_ops);
      std::vector<uint32_t> want_e2v;
      std::vector<int32_t> want_ops;
      const uint32_t V = m.nv;
      want_e2v.resize(V); want_ops.assign((size_t)3 * V, -1);
      for (uint32_t p = 0; p < V; ++p) {
        if (d2c[p] != pl.seq_pd.data_to_corner[p]) { fprintf(stderr, "mesh %u: entry %u of the prediction-degree order is corner %u, host %u\n", i, p, d2c[p], pl.seq_pd.data_to_corner[p]); return 1; }
        if (v2d[p] != pl.seq_pd.vertex_to_data[p]) { fprintf(stderr, "mesh %u: vertex %u is entry %d, host %d\n", i, p, v2d[p], pl.seq_pd.vertex_to_data[p]); return 1; }
        const uint32_t ci = pl.seq_pd.data_to_corner[p];
        want_e2v[p] = pl.ct.vertex(ci);
        const uint32_t oci = pl.ct.opposite(ci);
        if (p == 0 || oci == synth::kInvalid) continue;
        const int32_t vo = pl.seq_pd.vertex_to_data[pl.ct.vertex(oci)], vn = pl.seq_pd.vertex_to_data[pl.ct.vertex(synth::CornerTable::next(oci))], vp = pl.seq_pd.vertex_to_data[pl.ct.vertex(synth::CornerTable::prev(oci))];
        if (vo < (int32_t)p && vn < (int32_t)p && vp < (int32_t)p) { want_ops[3 * p] = vn; want_ops[3 * p + 1] = vp; want_ops[3 * p + 2] = vo; }
      }
      if (memcmp(e2v, want_e2v.data(), 4ull * V) != 0 || memcmp(ops, want_ops.data(), 12ull * V) != 0) { fprintf(stderr, "mesh %u: entry maps of the prediction-degree order differ\n", i); return 1; }
    } else ++plain;
    // the prediction kernels on the position table, both orders, both methods
    for (int method : {2, 4})
      for (int order = 0; order < 2; ++order) {
        const std::string why = check_stream(pl.ct, pl.ct, order ? pl.seq_pd : pl.seq, nullptr, m.nv, pl.ct.c2v, pl.ct.opp, method, i + 13u * order, creases);
        if (!why.empty()) { fprintf(stderr, "mesh %u, method %d, %s order: %s\n", i, method, order ? "prediction-degree" : "depth-first", why.c_str()); return 1; }
        ++streams;
      }
    // ... and on the table of an attribute with seams, in its own depth-first order
    if (m.rows) {
      bool ids_ok = true;
      for (uint32_t x : m.ids) ids_ok = ids_ok && x < m.rows;
      if (!ids_ok) continue;
      synth::AttrConn conn;
      synth::Sequence seq_att;
      bool att_ok = true;
      try {
        conn.build(pl.ct, m.ids.data());
        if (!conn.no_interior_seams) {
          synth::dfs_sequence(conn, pl.eb.processed_corners, seq_att);
          synth::check(seq_att.data_to_corner.size() == conn.nv(), "attribute traversal did not reach every attribute vertex");
        }
      } catch (const std::exception &) { att_ok = false; }
      if (!att_ok || conn.no_interior_seams) continue;
      std::vector<uint32_t> opp2(pl.ct.nc());
      for (uint32_t c = 0; c < pl.ct.nc(); ++c) opp2[c] = conn.opposite(c);
      for (int method : {2, 4}) {
        const std::string why = check_stream(conn, pl.ct, seq_att, m.ids.data(), m.rows, conn.c2v, opp2, method, i, creases);
        if (!why.empty()) { fprintf(stderr, "mesh %u, method %d, seamed attribute: %s\n", i, method, why.c_str()); return 1; }
        ++streams; ++seamed;
      }
    }
  }
  printf("encmulti: %u meshes, %u orders alike (%u with topology splits), %u without, %u refused alike, %u streams alike (%u seamed), crease flags %u %u %u %u\n",
         n, ordered, split_meshes, plain, refused, streams, seamed, creases[0], creases[1], creases[2], creases[3]);
  return 0;
}
