// draco-sharp_amd/csrc/dsa_encode_host.h
// -----------------------------------------------------------------------------
// Host half of the encode direction (BASELINE.json configs[4]) and of the synthetic
// input generator: corner table, Edgebreaker connectivity encoder, DFS sequencing, the stream layout of a
// Draco v2.2 mesh, symbol-scheme selection and rANS table construction, plus a complete CPU attribute coder.
//   * draco-sharp_amd/synth (tests / bench inputs) uses all of it, CPU only;
//   * the product encoder (dsa_encode.hip) uses the connectivity + layout + table parts and runs
//     quantisation, prediction, symbol statistics and the rANS coding on the GPU; its output is byte-identical
//     to the CPU coder's, which is what tests/test_gpu_encode.py checks.
// Follows the rules of SURVEY.md Appendix D:
//   IO/Mesh/MeshEdgeBreakerEncoder.cs:38-124,176-303  (connectivity traversal)
//   IO/Mesh/MeshEdgeBreakerTraversalEncoder.cs:40-71  (symbol/start-face/seam sections)
//   IO/Entropy/SymbolEncoding.cs:8-193, RAnsSymbolEncoder.cs:15-184,
//   RAnsEncoder.cs:22-30, AnsEncoder.cs:19-64, BitCoders/RAnsBitEncoder.cs
//   IO/Attributes/SequentialIntegerAttributeEncoder.cs:55-128,
//   AttributeQuantizationTransform.cs:66-177, OctahedronToolBox.cs:28-119,
//   PredictionSchemes/*Encoder.cs, *EncodingTransform.cs
// (each with the defects listed there, E-1..E-8, corrected to the bitstream's semantics).
// -----------------------------------------------------------------------------
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "dsa_symbol_plan.h"

namespace synth {

static const uint32_t kInvalid = 0xFFFFFFFFu;

struct Fail : std::runtime_error { using std::runtime_error::runtime_error; };
static inline void check(bool ok, const char *msg) { if (!ok) throw Fail(msg); }

// ------------------------------------------------------------------ writers
struct ByteWriter {
  std::vector<uint8_t> d;
  void u8(uint8_t v) { d.push_back(v); }
  void i8(int8_t v) { d.push_back((uint8_t)v); }
  void u16(uint16_t v) { u8(v & 0xFF); u8(v >> 8); }
  void u32(uint32_t v) { for (int i = 0; i < 4; ++i) u8((v >> (8 * i)) & 0xFF); }
  void i32(int32_t v) { u32((uint32_t)v); }
  void f32(float f) { uint32_t v; memcpy(&v, &f, 4); u32(v); }
  void varint(uint64_t v) { while (v >= 0x80) { u8((uint8_t)(v | 0x80)); v >>= 7; } u8((uint8_t)v); }
  void bytes(const std::vector<uint8_t> &b) { d.insert(d.end(), b.begin(), b.end()); }
};
struct BitWriter {   // LSB-first, EncoderBuffer.cs bit mode
  std::vector<uint8_t> d;
  uint64_t nbits = 0;
  void put(int count, uint32_t v) {       // the low `count` bits of v, least significant first; d always ends in the byte being filled
    if (count <= 0) return;
    uint64_t x = count >= 32 ? (uint64_t)v : (uint64_t)(v & ((1u << count) - 1u));
    const int off = (int)(nbits & 7);
    if (off) {
      d.back() |= (uint8_t)(x << off);
      const int took = 8 - off;
      if (count <= took) { nbits += (uint64_t)count; return; }
      x >>= took; count -= took; nbits += (uint64_t)took;
    }
    while (count > 0) { d.push_back((uint8_t)x); x >>= 8; const int t = count < 8 ? count : 8; nbits += (uint64_t)t; count -= t; }
  }
};

static inline int msb(uint32_t v) { int r = 0; while (v >>= 1) ++r; return r; }
static inline uint32_t zigzag(int32_t v) { return v >= 0 ? (uint32_t)v << 1 : (((uint32_t)(-(v + 1))) << 1) | 1; }

// ------------------------------------------------------------------ entropy
// rABS bit block: prob_zero u8, size varint, bytes (RAnsBitEncoder.cs:25-44,86-126)
static void write_rabs(ByteWriter &w, const std::vector<uint8_t> &bits) {
  uint64_t zeros = 0;
  for (uint8_t b : bits) zeros += b ? 0 : 1;
  uint64_t total = bits.size() ? bits.size() : 1;
  uint32_t raw = (uint32_t)(((double)zeros / (double)total) * 256.0 + 0.5);
  uint8_t p0 = 255;
  if (raw < 255) p0 = (uint8_t)raw;
  if (p0 == 0) p0 = 1;
  std::vector<uint8_t> buf;
  buf.reserve(bits.size() / 8 + 16);
  uint32_t state = 4096;
  const uint32_t p = 256u - p0;            // 1 .. 255, like p0
  // state / ls by a multiply-high with ceil(2^32 / ls): the quotient or one more (state < 2^32), one correction
  const uint32_t ls2[2] = {p0, p}, lim2[2] = {16u * 256u * p0, 16u * 256u * p}, add2[2] = {p, 0u};
  const uint64_t magic2[2] = {0xFFFFFFFFull / p0 + 1ull, 0xFFFFFFFFull / p + 1ull};
  for (size_t k = bits.size(); k-- > 0;) {
    const int val = bits[k] != 0;
    const uint32_t ls = ls2[val];
    if (state >= lim2[val]) { buf.push_back(state & 0xFF); state >>= 8; }
    uint32_t quot = (uint32_t)(((uint64_t)state * magic2[val]) >> 32);
    uint32_t rem = state - quot * ls;
    if ((int32_t)rem < 0) { --quot; rem += ls; }
    state = quot * 256 + rem + add2[val];
  }
  uint32_t s = state - 4096;   // AnsEncoder.cs:34-64
  if (s < (1u << 6)) buf.push_back((uint8_t)s);
  else if (s < (1u << 14)) { uint32_t v = 0x4000 + s; buf.push_back(v & 0xFF); buf.push_back(v >> 8); }
  else if (s < (1u << 22)) { uint32_t v = 0x800000 + s; buf.push_back(v & 0xFF); buf.push_back((v >> 8) & 0xFF); buf.push_back(v >> 16); }
  else check(false, "rABS state too large");
  w.u8(p0);
  w.varint(buf.size());
  w.bytes(buf);
}

struct RansEncoder {
  int precision_bits = 12;
  uint32_t precision = 4096, l_base = 16384;
  std::vector<uint32_t> prob, cum;
  uint32_t num_symbols = 0;
  // RAnsSymbolEncoder.cs:15-123 (normalisation) + :125-164 (table bytes, E-3 corrected)
  void create(ByteWriter &w, int max_bit_length, const std::vector<uint64_t> &freq) {
    prob.assign(freq.size() ? freq.size() : 1, 0);
    cum.assign(prob.size(), 0);
    std::vector<uint32_t> order(prob.size()), tmp(prob.size());
    const int rc = dsa::plan::rans_tables(max_bit_length, freq.data(), freq.size(), prob.data(), cum.data(), order.data(), tmp.data(), &precision_bits, &num_symbols);
    check(rc == dsa::plan::PLAN_OK, dsa::plan::plan_message(rc));
    prob.resize(num_symbols); cum.resize(num_symbols);
    precision = 1u << precision_bits;
    l_base = precision * 4;
    write_table(w);
  }
  // RAnsSymbolEncoder.cs:125-164 (E-3 corrected): the probability table as the stream carries it
  void write_table(ByteWriter &w) const {
    w.varint(num_symbols);
    for (uint32_t i = 0; i < num_symbols; ++i) {
      uint32_t pr = prob[i];
      int extra = 0;
      if (pr >= (1u << 6)) { extra++; if (pr >= (1u << 14)) { extra++; check(pr < (1u << 22), "probability too large"); } }
      if (pr == 0) {
        uint32_t offset = 0;
        for (; offset < 63; ++offset) if (prob[i + offset + 1] > 0) break;
        w.u8((uint8_t)((offset << 2) | 3));
        i += offset;
      } else {
        w.u8((uint8_t)((pr << 2) | (uint32_t)extra));
        for (int b = 0; b < extra; ++b) w.u8((uint8_t)(pr >> (8 * (b + 1) - 2)));
      }
    }
  }
  // symbols fed last->first (SymbolEncoding.cs:177-183); RAnsEncoder.cs:22-30; AnsEncoder.cs:34-64
  void encode(ByteWriter &w, const uint32_t *syms, size_t n, size_t stride = 1) {
    std::vector<uint8_t> buf;
    buf.reserve(n);
    uint32_t state = l_base;
    for (size_t k = n; k-- > 0;) {
      uint32_t s = syms[k * stride];
      uint32_t p = prob[s];
      uint64_t lim = (uint64_t)(l_base / precision) * 256u * p;
      while ((uint64_t)state >= lim) { buf.push_back(state & 0xFF); state >>= 8; }
      state = (state / p) * precision + state % p + cum[s];
    }
    uint32_t s = state - l_base;
    if (s < (1u << 6)) buf.push_back((uint8_t)s);
    else if (s < (1u << 14)) { uint32_t v = 0x4000 + s; buf.push_back(v & 0xFF); buf.push_back(v >> 8); }
    else if (s < (1u << 22)) { uint32_t v = 0x800000 + s; buf.push_back(v & 0xFF); buf.push_back((v >> 8) & 0xFF); buf.push_back(v >> 16); }
    else if (s < (1u << 30)) { uint32_t v = 0xC0000000u + s; for (int i = 0; i < 4; ++i) buf.push_back((v >> (8 * i)) & 0xFF); }
    else check(false, "rANS state too large");
    w.varint(buf.size());
    w.bytes(buf);
  }
};

// Statistics of one symbol stream: everything the scheme selection and the table construction need.  The CPU coder
// fills it from the symbol list; the GPU encoder fills it with histograms computed on the device.
struct SymbolStats {
  size_t n = 0;                       // symbols (entries * nc)
  int nc = 1;
  uint32_t max_value = 0;
  uint64_t total_bl = 0;              // sum of the per-entry bit lengths
  std::vector<uint64_t> tag_freq;     // [33] histogram of per-entry bit lengths
  std::vector<uint64_t> raw_freq;     // [max_value + 1] histogram of symbol values; empty where the raw scheme is out of the question
};
// force_scheme != 1 and symbols above 18 bits (32-bit integer attributes): the scheme is the tagged one whatever the histogram of
// values says (choose_scheme), so it is not built -- it would have up to 2^32 entries.
static void symbol_stats(const std::vector<uint32_t> &v, int nc, SymbolStats &st, std::vector<uint32_t> *bit_lengths_out = nullptr, int force_scheme = 1) {
  st.n = v.size(); st.nc = nc; st.max_value = 0; st.total_bl = 0;
  st.tag_freq.assign(33, 0);
  std::vector<uint32_t> bl;
  bl.reserve(v.size() / nc);
  for (size_t i = 0; i < v.size(); i += nc) {
    uint32_t mc = v[i];
    for (int j = 1; j < nc; ++j) mc = std::max(mc, v[i + j]);
    const uint32_t b = (uint32_t)(mc > 0 ? msb(mc) : 0) + 1;
    st.max_value = std::max(st.max_value, mc);
    bl.push_back(b);
    st.total_bl += b;
    ++st.tag_freq[b];
  }
  st.raw_freq.clear();
  if (force_scheme == 1 || st.max_value < (1u << 18)) {
    st.raw_freq.assign((size_t)st.max_value + 1, 0);
    for (uint32_t x : v) ++st.raw_freq[x];
  }
  if (bit_lengths_out) bit_lengths_out->swap(bl);
}
// SymbolEncoding.cs:8-40 (E-2 corrected): scheme choice, then the coder's tables.  `head` receives the bytes that
// precede the rANS payload: scheme byte, (raw: unique-symbols bit length), probability table.
struct SymbolPlan {
  int method = 1;                     // 0 tagged, 1 raw
  RansEncoder coder;                  // tagged: over bit lengths; raw: over symbol values
  ByteWriter head;
};
static void plan_symbols(const SymbolStats &st, int force_scheme, int compression_level, SymbolPlan &pl) {
  int usbl = 0;
  if (st.raw_freq.empty()) {          // symbols above 18 bits, raw scheme not forced: tagged (what choose_scheme answers for them)
    pl.method = 0;
    pl.head.u8(0);
    pl.coder.create(pl.head, 5, st.tag_freq);
    return;
  }
  const int rc = dsa::plan::choose_scheme(st.tag_freq.data(), st.raw_freq.data(), st.max_value, (uint64_t)st.n, (uint32_t)st.nc, st.total_bl,
                                          force_scheme, compression_level, &pl.method, &usbl);
  check(rc == dsa::plan::PLAN_OK, dsa::plan::plan_message(rc));
  pl.head.u8((uint8_t)pl.method);
  if (pl.method == 0) {
    pl.coder.create(pl.head, 5, st.tag_freq);
  } else {
    pl.head.u8((uint8_t)usbl);
    pl.coder.create(pl.head, usbl, st.raw_freq);
  }
}

// SymbolEncoding.cs:92-137 tagged, :139-193 raw -- the CPU coder
static void encode_symbols(ByteWriter &w, const std::vector<uint32_t> &v, int nc, int force_scheme, int compression_level) {
  if (v.empty()) return;
  SymbolStats st;
  std::vector<uint32_t> bit_lengths;
  symbol_stats(v, nc, st, &bit_lengths, force_scheme);
  SymbolPlan pl;
  plan_symbols(st, force_scheme, compression_level, pl);
  w.bytes(pl.head.d);
  if (pl.method == 0) {
    pl.coder.encode(w, bit_lengths.data(), bit_lengths.size());
    BitWriter bw;
    for (size_t e = 0; e < bit_lengths.size(); ++e)
      for (int c = 0; c < nc; ++c) bw.put((int)bit_lengths[e], v[e * nc + c]);
    w.bytes(bw.d);
  } else {
    pl.coder.encode(w, v.data(), v.size());
  }
}

// -------------------------------------------------------------- corner table
struct CornerTable {
  std::vector<uint32_t> opp, c2v, vcorner;
  uint32_t nf() const { return (uint32_t)(c2v.size() / 3); }
  uint32_t nc() const { return (uint32_t)c2v.size(); }
  uint32_t nv() const { return (uint32_t)vcorner.size(); }
  static uint32_t next(uint32_t c) { return c == kInvalid ? c : ((c + 1) % 3 ? c + 1 : c - 2); }
  static uint32_t prev(uint32_t c) { return c == kInvalid ? c : (c % 3 ? c - 1 : c + 2); }
  uint32_t opposite(uint32_t c) const { return c == kInvalid ? c : opp[c]; }
  uint32_t vertex(uint32_t c) const { return c == kInvalid ? kInvalid : c2v[c]; }
  uint32_t swing_right(uint32_t c) const { return prev(opposite(prev(c))); }
  uint32_t swing_left(uint32_t c) const { return next(opposite(next(c))); }
  uint32_t right_corner(uint32_t c) const { return opposite(next(c)); }
  uint32_t left_corner(uint32_t c) const { return opposite(prev(c)); }
  bool on_boundary(uint32_t v) const { return swing_left(vcorner[v]) == kInvalid; }

  void build(const uint32_t *faces, uint32_t num_faces, uint32_t num_vertices) {
    c2v.assign(faces, faces + (size_t)num_faces * 3);
    opp.assign((size_t)num_faces * 3, kInvalid);
    vcorner.assign(num_vertices, kInvalid);
    // half-edge matching: corner c is opposite to edge (next(c) -> prev(c))
    std::vector<std::pair<uint64_t, uint32_t>> edges;
    edges.reserve(c2v.size());
    for (uint32_t c = 0; c < nc(); ++c) {
      uint64_t a = c2v[next(c)], b = c2v[prev(c)];
      check(a != b, "degenerate face in input mesh");
      edges.push_back({(a << 32) | b, c});
    }
    std::sort(edges.begin(), edges.end());
    for (size_t i = 1; i < edges.size(); ++i) check(edges[i].first != edges[i - 1].first, "non-manifold edge (duplicate half-edge)");
    for (auto &e : edges) {
      uint64_t a = e.first >> 32, b = e.first & 0xFFFFFFFFu;
      uint64_t rev = (b << 32) | a;
      auto it = std::lower_bound(edges.begin(), edges.end(), std::make_pair(rev, (uint32_t)0));
      if (it != edges.end() && it->first == rev) opp[e.second] = it->second;
    }
    for (uint32_t c = 0; c < nc(); ++c) if (vcorner[c2v[c]] == kInvalid) vcorner[c2v[c]] = c;
    // left-most corner for boundary vertices (CornerTable.cs UpdateVertexToCornerMap)
    for (uint32_t v = 0; v < num_vertices; ++v) {
      uint32_t first = vcorner[v];
      if (first == kInvalid) continue;
      uint32_t act = swing_left(first), c = first;
      size_t guard = 0;
      while (act != kInvalid && act != first) { c = act; act = swing_left(act); check(++guard < c2v.size(), "vertex ring does not close"); }
      if (act != first) vcorner[v] = c;
    }
    // manifold vertex check: every corner of v must be reachable from its left-most corner
    std::vector<uint32_t> count(num_vertices, 0), reach(num_vertices, 0);
    for (uint32_t c = 0; c < nc(); ++c) ++count[c2v[c]];
    for (uint32_t v = 0; v < num_vertices; ++v) {
      uint32_t s = vcorner[v];
      if (s == kInvalid) continue;
      uint32_t c = s;
      do { ++reach[v]; c = swing_right(c); } while (c != kInvalid && c != s && reach[v] <= count[v]);
      check(reach[v] == count[v], "non-manifold vertex in input mesh");
    }
  }

  // ---- repair mode: the reference's corner table (CornerTable.cs:28-43) in place of the checks above.
  // What the three passes leave, over the caller's faces and vertex ids: c2v' (a fan behind the first of its vertex has a new
  // vertex V, V + 1, ...), the opposites, the parent of every new vertex, and the counts the stream's header needs.
  struct Repaired {
    std::vector<uint32_t> c2v, opp, parent;      // u32[3F], u32[3F], u32[V' - V]
    uint32_t num_vertices = 0, isolated = 0, degenerate = 0, breaks = 0;      // V'; unused vertices among the caller's V; faces with a repeated index; edges cut
  };
  // row[v]: the caller's value row of vertex v of this table (repair mode only; empty: the vertex is its own row)
  std::vector<uint32_t> row;
  bool needed_repair = false;      // build_repaired: the mesh is not one build() takes
  std::vector<uint32_t> cmap;      // from_repaired: source corner -> coded corner, kInvalid on a degenerate face (u32[3F])
  uint32_t row_of(uint32_t v) const { return row.empty() ? v : row[v]; }

  static void repair(const uint32_t *faces, uint32_t num_faces, uint32_t num_vertices, Repaired &r) {
    const uint32_t ncor = num_faces * 3;
    r.c2v.assign(faces, faces + (size_t)ncor);
    r.opp.assign(ncor, kInvalid);
    r.parent.clear();
    r.isolated = r.degenerate = r.breaks = 0;
    std::vector<uint32_t> &c2v = r.c2v, &opp = r.opp;
    auto degenerate = [&](uint32_t f) { return c2v[3 * f] == c2v[3 * f + 1] || c2v[3 * f] == c2v[3 * f + 2] || c2v[3 * f + 1] == c2v[3 * f + 2]; };
    std::vector<uint8_t> degen(num_faces, 0);
    for (uint32_t f = 0; f < num_faces; ++f) if (degenerate(f)) { degen[f] = 1; ++r.degenerate; }
    // ComputeOppositeCorners (:298-394), with the scan over the whole pending list of the sink vertex: corners in index order;
    // corner c faces source -> sink and takes the earliest pending sink -> source whose face has another tip; else it waits at
    // its source behind the entries already there.  (Degenerate faces were marked on the caller's indices, as :332-341 sees them.)
    {
      std::vector<uint32_t> off(num_vertices + 1, 0), cnt(num_vertices, 0);
      for (uint32_t c = 0; c < ncor; ++c) ++off[c2v[c] + 1];
      for (uint32_t v = 0; v < num_vertices; ++v) off[v + 1] += off[v];
      std::vector<uint32_t> p_sink(ncor), p_corner(ncor);
      for (uint32_t c = 0; c < ncor; ++c) {
        if (degen[c / 3]) continue;
        const uint32_t tip = c2v[c], source = c2v[next(c)], sink = c2v[prev(c)];
        uint32_t found = kInvalid;
        const uint32_t at = off[sink];
        for (uint32_t i = 0; i < cnt[sink]; ++i) {
          if (p_sink[at + i] != source || c2v[p_corner[at + i]] == tip) continue;
          found = p_corner[at + i];
          for (uint32_t j = i + 1; j < cnt[sink]; ++j) { p_sink[at + j - 1] = p_sink[at + j]; p_corner[at + j - 1] = p_corner[at + j]; }
          --cnt[sink];
          break;
        }
        if (found == kInvalid) { const uint32_t k = off[source] + cnt[source]++; p_sink[k] = sink; p_corner[k] = c; }
        else { opp[c] = found; opp[found] = c; }
      }
    }
    auto swing_l = [&](uint32_t c) { const uint32_t o = opp[next(c)]; return o == kInvalid ? kInvalid : next(o); };
    auto swing_r = [&](uint32_t c) { const uint32_t o = opp[prev(c)]; return o == kInvalid ? kInvalid : prev(o); };
    // BreakNonManifoldEdges (:396-469): around every fan, two edges that reach the same sink vertex and are not each other's
    // opposite are cut on both sides; sweeps until one changes nothing, the visited marks kept from sweep to sweep.  (The walk
    // ends at the fan's open end, as the loop it was ported from does; :466 tests the first corner, which never is invalid.)
    {
      std::vector<uint8_t> visited(ncor, 0);
      std::vector<std::pair<uint32_t, uint32_t>> sinks;
      bool updated;
      do {
        updated = false;
        for (uint32_t c = 0; c < ncor; ++c) {
          if (visited[c] || degen[c / 3]) continue;
          sinks.clear();
          uint32_t first = c, cur = c, nx = swing_l(cur);
          while (nx != first && nx != kInvalid && !visited[nx]) { cur = nx; nx = swing_l(cur); }
          first = cur;
          do {
            visited[cur] = 1;
            const uint32_t sink_c = next(cur), sink_v = c2v[sink_c], edge_c = prev(cur);
            bool cut = false;
            for (const auto &s : sinks) {
              if (s.first != sink_v) continue;
              const uint32_t other = s.second, o_edge = opp[edge_c];
              if (o_edge == other) continue;
              const uint32_t o_other = opp[other];
              if (o_edge != kInvalid) opp[o_edge] = kInvalid;
              if (o_other != kInvalid) opp[o_other] = kInvalid;
              opp[edge_c] = kInvalid; opp[other] = kInvalid;
              cut = true;
              break;
            }
            if (cut) { updated = true; ++r.breaks; break; }
            sinks.push_back({c2v[prev(cur)], sink_c});
            cur = swing_r(cur);
          } while (cur != first && cur != kInvalid);
        }
      } while (updated);
    }
    // ComputeVertexCorners (:471-547): faces in index order; the first fan met keeps the vertex, every later one gets a new
    // vertex with a parent; a vertex no fan reached is isolated.
    {
      std::vector<uint8_t> vvis(num_vertices, 0), cvis(ncor, 0);
      uint32_t nv = num_vertices;
      for (uint32_t f = 0; f < num_faces; ++f) {
        if (degen[f]) continue;
        for (uint32_t k = 0; k < 3; ++k) {
          const uint32_t c = 3 * f + k;
          if (cvis[c]) continue;
          uint32_t v = c2v[c];
          bool fresh = false;
          if (vvis[v]) { r.parent.push_back(v); v = nv++; fresh = true; }
          else vvis[v] = 1;
          uint32_t act = c;
          while (act != kInvalid) {
            cvis[act] = 1;
            if (fresh) c2v[act] = v;
            act = swing_l(act);
            if (act == c) break;
          }
          if (act == kInvalid) {
            act = swing_r(c);
            while (act != kInvalid) { cvis[act] = 1; if (fresh) c2v[act] = v; act = swing_r(act); }
          }
        }
      }
      for (uint32_t v = 0; v < num_vertices; ++v) if (!vvis[v]) ++r.isolated;
      r.num_vertices = nv;
    }
  }

  // The repaired table as every walk takes it: degenerate faces and isolated vertices counted out (faces and vertices keep their
  // order, so start faces, holes and symbols are those of the reference's walk over the table with the gaps), opposites carried
  // over from the repair -- matching the renumbered faces again would join edges the repair cut.
  void build_repaired(const uint32_t *faces, uint32_t num_faces, uint32_t num_vertices) {
    Repaired r;
    repair(faces, num_faces, num_vertices, r);
    from_repaired(r, faces, num_faces, num_vertices);
  }
  // (the device encoder's repair kernels give `r`: dsa_encode_repair.h)
  void from_repaired(const Repaired &r, const uint32_t *faces, uint32_t num_faces, uint32_t num_vertices) {
    check(r.degenerate < num_faces, "all triangles are degenerate");
    needed_repair = r.degenerate != 0 || r.isolated != 0 || r.breaks != 0 || r.num_vertices != num_vertices;
    std::vector<uint32_t> vmap(r.num_vertices, kInvalid);
    cmap.assign((size_t)num_faces * 3, kInvalid);
    uint32_t nf2 = 0;
    for (uint32_t f = 0; f < num_faces; ++f) {
      if (faces[3 * f] == faces[3 * f + 1] || faces[3 * f] == faces[3 * f + 2] || faces[3 * f + 1] == faces[3 * f + 2]) continue;
      for (uint32_t k = 0; k < 3; ++k) { cmap[3 * f + k] = 3 * nf2 + k; vmap[r.c2v[3 * f + k]] = 0; }
      ++nf2;
    }
    row.clear();
    for (uint32_t v = 0; v < r.num_vertices; ++v) {
      if (vmap[v] == kInvalid) continue;
      vmap[v] = (uint32_t)row.size();
      row.push_back(v < num_vertices ? v : r.parent[v - num_vertices]);
    }
    c2v.assign((size_t)nf2 * 3, kInvalid);
    opp.assign((size_t)nf2 * 3, kInvalid);
    for (uint32_t c = 0; c < num_faces * 3; ++c) {
      if (cmap[c] == kInvalid) continue;
      c2v[cmap[c]] = vmap[r.c2v[c]];
      if (r.opp[c] != kInvalid) opp[cmap[c]] = cmap[r.opp[c]];
    }
    vcorner.assign(row.size(), kInvalid);
    for (uint32_t c = 0; c < nc(); ++c) if (vcorner[c2v[c]] == kInvalid) vcorner[c2v[c]] = c;
    for (uint32_t v = 0; v < nv(); ++v) {          // the left-most corner of a boundary vertex, as build() leaves it
      const uint32_t first = vcorner[v];
      uint32_t act = swing_left(first), c = first;
      size_t guard = 0;
      while (act != kInvalid && act != first) { c = act; act = swing_left(act); check(++guard < c2v.size(), "vertex ring does not close"); }
      if (act != first) vcorner[v] = c;
    }
  }
};

// The connectivity of one attribute with seams (MeshAttributeCornerTable.cs, encoder side): the position corner
// table with every seam edge cut.  Built from a value id per corner (:32-78: an interior edge is a seam when either of
// its end points carries different value ids on its two faces); vertices are the fans between cuts (:95-155).  Same
// interface as CornerTable, so that the traversal and the prediction schemes are templates over either.
struct AttrConn {
  const CornerTable *ct = nullptr;
  std::vector<uint8_t> edge_seam, vert_seam;
  std::vector<uint32_t> c2v, v2lm;
  bool no_interior_seams = true;
  uint32_t nf() const { return ct->nf(); }
  uint32_t nc() const { return ct->nc(); }
  uint32_t nv() const { return (uint32_t)v2lm.size(); }
  static uint32_t next(uint32_t c) { return CornerTable::next(c); }
  static uint32_t prev(uint32_t c) { return CornerTable::prev(c); }
  uint32_t opposite(uint32_t c) const { return (c == kInvalid || edge_seam[c]) ? kInvalid : ct->opposite(c); }
  uint32_t vertex(uint32_t c) const { return c == kInvalid ? kInvalid : c2v[c]; }
  uint32_t swing_right(uint32_t c) const { return prev(opposite(prev(c))); }
  uint32_t swing_left(uint32_t c) const { return next(opposite(next(c))); }
  uint32_t right_corner(uint32_t c) const { return opposite(next(c)); }
  uint32_t left_corner(uint32_t c) const { return opposite(prev(c)); }
  bool on_boundary(uint32_t v) const { return swing_left(v2lm[v]) == kInvalid; }
  void mark(uint32_t c) {
    edge_seam[c] = 1;
    vert_seam[ct->vertex(next(c))] = 1;
    vert_seam[ct->vertex(prev(c))] = 1;
  }
  void build(const CornerTable &t, const uint32_t *corner_value) {
    ct = &t;
    edge_seam.assign(t.nc(), 0);
    vert_seam.assign(t.nv(), 0);
    c2v.assign(t.nc(), kInvalid);
    no_interior_seams = true;
    for (uint32_t c = 0; c < t.nc(); ++c) {
      const uint32_t o = t.opposite(c);
      if (o == kInvalid) { mark(c); continue; }
      if (o < c) continue;
      // the edge's end points: next(c) lies on prev(o), prev(c) on next(o)
      if (corner_value[next(c)] != corner_value[prev(o)] || corner_value[prev(c)] != corner_value[next(o)]) {
        no_interior_seams = false;
        mark(c); mark(o);
      }
    }
    // :95-155 vertices: around every position vertex a new one behind every cut
    v2lm.clear();
    for (uint32_t v = 0; v < t.nv(); ++v) {
      uint32_t first_c = t.vcorner[v];
      if (first_c == kInvalid) continue;
      if (vert_seam[v]) {
        uint32_t act = swing_left(first_c);
        size_t guard = 0;
        while (act != kInvalid) { first_c = act; act = swing_left(act); check(++guard <= t.nc(), "attribute seam loop"); }
      }
      uint32_t id = (uint32_t)v2lm.size();
      c2v[first_c] = id;
      v2lm.push_back(first_c);
      uint32_t act = t.swing_right(first_c);
      while (act != kInvalid && act != first_c) {
        if (edge_seam[next(act)]) { id = (uint32_t)v2lm.size(); v2lm.push_back(act); }
        c2v[act] = id;
        act = t.swing_right(act);
      }
    }
  }
};

// DFS traversal shared by attribute sequencing (Traverser/DepthFirstTraverser.cs:9-99)
struct Sequence {
  std::vector<uint32_t> data_to_corner;   // entry -> corner (source corner table)
  std::vector<int32_t> vertex_to_data;
};
template <class CT>
static void dfs_sequence(const CT &ct, const std::vector<uint32_t> &corner_order, Sequence &seq) {
  std::vector<uint8_t> fvis(ct.nf(), 0), vvis(ct.nv(), 0);
  seq.vertex_to_data.assign(ct.nv(), -1);
  seq.data_to_corner.clear();
  std::vector<uint32_t> stack;
  auto visit = [&](uint32_t v, uint32_t c) { vvis[v] = 1; seq.vertex_to_data[v] = (int32_t)seq.data_to_corner.size(); seq.data_to_corner.push_back(c); };
  auto fdone = [&](uint32_t f) { return f == kInvalid || fvis[f]; };
  for (uint32_t start : corner_order) {
    if (fdone(start / 3)) continue;
    stack.clear();
    stack.push_back(start);
    uint32_t nv = ct.vertex(CT::next(start)), pv = ct.vertex(CT::prev(start));
    if (!vvis[nv]) visit(nv, CT::next(start));
    if (!vvis[pv]) visit(pv, CT::prev(start));
    while (!stack.empty()) {
      uint32_t corner = stack.back();
      uint32_t face = corner == kInvalid ? kInvalid : corner / 3;
      if (corner == kInvalid || fdone(face)) { stack.pop_back(); continue; }
      for (;;) {
        fvis[face] = 1;
        uint32_t v = ct.vertex(corner);
        if (!vvis[v]) {
          bool ob = ct.on_boundary(v);
          visit(v, corner);
          if (!ob) { corner = ct.right_corner(corner); face = corner / 3; continue; }
        }
        uint32_t rc = ct.right_corner(corner), lc = ct.left_corner(corner);
        uint32_t rf = rc == kInvalid ? kInvalid : rc / 3, lf = lc == kInvalid ? kInvalid : lc / 3;
        if (fdone(rf)) {
          if (fdone(lf)) { stack.pop_back(); break; }
          corner = lc; face = lf;
        } else {
          if (fdone(lf)) { corner = rc; face = rf; }
          else { stack.back() = lc; stack.push_back(rc); break; }
        }
      }
    }
  }
}

// MaxPredictionDegreeTraverser.cs:22-152 (with the degree list sized, as in the bitstream): faces whose tip vertex is
// already coded first, then tips seen from two faces, then the rest.
static void prediction_degree_sequence(const CornerTable &ct, const std::vector<uint32_t> &corner_order, Sequence &seq) {
  std::vector<uint8_t> fvis(ct.nf(), 0), vvis(ct.nv(), 0);
  std::vector<uint32_t> degree(ct.nv(), 0), stacks[3];
  seq.vertex_to_data.assign(ct.nv(), -1);
  seq.data_to_corner.clear();
  int best = 0;
  auto visit = [&](uint32_t v, uint32_t c) { vvis[v] = 1; seq.vertex_to_data[v] = (int32_t)seq.data_to_corner.size(); seq.data_to_corner.push_back(c); };
  auto fdone = [&](uint32_t c) { return c == kInvalid || fvis[c / 3]; };
  auto pop = [&]() {
    for (int i = best; i < 3; ++i) if (!stacks[i].empty()) { uint32_t c = stacks[i].back(); stacks[i].pop_back(); best = i; return c; }
    return kInvalid;
  };
  auto push = [&](uint32_t c, int pr) { stacks[pr].push_back(c); if (pr < best) best = pr; };
  auto priority = [&](uint32_t c) { uint32_t v = ct.vertex(c); if (vvis[v]) return 0; return ++degree[v] > 1 ? 1 : 2; };
  for (uint32_t start : corner_order) {
    stacks[0].push_back(start);
    best = 0;
    uint32_t nv = ct.vertex(CornerTable::next(start)), pv = ct.vertex(CornerTable::prev(start)), tv = ct.vertex(start);
    if (!vvis[nv]) visit(nv, CornerTable::next(start));
    if (!vvis[pv]) visit(pv, CornerTable::prev(start));
    if (!vvis[tv]) visit(tv, start);
    uint32_t corner;
    while ((corner = pop()) != kInvalid) {
      if (fdone(corner)) continue;
      for (;;) {
        fvis[corner / 3] = 1;
        uint32_t v = ct.vertex(corner);
        if (!vvis[v]) visit(v, corner);
        uint32_t rc = ct.right_corner(corner), lc = ct.left_corner(corner);
        const bool rdone = fdone(rc), ldone = fdone(lc);
        if (!ldone) { int pr = priority(lc); if (rdone && pr <= best) { corner = lc; continue; } push(lc, pr); }
        if (!rdone) { int pr = priority(rc); if (pr <= best) { corner = rc; continue; } push(rc, pr); }
        break;
      }
    }
  }
}

// ------------------------------------------------- Edgebreaker connectivity
struct EbResult {
  std::vector<uint8_t> symbols;               // encoder order, bit patterns (0,1,3,5,7)
  std::vector<uint8_t> start_face_bits;
  std::vector<uint32_t> processed_corners;    // decoder face order
  struct Split { uint32_t source, split, edge; };
  std::vector<Split> splits;
  uint32_t num_split_symbols = 0;
  std::vector<uint32_t> face_time;            // face -> index of the first symbol coded with the face already visited
};

struct EbEncoder {
  const CornerTable &ct;
  EbResult &r;
  std::vector<uint8_t> visited_faces, visited_verts, visited_holes;
  std::vector<int32_t> vertex_hole_id;
  std::map<int, int> face_to_split_symbol;
  int last_symbol_id = -1;
  EbEncoder(const CornerTable &t, EbResult &res) : ct(t), r(res) {}

  void find_holes() {     // MeshEdgeBreakerEncoder.cs:331-361
    for (uint32_t i = 0; i < ct.nc(); ++i) {
      if (ct.opposite(i) != kInvalid) continue;
      uint32_t bv = ct.vertex(CornerTable::next(i));
      if (vertex_hole_id[bv] != -1) continue;
      int id = (int)visited_holes.size();
      visited_holes.push_back(0);
      uint32_t c = i;
      while (vertex_hole_id[bv] == -1) {
        vertex_hole_id[bv] = id;
        c = CornerTable::next(c);
        while (ct.opposite(c) != kInvalid) c = CornerTable::next(ct.opposite(c));
        bv = ct.vertex(CornerTable::next(c));
      }
    }
  }
  bool find_init_face(uint32_t face, uint32_t *out) {   // :158-183
    uint32_t corner = 3 * face;
    for (int i = 0; i < 3; ++i) {
      if (ct.opposite(corner) == kInvalid) { *out = corner; return false; }
      if (vertex_hole_id[ct.vertex(corner)] != -1) {
        uint32_t rc = corner;
        while (rc != kInvalid) { corner = rc; rc = ct.swing_right(rc); }
        *out = CornerTable::prev(corner);
        return false;
      }
      corner = CornerTable::next(corner);
    }
    *out = corner;
    return true;
  }
  void encode_hole(uint32_t start_corner, bool encode_first) {   // :276-303
    uint32_t c = CornerTable::prev(start_corner);
    while (ct.opposite(c) != kInvalid) c = CornerTable::next(ct.opposite(c));
    uint32_t start_v = ct.vertex(start_corner);
    if (encode_first) visited_verts[start_v] = 1;
    visited_holes[vertex_hole_id[start_v]] = 1;
    uint32_t act = ct.vertex(CornerTable::prev(c));
    while (act != start_v) {
      visited_verts[act] = 1;
      c = CornerTable::next(c);
      while (ct.opposite(c) != kInvalid) c = CornerTable::next(ct.opposite(c));
      act = ct.vertex(CornerTable::prev(c));
    }
  }
  bool right_visited(uint32_t c) const { uint32_t o = ct.opposite(CornerTable::next(c)); return o == kInvalid || visited_faces[o / 3]; }
  bool left_visited(uint32_t c) const { uint32_t o = ct.opposite(CornerTable::prev(c)); return o == kInvalid || visited_faces[o / 3]; }
  void check_split(int src_symbol, uint32_t edge, uint32_t neighbor_face) {   // :373-390
    auto it = face_to_split_symbol.find((int)neighbor_face);
    if (it == face_to_split_symbol.end()) return;
    r.splits.push_back({(uint32_t)src_symbol, (uint32_t)it->second, edge});
  }
  void encode_from_corner(uint32_t corner) {   // :185-274
    std::vector<uint32_t> stack{corner};
    while (!stack.empty()) {
      corner = stack.back();
      if (corner == kInvalid || visited_faces[corner / 3]) { stack.pop_back(); continue; }
      for (;;) {
        ++last_symbol_id;
        uint32_t face = corner / 3;
        visited_faces[face] = 1;
        r.face_time[face] = (uint32_t)last_symbol_id;
        r.processed_corners.push_back(corner);
        uint32_t v = ct.vertex(corner);
        bool on_boundary = vertex_hole_id[v] != -1;
        if (!visited_verts[v]) {
          visited_verts[v] = 1;
          if (!on_boundary) { r.symbols.push_back(0); corner = ct.right_corner(corner); continue; }
        }
        uint32_t rc = ct.right_corner(corner), lc = ct.left_corner(corner);
        uint32_t rf = rc == kInvalid ? kInvalid : rc / 3, lf = lc == kInvalid ? kInvalid : lc / 3;
        if (right_visited(corner)) {
          if (rf != kInvalid) check_split(last_symbol_id, 1, rf);
          if (left_visited(corner)) {
            if (lf != kInvalid) check_split(last_symbol_id, 0, lf);
            r.symbols.push_back(7);
            stack.pop_back();
            break;
          }
          r.symbols.push_back(5);
          corner = lc;
        } else {
          if (left_visited(corner)) {
            if (lf != kInvalid) check_split(last_symbol_id, 0, lf);
            r.symbols.push_back(3);
            corner = rc;
          } else {
            r.symbols.push_back(1);
            ++r.num_split_symbols;
            if (on_boundary) {
              int hid = vertex_hole_id[v];
              if (!visited_holes[hid]) encode_hole(corner, false);
            }
            face_to_split_symbol[(int)face] = last_symbol_id;
            stack.back() = lc;
            stack.push_back(rc);
            break;
          }
        }
      }
    }
  }
  void run() {   // MeshEdgeBreakerEncoder.cs:38-124
    visited_faces.assign(ct.nf(), 0);
    r.face_time.assign(ct.nf(), kInvalid);
    visited_verts.assign(ct.nv(), 0);
    vertex_hole_id.assign(ct.nv(), -1);
    find_holes();
    std::vector<uint32_t> init_corners;
    for (uint32_t c = 0; c < ct.nc(); ++c) {
      uint32_t face = c / 3;
      if (visited_faces[face]) continue;
      uint32_t start;
      bool interior = find_init_face(face, &start);
      r.start_face_bits.push_back(interior ? 1 : 0);
      if (interior) {
        visited_verts[ct.vertex(start)] = 1;
        visited_verts[ct.vertex(CornerTable::next(start))] = 1;
        visited_verts[ct.vertex(CornerTable::prev(start))] = 1;
        visited_faces[face] = 1;
        r.face_time[face] = (uint32_t)(last_symbol_id + 1);
        init_corners.push_back(CornerTable::next(start));
        uint32_t o = ct.opposite(CornerTable::next(start));
        if (o != kInvalid && !visited_faces[o / 3]) encode_from_corner(o);
      } else {
        encode_hole(CornerTable::next(start), true);
        encode_from_corner(start);
      }
    }
    std::reverse(r.processed_corners.begin(), r.processed_corners.end());
    r.processed_corners.insert(r.processed_corners.end(), init_corners.begin(), init_corners.end());
  }
};

// Predictive Edgebreaker traversal, encoder side (the reference has only the decoder,
// MeshEdgeBreakerTraversalPredictiveDecoder.cs:19-93; this follows the format's encoder): valences of the not yet
// coded part of the mesh are what the decoder will have built when it gets there.  Before a C or R symbol the
// previous symbol (the decoder's next) is predicted from the valence of the pivot: a hit costs one bit, a miss one
// bit and the symbol.  The tip of a split face is poisoned (two decoder vertices until the S merges them).
static void predictive_symbols(const CornerTable &ct, const EbResult &eb, std::vector<uint8_t> &explicit_symbols, std::vector<uint8_t> &predictions) {
  const size_t n = eb.symbols.size();
  std::vector<int32_t> valence(ct.nv(), 0);
  for (uint32_t c = 0; c < ct.nc(); ++c) {                 // edges around a vertex: faces, +1 on a boundary
    valence[ct.vertex(c)] += 1;
    if (ct.opposite(CornerTable::prev(c)) == kInvalid) valence[ct.vertex(c)] += 1;   // the boundary edge leaving the fan on this side
  }
  explicit_symbols.clear();
  predictions.clear();
  int prev_symbol = -1;
  for (size_t i = 0; i < n; ++i) {
    const uint8_t symbol = eb.symbols[i];
    const uint32_t corner = eb.processed_corners[n - 1 - i], next = CornerTable::next(corner), prev = CornerTable::prev(corner);
    const uint32_t a = ct.vertex(corner), b = ct.vertex(next), c = ct.vertex(prev);
    auto predict = [&](uint32_t pivot) { const int32_t v = valence[pivot]; return v < 0 ? -2 : (v < 6 ? 5 : 0); };
    int predicted = -1;
    switch (symbol) {
      case 0: predicted = predict(b); valence[b] -= 1; valence[c] -= 1; break;
      case 1: valence[b] -= 1; valence[c] -= 1; valence[a] = -1; break;
      case 5: predicted = predict(b); valence[a] -= 1; valence[b] -= 1; valence[c] -= 2; break;
      case 3: valence[a] -= 1; valence[b] -= 2; valence[c] -= 1; break;
      default: valence[a] -= 2; valence[b] -= 2; valence[c] -= 2; break;
    }
    bool store_prev = true;
    if (predicted != -1) {
      if (predicted == prev_symbol) { predictions.push_back(1); store_prev = false; }
      else if (prev_symbol != -1) predictions.push_back(0);
    }
    if (store_prev && prev_symbol != -1) explicit_symbols.push_back((uint8_t)prev_symbol);
    prev_symbol = symbol;
  }
  if (prev_symbol != -1) explicit_symbols.push_back((uint8_t)prev_symbol);
}

// Valence Edgebreaker traversal, encoder side (decoder: MeshEdgeBreakerTraversalValenceDecoder.cs:22-154): every
// symbol but the last coded one goes into one of six lists chosen by the valence, in the not yet coded part of the
// mesh, of the vertex the decoder will stand on when it reads it.  A split face's tip is two decoder vertices until
// the S merges them: the encoder splits it the same way (faces left of the split keep the vertex, faces right of it
// get a new one).  Symbol ids: C 0, S 1, L 2, R 3, E 4 (Constants.cs:88-95).
static void valence_context_symbols(const CornerTable &ct, const EbResult &eb, std::vector<uint32_t> ctx[6]) {
  const size_t n = eb.symbols.size();
  std::vector<int32_t> valence(ct.nv(), 0);
  for (uint32_t c = 0; c < ct.nc(); ++c) {
    valence[ct.vertex(c)] += 1;
    if (ct.opposite(CornerTable::prev(c)) == kInvalid) valence[ct.vertex(c)] += 1;
  }
  std::vector<uint32_t> c2v(ct.nc());
  for (uint32_t c = 0; c < ct.nc(); ++c) c2v[c] = ct.vertex(c);
  for (int i = 0; i < 6; ++i) ctx[i].clear();
  int prev_symbol = -1;
  for (size_t i = 0; i < n; ++i) {
    const uint8_t symbol = eb.symbols[i];
    const uint32_t corner = eb.processed_corners[n - 1 - i], next = CornerTable::next(corner), prev = CornerTable::prev(corner);
    auto coded = [&](uint32_t c) { return eb.face_time[c / 3] <= i; };
    const int32_t active_valence = valence[c2v[next]];
    switch (symbol) {
      case 0: valence[c2v[next]] -= 1; valence[c2v[prev]] -= 1; break;
      case 1: {
        valence[c2v[next]] -= 1; valence[c2v[prev]] -= 1;
        int left = 0, right = 0;
        uint32_t a = ct.opposite(prev);
        while (a != kInvalid && !coded(a)) { ++left; a = ct.opposite(CornerTable::next(a)); }
        valence[c2v[corner]] = left + 1;
        const uint32_t nv = (uint32_t)valence.size();
        a = ct.opposite(next);
        while (a != kInvalid && !coded(a)) { ++right; c2v[CornerTable::next(a)] = nv; a = ct.opposite(CornerTable::prev(a)); }
        valence.push_back(right + 1);
        break;
      }
      case 5: valence[c2v[corner]] -= 1; valence[c2v[next]] -= 1; valence[c2v[prev]] -= 2; break;
      case 3: valence[c2v[corner]] -= 1; valence[c2v[next]] -= 2; valence[c2v[prev]] -= 1; break;
      default: valence[c2v[corner]] -= 2; valence[c2v[next]] -= 2; valence[c2v[prev]] -= 2; break;
    }
    if (prev_symbol != -1) {
      const int clamped = active_valence < 2 ? 2 : (active_valence > 7 ? 7 : active_valence);
      static const uint32_t id_of[8] = {0, 1, 0, 2, 0, 3, 0, 4};
      ctx[clamped - 2].push_back(id_of[prev_symbol]);
    }
    prev_symbol = symbol;
  }
}

// ----------------------------------------------------------------- options
struct Options {
  int32_t pos_bits = 11, uv_bits = 10, normal_bits = 8;
  int32_t single_connectivity = 0;   // split_mesh_on_seams=false at speed 5 -> per-attribute connectivity
  int32_t force_scheme = -1;         // -1 auto, 0 tagged, 1 raw
  int32_t compression_level = 5;     // 10 - speed
  int32_t pos_prediction = 1;        // 1 parallelogram, 0 difference
  int32_t uv_prediction = 1;
  int32_t generic_u8 = 0;            // add a per-vertex uint8 generic attribute (Integer decoder) when generic data is given
  int32_t normal_prediction = 0;     // 0 difference, 6 geometric normal (the CPU coder only)
  int32_t predictive_connectivity = 0;   // 1: predictive Edgebreaker traversal (deprecated in the format); 2: valence traversal, what stock
                                         // encoders write at their default level (CPU coder only)
  int32_t traversal_method = 0;      // attribute sequencing: 0 depth first; 1 prediction degree for the decoder of the positions
                                     // (what stock encoders do at their highest level); 2 prediction degree for every decoder (CPU coder only)
  // Decoder branches no stock encoder setting reaches (CPU coder only; tests and tools/soak.py):
  int32_t normal_transform = 3;      // 3 NormalOctahedronCanonicalized, 2 NormalOctahedron (difference prediction)
  int32_t raw_integers = 0;          // 1 / 2 / 3 / 4: values of the difference / parallelogram attributes stored uncompressed at that many
                                     // bytes (SequentialIntegerAttributeDecoder.cs:68-84)
  int32_t no_prediction = 0;         // bit 0 positions, bit 1 texture coordinates, bit 2 normals, bit 3 the generic attribute: prediction
                                     // method -2 (none)
  int32_t generic_components = 1;    // components of the generic attribute (4 = the RGBA colours of a scan)
  int32_t generic_data_type = 2;     // element type of the generic attribute, Draco's ids: 1 int8, 2 uint8, 3 int16, 4 uint16, 5 int32,
                                     // 6 uint32 (joint indices, 16-bit colours, feature ids); the device encoder's generic attribute is
                                     // uint8, it writes the other types from MeshIn::extras (dsa_mesh_attr_input)
  int32_t repair_topology = 0;       // 1: the reference's corner table (CornerTable::build_repaired) in place of the refusal of degenerate
                                     // faces, non-manifold edges and vertices and isolated vertices; a clean mesh gives the same bytes
                                     // 2: as 1, and attributes given per corner are coded over the repaired table (1 refuses them)
};

// Octahedral quantisation (OctahedronToolBox.cs:28-119)
struct Octa {
  int q, max_q, max_value, center;
  explicit Octa(int bits) { q = bits; max_q = (1 << bits) - 1; max_value = max_q - 1; center = max_value / 2; }
  void canonicalize(int &s, int &t) const {
    if ((s == 0 && t == 0) || (s == 0 && t == max_value) || (s == max_value && t == 0)) { s = max_value; t = max_value; }
    else if (s == 0 && t > center) t = center - (t - center);
    else if (s == max_value && t < center) t = center + (center - t);
    else if (t == max_value && s < center) s = center + (center - s);
    else if (t == 0 && s > center) s = center - (s - center);
  }
  void from_int_vector(const int v[3], int &s, int &t) const {
    if (v[0] >= 0) { s = v[1] + center; t = v[2] + center; }
    else {
      s = v[1] < 0 ? std::abs(v[2]) : max_value - std::abs(v[2]);
      t = v[2] < 0 ? std::abs(v[1]) : max_value - std::abs(v[1]);
    }
    canonicalize(s, t);
  }
  void from_float_vector(const float in[3], int &s, int &t) const {
    double v[3] = {in[0], in[1], in[2]};
    double abs_sum = std::fabs(v[0]) + std::fabs(v[1]) + std::fabs(v[2]);
    double sv[3];
    if (abs_sum > 1e-6) { double sc = 1.0 / abs_sum; sv[0] = v[0] * sc; sv[1] = v[1] * sc; sv[2] = v[2] * sc; }
    else { sv[0] = 1; sv[1] = 0; sv[2] = 0; }
    from_scaled((int)std::floor(sv[0] * center + 0.5), (int)std::floor(sv[1] * center + 0.5), sv[2] < 0, s, t);
  }
  // the quantiser's tail, shared with merge_mean_normals: the code of the vector scaled to L1 norm `center` whose first two
  // components rounded to i0 and i1 and whose third is negative or not
  void from_scaled(int i0, int i1, bool z_negative, int &s, int &t) const {
    int iv[3] = {i0, i1, center - std::abs(i0) - std::abs(i1)};
    if (iv[2] < 0) { if (iv[1] > 0) iv[1] += iv[2]; else iv[1] -= iv[2]; iv[2] = 0; }
    if (z_negative) iv[2] *= -1;
    from_int_vector(iv, s, t);
  }
  bool in_diamond(int s, int t) const { return (uint32_t)std::abs(s) + (uint32_t)std::abs(t) <= (uint32_t)center; }
  void invert_diamond(int &s, int &t) const {
    int ss, st;
    if (s >= 0 && t >= 0) { ss = 1; st = 1; }
    else if (s <= 0 && t <= 0) { ss = -1; st = -1; }
    else { ss = s > 0 ? 1 : -1; st = t > 0 ? 1 : -1; }
    int cs = ss * center, ctt = st * center;
    int us = s + s - cs, ut = t + t - ctt, tmp = us;
    if (ss * st >= 0) { us = -ut; ut = -tmp; } else { us = ut; ut = tmp; }
    us += cs; ut += ctt;
    s = us / 2; t = ut / 2;
  }
  int make_positive(int x) const { return x < 0 ? x + max_q : x; }
};

// A quantisation grid given by the caller (the layout of dsa_quantization_grid): mode 0 the attribute's own bounds, 1 explicit
// (origin per component, one range), 2 shared by the meshes of a group -- which whoever holds the batch resolves to mode 1
// (shared_grid below); the coder of one mesh takes 0 and 1.
struct Grid { float origin[4]; float range; int32_t mode; uint32_t reserved[2]; };
static inline bool f32_finite(float f) { uint32_t u; memcpy(&u, &f, 4); return (u & 0x7F800000u) != 0x7F800000u; }
// the attribute slots a grid can name, as the messages call them
static inline std::string grid_slot_name(int att_type, int extra) {
  if (extra >= 0) return "attribute " + std::to_string(extra);
  return att_type == 0 ? "positions" : (att_type == 1 ? "normals" : (att_type == 3 ? "texcoords" : "generic"));
}
// Why grid `g` cannot shape an attribute of nc components ("" when it can); quantised: the attribute is one that has a grid.
static std::string grid_error(const Grid &g, int nc, bool quantised, const std::string &name) {
  char buf[160];
  if (g.reserved[0] != 0 || g.reserved[1] != 0) return name + ": grid.reserved is not zero";
  if (g.mode < 0 || g.mode > 2) { snprintf(buf, sizeof(buf), ": grid.mode %d: 0 (own bounds), 1 (explicit) or 2 (shared within the group)", (int)g.mode); return name + buf; }
  if (g.mode != 0 && !quantised) { snprintf(buf, sizeof(buf), ": grid.mode %d on an attribute that is not quantised (normals and integer attributes have no grid)", (int)g.mode); return name + buf; }
  if (g.mode != 1) return "";
  if (!f32_finite(g.range) || !(g.range > 0.0f)) { snprintf(buf, sizeof(buf), ": grid.range %g: finite and above 0", (double)g.range); return name + buf; }
  for (int c = 0; c < nc; ++c)
    if (!f32_finite(g.origin[c])) { snprintf(buf, sizeof(buf), ": grid.origin[%d] is not finite", c); return name + buf; }
  return "";
}
// the same for an attribute the mesh does not have: only mode 0 is legal
static std::string grid_error_absent(const Grid &g, const std::string &name) {
  Grid z = g;
  z.mode = g.mode >= 1 && g.mode <= 2 ? 0 : g.mode;
  const std::string why = grid_error(z, 0, true, name);
  if (!why.empty() || g.mode == 0) return why;
  return name + ": grid.mode " + std::to_string(g.mode) + " for an attribute the mesh does not have";
}
// The refusal of a mesh whose attribute does not fit its grid: the smallest row with a value that is not finite, else the
// smallest row with a value whose integer lies outside 0 .. max_q.
static inline std::string grid_row_message(const std::string &name, uint32_t row, bool finite) {
  return name + ": row " + std::to_string(row) + (finite ? " lies off the quantisation grid" : " is not finite");
}
// -0.0 below +0.0, so that minima and maxima do not depend on the order they are taken in
static inline uint32_t f32_order_key(float f) { uint32_t u; memcpy(&u, &f, 4); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
static inline float f32_from_order_key(uint32_t k) { const uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; float f; memcpy(&f, &u, 4); return f; }
// The grid of a group (mode 2): ComputeParameters over the union of `count` arrays of nc components -- minimum per component
// over all rows of every array whose values are all finite, range the largest extent, 1 if that is 0.  False: no such array.
static bool shared_grid(const float *const *arrays, const uint32_t *rows, uint32_t count, int nc, Grid &out) {
  uint32_t mn[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[4] = {0, 0, 0, 0};
  bool any = false;
  for (uint32_t k = 0; k < count; ++k) {
    const size_t total = (size_t)rows[k] * nc;
    bool finite = total > 0;
    for (size_t i = 0; i < total && finite; ++i) finite = f32_finite(arrays[k][i]);
    if (!finite) continue;
    any = true;
    for (size_t i = 0; i < total; ++i) { const uint32_t key = f32_order_key(arrays[k][i]); const int c = (int)(i % nc); if (key < mn[c]) mn[c] = key; if (key > mx[c]) mx[c] = key; }
  }
  memset(&out, 0, sizeof(out));
  out.mode = 1; out.range = 1.0f;
  if (!any) return false;
  float range = 0.0f;
  for (int c = 0; c < nc; ++c) {
    out.origin[c] = f32_from_order_key(mn[c]);
    volatile float d = f32_from_order_key(mx[c]) - out.origin[c];
    if (d > range) range = d;
  }
  out.range = range == 0.0f ? 1.0f : range;
  return true;
}

struct PortableAttr {
  int att_type, nc_out, nc;            // nc = portable components
  int seq_type;                        // 1 integer, 2 quantisation, 3 normals
  int data_type;
  std::vector<int32_t> vals;           // per value id, AoS (value id = vertex unless corner_value is set)
  const uint32_t *corner_value = nullptr;   // value id per corner of the source mesh (attributes given per corner: seams)
  std::vector<float> qmin; float qrange = 1; int bits = 0;
  int prediction = 1;
  int normalized = 0;                  // the descriptor's flag
  uint32_t unique_id = kInvalid;       // kInvalid: the attribute's index in the stream
  const void *extra_values = nullptr;  // an attribute of MeshIn::extras: its rows, nc elements of data_type each (else the built-in source)
  const Grid *grid = nullptr;          // seq_type 2: the caller's grid (mode 1; null or mode 0: the attribute's own bounds)
  int extra_index = -1;                // its index in MeshIn::extras (the messages name it)
  uint32_t extra_rows = 0;             // an attribute of MeshIn::extras given per corner: the rows of extra_values (corner_value indexes them)
  const int32_t *portable = nullptr;   // seq_type 2: the integers to code, one row per value id, in place of the quantiser's output (bounds and grid as the floats give them)
};

// AttributeQuantizationTransform.cs:66-108,136-177 + Core/Quantizer.cs (E-1 corrected)
// A grid of the caller's (a.grid, mode 1) takes the place of the bounds: the arithmetic is the same, and a value that is not
// finite or whose integer leaves 0 .. max_q refuses the mesh (grid_row_message).
static void quantize_on_grid(const float *src, uint32_t n, int nc, int bits, PortableAttr &a) {
  const Grid &g = *a.grid;
  const std::string name = grid_slot_name(a.att_type, a.extra_index);
  const std::string why = grid_error(g, nc, true, name);
  check(why.empty(), why.c_str());
  check(g.mode == 1, (name + ": grid.mode 2 (shared) is resolved to an explicit grid by whoever holds the batch").c_str());
  a.qmin.assign(g.origin, g.origin + nc);
  a.qrange = g.range;
  a.bits = bits;
  const int32_t max_q = (1 << bits) - 1;
  volatile float inv_delta = (float)max_q / a.qrange;
  a.vals.assign((size_t)n * nc, 0);
  uint32_t bad_finite = kInvalid, bad_off = kInvalid;
  for (uint32_t i = 0; i < n; ++i)
    for (int c = 0; c < nc; ++c) {
      const float x = src[(size_t)i * nc + c];
      if (!f32_finite(x)) { if (bad_finite == kInvalid) bad_finite = i; continue; }
      volatile float v = x - a.qmin[c];
      volatile float s = v * inv_delta;
      const float f = std::floor(s + 0.5f);
      if (!(f >= 0.0f && f <= (float)max_q)) { if (bad_off == kInvalid) bad_off = i; continue; }
      a.vals[(size_t)i * nc + c] = (int32_t)f;
    }
  if (bad_finite != kInvalid) check(false, grid_row_message(name, bad_finite, false).c_str());
  if (bad_off != kInvalid) check(false, grid_row_message(name, bad_off, true).c_str());
}
// The attribute's own bounds can refuse a mesh too.  A value that is not finite does, in the words of a grid (the reference
// throws "NaN values are not supported", AttributeQuantizationTransform.cs:82,96): grid_row_message with the smallest such row.
// So does a range the bit depth cannot carry: the extent max - min overflowed to infinity, or max_q / range did (a range
// below about max_q * 2.9e-39) -- every integer would be what an undefined float-to-int cast makes of an infinity or a NaN.
static inline bool quant_range_ok(float range, int bits) {
  volatile float inv_delta = (float)((1 << bits) - 1) / range;
  return f32_finite(range) && f32_finite(inv_delta);
}
static inline std::string quant_range_message(const std::string &name, float range, int bits) {
  char buf[160];
  snprintf(buf, sizeof(buf), ": the range %g of its values cannot carry %d quantisation bits (the range and (2^bits - 1) / range must be finite)", (double)range, bits);
  return name + buf;
}
// The minimum of a component carries the bits of the first row that attains it (a strict compare, taken serially, as the
// reference takes it: `MinValues[c] > v`, :76-92), which decides the sign of a zero minimum in the header.
static void quantize(const float *src, uint32_t n, int nc, int bits, PortableAttr &a) {
  if (a.grid && a.grid->mode != 0) return quantize_on_grid(src, n, nc, bits, a);
  const std::string name = grid_slot_name(a.att_type, a.extra_index);
  for (size_t i = 0, total = (size_t)n * nc; i < total; ++i)
    if (!f32_finite(src[i])) check(false, grid_row_message(name, (uint32_t)(i / nc), false).c_str());
  a.qmin.assign(nc, 0);
  std::vector<float> mx(nc, 0);
  for (int c = 0; c < nc; ++c) { a.qmin[c] = src[c]; mx[c] = src[c]; }
  for (uint32_t i = 1; i < n; ++i)
    for (int c = 0; c < nc; ++c) { float v = src[(size_t)i * nc + c]; if (v < a.qmin[c]) a.qmin[c] = v; if (v > mx[c]) mx[c] = v; }
  a.qrange = 0;
  for (int c = 0; c < nc; ++c) { float d = mx[c] - a.qmin[c]; if (d > a.qrange) a.qrange = d; }
  if (a.qrange == 0.0f) a.qrange = 1.0f;
  a.bits = bits;
  if (!quant_range_ok(a.qrange, bits)) check(false, quant_range_message(name, a.qrange, bits).c_str());
  int32_t max_q = (1 << bits) - 1;
  volatile float inv_delta = (float)max_q / a.qrange;
  a.vals.resize((size_t)n * nc);
  for (uint32_t i = 0; i < n; ++i)
    for (int c = 0; c < nc; ++c) {
      volatile float v = src[(size_t)i * nc + c] - a.qmin[c];
      volatile float s = v * inv_delta;
      a.vals[(size_t)i * nc + c] = (int32_t)std::floor(s + 0.5f);
    }
}

// Corrections -----------------------------------------------------------------
struct WrapEnc {   // PredictionSchemeWrapEncodingTransform.cs:45-90 (E-5 corrected) + WrapTransform.cs:88-100
  int32_t mn = 0, mx = 0, max_dif = 0, max_corr = 0, min_corr = 0;
  void init(const std::vector<int32_t> &d) {
    if (d.empty()) return;
    mn = mx = d[0];
    for (int32_t v : d) { if (v < mn) mn = v; if (v > mx) mx = v; }
    max_dif = 1 + mx - mn;
    max_corr = max_dif / 2;
    min_corr = -max_corr;
    if ((max_dif & 1) == 0) max_corr -= 1;
  }
  int32_t corr(int32_t orig, int32_t pred) const {
    int32_t p = pred > mx ? mx : (pred < mn ? mn : pred);
    int32_t c = orig - p;
    if (c < min_corr) c += max_dif; else if (c > max_corr) c -= max_dif;
    return c;
  }
};

static void rotate(int &x, int &y, int rot) {
  int a = x, b = y;
  switch (rot) { case 1: x = b; y = -a; break; case 2: x = -a; y = -b; break; case 3: x = -b; y = a; break; default: break; }
}
// PredictionSchemeNormalOctahedronCanonicalizedEncodingTransform.cs:47-83
static void oct_canon_corr(const Octa &o, const int32_t orig_in[2], const int32_t pred_in[2], int32_t out[2]) {
  int os = orig_in[0] - o.center, ot = orig_in[1] - o.center;
  int ps = pred_in[0] - o.center, pt = pred_in[1] - o.center;
  if (!o.in_diamond(ps, pt)) { o.invert_diamond(os, ot); o.invert_diamond(ps, pt); }
  bool bottom_left = (ps == 0 && pt == 0) || (ps < 0 && pt <= 0);
  if (!bottom_left) {
    int rot;
    if (ps == 0) rot = pt == 0 ? 0 : (pt > 0 ? 3 : 1);
    else if (ps > 0) rot = pt >= 0 ? 2 : 1;
    else rot = pt <= 0 ? 0 : 3;
    rotate(os, ot, rot); rotate(ps, pt, rot);
  }
  out[0] = o.make_positive(os - ps);
  out[1] = o.make_positive(ot - pt);
}

// Element k of a generic attribute of Draco data type dt as its int32 value (uint32 by reinterpretation).
static int32_t generic_value(const void *g, size_t k, int dt) {
  switch (dt) {
    case 1: return ((const int8_t *)g)[k];
    case 2: return ((const uint8_t *)g)[k];
    case 3: return ((const int16_t *)g)[k];
    case 4: return ((const uint16_t *)g)[k];
    case 5: return ((const int32_t *)g)[k];
    case 6: return (int32_t)((const uint32_t *)g)[k];
    default: check(false, "generic_data_type must be 1 (int8) to 6 (uint32)"); return 0;
  }
}

// One more attribute behind the built-in ones (positions, normals, texture coordinates, the generic attribute):
// colours, joints and weights, a second UV set, feature ids.  Integer element types are coded as they are, float32 quantised.
// Per vertex, or -- like normals and texture coordinates -- per corner: `corners` holds a row id per corner of the faces into
// `values` (`rows` of them), and an interior edge across which the ids differ is a seam of this attribute alone (lightmap charts,
// a colour with a hard edge).  This library's decoder takes corner attributes for attribute data 0 to 6, so ids are for the
// attributes at indices 1 to 7 of the stream (extras_error).
struct ExtraAttr {
  int32_t att_type = 4;              // 2 colour, 3 texture coordinate, 4 generic
  int32_t data_type = 2;             // Draco's ids: 1 int8 ... 6 uint32, 9 float32
  uint32_t nc = 1;                   // 1..4
  int32_t normalized = 0;            // 0 / 1, into the descriptor (integer types)
  uint32_t unique_id = kInvalid;     // kInvalid: the attribute's index in the stream
  int32_t bits = 0;                  // float32: 1..20; 0: uv_bits for a texture coordinate, else 8
  const void *values = nullptr;      // nv rows, packed
  const Grid *grid = nullptr;        // float32: the caller's quantisation grid (null: its own bounds)
  const uint32_t *corners = nullptr; // 3 * nf row ids into `values`, or null: one row per vertex
  uint32_t rows = 0;                 // rows of `values` when `corners` is set
  const int32_t *portable = nullptr; // float32: the integers to code in place of the quantiser's output (merge_means' twin), bounds and grid untouched
};
static const size_t kMaxAttributes = 16;   // DSA_MAX_ATTRIBUTES: what the decode direction takes
static const size_t kMaxCornerAttributeIndex = 7;      // the last index of the stream whose attribute may have a connectivity of its own (attribute data 0 to 6)
static inline size_t data_type_size(int dt) { return (dt == 1 || dt == 2) ? 1 : ((dt == 3 || dt == 4) ? 2 : 4); }

struct MeshIn {
  const float *pos; uint32_t nv; const uint32_t *faces; uint32_t nf;
  const float *normals; const float *uvs;
  const void *generic;               // nv * generic_components elements of Options::generic_data_type (uint8 unless the CPU coder is told otherwise)
  // Attributes given per corner (the CPU coder only): value ids per corner of `faces` (3 * nf) into `normals` (nn rows) /
  // `uvs` (nu rows); an interior edge whose end points carry different ids on its two faces is an attribute seam
  // (MeshAttributeCornerTable.cs:32-78).  Null: one value per vertex.
  const uint32_t *normal_corners = nullptr; uint32_t nn = 0;
  const uint32_t *uv_corners = nullptr; uint32_t nu = 0;
  const ExtraAttr *extras = nullptr; uint32_t num_extras = 0;      // written behind the attributes above, in list order
  const Grid *pos_grid = nullptr, *uv_grid = nullptr;              // the caller's quantisation grids (null: the attribute's own bounds)
  const int32_t *uv_portable = nullptr;                            // sequential streams: the integers `uvs` is coded as, in place of the quantiser's output (ExtraAttr::portable)
  const int32_t *normal_portable = nullptr;                        // ... and the octahedral codes (s, t) `normals` is coded as, nv rows of 2
  const int32_t *pos_portable = nullptr;                           // ... and the integers `pos` is coded as, nv rows of 3 (voxel centroids)
};

// Why the extras of a mesh cannot be written ("" when they can): the attribute's index in the list and the field.
static std::string extras_error(const MeshIn &in) {
  const size_t builtins = 1 + (in.normals ? 1 : 0) + (in.uvs ? 1 : 0) + (in.generic ? 1 : 0);
  char buf[160];
  if (in.num_extras && !in.extras) return "attributes: the list is missing";
  if (builtins + in.num_extras > kMaxAttributes) {
    snprintf(buf, sizeof(buf), "attributes: %zu built-in and %u listed attributes exceed the %zu a stream may hold", builtins, in.num_extras, kMaxAttributes);
    return buf;
  }
  auto bad = [&](uint32_t k, const char *field, long long v, const char *legal) {
    snprintf(buf, sizeof(buf), "attribute %u: %s %lld: %s", k, field, v, legal);
    return std::string(buf);
  };
  for (uint32_t k = 0; k < in.num_extras; ++k) {
    const ExtraAttr &x = in.extras[k];
    if (x.att_type != 2 && x.att_type != 3 && x.att_type != 4) return bad(k, "attribute_type", x.att_type, "2 (colour), 3 (texture coordinate) or 4 (generic)");
    if (!((x.data_type >= 1 && x.data_type <= 6) || x.data_type == 9)) return bad(k, "data_type", x.data_type, "1 (int8) to 6 (uint32) or 9 (float32)");
    if (x.nc < 1 || x.nc > 4) return bad(k, "num_components", x.nc, "1 to 4");
    if (x.normalized != 0 && x.normalized != 1) return bad(k, "normalized", x.normalized, "0 or 1");
    if (x.data_type == 9 && (x.bits < 0 || x.bits > 20)) return bad(k, "quantization_bits", x.bits, "1 to 20, or 0 for the default");
    if (!x.values) { snprintf(buf, sizeof(buf), "attribute %u: values is NULL", k); return buf; }
    const uint32_t uid = x.unique_id == kInvalid ? (uint32_t)(builtins + k) : x.unique_id;
    for (uint32_t j = 0; j < builtins + k; ++j) {
      const uint32_t other = j < builtins ? j : (in.extras[j - builtins].unique_id == kInvalid ? j : in.extras[j - builtins].unique_id);
      if (other == uid) { snprintf(buf, sizeof(buf), "attribute %u: unique_id %u is the id of attribute %u of the stream", k, uid, j); return buf; }
    }
    if (x.corners && builtins + k > kMaxCornerAttributeIndex) {
      snprintf(buf, sizeof(buf), "attribute %u: corner ids on attribute %zu of the stream: corner attributes are decoded for attributes 1 to %zu", k, builtins + k, kMaxCornerAttributeIndex);
      return buf;
    }
  }
  return "";
}
static inline bool extras_have_corners(const MeshIn &in) {
  for (uint32_t k = 0; k < in.num_extras && in.extras; ++k) if (in.extras[k].corners) return true;
  return false;
}
// An id of a listed attribute at or above its row count refuses the mesh ("" when every id names a row).
static std::string extras_id_error(const MeshIn &in) {
  for (uint32_t k = 0; k < in.num_extras && in.extras; ++k) {
    const ExtraAttr &x = in.extras[k];
    if (!x.corners) continue;
    for (size_t c = 0; c < (size_t)in.nf * 3; ++c)
      if (x.corners[c] >= x.rows) return "attribute " + std::to_string(k) + " id out of range";
  }
  return "";
}
// The descriptors of the extras, behind the built-in ones.  `prediction`: what the generic attribute gets on this path.
static void plan_extra_attributes(const MeshIn &in, const Options &opt, int prediction, std::vector<PortableAttr> &atts);
// Portable values of an extra: integers as they are, floats quantised (AttributeQuantizationTransform).
static void fill_extra_values(const PortableAttr &a, uint32_t nv, PortableAttr &out);

// One attribute's value section: method, transform, compressed flag, symbols, prediction data
// (SequentialIntegerAttributeEncoder.cs:55-128)
// Area-weighted normal of the faces around a corner's vertex from the quantised positions, canonicalised to the
// octahedron (MeshPredictionSchemeGeometricNormalPredictorArea.cs:16-63 + OctahedronToolBox.cs:121-137, with the
// bitstream's 64-bit arithmetic).  Per-vertex attributes only: a data id's position is its vertex's.
template <class CT>
static void geometric_normal_prediction(const Octa &o, const CT &ct, const CornerTable &pos_ct, const std::vector<int32_t> &pos, uint32_t ci, int32_t v3[3]) {
  auto P = [&](uint32_t c, int k) { return (int64_t)pos[(size_t)pos_ct.row_of(pos_ct.vertex(c)) * 3 + k]; };
  uint64_t n[3] = {0, 0, 0};
  uint32_t c = ci;
  bool left = true;
  while (c != kInvalid) {
    uint32_t cn = CornerTable::next(c), cp = CornerTable::prev(c);
    uint64_t a[3], b[3];
    for (int k = 0; k < 3; ++k) { a[k] = (uint64_t)(P(cn, k) - P(ci, k)); b[k] = (uint64_t)(P(cp, k) - P(ci, k)); }
    n[0] += a[1] * b[2] - a[2] * b[1];
    n[1] += a[2] * b[0] - a[0] * b[2];
    n[2] += a[0] * b[1] - a[1] * b[0];
    if (left) {
      c = ct.swing_left(c);
      if (c == kInvalid) { c = ct.swing_right(ci); left = false; }
      else if (c == ci) break;
    } else c = ct.swing_right(c);
  }
  int64_t nv[3] = {(int64_t)n[0], (int64_t)n[1], (int64_t)n[2]};
  uint64_t as = 0;
  bool sat = false;
  for (int k = 0; k < 3; ++k) {
    uint64_t x = nv[k] < 0 ? (uint64_t)0 - (uint64_t)nv[k] : (uint64_t)nv[k];
    if (x > (uint64_t)INT64_MAX || as > (uint64_t)INT64_MAX - x) sat = true; else as += x;
  }
  int64_t abs_sum = sat ? INT64_MAX : (int64_t)as;
  const int64_t upper = (int64_t)1 << 29;
  if (abs_sum > upper) { int64_t q = abs_sum / upper; for (int k = 0; k < 3; ++k) nv[k] /= q; }
  for (int k = 0; k < 3; ++k) v3[k] = (int32_t)nv[k];
  int64_t s3 = std::llabs((int64_t)v3[0]) + std::llabs((int64_t)v3[1]) + std::llabs((int64_t)v3[2]);
  if (s3 == 0) v3[0] = o.center;
  else {
    v3[0] = (int32_t)(((int64_t)v3[0] * o.center) / s3);
    v3[1] = (int32_t)(((int64_t)v3[1] * o.center) / s3);
    int32_t rest = o.center - std::abs(v3[0]) - std::abs(v3[1]);
    v3[2] = v3[2] >= 0 ? rest : -rest;
  }
}

// PredictionSchemeNormalOctahedronEncodingTransform.cs (the non-canonicalised transform: no rotation step)
static void oct_plain_corr(const Octa &o, const int32_t orig_in[2], const int32_t pred_in[2], int32_t out[2]) {
  int os = orig_in[0] - o.center, ot = orig_in[1] - o.center;
  int ps = pred_in[0] - o.center, pt = pred_in[1] - o.center;
  if (!o.in_diamond(ps, pt)) { o.invert_diamond(os, ot); o.invert_diamond(ps, pt); }
  out[0] = o.make_positive(os - ps);
  out[1] = o.make_positive(ot - pt);
}

template <class CT>
static void write_attribute_values(ByteWriter &w, const PortableAttr &a, const CT &ct, const CornerTable &pos_ct, const Sequence &seq, const Options &opt,
                                   const PortableAttr *positions = nullptr) {
  int nc = a.nc;
  size_t entries = seq.data_to_corner.size();
  // compressed flag + symbols: through the entropy coder, or as they are at 1 / 2 / 4 bytes each
  auto put_symbols = [&](const std::vector<uint32_t> &sy) {
    if (opt.raw_integers == 0) { w.u8(1); encode_symbols(w, sy, nc, opt.force_scheme, opt.compression_level); return; }
    const int nb = opt.raw_integers;
    check(nb >= 1 && nb <= 4, "raw_integers must be 1, 2, 3 or 4");
    w.u8(0);
    w.u8((uint8_t)nb);
    for (uint32_t v : sy) {
      check(nb == 4 || v < (1u << (8 * nb)), "value does not fit the raw integer width");
      for (int k = 0; k < nb; ++k) w.u8((uint8_t)(v >> (8 * k)));
    }
  };
  // values in entry order
  std::vector<int32_t> d(entries * nc);
  for (size_t e = 0; e < entries; ++e) {
    const uint32_t corner = seq.data_to_corner[e];
    const uint32_t v = a.corner_value ? a.corner_value[corner] : pos_ct.row_of(pos_ct.vertex(corner));
    for (int c = 0; c < nc; ++c) d[e * nc + c] = a.vals[(size_t)v * nc + c];
  }
  std::vector<uint32_t> symbols(entries * nc);
  {
    const int none_bit = a.seq_type == 3 ? 4 : (a.att_type == 0 ? 1 : (a.att_type == 3 ? 2 : (a.att_type == 4 ? 8 : 0)));
    if (opt.no_prediction & none_bit) {        // PredictionSchemeMethod.None (-2): no transform byte, the values themselves, signed
      w.i8(-2);
      for (size_t i = 0; i < symbols.size(); ++i) symbols[i] = zigzag(d[i]);
      put_symbols(symbols);
      return;
    }
  }
  if (a.seq_type == 3 && a.prediction == 6) {
    // MeshPredictionSchemeGeometricNormalEncoder.cs:47-108: the prediction or its negation, whichever leaves the
    // smaller correction; one flip bit per entry behind the transform data
    check(positions != nullptr && positions->nc == 3, "geometric normal prediction needs quantised positions");
    w.i8(6);
    w.i8(3);
    Octa o(a.bits);
    std::vector<uint8_t> flips(entries);
    auto mod_max = [&](int x) { return x > o.center ? x - o.max_q : (x < -o.center ? x + o.max_q : x); };
    for (size_t e = 0; e < entries; ++e) {
      int32_t v3[3];
      geometric_normal_prediction(o, ct, pos_ct, positions->vals, seq.data_to_corner[e], v3);
      int32_t pp[2], pn[2], cp[2], cn[2];
      int s, t;
      o.from_int_vector(v3, s, t); pp[0] = s; pp[1] = t;
      int32_t neg[3] = {-v3[0], -v3[1], -v3[2]};
      o.from_int_vector(neg, s, t); pn[0] = s; pn[1] = t;
      oct_canon_corr(o, &d[e * 2], pp, cp);
      oct_canon_corr(o, &d[e * 2], pn, cn);
      int wp = std::abs(mod_max(cp[0])) + std::abs(mod_max(cp[1]));
      int wn = std::abs(mod_max(cn[0])) + std::abs(mod_max(cn[1]));
      const bool flip = !(wp < wn);
      flips[e] = flip;
      symbols[e * 2] = (uint32_t)(flip ? cn[0] : cp[0]); symbols[e * 2 + 1] = (uint32_t)(flip ? cn[1] : cp[1]);
    }
    w.u8(1);
    encode_symbols(w, symbols, nc, opt.force_scheme, opt.compression_level);
    w.i32(o.max_q);
    w.i32(o.center);
    write_rabs(w, flips);
    return;
  }
  if (a.seq_type == 3) {
    const bool canonical = opt.normal_transform != 2;
    w.i8(0);   // Difference
    w.i8(canonical ? 3 : 2);   // NormalOctahedronCanonicalized / NormalOctahedron
    Octa o(a.bits);
    int32_t zero[2] = {0, 0};
    for (size_t e = entries; e-- > 0;) {
      int32_t out[2];
      if (canonical) oct_canon_corr(o, &d[e * 2], e ? &d[(e - 1) * 2] : zero, out);
      else oct_plain_corr(o, &d[e * 2], e ? &d[(e - 1) * 2] : zero, out);
      symbols[e * 2] = (uint32_t)out[0]; symbols[e * 2 + 1] = (uint32_t)out[1];   // positive: no zig-zag
    }
    put_symbols(symbols);
    w.i32(o.max_q);
    if (canonical) w.i32(o.center);      // PredictionSchemeNormalOctahedronCanonicalizedDecodingTransform reads a centre it does not use
    return;
  }
  if (a.prediction == 5) {
    // MeshPredictionSchemeTexCoordsPortableEncoder.cs + ...PortablePredictor.cs:46-150 (encoder side: both candidate
    // predictions, the closer one wins and its orientation is recorded), last entry first
    check(nc == 2 && positions != nullptr && positions->nc == 3, "texture coordinate prediction needs 2 components and quantised positions");
    WrapEnc wr;
    wr.init(d);
    w.i8(5);
    w.i8(1);
    std::vector<uint8_t> orientations;
    auto isqrt = [](uint64_t number) {   // Core/MathUtilities.cs:5-25
      if (number == 0) return (uint64_t)0;
      uint64_t act = number, root = 1;
      while (act >= 2) { root *= 2; act /= 4; }
      do { root = (root + number / root) / 2; } while (root * root > number);
      return root;
    };
    auto P = [&](int32_t entry, int k) { return (int64_t)positions->vals[(size_t)pos_ct.row_of(pos_ct.vertex(seq.data_to_corner[entry])) * 3 + k]; };
    for (size_t p = entries; p-- > 0;) {
      const int32_t data_id = (int32_t)p;
      const uint32_t ci = seq.data_to_corner[p];
      const int32_t next_id = seq.vertex_to_data[ct.vertex(CornerTable::next(ci))], prev_id = seq.vertex_to_data[ct.vertex(CornerTable::prev(ci))];
      int32_t pred[2] = {0, 0};
      bool done = false;
      if (prev_id >= 0 && next_id >= 0 && prev_id < data_id && next_id < data_id) {
        const int64_t n_uv[2] = {d[next_id * 2], d[next_id * 2 + 1]}, p_uv[2] = {d[prev_id * 2], d[prev_id * 2 + 1]};
        if (p_uv[0] == n_uv[0] && p_uv[1] == n_uv[1]) { pred[0] = (int32_t)p_uv[0]; pred[1] = (int32_t)p_uv[1]; done = true; }
        else {
          int64_t pn[3], cn[3];
          for (int k = 0; k < 3; ++k) { pn[k] = P(prev_id, k) - P(next_id, k); cn[k] = P(data_id, k) - P(next_id, k); }
          const int64_t pn_norm2 = pn[0] * pn[0] + pn[1] * pn[1] + pn[2] * pn[2];
          if (pn_norm2 != 0) {
            const int64_t cn_dot_pn = pn[0] * cn[0] + pn[1] * cn[1] + pn[2] * cn[2];
            const int64_t pn_uv[2] = {p_uv[0] - n_uv[0], p_uv[1] - n_uv[1]};
            const int64_t x_uv[2] = {n_uv[0] * pn_norm2 + cn_dot_pn * pn_uv[0], n_uv[1] * pn_norm2 + cn_dot_pn * pn_uv[1]};
            int64_t cx[3];
            for (int k = 0; k < 3; ++k) cx[k] = P(data_id, k) - (P(next_id, k) + (cn_dot_pn * pn[k]) / pn_norm2);
            const uint64_t cx_norm2 = (uint64_t)(cx[0] * cx[0] + cx[1] * cx[1] + cx[2] * cx[2]);
            const int64_t norm = (int64_t)isqrt(cx_norm2 * (uint64_t)pn_norm2);
            const int64_t cx_uv[2] = {pn_uv[1] * norm, -pn_uv[0] * norm};
            const int64_t c0[2] = {(x_uv[0] + cx_uv[0]) / pn_norm2, (x_uv[1] + cx_uv[1]) / pn_norm2};
            const int64_t c1[2] = {(x_uv[0] - cx_uv[0]) / pn_norm2, (x_uv[1] - cx_uv[1]) / pn_norm2};
            const int64_t u = d[p * 2], v = d[p * 2 + 1];
            const uint64_t e0 = (uint64_t)((u - c0[0]) * (u - c0[0]) + (v - c0[1]) * (v - c0[1]));
            const uint64_t e1 = (uint64_t)((u - c1[0]) * (u - c1[0]) + (v - c1[1]) * (v - c1[1]));
            if (e0 < e1) { pred[0] = (int32_t)c0[0]; pred[1] = (int32_t)c0[1]; orientations.push_back(1); }
            else { pred[0] = (int32_t)c1[0]; pred[1] = (int32_t)c1[1]; orientations.push_back(0); }
            done = true;
          }
        }
      }
      if (!done) {
        int32_t data_offset = 0;
        bool zero = false;
        if (prev_id >= 0 && prev_id < data_id) data_offset = prev_id * 2;
        if (next_id >= 0 && next_id < data_id) data_offset = next_id * 2;
        else { if (data_id > 0) data_offset = (data_id - 1) * 2; else zero = true; }
        if (!zero) { pred[0] = d[data_offset]; pred[1] = d[data_offset + 1]; }
      }
      symbols[p * 2] = zigzag(wr.corr(d[p * 2], pred[0]));
      symbols[p * 2 + 1] = zigzag(wr.corr(d[p * 2 + 1], pred[1]));
    }
    w.u8(1);
    encode_symbols(w, symbols, nc, opt.force_scheme, opt.compression_level);
    // orientations in the order they were found (last entry first), delta-coded against `true`
    w.i32((int32_t)orientations.size());
    std::vector<uint8_t> bits(orientations.size());
    bool last = true;
    for (size_t i = 0; i < orientations.size(); ++i) { const bool o = orientations[i] != 0; bits[i] = o == last; last = o; }
    write_rabs(w, bits);
    w.i32(wr.mn);
    w.i32(wr.mx);
    return;
  }
  WrapEnc wr;
  wr.init(d);
  w.i8((int8_t)a.prediction);
  w.i8(1);     // Wrap
  std::vector<int32_t> pred(nc);
  if (a.prediction == 2 || a.prediction == 4) {
    // MeshPredictionSchemeMultiParallelogramEncoder.cs / ...ConstrainedMultiParallelogramEncoder.cs: averages of the
    // parallelograms around the entry's vertex.  The constrained scheme may drop any of (up to four) parallelograms
    // by a crease flag; this coder takes the subset with the smallest correction (the reference's entropy-driven
    // choice is an encoder heuristic, the stream is valid for any choice).
    auto para = [&](size_t p, uint32_t ci, int32_t *out) {
      const uint32_t oci = ct.opposite(ci);
      if (oci == kInvalid) return false;
      const int32_t vo = seq.vertex_to_data[ct.vertex(oci)], vn = seq.vertex_to_data[ct.vertex(CornerTable::next(oci))], vp = seq.vertex_to_data[ct.vertex(CornerTable::prev(oci))];
      if (!(vo < (int32_t)p && vn < (int32_t)p && vp < (int32_t)p)) return false;
      for (int c = 0; c < nc; ++c) out[c] = (int32_t)((uint32_t)d[vn * nc + c] + (uint32_t)d[vp * nc + c] - (uint32_t)d[vo * nc + c]);
      return true;
    };
    std::vector<uint8_t> crease[4];
    std::vector<int32_t> cand(4 * nc), sum(nc);
    for (int c = 0; c < nc; ++c) symbols[c] = zigzag(wr.corr(d[c], 0));
    for (size_t p = 1; p < entries; ++p) {
      const uint32_t start = seq.data_to_corner[p];
      uint32_t c = start;
      int found = 0;
      bool have = false;
      if (a.prediction == 2) {
        std::fill(sum.begin(), sum.end(), 0);
        while (c != kInvalid) {
          if (para(p, c, cand.data())) { for (int k = 0; k < nc; ++k) sum[k] = (int32_t)((uint32_t)sum[k] + (uint32_t)cand[k]); ++found; }
          c = ct.swing_right(c);
          if (c == start) c = kInvalid;
        }
        if (found) { for (int k = 0; k < nc; ++k) pred[k] = sum[k] / found; have = true; }
      } else {
        bool first_pass = true;
        while (c != kInvalid) {
          if (para(p, c, &cand[(size_t)found * nc])) { if (++found == 4) break; }
          c = first_pass ? ct.swing_left(c) : ct.swing_right(c);
          if (c == start) break;
          if (c == kInvalid && first_pass) { first_pass = false; c = ct.swing_right(start); }
        }
        if (found) {
          int64_t best_cost = -1;
          uint32_t best_mask = 0;
          for (uint32_t mask = 0; mask < (1u << found); ++mask) {      // bit i set: parallelogram i is used
            int used = 0;
            std::fill(sum.begin(), sum.end(), 0);
            for (int i = 0; i < found; ++i) if (mask >> i & 1) { ++used; for (int k = 0; k < nc; ++k) sum[k] = (int32_t)((uint32_t)sum[k] + (uint32_t)cand[(size_t)i * nc + k]); }
            int64_t cost = 0;
            for (int k = 0; k < nc; ++k) cost += std::abs((int64_t)wr.corr(d[p * nc + k], used ? sum[k] / used : d[(p - 1) * nc + k]));
            if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_mask = mask; }
          }
          int used = 0;
          std::fill(sum.begin(), sum.end(), 0);
          for (int i = 0; i < found; ++i) {
            const bool use = best_mask >> i & 1;
            crease[found - 1].push_back(use ? 0 : 1);
            if (use) { ++used; for (int k = 0; k < nc; ++k) sum[k] = (int32_t)((uint32_t)sum[k] + (uint32_t)cand[(size_t)i * nc + k]); }
          }
          if (used) { for (int k = 0; k < nc; ++k) pred[k] = sum[k] / used; have = true; }
        }
      }
      if (!have) for (int k = 0; k < nc; ++k) pred[k] = d[(p - 1) * nc + k];
      for (int k = 0; k < nc; ++k) symbols[p * nc + k] = zigzag(wr.corr(d[p * nc + k], pred[k]));
    }
    w.u8(1);
    encode_symbols(w, symbols, nc, opt.force_scheme, opt.compression_level);
    if (a.prediction == 4)
      for (int i = 0; i < 4; ++i) { w.varint(crease[i].size()); if (!crease[i].empty()) write_rabs(w, crease[i]); }
    w.i32(wr.mn);
    w.i32(wr.mx);
    return;
  }
  for (size_t p = entries; p-- > 0;) {
    bool have = false;
    if (a.prediction == 1 && p > 0) {   // MeshPredictionSchemeParallelogramEncoder.cs:35-56 (E-4 corrected)
      uint32_t ci = seq.data_to_corner[p];
      uint32_t oci = ct.opposite(ci);
      if (oci != kInvalid) {
        int32_t vo = seq.vertex_to_data[ct.vertex(oci)];
        int32_t vn = seq.vertex_to_data[ct.vertex(CornerTable::next(oci))];
        int32_t vp = seq.vertex_to_data[ct.vertex(CornerTable::prev(oci))];
        if (vo < (int32_t)p && vn < (int32_t)p && vp < (int32_t)p) {
          for (int c = 0; c < nc; ++c) pred[c] = d[vn * nc + c] + d[vp * nc + c] - d[vo * nc + c];
          have = true;
        }
      }
    }
    if (!have) for (int c = 0; c < nc; ++c) pred[c] = p > 0 ? d[(p - 1) * nc + c] : 0;
    for (int c = 0; c < nc; ++c) symbols[p * nc + c] = zigzag(wr.corr(d[p * nc + c], pred[c]));
  }
  put_symbols(symbols);
  w.i32(wr.mn);
  w.i32(wr.mx);
}

static void write_attribute_transform(ByteWriter &w, const PortableAttr &a) {
  if (a.seq_type == 2) { for (float f : a.qmin) w.f32(f); w.f32(a.qrange); w.u8((uint8_t)a.bits); }
  else if (a.seq_type == 3) w.u8((uint8_t)a.bits);
}

static void plan_extra_attributes(const MeshIn &in, const Options &opt, int prediction, std::vector<PortableAttr> &atts) {
  const std::string err = extras_error(in);
  check(err.empty(), err.c_str());
  for (uint32_t k = 0; k < in.num_extras; ++k) {
    const ExtraAttr &x = in.extras[k];
    PortableAttr a;
    a.att_type = x.att_type; a.nc = a.nc_out = (int)x.nc; a.data_type = x.data_type; a.prediction = prediction;
    a.unique_id = x.unique_id; a.extra_values = x.values; a.extra_index = (int)k;
    a.corner_value = x.corners; a.extra_rows = x.corners ? x.rows : 0;
    if (x.data_type == 9) a.portable = x.portable;
    if (x.grid) { const std::string why = grid_error(*x.grid, (int)x.nc, x.data_type == 9, grid_slot_name(x.att_type, (int)k)); check(why.empty(), why.c_str()); a.grid = x.grid; }
    if (x.data_type == 9) { a.seq_type = 2; a.bits = x.bits ? x.bits : (x.att_type == 3 ? opt.uv_bits : 8); }
    else { a.seq_type = 1; a.normalized = x.normalized; }
    atts.push_back(a);
  }
}
static void fill_extra_values(const PortableAttr &a, uint32_t nv, PortableAttr &out) {
  if (a.seq_type == 2) {
    const int32_t *portable = a.portable;                      // (a and out may be one object)
    quantize((const float *)a.extra_values, nv, a.nc, a.bits, out);
    if (portable) out.vals.assign(portable, portable + (size_t)nv * a.nc);       // the header is the floats', the integers are given
    return;
  }
  out.vals.resize((size_t)nv * a.nc);
  for (size_t k = 0; k < (size_t)nv * a.nc; ++k) out.vals[k] = generic_value(a.extra_values, k, a.data_type);
}

// Everything about a mesh that does not depend on attribute values: connectivity, traversal order, attribute list.
struct MeshPlan {
  CornerTable ct;
  EbResult eb;
  Sequence seq;                      // depth-first order
  Sequence seq_pd;                   // prediction-degree order (only when an attributes decoder asks for it)
  int traversal_method = 0;
  int force_scheme = -1, compression_level = 5;
  bool valence = false;              // valence Edgebreaker traversal: six context symbol lists
  std::vector<uint32_t> ctx_symbols[6];
  // The same coded elsewhere (the device encoder): per list its symbol count and its bytes as encode_symbols writes them
  bool ctx_given = false;
  uint32_t ctx_count[6] = {0, 0, 0, 0, 0, 0};
  std::vector<uint8_t> ctx_coded[6];
  bool predictive = false;           // predictive Edgebreaker traversal: explicit symbols + prediction bits below
  std::vector<uint8_t> explicit_symbols, predictions;   // encoder order
  // Attributes given per corner: conns[att] is the attribute's own connectivity, seq_att[att] its depth-first order
  // (corner attributes are always sequenced depth first: MeshEdgeBreakerEncoder.cs:556-564); both empty for meshes
  // whose attributes are all per vertex.
  std::vector<AttrConn> conns;
  std::vector<Sequence> seq_att;
  // The same found on the device (dsa_encode_seams.h), where there is no corner table here: per attribute 1 = seamed, and per
  // attribute the seam bits of every interior edge in decoder face order (all zero for an attribute without seams).
  std::vector<uint8_t> seamed_given;
  std::vector<std::vector<uint8_t>> seam_bits_given;
  bool seamed(size_t att) const {
    if (!seamed_given.empty()) return att < seamed_given.size() && seamed_given[att];
    return att < conns.size() && conns[att].ct && !conns[att].no_interior_seams;
  }
  bool uses_pd(size_t att) const { return !seamed(att) && (traversal_method == 2 || (traversal_method == 1 && (single || att == 0))); }
  const Sequence &seq_of(size_t att) const { return seamed(att) ? seq_att[att] : (uses_pd(att) ? seq_pd : seq); }
  std::vector<PortableAttr> atts;    // descriptors; vals / quantisation parameters are filled by whoever codes the values
  bool single = false;
  uint32_t num_att_data = 0;
  int64_t interior_edges = -1;       // >= 0: given (connectivity coded on the device, no corner table here); else counted from ct
  int64_t coded_vertices = -1, coded_faces = -1;      // >= 0: a repaired table's counts for the header (V' - isolated, F - degenerate); else the input's
  // repair_topology = 2 over a mesh that needed repair: per attribute with ids, the ids of the coded faces (the source's
  // non-degenerate faces in source order), which the attribute's corner_value then points at
  std::vector<std::vector<uint32_t>> coded_ids;
  void compact_ids() {
    coded_ids.assign(atts.size(), std::vector<uint32_t>());
    for (size_t k = 1; k < atts.size(); ++k) {
      if (!atts[k].corner_value) continue;
      coded_ids[k].resize(ct.nc());
      for (size_t c = 0; c < ct.cmap.size(); ++c) if (ct.cmap[c] != kInvalid) coded_ids[k][ct.cmap[c]] = atts[k].corner_value[c];
      atts[k].corner_value = coded_ids[k].data();
    }
  }
};
// What of a plan does not depend on the connectivity: attribute descriptors and the options that shape the stream.
static void plan_attributes(const MeshIn &in, const Options &opt, MeshPlan &pl) {
  pl.atts.clear();
  { PortableAttr a; a.att_type = 0; a.nc = a.nc_out = 3; a.seq_type = 2; a.data_type = 9; a.prediction = opt.pos_prediction; a.bits = opt.pos_bits; a.grid = in.pos_grid; pl.atts.push_back(a); }
  if (in.normals) { PortableAttr a; a.att_type = 1; a.nc_out = 3; a.nc = 2; a.seq_type = 3; a.data_type = 9; a.bits = opt.normal_bits; a.prediction = opt.normal_prediction == 6 ? 6 : 0; a.corner_value = in.normal_corners; pl.atts.push_back(a); }
  if (in.uvs) { PortableAttr a; a.att_type = 3; a.nc = a.nc_out = 2; a.seq_type = 2; a.data_type = 9; a.prediction = opt.uv_prediction; a.bits = opt.uv_bits; a.corner_value = in.uv_corners; a.grid = in.uvs ? in.uv_grid : nullptr; pl.atts.push_back(a); }
  // (the generic attribute takes the constrained multi-parallelogram scheme where the positions do: what an encoder at its highest levels writes)
  if (in.generic) { PortableAttr a; a.att_type = 4; a.nc = a.nc_out = opt.generic_components >= 1 && opt.generic_components <= 4 ? opt.generic_components : 1; a.seq_type = 1; a.data_type = opt.generic_data_type; a.prediction = opt.pos_prediction == 4 ? 4 : 1; pl.atts.push_back(a); }
  plan_extra_attributes(in, opt, opt.pos_prediction == 4 ? 4 : 1, pl.atts);
  pl.single = opt.single_connectivity != 0;
  pl.num_att_data = pl.single ? 0 : (uint32_t)pl.atts.size() - 1;
  pl.force_scheme = opt.force_scheme; pl.compression_level = opt.compression_level;
  pl.predictive = opt.predictive_connectivity == 1;
  pl.valence = opt.predictive_connectivity == 2;
  pl.traversal_method = opt.traversal_method;
}
static void plan_mesh(const MeshIn &in, const Options &opt, MeshPlan &pl) {
  if (opt.repair_topology) {
    pl.ct.build_repaired(in.faces, in.nf, in.nv);
    // (seam tables over a repaired table are not written yet: a mesh that needed no repair goes on as it always did)
    check(!(in.normal_corners || in.uv_corners || extras_have_corners(in)) || !pl.ct.needed_repair || opt.repair_topology == 2, "attributes given per corner over a mesh whose topology needs repair are not implemented");
    if (!pl.ct.needed_repair) pl.ct.row.clear();
    else { pl.coded_vertices = pl.ct.nv(); pl.coded_faces = pl.ct.nf(); }
  } else {
    pl.ct.build(in.faces, in.nf, in.nv);
    for (uint32_t v = 0; v < in.nv; ++v) check(pl.ct.vcorner[v] != kInvalid, "isolated vertex in input mesh");
  }
  const uint32_t coded_vertices = pl.ct.nv();                  // (repair mode: V' - isolated)
  EbEncoder enc(pl.ct, pl.eb);
  enc.run();
  dfs_sequence(pl.ct, pl.eb.processed_corners, pl.seq);
  check(pl.seq.data_to_corner.size() == coded_vertices, "traversal did not reach every vertex");
  plan_attributes(in, opt, pl);
  if (opt.repair_topology == 2 && pl.ct.needed_repair) pl.compact_ids();      // (value 1 has refused above)
  if (pl.valence) valence_context_symbols(pl.ct, pl.eb, pl.ctx_symbols);
  if (pl.predictive) predictive_symbols(pl.ct, pl.eb, pl.explicit_symbols, pl.predictions);
  if (pl.traversal_method != 0) {
    prediction_degree_sequence(pl.ct, pl.eb.processed_corners, pl.seq_pd);
    check(pl.seq_pd.data_to_corner.size() == coded_vertices, "traversal did not reach every vertex");
  }
  // attributes given per corner: their seams, their own vertices and traversal order (MeshEdgeBreakerEncoder.cs:403-414,
  // :545-566: the sequencer of a seamed attribute walks the attribute's corner table in the connectivity's face order)
  bool per_corner = false;
  for (auto &a : pl.atts) per_corner = per_corner || a.corner_value != nullptr;
  if (per_corner) {
    check(!pl.single, "attributes given per corner need a connectivity of their own (single_connectivity = 0)");
    pl.conns.assign(pl.atts.size(), AttrConn());
    pl.seq_att.assign(pl.atts.size(), Sequence());
    for (size_t i = 1; i < pl.atts.size(); ++i) {
      if (!pl.atts[i].corner_value) continue;
      pl.conns[i].build(pl.ct, pl.atts[i].corner_value);
      if (pl.conns[i].no_interior_seams) continue;
      dfs_sequence(pl.conns[i], pl.eb.processed_corners, pl.seq_att[i]);
      check(pl.seq_att[i].data_to_corner.size() == pl.conns[i].nv(), "attribute traversal did not reach every attribute vertex");
    }
  }
}

// Header, connectivity sections and the head of the attribute section; then values and transform parameters of
// every attribute through the two callbacks, in the order the decoder expects (ConnectivityEncoder.cs:39-56).
template <class ValuesWriter, class TransformWriter>
static void write_stream(ByteWriter &w, const MeshIn &in, const MeshPlan &pl, ValuesWriter &&values, TransformWriter &&transform) {
  const CornerTable &ct = pl.ct;
  const EbResult &eb = pl.eb;
  w.d.insert(w.d.end(), {'D', 'R', 'A', 'C', 'O'});
  w.u8(2); w.u8(2); w.u8(1); w.u8(1); w.u16(0);
  w.u8(pl.valence ? 2 : (pl.predictive ? 1 : 0));   // Edgebreaker traversal: standard (DracoEncoder.cs:90), predictive or valence
  // (a repaired table: the vertices and faces it codes, V' - isolated and F - degenerate; MeshEdgeBreakerEncoder.cs:46-47)
  w.varint(pl.coded_vertices >= 0 ? (uint64_t)pl.coded_vertices : in.nv);
  w.varint(pl.coded_faces >= 0 ? (uint64_t)pl.coded_faces : in.nf);
  w.u8((uint8_t)pl.num_att_data);
  w.varint(eb.symbols.size());
  w.varint(eb.num_split_symbols);
  // split events, MeshEdgeBreakerEncoder.cs:126-148
  w.varint(eb.splits.size());
  if (!eb.splits.empty()) {
    uint32_t last = 0;
    for (auto &s : eb.splits) { w.varint(s.source - last); w.varint(s.source - s.split); last = s.source; }
    BitWriter bw;
    for (auto &s : eb.splits) bw.put(1, s.edge);
    w.bytes(bw.d);
  }
  // traversal buffer: symbols last-first (size = bytes, E-8), start faces, seams
  {
    BitWriter bw;
    static const int len[8] = {1, 3, 0, 3, 0, 3, 0, 3};
    const std::vector<uint8_t> &syms = pl.predictive ? pl.explicit_symbols : eb.symbols;
    if (!pl.valence) {
      for (size_t i = syms.size(); i-- > 0;) bw.put(len[syms[i]], syms[i]);
      w.varint(bw.d.size());
      w.bytes(bw.d);
    }
    write_rabs(w, eb.start_face_bits);
    bool any_seams = false;
    for (size_t i = 1; i < pl.atts.size(); ++i) any_seams = any_seams || pl.seamed(i);
    if (pl.num_att_data && any_seams && !pl.seam_bits_given.empty()) {
      for (uint32_t i = 0; i < pl.num_att_data; ++i) write_rabs(w, pl.seam_bits_given[i + 1]);
    } else if (pl.num_att_data && any_seams) {
      // MeshEdgeBreakerEncoder.cs:418-440: in decoder face order, for every interior edge whose other face comes later,
      // one bit per attribute -- is the edge a seam of that attribute; a block per attribute (MeshEdgeBreakerTraversalEncoder.cs:62-70)
      std::vector<uint8_t> vis(ct.nf(), 0);
      std::vector<std::vector<uint8_t>> bits(pl.num_att_data);
      for (uint32_t c : eb.processed_corners) {
        const uint32_t corners[3] = {c, CornerTable::next(c), CornerTable::prev(c)};
        vis[c / 3] = 1;
        for (int k = 0; k < 3; ++k) {
          const uint32_t o = ct.opposite(corners[k]);
          if (o == kInvalid || vis[o / 3]) continue;
          for (uint32_t i = 0; i < pl.num_att_data; ++i) bits[i].push_back(pl.seamed(i + 1) ? pl.conns[i + 1].edge_seam[corners[k]] : 0);
        }
      }
      for (uint32_t i = 0; i < pl.num_att_data; ++i) write_rabs(w, bits[i]);
    } else if (pl.num_att_data) {
      // per-vertex attributes: no interior seams, one 0 bit per interior edge in decoder face order
      std::vector<uint8_t> vis(pl.interior_edges >= 0 ? 0 : ct.nf(), 0), bits;
      if (pl.interior_edges >= 0) bits.assign((size_t)pl.interior_edges, 0);
      else for (uint32_t c : eb.processed_corners) {
        uint32_t corners[3] = {c, CornerTable::next(c), CornerTable::prev(c)};
        vis[c / 3] = 1;
        for (int k = 0; k < 3; ++k) {
          uint32_t o = ct.opposite(corners[k]);
          if (o == kInvalid || vis[o / 3]) continue;
          bits.push_back(0);
        }
      }
      ByteWriter once;                       // the same block for every attribute: coded once
      write_rabs(once, bits);
      for (uint32_t i = 0; i < pl.num_att_data; ++i) w.bytes(once.d);
    }
    if (pl.valence)        // MeshEdgeBreakerTraversalValenceDecoder.cs:43-68: the six context lists, each through the symbol coder
      for (int i = 0; i < 6; ++i) {
        if (pl.ctx_given) { w.varint(pl.ctx_count[i]); w.bytes(pl.ctx_coded[i]); continue; }
        w.varint(pl.ctx_symbols[i].size());
        if (!pl.ctx_symbols[i].empty()) encode_symbols(w, pl.ctx_symbols[i], 1, pl.force_scheme, pl.compression_level);
      }
    if (pl.predictive) {   // MeshEdgeBreakerTraversalPredictiveDecoder.cs:19-27: split symbol count, then the prediction bits in decoder order
      w.i32((int32_t)eb.num_split_symbols);
      std::vector<uint8_t> bits(pl.predictions.rbegin(), pl.predictions.rend());
      write_rabs(w, bits);
    }
  }
  // attribute section (ConnectivityEncoder.cs:39-56)
  const std::vector<PortableAttr> &atts = pl.atts;
  uint32_t num_encoders = pl.single ? 1 : (uint32_t)atts.size();
  w.u8((uint8_t)num_encoders);
  // attribute data id, element type (1: corner attribute -- the attribute's own connectivity is used, :442-466), MeshTraversalMethod
  for (uint32_t i = 0; i < num_encoders; ++i) { w.i8(i == 0 ? -1 : (int8_t)(i - 1)); w.u8(pl.seamed(i) ? 1 : 0); w.u8(pl.uses_pd(i) ? 1 : 0); }
  auto write_desc = [&](const PortableAttr &a, uint32_t index) { w.u8((uint8_t)a.att_type); w.u8((uint8_t)a.data_type); w.u8((uint8_t)a.nc_out); w.u8((uint8_t)a.normalized); w.varint(a.unique_id == kInvalid ? index : a.unique_id); };
  if (pl.single) {
    w.varint(atts.size());
    for (size_t i = 0; i < atts.size(); ++i) write_desc(atts[i], (uint32_t)i);
    for (auto &a : atts) w.u8((uint8_t)a.seq_type);
    for (size_t i = 0; i < atts.size(); ++i) values(w, i);
    for (size_t i = 0; i < atts.size(); ++i) transform(w, i);
  } else {
    for (size_t i = 0; i < atts.size(); ++i) { w.varint(1); write_desc(atts[i], (uint32_t)i); w.u8((uint8_t)atts[i].seq_type); }
    for (size_t i = 0; i < atts.size(); ++i) { values(w, i); transform(w, i); }
  }
}

// The CPU coder: quantisation, prediction, entropy coding all on the host.
static void encode_mesh(const MeshIn &in, const Options &opt, std::vector<uint8_t> &out) {
  MeshPlan pl;
  plan_mesh(in, opt, pl);
  for (auto &a : pl.atts) {
    if (a.extra_values) fill_extra_values(a, a.corner_value ? a.extra_rows : in.nv, a);
    else if (a.att_type == 0) quantize(in.pos, in.nv, 3, opt.pos_bits, a);
    else if (a.att_type == 1) {
      const uint32_t n = in.normal_corners ? in.nn : in.nv;
      Octa o(opt.normal_bits);
      a.vals.resize((size_t)n * 2);
      for (uint32_t v = 0; v < n; ++v) { int s, t; o.from_float_vector(in.normals + (size_t)v * 3, s, t); a.vals[(size_t)v * 2] = s; a.vals[(size_t)v * 2 + 1] = t; }
    } else if (a.att_type == 3) quantize(in.uvs, in.uv_corners ? in.nu : in.nv, 2, opt.uv_bits, a);
    else { a.vals.resize((size_t)in.nv * a.nc); for (size_t k = 0; k < (size_t)in.nv * a.nc; ++k) a.vals[k] = generic_value(in.generic, k, a.data_type); }
  }
  ByteWriter w;
  write_stream(w, in, pl,
               [&](ByteWriter &bw, size_t i) {
                 if (pl.seamed(i)) write_attribute_values(bw, pl.atts[i], pl.conns[i], pl.ct, pl.seq_of(i), opt, &pl.atts[0]);
                 else write_attribute_values(bw, pl.atts[i], pl.ct, pl.ct, pl.seq_of(i), opt, &pl.atts[0]);
               },
               [&](ByteWriter &bw, size_t i) { write_attribute_transform(bw, pl.atts[i]); });
  out.swap(w.d);
}
// Entry rows (dsa_encoded_entry_rows; track_rows of dsa_encode_rows_batch): per attribute of the stream, in stream order, the row
// of the value array passed for it whose bytes entry e of the stream carries -- the loop by which write_attribute_values fills
// its values in entry order, with the row kept instead of the value.  A vertex the repair made reads its root parent's row
// (CornerTable::row_of); isolated vertices and degenerate faces have no entries.  What the device's k_enc_entry_rows is held to.
static void plan_entry_rows(const MeshPlan &pl, std::vector<std::vector<uint32_t>> &rows) {
  rows.assign(pl.atts.size(), std::vector<uint32_t>());
  for (size_t k = 0; k < pl.atts.size(); ++k) {
    const PortableAttr &a = pl.atts[k];
    const Sequence &seq = pl.seq_of(k);
    rows[k].resize(seq.data_to_corner.size());
    for (size_t e = 0; e < rows[k].size(); ++e) {
      const uint32_t corner = seq.data_to_corner[e];
      rows[k][e] = a.corner_value ? a.corner_value[corner] : pl.ct.row_of(pl.ct.vertex(corner));
    }
  }
}
static void entry_rows(const MeshIn &in, const Options &opt, std::vector<std::vector<uint32_t>> &rows) {
  MeshPlan pl;
  plan_mesh(in, opt, pl);
  plan_entry_rows(pl, rows);
}

// ------------------------------------------------------------------ the weld of per-point input
// A mesh given as one row per point (a glTF primitive, an OBJ after triangulation, Batch.vertex_arrays): a point is duplicated
// wherever a UV chart or a hard edge passes.  The weld finds the vertices under the points and hands the mesh on in the form
// encode_mesh takes: positions (and everything else that stays per vertex) per vertex, normals and texture coordinates as rows
// with ids per corner.  This is the specification the kernels of dsa_encode_weld.h are held against:
//   - a point is used when a face names it; unused points take no part and get kInvalid in every map;
//   - two used points are one vertex when the rows of every segment of `vertex_key` (positions, the generic attribute, every
//     listed attribute) are equal byte for byte (-0.0 is not +0.0, a NaN equals the NaN of the same bits);
//   - the representative of a class is its point of smallest index, classes are numbered by ascending representative;
//   - normals (12-byte rows) and texture coordinates (8-byte rows) likewise, each alone;
//   - an attribute whose row id is the same for all points of every vertex is handed on per vertex: the row of each vertex's
//     representative, no ids (what lets a table that needs repair keep its normals: seams over a repaired table are not written);
//   - weld_attributes: every listed attribute that may have a connectivity of its own in the stream (its index there is at most
//     kMaxCornerAttributeIndex: weld_listed_alone) leaves the vertex key and is a key set of its own, welded like normals and texture
//     coordinates (`listed`, in list order).  The vertex key is then positions + the generic attribute + the listed attributes
//     behind that index.  A lightmap UV set or a colour with a hard edge then cuts its own connectivity only.
struct WeldSeg { const void *rows; uint32_t row_bytes; };
struct WeldKeys {                      // one key set: the classes of the used points under its segments
  uint32_t count = 0;
  std::vector<uint32_t> of_point, point;      // class of every point (kInvalid: unused); representative of every class
};
struct Welded {
  uint32_t P = 0, F = 0;
  WeldKeys vertex, normal, texcoord;   // (normal / texcoord: count 0 and empty maps when the mesh has none)
  bool normals_per_vertex = true, texcoords_per_vertex = true;
  std::vector<uint32_t> faces, normal_corners, texcoord_corners;      // 3F each; the id lists empty when per vertex
  std::vector<std::vector<uint8_t>> vertex_rows;                       // per segment of the vertex key: V rows
  std::vector<uint8_t> normal_rows, texcoord_rows;                     // V rows when per vertex, else N / T rows
  // weld_attributes: per listed attribute welded alone, in list order
  struct Listed { WeldKeys keys; bool per_vertex = true; std::vector<uint32_t> corners; std::vector<uint8_t> rows; };
  std::vector<Listed> listed;
  // key set k >= 1 (1 the normal, 2 the texture coordinate, 3 + j listed attribute j, which `listed` must hold by then)
  struct KeySet { WeldKeys &keys; bool &per_vertex; std::vector<uint32_t> &corners; std::vector<uint8_t> &rows; };
  KeySet key_set(uint32_t k) {
    if (k == 1) return {normal, normals_per_vertex, normal_corners, normal_rows};
    if (k == 2) return {texcoord, texcoords_per_vertex, texcoord_corners, texcoord_rows};
    Listed &l = listed[k - 3u];
    return {l.keys, l.per_vertex, l.corners, l.rows};
  }
};
static inline uint32_t weld_hash(const std::vector<WeldSeg> &segs, uint32_t p) {
  uint32_t h = 0x9E3779B9u;
  for (const WeldSeg &s : segs) {
    const uint8_t *r = (const uint8_t *)s.rows + (size_t)p * s.row_bytes;
    for (uint32_t k = 0; k < s.row_bytes; ++k) { h ^= r[k]; h *= 0x01000193u; }
  }
  return h ^ (h >> 15);
}
static inline bool weld_equal(const std::vector<WeldSeg> &segs, uint32_t p, uint32_t q) {
  for (const WeldSeg &s : segs)
    if (memcmp((const uint8_t *)s.rows + (size_t)p * s.row_bytes, (const uint8_t *)s.rows + (size_t)q * s.row_bytes, s.row_bytes) != 0) return false;
  return true;
}
static void weld_classes(const std::vector<WeldSeg> &segs, const std::vector<uint8_t> &used, WeldKeys &out) {
  const uint32_t P = (uint32_t)used.size();
  uint32_t cap = 16;
  while (cap < 2ull * P) cap <<= 1;
  std::vector<uint32_t> table(cap, kInvalid);
  out.count = 0;
  out.of_point.assign(P, kInvalid);
  out.point.clear();
  for (uint32_t p = 0; p < P; ++p) {            // ascending: the point that opens a class is its representative
    if (!used[p]) continue;
    uint32_t s = weld_hash(segs, p) & (cap - 1);
    while (table[s] != kInvalid && !weld_equal(segs, table[s], p)) s = (s + 1) & (cap - 1);
    if (table[s] == kInvalid) { table[s] = p; out.of_point[p] = out.count++; out.point.push_back(p); }
    else out.of_point[p] = out.of_point[table[s]];
  }
}
static void weld_gather(const WeldSeg &s, const std::vector<uint32_t> &points, std::vector<uint8_t> &rows) {
  rows.resize((size_t)points.size() * s.row_bytes);
  for (size_t v = 0; v < points.size(); ++v) memcpy(rows.data() + v * s.row_bytes, (const uint8_t *)s.rows + (size_t)points[v] * s.row_bytes, s.row_bytes);
}
static void weld_points(uint32_t P, const uint32_t *faces, uint32_t F, const std::vector<WeldSeg> &vertex_key, const float *normals, const float *uvs, Welded &out,
                        const std::vector<WeldSeg> &listed = std::vector<WeldSeg>()) {
  check(F == 0 || faces != nullptr, "mesh needs positions and faces");
  for (const WeldSeg &s : vertex_key) check(P == 0 || s.rows != nullptr, "mesh needs positions and faces");
  for (const WeldSeg &s : listed) check(P == 0 || s.rows != nullptr, "mesh needs positions and faces");
  for (size_t k = 0; k < (size_t)F * 3; ++k) check(faces[k] < P, "face index out of range");      // (before anything indexes through the faces)
  out.P = P; out.F = F;
  std::vector<uint8_t> used(P, 0);
  for (size_t k = 0; k < (size_t)F * 3; ++k) used[faces[k]] = 1;
  weld_classes(vertex_key, used, out.vertex);
  out.faces.resize((size_t)F * 3);
  for (size_t k = 0; k < (size_t)F * 3; ++k) out.faces[k] = out.vertex.of_point[faces[k]];
  out.vertex_rows.resize(vertex_key.size());
  for (size_t g = 0; g < vertex_key.size(); ++g) weld_gather(vertex_key[g], out.vertex.point, out.vertex_rows[g]);
  out.listed.assign(listed.size(), Welded::Listed());
  for (uint32_t k = 1; k < 3 + listed.size(); ++k) {
    const WeldSeg seg = k == 1 ? WeldSeg{normals, 12u} : (k == 2 ? WeldSeg{uvs, 8u} : listed[k - 3u]);
    const Welded::KeySet a = out.key_set(k);
    a.keys = WeldKeys(); a.per_vertex = true; a.corners.clear(); a.rows.clear();
    if (!seg.rows) continue;
    weld_classes({seg}, used, a.keys);
    for (uint32_t p = 0; p < P; ++p)
      if (used[p] && a.keys.of_point[p] != a.keys.of_point[out.vertex.point[out.vertex.of_point[p]]]) { a.per_vertex = false; break; }
    if (a.per_vertex) { weld_gather(seg, out.vertex.point, a.rows); continue; }
    weld_gather(seg, a.keys.point, a.rows);
    a.corners.resize((size_t)F * 3);
    for (size_t c = 0; c < (size_t)F * 3; ++c) a.corners[c] = a.keys.of_point[faces[c]];
  }
}
// The welded mesh as the coder takes it: `in` is the per-point input (its corner ids unset, nv read as P), `key` the segments of
// its vertex key in the order positions, generic, extras (weld_vertex_key); `ex` receives the extras pointed at their welded rows.
// weld_attributes: is attribute k of the list welded alone (its index in the stream is one a corner attribute may have)
static inline bool weld_listed_alone(const MeshIn &in, uint32_t k) {
  return 1 + (in.normals ? 1 : 0) + (in.uvs ? 1 : 0) + (in.generic ? 1 : 0) + (size_t)k <= kMaxCornerAttributeIndex;
}
static std::vector<WeldSeg> weld_vertex_key(const MeshIn &in, size_t generic_row_bytes, bool weld_attributes = false, std::vector<WeldSeg> *listed = nullptr) {
  std::vector<WeldSeg> key;
  key.push_back({in.pos, 12u});
  if (in.generic) key.push_back({in.generic, (uint32_t)generic_row_bytes});
  if (listed) listed->clear();
  for (uint32_t k = 0; k < in.num_extras; ++k) {
    const WeldSeg seg{in.extras[k].values, (uint32_t)(data_type_size(in.extras[k].data_type) * in.extras[k].nc)};
    if (weld_attributes && listed && weld_listed_alone(in, k)) listed->push_back(seg);
    else key.push_back(seg);
  }
  return key;
}
static MeshIn welded_mesh_in(const MeshIn &in, const Welded &w, std::vector<ExtraAttr> &ex) {
  MeshIn m = in;
  size_t g = 0;
  m.pos = (const float *)w.vertex_rows[g++].data(); m.nv = w.vertex.count;
  m.faces = w.faces.data(); m.nf = w.F;
  if (in.generic) m.generic = w.vertex_rows[g++].data();
  ex.assign(in.extras, in.extras + in.num_extras);
  // (the listed attributes welded alone are the first w.listed.size() of the list: weld_listed_alone is monotone in k)
  for (uint32_t k = 0; k < in.num_extras; ++k) {
    if (k >= w.listed.size()) { ex[k].values = w.vertex_rows[g++].data(); continue; }
    const Welded::Listed &l = w.listed[k];
    ex[k].values = l.rows.data();
    ex[k].corners = l.per_vertex ? nullptr : l.corners.data(); ex[k].rows = l.per_vertex ? 0 : l.keys.count;
  }
  m.extras = ex.data();
  m.normals = in.normals ? (const float *)w.normal_rows.data() : nullptr;
  m.normal_corners = w.normals_per_vertex ? nullptr : w.normal_corners.data(); m.nn = w.normals_per_vertex ? 0 : w.normal.count;
  m.uvs = in.uvs ? (const float *)w.texcoord_rows.data() : nullptr;
  m.uv_corners = w.texcoords_per_vertex ? nullptr : w.texcoord_corners.data(); m.nu = w.texcoords_per_vertex ? 0 : w.texcoord.count;
  return m;
}
// Entry rows of a welded mesh: row r of the array the coder got for attribute `a` is the row of which point of the caller's --
// the representative of class r of the attribute's own key set where it went on with ids per corner, of vertex r where it went
// on per vertex (positions, the generic attribute, the listed attributes of the vertex key, and every set no vertex has two of).
static const std::vector<uint32_t> &weld_row_points(const Welded &w, const PortableAttr &a) {
  if (a.extra_index >= 0) return (size_t)a.extra_index < w.listed.size() && !w.listed[a.extra_index].per_vertex ? w.listed[a.extra_index].keys.point : w.vertex.point;
  if (a.att_type == 1 && !w.normals_per_vertex) return w.normal.point;
  if (a.att_type == 3 && !w.texcoords_per_vertex) return w.texcoord.point;
  return w.vertex.point;
}
static void welded_entry_rows(const MeshIn &welded, const Welded &w, const Options &opt, std::vector<std::vector<uint32_t>> &rows) {
  MeshPlan pl;
  plan_mesh(welded, opt, pl);
  plan_entry_rows(pl, rows);
  for (size_t k = 0; k < rows.size(); ++k) {
    const std::vector<uint32_t> &point = weld_row_points(w, pl.atts[k]);
    for (uint32_t &r : rows[k]) r = point[r];
  }
}

// ------------------------------------------------------------------ sequential streams
// Sequential mesh (Mesh/MeshSequentialEncoder.cs:9-121 with the bitstream's index widths) and sequential point cloud
// (PointCloud/PointCloudSequentialEncoder.cs): faces as point indices, compressed (differences, sign in the LSB, through the
// symbol coder) or raw; one attributes encoder with a linear sequencer (Attributes/LinearSequencer.cs), so values are in point
// order and predicted by Difference + Wrap / canonicalised octahedral delta.

// Attribute descriptors of a sequential stream: positions, normals, texture coordinates, the generic integer attribute; all Difference.
static void plan_sequential_attributes(const MeshIn &in, const Options &opt, std::vector<PortableAttr> &atts) {
  atts.clear();
  { PortableAttr a; a.att_type = 0; a.nc = a.nc_out = 3; a.seq_type = 2; a.data_type = 9; a.prediction = 0; a.bits = opt.pos_bits; a.grid = in.pos_grid; atts.push_back(a); }
  if (in.normals) { PortableAttr a; a.att_type = 1; a.nc_out = 3; a.nc = 2; a.seq_type = 3; a.data_type = 9; a.bits = opt.normal_bits; a.prediction = 0; atts.push_back(a); }
  if (in.uvs) { PortableAttr a; a.att_type = 3; a.nc = a.nc_out = 2; a.seq_type = 2; a.data_type = 9; a.prediction = 0; a.bits = opt.uv_bits; a.grid = in.uv_grid; atts.push_back(a); }
  if (in.generic) { PortableAttr a; a.att_type = 4; a.nc = a.nc_out = opt.generic_components >= 1 && opt.generic_components <= 4 ? opt.generic_components : 1; a.seq_type = 1; a.data_type = opt.generic_data_type; a.prediction = 0; atts.push_back(a); }
  plan_extra_attributes(in, opt, 0, atts);
}
// Compressed indices: symbol k = |f[k] - f[k-1]| << 1 | sign, f[-1] = 0 (MeshSequentialEncoder.cs:84-121)
static void sequential_index_symbols(const uint32_t *faces, size_t count, std::vector<uint32_t> &sym) {
  sym.resize(count);
  int64_t last = 0;
  for (size_t k = 0; k < count; ++k) {
    const int64_t diff = (int64_t)faces[k] - last;
    sym[k] = ((uint32_t)(diff < 0 ? -diff : diff) << 1) | (diff < 0 ? 1u : 0u);
    last = faces[k];
  }
}
// Raw indices at the bitstream's widths: u8 below 256 points, u16 below 65 536, varint below 2^21, u32 from there
// (MeshSequentialDecoder.cs:30-75); straight from the caller's array to the end of the stream.
static void write_raw_indices(ByteWriter &w, const uint32_t *faces, size_t count, uint32_t nv) {
  const size_t at = w.d.size();
  if (nv < 256) { w.d.resize(at + count); uint8_t *o = w.d.data() + at; for (size_t k = 0; k < count; ++k) o[k] = (uint8_t)faces[k]; }
  else if (nv < (1u << 16)) { w.d.resize(at + 2 * count); uint8_t *o = w.d.data() + at; for (size_t k = 0; k < count; ++k) { o[2 * k] = (uint8_t)faces[k]; o[2 * k + 1] = (uint8_t)(faces[k] >> 8); } }
  else if (nv < (1u << 21)) { w.d.reserve(at + 3 * count); for (size_t k = 0; k < count; ++k) w.varint(faces[k]); }
  else { w.d.resize(at + 4 * count); uint8_t *o = w.d.data() + at; for (size_t k = 0; k < count; ++k) for (int b = 0; b < 4; ++b) o[4 * k + b] = (uint8_t)(faces[k] >> (8 * b)); }
}
// The byte layout of both stream kinds from pieces coded on either side (the CPU coder below, the device encoder of
// dsa_encode_sequential.h): header, (mesh: counts, connectivity method, indices through `indices`), one attributes encoder,
// then every attribute's values and every attribute's transform parameters through the callbacks.
template <class IndexWriter, class ValuesWriter, class TransformWriter>
static void write_sequential_stream(ByteWriter &w, bool mesh, uint32_t nv, uint32_t nf, bool compressed, const std::vector<PortableAttr> &atts,
                                    IndexWriter &&indices, ValuesWriter &&values, TransformWriter &&transform) {
  w.d.insert(w.d.end(), {'D', 'R', 'A', 'C', 'O'});
  w.u8(2); w.u8(2); w.u8(mesh ? 1 : 0); w.u8(0); w.u16(0);
  if (mesh) {
    w.varint(nf);
    w.varint(nv);
    w.u8(compressed ? 0 : 1);
    indices(w);
  } else w.i32((int32_t)nv);
  w.u8(1);
  w.varint(atts.size());
  for (size_t i = 0; i < atts.size(); ++i) { w.u8((uint8_t)atts[i].att_type); w.u8((uint8_t)atts[i].data_type); w.u8((uint8_t)atts[i].nc_out); w.u8((uint8_t)atts[i].normalized); w.varint(atts[i].unique_id == kInvalid ? (uint32_t)i : atts[i].unique_id); }
  for (auto &a : atts) w.u8((uint8_t)a.seq_type);
  for (size_t i = 0; i < atts.size(); ++i) values(w, i);
  for (size_t i = 0; i < atts.size(); ++i) transform(w, i);
}
// The CPU coder of both kinds: `mesh` false writes a point cloud of in.nv points (in.faces is not read).
static void encode_sequential(const MeshIn &in, const Options &opt, bool mesh, bool compressed, std::vector<uint8_t> &out) {
  std::vector<PortableAttr> atts;
  check(!extras_have_corners(in), "a sequential stream has one value per point");
  plan_sequential_attributes(in, opt, atts);
  for (auto &a : atts) {
    if (a.extra_values) fill_extra_values(a, in.nv, a);
    else if (a.att_type == 0) { quantize(in.pos, in.nv, 3, opt.pos_bits, a); if (in.pos_portable) a.vals.assign(in.pos_portable, in.pos_portable + (size_t)in.nv * 3); }
    else if (a.att_type == 1) {
      Octa o(opt.normal_bits);
      a.vals.resize((size_t)in.nv * 2);
      for (uint32_t v = 0; v < in.nv; ++v) { int s, t; o.from_float_vector(in.normals + (size_t)v * 3, s, t); a.vals[(size_t)v * 2] = s; a.vals[(size_t)v * 2 + 1] = t; }
      if (in.normal_portable) a.vals.assign(in.normal_portable, in.normal_portable + (size_t)in.nv * 2);
    } else if (a.att_type == 3) { quantize(in.uvs, in.nv, 2, opt.uv_bits, a); if (in.uv_portable) a.vals.assign(in.uv_portable, in.uv_portable + (size_t)in.nv * 2); }
    else { a.vals.resize((size_t)in.nv * a.nc); for (size_t k = 0; k < (size_t)in.nv * a.nc; ++k) a.vals[k] = generic_value(in.generic, k, a.data_type); }
  }
  // linear order: entry i = point i.  write_attribute_values wants a corner table and a sequence: an identity stand-in
  CornerTable ct;
  ct.c2v.resize(in.nv);
  for (uint32_t v = 0; v < in.nv; ++v) ct.c2v[v] = v;
  Sequence seq;
  seq.data_to_corner.resize(in.nv);
  for (uint32_t v = 0; v < in.nv; ++v) seq.data_to_corner[v] = v;
  ByteWriter w;
  write_sequential_stream(w, mesh, in.nv, in.nf, compressed, atts,
                          [&](ByteWriter &bw) {
                            if (!compressed) { write_raw_indices(bw, in.faces, (size_t)in.nf * 3, in.nv); return; }
                            std::vector<uint32_t> sym;
                            sequential_index_symbols(in.faces, (size_t)in.nf * 3, sym);
                            encode_symbols(bw, sym, 1, opt.force_scheme, opt.compression_level);
                          },
                          [&](ByteWriter &bw, size_t i) { write_attribute_values(bw, atts[i], ct, ct, seq, opt); },
                          [&](ByteWriter &bw, size_t i) { write_attribute_transform(bw, atts[i]); });
  out.swap(w.d);
}
// (the entry points of before the generic attribute joined: positions, normals, texture coordinates)
static void encode_mesh_sequential(const MeshIn &in, const Options &opt, bool compressed, std::vector<uint8_t> &out) {
  MeshIn m = in;
  m.generic = nullptr;
  encode_sequential(m, opt, true, compressed, out);
}
// Morton order of the points of a sequential stream (dsa_encode_ordered_sequential_batch, point_order = 1; the device's kernels
// are dsa_encode_order.h): with q the integers the position stream codes (quantize: own bounds, or `grid` with mode 1) and B = bits,
// key(r) = sum over b < B, c < 3 of ((uint32(q[r][c]) >> b) & 1) << (3 b + 2 - c); perm lists the rows in ascending (key, row).
static inline uint64_t point_order_key(const int32_t *q, int bits) {
  uint64_t key = 0;
  for (int b = 0; b < bits; ++b)
    for (int c = 0; c < 3; ++c) key |= (uint64_t)(((uint32_t)q[c] >> b) & 1u) << (3 * b + 2 - c);
  return key;
}
static void point_order(const float *pos, uint32_t n, int bits, const Grid *grid, std::vector<uint32_t> &perm) {
  check(bits >= 1 && bits <= 20, "quantisation bits out of range (positions/texcoords 1..20, normals 2..20)");
  check(pos != nullptr && n > 0, "positions are missing");
  PortableAttr a;
  a.att_type = 0; a.nc = a.nc_out = 3; a.seq_type = 2; a.grid = grid;
  quantize(pos, n, 3, bits, a);
  std::vector<uint64_t> key(n);
  for (uint32_t r = 0; r < n; ++r) key[r] = point_order_key(a.vals.data() + (size_t)3 * r, bits);
  perm.resize(n);
  for (uint32_t r = 0; r < n; ++r) perm[r] = r;
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
}
// One point per occupied cell of the position grid (dsa_encode_merged_sequential_batch, merge_points = 1; the device's kernels are
// k_enc_merge_* of dsa_encode_order.h): with key and perm as above, entry e of the sorted order is a head iff e == 0 or
// key[perm[e]] != key[perm[e - 1]]; kept lists perm[e] over the heads in sorted order (the sort is stable: with voxel_bits = 0 the smallest row of
// every cell), row_entries[r] is the index in kept of the cell of row r.
static void merge_means(const int32_t *q, uint32_t n, int nc, const std::vector<uint32_t> &row_entries, uint32_t m, std::vector<int32_t> &means);
// dsa_encode_voxel_sequential_batch, voxel_bits = C >= 1: the cell is key >> 3 s, s = bits - C (0: the position cell), and
// voxel_point says which row of a voxel is kept and what its position is coded as -- 0: the voxel's first row in (key, row) order;
// 1 (centroid): that row, its position integers the mean of the voxel's by the rule of merge_means; 2 (nearest): the row with the
// smallest (dist, row), dist = the sum over c of (2 (q[r][c] & (2^s - 1)) - (2^s - 1))^2.  coded (where given): the integers the
// position stream codes for every row, the quantiser's output with the centroids at the kept rows -- what the levels and the part
// boxes read.  A serial pass over the voxels' rows; the device's kernels (the head predicate, k_enc_mean_*, k_enc_voxel_*) share
// nothing with it.
static void merge_points(const float *pos, uint32_t n, int bits, const Grid *grid, std::vector<uint32_t> &kept, std::vector<uint32_t> &row_entries,
                         int voxel_bits = 0, int voxel_point = 0, std::vector<int32_t> *coded = nullptr) {
  check(bits >= 1 && bits <= 20, "quantisation bits out of range (positions/texcoords 1..20, normals 2..20)");
  check(pos != nullptr && n > 0, "positions are missing");
  check(voxel_bits >= 0 && voxel_bits <= bits, "voxel_bits out of range (0, or 1 .. position bits)");
  check(voxel_point >= 0 && voxel_point <= 2 && (voxel_point == 0 || voxel_bits >= 1), "voxel_point: 0 (first), 1 (centroid) or 2 (nearest), the latter two with voxel_bits >= 1");
  const int s = voxel_bits ? bits - voxel_bits : 0;
  PortableAttr a;
  a.att_type = 0; a.nc = a.nc_out = 3; a.seq_type = 2; a.grid = grid;
  quantize(pos, n, 3, bits, a);
  std::vector<uint64_t> key(n);
  for (uint32_t r = 0; r < n; ++r) key[r] = point_order_key(a.vals.data() + (size_t)3 * r, bits);
  std::vector<uint32_t> perm(n);
  for (uint32_t r = 0; r < n; ++r) perm[r] = r;
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
  kept.clear(); row_entries.assign(n, 0);
  for (uint32_t e = 0; e < n; ++e) {
    if (e == 0 || (key[perm[e]] >> (3 * s)) != (key[perm[e - 1]] >> (3 * s))) kept.push_back(perm[e]);
    row_entries[perm[e]] = (uint32_t)kept.size() - 1u;
  }
  const uint32_t m = (uint32_t)kept.size();
  if (voxel_point == 2) {                                      // the row of every voxel with the smallest (dist, row): rows ascending, a strictly smaller dist wins
    const int64_t span = ((int64_t)1 << s) - 1;
    std::vector<uint64_t> best(m, ~0ull);
    for (uint32_t r = 0; r < n; ++r) {
      uint64_t dist = 0;
      for (int c = 0; c < 3; ++c) { const int64_t d = 2 * (int64_t)((uint32_t)a.vals[(size_t)3 * r + c] & (uint32_t)span) - span; dist += (uint64_t)(d * d); }
      const uint32_t j = row_entries[r];
      if (dist < best[j]) { best[j] = dist; kept[j] = r; }
    }
  }
  if (voxel_point == 1) {                                      // the mean of the voxel's position integers at the kept row
    std::vector<int32_t> mean;
    merge_means(a.vals.data(), n, 3, row_entries, m, mean);
    for (uint32_t j = 0; j < m; ++j) for (int c = 0; c < 3; ++c) a.vals[(size_t)3 * kept[j] + c] = mean[(size_t)3 * j + c];
  }
  if (coded) coded->swap(a.vals);
}
// The mean of every cell in an attribute of the kept points (dsa_encode_mean_sequential_batch, a bit of mean_attributes; the device's
// kernels are k_enc_mean_* of dsa_encode_order.h): q[n * nc] the integers the plain call codes for the rows -- the quantiser's output
// or the elements widened to int32 -- row_entries and m as merge_points has them; means[m * nc], entry j component c = floor((2 S +
// cnt) / (2 cnt)) with S the sum of q[r][c] over the cnt rows r of cell j, in 64 bits with floor division: the exact mean, ties
// toward +infinity, a function of the set of rows.
static inline int32_t cell_mean(int64_t sum, uint32_t cnt) {
  const int64_t num = 2 * sum + (int64_t)cnt, den = 2 * (int64_t)cnt;
  int64_t q = num / den;
  if (num % den < 0) --q;
  return (int32_t)q;
}
static void merge_means(const int32_t *q, uint32_t n, int nc, const std::vector<uint32_t> &row_entries, uint32_t m, std::vector<int32_t> &means) {
  check(q != nullptr && n > 0 && nc >= 1 && nc <= 4 && row_entries.size() == n, "merge_means: n rows of 1 - 4 integers and their row entries");
  std::vector<int64_t> sum((size_t)m * nc, 0);
  std::vector<uint32_t> cnt(m, 0);
  for (uint32_t r = 0; r < n; ++r) {
    const uint32_t j = row_entries[r];
    check(j < m, "merge_means: a row entry at or above m");
    ++cnt[j];
    for (int c = 0; c < nc; ++c) sum[(size_t)j * nc + c] += q[(size_t)r * nc + c];
  }
  means.resize((size_t)m * nc);
  for (uint32_t j = 0; j < m; ++j) {
    check(cnt[j] >= 1, "merge_means: a cell without rows");
    for (int c = 0; c < nc; ++c) means[(size_t)j * nc + c] = cell_mean(sum[(size_t)j * nc + c], cnt[j]);
  }
}
// The most frequent value of every cell in an attribute of the kept points (dsa_encode_vote_sequential_batch, a bit of
// vote_attributes; the device's kernels are k_enc_vote_* of dsa_encode_order.h, with which this shares nothing): q, row_entries and m as
// merge_means takes them, nc 1 or 2; votes[m * nc], entry j the tuple (q[r][0], .., q[r][nc - 1]) that the most rows r of cell j
// have, among tuples with equally many rows the lexicographically smallest (signed components, component 0 first).  By a sort of
// every cell's tuples: equal tuples are adjacent, the first longest run of the ascending order wins.
static void merge_votes(const int32_t *q, uint32_t n, int nc, const std::vector<uint32_t> &row_entries, uint32_t m, std::vector<int32_t> &votes) {
  check(q != nullptr && n > 0 && nc >= 1 && nc <= 2 && row_entries.size() == n, "merge_votes: n rows of 1 - 2 integers and their row entries");
  std::vector<std::vector<std::pair<int32_t, int32_t>>> of(m);
  for (uint32_t r = 0; r < n; ++r) {
    check(row_entries[r] < m, "merge_votes: a row entry at or above m");
    of[row_entries[r]].push_back({q[(size_t)r * nc], nc == 2 ? q[(size_t)r * nc + 1] : 0});
  }
  votes.resize((size_t)m * nc);
  for (uint32_t j = 0; j < m; ++j) {
    std::vector<std::pair<int32_t, int32_t>> &t = of[j];
    check(!t.empty(), "merge_votes: a cell without rows");
    std::sort(t.begin(), t.end());
    size_t best = 0, best_len = 0;
    for (size_t a = 0; a < t.size();) {
      size_t b = a;
      while (b < t.size() && t[b] == t[a]) ++b;
      if (b - a > best_len) { best = a; best_len = b - a; }
      a = b;
    }
    votes[(size_t)j * nc] = t[best].first;
    if (nc == 2) votes[(size_t)j * nc + 1] = t[best].second;
  }
}
// The mean normal of every cell of the kept points (dsa_encode_normal_mean_sequential_batch, mean_normals = 1; the device's kernels are
// k_enc_normal_* of dsa_encode_order.h, with which this shares nothing but the quantiser's tail, Octa::from_scaled): q[n * 2] the
// octahedral codes (s, t) the plain call codes for the rows at `bits` normal bits, row_entries and m as merge_points has them;
// codes[m * 2].  With c = center and rdiv(a, b) = floor((2 a + b) / (2 b)), floor division:
//   a row's code gives a = s - c, b = t - c and the integer vector v of L1 norm c it stands for: (c - |a| - |b|, a, b) inside the
//   diamond |a| + |b| <= c, else (c - |a| - |b|, sg(a) (c - |b|), sg(b) (c - |a|)), sg(0) = +1;
//   its unit vector in Q30 is u_k = rdiv(v_k 2^42, isqrt((v . v) 2^24)), isqrt the exact floor square root;
//   U = the sum of u over the cnt rows of the cell, M_k = rdiv(U_k, cnt), A = |M_0| + |M_1| + |M_2|;
//   A = 0 (the normals cancel): the code of (1, 0, 0), as the quantiser codes a zero vector; else the quantiser's tail on
//   i0 = rdiv(M_0 c, A), i1 = rdiv(M_1 c, A) and the sign of M_2.
// All in 64 bits: a function of the set of rows.  A cell of one row keeps its code.
static inline int64_t floor_div(int64_t a, int64_t b) { int64_t q = a / b; if ((a % b != 0) && ((a < 0) != (b < 0))) --q; return q; }
static inline int64_t round_div(int64_t num, int64_t den) { return floor_div(2 * num + den, 2 * den); }
static inline int64_t floor_sqrt(uint64_t x) {       // bit by bit, no floating point
  uint64_t r = 0;
  for (int b = 31; b >= 0; --b) { const uint64_t t = r | (1ull << b); if (t * t <= x) r = t; }
  return (int64_t)r;
}
static void merge_mean_normals(const int32_t *q, uint32_t n, int bits, const std::vector<uint32_t> &row_entries, uint32_t m, std::vector<int32_t> &codes) {
  check(q != nullptr && n > 0 && bits >= 2 && bits <= 20 && row_entries.size() == n, "merge_mean_normals: n rows of octahedral codes at 2 - 20 bits and their row entries");
  const Octa o(bits);
  const int64_t c = o.center;
  std::vector<int64_t> sum((size_t)m * 3, 0);
  std::vector<uint32_t> cnt(m, 0), first(m, 0);
  for (uint32_t r = 0; r < n; ++r) {
    const uint32_t j = row_entries[r];
    check(j < m, "merge_mean_normals: a row entry at or above m");
    const int64_t s = q[(size_t)r * 2], t = q[(size_t)r * 2 + 1];
    check(s >= 0 && s <= o.max_value && t >= 0 && t <= o.max_value, "merge_mean_normals: a code outside 0 .. max_value");
    const int64_t a = s - c, b = t - c, aa = std::llabs(a), ab = std::llabs(b);
    int64_t v[3] = {c - aa - ab, a, b};
    if (aa + ab > c) { v[1] = (a < 0 ? -1 : 1) * (c - ab); v[2] = (b < 0 ? -1 : 1) * (c - aa); }
    const int64_t len = floor_sqrt((uint64_t)(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) << 24);
    for (int k = 0; k < 3; ++k) sum[(size_t)j * 3 + k] += round_div(v[k] * ((int64_t)1 << 42), len);
    if (cnt[j]++ == 0) first[j] = r;
  }
  codes.resize((size_t)m * 2);
  for (uint32_t j = 0; j < m; ++j) {
    check(cnt[j] >= 1, "merge_mean_normals: a cell without rows");
    if (cnt[j] == 1) { codes[(size_t)j * 2] = q[(size_t)first[j] * 2]; codes[(size_t)j * 2 + 1] = q[(size_t)first[j] * 2 + 1]; continue; }
    int64_t M[3], A = 0;
    for (int k = 0; k < 3; ++k) { M[k] = round_div(sum[(size_t)j * 3 + k], cnt[j]); A += std::llabs(M[k]); }
    int s, t;
    if (A == 0) o.from_scaled(o.center, 0, false, s, t);
    else o.from_scaled((int)round_div(M[0] * c, A), (int)round_div(M[1] * c, A), M[2] < 0, s, t);
    codes[(size_t)j * 2] = s; codes[(size_t)j * 2 + 1] = t;
  }
}
// The sorted order of a cloud in parts of at most part_points points (dsa_encode_split_sequential_batch, part_points >= 1): P =
// ceil(n / part_points) parts, part p sorted entries [floor(p n / P), floor((p + 1) n / P)), in 64 bits -- 1 .. part_points points
// each, sizes that differ by at most one.  part_points 0: one part.
static inline uint64_t split_count(uint32_t n, uint32_t part_points) { return part_points ? ((uint64_t)n + part_points - 1u) / part_points : 1u; }
static inline uint32_t split_bound(uint32_t n, uint64_t parts, uint64_t p) { return (uint32_t)(p * (uint64_t)n / parts); }
static void split_parts(uint32_t n, uint32_t part_points, std::vector<std::pair<uint32_t, uint32_t>> &ranges) {
  check(n > 0, "positions are missing");
  const uint64_t parts = split_count(n, part_points);
  ranges.resize((size_t)parts);
  for (uint64_t p = 0; p < parts; ++p) ranges[(size_t)p] = {split_bound(n, parts, p), split_bound(n, parts, p + 1)};
}
// ... and what the device finds per part behind the sort (k_enc_part_bounds of dsa_encode_order.h): perm as point_order gives it,
// and per part and component the minimum and maximum of the integers the position stream codes, qmin / qmax[3 p + c].
static void part_boxes(const float *pos, uint32_t n, int bits, const Grid *grid, uint32_t part_points, std::vector<uint32_t> &perm,
                       std::vector<std::pair<uint32_t, uint32_t>> &ranges, std::vector<int32_t> &qmin, std::vector<int32_t> &qmax) {
  point_order(pos, n, bits, grid, perm);
  split_parts(n, part_points, ranges);
  PortableAttr a;
  a.att_type = 0; a.nc = a.nc_out = 3; a.seq_type = 2; a.grid = grid;
  quantize(pos, n, 3, bits, a);
  qmin.assign(3 * ranges.size(), INT32_MAX); qmax.assign(3 * ranges.size(), INT32_MIN);
  for (size_t p = 0; p < ranges.size(); ++p)
    for (uint32_t e = ranges[p].first; e < ranges[p].second; ++e)
      for (int c = 0; c < 3; ++c) {
        const int32_t x = a.vals[(size_t)3 * perm[e] + c];
        qmin[3 * p + c] = std::min(qmin[3 * p + c], x); qmax[3 * p + c] = std::max(qmax[3 * p + c], x);
      }
}
// The KEPT order of a cloud in parts of at most part_cells points (dsa_encode_cell_parts_sequential_batch, part_cells >= 1; the
// device sizes them in k_enc_part_cells of dsa_encode_order.h): merge_points, then split_parts over the m kept entries in place of
// the n rows, and per part and component the minimum and maximum of the position integers of rows kept[lo:hi], qmin / qmax[3 p + c].
static void cell_parts(const float *pos, uint32_t n, int bits, const Grid *grid, uint32_t part_cells, std::vector<uint32_t> &kept, std::vector<uint32_t> &row_entries,
                       std::vector<std::pair<uint32_t, uint32_t>> &ranges, std::vector<int32_t> &qmin, std::vector<int32_t> &qmax, int voxel_bits = 0, int voxel_point = 0) {
  PortableAttr a;              // (vals: the integers the position stream codes, the voxels' centroids among them)
  merge_points(pos, n, bits, grid, kept, row_entries, voxel_bits, voxel_point, &a.vals);
  split_parts((uint32_t)kept.size(), part_cells, ranges);
  qmin.assign(3 * ranges.size(), INT32_MAX); qmax.assign(3 * ranges.size(), INT32_MIN);
  for (size_t p = 0; p < ranges.size(); ++p)
    for (uint32_t e = ranges[p].first; e < ranges[p].second; ++e)
      for (int c = 0; c < 3; ++c) {
        const int32_t x = a.vals[(size_t)3 * kept[e] + c];
        qmin[3 * p + c] = std::min(qmin[3 * p + c], x); qmax[3 * p + c] = std::max(qmax[3 * p + c], x);
      }
}
// Additive levels of detail of the kept points (dsa_encode_lod_sequential_batch, lod_base_bits = D >= 1; the device's kernels are
// k_enc_lod_* of dsa_encode_order.h): with kept and key as merge_points has them, level(0) = 0 and for j >= 1 level(j) = max(0,
// c + 1 - D), c the leading bit-triples out of `bits` that key(kept[j]) and key(kept[j - 1]) share.  lod is kept in ascending
// (level, position in kept), row_entries the lod entry of the cell of every row; level l is cut by the rule of split_parts applied
// to its m_l points (an empty level has no part), ranges / levels / qmin / qmax say where every part lies in lod, which level it
// belongs to and the box of its position integers.
static void lod_parts(const float *pos, uint32_t n, int bits, const Grid *grid, uint32_t part_cells, int base_bits, std::vector<uint32_t> &lod, std::vector<uint32_t> &row_entries,
                      std::vector<std::pair<uint32_t, uint32_t>> &ranges, std::vector<uint32_t> &levels, std::vector<int32_t> &qmin, std::vector<int32_t> &qmax,
                      int voxel_bits = 0, int voxel_point = 0) {
  const int cell_bits = voxel_bits ? voxel_bits : bits;        // C: the kept points differ within their top C triples, L = C - D + 1
  check(base_bits >= 1 && base_bits <= cell_bits, "lod_base_bits out of range (1 .. position bits, 1 .. voxel_bits with voxels)");
  check(part_cells >= 1, "lod_base_bits needs part_cells >= 1");
  std::vector<uint32_t> kept;
  PortableAttr a;              // (vals: the integers the position stream codes, the voxels' centroids among them)
  merge_points(pos, n, bits, grid, kept, row_entries, voxel_bits, voxel_point, &a.vals);
  const uint32_t m = (uint32_t)kept.size(), L = (uint32_t)(cell_bits - base_bits + 1);
  std::vector<uint32_t> level(m, 0), count(L, 0), place(m, 0);
  for (uint32_t j = 1; j < m; ++j) {
    const uint64_t x = point_order_key(a.vals.data() + (size_t)3 * kept[j], bits), y = point_order_key(a.vals.data() + (size_t)3 * kept[j - 1], bits);
    int c = 0;
    while (c < bits && (x >> (3 * (bits - 1 - c))) == (y >> (3 * (bits - 1 - c)))) ++c;
    level[j] = (uint32_t)std::max(0, c + 1 - base_bits);
    check(level[j] < L, "lod_parts: two kept points share a cell");
  }
  for (uint32_t j = 0; j < m; ++j) ++count[level[j]];
  std::vector<uint32_t> base(L + 1, 0);
  for (uint32_t l = 0; l < L; ++l) base[l + 1] = base[l] + count[l];
  std::vector<uint32_t> next(base.begin(), base.end() - 1);
  lod.resize(m);
  for (uint32_t j = 0; j < m; ++j) { place[j] = next[level[j]]++; lod[place[j]] = kept[j]; }
  for (uint32_t r = 0; r < n; ++r) row_entries[r] = place[row_entries[r]];
  ranges.clear(); levels.clear();
  for (uint32_t l = 0; l < L; ++l) {
    const uint64_t parts = count[l] ? split_count(count[l], part_cells) : 0u;
    for (uint64_t p = 0; p < parts; ++p) { ranges.push_back({base[l] + split_bound(count[l], parts, p), base[l] + split_bound(count[l], parts, p + 1)}); levels.push_back(l); }
  }
  qmin.assign(3 * ranges.size(), INT32_MAX); qmax.assign(3 * ranges.size(), INT32_MIN);
  for (size_t p = 0; p < ranges.size(); ++p)
    for (uint32_t e = ranges[p].first; e < ranges[p].second; ++e)
      for (int c = 0; c < 3; ++c) {
        const int32_t x = a.vals[(size_t)3 * lod[e] + c];
        qmin[3 * p + c] = std::min(qmin[3 * p + c], x); qmax[3 * p + c] = std::max(qmax[3 * p + c], x);
      }
}
// The float this library's decoder returns for integer q of a component on a grid (k_finalize, Dequantizer.cs:15-23): every step
// rounded to float32, no fused multiply-add.
static inline float dequantized(int32_t q, float origin, float range, int bits) {
  volatile float delta = range / (float)(int32_t)((1u << bits) - 1u);
  volatile float prod = (float)q * delta;
  volatile float out = prod + origin;
  return out;
}

// Point cloud, sequential (BASELINE config 1), positions only: int32 num_points, one attributes decoder, positions quantised,
// Difference + Wrap in linear order, always through the symbol coder.
static void encode_point_cloud(const float *pos, uint32_t n, const Options &opt, std::vector<uint8_t> &out) {
  MeshIn in{pos, n, nullptr, 0, nullptr, nullptr, nullptr};
  Options o = opt;
  o.raw_integers = 0; o.no_prediction = 0;
  encode_sequential(in, o, false, false, out);
}

}  // namespace synth
