// tests/hostcheck/encorder_common.h -- TEST INFRASTRUCTURE ONLY.
//
// What the host checks of the encoder's point-order stage share (encorder, encmerge, encsplit, enccellparts, enclod, encmeans, encvotes): the
// kernels of draco-sharp_amd/csrc/dsa_encode_order.h compiled for the host with AddressSanitizer + UBSan and run thread by thread by
// the product's own launch sequence (enc_order_stage, dsa_encode_layout.h: what enc_stage_attributes runs for the request, nothing
// restated here) in the arena the product's layout hands out (enc_layout_sequential: records, tile lists and every region are the
// library's own), forwards or backwards, with every gap between two regions poisoned.  What the means and the votes accumulate in is
// filled with a pattern and poisoned until the stage zeroes each pass's one range, as the product's memset does.  Each program keeps the
// assertions that are its own.  Nothing here is linked into the product.
#pragma once
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../draco-sharp_amd/csrc/dsa_common.h"
#include "../../draco-sharp_amd/csrc/dsa_types.h"

#include "hip_on_host.h"

#include "../../draco-sharp_amd/csrc/dsa_encode_layout.h"

// a case of a case file: u32 n, bits, has_grid and `words` - 3 further words of the program's; f32 pos[3 n]; with a grid f32
// origin[3], range; with faces (the fourth word their number F) u32 faces[3 F]
struct In {
  uint32_t n = 0, bits = 0, has_grid = 0, more[2] = {0, 0};
  std::vector<float> pos;
  float grid[4] = {0, 0, 0, 0};
  std::vector<uint32_t> faces;
};
// the file: u32 count, then the cases.  False: the file is not one.
static bool read_cases(const char *path, uint32_t words, bool faces, std::vector<In> &cases) {
  FILE *f = fopen(path, "rb");
  if (!f) { perror(path); return false; }
  uint32_t count = 0;
  bool good = fread(&count, 4, 1, f) == 1;
  if (good) cases.resize(count);
  for (size_t k = 0; good && k < cases.size(); ++k) {
    In &c = cases[k];
    uint32_t head[5] = {0, 0, 0, 0, 0};
    good = words <= 5 && fread(head, 4, words, f) == words;
    c.n = head[0]; c.bits = head[1]; c.has_grid = head[2]; c.more[0] = head[3]; c.more[1] = head[4];
    good = good && c.n != 0 && c.bits >= 1 && c.bits <= 20;
    if (!good) break;
    c.pos.resize((size_t)3 * c.n);
    good = fread(c.pos.data(), 4, c.pos.size(), f) == c.pos.size() && (!c.has_grid || fread(c.grid, 4, 4, f) == 4);
    if (good && faces) {
      c.faces.resize((size_t)3 * c.more[0]);
      good = c.faces.empty() || fread(c.faces.data(), 4, c.faces.size(), f) == c.faces.size();
      for (uint32_t x : c.faces) if (x >= c.n) { fprintf(stderr, "index out of range in the input file\n"); good = false; }
    }
  }
  fclose(f);
  return good;
}

// the request of a chunk: point_order with what else the program checks
struct Ask {
  uint32_t bits = 0;
  bool merge = false;
  uint32_t part_points = 0, part_cells = 0, lod_base_bits = 0, mean_mask = 0, vote_mask = 0;
  bool normals = false, listed = false;     // every cloud carries normals; or texture coordinates and a generic attribute of three bytes
  bool label = false;                       // ... and behind them a listed uint8 attribute of one component
  bool is_mesh = false, compressed = false; // meshes with raw / with compressed indices
};

// One chunk: its request, layout and arena.  A step that returns false has left `why`.
struct Run {
  std::vector<const In *> which;
  uint32_t n = 0;
  Ask ask;
  std::vector<dsa_mesh_attr_input> meshes;
  std::vector<EncMeshGrids> grids;
  std::vector<dsa_attribute_input> labels;
  EncRequest rq;
  std::unique_ptr<EncChunk> ck;
  std::vector<std::pair<uint64_t, uint64_t>> log;
  std::vector<uint8_t> store;
  uint8_t *arena = nullptr;
  std::map<uint64_t, uint64_t> region;
  std::vector<dsa::EncStream> laid, records; // the stream records as the layout made them; the device's, which the kernels write
  std::string why;

  bool fail(const std::string &s) { why = s; return false; }
  const synth::Grid *grid(uint32_t i) const { return which[i]->has_grid ? &grids[i].slot[0] : nullptr; }
  bool sized(uint64_t off, uint64_t bytes) const { auto it = region.find(off); return it != region.end() && it->second >= bytes; }
  const EncLayout &L() const { return ck->L; }
  dsa::EncOrder *clouds() const { return (dsa::EncOrder *)(arena + ck->L.ord_at); }
  dsa::EncPart *parts() const { return (dsa::EncPart *)(arena + ck->L.parts_at); }

  // the request, the chunk with its checks and its layout (every region logged), the arena with the uploads as enc_upload copies
  // them and everything behind them zero, the region map
  bool begin(const std::vector<const In *> &cases, const Ask &a) {
    which = cases; n = (uint32_t)cases.size(); ask = a;
    meshes.resize(n); grids.resize(n); labels.assign(a.label ? n : 0, dsa_attribute_input());
    memset(meshes.data(), 0, sizeof(dsa_mesh_attr_input) * n);
    bool any_grid = false;
    for (uint32_t i = 0; i < n; ++i) {
      const In &c = *which[i];
      dsa_mesh_input &m = meshes[i].mesh.mesh;
      m.num_vertices = c.n; m.positions = c.pos.data();
      if (a.normals) m.normals = c.pos.data();
      // (texcoords: 2 n floats, generic: 3 n bytes -- both inside the 3 n floats of the positions; their values are not read here)
      if (a.listed) { m.texcoords = c.pos.data(); m.generic = (const uint8_t *)c.pos.data(); m.generic_components = 3; }
      if (a.label) {                                           // (its bytes are the positions' too)
        dsa_attribute_input &x = labels[i];
        memset(&x, 0, sizeof(x));
        x.attribute_type = 4; x.data_type = 2; x.num_components = 1; x.unique_id = DSA_UNIQUE_ID_DEFAULT; x.values = c.pos.data();
        meshes[i].attributes = &x; meshes[i].num_attributes = 1;
      }
      if (a.is_mesh) { m.num_faces = (uint32_t)(c.faces.size() / 3); m.faces = c.faces.data(); }
      if (c.has_grid) { synth::Grid &g = grids[i].slot[0]; memcpy(g.origin, c.grid, 12); g.range = c.grid[3]; g.mode = 1; any_grid = true; }
    }
    rq.n = n; rq.meshes = meshes.data(); rq.sequential = true; rq.point_order = true; rq.merge_points = a.merge;
    rq.part_points = a.part_points; rq.part_cells = a.part_cells; rq.lod_base_bits = a.lod_base_bits; rq.mean_attributes = a.mean_mask; rq.vote_attributes = a.vote_mask;
    if (any_grid) rq.grids = grids.data();
    memset(&rq.seq, 0, sizeof(rq.seq));
    synth::Options d;
    dsa_encode_options &o = rq.seq.base;
    o.position_bits = (int32_t)a.bits; o.texcoord_bits = d.uv_bits; o.normal_bits = d.normal_bits; o.symbol_scheme = d.force_scheme; o.compression_level = d.compression_level;
    rq.seq.geometry = a.is_mesh ? 1 : 0; rq.seq.compress_connectivity = a.compressed ? 1 : 0;
    ck.reset(new EncChunk(rq, 0, n, n));
    ck->region_log = &log;
    for (uint32_t i = 0; i < n; ++i) { enc_check_sequential_mesh(*ck, i); if (!ck->good(i)) return fail("case " + std::to_string(i) + " refused: " + ck->E->messages[i]); }
    enc_layout_sequential(*ck);
    const EncLayout &L = ck->L;
    if (L.ord.size() != n || L.ord_passes != (3 * a.bits + 7) / 8) return fail(std::to_string(L.ord.size()) + " order records for " + std::to_string(n) + " clouds, " + std::to_string(L.ord_passes) + " passes");
    store.assign(L.total_bytes + 256, 0);
    arena = store.data();
    for (const EncUpload &u : L.uploads) {
      if (u.off >= L.input_bytes || u.off + u.bytes > L.input_bytes || (u.narrow && !a.compressed)) return fail("an upload outside the inputs");
      if (!u.narrow) { if (u.bytes) memcpy(arena + u.off, u.src, u.bytes); continue; }
      for (size_t e = 0; e < u.bytes / 2; ++e) ((uint16_t *)(arena + u.off))[e] = (uint16_t)((const uint32_t *)u.src)[e];
    }
    for (const auto &r : log) { if (r.first + r.second > L.total_bytes) return fail("a region outside the arena"); region[r.first] = std::max(region[r.first], r.second); }
    laid = records = L.streams;
    return true;
  }
  // the position integers of cloud i where k_enc_quantize / k_enc_grid_quantize leave them: the twin's
  void write_positions(uint32_t i) {
    const In &c = *which[i];
    synth::PortableAttr a;
    a.att_type = 0; a.nc = a.nc_out = 3; a.seq_type = 2; a.grid = grid(i);
    synth::quantize(c.pos.data(), c.n, 3, (int)ask.bits, a);
    memcpy(arena + ck->L.ord[i].vals, a.vals.data(), 12ull * c.n);
  }
  // every gap between two regions poisoned, and the regions `untouched` (of slots that stay empty: no kernel touches them); the
  // means' and the votes' ranges hold what an arena used before leaves there, poisoned until the stage zeroes them
  void poison(const std::vector<std::pair<uint64_t, uint64_t>> &untouched = {}) {
    const EncLayout &L = ck->L;
    const std::pair<uint64_t, uint64_t> ranges[2] = {{L.mean_zero_at, L.mean_zero_bytes}, {L.vote_zero_at, L.vote_zero_bytes}};
    for (const auto &r : ranges) if (r.second) memset(arena + r.first, 0xAB, r.second);
    ASAN_POISON_MEMORY_REGION(arena, store.size());
    for (const auto &r : region) ASAN_UNPOISON_MEMORY_REGION(arena + r.first, r.second);
    for (const auto &r : untouched) ASAN_POISON_MEMORY_REGION(arena + r.first, r.second);
    for (const auto &r : ranges) if (r.second) ASAN_POISON_MEMORY_REGION(arena + r.first, r.second);
  }
  void unpoison() { ASAN_UNPOISON_MEMORY_REGION(arena, store.size()); }
  // the product's stage for the request, every thread of every grid one after the other
  bool stage(bool backwards, uint32_t gx_faces = 0u) {
    const EncLayout &L = ck->L;
    auto go = [backwards](auto kernel, uint32_t grid_x, uint32_t grid_y, uint32_t block, auto... args) { launch(kernel, grid_x, grid_y, block, backwards, args...); };
    auto zero = [&](uint64_t off, uint64_t bytes) {           // the product's memset: the one range, gaps between its regions included
      ASAN_UNPOISON_MEMORY_REGION(arena + off, bytes);
      memset(arena + off, 0, bytes);
      ASAN_POISON_MEMORY_REGION(arena + off, bytes);
      for (const auto &r : region) if (r.first >= off && r.first + r.second <= off + bytes) ASAN_UNPOISON_MEMORY_REGION(arena + r.first, r.second);
    };
    return enc_order_stage(go, zero, [](const char *) { return true; }, L, ask.is_mesh, gx_faces, arena, records.data(), (uint32_t)records.size()) || fail("the stage stopped");
  }
  // k_enc_gather itself lives in dsa_encode.h, which needs HIP: its accesses -- e2v[e], vals[nc e2v[e] + c], d[nc e + c] for e < nv of
  // every stream record it does not pass by (kind 3: an empty slot) -- are made here in its place, in the product's regions
  void gather() {
    for (const dsa::EncStream &S : records) {
      if (S.kind == 3) continue;
      const int32_t *vals = (const int32_t *)(arena + S.vals);
      const uint32_t *e2v = (const uint32_t *)(arena + S.e2v);
      int32_t *dst = (int32_t *)(arena + S.d);
      for (uint32_t e = 0; e < S.nv; ++e)
        for (uint32_t k = 0; k < S.nc; ++k) dst[(size_t)e * S.nc + k] = vals[(size_t)e2v[e] * S.nc + k];
    }
  }
  // nothing of record s moved but nv (slot: nor but e2v and the kind of an empty slot)
  bool same_beyond(size_t s, bool slot) const {
    dsa::EncStream a = records[s], b = laid[s];
    a.nv = b.nv;
    if (slot) { a.e2v = b.e2v; a.kind = b.kind; }
    return memcmp(&a, &b, sizeof(a)) == 0;
  }

  // ---- part_cells (with or without levels): the part SLOTS of cloud i, `slots` of them of which the host coder fills `live`
  typedef std::vector<std::pair<uint32_t, uint32_t>> Ranges;
  std::string at(uint32_t i, uint32_t p, const char *what) const { return "case " + std::to_string(i) + " slot " + std::to_string(p) + ": " + what; }
  // as the layout makes them: empty records and boxes from part_at on, tiles from tile_at on and a set of stream records for the
  // most a slot can hold, on the cloud's kept rows and values, with regions of their own; the regions of the slots that stay empty
  // go to `untouched`
  bool slots_laid(uint32_t i, uint32_t live, uint32_t slots, size_t &part_at, size_t &tile_at, std::vector<std::pair<uint64_t, uint64_t>> &untouched) {
    const EncLayout &L = ck->L;
    const In &c = *which[i];
    const dsa::EncOrder &O = L.ord[i];
    const uint32_t s0 = L.first_stream[i], na = O.streams, cap = std::min(ask.part_cells, c.n);
    if (O.part_cells != ask.part_cells || O.part0 != part_at || O.part_slots != slots) return fail("case " + std::to_string(i) + ": order record");
    if (live == 0 || live > slots || ck->num_parts(i) != slots || L.part_of_mesh[i] != part_at || L.first_stream[i + 1] != s0 + na * slots)
      return fail("case " + std::to_string(i) + ": " + std::to_string(ck->num_parts(i)) + " slots laid out, " + std::to_string(slots) + " expected for " + std::to_string(live) + " parts");
    for (uint32_t p = 0; p < slots; ++p, ++part_at) {
      const dsa::EncPart &P = L.parts[part_at];
      if (P.cloud != i || P.lo != 0 || P.n != 0 || P.pad != 0) return fail(at(i, p, "the record does not start empty"));
      for (int k = 0; k < 3; ++k) if (P.qmin[k] != INT32_MAX || P.qmax[k] != INT32_MIN) return fail(at(i, p, "the box does not start empty"));
      for (uint32_t t = 0; t < (cap + ORD_TILE - 1) / ORD_TILE; ++t, ++tile_at)
        if (tile_at >= L.part_tiles.size() || L.part_tiles[tile_at].part != part_at || L.part_tiles[tile_at].tile != t) return fail(at(i, p, "a tile is not in the list"));
      for (uint32_t k = 0; k < na; ++k) {
        const dsa::EncStream &S = L.streams[s0 + na * p + k], &first = L.streams[s0 + k];
        if (S.linear != 0 || S.rows != c.n || S.e2v != dsa::ord_kept(O) || S.vals == 0 || S.vals != first.vals || S.src != first.src || S.part != (p ? (dsa::ENC_PART_BEHIND | dsa::ENC_PART_SIZED) : 0u) || (p && S.nv != 0))
          return fail(at(i, p, "a stream is not a slot on the cloud's kept rows and values"));
        if (p && (S.grid_mode != 0 || S.d == first.d || S.syms == first.syms || S.hist_raw == first.hist_raw || S.out_rans == first.out_rans)) return fail(at(i, p, "a stream shares a region of the first slot's"));
        if (S.d == S.vals || !sized(S.d, 4ull * S.nc * cap) || !sized(S.syms, 4ull * S.nc * cap) || !sized(S.bl, cap) || !sized(first.vals, 4ull * S.nc * c.n) || S.out_cap < 4u * cap * S.nc + 16u ||
            !sized(S.out_rans, S.out_cap) || !sized(S.out_bits, S.out_cap) || !sized(S.hist_raw, 4ull * S.hist_cap) || !sized(S.prob, 4ull * 64) || !sized(S.cum, 4ull * 64) || !sized(S.plan_order, 4ull * 64) ||
            !sized(S.plan_tmp, 4ull * 64))
          return fail(at(i, p, "regions of a stream too small"));
        if (p >= live)
          for (uint64_t off : {S.d, S.syms, S.bl, S.hist_raw, S.out_rans, S.out_bits, S.prob, S.cum, S.plan_order, S.plan_tmp}) untouched.push_back({off, region[off]});
      }
    }
    return true;
  }
  // behind the stage, held to the host coder's ranges (levels: of every live part, or none), boxes and rows: lo, n and the level in
  // the slot records, nv and e2v on ord_part_rows in every stream record of the slot, nothing else of a record moved; a slot behind
  // the last part with n = nv = 0, kind 3 and no box; entry(p, e, r) holds what the gather left at entry e of slot p to row r
  template <class Entry>
  bool slots_sized(uint32_t i, const Ranges &ranges, const std::vector<uint32_t> *levels, const std::vector<uint32_t> &rows, const std::vector<int32_t> &want_min, const std::vector<int32_t> &want_max,
                   size_t &part_at, uint64_t &parts_seen, uint64_t &empty_seen, Entry &&entry) {
    const EncLayout &L = ck->L;
    const dsa::EncOrder &O = clouds()[i];
    const uint32_t s0 = L.first_stream[i], na = O.streams, live = (uint32_t)ranges.size(), slots = ck->num_parts(i);
    for (uint32_t p = 0; p < slots; ++p, ++part_at) {
      const dsa::EncPart &P = parts()[part_at], &was = L.parts[part_at];
      const uint32_t lo = p < live ? ranges[p].first : 0u, cnt = p < live ? ranges[p].second - lo : 0u;
      if (P.cloud != was.cloud || P.pad != (p < live && levels ? (*levels)[p] : 0u)) return fail(at(i, p, "the record changed beyond its range and box"));
      if (P.lo != lo || P.n != cnt || (p < live && (cnt == 0 || cnt > ask.part_cells))) return fail(at(i, p, "record says ") + std::to_string(P.lo) + " + " + std::to_string(P.n) + ", the host coder " + std::to_string(lo) + " + " + std::to_string(cnt));
      for (uint32_t k = 0; k < na; ++k) {
        const dsa::EncStream &a = records[s0 + na * p + k], &b = laid[s0 + na * p + k];
        if (a.nv != cnt || a.e2v != dsa::ord_part_rows(O) + 4ull * lo) return fail(at(i, p, "a stream has nv ") + std::to_string(a.nv) + " and reads from " + std::to_string(a.e2v));
        if (a.kind != (p < live ? b.kind : 3u) || (a.part & dsa::ENC_PART_SIZED) != (p ? dsa::ENC_PART_SIZED : 0u)) return fail(at(i, p, "a stream is of kind ") + std::to_string(a.kind));
        if (!same_beyond(s0 + na * p + k, true)) return fail(at(i, p, "the record of a stream changed beyond nv, e2v and the kind of an empty slot"));
      }
      if (p >= live) {
        for (int k = 0; k < 3; ++k) if (P.qmin[k] != INT32_MAX || P.qmax[k] != INT32_MIN) return fail(at(i, p, "an empty slot has a box"));
        ++empty_seen;
        continue;
      }
      for (int k = 0; k < 3; ++k)
        if (P.qmin[k] != want_min[3 * p + k] || P.qmax[k] != want_max[3 * p + k])
          return fail(at(i, p, "box ") + std::to_string(P.qmin[k]) + " .. " + std::to_string(P.qmax[k]) + " of component " + std::to_string(k) + ", the host coder " + std::to_string(want_min[3 * p + k]) + " .. " + std::to_string(want_max[3 * p + k]));
      for (uint32_t e = 0; e < P.n; ++e) if (!entry(p, e, rows[P.lo + e])) return fail(at(i, p, "entry ") + std::to_string(e) + " does not carry row " + std::to_string(rows[P.lo + e]));
      ++parts_seen;
    }
    return true;
  }
};
