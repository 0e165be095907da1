// tests/hostcheck/encweld_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The encoder's weld kernels (draco-sharp_amd/csrc/dsa_encode_weld.h: marks, the open-addressing insert with its minimum, the
// scan, the maps, the per-vertex test, the gather, over 3 + L key sets per mesh) compiled for the host with AddressSanitizer +
// UBSan and run thread by thread under the product's launch sequence (enc_weld_launch, its slicing included) -- once forwards,
// once backwards, so that other threads win the slots and the minima -- against the host coder's weld (dsa_encode_host.h:
// synth::weld_points) on the same points: the same counts, maps, faces, corner ids and welded rows, and not one access outside a
// mesh's arrays (the arena's gaps are poisoned).  Nothing here is linked into the product.
//
//   encweld_host <meshes.bin> [max_grid_y]
//                               file: u32 count, then per mesh u32 P, F, normals (0 / 1), texcoords (0 / 1), segments of the
//                               vertex key, listed attributes welded alone, u32 row_bytes[segments], u32 listed_row_bytes[listed];
//                               u32 faces[3 F]; per segment P rows; normals f32[3 P]; texture coordinates f32[2 P]; per listed
//                               attribute P rows.  max_grid_y: the most rows of a launch's grid y (the device's 65535 when absent)
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
#include "../../draco-sharp_amd/csrc/dsa_encode_weld.h"

struct In {
  uint32_t P = 0, F = 0, normals = 0, texcoords = 0;
  std::vector<uint32_t> row_bytes, listed_bytes, faces;
  std::vector<std::vector<uint8_t>> segs, listed;
  std::vector<float> nrm, uv;
};

static int run(const std::vector<In> &meshes, bool backwards, uint32_t max_grid_y) {
  const uint32_t n = (uint32_t)meshes.size();
  std::vector<dsa::EncWeld> recs(n);
  uint64_t cur = 0;
  std::vector<std::pair<uint64_t, uint64_t>> regions;
  auto take = [&](uint64_t bytes) { cur = (cur + 255) & ~255ull; cur += 64; const uint64_t at = cur; regions.push_back({at, bytes}); cur += bytes + 64; return at; };
  uint32_t maxp = 1, sets = 3;
  for (uint32_t i = 0; i < n; ++i) {
    const In &m = meshes[i];
    recs[i] = dsa::enc_weld_inputs(take, m.P, m.F, m.row_bytes.data(), (uint32_t)m.row_bytes.size(), m.normals != 0, m.texcoords != 0, m.listed_bytes.data(), (uint32_t)m.listed_bytes.size());
    maxp = std::max(maxp, std::max(m.P, 3u * m.F));
    sets = std::max(sets, recs[i].num_sets);
  }
  for (uint32_t i = 0; i < n; ++i) dsa::enc_weld_regions(take, recs[i]);
  std::vector<uint8_t> store(cur + 256, 0);
  uint8_t *arena = store.data();
  for (uint32_t i = 0; i < n; ++i) {
    const In &m = meshes[i];
    const dsa::EncWeld &W = recs[i];
    if (m.F) memcpy(arena + W.faces, m.faces.data(), 12ull * m.F);
    for (size_t j = 0; j < m.listed.size(); ++j) if (!m.listed[j].empty()) memcpy(arena + W.seg[W.set[3 + j].first_seg].src, m.listed[j].data(), m.listed[j].size());
    for (size_t g = 0; g < m.segs.size(); ++g) if (!m.segs[g].empty()) memcpy(arena + W.seg[g].src, m.segs[g].data(), m.segs[g].size());
    if (m.normals && m.P) memcpy(arena + W.seg[W.set[1].first_seg].src, m.nrm.data(), 12ull * m.P);
    if (m.texcoords && m.P) memcpy(arena + W.seg[W.set[2].first_seg].src, m.uv.data(), 8ull * m.P);
  }
  ASAN_POISON_MEMORY_REGION(arena, store.size());
  for (auto &rg : regions) ASAN_UNPOISON_MEMORY_REGION(arena + rg.first, rg.second);
  const uint32_t gx = std::max(1u, std::min(4u, (maxp + 1023u) / 1024u));
  dsa::enc_weld_launch([backwards](auto kernel, uint32_t grid_x, uint32_t grid_y, uint32_t block, auto... args) { launch(kernel, grid_x, grid_y, block, backwards, args...); },
                       arena, recs.data(), n, sets, gx, max_grid_y);
  for (uint32_t i = 0; i < n; ++i) {
    const In &m = meshes[i];
    const dsa::EncWeld &W = recs[i];
    std::vector<synth::WeldSeg> key, listed;
    for (size_t j = 0; j < m.listed.size(); ++j) listed.push_back({m.listed[j].data() ? (const void *)m.listed[j].data() : (const void *)"", m.listed_bytes[j]});
    for (size_t g = 0; g < m.segs.size(); ++g) key.push_back({m.segs[g].data() ? (const void *)m.segs[g].data() : (const void *)"", m.row_bytes[g]});
    synth::Welded want;
    static const char *const names[3] = {"", "normal", "texcoord"};
    synth::weld_points(m.P, m.faces.data(), m.F, key, m.normals ? (m.nrm.empty() ? (const float *)"" : m.nrm.data()) : nullptr,
                       m.texcoords ? (m.uv.empty() ? (const float *)"" : m.uv.data()) : nullptr, want, listed);
#define SAME(cond, what) do { if (!(cond)) { fprintf(stderr, "mesh %u (%s): %s differ\n", i, backwards ? "backwards" : "forwards", what); return 1; } } while (0)
    auto same = [&](uint64_t at, const void *data, size_t bytes) { return bytes == 0 || memcmp(arena + at, data, bytes) == 0; };
    SAME(W.status == dsa::ENC_WELD_OK, "status");
    SAME(W.num_sets == 3 + m.listed.size() && want.listed.size() == m.listed.size(), "key sets");
    SAME(W.set[0].count == want.vertex.count, "class counts");
    SAME(same(W.set[0].of, want.vertex.of_point.data(), 4ull * m.P), "*_of_point");
    SAME(same(W.set[0].point, want.vertex.point.data(), 4ull * W.set[0].count), "*_point");
    SAME(same(W.faces_out, want.faces.data(), 12ull * m.F), "welded faces");
    for (size_t g = 0; g < m.segs.size(); ++g) SAME(same(W.seg[g].dst, want.vertex_rows[g].data(), want.vertex_rows[g].size()), "welded vertex rows");
    SAME((W.set[1].num_segs != 0) == (m.normals != 0) && (W.set[2].num_segs != 0) == (m.texcoords != 0), "the attributes the mesh has");
    for (uint32_t k = 1; k < W.num_sets; ++k) {
      const dsa::EncWeldSet &S = W.set[k];
      SAME(k < 3 || S.num_segs == 1, "listed key sets");
      if (S.num_segs == 0) continue;
      const synth::Welded::KeySet a = want.key_set(k);
      const std::string what = k < 3 ? names[k] : "listed attribute";
      SAME(S.count == a.keys.count, (what + " class counts").c_str());
      SAME(same(S.of, a.keys.of_point.data(), 4ull * m.P), (what + " *_of_point").c_str());
      SAME(same(S.point, a.keys.point.data(), 4ull * S.count), (what + " *_point").c_str());
      SAME((W.differs[k] != 0) == !a.per_vertex, (what + " per vertex").c_str());
      SAME(a.rows.size() == (size_t)W.seg[S.first_seg].row_bytes * (a.per_vertex ? want.vertex.count : a.keys.count), (what + " row count").c_str());
      SAME(same(W.seg[S.first_seg].dst, a.rows.data(), a.rows.size()), ("welded " + what + " rows").c_str());
      if (W.differs[k]) SAME(a.corners.size() == 3ull * m.F && same(W.corners_out[k], a.corners.data(), 12ull * m.F), (what + " corners").c_str());
    }
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: encweld_host <meshes.bin> [max_grid_y]\n"); return 2; }
  const uint32_t max_grid_y = argc > 2 ? (uint32_t)strtoul(argv[2], nullptr, 10) : 65535u;
  if (max_grid_y == 0) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  std::vector<In> meshes(count);
  for (auto &m : meshes) {
    uint32_t head[6];
    if (fread(head, 4, 6, f) != 6) return 2;
    m.P = head[0]; m.F = head[1]; m.normals = head[2]; m.texcoords = head[3];
    m.row_bytes.resize(head[4]); m.listed_bytes.resize(head[5]);
    if (head[4] == 0 || head[5] > dsa::EW_MAX_LISTED || head[4] + head[5] > 18 || fread(m.row_bytes.data(), 4, head[4], f) != head[4]) return 2;
    if (head[5] && fread(m.listed_bytes.data(), 4, head[5], f) != head[5]) return 2;
    m.faces.resize((size_t)3 * m.F);
    if (m.F && fread(m.faces.data(), 4, m.faces.size(), f) != m.faces.size()) return 2;
    for (uint32_t x : m.faces) if (x >= m.P) { fprintf(stderr, "index out of range in the input file\n"); return 2; }      // (the library's host checks keep such a mesh from the device)
    m.segs.resize(head[4]);
    for (uint32_t g = 0; g < head[4]; ++g) {
      m.segs[g].resize((size_t)m.P * m.row_bytes[g]);
      if (!m.segs[g].empty() && fread(m.segs[g].data(), 1, m.segs[g].size(), f) != m.segs[g].size()) return 2;
    }
    if (m.normals) { m.nrm.resize((size_t)3 * m.P); if (m.P && fread(m.nrm.data(), 4, m.nrm.size(), f) != m.nrm.size()) return 2; }
    if (m.texcoords) { m.uv.resize((size_t)2 * m.P); if (m.P && fread(m.uv.data(), 4, m.uv.size(), f) != m.uv.size()) return 2; }
    m.listed.resize(head[5]);
    for (uint32_t j = 0; j < head[5]; ++j) {
      m.listed[j].resize((size_t)m.P * m.listed_bytes[j]);
      if (!m.listed[j].empty() && fread(m.listed[j].data(), 1, m.listed[j].size(), f) != m.listed[j].size()) return 2;
    }
  }
  fclose(f);
  if (run(meshes, false, max_grid_y) != 0 || run(meshes, true, max_grid_y) != 0) return 1;
  printf("encweld: %u meshes welded alike, forwards and backwards\n", count);
  return 0;
}
