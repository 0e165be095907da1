// tests/hostcheck/encvalence_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The encoder's valence pass of the product (draco-sharp_amd/csrc/dsa_encode_schemes.h: k_enc_val_init, k_enc_valence one lane per
// mesh, k_enc_val_split, behind the connectivity kernels of dsa_encode_conn.h with the start faces' times recorded) compiled for
// the host with AddressSanitizer + UBSan and run thread by thread, against the host coder (dsa_encode_host.h:
// valence_context_symbols over EbEncoder's face_time) on the same faces: the same six context lists, symbol for symbol, and not
// one access outside a mesh's arrays (the arena's gaps are poisoned).  Nothing here is linked into the product.
//
//   encvalence_host <meshes.bin>    file: u32 count, then per mesh u32 nv, u32 nf, u32 faces[3 nf]
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

struct ListStream { uint32_t nv; uint64_t syms, bl; uint32_t out_cap; uint64_t out_rans, out_bits; };   // what k_enc_val_split sets of an EncStream

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: encvalence_host <meshes.bin>\n"); return 2; }
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
  }
  fclose(f);
  // ---- the arena, laid out like dsa_encode.h lays a chunk out, every gap poisoned; every other mesh coded with standard symbols
  // (no valence regions) in the same launches
  const uint32_t n = count;
  std::vector<dsa::EncConn> hc(n);
  std::vector<ListStream> streams(6 * n);
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
      C.vstream = 6 * i;
      C.init_time = take(4 * F); C.vtime = take(4 * F); C.vval = take(4 * (V + F)); C.vc2v = take(12 * F);
      C.vctx = take(F); C.vsyms = take(4 * F); C.vbl = take(F); C.vrans = take(4 * F + 96); C.vbits = take(4 * F + 96);
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
  launch(dsa::k_enc_connectivity_timed, (n + lanes - 1) / lanes, 1, WAVE, arena, conns, n, lanes);
  launch(dsa::k_enc_val_init, gx, n, 256, arena, conns, n);
  launch(dsa::k_enc_valence, (n + lanes - 1) / lanes, 1, WAVE, arena, conns, n, lanes);
  launch(dsa::k_enc_val_split<ListStream>, n, 1, WAVE, arena, conns, n, streams.data());
  // ---- against the host coder
  uint32_t coded = 0, standard = 0, refused = 0, split_meshes = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const In &m = meshes[i];
    const dsa::EncConn &C = hc[i];
    std::vector<float> pos((size_t)3 * std::max(m.nv, 1u), 0.0f);
    synth::MeshIn in;
    in.pos = pos.data(); in.nv = m.nv; in.faces = m.faces.data(); in.nf = m.nf; in.normals = nullptr; in.uvs = nullptr; in.generic = nullptr;
    synth::MeshPlan pl;
    synth::Options opt;
    opt.predictive_connectivity = C.vstream != DSA_INVALID ? 2 : 0;
    bool host_ok = true;
    try {
      synth::check(m.nv >= 3 && m.nf >= 1, "mesh needs positions and faces");
      for (uint32_t x : m.faces) synth::check(x < m.nv, "face index out of range");
      synth::plan_mesh(in, opt, pl);
    } catch (const std::exception &) { host_ok = false; }
    const bool dev_ok = C.status == dsa::ENC_OK;
    if (host_ok != dev_ok) { fprintf(stderr, "mesh %u: host coder %s, device source status %u\n", i, host_ok ? "codes" : "refuses", C.status); return 1; }
    if (!host_ok) { ++refused; continue; }
    if (C.vstream == DSA_INVALID) { ++standard; continue; }
    ++coded;
    if (pl.eb.num_split_symbols) ++split_meshes;
    const uint32_t *syms = (const uint32_t *)(arena + C.vsyms);
    uint32_t off = 0;
    for (int k = 0; k < 6; ++k) {
      const ListStream &S = streams[C.vstream + k];
      const std::vector<uint32_t> &want = pl.ctx_symbols[k];
      if (C.vcount[k] != want.size() || S.nv != want.size() || S.syms != C.vsyms + 4ull * off || S.bl != C.vbl + off) {
        fprintf(stderr, "mesh %u: context %d holds %u symbols on the device, %zu on the host\n", i, k, C.vcount[k], want.size());
        return 1;
      }
      for (size_t q = 0; q < want.size(); ++q)
        if (syms[off + q] != want[q]) { fprintf(stderr, "mesh %u: context %d symbol %zu differs\n", i, k, q); return 1; }
      off += (uint32_t)want.size();
    }
  }
  printf("encvalence: %u meshes, %u valence lists alike (%u with topology splits), %u standard, %u refused alike\n", n, coded, split_meshes, standard, refused);
  return 0;
}
