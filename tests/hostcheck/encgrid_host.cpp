// tests/hostcheck/encgrid_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The encoder's grid kernels of the product (draco-sharp_amd/csrc/dsa_encode_grid.h: the bounds of every array with its finite
// flag, the fold of a group, the quantiser on a given grid with its smallest offending rows) compiled for the host with
// AddressSanitizer + UBSan and run thread by thread -- once forwards, once backwards, with one block per array and with three, so
// that other threads win the minima -- against the host coder (dsa_encode_host.h: synth::shared_grid, synth::quantize_on_grid) on
// the same arrays: the same keys, flags, grids, integers and refusals, and not one access outside an array (the arena's gaps
// are poisoned).  Nothing here is linked into the product.
//
//   encgrid_host <arrays.bin>   file: u32 count, then per array u32 group, nc, rows, bits; f32 origin[4], range (an explicit grid
//                               for the check; range 0: the grid of the array's group); f32 values[rows * nc].  Arrays of one
//                               group and component count lie side by side.
#include <sanitizer/asan_interface.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../draco-sharp_amd/csrc/dsa_common.h"
#include "../../draco-sharp_amd/csrc/dsa_types.h"
#include "../../draco-sharp_amd/csrc/dsa_encode_host.h"

#include "hip_on_host.h"

#include "../../draco-sharp_amd/csrc/dsa_encode_grid.h"

struct In { uint32_t group = 0, nc = 0, rows = 0, bits = 0; float origin[4] = {0, 0, 0, 0}, range = 0; std::vector<float> v; };
// what k_enc_grid_quantize reads of a stream's record
struct Stream { uint64_t src, vals; uint32_t kind, grid_mode, bits, nc_out, rows, grid_nonfinite, grid_off; float qmin[4], qrange; };

static int run(const std::vector<In> &arrays, bool backwards, uint32_t gx) {
  const uint32_t n = (uint32_t)arrays.size();
  uint64_t cur = 0;
  std::vector<std::pair<uint64_t, uint64_t>> regions;
  auto take = [&](uint64_t bytes) { cur = (cur + 255) & ~255ull; cur += 64; const uint64_t at = cur; regions.push_back({at, bytes}); cur += bytes + 64; return at; };
  std::vector<dsa::EncGridItem> items(n);
  std::vector<dsa::EncGridGroup> groups;
  std::vector<Stream> streams(n);
  for (uint32_t i = 0; i < n; ++i) {
    const In &a = arrays[i];
    dsa::EncGridItem &I = items[i];
    memset(&I, 0, sizeof(I));
    I.src = take(4ull * a.rows * a.nc); I.rows = a.rows; I.nc = a.nc;
    for (int c = 0; c < 4; ++c) I.mn[c] = 0xFFFFFFFFu;
    if (i == 0 || arrays[i - 1].group != a.group || arrays[i - 1].nc != a.nc) { dsa::EncGridGroup G; memset(&G, 0, sizeof(G)); G.first = i; G.nc = a.nc; groups.push_back(G); }
    ++groups.back().count;
    memset(&streams[i], 0, sizeof(Stream));
    streams[i].src = I.src; streams[i].vals = take(4ull * a.rows * a.nc);
  }
  std::vector<uint8_t> store(cur + 256, 0);
  uint8_t *arena = store.data();
  for (uint32_t i = 0; i < n; ++i) if (!arrays[i].v.empty()) memcpy(arena + items[i].src, arrays[i].v.data(), 4 * arrays[i].v.size());
  ASAN_POISON_MEMORY_REGION(arena, store.size());
  for (auto &rg : regions) ASAN_UNPOISON_MEMORY_REGION(arena + rg.first, rg.second);
#define SAME(cond, what) do { if (!(cond)) { fprintf(stderr, "array / group %u (%s, %u blocks): %s differ\n", i, backwards ? "backwards" : "forwards", gx, what); return 1; } } while (0)
  // step one: the bounds and the finite flag of every array
  launch(dsa::k_enc_grid_bounds, gx, n, 256, backwards, (const uint8_t *)arena, items.data(), n);
  for (uint32_t i = 0; i < n; ++i) {
    const In &a = arrays[i];
    uint32_t mn[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[4] = {0, 0, 0, 0}, bad = 0;
    for (size_t k = 0; k < a.v.size(); ++k) {
      if (!synth::f32_finite(a.v[k])) { bad = 1; continue; }
      const uint32_t key = synth::f32_order_key(a.v[k]);
      mn[k % a.nc] = std::min(mn[k % a.nc], key); mx[k % a.nc] = std::max(mx[k % a.nc], key);
    }
    SAME(items[i].nonfinite == bad, "finite flags");
    SAME(memcmp(items[i].mn, mn, sizeof(mn)) == 0 && memcmp(items[i].mx, mx, sizeof(mx)) == 0, "bounds");
  }
  // step two: the fold of every group
  const uint32_t ng = (uint32_t)groups.size();
  launch(dsa::k_enc_grid_fold, (ng + WAVE - 1) / WAVE, 1, WAVE, backwards, (const dsa::EncGridItem *)items.data(), groups.data(), ng);
  for (uint32_t i = 0; i < ng; ++i) {
    const dsa::EncGridGroup &G = groups[i];
    std::vector<const float *> ptrs;
    std::vector<uint32_t> rows;
    for (uint32_t k = G.first; k < G.first + G.count; ++k) { ptrs.push_back(arrays[k].v.empty() ? (const float *)"" : arrays[k].v.data()); rows.push_back(arrays[k].rows); }
    synth::Grid want;
    const bool any = synth::shared_grid(ptrs.data(), rows.data(), G.count, (int)G.nc, want);
    SAME((G.clean != 0) == any, "clean counts");
    SAME(memcmp(G.origin, want.origin, sizeof(want.origin)) == 0 && memcmp(&G.range, &want.range, 4) == 0, "grids");
  }
  // the chunk: every array quantised on its explicit grid, or on its group's
  for (uint32_t g = 0; g < ng; ++g)
    for (uint32_t i = groups[g].first; i < groups[g].first + groups[g].count; ++i) {
      const In &a = arrays[i];
      Stream &S = streams[i];
      S.kind = 0; S.grid_mode = 1; S.bits = a.bits; S.nc_out = a.nc; S.rows = a.rows;
      S.grid_nonfinite = S.grid_off = dsa::ENC_GRID_NO_ROW;
      memcpy(S.qmin, a.range != 0.0f ? a.origin : groups[g].origin, sizeof(S.qmin));
      S.qrange = a.range != 0.0f ? a.range : groups[g].range;
    }
  launch(dsa::k_enc_grid_quantize<Stream>, gx, n, 256, backwards, arena, streams.data(), n);
  for (uint32_t i = 0; i < n; ++i) {
    const In &a = arrays[i];
    const Stream &S = streams[i];
    synth::Grid grid;
    memset(&grid, 0, sizeof(grid));
    memcpy(grid.origin, S.qmin, sizeof(grid.origin)); grid.range = S.qrange; grid.mode = 1;
    synth::PortableAttr pa;
    pa.att_type = 0; pa.nc = pa.nc_out = (int)a.nc; pa.seq_type = 2; pa.data_type = 9; pa.grid = &grid;
    std::string want, got;
    try { synth::quantize(a.v.empty() ? (const float *)"" : a.v.data(), a.rows, (int)a.nc, (int)a.bits, pa); } catch (const std::exception &e) { want = e.what(); }
    if (S.grid_nonfinite != dsa::ENC_GRID_NO_ROW) got = synth::grid_row_message("positions", S.grid_nonfinite, false);
    else if (S.grid_off != dsa::ENC_GRID_NO_ROW) got = synth::grid_row_message("positions", S.grid_off, true);
    if (got != want) fprintf(stderr, "  device: \"%s\", host coder: \"%s\"\n", got.c_str(), want.c_str());
    SAME(got == want, "refusals");
    if (want.empty()) SAME(pa.vals.empty() || memcmp(arena + S.vals, pa.vals.data(), 4 * pa.vals.size()) == 0, "integers");
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: encgrid_host <arrays.bin>\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  std::vector<In> arrays(count);
  for (auto &a : arrays) {
    uint32_t head[4];
    if (fread(head, 4, 4, f) != 4) return 2;
    a.group = head[0]; a.nc = head[1]; a.rows = head[2]; a.bits = head[3];
    if (a.nc < 1 || a.nc > 4 || a.bits < 1 || a.bits > 20 || a.rows > (1u << 24)) return 2;
    if (fread(a.origin, 4, 4, f) != 4 || fread(&a.range, 4, 1, f) != 1) return 2;
    a.v.resize((size_t)a.rows * a.nc);
    if (!a.v.empty() && fread(a.v.data(), 4, a.v.size(), f) != a.v.size()) return 2;
  }
  fclose(f);
  for (int backwards = 0; backwards < 2; ++backwards)
    for (uint32_t gx : {1u, 3u})
      if (run(arrays, backwards != 0, gx) != 0) return 1;
  printf("encgrid: %u arrays bounded, folded and quantised alike, forwards and backwards\n", count);
  return 0;
}
