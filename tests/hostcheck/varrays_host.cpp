// tests/hostcheck/varrays_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The host-compilable part of the product's vertex arrays (draco-sharp_amd/csrc/dsa_vertex_arrays.h: va_layout_mesh, the sizing of
// the block, and va_store_element / va_index_pair / va_attr_written, the body of k_vertex_arrays' gather) compiled with
// AddressSanitizer + UBSan and run on decoded meshes the Python side wrote (oracle values, portable values, point maps).  The block
// is allocated with exactly the size the layout reports, so a store outside it, and a load outside a value array, is a sanitizer
// report.  Both formats, for all meshes in one block:
//   - every array is 64-byte aligned and lies inside the reported size, no two arrays overlap;
//   - one digest line per array (FNV-1a 64 over its num_points rows), which tests/test_hostcheck_varrays.py compares with
//     values[point_map] / portable[point_map] narrowed; "absent" where the layout leaves an attribute out.
// Nothing here is linked into the product.
//
//   varrays_host <meshes.bin>   file: u32 count, then per mesh u32 num_points, cap_points, num_faces, has_faces, num_attributes,
//                               i32 faces[3 num_faces], per attribute u8 att_type, data_type, nc, seq_type, map_rep, q_bits, pad[2],
//                               u32 num_entries, u8 values[num_entries * stride], (seq_type != 0) i32 portable[num_entries * ncp],
//                               (map_rep == own index) u32 map[num_points]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../draco-sharp_amd/csrc/dsa_vertex_arrays.h"

struct Att {
  VaAttrIn in; uint32_t q_bits = 0, num_entries = 0;
  std::vector<uint8_t> values; std::vector<int32_t> portable; std::vector<uint32_t> map;
};
struct Mesh { uint32_t num_points = 0, cap_points = 0, num_faces = 0, has_faces = 0; std::vector<int32_t> faces; std::vector<Att> atts; };

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static int fail(const char *what, unsigned mesh, int att) { printf("FAIL mesh %u attribute %d: %s\n", mesh, att, what); return 1; }
static uint64_t fnv(const uint8_t *p, size_t n) { uint64_t h = 1469598103934665603ull; for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; } return h; }

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t count = 0;
  if (!rd(f, &count, 4)) return 2;
  std::vector<Mesh> meshes(count);
  for (Mesh &m : meshes) {
    uint32_t head[5];
    if (!rd(f, head, sizeof(head))) return 2;
    m.num_points = head[0]; m.cap_points = head[1]; m.num_faces = head[2]; m.has_faces = head[3];
    m.faces.resize(3 * (size_t)m.num_faces);
    if (!rd(f, m.faces.data(), 4 * m.faces.size())) return 2;
    m.atts.resize(head[4]);
    for (size_t a = 0; a < m.atts.size(); ++a) {
      Att &A = m.atts[a];
      uint8_t d[8];
      if (!rd(f, d, 8) || !rd(f, &A.num_entries, 4)) return 2;
      A.in = {d[0], d[1], d[2], d[3], d[4]}; A.q_bits = d[5];
      A.values.resize((size_t)A.num_entries * va_dt_len(A.in.data_type) * A.in.nc);
      if (!rd(f, A.values.data(), A.values.size())) return 2;
      if (A.in.seq_type != 0) {
        A.portable.resize((size_t)A.num_entries * va_portable_nc(A.in.seq_type, A.in.nc));
        if (!rd(f, A.portable.data(), 4 * A.portable.size())) return 2;
      }
      if (A.in.map_rep == a) { A.map.resize(m.num_points); if (!rd(f, A.map.data(), 4 * A.map.size())) return 2; }
    }
  }
  fclose(f);
  for (int format = 0; format < 2; ++format) {
    for (uint32_t mask : {0u, (1u << 0) | (1u << 3)}) {
      // ---- layout of the whole batch
      std::vector<VaMesh> table(count);
      uint64_t total = 0;
      for (uint32_t i = 0; i < count; ++i) {
        const Mesh &m = meshes[i];
        VaAttrIn in[DSA_MAX_ATT] = {};
        for (size_t a = 0; a < m.atts.size(); ++a) in[a] = m.atts[a].in;
        total = va_layout_mesh(in, (uint32_t)m.atts.size(), m.cap_points, m.num_faces, m.has_faces != 0, format, mask, total, table[i]);
      }
      printf("bytes format %d mask %u: %llu\n", format, mask, (unsigned long long)total);
      std::vector<std::pair<uint64_t, uint64_t>> spans;
      for (uint32_t i = 0; i < count; ++i) {
        const VaMesh &T = table[i];
        if ((T.indices != VA_NONE) != (meshes[i].has_faces != 0)) return fail("index array of a point cloud / none for a mesh", i, -1);
        if (T.indices != VA_NONE) spans.push_back({T.indices, T.indices + (uint64_t)T.cap_faces * (T.u16 ? 6 : 12)});
        if (T.u16 != (meshes[i].cap_points <= 65536u ? 1u : 0u)) return fail("index width", i, -1);
        for (uint32_t a = 0; a < T.cap_attributes; ++a) {
          const bool masked = mask != 0 && !((mask >> meshes[i].atts[a].in.att_type) & 1u);
          if (masked != (T.att[a].offset == VA_NONE)) return fail("the mask and the layout disagree", i, (int)a);
          if (T.att[a].offset != VA_NONE) spans.push_back({T.att[a].offset, T.att[a].offset + (uint64_t)T.att[a].stride * T.cap_points});
        }
      }
      for (auto &s : spans) if (s.first % 64 != 0 || s.second > total || s.second < s.first) return fail("array misaligned or outside the block", 0, -1);
      std::sort(spans.begin(), spans.end());
      for (size_t k = 1; k < spans.size(); ++k) if (spans[k].first < spans[k - 1].second) return fail("two arrays overlap", 0, -1);
      if (mask != 0) continue;
      // ---- the gather, element by element as the kernel's lanes run it
      uint8_t *block = (uint8_t *)malloc(total ? (size_t)total : 1);        // exactly the reported size: the sanitizer guards its ends
      memset(block, 0xEE, (size_t)total);
      for (uint32_t i = 0; i < count; ++i) {
        const Mesh &m = meshes[i];
        const VaMesh &T = table[i];
        const uint32_t nc = 3 * m.num_faces;
        if (T.indices != VA_NONE) {
          if (T.u16) { uint32_t *dst = (uint32_t *)(block + T.indices); for (uint32_t w = 0; w < (nc + 1) / 2; ++w) dst[w] = va_index_pair(m.faces.data(), w, nc); }
          else memcpy(block + T.indices, m.faces.data(), 4 * (size_t)nc);
          printf("mesh %u format %d indices u16 %u digest %016llx\n", i, format, T.u16, (unsigned long long)fnv(block + T.indices, (size_t)nc * (T.u16 ? 2 : 4)));
        } else printf("mesh %u format %d indices none\n", i, format);
        for (uint32_t a = 0; a < T.cap_attributes; ++a) {
          const Att &A = m.atts[a];
          const VaAttr &t = T.att[a];
          AttrDesc D;
          memset(&D, 0, sizeof(D));
          D.att_type = A.in.att_type; D.data_type = A.in.data_type; D.nc = A.in.nc; D.seq_type = A.in.seq_type;
          D.nc_portable = (uint8_t)va_portable_nc(A.in.seq_type, A.in.nc); D.q_bits = (uint8_t)A.q_bits; D.num_entries = A.num_entries;
          D.source = A.in.seq_type == 0 ? SRC_BYTES : SRC_RAW;
          uint32_t ne = 0;
          if (!va_attr_written(t, D, (uint32_t)A.values.size(), (uint32_t)A.portable.size(), &ne)) { printf("mesh %u format %d attribute %u absent\n", i, format, a); continue; }
          const std::vector<uint32_t> *map = t.map_rep == VA_IDENTITY ? nullptr : &m.atts[t.map_rep].map;
          const void *src = t.kind == VA_KIND_QUANTIZED ? (const void *)A.portable.data() : (const void *)A.values.data();
          const uint32_t words = va_words(t);
          for (uint32_t p = 0; p < m.num_points; ++p) {
            const uint32_t entry = map ? (*map)[p] : p;
            if (words == 0) va_store_element(block + t.offset, t, src, ne, p, 0, entry);
            else for (uint32_t k = 0; k < words; ++k) va_store_element(block + t.offset, t, src, ne, p, k, entry);
          }
          printf("mesh %u format %d attribute %u stride %u type %u components %u digest %016llx\n", i, format, a, t.stride, t.data_type, t.nc,
                 (unsigned long long)fnv(block + t.offset, (size_t)t.stride * m.num_points));
        }
      }
      free(block);
    }
  }
  printf("varrays: %u meshes, both formats laid out and gathered\n", count);
  return 0;
}
