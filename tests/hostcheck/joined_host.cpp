// tests/hostcheck/joined_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The host-compilable part of the product's joined vertex arrays (draco-sharp_amd/csrc/dsa_joined_arrays.h: ja_layout_group, the
// sizing of the block, and ja_target_row / ja_store_element, the body of k_joined_arrays' gather) compiled with AddressSanitizer +
// UBSan and run on decoded part streams the Python side wrote (oracle values, portable values, the parts' rows).  The block is
// allocated with exactly the size the layout reports, so a store outside it, and a load outside a value array, is a sanitizer
// report.  Both formats and both orders, all groups in one block, the members run forwards and backwards:
//   - every array is 64-byte aligned and lies inside the reported size, no two arrays overlap;
//   - the block is filled with 0xEE first: every byte outside the rows of the arrays must still hold it afterwards;
//   - one digest line per array (FNV-1a 64 over its num_rows rows), which tests/test_hostcheck_joined.py compares with the numpy
//     concatenation / permutation of the per-part expectation; a target row at or beyond num_rows leaves its row unwritten;
//   - a group ja_layout_group refuses is reported with the reason and the member, and gathers nothing.
// Nothing here is linked into the product.
//
//   joined_host <groups.bin>   file: u32 groups, then per group u32 members, per member u32 num_points, has_faces, num_attributes,
//                              per attribute u8 att_type, data_type, nc, seq_type, q_bits, pad[3], u32 num_entries,
//                              u8 values[num_entries * stride], (seq_type != 0) i32 portable[num_entries * ncp]; then u32 rows[num_points]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../draco-sharp_amd/csrc/dsa_joined_arrays.h"

struct Att { VaAttrIn in; uint32_t q_bits = 0, num_entries = 0; std::vector<uint8_t> values; std::vector<int32_t> portable; };
struct Member { uint32_t num_points = 0, has_faces = 0; std::vector<Att> atts; std::vector<uint32_t> rows; };
typedef std::vector<Member> Group;

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static int fail(const char *what, unsigned group, int att) { printf("FAIL group %u attribute %d: %s\n", group, att, what); return 1; }
static uint64_t fnv(const uint8_t *p, size_t n) { uint64_t h = 1469598103934665603ull; for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; } return h; }

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t count = 0;
  if (!rd(f, &count, 4)) return 2;
  std::vector<Group> groups(count);
  for (Group &G : groups) {
    uint32_t members = 0;
    if (!rd(f, &members, 4)) return 2;
    G.resize(members);
    for (Member &m : G) {
      uint32_t head[3];
      if (!rd(f, head, sizeof(head))) return 2;
      m.num_points = head[0]; m.has_faces = head[1];
      m.atts.resize(head[2]);
      for (Att &A : m.atts) {
        uint8_t d[8];
        if (!rd(f, d, 8) || !rd(f, &A.num_entries, 4)) return 2;
        A.in = {d[0], d[1], d[2], d[3], VA_IDENTITY}; A.q_bits = d[4];
        A.values.resize((size_t)A.num_entries * va_dt_len(A.in.data_type) * A.in.nc);
        if (!rd(f, A.values.data(), A.values.size())) return 2;
        if (A.in.seq_type != 0) {
          A.portable.resize((size_t)A.num_entries * va_portable_nc(A.in.seq_type, A.in.nc));
          if (!rd(f, A.portable.data(), 4 * A.portable.size())) return 2;
        }
      }
      m.rows.resize(m.num_points);
      if (!rd(f, m.rows.data(), 4 * m.rows.size())) return 2;
    }
  }
  fclose(f);
  for (int format = 0; format < 2; ++format) {
    for (uint32_t mask : {0u, (1u << 0) | (1u << 2)}) {
      // ---- layout of all groups
      std::vector<JaGroup> table(count);
      std::vector<std::vector<uint32_t>> first_row(count);
      std::vector<int> why(count, JA_OK);
      uint64_t total = 0;
      for (uint32_t g = 0; g < count; ++g) {
        const Group &G = groups[g];
        std::vector<std::vector<VaAttrIn>> atts(G.size());
        std::vector<JaMemberIn> in(G.size());
        for (size_t k = 0; k < G.size(); ++k) {
          atts[k].resize(DSA_MAX_ATT);
          for (size_t a = 0; a < G[k].atts.size(); ++a) atts[k][a] = G[k].atts[a].in;
          in[k] = {atts[k].data(), (uint32_t)G[k].atts.size(), G[k].num_points, G[k].has_faces};
        }
        first_row[g].resize(G.size());
        uint32_t bad = 0;
        total = ja_layout_group(in.data(), (uint32_t)G.size(), format, mask, total, table[g], first_row[g].data(), &why[g], &bad);
        if (format == 0 && mask == 0) {
          if (why[g] != JA_OK) printf("group %u refused why %d member %u\n", g, why[g], bad);
          else { printf("group %u rows %u first", g, table[g].cap_points); for (uint32_t r : first_row[g]) printf(" %u", r); printf("\n"); }
        }
        uint64_t sum = 0;
        for (size_t k = 0; k < G.size(); ++k) { if (first_row[g][k] != sum) return fail("first_row is not the running sum", g, -1); sum += G[k].num_points; }
        if (table[g].cap_points != sum || table[g].indices != VA_NONE) return fail("rows of the group / an index array", g, -1);
      }
      printf("bytes format %d mask %u: %llu\n", format, mask, (unsigned long long)total);
      std::vector<std::pair<uint64_t, uint64_t>> spans;
      for (uint32_t g = 0; g < count; ++g) {
        const JaGroup &T = table[g];
        for (uint32_t a = 0; a < T.cap_attributes; ++a) {
          const bool masked = mask != 0 && !((mask >> groups[g][0].atts[a].in.att_type) & 1u);
          if (masked != (T.att[a].offset == VA_NONE)) return fail("the mask and the layout disagree", g, (int)a);
          if (T.att[a].map_rep != VA_IDENTITY) return fail("a map in a joined array", g, (int)a);
          if (T.att[a].offset != VA_NONE) spans.push_back({T.att[a].offset, T.att[a].offset + (uint64_t)T.att[a].stride * T.cap_points});
        }
      }
      for (auto &s : spans) if (s.first % 64 != 0 || s.second > total || s.second < s.first) return fail("array misaligned or outside the block", 0, -1);
      std::sort(spans.begin(), spans.end());
      for (size_t k = 1; k < spans.size(); ++k) if (spans[k].first < spans[k - 1].second) return fail("two arrays overlap", 0, -1);
      if (mask != 0) continue;
      // ---- the gather, element by element as the kernel's lanes run it
      for (int order = 0; order < 2; ++order) {
        for (int backwards = 0; backwards < 2; ++backwards) {
          uint8_t *block = (uint8_t *)malloc(total ? (size_t)total : 1);        // exactly the reported size: the sanitizer guards its ends
          memset(block, 0xEE, (size_t)total);
          for (uint32_t g = 0; g < count; ++g) {
            if (why[g] != JA_OK) continue;
            const Group &G = groups[g];
            const JaGroup &T = table[g];
            for (size_t kk = 0; kk < G.size(); ++kk) {
              const size_t k = backwards ? G.size() - 1 - kk : kk;
              const Member &m = G[k];
              const JaMember M = {(uint32_t)k, g, first_row[g][k], m.num_points, order == JA_ORDER_INPUT ? 0ull : JA_NO_ROWS};
              const uint32_t *rows = order == JA_ORDER_INPUT ? m.rows.data() : nullptr;
              for (uint32_t a = 0; a < T.cap_attributes; ++a) {
                const Att &A = m.atts[a];
                const VaAttr &t = T.att[a];
                AttrDesc D;
                memset(&D, 0, sizeof(D));
                D.att_type = A.in.att_type; D.data_type = A.in.data_type; D.nc = A.in.nc; D.seq_type = A.in.seq_type;
                D.nc_portable = (uint8_t)va_portable_nc(A.in.seq_type, A.in.nc); D.q_bits = (uint8_t)A.q_bits; D.num_entries = A.num_entries;
                D.source = A.in.seq_type == 0 ? SRC_BYTES : SRC_RAW;
                uint32_t ne = 0;
                if (!va_attr_written(t, D, (uint32_t)A.values.size(), (uint32_t)A.portable.size(), &ne)) continue;
                const void *src = t.kind == VA_KIND_QUANTIZED ? (const void *)A.portable.data() : (const void *)A.values.data();
                const uint32_t words = va_words(t);
                for (uint32_t pp = 0; pp < m.num_points; ++pp) {
                  const uint32_t p = backwards ? m.num_points - 1 - pp : pp, target = ja_target_row(M, rows, p);
                  if (words == 0) ja_store_element(block + t.offset, t, src, ne, T.cap_points, target, 0, p);
                  else for (uint32_t w = 0; w < words; ++w) ja_store_element(block + t.offset, t, src, ne, T.cap_points, target, w, p);
                }
              }
            }
          }
          // what lies outside the rows of the arrays is untouched; the arrays of a refused group too
          std::vector<uint8_t> covered((size_t)total, 0);
          for (uint32_t g = 0; g < count; ++g) {
            const JaGroup &T = table[g];
            for (uint32_t a = 0; a < T.cap_attributes; ++a) {
              const VaAttr &t = T.att[a];
              if (t.offset == VA_NONE) continue;
              if (why[g] == JA_OK) memset(covered.data() + t.offset, 1, (size_t)t.stride * T.cap_points);
              if (why[g] != JA_OK || backwards) continue;
              uint32_t ne = 0;
              AttrDesc D;
              memset(&D, 0, sizeof(D));
              const Att &A = groups[g][0].atts[a];
              D.data_type = A.in.data_type; D.nc = A.in.nc; D.seq_type = A.in.seq_type; D.nc_portable = (uint8_t)va_portable_nc(A.in.seq_type, A.in.nc); D.q_bits = (uint8_t)A.q_bits;
              D.source = A.in.seq_type == 0 ? SRC_BYTES : SRC_RAW;
              if (!va_attr_written(t, D, ~0u, ~0u, &ne)) { printf("group %u format %d order %d attribute %u absent\n", g, format, order, a); continue; }
              printf("group %u format %d order %d attribute %u stride %u type %u components %u digest %016llx\n", g, format, order, a, t.stride, t.data_type, t.nc,
                     (unsigned long long)fnv(block + t.offset, (size_t)t.stride * T.cap_points));
            }
          }
          for (size_t i = 0; i < (size_t)total; ++i) if (!covered[i] && block[i] != 0xEE) { free(block); return fail("a byte outside the arrays was written", 0, -1); }
          // forwards and backwards write the same block: keep the forward digest, compare the whole block
          static std::vector<uint8_t> forward;
          if (!backwards) forward.assign(block, block + total);
          else if (memcmp(forward.data(), block, (size_t)total) != 0) { free(block); return fail("the block depends on the order the members ran in", 0, -1); }
          free(block);
        }
      }
    }
  }
  printf("joined: %u groups, both formats and both orders laid out and gathered\n", count);
  return 0;
}
