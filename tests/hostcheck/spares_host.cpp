// tests/hostcheck/spares_host.cpp
// The cache policy of a decode context (draco-sharp_amd/csrc/dsa_spares.h) over malloc / free, under AddressSanitizer + UBSan with
// leak detection on: best fit, three blocks kept, and every row of the table of dsa_api.hip's blocks -- which cache a block comes
// from, what is asked of the allocator, which caches give way in which order before the one retry, and the arena's last resort --
// with none, the first, the first two and every allocation failing.  A block neither cached nor released fails the run.
#include <stdio.h>
#include <stdlib.h>

#include <thread>

#include "../../draco-sharp_amd/csrc/dsa_spares.h"

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
  } while (0)

namespace {

// what happened, in order: an allocation asked for (its size follows), a release by cache k, the last resort
enum { EV_ALLOC = -1, EV_LAST_RESORT = -2 };
std::vector<long long> events;
std::mutex count_mu;                 // (the counters are touched by the threads of the concurrency check)
int fail_next = 0;
long long allocs = 0, releases = 0;

int test_alloc(void **p, uint64_t bytes) {
  std::lock_guard<std::mutex> g(count_mu);
  events.push_back(EV_ALLOC);
  events.push_back((long long)bytes);
  if (fail_next > 0) { --fail_next; return 2; }          // (the number of hipErrorOutOfMemory)
  *p = malloc(bytes ? bytes : 1);
  ++allocs;
  return 0;
}
template <int K>
void test_release(void *p) {
  std::lock_guard<std::mutex> g(count_mu);
  events.push_back(K);
  ++releases;
  free(p);
}
template <int K> constexpr spares::Backend backend() { return {test_alloc, test_release<K>}; }

void *block(uint64_t bytes) { void *p = nullptr; CHECK(test_alloc(&p, bytes) == 0); return p; }
std::vector<uint64_t> drain(spares::SpareCache &c) {     // what a cache holds, smallest first; released
  std::vector<uint64_t> sizes;
  uint64_t got = 0;
  while (uint8_t *p = c.take(0, &got)) { sizes.push_back(got); c.backend.release(p); }
  return sizes;
}

void best_fit() {
  std::mutex mu;
  spares::SpareCache c(&mu, backend<0>());
  void *b100 = block(100), *b300 = block(300), *b200 = block(200);
  c.give(b100, 100); c.give(b300, 300); c.give(b200, 200);
  uint64_t got = 77;
  CHECK(c.take(400, &got) == nullptr && got == 77);       // nothing fits: the cache is as it was
  CHECK(c.take(150, &got) == (uint8_t *)b200 && got == 200);
  CHECK(c.take(150, &got) == (uint8_t *)b300 && got == 300);
  CHECK(c.take(100, &got) == (uint8_t *)b100 && got == 100);
  CHECK(c.take(0, &got) == nullptr);
  free(b100); free(b200); free(b300);
  releases += 3;
}

void three_are_kept() {
  const int orders[4][4] = {{4, 3, 2, 1}, {1, 2, 3, 4}, {2, 4, 1, 3}, {3, 1, 4, 2}};
  for (const auto &order : orders) {
    std::mutex mu;
    spares::SpareCache c(&mu, backend<0>());
    const long long before = releases;
    for (int k = 0; k < 4; ++k) {
      c.give(nullptr, 1000);                              // ignored
      c.give(block((uint64_t)order[k]), (uint64_t)order[k]);
    }
    CHECK(releases == before + 1);                        // the smallest, and only it
    CHECK((drain(c) == std::vector<uint64_t>{2, 3, 4}));
  }
  std::mutex mu;
  spares::SpareCache c(&mu, backend<0>());
  c.give(nullptr, 8);
  CHECK(drain(c).empty());
  {   // what a cache still holds when it goes is released with it
    spares::SpareCache d(&mu, backend<0>());
    d.give(block(16), 16);
    d.drop();
    d.give(block(32), 32);
  }
}

// the blocks of a batch, as dsa_api.hip gets them (caches: 0 arenas, 1 packed blocks, 2 vertex-array blocks, 3 mirrors, 4 descriptor zones)
// get: the call as dsa_api.hip makes it; the other fields: what the table says of it
using Caches = spares::SpareCache *const *;
struct Row { const char *name; int cache; uint64_t (*asked)(uint64_t need); std::vector<int> give_way; bool last_resort; spares::Acquired (*get)(Caches c, uint64_t need); };
uint64_t exactly(uint64_t need) { return need; }
uint64_t and_a_half(uint64_t need) { return need + need / 2; }
uint64_t at_least_256(uint64_t need) { return need < 256 ? 256 : need; }
const Row rows[] = {
    {"arena", 0, exactly, {0}, true, [](Caches c, uint64_t need) { return spares::acquire(*c[0], need, spares::grow_exact, {c[0]}, [] { events.push_back(EV_LAST_RESORT); }); }},
    {"packed block", 1, exactly, {1, 0}, false, [](Caches c, uint64_t need) { return spares::acquire(*c[1], need, spares::grow_exact, {c[1], c[0]}); }},
    {"vertex-array block", 2, exactly, {2, 1, 0}, false, [](Caches c, uint64_t need) { return spares::acquire(*c[2], need, spares::grow_exact, {c[2], c[1], c[0]}); }},
    {"host mirror", 3, at_least_256, {3}, false, [](Caches c, uint64_t need) { return spares::acquire(*c[3], need, spares::grow_floor256, {c[3]}); }},
    {"descriptor landing zone", 4, and_a_half, {}, false, [](Caches c, uint64_t need) { return spares::acquire(*c[4], need, spares::grow_half); }},
    {"vertex-array table staging", 4, exactly, {}, false, [](Caches c, uint64_t need) { return spares::acquire(*c[4], need, spares::grow_exact); }},
};

void one_row(const Row &r, uint64_t need, int failing) {
  std::mutex mu;
  spares::SpareCache c0(&mu, backend<0>()), c1(&mu, backend<1>()), c2(&mu, backend<2>()), c3(&mu, backend<3>()), c4(&mu, backend<4>());
  spares::SpareCache *caches[5] = {&c0, &c1, &c2, &c3, &c4};
  for (spares::SpareCache *c : caches) c->give(block(8), 8);        // idle blocks, too small to serve the request
  const uint64_t ask = r.asked(need);
  std::vector<long long> want = {EV_ALLOC, (long long)ask};
  const bool retried = failing >= 1 && !r.give_way.empty(), resorted = retried && failing >= 2 && r.last_resort;
  if (retried) { for (int k : r.give_way) want.push_back(k); want.push_back(EV_ALLOC); want.push_back((long long)ask); }
  if (resorted) { want.push_back(EV_LAST_RESORT); want.push_back(EV_ALLOC); want.push_back((long long)ask); }
  const bool ok = failing < 1 + (retried ? 1 : 0) + (resorted ? 1 : 0);
  events.clear();
  fail_next = failing;
  const spares::Acquired a = r.get(caches, need);
  fail_next = 0;
  if (events != want) {
    fprintf(stderr, "%s, %d allocations failing: events", r.name, failing);
    for (long long e : events) fprintf(stderr, " %lld", e);
    fprintf(stderr, "\n");
    exit(1);
  }
  if (ok) { CHECK(a.err == 0 && a.p != nullptr && a.cap == ask); if (ask) { a.p[0] = 1; a.p[ask - 1] = 2; } }
  else CHECK(a.err == 2 && a.p == nullptr && a.cap == 0);
  for (int k = 0; k < 5; ++k) {          // the caches that gave way are empty, every other one holds what it held
    bool gave = false;
    for (int g : r.give_way) gave = gave || g == k;
    const std::vector<uint64_t> held = drain(*caches[k]);
    CHECK(held == (retried && gave ? std::vector<uint64_t>{} : std::vector<uint64_t>{8}));
  }
  caches[r.cache]->give(a.p, a.cap);      // (a failed request gives nothing back)
}

void every_row() {
  for (const Row &r : rows)
    for (int failing = 0; failing <= 3; ++failing)
      for (uint64_t need : {1000ull, 100ull, 9ull}) one_row(r, need, failing);
  // a cached block that is large enough: its own size, and the allocator is not asked
  for (const Row &r : rows) {
    std::mutex mu;
    spares::SpareCache c(&mu, backend<0>());
    void *big = block(5000);
    c.give(block(600), 600); c.give(big, 5000); c.give(block(900), 900);
    events.clear();
    fail_next = 1;
    spares::SpareCache *const same[5] = {&c, &c, &c, &c, &c};
    const spares::Acquired a = r.get(same, 1000);
    CHECK(a.err == 0 && a.p == (uint8_t *)big && a.cap == 5000 && events.empty() && fail_next == 1);
    fail_next = 0;
    c.give(a.p, a.cap);
  }
}

// two threads give to and take from one cache through the shared mutex; every block is released exactly once (a second free or
// a block forgotten stops the run)
void two_threads() {
  std::mutex mu;
  spares::SpareCache c(&mu, backend<0>());
  auto body = [&c](unsigned seed) {
    for (int round = 0; round < 4000; ++round) {
      seed = seed * 1664525u + 1013904223u;
      const uint64_t need = 1 + (seed >> 16) % 512;
      uint64_t got = 0;
      uint8_t *p = c.take(need, &got);
      if (!p) { void *q = nullptr; CHECK(test_alloc(&q, need) == 0); p = (uint8_t *)q; got = need; }
      p[0] = (uint8_t)round; p[got - 1] = (uint8_t)seed;
      if ((seed >> 8) % 4 == 0) c.backend.release(p); else c.give(p, got);
    }
  };
  std::thread other(body, 1u);
  body(2u);
  other.join();
  c.drop();
  CHECK(drain(c).empty());
}

}  // namespace

int main() {
  best_fit();
  three_are_kept();
  every_row();
  two_threads();
  CHECK(allocs == releases);
  printf("spares: best fit, three kept, %zu rows x 4 failure counts, two threads: %lld blocks, each released once\n", sizeof(rows) / sizeof(rows[0]), allocs);
  return 0;
}
