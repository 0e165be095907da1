// draco-sharp_amd/csrc/dsa_spares.h
// What a context keeps between batches, and how a block is got when one is wanted: from a cache of freed blocks, else from the
// allocator, else from the allocator again once idle caches have given way.  Plain C++ over a two-function backend -- dsa_api.hip
// supplies hipMalloc / hipFree and hipHostMalloc / hipHostFree, tests/hostcheck/spares_host.cpp supplies malloc / free.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <vector>

namespace spares {

// alloc: 0 and the block, or the allocator's error code with nothing left pending (a sticky HIP error is cleared there: the
// next check behind a kernel launch would report it otherwise).
struct Backend { int (*alloc)(void **p, uint64_t bytes); void (*release)(void *p); };

// Blocks of freed batches, three at the most: two batches in flight + one being built.  hipMalloc / hipFree of tens of GB and
// pinning GBs of host memory cost as much as a decode, and both wait for the device -- with another batch in flight they would
// put the pipeline back in single file.  Every operation runs under the owner's mutex (the pool's worker threads and whichever
// thread frees a job share a context's caches); blocks are allocated outside it.
constexpr size_t kSpares = 3;
class SpareCache {
 public:
  SpareCache(std::mutex *mu, const Backend &backend) : backend(backend), mu_(mu) {}
  SpareCache(const SpareCache &) = delete;
  SpareCache &operator=(const SpareCache &) = delete;
  ~SpareCache() { drop(); }
  // best fit: the smallest block of at least `need` bytes (nullptr: none, and the cache is as it was)
  uint8_t *take(uint64_t need, uint64_t *got) {
    std::lock_guard<std::mutex> g(*mu_);
    int best = -1;
    for (size_t k = 0; k < blocks_.size(); ++k)
      if (blocks_[k].bytes >= need && (best < 0 || blocks_[k].bytes < blocks_[(size_t)best].bytes)) best = (int)k;
    if (best < 0) return nullptr;
    const Block b = blocks_[(size_t)best];
    blocks_.erase(blocks_.begin() + best);
    *got = b.bytes;
    return b.p;
  }
  void give(void *p, uint64_t bytes) {
    if (!p) return;
    std::lock_guard<std::mutex> g(*mu_);
    try { blocks_.push_back({(uint8_t *)p, bytes}); } catch (...) { backend.release(p); return; }
    while (blocks_.size() > kSpares) {       // drop the smallest
      size_t s = 0;
      for (size_t k = 1; k < blocks_.size(); ++k) if (blocks_[k].bytes < blocks_[s].bytes) s = k;
      backend.release(blocks_[s].p);
      blocks_.erase(blocks_.begin() + (ptrdiff_t)s);
    }
  }
  void drop() {
    std::lock_guard<std::mutex> g(*mu_);
    for (const Block &b : blocks_) backend.release(b.p);
    blocks_.clear();
  }
  const Backend backend;

 private:
  struct Block { uint8_t *p; uint64_t bytes; };
  std::vector<Block> blocks_;
  std::mutex *mu_;
};

// What is asked of the allocator for a block of `need` bytes that no cached block serves.
using Grow = uint64_t (*)(uint64_t need);
inline uint64_t grow_exact(uint64_t need) { return need; }
inline uint64_t grow_half(uint64_t need) { return need + need / 2; }            // a slowly growing sequence of batches does not re-pin every time
inline uint64_t grow_floor256(uint64_t need) { return std::max<uint64_t>(need, 256); }   // an empty batch still has a block

struct Acquired { uint8_t *p; uint64_t cap; int err; };

// A block of at least `need` bytes: from `cache`; else from its allocator; else -- what the context keeps idle may be what is in
// the way -- once more after the caches of `give_way` were emptied in that order, and, where that did not help either, once more
// after `last_resort`.  An empty `give_way`: no second attempt.
inline Acquired acquire(SpareCache &cache, uint64_t need, Grow grow, std::initializer_list<SpareCache *> give_way = {},
                        const std::function<void()> &last_resort = nullptr) {
  Acquired a{nullptr, 0, 0};
  if ((a.p = cache.take(need, &a.cap))) return a;
  void *p = nullptr;
  a.cap = grow(need);
  a.err = cache.backend.alloc(&p, a.cap);
  if (a.err && give_way.size()) {
    for (SpareCache *c : give_way) c->drop();
    a.err = cache.backend.alloc(&p, a.cap);
    if (a.err && last_resort) { last_resort(); a.err = cache.backend.alloc(&p, a.cap); }
  }
  if (a.err) { p = nullptr; a.cap = 0; }
  a.p = (uint8_t *)p;
  return a;
}

}  // namespace spares
