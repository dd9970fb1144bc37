// tail_lifetime.hpp — what has to outlive Plan::execute when it returns at the count point, while the emit pass (the execution's TAIL) still runs on the
// plan's stream: the device blocks of that execution and the fact that a tail is in flight.  Plain C++, no HIP: the device calls are the caller's callbacks
// ("free", "wait"), so the orders that matter — execute / execute / complete, execute / mutate, destroy with a tail pending — run on the CPU under a
// sanitizer (tests/host/tail_lifetime_check.cpp).
#pragma once
#include <cstddef>
#include <mutex>
#include <vector>

namespace rdfgpu {

// The blocks of an execution whose tail may be in flight.  The store's pool knows nothing of streams and is shared by every plan of the store: a block
// handed back to it could be given to another plan, on another stream, while the tail still writes it.  So the next execution of the SAME plan retires
// them here instead.  Its own kernels run on the plan's stream, behind the tail: it may take a retired block for itself at once (take — the pool's own
// rule: an exact fit, else the smallest block up to 1.5 x the size asked for, so a steady step finds every block the pool would have given it and makes
// no device allocation).  What it does not take goes back to the pool at the first host wait that is stream-ordered behind the tail (release).
class RetiredBlocks {
 public:
  void retire(void* p, size_t bytes) { if (p) blocks_.push_back(Block{p, bytes}); }
  void* take_exact(size_t bytes) {
    for (size_t i = 0; i < blocks_.size(); i++) if (blocks_[i].bytes == bytes) return remove(i);
    return nullptr;
  }
  void* take(size_t bytes) {
    size_t best = blocks_.size();
    for (size_t i = 0; i < blocks_.size(); i++) {
      const size_t b = blocks_[i].bytes;
      if (b < bytes || b > bytes + bytes / 2) continue;
      if (best == blocks_.size() || b < blocks_[best].bytes) best = i;
    }
    return best == blocks_.size() ? nullptr : remove(best);
  }
  template <class Free> void release(Free&& free) {
    std::vector<Block> gone;
    gone.swap(blocks_);                    // (emptied first: a callback that throws leaves nothing to free twice)
    for (const Block& b : gone) free(b.p);
  }
  bool empty() const { return blocks_.empty(); }
  size_t size() const { return blocks_.size(); }

 private:
  struct Block { void* p; size_t bytes; };
  void* remove(size_t i) { void* p = blocks_[i].p; blocks_[i] = blocks_.back(); blocks_.pop_back(); return p; }
  std::vector<Block> blocks_;
};

// The pending tails of one store's plans: owner (the plan) -> the event recorded behind its tail.  A plan enters itself before execute gives up its hold
// of the store and leaves when a call of its own has completed the tail; whoever is about to free or rebuild what a tail reads (the slice tables, the
// generation's columns) waits for all of them first, holding the store exclusively, so that no new tail can start meanwhile.  The entries stay: a tail that
// somebody else waited for is still the plan's to complete.  Its own mutex, held across the waits: a plan that is being destroyed cannot take its event away
// from under a waiter.
class TailRegistry {
 public:
  void add(const void* owner, void* event) {
    std::lock_guard<std::mutex> g(mu_);
    for (Entry& e : tails_) if (e.owner == owner) { e.event = event; return; }
    tails_.push_back(Entry{owner, event});
  }
  void remove(const void* owner) {
    std::lock_guard<std::mutex> g(mu_);
    for (size_t i = 0; i < tails_.size(); i++) if (tails_[i].owner == owner) { tails_[i] = tails_.back(); tails_.pop_back(); return; }
  }
  template <class Wait> void wait_all(Wait&& wait) {
    std::lock_guard<std::mutex> g(mu_);
    for (const Entry& e : tails_) wait(e.event);
  }
  size_t pending() {
    std::lock_guard<std::mutex> g(mu_);
    return tails_.size();
  }

 private:
  struct Entry { const void* owner; void* event; };
  std::mutex mu_;
  std::vector<Entry> tails_;
};

}  // namespace rdfgpu
