// tail_lifetime_check.cpp — the retired blocks and the registry of pending tails (rdf-fusion_amd/csrc/tail_lifetime.hpp) driven without a device, through the
// orders Plan::execute, Plan::complete, ~Plan and the store's mutations put them in.  A model plan follows the engine's protocol step for step; the pool, the
// stream and the events are fakes that know which blocks a running tail still writes, so the one rule that matters can be asserted where it would break:
// no block reaches the shared pool, and no table is freed, while a tail that uses it is in flight.  Built with -fsanitize=address,undefined by
// `make tail-lifetime-check SANITIZE=1`: a block freed twice, kept for ever or touched after its free is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <thread>
#include <vector>

#include "../../rdf-fusion_amd/csrc/tail_lifetime.hpp"

using namespace rdfgpu;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

// the store's pool: blocks are real heap memory, so that the sanitizer sees every one of them
struct Pool {
  std::multiset<std::pair<size_t, void*>> cached; std::set<void*> live; std::vector<struct Stream*> streams; int mallocs = 0;
  bool in_flight(void* p) const;
  void* alloc(size_t bytes) {
    void* p = nullptr;
    for (auto it = cached.begin(); it != cached.end(); ++it) if (it->first == bytes) { p = it->second; cached.erase(it); break; }
    if (!p) { p = std::malloc(bytes); mallocs++; }
    live.insert(p);
    return p;
  }
  void free(void* p, size_t bytes) {
    CHECK(live.count(p) == 1);
    CHECK(!in_flight(p));                            // the rule: the pool is shared with other streams
    live.erase(p); cached.insert({bytes, p});
  }
  ~Pool() { CHECK(live.empty()); for (auto& c : cached) std::free(c.second); }
};

// a stream with one event behind the tail: "waiting" ends whatever is in flight on it
struct Stream {
  std::set<void*> in_flight; bool tables_in_use = false; int waits = 0;
  void wait() { in_flight.clear(); tables_in_use = false; waits++; }
};

bool Pool::in_flight(void* p) const { for (const Stream* s : streams) if (s->in_flight.count(p)) return true; return false; }

struct Store {
  Pool pool; TailRegistry tails; bool tables = true;
  bool tables_in_use() const { for (const Stream* s : pool.streams) if (s->tables_in_use) return true; return false; }
  size_t blocks_in_flight() const { size_t n = 0; for (const Stream* s : pool.streams) n += s->in_flight.size(); return n; }
  void mutate() {      // extend / remove / drop_tables: holds the store exclusively, waits for every pending tail, then frees the tables
    tails.wait_all([](void* ev) { static_cast<Stream*>(ev)->wait(); });
    CHECK(!tables_in_use());
    tables = false;
  }
};

constexpr size_t kBlock = 4096;
struct Plan {
  Store& st; Stream s; std::vector<void*> allocs; RetiredBlocks retired; bool tail_pending = false;
  explicit Plan(Store& store) : st(store) { st.pool.streams.push_back(&s); }
  void* scratch() {
    void* p = retired.empty() ? nullptr : retired.take_exact(kBlock);
    if (!p && !retired.empty()) p = retired.take(kBlock);
    if (!p) p = st.pool.alloc(kBlock);
    allocs.push_back(p);
    return p;
  }
  void tail_waited() { retired.release([&](void* p) { st.pool.free(p, kBlock); }); }
  void execute(bool early, int blocks = 3) {
    const bool behind = tail_pending;
    if (behind) { for (void* p : allocs) retired.retire(p, kBlock); allocs.clear(); }
    else { s.wait(); for (void* p : allocs) st.pool.free(p, kBlock); allocs.clear(); }
    st.tables = true;
    for (int i = 0; i < blocks; i++) static_cast<char*>(scratch())[0] = 1;   // (the front passes write their scratch: behind the tail on the same stream)
    if (early) {   // the count wait: ordered behind the predecessor's tail, in front of this execution's
      if (behind) { s.wait(); tail_waited(); }     // (what this execution took over is in flight again at once: its own tail)
      for (void* p : allocs) s.in_flight.insert(p);
      s.tables_in_use = true;
      tail_pending = true; st.tails.add(this, &s);
    } else {
      s.wait();
      if (behind) { tail_waited(); tail_pending = false; st.tails.remove(this); }
    }
  }
  void complete() {
    if (!tail_pending) return;
    s.wait(); tail_pending = false; st.tails.remove(this); tail_waited();
  }
  ~Plan() {
    complete(); s.wait(); st.tails.remove(this); tail_waited();
    for (void* p : allocs) st.pool.free(p, kBlock);
    for (size_t i = 0; i < st.pool.streams.size(); i++) if (st.pool.streams[i] == &s) { st.pool.streams.erase(st.pool.streams.begin() + i); break; }
  }
};

static void execute_execute_complete() {
  Store st;
  {
    Plan p(st);
    p.execute(true);
    CHECK(p.tail_pending && st.tails.pending() == 1 && st.blocks_in_flight() == 3);
    const int mallocs = st.pool.mallocs;
    p.execute(true);                                  // behind the tail: no wait for the stream, the predecessor's blocks taken over, none allocated
    CHECK(st.pool.mallocs == mallocs && p.retired.empty() && st.tails.pending() == 1);
    p.execute(true, 2);                               // one block fewer: the third goes back to the pool at the count wait, not before
    CHECK(p.retired.empty() && st.pool.cached.size() == 1 && st.pool.mallocs == mallocs);
    p.complete();
    CHECK(!p.tail_pending && st.tails.pending() == 0 && st.blocks_in_flight() == 0);
    const int waits = p.s.waits;
    p.complete();                                     // idempotent
    CHECK(p.s.waits == waits);
    p.execute(false);                                 // the parent's route after an early one, and an early one after it
    p.execute(true);
    p.execute(false);
    CHECK(!p.tail_pending && st.tails.pending() == 0 && p.retired.empty());
  }
  CHECK(st.pool.live.empty());
}

static void two_plans_interleaved() {
  Store st;
  {
    Plan a(st), b(st);
    a.execute(true); b.execute(true); a.execute(true); b.execute(true);   // (Pool::free asserts that neither is handed a block the other's tail writes)
    CHECK(st.tails.pending() == 2);
    a.complete(); b.complete();
    CHECK(st.tails.pending() == 0);
  }
  CHECK(st.pool.live.empty());
}

static void execute_mutate() {
  Store st;
  Plan p(st);
  p.execute(true);
  st.mutate();                                        // waits for the tail before the tables go
  CHECK(!st.tables && st.blocks_in_flight() == 0);
  CHECK(p.tail_pending && st.tails.pending() == 1);   // somebody else's wait does not complete the plan's tail
  p.complete();
  CHECK(st.tails.pending() == 0);
  p.execute(true);                                    // rebuilds, early again
  st.mutate();
  p.execute(true);
  p.complete();
}

static void destroy_with_a_tail_pending() {
  Store st;
  {
    Plan p(st);
    p.execute(true);
    p.execute(true);
    CHECK(p.tail_pending);
  }
  CHECK(st.tails.pending() == 0 && st.pool.live.empty() && st.blocks_in_flight() == 0);
  st.mutate();                                        // nothing left to wait for
}

// The registry alone under two threads: a mutator waits for all tails while plans enter and leave (the sanitizer's and the mutex's business; the counts are asserted).
static void registry_under_threads() {
  TailRegistry reg;
  static Stream streams[8];
  std::thread owner([&] { for (int r = 0; r < 2000; r++) { reg.add(&streams[r % 8], &streams[r % 8]); if (r % 3) reg.remove(&streams[(r + 5) % 8]); } });
  std::thread mutator([&] { for (int r = 0; r < 2000; r++) reg.wait_all([](void* ev) { static_cast<Stream*>(ev)->waits++; }); });
  owner.join(); mutator.join();
  for (Stream& s : streams) reg.remove(&s);
  CHECK(reg.pending() == 0);
  reg.add(&streams[0], &streams[0]); reg.add(&streams[0], &streams[1]);   // one entry per owner: the second add replaces the event
  int seen = 0;
  reg.wait_all([&](void* ev) { seen++; CHECK(ev == &streams[1]); });
  CHECK(seen == 1 && reg.pending() == 1);
}

static void retired_blocks_alone() {
  RetiredBlocks r;
  char a[1], b[1], c[1];
  r.retire(a, 1024); r.retire(b, 4096); r.retire(c, 1536); r.retire(nullptr, 64);
  CHECK(r.size() == 3);
  CHECK(r.take_exact(2048) == nullptr);
  CHECK(r.take(2048) == nullptr);                     // 4096 is wastefully large for 2048 (> 1.5 x), the others too small
  CHECK(r.take(1024) == a);                           // the smallest that fits
  CHECK(r.take(1024) == c);                           // 1536 <= 1.5 x 1024
  CHECK(r.take(4096) == b && r.empty());
  int freed = 0;
  r.retire(a, 1); r.retire(b, 2);
  r.release([&](void*) { freed++; });
  r.release([&](void*) { freed++; });
  CHECK(freed == 2 && r.empty());
}

int main() {
  execute_execute_complete();
  two_plans_interleaved();
  execute_mutate();
  destroy_with_a_tail_pending();
  registry_under_threads();
  retired_blocks_alone();
  std::printf("\n%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
