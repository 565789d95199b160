// Host driver of tests/test_dispatch_queue.py: the thread-safe containers of the file dispatchers (otter_amd/csrc/otg_dispatch_queue.hpp,
// the only project header included) under ThreadSanitizer.  Every scenario runs under a watchdog: a waiter that is never released makes
// the driver exit 3 instead of hanging.  Exit 0 and no sanitizer report = pass.
#include "otg_dispatch_queue.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

namespace {

const int OK = 0, FAILED = -2;
int g_bad = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); ++g_bad; } } while (0)

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

// `producers` threads finish the batches 0..n-1 for one writer, cap < n.  As the hot-path threads of a shard do, each takes the next batch
// number from a common counter (so the lowest unfinished batch is always in the hands of a thread that is not waiting for room) and
// needs delay_us(k) for it, so that the batches arrive out of order.
template <class Delay>
void out_of_order(uint32_t n, uint32_t producers, size_t cap, Delay delay_us)
{
  std::atomic<int> status{OK};
  OrderedOutput<std::string> out(status, n);
  out.set_cap(cap);
  std::atomic<size_t> max_held{0};
  std::atomic<uint32_t> counter{0};
  std::vector<std::thread> th;
  for (uint32_t p = 0; p < producers; ++p)
    th.emplace_back([&] {
      for (uint32_t k; (k = counter.fetch_add(1)) < n;) {
        std::this_thread::sleep_for(std::chrono::microseconds(delay_us(k)));
        out.deliver(k, "batch " + std::to_string(k));
        size_t h = out.held(), m = max_held.load();
        while (h > m && !max_held.compare_exchange_weak(m, h)) {}
      }
    });
  std::vector<uint32_t> seen;
  std::string text;
  for (uint32_t k = 0; k < out.n_batches(); ++k) {
    CHECK(out.take(k, text));
    CHECK(text == "batch " + std::to_string(k));
    seen.push_back(k);
    std::this_thread::sleep_for(std::chrono::microseconds(200));      // a slow writer: the producers run into the cap
  }
  for (auto& t : th) t.join();
  CHECK(seen.size() == n);
  CHECK(out.held() == 0);
  // never more than `cap` held back, except for the one extra batch that is the writer's next
  CHECK(max_held.load() <= cap + 1);
}

// the batch the writer wants arrives last: the others fill the output up to its cap, and batch 0 still gets in
void wanted_batch_last()
{
  std::atomic<int> status{OK};
  const uint32_t n = 4;
  OrderedOutput<int> out(status, n);
  out.set_cap(n - 1);
  for (uint32_t k = 1; k < n; ++k) out.deliver(k, (int)k);            // room for all three
  CHECK(out.held() == n - 1);
  std::thread last([&] { std::this_thread::sleep_for(std::chrono::milliseconds(20)); out.deliver(0, 0); });     // full, but 0 is `next`
  int v = -1;
  for (uint32_t k = 0; k < n; ++k) { CHECK(out.take(k, v)); CHECK(v == (int)k); }
  last.join();
}

// a failure while producers are blocked on a full output and the writer on a missing batch: all of them return within a bounded wait
void failure_releases_everyone()
{
  std::atomic<int> status{OK};
  OrderedOutput<int> out(status, 8);
  out.set_cap(2);
  out.deliver(2, 2); out.deliver(3, 3);                               // full; batch 0 never comes
  std::atomic<int> returned{0};
  std::vector<std::thread> th;
  for (uint32_t k = 4; k < 7; ++k) th.emplace_back([&, k] { out.deliver(k, (int)k); ++returned; });           // blocked: full and not next
  bool took = true;
  std::thread writer([&] { int v; took = out.take(0, v); ++returned; });                                       // blocked: 0 is missing
  std::this_thread::sleep_for(std::chrono::milliseconds(120));
  CHECK(returned.load() == 0);
  const auto t0 = Clock::now();
  status.store(FAILED);                                               // as Job::fail does: nobody notifies, the waiters poll
  for (auto& t : th) t.join();
  writer.join();
  CHECK(!took);
  CHECK(returned.load() == 4);
  CHECK(ms_since(t0) < 5000.0);
  // and with wake() nobody waits out its poll interval either (no assertion on time: the call must simply be safe next to waiters)
  out.wake();
}

void queue_finish_and_abort()
{
  {
    BoundedQueue<int> q(8);
    for (int i = 0; i < 5; ++i) CHECK(q.push(i));
    q.finish();                                                       // items still queued: all are popped, then pop reports the end
    int v = -1;
    for (int i = 0; i < 5; ++i) { CHECK(q.pop(v)); CHECK(v == i); }
    CHECK(!q.pop(v));
  }
  {
    BoundedQueue<int> q(1);
    CHECK(q.push(1));
    bool pushed = true;
    std::thread producer([&] { pushed = q.push(2); });                // blocked: the queue is full
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
    q.abort();
    producer.join();
    CHECK(!pushed);
    int v = -1;
    CHECK(!q.pop(v));
    CHECK(!q.push(3));
  }
  {
    BoundedQueue<int> q(2);                                           // a consumer blocked on an empty queue is released by finish
    bool popped = true;
    std::thread consumer([&] { int v; popped = q.pop(v); });
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
    q.finish();
    consumer.join();
    CHECK(!popped);
  }
  {
    BoundedQueue<int> q(2);                                           // producer and consumer through a queue smaller than the stream
    long long sum = 0;
    std::thread consumer([&] { int v; while (q.pop(v)) sum += v; });
    for (int i = 1; i <= 1000; ++i) CHECK(q.push(i));
    q.finish();
    consumer.join();
    CHECK(sum == 500500);
  }
}

} // namespace

int main()
{
  std::atomic<bool> done{false};
  std::thread watchdog([&] {
    for (int i = 0; i < 300 && !done.load(); ++i) std::this_thread::sleep_for(std::chrono::milliseconds(100));
    if (!done.load()) { fprintf(stderr, "watchdog: a scenario did not return within 30 s\n"); _Exit(3); }
  });
  out_of_order(24, 3, 3, [](uint32_t) { return 0; });
  out_of_order(24, 3, 2, [](uint32_t k) { return ((k * 7 + 5) % 24) * 100; });
  out_of_order(24, 4, 2, [](uint32_t k) { return k % 4 == 0 ? 3000 : 100; });          // every fourth batch is slow: the others pile up behind it
  out_of_order(8, 8, 3, [](uint32_t k) { return (8 - k) * 2000; });                     // one thread per batch, the writer's batch 0 arrives last
  wanted_batch_last();
  failure_releases_everyone();
  queue_finish_and_abort();
  done.store(true);
  watchdog.join();
  if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
  printf("ok\n");
  return 0;
}
