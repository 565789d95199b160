// otg_dispatch_queue.hpp — the two thread-safe containers of the file dispatchers (dispatch.hip).  They need nothing from HIP or from
// otter_gpu.h, so tests/dispatch_queue_driver.cpp exercises them on the CPU under ThreadSanitizer.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <map>
#include <mutex>
#include <utility>

// Items from one producer stage to the next: push blocks while `cap` items wait, pop blocks while none does.
template <class T>
class BoundedQueue {
 public:
  explicit BoundedQueue(size_t cap) : cap_(cap) {}
  bool push(T v) {
    std::unique_lock<std::mutex> lk(m_);
    cv_space_.wait(lk, [&] { return q_.size() < cap_ || closed_; });
    if (closed_) return false;
    q_.push_back(std::move(v));
    cv_item_.notify_one();
    return true;
  }
  bool pop(T& out) {
    std::unique_lock<std::mutex> lk(m_);
    cv_item_.wait(lk, [&] { return !q_.empty() || done_ || closed_; });
    if (closed_ || q_.empty()) return false;
    out = std::move(q_.front());
    q_.pop_front();
    cv_space_.notify_one();
    return true;
  }
  void finish() { std::lock_guard<std::mutex> lk(m_); done_ = true; cv_item_.notify_all(); }           // no more items will come
  void abort() { std::lock_guard<std::mutex> lk(m_); closed_ = true; cv_item_.notify_all(); cv_space_.notify_all(); }
 private:
  std::mutex m_;
  std::condition_variable cv_item_, cv_space_;
  std::deque<T> q_;
  size_t cap_;
  bool done_ = false, closed_ = false;
};

// The finished batches of one shard on their way to the writer, which takes them strictly in order 0, 1, 2, ... while the shard's threads
// finish them in any order.  `status` is the job's: a value other than 0 means the job has failed, and then nobody waits here any longer
// (whoever fails the job need not know this object: waiters look at `status` every 50 ms).
template <class T>
class OrderedOutput {
 public:
  OrderedOutput(const std::atomic<int>& status, uint32_t n_batches) : status_(status), n_batches_(n_batches) {}
  uint32_t n_batches() const { return n_batches_; }
  void set_cap(size_t cap) { std::lock_guard<std::mutex> lk(m_); cap_ = cap; }
  // Back-pressure: the writer drains the shards one after the other, so a shard it has not reached yet may hold back `cap` finished
  // batches and no more (host memory stays bounded by the batch size, not by the shard).  The batch the writer wants next always gets
  // in — the threads of a shard finish out of order, and that batch may be the last one to arrive.
  void deliver(uint32_t k, T&& payload) {
    {
      std::unique_lock<std::mutex> lk(m_);
      while (!(ready_.size() < cap_ || k == next_ || status_.load() != 0)) cv_.wait_for(lk, std::chrono::milliseconds(50));
      ready_.emplace(k, std::move(payload));
    }
    cv_.notify_all();
  }
  // the writer's side: batch k (= the one after the last it took); false when the job failed before that batch arrived
  bool take(uint32_t k, T& out) {
    {
      std::unique_lock<std::mutex> lk(m_);
      while (!ready_.count(k) && status_.load() == 0) cv_.wait_for(lk, std::chrono::milliseconds(50));
      auto it = ready_.find(k);
      if (it == ready_.end()) return false;
      out = std::move(it->second);
      ready_.erase(it);
      next_ = k + 1;
    }
    cv_.notify_all();                       // room for the shard's threads
    return true;
  }
  size_t held() { std::lock_guard<std::mutex> lk(m_); return ready_.size(); }
  void wake() { cv_.notify_all(); }         // after `status` changed: spares the waiters the rest of their 50 ms
 private:
  const std::atomic<int>& status_;
  const uint32_t n_batches_;
  std::mutex m_;
  std::condition_variable cv_;
  std::map<uint32_t, T> ready_;             // batch index -> payload
  uint32_t next_ = 0;                       // the batch the writer takes next
  size_t cap_ = 3;                          // finished batches the shard may hold back
};
