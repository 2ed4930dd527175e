// The process-wide IO worker pool: parallel pread/pwrite/memcpy spans for the
// GPU engine's file IO (ext.cpp) and for the staged upload's background
// thread (hip/stage_upload.hip). One pool, shared: the header-defined
// instance() is a single object across the extension's translation units.
#pragma once

#include <fcntl.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

namespace tfrec {

// ---------------------------------------------------------------------------
// Parallel file IO: persistent pread/pwrite worker pool. A single-threaded
// write() to tmpfs tops out at ~9 GB/s (one kernel memcpy); splitting each
// chunk across workers scales that with cores. Used by the GPU engine to keep
// file IO off the critical path of the H2D/D2H pipeline
// (spark_tfrecord_amd/engine/gpu.py). Replaces what the reference delegates
// to Hadoop FS streams (DefaultSource.scala:118-136).
// ---------------------------------------------------------------------------

class IOPool {
 public:
  static IOPool& instance() {
    // leaked on purpose: workers block on the cv forever; destructing the
    // mutex/cv under them at exit would be UB
    // 8 workers: 14 bought nothing on the staged write or the staged read
    // (profiles/RESULTS.md r12, r13)
    static IOPool* pool = new IOPool(8);
    return *pool;
  }

  // op: false=read, true=write. Splits [off, off+n) across the workers and
  // blocks until all spans complete. Returns 0 or -errno.
  int run(bool is_write, int fd, uint8_t* ptr, int64_t n, int64_t off) {
    return run_spans(n, [=](int64_t o, int64_t m) {
      return is_write ? do_write(fd, ptr + o, m, off + o)
                      : do_read(fd, ptr + o, m, off + o);
    });
  }

  template <typename Fn>
  int run_spans(int64_t n, Fn&& fn) {
    return run_parts(n, 64 << 10, std::forward<Fn>(fn));
  }

  // Splits [0, n) into per-worker ranges of at least min_span and runs
  // fn(offset, count) on the pool; fn returns 0 or an error code (first
  // nonzero wins). Used for byte IO spans AND record ranges.
  template <typename Fn>
  int run_parts(int64_t n, int64_t min_span, Fn&& fn) {
    if (n <= 0) return 0;
    int nspan = (int)nthreads_;
    int64_t span = (n + nspan - 1) / nspan;
    if (span < min_span) {
      nspan = (int)((n + min_span - 1) / min_span);
      if (nspan < 1) nspan = 1;
      span = (n + nspan - 1) / nspan;
    }
    if (nspan == 1) return fn((int64_t)0, n);  // run inline, skip the pool
    if (getenv("TFREC_POOL_DEBUG"))
      fprintf(stderr, "[pool] n=%lld nspan=%d span=%lld\n", (long long)n,
              nspan, (long long)span);
    std::atomic<int> err{0};
    std::atomic<int> left{nspan};
    {
      std::unique_lock<std::mutex> lk(mu_);
      for (int t = 0; t < nspan; ++t) {
        int64_t o = (int64_t)t * span;
        int64_t m = std::min(span, n - o);
        tasks_.push_back([=, &err, &left] {
          int e = fn(o, m);
          if (e) err.store(e, std::memory_order_relaxed);
          if (left.fetch_sub(1) == 1) {
            std::lock_guard<std::mutex> dl(done_mu_);
            done_cv_.notify_all();
          }
        });
      }
      cv_.notify_all();
    }
    std::unique_lock<std::mutex> dl(done_mu_);
    done_cv_.wait(dl, [&] { return left.load() == 0; });
    return err.load();
  }

 private:
  explicit IOPool(int n) : nthreads_(n) {
    for (int i = 0; i < n; ++i)
      workers_.emplace_back([this] { worker(); });
  }

  static int do_write(int fd, const uint8_t* p, int64_t n, int64_t off) {
    while (n > 0) {
      ssize_t w = ::pwrite(fd, p, (size_t)n, (off_t)off);
      if (w < 0) {
        if (errno == EINTR) continue;
        return -errno;
      }
      p += w;
      n -= w;
      off += w;
    }
    return 0;
  }

  static int do_read(int fd, uint8_t* p, int64_t n, int64_t off) {
    while (n > 0) {
      ssize_t r = ::pread(fd, p, (size_t)n, (off_t)off);
      if (r < 0) {
        if (errno == EINTR) continue;
        return -errno;
      }
      if (r == 0) return -EIO;  // unexpected EOF
      p += r;
      n -= r;
      off += r;
    }
    return 0;
  }

  void worker() {
    for (;;) {
      std::function<void()> task;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [this] { return !tasks_.empty(); });
        task = std::move(tasks_.back());
        tasks_.pop_back();
      }
      task();
    }
  }

  size_t nthreads_;
  std::vector<std::thread> workers_;
  std::vector<std::function<void()>> tasks_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::mutex done_mu_;
  std::condition_variable done_cv_;
};

}  // namespace tfrec
