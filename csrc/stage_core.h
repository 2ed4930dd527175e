// Staged upload, host logic only (no HIP, no Python): the chunk plan of a
// sliced file and the background thread that walks it. The thread stages one
// chunk into pinned memory, enqueues its copy at once, and after a slice's
// last chunk records the slice's events and reports the slice issued. What
// "stage", "enqueue" and "record" do comes in as callbacks, so
// csrc/tests/stage_selftest.cpp drives this very code on the CPU under the
// sanitizers; csrc/hip/stage_upload.hip plugs in the IO pool and HIP.
//
// The ordering rule the Python side depends on: a device-side wait on an
// event that has not been recorded yet is a no-op, so nobody may make a
// stream wait on slice s's events before wait_issued(s) has returned.
#pragma once

#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <exception>
#include <functional>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace tfrec {
namespace stage {

struct Chunk {
  int64_t off;  // file offset == offset in the staging and device buffers
  int64_t len;  // 0 only for the one chunk of an empty slice
  int slice;
  bool last;  // the slice's last chunk: record and report after it
};

// Slice s is [bounds[s], bounds[s + 1]). Chunks tile the slices in file
// order, `chunk` bytes each, never across a slice bound; a slice's last
// chunk may be short.
inline std::vector<Chunk> plan_chunks(const std::vector<int64_t>& bounds,
                                      int64_t chunk) {
  if (bounds.size() < 2) throw std::invalid_argument("plan_chunks: no slice");
  if (chunk < 1) throw std::invalid_argument("plan_chunks: chunk < 1");
  std::vector<Chunk> out;
  for (size_t s = 0; s + 1 < bounds.size(); ++s) {
    int64_t b0 = bounds[s], b1 = bounds[s + 1];
    if (b0 < 0 || b1 < b0)
      throw std::invalid_argument("plan_chunks: bounds not ascending");
    if (b0 == b1) out.push_back({b0, 0, (int)s, true});
    for (int64_t o = b0; o < b1; o += chunk) {
      int64_t m = b1 - o < chunk ? b1 - o : chunk;
      out.push_back({o, m, (int)s, o + m == b1});
    }
  }
  return out;
}

class Stager {
 public:
  using InitFn = std::function<void()>;  // first thing on the thread
  // fills [off, off + len) of the staging buffer; 0 or -errno
  using StageFn = std::function<int(int64_t off, int64_t len)>;
  using EnqueueFn = std::function<void(int k, const Chunk&)>;
  using RecordFn = std::function<void(int slice)>;

  Stager(const std::vector<int64_t>& bounds, int64_t chunk, InitFn init,
         StageFn stage, EnqueueFn enqueue, RecordFn record)
      : chunks_(plan_chunks(bounds, chunk)),
        nslices_((int)bounds.size() - 1),
        init_(std::move(init)),
        stage_(std::move(stage)),
        enqueue_(std::move(enqueue)),
        record_(std::move(record)) {}

  Stager(const Stager&) = delete;
  Stager& operator=(const Stager&) = delete;
  ~Stager() { close(); }

  // The owner calls this once everything the callbacks touch exists.
  void start() {
    if (thread_.joinable() || closed_) throw std::logic_error("Stager: started");
    thread_ = std::thread([this] { run(); });
  }

  // Blocks until slice s has been reported issued: all its chunks enqueued
  // and its events recorded. Throws the thread's error if it stopped before
  // that (for s and every later slice; earlier slices stay good).
  void wait_issued(int s) {
    if (s < 0 || s >= nslices_) throw std::out_of_range("Stager: no such slice");
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return issued_ > s || done_; });
    if (issued_ > s) return;
    if (!error_.empty()) throw std::runtime_error(error_);
    throw std::runtime_error("staged upload closed before slice " +
                             std::to_string(s) + " was issued");
  }

  void wait_all() { wait_issued(nslices_ - 1); }

  // Stops the thread at the next chunk boundary and joins it. A slice
  // reported issued had every copy enqueued before the report, so nothing
  // of it is left behind.
  void close() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    if (thread_.joinable()) thread_.join();
    std::lock_guard<std::mutex> lk(mu_);
    done_ = closed_ = true;
    cv_.notify_all();
  }

  bool closed() {
    std::lock_guard<std::mutex> lk(mu_);
    return closed_;
  }
  int issued() {
    std::lock_guard<std::mutex> lk(mu_);
    return issued_;
  }
  bool stopping() {
    std::lock_guard<std::mutex> lk(mu_);
    return stop_;
  }
  int nslices() const { return nslices_; }
  const std::vector<Chunk>& chunks() const { return chunks_; }

 private:
  void run() {
    std::string err;
    try {
      init_();
      for (size_t k = 0; k < chunks_.size() && !stopping(); ++k) {
        const Chunk& c = chunks_[k];
        if (c.len) {
          int e = stage_(c.off, c.len);
          if (e)
            throw std::runtime_error(
                "staged read failed at byte " + std::to_string(c.off) + " (" +
                std::to_string(c.len) + " bytes): " + strerror(e < 0 ? -e : e));
          enqueue_((int)k, c);
        }
        if (c.last) {
          record_(c.slice);
          std::lock_guard<std::mutex> lk(mu_);
          issued_ = c.slice + 1;
          cv_.notify_all();
        }
      }
    } catch (const std::exception& e) {
      err = e.what();
      if (err.empty()) err = "staged upload failed";
    }
    std::lock_guard<std::mutex> lk(mu_);
    error_ = err;
    done_ = true;
    cv_.notify_all();
  }

  const std::vector<Chunk> chunks_;
  const int nslices_;
  InitFn init_;
  StageFn stage_;
  EnqueueFn enqueue_;
  RecordFn record_;

  std::mutex mu_;
  std::condition_variable cv_;
  int issued_ = 0;     // slices [0, issued_) are issued
  bool stop_ = false;  // close() asked the thread to stop
  bool done_ = false;  // the thread has left its loop (or never ran)
  bool closed_ = false;
  std::string error_;
  std::thread thread_;
};

}  // namespace stage
}  // namespace tfrec
