// Stand-alone host check of the staged upload's chunk planner and thread
// hand-off (csrc/stage_core.h), with the HIP side replaced by callbacks that
// copy bytes and log every call. Checked over kilobyte files: every byte
// reaches the destination exactly once, chunks never cross a slice bound,
// slices are reported in order and only after all their chunks were
// enqueued, wait_issued works from a second thread while the stager runs,
// close() mid-file joins and stops, and a stage error at chunk k surfaces in
// wait_issued for that slice and every later one. Built with sanitizers and
// run as its own executable on the CPU; it never touches a GPU:
//
//   clang++ -std=c++17 -O1 -g -pthread -fsanitize=thread \
//       csrc/tests/stage_selftest.cpp -o stage_selftest_tsan
//   clang++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined \
//       -fno-sanitize-recover=all csrc/tests/stage_selftest.cpp \
//       -o stage_selftest_asan
#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../stage_core.h"

using namespace tfrec::stage;

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

static std::vector<int64_t> even_bounds(int64_t n, int64_t span) {
  std::vector<int64_t> b;
  for (int64_t o = 0; o < n; o += span) b.push_back(o);
  b.push_back(n);
  return b;
}

// One fake upload: "file" -> staging (stage) -> "device" (enqueue). The
// buffers are exact-size heap blocks, so a byte past either end trips ASan.
struct Fake {
  int64_t n;
  std::vector<int64_t> bounds;
  std::unique_ptr<uint8_t[]> file, staging, device;
  std::unique_ptr<uint8_t[]> hits;  // copies that reached each device byte
  struct Call {
    char what;  // 's'tage, 'e'nqueue, 'r'ecord
    int64_t off, len;
    int slice;
  };
  std::vector<Call> log;  // written by the stager thread only
  int64_t file_len;       // bytes the "file" really has (short: stage fails)
  int init_calls = 0;
  std::atomic<int> staged{0};
  std::function<void(int)> on_stage;  // hook, called with the stage count

  Fake(int64_t n_, std::vector<int64_t> b)
      : n(n_), bounds(std::move(b)), file(new uint8_t[n_]),
        staging(new uint8_t[n_]), device(new uint8_t[n_]),
        hits(new uint8_t[n_]), file_len(n_) {
    for (int64_t i = 0; i < n; ++i) {
      file[i] = (uint8_t)(i * 131 + (i >> 8) + 7);
      staging[i] = device[i] = 0xEE;
      hits[i] = 0;
    }
  }

  std::unique_ptr<Stager> make(int64_t chunk) {
    return std::make_unique<Stager>(
        bounds, chunk, [this] { ++init_calls; },
        [this](int64_t off, int64_t len) {
          log.push_back({'s', off, len, -1});
          if (on_stage) on_stage(staged.load());
          ++staged;
          if (off + len > file_len) return -EIO;  // the file got shorter
          memcpy(staging.get() + off, file.get() + off, (size_t)len);
          return 0;
        },
        [this](int, const Chunk& c) {
          log.push_back({'e', c.off, c.len, c.slice});
          memcpy(device.get() + c.off, staging.get() + c.off, (size_t)c.len);
          for (int64_t i = c.off; i < c.off + c.len; ++i) ++hits[i];
        },
        [this](int s) { log.push_back({'r', 0, 0, s}); });
  }
};

static void check_plan(const std::vector<int64_t>& bounds, int64_t chunk) {
  auto cs = plan_chunks(bounds, chunk);
  int64_t pos = bounds.front();
  int slice = 0;
  for (const Chunk& c : cs) {
    CHECK(c.slice >= slice);
    slice = c.slice;
    CHECK(c.off == pos && c.len <= chunk);
    CHECK(c.off >= bounds[slice] && c.off + c.len <= bounds[slice + 1]);
    CHECK(c.last == (c.off + c.len == bounds[slice + 1]));
    // only a slice's last chunk may be short
    CHECK(c.len == chunk || c.last);
    CHECK(c.len > 0 || bounds[slice] == bounds[slice + 1]);
    pos += c.len;
  }
  CHECK(pos == bounds.back());
  CHECK(cs.empty() || cs.back().slice == (int)bounds.size() - 2);
}

// A whole upload; a second thread waits for every slice in turn and checks
// the slice's bytes the moment it is reported.
static void run_full(int64_t n, const std::vector<int64_t>& bounds,
                     int64_t chunk) {
  check_plan(bounds, chunk);
  Fake f(n, bounds);
  auto st = f.make(chunk);
  int S = st->nslices();
  std::atomic<int> seen{0};
  st->start();
  std::thread waiter([&] {
    for (int s = 0; s < S; ++s) {
      st->wait_issued(s);
      CHECK(st->issued() > s);
      for (int64_t i = bounds[s]; i < bounds[s + 1]; ++i)
        CHECK(f.device[i] == f.file[i] && f.hits[i] == 1);
      ++seen;
    }
  });
  st->wait_all();
  waiter.join();
  CHECK(seen == S && st->issued() == S);
  st->close();
  CHECK(st->closed());
  for (int64_t i = 0; i < n; ++i) CHECK(f.hits[i] == 1 && f.device[i] == f.file[i]);
  CHECK(f.init_calls == 1);
  // the log: stage then enqueue per chunk, in file order, inside one slice;
  // record(s) after slice s's last enqueue, slices ascending
  int next_slice = 0;
  int64_t pos = 0;
  for (size_t i = 0; i < f.log.size(); ++i) {
    const Fake::Call& c = f.log[i];
    if (c.what == 's') {
      CHECK(c.off == pos && i + 1 < f.log.size());
      const Fake::Call& e = f.log[i + 1];
      CHECK(e.what == 'e' && e.off == c.off && e.len == c.len);
    } else if (c.what == 'e') {
      CHECK(c.slice == next_slice);
      CHECK(c.off >= bounds[c.slice] && c.off + c.len <= bounds[c.slice + 1]);
      CHECK(c.len <= chunk && c.len > 0);
      pos = c.off + c.len;
    } else {
      CHECK(c.slice == next_slice && pos == bounds[c.slice + 1]);
      ++next_slice;
    }
  }
  CHECK(next_slice == S && pos == n);
}

// close() while the thread is mid-file: the hook holds the stager inside
// chunk `at` until close() has asked it to stop.
static void run_close_midfile(int64_t n, int64_t span, int64_t chunk, int at) {
  Fake f(n, even_bounds(n, span));
  std::atomic<bool> reached{false};
  Stager* self = nullptr;
  f.on_stage = [&](int k) {
    if (k == at) {
      reached = true;
      while (!self->stopping()) std::this_thread::yield();
    }
  };
  auto st = f.make(chunk);
  self = st.get();
  size_t planned = st->chunks().size();
  CHECK((size_t)at + 1 < planned);
  st->start();
  while (!reached) std::this_thread::yield();
  st->close();
  CHECK(st->closed());
  // the chunk under way is finished, none after it is started
  int staged = f.staged.load();
  CHECK(staged == at + 1);
  int issued = st->issued();
  CHECK(issued < st->nslices());
  // what was reported issued is complete; nothing past the stop was copied
  for (int64_t i = 0; i < f.bounds[issued]; ++i) CHECK(f.hits[i] == 1);
  const Chunk& stop = st->chunks()[staged - 1];
  for (int64_t i = stop.off + stop.len; i < n; ++i) CHECK(f.hits[i] == 0);
  for (int s = 0; s < st->nslices(); ++s) {
    bool threw = false;
    try {
      st->wait_issued(s);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw == (s >= issued));
  }
  st->close();  // idempotent
  CHECK(f.staged.load() == staged);
}

// The file is shorter than planned: stage fails at the first chunk that
// reaches past file_len.
static void run_stage_error(int64_t n, int64_t span, int64_t chunk,
                            int64_t file_len) {
  Fake f(n, even_bounds(n, span));
  f.file_len = file_len;
  auto st = f.make(chunk);
  int S = st->nslices();
  int bad = 0;  // the slice holding the first byte past file_len
  while (f.bounds[bad + 1] <= file_len) ++bad;
  st->start();
  std::vector<int> threw(S, 0);
  std::thread waiter([&] {
    for (int s = 0; s < S; ++s) {
      try {
        st->wait_issued(s);
      } catch (const std::runtime_error& e) {
        threw[s] = 1;
        CHECK(std::string(e.what()).find("staged read failed") !=
              std::string::npos);
      }
    }
  });
  waiter.join();
  for (int s = 0; s < S; ++s) CHECK(threw[s] == (s >= bad));
  bool all_threw = false;
  try {
    st->wait_all();
  } catch (const std::runtime_error&) {
    all_threw = true;
  }
  CHECK(all_threw);
  CHECK(st->issued() == bad);
  st->close();
  for (int64_t i = 0; i < f.bounds[bad]; ++i)
    CHECK(f.hits[i] == 1 && f.device[i] == f.file[i]);
  // nothing was enqueued from the failed chunk on
  for (int64_t i = file_len; i < n; ++i) CHECK(f.hits[i] == 0);
}

int main() {
  const int64_t C = 1024;
  // file sizes 1, chunk - 1, chunk, chunk + 1 in one slice
  for (int64_t n : {(int64_t)1, C - 1, C, C + 1}) run_full(n, {0, n}, C);
  // a slice of exactly one chunk; of three chunks plus a remainder
  run_full(C, {0, C}, C);
  run_full(3 * C + 300, {0, 3 * C + 300}, C);
  // two slices, the last one short; an uneven plan with an empty slice
  run_full(4 * C + 17, even_bounds(4 * C + 17, 4 * C), C);
  run_full(5000, {0, 1024, 1024, 4396, 5000}, C);
  // 21 slices of three chunks plus a remainder, short last slice
  {
    int64_t span = 3 * C + 100, n = 20 * span + 77;
    CHECK(even_bounds(n, span).size() == 22);
    run_full(n, even_bounds(n, span), C);
  }
  // chunk larger than every slice (whole-slice staging), chunk of one byte
  run_full(10 * C + 5, even_bounds(10 * C + 5, 2 * C), 64 * C);
  run_full(257, even_bounds(257, 100), 1);
  // no slices at all is refused
  {
    bool threw = false;
    try {
      plan_chunks({0}, C);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    CHECK(threw);
  }
  // never started: close() is clean and waits throw at once
  {
    Fake f(100, {0, 100});
    auto st = f.make(C);
    st->close();
    bool threw = false;
    try {
      st->wait_issued(0);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw && st->closed() && f.staged.load() == 0);
  }
  // destruction without close() joins the thread
  {
    Fake f(8 * C, even_bounds(8 * C, 2 * C));
    auto st = f.make(C);
    st->start();
    st.reset();
  }
  for (int at : {0, 1, 3, 6}) run_close_midfile(21 * C, 3 * C, C, at);
  // error in slice 0, in a middle slice at a chunk boundary and inside a
  // chunk, and in the last slice
  run_stage_error(12 * C, 3 * C, C, 10);
  run_stage_error(12 * C, 3 * C, C, 4 * C);
  run_stage_error(12 * C, 3 * C, C, 7 * C + 1);
  run_stage_error(12 * C + 9, 3 * C, C, 12 * C + 8);
  printf("stage_selftest: ok\n");
  return 0;
}
