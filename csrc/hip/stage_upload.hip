// Staged upload of one sliced file read, for files whose mapping cannot be
// registered: a background thread (csrc/stage_core.h) fills the pinned
// staging buffer chunk by chunk through the IO pool and enqueues each
// chunk's H2D copy the moment it is staged, so the host copy, the link and
// the Python thread's kernel launches run side by side. No kernels here.
//
// Source of a chunk: the file's cached, unregistered mapping (memcpy on the
// pool; the file's size is checked first, since touching a mapping past the
// end of a truncated file is a SIGBUS), or pread() on the pool when there is
// no mapping or TFREC_STAGE_SOURCE=pread.
//
// Each chunk is copied half on either DMA stream (TFREC_READ_SPLIT, see
// docs/TUNING.md: the streams share the link, so slice k has landed before
// slice k + 1 takes much of it); unsplit, a whole slice goes to one stream.
// After a slice's last chunk one event per stream used is recorded.
// wait_issued(s) hands those events out only once they have been recorded:
// a stream made to wait on an unrecorded event would not wait at all.

#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <sys/stat.h>

#include <array>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../io_pool.h"
#include "../stage_core.h"

namespace py = pybind11;

#define HIP_CHECK(expr)                                                          \
  do {                                                                           \
    hipError_t _e = (expr);                                                      \
    if (_e != hipSuccess)                                                        \
      throw std::runtime_error(std::string("HIP error: ") +                      \
                               hipGetErrorString(_e) + " at " __FILE__ ":" +     \
                               std::to_string(__LINE__));                        \
  } while (0)

namespace {

using tfrec::IOPool;
using tfrec::stage::Chunk;
using tfrec::stage::Stager;

class StagedUpload {
 public:
  StagedUpload(int fd, uintptr_t map, uintptr_t staging, uintptr_t dev,
               const std::vector<int64_t>& bounds, uintptr_t stream0,
               uintptr_t stream1, int64_t chunk, bool split, int device)
      : fd_(fd),
        map_((const uint8_t*)map),
        staging_((uint8_t*)staging),
        dev_((uint8_t*)dev),
        streams_{(hipStream_t)stream0, (hipStream_t)stream1},
        split_(split && stream1 != stream0),
        device_(device),
        stager_(bounds, chunk, [this] { HIP_CHECK(hipSetDevice(device_)); },
                [this](int64_t off, int64_t len) { return stage(off, len); },
                [this](int, const Chunk& c) { enqueue(c); },
                [this](int s) { record(s); }) {
    int prev = 0;
    HIP_CHECK(hipGetDevice(&prev));
    HIP_CHECK(hipSetDevice(device_));
    events_.resize((size_t)stager_.nslices() * nper());
    try {
      for (auto& ev : events_)
        HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    } catch (...) {
      destroy_events();
      (void)hipSetDevice(prev);
      throw;
    }
    HIP_CHECK(hipSetDevice(prev));
    stager_.start();
  }

  ~StagedUpload() {
    stager_.close();
    destroy_events();
  }

  // Event handles of slice s, once recorded (blocks; call without the GIL).
  std::vector<uintptr_t> wait_issued(int s) {
    stager_.wait_issued(s);
    std::vector<uintptr_t> out;
    for (int k = 0; k < nper(); ++k)
      out.push_back((uintptr_t)events_[(size_t)s * nper() + k]);
    return out;
  }
  void wait_all() { stager_.wait_all(); }
  void close() { stager_.close(); }
  bool closed() { return stager_.closed(); }
  int issued() { return stager_.issued(); }
  int nslices() const { return stager_.nslices(); }
  int nchunks() const { return (int)stager_.chunks().size(); }

 private:
  int nper() const { return split_ ? 2 : 1; }

  void destroy_events() {
    for (auto ev : events_)
      if (ev) (void)hipEventDestroy(ev);
    events_.clear();
  }

  int stage(int64_t off, int64_t len) {
    if (!map_)
      return IOPool::instance().run(false, fd_, staging_ + off, len, off);
    struct stat st {};
    if (fstat(fd_, &st) != 0) return -errno;
    if ((int64_t)st.st_size < off + len) return -EIO;  // the file got shorter
    const uint8_t* src = map_ + off;
    uint8_t* dst = staging_ + off;
    return IOPool::instance().run_parts(len, 256 << 10, [=](int64_t o, int64_t m) {
      memcpy(dst + o, src + o, (size_t)m);
      return 0;
    });
  }

  void copy(int64_t off, int64_t len, int k) {
    if (len > 0)
      HIP_CHECK(hipMemcpyAsync(dev_ + off, staging_ + off, (size_t)len,
                               hipMemcpyHostToDevice, streams_[k]));
  }

  void enqueue(const Chunk& c) {
    if (!split_) {
      copy(c.off, c.len, c.slice % 2);
      return;
    }
    int64_t half = c.len / 2;
    copy(c.off, half, 0);
    copy(c.off + half, c.len - half, 1);
  }

  void record(int s) {
    for (int k = 0; k < nper(); ++k)
      HIP_CHECK(hipEventRecord(events_[(size_t)s * nper() + k],
                               streams_[split_ ? k : s % 2]));
  }

  int fd_;
  const uint8_t* map_;
  uint8_t* staging_;
  uint8_t* dev_;
  std::array<hipStream_t, 2> streams_;
  bool split_;
  int device_;
  std::vector<hipEvent_t> events_;
  Stager stager_;  // last: its thread uses everything above
};

}  // namespace

void register_stage_upload(py::module_& m) {
  py::class_<StagedUpload>(m, "StagedUpload",
                           "Background staging + H2D of one sliced read")
      .def(py::init<int, uintptr_t, uintptr_t, uintptr_t,
                    const std::vector<int64_t>&, uintptr_t, uintptr_t, int64_t,
                    bool, int>(),
           py::arg("fd"), py::arg("map_ptr"), py::arg("stage_ptr"),
           py::arg("dev_ptr"), py::arg("bounds"), py::arg("stream0"),
           py::arg("stream1"), py::arg("chunk"), py::arg("split"),
           py::arg("device"))
      .def("wait_issued", &StagedUpload::wait_issued, py::arg("s"),
           py::call_guard<py::gil_scoped_release>(),
           "Block until slice s's events are recorded; their handles")
      .def("wait_all", &StagedUpload::wait_all,
           py::call_guard<py::gil_scoped_release>())
      .def("close", &StagedUpload::close,
           py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("closed", &StagedUpload::closed)
      .def_property_readonly("issued", &StagedUpload::issued)
      .def_property_readonly("nslices", &StagedUpload::nslices)
      .def_property_readonly("nchunks", &StagedUpload::nchunks);
  m.def("gpu_stream_wait_event",
        [](uintptr_t stream, uintptr_t event) {
          HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0));
        },
        py::arg("stream"), py::arg("event"),
        "Make `stream` wait for an event that HAS been recorded");
}
