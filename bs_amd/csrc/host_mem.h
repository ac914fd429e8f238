// host_mem.h — owning device / pinned buffers and events, the stream pool, DevicePool, the knobs,
// stream_wait, HCHECK / MCHECK, and what the passes share: a table of refs, timed marks, a header
// read back.
#pragma once

static int device_node(int device);  // NUMA node of a HIP device (below)

namespace {

const uint32_t kIV[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                         0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};

// Device memory that frees itself: move-only, so a buffer has one owner at a time.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {  // (which deletes the copies)
    if (this != &o) release(), p = o.p, cap = o.cap, o.p = nullptr, o.cap = 0;
    return *this;
  }
  ~DevBuf() { release(); }
  hipError_t ensure(size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (bytes <= cap) return hipSuccess;
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 8;  // headroom against regrowth
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      e = hipMalloc(&p, bytes);
      if (e != hipSuccess) return e;
      want = bytes;
    }
    cap = want;
    return hipSuccess;
  }
  // a buffer of a fixed size, allocated once and without headroom (a bsg_pool's bytes)
  hipError_t exact(size_t bytes) {
    release();
    const hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
    if (e == hipSuccess) cap = bytes ? bytes : 16;
    else p = nullptr;
    return e;
  }
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T> T* as() const { return static_cast<T*>(p); }
};

// Page-locked host memory. Two kinds:
//  * kernel-visible (default): hipHostMalloc, mapped for the device, so kernels can write
//    results straight into it (records, counters, snapshots);
//  * DMA staging (dma_only): an anonymous mapping with transparent huge pages requested, pinned
//    with hipHostRegister and only ever read by hipMemcpyAsync. On the MI355X box this takes
//    17 ms per 256 MiB (mostly zero-filling the pages) and 10 ms to free, against 50-65 ms and
//    29-43 ms for hipHostMalloc / hipHostFree (tools/ubench/pin_cost.cpp,
//    profiles/r03_pin_cost.log). Falls back to hipHostMalloc if registration fails.
// Host ThreadSanitizer builds (tools/tsan_host.sh): hipHostMalloc / hipHostFree recycle pinned
// buffers between threads under the HIP runtime's own (uninstrumented) locks, which TSan cannot
// see; a release before every free and an acquire after every allocation restore the
// happens-before a real allocator lock gives, so reuse of a freed buffer by another context is
// not reported as a race.
#if defined(__has_feature)
#if __has_feature(thread_sanitizer)
#define BSG_TSAN 1
#endif
#endif
#ifdef BSG_TSAN
extern "C" void __tsan_acquire(void* addr);
extern "C" void __tsan_release(void* addr);
static char g_tsan_pinned_sync;
static inline void tsan_after_alloc() { __tsan_acquire(&g_tsan_pinned_sync); }
static inline void tsan_before_free() { __tsan_release(&g_tsan_pinned_sync); }
#else
static inline void tsan_after_alloc() {}
static inline void tsan_before_free() {}
#endif

// DMA staging pages on the current device's NUMA node (preferred, not bound: a full node falls
// back to the other). The H2D of a stage on the far node ran at 49.4-49.7 GB/s against
// 56.2-56.3 from the GPU's own node, the same box and library (profiles/r06_c6_bench1.log /
// bench2.log, bsg_stream_stats), so the 1 GiB e2e took 31.0 ms a rep instead of 28.3: the pages
// were simply placed by first touch, on whichever node the registering thread ran.
void prefer_device_node(void* m, size_t n) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  const int node = device_node(dev);
  if (node < 0 || node >= 64) return;
  const unsigned long mask = 1ul << node;
  (void)syscall(SYS_mbind, m, n, 1 /* MPOL_PREFERRED */, &mask, 64UL, 0U);
}

// (move-only like DevBuf; a moved-from buffer is empty and keeps its kind)
struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;
  bool dma_only = false;
  size_t map_len = 0;  // > 0: p is an mmap of map_len bytes registered with hipHostRegister
  PinBuf() = default;
  PinBuf(PinBuf&& o) noexcept : p(o.p), cap(o.cap), dma_only(o.dma_only), map_len(o.map_len) {
    o.p = nullptr, o.cap = 0, o.map_len = 0;
  }
  PinBuf& operator=(PinBuf&& o) noexcept {
    if (this == &o) return *this;
    release();
    p = o.p, cap = o.cap, dma_only = o.dma_only, map_len = o.map_len;
    o.p = nullptr, o.cap = 0, o.map_len = 0;
    return *this;
  }
  ~PinBuf() { release(); }
  // the device-side address of p (kernels write results straight into pinned host memory)
  void* dev() const {
    void* d = nullptr;
    if (p && hipHostGetDevicePointer(&d, p, 0) != hipSuccess) {
      (void)hipGetLastError();
      d = nullptr;
    }
    return d;
  }
  static constexpr size_t kHuge = 2ull << 20;
  // allocates into (*q, *len): *len > 0 for the registered mapping, 0 for hipHostMalloc
  hipError_t alloc(size_t bytes, void** q, size_t* len) const {
    *q = nullptr;
    *len = 0;
    if (dma_only && bytes >= kHuge) {
      const size_t n = (bytes + kHuge - 1) & ~(kHuge - 1);
      void* m = ::mmap(nullptr, n, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
      if (m != MAP_FAILED) {
        (void)::madvise(m, n, MADV_HUGEPAGE);
        prefer_device_node(m, n);  // before the registration faults the pages in
        if (hipHostRegister(m, n, hipHostRegisterDefault) == hipSuccess) {
          *q = m;
          *len = n;
          return hipSuccess;
        }
        (void)hipGetLastError();
        ::munmap(m, n);
      }
    }
    const hipError_t e = hipHostMalloc(q, bytes, hipHostMallocDefault);
    tsan_after_alloc();
    return e;
  }
  static void free_(void* q, size_t len) {
    if (!q) return;
    if (len) {
      (void)hipHostUnregister(q);
      ::munmap(q, len);
    } else {
      tsan_before_free();
      (void)hipHostFree(q);
    }
  }
  hipError_t ensure(size_t bytes) { return grow(bytes, 0); }
  // ensure() that keeps the first `keep` bytes
  hipError_t grow(size_t bytes, size_t keep) {
    if (bytes == 0) bytes = 16;
    if (bytes <= cap) return hipSuccess;
    void* q = nullptr;
    size_t len = 0;
    hipError_t e = alloc(bytes, &q, &len);
    if (e != hipSuccess) return e;
    if (keep) std::memcpy(q, p, keep);
    free_(p, map_len);
    p = q;
    map_len = len;
    cap = len ? len : bytes;
    return hipSuccess;
  }
  void release() {
    free_(p, map_len);
    p = nullptr;
    cap = 0;
    map_len = 0;
  }
  template <class T> T* as() const { return static_cast<T*>(p); }
};

int herr(hipError_t e) { return e == hipSuccess ? BSG_OK : BSG_EDEVICE; }

// HIP streams come from a process-wide pool per device: creating one costs 12-13 ms for each
// of the process's first four (each gets a hardware queue) and ~4 ms after, destroying one
// ~3 ms (tools/ubench/first_use.hip, profiles/r03_first_use.log), which a context per file and
// an engine per tile slot paid every time. Streams go back to the pool instead.
constexpr size_t kStreamPoolMax = 32;
std::mutex g_stream_mu;
std::vector<hipStream_t>& stream_pool(int device) {
  static auto* pools = new std::vector<std::vector<hipStream_t>>(64);  // never destroyed
  return (*pools)[(size_t)device & 63];
}
hipError_t stream_acquire(int device, hipStream_t* s) {
  {
    std::lock_guard<std::mutex> g(g_stream_mu);
    auto& v = stream_pool(device);
    if (!v.empty()) {
      *s = v.back();
      v.pop_back();
      return hipSuccess;
    }
  }
  return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}
// The stream must be idle (callers synchronise it first); the device must be current.
void stream_release(int device, hipStream_t s) {
  if (!s) return;
  {
    std::lock_guard<std::mutex> g(g_stream_mu);
    auto& v = stream_pool(device);
    if (v.size() < kStreamPoolMax) {
      v.push_back(s);
      return;
    }
  }
  (void)hipStreamDestroy(s);
}

// A few idle T (an engine, a hasher: device buffers, pinned staging, a stream) kept for the next
// one-shot call on their device, which otherwise creates and frees one every time (~1 ms of
// allocations, profiles/r03_split_hash_batch_*). take() hands out one of `device` or nullptr;
// give() keeps t unless the pool is full, and then the caller frees it. What is given must be
// idle: its streams synchronised. The pool is never destroyed: what it holds lives until the
// process exits, when the HIP runtime its destructors would call may be gone already.
template <class T> class DevicePool {
 public:
  T* take(int device) {
    std::lock_guard<std::mutex> g(mu_);
    for (size_t i = 0; i < v_.size(); ++i)
      if (v_[i]->dev == device) {
        T* t = v_[i];
        v_.erase(v_.begin() + (long)i);
        return t;
      }
    return nullptr;
  }
  bool give(T* t) {
    std::lock_guard<std::mutex> g(mu_);
    if (v_.size() >= kKeep) return false;
    v_.push_back(t);
    return true;
  }
  static DevicePool& get() {
    static auto* p = new DevicePool();
    return *p;
  }

 private:
  static constexpr size_t kKeep = 2;
  std::mutex mu_;
  std::vector<T*> v_;
};

// CUs of a device (one attribute query; the device-properties call fills the whole struct and
// costs milliseconds, which an engine per tile slot paid on every bsg_open)
int device_cus(int device) {
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
      n <= 0) {
    (void)hipGetLastError();
    n = 256;
  }
  return n;
}

// BSG_DEBUG_SYNC=1: synchronise and report after every launch (debugging hangs/faults)
bool debug_sync() {
  static const bool v = [] {
    const char* e = std::getenv("BSG_DEBUG_SYNC");
    return e && *e == '1';
  }();
  return v;
}
hipError_t dbg(const char* what, hipStream_t s, hipError_t e) {
  if (!debug_sync() || e != hipSuccess) return e;
  std::fprintf(stderr, "bsgpu: %s ...", what);
  std::fflush(stderr);
  e = hipStreamSynchronize(s);
  std::fprintf(stderr, " %s\n", hipGetErrorString(e));
  std::fflush(stderr);
  return e;
}

// Test and debug knobs (bsg_debug_set). Each starts from its environment variable, read once
// (a getenv racing a test's setenv on another thread is a data race in glibc), and tests change
// it through bsg_debug_set instead of the environment.
std::atomic<int64_t>& knob(int k) {
  static std::atomic<int64_t> seq_wait{[] {
    // polls of a k_sha helper-wave handshake before it gives up and flags a device error
    // (~1 s); 0 makes every handshake fail at once, which is how the tests drive the
    // device-error path (Counters::error -> BSG_EDEVICE)
    const char* e = std::getenv("BSG_DEBUG_SEQ_WAIT");
    return e ? (int64_t)std::strtoul(e, nullptr, 10) : (int64_t)(1u << 24);
  }()};
  static std::atomic<int64_t> long_mode{[] {  // BSG_LONG_MODE = off | all (experiments)
    const char* e = std::getenv("BSG_LONG_MODE");
    if (e && !std::strcmp(e, "off")) return (int64_t)1;
    if (e && !std::strcmp(e, "all")) return (int64_t)2;
    return (int64_t)0;
  }()};
  static std::atomic<int64_t> verify_window{[] {  // split::Reader window (0: 256 MiB)
    const char* e = std::getenv("BSG_VERIFY_WINDOW");
    return e ? (int64_t)std::strtoull(e, nullptr, 10) : (int64_t)0;
  }()};
  static std::atomic<int64_t> early{[] {  // early chains (Early): 1 on, 0 off
    const char* e = std::getenv("BSG_EARLY");
    return e ? (int64_t)std::strtoull(e, nullptr, 10) : (int64_t)1;
  }()};
  static std::atomic<int64_t> poll{[] {  // bsg_engine_finish: 1 polls the stream, 0 blocks
    const char* e = std::getenv("BSG_POLL");
    return e ? (int64_t)(std::strtoull(e, nullptr, 10) != 0) : (int64_t)1;
  }()};
  static std::atomic<int64_t> copy_nt{[] {  // Write copies: 1 non-temporal stores, 0 memcpy
    const char* e = std::getenv("BSG_COPY_NT");
    return e ? (int64_t)(std::strtoull(e, nullptr, 10) != 0) : (int64_t)1;
  }()};
  static std::atomic<int64_t> light_bytes{(int64_t)(4ull << 30)};  // engine runs: light schedule
  static std::atomic<int64_t> host_tail{[] {  // host tail (bsg_engine): 1 on, 0 off
    const char* e = std::getenv("BSG_HOST_TAIL");
    return e ? (int64_t)(std::strtoull(e, nullptr, 10) != 0) : (int64_t)1;
  }()};
  static std::atomic<int64_t> none{0};
  switch (k) {
    case BSG_KNOB_SEQ_WAIT: return seq_wait;
    case BSG_KNOB_LONG_MODE: return long_mode;
    case BSG_KNOB_VERIFY_WINDOW: return verify_window;
    case BSG_KNOB_EARLY: return early;
    case BSG_KNOB_POLL: return poll;
    case BSG_KNOB_COPY_NT: return copy_nt;
    case BSG_KNOB_LIGHT_BYTES: return light_bytes;
    case BSG_KNOB_HOST_TAIL: return host_tail;
    default: return none;
  }
}
// bsg_engine_finish's wait. hipStreamSynchronize sleeps on an interrupt once its short active
// wait has passed and woke 7-43 us after the engine stream's last command ended (a configs[1]
// step is ~9 ms; tools/step_gaps.py, profiles/r05_step_gaps.txt). BSG_KNOB_POLL (default on)
// queries the stream instead, with a CPU pause between queries, for at most kPollMaxNs (a run
// longer than that pays the wake-up once, relatively nothing) and then blocks: no wake-up latency
// on a step-sized run, and no core spinning without bound.
constexpr int64_t kPollMaxNs = 100'000'000;
hipError_t stream_wait(hipStream_t s) {
  if (!knob(BSG_KNOB_POLL).load(std::memory_order_relaxed)) return hipStreamSynchronize(s);
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t e = hipStreamQuery(s);
    if (e != hipErrorNotReady) return e;
    (void)hipGetLastError();
    for (int i = 0; i < 32; ++i) _mm_pause();
    if (std::chrono::steady_clock::now() - t0 > std::chrono::nanoseconds(kPollMaxNs))
      return hipStreamSynchronize(s);
  }
}
uint32_t seq_wait_limit() { return (uint32_t)knob(BSG_KNOB_SEQ_WAIT).load(); }
int long_mode() { return (int)knob(BSG_KNOB_LONG_MODE).load(); }

#define HCHECK(x)                           \
  do {                                      \
    hipError_t e_ = (x);                    \
    if (e_ != hipSuccess) {                 \
      (void)hipGetLastError();              \
      return BSG_EDEVICE;                   \
    }                                       \
  } while (0)

// an allocation the dedup code reports as BSG_ENOMEM (the caller's state is still unchanged)
#define MCHECK(x)                           \
  do {                                      \
    if ((x) != hipSuccess) {                \
      (void)hipGetLastError();              \
      return BSG_ENOMEM;                    \
    }                                       \
  } while (0)

uint64_t pow2_at_least(uint64_t v) {
  uint64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

// The device table of indices by ref of one pass over n refs (bsgpu_engine_common.inc): at most
// half full, every slot kDedupEmpty before the pass inserts.
struct RefTable {
  DevBuf tab;
  uint64_t slots = 0;  // a power of two
  hipError_t reserve(uint64_t n) {
    slots = pow2_at_least(std::max<uint64_t>(64, 2 * n));
    return tab.ensure(8 * slots);
  }
  hipError_t clear(hipStream_t s) { return hipMemsetAsync(tab.p, 0xFF, 8 * slots, s); }
  uint64_t* p() const { return tab.as<uint64_t>(); }
  uint64_t mask() const { return slots - 1; }
};

// A bsg_pool's table and index where they lie on the device, for a pass (walk, restore, mark) that
// takes them in the place of a table it uploads and an index it builds. The pool's own invariant
// stands for the host's loop over the blobs: every blob lies in [0, used) at a multiple of 16.
struct PoolSrc {
  const PoolBlob* table;
  uint64_t* index;      // (read only)
  uint64_t mask;
  uint64_t used;        // the end of the last blob's last byte
  uint64_t blob_bytes;  // the blobs' lens, summed
};

// One HIP event, created at first use and destroyed with its owner (move-only).
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  hipError_t create(unsigned flags = hipEventDefault) {
    return e ? hipSuccess : hipEventCreateWithFlags(&e, flags);
  }
  operator hipEvent_t() const { return e; }
};

// Timed stage boundaries of one pass: events created when first recorded (callers record only
// with profiling on, so without it nothing is created), destroyed with their owner.
struct Marks {
  std::vector<Event> ev;
  // marks 0 .. n-1 exist afterwards (bsg_engine_profile reports a failure)
  hipError_t create(size_t n) {
    if (ev.size() < n) ev.resize(n);
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < n && e == hipSuccess; ++i) e = ev[i].create();
    return e;
  }
  // mark i on stream s (not recorded if its event cannot be created)
  void record(size_t i, hipStream_t s) {
    if (ev.size() <= i) ev.resize(i + 1);
    if (ev[i].create() != hipSuccess) (void)hipGetLastError();
    if (ev[i]) (void)hipEventRecord(ev[i], s);
  }
  // ms between marks i and j; `fail` if either is missing or has no time to give
  float ms(size_t i, size_t j, float fail = 0.f) const {
    float v = 0.f;
    if (i >= ev.size() || j >= ev.size() || !ev[i] || !ev[j] ||
        hipEventElapsedTime(&v, ev[i], ev[j]) != hipSuccess) {
      (void)hipGetLastError();
      return fail;
    }
    return v;
  }
};

// The header at d_hdr to the host through `pin`, after everything enqueued on s. error_of(*h)
// is the header's error word: BSG_EDEVICE, and `what` in the message, if a device check set it.
template <class Hdr, class ErrorOf>
int read_header(const PinBuf& pin, const void* d_hdr, hipStream_t s, Hdr* h, ErrorOf error_of,
                const char* what) {
  HCHECK(hipMemcpyAsync(pin.p, d_hdr, sizeof(Hdr), hipMemcpyDeviceToHost, s));
  HCHECK(stream_wait(s));
  *h = *pin.as<Hdr>();
  if (const uint64_t code = error_of(*h)) {
    std::fprintf(stderr, "bsgpu: %s sanity check failed (code %llu)\n", what,
                 (unsigned long long)code);
    return BSG_EDEVICE;
  }
  return BSG_OK;
}

}  // namespace

// NUMA node of a HIP device, from its PCI function in sysfs (-1 unknown)
static int device_node(int device) {
  static std::mutex mu;
  static int cache[64];
  static bool have[64];
  std::lock_guard<std::mutex> g(mu);
  const int k = device & 63;
  if (have[k]) return cache[k];
  char bus[64] = {0};
  int node = -1;
  if (hipDeviceGetPCIBusId(bus, sizeof bus, device) == hipSuccess) {
    for (char* q = bus; *q; ++q) *q = (char)std::tolower((unsigned char)*q);
    char path[160];
    std::snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    if (FILE* f = std::fopen(path, "r")) {
      if (std::fscanf(f, "%d", &node) != 1) node = -1;
      std::fclose(f);
    }
  } else {
    (void)hipGetLastError();
  }
  cache[k] = node;
  have[k] = true;
  return node;
}
