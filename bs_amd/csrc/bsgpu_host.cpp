// bsgpu_host.cpp — libbsgpu host side: device workspaces, the run pipeline and the C ABI
// declared in include/bsgpu.h.
//
// A run = one launch sequence over a batch of stream segments (bsgpu_internal.h):
//   k_start (descriptors in, counters zeroed) → k_scan (+ its exact pass) → prefix(strip counts) →
//   k_compact → k_select → prefix(flags) → k_chunks → … → k_sha (→ k_early_fix), with the early
//   chains (k_pick → k_early) on a second stream from k_compact on
// Everything after k_scan sizes itself from device-side counters, so a run never waits on the
// host; bsg_engine_finish() is the only synchronisation (and the place where a too-small
// candidate buffer is grown and the run repeated).
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <sched.h>
#include <sys/mman.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <emmintrin.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "../../include/bsgpu.h"
#include "bsgpu_internal.h"
#include "bsgpu_launch.h"
#include "buzhash32_table.inc"
#include "host_pool.h"

using namespace bsg;

static int device_node(int device);  // NUMA node of a HIP device (below)

namespace {

const uint32_t kIV[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                         0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
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

struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;
  bool dma_only = false;
  size_t map_len = 0;  // > 0: p is an mmap of map_len bytes registered with hipHostRegister
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
  static std::atomic<int64_t> none{0};
  switch (k) {
    case BSG_KNOB_SEQ_WAIT: return seq_wait;
    case BSG_KNOB_LONG_MODE: return long_mode;
    case BSG_KNOB_VERIFY_WINDOW: return verify_window;
    case BSG_KNOB_EARLY: return early;
    case BSG_KNOB_POLL: return poll;
    case BSG_KNOB_COPY_NT: return copy_nt;
    case BSG_KNOB_LIGHT_BYTES: return light_bytes;
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

int normalize(const bsg_params* in, Params* out, bsg_params* norm) {
  bsg_params p = in ? *in : bsg_params_default();
  // Every value split.Bits / split.MinSize accept (split/split.go:137-152 store them unchecked)
  // is valid: 0 takes hashsplit's default (SplitBits 13, MinSize 64 = the window); MinSize 1..63
  // lets a window span a boundary (the hash still depends only on the last 64 stream bytes, so
  // nothing changes but the greedy rule); Bits > 32 can never be met by TrailingZeros32 (<= 32),
  // so the stream is one final chunk. fanout 0 is our C default (Fanout(0) in Go would divide by
  // zero in split.go:86).
  if (p.split_bits == 0) p.split_bits = 13;  // hashsplit defaultSplitBits
  if (p.min_size == 0) p.min_size = 64;      // hashsplit defaultMinSize (window size)
  if (p.fanout == 0) p.fanout = 8;
  out->split_bits = p.split_bits;
  out->min_size = p.min_size;
  out->mask = p.split_bits >= 32 ? 0xffffffffu : ((1u << p.split_bits) - 1u);
  out->pad_ = 0;
  if (norm) *norm = p;
  return BSG_OK;
}

// The sizes of one run, computed once per enqueue (bsg_engine::plan_split / plan_hash) from the
// run's descriptors and parameters: every buffer reservation and argument block reads them here.
struct RunPlan {
  uint32_t ns = 0;         // streams
  uint64_t strips = 0;     // kStrip-byte strips of all streams
  uint64_t total_len = 0;  // bytes of all streams
  uint64_t data_span = 1;  // bytes from d_data to the end of the last stream (k_sha regions)
  uint64_t cand_cap = 0;   // candidate capacity
  uint64_t chunk_cap = 0;  // record capacity
  uint32_t lists = 0;      // k_scan's refine lists
  uint64_t list_cap = 0;   // entries per list
  uint64_t jobs = 0;       // k_sha's job bound: chunk_cap + ns
  bool scan = false;       // scan and selection stages (a split run; a hash run has neither)
  bool early = false;      // early chains on a second stream
  bool light = false;      // ... in the lightly loaded arrangement (bsg_engine, "Round 5")
};

// The sizes of one bsg_engine_trees call: the run's own (known when it finished), then the node
// count and height bound from the counting pass, then the arena size from the layout passes.
struct TreePlan {
  uint32_t ns = 0;       // streams of the run
  uint64_t M = 0;        // its records
  uint32_t fanout = 8;
  uint64_t nn = 0;       // listed nodes of all streams
  uint32_t H = 1;        // heights of the tallest tree
  uint64_t arena = 0;    // blob bytes (16-byte aligned blobs), without the read slack
};
// one hash run takes at most this many of a height's blobs (bsg_engine_hash's own bound)
constexpr uint32_t kTreeHashBatch = 65535;
// A height with at most this many nodes puts every node on a wave ticket (as bsg_hasher's small
// batches do): the call waits for each height's longest node, and a typical node (10-60 KB) is
// under kLongMinBlocks, where the engine's own choice would hash it per lane, ~4x slower per
// block. More nodes than this keep every wave busy per lane, and the engine's choice stands.
constexpr uint64_t kTreeWaveNodes = 4096;

// Counters::error after a run
int device_error(uint64_t code) {
  std::fprintf(stderr, "bsgpu: device sanity check failed (code %llu)\n", (unsigned long long)code);
  return BSG_EDEVICE;
}

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

// The buffers of one first-occurrence pass (launch_dedup) over n items, and its results. An
// engine owns one for bsg_engine_dedup, a set one for bsg_refset_add.
struct DedupWork {
  DevBuf tab, first, rank, bpre, uniq, pack_off, part, hdr;
  PinBuf h_hdr;
  DedupHdr last{};

  void release() {
    DevBuf* bufs[] = {&tab, &first, &rank, &bpre, &uniq, &pack_off, &part, &hdr};
    for (DevBuf* b : bufs) b->release();
    h_hdr.release();
  }

  int reserve(uint64_t n, uint64_t* slots) {
    const uint64_t n1 = n ? n : 1;
    *slots = pow2_at_least(std::max<uint64_t>(64, 2 * n1));
    MCHECK(tab.ensure(8 * *slots));
    MCHECK(first.ensure(8 * n1));
    MCHECK(rank.ensure(8 * (n1 + 1)));
    MCHECK(bpre.ensure(8 * (n1 + 1)));
    MCHECK(uniq.ensure(8 * n1));
    MCHECK(pack_off.ensure(8 * (n1 + 1)));
    MCHECK(part.ensure(8 * tree_scan_parts(n1)));
    MCHECK(hdr.ensure(sizeof(DedupHdr)));
    MCHECK(h_hdr.ensure(sizeof(DedupHdr)));
    return BSG_OK;
  }

  DedupArgs args(const uint8_t* refs, uint64_t stride, const uint8_t* lens, uint64_t len_stride,
                 uint64_t n, uint64_t slots) const {
    DedupArgs a{};
    a.refs = refs;
    a.stride = stride;
    a.lens = lens;
    a.len_stride = len_stride;
    a.n = n;
    a.tab = tab.as<uint64_t>();
    a.tab_mask = slots - 1;
    a.first = first.as<uint64_t>();
    a.rank = rank.as<uint64_t>();
    a.bpre = bpre.as<uint64_t>();
    a.uniq = uniq.as<uint64_t>();
    a.pack_off = pack_off.as<uint64_t>();
    a.part = part.as<uint64_t>();
    a.hdr = hdr.as<DedupHdr>();
    return a;
  }

  // the header to the host after everything enqueued on s; BSG_EDEVICE if a device check failed
  int readback(hipStream_t s) {
    HCHECK(hipMemcpyAsync(h_hdr.p, hdr.p, sizeof(DedupHdr), hipMemcpyDeviceToHost, s));
    HCHECK(stream_wait(s));
    last = *h_hdr.as<DedupHdr>();
    if (last.error) {
      std::fprintf(stderr, "bsgpu: dedup sanity check failed (code %llu)\n",
                   (unsigned long long)last.error);
      return BSG_EDEVICE;
    }
    return BSG_OK;
  }
};

}  // namespace

// A set of 32-byte refs on one device: an append-only key array and an open-addressing table of
// key indices (bsgpu_dedup.inc). Every entry point takes `mu`, so engines on several threads may
// share a set; each call has synchronised the stream it used before it lets go.
struct bsg_refset {
  int dev = 0;
  int num_cus = 256;
  hipStream_t stream = nullptr;  // bsg_refset_add's own
  std::mutex mu;
  DevBuf keys, tab;
  uint64_t slots = 0;            // of tab (a power of two)
  uint64_t key_cap = 0;          // keys the key array holds
  std::atomic<uint64_t> count{0};
  bool dead = false;             // a device error: BSG_ESTATE from then on
  DevBuf staged;                 // bsg_refset_add: the caller's refs
  DedupWork work;

  // the set's part of a first-occurrence pass
  void lookup_args(DedupArgs* a) const {
    a->set_keys = keys.as<uint8_t>();
    a->set_tab = tab.as<uint64_t>();
    a->set_mask = slots - 1;
    a->set_count = count.load();
  }

  // The m new items of a finished pass `d` (its uniq[0 .. m)) become keys, on stream s: the key
  // array and the table grow first (doubling, the table rehashed on the device), and nothing of
  // the set changes unless every allocation succeeded. Synchronises s and reads the pass's
  // header (`w`) back once more for its error word.
  int add_new(const DedupArgs& d, uint64_t m, DedupWork* w, hipStream_t s) {
    if (!m) return BSG_OK;
    const uint64_t cnt = count.load(), want = cnt + m;
    uint64_t nslots = slots;
    while (want * 100 > nslots * kRefSetLoadPct) nslots <<= 1;
    uint64_t ncap = key_cap;
    while (ncap < want) ncap <<= 1;
    DevBuf ntab, nkeys;
    if (nslots != slots) MCHECK(ntab.ensure(8 * nslots));
    if (ncap != key_cap && nkeys.ensure(32 * ncap) != hipSuccess) {
      (void)hipGetLastError();
      ntab.release();
      return BSG_ENOMEM;
    }
    SetArgs sa{};
    sa.keys = nkeys.p ? nkeys.as<uint8_t>() : keys.as<uint8_t>();
    sa.tab = ntab.p ? ntab.as<uint64_t>() : tab.as<uint64_t>();
    sa.mask = nslots - 1;
    sa.count = cnt;
    sa.hdr = d.hdr;
    hipError_t e = hipSuccess;
    if (nkeys.p && cnt)
      e = hipMemcpyAsync(nkeys.p, keys.p, 32 * cnt, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && ntab.p) {
      e = hipMemsetAsync(ntab.p, 0xFF, 8 * nslots, s);
      if (e == hipSuccess) e = launch_set_rehash(sa, s, num_cus);
    }
    if (e == hipSuccess) e = launch_set_add(sa, d, m, s, num_cus);
    int rc = e == hipSuccess ? w->readback(s) : BSG_EDEVICE;
    if (rc) {  // the old table may hold indices of keys that never arrived
      (void)hipGetLastError();
      (void)hipStreamSynchronize(s);
      ntab.release();
      nkeys.release();
      dead = true;
      return rc;
    }
    if (ntab.p) {
      tab.release();
      tab = ntab;
      slots = nslots;
    }
    if (nkeys.p) {
      keys.release();
      keys = nkeys;
      key_cap = ncap;
    }
    count.store(want);
    return BSG_OK;
  }
};

struct bsg_engine {
  int dev = 0;
  int num_cus = 256;
  hipStream_t stream = nullptr;
  DevBuf table, streams, strip0, counts, refine, slots, strip_off, partials_a, partials_b, cand, flags,
      fidx, bnd_end, bnd_info, scount, last_end, out, carry, ctr, long_list, order, buckets, jinfo, jdesc,
      regions, oreg, rorder;
  PinBuf h_streams, h_strip0, h_ctr;
  uint32_t htable[256];  // the table in `table` (a pooled batch engine may get another one)
  // Optional snapshot right after selection (streaming pipeline): the counters and every
  // stream's last chunk end land in pinned memory and sel_ev fires, long before k_sha ends.
  bool snapshot = false;
  PinBuf h_snap;  // Counters, then nstreams x u64 last_end
  hipEvent_t sel_ev = nullptr;
  // current run
  const uint8_t* d_data = nullptr;
  std::vector<StreamDesc> descs;
  Params p{};
  uint64_t retry_cap = 0;  // exact candidate capacity after an overflow (one re-run)
  uint32_t nstreams = 0;
  bool enqueued = false;
  bool hash_mode = false;  // bsg_engine_hash: every stream is one blob (enqueue_hash)
  int hash_long_mode = -1;  // >= 0: enqueue_hash's SHA path choice instead of the knob's
  Counters last{};
  // optional per-stage HIP events on the engine stream: [scan, compact..chunks, sha]
  int profile = 0;  // bsg_engine_profile mode
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  float stage_ms[3] = {0, 0, 0};
  // Early chains (bsgpu_internal.h, Early): the two longest sure chunks hashed on a second
  // stream from right after k_compact. The Early record lives after the Counters in `ctr`, so
  // the run's one memset clears both.
  hipStream_t estream = nullptr;
  hipEvent_t cand_ev = nullptr, pick_ev = nullptr, early_ev = nullptr;
  bool early_open = false;  // chains launched whose end the engine stream does not wait for yet
  static constexpr uint64_t kEarlyMinBytes = 256ull << 20;  // smaller runs: not worth a stream
  uint64_t early_min = kEarlyMinBytes;  // bsg_init's warm-up run lowers it to load the kernels
  bool early_ok() const {
    return !snapshot && !hash_mode && knob(BSG_KNOB_EARLY) != 0;
  }

  // bsg_engine_trees: split.Writer's tree per stream of the last finished split run. The tree
  // work owns every buffer here; its node blobs are hashed by `hasher`, a second engine in hash
  // mode on this engine's stream (it shares nothing with the run's buffers, so the records stay).
  uint32_t fanout = 8;        // the last bsg_engine_run's
  bool run_done = false;      // the last enqueue was a bsg_engine_run that finish() completed
  bool borrowed_stream = false;  // `stream` belongs to the engine this one hashes nodes for
  bsg_engine* hasher = nullptr;
  DevBuf t_hdr, t_cstart, t_rmax, t_kcnt, t_tmp, t_close, t_shbase, t_meta, t_pc, t_pn, t_aoff,
      t_part, t_descs, t_arena, t_nodes, t_roots, t_ncount;
  PinBuf h_thdr;
  TreePlan tree;              // the last bsg_engine_trees result's sizes
  bool tree_valid = false;
  std::vector<hipEvent_t> tev;  // profile: start, layout done, per height emit / hash done, end
  float tree_ms[4] = {0, 0, 0, 0};  // profile: counting + layout, emit, hash, whole call

  // bsg_engine_dedup / bsg_engine_pack_unique: which records of the last finished split run are
  // new, and their bytes packed. The dedup work owns every buffer in `dd` and reads the records.
  DedupWork dd;
  bool dd_valid = false;      // `dd` holds the current run's result
  uint64_t dd_n = 0, dd_nunique = 0, dd_bytes = 0;
  bool pack_funnel = false;   // measurement tooling: the aligned-load variant of k_pack
  hipEvent_t dd_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // profile: dedup, pack
  float dd_ms[2] = {0, 0};

  // bsg_engine_restore: streams written out from a pool of blobs. The call owns every buffer
  // here (and hashes the pool through `hasher`), so the last run's records, dedup result and
  // tree stay as they are.
  DevBuf r_in, r_tab, r_seg, r_runs, r_descs;
  PinBuf h_rin, h_rhdr;
  hipEvent_t rs_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // profile
  float rs_ms[3] = {0, 0, 0};  // profile: index + resolve + tiling, verify, scatter

  // Round 5: a lightly loaded run (at most BSG_KNOB_LIGHT_BYTES, default 4 GiB, where the
  // longest chunk's chain is the step: configs[1], [3], [4]) keeps its early chains on the
  // engine stream right after k_pick and moves selection and k_sha to the second stream, so the
  // chain pays no cross-stream wait (≈ 10-14 us between k_compact and k_pick,
  // profiles/r04_run_timelines_early.txt) and no dispatch gap; selection, which has slack there,
  // pays it instead. A loaded run (configs[2], where the hash work ends with the chain) keeps
  // selection on the engine stream. The knob lets the tests run one input both ways.

  // profile 1: every stage boundary; 2: the SHA-256 stage's two only (on the stream it runs on)
  void mark(int i, hipStream_t on = nullptr) {
    if (profile && ev[i] && (profile == 1 || i >= 2)) (void)hipEventRecord(ev[i], on ? on : stream);
  }

  int setdev() { return herr(hipSetDevice(dev)); }

  RunPlan plan_split() {
    RunPlan pl;
    pl.scan = true;
    pl.ns = nstreams;
    uint64_t chunk_bound = 0;
    for (uint32_t s = 0; s < pl.ns; ++s) {
      descs[s].strip0 = pl.strips;
      pl.strips += (descs[s].len + kStrip - 1) / kStrip;
      pl.total_len += descs[s].len;
      pl.data_span = std::max<uint64_t>(pl.data_span, descs[s].data_off + descs[s].len);
      chunk_bound += (descs[s].len + (descs[s].seg_base - descs[s].open_start)) / p.min_size + 2;
    }
    {
      // random input yields ~len/2^bits candidates; degenerate input (e.g. all zeros: one per
      // byte) overflows this estimate and is re-run once at its exact size by finish().
      const uint32_t b = std::min<uint32_t>(p.split_bits, 16);
      pl.cand_cap = std::max<uint64_t>(1u << 16, ((pl.total_len >> b) << 2) + 2ull * pl.ns + 1024);
      if (retry_cap > pl.cand_cap) pl.cand_cap = retry_cap;
    }
    // Every chunk ends at a candidate (the forced final one included), and a run whose
    // candidates overflow cand_cap selects nothing, so cand_cap also bounds the chunk count; it
    // is the tighter bound for small MinSize (len / MinSize records would be ~len for MinSize 1).
    pl.chunk_cap = std::min(chunk_bound, pl.cand_cap);
    // the refine lists: one per k_scan workgroup, scan_list_cap entries each
    pl.lists = pl.strips ? scan_lists(pl.strips, num_cus) : 0;
    pl.list_cap = scan_list_cap(pl.strips, pl.lists);
    pl.jobs = pl.chunk_cap + pl.ns;
    pl.early = early_ok() && pl.total_len >= early_min && pl.strips;
    pl.light = pl.early && pl.total_len <= (uint64_t)knob(BSG_KNOB_LIGHT_BYTES).load();
    return pl;
  }

  // bsg_engine_hash: one final chunk per stream, no candidates
  RunPlan plan_hash() {
    RunPlan pl;
    pl.ns = nstreams;
    for (uint32_t s = 0; s < pl.ns; ++s)
      pl.data_span = std::max<uint64_t>(pl.data_span, descs[s].data_off + descs[s].len);
    pl.chunk_cap = pl.ns;
    pl.jobs = pl.chunk_cap + pl.ns;
    return pl;
  }

  // The Early record lives after the Counters in `ctr`, so k_start clears both at once; a hash
  // run has no early chains and keeps (and clears) the Counters alone.
  static size_t ctr_bytes(const RunPlan& pl) {
    return sizeof(Counters) + (pl.scan ? sizeof(Early) : 0);
  }

  // Every work buffer at the size the plan needs (a buffer only ever grows).
  int reserve(const RunPlan& pl) {
    const uint64_t nn = pl.ns ? pl.ns : 1;
    // a hash run sizes its records and jobs for one blob at least (an empty batch)
    const uint64_t recs = pl.scan ? pl.chunk_cap : nn;
    const uint64_t jobs = pl.scan ? pl.jobs : 2 * nn;
    if (pl.scan) {
      const uint64_t st = pl.strips ? pl.strips : 1;
      HCHECK(strip0.ensure(sizeof(uint64_t) * (pl.ns + 1)));
      HCHECK(counts.ensure(sizeof(uint32_t) * st));
      // the refine lists, then their lengths (u32 per list)
      HCHECK(refine.ensure(sizeof(uint64_t) * (pl.lists * pl.list_cap + 1) +
                           sizeof(uint32_t) * (pl.lists + 1)));
      HCHECK(slots.ensure(sizeof(uint32_t) * kSlotCap * st));
      HCHECK(strip_off.ensure(sizeof(uint64_t) * st));
      HCHECK(partials_a.ensure(sizeof(uint64_t) * prefix_partials_needed(pl.strips)));
      HCHECK(partials_b.ensure(sizeof(uint64_t) * prefix_partials_needed(pl.cand_cap)));
      HCHECK(cand.ensure(sizeof(uint64_t) * pl.cand_cap));
      HCHECK(flags.ensure(sizeof(uint32_t) * pl.cand_cap));
      HCHECK(fidx.ensure(sizeof(uint64_t) * pl.cand_cap));
      HCHECK(h_strip0.ensure(sizeof(uint64_t) * (pl.ns + 1)));
    }
    HCHECK(streams.ensure(sizeof(StreamDesc) * nn));
    HCHECK(bnd_end.ensure(sizeof(uint64_t) * recs));
    HCHECK(bnd_info.ensure(sizeof(uint64_t) * recs));
    HCHECK(out.ensure(sizeof(ChunkRec) * recs));
    HCHECK(scount.ensure(sizeof(uint64_t) * nn));
    HCHECK(last_end.ensure(sizeof(uint64_t) * nn));
    HCHECK(carry.ensure(sizeof(CarryOut) * nn));
    HCHECK(ctr.ensure(ctr_bytes(pl)));
    HCHECK(long_list.ensure(sizeof(uint64_t) * jobs));
    HCHECK(order.ensure(sizeof(uint64_t) * jobs));
    HCHECK(jinfo.ensure(sizeof(uint32_t) * jobs));
    HCHECK(jdesc.ensure(sizeof(LaneJob) * jobs));
    HCHECK(regions.ensure(sizeof(Regions)));
    HCHECK(oreg.ensure(jobs));
    HCHECK(rorder.ensure(sizeof(uint64_t) * jobs));
    HCHECK(buckets.ensure(sizeof(uint32_t) * 4 * kLptBuckets));
    HCHECK(h_streams.ensure(sizeof(StreamDesc) * nn));
    HCHECK(h_ctr.ensure(sizeof(Counters)));
    return BSG_OK;
  }

  Counters* dctr() const { return ctr.as<Counters>(); }
  Early* dearly() const { return reinterpret_cast<Early*>(ctr.as<uint8_t>() + sizeof(Counters)); }

  // k_start reads the descriptors (and a split run's first strips) from pinned host memory
  StartArgs start_args(const RunPlan& pl) const {
    StartArgs a{};
    a.src = static_cast<const StreamDesc*>(h_streams.dev());
    a.streams = streams.as<StreamDesc>();
    a.nstreams = pl.ns;
    a.last_end = last_end.as<uint64_t>();
    a.scount = scount.as<uint64_t>();
    a.carry = carry.as<CarryOut>();
    a.zero0 = ctr.as<uint32_t>();
    a.nzero0 = (uint32_t)(ctr_bytes(pl) / 4);
    a.zero1 = buckets.as<uint32_t>();
    a.nzero1 = 2 * kLptBuckets;
    if (pl.scan) {
      a.src_strip0 = static_cast<const uint64_t*>(h_strip0.dev());
      a.strip0 = strip0.as<uint64_t>();
      a.zero2 = partials_a.as<uint32_t>();
      a.nzero2 = (uint32_t)(2 * prefix_partials_needed(pl.strips));
      a.zero3 = partials_b.as<uint32_t>();
      a.nzero3 = (uint32_t)(2 * prefix_partials_needed(pl.cand_cap));
    }
    return a;
  }

  ScanArgs scan_args(const RunPlan& pl) const {
    ScanArgs a{};
    a.data = d_data;
    a.streams = streams.as<StreamDesc>();
    a.strip0 = strip0.as<uint64_t>();
    a.nstreams = pl.ns;
    a.nstrips = pl.strips;
    a.table = table.as<uint32_t>();
    a.p = p;
    a.counts = counts.as<uint32_t>();
    a.refine = refine.as<uint64_t>();
    a.slots = slots.as<uint32_t>();
    a.cand_off = strip_off.as<uint64_t>();
    a.cand = cand.as<uint64_t>();
    a.cand_cap = pl.cand_cap;
    a.ctr = dctr();
    a.lists = pl.lists;
    a.list_cap = pl.list_cap;
    a.list_cnt = reinterpret_cast<uint32_t*>(refine.as<uint64_t>() + pl.lists * pl.list_cap + 1);
    return a;
  }

  // a hash run has no candidates: k_blob_jobs writes one final chunk per stream
  ChunkArgs chunk_args(const RunPlan& pl) const {
    ChunkArgs a{};
    if (pl.scan) {
      a.cand = cand.as<uint64_t>();
      a.flags = flags.as<uint32_t>();
      a.fidx = fidx.as<uint64_t>();
    }
    a.bnd_end = bnd_end.as<uint64_t>();
    a.bnd_info = bnd_info.as<uint64_t>();
    a.scount = scount.as<uint64_t>();
    a.last_end = last_end.as<uint64_t>();
    a.chunk_cap = pl.chunk_cap;
    a.p = p;
    a.ctr = dctr();
    a.streams = streams.as<StreamDesc>();
    return a;
  }

  // k_lens .. k_sha and the early chains; `early`: this run's Early record, or nullptr
  ShaArgs sha_args(const RunPlan& pl, int long_mode, Early* early) const {
    ShaArgs a{};
    a.data = d_data;
    a.streams = streams.as<StreamDesc>();
    a.nstreams = pl.ns;
    a.bnd_end = bnd_end.as<uint64_t>();
    a.bnd_info = bnd_info.as<uint64_t>();
    a.last_end = last_end.as<uint64_t>();
    a.ctr = dctr();
    a.out = out.as<ChunkRec>();
    a.carry = carry.as<CarryOut>();
    a.chunk_cap = pl.chunk_cap;
    a.long_list = long_list.as<uint64_t>();
    a.order = order.as<uint64_t>();
    a.bucket_cnt = buckets.as<uint32_t>();
    a.bucket_elig = buckets.as<uint32_t>() + kLptBuckets;
    a.bucket_off = buckets.as<uint32_t>() + 2 * kLptBuckets;
    a.bucket_loff = buckets.as<uint32_t>() + 3 * kLptBuckets;
    a.jinfo = jinfo.as<uint32_t>();
    a.jdesc = jdesc.as<LaneJob>();
    a.reg = regions.as<Regions>();
    a.oreg = oreg.as<uint8_t>();
    a.rorder = pl.data_span > kRegionBytes ? rorder.as<uint64_t>() : order.as<uint64_t>();
    a.span = pl.data_span;
    a.long_mode = long_mode;
    a.waves = 4u * (uint32_t)num_cus;
    a.seq_wait_limit = seq_wait_limit();
    a.cand = pl.scan ? cand.as<uint64_t>() : nullptr;
    a.early = early;
    return a;
  }

  // descriptors in, counters and bucket counts zeroed, streams initialised: one dispatch
  int run_start(const RunPlan& pl, hipStream_t s) {
    // The pinned staging of the previous run may still be in flight: finish() synchronised.
    std::memcpy(h_streams.p, descs.data(), sizeof(StreamDesc) * pl.ns);
    if (pl.scan) {
      uint64_t* h0 = h_strip0.as<uint64_t>();
      for (uint32_t k = 0; k < pl.ns; ++k) h0[k] = descs[k].strip0;
      h0[pl.ns] = pl.strips;
    }
    const StartArgs st = start_args(pl);
    if (!st.src || (pl.scan && !st.src_strip0)) return BSG_EDEVICE;
    HCHECK(dbg("launch_start", s, launch_start(st, s)));
    return BSG_OK;
  }

  // the second stream and the events of the early chains, at the engine's first run with them
  int early_prepare() {
    if (!estream) HCHECK(stream_acquire(dev, &estream));
    // device-side dependencies only: no system-scope release (an L2 write-back) at record
    const unsigned fl = hipEventDisableTiming | hipEventDisableSystemFence;
    if (!cand_ev) HCHECK(hipEventCreateWithFlags(&cand_ev, fl));
    if (!pick_ev) HCHECK(hipEventCreateWithFlags(&pick_ev, fl));
    if (!early_ev) HCHECK(hipEventCreateWithFlags(&early_ev, fl));
    return BSG_OK;
  }

  // k_scan, the candidate offsets, k_compact: the sorted candidates of the run
  int run_scan(const RunPlan& pl, hipStream_t s) {
    const ScanArgs sa = scan_args(pl);
    mark(0);
    // k_scan: the fast pass, then each workgroup's exact pass over its own refine list
    if (pl.strips) HCHECK(dbg("launch_scan", s, launch_scan(sa, s, num_cus)));
    mark(1);

    PrefixArgs pa{};
    pa.in = counts.as<uint32_t>();
    pa.out = strip_off.as<uint64_t>();
    pa.partials = partials_a.as<uint64_t>();
    pa.n_bound = pl.strips;
    pa.total = &dctr()->ncand;
    pa.overflow = &dctr()->overflow;
    pa.cap = pl.cand_cap;
    pa.error = &dctr()->error;
    HCHECK(dbg("launch_prefix", s, launch_prefix(pa, s)));

    if (pl.strips) HCHECK(dbg("launch_compact", s, launch_compact(sa, s, num_cus)));
    // (exits at once unless a strip had more candidates than slots; k_pick needs them all)
    if (pl.strips) HCHECK(dbg("launch_rescan", s, launch_rescan(sa, s, num_cus)));
    return BSG_OK;
  }

  // k_pick and k_early on stream s
  int run_pick(const RunPlan& pl, const ShaArgs& sh, hipStream_t s) {
    HCHECK(dbg("launch_pick", s,
               launch_pick(cand.as<uint64_t>(), pl.cand_cap, dctr(), p.min_size, dearly(), s,
                           num_cus)));
    HCHECK(hipEventRecord(pick_ev, s));
    HCHECK(dbg("launch_early", s, launch_early(sh, p.split_bits, s)));
    return BSG_OK;
  }

  // The early chains beside selection; *sel_stream: where selection and k_sha then run.
  int run_early(const RunPlan& pl, const ShaArgs& sh, hipStream_t* sel_stream) {
    int rc;
    if (pl.light) {  // chains on the engine stream, selection beside them
      if ((rc = run_pick(pl, sh, stream))) return rc;
      HCHECK(hipStreamWaitEvent(estream, pick_ev, 0));
      *sel_stream = estream;
      early_open = true;  // until the engine stream waits for the selection stream's end
    } else {  // the sorted candidates are final: pick and start two chains beside selection
      HCHECK(hipEventRecord(cand_ev, stream));
      HCHECK(hipStreamWaitEvent(estream, cand_ev, 0));
      if ((rc = run_pick(pl, sh, estream))) return rc;
      HCHECK(hipEventRecord(early_ev, estream));
      early_open = true;
    }
    return BSG_OK;
  }

  // k_select, the chunk indices, k_chunks (and the streaming pipeline's snapshot)
  int run_select(const RunPlan& pl, hipStream_t s) {
    SelArgs sel{cand.as<uint64_t>(), streams.as<StreamDesc>(), flags.as<uint32_t>(), p, dctr()};
    HCHECK(dbg("launch_select", s, launch_select(sel, pl.cand_cap, s, num_cus)));

    PrefixArgs pf{};
    pf.in = flags.as<uint32_t>();
    pf.out = fidx.as<uint64_t>();
    pf.partials = partials_b.as<uint64_t>();
    pf.n_bound = pl.cand_cap;
    pf.n_dev = &dctr()->ncand;
    pf.total = &dctr()->nchunks;
    pf.skip_if = &dctr()->overflow;
    pf.error = &dctr()->error;
    HCHECK(dbg("launch_prefix", s, launch_prefix(pf, s)));

    HCHECK(dbg("launch_chunks", s, launch_chunks(chunk_args(pl), pl.cand_cap, pl.ns, s, num_cus)));
    if (snapshot) {  // by kernel, not by the copy engine (see launch_copy_out)
      HCHECK(h_snap.ensure(sizeof(Counters) + 8ull * (pl.ns ? pl.ns : 1)));
      if (!sel_ev) HCHECK(hipEventCreateWithFlags(&sel_ev, hipEventDisableTiming));
      uint8_t* hs = static_cast<uint8_t*>(h_snap.dev());
      if (!hs) return BSG_EDEVICE;
      HCHECK(launch_copy_out(ctr.p, hs, sizeof(Counters), stream));
      if (pl.ns) HCHECK(launch_copy_out(last_end.p, hs + sizeof(Counters), 8ull * pl.ns, stream));
      HCHECK(hipEventRecord(sel_ev, stream));
    }
    return BSG_OK;
  }

  // the job lists (k_lens .. k_order), then k_sha
  int run_sha(const RunPlan& pl, const ShaArgs& sh, hipStream_t s) {
    HCHECK(dbg("launch_longlist", s, launch_longlist(sh, pl.jobs, s, num_cus)));
    mark(2, s);
    HCHECK(dbg("launch_sha", s, launch_sha(sh, pl.jobs, s, num_cus)));
    return BSG_OK;
  }

  // the early chains' records into place, once they (and k_sha) are done
  int run_early_fix(const RunPlan& pl) {
    if (pl.light) HCHECK(hipEventRecord(early_ev, estream));  // selection + k_sha done
    HCHECK(hipStreamWaitEvent(stream, early_ev, 0));
    early_open = false;  // the engine stream now orders everything after the chains
    HCHECK(dbg("launch_early_fix", stream,
               launch_early_fix(dearly(), out.as<ChunkRec>(), dctr(), stream)));
    return BSG_OK;
  }

  int enqueue() {
    int rc;
    run_done = false;
    dd_valid = false;  // a dedup result belongs to the run it was made from
    if (early_open) {  // a failed run left second-stream work its engine stream never waited for
      HCHECK(hipStreamSynchronize(estream));
      early_open = false;
    }
    const RunPlan pl = plan_split();
    if ((rc = reserve(pl)) || (rc = run_start(pl, stream))) return rc;
    if (pl.early && (rc = early_prepare())) return rc;
    const ShaArgs sh = sha_args(pl, long_mode(), pl.early ? dearly() : nullptr);
    if ((rc = run_scan(pl, stream))) return rc;
    hipStream_t sel_stream = stream;  // where selection and k_sha run
    if (pl.early && (rc = run_early(pl, sh, &sel_stream))) return rc;
    if ((rc = run_select(pl, sel_stream))) return rc;
    if (pl.early && !pl.light) HCHECK(hipStreamWaitEvent(stream, pick_ev, 0));  // k_lens reads the picks
    if ((rc = run_sha(pl, sh, sel_stream))) return rc;
    if (pl.early && (rc = run_early_fix(pl))) return rc;
    mark(3);
    enqueued = true;
    return BSG_OK;
  }

  // bsg_engine_hash: every stream is one blob, hashed whole (Blob.Ref of many blobs): no scan or
  // selection, one final chunk per stream, then the same job ordering and k_sha as a split run.
  // (No candidates, so such a run cannot overflow: finish() never re-runs it.)
  int enqueue_hash() {
    int rc;
    run_done = false;
    dd_valid = false;  // a dedup result belongs to the run it was made from
    const RunPlan pl = plan_hash();
    if ((rc = reserve(pl)) || (rc = run_start(pl, stream))) return rc;
    mark(0);
    mark(1);  // no scan / selection stage
    if (pl.ns) HCHECK(dbg("launch_blob_jobs", stream,
                          launch_blob_jobs(chunk_args(pl), streams.as<StreamDesc>(), pl.ns, stream,
                                           num_cus)));
    const ShaArgs sh = sha_args(pl, hash_long_mode >= 0 ? hash_long_mode : long_mode(), nullptr);
    if ((rc = run_sha(pl, sh, stream))) return rc;
    mark(3);
    enqueued = true;
    return BSG_OK;
  }

  int finish(uint64_t* nchunks) {
    if (!enqueued) return BSG_ESTATE;
    for (int attempt = 0; attempt < 3; ++attempt) {
      HCHECK(hipMemcpyAsync(h_ctr.p, ctr.p, sizeof(Counters), hipMemcpyDeviceToHost, stream));
      HCHECK(stream_wait(stream));
      last = *h_ctr.as<Counters>();
      if (!last.overflow) break;
      retry_cap = last.ncand + 1024;  // exact size for this input, then run again
      int rc = hash_mode ? enqueue_hash() : enqueue();
      if (rc) return rc;
    }
    retry_cap = 0;
    if (last.overflow) return BSG_ENOMEM;
    enqueued = false;
    if (last.error) return device_error(last.error);
    if (profile) {
      for (int i = 0; i < 3; ++i)
        if ((profile == 2 && i < 2) ||
            hipEventElapsedTime(&stage_ms[i], ev[i], ev[i + 1]) != hipSuccess) {
          (void)hipGetLastError();
          stage_ms[i] = -1.f;
        }
    }
    if (nchunks) *nchunks = last.nchunks;
    run_done = !hash_mode && !snapshot;
    return BSG_OK;
  }

  // A hash run whose descriptors a kernel wrote (d_src, device memory) instead of the host:
  // blob i = data[desc[i].data_off .. + desc[i].len), record i = its ref. Enqueued on `stream`;
  // the caller reads out / ctr on the same stream.
  int enqueue_hash_device(const uint8_t* data, uint64_t span, const StreamDesc* d_src,
                          uint32_t n, int sha_mode) {
    int rc;
    RunPlan pl;
    pl.ns = n;
    pl.data_span = std::max<uint64_t>(1, span);
    pl.chunk_cap = n;
    pl.jobs = 2ull * n;
    if ((rc = reserve(pl))) return rc;
    d_data = data;
    nstreams = n;
    hash_mode = true;
    normalize(nullptr, &p, nullptr);
    StartArgs st = start_args(pl);
    st.src = d_src;
    HCHECK(dbg("launch_start", stream, launch_start(st, stream)));
    HCHECK(dbg("launch_blob_jobs", stream,
               launch_blob_jobs(chunk_args(pl), streams.as<StreamDesc>(), pl.ns, stream, num_cus)));
    const ShaArgs sh = sha_args(pl, sha_mode, nullptr);
    return run_sha(pl, sh, stream);
  }

  TreeArgs tree_args(const TreePlan& tp) const {
    TreeArgs a{};
    a.rec = out.as<ChunkRec>();
    a.M = tp.M;
    a.scount = scount.as<uint64_t>();
    a.ns = tp.ns;
    a.fanout = tp.fanout;
    a.H = tp.H;
    a.nn = tp.nn;
    a.arena_bytes = tp.arena;
    a.hdr = t_hdr.as<TreeHdr>();
    a.cstart = t_cstart.as<uint64_t>();
    a.rmax = t_rmax.as<uint32_t>();
    a.kcnt = t_kcnt.as<uint8_t>();
    a.tmp = t_tmp.as<uint64_t>();
    a.close = t_close.as<uint64_t>();
    a.shbase = t_shbase.as<uint64_t>();
    a.meta = t_meta.as<TreeNodeMeta>();
    a.pc = t_pc.as<uint64_t>();
    a.pn = t_pn.as<uint64_t>();
    a.aoff = t_aoff.as<uint64_t>();
    a.part = t_part.as<uint64_t>();
    a.arena = t_arena.as<uint8_t>();
    a.nodes = t_nodes.as<TreeNode>();
    a.roots = t_roots.as<uint8_t>();
    a.ncount = t_ncount.as<uint64_t>();
    return a;
  }

  // the header to the host; BSG_EDEVICE if a device-side check failed
  int tree_readback(TreeHdr* h) {
    HCHECK(hipMemcpyAsync(h_thdr.p, t_hdr.p, sizeof(TreeHdr), hipMemcpyDeviceToHost, stream));
    HCHECK(stream_wait(stream));
    *h = *h_thdr.as<TreeHdr>();
    if (h->error) {
      std::fprintf(stderr, "bsgpu: tree sanity check failed (code %llu)\n",
                   (unsigned long long)h->error);
      return BSG_EDEVICE;
    }
    return BSG_OK;
  }

  hipEvent_t tree_event(size_t i) {
    while (tev.size() <= i) {
      hipEvent_t e = nullptr;
      if (hipEventCreate(&e) != hipSuccess) (void)hipGetLastError();
      tev.push_back(e);
    }
    if (tev[i]) (void)hipEventRecord(tev[i], stream);
    return tev[i];
  }

  // the second engine, in hash mode on this engine's stream (bsg_engine_trees' node blobs,
  // bsg_engine_restore's pool blobs)
  int need_hasher() {
    if (hasher) return BSG_OK;
    hasher = new (std::nothrow) bsg_engine();
    if (!hasher) return BSG_ENOMEM;
    hasher->dev = dev;
    hasher->num_cus = num_cus;
    hasher->stream = stream;
    hasher->borrowed_stream = true;
    return BSG_OK;
  }

  int trees() {
    if (!run_done || snapshot || hash_mode) return BSG_ESTATE;
    int rc;
    tree_valid = false;
    TreePlan tp;
    tp.ns = nstreams;
    tp.M = last.nchunks;
    tp.fanout = fanout ? fanout : 8;
    const uint64_t nn1 = tp.ns ? tp.ns : 1, m1 = tp.M ? tp.M : 1;
    const bool prof = profile != 0;
    size_t nev = 0;

    // counting: chunk ranges, Root heights, node total
    HCHECK(t_hdr.ensure(sizeof(TreeHdr)));
    HCHECK(h_thdr.ensure(sizeof(TreeHdr)));
    HCHECK(t_cstart.ensure(8 * (nn1 + 1)));
    HCHECK(t_rmax.ensure(4 * nn1));
    HCHECK(t_kcnt.ensure(m1));
    HCHECK(t_tmp.ensure(8 * (m1 + 1)));
    HCHECK(t_pc.ensure(8 * (m1 + 1)));
    HCHECK(t_part.ensure(8 * tree_scan_parts(std::max<uint64_t>(m1, nn1))));
    HCHECK(t_roots.ensure(32 * nn1));
    HCHECK(t_ncount.ensure(8 * nn1));
    if (prof) tree_event(nev++);
    HCHECK(hipMemsetAsync(t_hdr.p, 0, sizeof(TreeHdr), stream));
    HCHECK(hipMemsetAsync(t_rmax.p, 0, 4 * nn1, stream));
    HCHECK(dbg("launch_tree_count", stream, launch_tree_count(tree_args(tp), stream, num_cus)));
    TreeHdr h;
    if ((rc = tree_readback(&h))) return rc;
    tp.nn = h.nnodes;
    tp.H = (uint32_t)h.max_r + 1;
    if (tp.H > kTreeMaxHeights) return BSG_EDEVICE;

    if (tp.nn) {
      // layout: every node's children, listed place, blob length and arena offset
      HCHECK(t_close.ensure(8 * tp.nn));
      HCHECK(t_shbase.ensure(8 * ((uint64_t)tp.ns * tp.H + 1)));
      HCHECK(t_meta.ensure(sizeof(TreeNodeMeta) * tp.nn));
      HCHECK(t_pn.ensure(8 * (tp.nn + 1)));
      HCHECK(t_aoff.ensure(8 * (tp.nn + 1)));
      HCHECK(t_nodes.ensure(sizeof(TreeNode) * tp.nn));
      HCHECK(t_part.ensure(8 * tree_scan_parts(std::max<uint64_t>(
                                   std::max<uint64_t>(m1, tp.nn), (uint64_t)tp.ns * tp.H))));
      HCHECK(dbg("launch_tree_layout", stream, launch_tree_layout(tree_args(tp), stream, num_cus)));
      if ((rc = tree_readback(&h))) return rc;
      if (h.hoff[tp.H] != tp.nn) return BSG_EDEVICE;
      tp.arena = h.arena_bytes;
      HCHECK(t_arena.ensure(tp.arena + kReadSlack));
      HCHECK(hipMemsetAsync(t_arena.p, 0, tp.arena + kReadSlack, stream));
      if (prof) tree_event(nev++);

      if ((rc = need_hasher())) return rc;
      // height by height: emit the blobs, hash them, refs into the listed records (where the
      // next height's emit reads them)
      TreeArgs ta = tree_args(tp);
      for (ta.h = 0; ta.h < tp.H; ++ta.h) {
        const uint64_t u0 = h.hoff[ta.h], n = h.hoff[ta.h + 1] - u0;
        const uint64_t children = ta.h ? u0 - h.hoff[ta.h - 1] : tp.M;
        HCHECK(dbg("launch_tree_emit", stream, launch_tree_emit(ta, children, stream, num_cus)));
        if (prof) tree_event(nev++);
        for (uint64_t b = 0; b < n; b += kTreeHashBatch) {
          const uint32_t nb = (uint32_t)std::min<uint64_t>(kTreeHashBatch, n - b);
          HCHECK(t_descs.ensure(sizeof(StreamDesc) * nb));
          HCHECK(launch_tree_descs(ta, u0 + b, nb, t_descs.as<StreamDesc>(), stream, num_cus));
          if ((rc = hasher->enqueue_hash_device(t_arena.as<uint8_t>(), tp.arena,
                                                t_descs.as<StreamDesc>(), nb,
                                                n <= kTreeWaveNodes ? 2 : long_mode())))
            return rc;
          HCHECK(launch_tree_refs(ta, u0 + b, nb, hasher->out.as<ChunkRec>(), hasher->dctr(),
                                  stream, num_cus));
        }
        if (prof) tree_event(nev++);
      }
    }
    HCHECK(dbg("launch_tree_roots", stream, launch_tree_roots(tree_args(tp), stream, num_cus)));
    if (prof) tree_event(nev++);
    if ((rc = tree_readback(&h))) return rc;
    if (prof) {
      auto ms = [&](size_t i, size_t j) {
        float v = 0.f;
        if (i >= nev || j >= nev || !tev[i] || !tev[j] ||
            hipEventElapsedTime(&v, tev[i], tev[j]) != hipSuccess) {
          (void)hipGetLastError();
          return 0.f;
        }
        return v;
      };
      tree_ms[0] = tree_ms[1] = tree_ms[2] = 0.f;
      if (tp.nn) {
        tree_ms[0] = ms(0, 1);
        for (uint32_t k = 0; k < tp.H; ++k) {
          tree_ms[1] += ms(1 + 2 * k, 2 + 2 * k);
          tree_ms[2] += ms(2 + 2 * k, 3 + 2 * k);
        }
      }
      tree_ms[3] = ms(0, nev - 1);
    }
    tree = tp;
    tree_valid = true;
    return BSG_OK;
  }

  void dd_mark(int i) {
    if (!profile) return;
    if (!dd_ev[i] && hipEventCreate(&dd_ev[i]) != hipSuccess) {
      (void)hipGetLastError();
      dd_ev[i] = nullptr;
    }
    if (dd_ev[i]) (void)hipEventRecord(dd_ev[i], stream);
  }
  void dd_elapsed(int k) {
    dd_ms[k] = 0.f;
    if (profile && dd_ev[2 * k] && dd_ev[2 * k + 1] &&
        hipEventElapsedTime(&dd_ms[k], dd_ev[2 * k], dd_ev[2 * k + 1]) != hipSuccess) {
      (void)hipGetLastError();
      dd_ms[k] = 0.f;
    }
  }

  // first occurrence per ref over the run's records (and `set`), then the new refs into the set
  int dedup(bsg_refset* set) {
    if (!run_done || snapshot || hash_mode) return BSG_ESTATE;
    dd_valid = false;
    std::unique_lock<std::mutex> lk;
    if (set) {
      lk = std::unique_lock<std::mutex>(set->mu);
      if (set->dead) return BSG_ESTATE;
    }
    int rc;
    const uint64_t n = last.nchunks;
    uint64_t slots = 0;
    if ((rc = dd.reserve(n, &slots))) return rc;
    dd_mark(0);
    HCHECK(hipMemsetAsync(dd.hdr.p, 0, sizeof(DedupHdr), stream));
    const uint8_t* rec = out.as<uint8_t>();
    DedupArgs a = dd.args(rec + offsetof(ChunkRec, ref), sizeof(ChunkRec),
                          rec + offsetof(ChunkRec, len), sizeof(ChunkRec), n, slots);
    if (set) set->lookup_args(&a);
    if (n) {
      HCHECK(hipMemsetAsync(dd.tab.p, 0xFF, 8 * slots, stream));
      HCHECK(dbg("launch_dedup", stream, launch_dedup(a, stream, num_cus)));
    } else {
      HCHECK(hipMemsetAsync(dd.pack_off.p, 0, 8, stream));
    }
    if ((rc = dd.readback(stream))) return rc;
    const DedupHdr h = dd.last;
    if (h.nunique > n) return BSG_EDEVICE;
    if (set && (rc = set->add_new(a, h.nunique, &dd, stream))) return rc;
    dd_mark(1);
    if (profile) {
      HCHECK(stream_wait(stream));
      dd_elapsed(0);
    }
    dd_n = n;
    dd_nunique = h.nunique;
    dd_bytes = h.unique_bytes;
    dd_valid = true;
    return BSG_OK;
  }

  // bytes from d_data to the end of the run's last stream
  uint64_t run_span() const {
    uint64_t hi = 0;
    for (const StreamDesc& d : descs) hi = std::max<uint64_t>(hi, d.data_off + d.len);
    return hi;
  }

  int pack_unique(uint8_t* d_out, uint64_t cap) {
    if (!dd_valid || !run_done) return BSG_ESTATE;
    if (!d_out || reinterpret_cast<uintptr_t>(d_out) % 16 != 0 || cap < dd_bytes) return BSG_EINVAL;
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_out), o1 = o0 + dd_bytes;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_data), s1 = s0 + run_span();
    if (o1 < o0 || (dd_bytes && o0 < s1 && s0 < o1)) return BSG_EINVAL;
    PackArgs a{};
    a.data = d_data;
    a.streams = streams.as<StreamDesc>();
    a.nstreams = nstreams;
    a.rec = out.as<ChunkRec>();
    a.nrec = dd_n;
    a.uniq = dd.uniq.as<uint64_t>();
    a.pack_off = dd.pack_off.as<uint64_t>();
    a.nunique = dd_nunique;
    a.total = dd_bytes;
    a.out = d_out;
    a.hdr = dd.hdr.as<DedupHdr>();
    dd_mark(2);
    HCHECK(hipMemsetAsync(dd.hdr.p, 0, sizeof(DedupHdr), stream));
    HCHECK(dbg("launch_pack", stream, launch_pack(a, pack_funnel, stream)));
    dd_mark(3);
    int rc;
    if ((rc = dd.readback(stream))) return rc;
    dd_elapsed(1);
    return BSG_OK;
  }

  void rs_mark(int i) {
    if (!profile) return;
    if (!rs_ev[i] && hipEventCreate(&rs_ev[i]) != hipSuccess) {
      (void)hipGetLastError();
      rs_ev[i] = nullptr;
    }
    if (rs_ev[i]) (void)hipEventRecord(rs_ev[i], stream);
  }
  float rs_elapsed(int i, int j) {
    float v = 0.f;
    if (!profile || !rs_ev[i] || !rs_ev[j] ||
        hipEventElapsedTime(&v, rs_ev[i], rs_ev[j]) != hipSuccess) {
      (void)hipGetLastError();
      return 0.f;
    }
    return v;
  }

  // the header to the host after everything enqueued on the stream
  int restore_readback(RestoreHdr* h) {
    HCHECK(hipMemcpyAsync(h_rhdr.p, r_in.p, sizeof(RestoreHdr), hipMemcpyDeviceToHost, stream));
    HCHECK(stream_wait(stream));
    *h = *h_rhdr.as<RestoreHdr>();
    if (h->dd.error) {
      std::fprintf(stderr, "bsgpu: restore sanity check failed (code %llu)\n",
                   (unsigned long long)h->dd.error);
      return BSG_EDEVICE;
    }
    return BSG_OK;
  }

  // bsg_engine_restore. The host checks what it can from its own arrays (pointers, alignment,
  // the output ranges, the blobs' bounds); the records, in their hundreds of thousands, are
  // resolved and checked on the device. Nothing is written to d_out before the header has come
  // back clean.
  int restore(const uint8_t* d_pool, uint64_t pool_bytes, const bsg_pool_blob* blobs,
              uint64_t nblobs, const bsg_chunk* recs, uint64_t nrecs, uint8_t* d_out,
              uint64_t out_cap, const uint64_t* out_off, const uint64_t* out_len, uint32_t ns,
              int flags, bsg_restore_info* info) {
    const bool verify = (flags & BSG_RESTORE_VERIFY) != 0;
    if (flags & ~BSG_RESTORE_VERIFY) return BSG_EINVAL;
    if ((!d_pool && pool_bytes) || (!blobs && nblobs) || (!recs && nrecs) || (!d_out && out_cap) ||
        (ns && (!out_off || !out_len)))
      return BSG_EINVAL;
    if (reinterpret_cast<uintptr_t>(d_out) % 16 != 0) return BSG_EINVAL;
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(d_pool), p1 = p0 + pool_bytes;
    const uintptr_t ob = reinterpret_cast<uintptr_t>(d_out);
    if (p1 < p0 || ob + out_cap < ob) return BSG_EINVAL;

    // the input block: header | blobs | records | out_off | out_len | tile prefix
    auto pad16 = [](uint64_t v) { return (v + 15) & ~15ull; };
    const uint64_t o_blobs = sizeof(RestoreHdr);
    const uint64_t o_recs = o_blobs + pad16(sizeof(PoolBlob) * nblobs);
    const uint64_t o_off = o_recs + pad16(sizeof(ChunkRec) * nrecs);
    const uint64_t o_len = o_off + pad16(8ull * ns);
    const uint64_t o_tpre = o_len + pad16(8ull * ns);
    const uint64_t in_bytes = o_tpre + pad16(8ull * (ns + 1ull));
    MCHECK(h_rin.ensure(in_bytes));
    MCHECK(h_rhdr.ensure(sizeof(RestoreHdr)));
    uint8_t* hin = h_rin.as<uint8_t>();
    uint64_t* tpre = reinterpret_cast<uint64_t*>(hin + o_tpre);

    uint64_t total = 0, tiles = 0;
    std::vector<std::pair<uint64_t, uint64_t>> spans;  // the non-empty output ranges
    for (uint32_t s = 0; s < ns; ++s) {
      if (out_off[s] % 16 != 0 || out_off[s] > out_cap || out_len[s] > out_cap - out_off[s])
        return BSG_EINVAL;
      tpre[s] = tiles;
      if (!out_len[s]) continue;
      const uintptr_t o0 = ob + out_off[s], o1 = o0 + out_len[s];
      if (pool_bytes && o0 < p1 && p0 < o1) return BSG_EINVAL;  // the output inside the pool
      spans.emplace_back(out_off[s], out_off[s] + out_len[s]);
      total += out_len[s];
      tiles += (out_len[s] + kRestoreTile - 1) / kRestoreTile;
    }
    tpre[ns] = tiles;
    std::sort(spans.begin(), spans.end());
    for (size_t k = 1; k < spans.size(); ++k)
      if (spans[k].first < spans[k - 1].second) return BSG_EINVAL;
    if (tiles > 0x7fffffffull) return BSG_EINVAL;

    uint64_t blob_bytes = 0, blob_hi = 0;
    for (uint64_t k = 0; k < nblobs; ++k) {
      if (blobs[k].off > pool_bytes || blobs[k].len > pool_bytes - blobs[k].off) return BSG_EINVAL;
      if (verify && (blobs[k].off % 16 != 0 || blobs[k].len >= (1ull << 40))) return BSG_EINVAL;
      blob_bytes += blobs[k].len;
      blob_hi = std::max<uint64_t>(blob_hi, blobs[k].off + blobs[k].len);
    }
    // the engine hash path's own rules (bsg_engine_hash)
    if (verify && nblobs && (p0 % 16 != 0 || pool_bytes - blob_hi < kReadSlack)) return BSG_EINVAL;

    RestoreHdr* h0 = reinterpret_cast<RestoreHdr*>(hin);
    *h0 = RestoreHdr{};
    h0->missing = h0->mismatch = h0->bad_blob = ~0ull;
    if (nblobs) std::memcpy(hin + o_blobs, blobs, sizeof(PoolBlob) * nblobs);
    if (nrecs) std::memcpy(hin + o_recs, recs, sizeof(ChunkRec) * nrecs);
    if (ns) {
      std::memcpy(hin + o_off, out_off, 8ull * ns);
      std::memcpy(hin + o_len, out_len, 8ull * ns);
    }

    const uint64_t slots = pow2_at_least(std::max<uint64_t>(64, 2 * nblobs));
    const uint64_t ns1 = ns ? ns : 1;
    MCHECK(r_in.ensure(in_bytes));
    MCHECK(r_tab.ensure(8 * slots));
    MCHECK(r_seg.ensure(8 * (nrecs ? nrecs : 1)));
    MCHECK(r_runs.ensure(16 * ns1));
    RestoreArgs a{};
    a.pool = d_pool;
    a.pool_bytes = pool_bytes;
    a.blobs = reinterpret_cast<const PoolBlob*>(r_in.as<uint8_t>() + o_blobs);
    a.nblobs = nblobs;
    a.rec = reinterpret_cast<const ChunkRec*>(r_in.as<uint8_t>() + o_recs);
    a.nrec = nrecs;
    a.out_off = reinterpret_cast<const uint64_t*>(r_in.as<uint8_t>() + o_off);
    a.out_len = reinterpret_cast<const uint64_t*>(r_in.as<uint8_t>() + o_len);
    a.tpre = reinterpret_cast<const uint64_t*>(r_in.as<uint8_t>() + o_tpre);
    a.ns = ns;
    a.tab = r_tab.as<uint64_t>();
    a.tab_mask = slots - 1;
    a.seg = r_seg.as<uint64_t>();
    a.sfirst = r_runs.as<uint64_t>();
    a.slast = r_runs.as<uint64_t>() + ns1;
    a.out = d_out;
    a.hdr = r_in.as<RestoreHdr>();

    int rc;
    rs_mark(0);
    HCHECK(hipMemcpyAsync(r_in.p, hin, in_bytes, hipMemcpyHostToDevice, stream));
    HCHECK(hipMemsetAsync(r_tab.p, 0xFF, 8 * slots, stream));
    HCHECK(hipMemsetAsync(r_runs.p, 0xFF, 16 * ns1, stream));
    HCHECK(dbg("launch_restore_resolve", stream, launch_restore_resolve(a, stream, num_cus)));
    rs_mark(1);
    if (verify && nblobs) {
      if ((rc = need_hasher())) return rc;
      for (uint64_t b = 0; b < nblobs; b += kTreeHashBatch) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(kTreeHashBatch, nblobs - b);
        HCHECK(r_descs.ensure(sizeof(StreamDesc) * nb));
        HCHECK(launch_restore_descs(a, b, nb, r_descs.as<StreamDesc>(), stream, num_cus));
        if ((rc = hasher->enqueue_hash_device(d_pool, blob_hi, r_descs.as<StreamDesc>(), nb,
                                              long_mode())))
          return rc;
        HCHECK(launch_restore_compare(a, b, nb, hasher->out.as<ChunkRec>(), hasher->dctr(),
                                      stream, num_cus));
      }
    }
    rs_mark(2);
    RestoreHdr h;
    if ((rc = restore_readback(&h))) return rc;
    rs_ms[0] = rs_elapsed(0, 1);
    rs_ms[1] = rs_elapsed(1, 2);
    rs_ms[2] = 0.f;
    if (h.invalid) return BSG_EINVAL;
    if (info && verify) {
      info->verified = blob_bytes;
      info->bad_blob = h.bad_blob;
    }
    if (h.missing != ~0ull) {
      if (info) info->bad_record = h.missing;
      return BSG_ENOTFOUND;
    }
    if (info) info->bad_record = h.mismatch;
    if (h.mismatch != ~0ull || (verify && h.bad_blob != ~0ull)) return BSG_ECORRUPT;
    if (enqueued) return BSG_ESTATE;

    rs_mark(3);
    HCHECK(dbg("launch_restore_scatter", stream, launch_restore_scatter(a, tiles, stream)));
    rs_mark(4);
    if ((rc = restore_readback(&h))) return rc;
    rs_ms[2] = rs_elapsed(3, 4);
    if (info) info->bytes = total;
    return BSG_OK;
  }
};

// ------------------------------------------------------------------------------------------
// Streaming split.Writer (bsg_open / bsg_write / bsg_close / bsg_drain): a pipeline of tiles.
// Tile i's bytes go through a ring of pinned stages, by H2D on the context's copy stream, into
// data slot i mod ndata; its kernels run on engine slot i mod nslots (HIP stream + work buffers).
//
//   host:    copy Write()s into stage s ... flush s (H2D) ... stage s+1 ... submit tile i ...
//   data:    [carry area kCarryCap | tile bytes | read slack]
//   copies:  H2D(i, stage 0..3) -> copied_ev(i)      (waits for data slot i's previous tile)
//   engine:  wait copied_ev(i) -> scan/select(i) -> sel_ev(i) -> k_sha(i) -> records(i)
//
// Tile i+1 needs from tile i only where its open chunk starts, which is known at sel_ev(i), a
// fraction of a millisecond into tile i: the open chunk's bytes (at most kCarryCap; k_sha
// leaves such a chunk unhashed) are copied device-to-device in front of tile i+1's bytes and
// hashed there from the start. Tile i's k_sha — bound by its longest chunk's serial SHA-256
// chain — therefore runs concurrently with tiles i+1, i+2, ... instead of in front of them.
// A longer open chunk falls back to the midstate carry: tile i hashes its whole blocks, and
// tile i+1 waits for tile i's k_sha and continues from the exported midstate.
// Records complete in tile order; bsg_pending/bsg_drain hand them out in stream order.
// ------------------------------------------------------------------------------------------
namespace bsg {

// Host threads copying a large Write into pinned staging (BSG_COPY_THREADS, default 8).
int copy_threads() {
  static const int v = [] {
    const char* e = std::getenv("BSG_COPY_THREADS");
    const int hw = (int)std::max(1u, std::thread::hardware_concurrency());
    return std::max(1, std::min(hw, e ? std::min(64, std::atoi(e)) : 8));
  }();
  return v;
}

namespace {
// One parallel_for call: workers and the caller take indices from `next` until none are left.
struct PoolJob {
  const std::function<void(size_t)>* fn = nullptr;
  size_t n = 0;
  std::atomic<size_t> next{0}, done{0};
  std::mutex mu;
  std::condition_variable cv;
  void run() {
    for (size_t i; (i = next.fetch_add(1)) < n;) {
      (*fn)(i);
      if (done.fetch_add(1) + 1 == n) {
        std::lock_guard<std::mutex> g(mu);
        cv.notify_all();
      }
    }
  }
};

class CopyPool {
 public:
  explicit CopyPool(int workers) {
    for (int i = 0; i < workers; ++i) th_.emplace_back([this] { Work(); });
  }
  void Run(size_t n, const std::function<void(size_t)>& fn) {
    auto job = std::make_shared<PoolJob>();
    job->fn = &fn;
    job->n = n;
    {
      std::lock_guard<std::mutex> g(mu_);
      q_.push_back(job);
    }
    cv_.notify_all();
    job->run();  // the caller works too
    {
      std::unique_lock<std::mutex> g(job->mu);
      job->cv.wait(g, [&] { return job->done.load() == job->n; });
    }
    std::lock_guard<std::mutex> g(mu_);
    for (auto it = q_.begin(); it != q_.end(); ++it)
      if (*it == job) {
        q_.erase(it);
        break;
      }
  }

 private:
  void Work() {
    for (;;) {
      std::shared_ptr<PoolJob> job;
      {
        std::unique_lock<std::mutex> g(mu_);
        cv_.wait(g, [&] { return !q_.empty(); });
        job = q_.front();
        if (job->next.load() >= job->n) {  // every index taken: nothing left to help with
          q_.pop_front();
          continue;
        }
      }
      job->run();
    }
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::shared_ptr<PoolJob>> q_;
  std::vector<std::thread> th_;
};

CopyPool* copy_pool() {
  // never destroyed: its workers stay blocked on the queue until the process exits
  static CopyPool* pool = copy_threads() > 1 ? new CopyPool(copy_threads() - 1) : nullptr;
  return pool;
}
}  // namespace

void parallel_for(size_t n, const std::function<void(size_t)>& fn) {
  if (n == 0) return;
  if (n == 1 || copy_threads() <= 1) {
    for (size_t i = 0; i < n; ++i) fn(i);
    return;
  }
  copy_pool()->Run(n, fn);
}

bool copy_nt_enabled() { return knob(BSG_KNOB_COPY_NT).load(std::memory_order_relaxed) != 0; }

namespace {
// 64 bytes (one cache line) per iteration: four unaligned 16-byte loads, four streaming stores
// to a 16-byte aligned destination (SSE2, every x86-64 host)
inline void nt_lines(uint8_t* d, const uint8_t* s, size_t lines) {
  for (size_t i = 0; i < lines; ++i, d += 64, s += 64) {
    const __m128i a = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s));
    const __m128i b = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + 16));
    const __m128i c = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + 32));
    const __m128i e = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + 48));
    _mm_stream_si128(reinterpret_cast<__m128i*>(d), a);
    _mm_stream_si128(reinterpret_cast<__m128i*>(d + 16), b);
    _mm_stream_si128(reinterpret_cast<__m128i*>(d + 32), c);
    _mm_stream_si128(reinterpret_cast<__m128i*>(d + 48), e);
  }
}
// the same into two destinations; d2 streams only if it has d1's alignment mod 16, else it
// takes ordinary stores
inline void nt_lines2(uint8_t* d1, uint8_t* d2, const uint8_t* s, size_t lines, bool d2nt) {
  for (size_t i = 0; i < lines; ++i, d1 += 64, d2 += 64, s += 64) {
    __m128i v[4];
    for (int j = 0; j < 4; ++j) v[j] = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + 16 * j));
    for (int j = 0; j < 4; ++j) _mm_stream_si128(reinterpret_cast<__m128i*>(d1 + 16 * j), v[j]);
    if (d2nt) {
      for (int j = 0; j < 4; ++j) _mm_stream_si128(reinterpret_cast<__m128i*>(d2 + 16 * j), v[j]);
    } else {
      for (int j = 0; j < 4; ++j) _mm_storeu_si128(reinterpret_cast<__m128i*>(d2 + 16 * j), v[j]);
    }
  }
}
}  // namespace

// The streaming stores are weakly ordered: each copy ends with an sfence, so the bytes are in
// memory before the caller publishes them (a parallel_for's completion, then an H2D copy).
void copy_nt(uint8_t* dst, const uint8_t* src, size_t n) {
  const size_t head = std::min(n, (size_t)(-(uintptr_t)dst & 63));
  std::memcpy(dst, src, head);
  const size_t lines = (n - head) / 64;
  nt_lines(dst + head, src + head, lines);
  const size_t done = head + lines * 64;
  std::memcpy(dst + done, src + done, n - done);
  _mm_sfence();
}

void copy_nt2(uint8_t* d1, uint8_t* d2, const uint8_t* src, size_t n) {
  const size_t head = std::min(n, (size_t)(-(uintptr_t)d1 & 63));
  std::memcpy(d1, src, head);
  std::memcpy(d2, src, head);
  const size_t lines = (n - head) / 64;
  const bool d2nt = (((uintptr_t)d1 ^ (uintptr_t)d2) & 15) == 0;
  nt_lines2(d1 + head, d2 + head, src + head, lines, d2nt);
  const size_t done = head + lines * 64;
  std::memcpy(d1 + done, src + done, n - done);
  std::memcpy(d2 + done, src + done, n - done);
  _mm_sfence();
}

int cpu_node() {
  unsigned cpu = 0, node = 0;
  if (syscall(SYS_getcpu, &cpu, &node, nullptr) != 0) return -1;
  return (int)node;
}

}  // namespace bsg

constexpr int kMaxSlots = 8;
constexpr uint64_t kDefaultCarryCap = 8ull << 20;
// Tiles in flight. Each has its own HIP stream, and streams beyond the process's hardware
// queues (GPU_MAX_HW_QUEUES, 4 by default) share a queue and serialise behind each other's
// k_sha, so the default stays below that.
static int default_slots() {
  const char* e = std::getenv("BSG_STREAM_SLOTS");
  const int v = e ? std::atoi(e) : 3;
  return std::max(2, std::min(kMaxSlots, v));
}

// Device copies of the tiles' bytes, decoupled from the engines: tile i's bytes go to data slot
// i mod ndata and its kernels run on engine slot i mod nslots. With one more data slot than
// engines, tile i's H2D does not wait for tile i - nslots' k_sha (which still reads that engine's
// previous tile), only for tile i - ndata's: the copies run back to back on their own stream
// while the chains of earlier tiles finish.
constexpr int kMaxData = 8;
static int default_data_slots(int nslots) {
  const char* e = std::getenv("BSG_DATA_SLOTS");
  const int v = e ? std::atoi(e) : nslots + 1;
  return std::max(std::max(2, nslots), std::min(kMaxData, v));
}

struct DataSlot {
  DevBuf dbuf;                  // carry area + tile + slack
  hipEvent_t free_ev = nullptr; // recorded on an engine stream after the last reader of dbuf
  bool free_pending = false;    // free_ev recorded, not yet waited for by the copy stream
};

struct TileSlot {
  bsg_engine* eng = nullptr;  // created at the slot's first tile (a small stream needs one)
  PinBuf recs;            // records, D2H'd after k_sha
  hipEvent_t h2d_ev = nullptr, done_ev = nullptr, copied_ev = nullptr;
  int dslot = 0;          // data slot of the tile using this engine
  // state of the tile currently using the slot
  bool busy = false;          // submitted, records not yet collected
  bool sel_read = false;      // selection snapshot consumed (open_next / nchunks known)
  bool recs_enq = false;      // D2H of records enqueued (done_ev recorded)
  bool final_seg = false;
  uint64_t seg_base = 0, len = 0, nchunks = 0, open_next = 0;
};

// Host staging of the streaming path: a ring of pinned buffers, independent of the device tiles.
// The host fills one stage; a full stage is copied (hipMemcpyAsync, on the engine stream of the
// tile it belongs to) into that tile's device slot right away, so a tile's H2D runs while the
// host is still filling the rest of it, and the pinned memory a context holds is the ring
// (4 x 64 MiB: as much host-side slack as one whole tile), not three whole tiles (3 x 256 MiB).
constexpr int kStages = 4;
constexpr size_t kStageMax = 64ull << 20;
// Full-size stages (kStageMax) are shared process-wide: a context takes them from this pool as
// its stream grows past a stage and gives them back at bsg_reset / bsg_free, so an idle pooled
// context holds no pinned staging, N concurrent contexts share what they use, and bsg_init can
// pin a ring's worth ahead of the first Writer. (Smaller stages — small tiles, a stream's first
// stage while it grows — stay with their context.)
class StagePool {
 public:
  static StagePool& get() {
    static auto* p = new StagePool();  // never destroyed (its buffers live until exit)
    return *p;
  }
  bool take(PinBuf* out) {  // out: empty
    std::lock_guard<std::mutex> g(mu_);
    if (free_.empty()) return false;
    *out = free_.back();
    free_.pop_back();
    return true;
  }
  void give(PinBuf* b) {  // takes b's buffer if it is a full-size one; b is empty afterwards
    if (!b->p) return;
    if (b->cap >= kStageMax && b->map_len) {
      std::lock_guard<std::mutex> g(mu_);
      if (free_.size() < kMaxFree) {
        free_.push_back(*b);
        *b = PinBuf{};
        b->dma_only = true;
        return;
      }
    }
    b->release();
  }
  int fill(int n) {  // bsg_init: make sure n full-size stages are pinned and waiting
    for (;;) {
      {
        std::lock_guard<std::mutex> g(mu_);
        if ((int)free_.size() >= n) return BSG_OK;
      }
      PinBuf b;
      b.dma_only = true;
      if (b.ensure(kStageMax) != hipSuccess) return BSG_ENOMEM;
      give(&b);
      if (b.p) {  // not taken (not a registered mapping): leave the pool as it is
        b.release();
        return BSG_OK;
      }
    }
  }

 private:
  static constexpr size_t kMaxFree = 16;  // at most 1 GiB of idle pinned staging
  std::mutex mu_;
  std::vector<PinBuf> free_;
};

struct Stage {
  PinBuf buf;                // DMA staging (PinBuf::dma_only)
  hipEvent_t ev = nullptr;   // recorded after the H2D that reads the stage
  bool inflight = false;     // an H2D from it may still be running
  hipEvent_t t0 = nullptr, t1 = nullptr;  // timing events around that H2D (bsg_stream_stats)
  bool timed = false;        // t0/t1 recorded and not yet read
};

// NUMA node of the page holding p (get_mempolicy MPOL_F_NODE | MPOL_F_ADDR; -1 unknown)
static int page_node(const void* p) {
  int node = -1;
  if (!p || syscall(SYS_get_mempolicy, &node, nullptr, 0UL, p, 3UL) != 0) return -1;
  return node;
}

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

static uint64_t ns_since(std::chrono::steady_clock::time_point t0) {
  return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now() - t0).count();
}

// hipEventElapsedTime(a, b) in nanoseconds into *out, negatives as 0; *out is left alone when the
// events have no time to give
static bool elapsed_ns(hipEvent_t a, hipEvent_t b, uint64_t* out) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, a, b) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  *out = ms > 0.f ? (uint64_t)((double)ms * 1e6) : 0;
  return true;
}

// Where a context is in its current stream: everything a new stream starts over. bsg_ctx is
// one of these plus the resources that outlive a stream, so reset() assigns a fresh value and a
// field added here needs no second mention.
struct StreamState {
  int dcur = 0;             // data slot of the tile the host is filling
  bool dready = false;      // the copy stream waits for data[dcur]'s previous readers already
  int cur = 0;              // slot of the tile the host is filling
  size_t fill = 0;          // bytes of the current tile (copied to the device or staged)
  int scur = 0;             // stage the host is filling
  size_t sfill = 0;         // bytes in stages[scur] (the current tile's last sfill bytes)
  int prev = -1;            // last submitted slot (its open chunk continues into `cur`)
  uint64_t pos = 0;         // stream offset of slots[cur]'s first byte
  uint64_t stream0 = 0;     // stream offset of the stream's first byte (0; bsg_set_stream_base)
  uint8_t hist[64] = {};    // the 64 stream bytes before pos
  uint8_t tail[64] = {};    // the last 64 stream bytes copied to the device so far
  bool closed = false, started = false;
  int sticky = BSG_OK;
  bsg_stream_stats stats{};  // bsg_stream_stats: counters since open / reset
  bool span_set = false;     // span0 recorded
  bool tail_set = false;     // tail1 recorded
  int slast = -1;            // stage of the latest H2D
  bool sent = false;         // the stream's first H2D is issued (first_flush())
};

struct bsg_ctx : StreamState {
  bsg_params params{};
  Params p{};
  int dev = 0;
  uint32_t table[256];
  size_t tile = 256ull << 20;  // (tile and carry_cap are settings: they survive reset())
  uint64_t carry_cap = kDefaultCarryCap;
  int nslots = default_slots();
  TileSlot slots[kMaxSlots];
  int ndata = default_data_slots(nslots);
  DataSlot data[kMaxData];
  hipStream_t cstream = nullptr;  // H2D copies of every tile (from the process's stream pool)
  Stage stages[kStages];
  std::deque<int> inflight; // submitted slots in stream order
  std::deque<bsg_chunk> ready;
  std::atomic<uint64_t> node_bytes[4] = {};  // bsg_stream_stats::copy_bytes_node
  hipEvent_t span0 = nullptr;  // recorded before the first H2D of the stream
  hipEvent_t tail0 = nullptr, tail1 = nullptr;  // the final tile's kernels: start, records out

  size_t stage_size() const { return std::min(tile, kStageMax); }

  int init(int device, const uint32_t* tab) {
    dev = device;
    std::memcpy(table, tab ? tab : kBuzhash32Seed1, sizeof table);
    for (Stage& st : stages) {
      st.buf.dma_only = true;
      HCHECK(hipEventCreateWithFlags(&st.ev, hipEventDisableTiming));
      HCHECK(hipEventCreate(&st.t0));
      HCHECK(hipEventCreate(&st.t1));
    }
    HCHECK(hipEventCreate(&span0));
    HCHECK(hipEventCreate(&tail0));
    HCHECK(hipEventCreate(&tail1));
    return ensure_slot(0);  // the first tile's engine: errors surface at bsg_open
  }

  int ensure_slot(int i) {
    TileSlot& t = slots[i];
    if (t.eng) return BSG_OK;
    int err = BSG_OK;
    t.eng = bsg_engine_create(dev, table, &err);
    if (!t.eng) return err;
    t.eng->snapshot = true;
    HCHECK(hipEventCreateWithFlags(&t.h2d_ev, hipEventDisableTiming));
    HCHECK(hipEventCreateWithFlags(&t.done_ev, hipEventDisableTiming));
    HCHECK(hipEventCreateWithFlags(&t.copied_ev, hipEventDisableTiming));
    return BSG_OK;
  }

  // data[dcur] ready to receive the current tile's bytes on the copy stream: allocated, and
  // ordered after the kernels of the tile that used it last.
  int copy_prepare() {
    if (!cstream) HCHECK(stream_acquire(dev, &cstream));
    DataSlot& ds = data[dcur];
    HCHECK(ds.dbuf.ensure(carry_cap + tile + kReadSlack));
    if (!ds.free_ev) HCHECK(hipEventCreateWithFlags(&ds.free_ev, hipEventDisableTiming));
    if (!dready) {
      if (ds.free_pending) HCHECK(hipStreamWaitEvent(cstream, ds.free_ev, 0));
      ds.free_pending = false;
      dready = true;
    }
    return BSG_OK;
  }

  void release() {
    (void)hipSetDevice(dev);
    if (cstream) (void)hipStreamSynchronize(cstream);
    for (TileSlot& t : slots) {
      if (t.eng) (void)hipStreamSynchronize(t.eng->stream);
      t.recs.release();
      if (t.h2d_ev) (void)hipEventDestroy(t.h2d_ev);
      if (t.done_ev) (void)hipEventDestroy(t.done_ev);
      if (t.copied_ev) (void)hipEventDestroy(t.copied_ev);
      bsg_engine_destroy(t.eng);
      t.eng = nullptr;
    }
    for (DataSlot& ds : data) {
      ds.dbuf.release();
      if (ds.free_ev) (void)hipEventDestroy(ds.free_ev);
      ds.free_ev = nullptr;
    }
    if (cstream) stream_release(dev, cstream);
    cstream = nullptr;
    for (Stage& st : stages) {
      if (st.ev) (void)hipEventSynchronize(st.ev);
      StagePool::get().give(&st.buf);
      for (hipEvent_t* e : {&st.ev, &st.t0, &st.t1}) {
        if (*e) (void)hipEventDestroy(*e);
        *e = nullptr;
      }
    }
    for (hipEvent_t* e : {&span0, &tail0, &tail1}) {
      if (*e) (void)hipEventDestroy(*e);
      *e = nullptr;
    }
  }

  // the finished H2D of stage st into the busy time
  void harvest(Stage& st) {
    if (!st.timed) return;
    uint64_t ns = 0;
    if (elapsed_ns(st.t0, st.t1, &ns)) stats.h2d_busy_ns += ns;
    st.timed = false;
  }

  int get_stats(bsg_stream_stats* out) {
    if (cstream) HCHECK(hipStreamSynchronize(cstream));
    for (Stage& st : stages) harvest(st);
    bsg_stream_stats s = stats;
    if (span_set && slast >= 0) elapsed_ns(span0, stages[slast].t1, &s.h2d_span_ns);
    if (tail_set) {
      if (hipEventSynchronize(tail1) == hipSuccess)
        elapsed_ns(tail0, tail1, &s.last_tile_ns);
      else
        (void)hipGetLastError();
      if (slast >= 0) elapsed_ns(stages[slast].t1, tail1, &s.tail_ns);
    }
    for (int k = 0; k < 4; ++k) s.copy_bytes_node[k] = node_bytes[k].load();
    s.gpu_node = device_node(dev);
    for (const Stage& st : stages) {
      if (!st.buf.p) continue;
      for (size_t at : {(size_t)0, st.buf.cap / 2}) {
        const int nd = page_node(st.buf.as<uint8_t>() + at);
        if (nd >= 0 && nd < 32) s.stage_nodes |= 1u << nd;
      }
    }
    s.copy_nt = bsg::copy_nt_enabled() ? 1u : 0u;
    *out = s;
    return BSG_OK;
  }

  // Selection of slot i is done: learn its chunk count and where its open chunk starts. A
  // candidate-buffer overflow (degenerate input) is re-run synchronously at exact capacity.
  int read_sel(int i) {
    TileSlot& t = slots[i];
    if (t.sel_read) return BSG_OK;
    HCHECK(hipEventSynchronize(t.eng->sel_ev));
    Counters c = *t.eng->h_snap.as<Counters>();
    uint64_t last_end =
        *reinterpret_cast<const uint64_t*>(t.eng->h_snap.as<uint8_t>() + sizeof(Counters));
    if (c.overflow || c.error) {
      uint64_t n = 0;
      int rc = t.eng->finish(&n);  // synchronous; re-runs after an overflow
      if (rc) return rc;
      c = t.eng->last;
      HCHECK(hipMemcpy(&last_end, t.eng->last_end.p, 8, hipMemcpyDeviceToHost));
    }
    t.nchunks = c.nchunks;
    t.open_next = last_end;
    t.sel_read = true;
    return BSG_OK;
  }

  // Enqueue the D2H of slot i's records behind its k_sha.
  int enqueue_recs(int i) {
    TileSlot& t = slots[i];
    if (t.recs_enq) return BSG_OK;
    int rc = read_sel(i);
    if (rc) return rc;
    // by kernel behind k_sha: a hipMemcpyAsync D2H queued here would wait for k_sha inside the
    // shared copy-engine queue and hold up the next tiles' H2D copies behind it
    HCHECK(t.recs.ensure(sizeof(bsg_chunk) * (t.nchunks ? t.nchunks : 1)));
    void* rd = t.recs.dev();
    void* cd = t.eng->h_ctr.dev();
    if (!rd || !cd) return BSG_EDEVICE;
    if (t.nchunks)
      HCHECK(launch_copy_out(t.eng->out.p, rd, sizeof(bsg_chunk) * t.nchunks, t.eng->stream));
    HCHECK(launch_copy_out(t.eng->ctr.p, cd, sizeof(Counters), t.eng->stream));
    HCHECK(hipEventRecord(t.done_ev, t.eng->stream));
    if (t.final_seg) {
      HCHECK(hipEventRecord(tail1, t.eng->stream));
      tail_set = true;
    }
    t.recs_enq = true;
    return BSG_OK;
  }

  // Wait for the oldest in-flight tile (if `wait`) and move its records to `ready`.
  int collect_front(bool wait, bool* got) {
    *got = false;
    if (inflight.empty()) return BSG_OK;
    const int i = inflight.front();
    TileSlot& t = slots[i];
    if (!t.recs_enq) {
      if (!wait) return BSG_OK;
      int rc = enqueue_recs(i);
      if (rc) return rc;
    }
    if (!wait) {
      hipError_t q = hipEventQuery(t.done_ev);
      if (q == hipErrorNotReady) {
        (void)hipGetLastError();
        return BSG_OK;
      }
      HCHECK(q);
    }
    HCHECK(hipEventSynchronize(t.done_ev));
    const Counters& c = *t.eng->h_ctr.as<Counters>();
    if (c.error) return device_error(c.error);
    const bsg_chunk* r = t.recs.as<bsg_chunk>();
    for (uint64_t k = 0; k < t.nchunks; ++k) ready.push_back(r[k]);
    t.busy = false;
    t.eng->enqueued = false;
    inflight.pop_front();
    *got = true;
    return BSG_OK;
  }

  int poll() {
    bool got = true;
    while (got) {
      int rc = collect_front(false, &got);
      if (rc) return rc;
    }
    return BSG_OK;
  }

  // Make slots[i] free for a new tile: its previous tile's records are collected.
  int reclaim(int i) {
    while (slots[i].busy) {
      bool got = false;
      int rc = collect_front(true, &got);
      if (rc) return rc;
    }
    return BSG_OK;
  }

  // Copy the staged bytes of the current tile to its data slot (on the copy stream) and move to
  // the next stage.
  int flush_stage() {
    if (sfill == 0) return BSG_OK;
    int rc = copy_prepare();
    if (rc) return rc;
    Stage& st = stages[scur];
    tail_append(st.buf.as<uint8_t>(), sfill);  // history for the next tile
    if (!span_set) {
      HCHECK(hipEventRecord(span0, cstream));
      span_set = true;
    }
    HCHECK(hipEventRecord(st.t0, cstream));
    HCHECK(hipMemcpyAsync(data[dcur].dbuf.as<uint8_t>() + carry_cap + (fill - sfill), st.buf.p,
                          sfill, hipMemcpyHostToDevice, cstream));
    HCHECK(hipEventRecord(st.t1, cstream));
    HCHECK(hipEventRecord(st.ev, cstream));
    st.inflight = true;
    st.timed = true;
    sent = true;
    stats.h2d_bytes += sfill;
    stats.h2d_copies++;
    slast = scur;
    scur = (scur + 1) % kStages;
    sfill = 0;
    return BSG_OK;
  }

  // stages[scur] ready to take bytes: its previous H2D has run, and it can hold `need` bytes.
  // A stream's first stage grows (doubling from 4 MiB) so a small stream pins a few MiB; once
  // the stream has passed a stage's worth of bytes, stages are allocated whole.
  static constexpr size_t kMinStaging = 4ull << 20;
  int stage_ready(size_t need) {
    Stage& st = stages[scur];
    if (st.inflight) {
      const auto t0 = std::chrono::steady_clock::now();
      HCHECK(hipEventSynchronize(st.ev));
      stats.stage_wait_ns += ns_since(t0);
      st.inflight = false;
      harvest(st);
    }
    const size_t full = stage_size();
    const bool big = pos - stream0 + fill >= full;  // past a stage's worth: whole stages
    const size_t want = big ? full : std::min(full, std::max(need, kMinStaging));
    const size_t have = std::min(st.buf.cap, full);
    if (have >= want) return BSG_OK;
    const size_t nc = big ? full : std::min(full, std::max(want, 2 * have));
    PinBuf pooled;
    // a full-size stage already pinned in the pool beats pinning a new one of any size
    if (full == kStageMax && StagePool::get().take(&pooled)) {
      if (sfill) std::memcpy(pooled.p, st.buf.p, sfill);
      st.buf.release();
      st.buf = pooled;
      return BSG_OK;
    }
    HCHECK(st.buf.grow(nc, sfill));
    return BSG_OK;
  }
  size_t stage_room() const {
    return std::min(stages[scur].buf.cap, stage_size()) - sfill;
  }
  // The stream's first kFirstFlush staged bytes go to the device at once instead of when the
  // first stage is full, so the H2D pipeline starts a 32 MiB Write earlier (with a full 64 MiB
  // first stage the copy stream idled until the second Write was copied). Later stages flush
  // full, as before; not the tile's last bytes (a final segment keeps them, see write()).
  static constexpr size_t kFirstFlush = 8ull << 20;
  int first_flush() {
    if (sent || sfill < kFirstFlush || fill >= tile) return BSG_OK;
    return flush_stage();
  }

  int submit(bool final_seg) {
    int rc0 = flush_stage();  // every byte of the tile is on its way to the device slot
    if (rc0) return rc0;
    const int i = cur;
    if ((rc0 = ensure_slot(i))) return rc0;
    TileSlot& t = slots[i];
    bsg_engine* e = t.eng;
    // Two invariants keep a tile's buffers safe. reclaim(i) protects the ENGINE's work buffers:
    // the records of the tile kSlots back on this engine are collected before its buffers are
    // reused. The DATA slot is protected by copy_prepare() and its free_ev: the H2D copies run
    // on the context's copy stream (cstream), which waits for the event recorded after the last
    // kernels (and the carry copy) that read the slot, before refilling it.
    rc0 = reclaim(i);
    if (rc0) return rc0;
    if ((rc0 = copy_prepare())) return rc0;
    // the tile's kernels (and the carry copy into its data slot) run after its H2D copies
    HCHECK(hipEventRecord(t.copied_ev, cstream));
    HCHECK(hipStreamWaitEvent(e->stream, t.copied_ev, 0));
    if (final_seg) HCHECK(hipEventRecord(tail0, e->stream));
    uint8_t* base = data[dcur].dbuf.as<uint8_t>();
    StreamDesc d{};
    d.data_off = carry_cap;
    d.len = fill;
    d.seg_base = pos;
    d.open_start = stream0;  // the first tile; later tiles take the previous tile's open chunk
    d.finalize = final_seg ? 1u : 0u;
    d.carry_cap = final_seg ? 0u : (uint32_t)std::min<uint64_t>(carry_cap, 0xffffffffu);
    std::memcpy(d.hist, hist, 64);
    std::memcpy(d.mid, kIV, sizeof kIV);
    if (prev >= 0) {
      TileSlot& pt = slots[prev];
      int rc = read_sel(prev);
      if (rc) return rc;
      const uint64_t open = pt.open_next;
      const uint64_t carry = pos - open;
      d.open_start = open;
      if (carry <= pt.eng->descs[0].carry_cap) {  // bytes carried on the device
        if (carry) {
          // the open chunk may itself have started in front of pt's tile (carried into it)
          const uint8_t* src = data[pt.dslot].dbuf.as<uint8_t>() + (int64_t)carry_cap +
                               ((int64_t)open - (int64_t)pt.seg_base);
          HCHECK(hipMemcpyAsync(base + carry_cap - carry, src, carry, hipMemcpyDeviceToDevice,
                                e->stream));
          // the previous slot must not be overwritten before this copy has read it
          HCHECK(hipEventRecord(t.h2d_ev, e->stream));
          HCHECK(hipStreamWaitEvent(pt.eng->stream, t.h2d_ev, 0));
          d.flags = kDescOpenInDevice;
        }
      } else {  // midstate carry: wait for the previous tile's k_sha
        rc = enqueue_recs(prev);
        if (rc) return rc;
        HCHECK(hipEventSynchronize(pt.done_ev));
        CarryOut co;
        HCHECK(hipMemcpy(&co, pt.eng->carry.p, sizeof co, hipMemcpyDeviceToHost));
        if (!co.valid || co.open_start != open) return BSG_EDEVICE;
        d.consumed = co.consumed;
        d.prefix_len = co.prefix_len;
        std::memcpy(d.mid, co.mid, sizeof co.mid);
      }
      // the previous tile's records can be fetched as soon as its k_sha is done
      rc = enqueue_recs(prev);
      if (rc) return rc;
      // the previous tile's data slot is free once its kernels (and the carry copy above, which
      // its stream now waits for) are done: the copy stream waits for this before refilling it
      DataSlot& pd = data[pt.dslot];
      HCHECK(hipEventRecord(pd.free_ev, pt.eng->stream));
      pd.free_pending = true;
    }
    e->d_data = base;
    e->descs.assign(1, d);
    e->nstreams = 1;
    e->p = p;
    int rc = e->enqueue();
    if (rc) return rc;
    t.busy = true;
    t.sel_read = false;
    t.recs_enq = false;
    t.final_seg = final_seg;
    t.seg_base = pos;
    t.len = fill;
    t.dslot = dcur;
    dcur = (dcur + 1) % ndata;
    dready = false;
    inflight.push_back(i);
    std::memcpy(hist, tail, 64);  // window history for the next tile
    pos += fill;
    fill = 0;
    prev = i;
    cur = (cur + 1) % nslots;
    if (final_seg) return enqueue_recs(i);
    return BSG_OK;
  }

  // Host side of Write: bytes into the staging ring (large pieces on several threads), each full
  // stage on its way to the device at once, full tiles submitted as more data arrives. A stream
  // has no length limit (split.Writer.Write has none, split/split.go:99-101): stream offsets are
  // u64 everywhere; only candidate positions inside one tile travel in 40-bit fields.
  int write(const uint8_t* p, size_t n) {
    if (n >= (1u << 20)) {
      const int nd = page_node(p);
      if (nd >= 0 && nd < 32) stats.src_nodes |= 1u << nd;
    }
    while (n) {
      if (fill == tile) {  // full tile and more data coming: submit it (never the last one)
        int rc = submit(false);
        if (rc) return rc;
      }
      int rc = stage_ready(sfill + std::min(n, tile - fill));
      if (rc) return rc;
      const size_t k = std::min({n, tile - fill, stage_room()});
      const auto t0 = std::chrono::steady_clock::now();
      par_copy(stages[scur].buf.as<uint8_t>() + sfill, p, k);
      stats.host_copy_ns += ns_since(t0);
      stats.host_bytes += k;
      sfill += k;
      fill += k;
      p += k;
      n -= k;
      // a full stage goes to the device now, except the tile's last one: if the stream ends
      // here, it is submitted as the final segment
      if (stage_room() == 0 && fill < tile && (rc = flush_stage())) return rc;
    }
    if (int rc = first_flush()) return rc;
    return poll();
  }

  // Appends bytes that already went to the device (or are on their way) to the running tail.
  void tail_append(const uint8_t* q, size_t k) {
    if (k >= 64) {
      std::memcpy(tail, q + k - 64, 64);
    } else {
      std::memmove(tail, tail + k, 64 - k);
      std::memcpy(tail + 64 - k, q, k);
    }
  }

  // write() from host memory the caller registered (bsg_host_register): no staging copy, the
  // H2D reads the caller's bytes directly, on the engine stream of the tile they belong to. The
  // last bytes (up to 4 KiB) of a segment that completes a tile are staged instead, so that a
  // full tile always keeps unflushed bytes that window() can hold back for the next tile (a
  // final segment needs at least one byte).
  int write_pinned(const uint8_t* q, size_t n) {
    while (n) {
      if (fill == tile) {
        int rc = submit(false);
        if (rc) return rc;
      }
      int rc = flush_stage();  // staged bytes of this tile go first (offsets stay in order)
      if (rc) return rc;
      if ((rc = copy_prepare())) return rc;
      const size_t k = std::min(n, tile - fill);
      const size_t staged = fill + k == tile ? std::min<size_t>(k, 4096) : 0;
      const size_t direct = k - staged;
      if (direct) {
        HCHECK(hipMemcpyAsync(data[dcur].dbuf.as<uint8_t>() + carry_cap + fill, q, direct,
                              hipMemcpyHostToDevice, cstream));
        tail_append(q, direct);
        fill += direct;
      }
      if (staged) {
        if ((rc = stage_ready(staged))) return rc;
        std::memcpy(stages[scur].buf.as<uint8_t>(), q + direct, staged);
        sfill = staged;
        fill += staged;
      }
      q += k;
      n -= k;
    }
    return poll();
  }

  // Zero-copy form of write(): the caller fills pinned staging directly (an io.Reader reads
  // into it), then commits. The window is the rest of the current stage (within the tile).
  int window(uint8_t** p, size_t* cap) {
    if (fill == tile) {
      // The caller may be at EOF, so this tile cannot be the last one submitted as non-final:
      // hold its last bytes (still in the current stage) back for the next tile. (A final
      // segment must hold at least one byte: the flush of the open chunk is emitted by the scan
      // of the final segment's last strip, and an empty segment has none.)
      constexpr size_t kHold = 4096;
      uint8_t held[kHold];
      const size_t hold = std::min({kHold, tile / 2, sfill});
      std::memcpy(held, stages[scur].buf.as<uint8_t>() + sfill - hold, hold);
      sfill -= hold;
      fill -= hold;
      int rc = submit(false);
      if (rc) return rc;
      if ((rc = stage_ready(hold))) return rc;
      std::memcpy(stages[scur].buf.p, held, hold);
      sfill = fill = hold;
    }
    // the window is the stage's free part (within the tile); a full stage grows or is flushed
    int rc = stage_ready(sfill + 1);
    if (rc) return rc;
    if (stage_room() == 0) {  // a full stage below the tile's end: move on to the next one
      if ((rc = flush_stage()) || (rc = stage_ready(1))) return rc;
    }
    *p = stages[scur].buf.as<uint8_t>() + sfill;
    *cap = std::min(stage_room(), tile - fill);
    return BSG_OK;
  }
  int commit(size_t n) {
    if (n > std::min(stage_room(), tile - fill)) return BSG_EINVAL;
    sfill += n;
    fill += n;
    if (stage_room() == 0 && fill < tile) {
      int rc = flush_stage();
      if (rc) return rc;
    }
    if (int rc = first_flush()) return rc;
    return poll();
  }

  // Bytes into pinned staging on the copy pool; the bytes each thread copied are counted by the
  // NUMA node it ran on (bsg_stream_stats)
  void par_copy(uint8_t* dst, const uint8_t* src, size_t n) {
    constexpr size_t kPiece = 2ull << 20;  // per thread, at least
    const bool nt_ok = bsg::copy_nt_enabled() && n >= kPiece;
    auto one = [this, nt_ok](uint8_t* d, const uint8_t* s, size_t m) {
      if (nt_ok)
        bsg::copy_nt(d, s, m);
      else
        std::memcpy(d, s, m);
      const int nd = bsg::cpu_node();
      if (nd >= 0 && nd < 4) node_bytes[nd].fetch_add(m, std::memory_order_relaxed);
    };
    const size_t nt = std::min<size_t>((size_t)copy_threads(), n / kPiece);
    if (nt <= 1) {
      one(dst, src, n);
      return;
    }
    // 1 MiB slices taken dynamically, so a thread that wakes late or runs slow takes fewer
    // (one slice per thread left the others waiting for it)
    const size_t ns = (n + kCopySlice - 1) / kCopySlice;
    parallel_for(ns, [=](size_t k) {
      const size_t o = k * kCopySlice;
      one(dst + o, src + o, std::min(kCopySlice, n - o));
    });
  }

  // Start a new stream on the same buffers (bsg_reset): everything in flight is waited for and
  // discarded, also after a device error (Counters::error is per run: the buffers stay valid).
  // Only a failing HIP call (a real fault) leaves the context unusable: bsg_free it.
  int reset() {
    if (cstream) HCHECK(hipStreamSynchronize(cstream));
    for (DataSlot& ds : data) ds.free_pending = false;
    for (int k = 0; k < nslots; ++k) {
      TileSlot& t = slots[k];
      if (t.eng) HCHECK(hipStreamSynchronize(t.eng->stream));
      t.busy = false;
      t.sel_read = t.recs_enq = false;
      if (t.eng) t.eng->enqueued = false;
    }
    // Full-size stages go back to the process-wide pool, last stage first: the pool is a stack
    // and the next stream takes stage 0's buffer first, so every stream of the context gets the
    // same buffer in the same stage. In the given order, the buffers came back reversed at every
    // reset, and every other 1 GiB rep ran ~3.5 ms (12 %) longer (profiles/r05_bench_final.log,
    // end_to_end.reps_ms: 28.1 / 32.3 / 28.4 ms).
    for (int k = kStages - 1; k >= 0; --k) {
      Stage& st = stages[k];
      if (st.inflight) HCHECK(hipEventSynchronize(st.ev));
      st.inflight = false;
      st.timed = false;
      StagePool::get().give(&st.buf);
    }
    for (auto& b : node_bytes) b.store(0);
    inflight.clear();
    ready.clear();
    static_cast<StreamState&>(*this) = StreamState{};
    return BSG_OK;
  }

  int close_begin() {
    if (fill == 0 && pos == stream0) return BSG_OK;  // empty stream: no chunks
    // The final segment must hold at least one byte: the open chunk's flush is emitted by the
    // scan of its last strip. write() and window() never submit a tile without leaving bytes
    // behind, so this cannot happen; fail loudly rather than drop the last chunk.
    if (fill == 0) return BSG_ESTATE;
    return submit(true);
  }
  int close_step(size_t* left) {  // the oldest tile on the device: wait, collect its records
    bool got = false;
    int rc = collect_front(true, &got);
    *left = inflight.size();
    return rc;
  }
  int close() {
    int rc = close_begin();
    for (size_t left = inflight.size(); rc == BSG_OK && left;) rc = close_step(&left);
    return rc;
  }
};

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

int64_t bsg_debug_get(int k) {
  if (k < BSG_KNOB_SEQ_WAIT || k > BSG_KNOB_LAST) return -1;
  return knob(k).load();
}

int bsg_debug_set(int k, int64_t value) {
  if (k < BSG_KNOB_SEQ_WAIT || k > BSG_KNOB_LAST || value < 0) return BSG_EINVAL;
  if (k == BSG_KNOB_LONG_MODE && value > 2) return BSG_EINVAL;
  if ((k == BSG_KNOB_EARLY || k == BSG_KNOB_POLL || k == BSG_KNOB_COPY_NT) && value > 1)
    return BSG_EINVAL;
  if (k == BSG_KNOB_SEQ_WAIT && value > (int64_t)UINT32_MAX) return BSG_EINVAL;  // a u32 poll count
  knob(k).store(value);
  return BSG_OK;
}

const char* bsg_errstr(int err) {
  switch (err) {
    case BSG_OK: return "ok";
    case BSG_EINVAL: return "invalid argument";
    case BSG_ENOMEM: return "out of memory";
    case BSG_EDEVICE: return "HIP device error";
    case BSG_ESTATE: return "invalid state (write after close?)";
    case BSG_ENODEV: return "no such HIP device";
    case BSG_ENOTFOUND: return "not found";
    case BSG_ECORRUPT: return "blob does not match its ref";
    case BSG_EIO: return "filesystem error";
    default: return "unknown error";
  }
}

bsg_params bsg_params_default(void) {
  bsg_params p;
  p.split_bits = 16;  // split/split.go:89
  p.min_size = 1024;  // split/split.go:88
  p.fanout = 8;       // split/split.go:48
  p.reserved = 0;
  return p;
}

void bsg_default_table(uint32_t out[256]) { std::memcpy(out, kBuzhash32Seed1, 1024); }

int bsg_init(int device) {
  if (device < 0 || device >= bsg_device_count()) return BSG_ENODEV;
  HCHECK(hipSetDevice(device));
  // streams for the pool. The first four get the process's hardware queues (GPU_MAX_HW_QUEUES,
  // 4); every further one still costs ~2.4 ms to create, and each live split::Writer holds
  // three (its hasher's, its first engine's, its copy stream): a Writer opened while others are
  // alive spent 7.5 of its 13 ms creating them (profiles/r03_fresh_ctx_api_trace.txt). So the
  // pool starts with BSG_INIT_STREAMS of them (default 16: five live Writers' worth).
  static const int kWarmStreams = [] {
    const char* v = std::getenv("BSG_INIT_STREAMS");
    const int n = v ? std::atoi(v) : 16;
    return std::max(1, std::min<int>(n, (int)kStreamPoolMax));
  }();
  hipStream_t s[kStreamPoolMax] = {};
  int got = 0;
  hipError_t e = hipSuccess;
  for (; got < kWarmStreams && e == hipSuccess; ++got) e = stream_acquire(device, &s[got]);
  if (e != hipSuccess) --got;
  // the device context, the copy engines and libbsgpu's code object: one small H2D, kernel and
  // D2H on each warm stream (the process's first DMA copy alone costs tens of ms)
  void* d = nullptr;
  PinBuf h;
  if (e == hipSuccess) e = hipMalloc(&d, 4096);
  if (e == hipSuccess) e = h.ensure(4096);
  for (int i = 0; i < got && e == hipSuccess; ++i) {
    e = hipMemcpyAsync(d, h.p, 2048, hipMemcpyHostToDevice, s[i]);
    if (e == hipSuccess) e = launch_copy_out(d, static_cast<uint8_t*>(d) + 2048, 64, s[i]);
    if (e == hipSuccess) e = hipMemcpyAsync(h.p, d, 64, hipMemcpyDeviceToHost, s[i]);
    if (e == hipSuccess) e = hipStreamSynchronize(s[i]);
  }
  if (d) (void)hipFree(d);
  h.release();
  for (int i = 0; i < got; ++i) stream_release(device, s[i]);
  HCHECK(e);
  // every kernel of the split and hash paths once (HIP loads a kernel at its first launch,
  // ~0.5 ms each, ~20 of them): a 64 KiB split, the same bytes as one blob, one blob per lane
  int rc = BSG_OK;
  bsg_engine* eng = bsg_engine_create(device, nullptr, &rc);
  if (!eng) return rc;
  constexpr uint64_t kWarm = 64 << 10;
  uint8_t* buf = static_cast<uint8_t*>(bsg_device_malloc(device, kWarm + kReadSlack));
  const uint64_t off = 0, len = kWarm;
  uint64_t n = 0;
  if (!buf) rc = BSG_ENOMEM;
  eng->early_min = 0;  // the early-chain kernels too (they pick nothing in 64 KiB)
  if (rc == BSG_OK) rc = bsg_fill_splitmix(device, buf, kWarm, 1, eng->stream);
  if (rc == BSG_OK) rc = bsg_engine_run(eng, buf, &off, &len, 1, nullptr);
  if (rc == BSG_OK) rc = bsg_engine_finish(eng, &n);
  if (rc == BSG_OK) rc = bsg_engine_hash(eng, buf, &off, &len, 1);
  if (rc == BSG_OK) rc = bsg_engine_finish(eng, &n);
  if (rc == BSG_OK) {
    uint8_t ref[32];
    uint8_t blob[64] = {0};
    const uint64_t boff = 0, blen = sizeof blob;
    bsg_hasher* hs = bsg_hasher_new(device);
    rc = hs ? bsg_hasher_sum(hs, blob, &boff, &blen, 1, ref) : BSG_EDEVICE;
    bsg_hasher_free(hs);
  }
  bsg_device_free(device, buf);
  bsg_engine_destroy(eng);
  if (rc) return rc;
  bsg::parallel_for(bsg::copy_threads(), [](size_t) {});  // the host copy pool's threads
  // a ring's worth of full-size pinned stages for the first large stream
  if ((rc = StagePool::get().fill(kStages))) return rc;
  // the streaming path once (registered staging, H2D from it, kernels writing into mapped
  // host memory, events): first uses the process would otherwise pay in its first Writer
  bsg_ctx* c = bsg_open(device, nullptr, nullptr, &rc);
  if (!c) return rc;
  std::vector<uint8_t> bytes(kWarm);
  for (size_t i = 0; i < bytes.size(); ++i) bytes[i] = (uint8_t)(i * 2654435761u >> 24);
  rc = bsg_write(c, bytes.data(), bytes.size());
  if (rc == BSG_OK) rc = bsg_close(c);
  bsg_free(c);
  return rc;
}

int bsg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

bsg_engine* bsg_engine_create(int device, const uint32_t* table, int* err) {
  int dummy;
  if (!err) err = &dummy;
  int n = bsg_device_count();
  if (device < 0 || device >= n) {
    *err = BSG_ENODEV;
    return nullptr;
  }
  bsg_engine* e = new (std::nothrow) bsg_engine();
  if (!e) {
    *err = BSG_ENOMEM;
    return nullptr;
  }
  e->dev = device;
  if (hipSetDevice(device) != hipSuccess ||
      stream_acquire(device, &e->stream) != hipSuccess) {
    delete e;
    *err = BSG_EDEVICE;
    return nullptr;
  }
  e->num_cus = device_cus(device);
  std::memcpy(e->htable, table ? table : kBuzhash32Seed1, sizeof e->htable);
  if (e->table.ensure(1024) != hipSuccess ||
      hipMemcpy(e->table.p, e->htable, 1024, hipMemcpyHostToDevice) != hipSuccess) {
    bsg_engine_destroy(e);
    *err = BSG_EDEVICE;
    return nullptr;
  }
  *err = BSG_OK;
  return e;
}

void bsg_engine_destroy(bsg_engine* e) {
  if (!e) return;
  hipSetDevice(e->dev);
  if (e->stream) hipStreamSynchronize(e->stream);
  if (e->hasher) {  // (it ran on e->stream, synchronised above)
    bsg_engine_destroy(e->hasher);
    e->hasher = nullptr;
  }
  DevBuf* tbufs[] = {&e->t_hdr, &e->t_cstart, &e->t_rmax, &e->t_kcnt, &e->t_tmp, &e->t_close,
                     &e->t_shbase, &e->t_meta, &e->t_pc, &e->t_pn, &e->t_aoff, &e->t_part,
                     &e->t_descs, &e->t_arena, &e->t_nodes, &e->t_roots, &e->t_ncount};
  for (DevBuf* b : tbufs) b->release();
  e->h_thdr.release();
  e->dd.release();
  for (hipEvent_t ev : e->dd_ev)
    if (ev) hipEventDestroy(ev);
  DevBuf* rbufs[] = {&e->r_in, &e->r_tab, &e->r_seg, &e->r_runs, &e->r_descs};
  for (DevBuf* b : rbufs) b->release();
  e->h_rin.release();
  e->h_rhdr.release();
  for (hipEvent_t ev : e->rs_ev)
    if (ev) hipEventDestroy(ev);
  for (hipEvent_t ev : e->tev)
    if (ev) hipEventDestroy(ev);
  // a failed run may have left early chains (k_pick / k_early on estream) that the engine
  // stream never waited for: they read cand, ctr and the data, so they end before any release
  if (e->estream) hipStreamSynchronize(e->estream);
  DevBuf* bufs[] = {&e->table, &e->streams, &e->strip0, &e->counts, &e->refine, &e->slots,
                    &e->strip_off, &e->partials_a, &e->partials_b, &e->cand, &e->flags,
                    &e->fidx, &e->bnd_end, &e->bnd_info, &e->scount, &e->last_end,
                    &e->out, &e->carry, &e->ctr, &e->long_list, &e->order, &e->buckets, &e->jinfo, &e->jdesc,
                    &e->regions, &e->oreg, &e->rorder};
  for (DevBuf* b : bufs) b->release();
  for (int i = 0; i < 4; ++i)
    if (e->ev[i]) hipEventDestroy(e->ev[i]);
  e->h_streams.release();
  e->h_strip0.release();
  e->h_ctr.release();
  e->h_snap.release();
  if (e->sel_ev) hipEventDestroy(e->sel_ev);
  if (e->cand_ev) hipEventDestroy(e->cand_ev);
  if (e->pick_ev) hipEventDestroy(e->pick_ev);
  if (e->early_ev) hipEventDestroy(e->early_ev);
  if (e->estream) stream_release(e->dev, e->estream);  // (synchronised above)
  if (e->stream && !e->borrowed_stream) stream_release(e->dev, e->stream);
  delete e;
}

// Checks a device-resident batch (a 16-byte aligned base and offsets, streams under 2^40 bytes
// whose ends do not wrap, the read slack inside the allocation) and fills the engine's
// descriptors: fresh, final streams. The streams may lie in any order, apart or on top of each
// other. The argument checks come before the first HIP call: a wrapped off + len would pass the
// allocation check below and hand the kernels a wild address.
static int engine_batch(bsg_engine* e, const uint8_t* d_data, const uint64_t* off,
                        const uint64_t* len, uint32_t nstreams) {
  if (!e || (nstreams && (!d_data || !off || !len)) || nstreams > 65535) return BSG_EINVAL;
  if (reinterpret_cast<uintptr_t>(d_data) % 16 != 0) return BSG_EINVAL;
  uint64_t hi = 0;  // an empty stream's offset counts too: it is still an address in d_data
  for (uint32_t s = 0; s < nstreams; ++s) {
    if (off[s] % 16 != 0 || len[s] >= (1ull << 40)) return BSG_EINVAL;
    if (off[s] > UINT64_MAX - len[s]) return BSG_EINVAL;
    hi = std::max<uint64_t>(hi, off[s] + len[s]);
  }
  int rc;
  if ((rc = e->setdev())) return rc;
  // the SHA-256 loader reads up to kReadSlack bytes past a stream's end (masked): that memory
  // must belong to the same allocation
  if (nstreams) {
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)d_data) != hipSuccess) {
      (void)hipGetLastError();
      return BSG_EINVAL;  // not a HIP device allocation
    }
    const uint64_t avail = (uint64_t)((const uint8_t*)base + size - d_data);
    if (avail < kReadSlack || hi > avail - kReadSlack) {  // (hi + kReadSlack could wrap)
      std::fprintf(stderr, "bsgpu: device buffer needs %llu readable bytes after the last "
                           "stream (has %llu)\n", (unsigned long long)kReadSlack,
                   (unsigned long long)(avail > hi ? avail - hi : 0));
      return BSG_EINVAL;
    }
  }
  e->descs.assign(nstreams, StreamDesc{});
  for (uint32_t s = 0; s < nstreams; ++s) {
    StreamDesc& d = e->descs[s];
    d.data_off = off[s];
    d.len = len[s];
    d.seg_base = 0;
    d.open_start = 0;
    d.consumed = 0;
    d.finalize = 1;
    d.prefix_len = 0;
    std::memcpy(d.mid, kIV, sizeof kIV);
  }
  e->d_data = d_data;
  e->nstreams = nstreams;
  return BSG_OK;
}

int bsg_engine_run(bsg_engine* e, const uint8_t* d_data, const uint64_t* off, const uint64_t* len,
                   uint32_t nstreams, const bsg_params* params) {
  Params p;
  bsg_params norm;
  int rc = normalize(params, &p, &norm);
  if (rc) return rc;
  if (e) e->run_done = false;
  if ((rc = engine_batch(e, d_data, off, len, nstreams))) return rc;
  e->p = p;
  e->fanout = norm.fanout;
  e->hash_mode = false;
  return e->enqueue();
}

int bsg_engine_hash(bsg_engine* e, const uint8_t* d_data, const uint64_t* off, const uint64_t* len,
                    uint32_t nblobs) {
  if (e) e->run_done = false;
  int rc = engine_batch(e, d_data, off, len, nblobs);
  if (rc) return rc;
  normalize(nullptr, &e->p, nullptr);
  e->hash_mode = true;
  return e->enqueue_hash();
}

int bsg_engine_finish(bsg_engine* e, uint64_t* nchunks) {
  if (!e) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  return e->finish(nchunks);
}

const bsg_chunk* bsg_engine_chunks_device(const bsg_engine* e) {
  return e ? static_cast<const bsg_chunk*>(e->out.p) : nullptr;
}

int bsg_engine_copy_chunks(bsg_engine* e, bsg_chunk* out, uint64_t cap) {
  if (!e || (!out && cap)) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  const uint64_t n = std::min<uint64_t>(cap, e->last.nchunks);
  if (n) HCHECK(hipMemcpy(out, e->out.p, sizeof(bsg_chunk) * n, hipMemcpyDeviceToHost));
  return BSG_OK;
}

int bsg_engine_copy_counts(bsg_engine* e, uint64_t* counts, uint32_t nstreams) {
  if (!e || !counts || nstreams > e->nstreams) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  if (nstreams)
    HCHECK(hipMemcpy(counts, e->scount.p, sizeof(uint64_t) * nstreams, hipMemcpyDeviceToHost));
  return BSG_OK;
}

void* bsg_engine_stream(bsg_engine* e) { return e ? (void*)e->stream : nullptr; }

int bsg_engine_trees(bsg_engine* e, uint64_t* nnodes, uint64_t* arena_bytes) {
  if (!e || !nnodes || !arena_bytes) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  if ((rc = e->trees())) return rc;
  *nnodes = e->tree.nn;
  *arena_bytes = e->tree.arena;
  return BSG_OK;
}

int bsg_engine_copy_roots(bsg_engine* e, uint8_t* roots, uint64_t* node_counts,
                          uint32_t nstreams) {
  if (!e || !roots) return BSG_EINVAL;
  if (!e->tree_valid || !e->run_done) return BSG_ESTATE;
  if (nstreams > e->tree.ns) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  if (nstreams) {
    HCHECK(hipMemcpy(roots, e->t_roots.p, 32ull * nstreams, hipMemcpyDeviceToHost));
    if (node_counts)
      HCHECK(hipMemcpy(node_counts, e->t_ncount.p, 8ull * nstreams, hipMemcpyDeviceToHost));
  }
  return BSG_OK;
}

int bsg_engine_copy_tree_nodes(bsg_engine* e, bsg_tree_node* out, uint64_t cap, uint8_t* arena,
                               uint64_t arena_cap) {
  if (!e || (!out && cap) || (!arena && arena_cap)) return BSG_EINVAL;
  if (!e->tree_valid || !e->run_done) return BSG_ESTATE;
  int rc = e->setdev();
  if (rc) return rc;
  const uint64_t n = std::min<uint64_t>(cap, e->tree.nn);
  const uint64_t nb = std::min<uint64_t>(arena_cap, e->tree.arena);
  if (n) HCHECK(hipMemcpy(out, e->t_nodes.p, sizeof(bsg_tree_node) * n, hipMemcpyDeviceToHost));
  if (nb) HCHECK(hipMemcpy(arena, e->t_arena.p, nb, hipMemcpyDeviceToHost));
  return BSG_OK;
}

const bsg_tree_node* bsg_engine_tree_nodes_device(const bsg_engine* e) {
  return e && e->tree_valid && e->run_done ? static_cast<const bsg_tree_node*>(e->t_nodes.p)
                                           : nullptr;
}

const uint8_t* bsg_engine_tree_arena_device(const bsg_engine* e) {
  return e && e->tree_valid && e->run_done ? e->t_arena.as<uint8_t>() : nullptr;
}

const uint8_t* bsg_engine_roots_device(const bsg_engine* e) {
  return e && e->tree_valid && e->run_done ? e->t_roots.as<uint8_t>() : nullptr;
}

int bsg_engine_dedup(bsg_engine* e, bsg_refset* set, uint64_t* nunique, uint64_t* unique_bytes) {
  if (!e || !nunique || !unique_bytes || (set && set->dev != e->dev)) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  if ((rc = e->dedup(set))) return rc;
  *nunique = e->dd_nunique;
  *unique_bytes = e->dd_bytes;
  return BSG_OK;
}

int bsg_engine_copy_dedup(bsg_engine* e, uint64_t* first, uint64_t cap_first, uint64_t* uniq,
                          uint64_t* pack_off, uint64_t cap_uniq) {
  if (!e) return BSG_EINVAL;
  if (!e->dd_valid || !e->run_done) return BSG_ESTATE;
  int rc = e->setdev();
  if (rc) return rc;
  const uint64_t nf = std::min<uint64_t>(cap_first, e->dd_n);
  const uint64_t nu = std::min<uint64_t>(cap_uniq, e->dd_nunique);
  if (first && nf) HCHECK(hipMemcpy(first, e->dd.first.p, 8 * nf, hipMemcpyDeviceToHost));
  if (uniq && nu) HCHECK(hipMemcpy(uniq, e->dd.uniq.p, 8 * nu, hipMemcpyDeviceToHost));
  if (pack_off) HCHECK(hipMemcpy(pack_off, e->dd.pack_off.p, 8 * (nu + 1), hipMemcpyDeviceToHost));
  return BSG_OK;
}

const uint64_t* bsg_engine_dedup_first_device(const bsg_engine* e) {
  return e && e->dd_valid && e->run_done ? e->dd.first.as<uint64_t>() : nullptr;
}

const uint64_t* bsg_engine_dedup_uniq_device(const bsg_engine* e) {
  return e && e->dd_valid && e->run_done ? e->dd.uniq.as<uint64_t>() : nullptr;
}

const uint64_t* bsg_engine_dedup_pack_off_device(const bsg_engine* e) {
  return e && e->dd_valid && e->run_done ? e->dd.pack_off.as<uint64_t>() : nullptr;
}

int bsg_engine_pack_unique(bsg_engine* e, uint8_t* d_out, uint64_t cap) {
  if (!e) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  return e->pack_unique(d_out, cap);
}

static_assert(sizeof(bsg_pool_blob) == sizeof(PoolBlob), "bsg_pool_blob layout");
static_assert(sizeof(bsg_restore_info) == 32, "bsg_restore_info layout");

int bsg_engine_restore(bsg_engine* e, const uint8_t* d_pool, uint64_t pool_bytes,
                       const bsg_pool_blob* blobs, uint64_t nblobs, const bsg_chunk* recs,
                       uint64_t nrecs, uint8_t* d_out, uint64_t out_cap, const uint64_t* out_off,
                       const uint64_t* out_len, uint32_t nstreams, int flags,
                       bsg_restore_info* info) {
  if (info) *info = bsg_restore_info{UINT64_MAX, UINT64_MAX, 0, 0};
  if (!e) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  return e->restore(d_pool, pool_bytes, blobs, nblobs, recs, nrecs, d_out, out_cap, out_off,
                    out_len, nstreams, flags, info);
}

// Test and measurement tooling (not in bsgpu.h): the last bsg_engine_restore call's passes in
// ms (index + resolve + tiling check, verify, scatter), with bsg_engine_profile on.
extern "C" int bsg_engine_restore_ms_debug(const bsg_engine* e, float out[3]) {
  if (!e || !out) return BSG_EINVAL;
  if (!e->profile) return BSG_ESTATE;
  for (int i = 0; i < 3; ++i) out[i] = e->rs_ms[i];
  return BSG_OK;
}

// Test and measurement tooling (not in bsgpu.h): the last bsg_engine_dedup and
// bsg_engine_pack_unique calls in ms, timed with HIP events on the engine stream when
// bsg_engine_profile is on; the pack kernel's load variant (1: aligned loads and a byte funnel);
// one hipMemcpyDtoDAsync of n bytes on the engine stream timed the same way.
extern "C" int bsg_engine_dedup_ms_debug(const bsg_engine* e, float out[2]) {
  if (!e || !out) return BSG_EINVAL;
  if (!e->profile || !e->dd_valid) return BSG_ESTATE;
  out[0] = e->dd_ms[0];
  out[1] = e->dd_ms[1];
  return BSG_OK;
}

extern "C" int bsg_engine_pack_mode_debug(bsg_engine* e, int funnel) {
  if (!e || funnel < 0 || funnel > 1) return BSG_EINVAL;
  e->pack_funnel = funnel != 0;
  return BSG_OK;
}

extern "C" int bsg_engine_d2d_ms_debug(bsg_engine* e, void* dst, const void* src, uint64_t n,
                                       float* ms) {
  if (!e || !dst || !src || !ms) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  hipEvent_t a = nullptr, b = nullptr;
  HCHECK(hipEventCreate(&a));
  if (hipEventCreate(&b) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipEventDestroy(a);
    return BSG_EDEVICE;
  }
  hipError_t err = hipEventRecord(a, e->stream);
  if (err == hipSuccess)
    err = hipMemcpyDtoDAsync((hipDeviceptr_t)dst, (hipDeviceptr_t)src, n, e->stream);
  if (err == hipSuccess) err = hipEventRecord(b, e->stream);
  if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
  if (err == hipSuccess) err = hipEventElapsedTime(ms, a, b);
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  if (err != hipSuccess) (void)hipGetLastError();
  return herr(err);
}

// ---- bsg_refset ---------------------------------------------------------------------------
bsg_refset* bsg_refset_new(int device, int* err) {
  int dummy;
  if (!err) err = &dummy;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    n = 0;
  }
  if (device < 0 || device >= n) {
    *err = BSG_ENODEV;
    return nullptr;
  }
  bsg_refset* s = new (std::nothrow) bsg_refset();
  if (!s) {
    *err = BSG_ENOMEM;
    return nullptr;
  }
  s->dev = device;
  *err = BSG_EDEVICE;
  if (hipSetDevice(device) == hipSuccess && stream_acquire(device, &s->stream) == hipSuccess) {
    s->num_cus = device_cus(device);
    s->slots = kRefSetSlots0;
    s->key_cap = kRefSetSlots0;
    *err = BSG_ENOMEM;
    if (s->tab.ensure(8 * s->slots) == hipSuccess && s->keys.ensure(32 * s->key_cap) == hipSuccess) {
      *err = herr(hipMemset(s->tab.p, 0xFF, 8 * s->slots));
      if (*err == BSG_OK) return s;
    }
  }
  (void)hipGetLastError();
  bsg_refset_free(s);
  return nullptr;
}

void bsg_refset_free(bsg_refset* s) {
  if (!s) return;
  hipSetDevice(s->dev);
  if (s->stream) {
    hipStreamSynchronize(s->stream);
    stream_release(s->dev, s->stream);
  }
  s->keys.release();
  s->tab.release();
  s->staged.release();
  s->work.release();
  delete s;
}

uint64_t bsg_refset_count(const bsg_refset* s) { return s ? s->count.load() : 0; }

int bsg_refset_add(bsg_refset* s, const uint8_t* refs, uint64_t n, uint8_t* added) {
  if (!s || (n && !refs) || n > (1ull << 40)) return BSG_EINVAL;
  std::lock_guard<std::mutex> g(s->mu);
  if (s->dead) return BSG_ESTATE;
  HCHECK(hipSetDevice(s->dev));
  if (!n) return BSG_OK;
  int rc;
  uint64_t slots = 0;
  if ((rc = s->work.reserve(n, &slots))) return rc;
  MCHECK(s->staged.ensure(32 * n));
  HCHECK(hipMemcpyAsync(s->staged.p, refs, 32 * n, hipMemcpyHostToDevice, s->stream));
  HCHECK(hipMemsetAsync(s->work.hdr.p, 0, sizeof(DedupHdr), s->stream));
  HCHECK(hipMemsetAsync(s->work.tab.p, 0xFF, 8 * slots, s->stream));
  DedupArgs a = s->work.args(s->staged.as<uint8_t>(), 32, nullptr, 0, n, slots);
  s->lookup_args(&a);
  HCHECK(dbg("launch_dedup", s->stream, launch_dedup(a, s->stream, s->num_cus)));
  if ((rc = s->work.readback(s->stream))) {
    if (rc == BSG_EDEVICE) s->dead = true;
    return rc;
  }
  const uint64_t m = s->work.last.nunique;
  if (m > n) {
    s->dead = true;
    return BSG_EDEVICE;
  }
  std::vector<uint64_t> first;
  if (added) {
    try {
      first.resize(n);
    } catch (const std::bad_alloc&) {
      return BSG_ENOMEM;
    }
    HCHECK(hipMemcpy(first.data(), s->work.first.p, 8 * n, hipMemcpyDeviceToHost));
  }
  if ((rc = s->add_new(a, m, &s->work, s->stream))) return rc;
  if (added)
    for (uint64_t i = 0; i < n; ++i) added[i] = first[i] == i ? 1 : 0;
  return BSG_OK;
}

int bsg_engine_profile(bsg_engine* e, int enable) {
  if (!e || enable < 0 || enable > 2) return BSG_EINVAL;
  int rc = e->setdev();
  if (rc) return rc;
  if (enable && !e->ev[0])
    for (int i = 0; i < 4; ++i) HCHECK(hipEventCreate(&e->ev[i]));
  e->profile = enable;
  return BSG_OK;
}

int bsg_engine_stage_ms(const bsg_engine* e, float out[3]) {
  if (!e || !out || !e->profile) return BSG_EINVAL;
  for (int i = 0; i < 3; ++i) out[i] = e->stage_ms[i];
  return BSG_OK;
}

uint64_t bsg_engine_candidates(const bsg_engine* e) { return e ? e->last.ncand : 0; }

int bsg_engine_diag(const bsg_engine* e, uint64_t out[16]) {
  if (!e || !out) return BSG_EINVAL;
  out[0] = e->last.nlong;
  out[1] = e->last.long_thresh;
  out[2] = e->last.max_nblocks;
  for (int i = 0; i < 5; ++i) out[3 + i] = e->last.diag[i];
  for (int i = 0; i < 5; ++i) out[8 + i] = e->last.diag2[i];
  out[13] = e->last.nshort;
  out[14] = e->last.ntickets;
  out[15] = e->last.total_blocks;
  return BSG_OK;
}

// Experiment tooling (not in include/bsgpu.h): copies the region queues' state after the last
// run (tools/stress_regions.py).
extern "C" int bsg_engine_regions_debug(bsg_engine* e, void* out, uint64_t nbytes) {
  if (!e || !out || !e->regions.p) return BSG_EINVAL;
  if (e->setdev()) return BSG_EDEVICE;
  const uint64_t n = std::min<uint64_t>(nbytes, sizeof(Regions));
  if (hipStreamSynchronize(e->stream) != hipSuccess) return BSG_EDEVICE;
  return hipMemcpy(out, e->regions.p, n, hipMemcpyDeviceToHost) == hipSuccess ? BSG_OK : BSG_EDEVICE;
}

// Test tooling (not in include/bsgpu.h): which SHA-256 path the last finished run's jobs took.
// out[0..3]: jobs on solo / group tickets, those tickets, the solo tickets run with a helper
// wave, all wave tickets (k_bucket_scan); out[4], out[5]: 1 if early chain 0 / 1 hashed a chunk
// (k_pick picked one and k_lens took it out of k_sha's queues), read from the Early record
// behind the device Counters; 0 after a hash run or a run without early chains.
extern "C" int bsg_engine_tiers_debug(bsg_engine* e, uint64_t out[6]) {
  if (!e || !out || e->enqueued) return BSG_EINVAL;
  out[0] = e->last.nlong_grp;
  out[1] = e->last.tickets_grp;
  out[2] = e->last.helped;
  out[3] = e->last.ntickets;
  out[4] = out[5] = 0;
  if (e->hash_mode || !e->ctr.p || e->ctr.cap < sizeof(Counters) + sizeof(Early)) return BSG_OK;
  if (e->setdev()) return BSG_EDEVICE;
  Early ea;
  if (hipStreamSynchronize(e->stream) != hipSuccess) return BSG_EDEVICE;
  if (hipMemcpy(&ea, e->dearly(), sizeof(Early), hipMemcpyDeviceToHost) != hipSuccess)
    return BSG_EDEVICE;
  for (int k = 0; k < kEarly; ++k) out[4 + k] = (ea.top[k] && ea.idx[k]) ? 1 : 0;
  return BSG_OK;
}

// Test tooling (not in include/bsgpu.h): the run size from which this engine's later runs take
// early chains (bsg_engine::early_min; kEarlyMinBytes by default, 0: every run). Nothing else
// changes: BSG_KNOB_EARLY, BSG_KNOB_LIGHT_BYTES, the snapshot and hash-mode gates hold as before.
// With it a planted run of a few hundred KiB goes through k_pick, k_early and k_early_fix.
extern "C" int bsg_engine_early_min_debug(bsg_engine* e, uint64_t bytes) {
  if (!e || e->enqueued) return BSG_EINVAL;
  e->early_min = bytes;
  return BSG_OK;
}

// Test tooling (not in include/bsgpu.h): what k_pick and k_lens left in the last finished run's
// Early record: out[0], out[1] = Early::top[0..1] ((blocks << 32) | candidate index, 0: no
// pick), out[2], out[3] = Early::idx[0..1] (1 + the picked chunk's record index, 0: not
// matched). Zeros after a hash run or a run without early chains (k_start clears the record of
// every split run, and only k_pick writes top).
extern "C" int bsg_engine_early_picks_debug(bsg_engine* e, uint64_t out[4]) {
  if (!e || !out || e->enqueued) return BSG_EINVAL;
  for (int k = 0; k < 2 * kEarly; ++k) out[k] = 0;
  if (e->hash_mode || !e->ctr.p || e->ctr.cap < sizeof(Counters) + sizeof(Early)) return BSG_OK;
  if (e->setdev()) return BSG_EDEVICE;
  Early ea;
  if (hipStreamSynchronize(e->stream) != hipSuccess) return BSG_EDEVICE;
  if (hipMemcpy(&ea, e->dearly(), sizeof(Early), hipMemcpyDeviceToHost) != hipSuccess)
    return BSG_EDEVICE;
  for (int k = 0; k < kEarly; ++k) {
    out[k] = ea.top[k];
    out[kEarly + k] = ea.idx[k];
  }
  return BSG_OK;
}

// Test tooling (not in include/bsgpu.h): Counters::rescan of the last finished run, the strips
// whose candidates outnumbered their kSlotCap slots and went through k_rescan; ~0 while a run is
// in flight or without an engine.
extern "C" uint64_t bsg_engine_rescan_debug(const bsg_engine* e) {
  return e && !e->enqueued ? e->last.rescan : ~0ull;
}

// Test and measurement tooling (not in bsgpu.h): the last bsg_engine_trees call's passes in ms,
// timed with HIP events on the engine stream when bsg_engine_profile is on: [0] counting and
// layout, [1] emit, [2] node hashes, [3] the whole call.
extern "C" int bsg_engine_trees_ms_debug(const bsg_engine* e, float out[4]) {
  if (!e || !out) return BSG_EINVAL;
  if (!e->profile || !e->tree_valid) return BSG_ESTATE;
  for (int i = 0; i < 4; ++i) out[i] = e->tree_ms[i];
  return BSG_OK;
}

int bsg_engine_timeline(const bsg_engine* e, uint64_t out[4]) {
  if (!e || !out) return BSG_EINVAL;
  out[0] = e->last.sha_start_rt;
  out[1] = e->last.diag[2];  // longest wave-mode job: start, end
  out[2] = e->last.diag[3];
  out[3] = e->last.lane_end_rt;
  return BSG_OK;
}

bsg_ctx* bsg_open(int device, const bsg_params* params, const uint32_t* table, int* err) {
  int dummy;
  if (!err) err = &dummy;
  Params p;
  bsg_params norm;
  int rc = normalize(params, &p, &norm);
  if (rc) {
    *err = rc;
    return nullptr;
  }
  if (device < 0 || device >= bsg_device_count()) {
    *err = BSG_ENODEV;
    return nullptr;
  }
  bsg_ctx* c = new (std::nothrow) bsg_ctx();
  if (!c) {
    *err = BSG_ENOMEM;
    return nullptr;
  }
  c->params = norm;
  c->p = p;
  if (hipSetDevice(device) != hipSuccess || (rc = c->init(device, table)) != BSG_OK) {
    c->release();
    delete c;
    *err = rc ? rc : BSG_EDEVICE;
    return nullptr;
  }
  *err = BSG_OK;
  return c;
}

int bsg_set_tile(bsg_ctx* c, size_t tile) {
  if (!c || tile < 4096 || c->fill || c->pos != c->stream0 || c->started) return BSG_EINVAL;
  c->tile = tile;
  return BSG_OK;
}

int bsg_set_carry_cap(bsg_ctx* c, size_t bytes) {
  if (!c || c->fill || c->pos != c->stream0 || c->started || bytes > 0xffffffffull)
    return BSG_EINVAL;
  c->carry_cap = bytes;
  return BSG_OK;
}

int bsg_set_stream_base(bsg_ctx* c, uint64_t base) {
  if (!c || c->fill || c->pos != c->stream0 || c->started || c->closed) return BSG_EINVAL;
  c->stream0 = c->pos = base;
  return BSG_OK;
}

int bsg_write(bsg_ctx* c, const uint8_t* p, size_t n) {
  if (!c) return BSG_EINVAL;
  if (c->closed) return BSG_ESTATE;
  if (c->sticky) return c->sticky;
  if (n && !p) return BSG_EINVAL;
  if (hipSetDevice(c->dev) != hipSuccess) return BSG_EDEVICE;
  c->started = true;
  int rc = c->write(p, n);
  if (rc) c->sticky = rc;
  return rc;
}

int bsg_host_register(void* p, size_t n) {
  if (!p || !n) return BSG_EINVAL;
  HCHECK(hipHostRegister(p, n, hipHostRegisterDefault));
  return BSG_OK;
}

int bsg_host_unregister(void* p) {
  if (!p) return BSG_EINVAL;
  HCHECK(hipHostUnregister(p));
  return BSG_OK;
}

int bsg_write_pinned(bsg_ctx* c, const uint8_t* p, size_t n) {
  if (!c) return BSG_EINVAL;
  if (c->closed) return BSG_ESTATE;
  if (c->sticky) return c->sticky;
  if (n && !p) return BSG_EINVAL;
  if (hipSetDevice(c->dev) != hipSuccess) return BSG_EDEVICE;
  c->started = true;
  int rc = c->write_pinned(p, n);
  if (rc) c->sticky = rc;
  return rc;
}

int bsg_write_window(bsg_ctx* c, uint8_t** p, size_t* cap) {
  if (!c || !p || !cap) return BSG_EINVAL;
  if (c->closed) return BSG_ESTATE;
  if (c->sticky) return c->sticky;
  if (hipSetDevice(c->dev) != hipSuccess) return BSG_EDEVICE;
  c->started = true;
  int rc = c->window(p, cap);
  if (rc) c->sticky = rc;
  return rc;
}

int bsg_write_commit(bsg_ctx* c, size_t n) {
  if (!c) return BSG_EINVAL;
  if (c->closed) return BSG_ESTATE;
  if (c->sticky) return c->sticky;
  if (hipSetDevice(c->dev) != hipSuccess) return BSG_EDEVICE;
  int rc = c->commit(n);
  if (rc) c->sticky = rc;
  return rc;
}

int bsg_close(bsg_ctx* c) {
  if (!c) return BSG_EINVAL;
  if (c->closed) return c->sticky;
  c->closed = true;
  if (c->sticky) return c->sticky;
  if (hipSetDevice(c->dev) != hipSuccess) return c->sticky = BSG_EDEVICE;
  int rc = c->close();
  if (rc) c->sticky = rc;
  return rc;
}

int bsg_close_begin(bsg_ctx* c) {
  if (!c) return BSG_EINVAL;
  if (c->closed) return c->sticky;
  c->closed = true;
  if (c->sticky) return c->sticky;
  if (hipSetDevice(c->dev) != hipSuccess) return c->sticky = BSG_EDEVICE;
  int rc = c->close_begin();
  if (rc) c->sticky = rc;
  return rc;
}

int bsg_close_step(bsg_ctx* c, size_t* left) {
  if (!c || !left) return BSG_EINVAL;
  *left = 0;
  if (!c->closed) return BSG_ESTATE;
  if (c->sticky) return c->sticky;
  if (c->inflight.empty()) return BSG_OK;
  if (hipSetDevice(c->dev) != hipSuccess) return c->sticky = BSG_EDEVICE;
  int rc = c->close_step(left);
  if (rc) c->sticky = rc;
  return rc;
}

size_t bsg_pending(const bsg_ctx* c) {
  if (!c) return 0;
  bsg_ctx* m = const_cast<bsg_ctx*>(c);  // polling completed tiles is not a visible change
  if (!m->sticky && hipSetDevice(m->dev) == hipSuccess) {
    int rc = m->poll();
    if (rc) m->sticky = rc;
  }
  return m->ready.size();
}

size_t bsg_drain(bsg_ctx* c, bsg_chunk* out, size_t cap) {
  if (!c || !out) return 0;
  if (!c->sticky && hipSetDevice(c->dev) == hipSuccess) {
    int rc = c->poll();
    if (rc) c->sticky = rc;
  }
  size_t k = 0;
  while (k < cap && !c->ready.empty()) {
    out[k++] = c->ready.front();
    c->ready.pop_front();
  }
  return k;
}

int bsg_reset(bsg_ctx* c) {
  if (!c) return BSG_EINVAL;
  if (hipSetDevice(c->dev) != hipSuccess) return BSG_EDEVICE;
  return c->reset();
}

void bsg_free(bsg_ctx* c) {
  if (!c) return;
  c->release();
  delete c;
}

int bsg_stream_stats_get(bsg_ctx* c, bsg_stream_stats* out) {
  if (!c || !out) return BSG_EINVAL;
  if (hipSetDevice(c->dev) != hipSuccess) return BSG_EDEVICE;
  return c->get_stats(out);
}

// bsg_split_hash_batch's engine: a pooled one (DevicePool) with the call's table, or a new one
static bsg_engine* batch_engine_take(int device, const uint32_t* table, int* rc) {
  bsg_engine* e = DevicePool<bsg_engine>::get().take(device);
  if (!e) return bsg_engine_create(device, table, rc);
  *rc = BSG_OK;
  const uint32_t* t = table ? table : kBuzhash32Seed1;
  if (std::memcmp(e->htable, t, sizeof e->htable) != 0) {
    std::memcpy(e->htable, t, sizeof e->htable);
    if (hipSetDevice(device) != hipSuccess ||
        hipMemcpy(e->table.p, e->htable, 1024, hipMemcpyHostToDevice) != hipSuccess) {
      bsg_engine_destroy(e);
      *rc = BSG_EDEVICE;
      return nullptr;
    }
  }
  return e;
}
static void batch_engine_give(bsg_engine* e, bool ok) {
  if (ok && hipSetDevice(e->dev) == hipSuccess && hipStreamSynchronize(e->stream) == hipSuccess) {
    e->retry_cap = 0;
    if (DevicePool<bsg_engine>::get().give(e)) return;
  }
  (void)hipGetLastError();
  bsg_engine_destroy(e);
}

int bsg_split_hash_batch(int device, const uint8_t* host_data, const uint64_t* off,
                         const uint64_t* len, uint32_t nstreams, const bsg_params* params,
                         const uint32_t* table, bsg_chunk* out, uint64_t cap, uint64_t* counts,
                         uint64_t* nchunks) {
  if (nstreams && (!host_data || !off || !len)) return BSG_EINVAL;
  if (!out && cap) return BSG_EINVAL;
  int rc;
  bsg_engine* e = batch_engine_take(device, table, &rc);
  if (!e) return rc;
  // Runs of at most 65,535 streams (the engine's limit) and about 8 GiB of device bytes (a
  // larger stream goes alone); each run's streams are packed 16-byte aligned into one buffer.
  constexpr uint32_t kRunStreams = 65535;
  constexpr uint64_t kRunBytes = 8ull << 30;
  constexpr uint64_t kPackWindow = 64ull << 20;
  DevBuf d;
  PinBuf pack;  // the packing window: a full-size stage from the process's pool when one is free
  pack.dma_only = true;
  std::vector<uint64_t> doff;
  uint64_t n = 0;  // records of all runs so far (written to out while they fit in cap)
  for (uint32_t s0 = 0; s0 < nstreams && rc == BSG_OK;) {
    uint32_t s1 = s0;
    uint64_t total = 0;
    doff.clear();
    while (s1 < nstreams && s1 - s0 < kRunStreams &&
           (s1 == s0 || total + len[s1] <= kRunBytes)) {
      doff.push_back(total);
      total += (len[s1] + 15) & ~15ull;
      ++s1;
    }
    if (d.ensure(total + kReadSlack) != hipSuccess) {
      rc = BSG_ENOMEM;
      break;
    }
    // Streams shorter than the pinned window are packed at their device offsets into it and
    // copied a window at a time (one H2D for many small streams); longer ones directly.
    const uint64_t win = std::min<uint64_t>(total, kPackWindow);
    static_assert(kPackWindow <= kStageMax, "a pooled stage holds the packing window");
    if (win && !pack.p) (void)StagePool::get().take(&pack);
    if (win && pack.ensure(win) != hipSuccess) {
      rc = BSG_ENOMEM;
      break;
    }
    uint64_t wlo = 0, whi = 0;  // device span [wlo, whi) staged in pack
    auto flush = [&]() {
      if (whi > wlo && hipMemcpy(static_cast<uint8_t*>(d.p) + wlo, pack.p, whi - wlo,
                                 hipMemcpyHostToDevice) != hipSuccess)
        rc = BSG_EDEVICE;
      wlo = whi;
    };
    for (uint32_t s = s0; s < s1 && rc == BSG_OK; ++s) {
      const uint64_t at = doff[s - s0];
      if (!len[s]) continue;
      if (len[s] > win / 2) {
        flush();
        if (rc == BSG_OK &&
            hipMemcpy(static_cast<uint8_t*>(d.p) + at, host_data + off[s], len[s],
                      hipMemcpyHostToDevice) != hipSuccess)
          rc = BSG_EDEVICE;
        wlo = whi = at + len[s];
        continue;
      }
      if (at + len[s] - wlo > win) flush();
      if (whi == wlo) wlo = whi = at;
      std::memcpy(pack.as<uint8_t>() + (at - wlo), host_data + off[s], len[s]);
      whi = at + len[s];
    }
    if (rc == BSG_OK) flush();
    uint64_t rn = 0;
    if (rc == BSG_OK) rc = bsg_engine_run(e, d.as<uint8_t>(), doff.data(), len + s0, s1 - s0, params);
    if (rc == BSG_OK) rc = bsg_engine_finish(e, &rn);
    if (rc == BSG_OK && n < cap) {
      rc = bsg_engine_copy_chunks(e, out + n, cap - n);
      // records name their stream within the run: make them batch indices
      for (uint64_t k = n; rc == BSG_OK && s0 && k < std::min(cap, n + rn); ++k) out[k].stream += s0;
    }
    if (rc == BSG_OK && counts) rc = bsg_engine_copy_counts(e, counts + s0, s1 - s0);
    n += rn;
    s0 = s1;
  }
  if (nchunks) *nchunks = n;
  d.release();
  StagePool::get().give(&pack);  // keeps a full-size registered stage, frees anything else
  batch_engine_give(e, rc == BSG_OK);
  return rc;
}

void* bsg_device_malloc(int device, size_t bytes) {
  if (device < 0 || device >= bsg_device_count() || hipSetDevice(device) != hipSuccess)
    return nullptr;
  void* p = nullptr;
  if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}

int bsg_device_free(int device, void* p) {
  if (!p) return BSG_OK;
  HCHECK(hipSetDevice(device));
  HCHECK(hipFree(p));
  return BSG_OK;
}

int bsg_memcpy(int device, void* dst, const void* src, size_t n, int kind) {
  if (n && (!dst || !src)) return BSG_EINVAL;
  HCHECK(hipSetDevice(device));
  hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice
                  : kind == 1 ? hipMemcpyDeviceToHost
                              : hipMemcpyDeviceToDevice;
  if (n) HCHECK(hipMemcpy(dst, src, n, k));
  return BSG_OK;
}

int bsg_device_synchronize(int device) {
  HCHECK(hipSetDevice(device));
  HCHECK(hipDeviceSynchronize());
  return BSG_OK;
}

int bsg_fill_splitmix(int device, uint8_t* d_ptr, uint64_t nbytes, uint64_t seed, void* stream) {
  if (!d_ptr && nbytes) return BSG_EINVAL;
  if (device < 0 || device >= bsg_device_count()) return BSG_ENODEV;
  HCHECK(hipSetDevice(device));
  const int cus = device_cus(device);
  if (nbytes) HCHECK(launch_fill_splitmix(d_ptr, nbytes, seed, (hipStream_t)stream, cus));
  return BSG_OK;
}

}  // extern "C"

// Batched Blob.Ref() with persistent device buffers and stream (bsg_hasher_*): a Writer hashes
// every tree node through one, so a call costs one H2D, one launch and one D2H, not four
// allocations.
// Copies n blobs src[so[k] .. +sl[k]) to dst + dofs[k], on up to copy_threads() threads, each
// taking a run of whole blobs of about total / threads bytes.
static void par_gather(uint8_t* dst, const uint8_t* src, const uint64_t* so,
                       const uint8_t* const* sp, const uint64_t* sl, const uint64_t* dofs,
                       uint32_t n, uint64_t total) {
  constexpr uint64_t kPiece = 2ull << 20;  // per thread, at least
  const uint64_t nt = std::min<uint64_t>((uint64_t)copy_threads(), total / kPiece);
  auto run = [=](uint32_t a, uint32_t b) {
    for (uint32_t k = a; k < b; ++k)
      if (sl[k]) std::memcpy(dst + dofs[k], sp ? sp[k] : src + so[k], sl[k]);
  };
  if (nt <= 1) {
    run(0, n);
    return;
  }
  std::vector<std::pair<uint32_t, uint32_t>> runs;
  const uint64_t per = (total + nt - 1) / nt;
  uint32_t a = 0;
  uint64_t acc = 0;
  for (uint32_t k = 0; k < n; ++k) {
    acc += sl[k];
    if (acc >= per || k + 1 == n) {
      runs.emplace_back(a, k + 1);
      a = k + 1;
      acc = 0;
    }
  }
  parallel_for(runs.size(), [&](size_t i) { run(runs[i].first, runs[i].second); });
}

struct bsg_hasher {
  int dev = 0;
  int num_cus = 256;
  hipStream_t stream = nullptr;
  DevBuf data, off, len, refs;
  PinBuf h_meta;  // off[n] | len[n] staged for one H2D
  PinBuf h_small; // a small batch's host bytes, then its refs: pinned, so both copies are DMA
  // Large batches (the verifying split.Reader, bsg_sha256_batch of many blobs): the blobs are
  // packed at 16-byte offsets into pinned staging and hashed by an engine in bsg_engine_hash
  // mode, whose wave-mode chains take the longest blobs (k_sha_blobs hashes one blob per lane,
  // so a batch waits for its longest blob at per-lane speed, ~2.5x slower per block).
  static constexpr uint32_t kEngineMinBlobs = 16;
  static constexpr uint64_t kEngineMinBytes = 4ull << 20;
  static constexpr uint64_t kEngineLongBlob = 16ull << 10;  // (small batches, see sum())
  static constexpr uint64_t kEngineBatch = 256ull << 20;  // bytes per engine run (one blob may exceed)
  static constexpr uint64_t kGatherPiece = 32ull << 20;   // packed and copied to the device at once
  bsg_engine* eng = nullptr;
  PinBuf stage;
  PinBuf h_recs;  // an engine run's records, D2H
  DevBuf dstage;
  std::vector<uint64_t> aoff;

  // blob k is base + o[k], or ptrs[k] when ptrs is given (scattered blobs, e.g. a store's)
  int sum_engine(const uint8_t* base, const uint64_t* o, const uint8_t* const* ptrs,
                 const uint64_t* l, uint32_t n, uint8_t* out) {
    int err = 0;
    if (!eng && !(eng = bsg_engine_create(dev, nullptr, &err))) return err ? err : BSG_EDEVICE;
    hipStream_t es = static_cast<hipStream_t>(bsg_engine_stream(eng));
    stage.dma_only = true;  // read only by the H2D: a registered huge-page mapping pins faster
    uint64_t left = 0;      // bytes of the blobs not yet in a run
    for (uint32_t k = 0; k < n; ++k) left += l[k];
    // a small batch (see sum()) puts every blob on wave tickets: the engine's own choice keeps
    // blobs under kLongMinBlocks (64 KiB) per-lane
    eng->hash_long_mode = left < kEngineMinBytes ? 2 : -1;
    for (uint32_t i = 0; i < n;) {
      // A run is up to kEngineBatch bytes, or everything left if that is at most a quarter more:
      // every run waits for its longest blob's chain (~10 ms for a 256 MiB run), so a small
      // remainder run (a verifying Reader's window just over 256 MiB) doubled the wait.
      const uint64_t cap = left <= kEngineBatch + kEngineBatch / 4 ? UINT64_MAX : kEngineBatch;
      uint64_t bytes = 0;
      uint32_t j = i;
      aoff.clear();
      while (j < n && j - i < 65535u) {
        const uint64_t a = (bytes + 15) & ~15ull;
        if (j > i && a + l[j] > cap) break;
        aoff.push_back(a);
        bytes = a + l[j];
        left -= l[j];
        ++j;
      }
      // sized once for the largest run (a growth re-pins: ~35 ms per 256 MiB)
      const uint64_t want =
          bytes >= kEngineBatch / 2 ? std::max(bytes, kEngineBatch + kEngineBatch / 4) : bytes;
      HCHECK(stage.ensure(want + kReadSlack));
      HCHECK(dstage.ensure(want + kReadSlack));
      // gathered a piece at a time, each piece's H2D queued as soon as it is packed, so the copy
      // engine moves piece k while the host threads pack piece k+1
      for (uint32_t a = 0; a < j - i;) {
        uint32_t b = a;
        uint64_t pbytes = 0;
        while (b < j - i && (b == a || pbytes < kGatherPiece)) pbytes += l[i + b++];
        const uint64_t lo = aoff[a];
        const uint64_t hi = (b < j - i) ? aoff[b] : bytes;
        par_gather(stage.as<uint8_t>(), base, o ? o + i + a : nullptr,
                   ptrs ? ptrs + i + a : nullptr, l + i + a, aoff.data() + a, b - a, pbytes);
        if (hi > lo)
          HCHECK(hipMemcpyAsync(dstage.as<uint8_t>() + lo, stage.as<uint8_t>() + lo, hi - lo,
                                hipMemcpyHostToDevice, es));
        a = b;
      }
      int rc = bsg_engine_hash(eng, dstage.as<uint8_t>(), aoff.data(), l + i, j - i);
      uint64_t nch = 0;
      if (!rc) rc = bsg_engine_finish(eng, &nch);
      if (!rc && nch != j - i) rc = BSG_EDEVICE;
      if (rc) return rc;
      // the records through pinned memory (a D2H into a fresh pageable vector cost ~12 ms the
      // first time: the runtime pins its pages)
      HCHECK(h_recs.ensure(sizeof(bsg_chunk) * (j - i)));
      HCHECK(hipMemcpyAsync(h_recs.p, eng->out.p, sizeof(bsg_chunk) * (j - i),
                            hipMemcpyDeviceToHost, es));
      HCHECK(hipStreamSynchronize(es));
      const bsg_chunk* rec = h_recs.as<bsg_chunk>();
      for (uint32_t k = 0; k < j - i; ++k) std::memcpy(out + 32ull * (i + k), rec[k].ref, 32);
      i = j;
    }
    return BSG_OK;
  }

  int sum(const uint8_t* base, const uint64_t* o, const uint64_t* l, uint32_t n, uint8_t* out) {
    static const bool dbg_times = std::getenv("BSG_DEBUG_HASHER") != nullptr;
    const auto t_in = std::chrono::steady_clock::now();
    struct Report {  // BSG_DEBUG_HASHER: where one call's time went (stderr)
      bool on;
      std::chrono::steady_clock::time_point t0;
      uint32_t n;
      uint64_t marks[4] = {};
      ~Report() {
        if (on)
          std::fprintf(stderr, "bsgpu hasher: %u blobs, %.3f ms (ensure %.3f, copies %.3f, launch %.3f)\n",
                       n, ns_since(t0) / 1e6, marks[0] / 1e6, (marks[1] - marks[0]) / 1e6,
                       (marks[2] - marks[1]) / 1e6);
      }
    } rep{dbg_times, t_in, n};
    // a wrapped off + len would size the private copy below by a small `hi` and leave the
    // kernel a wild address: refused before anything is allocated or copied
    for (uint32_t i = 0; i < n; ++i)
      if (o[i] > UINT64_MAX - l[i]) return BSG_EINVAL;
    hipPointerAttribute_t attr;
    bool on_device = false;
    if (hipPointerGetAttributes(&attr, base) == hipSuccess)
      on_device = (attr.type == hipMemoryTypeDevice);
    else
      (void)hipGetLastError();
    uint64_t hi = 0, total = 0, longest = 0;
    for (uint32_t i = 0; i < n; ++i) {
      hi = std::max<uint64_t>(hi, o[i] + l[i]);
      total += l[i];
      longest = std::max<uint64_t>(longest, l[i]);
    }
    if (!on_device && n >= kEngineMinBlobs && total >= kEngineMinBytes)
      return sum_engine(base, o, nullptr, l, n, out);
    // A small batch with a long blob goes to the engine too, every blob on a wave ticket: one
    // blob per lane hashes a block per ~6,000-8,000 cycles and the batch waits for its longest
    // blob, where a solo wave chain takes ~2,300 (plus ~0.1 ms of launches). A split::Writer's tree nodes are such a batch:
    // their leaf counts are geometric, so 1 GiB's 63 nodes of ~11 KB include one of ~50 KB, and
    // k_sha_blobs took 2.7-3.1 ms for them (profiles/r06_writer_trace_kernel_stats.csv). Its
    // staging stays the batch's size (< kEngineMinBytes), so a pooled hasher pins nothing big.
    if (!on_device && n >= 2 && total < kEngineMinBytes && longest >= kEngineLongBlob)
      return sum_engine(base, o, nullptr, l, n, out);
    // always hash from a private copy with kReadSlack bytes of tail padding
    HCHECK(data.ensure(hi + kReadSlack));
    HCHECK(off.ensure(8ull * n));
    HCHECK(len.ensure(8ull * n));
    HCHECK(refs.ensure(32ull * n));
    HCHECK(h_meta.ensure(16ull * n));
    std::memcpy(h_meta.p, o, 8ull * n);
    std::memcpy(h_meta.as<uint8_t>() + 8ull * n, l, 8ull * n);
    // Small host batches (tree nodes: pageable std::string) go through pinned memory, whose
    // H2D / D2H are single DMAs instead of the runtime's chunked staging of pageable memory.
    // The path is chosen by blob count, so one large blob can land here too: above
    // kEngineMinBytes its bytes are copied straight from pageable memory instead, so that a
    // pooled hasher never keeps a blob-sized pinned buffer (pinning costs ~50-65 ms per 256 MiB
    // and would stay held for the life of the process).
    const bool via_pinned = !on_device && hi <= kEngineMinBytes;
    HCHECK(h_small.ensure(std::max<uint64_t>(via_pinned ? hi : 0, 32ull * n)));
    rep.marks[0] = ns_since(t_in);
    if (hi) {
      if (on_device) {
        HCHECK(hipMemcpyAsync(data.p, base, hi, hipMemcpyDeviceToDevice, stream));
      } else if (!via_pinned) {
        HCHECK(hipMemcpyAsync(data.p, base, hi, hipMemcpyHostToDevice, stream));
      } else {
        std::memcpy(h_small.p, base, hi);
        HCHECK(hipMemcpyAsync(data.p, h_small.p, hi, hipMemcpyHostToDevice, stream));
      }
    }
    HCHECK(hipMemcpyAsync(off.p, h_meta.p, 8ull * n, hipMemcpyHostToDevice, stream));
    HCHECK(hipMemcpyAsync(len.p, h_meta.as<uint8_t>() + 8ull * n, 8ull * n,
                          hipMemcpyHostToDevice, stream));
    rep.marks[1] = ns_since(t_in);
    BlobShaArgs a{data.as<uint8_t>(), off.as<uint64_t>(), len.as<uint64_t>(), n,
                  refs.as<uint8_t>()};
    HCHECK(launch_sha_blobs(a, stream, num_cus));
    rep.marks[2] = ns_since(t_in);
    HCHECK(hipMemcpyAsync(h_small.p, refs.p, 32ull * n, hipMemcpyDeviceToHost, stream));
    HCHECK(hipStreamSynchronize(stream));
    std::memcpy(out, h_small.p, 32ull * n);
    return BSG_OK;
  }
};

extern "C" {

bsg_hasher* bsg_hasher_new(int device) {
  if (device < 0 || device >= bsg_device_count() || hipSetDevice(device) != hipSuccess)
    return nullptr;
  bsg_hasher* h = new (std::nothrow) bsg_hasher();
  if (!h) return nullptr;
  h->dev = device;
  h->num_cus = device_cus(device);
  if (stream_acquire(device, &h->stream) != hipSuccess) {
    delete h;
    return nullptr;
  }
  return h;
}

int bsg_hasher_sum(bsg_hasher* h, const uint8_t* base, const uint64_t* off, const uint64_t* len,
                   uint32_t n, uint8_t* refs) {
  if (!h || (n && (!base || !off || !len || !refs))) return BSG_EINVAL;
  if (n == 0) return BSG_OK;
  HCHECK(hipSetDevice(h->dev));
  return h->sum(base, off, len, n, refs);
}

int bsg_hasher_sum_ptrs(bsg_hasher* h, const uint8_t* const* ptrs, const uint64_t* len,
                        uint32_t n, uint8_t* refs) {
  if (!h || (n && (!ptrs || !len || !refs))) return BSG_EINVAL;
  if (n == 0) return BSG_OK;
  HCHECK(hipSetDevice(h->dev));
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (len[i] && !ptrs[i]) return BSG_EINVAL;
    total += len[i];
  }
  if (n >= bsg_hasher::kEngineMinBlobs && total >= bsg_hasher::kEngineMinBytes)
    return h->sum_engine(nullptr, nullptr, ptrs, len, n, refs);
  // small batches: packed, then the one-blob-per-lane kernel
  std::vector<uint8_t> packed(total ? total : 1);
  std::vector<uint64_t> off(n);
  uint64_t o = 0;
  for (uint32_t i = 0; i < n; ++i) {
    off[i] = o;
    if (len[i]) std::memcpy(packed.data() + o, ptrs[i], len[i]);
    o += len[i];
  }
  return h->sum(packed.data(), off.data(), len, n, refs);
}

size_t bsg_hasher_pinned_bytes(const bsg_hasher* h) {
  if (!h) return 0;
  return h->h_meta.cap + h->h_small.cap + h->stage.cap + h->h_recs.cap;
}

void bsg_hasher_free(bsg_hasher* h) {
  if (!h) return;
  hipSetDevice(h->dev);
  if (h->stream) hipStreamSynchronize(h->stream);
  h->data.release();
  h->off.release();
  h->len.release();
  h->refs.release();
  h->h_meta.release();
  h->h_small.release();
  h->stage.release();
  h->h_recs.release();
  h->dstage.release();
  if (h->eng) bsg_engine_destroy(h->eng);
  if (h->stream) stream_release(h->dev, h->stream);
  delete h;
}

// (hashers, with their device buffers, pinned staging and engine, are pooled: DevicePool)
int bsg_sha256_batch(int device, const uint8_t* base, const uint64_t* off, const uint64_t* len,
                     uint32_t n, uint8_t* refs) {
  if (n && (!base || !off || !len || !refs)) return BSG_EINVAL;
  if (n == 0) return BSG_OK;
  if (device < 0 || device >= bsg_device_count()) return BSG_ENODEV;
  bsg_hasher* h = DevicePool<bsg_hasher>::get().take(device);
  if (!h && !(h = bsg_hasher_new(device))) return BSG_EDEVICE;
  if (hipSetDevice(device) != hipSuccess) {
    bsg_hasher_free(h);
    return BSG_EDEVICE;
  }
  const int rc = h->sum(base, off, len, n, refs);
  // (sum() synchronised the hasher's streams)
  if (rc != BSG_OK || !DevicePool<bsg_hasher>::get().give(h)) bsg_hasher_free(h);
  return rc;
}

}  // extern "C"
