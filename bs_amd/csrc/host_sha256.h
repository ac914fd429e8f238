// host_sha256.h — SHA-256 on the host (FIPS 180-4, portable and x86 SHA extensions) and the pool
// of hash workers an engine's host tail runs on (bsg_engine, "Host tail").
//
// A step of a lightly loaded run is its longest chunk's serial SHA-256 chain, ~0.95 us per
// 64-byte block on a lone GPU wave; a host core with the SHA extensions runs the same block tens
// of times faster. The run's few longest chunks are therefore hashed here, from a pinned ring the
// GPU copies them into, while the GPU hashes everything else.
//
// No HIP in this file: the workers see plain host memory and flags, so a stand-alone program
// (tools/host_tail_check.cpp) can drive them under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

namespace bsg {

enum ShaImpl : int { kShaAuto = -1, kShaPortable = 0, kShaX86 = 1 };

// cpuid: SHA extensions with SSE4.1 / SSSE3 (what sha256_x86 uses)
bool sha256_have_x86();
// the implementation kShaAuto resolves to on this host
int sha256_best_impl();
const char* sha256_impl_name(int impl);
// SHA-256 of p[0 .. n) into out[32]. impl: kShaAuto, or one of the two (kShaX86 on a host
// without the extension falls back to the portable one).
void sha256_range(const uint8_t* p, size_t n, uint8_t out[32], int impl = kShaAuto);
// bytes per second of one thread over a resident buffer of `bytes`, for about `ms` milliseconds
double sha256_measure_rate(int impl, size_t bytes, double ms);

// One range of a batch: base[off .. off + len) hashes to refs[32 * i].
struct HashItem {
  uint64_t job;     // the submitter's own tag (an engine: the chunk's record index)
  uint64_t start;   // (an engine: the chunk's stream offset)
  uint64_t len;
  uint64_t off;     // of the first byte, from the batch's base
  uint32_t stream;
  uint32_t level;
};
static_assert(sizeof(HashItem) == 40, "HashItem layout");

// A batch whose items, count and bytes arrive while the workers already run. Everything the
// producer (a GPU kernel writing pinned memory, or another thread) writes is read through
// acquire loads: *count first (kCountUnknown until the list is final), then per item ready[i]
// (nonzero once item i and its bytes are in place).
constexpr uint64_t kCountUnknown = ~0ull;
struct HashBatch {
  const uint64_t* count = nullptr;
  const HashItem* items = nullptr;
  const uint32_t* ready = nullptr;
  const uint8_t* base = nullptr;
  uint64_t base_len = 0;   // an item outside [0, base_len) is skipped and counted in `bad`
  uint64_t max_items = 0;  // a count above this is treated as max_items (and counted in `bad`)
  uint8_t* refs = nullptr;
  int impl = kShaAuto;
};

// At most 16 threads, created once and reused: sized from OMP_NUM_THREADS when set, else
// min(16, hardware_concurrency). A worker waits for a batch on a condition variable; inside a
// batch it polls the producer's flags with CPU pauses for a bounded time, then naps between polls.
class HashWorkers {
 public:
  explicit HashWorkers(int threads = 0);  // 0: the default size
  ~HashWorkers();                         // joins
  HashWorkers(const HashWorkers&) = delete;
  HashWorkers& operator=(const HashWorkers&) = delete;
  int threads() const { return (int)th_.size(); }
  static int default_threads();
  // One batch at a time: start() returns at once, wait() blocks until every item is hashed (or
  // the batch cancelled) and returns the number of bad items. cancel() makes the workers leave a
  // batch whose producer failed; wait() must still follow.
  void start(const HashBatch& b);
  void cancel();
  uint64_t wait();
  bool busy() const { return open_; }
  // steady_clock ns at which the last item of the last batch was finished (0: none was)
  int64_t last_done_ns() const { return last_ns_.load(std::memory_order_relaxed); }
  uint64_t hashed_items() const { return nhashed_.load(std::memory_order_relaxed); }

 private:
  void loop();
  void work(const HashBatch& b);
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_work_, cv_done_;
  HashBatch cur_{};
  uint64_t gen_ = 0;        // batches started
  int inside_ = 0;          // workers that have not left the current batch
  bool quit_ = false;
  bool open_ = false;       // start() without its wait()
  std::atomic<bool> cancel_{false};
  std::atomic<uint64_t> next_{0}, bad_{0}, nhashed_{0};
  std::atomic<int64_t> last_ns_{0};
};

}  // namespace bsg
