// host_tail_check.cpp — the host tail's hash workers (bs_amd/csrc/host_sha256.*) driven without a
// GPU: producer threads stand in for the gather kernel. They copy ranges into a shared ring and
// raise the ready flags out of order, and the count arrives after the workers have started. Every
// digest is compared with the portable implementation run on this thread. Built with the host
// sanitizers by tests/test_host_tail_workers_cpu.py:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread tools/host_tail_check.cpp
//       bs_amd/csrc/host_sha256.cpp -o host_tail_check   (one line), then ./host_tail_check
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../bs_amd/csrc/host_sha256.h"

using namespace bsg;

static int run(int threads, int impl, int producers) {
  const size_t lens[] = {0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 1000, 4096 + 7, 64 * 37 - 9,
                         64 * 37 - 8, 64 * 37, 64 * 37 + 1, 100003};
  const size_t nl = sizeof lens / sizeof lens[0];
  const size_t n = 3 * nl;  // each length at three misalignments
  std::vector<HashItem> items(n);
  std::vector<uint8_t> src, ring;
  size_t off = 0;
  for (size_t i = 0; i < n; ++i) {
    items[i] = HashItem{i, 0, lens[i % nl], off + (i / nl), 0, 0};
    off += (lens[i % nl] + 16 + 255) & ~(size_t)255;
  }
  src.resize(off + 64);
  ring.assign(off + 64, 0xEE);
  uint64_t x = 88172645463325252ull;
  for (uint8_t& b : src) {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    b = (uint8_t)(x >> 32);
  }
  std::vector<uint8_t> want(32 * n), got(32 * n, 0);
  for (size_t i = 0; i < n; ++i)
    sha256_range(src.data() + items[i].off, items[i].len, want.data() + 32 * i, kShaPortable);

  std::vector<uint32_t> ready(n, 0);
  uint64_t count = kCountUnknown;
  HashWorkers pool(threads);
  HashBatch b;
  b.count = &count;
  b.items = items.data();
  b.ready = ready.data();
  b.base = ring.data();
  b.base_len = ring.size();
  b.max_items = n;
  b.refs = got.data();
  b.impl = impl;
  pool.start(b);
  std::vector<std::thread> prod;
  for (int p = 0; p < producers; ++p)
    prod.emplace_back([&, p] {
      // producer p takes items p, p + producers, ... from the far end: flags rise out of order
      for (size_t k = 0; k < n; ++k) {
        const size_t i = n - 1 - k;
        if ((int)(i % (size_t)producers) != p) continue;
        std::memcpy(ring.data() + items[i].off, src.data() + items[i].off, items[i].len);
        __atomic_store_n(&ready[i], 1u, __ATOMIC_RELEASE);
      }
      if (p == 0) __atomic_store_n(&count, (uint64_t)n, __ATOMIC_RELEASE);
    });
  for (std::thread& t : prod) t.join();
  const uint64_t bad = pool.wait();
  int fails = bad ? 1 : 0;
  for (size_t i = 0; i < n; ++i)
    if (std::memcmp(got.data() + 32 * i, want.data() + 32 * i, 32) != 0) {
      std::fprintf(stderr, "digest %zu (len %zu) differs (impl %s, %d threads)\n", i,
                   (size_t)items[i].len, sha256_impl_name(impl), threads);
      ++fails;
    }
  if (pool.hashed_items() != n) ++fails;

  // a batch whose producer fails: cancel() frees the workers, wait() returns
  uint64_t never = kCountUnknown;
  b.count = &never;
  pool.start(b);
  pool.cancel();
  (void)pool.wait();
  return fails;
}

int main() {
  // "abc" (FIPS 180-4 appendix B.1) through both implementations
  static const uint8_t abc[32] = {0xba, 0x78, 0x16, 0xbf, 0x8f, 0x01, 0xcf, 0xea, 0x41, 0x41, 0x40,
                                  0xde, 0x5d, 0xae, 0x22, 0x23, 0xb0, 0x03, 0x61, 0xa3, 0x96, 0x17,
                                  0x7a, 0x9c, 0xb4, 0x10, 0xff, 0x61, 0xf2, 0x00, 0x15, 0xad};
  uint8_t d[32];
  int fails = 0;
  const int impls[2] = {kShaPortable, sha256_best_impl()};
  for (int impl : impls) {
    sha256_range(reinterpret_cast<const uint8_t*>("abc"), 3, d, impl);
    if (std::memcmp(d, abc, 32) != 0) {
      std::fprintf(stderr, "abc differs (%s)\n", sha256_impl_name(impl));
      ++fails;
    }
  }
  for (int impl : impls)
    for (int threads : {1, 4, 16}) fails += run(threads, impl, 3);
  std::printf("host_tail_check: %s (x86 sha: %d)\n", fails ? "FAILED" : "ok",
              (int)sha256_have_x86());
  return fails ? 1 : 0;
}
