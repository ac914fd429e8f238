// host_sha256.cpp — see host_sha256.h.
#include "host_sha256.h"

#include <time.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

#if defined(__x86_64__) || defined(__i386__)
#define BSG_X86 1
#include <cpuid.h>
#include <immintrin.h>
#endif

namespace bsg {
namespace {

alignas(64) const uint32_t kK[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

const uint32_t kInit[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                           0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};

inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
inline uint32_t be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

// FIPS 180-4 section 6.2.2, nblocks whole blocks
void blocks_portable(uint32_t st[8], const uint8_t* p, size_t nblocks) {
  uint32_t w[64];
  for (; nblocks; --nblocks, p += 64) {
    for (int t = 0; t < 16; ++t) w[t] = be32(p + 4 * t);
    for (int t = 16; t < 64; ++t) {
      const uint32_t s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3);
      const uint32_t s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10);
      w[t] = w[t - 16] + s0 + w[t - 7] + s1;
    }
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    for (int t = 0; t < 64; ++t) {
      const uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25);
      const uint32_t ch = (e & f) ^ (~e & g);
      const uint32_t t1 = h + S1 + ch + kK[t] + w[t];
      const uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22);
      const uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
      const uint32_t t2 = S0 + mj;
      h = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
    }
    st[0] += a, st[1] += b, st[2] += c, st[3] += d, st[4] += e, st[5] += f, st[6] += g, st[7] += h;
  }
}

#ifdef BSG_X86
// The SHA extensions keep the state as (A,B,E,F) and (C,D,G,H); sha256rnds2 runs two rounds on
// the two low words of K+W, sha256msg1 / sha256msg2 the two halves of the schedule recurrence.
// Compiled for the extension by attribute only, so the library loads on a host without it.
__attribute__((target("sha,sse4.1,ssse3")))
void blocks_x86(uint32_t st[8], const uint8_t* p, size_t nblocks) {
  const __m128i kSwap = _mm_set_epi64x(0x0c0d0e0f08090a0bll, 0x0405060700010203ll);
  __m128i t = _mm_shuffle_epi32(_mm_loadu_si128(reinterpret_cast<const __m128i*>(st)), 0xB1);
  __m128i s1 = _mm_shuffle_epi32(_mm_loadu_si128(reinterpret_cast<const __m128i*>(st + 4)), 0x1B);
  __m128i s0 = _mm_alignr_epi8(t, s1, 8);  // ABEF
  s1 = _mm_blend_epi16(s1, t, 0xF0);       // CDGH
  for (; nblocks; --nblocks, p += 64) {
    const __m128i save0 = s0, save1 = s1;
    __m128i m[4];
#pragma GCC unroll 16
    for (int g = 0; g < 16; ++g) {
      if (g < 4)
        m[g] = _mm_shuffle_epi8(_mm_loadu_si128(reinterpret_cast<const __m128i*>(p + 16 * g)), kSwap);
      __m128i kw = _mm_add_epi32(m[g & 3], _mm_load_si128(reinterpret_cast<const __m128i*>(kK + 4 * g)));
      s1 = _mm_sha256rnds2_epu32(s1, s0, kw);
      if (g >= 3 && g < 15) {  // the next group's four schedule words
        const __m128i a = _mm_alignr_epi8(m[g & 3], m[(g + 3) & 3], 4);
        m[(g + 1) & 3] = _mm_sha256msg2_epu32(_mm_add_epi32(m[(g + 1) & 3], a), m[g & 3]);
      }
      kw = _mm_shuffle_epi32(kw, 0x0E);
      s0 = _mm_sha256rnds2_epu32(s0, s1, kw);
      if (g >= 1 && g < 13) m[(g + 3) & 3] = _mm_sha256msg1_epu32(m[(g + 3) & 3], m[g & 3]);
    }
    s0 = _mm_add_epi32(s0, save0);
    s1 = _mm_add_epi32(s1, save1);
  }
  t = _mm_shuffle_epi32(s0, 0x1B);       // FEBA
  s1 = _mm_shuffle_epi32(s1, 0xB1);      // DCHG
  s0 = _mm_blend_epi16(t, s1, 0xF0);     // DCBA
  s1 = _mm_alignr_epi8(s1, t, 8);        // HGFE
  _mm_storeu_si128(reinterpret_cast<__m128i*>(st), s0);
  _mm_storeu_si128(reinterpret_cast<__m128i*>(st + 4), s1);
}
#endif

void blocks(uint32_t st[8], const uint8_t* p, size_t nblocks, int impl) {
#ifdef BSG_X86
  if (impl == kShaX86) return blocks_x86(st, p, nblocks);
#endif
  (void)impl;
  blocks_portable(st, p, nblocks);
}

int64_t now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline void cpu_pause() {
#ifdef BSG_X86
  _mm_pause();
#endif
}

// Waits until pred() holds or stop is set: CPU pauses between polls for at most kSpinNs, then a
// short sleep between polls (a flag a GPU kernel raises has nothing to wake a sleeper with).
constexpr int64_t kSpinNs = 200'000;
template <class Pred>
bool poll_until(Pred pred, const std::atomic<bool>& stop) {
  const int64_t t0 = now_ns();
  bool spin = true;  // (the clock is read every 64th poll while spinning)
  for (uint32_t it = 0;; ++it) {
    if (pred()) return true;
    if (stop.load(std::memory_order_acquire)) return false;
    if (spin && (it & 63u) == 63u && now_ns() - t0 >= kSpinNs) spin = false;
    if (spin) {
      for (int i = 0; i < 16; ++i) cpu_pause();
    } else {  // from here on every poll is followed by a nap
      const timespec ts{0, 20'000};
      nanosleep(&ts, nullptr);
    }
  }
}

template <class T>
inline T load_acquire(const T* p) {
  return __atomic_load_n(p, __ATOMIC_ACQUIRE);
}

}  // namespace

bool sha256_have_x86() {
#ifdef BSG_X86
  static const bool have = [] {
    unsigned a = 0, b = 0, c = 0, d = 0;
    if (!__get_cpuid(1, &a, &b, &c, &d)) return false;
    if (!(c & (1u << 9)) || !(c & (1u << 19))) return false;  // SSSE3, SSE4.1
    if (!__get_cpuid_count(7, 0, &a, &b, &c, &d)) return false;
    return (b & (1u << 29)) != 0;  // SHA
  }();
  return have;
#else
  return false;
#endif
}

int sha256_best_impl() { return sha256_have_x86() ? kShaX86 : kShaPortable; }

const char* sha256_impl_name(int impl) { return impl == kShaX86 ? "x86-sha" : "portable"; }

void sha256_range(const uint8_t* p, size_t n, uint8_t out[32], int impl) {
  if (impl != kShaPortable) impl = sha256_best_impl();  // auto, or the extension where it exists
  uint32_t st[8];
  std::memcpy(st, kInit, sizeof st);
  const size_t whole = n / 64;
  if (whole) blocks(st, p, whole, impl);
  // the rest, 0x80, zeros and the bit length: one or two blocks
  uint8_t tail[128] = {0};
  const size_t rest = n - 64 * whole;
  if (rest) std::memcpy(tail, p + 64 * whole, rest);
  tail[rest] = 0x80;
  const size_t tb = rest + 9 <= 64 ? 1 : 2;
  const uint64_t bits = (uint64_t)n * 8;
  for (int i = 0; i < 8; ++i) tail[64 * tb - 1 - i] = (uint8_t)(bits >> (8 * i));
  blocks(st, tail, tb, impl);
  for (int i = 0; i < 8; ++i) {
    out[4 * i] = (uint8_t)(st[i] >> 24);
    out[4 * i + 1] = (uint8_t)(st[i] >> 16);
    out[4 * i + 2] = (uint8_t)(st[i] >> 8);
    out[4 * i + 3] = (uint8_t)st[i];
  }
}

double sha256_measure_rate(int impl, size_t bytes, double ms) {
  std::vector<uint8_t> buf(std::max<size_t>(bytes, 64));
  for (size_t i = 0; i < buf.size(); ++i) buf[i] = (uint8_t)(i * 2654435761u >> 24);
  uint8_t ref[32];
  sha256_range(buf.data(), buf.size(), ref, impl);  // touch the buffer and the code once
  const int64_t t0 = now_ns();
  uint64_t done = 0;
  int64_t t1 = t0;
  do {
    sha256_range(buf.data(), buf.size(), ref, impl);
    done += buf.size();
    t1 = now_ns();
  } while ((double)(t1 - t0) < ms * 1e6);
  return (double)done * 1e9 / (double)std::max<int64_t>(1, t1 - t0);
}

int HashWorkers::default_threads() {
  int n = 0;
  if (const char* e = std::getenv("OMP_NUM_THREADS")) n = std::atoi(e);
  if (n <= 0) n = (int)std::thread::hardware_concurrency();
  return std::max(1, std::min(16, n));
}

HashWorkers::HashWorkers(int threads) {
  const int n = threads > 0 ? std::min(16, threads) : default_threads();
  th_.reserve((size_t)n);
  for (int i = 0; i < n; ++i) th_.emplace_back([this] { loop(); });
}

HashWorkers::~HashWorkers() {
  if (open_) {
    cancel();
    (void)wait();
  }
  {
    std::lock_guard<std::mutex> g(mu_);
    quit_ = true;
  }
  cv_work_.notify_all();
  for (std::thread& t : th_) t.join();
}

void HashWorkers::start(const HashBatch& b) {
  std::lock_guard<std::mutex> g(mu_);
  cur_ = b;
  next_.store(0, std::memory_order_relaxed);
  bad_.store(0, std::memory_order_relaxed);
  nhashed_.store(0, std::memory_order_relaxed);
  last_ns_.store(0, std::memory_order_relaxed);
  cancel_.store(false, std::memory_order_relaxed);
  inside_ = (int)th_.size();
  open_ = true;
  ++gen_;
  cv_work_.notify_all();
}

void HashWorkers::cancel() { cancel_.store(true, std::memory_order_release); }

uint64_t HashWorkers::wait() {
  std::unique_lock<std::mutex> g(mu_);
  cv_done_.wait(g, [this] { return inside_ == 0; });
  open_ = false;
  return bad_.load(std::memory_order_relaxed);
}

void HashWorkers::loop() {
  uint64_t seen = 0;
  for (;;) {
    HashBatch b;
    {
      std::unique_lock<std::mutex> g(mu_);
      cv_work_.wait(g, [&] { return quit_ || gen_ != seen; });
      if (quit_) return;
      seen = gen_;
      b = cur_;
    }
    work(b);
    {
      std::lock_guard<std::mutex> g(mu_);
      if (--inside_ == 0) cv_done_.notify_all();
    }
  }
}

void HashWorkers::work(const HashBatch& b) {
  uint64_t n = kCountUnknown;
  if (!poll_until([&] { return (n = load_acquire(b.count)) != kCountUnknown; }, cancel_)) return;
  if (n > b.max_items) {
    bad_.fetch_add(1, std::memory_order_relaxed);
    n = b.max_items;
  }
  for (;;) {
    const uint64_t i = next_.fetch_add(1, std::memory_order_relaxed);
    if (i >= n) return;
    if (!poll_until([&] { return load_acquire(b.ready + i) != 0; }, cancel_)) return;
    const HashItem it = b.items[i];
    if (it.off > b.base_len || it.len > b.base_len - it.off) {
      bad_.fetch_add(1, std::memory_order_relaxed);
      continue;
    }
    sha256_range(b.base + it.off, (size_t)it.len, b.refs + 32 * i, b.impl);
    const int64_t t = now_ns();
    int64_t prev = last_ns_.load(std::memory_order_relaxed);
    while (prev < t && !last_ns_.compare_exchange_weak(prev, t, std::memory_order_relaxed)) {
    }
    nhashed_.fetch_add(1, std::memory_order_relaxed);
  }
}

}  // namespace bsg

// The two implementations for the tests (tests/test_host_sha256_cpu.py), by ctypes.
extern "C" int bsg_host_sha256_debug(const uint8_t* p, uint64_t n, int impl, uint8_t out[32]) {
  if ((!p && n) || !out) return -1;
  if (impl == bsg::kShaX86 && !bsg::sha256_have_x86()) return 1;  // not on this host
  static const uint8_t none = 0;
  bsg::sha256_range(p ? p : &none, (size_t)n, out, impl);
  return 0;
}
