// bsgpu_engine_common.inc — what the engine's passes over a finished run share on the device:
// the multi-workgroup prefix sum, the table of indices by 32-byte ref (its insert kernel, its
// read-only lookup, the index of a pool's blobs), the search for the segment that holds a
// position and the per-thread gather of 16-byte output vectors from segments. Included from
// bsgpu_kernels.hip before bsgpu_tree.inc, bsgpu_dedup.inc, bsgpu_restore.inc, bsgpu_walk.inc,
// bsgpu_gc.inc, bsgpu_pool.inc, bsgpu_read.inc and bsgpu_blobs.inc, inside namespace bsg.
// DESIGN §4.6b.

// workgroups of a grid-stride pass over `items`, 256 threads each
static inline uint32_t engine_grid(uint64_t items, int num_cus) {
  return grid_for(items, 256, 8u * (uint32_t)num_cus);
}

// ---- exclusive prefix sums over n host-known items: out[0 .. n], out[n] = the total ----------
// Three launches: every workgroup's sum (k_sum_part), the prefix of those (k_sum_mid, one
// workgroup), every item's prefix (k_sum_final). V()(a, i) is item i's value, a.part the
// workgroup sums (sum_parts(n) of them).
constexpr uint32_t kSumTile = 2048;  // items per workgroup of the prefix passes (256 x 8)

// blockDim.x == 256. Returns this thread's exclusive prefix of v within the workgroup.
__device__ __forceinline__ uint64_t wg_exclusive_sum(uint64_t v, uint64_t* total) {
  __shared__ uint64_t wsum[4];
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t x = v;
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t y = (uint64_t)__shfl_up((unsigned long long)x, o);
    if (lane >= (uint32_t)o) x += y;
  }
  __syncthreads();  // wsum of a previous call has been read
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  uint64_t base = 0, tot = 0;
  for (uint32_t k = 0; k < 4; ++k) {
    if (k < w) base += wsum[k];
    tot += wsum[k];
  }
  *total = tot;
  return base + x - v;
}

template <class Args, class V>
__global__ __launch_bounds__(256) void k_sum_part(Args a, uint64_t n) {
  const uint64_t i0 = (uint64_t)blockIdx.x * kSumTile + threadIdx.x * 8ull;
  uint64_t v = 0;
  for (uint32_t k = 0; k < 8; ++k)
    if (i0 + k < n) v += V()(a, i0 + k);
  uint64_t tot;
  (void)wg_exclusive_sum(v, &tot);
  if (threadIdx.x == 0) a.part[blockIdx.x] = tot;
}

// one workgroup: part[0 .. nb) -> its exclusive prefix, part[nb] = the total
__global__ __launch_bounds__(256) void k_sum_mid(uint64_t* part, uint64_t nb) {
  const uint64_t per = (nb + 255) / 256;
  const uint64_t b0 = threadIdx.x * per;
  uint64_t v = 0;
  for (uint64_t k = b0; k < b0 + per && k < nb; ++k) v += part[k];
  uint64_t tot;
  uint64_t run = wg_exclusive_sum(v, &tot);
  for (uint64_t k = b0; k < b0 + per && k < nb; ++k) {
    const uint64_t x = part[k];
    part[k] = run;
    run += x;
  }
  if (threadIdx.x == 0) part[nb] = tot;
}

template <class Args, class V>
__global__ __launch_bounds__(256) void k_sum_final(Args a, uint64_t n, uint64_t nb,
                                                   uint64_t* out) {
  const uint64_t i0 = (uint64_t)blockIdx.x * kSumTile + threadIdx.x * 8ull;
  uint64_t x[8], v = 0;
  for (uint32_t k = 0; k < 8; ++k) {
    x[k] = i0 + k < n ? V()(a, i0 + k) : 0;
    v += x[k];
  }
  uint64_t tot;
  uint64_t run = a.part[blockIdx.x] + wg_exclusive_sum(v, &tot);
  for (uint32_t k = 0; k < 8; ++k) {
    if (i0 + k < n) out[i0 + k] = run;
    run += x[k];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = a.part[nb];
}

uint64_t sum_parts(uint64_t n) {
  const uint64_t nb = (n + kSumTile - 1) / kSumTile;
  return (nb ? nb : 1) + 1;  // one per workgroup, then the total
}

template <class V, class Args>
static hipError_t launch_sum(const Args& a, uint64_t n, uint64_t* out, hipStream_t s) {
  const uint64_t nb = sum_parts(n) - 1;
  hipLaunchKernelGGL((k_sum_part<Args, V>), dim3((uint32_t)nb), dim3(256), 0, s, a, n);
  hipLaunchKernelGGL(k_sum_mid, dim3(1), dim3(256), 0, s, a.part, nb);
  hipLaunchKernelGGL((k_sum_final<Args, V>), dim3((uint32_t)nb), dim3(256), 0, s, a, n, nb, out);
  return hipGetLastError();
}

// ---- a table of indices by ref --------------------------------------------------------------
// An open-addressing table whose slots hold item indices (kDedupEmpty: free), probed linearly
// from the ref's first 8 bytes. k_dd_insert: an item claims the first free slot of its probe
// sequence (atomicCAS) or, meeting a slot whose item has the same 32 bytes, lowers that slot to
// its own index (atomicMin). A slot's key never changes once claimed and equal keys walk the same
// sequence, so a key owns exactly one slot and that slot ends at the key's smallest index,
// whatever the order of the threads. Every probe loop is bounded by the table size and flags
// DedupHdr::error if it runs out.
__device__ __forceinline__ void dd_error(DedupHdr* h, uint64_t code) {
  atomicOr(reinterpret_cast<unsigned long long*>(&h->error), (unsigned long long)code);
}

// item i's ref and length: items [0, n1) lie in refs / lens, the others in a second array with
// the same strides (refs2; null: every item lies in the first)
__device__ __forceinline__ const uint64_t* dd_ref(const DedupArgs& a, uint64_t i) {
  if (a.refs2 && i >= a.n1)
    return reinterpret_cast<const uint64_t*>(a.refs2 + (i - a.n1) * a.stride);
  return reinterpret_cast<const uint64_t*>(a.refs + i * a.stride);
}

__device__ __forceinline__ uint64_t dd_len(const DedupArgs& a, uint64_t i) {
  if (a.refs2 && i >= a.n1)  // (a 4-byte length)
    return *reinterpret_cast<const uint32_t*>(a.lens2 + (i - a.n1) * a.len_stride);
  return a.lens ? *reinterpret_cast<const uint64_t*>(a.lens + i * a.len_stride) : 0;
}

__device__ __forceinline__ bool ref_eq(const uint64_t* x, const uint64_t* y) {
  return x[0] == y[0] && x[1] == y[1] && x[2] == y[2] && x[3] == y[3];
}

__global__ __launch_bounds__(256) void k_dd_insert(DedupArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    const uint64_t* r = dd_ref(a, i);
    const uint64_t h = r[0];
    bool done = false;
    for (uint64_t p = 0; p <= a.tab_mask && !done; ++p) {
      unsigned long long* slot = reinterpret_cast<unsigned long long*>(a.tab + ((h + p) & a.tab_mask));
      const uint64_t cur = atomicCAS(slot, (unsigned long long)kDedupEmpty, (unsigned long long)i);
      if (cur == kDedupEmpty) {
        done = true;
      } else if (cur >= a.n) {
        dd_error(a.hdr, 2);
        done = true;
      } else if (cur == i || ref_eq(r, dd_ref(a, cur))) {
        atomicMin(slot, (unsigned long long)i);
        done = true;
      }
    }
    if (!done) dd_error(a.hdr, 1);
  }
}

// The read-only probe of a finished table: the index whose key is the 32 bytes at r, or
// kDedupEmpty. key(k) is index k's key, for k < n. A slot that holds an index >= n raises
// e_range in hdr->error, a probe that never meets a free slot e_full (no table is ever full);
// either ends as a miss.
template <class Key>
__device__ __forceinline__ uint64_t ref_lookup(const uint64_t* tab, uint64_t mask, uint64_t n,
                                               const uint64_t* r, Key key, DedupHdr* hdr,
                                               uint64_t e_range, uint64_t e_full) {
  const uint64_t h = r[0];
  uint64_t f = kDedupEmpty;
  bool ended = false;
  for (uint64_t p = 0; p <= mask && !ended; ++p) {
    const uint64_t cur = tab[(h + p) & mask];
    if (cur == kDedupEmpty) {
      ended = true;
    } else if (cur >= n) {
      dd_error(hdr, e_range);
      ended = true;
    } else if (ref_eq(r, key(cur))) {
      f = cur;
      ended = true;
    }
  }
  if (!ended) dd_error(hdr, e_full);
  return f;
}

// the smallest blob index named r in a pool's index (launch_ref_index), or kDedupEmpty
__device__ __forceinline__ uint64_t pool_lookup(const PoolBlob* blobs, uint64_t nblobs,
                                                const uint64_t* tab, uint64_t mask,
                                                const uint64_t* r, DedupHdr* hdr) {
  if (!nblobs) return kDedupEmpty;
  return ref_lookup(
      tab, mask, nblobs, r,
      [blobs](uint64_t k) { return reinterpret_cast<const uint64_t*>(blobs[k].ref); }, hdr, 2, 1);
}

// The index of a pool's blobs by ref: k_dd_insert over PoolBlob::ref, so a ref's slot ends at its
// smallest index. tab is kDedupEmpty-filled and at most half full, hdr's error word zeroed.
hipError_t launch_ref_index(const PoolBlob* blobs, uint64_t nblobs, uint64_t* tab, uint64_t mask,
                            DedupHdr* hdr, hipStream_t s, int num_cus) {
  if (!nblobs) return hipSuccess;
  DedupArgs d{};
  d.refs = reinterpret_cast<const uint8_t*>(blobs) + offsetof(PoolBlob, ref);
  d.stride = sizeof(PoolBlob);
  d.n = nblobs;
  d.tab = tab;
  d.tab_mask = mask;
  d.hdr = hdr;
  hipLaunchKernelGGL(k_dd_insert, dim3(engine_grid(nblobs, num_cus)), dim3(256), 0, s, d);
  return hipGetLastError();
}

// ---- segments -------------------------------------------------------------------------------
// the largest k in [lo, hi) with key(k) <= t (key never descends, key(lo) <= t)
template <class Key>
__device__ __forceinline__ uint64_t seg_find(uint64_t lo, uint64_t hi, uint64_t t, Key key) {
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (key(mid) <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

typedef uint32_t pk_u32x4u __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t pk_u32x4a __attribute__((ext_vector_type(4), aligned(16)));

template <bool FUNNEL>
__device__ __forceinline__ pk_u32x4a pack_load16(const uint8_t* s) {
  if (!FUNNEL) {
    const pk_u32x4u v = *reinterpret_cast<const pk_u32x4u*>(s);
    return pk_u32x4a{v.x, v.y, v.z, v.w};
  }
  // two aligned vectors and a shift by the source's residue (the second one lies inside the
  // segment or the read slack)
  const uintptr_t al = reinterpret_cast<uintptr_t>(s) & ~(uintptr_t)15;
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 15);
  const pk_u32x4a lo = *reinterpret_cast<const pk_u32x4a*>(al);
  const pk_u32x4a hi = *reinterpret_cast<const pk_u32x4a*>(al + 16);
  uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  uint32_t x[7], y[5];
  for (int j = 0; j < 7; ++j) x[j] = (sh & 8) ? (j + 2 < 8 ? w[j + 2] : 0u) : w[j];
  for (int j = 0; j < 5; ++j) y[j] = (sh & 4) ? x[j + 1] : x[j];
  pk_u32x4a r;
  r.x = __builtin_amdgcn_alignbyte(y[1], y[0], sh & 3);
  r.y = __builtin_amdgcn_alignbyte(y[2], y[1], sh & 3);
  r.z = __builtin_amdgcn_alignbyte(y[3], y[2], sh & 3);
  r.w = __builtin_amdgcn_alignbyte(y[4], y[3], sh & 3);
  return r;
}

// source bytes that land at output positions [b0, b1): position p is src[p - b0]
struct GatherSeg {
  const uint8_t* src;  // (null: none)
  uint64_t b0, b1;
};

// One thread's share of the output tile [t0, t1) of out[0 .. end), for a workgroup of 256: the
// thread owns 16-byte output vectors (out is 16-byte aligned, so every store but the last
// partial vector's is a whole aligned vector). locate(pos, &g) fills g with the segment that
// holds pos, or raises its caller's error flag, nulls g.src and returns false. The thread keeps
// its previous vector's segment: a segment is mostly longer than the 4 KiB between two vectors
// of a thread, so the search and the segment's dependent loads are paid once. A vector inside
// one segment is one 16-byte load at whatever residue the source has; a vector across segment
// ends is gathered byte by byte; the last partial vector before `end` is stored byte by byte.
template <bool FUNNEL, class Locate>
__device__ __forceinline__ void gather_tile(uint8_t* out, uint64_t t0, uint64_t t1, uint64_t end,
                                            Locate locate) {
  GatherSeg g = {nullptr, 0, 0};
  for (uint64_t o = t0 + 16ull * threadIdx.x; o < t1; o += 16ull * 256) {
    if ((!g.src || o >= g.b1) && !locate(o, &g)) continue;
    if (o + 16 <= g.b1) {  // (b1 <= end)
      *reinterpret_cast<pk_u32x4a*>(out + o) = pack_load16<FUNNEL>(g.src + (o - g.b0));
      continue;
    }
    uint32_t w[4] = {0, 0, 0, 0};
    uint32_t nb = 0;
    bool live = true;  // (no break: the loop unrolls and w[] stays in registers)
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b) {
      const uint64_t ob = o + b;
      live = live && ob < end;
      if (live && ob >= g.b1) live = locate(ob, &g);  // the next segment that has a byte
      if (live) {
        w[b >> 2] |= (uint32_t)g.src[ob - g.b0] << (8 * (b & 3));
        nb = b + 1;
      }
    }
    if (!g.src) continue;
    if (nb == 16) {
      *reinterpret_cast<pk_u32x4a*>(out + o) = pk_u32x4a{w[0], w[1], w[2], w[3]};
    } else {  // the last vector: only its own bytes
#pragma unroll
      for (uint32_t b = 0; b < 16; ++b)
        if (b < nb) out[o + b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
    }
  }
}
