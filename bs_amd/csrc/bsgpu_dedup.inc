// bsgpu_dedup.inc — which chunks of a finished run are new (bsg_engine_dedup), a set of refs kept
// on the device across runs (bsg_refset) and the new chunks' bytes gathered into one contiguous
// buffer (bsg_engine_pack_unique). Included from bsgpu_kernels.hip after bsgpu_tree.inc (whose
// workgroup scan it uses), inside namespace bsg. DESIGN §4.8.
//
// First occurrence: an open-addressing table whose slots hold item indices. An item claims the
// first free slot of its probe sequence (atomicCAS) or, meeting a slot whose item has the same 32
// bytes, lowers that slot to its own index (atomicMin). A slot's key never changes once claimed
// and equal keys walk the same sequence, so a key owns exactly one slot and that slot ends at the
// key's smallest index, whatever the order of the threads. Every probe loop is bounded by the
// table size and flags DedupHdr::error if it runs out.

__device__ __forceinline__ void dd_error(DedupHdr* h, uint64_t code) {
  atomicOr(reinterpret_cast<unsigned long long*>(&h->error), (unsigned long long)code);
}

__device__ __forceinline__ const uint64_t* dd_ref(const DedupArgs& a, uint64_t i) {
  return reinterpret_cast<const uint64_t*>(a.refs + i * a.stride);
}

__device__ __forceinline__ bool dd_eq(const uint64_t* x, const uint64_t* y) {
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
      } else if (cur == i || dd_eq(r, dd_ref(a, cur))) {
        atomicMin(slot, (unsigned long long)i);
        done = true;
      }
    }
    if (!done) dd_error(a.hdr, 1);
  }
}

// first[i]: the smallest index with item i's ref, and whether the set already held the ref
__global__ __launch_bounds__(256) void k_dd_first(DedupArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    const uint64_t* r = dd_ref(a, i);
    const uint64_t h = r[0];
    uint64_t f = kDedupEmpty;
    for (uint64_t p = 0; p <= a.tab_mask; ++p) {
      const uint64_t cur = a.tab[(h + p) & a.tab_mask];
      if (cur >= a.n) break;  // a free slot: the ref was never inserted
      if (cur == i || dd_eq(r, dd_ref(a, cur))) {
        f = cur;
        break;
      }
    }
    if (f > i) {  // every item finds its own key at an index no larger than its own
      dd_error(a.hdr, 4);
      f = i;
    }
    if (a.set_tab) {
      bool ended = false;
      for (uint64_t p = 0; p <= a.set_mask && !ended; ++p) {
        const uint64_t c = a.set_tab[(h + p) & a.set_mask];
        if (c == kDedupEmpty) {
          ended = true;
        } else if (c >= a.set_count) {
          dd_error(a.hdr, 8);
          ended = true;
        } else if (dd_eq(r, reinterpret_cast<const uint64_t*>(a.set_keys + 32 * c))) {
          f |= kDedupInSet;
          ended = true;
        }
      }
      if (!ended) dd_error(a.hdr, 16);  // a set's table is never full
    }
    a.first[i] = f;
  }
}

// ---- prefix sums over the items (the tree's three-kernel form) ------------------------------
struct DvNew {
  __device__ uint64_t operator()(const DedupArgs& a, uint64_t i) const { return a.first[i] == i; }
};
struct DvNewBytes {
  __device__ uint64_t operator()(const DedupArgs& a, uint64_t i) const {
    if (a.first[i] != i || !a.lens) return 0;
    return *reinterpret_cast<const uint64_t*>(a.lens + i * a.len_stride);
  }
};

template <class V>
__global__ __launch_bounds__(256) void k_dd_scan_part(DedupArgs a) {
  const uint64_t i0 = (uint64_t)blockIdx.x * kTreeTile + threadIdx.x * 8ull;
  uint64_t v = 0;
  for (uint32_t k = 0; k < 8; ++k)
    if (i0 + k < a.n) v += V()(a, i0 + k);
  uint64_t tot;
  (void)tree_block_scan(v, &tot);
  if (threadIdx.x == 0) a.part[blockIdx.x] = tot;
}

template <class V>
__global__ __launch_bounds__(256) void k_dd_scan_final(DedupArgs a, uint64_t nb, uint64_t* out) {
  const uint64_t i0 = (uint64_t)blockIdx.x * kTreeTile + threadIdx.x * 8ull;
  uint64_t x[8], v = 0;
  for (uint32_t k = 0; k < 8; ++k) {
    x[k] = i0 + k < a.n ? V()(a, i0 + k) : 0;
    v += x[k];
  }
  uint64_t tot;
  uint64_t run = a.part[blockIdx.x] + tree_block_scan(v, &tot);
  for (uint32_t k = 0; k < 8; ++k) {
    if (i0 + k < a.n) out[i0 + k] = run;
    run += x[k];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[a.n] = a.part[nb];
}

// the new items, ascending, and where each one's bytes start in the packed output
__global__ __launch_bounds__(256) void k_dd_compact(DedupArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t nu = a.rank[a.n];
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    if (a.first[i] != i) continue;
    const uint64_t k = a.rank[i];
    if (k >= nu || nu > a.n) {
      dd_error(a.hdr, 32);
      continue;
    }
    a.uniq[k] = i;
    a.pack_off[k] = a.bpre[i];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (nu <= a.n) a.pack_off[nu] = a.bpre[a.n];
    else dd_error(a.hdr, 32);
    a.hdr->nunique = nu;
    a.hdr->unique_bytes = a.bpre[a.n];
  }
}

// ---- a set's table ----------------------------------------------------------------------------
// key index `idx` (its first 8 bytes h) into the first free slot of its sequence
__device__ __forceinline__ void set_insert(const SetArgs& a, uint64_t h, uint64_t idx) {
  for (uint64_t p = 0; p <= a.mask; ++p) {
    unsigned long long* slot = reinterpret_cast<unsigned long long*>(a.tab + ((h + p) & a.mask));
    if (atomicCAS(slot, (unsigned long long)kDedupEmpty, (unsigned long long)idx) == kDedupEmpty)
      return;
  }
  dd_error(a.hdr, 64);
}

__global__ __launch_bounds__(256) void k_set_rehash(SetArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += stride)
    set_insert(a, *reinterpret_cast<const uint64_t*>(a.keys + 32 * i), i);
}

__global__ __launch_bounds__(256) void k_set_add(SetArgs a, DedupArgs d, uint64_t m) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += stride) {
    const uint64_t i = d.uniq[k];
    if (i >= d.n) {
      dd_error(a.hdr, 128);
      continue;
    }
    const uint64_t* r = dd_ref(d, i);
    uint64_t* key = reinterpret_cast<uint64_t*>(a.keys + 32 * (a.count + k));
    for (int w = 0; w < 4; ++w) key[w] = r[w];
    set_insert(a, r[0], a.count + k);
  }
}

// ---- pack: the new records' bytes, contiguous -------------------------------------------------
// Partitioned by output tiles of kPackTile bytes, so one long chunk spreads over the chip and
// thousands of short ones share a workgroup. A thread owns 16-byte output vectors (out is 16-byte
// aligned, so every store but the output's last is a whole aligned vector). A vector inside one
// segment is one 16-byte load at whatever residue the source has; a vector across segment ends
// is gathered byte by byte.
typedef uint32_t pk_u32x4u __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t pk_u32x4a __attribute__((ext_vector_type(4), aligned(16)));

// the largest k in [lo, hi) with p[k] <= key (p[lo] <= key)
__device__ __forceinline__ uint64_t pack_seg(const uint64_t* p, uint64_t lo, uint64_t hi,
                                             uint64_t key) {
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (p[mid] <= key) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the first byte of segment k's record (null, and the error flag, if the record is not sane)
__device__ __forceinline__ const uint8_t* pack_src(const PackArgs& a, uint64_t k) {
  const uint64_t u = a.uniq[k];
  if (u >= a.nrec) {
    dd_error(a.hdr, 256);
    return nullptr;
  }
  const uint64_t off = a.rec[u].offset, len = a.rec[u].len;
  const uint32_t s = a.rec[u].stream;
  if (s >= a.nstreams || len != a.pack_off[k + 1] - a.pack_off[k] ||
      off + len > a.streams[s].len) {
    dd_error(a.hdr, 256);
    return nullptr;
  }
  return a.data + a.streams[s].data_off + off;
}

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

template <bool FUNNEL>
__global__ __launch_bounds__(256) void k_pack(PackArgs a) {
  const uint64_t t0 = (uint64_t)blockIdx.x * kPackTile;
  if (t0 >= a.total) return;
  const uint64_t t1 = min(t0 + (uint64_t)kPackTile, a.total);
  __shared__ uint64_t seg[2];
  if (threadIdx.x == 0) {
    seg[0] = pack_seg(a.pack_off, 0, a.nunique, t0);
    seg[1] = pack_seg(a.pack_off, seg[0], a.nunique, t1 - 1);
  }
  __syncthreads();
  const uint64_t k0 = seg[0], k1 = seg[1];
  // the segment of the thread's previous vector: a chunk is mostly longer than the 4 KiB between
  // two vectors of a thread, so the search and the record's dependent loads are paid once
  uint64_t k = k0, b0 = 0, b1 = 0;
  const uint8_t* src = nullptr;
  for (uint64_t o = t0 + 16ull * threadIdx.x; o < t1; o += 16ull * 256) {
    if (o >= b1 || !src) {
      k = pack_seg(a.pack_off, k, k1 + 1, o);
      src = pack_src(a, k);
      if (!src) continue;
      b0 = a.pack_off[k];
      b1 = a.pack_off[k + 1];
    }
    if (o + 16 <= b1) {  // (b1 <= total)
      *reinterpret_cast<pk_u32x4a*>(a.out + o) = pack_load16<FUNNEL>(src + (o - b0));
      continue;
    }
    uint32_t w[4] = {0, 0, 0, 0};
    uint32_t nb = 0;
    bool live = true;  // (no break: the loop unrolls and w[] stays in registers)
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b) {
      const uint64_t ob = o + b;
      live = live && ob < a.total;
      if (live && ob >= b1) {  // the next segment that has a byte
        k = pack_seg(a.pack_off, k, k1 + 1, ob);
        src = pack_src(a, k);
        live = src != nullptr;
        if (live) {
          b0 = a.pack_off[k];
          b1 = a.pack_off[k + 1];
        }
      }
      if (live) {
        w[b >> 2] |= (uint32_t)src[ob - b0] << (8 * (b & 3));
        nb = b + 1;
      }
    }
    if (!src) continue;
    if (nb == 16) {
      *reinterpret_cast<pk_u32x4a*>(a.out + o) = pk_u32x4a{w[0], w[1], w[2], w[3]};
    } else {  // the output's last vector: only its own bytes
#pragma unroll
      for (uint32_t b = 0; b < 16; ++b)
        if (b < nb) a.out[o + b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
    }
  }
}

// ---- launchers ------------------------------------------------------------------------------
template <class V>
static hipError_t dd_scan(const DedupArgs& a, uint64_t* out, hipStream_t s) {
  const uint64_t nb = tree_scan_parts(a.n) - 1;
  hipLaunchKernelGGL(k_dd_scan_part<V>, dim3((uint32_t)nb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_tree_scan_mid, dim3(1), dim3(256), 0, s, a.part, nb);
  hipLaunchKernelGGL(k_dd_scan_final<V>, dim3((uint32_t)nb), dim3(256), 0, s, a, nb, out);
  return hipGetLastError();
}

// a.n >= 1; a.tab is kDedupEmpty-filled and a.hdr zeroed by the caller
hipError_t launch_dedup(const DedupArgs& a, hipStream_t s, int num_cus) {
  const uint32_t g = tree_grid(a.n, num_cus);
  hipLaunchKernelGGL(k_dd_insert, dim3(g), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_dd_first, dim3(g), dim3(256), 0, s, a);
  hipError_t e;
  if ((e = dd_scan<DvNew>(a, a.rank, s)) != hipSuccess) return e;
  if ((e = dd_scan<DvNewBytes>(a, a.bpre, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_dd_compact, dim3(g), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_set_rehash(const SetArgs& a, hipStream_t s, int num_cus) {
  if (!a.count) return hipSuccess;
  hipLaunchKernelGGL(k_set_rehash, dim3(tree_grid(a.count, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_set_add(const SetArgs& a, const DedupArgs& d, uint64_t m, hipStream_t s,
                          int num_cus) {
  if (!m) return hipSuccess;
  hipLaunchKernelGGL(k_set_add, dim3(tree_grid(m, num_cus)), dim3(256), 0, s, a, d, m);
  return hipGetLastError();
}

hipError_t launch_pack(const PackArgs& a, bool funnel, hipStream_t s) {
  if (!a.total) return hipSuccess;
  const uint64_t tiles = (a.total + kPackTile - 1) / kPackTile;
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  if (funnel) hipLaunchKernelGGL(k_pack<true>, dim3((uint32_t)tiles), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_pack<false>, dim3((uint32_t)tiles), dim3(256), 0, s, a);
  return hipGetLastError();
}
