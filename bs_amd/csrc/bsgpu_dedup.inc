// bsgpu_dedup.inc — which chunks of a finished run are new (bsg_engine_dedup), a set of refs kept
// on the device across runs (bsg_refset) and the new chunks' bytes gathered into one contiguous
// buffer (bsg_engine_pack_unique). Included from bsgpu_kernels.hip, inside namespace bsg. From
// bsgpu_engine_common.inc it takes the table of indices by ref (k_dd_insert, ref_lookup, ref_eq,
// dd_error), the prefix sum (launch_sum), seg_find and, for k_pack, gather_tile. DESIGN §4.8.

// first[i]: the smallest index with item i's ref, and whether the set already held the ref
__global__ __launch_bounds__(256) void k_dd_first(DedupArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    const uint64_t* r = dd_ref(a, i);
    const uint64_t h = r[0];
    uint64_t f = kDedupEmpty;
    // Not ref_lookup: in the run's own table any index >= n ends the probe quietly, an exhausted
    // table shows as f > i below and cur == i spares comparing an item with itself, so a
    // damaged table would raise other error bits through ref_lookup than it does here.
    for (uint64_t p = 0; p <= a.tab_mask; ++p) {
      const uint64_t cur = a.tab[(h + p) & a.tab_mask];
      if (cur >= a.n) break;  // a free slot: the ref was never inserted
      if (cur == i || ref_eq(r, dd_ref(a, cur))) {
        f = cur;
        break;
      }
    }
    if (f > i) {  // every item finds its own key at an index no larger than its own
      dd_error(a.hdr, 4);
      f = i;
    }
    if (a.set_tab) {  // (a set's table is never full)
      const uint8_t* keys = a.set_keys;
      const uint64_t ks = a.set_stride;
      const uint64_t c = ref_lookup(
          a.set_tab, a.set_mask, a.set_count, r,
          [keys, ks](uint64_t k) { return reinterpret_cast<const uint64_t*>(keys + ks * k); },
          a.hdr, 8, 16);
      if (c != kDedupEmpty) f |= kDedupInSet;
    }
    a.first[i] = f;
  }
}

// ---- the values the prefix passes sum ---------------------------------------------------------
struct DvNew {
  __device__ uint64_t operator()(const DedupArgs& a, uint64_t i) const { return a.first[i] == i; }
};
struct DvNewBytes {
  __device__ uint64_t operator()(const DedupArgs& a, uint64_t i) const {
    return a.first[i] == i ? dd_len(a, i) : 0;
  }
};

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
// thousands of short ones share a workgroup. Segment k is record uniq[k], its bytes of the output
// [pack_off[k], pack_off[k + 1]); gather_tile does the rest.

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
__global__ __launch_bounds__(256) void k_pack(PackArgs a) {
  const uint64_t t0 = (uint64_t)blockIdx.x * kPackTile;
  if (t0 >= a.total) return;
  const uint64_t t1 = min(t0 + (uint64_t)kPackTile, a.total);
  const auto off = [&a](uint64_t k) { return a.pack_off[k]; };
  __shared__ uint64_t seg[2];
  if (threadIdx.x == 0) {
    seg[0] = seg_find(0, a.nunique, t0, off);
    seg[1] = seg_find(seg[0], a.nunique, t1 - 1, off);
  }
  __syncthreads();
  const uint64_t k1 = seg[1];
  uint64_t k = seg[0];
  gather_tile<FUNNEL>(a.out, t0, t1, a.total, [&](uint64_t pos, GatherSeg* g) {
    k = seg_find(k, k1 + 1, pos, off);
    g->src = pack_src(a, k);
    if (!g->src) return false;
    g->b0 = a.pack_off[k];
    g->b1 = a.pack_off[k + 1];
    return true;
  });
}

// ---- launchers ------------------------------------------------------------------------------
// a.n >= 1; a.tab is kDedupEmpty-filled and a.hdr zeroed by the caller
hipError_t launch_dedup(const DedupArgs& a, hipStream_t s, int num_cus) {
  const uint32_t g = engine_grid(a.n, num_cus);
  hipLaunchKernelGGL(k_dd_insert, dim3(g), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_dd_first, dim3(g), dim3(256), 0, s, a);
  hipError_t e;
  if ((e = launch_sum<DvNew>(a, a.n, a.rank, s)) != hipSuccess) return e;
  if ((e = launch_sum<DvNewBytes>(a, a.n, a.bpre, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_dd_compact, dim3(g), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_set_rehash(const SetArgs& a, hipStream_t s, int num_cus) {
  if (!a.count) return hipSuccess;
  hipLaunchKernelGGL(k_set_rehash, dim3(engine_grid(a.count, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_set_add(const SetArgs& a, const DedupArgs& d, uint64_t m, hipStream_t s,
                          int num_cus) {
  if (!m) return hipSuccess;
  hipLaunchKernelGGL(k_set_add, dim3(engine_grid(m, num_cus)), dim3(256), 0, s, a, d, m);
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
