// bsgpu_pool.inc — store/mem's Put for a pool that lives in device memory (bsg_pool,
// bsg_engine_pool_put): the last run's new chunks and new tree nodes appended to the pool's bytes,
// blob table and index. Included from bsgpu_kernels.hip after bsgpu_gc.inc, inside namespace bsg.
// From bsgpu_engine_common.inc it takes the items' accessors (dd_ref, dd_len), the prefix sum
// (launch_sum), pool_lookup, seg_find and gather_tile; from bsgpu_dedup.inc the first-occurrence
// pass (launch_dedup, the pool's index in the place of a set's table) and set_insert. DESIGN §4.12.
//
// The items are the run's records and then its tree nodes, one index space (DedupArgs::refs2), so
// launch_dedup's `first` and `rank` are the order of the append: the k-th new item becomes table
// entry nblobs + k. Nothing before launch_pool_append writes the pool; the host reads the header
// back in between and holds it to the pool's capacity. Every loop is bounded, every place read
// from device memory is checked against a host-known bound before it forms an address, and every
// atomic is a vector atomic on a device word.

__device__ __forceinline__ uint64_t align16(uint64_t x) { return (x + 15) & ~15ull; }

struct PvLen16 {
  __device__ uint64_t operator()(const DedupArgs& a, uint64_t i) const {
    return a.first[i] == i ? align16(dd_len(a, i)) : 0;
  }
};

// ---- plan: the new blobs' places by rank, and the totals --------------------------------------
__global__ __launch_bounds__(256) void k_pool_plan(PoolArgs a) {
  const DedupArgs& d = a.d;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t nu = d.rank[d.n];
  unsigned long long known = 0, repeats = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.n; i += stride) {
    const uint64_t f = d.first[i];
    known += (f & kDedupInSet) != 0;
    repeats += (f & ~kDedupInSet) != i;
    if (f != i) continue;
    const uint64_t k = d.rank[i];
    if (k >= nu || nu > d.n) {
      dd_error(d.hdr, 1 << 10);
      continue;
    }
    a.seg16[k] = a.off16[i];
    if (k + 1 == nu) a.hdr->last_len = dd_len(d, i);
  }
  if (known) atomicAdd(reinterpret_cast<unsigned long long*>(&a.hdr->known), known);
  if (repeats) atomicAdd(reinterpret_cast<unsigned long long*>(&a.hdr->repeats), repeats);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (nu <= d.n) a.seg16[nu] = a.off16[d.n];
    else dd_error(d.hdr, 1 << 10);
    a.hdr->total16 = a.off16[d.n];
  }
}

// ---- append: table entries and index slots ----------------------------------------------------
// The new refs are distinct from each other and from the pool's (launch_dedup's result), so an
// entry claims the first free slot of its probe sequence and no key is compared, as k_set_add.
__global__ __launch_bounds__(256) void k_pool_append(PoolArgs a) {
  const DedupArgs& d = a.d;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  SetArgs ix{};
  ix.tab = a.index;
  ix.mask = a.index_mask;
  ix.hdr = d.hdr;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.n; i += stride) {
    if (d.first[i] != i) continue;
    const uint64_t k = d.rank[i], len = dd_len(d, i), o = a.off16[i];
    if (k >= a.nnew || o > a.total16 || align16(len) > a.total16 - o) {
      dd_error(d.hdr, 1 << 11);
      continue;
    }
    const uint64_t* r = dd_ref(d, i);
    uint64_t* e = reinterpret_cast<uint64_t*>(a.table + a.nblobs + k);
    e[0] = a.base + o;
    e[1] = len;
    for (int w = 0; w < 4; ++w) e[2 + w] = r[w];
    set_insert(ix, r[0], a.nblobs + k);
  }
}

// ---- gather: the new blobs' bytes -------------------------------------------------------------
// item u's bytes: a record's in the run's input, a node's in the tree arena (null, and the error
// flag, if the item is not sane or its len is not `len`)
__device__ __forceinline__ const uint8_t* pool_src(const PoolArgs& a, uint64_t u, uint64_t len) {
  const uint8_t* src = nullptr;
  if (u < a.d.n1) {
    const ChunkRec& r = a.rec[u];
    const uint32_t s = r.stream;
    if (s < a.nstreams && r.len == len && r.offset <= a.streams[s].len &&
        len <= a.streams[s].len - r.offset)
      src = a.data + a.streams[s].data_off + r.offset;
  } else if (u < a.d.n) {
    const TreeNode& t = a.nodes[u - a.d.n1];
    if (t.blob_len == len && t.blob_off <= a.arena_bytes && len <= a.arena_bytes - t.blob_off)
      src = a.arena + t.blob_off;
  }
  if (!src) dd_error(a.d.hdr, 1 << 12);
  return src;
}

// Partitioned by output tiles of kPoolTile bytes, as k_pack and k_gc_compact. Segment k is new
// blob k: its bytes at base + seg16[k], then the zero bytes (at most 15) up to seg16[k + 1].
// src(u, len): where item u's len bytes lie (pool_src for a run's items; bsgpu_blobs.inc has the
// one for a caller's blobs).
template <class Src>
__device__ __forceinline__ void pool_gather_tiles(const PoolArgs& a, Src src) {
  const uint64_t t0 = (uint64_t)blockIdx.x * kPoolTile;
  if (t0 >= a.total16 || !a.nnew) return;
  const uint64_t t1 = min(t0 + (uint64_t)kPoolTile, a.total16);
  const auto off = [&a](uint64_t k) { return a.seg16[k]; };
  __shared__ uint64_t seg[2];
  if (threadIdx.x == 0) {
    seg[0] = seg_find(0, a.nnew, t0, off);
    seg[1] = seg_find(seg[0], a.nnew, t1 - 1, off);
  }
  __syncthreads();
  const uint64_t k1 = seg[1];
  uint64_t k = seg[0];
  gather_tile<false>(a.bytes + a.base, t0, t1, a.total16, [&](uint64_t pos, GatherSeg* g) {
    k = seg_find(k, k1 + 1, pos, off);
    const uint64_t o = a.seg16[k], nx = a.seg16[k + 1], u = a.d.uniq[k];
    g->src = nullptr;
    if (pos < o || pos >= nx || nx > a.total16 || u >= a.d.n) {
      dd_error(a.d.hdr, 1 << 12);
      return false;
    }
    const uint64_t len = dd_len(a.d, u);
    if (align16(len) != nx - o) {
      dd_error(a.d.hdr, 1 << 12);
      return false;
    }
    if (pos - o < len) {
      g->src = src(u, len);
      g->b0 = o;
      g->b1 = o + len;
    } else {
      g->src = a.hdr->zero;
      g->b0 = o + len;
      g->b1 = nx;
    }
    return g->src != nullptr;
  });
}

__global__ __launch_bounds__(256) void k_pool_gather(PoolArgs a) {
  pool_gather_tiles(a, [&a](uint64_t u, uint64_t len) { return pool_src(a, u, len); });
}

// ---- where: every item's blob -----------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pool_where(PoolArgs a) {
  const DedupArgs& d = a.d;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.n; i += stride) {
    const uint64_t f =
        pool_lookup(a.table, a.nblobs + a.nnew, a.index, a.index_mask, dd_ref(d, i), d.hdr);
    if (f == kDedupEmpty) dd_error(d.hdr, 1 << 13);  // every item's ref is in the pool by now
    a.where[i] = f;
  }
}

// ---- adopt: a marked pool's live blobs become an empty pool's entries (bsg_pool_collect) --------
// Live blob k of the source becomes entry rank[k] at offset noff16[k], the place k_gc_compact
// (coff = noff16) gives its bytes. The source holds no ref twice, so an entry claims the first free
// slot of its probe sequence and no key is compared, as k_pool_append. DESIGN §4.13.
__global__ __launch_bounds__(256) void k_pool_adopt(AdoptArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  SetArgs ix{};
  ix.tab = a.index;
  ix.mask = a.index_mask;
  ix.hdr = a.hdr;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.n; k += stride) {
    a.remap[k] = ~0ull;
    if (!a.live[k]) continue;
    const uint64_t j = a.rank[k], len = a.src[k].len, o = a.noff16[k];
    if (j >= a.nlive || o % 16 || o > a.total || len > a.total - o) {
      dd_error(a.hdr, 1 << 14);
      continue;
    }
    const uint64_t* r = reinterpret_cast<const uint64_t*>(a.src[k].ref);
    uint64_t* e = reinterpret_cast<uint64_t*>(a.table + j);
    e[0] = o;
    e[1] = len;
    for (int w = 0; w < 4; ++w) e[2 + w] = r[w];
    set_insert(ix, r[0], j);
    a.remap[k] = j;
  }
}

// ---- merge: a pool's selected blobs behind what another pool holds (bsg_pool_merge) -------------
// A pool's refs are pairwise distinct, so which blobs are new is one read-only probe of the
// destination's index per selected blob; nothing here needs a first-occurrence pass. The probe and
// the plan write the call's own buffers only. DESIGN §4.15.
__device__ __forceinline__ void mg_add(uint64_t* w, uint64_t v) {  // one atomic per wave
  for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_down((unsigned long long)v, o);
  if ((threadIdx.x & 63) == 0 && v)
    atomicAdd(reinterpret_cast<unsigned long long*>(w), (unsigned long long)v);
}

__global__ __launch_bounds__(256) void k_pool_probe(MergeArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  DedupHdr* eh = &a.hdr->g.w.dd;
  uint64_t selected = 0, known = 0, bytes = 0;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.n; k += stride) {
    uint64_t to = ~0ull;
    uint8_t fresh = 0;
    if (!a.sel || a.sel[k]) {
      ++selected;
      to = pool_lookup(a.dtable, a.dn, a.index, a.index_mask,
                       reinterpret_cast<const uint64_t*>(a.src[k].ref), eh);
      if (to == kDedupEmpty) {  // (its entry is the append's to name)
        fresh = 1;
        bytes += a.src[k].len;
      } else {
        ++known;
      }
    }
    a.remap[k] = to;
    a.isnew[k] = fresh;
  }
  mg_add(&a.hdr->selected, selected);
  mg_add(&a.hdr->known, known);
  mg_add(&a.hdr->added_bytes, bytes);
}

struct MvNew {
  __device__ uint64_t operator()(const MergeArgs& a, uint64_t k) const { return a.isnew[k] ? 1 : 0; }
};
struct MvLen16 {
  __device__ uint64_t operator()(const MergeArgs& a, uint64_t k) const {
    return a.isnew[k] ? align16(a.src[k].len) : 0;
  }
};

// the end of the last new blob's bytes (the offsets ascend, so the largest), as k_gc_offsets; a
// wave takes the largest of its lanes first and adds one atomic
__global__ __launch_bounds__(256) void k_pool_merge_end(MergeArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint64_t end = 0;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.n; k += stride)
    if (a.isnew[k]) end = max(end, a.off16[k] + a.src[k].len);
  for (int o = 32; o > 0; o >>= 1)
    end = max(end, (uint64_t)__shfl_down((unsigned long long)end, o));
  if ((threadIdx.x & 63) == 0 && end)
    atomicMax(reinterpret_cast<unsigned long long*>(&a.hdr->end), (unsigned long long)end);
}

// New blob k becomes entry dn + rank[k] at base + off16[k], the place launch_gc_compact (live =
// isnew, coff = off16, out = the destination's bytes + base) gives its bytes. Neither pool holds a
// ref twice and the destination lacks every new one, so an entry claims the first free slot of its
// probe sequence and no key is compared, as k_pool_append and k_pool_adopt.
__global__ __launch_bounds__(256) void k_pool_merge_append(MergeArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  DedupHdr* eh = &a.hdr->g.w.dd;
  SetArgs ix{};
  ix.tab = a.index;
  ix.mask = a.index_mask;
  ix.hdr = eh;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.n; k += stride) {
    if (!a.isnew[k]) continue;
    const uint64_t j = a.rank[k], len = a.src[k].len, o = a.off16[k];
    if (j >= a.nnew || a.dn + j >= a.cap_blobs || o % 16 || a.base > a.need_bytes ||
        o > a.need_bytes - a.base || len > a.need_bytes - a.base - o) {
      dd_error(eh, 1 << 15);
      continue;
    }
    const uint64_t* r = reinterpret_cast<const uint64_t*>(a.src[k].ref);
    uint64_t* e = reinterpret_cast<uint64_t*>(a.table + a.dn + j);
    e[0] = a.base + o;
    e[1] = len;
    for (int w = 0; w < 4; ++w) e[2 + w] = r[w];
    set_insert(ix, r[0], a.dn + j);
    a.remap[k] = a.dn + j;
  }
}

// ---- launchers --------------------------------------------------------------------------------
hipError_t launch_pool_probe(const MergeArgs& a, hipStream_t s, int num_cus) {
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(k_pool_probe, dim3(engine_grid(a.n, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pool_merge_plan(const MergeArgs& a, hipStream_t s, int num_cus) {
  if (!a.n) return hipSuccess;
  hipError_t e;
  if ((e = launch_sum<MvNew>(a, a.n, a.rank, s)) != hipSuccess) return e;
  if ((e = launch_sum<MvLen16>(a, a.n, a.off16, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_pool_merge_end, dim3(engine_grid(a.n, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pool_merge_append(const MergeArgs& a, hipStream_t s, int num_cus) {
  if (!a.nnew) return hipSuccess;
  hipLaunchKernelGGL(k_pool_merge_append, dim3(engine_grid(a.n, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pool_adopt(const AdoptArgs& a, hipStream_t s, int num_cus) {
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(k_pool_adopt, dim3(engine_grid(a.n, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// a.d.n >= 1, after launch_dedup(a.d) on the same stream
hipError_t launch_pool_plan(const PoolArgs& a, hipStream_t s, int num_cus) {
  hipError_t e;
  if ((e = launch_sum<PvLen16>(a.d, a.d.n, a.off16, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_pool_plan, dim3(engine_grid(a.d.n, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pool_append(const PoolArgs& a, hipStream_t s, int num_cus) {
  if (!a.nnew) return hipSuccess;
  hipLaunchKernelGGL(k_pool_append, dim3(engine_grid(a.d.n, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pool_gather(const PoolArgs& a, hipStream_t s) {
  if (!a.total16) return hipSuccess;
  const uint64_t tiles = (a.total16 + kPoolTile - 1) / kPoolTile;
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pool_gather, dim3((uint32_t)tiles), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pool_where(const PoolArgs& a, hipStream_t s, int num_cus) {
  if (!a.d.n) return hipSuccess;
  hipLaunchKernelGGL(k_pool_where, dim3(engine_grid(a.d.n, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}
