// bsgpu_gc.inc — gc.Protect + split.Protect + gc.Run's sweep for a pool in device memory
// (bsg_engine_gc_mark, bsg_engine_gc_compact): which blobs of a pool are reachable from a set of
// Roots, and the reachable ones gathered into a new pool. Included from bsgpu_kernels.hip after
// bsgpu_walk.inc, inside namespace bsg. From bsgpu_engine_common.inc it takes the pool's index
// (launch_ref_index on the host's side, pool_lookup here), the prefix sum (launch_sum), seg_find
// and gather_tile; from bsgpu_walk.inc the count pass (k_wk_count with kWalkNoCover entries: one
// wave per frontier node, the run table) and wk_entry. DESIGN §4.11.
//
// The mark is the walk's breadth-first search with two differences. A blob is expanded once: a
// thread that names a blob under a Root or a `nodes` entry claims it with an atomic test-and-set
// on state[blob]; the one winner puts it into the next frontier, every loser a dead entry, at the
// place the walk would use (cnode[i] + k), so no counter is needed and a level's frontier is at
// most the `nodes` entries of the level above. Level L therefore holds the blobs whose nearest
// Root is L edges away, whichever thread won. And nothing is held to a cover: a node must meet
// its own rules, a child only has to be in the pool. live[k] is written 1 by whoever names blob
// k; which thread does is immaterial.
//
// The sweep: three prefix sums over the blobs in index order (live, live lens, live lens rounded
// up to 16) give every live blob its place; k_gc_compact gathers by output tiles, finding an
// output byte's blob in that prefix (dead and empty blobs add nothing, so the largest index whose
// offset is not past the byte is the live blob that holds it, or whose padding does).
//
// Every loop is bounded (by the blob length, the table size, kWalkMaxDepth), every offset read
// from a blob is checked against the blob's length before it forms an address, and every atomic
// is a vector atomic on a device word.

__device__ __forceinline__ void gc_verdict(const GcArgs& a, uint32_t v) {
  atomicMax(reinterpret_cast<unsigned long long*>(&a.g->verdict), (unsigned long long)v);
}

__device__ __forceinline__ void gc_lower(uint64_t* w, uint64_t v) {
  atomicMin(reinterpret_cast<unsigned long long*>(w), (unsigned long long)v);
}

// blob f (in the pool's index, so f < nblobs) is live; true for the one caller that expands it
__device__ __forceinline__ bool gc_claim(const GcArgs& a, uint64_t f) {
  a.live[f] = 1;
  return !(atomicOr(a.state + f, kGcClaimed) & kGcClaimed);
}

// ---- level 0: the Roots ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gc_roots(GcArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.nroots; r += stride) {
    const uint64_t* ref = reinterpret_cast<const uint64_t*>(a.roots + 32 * r);
    WalkItem w = {kWalkDead, 0, 0, r, 0, kWalkNoCover};
    uint64_t f = kWalkDead;
    uint32_t st = 0;
    if (ref[0] | ref[1] | ref[2] | ref[3]) {  // (bs.Zero is skipped)
      f = wk_probe(a.w, ref);
      if (f == kDedupEmpty) {
        st = kWalkNotFound;
        gc_verdict(a, kWalkNotFound);
      } else if (gc_claim(a, f)) {
        w.blob = f;
      }
    }
    a.rblob[r] = f;
    a.rstatus[r] = st;
    a.w.items[r] = w;
  }
}

// ---- emit ----------------------------------------------------------------------------------------
// where child k of frontier node i keeps its ref, as a pool offset (false, and the error flag, if
// the count pass's runs do not hold it)
__device__ __forceinline__ bool gc_child(const WalkArgs& w, uint64_t i, uint64_t k, uint64_t* at) {
  const WalkNode* nd = w.nodes + i;
  const uint64_t pb = w.items[i].blob;
  uint64_t len, pos;
  uint32_t elen;
  const uint8_t* b = pb == kWalkDead ? nullptr : wk_blob(w, pb, &len);
  if (!b || k >= nd->nchild) {
    wk_error(w, 32);
    return false;
  }
  if (!wk_entry(w, nd, len, k, &pos, &elen)) return false;
  *at = w.blobs[pb].off + pos + 4;  // (pos + elen <= len and elen >= 36: the ref lies in the blob)
  return true;
}

// First the level's nodes that failed the count pass (a live entry without a kind), then one
// thread per child of the others.
__global__ __launch_bounds__(256) void k_gc_emit(GcArgs a) {
  const WalkArgs& w = a.w;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (uint64_t i = tid; i < w.n; i += stride) {
    const uint64_t pb = w.items[i].blob;
    if (pb == kWalkDead || w.nodes[i].kind != 0) continue;
    if (pb >= w.nblobs) {
      wk_error(w, 1 << 12);
      continue;
    }
    atomicOr(a.state + pb, kGcFailed);
    gc_lower(&a.g->bad_form, pb);
    gc_verdict(a, kWalkCorrupt);
  }
  for (uint64_t t = tid; t < w.nchild; t += stride) {
    const uint64_t i = seg_find(0, w.n, t, [&w](uint64_t j) { return w.call[j]; });
    const uint64_t k = t - w.call[i], pb = w.items[i].blob;
    uint64_t at, ref[4];
    if (t < w.call[i] || !gc_child(w, i, k, &at)) {
      wk_error(w, 64);
      continue;
    }
    __builtin_memcpy(ref, w.pool + at, 32);
    if (w.nodes[i].kind == 1) {
      if (w.last) {  // its children would lie deeper than kWalkMaxDepth: refused unread
        gc_lower(&a.g->bad_form, pb);
        gc_verdict(a, kWalkCorrupt);
        continue;
      }
      const uint64_t slot = w.cnode[i] + k;
      if (slot >= w.nnext) {
        wk_error(w, 128);
        continue;
      }
      WalkItem x = {kWalkDead, 0, 0, i, 0, kWalkNoCover};
      const uint64_t f = wk_probe(w, ref);
      if (f == kDedupEmpty) {
        gc_lower(&a.g->bad_miss, pb);
        gc_verdict(a, kWalkNotFound);
      } else if (gc_claim(a, f)) {
        x.blob = f;
      }
      w.next[slot] = x;
    } else {
      const uint64_t f = wk_probe(w, ref);
      if (f != kDedupEmpty) {
        a.live[f] = 1;
      } else if (a.forgive) {
        atomicOr(reinterpret_cast<unsigned long long*>(&a.g->leaf_miss), 1ull);
      } else {
        gc_lower(&a.g->bad_miss, pb);
        gc_verdict(a, kWalkNotFound);
      }
    }
  }
}

// ---- the Roots' own verdicts ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gc_status(GcArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.nroots; r += stride) {
    const uint64_t f = a.rblob[r];
    if (f < a.w.nblobs && (a.state[f] & kGcFailed)) a.rstatus[r] = kWalkCorrupt;
  }
}

// ---- BSG_GC_MISSING_LEAVES: the distinct refs the pool lacks -------------------------------------
// A level's `leaves` children once more. A miss enters a table of pool offsets by the 32 bytes
// there (k_dd_insert's scheme: a slot's key never changes once claimed); a claimed slot is one
// more distinct ref.
__global__ __launch_bounds__(256) void k_gc_missing(GcArgs a) {
  const WalkArgs& w = a.w;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < w.nchild; t += stride) {
    const uint64_t i = seg_find(0, w.n, t, [&w](uint64_t j) { return w.call[j]; });
    if (w.nodes[i].kind != 2) continue;
    uint64_t at, ref[4], other[4];
    if (t < w.call[i] || !gc_child(w, i, t - w.call[i], &at)) {
      wk_error(w, 1 << 13);
      continue;
    }
    __builtin_memcpy(ref, w.pool + at, 32);
    if (wk_probe(w, ref) != kDedupEmpty) continue;
    bool done = false;
    for (uint64_t p = 0; p <= a.mmask && !done; ++p) {
      unsigned long long* slot =
          reinterpret_cast<unsigned long long*>(a.mtab + ((ref[0] + p) & a.mmask));
      const uint64_t cur = atomicCAS(slot, (unsigned long long)kDedupEmpty, (unsigned long long)at);
      if (cur == kDedupEmpty) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&a.g->missing_leaves), 1ull);
        done = true;
      } else if (cur > w.pool_bytes || w.pool_bytes - cur < 32) {
        wk_error(w, 1 << 14);
        done = true;
      } else {
        __builtin_memcpy(other, w.pool + cur, 32);
        done = ref_eq(ref, other);
      }
    }
    if (!done) wk_error(w, 1 << 15);
  }
}

// ---- the new offsets -----------------------------------------------------------------------------
struct GvLive {
  __device__ uint64_t operator()(const GcArgs& a, uint64_t k) const { return a.live[k] ? 1 : 0; }
};
struct GvLen {
  __device__ uint64_t operator()(const GcArgs& a, uint64_t k) const {
    return a.live[k] ? a.w.blobs[k].len : 0;
  }
};
struct GvLen16 {
  __device__ uint64_t operator()(const GcArgs& a, uint64_t k) const {
    return a.live[k] ? (a.w.blobs[k].len + 15) & ~15ull : 0;
  }
};

// the end of the last live blob's bytes in either variant (the offsets ascend, so the largest)
__global__ __launch_bounds__(256) void k_gc_offsets(GcArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.w.nblobs; k += stride) {
    if (!a.live[k]) continue;
    const uint64_t len = a.w.blobs[k].len;
    atomicMax(reinterpret_cast<unsigned long long*>(&a.g->end),
              (unsigned long long)(a.noff[k] + len));
    atomicMax(reinterpret_cast<unsigned long long*>(&a.g->end16),
              (unsigned long long)(a.noff16[k] + len));
  }
}

// ---- compact -------------------------------------------------------------------------------------
// Partitioned by output tiles of kGcTile bytes, as k_pack. A segment is a live blob's bytes at its
// new offset or, with BSG_GC_ALIGN16, the zero bytes (at most 15) between its end and the next
// blob's start; gather_tile does the rest.
__global__ __launch_bounds__(256) void k_gc_compact(GcArgs a) {
  const WalkArgs& w = a.w;
  const uint64_t t0 = (uint64_t)blockIdx.x * kGcTile;
  if (t0 >= a.total || !w.nblobs) return;
  const uint64_t t1 = min(t0 + (uint64_t)kGcTile, a.total);
  const auto off = [&a](uint64_t k) { return a.coff[k]; };
  __shared__ uint64_t seg[2];
  if (threadIdx.x == 0) {
    seg[0] = seg_find(0, w.nblobs, t0, off);
    seg[1] = seg_find(seg[0], w.nblobs, t1 - 1, off);
  }
  __syncthreads();
  const uint64_t k1 = seg[1];
  uint64_t k = seg[0];
  gather_tile<false>(a.out, t0, t1, a.total, [&](uint64_t pos, GatherSeg* g) {
    k = seg_find(k, k1 + 1, pos, off);
    const uint64_t o = a.coff[k], nx = a.coff[k + 1], len = w.blobs[k].len, so = w.blobs[k].off;
    g->src = nullptr;
    if (!a.live[k] || pos < o || pos >= nx || so > w.pool_bytes || len > w.pool_bytes - so ||
        nx - o < len || nx - o - len > 15) {
      wk_error(w, 1 << 16);
      return false;
    }
    if (pos - o < len) {
      g->src = w.pool + so;
      g->b0 = o;
      g->b1 = o + len;
    } else {
      g->src = a.g->zero;
      g->b0 = o + len;
      g->b1 = nx;
    }
    return true;
  });
}

// ---- launchers ---------------------------------------------------------------------------------
hipError_t launch_gc_roots(const GcArgs& a, hipStream_t s, int num_cus) {
  if (a.nroots)
    hipLaunchKernelGGL(k_gc_roots, dim3(engine_grid(a.nroots, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_gc_emit(const GcArgs& a, hipStream_t s, int num_cus) {
  const uint64_t items = a.w.n > a.w.nchild ? a.w.n : a.w.nchild;
  if (items)
    hipLaunchKernelGGL(k_gc_emit, dim3(engine_grid(items, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_gc_status(const GcArgs& a, hipStream_t s, int num_cus) {
  if (a.nroots)
    hipLaunchKernelGGL(k_gc_status, dim3(engine_grid(a.nroots, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_gc_missing(const GcArgs& a, hipStream_t s, int num_cus) {
  if (a.w.nchild)
    hipLaunchKernelGGL(k_gc_missing, dim3(engine_grid(a.w.nchild, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// rank, noff and noff16 over the blobs, then the two ends
hipError_t launch_gc_offsets(const GcArgs& a, hipStream_t s, int num_cus) {
  const uint64_t n = a.w.nblobs;
  hipError_t e;
  if ((e = launch_sum<GvLive>(a, n, a.rank, s)) != hipSuccess) return e;
  if ((e = launch_sum<GvLen>(a, n, a.noff, s)) != hipSuccess) return e;
  if ((e = launch_sum<GvLen16>(a, n, a.noff16, s)) != hipSuccess) return e;
  if (n) hipLaunchKernelGGL(k_gc_offsets, dim3(engine_grid(n, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_gc_compact(const GcArgs& a, hipStream_t s) {
  if (!a.total) return hipSuccess;
  const uint64_t tiles = (a.total + kGcTile - 1) / kGcTile;
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gc_compact, dim3((uint32_t)tiles), dim3(256), 0, s, a);
  return hipGetLastError();
}
