// bsgpu_read.inc — split.Reader's Seek + Read for many byte ranges at once, on the device
// (bsg_engine_read): range q is bytes [offset, offset + len) of the stream under a Root, and only
// the nodes on the way to those bytes and the chunks under them are visited. Included from
// bsgpu_kernels.hip after bsgpu_walk.inc and bsgpu_restore.inc, inside namespace bsg. DESIGN §4.14.
//
// A range is a stream of the walk with a window (WalkArgs::win): k_wk_roots, k_wk_count and
// k_wk_emit run as in bsg_engine_walk, and k_wk_emit follows a child only if its cover has a byte
// in the window. A child that is not followed leaves a dead frontier entry (`nodes`) or nothing
// (`leaves`), so a frontier keeps its places and its order. What differs from the walk's placement
// is here: child offsets ascend, so the followed children of a leaf node are one run
// [lfirst, lfirst + nrec) of its children, found by two binary searches (k_rd_nrec); the records
// below every node follow as in the walk, and one thread per followed leaf child writes its record
// (k_rd_records). The records of a range are then exactly the chunks under it, in order, with
// their own stream offsets and whole lens.
//
// The records are resolved as in bsg_engine_restore and every range's run is held to cover its
// window (k_rd_check, k_rd_streams); the scatter is k_rs_scatter with RestoreArgs::win0. One byte
// per pool blob says whether the read touched it (the Roots and the followed `nodes` children in
// the walk, the followed leaves in k_rd_resolve); with BSG_READ_VERIFY the touched blobs alone, as
// a list of indices (k_rd_tlist), go through the hash runs.
//
// Every loop is bounded (64 steps of a binary search, the grid strides), and every index or offset
// read from device memory is checked against its range before it forms an address; a bound that
// runs out sets the error word.

// ---- placement ---------------------------------------------------------------------------------
// the offset of child k of a leaf node (false, and the error flag, if the runs do not hold it)
__device__ __forceinline__ bool rd_child_off(const WalkArgs& a, const WalkNode* nd,
                                             const uint8_t* b, uint64_t len, uint64_t k,
                                             uint64_t* off) {
  uint64_t pos;
  uint32_t elen;
  if (!wk_entry(a, nd, len, k, &pos, &elen)) return false;
  *off = wk_entry_offset(b + pos, elen);
  return true;
}

// how many of the node's n children have an offset below t (incl: at or below); offsets ascend
__device__ __forceinline__ bool rd_count_below(const WalkArgs& a, const WalkNode* nd,
                                               const uint8_t* b, uint64_t len, uint64_t n,
                                               uint64_t t, bool incl, uint64_t* out) {
  uint64_t lo = 0, hi = n;
  for (uint32_t it = 0; it < 64 && lo < hi; ++it) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    uint64_t off;
    if (!rd_child_off(a, nd, b, len, mid, &off)) return false;
    if (off < t || (incl && off == t)) lo = mid + 1;
    else hi = mid;
  }
  *out = lo;
  return lo == hi;
}

// bottom-up, one thread per node: a leaf node's run of followed children, a `nodes` node's records
// as the walk counts them (a dead child has none)
__global__ __launch_bounds__(256) void k_rd_nrec(WalkArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    WalkNode* nd = a.nodes + i;
    uint64_t v = 0, first = 0;
    if (nd->kind == 2) {
      const uint32_t s = a.items[i].stream;
      uint64_t len = 0;
      const uint8_t* b =
          a.items[i].blob == kWalkDead ? nullptr : wk_blob(a, a.items[i].blob, &len);
      if (!b || s >= a.ns) {
        wk_error(a, 1 << 13);
      } else {
        const uint64_t w0 = a.win[2ull * s], w1 = a.win[2ull * s + 1], n = nd->nchild;
        uint64_t upto = 0, below = 0;  // children that start at or before w0, and before w1
        if (w0 < w1) {
          if (!rd_count_below(a, nd, b, len, n, w0, true, &upto) ||
              !rd_count_below(a, nd, b, len, n, w1, false, &below)) {
            wk_error(a, 1 << 14);
          } else {
            // child upto - 1 holds w0, unless it is the last and the node ends at or before w0
            first = upto ? upto - 1 : 0;
            if (upto == n && nd->offset + nd->size <= w0) first = n;
            v = below > first ? below - first : 0;
          }
        }
      }
    } else if (nd->kind == 1) {
      const uint64_t c0 = a.cnode[i];
      if (!a.down_prec || c0 > a.down_n || nd->nchild > a.down_n - c0) wk_error(a, 256);
      else v = a.down_prec[c0 + nd->nchild] - a.down_prec[c0];
    }
    nd->nrec = v;
    a.lfirst[i] = first;
  }
}

struct WvLeafRecs {  // the followed children of a leaf node
  __device__ uint64_t operator()(const WalkArgs& a, uint64_t i) const {
    return a.nodes[i].kind == 2 ? a.nodes[i].nrec : 0;
  }
};

// one thread per followed `leaves` child of the level (lpre[n] of them, at most a.nchild): its
// record, at its place in stream order
__global__ __launch_bounds__(256) void k_rd_records(WalkArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t nt = a.lpre[a.n];
  if (nt > a.nchild) {
    if (blockIdx.x == 0 && threadIdx.x == 0) wk_error(a, 1 << 15);
    return;
  }
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += stride) {
    const uint64_t i = seg_find(0, a.n, t, [&a](uint64_t j) { return a.lpre[j]; });
    const uint64_t l0 = a.lpre[i];
    WkChild c;
    if (t < l0 || a.nodes[i].kind != 2 || t - l0 >= a.nodes[i].nrec ||
        a.lfirst[i] >= a.nodes[i].nchild || !wk_child(a, i, a.lfirst[i] + (t - l0), &c)) {
      wk_error(a, 1024);
      continue;
    }
    const uint64_t at = a.nodes[i].rbase + (t - l0);
    if (at >= a.nrec || c.off >= c.end) {
      wk_error(a, 2048);
      continue;
    }
    ChunkRec* r = a.rec + at;
    r->offset = c.off;
    r->len = c.end - c.off;
    r->level = 0;
    r->stream = a.items[i].stream;
    uint64_t* ref = reinterpret_cast<uint64_t*>(r->ref);
    for (int w = 0; w < 4; ++w) ref[w] = c.ref[w];
  }
}

// ---- resolve and tiling --------------------------------------------------------------------------
// record i -> its blob's pool offset, and the blob is touched (the emit pass found every one of
// them with the same len, so a miss here is a fault of the passes, not of the pool)
__global__ __launch_bounds__(256) void k_rd_resolve(RestoreArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.nrec; i += stride) {
    const uint64_t f = pool_lookup(a.blobs, a.nblobs, a.tab, a.tab_mask,
                                   reinterpret_cast<const uint64_t*>(a.rec[i].ref), &a.hdr->dd);
    uint64_t so = 0;
    if (f == kDedupEmpty) {
      rs_lower(&a.hdr->missing, i);
    } else if (a.blobs[f].len != a.rec[i].len) {
      rs_lower(&a.hdr->mismatch, i);
    } else {
      so = a.blobs[f].off;
      if (so > a.pool_bytes || a.rec[i].len > a.pool_bytes - so) {  // (the host checked the blobs)
        rs_error(a.hdr, 4);
        so = 0;
      } else {
        a.touched[f] = 1;
      }
    }
    a.seg[i] = so;
  }
}

// Pairwise over neighbours: streams never descend and a stream's records follow each other
// without gap or overlap, so every stream has one run of records and its first and last index
// are each written once.
__global__ __launch_bounds__(256) void k_rd_check(RestoreArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.nrec; i += stride) {
    const uint64_t off = a.rec[i].offset, len = a.rec[i].len;
    const uint32_t s = a.rec[i].stream;
    bool bad = s >= a.ns || len == 0 || off + len < off;
    bool first = i == 0;
    if (i) {
      const uint32_t ps = a.rec[i - 1].stream;
      const uint64_t pend = a.rec[i - 1].offset + a.rec[i - 1].len;
      if (ps > s) bad = true;
      else if (ps == s) bad = bad || pend != off;
      else first = true;
      if (ps != s && ps < a.ns) a.slast[ps] = i - 1;
    }
    if (first && s < a.ns) a.sfirst[s] = i;
    if (i + 1 == a.nrec && s < a.ns) a.slast[s] = i;
    if (bad) atomicOr(reinterpret_cast<unsigned long long*>(&a.hdr->invalid), 1ull);
  }
}

// a range's run covers its window and no more: the first record holds the window's first byte,
// the last one its last byte; an empty window has no records
__global__ __launch_bounds__(256) void k_rd_streams(RestoreArgs a) {
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < a.ns; s += gridDim.x * blockDim.x) {
    const uint64_t f = a.sfirst[s], l = a.slast[s], got = a.out_len[s], w0 = a.win0[s];
    bool bad;
    if (got == 0) {
      bad = f != kDedupEmpty || l != kDedupEmpty;
    } else {
      bad = f >= a.nrec || l >= a.nrec || f > l || w0 + got < w0;
      if (!bad) {
        const uint64_t last = w0 + got - 1;
        bad = a.rec[f].stream != s || a.rec[l].stream != s || a.rec[f].offset > w0 ||
              a.rec[f].offset + a.rec[f].len <= w0 || a.rec[l].offset > last ||
              a.rec[l].offset + a.rec[l].len <= last;
      }
    }
    if (bad) atomicOr(reinterpret_cast<unsigned long long*>(&a.hdr->invalid), 2ull);
  }
}

// ---- verify: the touched blobs alone -------------------------------------------------------------
struct TvTouched {
  __device__ uint64_t operator()(const TouchArgs& a, uint64_t k) const {
    return a.r.touched[k] ? 1 : 0;
  }
};

// touched blob k becomes entry tpre[k] of the list (a.ntouched: its capacity) and is held to the
// hash path's layout rules; a wave adds its blobs' lens to *verified with one atomic
__global__ __launch_bounds__(256) void k_rd_tlist(TouchArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t rounds = (a.r.nblobs + stride - 1) / stride;
  const uint64_t k0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t sum = 0;
  for (uint64_t r = 0; r < rounds; ++r) {
    const uint64_t k = k0 + r * stride;
    if (k >= a.r.nblobs || !a.r.touched[k]) continue;
    const uint64_t at = a.tpre[k], off = a.r.blobs[k].off, len = a.r.blobs[k].len;
    if (at >= a.ntouched) {
      rs_error(a.r.hdr, 512);
      continue;
    }
    a.tlist[at] = k;
    if ((off & 15) || len >= (1ull << 40) || off > a.r.pool_bytes ||
        len > a.r.pool_bytes - off || a.r.pool_bytes - off - len < kReadSlack)
      atomicOr(reinterpret_cast<unsigned long long*>(&a.r.hdr->invalid), 4ull);
    sum += len;
  }
  for (int o = 32; o > 0; o >>= 1) sum += (uint64_t)__shfl_down((unsigned long long)sum, o);
  if ((threadIdx.x & 63) == 0 && sum)
    atomicAdd(reinterpret_cast<unsigned long long*>(a.verified), (unsigned long long)sum);
}

// entry t of the list: a touched blob's index (the error flag, and blob 0's place, if it is none)
__device__ __forceinline__ bool rd_touched_at(const TouchArgs& a, uint64_t t, uint64_t* k) {
  *k = t < a.ntouched ? a.tlist[t] : ~0ull;
  if (*k < a.r.nblobs) return true;
  rs_error(a.r.hdr, 1024);
  return false;
}

__global__ __launch_bounds__(256) void k_rd_descs(TouchArgs a, uint64_t t0, uint32_t n,
                                                  StreamDesc* d) {
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < n; b += gridDim.x * blockDim.x) {
    uint64_t k;
    StreamDesc sd = {};
    if (rd_touched_at(a, t0 + b, &k)) sd = rs_blob_desc(a.r, k);
    else sd.finalize = 1;  // (an empty blob: the run stays well formed)
    d[b] = sd;
  }
}

__global__ __launch_bounds__(256) void k_rd_compare(TouchArgs a, uint64_t t0, uint32_t n,
                                                    const ChunkRec* hashed, const Counters* hctr) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && (hctr->error || hctr->overflow))
    rs_error(a.r.hdr, 16 | (hctr->error << 16));
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < n; b += gridDim.x * blockDim.x) {
    uint64_t k;
    if (!rd_touched_at(a, t0 + b, &k)) continue;
    const PoolBlob* pb = a.r.blobs + k;
    if (hashed[b].len != pb->len) rs_error(a.r.hdr, 32);
    if (!ref_eq(reinterpret_cast<const uint64_t*>(hashed[b].ref),
                reinterpret_cast<const uint64_t*>(pb->ref)))
      rs_lower(&a.r.hdr->bad_blob, k);
  }
}

// ---- launchers ---------------------------------------------------------------------------------
hipError_t launch_read_nrec(const WalkArgs& a, hipStream_t s, int num_cus) {
  hipLaunchKernelGGL(k_rd_nrec, dim3(engine_grid(a.n, num_cus)), dim3(256), 0, s, a);
  hipError_t e;
  if ((e = launch_sum<WvRecs>(a, a.n, a.prec, s)) != hipSuccess) return e;
  return launch_sum<WvLeafRecs>(a, a.n, a.lpre, s);
}

hipError_t launch_read_place(const WalkArgs& a, uint64_t leaf_bound, hipStream_t s, int num_cus) {
  hipLaunchKernelGGL(k_wk_rbase, dim3(engine_grid(a.n, num_cus)), dim3(256), 0, s, a);
  if (leaf_bound && a.nrec) {
    WalkArgs r = a;
    r.nchild = leaf_bound;
    const uint64_t want = leaf_bound < a.nrec ? leaf_bound : a.nrec;
    hipLaunchKernelGGL(k_rd_records, dim3(engine_grid(want, num_cus)), dim3(256), 0, s, r);
  }
  return hipGetLastError();
}

hipError_t launch_read_resolve(const RestoreArgs& a, hipStream_t s, int num_cus) {
  if (a.nrec) {
    const uint32_t g = engine_grid(a.nrec, num_cus);
    hipLaunchKernelGGL(k_rd_resolve, dim3(g), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_rd_check, dim3(g), dim3(256), 0, s, a);
  }
  if (a.ns)
    hipLaunchKernelGGL(k_rd_streams, dim3(engine_grid(a.ns, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_read_touched(const TouchArgs& a, hipStream_t s, int num_cus) {
  if (!a.r.nblobs) return hipSuccess;
  const hipError_t e = launch_sum<TvTouched>(a, a.r.nblobs, a.tpre, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_rd_tlist, dim3(engine_grid(a.r.nblobs, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_read_descs(const TouchArgs& a, uint64_t t0, uint32_t n, StreamDesc* d,
                             hipStream_t s, int num_cus) {
  hipLaunchKernelGGL(k_rd_descs, dim3(engine_grid(n, num_cus)), dim3(256), 0, s, a, t0, n, d);
  return hipGetLastError();
}

hipError_t launch_read_compare(const TouchArgs& a, uint64_t t0, uint32_t n, const ChunkRec* hashed,
                               const Counters* hctr, hipStream_t s, int num_cus) {
  hipLaunchKernelGGL(k_rd_compare, dim3(engine_grid(n, num_cus)), dim3(256), 0, s, a, t0, n,
                     hashed, hctr);
  return hipGetLastError();
}
