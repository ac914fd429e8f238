// bsgpu_walk.inc — split.NewReader's walk for many streams at once, on the device
// (bsg_engine_walk): the inverse of bsg_engine_trees. A pool holds node blobs and chunk blobs side
// by side; from one Root per stream the walk follows `nodes` down to the `leaves` and leaves every
// stream's size and its records in the form bsg_engine_restore takes. Included from
// bsgpu_kernels.hip, inside namespace bsg. From bsgpu_engine_common.inc it takes the pool's index
// (launch_ref_index on the host's side, pool_lookup here), the prefix sum (launch_sum) and
// seg_find. DESIGN §4.10.
//
// Breadth first, every stream at once. Level L's frontier is every node at depth L, sorted by
// (stream, offset). Per level: one wave per node validates the blob's bytes and counts its
// children (k_wk_count), two prefix sums give every child its place, one thread per child probes
// the index and either queues a node for the next level or checks a leaf against its cover
// (k_wk_emit). When every level has passed, the records below each node are counted bottom-up
// (k_wk_nrec), each node's first record place follows top-down (k_wk_rbase) and one thread per
// leaf child writes its record (k_wk_records), so records come out in stream order whatever the
// depth of their leaf nodes.
//
// A node blob is PutProto's bytes (oracle.proto_node): entries `tag len 0a 20 <ref> [10 varint]`
// of one kind, then `18 varint(offset)` if non-zero, then `20 varint(size)`. With minimal varints
// and strictly ascending offsets an entry is 36 bytes (offset 0, only the first) or
// 37 + varint_len(offset), and that length never decreases along a node, so the entries lie in at
// most kWalkRuns runs of equal length. Every loop is bounded (by the blob length, the table size,
// kWalkMaxDepth), and every byte offset read from a blob is checked against the blob's length
// before it forms an address.

__device__ __forceinline__ void wk_error(const WalkArgs& a, uint64_t code) {
  dd_error(&a.hdr->dd, code);
}

// the verdict of stream s never falls: not found outranks corrupt outranks ok
__device__ __forceinline__ void wk_status(const WalkArgs& a, uint32_t s, uint32_t v) {
  if (s < a.ns) atomicMax(a.status + s, v);
  else wk_error(a, 1 << 10);
}

// the smallest pool blob index named r, or kDedupEmpty
__device__ __forceinline__ uint64_t wk_probe(const WalkArgs& a, const uint64_t* r) {
  return pool_lookup(a.blobs, a.nblobs, a.tab, a.tab_mask, r, &a.hdr->dd);
}

// blob k's bytes and length (null, and the error flag, if it does not lie in the pool)
__device__ __forceinline__ const uint8_t* wk_blob(const WalkArgs& a, uint64_t k, uint64_t* len) {
  *len = 0;
  if (k >= a.nblobs) {
    wk_error(a, 4);
    return nullptr;
  }
  const uint64_t off = a.blobs[k].off, n = a.blobs[k].len;
  if (off > a.pool_bytes || n > a.pool_bytes - off) {  // (the host checked the blobs)
    wk_error(a, 4);
    return nullptr;
  }
  *len = n;
  return a.pool + off;
}

// ---- level 0: the Roots ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_wk_roots(WalkArgs a) {
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < a.ns; s += gridDim.x * blockDim.x) {
    const uint64_t* r = reinterpret_cast<const uint64_t*>(a.roots + 32ull * s);
    WalkItem w = {kWalkDead, 0, 0, s, s, 0};
    if (r[0] | r[1] | r[2] | r[3]) {  // (bs.Zero: an empty stream)
      w.blob = wk_probe(a, r);
      if (w.blob == kWalkDead) wk_status(a, s, kWalkNotFound);
      else if (a.touched) a.touched[w.blob] = 1;  // (bsg_engine_read)
    }
    a.items[s] = w;
  }
}

// ---- count: one wave per frontier node ---------------------------------------------------------
// a wave-uniform byte of the blob
__device__ __forceinline__ uint32_t wk_u8(const uint8_t* b, uint64_t pos) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)b[pos]);
}

// a minimal, non-zero varint at b[*pos ..), inside the blob's len bytes
__device__ __forceinline__ bool wk_varint(const uint8_t* b, uint64_t len, uint64_t* pos,
                                          uint64_t* v) {
  uint64_t x = 0;
  for (uint32_t j = 0; j < 10; ++j) {
    if (*pos >= len) return false;
    const uint32_t c = wk_u8(b, *pos);
    ++*pos;
    x |= (uint64_t)(c & 0x7f) << (7 * j);
    if (!(c & 0x80)) {
      *v = x;
      return c != 0 && !(j == 9 && c > 1);
    }
  }
  return false;
}

// The wave walks the entries 64 at a time at the stride the entry at `pos` names: lane l holds
// the entry at pos + l * elen to the form and to ascending offsets, the ballot's leading run is
// taken, and a shorter run means a change of stride, the end of the entries or a fault, which
// the next step's lane 0 tells apart. Every branch on the way is wave-uniform.
__global__ __launch_bounds__(256) void k_wk_count(WalkArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t w0 = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), wstride = 4ull * gridDim.x;
  for (uint64_t i = w0; i < a.n; i += wstride) {
    const WalkItem it = a.items[i];
    WalkNode* nd = a.nodes + i;
    uint64_t len = 0, count = 0, pos = 0, prev = 0, first = 0, noff = 0, size = 0;
    uint32_t kind = 0, tag0 = 0, nruns = 0, last_elen = 0;
    const uint8_t* b = it.blob == kWalkDead ? nullptr : wk_blob(a, it.blob, &len);
    bool bad = false;
    while (b && !bad && pos < len) {
      const uint32_t tag = wk_u8(b, pos);
      if (tag != 0x0a && tag != 0x12) break;  // the entries have ended
      if (!kind) kind = tag == 0x0a ? 1 : 2, tag0 = tag;
      if (tag != tag0 || len - pos < 2) {
        bad = true;
        break;
      }
      const uint32_t lb = wk_u8(b, pos + 1), elen = lb + 2;
      if (lb < 34 || lb == 35 || lb > 45) {
        bad = true;
        break;
      }
      const uint64_t room = (len - pos) / elen;  // whole entries that fit
      bool ok = lane < room;
      uint64_t off = 0;
      if (ok) {
        const uint8_t* p = b + pos + (uint64_t)lane * elen;
        ok = p[0] == tag && p[1] == lb && p[2] == 0x0a && p[3] == 0x20;
        if (elen > 36) {
          const uint32_t vl = elen - 37;
          ok = ok && p[36] == 0x10;
          for (uint32_t j = 0; j < 10; ++j) {
            if (j >= vl) continue;
            const uint32_t c = p[37 + j];
            off |= (uint64_t)(c & 0x7f) << (7 * j);
            if (j + 1 < vl) ok = ok && (c & 0x80);
            else ok = ok && !(c & 0x80) && c != 0 && !(j == 9 && c > 1);
          }
        }
      }
      uint64_t before = (uint64_t)__shfl_up((unsigned long long)off, 1);
      if (lane == 0) before = prev;
      ok = ok && ((lane == 0 && count == 0) || off > before);
      const unsigned long long m = __ballot(ok);
      const uint32_t run = ~m ? (uint32_t)__builtin_ctzll(~m) : 64u;
      if (run == 0) {
        bad = true;
        break;
      }
      if (count == 0) first = (uint64_t)__shfl((unsigned long long)off, 0);
      prev = (uint64_t)__shfl((unsigned long long)off, (int)run - 1);
      if (elen != last_elen) {
        if (nruns < kWalkRuns) {
          if (lane == 0) {
            nd->run_pos[nruns] = pos;
            nd->run_idx[nruns] = count;
            nd->run_len[nruns] = elen;
          }
          ++nruns;
        } else {  // (lengths only grow, so this cannot be)
          wk_error(a, 8);
          bad = true;
        }
        last_elen = elen;
      }
      count += run;
      pos += (uint64_t)run * elen;
    }
    if (b && !bad) {  // offset if non-zero, size, and nothing after
      if (pos < len && wk_u8(b, pos) == 0x18) {
        ++pos;
        bad = !wk_varint(b, len, &pos, &noff);
      }
      if (!bad && pos < len && wk_u8(b, pos) == 0x20) {
        ++pos;
        bad = !wk_varint(b, len, &pos, &size);
      } else {
        bad = true;
      }
      bad = bad || pos != len || count == 0 || first != noff || noff + size < noff;
      // (a kWalkNoCover entry is held to the node's own rules alone: bsg_engine_gc_mark)
      if (!(it.flags & kWalkNoCover))
        bad = bad || noff != it.exp_off || (it.exp_size && size != it.exp_size);
    }
    if (lane == 0) {
      const bool live = b && !bad;
      nd->nchild = live ? count : 0;
      nd->offset = noff;
      nd->size = size;
      nd->nrec = 0;
      nd->rbase = 0;
      nd->kind = live ? kind : 0;
      nd->nruns = live ? nruns : 0;
      if (b) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&a.hdr->nnodes), 1ull);
        atomicMax(reinterpret_cast<unsigned long long*>(&a.hdr->depth),
                  (unsigned long long)a.level);
        if (bad) wk_status(a, it.stream, kWalkCorrupt);
      }
      if (live) {
        if (a.level == 0 && it.stream < a.ns) a.sizes[it.stream] = size;
        atomicAdd(reinterpret_cast<unsigned long long*>(&a.hdr->lvl_all[a.level]),
                  (unsigned long long)count);
        if (kind == 1)
          atomicAdd(reinterpret_cast<unsigned long long*>(&a.hdr->lvl_nodes[a.level]),
                    (unsigned long long)count);
      }
    }
  }
}

// ---- the values the prefix passes sum over a level's nodes -------------------------------------
struct WvAll {
  __device__ uint64_t operator()(const WalkArgs& a, uint64_t i) const { return a.nodes[i].nchild; }
};
struct WvNodes {
  __device__ uint64_t operator()(const WalkArgs& a, uint64_t i) const {
    return a.nodes[i].kind == 1 ? a.nodes[i].nchild : 0;
  }
};
struct WvRecs {
  __device__ uint64_t operator()(const WalkArgs& a, uint64_t i) const { return a.nodes[i].nrec; }
};

// ---- a node's child k ----------------------------------------------------------------------------
// where entry k lies in the blob's len bytes, by the node's runs (false, and the error flag, if
// the count pass's runs do not hold it)
__device__ __forceinline__ bool wk_entry(const WalkArgs& a, const WalkNode* nd, uint64_t len,
                                         uint64_t k, uint64_t* pos, uint32_t* elen) {
  uint32_t r = 0;
  for (uint32_t j = 1; j < kWalkRuns; ++j)
    if (j < nd->nruns && nd->run_idx[j] <= k) r = j;
  const uint64_t k0 = nd->run_idx[r];
  *elen = nd->run_len[r];
  *pos = nd->run_pos[r];
  if (k < k0 || *elen < 36 || *elen > 47 || (k - k0) > len / *elen) {
    wk_error(a, 16);
    return false;
  }
  *pos += (k - k0) * *elen;
  if (*pos > len || len - *pos < *elen) {
    wk_error(a, 16);
    return false;
  }
  return true;
}

__device__ __forceinline__ uint64_t wk_entry_offset(const uint8_t* p, uint32_t elen) {
  uint64_t off = 0;
  for (uint32_t j = 0; j < 10; ++j)
    if (37 + j < elen) off |= (uint64_t)(p[37 + j] & 0x7f) << (7 * j);
  return off;
}

// child k of node i: its ref, its offset and the end of its cover
struct WkChild {
  uint64_t ref[4];
  uint64_t off, end;
};
__device__ __forceinline__ bool wk_child(const WalkArgs& a, uint64_t i, uint64_t k, WkChild* c) {
  const WalkNode* nd = a.nodes + i;
  uint64_t len, pos;
  uint32_t elen;
  const uint8_t* b = a.items[i].blob == kWalkDead ? nullptr : wk_blob(a, a.items[i].blob, &len);
  if (!b || k >= nd->nchild) {
    wk_error(a, 32);
    return false;
  }
  if (!wk_entry(a, nd, len, k, &pos, &elen)) return false;
  __builtin_memcpy(c->ref, b + pos + 4, 32);
  c->off = wk_entry_offset(b + pos, elen);
  c->end = nd->offset + nd->size;
  if (k + 1 < nd->nchild) {
    if (!wk_entry(a, nd, len, k + 1, &pos, &elen)) return false;
    c->end = wk_entry_offset(b + pos, elen);
  }
  return true;
}

// ---- stream s's window (bsg_engine_read; a.win null: none, every child is followed) -------------
// true if the cover [off, end) has a byte in [win[2s], win[2s + 1])
__device__ __forceinline__ bool wk_in_window(const WalkArgs& a, uint32_t s, uint64_t off,
                                             uint64_t end) {
  if (!a.win) return true;
  if (s >= a.ns) return false;
  const uint64_t w0 = a.win[2ull * s], w1 = a.win[2ull * s + 1];
  return w0 < w1 && off < w1 && w0 < end;
}

// ---- emit: one thread per child ------------------------------------------------------------------
// A `nodes` child becomes the next frontier's entry cnode[i] + k (dead if the pool lacks it), so a
// frontier stays sorted by (stream, offset); a `leaves` child is held to its cover. With windows a
// child whose cover misses its stream's window is not probed: a `nodes` child leaves a dead entry
// without a verdict, a `leaves` child nothing; an empty cover is the listing node's fault.
__global__ __launch_bounds__(256) void k_wk_emit(WalkArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < a.nchild; t += stride) {
    const uint64_t i = seg_find(0, a.n, t, [&a](uint64_t j) { return a.call[j]; });
    const uint64_t k = t - a.call[i];
    const uint32_t s = a.items[i].stream;
    WkChild c;
    if (t < a.call[i] || !wk_child(a, i, k, &c)) {
      wk_error(a, 64);
      continue;
    }
    const bool covered = c.off < c.end;
    if (a.win && !(covered && wk_in_window(a, s, c.off, c.end))) {
      if (!covered) wk_status(a, s, kWalkCorrupt);
      if (a.nodes[i].kind == 1 && !a.last) {
        const uint64_t slot = a.cnode[i] + k;
        if (slot >= a.nnext) wk_error(a, 128);
        else a.next[slot] = WalkItem{kWalkDead, c.off, 0, i, s, 0};
      }
      continue;
    }
    if (a.nodes[i].kind == 1) {
      if (a.last) {  // its children would lie deeper than kWalkMaxDepth
        wk_status(a, s, kWalkCorrupt);
        continue;
      }
      const uint64_t slot = a.cnode[i] + k;
      if (slot >= a.nnext) {
        wk_error(a, 128);
        continue;
      }
      WalkItem w = {kWalkDead, c.off, c.end - c.off, i, s, 0};
      const uint64_t f = wk_probe(a, c.ref);
      if (f == kDedupEmpty) wk_status(a, s, kWalkNotFound);
      else if (!covered) wk_status(a, s, kWalkCorrupt);
      else w.blob = f;
      if (a.touched && w.blob != kWalkDead) a.touched[f] = 1;
      a.next[slot] = w;
    } else {
      const uint64_t f = wk_probe(a, c.ref);
      if (f == kDedupEmpty) wk_status(a, s, kWalkNotFound);
      else if (!covered || a.blobs[f].len != c.end - c.off) wk_status(a, s, kWalkCorrupt);
    }
  }
}

// ---- placement -------------------------------------------------------------------------------
// bottom-up: the records below a node. A node's children are one contiguous range of the level
// below, so the sum is a difference of that level's prefix.
__global__ __launch_bounds__(256) void k_wk_nrec(WalkArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    WalkNode* nd = a.nodes + i;
    uint64_t v = 0;
    if (nd->kind == 2) {
      v = nd->nchild;
    } else if (nd->kind == 1) {
      const uint64_t c0 = a.cnode[i];
      if (!a.down_prec || c0 > a.down_n || nd->nchild > a.down_n - c0) wk_error(a, 256);
      else v = a.down_prec[c0 + nd->nchild] - a.down_prec[c0];
    }
    nd->nrec = v;
  }
}

// top-down: a node's first record follows its parent's by the records below its elder siblings
__global__ __launch_bounds__(256) void k_wk_rbase(WalkArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < a.n; j += stride) {
    uint64_t v = a.prec[j];
    if (a.level) {
      const uint64_t i = a.items[j].parent;
      if (i >= a.up_n || a.up_cnode[i] > j) {
        wk_error(a, 512);
        continue;
      }
      v = a.up_nodes[i].rbase + v - a.prec[a.up_cnode[i]];
    }
    a.nodes[j].rbase = v;
  }
}

// one thread per `leaves` child of the level: its record, at its place in stream order
__global__ __launch_bounds__(256) void k_wk_records(WalkArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < a.nchild; t += stride) {
    // the node whose leaf children hold t (call - cnode: the prefix of the `leaves` children alone)
    const uint64_t i = seg_find(0, a.n, t, [&a](uint64_t j) { return a.call[j] - a.cnode[j]; });
    const uint64_t l0 = a.call[i] - a.cnode[i];
    WkChild c;
    if (t < l0 || a.nodes[i].kind != 2 || !wk_child(a, i, t - l0, &c)) {
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

// ---- launchers ---------------------------------------------------------------------------------
hipError_t launch_walk_roots(const WalkArgs& a, hipStream_t s, int num_cus) {
  if (a.ns) hipLaunchKernelGGL(k_wk_roots, dim3(engine_grid(a.ns, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// a.n >= 1 frontier entries: every node validated and counted, call / cnode filled
hipError_t launch_walk_count(const WalkArgs& a, hipStream_t s, int num_cus) {
  const uint64_t want = (a.n + 3) / 4, cap = 64ull * (uint32_t)num_cus;
  const uint64_t g = want < cap ? want : cap;
  hipLaunchKernelGGL(k_wk_count, dim3((uint32_t)g), dim3(256), 0, s, a);
  hipError_t e;
  if ((e = launch_sum<WvAll>(a, a.n, a.call, s)) != hipSuccess) return e;
  return launch_sum<WvNodes>(a, a.n, a.cnode, s);
}

hipError_t launch_walk_emit(const WalkArgs& a, hipStream_t s, int num_cus) {
  if (!a.nchild) return hipSuccess;
  hipLaunchKernelGGL(k_wk_emit, dim3(engine_grid(a.nchild, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_walk_nrec(const WalkArgs& a, hipStream_t s, int num_cus) {
  hipLaunchKernelGGL(k_wk_nrec, dim3(engine_grid(a.n, num_cus)), dim3(256), 0, s, a);
  return launch_sum<WvRecs>(a, a.n, a.prec, s);
}

// a.nchild: the level's `leaves` children
hipError_t launch_walk_place(const WalkArgs& a, hipStream_t s, int num_cus) {
  hipLaunchKernelGGL(k_wk_rbase, dim3(engine_grid(a.n, num_cus)), dim3(256), 0, s, a);
  if (a.nchild)
    hipLaunchKernelGGL(k_wk_records, dim3(engine_grid(a.nchild, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}
