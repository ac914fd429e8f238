// bsgpu_tree.inc — split.Writer's tree (split/split.go:51-126) for every stream of a finished
// run, built on the device from the run's chunk records (bsg_engine_trees). Included from
// bsgpu_kernels.hip, inside namespace bsg. From bsgpu_engine_common.inc it takes the prefix sum
// (launch_sum, wg_exclusive_sum) and engine_grid.
//
// Closed form (DESIGN §4, "Trees on the device"). With q_i = level_i / fanout, a stream's tree
// after the single-child prune has its Root at height R = max q_i over every chunk but the last
// (0 for a one-chunk stream): the last chunk closes every level whatever its own level is, and
// a top node with one child is pruned down to the first height where the stream has a second
// node. So chunk i closes k_i nodes, of heights 0 .. k_i - 1, with k_i = q_i for every chunk but
// the last and k_last = R + 1; a node of height h covers the chunks after the previous close at
// height h (or the stream's start) up to its closing chunk.
//
// Internal node ids are height-major: height h's nodes are close[hoff[h] .. hoff[h + 1]), the
// global indices of their closing chunks in stream-major order, so a node's children are one
// contiguous range of chunks (height 0) or of internal ids (height h - 1) and every byte
// position inside a blob is a difference of two prefix sums. No pass loops over a node's
// children on one thread.

// The tile of the shared prefix sum, under the name and in the file where the trees' limit tests
// read it (tests/tree_cases.py): they put a run on each side of one tile and of 256 tiles.
constexpr uint32_t kTreeTile = 2048;
static_assert(kTreeTile == kSumTile, "the tree limit tests pin the prefix sum's tile");

__device__ __forceinline__ void tree_error(const TreeArgs& a, uint64_t code) {
  atomicOr(reinterpret_cast<unsigned long long*>(&a.hdr->error), (unsigned long long)code);
}

__device__ __forceinline__ uint32_t varint_len(uint64_t v) {
  uint32_t n = 1;
  while (v >= 0x80) {
    v >>= 7;
    ++n;
  }
  return n;
}

// a Child inside a Node: tag, len, 0a 20 <ref>, and 10 varint(offset) when the offset is not 0
__device__ __forceinline__ uint32_t child_entry_len(uint64_t offset) {
  return offset ? 37u + varint_len(offset) : 36u;
}

__device__ __forceinline__ uint8_t* put_varint(uint8_t* p, uint64_t v) {
  while (v >= 0x80) {
    *p++ = (uint8_t)(v | 0x80);
    v >>= 7;
  }
  *p++ = (uint8_t)v;
  return p;
}

// first index in [0, n) with p[index] >= key (n if none)
__device__ __forceinline__ uint64_t tree_lower_bound(const uint64_t* p, uint64_t n, uint64_t key) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (p[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---- the values the prefix passes sum -------------------------------------------------------
struct TvCount {  // chunks per stream -> cstart
  __device__ uint64_t operator()(const TreeArgs& a, uint64_t i) const { return a.scount[i]; }
};
struct TvCloses {  // chunk i closes a node of height a.h
  __device__ uint64_t operator()(const TreeArgs& a, uint64_t i) const { return a.kcnt[i] > a.h; }
};
struct TvStreamHeight {  // nodes of stream s = i / H at height i % H -> listed order
  __device__ uint64_t operator()(const TreeArgs& a, uint64_t i) const {
    const uint32_t s = (uint32_t)(i / a.H), h = (uint32_t)(i % a.H);
    const uint64_t c0 = a.cstart[s], c1 = a.cstart[s + 1];
    if (c1 == c0 || h > a.rmax[s]) return 0;
    const uint64_t lo = a.hdr->hoff[h], n = a.hdr->hoff[h + 1] - lo;
    return tree_lower_bound(a.close + lo, n, c1) - tree_lower_bound(a.close + lo, n, c0);
  }
};
struct TvLeafEntry {
  __device__ uint64_t operator()(const TreeArgs& a, uint64_t i) const {
    return child_entry_len(a.rec[i].offset);
  }
};
struct TvNodeEntry {
  __device__ uint64_t operator()(const TreeArgs& a, uint64_t u) const {
    return child_entry_len(a.meta[u].offset);
  }
};
struct TvArena {  // blobs start 16-byte aligned (the SHA-256 loaders)
  __device__ uint64_t operator()(const TreeArgs& a, uint64_t u) const {
    return ((uint64_t)a.meta[u].blob_len + 15u) & ~15ull;
  }
};

// ---- counting -------------------------------------------------------------------------------
// rmax[s] = R: the largest q over every chunk of the stream but its last (rmax starts zeroed)
__global__ __launch_bounds__(256) void k_tree_rmax(TreeArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t rounds = (a.M + stride - 1) / stride;
  for (uint64_t r = 0; r < rounds; ++r) {
    const uint64_t i = r * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t s = ~0u, q = 0;
    if (i < a.M) {
      s = a.rec[i].stream;
      const bool last = i + 1 == a.M || a.rec[i + 1].stream != s;
      if (s >= a.ns) {
        tree_error(a, 1);
        s = ~0u;
      } else if (!last) {
        q = a.rec[i].level / a.fanout;
        if (q > kTreeMaxHeights - 2) {  // levels are at most 32: cannot happen
          tree_error(a, 2);
          q = kTreeMaxHeights - 2;
        }
      }
    }
    // one stream per wave is the common case: one atomic per wave, not 64 on one address
    const uint32_t s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s);
    if (__all(s == s0)) {
      for (int o = 32; o > 0; o >>= 1) q = max(q, (uint32_t)__shfl_xor((int)q, o));
      if ((threadIdx.x & 63) == 0 && s0 != ~0u && q) atomicMax(a.rmax + s0, q);
    } else if (s != ~0u && q) {
      atomicMax(a.rmax + s, q);
    }
  }
}

// kcnt[i] = k_i, and the totals: nodes of all streams, the largest R
__global__ __launch_bounds__(256) void k_tree_kcnt(TreeArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint64_t sum = 0;
  uint32_t mx = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.M; i += stride) {
    const uint32_t s = a.rec[i].stream;
    if (s >= a.ns) continue;  // flagged by k_tree_rmax
    const bool last = i + 1 == a.M || a.rec[i + 1].stream != s;
    uint32_t k;
    if (last) {
      k = a.rmax[s] + 1;
      mx = max(mx, k - 1);
    } else {
      k = min(a.rec[i].level / a.fanout, kTreeMaxHeights - 2);
    }
    a.kcnt[i] = (uint8_t)k;
    sum += k;
  }
  uint64_t tot;
  (void)wg_exclusive_sum(sum, &tot);
  __shared__ uint32_t smx;
  if (threadIdx.x == 0) smx = 0;
  __syncthreads();
  if (mx) atomicMax(&smx, mx);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (tot) atomicAdd(reinterpret_cast<unsigned long long*>(&a.hdr->nnodes), (unsigned long long)tot);
    if (smx) atomicMax(reinterpret_cast<unsigned long long*>(&a.hdr->max_r), (unsigned long long)smx);
  }
}

// height a.h's closing chunks, in order: tmp = the exclusive prefix of TvCloses over the chunks
__global__ __launch_bounds__(256) void k_tree_compact(TreeArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t base = a.hdr->hoff[a.h];
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.M; i += stride) {
    if (a.kcnt[i] <= a.h) continue;
    const uint64_t u = base + a.tmp[i];
    if (u >= a.nn) {
      tree_error(a, 4);
      continue;
    }
    a.close[u] = i;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.hdr->hoff[a.h + 1] = base + a.tmp[a.M];
}

// every node's range, children and place in the listed order
__global__ __launch_bounds__(256) void k_tree_meta(TreeArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  if (a.hdr->hoff[a.H] != a.nn) {
    if (blockIdx.x == 0 && threadIdx.x == 0) tree_error(a, 8);
    return;
  }
  for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < a.nn; u += stride) {
    uint32_t h = 0;
    while (h + 1 < a.H && u >= a.hdr->hoff[h + 1]) ++h;
    const uint64_t lo = a.hdr->hoff[h], n = a.hdr->hoff[h + 1] - lo, j = u - lo;
    const uint64_t e = a.close[u];
    const uint32_t s = a.rec[e].stream;
    const uint64_t first = tree_lower_bound(a.close + lo, n, a.cstart[s]);
    const uint64_t sc = j > first ? a.close[u - 1] + 1 : a.cstart[s];
    TreeNodeMeta m;
    m.offset = a.rec[sc].offset;
    m.size = a.rec[e].offset + a.rec[e].len - m.offset;
    if (h == 0) {
      m.child0 = sc;
      m.nchild = e - sc + 1;
    } else {
      const uint64_t clo = a.hdr->hoff[h - 1], cn = lo - clo;
      const uint64_t cf = tree_lower_bound(a.close + clo, cn, sc);
      const uint64_t cl = tree_lower_bound(a.close + clo, cn, e);
      if (cl >= cn || a.close[clo + cl] != e || cf > cl) {  // a close at h is a close at h - 1
        tree_error(a, 16);
        m.child0 = clo;
        m.nchild = 0;
      } else {
        m.child0 = clo + cf;
        m.nchild = cl - cf + 1;
      }
    }
    m.out_idx = a.shbase[(uint64_t)s * a.H + h] + (j - first);
    if (m.out_idx >= a.nn) {
      tree_error(a, 32);
      m.out_idx = 0;
      m.nchild = 0;
    }
    m.blob_off = 0;
    m.blob_len = 0;
    m.stream = s;
    a.meta[u] = m;
  }
}

// blob lengths: the children's entries (a difference of two prefix sums), then offset and size
__global__ __launch_bounds__(256) void k_tree_len(TreeArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t h1 = a.hdr->hoff[1 < a.H ? 1 : a.H];  // ids below it are height 0
  for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < a.nn; u += stride) {
    const TreeNodeMeta m = a.meta[u];
    const uint64_t* pre = u < h1 ? a.pc : a.pn;
    uint64_t len = m.nchild ? pre[m.child0 + m.nchild] - pre[m.child0] : 0;
    if (m.offset) len += 1 + varint_len(m.offset);
    if (m.size) len += 1 + varint_len(m.size);
    if (len > 0xffffffffull - 64) {
      tree_error(a, 64);
      len = 0;
    }
    a.meta[u].blob_len = (uint32_t)len;
  }
}

__global__ __launch_bounds__(256) void k_tree_place(TreeArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < a.nn; u += stride)
    a.meta[u].blob_off = a.aoff[u];
  if (blockIdx.x == 0 && threadIdx.x == 0) a.hdr->arena_bytes = a.aoff[a.nn];
}

// ---- emit: one thread per child ------------------------------------------------------------
// The entry of child `c` of node m at prefix position pre[c] - pre[m.child0], and after the
// node's last child its offset and size. Every write is checked against the blob's own bytes.
__device__ __forceinline__ void tree_put_child(const TreeArgs& a, const TreeNodeMeta& m,
                                               const uint64_t* pre, uint64_t c, uint8_t tag,
                                               const uint8_t* ref, uint64_t coff) {
  const uint64_t pos = pre[c] - pre[m.child0];
  const uint32_t elen = child_entry_len(coff);
  const bool lastc = c + 1 == m.child0 + m.nchild;
  uint32_t tail = 0;
  if (lastc) tail = (m.offset ? 1 + varint_len(m.offset) : 0) + (m.size ? 1 + varint_len(m.size) : 0);
  if (pos + elen + tail > m.blob_len || (lastc && pos + elen + tail != m.blob_len) ||
      m.blob_off + m.blob_len > a.arena_bytes) {
    tree_error(a, 128);
    return;
  }
  uint8_t* p = a.arena + m.blob_off + pos;
  *p++ = tag;
  *p++ = (uint8_t)(elen - 2);
  *p++ = 0x0a;
  *p++ = 0x20;
  for (int k = 0; k < 32; ++k) *p++ = ref[k];
  if (coff) {
    *p++ = 0x10;
    p = put_varint(p, coff);
  }
  if (lastc) {
    if (m.offset) {
      *p++ = 0x18;
      p = put_varint(p, m.offset);
    }
    if (m.size) {
      *p++ = 0x20;
      p = put_varint(p, m.size);
    }
  }
}

__global__ __launch_bounds__(256) void k_tree_emit_leaves(TreeArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t n0 = a.hdr->hoff[1];
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.M; i += stride) {
    const uint64_t u = tree_lower_bound(a.close, n0, i);
    if (u >= n0) {  // a stream's last chunk closes height 0
      tree_error(a, 256);
      continue;
    }
    const TreeNodeMeta m = a.meta[u];
    if (i < m.child0 || i >= m.child0 + m.nchild) {
      tree_error(a, 256);
      continue;
    }
    tree_put_child(a, m, a.pc, i, 0x12, a.rec[i].ref, a.rec[i].offset);
  }
}

// height a.h >= 1: the children are the nodes of height a.h - 1 (their refs are in `nodes`)
__global__ __launch_bounds__(256) void k_tree_emit_nodes(TreeArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t c0 = a.hdr->hoff[a.h - 1], lo = a.hdr->hoff[a.h], n = a.hdr->hoff[a.h + 1] - lo;
  for (uint64_t v = c0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < lo; v += stride) {
    const uint64_t j = tree_lower_bound(a.close + lo, n, a.close[v]);
    if (j >= n) continue;  // a Root of height a.h - 1
    const TreeNodeMeta m = a.meta[lo + j];
    if (v < m.child0 || v >= m.child0 + m.nchild) continue;  // a Root before another stream
    const TreeNodeMeta c = a.meta[v];
    tree_put_child(a, m, a.pn, v, 0x0a, a.nodes[c.out_idx].ref, c.offset);
  }
}

// ---- hashing: a height's blobs as the descriptors of a hash run (k_start's source) ----------
__global__ __launch_bounds__(256) void k_tree_descs(TreeArgs a, uint64_t u0, uint32_t n,
                                                    StreamDesc* d) {
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < n; b += gridDim.x * blockDim.x) {
    const TreeNodeMeta m = a.meta[u0 + b];
    StreamDesc sd = {};
    sd.data_off = m.blob_off;
    sd.len = m.blob_len;
    sd.finalize = 1;
    sd.mid[0] = 0x6a09e667; sd.mid[1] = 0xbb67ae85; sd.mid[2] = 0x3c6ef372; sd.mid[3] = 0xa54ff53a;
    sd.mid[4] = 0x510e527f; sd.mid[5] = 0x9b05688c; sd.mid[6] = 0x1f83d9ab; sd.mid[7] = 0x5be0cd19;
    d[b] = sd;
  }
}

// the hash run's records (blob b = node u0 + b) into the listed node records
__global__ __launch_bounds__(256) void k_tree_refs(TreeArgs a, uint64_t u0, uint32_t n,
                                                   const ChunkRec* hashed, const Counters* hctr) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && (hctr->error || hctr->overflow))
    tree_error(a, 512 | (hctr->error << 16));
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < n; b += gridDim.x * blockDim.x) {
    const TreeNodeMeta m = a.meta[u0 + b];
    TreeNode t;
    t.blob_off = m.blob_off;
    t.blob_len = m.blob_len;
    t.stream = m.stream;
    t.height = a.h;
    t.reserved = 0;
    for (int k = 0; k < 32; ++k) t.ref[k] = hashed[b].ref[k];
    if (hashed[b].len != m.blob_len) tree_error(a, 1024);
    a.nodes[m.out_idx] = t;
  }
}

// Root and node count per stream: a stream's last listed node is its Root
__global__ __launch_bounds__(256) void k_tree_roots(TreeArgs a) {
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < a.ns; s += gridDim.x * blockDim.x) {
    uint64_t b0 = 0, b1 = 0;
    if (a.nn) {
      b0 = a.shbase[(uint64_t)s * a.H];
      b1 = a.shbase[(uint64_t)(s + 1) * a.H];
    }
    a.ncount[s] = b1 - b0;
    uint32_t* r = reinterpret_cast<uint32_t*>(a.roots + 32ull * s);
    const uint32_t* src = b1 > b0 ? reinterpret_cast<const uint32_t*>(a.nodes[b1 - 1].ref) : nullptr;
    for (int k = 0; k < 8; ++k) r[k] = src ? src[k] : 0u;
  }
}

// ---- launchers ------------------------------------------------------------------------------
hipError_t launch_tree_count(const TreeArgs& a, hipStream_t s, int num_cus) {
  hipError_t e = launch_sum<TvCount>(a, a.ns, a.cstart, s);
  if (e != hipSuccess) return e;
  const uint32_t g = engine_grid(a.M, num_cus);
  hipLaunchKernelGGL(k_tree_rmax, dim3(g), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_tree_kcnt, dim3(g), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_tree_layout(TreeArgs a, hipStream_t s, int num_cus) {
  hipError_t e;
  for (a.h = 0; a.h < a.H; ++a.h) {
    if ((e = launch_sum<TvCloses>(a, a.M, a.tmp, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_tree_compact, dim3(engine_grid(a.M, num_cus)), dim3(256), 0, s, a);
  }
  a.h = 0;
  e = launch_sum<TvStreamHeight>(a, (uint64_t)a.ns * a.H, a.shbase, s);
  if (e != hipSuccess) return e;
  const uint32_t gn = engine_grid(a.nn, num_cus);
  hipLaunchKernelGGL(k_tree_meta, dim3(gn), dim3(256), 0, s, a);
  if ((e = launch_sum<TvLeafEntry>(a, a.M, a.pc, s)) != hipSuccess) return e;
  if ((e = launch_sum<TvNodeEntry>(a, a.nn, a.pn, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_tree_len, dim3(gn), dim3(256), 0, s, a);
  if ((e = launch_sum<TvArena>(a, a.nn, a.aoff, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_tree_place, dim3(gn), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_tree_emit(const TreeArgs& a, uint64_t children, hipStream_t s, int num_cus) {
  const uint32_t g = engine_grid(children, num_cus);
  if (a.h == 0) hipLaunchKernelGGL(k_tree_emit_leaves, dim3(g), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_tree_emit_nodes, dim3(g), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_tree_descs(const TreeArgs& a, uint64_t u0, uint32_t n, StreamDesc* d,
                             hipStream_t s, int num_cus) {
  hipLaunchKernelGGL(k_tree_descs, dim3(engine_grid(n, num_cus)), dim3(256), 0, s, a, u0, n, d);
  return hipGetLastError();
}

hipError_t launch_tree_refs(const TreeArgs& a, uint64_t u0, uint32_t n, const ChunkRec* hashed,
                            const Counters* hctr, hipStream_t s, int num_cus) {
  hipLaunchKernelGGL(k_tree_refs, dim3(engine_grid(n, num_cus)), dim3(256), 0, s, a, u0, n, hashed,
                     hctr);
  return hipGetLastError();
}

hipError_t launch_tree_roots(const TreeArgs& a, hipStream_t s, int num_cus) {
  hipLaunchKernelGGL(k_tree_roots, dim3(engine_grid(a.ns, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}
