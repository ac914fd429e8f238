"""Python binding of libbsgpu (include/bsgpu.h) via ctypes.

This is plumbing for tests and bench.py; it carries no compute of its own. Every function
runs on the HIP path and raises if the shared library is missing or a call fails — there is no
CPU fallback anywhere in bs_amd.

Reference surface mirrored: split.NewWriter / Write / Close / Root options Bits, MinSize,
Fanout (/root/reference/split/split.go:44-165) and bs.Blob.Ref (/root/reference/bs.go:24-26).
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BSG_LIB_PATH") or os.path.join(_HERE, "libbsgpu.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "bsgpu.h")

BSG_OK = 0
READ_SLACK = 256  # BSG_READ_SLACK: readable bytes required after the last stream
ERRORS = {-22: "EINVAL", -12: "ENOMEM", -5: "EDEVICE", -71: "ESTATE", -19: "ENODEV",
          -2: "ENOTFOUND", -74: "ECORRUPT", -1001: "EIO"}


class BsgError(RuntimeError):
    def __init__(self, code: int, what: str = "", info: dict | None = None):
        self.code = code
        self.info = info  # Engine.restore: the bsg_restore_info of the failed call
        super().__init__(f"{what}: bsgpu error {code} ({ERRORS.get(code, '?')})")


class Params(ctypes.Structure):
    _fields_ = [("split_bits", ctypes.c_uint32), ("min_size", ctypes.c_uint32),
                ("fanout", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class StreamStats(ctypes.Structure):
    """bsg_stream_stats (include/bsgpu.h): where a stream's host-to-device time went."""
    _fields_ = [("host_bytes", ctypes.c_uint64), ("host_copy_ns", ctypes.c_uint64),
                ("stage_wait_ns", ctypes.c_uint64), ("h2d_bytes", ctypes.c_uint64),
                ("h2d_copies", ctypes.c_uint64), ("h2d_busy_ns", ctypes.c_uint64),
                ("h2d_span_ns", ctypes.c_uint64), ("copy_bytes_node", ctypes.c_uint64 * 4),
                ("last_tile_ns", ctypes.c_uint64), ("tail_ns", ctypes.c_uint64),
                ("gpu_node", ctypes.c_int32), ("stage_nodes", ctypes.c_uint32),
                ("src_nodes", ctypes.c_uint32), ("copy_nt", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        def gbs(b, ns):
            return round(b / ns, 2) if ns else None  # bytes per ns = GB/s

        def nodes(mask):
            return [k for k in range(32) if mask >> k & 1]
        return {"host_copy_ms": round(self.host_copy_ns / 1e6, 3),
                "host_copy_gbs": gbs(self.host_bytes, self.host_copy_ns),
                "stage_wait_ms": round(self.stage_wait_ns / 1e6, 3),
                "h2d_busy_ms": round(self.h2d_busy_ns / 1e6, 3),
                "h2d_busy_gbs": gbs(self.h2d_bytes, self.h2d_busy_ns),
                "h2d_span_ms": round(self.h2d_span_ns / 1e6, 3),
                "h2d_span_gbs": gbs(self.h2d_bytes, self.h2d_span_ns),
                "h2d_copies": int(self.h2d_copies),
                "last_tile_ms": round(self.last_tile_ns / 1e6, 3),
                "tail_after_h2d_ms": round(self.tail_ns / 1e6, 3),
                "copy_mib_by_node": [int(b) >> 20 for b in self.copy_bytes_node],
                "gpu_node": int(self.gpu_node), "stage_nodes": nodes(self.stage_nodes),
                "src_nodes": nodes(self.src_nodes), "copy_nt": int(self.copy_nt)}


CHUNK_DTYPE = np.dtype(
    [("offset", "<u8"), ("len", "<u8"), ("level", "<u4"), ("stream", "<u4"), ("ref", "u1", (32,))]
)
assert CHUNK_DTYPE.itemsize == 56

# bsg_tree_node: one split.Node blob of a stream's tree (Engine.trees)
TREE_NODE_DTYPE = np.dtype(
    [("blob_off", "<u8"), ("blob_len", "<u4"), ("stream", "<u4"), ("height", "<u4"),
     ("reserved", "<u4"), ("ref", "u1", (32,))]
)
assert TREE_NODE_DTYPE.itemsize == 56

# bsg_pool_blob: one blob of the pool that Engine.restore reads (pool[off : off + len], named ref)
POOL_BLOB_DTYPE = np.dtype([("off", "<u8"), ("len", "<u8"), ("ref", "u1", (32,))])
assert POOL_BLOB_DTYPE.itemsize == 48
RESTORE_VERIFY = 1     # BSG_RESTORE_VERIFY
RESTORE_TILE = 32768   # kRestoreTile: output bytes of one stream per scatter workgroup
NONE64 = (1 << 64) - 1


class RestoreInfo(ctypes.Structure):
    """bsg_restore_info (include/bsgpu.h)."""
    _fields_ = [("bad_record", ctypes.c_uint64), ("bad_blob", ctypes.c_uint64),
                ("bytes", ctypes.c_uint64), ("verified", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {"bad_record": int(self.bad_record), "bad_blob": int(self.bad_blob),
                "bytes": int(self.bytes), "verified": int(self.verified)}


assert ctypes.sizeof(RestoreInfo) == 32
WALK_MAX_DEPTH = 64    # kWalkMaxDepth: a node deeper than this (Root = 0) is refused


class WalkInfo(ctypes.Structure):
    """bsg_walk_info (include/bsgpu.h)."""
    _fields_ = [("bad_stream", ctypes.c_uint64), ("nrecs", ctypes.c_uint64),
                ("nnodes", ctypes.c_uint64), ("bytes", ctypes.c_uint64),
                ("depth", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {"bad_stream": int(self.bad_stream), "nrecs": int(self.nrecs),
                "nnodes": int(self.nnodes), "bytes": int(self.bytes), "depth": int(self.depth)}


assert ctypes.sizeof(WalkInfo) == 40
GC_MISSING_LEAVES = 1  # BSG_GC_MISSING_LEAVES (gc_mark)
GC_ALIGN16 = 1         # BSG_GC_ALIGN16 (copy_gc, gc_compact)


class GcInfo(ctypes.Structure):
    """bsg_gc_info (include/bsgpu.h)."""
    _fields_ = [("bad_root", ctypes.c_uint64), ("bad_blob", ctypes.c_uint64),
                ("nlive", ctypes.c_uint64), ("live_bytes", ctypes.c_uint64),
                ("ndead", ctypes.c_uint64), ("dead_bytes", ctypes.c_uint64),
                ("nnodes", ctypes.c_uint64), ("missing_leaves", ctypes.c_uint64),
                ("depth", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


assert ctypes.sizeof(GcInfo) == 72
POOL_CHUNKS = 1        # BSG_POOL_CHUNKS (Engine.pool_put)
POOL_NODES = 2         # BSG_POOL_NODES


class POOL_PUT_INFO(ctypes.Structure):
    """bsg_pool_put_info (include/bsgpu.h)."""
    _fields_ = [(k, ctypes.c_uint64) for k in
                ("items", "added", "added_bytes", "known", "repeats", "first_blob", "need_bytes",
                 "need_blobs")]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class PoolStats(ctypes.Structure):
    """bsg_pool_stats (include/bsgpu.h)."""
    _fields_ = [(k, ctypes.c_uint64) for k in
                ("nblobs", "bytes", "cap_blobs", "cap_bytes", "pool_bytes")]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert ctypes.sizeof(POOL_PUT_INFO) == 64 and ctypes.sizeof(PoolStats) == 40


class PoolCollectInfo(ctypes.Structure):
    """bsg_pool_collect_info (include/bsgpu.h)."""
    _fields_ = [("gc", GcInfo), ("need_bytes", ctypes.c_uint64), ("need_blobs", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {"gc": self.gc.as_dict(), "need_bytes": int(self.need_bytes),
                "need_blobs": int(self.need_blobs)}


assert ctypes.sizeof(PoolCollectInfo) == 88
MERGE_ALL = 2          # BSG_MERGE_ALL (Engine.pool_merge)
MERGE_VERIFY = 4       # BSG_MERGE_VERIFY (Engine.pool_merge, Engine.pool_sync)


class PoolMergeInfo(ctypes.Structure):
    """bsg_pool_merge_info (include/bsgpu.h)."""
    _fields_ = [("gc", GcInfo)] + [(k, ctypes.c_uint64) for k in
                                   ("selected", "added", "added_bytes", "known", "first_blob",
                                    "need_bytes", "need_blobs", "bad_blob", "verified")]

    def as_dict(self) -> dict:
        d = {k: int(getattr(self, k)) for k, _ in self._fields_[1:]}
        d["gc"] = self.gc.as_dict()
        return d


assert ctypes.sizeof(PoolMergeInfo) == 144
GET_VERIFY = 1         # BSG_GET_VERIFY (Pool.get)


class PoolGetInfo(ctypes.Structure):
    """bsg_pool_get_info (include/bsgpu.h)."""
    _fields_ = [(k, ctypes.c_uint64) for k in
                ("found", "missing", "bytes", "need_bytes", "bad_blob", "verified")]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


assert ctypes.sizeof(PoolGetInfo) == 48
READ_VERIFY = 1        # BSG_READ_VERIFY (Engine.read, Pool.read)
READ_RANGE_DTYPE = np.dtype([("root", "u1", (32,)), ("offset", "<u8"), ("len", "<u8")])
assert READ_RANGE_DTYPE.itemsize == 48


class ReadInfo(ctypes.Structure):
    """bsg_read_info (include/bsgpu.h)."""
    _fields_ = [("bad_range", ctypes.c_uint64), ("bad_blob", ctypes.c_uint64),
                ("nnodes", ctypes.c_uint64), ("nleaves", ctypes.c_uint64),
                ("bytes", ctypes.c_uint64), ("verified", ctypes.c_uint64),
                ("depth", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


assert ctypes.sizeof(ReadInfo) == 56


def read_ranges(ranges) -> np.ndarray:
    """A READ_RANGE_DTYPE array from one, or from (root, offset, len) triples."""
    if isinstance(ranges, np.ndarray) and ranges.dtype == READ_RANGE_DTYPE:
        return np.ascontiguousarray(ranges)
    out = np.zeros(len(ranges), dtype=READ_RANGE_DTYPE)
    for q, (root, offset, n) in enumerate(ranges):
        out[q]["root"] = np.frombuffer(bytes(root), dtype=np.uint8)
        out[q]["offset"], out[q]["len"] = offset, n
    return out

_lib = None


def exported_symbols_from_header(path: str = HEADER_PATH) -> list[str]:
    """Every function name declared in include/bsgpu.h."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(bsg_[a-z0-9_]+)\s*\(", text)))


def lib() -> ctypes.CDLL:
    """Load libbsgpu.so (built by `python -m bs_amd.build`). Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not built: run `python -m bs_amd.build` "
                           "(the HIP path is the only path; there is no CPU fallback)")
    L = ctypes.CDLL(LIB_PATH)
    vp, u8p, u32p, u64p = (ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8),
                           ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64))
    sig = {
        "bsg_errstr": (ctypes.c_char_p, [ctypes.c_int]),
        "bsg_params_default": (Params, []),
        "bsg_default_table": (None, [u32p]),
        "bsg_device_count": (ctypes.c_int, []),
        "bsg_init": (ctypes.c_int, [ctypes.c_int]),
        "bsg_open": (vp, [ctypes.c_int, ctypes.POINTER(Params), u32p, ctypes.POINTER(ctypes.c_int)]),
        "bsg_write": (ctypes.c_int, [vp, vp, ctypes.c_size_t]),
        "bsg_close": (ctypes.c_int, [vp]),
        "bsg_close_begin": (ctypes.c_int, [vp]),
        "bsg_close_step": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_size_t)]),
        "bsg_pending": (ctypes.c_size_t, [vp]),
        "bsg_drain": (ctypes.c_size_t, [vp, vp, ctypes.c_size_t]),
        "bsg_set_tile": (ctypes.c_int, [vp, ctypes.c_size_t]),
        "bsg_set_carry_cap": (ctypes.c_int, [vp, ctypes.c_size_t]),
        "bsg_write_window": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_void_p),
                                            ctypes.POINTER(ctypes.c_size_t)]),
        "bsg_write_commit": (ctypes.c_int, [vp, ctypes.c_size_t]),
        "bsg_host_register": (ctypes.c_int, [vp, ctypes.c_size_t]),
        "bsg_host_unregister": (ctypes.c_int, [vp]),
        "bsg_write_pinned": (ctypes.c_int, [vp, vp, ctypes.c_size_t]),
        "bsg_free": (None, [vp]),
        "bsg_reset": (ctypes.c_int, [vp]),
        "bsg_engine_create": (vp, [ctypes.c_int, u32p, ctypes.POINTER(ctypes.c_int)]),
        "bsg_engine_destroy": (None, [vp]),
        "bsg_engine_run": (ctypes.c_int, [vp, vp, u64p, u64p, ctypes.c_uint32,
                                          ctypes.POINTER(Params)]),
        "bsg_engine_hash": (ctypes.c_int, [vp, vp, u64p, u64p, ctypes.c_uint32]),
        "bsg_engine_finish": (ctypes.c_int, [vp, u64p]),
        "bsg_engine_chunks_device": (vp, [vp]),
        "bsg_engine_copy_chunks": (ctypes.c_int, [vp, vp, ctypes.c_uint64]),
        "bsg_engine_copy_counts": (ctypes.c_int, [vp, u64p, ctypes.c_uint32]),
        "bsg_engine_stream": (vp, [vp]),
        "bsg_engine_trees": (ctypes.c_int, [vp, u64p, u64p]),
        "bsg_engine_copy_roots": (ctypes.c_int, [vp, vp, u64p, ctypes.c_uint32]),
        "bsg_engine_copy_tree_nodes": (ctypes.c_int, [vp, vp, ctypes.c_uint64, vp,
                                                      ctypes.c_uint64]),
        "bsg_engine_tree_nodes_device": (vp, [vp]),
        "bsg_engine_tree_arena_device": (vp, [vp]),
        "bsg_engine_roots_device": (vp, [vp]),
        "bsg_engine_trees_ms_debug": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        "bsg_refset_new": (vp, [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
        "bsg_refset_free": (None, [vp]),
        "bsg_refset_count": (ctypes.c_uint64, [vp]),
        "bsg_refset_add": (ctypes.c_int, [vp, vp, ctypes.c_uint64, vp]),
        "bsg_engine_dedup": (ctypes.c_int, [vp, vp, u64p, u64p]),
        "bsg_engine_copy_dedup": (ctypes.c_int, [vp, vp, ctypes.c_uint64, vp, vp,
                                                 ctypes.c_uint64]),
        "bsg_engine_dedup_first_device": (vp, [vp]),
        "bsg_engine_dedup_uniq_device": (vp, [vp]),
        "bsg_engine_dedup_pack_off_device": (vp, [vp]),
        "bsg_engine_pack_unique": (ctypes.c_int, [vp, vp, ctypes.c_uint64]),
        "bsg_engine_dedup_ms_debug": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        "bsg_engine_restore": (ctypes.c_int, [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp,
                                              ctypes.c_uint64, vp, ctypes.c_uint64, u64p, u64p,
                                              ctypes.c_uint32, ctypes.c_int,
                                              ctypes.POINTER(RestoreInfo)]),
        "bsg_engine_restore_ms_debug": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        "bsg_engine_walk": (ctypes.c_int, [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp,
                                           ctypes.c_uint32, ctypes.c_int, vp,
                                           ctypes.POINTER(WalkInfo)]),
        "bsg_engine_copy_walk": (ctypes.c_int, [vp, vp, ctypes.c_uint64, vp, vp,
                                                ctypes.c_uint32]),
        "bsg_engine_walk_records_device": (vp, [vp]),
        "bsg_engine_restore_walk": (ctypes.c_int, [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64,
                                                   vp, ctypes.c_uint64, u64p, ctypes.c_uint32,
                                                   ctypes.c_int, ctypes.POINTER(RestoreInfo)]),
        "bsg_engine_walk_ms_debug": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        "bsg_engine_gc_mark": (ctypes.c_int, [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp,
                                              ctypes.c_uint64, ctypes.c_int, vp,
                                              ctypes.POINTER(GcInfo)]),
        "bsg_engine_copy_gc": (ctypes.c_int, [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64,
                                              ctypes.c_int]),
        "bsg_engine_gc_live_device": (vp, [vp]),
        "bsg_engine_gc_compact": (ctypes.c_int, [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64,
                                                 ctypes.c_int, u64p]),
        "bsg_engine_gc_ms_debug": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        "bsg_pool_new": (vp, [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64,
                              ctypes.POINTER(ctypes.c_int)]),
        "bsg_pool_free": (None, [vp]),
        "bsg_pool_stat": (ctypes.c_int, [vp, ctypes.POINTER(PoolStats)]),
        "bsg_pool_bytes_device": (vp, [vp]),
        "bsg_pool_table_device": (vp, [vp]),
        "bsg_pool_copy_table": (ctypes.c_int, [vp, vp, ctypes.c_uint64, ctypes.c_uint64]),
        "bsg_engine_pool_put": (ctypes.c_int, [vp, vp, ctypes.c_int,
                                               ctypes.POINTER(POOL_PUT_INFO)]),
        "bsg_pool_copy_where": (ctypes.c_int, [vp, vp, ctypes.c_uint64]),
        "bsg_pool_where_device": (vp, [vp]),
        "bsg_pool_put_ms_debug": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        "bsg_pool_collect": (ctypes.c_int, [vp, vp, vp, vp, ctypes.c_uint64, ctypes.c_int, vp,
                                            ctypes.POINTER(PoolCollectInfo)]),
        "bsg_pool_copy_remap": (ctypes.c_int, [vp, vp, ctypes.c_uint64]),
        "bsg_pool_remap_device": (vp, [vp]),
        "bsg_pool_reset": (ctypes.c_int, [vp]),
        "bsg_pool_walk": (ctypes.c_int, [vp, vp, vp, ctypes.c_uint32, ctypes.c_int, vp,
                                         ctypes.POINTER(WalkInfo)]),
        "bsg_pool_restore_walk": (ctypes.c_int, [vp, vp, vp, ctypes.c_uint64, u64p,
                                                 ctypes.c_uint32, ctypes.c_int,
                                                 ctypes.POINTER(RestoreInfo)]),
        "bsg_engine_read": (ctypes.c_int, [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp,
                                           ctypes.c_uint32, vp, ctypes.c_uint64, vp, ctypes.c_int,
                                           vp, vp, ctypes.POINTER(ReadInfo)]),
        "bsg_pool_read": (ctypes.c_int, [vp, vp, vp, ctypes.c_uint32, vp, ctypes.c_uint64, vp,
                                         ctypes.c_int, vp, vp, ctypes.POINTER(ReadInfo)]),
        "bsg_pool_kill_debug": (ctypes.c_int, [vp]),
        "bsg_engine_read_ms_debug": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        "bsg_pool_collect_ms_debug": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        "bsg_pool_merge": (ctypes.c_int, [vp, vp, vp, vp, ctypes.c_uint64, ctypes.c_int, vp,
                                          ctypes.POINTER(PoolMergeInfo)]),
        "bsg_pool_sync": (ctypes.c_int, [vp, vp, vp, ctypes.c_int, ctypes.POINTER(PoolMergeInfo)]),
        "bsg_pool_merge_ms_debug": (ctypes.c_int, [vp, ctypes.c_int,
                                                   ctypes.POINTER(ctypes.c_float)]),
        "bsg_pool_put_blobs": (ctypes.c_int, [vp, vp, vp, u64p, u64p, ctypes.c_uint64,
                                              ctypes.c_int, vp, ctypes.POINTER(POOL_PUT_INFO)]),
        "bsg_pool_get": (ctypes.c_int, [vp, vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64,
                                        ctypes.c_int, vp, vp, ctypes.POINTER(PoolGetInfo)]),
        "bsg_pool_blobs_ms_debug": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        "bsg_engine_pack_mode_debug": (ctypes.c_int, [vp, ctypes.c_int]),
        "bsg_engine_d2d_ms_debug": (ctypes.c_int, [vp, vp, vp, ctypes.c_uint64,
                                                   ctypes.POINTER(ctypes.c_float)]),
        "bsg_engine_candidates": (ctypes.c_uint64, [vp]),
        "bsg_engine_profile": (ctypes.c_int, [vp, ctypes.c_int]),
        "bsg_engine_diag": (ctypes.c_int, [vp, u64p]),
        "bsg_engine_timeline": (ctypes.c_int, [vp, u64p]),
        "bsg_engine_tiers_debug": (ctypes.c_int, [vp, u64p]),
        "bsg_engine_early_min_debug": (ctypes.c_int, [vp, ctypes.c_uint64]),
        "bsg_engine_host_tail": (ctypes.c_int, [vp, u64p]),
        "bsg_engine_host_tail_debug": (ctypes.c_int, [vp, ctypes.c_uint64, ctypes.c_uint32,
                                                      ctypes.c_int, ctypes.c_uint64]),
        "bsg_host_sha256_debug": (ctypes.c_int, [vp, ctypes.c_uint64, ctypes.c_int, vp]),
        "bsg_engine_early_picks_debug": (ctypes.c_int, [vp, u64p]),
        "bsg_engine_rescan_debug": (ctypes.c_uint64, [vp]),
        "bsg_engine_regions_debug": (ctypes.c_int, [vp, vp, ctypes.c_uint64]),
        "bsg_engine_stage_ms": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        "bsg_split_hash_batch": (ctypes.c_int, [ctypes.c_int, vp, u64p, u64p, ctypes.c_uint32,
                                                ctypes.POINTER(Params), u32p, vp,
                                                ctypes.c_uint64, u64p, u64p]),
        "bsg_sha256_batch": (ctypes.c_int, [ctypes.c_int, vp, u64p, u64p, ctypes.c_uint32, vp]),
        "bsg_hasher_new": (vp, [ctypes.c_int]),
        "bsg_hasher_sum": (ctypes.c_int, [vp, vp, u64p, u64p, ctypes.c_uint32, vp]),
        "bsg_hasher_sum_ptrs": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_void_p), u64p,
                                               ctypes.c_uint32, vp]),
        "bsg_hasher_free": (None, [vp]),
        "bsg_hasher_pinned_bytes": (ctypes.c_size_t, [vp]),
        "bsg_fill_splitmix": (ctypes.c_int, [ctypes.c_int, vp, ctypes.c_uint64, ctypes.c_uint64,
                                             vp]),
        "bsg_device_malloc": (vp, [ctypes.c_int, ctypes.c_size_t]),
        "bsg_device_free": (ctypes.c_int, [ctypes.c_int, vp]),
        "bsg_memcpy": (ctypes.c_int, [ctypes.c_int, vp, vp, ctypes.c_size_t, ctypes.c_int]),
        "bsg_device_synchronize": (ctypes.c_int, [ctypes.c_int]),
        "bsg_memstore_new": (vp, [ctypes.c_int]),
        "bsg_filestore_new": (vp, [ctypes.c_char_p, ctypes.c_int]),
        "bsg_store_free": (None, [vp]),
        "bsg_store_count": (ctypes.c_size_t, [vp]),
        "bsg_filestore_set_write_behind": (ctypes.c_int, [vp, ctypes.c_uint64]),
        "bsg_store_held_bytes": (ctypes.c_size_t, [vp]),
        "bsg_store_get": (ctypes.c_int, [vp, vp, vp, ctypes.c_size_t,
                                         ctypes.POINTER(ctypes.c_size_t)]),
        "bsg_store_put": (ctypes.c_int, [vp, vp, ctypes.c_size_t, vp,
                                         ctypes.POINTER(ctypes.c_int)]),
        "bsg_store_list": (ctypes.c_size_t, [vp, vp, ctypes.c_size_t]),
        "bsg_store_put_ref": (ctypes.c_int, [vp, vp, vp, ctypes.c_size_t,
                                             ctypes.POINTER(ctypes.c_int)]),
        "bsg_store_list_from": (ctypes.c_size_t, [vp, vp, vp, ctypes.c_size_t]),
        "bsg_store_delete": (ctypes.c_int, [vp, vp]),
        "bsg_split_protect": (ctypes.c_int, [vp, vp, vp, vp, ctypes.c_size_t,
                                             ctypes.POINTER(ctypes.c_size_t)]),
        "bsg_writer_new": (vp, [ctypes.c_int, vp, ctypes.POINTER(Params), ctypes.c_size_t,
                                ctypes.POINTER(ctypes.c_int)]),
        "bsg_writer_write": (ctypes.c_int, [vp, vp, ctypes.c_size_t]),
        "bsg_writer_close": (ctypes.c_int, [vp]),
        "bsg_writer_root": (ctypes.c_int, [vp, vp]),
        "bsg_writer_timings": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_double)]),
        "bsg_stream_stats_get": (ctypes.c_int, [vp, ctypes.POINTER(StreamStats)]),
        "bsg_writer_free": (None, [vp]),
        "bsg_reader_new": (vp, [vp, vp, ctypes.POINTER(ctypes.c_int)]),
        "bsg_reader_open": (vp, [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
        "bsg_reader_read": (ctypes.c_int64, [vp, vp, ctypes.c_size_t]),
        "bsg_reader_seek": (ctypes.c_int64, [vp, ctypes.c_int64, ctypes.c_int]),
        "bsg_reader_size": (ctypes.c_uint64, [vp]),
        "bsg_reader_stats": (ctypes.c_int, [vp, u64p]),
        "bsg_debug_set": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64]),
        "bsg_debug_get": (ctypes.c_int64, [ctypes.c_int]),
        "bsg_set_stream_base": (ctypes.c_int, [vp, ctypes.c_uint64]),
        "bsg_writer_set_stream_base": (ctypes.c_int, [vp, ctypes.c_uint64]),
        "bsg_reader_free": (None, [vp]),
    }
    partial = os.environ.get("BSG_LIB_PARTIAL") == "1"  # A/B of older builds (tools/)
    for name, (res, args) in sig.items():
        if partial and not hasattr(L, name):
            continue
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def _check(rc: int, what: str) -> None:
    if rc != BSG_OK:
        raise BsgError(rc, what)


def _as_u8(data) -> np.ndarray:
    """Zero-copy uint8 view of bytes / bytearray / memoryview / ndarray."""
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data.reshape(-1).view(np.uint8))
    return np.frombuffer(data, dtype=np.uint8)


def _u64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


def _p(a: np.ndarray, ct):
    return a.ctypes.data_as(ctypes.POINTER(ct))


# bsg_debug_set
(KNOB_SEQ_WAIT, KNOB_LONG_MODE, KNOB_VERIFY_WINDOW, KNOB_EARLY, KNOB_POLL, KNOB_COPY_NT,
 KNOB_LIGHT_BYTES, KNOB_HOST_TAIL) = range(1, 9)


def debug_get(knob: int) -> int:
    return int(lib().bsg_debug_get(knob))


def debug_set(knob: int, value: int) -> None:
    """bsg_debug_set: a process-wide test knob (no environment changes at run time)."""
    _check(lib().bsg_debug_set(knob, value), "bsg_debug_set")


@contextlib.contextmanager
def debug_knob(knob: int, value: int):
    old = debug_get(knob)
    debug_set(knob, value)
    try:
        yield
    finally:
        debug_set(knob, old)


def device_count() -> int:
    return lib().bsg_device_count()


def init(device: int = 0) -> None:
    """bsg_init: the process's one-time device / kernel / thread start-up, done up front."""
    _check(lib().bsg_init(device), "bsg_init")


def default_table() -> np.ndarray:
    t = np.zeros(256, dtype=np.uint32)
    lib().bsg_default_table(_p(t, ctypes.c_uint32))
    return t


def params(bits: int = 16, min_size: int = 1024, fanout: int = 8) -> Params:
    """split.NewWriter defaults (split/split.go:48,88-89); pass Bits/MinSize/Fanout overrides."""
    return Params(bits, min_size, fanout, 0)


def _table_arg(table):
    if table is None:
        return None, None
    t = np.ascontiguousarray(np.asarray(table, dtype=np.uint32))
    assert t.shape == (256,)
    return t, _p(t, ctypes.c_uint32)


def split_hash_batch(streams: list[bytes] | list[np.ndarray], bits: int = 16,
                     min_size: int = 1024, table=None, device: int = 0):
    """Split + hash host-resident streams on the GPU. Returns (chunks, counts)."""
    arrs = [np.frombuffer(bytes(s), dtype=np.uint8) if not isinstance(s, np.ndarray)
            else np.ascontiguousarray(s, dtype=np.uint8) for s in streams]
    lens = _u64([len(a) for a in arrs])
    off = _u64(np.concatenate([[0], np.cumsum(lens)[:-1]]) if len(arrs) else [])
    base = np.concatenate(arrs) if arrs else np.zeros(1, np.uint8)
    if base.size == 0:
        base = np.zeros(1, np.uint8)
    cap = int(sum(int(l) // (min_size or 64) + 2 for l in lens)) + 1
    out = np.zeros(cap, dtype=CHUNK_DTYPE)
    counts = np.zeros(max(len(arrs), 1), dtype=np.uint64)
    n = ctypes.c_uint64(0)
    p = params(bits, min_size)
    _t, tp = _table_arg(table)
    rc = lib().bsg_split_hash_batch(device, base.ctypes.data, _p(off, ctypes.c_uint64),
                                    _p(lens, ctypes.c_uint64), len(arrs), ctypes.byref(p), tp,
                                    out.ctypes.data, cap, _p(counts, ctypes.c_uint64),
                                    ctypes.byref(n))
    _check(rc, "bsg_split_hash_batch")
    return out[: n.value], counts[: len(arrs)]


def _refs_list(refs: np.ndarray, n: int) -> list[bytes]:
    return [refs[32 * i:32 * i + 32].tobytes() for i in range(n)]


def _base_ptr(base) -> int:
    """A base address: a host array's data pointer, or an int (a host or device address)."""
    return int(base.ctypes.data) if isinstance(base, np.ndarray) else int(base)


def split_hash_batch_at(base: np.ndarray, off, lens, bits: int = 16, min_size: int = 1024,
                        table=None, device: int = 0):
    """bsg_split_hash_batch over the caller's layout: stream i is base[off[i] : off[i] + lens[i]]
    of one host array (any order, gaps, overlaps; no alignment). Returns (chunks, counts)."""
    assert isinstance(base, np.ndarray) and base.dtype == np.uint8 and base.flags.c_contiguous
    off, lens = _u64(off), _u64(lens)
    assert len(off) == len(lens)
    ns = len(off)
    cap = int(sum(int(l) // (min_size or 64) + 2 for l in lens)) + 1
    out = np.zeros(cap, dtype=CHUNK_DTYPE)
    counts = np.zeros(max(ns, 1), dtype=np.uint64)
    n = ctypes.c_uint64(0)
    p = params(bits, min_size)
    _t, tp = _table_arg(table)
    rc = lib().bsg_split_hash_batch(device, base.ctypes.data, _p(off, ctypes.c_uint64),
                                    _p(lens, ctypes.c_uint64), ns, ctypes.byref(p), tp,
                                    out.ctypes.data, cap, _p(counts, ctypes.c_uint64),
                                    ctypes.byref(n))
    _check(rc, "bsg_split_hash_batch")
    return out[: n.value], counts[:ns]


def sha256_batch_at(base, off, lens, device: int = 0) -> list[bytes]:
    """bsg_sha256_batch over the caller's layout: blob i is base[off[i] .. off[i] + lens[i]),
    base a host uint8 array or an address (host or device memory)."""
    off, lens = _u64(off), _u64(lens)
    assert len(off) == len(lens)
    refs = np.zeros(32 * max(len(off), 1), dtype=np.uint8)
    rc = lib().bsg_sha256_batch(device, _base_ptr(base), _p(off, ctypes.c_uint64),
                                _p(lens, ctypes.c_uint64), len(off), refs.ctypes.data)
    _check(rc, "bsg_sha256_batch")
    return _refs_list(refs, len(off))


def sha256_batch(blobs: list[bytes], device: int = 0) -> list[bytes]:
    arrs = [np.frombuffer(bytes(b), dtype=np.uint8) for b in blobs]
    lens = _u64([len(a) for a in arrs])
    off = _u64(np.concatenate([[0], np.cumsum(lens)[:-1]]) if arrs else [])
    base = np.concatenate(arrs) if arrs else np.zeros(1, np.uint8)
    if base.size == 0:
        base = np.zeros(1, np.uint8)
    refs = np.zeros(32 * max(len(arrs), 1), dtype=np.uint8)
    rc = lib().bsg_sha256_batch(device, base.ctypes.data, _p(off, ctypes.c_uint64),
                                _p(lens, ctypes.c_uint64), len(arrs), refs.ctypes.data)
    _check(rc, "bsg_sha256_batch")
    return [refs[32 * i:32 * i + 32].tobytes() for i in range(len(arrs))]


class Hasher:
    """bsg_hasher: persistent batched SHA-256 (Blob.Ref of many blobs)."""

    def __init__(self, device: int = 0):
        self.h = lib().bsg_hasher_new(device)
        if not self.h:
            raise BsgError(-19, "bsg_hasher_new")

    def sum_ptrs(self, blobs: list) -> list[bytes]:
        """Scattered host blobs (bsg_hasher_sum_ptrs): one GPU call, no packing by the caller."""
        keep = [np.frombuffer(bytes(b), dtype=np.uint8) if len(b) else np.zeros(1, np.uint8)
                for b in blobs]
        ptrs = (ctypes.c_void_p * max(len(keep), 1))(*[a.ctypes.data for a in keep])
        lens = _u64([len(b) for b in blobs])
        refs = np.zeros(32 * max(len(blobs), 1), dtype=np.uint8)
        _check(lib().bsg_hasher_sum_ptrs(self.h, ptrs, _p(lens, ctypes.c_uint64), len(blobs),
                                         refs.ctypes.data), "bsg_hasher_sum_ptrs")
        return [refs[32 * i:32 * i + 32].tobytes() for i in range(len(blobs))]

    def sum(self, blobs: list) -> list[bytes]:
        """Blobs packed into one host buffer (bsg_hasher_sum)."""
        arrs = [np.frombuffer(bytes(b), dtype=np.uint8) for b in blobs]
        lens = _u64([len(a) for a in arrs])
        off = _u64(np.concatenate([[0], np.cumsum(lens)[:-1]]) if arrs else [])
        base = np.concatenate(arrs) if arrs and sum(len(a) for a in arrs) else np.zeros(1, np.uint8)
        refs = np.zeros(32 * max(len(arrs), 1), dtype=np.uint8)
        _check(lib().bsg_hasher_sum(self.h, base.ctypes.data, _p(off, ctypes.c_uint64),
                                    _p(lens, ctypes.c_uint64), len(arrs), refs.ctypes.data),
               "bsg_hasher_sum")
        return [refs[32 * i:32 * i + 32].tobytes() for i in range(len(blobs))]

    def sum_at(self, base, off, lens) -> list[bytes]:
        """bsg_hasher_sum over the caller's layout: blob i is base[off[i] .. off[i] + lens[i]),
        base a host uint8 array or an address (host or device memory)."""
        off, lens = _u64(off), _u64(lens)
        assert len(off) == len(lens)
        refs = np.zeros(32 * max(len(off), 1), dtype=np.uint8)
        _check(lib().bsg_hasher_sum(self.h, _base_ptr(base), _p(off, ctypes.c_uint64),
                                    _p(lens, ctypes.c_uint64), len(off), refs.ctypes.data),
               "bsg_hasher_sum")
        return _refs_list(refs, len(off))

    def pinned_bytes(self) -> int:
        """bsg_hasher_pinned_bytes: pinned host memory the hasher holds (diagnostics)."""
        return int(lib().bsg_hasher_pinned_bytes(self.h))

    def free(self):
        if self.h:
            lib().bsg_hasher_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def host_register(ptr: int, n: int) -> None:
    """bsg_host_register: page-lock caller memory for bsg_write_pinned."""
    _check(lib().bsg_host_register(ptr, n), "bsg_host_register")


def host_unregister(ptr: int) -> None:
    _check(lib().bsg_host_unregister(ptr), "bsg_host_unregister")


def fill_splitmix(ptr: int, nbytes: int, seed: int, stream: int | None = None,
                  device: int = 0) -> None:
    _check(lib().bsg_fill_splitmix(device, ptr, nbytes, seed, stream), "bsg_fill_splitmix")


class DeviceBuffer:
    """Raw HIP allocation owned by libbsgpu (torch ships its own HIP runtime, so GPU processes
    here never initialise torch's CUDA/HIP side)."""

    def __init__(self, nbytes: int, device: int = 0):
        self.device, self.nbytes = device, nbytes
        self.ptr = lib().bsg_device_malloc(device, nbytes + READ_SLACK)
        if not self.ptr:
            raise BsgError(-12, "bsg_device_malloc")

    def to_host(self, offset: int = 0, n: int | None = None) -> np.ndarray:
        n = self.nbytes - offset if n is None else n
        out = np.empty(max(n, 1), dtype=np.uint8)
        _check(lib().bsg_memcpy(self.device, out.ctypes.data, self.ptr + offset, n, 1),
               "bsg_memcpy")
        return out[:n]

    def from_host(self, a: np.ndarray, offset: int = 0) -> None:
        a = np.ascontiguousarray(a, dtype=np.uint8)
        _check(lib().bsg_memcpy(self.device, self.ptr + offset, a.ctypes.data, a.nbytes, 0),
               "bsg_memcpy")

    def free(self) -> None:
        if self.ptr:
            lib().bsg_device_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def synchronize(device: int = 0) -> None:
    _check(lib().bsg_device_synchronize(device), "bsg_device_synchronize")


class Engine:
    """Device-resident batch of independent streams (bsg_engine_*)."""

    def __init__(self, device: int = 0, table=None):
        err = ctypes.c_int(0)
        self._t, tp = _table_arg(table)
        self.h = lib().bsg_engine_create(device, tp, ctypes.byref(err))
        if not self.h:
            raise BsgError(err.value, "bsg_engine_create")
        self.nstreams = 0
        self._walk_ns = self._walk_nrecs = 0
        self._gc_nblobs = self._gc_nlive = 0

    def run(self, d_ptr: int, off, lens, bits: int = 16, min_size: int = 1024,
            fanout: int = 8) -> None:
        self._off, self._len = _u64(off), _u64(lens)
        self._p = params(bits, min_size, fanout)
        self.nstreams = len(self._off)
        _check(lib().bsg_engine_run(self.h, d_ptr, _p(self._off, ctypes.c_uint64),
                                    _p(self._len, ctypes.c_uint64), self.nstreams,
                                    ctypes.byref(self._p)), "bsg_engine_run")

    def hash(self, d_ptr: int, off, lens) -> None:
        """bsg_engine_hash: SHA-256 of whole blobs (record i: blob i's ref), no splitting."""
        self._off, self._len = _u64(off), _u64(lens)
        self.nstreams = len(self._off)
        _check(lib().bsg_engine_hash(self.h, d_ptr, _p(self._off, ctypes.c_uint64),
                                     _p(self._len, ctypes.c_uint64), self.nstreams),
               "bsg_engine_hash")

    def finish(self) -> int:
        n = ctypes.c_uint64(0)
        _check(lib().bsg_engine_finish(self.h, ctypes.byref(n)), "bsg_engine_finish")
        self.nchunks = n.value
        return n.value

    def chunks(self) -> np.ndarray:
        out = np.zeros(max(self.nchunks, 1), dtype=CHUNK_DTYPE)
        _check(lib().bsg_engine_copy_chunks(self.h, out.ctypes.data, self.nchunks),
               "bsg_engine_copy_chunks")
        return out[: self.nchunks]

    def counts(self) -> np.ndarray:
        c = np.zeros(max(self.nstreams, 1), dtype=np.uint64)
        _check(lib().bsg_engine_copy_counts(self.h, _p(c, ctypes.c_uint64), self.nstreams),
               "bsg_engine_copy_counts")
        return c[: self.nstreams]

    def trees(self):
        """bsg_engine_trees: split.Writer's tree per stream of the last finished run, built on
        the device. Returns (roots[ns, 32], node_counts[ns], nodes[TREE_NODE_DTYPE], arena[u8]):
        node i's blob is arena[blob_off : blob_off + blob_len], a stream's last node its Root."""
        nn, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(lib().bsg_engine_trees(self.h, ctypes.byref(nn), ctypes.byref(nb)),
               "bsg_engine_trees")
        roots = np.zeros((max(self.nstreams, 1), 32), dtype=np.uint8)
        counts = np.zeros(max(self.nstreams, 1), dtype=np.uint64)
        _check(lib().bsg_engine_copy_roots(self.h, roots.ctypes.data,
                                           _p(counts, ctypes.c_uint64), self.nstreams),
               "bsg_engine_copy_roots")
        nodes = np.zeros(max(nn.value, 1), dtype=TREE_NODE_DTYPE)
        arena = np.zeros(max(nb.value, 1), dtype=np.uint8)
        _check(lib().bsg_engine_copy_tree_nodes(self.h, nodes.ctypes.data, nn.value,
                                                arena.ctypes.data, nb.value),
               "bsg_engine_copy_tree_nodes")
        return (roots[: self.nstreams], counts[: self.nstreams], nodes[: nn.value],
                arena[: nb.value])

    def trees_ms(self) -> dict:
        """The last trees() call's passes in ms (test tooling; needs profile() on)."""
        out = (ctypes.c_float * 4)()
        _check(lib().bsg_engine_trees_ms_debug(self.h, out), "bsg_engine_trees_ms_debug")
        return {"layout": float(out[0]), "emit": float(out[1]), "hash": float(out[2]),
                "total": float(out[3])}

    def dedup(self, refset: "RefSet | None" = None):
        """bsg_engine_dedup: first occurrence per ref over the last finished run's records, on
        the device. Returns (first[n], uniq[nunique], pack_off[nunique + 1]) as uint64 arrays:
        record i is new iff first[i] == i (bit 63, IN_SET, marks a ref `refset` already held).
        With a refset the new refs are in it afterwards. Sets nunique and unique_bytes."""
        nu, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(lib().bsg_engine_dedup(self.h, refset.h if refset is not None else None,
                                      ctypes.byref(nu), ctypes.byref(nb)), "bsg_engine_dedup")
        self.nunique, self.unique_bytes = nu.value, nb.value
        first = np.zeros(max(self.nchunks, 1), dtype=np.uint64)
        uniq = np.zeros(max(nu.value, 1), dtype=np.uint64)
        pack_off = np.zeros(nu.value + 1, dtype=np.uint64)
        _check(lib().bsg_engine_copy_dedup(self.h, first.ctypes.data, self.nchunks,
                                           uniq.ctypes.data, pack_off.ctypes.data, nu.value),
               "bsg_engine_copy_dedup")
        return first[: self.nchunks], uniq[: nu.value], pack_off

    def pack_unique(self, buf: "DeviceBuffer", offset: int = 0, cap: int | None = None) -> None:
        """bsg_engine_pack_unique: the new records' bytes, contiguous, into buf (device memory)
        from `offset` on: buf[offset + pack_off[k] : offset + pack_off[k + 1]] = record uniq[k]."""
        cap = buf.nbytes - offset if cap is None else cap
        _check(lib().bsg_engine_pack_unique(self.h, buf.ptr + offset, cap),
               "bsg_engine_pack_unique")

    def restore(self, pool, blobs, recs, out, out_off, out_len, verify: bool = False,
                pool_bytes: int | None = None, out_cap: int | None = None) -> dict:
        """bsg_engine_restore: the streams that `recs` (CHUNK_DTYPE) describe, written to device
        memory from the pool's blobs (POOL_BLOB_DTYPE): stream s to out + out_off[s]. pool / out:
        a DeviceBuffer or a device address (then pool_bytes / out_cap must be given). Returns the
        call's bsg_restore_info as a dict; raises BsgError (code, info) on any failure."""
        pp = pool.ptr if isinstance(pool, DeviceBuffer) else pool
        op = out.ptr if isinstance(out, DeviceBuffer) else out
        pool_bytes = pool.nbytes + READ_SLACK if pool_bytes is None else pool_bytes
        out_cap = out.nbytes if out_cap is None else out_cap
        blobs = np.ascontiguousarray(blobs, dtype=POOL_BLOB_DTYPE)
        recs = np.ascontiguousarray(recs, dtype=CHUNK_DTYPE)
        oo, ol = _u64(out_off), _u64(out_len)
        assert len(oo) == len(ol)
        info = RestoreInfo()
        rc = lib().bsg_engine_restore(self.h, pp, pool_bytes, blobs.ctypes.data, len(blobs),
                                      recs.ctypes.data, len(recs), op, out_cap,
                                      _p(oo, ctypes.c_uint64), _p(ol, ctypes.c_uint64), len(oo),
                                      RESTORE_VERIFY if verify else 0, ctypes.byref(info))
        if rc != BSG_OK:
            raise BsgError(rc, "bsg_engine_restore", info.as_dict())
        return info.as_dict()

    def restore_ms(self) -> dict:
        """The last restore() call's passes in ms (test tooling; needs profile() on)."""
        out = (ctypes.c_float * 3)()
        _check(lib().bsg_engine_restore_ms_debug(self.h, out), "bsg_engine_restore_ms_debug")
        return {"resolve": float(out[0]), "verify": float(out[1]), "scatter": float(out[2])}

    def walk(self, pool, blobs, roots, pool_bytes: int | None = None, flags: int = 0):
        """bsg_engine_walk: every stream's size and records read out of the split trees under
        `roots` ([ns, 32] uint8, or ns * 32 bytes), whose node and chunk blobs lie in the pool
        (POOL_BLOB_DTYPE; a DeviceBuffer, or a device address with pool_bytes). Returns
        (rc, info, status): the return code, the bsg_walk_info as a dict and the per-stream
        status (int32); a negative rc is returned, not raised."""
        pp = pool.ptr if isinstance(pool, DeviceBuffer) else pool
        pool_bytes = pool.nbytes + READ_SLACK if pool_bytes is None else pool_bytes
        blobs = np.ascontiguousarray(blobs, dtype=POOL_BLOB_DTYPE)
        roots = np.ascontiguousarray(np.frombuffer(roots, dtype=np.uint8)
                                     if isinstance(roots, (bytes, bytearray)) else roots,
                                     dtype=np.uint8).reshape(-1)
        assert len(roots) % 32 == 0
        ns = len(roots) // 32
        status = np.zeros(max(ns, 1), dtype=np.int32)
        info = WalkInfo()
        rc = lib().bsg_engine_walk(self.h, pp, pool_bytes, blobs.ctypes.data, len(blobs),
                                   roots.ctypes.data, ns, flags, status.ctypes.data,
                                   ctypes.byref(info))
        self._walk_ns, self._walk_nrecs = ns, int(info.nrecs)
        return rc, info.as_dict(), status[:ns]

    def copy_walk(self):
        """bsg_engine_copy_walk: (recs[CHUNK_DTYPE], sizes[ns], counts[ns]) of the last
        successful walk(); raises BsgError (ESTATE) without one."""
        ns, n = self._walk_ns, self._walk_nrecs
        recs = np.zeros(max(n, 1), dtype=CHUNK_DTYPE)
        sizes = np.zeros(max(ns, 1), dtype=np.uint64)
        counts = np.zeros(max(ns, 1), dtype=np.uint64)
        _check(lib().bsg_engine_copy_walk(self.h, recs.ctypes.data, n, sizes.ctypes.data,
                                          counts.ctypes.data, ns), "bsg_engine_copy_walk")
        return recs[:n], sizes[:ns], counts[:ns]

    def walk_records_device(self) -> int:
        """bsg_engine_walk_records_device: the records' device address (0 without a walk)."""
        return lib().bsg_engine_walk_records_device(self.h) or 0

    def restore_walk(self, pool, blobs, out, out_off, verify: bool = False,
                     pool_bytes: int | None = None, out_cap: int | None = None):
        """bsg_engine_restore_walk: restore() with the last successful walk's records, read on
        the device, and its sizes as out_len. Returns (rc, info): the return code and the
        bsg_restore_info as a dict; a negative rc is returned, not raised."""
        pp = pool.ptr if isinstance(pool, DeviceBuffer) else pool
        op = out.ptr if isinstance(out, DeviceBuffer) else out
        pool_bytes = pool.nbytes + READ_SLACK if pool_bytes is None else pool_bytes
        out_cap = out.nbytes if out_cap is None else out_cap
        blobs = np.ascontiguousarray(blobs, dtype=POOL_BLOB_DTYPE)
        oo = _u64(out_off)
        info = RestoreInfo()
        rc = lib().bsg_engine_restore_walk(self.h, pp, pool_bytes, blobs.ctypes.data, len(blobs),
                                           op, out_cap, _p(oo, ctypes.c_uint64), len(oo),
                                           RESTORE_VERIFY if verify else 0, ctypes.byref(info))
        return rc, info.as_dict()

    def walk_ms(self) -> dict:
        """The last walk() call's passes in ms (test tooling; needs profile() on)."""
        out = (ctypes.c_float * 3)()
        _check(lib().bsg_engine_walk_ms_debug(self.h, out), "bsg_engine_walk_ms_debug")
        return {"index": float(out[0]), "levels": float(out[1]), "placement": float(out[2])}

    def gc_mark(self, pool, blobs, roots, pool_bytes: int | None = None, flags: int = 0):
        """bsg_engine_gc_mark: which blobs of the pool (POOL_BLOB_DTYPE; a DeviceBuffer, or a
        device address with pool_bytes) the `roots` ([n, 32] uint8, or n * 32 bytes) reach.
        Returns (rc, info, status): the return code, the bsg_gc_info as a dict and the per-Root
        status (int32); a negative rc is returned, not raised."""
        pp = pool.ptr if isinstance(pool, DeviceBuffer) else pool
        pool_bytes = pool.nbytes + READ_SLACK if pool_bytes is None else pool_bytes
        blobs = np.ascontiguousarray(blobs, dtype=POOL_BLOB_DTYPE)
        roots = np.ascontiguousarray(np.frombuffer(roots, dtype=np.uint8)
                                     if isinstance(roots, (bytes, bytearray)) else roots,
                                     dtype=np.uint8).reshape(-1)
        assert len(roots) % 32 == 0
        nr = len(roots) // 32
        status = np.zeros(max(nr, 1), dtype=np.int32)
        info = GcInfo()
        rc = lib().bsg_engine_gc_mark(self.h, pp, pool_bytes, blobs.ctypes.data, len(blobs),
                                      roots.ctypes.data, nr, flags, status.ctypes.data,
                                      ctypes.byref(info))
        self._gc_nblobs, self._gc_nlive = len(blobs), int(info.nlive)
        return rc, info.as_dict(), status[:nr]

    def copy_gc(self, align16: bool = False):
        """bsg_engine_copy_gc: (live[nblobs] uint8, table[nlive] POOL_BLOB_DTYPE) of the last
        successful gc_mark(), the table with the tight or the 16-aligned new offsets; raises
        BsgError (ESTATE) without one."""
        nb, nl = self._gc_nblobs, self._gc_nlive
        live = np.zeros(max(nb, 1), dtype=np.uint8)
        table = np.zeros(max(nl, 1), dtype=POOL_BLOB_DTYPE)
        _check(lib().bsg_engine_copy_gc(self.h, live.ctypes.data, nb, table.ctypes.data, nl,
                                        GC_ALIGN16 if align16 else 0), "bsg_engine_copy_gc")
        return live[:nb], table[:nl]

    def gc_live_device(self) -> int:
        """bsg_engine_gc_live_device: live[]'s device address (0 without a mark)."""
        return lib().bsg_engine_gc_live_device(self.h) or 0

    def gc_compact(self, pool, out, align16: bool = False, pool_bytes: int | None = None,
                   cap: int | None = None):
        """bsg_engine_gc_compact: the last mark's live blobs gathered into `out` (a DeviceBuffer,
        or a device address with cap). Returns (rc, out_bytes); a negative rc is returned, not
        raised."""
        pp = pool.ptr if isinstance(pool, DeviceBuffer) else pool
        op = out.ptr if isinstance(out, DeviceBuffer) else out
        pool_bytes = pool.nbytes + READ_SLACK if pool_bytes is None else pool_bytes
        cap = out.nbytes if cap is None else cap
        n = ctypes.c_uint64(0)
        rc = lib().bsg_engine_gc_compact(self.h, pp, pool_bytes, op, cap,
                                         GC_ALIGN16 if align16 else 0, ctypes.byref(n))
        return rc, n.value

    def gc_ms(self) -> dict:
        """The last gc_mark() call's stages and the last gc_compact() in ms (test tooling; needs
        profile() on)."""
        out = (ctypes.c_float * 4)()
        _check(lib().bsg_engine_gc_ms_debug(self.h, out), "bsg_engine_gc_ms_debug")
        return {"index": float(out[0]), "levels": float(out[1]), "offsets": float(out[2]),
                "compact": float(out[3])}

    def pool_put(self, pool: "Pool", chunks: bool = True, nodes: bool = True) -> dict:
        """bsg_engine_pool_put: the last finished run's new chunks (its records) and new tree
        nodes (needs trees()) appended to `pool`, on the device. Returns the call's
        bsg_pool_put_info as a dict; raises BsgError (code, info) on any failure."""
        flags = (POOL_CHUNKS if chunks else 0) | (POOL_NODES if nodes else 0)
        info = POOL_PUT_INFO()
        rc = lib().bsg_engine_pool_put(self.h, pool.h, flags, ctypes.byref(info))
        if rc != BSG_OK:
            raise BsgError(rc, "bsg_engine_pool_put", info.as_dict())
        pool._items = int(info.items)
        return info.as_dict()

    def pool_collect(self, src: "Pool", dst: "Pool", roots, flags: int = 0):
        """bsg_pool_collect: `src` marked from `roots` ([n, 32] uint8, or n * 32 bytes) where it
        lies, its live blobs appended to the empty pool `dst`. Returns (rc, info, status): the
        return code, the bsg_pool_collect_info as a dict and the per-Root status (int32); a
        negative rc is returned, not raised. The mark is this engine's gc result afterwards
        (copy_gc, gc_live_device, gc_compact on src.ptr)."""
        roots = np.ascontiguousarray(np.frombuffer(roots, dtype=np.uint8)
                                     if isinstance(roots, (bytes, bytearray)) else roots,
                                     dtype=np.uint8).reshape(-1)
        assert len(roots) % 32 == 0
        nr = len(roots) // 32
        status = np.zeros(max(nr, 1), dtype=np.int32)
        info = PoolCollectInfo()
        nsrc = src.stat()["nblobs"] if src is not None and src.h else 0
        rc = lib().bsg_pool_collect(self.h, src.h if src is not None else None,
                                    dst.h if dst is not None else None, roots.ctypes.data, nr,
                                    flags, status.ctypes.data, ctypes.byref(info))
        self._gc_nblobs, self._gc_nlive = nsrc, int(info.gc.nlive)
        if rc == BSG_OK:
            dst._nremap = nsrc
        return rc, info.as_dict(), status[:nr]

    def pool_merge(self, src: "Pool", dst: "Pool", roots=None, all: bool = False,
                   verify: bool = False, missing_leaves: bool = False):
        """bsg_pool_merge: the blobs of `src` that are live from `roots` (every blob with
        all=True, which takes no roots) and whose refs `dst` lacks, appended to `dst`. Returns
        (rc, info, status) like pool_collect: the bsg_pool_merge_info as a dict and the per-Root
        status; a negative rc is returned, not raised. Without all=True the mark is this engine's
        gc result afterwards; dst.remap() serves the remap."""
        if roots is None:
            rp, nr = None, 0
        else:
            roots = np.ascontiguousarray(np.frombuffer(roots, dtype=np.uint8)
                                         if isinstance(roots, (bytes, bytearray)) else roots,
                                         dtype=np.uint8).reshape(-1)
            assert len(roots) % 32 == 0
            rp, nr = roots.ctypes.data, len(roots) // 32
        flags = ((MERGE_ALL if all else 0) | (MERGE_VERIFY if verify else 0)
                 | (GC_MISSING_LEAVES if missing_leaves else 0))
        status = np.zeros(max(nr, 1), dtype=np.int32)
        info = PoolMergeInfo()
        nsrc = src.stat()["nblobs"] if src is not None and src.h else 0
        rc = lib().bsg_pool_merge(self.h, src.h if src is not None else None,
                                  dst.h if dst is not None else None, rp, nr, flags,
                                  status.ctypes.data, ctypes.byref(info))
        if not all:
            self._gc_nblobs, self._gc_nlive = nsrc, int(info.gc.nlive)
        if rc == BSG_OK:
            dst._nremap = nsrc
        return rc, info.as_dict(), status[:nr]

    def pool_sync(self, a: "Pool", b: "Pool", verify: bool = False):
        """bsg_pool_sync: afterwards `a` and `b` hold the same set of refs. Returns (rc, info,
        status): info is the two directions' bsg_pool_merge_info ([0]: a -> b, [1]: b -> a) as
        dicts, status an empty array (no Roots are involved); a negative rc is returned, not
        raised. b.remap() covers a's blobs at the call, a.remap() b's."""
        info = (PoolMergeInfo * 2)()
        na = a.stat()["nblobs"] if a is not None and a.h else 0
        nb = b.stat()["nblobs"] if b is not None and b.h else 0
        rc = lib().bsg_pool_sync(self.h, a.h if a is not None else None,
                                 b.h if b is not None else None, MERGE_VERIFY if verify else 0,
                                 info)
        if rc == BSG_OK:
            b._nremap, a._nremap = na, nb
        return rc, [info[0].as_dict(), info[1].as_dict()], np.zeros(0, dtype=np.int32)

    def pool_merge_ms(self, direction: int = 0) -> dict:
        """The last pool_merge (direction 0) or a direction of the last pool_sync on this engine,
        in ms (test tooling; needs profile() on)."""
        out = (ctypes.c_float * 5)()
        _check(lib().bsg_pool_merge_ms_debug(self.h, direction, out), "bsg_pool_merge_ms_debug")
        return dict(zip(("probe", "plan", "verify", "append", "gather"), map(float, out)))

    def pool_walk(self, pool: "Pool", roots, flags: int = 0):
        """bsg_pool_walk: walk() on a bsg_pool where it lies (its device table and index).
        Returns (rc, info, status) as walk(); copy_walk() serves the result."""
        roots = np.ascontiguousarray(np.frombuffer(roots, dtype=np.uint8)
                                     if isinstance(roots, (bytes, bytearray)) else roots,
                                     dtype=np.uint8).reshape(-1)
        assert len(roots) % 32 == 0
        ns = len(roots) // 32
        status = np.zeros(max(ns, 1), dtype=np.int32)
        info = WalkInfo()
        rc = lib().bsg_pool_walk(self.h, pool.h if pool is not None else None, roots.ctypes.data,
                                 ns, flags, status.ctypes.data, ctypes.byref(info))
        self._walk_ns, self._walk_nrecs = ns, int(info.nrecs)
        return rc, info.as_dict(), status[:ns]

    def pool_restore_walk(self, pool: "Pool", out, out_off, verify: bool = False,
                          out_cap: int | None = None):
        """bsg_pool_restore_walk: restore_walk() on a bsg_pool where it lies. Returns (rc, info)
        as restore_walk()."""
        op = out.ptr if isinstance(out, DeviceBuffer) else out
        out_cap = out.nbytes if out_cap is None else out_cap
        oo = _u64(out_off)
        info = RestoreInfo()
        rc = lib().bsg_pool_restore_walk(self.h, pool.h if pool is not None else None, op, out_cap,
                                         _p(oo, ctypes.c_uint64), len(oo),
                                         RESTORE_VERIFY if verify else 0, ctypes.byref(info))
        return rc, info.as_dict()

    def read(self, pool, blobs, ranges, out, out_off, flags: int = 0,
             pool_bytes: int | None = None, out_cap: int | None = None):
        """bsg_engine_read: the byte ranges `ranges` (READ_RANGE_DTYPE, or (root, offset, len)
        triples) of the streams under their Roots, read out of the pool (POOL_BLOB_DTYPE table; a
        DeviceBuffer, or a device address with pool_bytes) into out + out_off[q] (a DeviceBuffer,
        or a device address with out_cap). Returns (rc, status, got, info): the return code, the
        per-range status (int32) and byte counts (uint64) and the bsg_read_info as a dict; a
        negative rc is returned, not raised."""
        pp = pool.ptr if isinstance(pool, DeviceBuffer) else pool
        op = out.ptr if isinstance(out, DeviceBuffer) else out
        pool_bytes = pool.nbytes + READ_SLACK if pool_bytes is None else pool_bytes
        out_cap = out.nbytes if out_cap is None else out_cap
        blobs = np.ascontiguousarray(blobs, dtype=POOL_BLOB_DTYPE)
        rg, oo = read_ranges(ranges), _u64(out_off)
        assert len(rg) == len(oo)
        status = np.zeros(max(len(rg), 1), dtype=np.int32)
        got = np.zeros(max(len(rg), 1), dtype=np.uint64)
        info = ReadInfo()
        rc = lib().bsg_engine_read(self.h, pp, pool_bytes, blobs.ctypes.data, len(blobs),
                                   rg.ctypes.data, len(rg), op, out_cap, oo.ctypes.data, flags,
                                   status.ctypes.data, got.ctypes.data, ctypes.byref(info))
        return rc, status[:len(rg)], got[:len(rg)], info.as_dict()

    def read_ms(self) -> dict:
        """The last read() / Pool.read() call's stages in ms (test tooling; needs profile() on)."""
        out = (ctypes.c_float * 6)()
        _check(lib().bsg_engine_read_ms_debug(self.h, out), "bsg_engine_read_ms_debug")
        return dict(zip(("index", "levels", "placement", "resolve", "verify", "scatter"),
                        (float(x) for x in out)))

    def dedup_ms(self) -> dict:
        """The last dedup() and pack_unique() calls in ms (test tooling; needs profile() on)."""
        out = (ctypes.c_float * 2)()
        _check(lib().bsg_engine_dedup_ms_debug(self.h, out), "bsg_engine_dedup_ms_debug")
        return {"dedup": float(out[0]), "pack": float(out[1])}

    @property
    def stream(self) -> int:
        return lib().bsg_engine_stream(self.h) or 0

    def profile(self, enable: int = 1) -> None:
        """bsg_engine_profile: 0 off, 1 (or True) every stage, 2 the SHA-256 stage only."""
        _check(lib().bsg_engine_profile(self.h, int(enable)), "bsg_engine_profile")

    def stage_ms(self) -> list[float]:
        out = (ctypes.c_float * 3)()
        _check(lib().bsg_engine_stage_ms(self.h, out), "bsg_engine_stage_ms")
        return [float(x) for x in out]

    def diag(self) -> dict:
        d = np.zeros(16, dtype=np.uint64)
        _check(lib().bsg_engine_diag(self.h, _p(d, ctypes.c_uint64)), "bsg_engine_diag")
        out = {"nlong": int(d[0]), "long_thresh": int(d[1]), "max_nblocks": int(d[2]),
               "nshort": int(d[13]), "wave_tickets": int(d[14]), "total_blocks": int(d[15])}
        t = np.zeros(4, dtype=np.uint64)
        _check(lib().bsg_engine_timeline(self.h, _p(t, ctypes.c_uint64)), "bsg_engine_timeline")
        if t[0] and t[1] and t[3]:  # microseconds after the first k_sha wave started (an
            t0 = int(t[0])           # early chain, KNOB_EARLY, starts before it: negative)
            out["timeline_us"] = {"long_start": round((int(t[1]) - t0) * 0.01, 1),
                                  "long_end": round((int(t[2]) - t0) * 0.01, 1),
                                  "lane_end": round((int(t[3]) - t0) * 0.01, 1)}
        if os.environ.get("BSG_DIAG_RAW") == "1":  # experiment builds (BSG_LANE_DIAG)
            out["diag2_raw"] = [int(x) for x in d[8:13]]
        for tag, o in (("long", 3), ("lane", 8)):
            cyc, rt, nb = int(d[o + 1] - d[o]), int(d[o + 3] - d[o + 2]), int(d[o + 4])
            if nb and rt:
                out[tag] = {"blocks": nb, "cycles_per_block": round(cyc / nb, 1),
                            "clock_ghz": round(cyc / (rt * 10.0), 3),
                            "us_per_block": round(rt * 0.01 / nb, 4)}
        t = np.zeros(12, dtype=np.uint64)
        _check(lib().bsg_engine_host_tail(self.h, _p(t, ctypes.c_uint64)), "bsg_engine_host_tail")
        out["host_tail"] = {"chunks": int(t[0]), "bytes": int(t[1]), "cut_blocks": int(t[2]),
                            "gather_us": int(t[3]), "host_done_us": int(t[4]),
                            "impl": "x86-sha" if int(t[5]) == 1 else "portable",
                            "threads": int(t[6]), "host_rate_bytes_s": int(t[7]),
                            "longest_blocks": int(t[8]), "longest_left_blocks": int(t[9]),
                            "host_blocks": int(t[10]), "cpuid_sha": bool(t[11])}
        return out

    def set_host_tail(self, min_bytes: int = 512 << 20, force_cut: int = 0,
                      portable: bool = False, ring_bytes: int = 0) -> None:
        """bsg_engine_host_tail_debug (test tooling, not in bsgpu.h): this engine's later runs may
        hand chunks to the host from `min_bytes` on; `force_cut` > 0 takes every chunk of at least
        that many SHA-256 blocks (as far as the ring holds them) instead of the cost model's
        choice; `portable` forces the portable hash; `ring_bytes` > 0 sets the ring's size."""
        _check(lib().bsg_engine_host_tail_debug(self.h, int(min_bytes), int(force_cut),
                                                int(bool(portable)), int(ring_bytes)),
               "bsg_engine_host_tail_debug")

    def tiers(self) -> dict:
        """bsg_engine_tiers_debug (test tooling, not in bsgpu.h): how k_bucket_scan split the last
        finished run's wave-mode jobs. `nlong_grp` jobs on `tickets_grp` solo / group tickets, the
        first `helped` of them solo chains with a helper wave; `wave_tickets` counts the pair
        tickets too (diag()'s nlong - nlong_grp jobs). `early`: whether early chains 0 and 1
        each hashed a chunk."""
        d = np.zeros(6, dtype=np.uint64)
        _check(lib().bsg_engine_tiers_debug(self.h, _p(d, ctypes.c_uint64)),
               "bsg_engine_tiers_debug")
        return {"nlong_grp": int(d[0]), "tickets_grp": int(d[1]), "helped": int(d[2]),
                "wave_tickets": int(d[3]), "early": (bool(d[4]), bool(d[5]))}

    def set_early_min(self, nbytes: int) -> None:
        """bsg_engine_early_min_debug (test tooling, not in bsgpu.h): this engine's later runs
        take early chains from `nbytes` on (256 MiB by default; 0: every run). KNOB_EARLY and
        KNOB_LIGHT_BYTES apply as before."""
        _check(lib().bsg_engine_early_min_debug(self.h, int(nbytes)),
               "bsg_engine_early_min_debug")

    def early_picks(self) -> list:
        """bsg_engine_early_picks_debug (test tooling, not in bsgpu.h): the last finished run's
        early chains, per filled slot (blocks, cand_index, record_index or None): k_pick's key,
        (blocks << 32) | index of the chunk's start candidate in the sorted candidate list, and
        the index k_lens matched it to in the run's records. Empty slots are left out (slot 1 is
        never filled without slot 0); [] after a hash run or a run without early chains."""
        d = np.zeros(4, dtype=np.uint64)
        _check(lib().bsg_engine_early_picks_debug(self.h, _p(d, ctypes.c_uint64)),
               "bsg_engine_early_picks_debug")
        out = []
        for k in range(2):
            top, idx = int(d[k]), int(d[2 + k])
            if top:
                out.append((top >> 32, top & 0xFFFFFFFF, idx - 1 if idx else None))
            elif idx:
                raise BsgError(-5, f"bsg_engine_early_picks_debug: idx[{k}] without top[{k}]")
        if not d[0] and d[1]:
            raise BsgError(-5, "bsg_engine_early_picks_debug: top[1] without top[0]")
        return out

    def regions(self) -> dict:
        """bsg_engine_regions_debug (test tooling, not in bsgpu.h): the address regions of the
        last finished run's per-lane SHA-256 jobs (Regions in bsgpu_internal.h). `nregions` = R
        and `off[0..R]`: region r holds off[r + 1] - off[r] jobs."""
        kmax = 256  # kMaxRegions; the record starts nregions, rr, pad[6], head[kmax], off[kmax+1]
        d = np.zeros(8 + kmax + kmax + 1, dtype=np.uint64)
        _check(lib().bsg_engine_regions_debug(self.h, d.ctypes.data, d.nbytes),
               "bsg_engine_regions_debug")
        R = int(d[0])
        if not 1 <= R <= kmax:
            raise BsgError(-5, f"bsg_engine_regions_debug: nregions {R}")
        return {"nregions": R, "off": [int(x) for x in d[8 + kmax: 8 + kmax + R + 1]]}

    @property
    def candidates(self) -> int:
        return lib().bsg_engine_candidates(self.h)

    @property
    def rescan_strips(self) -> int:
        """bsg_engine_rescan_debug (test tooling, not in bsgpu.h): strips of the last finished
        run with more candidates than slots, which k_rescan scanned again."""
        return int(lib().bsg_engine_rescan_debug(self.h))

    def close(self) -> None:
        if self.h:
            lib().bsg_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


IN_SET = 1 << 63  # Engine.dedup: first[i] bit 63, the ref was in the refset before the call


class RefSet:
    """bsg_refset: the refs a store already holds, kept on the device across runs."""

    def __init__(self, device: int = 0):
        err = ctypes.c_int(0)
        self.h = lib().bsg_refset_new(device, ctypes.byref(err))
        if not self.h:
            raise BsgError(err.value, "bsg_refset_new")

    def add(self, refs) -> np.ndarray:
        """bsg_refset_add: refs as an (n, 32) uint8 array or a list of 32-byte strings. Returns
        added[n] (uint8): 1 iff the ref was not in the set and is no earlier entry of this call."""
        if not isinstance(refs, np.ndarray):
            refs = np.frombuffer(b"".join(bytes(r) for r in refs), dtype=np.uint8)
        a = np.ascontiguousarray(refs, dtype=np.uint8).reshape(-1, 32)
        added = np.zeros(max(len(a), 1), dtype=np.uint8)
        _check(lib().bsg_refset_add(self.h, a.ctypes.data, len(a), added.ctypes.data),
               "bsg_refset_add")
        return added[: len(a)]

    def count(self) -> int:
        return int(lib().bsg_refset_count(self.h))

    def free(self) -> None:
        if self.h:
            lib().bsg_refset_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Pool:
    """bsg_pool: a pool of blobs that lives in device memory across runs (Engine.pool_put fills
    it). Engine.walk, restore, restore_walk and gc_mark take it as
    `pool.ptr, pool.table(), ..., pool_bytes=pool.pool_bytes`; Engine.pool_walk,
    pool_restore_walk, pool_collect and Pool.read take it where it lies."""

    def __init__(self, cap_bytes: int, cap_blobs: int, device: int = 0):
        err = ctypes.c_int(0)
        self.device, self._items, self._nremap = device, 0, 0
        self.h = lib().bsg_pool_new(device, cap_bytes, cap_blobs, ctypes.byref(err))
        if not self.h:
            raise BsgError(err.value, "bsg_pool_new")

    def stat(self) -> dict:
        st = PoolStats()
        _check(lib().bsg_pool_stat(self.h, ctypes.byref(st)), "bsg_pool_stat")
        return st.as_dict()

    @property
    def ptr(self) -> int:
        """bsg_pool_bytes_device: the d_pool argument of walk / restore / gc."""
        return lib().bsg_pool_bytes_device(self.h) or 0

    @property
    def pool_bytes(self) -> int:
        return self.stat()["pool_bytes"]

    def table(self, first: int = 0) -> np.ndarray:
        """bsg_pool_copy_table: entries [first, nblobs) as POOL_BLOB_DTYPE."""
        n = self.stat()["nblobs"] - first
        out = np.zeros(max(n, 1), dtype=POOL_BLOB_DTYPE)
        _check(lib().bsg_pool_copy_table(self.h, out.ctypes.data, first, max(n, 0)),
               "bsg_pool_copy_table")
        return out[:max(n, 0)]

    def where(self) -> np.ndarray:
        """bsg_pool_copy_where: the blob index of every item of the last successful put."""
        out = np.zeros(max(self._items, 1), dtype=np.uint64)
        _check(lib().bsg_pool_copy_where(self.h, out.ctypes.data, self._items),
               "bsg_pool_copy_where")
        return out[:self._items]

    def to_host(self, n: int | None = None) -> np.ndarray:
        """The pool's first n bytes (default: up to the end of its last blob)."""
        n = self.stat()["bytes"] if n is None else n
        out = np.empty(max(n, 1), dtype=np.uint8)
        if n:
            _check(lib().bsg_memcpy(self.device, out.ctypes.data, self.ptr, n, 1), "bsg_memcpy")
        return out[:n]

    def read(self, eng: "Engine", ranges, out, out_off, flags: int = 0,
             out_cap: int | None = None):
        """bsg_pool_read: Engine.read() on this pool where it lies (its device table and index),
        on `eng`. Returns (rc, status, got, info) as Engine.read()."""
        op = out.ptr if isinstance(out, DeviceBuffer) else out
        out_cap = out.nbytes if out_cap is None else out_cap
        rg, oo = read_ranges(ranges), _u64(out_off)
        assert len(rg) == len(oo)
        status = np.zeros(max(len(rg), 1), dtype=np.int32)
        got = np.zeros(max(len(rg), 1), dtype=np.uint64)
        info = ReadInfo()
        rc = lib().bsg_pool_read(eng.h if eng is not None else None, self.h, rg.ctypes.data,
                                 len(rg), op, out_cap, oo.ctypes.data, flags, status.ctypes.data,
                                 got.ctypes.data, ctypes.byref(info))
        return rc, status[:len(rg)], got[:len(rg)], info.as_dict()

    def put_blobs(self, eng: "Engine", src, off, lens, flags: int = 0):
        """bsg_pool_put_blobs: the blobs src[off[i] .. off[i] + lens[i]) (a DeviceBuffer or a
        device address) hashed on `eng` and the new ones appended. Returns (rc, info, refs): the
        return code, the bsg_pool_put_info as a dict and the blobs' refs ([n, 32] uint8); a
        negative rc is returned, not raised. where() serves the items' blob indices."""
        sp = src.ptr if isinstance(src, DeviceBuffer) else src
        oo, ll = _u64(off), _u64(lens)
        assert len(oo) == len(ll)
        refs = np.zeros((max(len(oo), 1), 32), dtype=np.uint8)
        info = POOL_PUT_INFO()
        rc = lib().bsg_pool_put_blobs(eng.h if eng is not None else None, self.h, sp,
                                      _p(oo, ctypes.c_uint64), _p(ll, ctypes.c_uint64), len(oo),
                                      flags, refs.ctypes.data, ctypes.byref(info))
        if rc == BSG_OK:
            self._items = int(info.items)
        return rc, info.as_dict(), refs[:len(oo)]

    def get(self, eng: "Engine", refs, out=None, verify: bool = False,
            out_cap: int | None = None, flags: int | None = None):
        """bsg_pool_get: the blobs under `refs` ([n, 32] uint8, n * 32 bytes or a list of
        32-byte refs) gathered into `out` (a DeviceBuffer, or a device address with out_cap;
        None: nothing is gathered, a Has / size call). Returns (rc, info, idx, out_off): the
        return code, the bsg_pool_get_info as a dict, every request's blob index (NONE64 for a
        missing ref) and its place in `out` (n + 1 entries); a negative rc is returned, not
        raised."""
        if isinstance(refs, (list, tuple)):
            refs = b"".join(bytes(r) for r in refs)
        refs = np.ascontiguousarray(np.frombuffer(refs, dtype=np.uint8)
                                    if isinstance(refs, (bytes, bytearray)) else refs,
                                    dtype=np.uint8).reshape(-1)
        assert len(refs) % 32 == 0
        n = len(refs) // 32
        op = out.ptr if isinstance(out, DeviceBuffer) else out
        if out_cap is None:
            out_cap = out.nbytes if isinstance(out, DeviceBuffer) else 0
        idx = np.zeros(max(n, 1), dtype=np.uint64)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        info = PoolGetInfo()
        fl = (GET_VERIFY if verify else 0) if flags is None else flags
        rc = lib().bsg_pool_get(eng.h if eng is not None else None, self.h,
                                refs.ctypes.data if n else None, n, op, out_cap, fl,
                                idx.ctypes.data, out_off.ctypes.data, ctypes.byref(info))
        return rc, info.as_dict(), idx[:n], out_off

    def blobs_ms(self, eng: "Engine") -> dict:
        """The last put_blobs() and the last get() on `eng` in ms (test tooling; needs the
        engine's profile() on)."""
        out = (ctypes.c_float * 6)()
        _check(lib().bsg_pool_blobs_ms_debug(eng.h, out), "bsg_pool_blobs_ms_debug")
        return dict(zip(("hash", "plan", "append", "probe", "verify", "gather"),
                        (float(x) for x in out)))

    def remap(self) -> np.ndarray:
        """bsg_pool_copy_remap: for every blob index of the source of the last successful collect
        into this pool, its index here (NONE64 for a dead blob)."""
        out = np.zeros(max(self._nremap, 1), dtype=np.uint64)
        _check(lib().bsg_pool_copy_remap(self.h, out.ctypes.data, self._nremap),
               "bsg_pool_copy_remap")
        return out[:self._nremap]

    def remap_device(self) -> int:
        """bsg_pool_remap_device: remap's device address (0 without a collect)."""
        return lib().bsg_pool_remap_device(self.h) or 0

    def where_device(self) -> int:
        """bsg_pool_where_device: where[]'s device address (0 without a put with items)."""
        return lib().bsg_pool_where_device(self.h) or 0

    def reset(self) -> None:
        """bsg_pool_reset: the pool emptied for reuse, as new."""
        _check(lib().bsg_pool_reset(self.h), "bsg_pool_reset")
        self._items = self._nremap = 0

    def collect_ms(self) -> float:
        """The last successful collect into this pool: its k_pool_adopt in ms (test tooling; the
        collecting engine's profile() must be on)."""
        out = ctypes.c_float(0)
        _check(lib().bsg_pool_collect_ms_debug(self.h, ctypes.byref(out)),
               "bsg_pool_collect_ms_debug")
        return float(out.value)

    def put_ms(self) -> dict:
        """The last successful put's parts in ms (test tooling; the putting engine's profile()
        must be on)."""
        out = (ctypes.c_float * 4)()
        _check(lib().bsg_pool_put_ms_debug(self.h, out), "bsg_pool_put_ms_debug")
        return {"first": float(out[0]), "append": float(out[1]), "gather": float(out[2]),
                "where": float(out[3])}

    def free(self) -> None:
        if self.h:
            lib().bsg_pool_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class StreamingSplitter:
    """bsg_open/bsg_write/bsg_close/bsg_drain: the C-ABI form of split.Writer's chunking."""

    def __init__(self, bits: int = 16, min_size: int = 1024, fanout: int = 8, table=None,
                 device: int = 0, tile: int | None = None, carry_cap: int | None = None):
        err = ctypes.c_int(0)
        self._p = params(bits, min_size, fanout)
        self._t, tp = _table_arg(table)
        self.h = lib().bsg_open(device, ctypes.byref(self._p), tp, ctypes.byref(err))
        if not self.h:
            raise BsgError(err.value, "bsg_open")
        if tile is not None:
            _check(lib().bsg_set_tile(self.h, tile), "bsg_set_tile")
        if carry_cap is not None:
            _check(lib().bsg_set_carry_cap(self.h, carry_cap), "bsg_set_carry_cap")

    def set_stream_base(self, base: int) -> None:
        """bsg_set_stream_base (tests): the stream's first byte has offset `base`."""
        _check(lib().bsg_set_stream_base(self.h, base), "bsg_set_stream_base")

    def write(self, data) -> int:
        a = _as_u8(data)
        _check(lib().bsg_write(self.h, a.ctypes.data, a.nbytes), "bsg_write")
        return a.nbytes

    def write_pinned(self, ptr: int, n: int) -> None:
        """bsg_write_pinned: n bytes at ptr, host memory registered with host_register; the
        caller keeps them unchanged until close()."""
        _check(lib().bsg_write_pinned(self.h, ptr, n), "bsg_write_pinned")

    def close(self) -> None:
        _check(lib().bsg_close(self.h), "bsg_close")

    def close_steps(self):
        """bsg_close_begin, then one bsg_close_step per tile still on the device; yields the
        chunks each step made drainable (their concatenation is what close() + drain() give)."""
        _check(lib().bsg_close_begin(self.h), "bsg_close_begin")
        left = ctypes.c_size_t(1)
        while left.value:
            _check(lib().bsg_close_step(self.h, ctypes.byref(left)), "bsg_close_step")
            yield self.drain()

    def reset(self) -> None:
        _check(lib().bsg_reset(self.h), "bsg_reset")

    def window(self) -> memoryview:
        """bsg_write_window: writable memoryview of pinned staging; fill, then commit(n)."""
        p, cap = ctypes.c_void_p(), ctypes.c_size_t()
        _check(lib().bsg_write_window(self.h, ctypes.byref(p), ctypes.byref(cap)),
               "bsg_write_window")
        return memoryview((ctypes.c_uint8 * cap.value).from_address(p.value)).cast("B")

    def commit(self, n: int) -> None:
        _check(lib().bsg_write_commit(self.h, n), "bsg_write_commit")

    def pread_file(self, path: str, threads: int = 8, piece: int = 16 << 20) -> int:
        """Reads a whole file straight into pinned staging with `threads` parallel preads per
        staging window (the form a Go caller gets with io.ReaderAt and goroutines)."""
        from concurrent.futures import ThreadPoolExecutor
        fd = os.open(path, os.O_RDONLY)
        try:
            size = os.fstat(fd).st_size
            pos = 0
            with ThreadPoolExecutor(threads) as ex:
                while pos < size:
                    win = self.window()
                    n = min(len(win), size - pos)
                    parts = [(o, min(piece, n - o)) for o in range(0, n, piece)]
                    got = list(ex.map(lambda p: os.preadv(fd, [win[p[0]:p[0] + p[1]]], pos + p[0]),
                                      parts))
                    if sum(got) != n:
                        raise OSError("short read")
                    self.commit(n)
                    pos += n
            return pos
        finally:
            os.close(fd)

    def read_from(self, f, piece: int = 32 << 20) -> int:
        """Reads a file object to EOF straight into pinned staging (readinto); returns bytes."""
        total = 0
        while True:
            win = self.window()
            k = f.readinto(win[:piece])
            if not k:
                return total
            self.commit(k)
            total += k

    def stats(self) -> dict:
        """bsg_stream_stats_get: host copy / H2D times and NUMA placement since open / reset."""
        st = StreamStats()
        _check(lib().bsg_stream_stats_get(self.h, ctypes.byref(st)), "bsg_stream_stats_get")
        return st.as_dict()

    def drain(self) -> np.ndarray:
        n = lib().bsg_pending(self.h)
        out = np.zeros(max(n, 1), dtype=CHUNK_DTYPE)
        got = lib().bsg_drain(self.h, out.ctypes.data, n)
        return out[:got]

    def free(self) -> None:
        if self.h:
            lib().bsg_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------
# C++ host mirror (include/bs_split.hpp) through its C ABI: store/mem, split.Writer/Reader.
# ---------------------------------------------------------------------------------------------
NOT_FOUND = -2    # BSG_ENOTFOUND = bs.ErrNotFound
CORRUPT = -74     # BSG_ECORRUPT: a fetched chunk does not hash to its ref (Reader verify)
READER_VERIFY = 1


class MemStore:
    """store/mem (store/mem/mem.go): refs are computed on the GPU."""

    def __init__(self, device: int = 0):
        self.h = lib().bsg_memstore_new(device)
        if not self.h:
            raise BsgError(-12, "bsg_memstore_new")

    def put(self, blob: bytes) -> tuple[bytes, bool]:
        ref = ctypes.create_string_buffer(32)
        added = ctypes.c_int(0)
        b = bytes(blob)
        _check(lib().bsg_store_put(self.h, b, len(b), ref, ctypes.byref(added)), "put")
        return ref.raw, bool(added.value)

    def put_ref(self, ref: bytes, blob: bytes) -> bool:
        """PutWithRef: store blob under a ref the caller computed (no hashing)."""
        added = ctypes.c_int(0)
        b = bytes(blob)
        _check(lib().bsg_store_put_ref(self.h, bytes(ref), b, len(b), ctypes.byref(added)),
               "put_ref")
        return bool(added.value)

    def refs_after(self, start: bytes) -> list[bytes]:
        """ListRefs(start, ...): refs > start, lexicographic."""
        n = lib().bsg_store_list_from(self.h, bytes(start), None, 0)
        buf = ctypes.create_string_buffer(32 * max(n, 1))
        lib().bsg_store_list_from(self.h, bytes(start), buf, n)
        return [buf.raw[32 * i:32 * i + 32] for i in range(n)]

    def get(self, ref: bytes) -> bytes:
        n = ctypes.c_size_t(0)
        rc = lib().bsg_store_get(self.h, bytes(ref), None, 0, ctypes.byref(n))
        if rc == NOT_FOUND:
            raise KeyError(bytes(ref).hex())
        _check(rc, "get")
        buf = ctypes.create_string_buffer(max(n.value, 1))
        _check(lib().bsg_store_get(self.h, bytes(ref), buf, n.value, ctypes.byref(n)), "get")
        return buf.raw[: n.value]

    def refs(self) -> list[bytes]:
        n = lib().bsg_store_list(self.h, None, 0)
        buf = ctypes.create_string_buffer(32 * max(n, 1))
        lib().bsg_store_list(self.h, buf, n)
        return [buf.raw[32 * i:32 * i + 32] for i in range(n)]

    def __len__(self) -> int:
        return lib().bsg_store_count(self.h)

    def held_bytes(self) -> int:
        """Host bytes the store keeps alive (store/mem: copies + aliased Write pieces)."""
        return lib().bsg_store_held_bytes(self.h)

    def delete(self, ref: bytes) -> None:
        """bs.DeleterStore.Delete (store/mem only)."""
        _check(lib().bsg_store_delete(self.h, bytes(ref)), "Delete")

    def protect_children(self, ref: bytes) -> list[tuple[bytes, bool]]:
        """split.Protect (split/split.go:306-322): [(child ref, traverse?)] of the Node at ref,
        child nodes (traverse=True) first, then leaves."""
        n = ctypes.c_size_t(0)
        _check(lib().bsg_split_protect(self.h, bytes(ref), None, None, 0, ctypes.byref(n)),
               "Protect")
        refs = ctypes.create_string_buffer(32 * max(n.value, 1))
        trav = ctypes.create_string_buffer(max(n.value, 1))
        _check(lib().bsg_split_protect(self.h, bytes(ref), refs, trav, n.value, ctypes.byref(n)),
               "Protect")
        return [(refs.raw[32 * i:32 * i + 32], trav.raw[i] == 1) for i in range(n.value)]

    def free(self):
        if self.h:
            lib().bsg_store_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class FileStore(MemStore):
    """store/file (store/file/file.go): one file per blob at root/blobs/hh/hhhh/<hex>; refs are
    computed on the GPU (or taken from the split kernels' chunk records by the Writer)."""

    def __init__(self, root: str, device: int = 0):  # noqa: D107 (no MemStore.__init__)
        self.root = root
        self.h = lib().bsg_filestore_new(os.fsencode(root), device)
        if not self.h:
            raise BsgError(-22, "bsg_filestore_new")

    def set_write_behind(self, nbytes: int) -> None:
        _check(lib().bsg_filestore_set_write_behind(self.h, nbytes), "set_write_behind")


class Writer:
    """split.NewWriter(ctx, st, Bits(..), MinSize(..), Fanout(..)) -> Write / Close / Root."""

    def __init__(self, store: MemStore, bits: int = 16, min_size: int = 1024, fanout: int = 8,
                 device: int = 0, tile: int = 0):
        err = ctypes.c_int(0)
        self._p = params(bits, min_size, fanout)
        self.h = lib().bsg_writer_new(device, store.h, ctypes.byref(self._p), tile,
                                      ctypes.byref(err))
        if not self.h:
            raise BsgError(err.value, "bsg_writer_new")
        self.store = store

    def set_stream_base(self, base: int) -> None:
        """bsg_writer_set_stream_base (tests), before the first write."""
        _check(lib().bsg_writer_set_stream_base(self.h, base), "bsg_writer_set_stream_base")

    def write(self, data) -> int:
        a = _as_u8(data)
        _check(lib().bsg_writer_write(self.h, a.ctypes.data, a.nbytes), "Write")
        return a.nbytes

    def close(self) -> None:
        _check(lib().bsg_writer_close(self.h), "Close")

    @property
    def root(self) -> bytes:
        out = ctypes.create_string_buffer(32)
        _check(lib().bsg_writer_root(self.h, out), "Root")
        return out.raw

    def timings(self) -> dict:
        """bsg_writer_timings, in ms: Write copies, background Put + tree, waits for it, node
        hashes, Close, Close's wait for the device, node-hash calls."""
        t = (ctypes.c_double * 7)()
        _check(lib().bsg_writer_timings(self.h, t), "bsg_writer_timings")
        keys = ("copy_ms", "put_tree_ms", "join_ms", "node_hash_ms", "close_ms", "close_dev_ms")
        out = {k: round(t[i] * 1e3, 3) for i, k in enumerate(keys)}
        out["node_hash_calls"] = int(t[6])
        return out

    def free(self):
        if self.h:
            lib().bsg_writer_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Reader:
    """split.NewReader(ctx, g, ref) -> Read / Seek / Size. verify=True checks each leaf node's
    chunks against their refs with one batched GPU SHA-256 call (BSG_READER_VERIFY)."""

    def __init__(self, store: MemStore, root: bytes, verify: bool = False, device: int = 0):
        err = ctypes.c_int(0)
        self.h = lib().bsg_reader_open(store.h, bytes(root), READER_VERIFY if verify else 0,
                                       device, ctypes.byref(err))
        if not self.h:
            raise BsgError(err.value, "bsg_reader_open")
        self.store = store

    def read(self, n: int) -> bytes:
        buf = ctypes.create_string_buffer(max(n, 1))
        got = lib().bsg_reader_read(self.h, buf, n)
        if got < 0:
            raise BsgError(int(got), "Read")
        return buf.raw[:got]

    def read_all(self) -> bytes:
        parts = []
        while True:
            b = self.read(1 << 20)
            if not b:
                return b"".join(parts)
            parts.append(b)

    def seek(self, off: int, whence: int = 0) -> int:
        return lib().bsg_reader_seek(self.h, off, whence)

    @property
    def size(self) -> int:
        return lib().bsg_reader_size(self.h)

    def stats(self) -> dict:
        """bsg_reader_stats (verify mode): windows verified on the reading thread / taken from
        the read-ahead, bytes verified, read-ahead windows dropped after a seek."""
        out = np.zeros(4, dtype=np.uint64)
        _check(lib().bsg_reader_stats(self.h, _p(out, ctypes.c_uint64)), "bsg_reader_stats")
        return {"sync_windows": int(out[0]), "ahead_windows": int(out[1]),
                "bytes": int(out[2]), "dropped": int(out[3])}

    def free(self):
        if self.h:
            lib().bsg_reader_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
