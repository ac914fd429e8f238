"""Inputs and the model for bsg_engine_restore.

The model is a dict from ref bytes to the smallest pool blob index; the return code, the
bsg_restore_info and every output byte follow from it and from the layout rules of
include/bsgpu.h, checked here in plain Python (hashlib for the verification).
tests/test_restore_cases_cpu.py holds the model to the oracle's records of the dedup_cases
inputs; tests/test_gpu_restore*.py hold the device to the model."""
from __future__ import annotations

import hashlib

import numpy as np

import dedup_cases as DC
from bs_amd.bsgpu import CHUNK_DTYPE, POOL_BLOB_DTYPE, READ_SLACK, RESTORE_TILE

OK, EINVAL, ENOTFOUND, ECORRUPT, ESTATE = 0, -22, -2, -74, -71
NONE = (1 << 64) - 1
T = RESTORE_TILE
FILL = 0xA5   # what every output buffer holds before a call
GUARD = 256   # bytes kept before and after the output, which no call may touch


def sha(b) -> bytes:
    return hashlib.sha256(bytes(b)).digest()


# ---- the model ---------------------------------------------------------------------------------
def _layout_ok(blobs, recs, out_off, out_len, cap, verify, pool_bytes, out_shift, out_in_pool):
    ns = len(out_off)
    if out_shift % 16:
        return False
    spans = []
    for o, n in zip(out_off, out_len):
        o, n = int(o), int(n)
        if o % 16 or o + n > cap or o + n >= 1 << 64:
            return False
        if n:
            spans.append((o, o + n))
            if out_in_pool is not None and out_in_pool + o < pool_bytes and out_in_pool + o + n > 0:
                return False
    spans.sort()
    if any(b[0] < a[1] for a, b in zip(spans, spans[1:])):
        return False
    hi = 0
    for b in blobs:
        o, n = int(b["off"]), int(b["len"])
        if o + n > pool_bytes:
            return False
        if verify and o % 16:
            return False
        hi = max(hi, o + n)
    if verify and len(blobs) and pool_bytes - hi < READ_SLACK:
        return False
    # the records: stream-major, ascending, every stream tiled exactly
    end = [0] * ns
    prev = -1
    for r in recs:
        s, o, n = int(r["stream"]), int(r["offset"]), int(r["len"])
        if s >= ns or n == 0 or s < prev or o != end[s]:
            return False
        end[s] = o + n
        prev = s
    return all(end[s] == int(out_len[s]) for s in range(ns))


def expected(pool, blobs, recs, out_off, out_len, out0, verify, pool_bytes=None, out_shift=0,
             out_in_pool=None):
    """(rc, info, out): what bsg_engine_restore returns, its bsg_restore_info as a dict and the
    out_cap = len(out0) bytes at d_out afterwards. pool: the host copy of d_pool's bytes;
    pool_bytes: the argument (default len(pool)); out_shift: d_out's address modulo 16;
    out_in_pool: d_out - d_pool if the output lies in the pool's buffer."""
    pool = np.asarray(pool, dtype=np.uint8)
    pool_bytes = len(pool) if pool_bytes is None else pool_bytes
    info = {"bad_record": NONE, "bad_blob": NONE, "bytes": 0, "verified": 0}
    out = np.array(out0, dtype=np.uint8, copy=True)
    if not _layout_ok(blobs, recs, out_off, out_len, len(out0), verify, pool_bytes, out_shift,
                      out_in_pool):
        return EINVAL, info, out
    index = {}
    for k, b in enumerate(blobs):
        index.setdefault(b["ref"].tobytes(), k)
    if verify:
        info["verified"] = int(sum(int(b["len"]) for b in blobs))
        for k, b in enumerate(blobs):
            o, n = int(b["off"]), int(b["len"])
            if sha(pool[o:o + n]) != b["ref"].tobytes():
                info["bad_blob"] = k
                break
    which = [index.get(r["ref"].tobytes()) for r in recs]
    missing = [i for i, k in enumerate(which) if k is None]
    if missing:
        info["bad_record"] = missing[0]
        return ENOTFOUND, info, out
    wrong = [i for i, k in enumerate(which) if int(blobs[k]["len"]) != int(recs[i]["len"])]
    if wrong:
        info["bad_record"] = wrong[0]
    if wrong or info["bad_blob"] != NONE:
        return ECORRUPT, info, out
    for r, k in zip(recs, which):
        d = int(out_off[int(r["stream"])]) + int(r["offset"])
        o, n = int(blobs[k]["off"]), int(blobs[k]["len"])
        out[d:d + n] = pool[o:o + n]
        info["bytes"] += n
    return OK, info, out


# ---- pools -------------------------------------------------------------------------------------
def make_blobs(offs, lens, refs) -> np.ndarray:
    b = np.zeros(len(offs), dtype=POOL_BLOB_DTYPE)
    b["off"], b["len"] = offs, lens
    if len(offs):
        b["ref"] = refs
    return b


def packed_pool(streams, recs):
    """The tight pool bsg_engine_pack_unique writes: (bytes, blobs) with
    blobs[k] = {pack_off[k], len, ref} of record uniq[k]."""
    _, uniq, pack_off = DC.expected(recs)
    pool = np.frombuffer(DC.packed(streams, recs, uniq), dtype=np.uint8).copy()
    u = uniq.astype(np.int64)
    return pool, make_blobs(pack_off[:-1], recs["len"][u], recs["ref"][u])


def aligned_pool(datas, residue=0, slack=READ_SLACK):
    """Blobs `datas` (byte strings) each at the next address that is `residue` modulo 16, then
    `slack` zero bytes after the last one's 16-byte vector: (bytes, blobs), refs computed with
    hashlib."""
    offs, o = [], 0
    for d in datas:
        o += (residue - o) % 16
        offs.append(o)
        o += len(d)
    pool = np.zeros(((o + 15) & ~15) + slack, dtype=np.uint8)
    for d, p in zip(datas, offs):
        pool[p:p + len(d)] = np.frombuffer(bytes(d), dtype=np.uint8)
    refs = np.array([np.frombuffer(sha(d), dtype=np.uint8) for d in datas]).reshape(-1, 32)
    return pool, make_blobs(offs, [len(d) for d in datas], refs)


def unique_datas(streams, recs):
    """The bytes of every record that is the first with its ref, in record order."""
    _, uniq, _ = DC.expected(recs)
    out = []
    for i in uniq:
        r = recs[int(i)]
        d = streams[int(r["stream"])]
        out.append(bytes(d[int(r["offset"]):int(r["offset"]) + int(r["len"])]))
    return out


def make_recs(streams_of_pieces) -> np.ndarray:
    """Records for streams given as lists of byte strings (one record per piece)."""
    rows = []
    for s, pieces in enumerate(streams_of_pieces):
        o = 0
        for d in pieces:
            rows.append((o, len(d), 0, s, np.frombuffer(sha(d), dtype=np.uint8)))
            o += len(d)
    r = np.zeros(len(rows), dtype=CHUNK_DTYPE)
    for i, row in enumerate(rows):
        r[i] = row
    return r


def out_layout(lens, order=None, gap=48):
    """16-aligned output offsets for streams of `lens` laid out in `order` with `gap` spare bytes
    between them: (out_off, cap)."""
    order = list(range(len(lens))) if order is None else order
    off, o = [0] * len(lens), 16
    for s in order:
        off[s] = o
        o = ((o + lens[s] + 15) & ~15) + gap
    return off, o


# ---- case builders: dicts with pool, blobs, recs, out_off, out_len, cap (and want: the streams) --
def case(pool, blobs, recs, lens, order=None, verify=False, want=None):
    out_off, cap = out_layout(lens, order)
    return {"pool": pool, "blobs": blobs, "recs": recs, "out_off": out_off, "out_len": list(lens),
            "cap": cap, "verify": verify, "want": want}


def one_byte_records(data: np.ndarray, stream: int, table: np.ndarray) -> np.ndarray:
    """One record per byte of `data` (table[v]: the ref of the one-byte blob v)."""
    r = np.zeros(len(data), dtype=CHUNK_DTYPE)
    r["offset"] = np.arange(len(data))
    r["len"] = 1
    r["stream"] = stream
    r["ref"] = table[data]
    return r


def segment_edges():
    """1-byte chunks (16 segments per output vector) in streams of 0, 1, 15, 16, 17, T-1, T and
    T+1 bytes, and a last stream that is one chunk of 3T+5 bytes. The pool: the 256 one-byte
    blobs packed tight, then the long one."""
    table = np.array([np.frombuffer(sha(bytes([v])), dtype=np.uint8) for v in range(256)])
    lens = [0, 1, 15, 16, 17, T - 1, T, T + 1]
    streams = [DC.splitmix_array(900 + s, n) if n else np.zeros(0, np.uint8)
               for s, n in enumerate(lens)]
    big = DC.splitmix_array(77, 3 * T + 5)
    recs = [one_byte_records(d, s, table) for s, d in enumerate(streams)]
    last = np.zeros(1, dtype=CHUNK_DTYPE)
    last[0] = (0, len(big), 0, len(lens), np.frombuffer(sha(big), dtype=np.uint8))
    pool = np.concatenate([np.arange(256, dtype=np.uint8), big])
    blobs = make_blobs(list(range(257)), [1] * 256 + [len(big)],
                       np.concatenate([table, last["ref"]]))
    return case(pool, blobs, np.concatenate(recs + [last]), lens + [len(big)],
                order=[8, 3, 0, 7, 1, 6, 2, 5, 4], want=streams + [big])


RESIDUE_LENS = (1, 15, 16, 17, 31, 33)


def source_residue(residue: int):
    """40 records of lengths 1, 15, 16, 17, 31, 33 in one stream, from a pool whose blobs all
    start at `residue` modulo 16."""
    datas = [bytes(DC.splitmix_array(4000 + i, RESIDUE_LENS[i % 6])) for i in range(40)]
    pool, blobs = aligned_pool(datas, residue, slack=0)
    return case(pool, blobs, make_recs([datas]), [sum(len(d) for d in datas)],
                want=[np.frombuffer(b"".join(datas), dtype=np.uint8)])


def many_blobs(n: int = 65537):
    """n pool blobs of 16 bytes, 16-aligned, each referenced once by one stream (one more than
    a hash batch holds, and one past that)."""
    raw = DC.splitmix_array(5150, 16 * n)
    raw[:16 * n].reshape(n, 16)[:, :4] = np.arange(n, dtype="<u4").view(np.uint8).reshape(n, 4)
    refs = np.array([np.frombuffer(sha(raw[16 * i:16 * i + 16]), dtype=np.uint8)
                     for i in range(n)])
    pool = np.concatenate([raw, np.zeros(READ_SLACK, np.uint8)])
    blobs = make_blobs(16 * np.arange(n), [16] * n, refs)
    recs = np.zeros(n, dtype=CHUNK_DTYPE)
    recs["offset"] = 16 * np.arange(n)
    recs["len"] = 16
    recs["ref"] = refs
    return case(pool, blobs, recs, [16 * n], verify=True, want=[raw])


def small_valid():
    """Three streams (one empty) of a few odd-sized pieces, two of them shared: the valid call
    that test_gpu_restore_errors.py mutates. The pool is 16-aligned with read slack."""
    p = [bytes(DC.splitmix_array(300 + i, n)) for i, n in enumerate((40, 7, 100, 33, 64, 19))]
    streams = [[p[0], p[1], p[2]], [], [p[3], p[1], p[4], p[5], p[0]]]
    pool, blobs = aligned_pool(p)
    lens = [sum(len(d) for d in s) for s in streams]
    return case(pool, blobs, make_recs(streams), lens, order=[2, 0, 1],
                want=[np.frombuffer(b"".join(s), dtype=np.uint8) for s in streams])


def wrap_pool():
    """96 blobs of the distinct lengths 1 .. 96 labelled (verify off) with dedup_cases.wrap_base's
    refs in a shuffled order, packed tight; each is named once by the records of two streams, in
    another order. The pool index's probes for the 48 refs with an all-0xFF head start at the
    table's last slot and go on from slot 0, through the homes of the other 48."""
    rng = np.random.default_rng(61)
    refs = DC.wrap_base()[rng.permutation(96)]
    datas = [bytes(DC.splitmix_array(6100 + k, k + 1)) for k in range(96)]
    offs = np.concatenate([[0], np.cumsum([len(d) for d in datas])])[:-1]
    blobs = make_blobs(offs, [len(d) for d in datas], refs)
    pool = np.frombuffer(b"".join(datas), dtype=np.uint8).copy()
    order = rng.permutation(96)
    pieces = [[int(k) for k in order[:50]], [int(k) for k in order[50:]]]
    recs = make_recs([[datas[k] for k in s] for s in pieces])
    recs["ref"] = refs[order]
    streams = [np.frombuffer(b"".join(datas[k] for k in s), dtype=np.uint8) for s in pieces]
    return case(pool, blobs, recs, [len(d) for d in streams], order=[1, 0], want=streams)


def wrap_pool_absent(k: int = 37):
    """wrap_pool with record k naming dedup_cases.wrap_absent: an all-0xFF head, in no blob."""
    c = wrap_pool()
    recs = c["recs"].copy()
    recs[k]["ref"] = DC.wrap_absent()
    return dict(c, recs=recs, want=None), k


# ---- the device against the model (tests/test_gpu_restore*.py) ---------------------------------
def run(gpu, eng, c, verify=None, pool_bytes=None, out_shift=0, pool_buf=None, expect=None):
    """One bsg_engine_restore of case `c` into a FILL-ed buffer with GUARD bytes at both ends;
    the return code, the info and the whole buffer are held to the model. Returns (rc, info,
    out) of the device, out being the out_cap bytes at d_out."""
    verify = c["verify"] if verify is None else verify
    cap = c["cap"]
    pool = np.asarray(c["pool"], dtype=np.uint8)
    pool_bytes = len(pool) if pool_bytes is None else pool_bytes
    out0 = np.full(cap, FILL, dtype=np.uint8)
    want = expected(pool, c["blobs"], c["recs"], c["out_off"], c["out_len"], out0, verify,
                    pool_bytes=pool_bytes, out_shift=out_shift)
    pbuf = pool_buf
    if pbuf is None:
        pbuf = gpu.DeviceBuffer(max(len(pool), 16))
        pbuf.from_host(pool)
    size = GUARD + cap + 16 + GUARD
    obuf = gpu.DeviceBuffer(size)
    try:
        obuf.from_host(np.full(size, FILL, dtype=np.uint8))
        rc, info = OK, None
        try:
            info = eng.restore(pbuf.ptr, c["blobs"], c["recs"], obuf.ptr + GUARD + out_shift,
                               c["out_off"], c["out_len"], verify=verify, pool_bytes=pool_bytes,
                               out_cap=cap)
        except gpu.BsgError as e:
            rc, info = e.code, e.info
        got = obuf.to_host()
    finally:
        obuf.free()
        if pool_buf is None:
            pbuf.free()
    assert (rc, info) == want[:2], (rc, info, want[:2])
    if expect is not None:
        assert rc == expect, (rc, expect)
    lo = GUARD + out_shift
    assert (got[:lo] == FILL).all() and (got[lo + cap:] == FILL).all(), "guards"
    out = got[lo:lo + cap]
    bad = np.flatnonzero(out != want[2])
    assert not len(bad), (len(bad), int(bad[0]))
    return rc, info, out


def check_streams(c, out):
    """The restored streams are the bytes the case was built from."""
    for s, d in enumerate(c["want"]):
        o = c["out_off"][s]
        assert out[o:o + len(d)].tobytes() == bytes(d), s
