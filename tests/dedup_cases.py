"""Inputs and the model for bsg_engine_dedup / bsg_refset / bsg_engine_pack_unique.

The model is a dict from ref bytes to first index over the ORACLE's records of the same bytes;
expected first / uniq / pack_off and the packed bytes follow from it. Every builder returns host
streams (uint8 arrays) and the split parameters; tests/test_dedup_cpu.py holds each builder to
the properties it claims, tests/test_gpu_dedup.py runs them on the device."""
from __future__ import annotations

import os
import re

import numpy as np

from bs_amd.synth import edit_stream, splitmix_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bs_amd", "csrc")
IN_SET = 1 << 63


def constants() -> dict:
    """The set's starting size and load limit and the pack tile, read from the source."""
    out = {}
    with open(os.path.join(CSRC, "bsgpu_internal.h")) as f:
        text = f.read()
    for name in ("kRefSetSlots0", "kRefSetLoadPct", "kPackTile"):
        m = re.findall(r"^constexpr\s+uint(?:32|64)_t\s+%s\s*=\s*(\d+)\s*;" % name, text, re.M)
        assert len(m) == 1, (name, m)
        out[name] = int(m[0])
    return out


def doubling_points(k: int = 2) -> list[int]:
    """The key counts at which a set's table is full to its load limit: one more key doubles it."""
    c = constants()
    return [(c["kRefSetSlots0"] << j) * c["kRefSetLoadPct"] // 100 for j in range(k)]


# ---- layout and the oracle's records ----------------------------------------------------------
def place(streams):
    """Streams packed at 16-byte offsets: (host buffer, off, lens)."""
    off, o = [], 0
    for d in streams:
        off.append(o)
        o += (len(d) + 15) & ~15
    host = np.zeros(max(o, 16), dtype=np.uint8)
    for d, p in zip(streams, off):
        host[p:p + len(d)] = d
    return host, off, [len(d) for d in streams]


def oracle_records(O, table, streams, bits, min_size):
    """The oracle's records of every stream, stream-major, `stream` filled in."""
    parts = []
    for s, d in enumerate(streams):
        r = O.split(table, np.ascontiguousarray(d), bits=bits, min_size=min_size).copy()
        r["stream"] = s
        parts.append(r)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=O.CHUNK_DTYPE)


# ---- the model -----------------------------------------------------------------------------
def first_index(refs, seen=frozenset()):
    """refs: a list of bytes. Returns (first, new): first[i] = the smallest j with refs[j] ==
    refs[i], | IN_SET if refs[i] is in `seen`; new = the indices i with first[i] == i."""
    where, first, new = {}, [], []
    for i, r in enumerate(refs):
        j = where.setdefault(r, i)
        if r in seen:
            first.append(j | IN_SET)
        else:
            first.append(j)
            if j == i:
                new.append(i)
    return first, new


def brute_first(refs, seen=frozenset()):
    """first_index by comparing every pair."""
    first, new = [], []
    for i, r in enumerate(refs):
        j = min(k for k in range(i + 1) if refs[k] == r)
        inset = any(r == q for q in seen)
        first.append(j | (IN_SET if inset else 0))
        if j == i and not inset:
            new.append(i)
    return first, new


def ref_list(recs):
    return [r.tobytes() for r in recs["ref"]]


def expected(recs, seen=frozenset()):
    """(first, uniq, pack_off) as uint64 arrays for records `recs` and the set `seen`."""
    first, new = first_index(ref_list(recs), seen)
    lens = [int(recs["len"][i]) for i in new]
    pack_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64) if new \
        else np.zeros(1, np.uint64)
    return (np.array(first, dtype=np.uint64), np.array(new, dtype=np.uint64), pack_off)


def packed(streams, recs, uniq) -> bytes:
    """The host copies of the new chunks, concatenated."""
    out = []
    for i in uniq:
        r = recs[int(i)]
        d = streams[int(r["stream"])]
        out.append(bytes(d[int(r["offset"]):int(r["offset"]) + int(r["len"])]))
    return b"".join(out)


# ---- builders: (streams, bits, min_size) ------------------------------------------------------
MIB = 1 << 20


def edited_copies():
    """BASELINE configs[4] scaled to 2 x 1 MiB: stream B = stream A with 16 seeded edits
    (overwrite / insert / delete) of 256 bytes. More than half of B's chunks are A's."""
    a = splitmix_array(0xB5B52026, MIB)
    b = edit_stream(a, 5, sites=16, span=256)
    return [a, b], 8, 64


def residues():
    """512 KiB of SplitMix at Bits 5 / MinSize 64 (about 5,000 chunks of every length residue),
    listed after 80 excerpts of 2,000 bytes of itself: each excerpt's chunks are duplicates when
    the long stream reaches them, which shifts the packed offset against the source offset by
    another amount, so every pair (source address mod 16, packed offset mod 16) occurs."""
    d = splitmix_array(77, 512 << 10)
    cuts = [d[3000 + 6400 * j:5000 + 6400 * j] for j in range(80)]
    return cuts + [d], 5, 64


def tiny_chunks():
    """4 KiB at Bits 1 / MinSize 1: chunks of 1 to a few bytes; the 1-byte ones have only 256
    values, so at least a third of the chunks repeat an earlier one and the new ones lie between
    them (packing skips segments, and many segments share one 16-byte vector)."""
    return [splitmix_array(31, 4 << 10)], 1, 1


def zeros():
    """An all-zero stream at MinSize 64: every chunk but possibly the last is identical."""
    return [np.zeros(10_000, dtype=np.uint8)], 6, 64


def one_chunk_streams(n: int = 3000):
    """n one-chunk streams (Bits 33 never splits) of 64 bytes; every third repeats the stream two
    before it."""
    out = []
    for s in range(n):
        seed = s - 2 if s % 3 == 2 else s
        out.append(splitmix_array(9000 + seed, 64))
    return out, 33, 64


def long_segment():
    """One 3 MiB stream at Bits 33: a single chunk longer than the pack tile, at an odd length."""
    return [splitmix_array(41, 3 * MIB + 5)], 33, 64


def long_among_short(n: int = 2000):
    """That chunk with n one-chunk streams of 64-200 bytes before it and n after it."""
    rng = np.random.default_rng(12)
    lens = rng.integers(64, 201, 2 * n)
    short = [splitmix_array(50_000 + s, int(m)) for s, m in enumerate(lens)]
    return short[:n] + long_segment()[0] + short[n:], 33, 64


def shared_halves():
    """Two groups of 8 streams of 24 KiB: the first 4 streams of each group are the same bytes,
    the other 4 differ (two engines, one set)."""
    common = [splitmix_array(600 + s, 24 << 10) for s in range(4)]
    own = [[splitmix_array(700 + 10 * g + s, 24 << 10) for s in range(4)] for g in range(2)]
    return [common + own[0], common + own[1]], 7, 64


def planted_refs() -> np.ndarray:
    """Host refs for bsg_refset_add, (n, 32) uint8, in this order:
    64 that share their first 8 bytes and differ only in byte 31; 64 equal except in byte 8;
    4,096 random ones that all share their low 16 bits (bytes 0 and 1); an all-zero and an
    all-0xFF ref; then exact repeats of 200 earlier entries."""
    rng = np.random.default_rng(4)
    a = np.tile(rng.integers(0, 256, 32, dtype=np.uint8), (64, 1))
    a[:, 31] = np.arange(64)
    b = np.tile(rng.integers(0, 256, 32, dtype=np.uint8), (64, 1))
    b[:, 8] = np.arange(64) + 100
    c = rng.integers(0, 256, (4096, 32), dtype=np.uint8)
    c[:, 0], c[:, 1] = 0x34, 0x12
    d = np.stack([np.zeros(32, np.uint8), np.full(32, 0xFF, np.uint8)])
    base = np.concatenate([a, b, c, d])
    again = base[rng.integers(0, len(base), 200)]
    return np.concatenate([base, again])


def random_refs(seed: int, n: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)
