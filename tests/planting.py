"""Candidates planted at chosen byte positions: the shared tool of test_gpu_scan_edges.py,
test_planting_cpu.py and test_gpu_planted.py.

A window's buzhash32 depends only on its 64 bytes (closed form, oracle.py:py_window_hash:
h(p) = XOR_k rotl(T[x[p-k]], k mod 32)), so a 64-byte window whose hash has its low bits zero
makes its last byte a candidate wherever it is written. zero_windows() searches such windows,
plant() writes them, and the layout_* builders place them where k_scan and k_select can be
subtly wrong without random data ever noticing (the 2 KiB strip is kStrip, a block 64 bytes):

  A  every (nfull, block, byte parity) of a stream's last strip, streams ordered so that a wave
     of 64 consecutive strips mixes block counts (the WIDE pass's exec-mask drop-out)
  B  every byte 0..63 of the last block, for ten block counts
  C  every offset of a < 64-byte tail, and the final flush with and without a tail
  D  strips of 3, 4, 5, 6 and 31 candidates around kSlotCap = 4
  E  windows with 0..64 bytes in the previous streaming tile
  F  gaps of MinSize - 1, MinSize and MinSize + 1 between candidates

Every builder returns (streams, planted_ends_per_stream); the streaming ones add the tile and
the Write sizes. A builder draws a stream's filler from a seeded generator and keeps the first
draw in which no position of the layout's "clean" ranges but the planted ends has tz >= bits
(window_hashes() below, the closed form in numpy): a random candidate within MinSize bytes
before a planted end is the only thing that keeps the end from being a boundary, and at
Bits = 12 a batch of a thousand streams always has some, so the seed is chosen per stream.
test_planting_cpu.py checks the outcome against the oracle.

level_windows() and level_stream() (at the end) serve the tree tests (tree_cases.py): streams cut
into chunks of chosen levels.
"""
import numpy as np

STRIP = 2048                      # kStrip
PARAMS = [(16, 16), (20, 20), (12, 12)]   # (bits, low); (12, 12) is the narrow loop, the control
REJECT = (20, 16)                 # the pre-filter fires, the exact test rejects


def _rotl(x, r):
    r %= 32
    if r == 0:
        return x
    return ((x << np.uint32(r)) | (x >> np.uint32(32 - r))).astype(np.uint32)


_ROT63 = np.array([(63 - i) % 32 for i in range(62)], dtype=np.uint32)


def _rotl_each(x, r):
    """rotl of x[..., i] by r[i] (0 <= r < 32)."""
    r = r.astype(np.uint32)
    return np.where(r == 0, x, (x << r) | (x >> ((np.uint32(32) - r) & np.uint32(31)))
                    ).astype(np.uint32)


def zero_windows(table, count, low, seed, exact_tz=None):
    """`count` 64-byte windows whose window hash has its `low` low bits zero: 62 random bytes,
    then the two last bytes searched over all 65,536 pairs; further prefixes are drawn until a
    pair exists (about 2^(low - 16) of them). exact_tz: the hash has exactly that many trailing
    zeros (low <= exact_tz < 32), so the level at Bits = b is exact_tz - b."""
    T = np.asarray(table, dtype=np.uint32)
    if exact_tz is None:
        mask, want = np.uint32((1 << low) - 1), np.uint32(0)
    else:
        assert low <= exact_tz < 32
        mask, want = np.uint32((1 << (exact_tz + 1)) - 1), np.uint32(1 << exact_tz)
    rng = np.random.default_rng(seed)
    a62 = _rotl(T, 1)          # byte 62 (one step before the newest): rotl 1
    out = []
    while len(out) < count:
        pre = rng.integers(0, 256, 62, dtype=np.uint8)
        h = np.bitwise_xor.reduce(_rotl_each(T[pre], _ROT63))
        hh = (h ^ a62[:, None] ^ T[None, :]) & mask   # [b62, b63]
        hit = np.argwhere(hh == want)
        if len(hit):
            b62, b63 = hit[rng.integers(0, len(hit))]
            out.append(np.concatenate([pre, np.array([b62, b63], dtype=np.uint8)]))
    return out


def planted_stream(table, n, low, seed):
    """n random bytes with a zero window ending at offset (j mod 64) of every strip j >= 1 that
    holds it; returns (bytes, planted end positions)."""
    rng = np.random.default_rng(seed + 7)
    data = rng.integers(0, 256, n, dtype=np.uint8)
    ends = [STRIP * j + (j % 64) for j in range(1, n // STRIP + 1) if STRIP * j + (j % 64) < n]
    wins = zero_windows(table, len(ends), low, seed)
    for p, w in zip(ends, wins):
        data[p - 63:p + 1] = w
    return data, ends


def plant(data, ends, windows):
    """Writes window i so that it ends at ends[i] (its last byte is data[ends[i]])."""
    order = sorted(range(len(ends)), key=lambda i: ends[i])
    prev = -1
    for i in order:
        e = int(ends[i])
        assert e >= 63 and e < len(data), (e, len(data))
        assert e - 63 > prev, ("windows overlap", prev, e)
        data[e - 63:e + 1] = windows[i]
        prev = e
    return data


_K = np.arange(64)
_KROT = (_K % 32).astype(np.uint32)


def window_hashes(table, data, lo, hi):
    """The rolling hash at positions lo..hi-1 of `data` (bytes before the stream are zero, as
    after the Splitter's 64 zero bytes): the closed form, vectorised."""
    T = np.asarray(table, dtype=np.uint32)
    pos = np.arange(lo, hi)
    idx = pos[:, None] - _K[None, :]
    x = np.where(idx >= 0, data[np.maximum(idx, 0)], 0)
    return np.bitwise_xor.reduce(_rotl_each(T[x], _KROT[None, :]), axis=1)


def _tz(h):
    h = np.asarray(h, dtype=np.uint32)
    low = h & (~h + np.uint32(1))
    return np.where(h == 0, 32, np.log2(np.maximum(low, 1).astype(np.float64)).astype(np.int64))


# One pool of windows per (low, exact_tz): a window's hash does not depend on where it sits, so
# every layout takes its windows from the pool in turn.
_POOL = {}
POOL = 32


def windows(table, low, exact_tz=None):
    key = (np.asarray(table).tobytes(), low, exact_tz)
    if key not in _POOL:
        _POOL[key] = zero_windows(table, POOL, low, 9000 + 100 * low + (exact_tz or 0), exact_tz)
    return _POOL[key]


def pool_for(table, bits, low):
    """The windows of a (bits, low) run: tz >= low; with low < bits exactly low trailing zeros,
    so that the exact test rejects every one of them."""
    return windows(table, low, low if low < bits else None)


def make_stream(table, n, ends, wins, bits, seed, clean=None, tries=4000):
    """n seeded random bytes with wins[i] ending at ends[i], the first draw in which no position
    of the `clean` ranges [(lo, hi), ...] other than a planted end has tz >= bits. clean=None:
    the 63 positions before every planted end."""
    ends = [int(e) for e in ends]
    if clean is None:
        clean = [(e - 63, e) for e in ends]
    keep = set(ends)
    for attempt in range(tries):
        rng = np.random.default_rng([seed, attempt])
        data = rng.integers(0, 256, n, dtype=np.uint8)
        plant(data, ends, wins)
        ok = True
        for lo, hi in clean:
            lo = max(lo, 0)
            if hi <= lo:
                continue
            bad = np.nonzero(_tz(window_hashes(table, data, lo, hi)) >= bits)[0] + lo
            if any(int(p) not in keep for p in bad):
                ok = False
                break
        if ok:
            return data
    raise AssertionError(("no clean draw", n, ends[:4], bits, seed))


# ---------------------------------------------------------------------------------------------
# A: mixed nfull in one wave
# ---------------------------------------------------------------------------------------------
def a_cases():
    """[(nfull, b, k)]: for every nfull in 1..32 and block b < nfull one even and one odd byte k
    of block b of the last strip, ordered so that neighbouring streams differ in nfull
    (nfull = 7 s mod 32 + 1 while that nfull has cases left)."""
    per = {}
    for nfull in range(1, 33):
        per[nfull] = []
        for b in range(nfull):
            ke = 2 * ((nfull + 11 * b) % 32)
            ko = 2 * ((nfull + 11 * b + 13) % 32) + 1
            per[nfull] += [(nfull, b, ke), (nfull, b, ko)]
    out, s = [], 0
    while any(per.values()):
        nfull = (7 * s) % 32 + 1
        s += 1
        if per[nfull]:
            out.append(per[nfull].pop(0))
    return out


def _last_strip_stream(table, pool, i, nfull, b, k, m, bits, seed, rem=0):
    n = STRIP * m + 64 * nfull + rem
    end = STRIP * m + 64 * b + k
    return make_stream(table, n, [end], [pool[i % len(pool)]], bits, seed), [end]


def layout_a(table, bits, low, seed=1):
    """About 1,100 streams; returns (streams, ends, cases) with cases[i] = (nfull, b, k) or None
    for the full streams put in between."""
    pool = pool_for(table, bits, low)
    streams, ends, cases = [], [], []
    rng = np.random.default_rng([seed, 77])
    for i, (nfull, b, k) in enumerate(a_cases()):
        if i % 25 == 12:   # a full stream of 1..3 strips, no window
            streams.append(rng.integers(0, 256, STRIP * (1 + i % 3), dtype=np.uint8))
            ends.append([])
            cases.append(None)
        m = 1 if b == 0 else (nfull + b) % 2
        d, e = _last_strip_stream(table, pool, i, nfull, b, k, m, bits, [seed, 1, i])
        streams.append(d)
        ends.append(e)
        cases.append((nfull, b, k))
    return streams, ends, cases


# ---------------------------------------------------------------------------------------------
# B: every byte of the last block
# ---------------------------------------------------------------------------------------------
B_NFULL = (1, 2, 3, 4, 5, 6, 7, 8, 31, 32)


def b_cases():
    return [(nfull, nfull - 1, k) for k in range(64) for nfull in B_NFULL]


def layout_b(table, bits, low, seed=2):
    pool = pool_for(table, bits, low)
    streams, ends, cases = [], [], []
    for i, (nfull, b, k) in enumerate(b_cases()):
        m = 1 if nfull == 1 else k % 2
        d, e = _last_strip_stream(table, pool, i, nfull, b, k, m, bits, [seed, 2, i])
        streams.append(d)
        ends.append(e)
        cases.append((nfull, b, k))
    return streams, ends, cases


# ---------------------------------------------------------------------------------------------
# C: tails and the final flush. Windows have exactly bits + 3 trailing zeros: level 3.
# ---------------------------------------------------------------------------------------------
C_REM = (1, 2, 31, 63)
C_N = (0, 1, 31)
C_LEVEL = 3
C_CLOSE_MIN = 256


def layout_c_tails(table, bits, seed=3):
    """min_size = 64. One stream per tail offset t < rem of 2048 m + 64 n + rem bytes, the
    window ending at that offset (t = rem - 1: the stream's last byte, a final chunk of at least
    MinSize that the per-byte rule emits), and one with rem = 0 per n, ending on the last byte.
    cases[i] = (rem, n, t)."""
    pool = windows(table, bits, bits + C_LEVEL)
    streams, ends, cases = [], [], []
    i = 0
    for rem in (0,) + C_REM:
        for n in C_N:
            m = 1 if n == 0 else (1 + rem + n) % 2
            for t in (range(rem) if rem else [-1]):
                size = STRIP * m + 64 * n + rem
                end = STRIP * m + 64 * n + t
                streams.append(make_stream(table, size, [end], [pool[i % len(pool)]], bits,
                                           [seed, 3, i]))
                ends.append([end])
                cases.append((rem, n, t))
                i += 1
    return streams, ends, cases


def layout_c_close(table, bits, seed=4):
    """min_size = C_CLOSE_MIN. For rem in {0} + C_REM and every n two streams whose last byte
    ends a window: "long", the only window, so the final chunk is at least MinSize and the
    per-byte rule emits it; "short", with one more window ending 128 bytes earlier, a boundary,
    so the final chunk is 128 bytes, below MinSize, and Close emits it with the level of the
    hash at the last byte. cases[i] = (rem, n, "long" | "short")."""
    pool = windows(table, bits, bits + C_LEVEL)
    streams, ends, cases = [], [], []
    i = 0
    for rem in (0,) + C_REM:
        for n in C_N:
            size = STRIP * (1 + (rem + n) % 2) + 64 * n + rem
            last = size - 1
            for kind in ("long", "short"):
                e = [last] if kind == "long" else [last - 128, last]
                clean = [(x - C_CLOSE_MIN + 1, x) for x in e]
                w = [pool[(i + j) % len(pool)] for j in range(len(e))]
                streams.append(make_stream(table, size, e, w, bits, [seed, 4, i], clean))
                ends.append(e)
                cases.append((rem, n, kind))
                i += 1
    return streams, ends, cases


# ---------------------------------------------------------------------------------------------
# D: the slot limit (kSlotCap = 4 candidates per strip go through slots)
# ---------------------------------------------------------------------------------------------
D_COUNTS = (0, 3, 4, 5, 6, 31)   # planted windows in full strips 0..5
D_SHORT = 593                    # the stream's last, short strip (9 blocks and 17 bytes) ...
D_SHORT_COUNT = 5                # ... holds 5 (and the forced final candidate)


def _d_ends(counts, short, short_count):
    ends = []
    for j, c in enumerate(counts):
        s = STRIP * j
        if c == 31:
            ends += [s + 64 * i + 63 for i in range(31)]
        elif c:
            gap = (STRIP - 100) // c | 1
            ends += [s + 90 + gap * i for i in range(c)]
    s = STRIP * len(counts)
    ends += [s + 80 + 100 * i for i in range(short_count)]
    return STRIP * len(counts) + short, ends


def layout_d(table, bits, low, seed=5):
    """One stream; no position of it but the planted ends has tz >= bits. Returns (streams,
    ends, per_strip) with per_strip[j] = planted ends in strip j."""
    n, ends = _d_ends(D_COUNTS, D_SHORT, D_SHORT_COUNT)
    pool = pool_for(table, bits, low)
    w = [pool[i % len(pool)] for i in range(len(ends))]
    d = make_stream(table, n, ends, w, bits, [seed, 5], clean=[(0, n)])
    return [d], [ends], list(D_COUNTS) + [D_SHORT_COUNT]


def layout_d_control(table, bits, low, seed=6):
    """The same shape with at most 4 planted windows per strip (none goes to k_rescan)."""
    counts = (0, 3, 4, 4, 2, 4)
    n, ends = _d_ends(counts, D_SHORT, 3)   # 3 and the forced final candidate: 4
    pool = pool_for(table, bits, low)
    w = [pool[i % len(pool)] for i in range(len(ends))]
    d = make_stream(table, n, ends, w, bits, [seed, 6], clean=[(0, n)])
    return [d], [ends], list(counts) + [3]


# ---------------------------------------------------------------------------------------------
# E: tile heads and tile ends, streaming
# ---------------------------------------------------------------------------------------------
E_TILES = 70
E_WRITES = (1, 7, 100, 4096, 32768)


def write_sizes(n, seed):
    """Write sizes from E_WRITES by a seeded generator, summing to n."""
    rng = np.random.default_rng([seed, 99])
    out, left = [], n
    while left:
        k = min(int(rng.choice(E_WRITES)), left)
        out.append(k)
        left -= k
    return out


E_HELPER_GAPS = (1023, 1024, 700, 1500, 1025, 300)


def layout_e(table, bits, low, tile, helpers=False, seed=7):
    """One stream of E_TILES tiles and a bit: tile j >= 1 holds a window with
    s = (j - 1) mod 65 bytes in tile j - 1 (s = 0: it starts at the tile's first byte; 64: it
    ends on tile j - 1's last byte). helpers (for min_size = 1024): one more window ends
    E_HELPER_GAPS[j mod 6] bytes before each of those ends, in tile j - 1, so the end at the
    tile head is dropped or kept according to the open chunk's start carried over the boundary.
    Returns (streams, ends, tile, writes, heads) with heads = [(end, s)], the windows at the
    tile heads."""
    n = E_TILES * tile + 777
    heads = [(j * tile - (j - 1) % 65 + 63, (j - 1) % 65) for j in range(1, E_TILES)]
    ends = [e for e, _ in heads]
    if helpers:
        ends += [e - E_HELPER_GAPS[j % 6] for j, (e, _) in enumerate(heads, 1)]
    pool = pool_for(table, bits, low)
    w = [pool[i % len(pool)] for i in range(len(ends))]
    d = make_stream(table, n, ends, w, bits, [seed, 7, tile])
    assert n % tile and (n - 777) % tile == 0
    return [d], [sorted(ends)], tile, write_sizes(n, seed + tile), heads


# ---------------------------------------------------------------------------------------------
# F: exact MinSize spacing
# ---------------------------------------------------------------------------------------------
F_GAPS_128 = [128, 127, 127, 129, 127, 128, 128, 127, 255, 256, 64, 64, 64, 191, 192]
F_GAPS_1024 = [1024, 1023, 1025, 512, 511, 513, 1023, 512, 512, 1024, 511, 513, 1025]


def layout_f(table, bits, low, min_size, seed=8):
    """One stream whose planted ends follow each other at the gaps of F_GAPS_128 x 20
    (min_size = 128) or F_GAPS_1024 x 8 (min_size = 1024)."""
    gaps = F_GAPS_128 * 20 if min_size == 128 else F_GAPS_1024 * 8
    ends = list(200 + np.cumsum(gaps))
    n = int(ends[-1]) + 500
    pool = pool_for(table, bits, low)
    w = [pool[i % len(pool)] for i in range(len(ends))]
    rng = np.random.default_rng([seed, 8, min_size])
    d = plant(rng.integers(0, 256, n, dtype=np.uint8), ends, w)
    return [d], [[int(e) for e in ends]]


# ---------------------------------------------------------------------------------------------
# What the oracle says
# ---------------------------------------------------------------------------------------------
def candidate_positions(oracle, table, stream, bits):
    """Positions of `stream` whose rolling hash has at least `bits` trailing zeros."""
    if len(stream) == 0:
        return np.zeros(0, dtype=np.int64)
    return np.nonzero(_tz(oracle.rolling_sums(table, stream)) >= bits)[0]


def expected_candidates(oracle, table, stream, bits):
    """Counters::ncand (Engine.candidates) for one stream of a batch run: refine_strip's exact
    pass emits one candidate for every position whose hash has tz >= Bits (hit blocks and the
    tail alike, whatever MinSize is), and one more, forced, at the last byte of a non-empty
    stream for Splitter.Close's flush: that one is emitted besides the per-byte candidate when
    the last byte's hash qualifies too, so the sum is a plain count plus one. tz is at most 32
    (a zero hash), so Bits > 32 leaves the forced candidate alone."""
    n = len(stream)
    return int(len(candidate_positions(oracle, table, stream, bits))) + (1 if n else 0)


def greedy_walk(cands, n, min_size):
    """hashsplit's MinSize rule over sorted candidate positions: a candidate is a boundary if
    the chunk it would end has at least min_size bytes; the stream's last byte always is.
    Returns the chunks' last bytes."""
    out, last = [], 0   # last: start of the open chunk
    for p in cands:
        if int(p) + 1 - last >= min_size:
            out.append(int(p))
            last = int(p) + 1
    if last < n:
        out.append(n - 1)
    return out


def chunk_ends(chunks):
    return [int(c["offset"]) + int(c["len"]) - 1 for c in chunks]


# ---------------------------------------------------------------------------------------------
# Chunks of chosen levels (the tree tests): 64-byte windows written back to back
# ---------------------------------------------------------------------------------------------
# At MinSize 64 a stream made of planted 64-byte windows written back to back is cut into exactly
# those windows: every other position lies less than MinSize after the previous boundary, so
# chunk i is window i, 64 bytes, with level tz(hash(window i)) - Bits.
#
# A window with a chosen hash is built, not searched. Bytes i and i + 32 of a window are rotated
# alike (k = 63 - i and k - 32), so a window whose two halves are equal hashes to 0 (tz = 32).
# Replacing bytes 31, 63 by (a, b) and bytes 31 - r, 63 - r by (c, d) gives
#   h = (T[a] ^ T[b]) ^ rotl(T[c] ^ T[d], r),
# and among the 32,640 x 32,640 x 31 choices some pair meets any 32-bit target (found by lookup).
_LEVEL_POOL = {}
LEVEL_POOL = 2                    # distinct windows per level


def _pair_xors(T):
    a, b = np.triu_indices(256, 1)
    d = T[a] ^ T[b]
    order = np.argsort(d, kind="stable")
    return d[order], a[order].astype(np.uint8), b[order].astype(np.uint8)


def window_with_hash(table, target, seed):
    """One 64-byte window whose window hash is exactly `target`."""
    T = np.asarray(table, dtype=np.uint32)
    rng = np.random.default_rng([4242, int(target), seed])
    half = rng.integers(0, 256, 32, dtype=np.uint8)
    w = np.concatenate([half, half])
    if target == 0:
        return w
    d, a, b = _pair_xors(T)
    for r in rng.permutation(np.arange(1, 32)):
        want = np.uint32(target) ^ _rotl(d, int(r))      # T[a] ^ T[b] for every (c, d)
        at = np.searchsorted(d, want)
        hit = np.nonzero(d[np.minimum(at, len(d) - 1)] == want)[0]
        if len(hit):
            j = int(hit[rng.integers(0, len(hit))])
            i = int(at[j])
            w[31], w[63] = a[i], b[i]
            w[31 - r], w[63 - r] = a[j], b[j]
            return w
    raise AssertionError(("no window", hex(int(target))))


def level_windows(table, bits, levels):
    """{level: [LEVEL_POOL, 64] uint8}: distinct windows whose hash has exactly bits + level
    trailing zeros (a zero hash, tz = 32, for level 32 - bits), for every level in `levels`."""
    out = {}
    for lv in sorted(set(int(x) for x in levels)):
        tz = bits + lv
        assert 0 <= lv and tz <= 32, (bits, lv)
        key = (np.asarray(table).tobytes(), tz)
        if key not in _LEVEL_POOL:
            rng = np.random.default_rng([77, tz])
            wins = []
            while len(wins) < LEVEL_POOL:
                # any odd multiple of 2^tz has exactly tz trailing zeros
                odd = int(rng.integers(0, 1 << (31 - tz))) * 2 + 1 if tz < 31 else 1
                target = (odd << tz) & 0xFFFFFFFF if tz < 32 else 0
                w = window_with_hash(table, target, len(wins))
                h = window_hashes(table, w, 63, 64)
                assert int(_tz(h)[0]) == tz, (tz, hex(int(h[0])))
                if not any((w == x).all() for x in wins):
                    wins.append(w)
            _LEVEL_POOL[key] = np.stack(wins)
        out[lv] = _LEVEL_POOL[key]
    return out


def level_stream(table, bits, levels):
    """A stream that Bits = bits / MinSize = 64 cuts into len(levels) chunks of 64 bytes, chunk i
    of level levels[i]: the level's windows from the pool in turn, back to back."""
    levels = np.asarray(levels, dtype=np.int64)
    pool = level_windows(table, bits, np.unique(levels))
    out = np.zeros((len(levels), 64), dtype=np.uint8)
    for lv, wins in pool.items():
        at = np.nonzero(levels == lv)[0]
        out[at] = wins[np.arange(len(at)) % len(wins)]
    return out.reshape(-1)
