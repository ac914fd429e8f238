"""Small planted runs for the early chains (k_pick, k_early, k_early_fix and k_lens's match;
DESIGN §5.3), and a model of the pick rule. Shared by test_early_cases_cpu.py, which holds every
builder to its claims against the oracle, and test_gpu_early_small.py, which runs the cases on the
device with Engine.set_early_min(0). No test in here.

A case is one engine run of at most about 2 MiB at Bits = 20 / MinSize = 1024, built from a plan
per stream (make()):

    ("c", L)        L bytes that end in a planted window: a candidate at the span's last byte
    ("c", L, lv)    the same, the window's hash with exactly Bits + lv trailing zeros
    ("z", K)        K zero bytes: an all-zero window hashes to 0, so every position whose whole
                    window lies in the run is a candidate (K at a stream's start, where the bytes
                    before the stream are zeros too; K - 63 elsewhere). This moves the index of
                    every later candidate by a chosen amount.
    ("r", L)        L random bytes with no candidate (the stream's tail, the bytes before a zero
                    run)

Apart from the planted ends and the zero runs no position of a stream is a candidate: at Bits = 20
about one position per MiB is one by chance, and make() re-draws one byte next to each until none
is left (planting.make_stream re-draws the whole stream, which at a megabyte of clean range takes
too many draws). hashes() is the rolling hash of a whole stream in six numpy passes; the CPU tests
compare the candidates it finds, and the chunks planting.greedy_walk cuts from them, with the
oracle's.

The model (model_picks) restates the rule in DESIGN §5.3 and the comment above pick_key: the
candidates of a run are numbered stream by stream in position order, the forced candidate of
Splitter.Close's flush last in its stream (after the natural candidate at the same byte when the
last byte qualifies too). That is the order of the engine's candidate list: k_compact and k_rescan
write a strip's candidates in position order (refine_strip: hit blocks, the tail, the flush) at the
strip's prefix offset (cand_off), and strips are numbered stream by stream in the order the streams
are listed (RunPlan: descs[s].strip0), wherever their bytes lie. So the model's candidate index is
the index k_pick puts in Early::top, and the tests compare it exactly.

The chunk between the neighbouring candidates c_i and c_i+1 is a sure chunk when
  * c_i-1 and c_i+1 exist and lie in c_i's stream,
  * c_i is not the forced candidate,
  * c_i lies at least MinSize after c_i-1 (a boundary wherever the open chunk began),
  * c_i+1 lies at least MinSize after c_i, or is the forced candidate.
The picks are the two largest (blocks, i) among sure chunks of at least `floor` = 1,024 SHA-256
blocks, largest first.
"""
import numpy as np

import planting as P
import sha_edges as E

BITS, MIN = 20, 1024
FLOOR = 1024                      # kLongMinBlocks
GRID = 64 * 1024                  # k_pick's threads for up to 4 M candidates: 64 x 1024
SLACK = 256                       # BSG_READ_SLACK


# ---------------------------------------------------------------------------------------------
# The rolling hash of a whole stream, and streams from plans
# ---------------------------------------------------------------------------------------------
def _rotl(x, r):
    r %= 32
    return x if r == 0 else ((x << np.uint32(r)) | (x >> np.uint32(32 - r))).astype(np.uint32)


def hashes(table, data):
    """The window hash at every position of `data` (zeros before the stream): with
    H_m(p) = XOR_{k<m} rotl(T[x[p-k]], k), H_2m(p) = H_m(p) ^ rotl(H_m(p-m), m)."""
    T = np.asarray(table, dtype=np.uint32)
    h = T[np.concatenate([np.zeros(64, dtype=np.uint8), np.asarray(data, dtype=np.uint8)])]
    m = 1
    while m < 64:
        nxt = h.copy()
        nxt[m:] ^= _rotl(h[:-m], m)
        h, m = nxt, 2 * m
    return h[64:]


def cand_mask(h, bits):
    return (h & np.uint32((1 << bits) - 1)) == 0 if bits < 32 else h == 0


def _window(table, bits, k, lv=None):
    if lv is None:
        pool = P.windows(table, bits)
        return pool[k % len(pool)]
    pool = P.level_windows(table, bits, [lv])[lv]
    return pool[k % len(pool)]


def make(table, plan, seed, bits=BITS):
    """The stream of `plan` (see the module docstring). Returns (bytes, planned candidate
    positions in order, without the forced one)."""
    parts, ends, zeros, wins, o = [], [], [], [], 0
    for k, seg in enumerate(plan):
        kind, n = seg[0], int(seg[1])
        rng = np.random.default_rng([seed, k])
        if kind == "z":
            assert n >= 64
            parts.append(np.zeros(n, dtype=np.uint8))
            zeros.append((o, o + n))
        else:
            d = rng.integers(0, 256, n, dtype=np.uint8)
            if kind == "c":
                assert n >= 128, seg
                d[n - 64:] = _window(table, bits, len(ends), seg[2] if len(seg) > 2 else None)
                wins.append((o + n - 64, o + n))
                ends.append(o + n - 1)
            else:
                assert kind == "r"
            parts.append(d)
        o += n
    data = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    planned = set(ends)
    for lo, hi in zeros:
        planned.update(range(lo if lo == 0 else lo + 63, hi))
    fixed = wins + zeros            # byte ranges a repair leaves alone
    rng = np.random.default_rng([seed, 9999])
    h = hashes(table, data)
    for _ in range(200):
        got = np.nonzero(cand_mask(h, bits))[0]
        stray = [int(p) for p in got if int(p) not in planned]
        missing = planned.difference(int(p) for p in got)
        assert not missing, ("planted candidate lost", sorted(missing)[:4])
        if not stray:
            return data, sorted(planned)
        p = stray[0]
        q = next(q for q in range(p, max(p - 64, -1), -1)
                 if not any(lo <= q < hi for lo, hi in fixed))
        data[q] = rng.integers(0, 256)
        h[q:q + 64] = P.window_hashes(table, data, q, min(q + 64, len(data)))
    raise AssertionError("stray candidates left")


# ---------------------------------------------------------------------------------------------
# The model
# ---------------------------------------------------------------------------------------------
def run_candidates(cands, lens):
    """The run's candidate list: [(stream, position, forced)], stream by stream in position
    order, the forced candidate at the last byte of every non-empty stream last."""
    out = []
    for s, (c, n) in enumerate(zip(cands, lens)):
        out += [(s, int(p), False) for p in c]
        if n:
            out.append((s, int(n) - 1, True))
    return out


def sure_chunk(flat, i, min_size):
    """(stream, start, length) of the chunk between candidates i and i + 1 if it is a sure
    chunk, else None."""
    if i < 1 or i + 1 >= len(flat):
        return None
    (sp, pp, _), (s, p, forced), (sn, pn, fn) = flat[i - 1], flat[i], flat[i + 1]
    if sp != s or sn != s or forced:
        return None
    if p - pp < min_size:
        return None
    if pn - p < min_size and not fn:
        return None
    if pn == p:                    # the flush behind a natural candidate at the last byte
        return None
    return s, p + 1, pn - p


def model_picks(cands, lens, min_size=MIN, floor=FLOOR, slots=2):
    """[(blocks, candidate index, record index)]: the picks of a run whose stream s has the
    natural candidates cands[s] and lens[s] bytes, largest first; the record index is the
    chunk's place in the run's records (stream by stream, planting.greedy_walk's chunks)."""
    flat = run_candidates(cands, lens)
    keys = []
    for i in range(len(flat)):
        ch = sure_chunk(flat, i, min_size)
        if ch and E.nblocks(ch[2]) >= floor:
            keys.append((E.nblocks(ch[2]), i, ch))
    keys.sort(reverse=True)
    first, ends = [], []
    for c, n in zip(cands, lens):
        first.append(sum(len(e) for e in ends))
        ends.append(P.greedy_walk(c, n, min_size))
    out = []
    for blocks, i, (s, start, length) in keys[:slots]:
        k = ends[s].index(start + length - 1)
        assert k > 0 and ends[s][k - 1] == start - 1, ("a sure chunk is no chunk", s, start, length)
        out.append((blocks, i, first[s] + k))
    return out


def brute_picks(cands, lens, min_size, floor, slots=2):
    """The same from the definition, chunk by chunk: a chunk of the greedy walk that lies between
    two neighbouring candidates of its stream, whose start is a candidate that has an earlier one
    in the stream and stays a boundary when the walk is started afresh behind any earlier
    candidate, and whose end stays one in the same way or is the flush of the stream's end (not a
    natural candidate there). Quadratic: for small streams."""
    def stays(c, j):               # candidate j of c is cut by the walk begun behind any earlier one
        for k in range(j):
            last = int(c[k]) + 1
            for p in c[k + 1:j + 1]:
                if int(p) + 1 - last >= min_size:
                    if int(p) == int(c[j]):
                        break
                    last = int(p) + 1
            else:
                return False
        return True

    keys, base, rec = [], 0, 0
    for s, (c, n) in enumerate(zip(cands, lens)):
        c = [int(p) for p in c]
        ends = P.greedy_walk(c, n, min_size)
        for k in range(1, len(ends)):
            start, end = ends[k - 1] + 1, ends[k]
            j = c.index(start - 1)          # every boundary but the flush is a candidate
            if j < 1 or not stays(c, j):
                continue
            if j + 1 < len(c):
                if c[j + 1] != end or not stays(c, j + 1):
                    continue
            elif end != n - 1:
                continue
            blocks = E.nblocks(end + 1 - start)
            if blocks >= floor:
                keys.append((blocks, base + j, rec + k))
        base += len(c) + (1 if n else 0)
        rec += len(ends)
    return sorted(keys, reverse=True)[:slots]


# ---------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------
class Case:
    """streams: the bytes; off: where stream s lies in the run's buffer (16-byte aligned);
    cands: the planned natural candidates per stream; longs: [(stream, start, length, sure)] for
    every chunk the case is about; picks: the intended picks as indices into longs, slot 0
    first; note: what a test of one family needs besides."""

    def __init__(self, name, plans, seed, off=None, note=None):
        self.name, self.plans, self.seed, self.note = name, plans, seed, note or {}
        self.bits, self.min_size = BITS, MIN
        self._off = off
        self.longs, self.picks = [], []

    def build(self, table):
        made = [make(table, pl, [self.seed, s]) for s, pl in enumerate(self.plans)]
        self.streams = [d for d, _ in made]
        self.cands = [c for _, c in made]
        self.lens = [len(d) for d in self.streams]
        if self._off is None:
            self.off, o = [], 0
            for n in self.lens:
                self.off.append(o)
                o += (n + 15) & ~15
        else:
            self.off = list(self._off)
        assert all(o % 16 == 0 for o in self.off)
        return self

    def buffer(self):
        size = max(o + n for o, n in zip(self.off, self.lens)) + SLACK
        buf = np.random.default_rng([self.seed, 777]).integers(0, 256, size, dtype=np.uint8)
        for o, d in zip(self.off, self.streams):
            buf[o:o + len(d)] = d
        return buf

    def long(self, stream, seg, sure):
        """Marks segment `seg` of stream's plan as a chunk of interest; returns its index."""
        start = sum(int(x[1]) for x in self.plans[stream][:seg])
        self.longs.append((stream, start, int(self.plans[stream][seg][1]), sure))
        return len(self.longs) - 1


def L(blocks, tail=0):
    return E.length(blocks, tail)


def _c(*lens):
    return [("c", n) for n in lens]


def case_a():
    """One stream, five long chunks of distinct block counts among short ones."""
    blocks = [1210, 1705, 1333, 2050, 1499]
    plan = _c(1100, 1300)
    for i, b in enumerate(blocks):
        plan += _c(L(b, E.TAILS[i]), 1100 + 97 * i)
    plan.append(("r", 700))
    c = Case("a-basic", [plan], 11)
    ids = [c.long(0, 2 + 2 * i, True) for i in range(5)]
    c.picks = [ids[3], ids[1]]
    return [c]


def case_b():
    """The floor: 1,024 blocks (65,464 bytes, and 65,472) are picked, 1,023 (65,463) are not."""
    assert (L(1024, 56), L(1024, 0), L(1023, 55), L(1023, 0)) == (65464, 65472, 65463, 65408)
    c = Case("b-floor", [_c(1100, 1100, 65464, 1100, 65463, 1100, 65472) + [("r", 500)]], 12)
    ids = [c.long(0, 2, True), c.long(0, 4, True), c.long(0, 6, True)]
    c.picks = [ids[2], ids[0]]     # a tie at 1,024 blocks: the larger index first
    n = Case("b-below", [_c(1100, 1100, 65463, 1200, 65408) + [("r", 900)]], 13)
    n.long(0, 2, True)
    n.long(0, 4, True)
    return [c, n]


def case_c():
    """The longest chunk starts at a boundary c_i whose preceding candidate, 500 bytes after the
    last boundary and so not one itself, lies `gap` bytes before it."""
    out = []
    for gap in (MIN - 1, MIN, MIN + 1):
        plan = _c(1100, 2000, 500, gap, L(1500, 1), 1200, L(1300, 55), 1100, L(1200, 63))
        plan.append(("r", 640))
        c = Case(f"c-start-gap{gap}", [plan], 14)
        sure = gap >= MIN
        ids = [c.long(0, 4, sure), c.long(0, 6, True), c.long(0, 8, True)]
        c.picks = ids[:2] if sure else ids[1:]
        out.append(c)
    return out


def case_d():
    """A 1,500-block chunk with a candidate 700 bytes after its start: it spans two candidate
    gaps, the first too short, the second (itself above the floor) starting at no boundary."""
    whole = L(1500, 0)
    plan = _c(1100, 1200, 700, whole - 700, 1100, L(1200, 56), 1100, L(1100, 1)) + [("r", 333)]
    c = Case("d-inside", [plan], 15)
    c.note["spans"] = (0, 2300, whole)      # the real chunk: stream, start, length
    ids = [c.long(0, 3, False), c.long(0, 5, True), c.long(0, 7, True)]
    c.picks = ids[1:]
    return [c]


def case_e():
    """The forced end, the stream's first chunk, a stream of one chunk."""
    head = _c(1100, 1100, L(1100, 55), 1300)
    f = Case("e-forced", [head + [("r", L(1500, 63))]], 16)
    ids = [f.long(0, 2, True), f.long(0, 4, True)]
    f.picks = ids[::-1]
    # the last byte ends a planted window too: a natural candidate and the forced one behind it
    g = Case("e-forced-natural", [head + [("c", L(1500, 0), 3)]], 17)
    ids = [g.long(0, 2, True), g.long(0, 4, True)]
    g.picks = ids[::-1]
    g.note["double_end"] = True
    one = Case("e-one-chunk", [[("r", L(1200, 56))]], 18)
    one.long(0, 0, False)
    first = Case("e-first-longest", [_c(L(1500, 1), 1100, 1100, L(1100, 0), 1200) + [("r", 500)]],
                 19)
    ids = [first.long(0, 0, False), first.long(0, 3, True)]
    first.picks = ids[1:]
    return [f, g, one, first]


def case_f():
    """Three streams: the longest chunks are stream 1's first chunk (no pick), a middle chunk of
    stream 2 and the forced last chunk of stream 0. Stream 0 lies in the middle of the buffer,
    stream 1 at its end, stream 2 near its start, with gaps between."""
    s0 = _c(1100, 1200, 1300) + [("r", L(1300, 56))]
    s1 = _c(L(1600, 0), 1100, 2000) + [("r", 400)]
    s2 = _c(1100, 1500, L(1200, 63), 1100) + [("r", 600)]
    n = [sum(x[1] for x in s) for s in (s0, s1, s2)]
    o2 = 48
    o0 = ((o2 + n[2] + 15) & ~15) + 4096
    o1 = ((o0 + n[0] + 15) & ~15) + 272
    c = Case("f-stream-edges", [s0, s1, s2], 20, off=[o0, o1, o2])
    ids = [c.long(0, 3, True), c.long(1, 0, False), c.long(2, 2, True)]
    c.picks = [ids[0], ids[2]]
    return [c]


def case_g():
    """Three chunks of 1,100 blocks and different lengths, shorter ones beside them: the picks
    are the two of the largest candidate index. In one stream, and one in each of three."""
    t = [L(1100, 0), L(1100, 55), L(1100, 56)]
    assert len(set(t)) == 3
    one = Case("g-ties", [_c(1100, 1100, t[0], 1200, t[1], 1300, L(1050, 1), 1100, t[2])
                          + [("r", 450)]], 21)
    ids = [one.long(0, 2, True), one.long(0, 4, True), one.long(0, 6, True), one.long(0, 8, True)]
    one.picks = [ids[3], ids[1]]
    three = Case("g-ties-streams", [_c(1100, 1100, t[2], 1200) + [("r", 300)],
                                    _c(1100, 1300, L(1050, 63), 1100, t[0]) + [("r", 200)],
                                    _c(1500, 1100, t[1], 1100) + [("r", 100)]], 22)
    ids = [three.long(0, 2, True), three.long(1, 2, True), three.long(1, 4, True),
           three.long(2, 2, True)]
    three.picks = [ids[3], ids[2]]
    return [one, three]


def case_h():
    """The two longest chunks share a candidate."""
    c = Case("h-adjacent", [_c(1100, 1100, L(1500, 55), L(1400, 56), 1100, L(1100, 0))
                            + [("r", 800)]], 23)
    ids = [c.long(0, 2, True), c.long(0, 3, True), c.long(0, 5, True)]
    c.picks = ids[:2]
    return [c]


def case_i():
    one = Case("i-one", [_c(1100, 1100, L(1100, 1), 1100) + [("r", 3000)]], 24)
    one.picks = [one.long(0, 2, True)]
    none = Case("i-none", [_c(L(1200, 0), 1100, 1200, 40000) + [("r", 5000)]], 25)
    none.long(0, 0, False)
    return [one, none]


J_PAIRS = {"wave": (4200, 4210), "waves": (4200, 4400), "workgroups": (4200, 7300),
           "thread": (4200, 4200 + GRID)}


def case_j():
    """Zero runs put the start candidates of the two longest chunks, A and B, at chosen indices
    iA < iB of the candidate list; a third, slightly shorter sure chunk C starts at candidate 1.
    A is the longer one, in the mirror cases B. Thread t of k_pick's 64 x 1,024 grid sees the
    candidates i = t mod 65,536."""
    out = []
    for kind, (ia, ib) in J_PAIRS.items():
        for mirror in (False, True):
            la, lb = L(1500, 55), L(1400, 0)
            if mirror:
                la, lb = lb, la
            k0, k1 = ia + 60, ib - ia + 60
            plan = _c(1100, 1100, L(1390, 63)) + [("r", 100), ("z", k0)] + _c(1500, la, 1300) + \
                [("r", 100), ("z", k1)] + _c(1500, lb) + [("r", 500)]
            c = Case(f"j-{kind}{'-mirror' if mirror else ''}", [plan], 26)
            ids = [c.long(0, 6, True), c.long(0, 11, True), c.long(0, 2, True)]
            c.picks = ids[:2][::-1] if mirror else ids[:2]
            c.note.update(kind=kind, index=(ia, ib, 1))
            out.append(c)
    return out


K_BLOCKS = (1024, 1025, 1087, 1088, 1089, 1151, 1152, 1153)


def k_pairs():
    """Every (blocks, tail) of K_BLOCKS x TAILS once, two to a run, the two of a run with
    different block counts and tails."""
    combos = [(b, t) for b in K_BLOCKS for t in E.TAILS]
    half = len(combos) // 2
    return [(combos[i], combos[(i + half + 1) % half + half]) for i in range(half)]


def case_k():
    """k_early's chains at 16, 17 and 18 fills of 64 blocks and next to them, with every tail."""
    out = []
    for n, ((b1, t1), (b2, t2)) in enumerate(k_pairs()):
        c = Case(f"k-{b1}b{t1}-{b2}b{t2}", [_c(1100, 1100 + 3 * n, L(b1, t1), 1200, L(b2, t2))
                                            + [("r", 300 + n)]], 27)
        c.long(0, 2, True)
        c.long(0, 4, True)
        c.picks = [1, 0] if b2 >= b1 else [0, 1]
        c.note["edges"] = ((b1, t1), (b2, t2))
        out.append(c)
    return out


def case_l():
    """The picked chunks' first byte at every address residue mod 64, two per run: the filler
    chunk before each is as long as that takes."""
    out = []
    for n in range(32):
        r1, r2 = n, 63 - n
        off = 16 * (n % 4)
        la, lb = L(1030 + n, E.TAILS[n % 5]), L(1100 + n, E.TAILS[(n + 2) % 5])
        f1 = 1100 + (r1 - (off + 1100 + 1100)) % 64
        start1 = 1100 + f1
        f2 = 1200 + (r2 - (off + start1 + la + 1200)) % 64
        c = Case(f"l-residues-{r1}-{r2}", [_c(1100, f1, la, f2, lb) + [("r", 400)]], 28, off=[off])
        c.long(0, 2, True)
        c.long(0, 4, True)
        c.picks = [1, 0]
        c.note["residues"] = (r1, r2)
        out.append(c)
    return out


M_LEVELS = (0, 5, 31 - BITS)


def case_m():
    """Picked chunks that end on windows of exactly Bits + level trailing zeros (level 0, a middle
    one, and tz = 31; windows built by planting.level_windows, a search with exact_tz takes 2^32
    draws at tz = 31), and a picked forced final chunk."""
    lv = M_LEVELS
    a = Case("m-levels", [[("c", 1100), ("c", 1200), ("c", L(1300, 1), lv[0]), ("c", 1100),
                           ("c", L(1400, 56), lv[1]), ("r", 600)]], 29)
    a.long(0, 2, True)
    a.long(0, 4, True)
    a.picks = [1, 0]
    a.note["levels"] = (lv[0], lv[1])
    b = Case("m-level-top-forced", [[("c", 1100), ("c", 1200, 2), ("c", L(1250, 63), lv[2]),
                                     ("c", 1100), ("r", L(1200, 0))]], 30)
    b.long(0, 2, True)
    b.long(0, 4, True)
    b.picks = [0, 1]
    b.note["levels"] = (lv[2], None)
    return [a, b]


FAMILIES = {"a": case_a, "b": case_b, "c": case_c, "d": case_d, "e": case_e, "f": case_f,
            "g": case_g, "h": case_h, "i": case_i, "j": case_j, "k": case_k, "l": case_l,
            "m": case_m}
NAMES = [c.name for f in FAMILIES.values() for c in f()]
_BUILT = {}


def get(table, name):
    """The built case `name` (built once per session)."""
    if name not in _BUILT:
        for f in FAMILIES.values():
            for c in f():
                if c.name == name:
                    _BUILT[name] = c.build(table)
    return _BUILT[name]


def intended(case):
    """The intended picks as (stream, start, length), slot 0 first."""
    return [case.longs[k][:3] for k in case.picks]


_EXPECT = {}


def expect(case, oracle, table):
    """What a run of `case` must give, from the oracle alone (computed once per session):
    records [(offset, len, level, ref hex, stream)] stream by stream, counts per stream, the
    candidate count, and the model's picks over the oracle's candidates."""
    if case.name not in _EXPECT:
        recs, counts, cands = [], [], []
        for s, d in enumerate(case.streams):
            ch = oracle.split(table, d, bits=case.bits, min_size=case.min_size)
            recs += [(int(c["offset"]), int(c["len"]), int(c["level"]), bytes(c["ref"]).hex(), s)
                     for c in ch]
            counts.append(len(ch))
            cands.append(P.candidate_positions(oracle, table, d, case.bits))
        ncand = sum(len(c) + (1 if n else 0) for c, n in zip(cands, case.lens))
        _EXPECT[case.name] = {"records": recs, "counts": counts, "ncand": ncand, "cands": cands,
                              "picks": model_picks(cands, case.lens, case.min_size)}
    return _EXPECT[case.name]
