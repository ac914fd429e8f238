"""tests/tier_cases.py held to its claims (no GPU): what keeps test_gpu_tier_counts.py from
passing vacuously.

For every case the model at waves = 1024 gives exactly the counts the case states as literals
(derived by hand in tier_cases.py), the launch is on the light or loaded side it claims, and the
jobs the case is about sit on the side of the threshold it names. The model is checked once
against a second, bucket-by-bucket restatement of k_bucket_scan over all 4,096 buckets on random
censuses, at several wave counts and under every long mode. The builders give distinct (off, len)
pairs at 16-byte offsets inside the buffer with its slack behind them, and the split cases'
records land exactly on the slot counts they name."""
import numpy as np
import pytest

import sha_edges as E
import tier_cases as T

WAVES = 1024


def test_constants_and_waves():
    c = T.constants()
    assert T.waves() == c["waves_per_cu"] * c["num_cus"] == WAVES, "literals are for 256 CUs"
    assert T.grid_slots() == 262_144
    assert T.waves(304) == 1216
    # what the cases' hand derivations use
    assert (c["kSolo"], c["kGroup"], c["kPairGroup"], c["kLongMinBlocks"], c["kLptBuckets"]) == \
        (16, 8, 32, 1024, 4096)
    assert (c["BSG_TLEN_PCT"], c["BSG_TLEN_PCT_LIGHT"], c["BSG_PAIR_PCT"],
            c["BSG_PAIR_PCT_LIGHT"]) == (55, 48, 34, 30)


def test_names():
    assert [c.name for c in T.cases()] == T.NAMES and len(set(T.NAMES)) == len(T.NAMES)


@pytest.mark.parametrize("name", T.NAMES)
def test_model_gives_the_literals(name):
    c = T.get(name)
    m = T.model(c.blocks, WAVES)
    got = {k: m[k] for k in T.COUNTS}
    print(name, got, "total_blocks", m["total_blocks"], "light below",
          m["max_nblocks"] * 64 * WAVES / 10, "tlen", m["tlen"], "tlen2", m["tlen2"])
    assert got == c.want, (name, got, c.want)
    assert m["light"] == c.light, (name, m["total_blocks"], m["max_nblocks"] * 64 * WAVES / 10)
    assert m["nlong"] + m["nshort"] == len(c.blocks)
    assert m["wave_tickets"] <= WAVES // 2


def _tiers(name):
    c = T.get(name)
    m = T.model(c.blocks, WAVES)
    return c, m, {n: t for n, t in zip(c.blocks, m["tier"])}


def test_case_a_and_b_shapes():
    for n in T.A_COUNTS:
        c, m, _ = _tiers(f"A-n{n}")
        assert m["bucket_width"] == 1 and m["tlen"] == m["tlen2"] == 1024
        longs = [b for b in c.blocks if b >= 1024]
        assert len(longs) == len(set(longs)) == n and min(longs) >= 2000 and max(longs) == 2100
        assert max(b for b in c.blocks if b < 1024) <= 900
        # the long jobs lie scattered among the short ones
        assert n < 2 or max(i for i, b in enumerate(c.blocks) if b >= 1024) > n
    for p in T.B_COUNTS:
        c, m, tier = _tiers(f"B-p{p}")
        assert (m["tlen"], m["tlen2"]) == (1632, 1024)
        assert sorted(b for b in c.blocks if tier[b] == "group")[0] >= 3355
        pair = [b for b in c.blocks if tier[b] == "pair"]
        assert len(pair) == len(set(pair)) == p and 1100 <= min(pair) and max(pair) <= 1600
    # the last tickets: ragged and full
    assert (17 - 16) % 8 == 1 and (24 - 16) % 8 == 0 and 32 % 32 == 0 and 64 % 32 == 0


def test_case_c_d_e():
    c, m, tier = _tiers("C-pairs-after-3")
    assert m["tickets_grp"] == m["nlong_grp"] == 3 < T.constants()["kSolo"]
    assert m["nlong"] - m["nlong_grp"] == 5
    c, m, tier = _tiers("D-no-lane-job")
    assert m["nshort"] == 0 and set(m["tier"]) == {"group", "pair"}
    assert (m["nlong_grp"] - 16) % 8 == 0 and (m["nlong"] - m["nlong_grp"]) % 32 == 0
    for n in T.E_COUNTS:
        c, m, _ = _tiers(f"E-equal{n}")
        assert set(c.blocks) == {T.constants()["kLongMinBlocks"]} and len(c.blocks) == n
        assert m["cap"] == 3984 and m["tlen"] == 1024
    assert T.model([1024] * 3984, WAVES)["tickets_grp"] == WAVES // 2
    assert set(T.get("E-floor").blocks) == {1023}


def test_case_f_thresholds():
    c, m, tier = _tiers("F-w1")
    assert (m["bucket_width"], m["tlen"], m["tlen2"]) == (1, 1920, 1200)
    assert [tier[n] for n in (4000, 1920, 1919, 1200, 1199)] == \
        ["group", "group", "pair", "pair", "lane"]
    c, m, tier = _tiers("F-w3")
    assert (m["bucket_width"], m["tlen"], m["tlen2"]) == (3, 4800, 3000)
    assert [tier[n] for n in (4801, 4800, 4799, 4798, 4797)] == \
        ["group", "group", "group", "pair", "pair"]
    assert [tier[n] for n in (3001, 3000, 2999, 2998, 2997)] == \
        ["pair", "pair", "pair", "lane", "lane"]


def test_case_g_load():
    loaded, light = T.get("G-loaded"), T.get("G-light")
    ml, mt = T.model(loaded.blocks, WAVES), T.model(light.blocks, WAVES)
    edge = 2100 * 64 * WAVES          # light iff total * 10 < edge
    print("G total_blocks", ml["total_blocks"], mt["total_blocks"], "threshold", edge / 10)
    assert ml["total_blocks"] * 10 >= edge > mt["total_blocks"] * 10
    assert (ml["total_blocks"], mt["total_blocks"]) == (14_041_810, 13_041_810)
    assert (ml["tlen"], mt["tlen"]) == (1155, 1024) and ml["tlen2"] == mt["tlen2"] == 1024
    assert ml["helped"] == 0 and mt["helped"] == 16
    # the light case's pairs are the loaded case's, so the host hashes them once
    assert set(zip(light.off, light.lens)) <= set(zip(loaded.off, loaded.lens))
    assert sum(loaded.lens) > 890_000_000


def test_case_h_modes():
    c = T.get("H-sort")
    assert sorted(c.blocks) == list(range(1, 2501)) and c.blocks != sorted(c.blocks)
    assert T.model(c.blocks, WAVES)["bucket_width"] == 1
    for mode, want in T.H_MODE_WANT.items():
        m = T.model(c.blocks, WAVES, long_mode=mode)
        assert {k: m[k] for k in T.COUNTS} == want, mode
    assert T.H_MODE_WANT[1]["nlong"] == 0 and T.H_MODE_WANT[2]["nlong"] == len(c.blocks)


# ---------------------------------------------------------------------------------------------
# The model against k_bucket_scan restated bucket by bucket
# ---------------------------------------------------------------------------------------------
def _scan(nb, waves, long_mode):
    """k_bucket_scan as written: all kLptBuckets buckets, inclusive prefix counts, the number of
    qualifying buckets taken as a prefix length."""
    c = T.constants()
    B = c["kLptBuckets"]
    mx, total = max(nb), sum(nb)
    w = (mx + B) // B
    e = [0] * B
    for n in nb:
        e[min((mx - n) // w, B - 1)] += 1
    light = total * 10 < mx * 64 * waves
    tlen = max(mx * (c["BSG_TLEN_PCT_LIGHT"] if light else c["BSG_TLEN_PCT"]) // 100,
               total * 9 // (640 * waves), c["kLongMinBlocks"])
    cap = c["kSolo"] + c["kGroup"] * max(waves // 2 - c["kSolo"], 0)
    if long_mode == 2:
        tlen, cap = 0, 1 << 62
    e, incl, b = np.array(e), np.cumsum(e), np.arange(B)
    top = np.maximum(mx - b * w, 0)
    nlb8 = int(((top >= tlen) & (incl <= cap)).sum()) if long_mode != 1 else 0
    n8 = int(e[:nlb8].sum())
    t8 = n8 if n8 <= c["kSolo"] else c["kSolo"] + -(-(n8 - c["kSolo"]) // c["kGroup"])
    nlb = nlb8
    if long_mode == 0:
        tlen2 = max(mx * (c["BSG_PAIR_PCT_LIGHT"] if light else c["BSG_PAIR_PCT"]) // 100,
                    c["kLongMinBlocks"])
        cap2 = max(waves // 2 - t8, 0) * c["kPairGroup"]
        nlb += int(((b >= nlb8) & (top >= tlen2) & (incl - n8 <= cap2)).sum())
    nlong = int(e[:nlb].sum())
    helped = min(n8, c["kSolo"], waves // 2) if light and long_mode == 0 else 0
    return dict(zip(T.COUNTS, (n8, t8, helped, nlong, len(nb) - nlong,
                               t8 + -(-(nlong - n8) // c["kPairGroup"]))))


@pytest.mark.parametrize("waves", [1024, 1216, 64, 16])
def test_model_equals_the_bucket_scan(waves):
    rng = np.random.default_rng(waves)
    for k in range(60):
        mx = int(rng.choice([700, 1024, 1500, 4095, 4096, 9000, 40_000]))
        n = int(rng.choice([1, 5, 40, 700, 6000]))
        nb = rng.integers(1, mx + 1, n).tolist()
        if k % 3 == 0:                       # many equal jobs near the top: the caps
            nb += [mx - int(x) for x in rng.integers(0, 4, int(rng.choice([20, 600, 5000])))]
        for mode in (0, 1, 2):
            m = T.model(nb, waves, long_mode=mode)
            assert {key: m[key] for key in T.COUNTS} == _scan(nb, waves, mode), (k, mode, mx, n)
    for name in T.NAMES:
        c = T.get(name)
        assert T.get(name).want == _scan(c.blocks, 1024, 0), name


# ---------------------------------------------------------------------------------------------
# The builders
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.NAMES)
def test_layout(name):
    c = T.get(name)
    off, lens = np.array(c.off), np.array(c.lens)
    assert len(off) == len(lens) == len(c.blocks)
    assert [E.nblocks(n) for n in c.lens] == c.blocks
    assert (off % 16 == 0).all() and (lens > 0).all()
    assert int((off + lens).max()) <= T.BUF_BYTES
    assert T.buffer().size == T.BUF_BYTES + T.READ_SLACK
    assert len(set(zip(c.off, c.lens))) == len(c.blocks)
    # wave jobs start at every 16-byte residue of a 64-byte line
    if sum(b >= 1024 for b in c.blocks) >= 16:
        assert {o % 64 for o, b in zip(c.off, c.blocks) if b >= 1024} == {0, 16, 32, 48}


def test_refs_are_hashlibs_and_cached():
    import hashlib
    c = T.get("F-w1")
    want = [hashlib.sha256(bytes(T.buffer()[o:o + n])).digest() for o, n in zip(c.off, c.lens)]
    assert c.refs() == want and len(set(want)) == len(want)
    assert c.refs() is not None and all((o, n) in T._REFS for o, n in zip(c.off, c.lens))
    assert not T.buffer().flags.writeable


@pytest.mark.parametrize("passes", T.I_PASSES)
def test_split_slots(oracle, table, passes):
    """Case I: records + streams = passes * 4 * CUs * 256 + 1, the stream ends at a chunk end."""
    data, recs = T.slots_stream(oracle, table, passes)
    assert len(recs) + 1 == passes * 262_144 + 1
    assert int(recs["offset"][-1] + recs["len"][-1]) == data.size
    nb = [E.nblocks(n) for n in recs["len"]]
    m = T.model(nb, WAVES)
    print("I", passes, "bytes", data.size, "max_nblocks", m["max_nblocks"])
    assert m["nlong"] == 0 and m["nshort"] == len(recs)


def test_planted_run(oracle, table):
    """Case J: the oracle cuts the streams into exactly the planned lengths."""
    streams, lens = T.planted_run()
    nb = []
    for d, want in zip(streams, lens):
        got = oracle.split(table, d, bits=T.J_BITS, min_size=T.J_MIN)["len"].tolist()
        assert got == want
        nb += [E.nblocks(n) for n in got]
    assert sorted(nb)[-3:] == sorted(T.J_LONG) and sorted(nb)[-4] <= 900
    m = T.model(nb, WAVES)
    assert {k: m[k] for k in T.COUNTS} == T.J_WANT and m["light"]
