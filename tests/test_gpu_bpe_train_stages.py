"""GPU: the BPE trainer's two device stages (csrc/bpe_train_kernels.hip) called
directly, against the restatement of the reference (tests/bpe_train_ref.py).
Every comparison is exact integer equality.

* spm_hip_bpe_pair_census: all seven views equal census() -- equal-char runs
  across the 64- and 256-lane edges, every UTF-8 class and malformed form,
  degenerate batches and the 65536-char limit of EncodePos.
* spm_hip_bpe_refresh_create / _run on hand-built states: chains of
  overlapping (a, a) positions placed against the 64-entry chunks of
  refresh_freq_kernel, dead and invalid entries, the link conditions, todo
  list shapes, every kind of insert, growth of the entry buffers and repeated
  calls.  A Mirror holds the same sets on the host and advances them with the
  restatement's compute_freq.
* the same entry points in lockstep with the restatement's merge loop, fed
  with the change log include/spm_hip.h describes, compared at every
  UpdateActiveSymbols.

The erased positions come back in no fixed order (they are appended with
atomics): they are compared as sorted (symbol, position) lists.
"""
import random

import numpy as np
import pytest

import bpe_train_ref as B
import spm_amd as S

pytestmark = pytest.mark.gpu

A, Bc = 0, 1  # symbol ids of the two chars in the hand-built states
F40 = 1 << 40


# ----------------------------------------------------------------- census

def check_census(sents, freqs):
    got = S.bpe_pair_census(sents, freqs)
    want = B.census(sents, freqs)
    for f in B.CENSUS_FIELDS:
        assert got[f].dtype == want[f].dtype, f
        assert got[f].shape == want[f].shape, (f, got[f].shape, want[f].shape)
        assert np.array_equal(got[f], want[f]), f
    return want


def random_corpus(seed, n, alphabet):
    rng = random.Random(seed)
    sents = []
    for i in range(n):
        k = rng.choice([0, 1, 1, 2, 3, 5, 8, 13]) if i % 3 else rng.randint(0, 12)
        sents.append("".join(rng.choice(alphabet) for _ in range(k)).encode())
    return sents, [rng.choice([1, 2, F40]) for _ in range(n)]


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 600])
@pytest.mark.parametrize("alphabet", ["ab", "abc", "aé猫😀"])
def test_census_random_corpora(n, alphabet):
    """One sentence per lane, 256 lanes a block: 255 / 256 / 257 / 600
    sentences; empty and one-char sentences mixed in; freqs of 1, 2 and 2^40
    (a 32-bit sum would show)."""
    sents, freqs = random_corpus(1000 + n, n, alphabet)
    if n >= 255:
        assert b"" in sents and any(len(B.utf8_to_unicode(s)) == 1 for s in sents)
    want = check_census(sents, freqs)
    if n >= 255:
        assert int(want["pair_freq"].max()) > 1 << 41


RUN_LENGTHS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 129, 1000]


@pytest.mark.parametrize("a,b", [("a", "b"), ("猫", "b"), ("😀", "é")])
def test_census_equal_char_runs(a, b):
    """Runs of one char of length k, alone in a sentence and with another
    char before, after and inside ("baaaa", "aaaab", "aabaaa"): the kept
    positions are the even offsets from each run's start."""
    sents = []
    for k in RUN_LENGTHS:
        sents += [(a * k).encode(), (b + a * k).encode(), (a * k + b).encode(), (a * 2 + b + a * k).encode()]
    freqs = [1 + (i % 3) for i in range(len(sents))]
    want = check_census(sents, freqs)
    # By hand for the run alone: ceil((k - 1) / 2) kept positions.
    ca = ord(a)
    k_aa = want["pair_keys"].tolist().index(ca << 21 | ca)
    off = want["pair_pos_offsets"].tolist()
    kept = want["pair_positions"].tolist()[off[k_aa]:off[k_aa + 1]]
    for j, k in enumerate(RUN_LENGTHS):
        assert sum(1 for p in kept if p >> 32 == 4 * j) == k // 2


MALFORMED = [
    b"\x80", b"a\x80b", b"\x80\x80\x80\x80\x80",            # stray continuation bytes
    b"\xc0\x80", b"\xc1\xbfz",                              # overlong 2-byte forms
    b"\xe0\x80\x80", b"\xe0\x9f\xbf",                       # overlong 3-byte forms
    b"\xf0\x80\x80\x80", b"\xf0\x8f\xbf\xbf",               # overlong 4-byte forms
    b"\xed\xa0\x80", b"\xed\xbf\xbf\xed\xa0\x80",           # surrogates
    b"\xf4\x90\x80\x80", b"\xf7\xbf\xbf\xbf", b"\xf8\x88\x80\x80\x80",  # above U+10FFFF
    b"ab\xe3\x81", b"ab\xc3", b"\xf0\x9f\x98", b"\xe7\x8c",  # truncated at the end
    "\ufffd".encode() + b"\x80\x80" + "\ufffd\ufffd".encode(),  # a real U+FFFD inside a run of them
    b"\xff\xfe\xff\xfe\xff\xfe\xff",
]


def test_census_utf8_classes():
    sents = [
        "aé猫😀".encode(), "😀猫éa".encode(), "ééé猫猫猫😀😀😀😀".encode(),
        "\U0010ffff\U0010ffff".encode(), "\U0010ffff\U0010ffff\U0010ffff\U0010ffffa".encode(),
        b"\x00", b"\x00\x00\x00", b"a\x00b\x00\x00", "\x7f\x80\u07ff\u0800\uffff\U00010000".encode(),
        # Pairs that differ in the key's top bit (bit 20 of the left char) alone, in turn.
        "\U00100061b".encode(), b"ab", "\U00100061b".encode(), b"ab",
        "\U0010ffff\U0010ffff".encode(), "\U000fffff\U0010ffff".encode(), "\U0010ffff\U0010ffff".encode(),
    ]
    want = check_census(sents, [1, 2, F40, 3, 1, 1, 2, 1, 1, 1, 2, 4, 8, 1, 2, 4])
    assert len(set(want["pair_keys"].tolist())) == len(want["pair_keys"])
    # The largest key there is: bit 41 is set, so all 42 bits have to be sorted.
    assert int(want["pair_keys"].max()) == 0x10FFFF << 21 | 0x10FFFF and int(want["pair_keys"].max()) >> 41 == 1


def test_census_malformed_utf8():
    """Each malformed byte is one U+FFFD; runs of them follow the overlap
    rule like any other char."""
    want = check_census(MALFORMED, [1 + (i % 2) * F40 for i in range(len(MALFORMED))])
    E = B.UNICODE_ERROR
    k = want["pair_keys"].tolist().index(E << 21 | E)
    off = want["pair_pos_offsets"].tolist()
    kept = want["pair_positions"].tolist()[off[k]:off[k + 1]]
    # b"\x80" * 5 (sentence 2): positions 0 and 2 of its four pairs.
    assert [p & 0xFFFFFFFF for p in kept if p >> 32 == 2] == [0 << 16 | 1, 2 << 16 | 3]


@pytest.mark.parametrize("sents", [[], [b""], [b""] * 5, [b""] * 300, [b"a"], [b"a", b"b", b"a"] * 100,
                                   [b"", b"x", b""] * 90], ids=["n0", "empty1", "empty5", "empty300", "one", "ones300",
                                                                "ones_and_empties"])
def test_census_degenerate_batches(sents):
    """No sentence, only empty sentences, only one-char sentences (chars but
    no pair record): SPM_OK, and views equal to the restatement's."""
    want = check_census(sents, [2] * len(sents))
    assert len(want["pair_keys"]) == 0 and want["pair_pos_offsets"].tolist() == [0]


def long_batch(nchars, index):
    """A sentence of nchars chars that ends in "ab" (so its last position is
    kept whatever came before) at `index` of a batch of short ones."""
    rng = random.Random(nchars)
    long = "".join(rng.choice("aab") for _ in range(nchars - 2)) + "ab"
    sents = [b"ab", b"", b"aaa", b"b"] * 100
    sents.insert(index, long.encode())
    return sents, [1 + (i % 2) for i in range(len(sents))]


@pytest.mark.parametrize("index", [0, 300])
def test_census_encodepos_limit(index):
    """EncodePos CHECK_LE(l, kuint16max): 65536 chars fit (the last position
    is 65534 << 16 | 65535), 65537 do not."""
    sents, freqs = long_batch(65536, index)
    want = check_census(sents, freqs)
    assert (index << 32 | 65534 << 16 | 65535) in want["pair_positions"].tolist()

    sents, freqs = long_batch(65537, index)
    with pytest.raises(S.SpmError) as e:
        S.bpe_pair_census(sents, freqs)
    assert e.value.code == S.SPM_OUT_OF_RANGE and "EncodePos" in str(e.value)
    with pytest.raises(AssertionError):
        B.census(sents, freqs)


# ------------------------------------------------- refresh, hand-built

class Mirror:
    """A BpeRefresh and its host twin: the same symbol arrays and position
    sets, advanced by the restatement.  symbols: {id: (left, right,
    positions)}; ids, left and right are ints, a merged-away char is -1."""

    def __init__(self, syms, freqs, symbols):
        self.syms = [list(r) for r in syms]
        self.freqs = list(freqs)
        self.off = [0]
        for r in self.syms:
            self.off.append(self.off[-1] + len(r))
        self.sym = {i: B.Symbol(id=i, left=l, right=r, positions=p) for i, (l, r, p) in symbols.items()}
        pos = sorted((i, n) for i, s in self.sym.items() for n in s.positions)
        self._in_bounds(n for _, n in pos)
        self.dev = S.BpeRefresh([x for r in self.syms for x in r], self.off, self.freqs, [i for i, _ in pos],
                                [n for _, n in pos])

    def _in_bounds(self, keys):
        for n in keys:
            sid, l, r = B.decode_pos(n)
            assert sid < len(self.syms) and l < len(self.syms[sid]) and r < len(self.syms[sid]), (sid, l, r)

    def close(self):
        self.dev.close()

    def run(self, writes=(), ins=(), dels=(), todo=()):
        """writes: (sid, index, value); ins / dels: (symbol, position); todo:
        symbol ids, or (id, left, right) for a symbol with no set yet.
        Returns (freqs, sorted erased) after comparing them with the device's."""
        ins = sorted(set(ins))
        self._in_bounds(n for _, n in ins)
        for t in todo:
            if not isinstance(t, int) and t[0] not in self.sym:
                self.sym[t[0]] = B.Symbol(id=t[0], left=t[1], right=t[2])
        ids = [t if isinstance(t, int) else t[0] for t in todo]
        w = [(self.off[sid] + i) << 32 | (v & 0xFFFFFFFF) for sid, i, v in writes]
        assert len(set(x >> 32 for x in w)) == len(w)
        freq, es, ek = self.dev.run(w, [s for s, _ in ins], [n for _, n in ins], [s for s, _ in dels],
                                    [n for _, n in dels], [(i, self.sym[i].left, self.sym[i].right) for i in ids])
        # The host twin, in the order the header gives: writes, erases, inserts.
        for sid, i, v in writes:
            self.syms[sid][i] = v
        for s, n in dels:
            if s in self.sym:
                self.sym[s].positions.discard(n)
        for s, n in ins:
            self.sym[s].positions.add(n)
        want_freq, want_erased = [], []
        for i in ids:
            erased = []
            self.sym[i].freq = 0
            B.compute_freq(self.sym[i], self.syms, self.freqs, erased)
            want_freq.append(self.sym[i].freq)
            want_erased += [(i, n) for n in erased]
        assert freq.tolist() == want_freq
        assert sorted(zip(es.tolist(), ek.tolist())) == sorted(want_erased)
        return want_freq, sorted(want_erased)


P, C, H = 5, 9, 12  # a lower symbol, the chain's symbol, a higher symbol (all (a, a))


def chain_state(o, L, mode, extra=()):
    """Sentence 0 "aab" * o: o unlinked (a, a) positions, given to the chain's
    own symbol (mode "same": the chain starts at lane o of the symbol's
    range) or to a lower symbol (mode "lower": at entry offset o of the whole
    array).  Sentence 1 a run of L + 1 chars: L positions (i, i + 1), one
    chain.  Sentence 2 "aa" belongs to a higher symbol."""
    syms = [[A, A, Bc] * o, [A] * (L + 1), [A, A]]
    pad = [B.encode_pos(0, 3 * i, 3 * i + 1) for i in range(o)]
    chain = [B.encode_pos(1, i, i + 1) for i in range(L)] + list(extra)
    symbols = {C: (A, A, chain + (pad if mode == "same" else [])), H: (A, A, [B.encode_pos(2, 0, 1)])}
    if mode == "lower":
        symbols[P] = (A, A, pad)
    return Mirror(syms, [3, F40, 5], symbols)


CHAIN_L = [1, 2, 3, 63, 64, 65, 127, 128, 129, 200]


@pytest.mark.parametrize("mode", ["same", "lower"])
@pytest.mark.parametrize("o", [0, 1, 62, 63, 64, 65])
def test_refresh_chain_against_chunk_edges(o, mode):
    for L in CHAIN_L:
        m = chain_state(o, L, mode)
        try:
            freq, erased = m.run(todo=[C, H] + ([P] if mode == "lower" else []))
            # By hand: every second link of the chain goes.
            assert freq[0] == ((L + 1) // 2) * F40 + (3 * o if mode == "same" else 0), (o, L)
            assert [n for s, n in erased] == [B.encode_pos(1, i, i + 1) for i in range(1, L, 2)], (o, L)
            assert freq[1] == 5
            # Nothing more to erase the second time.
            assert m.run(todo=[C])[1] == []
        finally:
            m.close()


def sorted_entries(m, sym):
    return sorted(m.sym[sym].positions)


@pytest.mark.parametrize("o", [0, 1, 63])
@pytest.mark.parametrize("L", [65, 129, 200])
@pytest.mark.parametrize("kill", ["lane0", "lane63", "lane64", "second", "chunk", "chunk0"])
def test_refresh_chain_with_dead_entries(o, L, kill):
    """Entries of the chain's symbol killed through the del list of the same
    call, by their index in the symbol's range: one at lane 0, 63, 64, every
    second one, and a whole aligned chunk (the second, or the first)."""
    m = chain_state(o, L, "same")
    try:
        ent = sorted_entries(m, C)
        idx = {"lane0": [0], "lane63": [63], "lane64": [64], "second": range(0, len(ent), 2),
               "chunk": range(64, 128), "chunk0": range(0, 64)}[kill]
        dels = [(C, ent[i]) for i in idx if i < len(ent)]
        m.run(dels=dels, todo=[C, H])
        assert m.run(todo=[C])[1] == []
    finally:
        m.close()


@pytest.mark.parametrize("o", [0, 1])
@pytest.mark.parametrize("gap", [64, 128, 130])
def test_refresh_carry_survives_dead_chunk(o, gap):
    """Dead entries BETWEEN two linked alive ones: after (62, 63) come `gap`
    entries (62, 64 + k), all killed, then (63, 64), which links to (62, 63)
    across one or two chunks without an alive entry.  With o = 1 entry
    (62, 63) is kept and sits on lane 63, so (63, 64) must go; with o = 0 it
    was erased itself, so (63, 64) is kept."""
    L = 200
    extra = [B.encode_pos(1, 62, 64 + k) for k in range(gap)]
    m = chain_state(o, L, "same", extra=extra)
    try:
        ent = sorted_entries(m, C)
        assert ent[o + 62] == B.encode_pos(1, 62, 63) and ent[o + 63 + gap] == B.encode_pos(1, 63, 64)
        freq, erased = m.run(dels=[(C, n) for n in extra], todo=[C])
        # The chain alternates as if the dead entries were not there.
        assert [n for _, n in erased] == [B.encode_pos(1, i, i + 1) for i in range(1, L, 2)]
    finally:
        m.close()


@pytest.mark.parametrize("c", [1, 63, 64, 65, 128, 199, 200])
@pytest.mark.parametrize("value", [Bc, -1])
def test_refresh_invalid_entries(c, value):
    """A write at char c of the run makes positions (c - 1, c) and (c, c + 1)
    invalid (entries c - 1 and c of the symbol's range: the last lane of a
    chunk and the first of the next for c = 64 and 128); the entry after them
    restarts the chain as kept."""
    L = 200
    m = chain_state(0, L, "same")
    try:
        freq, erased = m.run(writes=[(1, c, value)], todo=[C])
        gone = set(n for _, n in erased)
        assert B.encode_pos(1, c - 1, c) in gone
        if c < L:
            assert B.encode_pos(1, c, c + 1) in gone
        if c + 2 <= L:
            assert B.encode_pos(1, c + 1, c + 2) not in gone
    finally:
        m.close()


@pytest.mark.parametrize("o", [0, 62, 63, 64])
def test_refresh_link_conditions(o):
    """prev.r == l but another sentence: both kept.  Same sentence but
    prev.r != l: both kept.  o unlinked entries in front put the pairs on
    both sides of a chunk edge."""
    syms = [[A, A, Bc] * o, [], [], [A, A], [Bc, A, A], [A, A, Bc, A, A]]
    pos = [B.encode_pos(0, 3 * i, 3 * i + 1) for i in range(o)]
    pos += [B.encode_pos(3, 0, 1), B.encode_pos(4, 1, 2), B.encode_pos(5, 0, 1), B.encode_pos(5, 3, 4)]
    m = Mirror(syms, [1, 1, 1, F40, 2 * F40, 7], {C: (A, A, pos)})
    try:
        freq, erased = m.run(todo=[C])
        assert erased == [] and freq == [o + 3 * F40 + 14]
    finally:
        m.close()


@pytest.mark.parametrize("T", [1, 4, 5, 257])
def test_refresh_todo_shapes(T):
    """One wave per todo symbol, four waves a block: 1, 4, 5 and 257 symbols
    in one call, in shuffled order, the lowest and the highest id and a symbol
    without entries among them.  Sentence 70000 has freq 2^40 and gives one
    symbol 2^10 kept entries: sid << 32 and the 64-bit sum matter."""
    big_sid = 70000
    syms = [[] for _ in range(big_sid + 1)]
    freqs = [1] * (big_sid + 1)
    symbols = {}
    ids = list(range(2, 2 + T))
    for k, i in enumerate(ids):
        sid = 10 + 3 * k
        syms[sid] = [A] * (4 + k % 3)
        freqs[sid] = 1 + k
        symbols[i] = (A, A, [B.encode_pos(sid, j, j + 1) for j in range(len(syms[sid]) - 1)])
    syms[big_sid] = [A, A, Bc] * 1024
    freqs[big_sid] = F40
    symbols[ids[-1]][2].extend(B.encode_pos(big_sid, 3 * j, 3 * j + 1) for j in range(1024))
    m = Mirror(syms, freqs, symbols)
    try:
        todo = ids + [(ids[-1] + 7, A, Bc)]
        random.Random(T).shuffle(todo)
        freq, erased = m.run(todo=todo)
        by_id = dict(zip([t if isinstance(t, int) else t[0] for t in todo], freq))
        assert by_id[ids[-1] + 7] == 0
        assert by_id[ids[-1]] >= 1 << 50
        if T > 1:
            assert by_id[ids[0]] == 2
    finally:
        m.close()


def ab_state(positions_by_symbol, n=40):
    """Sentences 0..3, each "ab" * n; symbols over (a, b) with the given
    positions (sid, i) -> (i, i + 1), i even."""
    syms = [[A, Bc] * n for _ in range(4)]
    symbols = {s: (A, Bc, [B.encode_pos(sid, i, i + 1) for sid, i in p]) for s, p in positions_by_symbol.items()}
    return Mirror(syms, [1, 10, 100, F40], symbols)


def test_refresh_inserts_into_empty_set():
    m = ab_state({})
    try:
        assert m.dev.stats()[0] == 0
        freq, _ = m.run(ins=[(7, B.encode_pos(1, 2, 3)), (4, B.encode_pos(3, 0, 1)), (7, B.encode_pos(0, 0, 1))],
                        todo=[(4, A, Bc), (7, A, Bc), (5, A, Bc)])
        assert freq == [F40, 11, 0] and m.dev.stats()[0] == 3
    finally:
        m.close()


def test_refresh_inserts_before_after_between():
    """Inserts before every existing entry, after every existing entry,
    between two symbols and interleaved inside one symbol's range."""
    m = ab_state({5: [(1, i) for i in range(10, 30, 4)], 8: [(2, i) for i in range(10, 30, 4)]})
    try:
        E = B.encode_pos
        m.run(ins=[(3, E(0, 0, 1)), (5, E(0, 2, 3))], todo=[(3, A, Bc), 5, 8])
        m.run(ins=[(8, E(3, 4, 5)), (11, E(0, 0, 1))], todo=[(11, A, Bc), 8])
        m.run(ins=[(6, E(1, 0, 1)), (7, E(1, 0, 1))], todo=[(6, A, Bc), (7, A, Bc), 5, 8])
        m.run(ins=[(5, E(1, i, i + 1)) for i in range(12, 30, 4)] + [(5, E(1, 8, 9)), (5, E(1, 36, 37))],
              todo=[5])
        freq, erased = m.run(todo=[3, 5, 6, 7, 8, 11])
        assert erased == [] and freq == [1, 1 + 10 * 12, 10, 10, 100 * 5 + F40, 1]
        assert m.dev.stats()[0] == 10 + 2 + 2 + 2 + 7
    finally:
        m.close()


def test_refresh_reinsert_del_and_ins():
    E = B.encode_pos
    K = E(1, 12, 13)
    m = ab_state({5: [(1, i) for i in range(10, 20, 2)]})
    try:
        assert m.run(todo=[5])[0] == [50]
        # Erased in one call, inserted again in a later one: alive exactly once.
        assert m.run(dels=[(5, K)], todo=[5])[0] == [40]
        assert m.run(ins=[(5, K)], todo=[5])[0] == [50]
        assert m.dev.stats()[0] == 6
        # A key in both lists of one call ends alive.
        K2 = E(1, 16, 17)
        assert m.run(dels=[(5, K2)], ins=[(5, K2)], todo=[5])[0] == [50]
        # ... also when it was not there before.
        K3 = E(2, 0, 1)
        assert m.run(dels=[(5, K3)], ins=[(5, K3)], todo=[5])[0] == [150]
        # A del of a key that was never there: no effect.
        assert m.run(dels=[(5, E(3, 0, 1)), (4, K), (6, K), (5, E(1, 11, 12))], todo=[5])[0] == [150]
        # Erased by ComputeFreq itself (a stale position), then inserted again
        # once the symbols are back.
        _, erased = m.run(writes=[(1, 12, -1)], todo=[5])
        assert erased == [(5, K)]
        assert m.run(writes=[(1, 12, A)], ins=[(5, K)], todo=[5])[0] == [150]
        assert m.run(dels=[(5, K)], todo=[5])[0] == [140]
    finally:
        m.close()


def test_refresh_growth_and_erase_all():
    """10 positions at create (capacity 65536), 70000 inserted in one call on
    both sides of them, then a call whose writes invalidate every entry: the
    erased list is as long as the set."""
    n = 32768
    syms = [[A, Bc] * n, [A, Bc] * n, [A, Bc] * 10]
    E = B.encode_pos
    old = [E(2, i, i + 1) for i in range(0, 20, 2)]
    m = Mirror(syms, [1, F40, 3], {50: (A, Bc, old)})
    try:
        ab = [E(sid, i, i + 1) for sid in (0, 1) for i in range(0, 2 * n, 2)][:35000]
        ba = [E(sid, i, i + 1) for sid in (0, 1) for i in range(1, 2 * n - 1, 2)][-35000:]
        freq, erased = m.run(ins=[(10, k) for k in ab] + [(90, k) for k in ba],
                             todo=[(90, Bc, A), 50, (10, A, Bc)])
        assert erased == [] and freq[1] == 30 and freq[2] == 32768 + (35000 - 32768) * F40
        assert m.dev.stats()[0] == 70010
        writes = [(sid, i, -1) for sid in (0, 1, 2) for i in range(0, len(syms[sid]), 2)]
        freq, erased = m.run(writes=writes, todo=[10, 50, 90])
        assert freq == [0, 0, 0] and len(erased) == 70010
        assert m.run(todo=[10, 50, 90]) == ([0, 0, 0], [])
    finally:
        m.close()


def test_refresh_repeated_calls():
    """Positions erased by one run are not returned again by the next; a call
    without todo symbols applies its changes and reports nothing erased."""
    m = chain_state(3, 130, "same")
    try:
        first = m.run(todo=[C])[1]
        assert len(first) == 65
        assert m.run(todo=[C, H])[1] == []
        E = B.encode_pos
        freq, erased = m.run(writes=[(1, 7, Bc), (2, 1, -1)], ins=[(H, E(1, 0, 1))], dels=[(C, E(1, 20, 21))])
        assert (freq, erased) == ([], [])
        freq, erased = m.run(todo=[H, C])
        assert sorted(erased) == [(C, E(1, 6, 7)), (H, E(2, 0, 1))]
        assert freq[0] == F40
    finally:
        m.close()


def test_refresh_create_rejects_unsorted_positions():
    E = B.encode_pos
    for ps, pk in [([5, 4], [E(0, 0, 1), E(0, 0, 1)]), ([5, 5], [E(0, 2, 3), E(0, 0, 1)])]:
        with pytest.raises(S.SpmError) as e:
            S.BpeRefresh([A, Bc, A, Bc], [0, 4], [1], ps, pk)
        assert e.value.code == S.SPM_INVALID_ARGUMENT and "sorted" in str(e.value)


# ------------------------------------------- refresh, with the merge loop

def runs_corpus(seed, chars, sentences=10, max_run=300, budget=3000):
    rng = random.Random(seed)
    out = []
    for _ in range(sentences):
        s, c = "", rng.randrange(len(chars))
        for _ in range(rng.randint(1, 6)):
            s += chars[c] * rng.choice([1, 2, 3, 5, 64, 65, rng.randint(1, max_run)])
            c = (c + 1) % len(chars)
        out.append(s[:budget // sentences].encode())
    return out, [rng.choice([1, 2, F40]) for _ in out]


def lockstep_corpora():
    sevens = [b"aaaaaaa"] * 200
    return {
        "ab_runs": runs_corpus(11, "ab"),
        "run1000": ([b"a" * 1000], [3]),
        "sevens": (sevens, [1 + (i * 7) % 13 for i in range(200)]),
        "abab": ([b"ab" * 400, b"ab" * 3, b"b" + b"ab" * 70], [1, 2, F40]),
        "aab": ([b"aab" * 300, b"aab", b"baa" * 50], [5, 1, 2]),
        "four_byte": runs_corpus(12, "😀😁"),
    }


LOCKSTEP = lockstep_corpora()


@pytest.mark.parametrize("interval,merges", [(1, 40), (7, 60), (100, 150)])
@pytest.mark.parametrize("name", sorted(LOCKSTEP))
def test_refresh_in_lockstep_with_merge_loop(name, interval, merges):
    """The restatement's merge loop (every piece valid: validity is the
    host's business) hands its change log to the device at every
    UpdateActiveSymbols; freq and erased positions of every todo symbol equal
    ComputeFreq's, and the loop goes on from the reference's result."""
    sents, freqs = LOCKSTEP[name]
    seen = {"calls": 0, "erased": 0, "todo": 0, "ins": 0}
    dev = []

    def hook(log):
        freq, es, ek = dev[0].run(log.writes, log.ins_sym, log.ins_key, log.del_sym, log.del_key, log.todo)
        assert freq.tolist() == log.freq, (name, seen["calls"])
        assert sorted(zip(es.tolist(), ek.tolist())) == log.erased, (name, seen["calls"])
        seen["calls"] += 1
        seen["erased"] += len(log.erased)
        seen["todo"] += len(log.todo)
        seen["ins"] += len(log.ins_sym)

    t = B.Trainer(sents, freqs, interval=interval, refresh=hook)
    dev.append(S.BpeRefresh(*t.device_state()))
    try:
        pieces = t.train(merges)
        assert len(pieces) >= 5
        assert seen["calls"] >= 1 + (len(pieces) - 1) // interval
        assert seen["todo"] > 0
        if name in ("ab_runs", "run1000", "sevens", "four_byte"):  # runs of three equal chars from the start
            assert seen["erased"] > 0
        if len(pieces) > interval:
            assert seen["ins"] > 0
    finally:
        dev[0].close()
