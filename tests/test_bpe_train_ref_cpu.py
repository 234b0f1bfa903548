"""CPU: the BPE trainer restatement (tests/bpe_train_ref.py) pinned -- no GPU
calls.

The merge-loop driver against the reference's own BasicTest answers and
against the oracle's trainer on a seeded corpus; ComputeFreq on the runs the
reference's comments speak of; the census against the driver's state before
its first merge.

The driver takes piece validity from a callback.  `valid` below restates only
what these texts can meet of IsValidSentencePiece (trainer_interface.cc:
178-265): the length limit (max_sentencepiece_length, 16), no kUPPBoundaryChar
(the tab a user-defined symbol is replaced by, :206), and kWSChar at the first
place only (:236, split_by_whitespace).  The texts are lower-case ASCII, so the
script, number, NUL, space and kUNKChar rules never fire.
"""
import random

import pytest

import bpe_train_ref as B
import oracle_lib
from test_trainer_cpu import BPE_BASIC

WS = 0x2581
TAB = 0x09


def valid(chars):
    return len(chars) <= 16 and TAB not in chars and WS not in chars[1:]


def load(lines, uds=(), dummy_prefix=False):
    """What LoadSentences and SplitSentencesByWhitespace leave of lines that
    hold no space (trainer_interface.cc:347-424, :465-477): user-defined
    symbols replaced by a tab, one word per line with its count, Sorted; the
    required chars are all chars but the tab."""
    tokens = {}
    for l in lines:
        s = ("▁" if dummy_prefix else "") + l
        for u in uds:
            s = s.replace(u, "\t")
        tokens[s] = tokens.get(s, 0) + 1
    sents = B.sorted_pairs(tokens.items())
    chars = {}
    for s, f in sents:
        for c in s:
            if ord(c) != TAB:
                chars[ord(c)] = chars.get(ord(c), 0) + f
    return [s.encode() for s, _ in sents], [f for _, f in sents], chars


@pytest.mark.parametrize("interval", [100, 1, 7])
@pytest.mark.parametrize("lines,size,uds,want", BPE_BASIC)
def test_driver_reproduces_basic_test(lines, size, uds, want, interval):
    """bpe_model_trainer_test.cc:26-91.  vocab_size = size - 3 holds <unk>,
    <s>, </s>, the user-defined symbols and the required chars; the merge
    loop fills the rest.  The refresh interval does not change the answer on
    texts this small (every bigram stays active)."""
    sents, freqs, chars = load(lines, uds)
    t = B.Trainer(sents, freqs, is_valid=valid, required_chars=chars, interval=interval)
    merges = (size - 3) - 3 - len(uds) - len(chars)
    got = list(uds) + [p.decode() for p in t.train(merges)] + [p.decode() for p in t.required_char_pieces()]
    assert " ".join(got) == want
    assert not t.cut


def seeded_lines(seed, count, alphabet, lo, hi):
    rng = random.Random(seed)
    return ["".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(count)]


@pytest.mark.parametrize("seed,alphabet,merges", [(1, "abcde", 300), (2, "abc", 250), (3, "etaoin", 150)])
def test_driver_equals_oracle_trainer(seed, alphabet, merges):
    lines = seeded_lines(seed, 400, alphabet, 1, 12)
    sents, freqs, chars = load(lines, dummy_prefix=True)
    args = ("--model_type=bpe --normalization_rule_name=identity --vocab_size=%d" % (3 + merges + len(chars)))
    p, s, ty = oracle_lib.OracleTrainer(args, [l.encode() for l in lines]).train()
    t = B.Trainer(sents, freqs, is_valid=valid, required_chars=chars)
    got = t.train(merges) + t.required_char_pieces()
    assert len(t.final_pieces) == merges
    assert got == p[3:]
    # With every bigram active, neither unordered_map's order nor
    # partial_sort's handling of ties had a say.
    assert not t.cut


def sym_of(text, left, right):
    """A fresh (left, right) bigram over one sentence of char codes, every
    adjacent occurrence in its position set."""
    s = B.Symbol(left=left, right=right)
    for i in range(1, len(text)):
        if (text[i - 1], text[i]) == (left, right):
            s.positions.add(B.encode_pos(0, i - 1, i))
    return s


@pytest.mark.parametrize("text,kept", [("aaa", [0]), ("aaaa", [0, 2]), ("aaaaa", [0, 2]), ("aaaaaa", [0, 2, 4]),
                                        ("aabaaa", [0, 3]), ("abab", [0, 2])])
def test_compute_freq_overlap_rule(text, kept):
    """bpe_model_trainer.cc:95-109: of two overlapping bigrams the second goes,
    and the one after an erased one counts again."""
    codes = [ord(c) for c in text]
    l, r = (ord("a"), ord("a")) if "aa" in text else (ord("a"), ord("b"))
    s = sym_of(codes, l, r)
    all_pos = sorted(s.positions)
    erased = []
    B.compute_freq(s, [codes], [7], erased)
    assert sorted(B.decode_pos(n)[1] for n in s.positions) == kept
    assert s.freq == 7 * len(kept)
    assert sorted(erased + list(s.positions)) == all_pos
    # freq > 0: no re-computation.
    s.positions.clear()
    B.compute_freq(s, [codes], [7])
    assert s.freq == 7 * len(kept)


def test_compute_freq_erases_stale_positions():
    """A position whose symbols no longer are (left, right) is erased, the
    chain restarts after it, and another sentence never links."""
    a, b = 1, 2
    syms = [[a, a, a, a, a, a], [a, a]]
    s = B.Symbol(left=a, right=a, positions=[B.encode_pos(0, i, i + 1) for i in range(5)] + [B.encode_pos(1, 0, 1)])
    syms[0][2] = b  # positions (1,2) and (2,3) are stale
    erased = []
    B.compute_freq(s, syms, [1, 1 << 40], erased)
    # By hand: (0,1) kept; (1,2) and (2,3) stale; (3,4) kept; (4,5) overlaps
    # (3,4) and goes; sentence 1's (0,1) starts where sentence 0's kept (0,1)
    # ended only by index, not by sentence: kept.
    assert sorted(erased) == [B.encode_pos(0, 1, 2), B.encode_pos(0, 2, 3), B.encode_pos(0, 4, 5)]
    assert sorted(s.positions) == [B.encode_pos(0, 0, 1), B.encode_pos(0, 3, 4), B.encode_pos(1, 0, 1)]
    assert s.freq == 2 + (1 << 40)


def test_compute_freq_merged_away_is_stale():
    """A merged-away char (None / -1 in the symbol array) never matches."""
    a = 1
    s = B.Symbol(left=a, right=a, positions=[B.encode_pos(0, 0, 1), B.encode_pos(0, 1, 2), B.encode_pos(0, 2, 3)])
    erased = []
    B.compute_freq(s, [[a, -1, a, a]], [3], erased)
    assert sorted(erased) == [B.encode_pos(0, 0, 1), B.encode_pos(0, 1, 2)]
    assert s.freq == 3 and s.positions == {B.encode_pos(0, 2, 3)}


CENSUS_CORPORA = {
    "runs": [b"aaaa", b"baaaa", b"aaaab", b"aabaaa", b"", b"a", b"ab" * 5],
    "utf8": ["aé猫😀😀😀é".encode(), "猫猫猫猫猫".encode(), b"\x00\x00\x00a"],
    "malformed": [b"\x80\x80\x80a", b"a\xc0\x80b", b"\xe0\x80\x80", b"\xf0\x80\x80\x80", b"\xed\xa0\x80",
                  b"\xf4\x90\x80\x80", b"ab\xe3\x81"],
    "random": [l.encode() for l in seeded_lines(5, 120, "ab", 0, 9)],
}


@pytest.mark.parametrize("name", sorted(CENSUS_CORPORA))
def test_census_equals_driver_state_before_first_merge(name):
    """Two code paths of the restatement against each other: census() builds
    its pairs with plain dicts; the driver goes through GetPairSymbol and
    AddNewPair, and its first UpdateActiveSymbols runs ComputeFreq."""
    sents = CENSUS_CORPORA[name]
    rng = random.Random(9)
    freqs = [rng.choice([1, 2, 1 << 40]) for _ in sents]
    c = B.census(sents, freqs)
    t = B.Trainer(sents, freqs)
    t.update_active_symbols()
    chars = [s for s in t.allocated if not s.is_bigram()]
    pairs = [s for s in t.allocated if s.is_bigram()]
    assert c["unique_chars"].tolist() == [s.chars[0] for s in chars]
    assert c["char_codes"].tolist() == [s.chars[0] for row in t.syms for s in row]
    assert c["char_offsets"].tolist() == t.offsets
    assert c["pair_keys"].tolist() == [s.chars[0] << 21 | s.chars[1] for s in pairs]
    assert c["pair_freq"].tolist() == [s.freq for s in pairs]
    off = c["pair_pos_offsets"].tolist()
    pos = c["pair_positions"].tolist()
    assert [pos[off[k]:off[k + 1]] for k in range(len(pairs))] == [sorted(s.positions) for s in pairs]


def test_census_of_known_text():
    """"aaab" with freq 5, by hand."""
    c = B.census([b"aaab"], [5])
    a, b = ord("a"), ord("b")
    assert c["char_codes"].tolist() == [a, a, a, b]
    assert c["unique_chars"].tolist() == [a, b]
    assert c["pair_keys"].tolist() == [a << 21 | a, a << 21 | b]
    assert c["pair_freq"].tolist() == [5, 5]
    assert c["pair_pos_offsets"].tolist() == [0, 1, 2]
    assert c["pair_positions"].tolist() == [B.encode_pos(0, 0, 1), B.encode_pos(0, 2, 3)]


def test_decode_utf8_rules():
    """util.cc:187-220: every malformed byte is one U+FFFD."""
    E = B.UNICODE_ERROR
    assert B.utf8_to_unicode("aé猫😀".encode()) == [0x61, 0xE9, 0x732B, 0x1F600]
    assert B.utf8_to_unicode(b"\x80") == [E]                      # stray continuation
    assert B.utf8_to_unicode(b"\xc0\x80") == [E, E]               # overlong 2
    assert B.utf8_to_unicode(b"\xe0\x80\x80") == [E, E, E]        # overlong 3
    assert B.utf8_to_unicode(b"\xf0\x80\x80\x80") == [E] * 4      # overlong 4
    assert B.utf8_to_unicode(b"\xed\xa0\x80") == [E] * 3          # surrogate
    assert B.utf8_to_unicode(b"\xf4\x90\x80\x80") == [E] * 4      # above U+10FFFF
    assert B.utf8_to_unicode(b"a\xe3\x81") == [0x61, E, E]        # truncated at the end
    assert B.utf8_to_unicode(b"\xf4\x8f\xbf\xbf\x00") == [0x10FFFF, 0]


def test_driver_log_is_what_the_header_describes():
    """One write per flat index (the last), inserts sorted and unique and
    still in their sets, todo triples of cached bigrams with freq 0; the
    expected freq and erased lists line up with the todo list."""
    logs = []
    t = B.Trainer([b"aaaaaaa", b"abababab", b"aabaab"], [3, 1, 2], interval=1, refresh=logs.append)
    t.device_state()
    t.train(6)
    assert len(logs) >= 6 and len(logs[0].writes) == 0 and len(logs[0].ins_sym) == 0
    assert len(logs[0].todo) == len([s for s in t.allocated[:5] if s.is_bigram()])
    seen_writes = False
    for g in logs:
        idx = [int(w) >> 32 for w in g.writes]
        assert idx == sorted(set(idx))
        ins = list(zip(g.ins_sym.tolist(), g.ins_key.tolist()))
        assert ins == sorted(set(ins))
        assert len(g.freq) == len(g.todo)
        for s, l, r in g.todo.tolist():
            assert (t.allocated[s].left.id, t.allocated[s].right.id) == (l, r)
        assert set(s for s, _ in g.erased) <= set(g.todo[:, 0].tolist())
        seen_writes |= len(g.writes) > 0
    assert seen_writes
