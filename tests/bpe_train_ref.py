"""Plain-Python restatement of the reference's BPE trainer (test yardstick),
written from the reference's source with sets and dicts:

  DecodeUTF8 / UTF8ToUnicodeText      util.cc:187-220, :303-316, util.h:401-412
  EncodePos / DecodePos               bpe_model_trainer.h:84-101
  GetCharSymbol / GetPairSymbol       bpe_model_trainer.cc:32-82
  ComputeFreq                         bpe_model_trainer.cc:85-116
  GetNextIndex / GetPrevIndex         bpe_model_trainer.cc:119-134
  AddNewPair / ResetFreq              bpe_model_trainer.cc:137-153
  UpdateActiveSymbols                 bpe_model_trainer.cc:156-183
  Train: the census                   bpe_model_trainer.cc:200-230
  Train: the merge loop               bpe_model_trainer.cc:233-314
  Sorted                              trainer_interface.h:35-49

Where the reference leaves an order to the C++ library, this file fixes one
and says so:
  * Symbol::fp is FingerprintCat(left->fp, right->fp), a 64-bit hash; here the
    pair (left fp, right fp) itself, which is what the hash stands for.
  * active_symbols_ is a std::set<Symbol *>, ordered by address; here by
    creation sequence.  The order decides only between two bigrams of equal
    freq, length AND string (two splits of one string).
  * UpdateActiveSymbols partial_sorts the bigrams in unordered_map order by
    freq alone; here a stable sort over the cache's insertion order.  The kept
    set depends on that order only when there are more bigrams than it keeps
    (at least 1000); Trainer.cut says whether that ever happened.

The driver also keeps the change log include/spm_hip.h describes for
spm_hip_bpe_refresh_run, so a test can run the device refresh on the state
each UpdateActiveSymbols sees (Trainer.refresh).
"""
import numpy as np

UNK_CHAR = 0x2585      # TrainerInterface::kUNKChar
UNICODE_ERROR = 0xFFFD  # kUnicodeError


def _trail(x):
    """IsTrailByte (util.h:401): signed char < -0x40."""
    return (x & 0xC0) == 0x80


def _valid_cp(c):
    """IsValidCodepoint (util.h:410-412)."""
    return c < 0xD800 or 0xE000 <= c <= 0x10FFFF


def decode_utf8(b, p):
    """DecodeUTF8 (util.cc:187-220) at b[p:]: (code point, mblen).  Anything
    malformed is one byte long and decodes to U+FFFD."""
    n = len(b) - p
    c0 = b[p]
    if c0 < 0x80:
        return c0, 1
    elif n >= 2 and (c0 & 0xE0) == 0xC0:
        cp = ((c0 & 0x1F) << 6) | (b[p + 1] & 0x3F)
        if _trail(b[p + 1]) and cp >= 0x80 and _valid_cp(cp):
            return cp, 2
    elif n >= 3 and (c0 & 0xF0) == 0xE0:
        cp = ((c0 & 0x0F) << 12) | ((b[p + 1] & 0x3F) << 6) | (b[p + 2] & 0x3F)
        if _trail(b[p + 1]) and _trail(b[p + 2]) and cp >= 0x800 and _valid_cp(cp):
            return cp, 3
    elif n >= 4 and (c0 & 0xF8) == 0xF0:
        cp = ((c0 & 0x07) << 18) | ((b[p + 1] & 0x3F) << 12) | ((b[p + 2] & 0x3F) << 6) | (b[p + 3] & 0x3F)
        if _trail(b[p + 1]) and _trail(b[p + 2]) and _trail(b[p + 3]) and cp >= 0x10000 and _valid_cp(cp):
            return cp, 4
    return UNICODE_ERROR, 1


def utf8_to_unicode(b):
    """UTF8ToUnicodeText (util.cc:303-316)."""
    out, p = [], 0
    while p < len(b):
        c, m = decode_utf8(b, p)
        out.append(c)
        p += m
    return out


def unicode_to_utf8(chars):
    """UnicodeTextToUTF8 of code points DecodeUTF8 can return."""
    return "".join(chr(c) for c in chars).encode("utf-8")


def encode_pos(sid, l, r):
    """EncodePos (bpe_model_trainer.h:84-91), its CHECK_LE(l, kuint16max) included."""
    assert 0 <= l <= 0xFFFF and 0 <= r <= 0xFFFF, "EncodePos: index over kuint16max"
    return sid << 32 | (l << 16 | r)


def decode_pos(n):
    """DecodePos (bpe_model_trainer.h:95-101): (sid, left, right)."""
    return n >> 32, (n >> 16) & 0xFFFF, n & 0xFFFF


def sorted_pairs(items):
    """Sorted (trainer_interface.h:35-43): by value descending, then key ascending."""
    return sorted(items, key=lambda kv: (-kv[1], kv[0]))


class Symbol:
    """Trainer::Symbol (bpe_model_trainer.h:42-66).  left / right are Symbols
    in the driver; a hand-built test may use any values that compare with
    the entries of its own symbol arrays (ids, with -1 for a merged-away
    char)."""
    __slots__ = ("id", "left", "right", "chars", "is_unk", "fp", "freq", "positions")

    def __init__(self, id=0, left=None, right=None, chars=(), is_unk=False, fp=0, freq=0, positions=()):
        self.id, self.left, self.right = id, left, right
        self.chars, self.is_unk, self.fp, self.freq = tuple(chars), is_unk, fp, freq
        self.positions = set(positions)

    def is_bigram(self):
        return self.left is not None and self.right is not None

    def to_string(self):
        return unicode_to_utf8(self.chars)


def compute_freq(symbol, syms, sent_freq, erased=None):
    """ComputeFreq (bpe_model_trainer.cc:85-116).  syms[sid][i] is the symbol
    at char index i of sentence sid.  Erased positions leave symbol.positions
    and, if `erased` is a list, are appended to it."""
    if symbol.freq > 0:  # if freq == 0, re-computation is required.
        return
    prev_sid, prev_right = -1, 0
    # std::set<uint64>: ascending; an erase does not disturb the walk.
    for n in sorted(symbol.positions):
        sid, left, right = decode_pos(n)
        if ((sid == prev_sid and left == prev_right) or symbol.left != syms[sid][left] or
                symbol.right != syms[sid][right]):
            symbol.positions.discard(n)
            if erased is not None:
                erased.append(n)
            prev_sid, prev_right = -1, 0  # In "AAAA", the last "AA" can be counted.
        else:
            symbol.freq += sent_freq[sid]
            prev_sid, prev_right = sid, right


def census(sentences, freqs):
    """The state of bpe_model_trainer.cc:200-230 before the first merge, with
    ComputeFreq run on every fresh pair, in the layout of
    spm_hip_bpe_census_view: the GetCharSymbol loop over every sentence, then
    the AddNewPair loop over EVERY adjacent pair (piece validity is the
    caller's filter), then ComputeFreq.  Pair keys are left << 21 | right."""
    text = [utf8_to_unicode(s) for s in sentences]
    chars = {}  # code point -> its symbol (first-occurrence order)
    for t in text:
        for c in t:
            if c not in chars:
                chars[c] = Symbol(id=len(chars), chars=(c,), fp=c)
    syms = [[chars[c] for c in t] for t in text]
    pairs = {}  # (left, right) -> bigram symbol (first-occurrence order)
    for sid, t in enumerate(text):
        for i in range(1, len(t)):
            key = (t[i - 1], t[i])
            if key not in pairs:
                pairs[key] = Symbol(left=chars[t[i - 1]], right=chars[t[i]], chars=key)
            pairs[key].positions.add(encode_pos(sid, i - 1, i))
    for s in pairs.values():
        compute_freq(s, syms, freqs)
    char_off = np.zeros(len(text) + 1, dtype=np.uint64)
    if text:
        char_off[1:] = np.cumsum([len(t) for t in text], dtype=np.uint64)
    pos_off = np.zeros(len(pairs) + 1, dtype=np.uint64)
    if pairs:
        pos_off[1:] = np.cumsum([len(s.positions) for s in pairs.values()], dtype=np.uint64)
    return {
        "char_codes": np.array([c for t in text for c in t], dtype=np.uint32),
        "char_offsets": char_off,
        "unique_chars": np.array(list(chars), dtype=np.uint32),
        "pair_keys": np.array([l << 21 | r for l, r in pairs], dtype=np.uint64),
        "pair_freq": np.array([s.freq for s in pairs.values()], dtype=np.uint64),
        "pair_pos_offsets": pos_off,
        "pair_positions": np.array([n for s in pairs.values() for n in sorted(s.positions)], dtype=np.uint64),
    }


CENSUS_FIELDS = ("char_codes", "char_offsets", "unique_chars", "pair_keys", "pair_freq", "pair_pos_offsets",
                 "pair_positions")


class RefreshLog:
    """What one UpdateActiveSymbols hands to spm_hip_bpe_refresh_run, and what
    ComputeFreq then made of it: writes (flat index << 32 | uint32 value, the
    last per index), ins_* (inserts still in their sets, sorted, unique),
    del_* (positions the main loop's ComputeFreq erased), todo ([k, 3]:
    symbol, left, right ids of the cached bigrams whose freq is 0), freq (the
    reference's freq per todo symbol) and erased (sorted (symbol, position)
    pairs the reference erased)."""

    def __init__(self, writes, ins, dels, todo):
        self.writes = np.array(writes, dtype=np.uint64)
        self.ins_sym = np.array([s for s, _ in ins], dtype=np.uint32)
        self.ins_key = np.array([k for _, k in ins], dtype=np.uint64)
        self.del_sym = np.array([s for s, _ in dels], dtype=np.uint32)
        self.del_key = np.array([k for _, k in dels], dtype=np.uint64)
        self.todo = np.array(todo, dtype=np.uint32).reshape(-1, 3)
        self.freq, self.erased = [], []


class Trainer:
    """bpe::Trainer::Train (bpe_model_trainer.cc:186-314) from the loaded
    sentences on.  sentences: list[bytes]; freqs: one int per sentence;
    is_valid(chars) stands for IsValidSentencePiece; required_chars: {code
    point: count} (default: every char counts 1, as GetCharSymbol's
    FindWithDefault); interval: kUpdateActiveSymbolsInteval (the reference's
    100); refresh(log): called at each UpdateActiveSymbols with a RefreshLog."""

    def __init__(self, sentences, freqs, is_valid=None, required_chars=None, interval=100, refresh=None):
        self.freqs = [int(f) for f in freqs]
        self.is_valid = is_valid or (lambda chars: True)
        self.required_chars = dict(required_chars or {})
        self.interval, self.refresh = interval, refresh
        self.allocated = []        # allocated_: every Symbol, id = index
        self.cache = {}            # symbols_cache_: fp -> Symbol
        self.active = set()        # active_symbols_
        self.final_pieces = []
        self.dup = set()
        self.cut = False           # UpdateActiveSymbols kept fewer bigrams than exist
        self.refreshes = 0
        self._writes, self._ins, self._dels = {}, [], []
        # :207-212 symbols_[sid][i] stores an unary symbol.
        self.syms = [[self.get_char_symbol(c) for c in utf8_to_unicode(s)] for s in sentences]
        self.offsets = [0]
        for row in self.syms:
            self.offsets.append(self.offsets[-1] + len(row))
        # :216-220 makes all bigram symbols.
        for sid, row in enumerate(self.syms):
            for i in range(1, len(row)):
                self.add_new_pair(sid, i - 1, i)
        self._ins = []  # the positions so far are the device's initial state

    def _new_symbol(self, **kw):
        s = Symbol(id=len(self.allocated), **kw)
        self.allocated.append(s)
        return s

    def get_char_symbol(self, c):  # :32-47
        freq = self.required_chars.get(c, 1)
        assert freq > 0
        if c in self.cache:
            return self.cache[c]
        s = self._new_symbol(chars=(c,), is_unk=(c == UNK_CHAR), fp=c, freq=freq)
        self.cache[s.fp] = s
        return s

    def get_pair_symbol(self, left, right):  # :50-82
        if left is None or right is None or left.is_unk or right.is_unk:
            return None
        fp = (left.fp, right.fp)
        if fp in self.cache:
            return self.cache[fp]
        ut = left.chars + right.chars
        if not self.is_valid(ut):  # Do not make an invalid piece.
            return None
        s = self._new_symbol(left=left, right=right, chars=ut, fp=fp)
        self.cache[fp] = s
        return s

    def compute_freq(self, symbol, erased=None):
        compute_freq(symbol, self.syms, self.freqs, erased)

    def get_next_index(self, sid, index):  # :119-125
        for i in range(index + 1, len(self.syms[sid])):
            if self.syms[sid][i] is not None:
                return i
        return -1

    def get_prev_index(self, sid, index):  # :128-134
        for i in range(index - 1, -1, -1):
            if self.syms[sid][i] is not None:
                return i
        return -1

    def add_new_pair(self, sid, left, right):  # :137-144
        if left == -1 or right == -1:
            return
        symbol = self.get_pair_symbol(self.syms[sid][left], self.syms[sid][right])
        if symbol is not None:
            self.active.add(symbol)
            n = encode_pos(sid, left, right)
            if n not in symbol.positions:
                symbol.positions.add(n)
                self._ins.append((symbol.id, n))

    def reset_freq(self, sid, left, right, best):  # :147-153
        if left == -1 or right == -1:
            return
        symbol = self.get_pair_symbol(self.syms[sid][left], self.syms[sid][right])
        if symbol is not None and symbol is not best:
            symbol.freq = 0

    def _write(self, sid, index, symbol):
        self.syms[sid][index] = symbol
        self._writes[self.offsets[sid] + index] = 0xFFFFFFFF if symbol is None else symbol.id

    def device_state(self):
        """(syms int32 flat, sent_offsets, sent_freq, pos_sym, pos_key) of the
        current state, as spm_hip_bpe_refresh_create takes it; the change log
        restarts here."""
        flat = [-1 if s is None else s.id for row in self.syms for s in row]
        pos = sorted((s.id, n) for s in self.allocated for n in s.positions)
        self._writes, self._ins, self._dels = {}, [], []
        return (np.array(flat, dtype=np.int32), np.array(self.offsets, dtype=np.uint64),
                np.array(self.freqs, dtype=np.int64), np.array([s for s, _ in pos], dtype=np.uint32),
                np.array([n for _, n in pos], dtype=np.uint64))

    def _take_log(self, todo):
        writes = [i << 32 | v for i, v in sorted(self._writes.items())]
        ins = sorted(set((s, n) for s, n in self._ins if n in self.allocated[s].positions))
        log = RefreshLog(writes, ins, self._dels, [(s.id, s.left.id, s.right.id) for s in todo])
        self._writes, self._ins, self._dels = {}, [], []
        return log

    def update_active_symbols(self):  # :156-183
        bigrams = [s for s in self.cache.values() if s.is_bigram()]
        todo = [s for s in bigrams if s.freq == 0]
        log = self._take_log(todo) if self.refresh else None
        for s in bigrams:
            erased = []
            was_zero = s.freq == 0
            self.compute_freq(s, erased)
            if log is not None and was_zero:
                log.freq.append(s.freq)
                log.erased.extend((s.id, n) for n in erased)
        self.refreshes += 1
        if log is not None:
            log.erased.sort()
            self.refresh(log)
        # At least kMinActiveSymbolsSize symbols; keeps top 5% frequent symbols.
        size = min(max(1000, int(len(self.cache) * 0.05)), len(bigrams))
        if size < len(bigrams):
            self.cut = True
        bigrams.sort(key=lambda s: -s.freq)  # stable: see the module docstring
        self.active = set(bigrams[:size])

    def train(self, vocab_size):
        """The main loop (:233-314) until `vocab_size` merged pieces exist (or
        no symbol is left).  Returns the pieces as bytes, in merge order."""
        while len(self.final_pieces) < vocab_size:
            if len(self.final_pieces) % self.interval == 0:
                self.update_active_symbols()
            # Scanning active symbols, finds the best_symbol with highest freq.
            best = None
            for symbol in sorted(self.active, key=lambda s: s.id):
                erased = []
                self.compute_freq(symbol, erased)
                self._dels.extend((symbol.id, n) for n in erased)
                # Same freq: the shorter symbol; same length: lexicographical.
                if best is None or (symbol.freq > best.freq or (symbol.freq == best.freq and (
                        len(symbol.chars) < len(best.chars) or (
                            len(symbol.chars) == len(best.chars) and symbol.to_string() < best.to_string())))):
                    best = symbol
            if best is None:
                break  # "No valid symbol found"
            if best.to_string() in self.dup:
                # Removes best_symbol so it is not selected again.
                self.cache.pop(best.fp, None)
                self.active.discard(best)
                continue
            self.dup.add(best.to_string())
            self.final_pieces.append(best.to_string())
            # Add new bigrams which are created after symbol replacement.
            for n in sorted(best.positions):
                sid, left, right = decode_pos(n)
                if self.syms[sid][left] is None:
                    # left index might be NULL (set in the previous iteration)
                    # when left_symbol == right_symbol.
                    continue
                assert self.syms[sid][right] is not None
                nxt = self.get_next_index(sid, right)
                prev = self.get_prev_index(sid, left)
                # Resets the frequencies of bigrams [prev, left] and [right, next].
                self.reset_freq(sid, prev, left, best)
                self.reset_freq(sid, right, nxt, best)
                # Merges two symbols.
                self._write(sid, left, best)
                self._write(sid, right, None)
                # Makes new symbol bigrams [prev, left] and [left, next].
                self.add_new_pair(sid, prev, left)
                self.add_new_pair(sid, left, nxt)
            self.cache.pop(best.fp, None)
            self.active.discard(best)
        return list(self.final_pieces)

    def required_char_pieces(self):
        """:317-321: the required chars, Sorted, after the merged pieces."""
        return [self.get_char_symbol(c).to_string() for c, _ in sorted_pairs(self.required_chars.items())]
