"""Plain-Python restatement of the reference's WORD and CHAR models (test
yardstick), written from the reference's source:

  character::Model::Encode        char_model.cc:42-58
  word::Model::Encode             word_model.cc:33-46
  PrefixMatcher::PrefixMatch      normalizer.cc (longest user-defined symbol, else one char)
  SplitIntoWords                  model_interface.cc:155-192
  ModelInterface::PieceToId       model_interface.cc:87-97
  the unknown-run merge           sentencepiece_processor.cc (PopulateSentencePieceText)
  character::Trainer::Train       char_model_trainer.cc:31-64, trainer_interface.cc:385-424

Everything works on bytes; a token is (piece bytes, id).
"""
import math

import numpy as np

NORMAL, UNKNOWN, CONTROL, USER_DEFINED, UNUSED = 1, 2, 3, 4, 5
WORD, CHAR = 3, 4
SPACE = b"\xe2\x96\x81"  # U+2581
UNK_CHAR = 0x2585        # TrainerInterface::kUNKChar
UPP_BOUNDARY = 0x0009    # TrainerInterface::kUPPBoundaryChar

_ONE_CHAR_LEN = (1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 3, 4)


def one_char_len(first_byte):
    """string_util::OneCharLen (util.h): the first byte's high nibble only."""
    return _ONE_CHAR_LEN[first_byte >> 4]


class Model:
    """InitializePieces: pieces_, reserved_id_map_, the user-defined symbols."""

    def __init__(self, pieces, model_type):
        """pieces: list of (bytes|str, score, type)."""
        self.model_type = model_type
        self.pieces, self.reserved, self.user_defined = {}, {}, set()
        self.types = []
        self.unk_id = -1
        for i, (p, _score, t) in enumerate(pieces):
            if isinstance(p, str):
                p = p.encode()
            assert p, "piece must not be empty."
            dst = self.pieces if t in (NORMAL, USER_DEFINED, UNUSED) else self.reserved
            assert p not in dst, "%r is already defined." % p
            dst[p] = i
            self.types.append(t)
            if t == USER_DEFINED:
                self.user_defined.add(p)
            if t == UNKNOWN:
                assert self.unk_id < 0, "unk is already defined."
                self.unk_id = i
        assert self.unk_id >= 0, "unk is not defined."

    def piece_to_id(self, piece):
        if piece in self.reserved:
            return self.reserved[piece]
        return self.pieces.get(piece, self.unk_id)

    def prefix_match(self, w):
        """Longest user-defined symbol that prefixes w, else one char."""
        best = 0
        for u in self.user_defined:
            if len(u) > best and w.startswith(u):
                best = len(u)
        if best:
            return best
        return min(len(w), one_char_len(w[0]))

    def encode(self, normalized):
        """[(piece bytes, id)] of ModelInterface::Encode."""
        if self.model_type == CHAR:
            out, p = [], 0
            while p < len(normalized):
                n = self.prefix_match(normalized[p:])
                w = normalized[p:p + n]
                out.append((w, self.piece_to_id(w)))
                p += n
            return out
        return [(w, self.piece_to_id(w)) for w in split_into_words(normalized)]

    def merge_unk(self, tokens):
        """PopulateSentencePieceText: consecutive unknown tokens become one
        (CONTROL tokens never take part)."""
        out, prev_unk = [], False
        for w, i in tokens:
            is_unk = i == self.unk_id
            if self.types[i] != CONTROL and prev_unk and is_unk:
                out[-1] = (out[-1][0] + w, i)
            else:
                out.append((w, i))
            prev_unk = is_unk
        return out


def split_into_words(text, treat_whitespace_as_suffix=False):
    """SplitIntoWords: a list of byte strings that concatenate to text."""
    out, p = [], 0
    if treat_whitespace_as_suffix:
        if text:
            out.append(b"")
        while p < len(text):
            n = min(one_char_len(text[p]), len(text) - p)
            is_ws = text[p:p + n] == SPACE
            out[-1] += text[p:p + n]
            p += n
            if p < len(text) and is_ws:
                out.append(b"")
    else:
        while p < len(text):
            n = min(one_char_len(text[p]), len(text) - p)
            if p == 0 or text[p:p + n] == SPACE:
                out.append(b"")
            out[-1] += text[p:p + n]
            p += n
    return out


def encode_csr(model, sentences):
    """(ids int32, lens uint32, tok_off uint64) of a batch, as the device API
    returns them (no unknown-run merge)."""
    ids, lens, tok = [], [], [0]
    for s in sentences:
        for w, i in model.encode(s):
            ids.append(i)
            lens.append(len(w))
        tok.append(len(ids))
    return np.array(ids, np.int32), np.array(lens, np.uint32), np.array(tok, np.uint64)


def shortcut_is_exact(sentence):
    """The tile tier's condition: the sentence does not begin with a
    continuation byte and every lead byte's OneCharLen equals 1 + its run of
    continuation bytes (a run cut by the sentence end may be shorter)."""
    s = sentence
    if s and (s[0] & 0xC0) == 0x80:
        return False
    p = 0
    while p < len(s):
        q = p + 1
        while q < len(s) and (s[q] & 0xC0) == 0x80:
            q += 1
        n = one_char_len(s[p])
        if not (q - p == n or (q == len(s) and q - p <= n)):
            return False
        p = q
    return True


def _sorted(counts):
    """Sorted() of util.h: count descending, then key ascending."""
    return sorted(counts.items(), key=lambda kv: (-kv[1], kv[0]))


def char_counts(sentences):
    """chars_count of LoadSentences over (text, freq) pairs; text is valid
    UTF-8 (the normalizer's output).  U+0000, U+0020 and invalid code points
    are skipped; the caller leaves U+2585 lines out (LoadSentences drops them)."""
    counts = {}
    for text, freq in sentences:
        for ch in text.decode("utf-8"):
            c = ord(ch)
            if c == 0 or c == 0x20 or 0xD800 <= c < 0xE000:
                continue
            counts[c] = counts.get(c, 0) + freq
    return counts


def required_chars(counts, character_coverage, use_all_vocab):
    all_count = sum(counts.values())
    acc, req = 0, {}
    for c, k in _sorted(counts):
        coverage = np.float32(1.0 * acc / all_count)
        if not use_all_vocab and coverage >= np.float32(character_coverage):
            break
        acc += k
        if c == UPP_BOUNDARY:
            continue
        req[c] = k
    return req


def train_char(req, vocab_size, num_meta, use_all_vocab=False):
    """character::Trainer::Train over required_chars_: [(piece bytes, float32
    score)] and the vocab_size that Save sees."""
    size = vocab_size - num_meta
    assert size >= 0
    logsum = np.float32(math.log(sum(req.values())))
    out = []
    for c, k in _sorted(req):
        if not use_all_vocab and len(out) == size:
            break
        # log(count) is a double; minus the float logsum; narrowed to float.
        out.append((chr(c).encode("utf-8"), np.float32(math.log(k) - float(logsum))))
    if use_all_vocab:
        vocab_size = len(out) + num_meta
    return out, vocab_size
