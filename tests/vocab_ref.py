"""Python restatement of the vocabulary restriction (test infrastructure).

The checker of SetVocabulary / ResetVocabulary / LoadVocabulary and of
spm_encode --generate_vocabulary, written from the rules include/spm_hip.h
and csrc/processor.h spell out:

  * set_vocabulary / reset_vocabulary: the type rule over (piece, score, type)
    lists (sentencepiece_processor.cc:203-245),
  * parse_vocabulary: LoadVocabulary's line format (:256-274) with
    string_util::Split's dropping of empty fields,
  * vocabulary_file: the "piece\\tcount" lines of --generate_vocabulary, by
    count descending, then piece ascending (bytes),
  * retype: a serialized ModelProto with other piece types, everything else
    byte for byte,
  * viterbi: a plain best-path search with an explicit unknown score, for the
    case where the restricted processor (scores frozen at load) and a reload
    of the retyped proto differ.
"""
from model_builder import _key, _ld, _varint, piece
from model_reader import fields, read_pieces

NORMAL, UNKNOWN, CONTROL, USER_DEFINED, UNUSED = 1, 2, 3, 4, 5
_CHAR_LEN = (1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 3, 4)


def _b(s):
    return s if isinstance(s, bytes) else s.encode()


def one_char(p):
    """OneCharLen(piece.c_str()) == piece.size()."""
    p = _b(p)
    return _CHAR_LEN[(p[0] if p else 0) >> 4] == len(p)


def set_vocabulary(pieces, vocab):
    """Types after SetVocabulary(vocab); pieces: [(piece, score, type)]."""
    vocab = {_b(v) for v in vocab}
    out = []
    for p, _, t in pieces:
        if t in (CONTROL, UNKNOWN, USER_DEFINED):
            out.append(t)
        else:
            out.append(NORMAL if _b(p) in vocab or one_char(p) else UNUSED)
    return out


def reset_vocabulary(types):
    return [NORMAL if t == UNUSED else t for t in types]


def parse_vocabulary(data, threshold):
    """The pieces LoadVocabulary passes to SetVocabulary; ValueError where it fails."""
    lines = _b(data).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    vocab = []
    for line in lines:
        v = [f for f in line.split(b"\t") if f]
        if not v:
            raise ValueError("a line without fields")
        freq = 1
        if len(v) >= 2:
            freq = _atoi(v[1])
        if freq >= threshold:
            vocab.append(v[0])
    return vocab


def _atoi(b):
    b = b.lstrip(b" \t\n\v\f\r")
    sign, i = 1, 0
    if b[:1] in (b"+", b"-"):
        sign, i = (-1 if b[:1] == b"-" else 1), 1
    v = 0
    while i < len(b) and 48 <= b[i] <= 57:
        v = v * 10 + b[i] - 48
        i += 1
    return sign * v


def vocabulary_file(counts, pieces):
    """--generate_vocabulary's output from per-id counts."""
    rows = [(_b(pieces[i][0]), int(c)) for i, c in enumerate(counts)
            if c and pieces[i][2] not in (UNKNOWN, CONTROL)]
    rows.sort(key=lambda r: (-r[1], r[0]))
    return b"".join(p + b"\t" + str(c).encode() + b"\n" for p, c in rows)


def retype(model_bytes, types):
    """model_bytes with piece i's type replaced by types[i]."""
    out, i = b"", 0
    old = read_pieces(model_bytes)
    for f, wt, v in fields(model_bytes):
        if f == 1 and wt == 2:
            out += _ld(1, piece(old[i][0], old[i][1], int(types[i])))
            i += 1
        elif wt == 0:
            out += _key(f, 0) + _varint(v)
        elif wt == 2:
            out += _ld(f, bytes(v))
        else:
            out += _key(f, wt) + bytes(v)
    assert i == len(types)
    return out


def viterbi(pieces, types, s, unk_score):
    """Best segmentation of the normalized bytes s: ids.  Nodes: every NORMAL
    piece (USER_DEFINED pieces are not modelled); a char position without a
    one-char node gets the unknown node with unk_score.  Strict >, the first
    candidate wins, as unigram_model.cc:222-261."""
    s = _b(s)
    table = {_b(p): (i, sc) for i, ((p, sc, _), t) in enumerate(zip(pieces, types)) if t == NORMAL}
    unk = [i for i, t in enumerate(types) if t == UNKNOWN][0]
    cs, q = [], 0
    while q < len(s):
        cs.append(q)
        q += min(_CHAR_LEN[s[q] >> 4], len(s) - q)
    cs.append(len(s))
    nc = len(cs) - 1
    best = [None] * (nc + 1)   # (score, previous position, id)
    best[0] = (0.0, -1, -1)
    for b in range(nc):
        cands, single = [], False
        for e in range(b + 1, nc + 1):
            ent = table.get(s[cs[b]:cs[e]])
            if ent:
                cands.append((e, ent[1], ent[0]))
                single |= e == b + 1
        if not single:
            cands.append((b + 1, unk_score, unk))
        for e, sc, i in cands:
            t = best[b][0] + sc
            if best[e] is None or t > best[e][0]:
                best[e] = (t, b, i)
    ids, p = [], nc
    while p > 0:
        ids.append(best[p][2])
        p = best[p][1]
    return ids[::-1]
