"""Python restatement of byte fallback (test infrastructure).

A model trained with byte_fallback=true carries 256 pieces "<0x00>" ...
"<0xFF>" of type BYTE (6) and sets TrainerSpec.byte_fallback (field 35).  The
rules, as the `sentencepiece` package (0.2.2) shows them:

  load    BYTE pieces are reserved like CONTROL pieces (never matched against
          text); the byte -> id map comes from the pieces' names.
  expand  PopulateSentencePieceText does not merge UNKNOWN tokens; each becomes
          one BYTE id per byte of its normalized text.  All byte pieces of a
          token but the last have an empty surface at the token's begin, the
          last one carries the whole surface.  Extra options apply afterwards.
  decode  a maximal run of consecutive BYTE pieces of one sentence (final
          order) is decoded greedily as UTF-8: a valid sequence of k bytes gives
          k - 1 empty surfaces and the char on its last piece, any other byte
          U+FFFD.  Byte surfaces are never space-converted or stripped.

The model-level encode does not change, so it comes from the CPU oracle over
control_view(model): the same model with its BYTE rows typed CONTROL (the
oracle predates BYTE and skips field 35).  Everything after it is restated
here on top of decode_ref.
"""
import gzip
import os
import struct

import numpy as np

import decode_ref
import model_builder as mb
import model_reader
import vocab_ref

BYTE = 6
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FFFD = b"\xef\xbf\xbd"


def byte_piece(b):
    return b"<0x%02X>" % b


def piece_to_byte(piece):
    if len(piece) == 6 and piece[:3] == b"<0x" and piece[5:] == b">":
        h = piece[3:5]
        if all(c in b"0123456789ABCDEF" for c in h):
            return int(h, 16)
    return -1


def read_pieces(model_bytes):
    """[(piece, score, type)] with type BYTE kept (model_reader.read_pieces
    knows the five older types and reads any other as NORMAL)."""
    out = []
    for f, wt, v in model_reader.fields(model_bytes):
        if f == 1 and wt == 2:
            p, s, t = b"", 0.0, 1
            for g, gt, w in model_reader.sub_fields(v):
                if g == 1:
                    p = bytes(w)
                elif g == 2:
                    s = struct.unpack("<f", w)[0]
                elif g == 3:
                    t = w if 1 <= w <= BYTE else 1
            out.append((p, s, t))
    return out


def byte_ids(model_bytes):
    """byte -> id of its BYTE piece, from the names."""
    out = [-1] * 256
    for i, (p, _, t) in enumerate(read_pieces(model_bytes)):
        if t == BYTE:
            out[piece_to_byte(p)] = i
    return out


def control_view(model_bytes):
    """The model with its BYTE rows typed CONTROL: what a reader that predates
    BYTE needs in order to run the unchanged model-level encode."""
    types = [mb.CONTROL if t == BYTE else t for _, _, t in read_pieces(model_bytes)]
    return vocab_ref.retype(model_bytes, types)


def plain_view(model_bytes):
    """control_view with byte_fallback cleared (a later trainer_spec occurrence
    merges): a model without byte fallback that gives the same model-level
    tokens, for this engine, which checks the flag against the BYTE rows."""
    return control_view(model_bytes) + mb._ld(2, mb._key(35, 0) + mb._varint(0))


def expand(ids, lens, norm, unk_id, bids, n2o=None):
    """Model-level tokens of one sentence -> [(id, begin, end)] (begin / end in
    normalized bytes, or through n2o in raw bytes)."""
    a = n2o if n2o is not None else range(len(norm) + 1)
    out, c = [], 0
    for tid, ln in zip(ids, lens):
        tid, ln = int(tid), int(ln)
        if tid == unk_id:
            for j in range(ln):
                last = j == ln - 1
                out.append((bids[norm[c + j]], int(a[c]), int(a[c + ln]) if last else int(a[c])))
        else:
            out.append((tid, int(a[c]), int(a[c + ln])))
        c += ln
    assert c == len(norm)
    return out


def apply_options(rows, options, bos_row, eos_row):
    rows = list(rows)
    for o in (s for s in options.split(":") if s):
        if o == "reverse":
            rows.reverse()
        elif o == "bos":
            rows.insert(0, bos_row)
        elif o == "eos":
            rows.append(eos_row)
        else:
            raise ValueError(o)
    return rows


def utf8_valid_len(b):
    """Bytes of the valid UTF-8 sequence at the start of b, 0 if there is none."""
    def trail(x):
        return 0x80 <= x <= 0xBF
    b0 = b[0]
    if b0 < 0x80:
        return 1
    if len(b) >= 2 and b0 & 0xE0 == 0xC0:
        cp = (b0 & 0x1F) << 6 | (b[1] & 0x3F)
        return 2 if trail(b[1]) and cp >= 0x80 else 0
    if len(b) >= 3 and b0 & 0xF0 == 0xE0:
        cp = (b0 & 0x0F) << 12 | (b[1] & 0x3F) << 6 | (b[2] & 0x3F)
        return 3 if trail(b[1]) and trail(b[2]) and cp >= 0x800 and not 0xD800 <= cp < 0xE000 else 0
    if len(b) >= 4 and b0 & 0xF8 == 0xF0:
        cp = (b0 & 0x07) << 18 | (b[1] & 0x3F) << 12 | (b[2] & 0x3F) << 6 | (b[3] & 0x3F)
        return 4 if trail(b[1]) and trail(b[2]) and trail(b[3]) and 0x10000 <= cp <= 0x10FFFF else 0
    return 0


def run_surfaces(run):
    """The surfaces of one byte run, decoded greedily from its start."""
    out, k = [], 0
    while k < len(run):
        v = utf8_valid_len(run[k:k + 4])
        if v == 0:
            out.append(FFFD)
            k += 1
        else:
            out.extend([b""] * (v - 1) + [bytes(run[k:k + v])])
            k += v
    return out


class Model(decode_ref.Model):
    """decode_ref.Model plus the byte-run rule."""

    def __init__(self, model_bytes):
        super().__init__(model_bytes)
        self.pieces = read_pieces(model_bytes)
        self.normal, self.reserved = {}, {}
        for i, (p, _, t) in enumerate(self.pieces):
            (self.normal if t in (mb.NORMAL, mb.USER_DEFINED, mb.UNUSED) else self.reserved)[p] = i
        self.byte_of = {i: piece_to_byte(p) for i, (p, _, t) in enumerate(self.pieces) if t == BYTE}

    def decode_ids(self, ids, options=""):
        rows = [(self.pieces[i][0], self.piece_to_id(self.pieces[i][0])) for i in ids]
        bos = (self.bos_piece, self.piece_to_id(self.bos_piece))
        eos = (self.eos_piece, self.piece_to_id(self.eos_piece))
        rows = apply_options(rows, ":".join(self.parse_options(options)), bos, eos)
        surfaces = [None] * len(rows)
        k = 0
        while k < len(rows):
            if rows[k][1] in self.byte_of:
                e = k
                while e < len(rows) and rows[e][1] in self.byte_of:
                    e += 1
                surfaces[k:e] = run_surfaces(bytes(self.byte_of[r[1]] for r in rows[k:e]))
                k = e
            else:
                k += 1
        text, out = b"", []
        for (piece, pid), s in zip(rows, surfaces):
            if s is None:
                t = self.pieces[pid][2]
                if t == decode_ref.CONTROL:
                    s = b""
                elif t == decode_ref.UNKNOWN:
                    s = self.unk_surface
                else:
                    rest = piece[len(decode_ref.WS):] if not text and piece.startswith(decode_ref.WS) else piece
                    s = rest.replace(decode_ref.WS, b" ")
            out.append((piece, pid, s, len(text), len(text) + len(s)))
            text += s
        return text, out


# ---- fixtures: the package's recorded answers ----
# botchan_bf_{unigram,bpe}1k.model: sentencepiece 0.2.2, SentencePieceTrainer.train(input=botchan.txt,
# vocab_size=1000, byte_fallback=True, character_coverage=0.98, model_type=...).  Per corpus and model,
# .spt.gz holds encode(line, out_type="proto") of every line (ids, begins, ends) and .decoded.gz
# decode(ids) of every line, one per row.

FIXTURES = ("botchan_bf_unigram1k", "botchan_bf_bpe1k")
CORPORA = (("botchan", "botchan.txt"), ("wagahaiwa", "wagahaiwa_nekodearu.txt"))


def fixture_model(name):
    return open(os.path.join(GOLD, name + ".model"), "rb").read()


def corpus_lines(corpus_file):
    data = open(os.path.join(GOLD, corpus_file), "rb").read().split(b"\n")
    return data[:-1] if data and data[-1] == b"" else data


def recorded_spt(corpus, fixture):
    """<corpus>_bf_<type>1k.spt.gz: little-endian uint32 n, uint32 counts[n], then
    for all tokens int16 ids, uint32 begins, uint32 ends (raw byte offsets), as
    sentencepiece 0.2.2 encodes every line of the corpus.  Returns (off, ids,
    begins, ends), off the CSR offsets of the lines."""
    name = corpus + fixture[len("botchan"):]
    raw = gzip.open(os.path.join(GOLD, name + ".spt.gz"), "rb").read()
    n = int(np.frombuffer(raw, "<u4", 1)[0])
    counts = np.frombuffer(raw, "<u4", n, 4)
    t = int(counts.sum())
    at = 4 + 4 * n
    ids = np.frombuffer(raw, "<i2", t, at).astype(np.int32)
    begins = np.frombuffer(raw, "<u4", t, at + 2 * t)
    ends = np.frombuffer(raw, "<u4", t, at + 6 * t)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(counts, dtype=np.uint64)
    return off, ids, begins, ends


def recorded_texts(corpus, fixture):
    name = corpus + fixture[len("botchan"):]
    return gzip.open(os.path.join(GOLD, name + ".decoded.gz"), "rb").read().split(b"\n")[:-1]


# ---- hand models ----

def byte_rows():
    return [(byte_piece(b), 0.0, BYTE) for b in range(256)]


def with_byte_fallback(model_bytes):
    """A second trainer_spec occurrence (it merges) that sets byte_fallback, field 35."""
    return model_bytes + mb._ld(2, mb._key(35, 0) + mb._varint(1))


def hand_model(pieces, model_type=mb.UNIGRAM, byte_pieces=None, flag=True, **kw):
    """base pieces + 256 BYTE rows + `pieces`, with byte_fallback set."""
    rows = mb.base_pieces() + (byte_rows() if byte_pieces is None else byte_pieces) + list(pieces)
    m = mb.model(rows, model_type=model_type, **kw)
    return with_byte_fallback(m) if flag else m


FIRST_BYTE_ID = 3  # hand_model: <unk>, <s>, </s>, then the bytes in order
