"""Python restatement of SentencePieceProcessor::Decode (test infrastructure).

The checker of spm_hip_decode_batch, its host loop and the processor's Decode,
written from the rules of the reference (sentencepiece_processor.cc:670-733,
ApplyExtraOptions :945-979, ParseExtraOptions :981-1023):

  * Decode(ids) turns each id into IdToPiece(id) and goes on as Decode(pieces);
    Decode(pieces) gives each piece id = PieceToId(piece), unk_id when the
    piece is not in the vocabulary;
  * the decode extra options act on the piece list in the order given:
    reverse reverses it, bos prepends bos_piece, eos appends eos_piece;
  * the text grows left to right.  A CONTROL piece adds "".  An UNKNOWN id
    adds unk_surface when the piece text is IdToPiece(id), else the piece's
    own bytes, verbatim.  Any other piece loses one leading U+2581 if the
    text so far is empty, then every U+2581 becomes one space;
  * begin / end of a piece are the byte offsets of its surface in the text.

Model(model_bytes).decode_ids / decode_pieces return (text, rows), rows =
[(piece, id, surface, begin, end)].
"""
import model_reader

NORMAL, UNKNOWN, CONTROL, USER_DEFINED, UNUSED = 1, 2, 3, 4, 5
WS = b"\xe2\x96\x81"  # U+2581
DEFAULT_UNK_SURFACE = b" \xe2\x81\x87 "


class DecodeError(Exception):
    pass


class Model:
    def __init__(self, model_bytes):
        self.pieces = model_reader.read_pieces(model_bytes)
        self.bos_piece, self.eos_piece = b"<s>", b"</s>"
        self.unk_surface = DEFAULT_UNK_SURFACE
        for f, wt, v in model_reader.fields(model_bytes):
            if f == 2 and wt == 2:  # trainer_spec (a repeated occurrence merges)
                for g, gt, w in model_reader.sub_fields(v):
                    if g == 44 and gt == 2:
                        self.unk_surface = bytes(w)
                    elif g == 46 and gt == 2:
                        self.bos_piece = bytes(w)
                    elif g == 47 and gt == 2:
                        self.eos_piece = bytes(w)
        self.normal, self.reserved = {}, {}
        self.unk_id = -1
        for i, (p, _, t) in enumerate(self.pieces):
            (self.normal if t in (NORMAL, USER_DEFINED, UNUSED) else self.reserved)[p] = i
            if t == UNKNOWN:
                self.unk_id = i

    def piece_to_id(self, piece):
        if piece in self.reserved:
            return self.reserved[piece]
        return self.normal.get(piece, self.unk_id)

    def parse_options(self, options):
        """ParseExtraOptions: the option list, or DecodeError with its message."""
        out = []
        for o in (s for s in options.split(":") if s):
            if o not in ("bos", "eos", "reverse"):
                raise DecodeError('option "%s" is not available.' % o)
            out.append(o)
            for name, piece in (("bos", self.bos_piece), ("eos", self.eos_piece)):
                if o == name and self.piece_to_id(piece) == self.unk_id:
                    raise DecodeError("id for `%s` is not defined." % piece.decode())
        return out

    def decode_pieces(self, pieces, options=""):
        rows = [(bytes(p), self.piece_to_id(bytes(p))) for p in pieces]
        for o in self.parse_options(options):
            if o == "reverse":
                rows.reverse()
            elif o == "eos":
                rows.append((self.eos_piece, self.piece_to_id(self.eos_piece)))
            else:
                rows.insert(0, (self.bos_piece, self.piece_to_id(self.bos_piece)))
        text = b""
        out = []
        for piece, pid in rows:
            t = self.pieces[pid][2]
            if t == CONTROL:
                surface = b""
            elif t == UNKNOWN:
                surface = self.unk_surface if self.pieces[pid][0] == piece else piece
            else:
                if not text and piece.startswith(WS):
                    piece_rest = piece[len(WS):]
                else:
                    piece_rest = piece
                surface = piece_rest.replace(WS, b" ")
            out.append((piece, pid, surface, len(text), len(text) + len(surface)))
            text += surface
        return text, out

    def decode_ids(self, ids, options=""):
        return self.decode_pieces([self.pieces[i][0] for i in ids], options)

    def decode_batch(self, ids, tok_off, options=""):
        """The id CSR of a batch -> (text bytes, out_off list, begins list)."""
        text, off, begins = b"", [0], []
        for i in range(len(tok_off) - 1):
            t, rows = self.decode_ids([int(x) for x in ids[int(tok_off[i]):int(tok_off[i + 1])]], options)
            text += t
            off.append(len(text))
            begins.extend(r[3] for r in rows)
        return text, off, begins
