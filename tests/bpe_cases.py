"""Models and sentences that put BPE encode on every kernel tier (test
infrastructure, shared by test_bpe_tiers_cpu.py and test_gpu_bpe_tiers.py).

EncodeBpe picks its first kernel from the model (spm_hip_model_info.fast_variant
of a BPE model): 1 lane kernel with rank ids, merged id = base - rank; 2 lane
kernel with rank ids from the rank table; 3 lane kernel with 32-bit symbol
words (tied merge scores); 4 half kernel (>= 32768 pieces); 0 general kernel
only (user-defined symbols).  What the first kernel refuses goes to the fast
kernel (<= 64 bytes), what that refuses is flagged for the general kernel.

build_model() makes one small merge table reach each tier by parameters;
pool() is ~1000 short sentences that sit on and around every limit of those
kernels; route() predicts from the documented limits alone which kernel must
take a sentence.
"""
import random

from model_builder import BPE, CONTROL, NORMAL, UNUSED, USER_DEFINED, base_pieces, model

WS = "▁"
ASCII = "abcdefghijkl"
C2, C3, C4 = "éüñö", "あいうえ", "😀𝄞"
ALPHABET = list(ASCII) + [WS] + list(C2) + list(C3) + list(C4)  # 23 chars
# Chars of 1, 2, 3 and 4 bytes outside every variant's vocabulary ("z" is the
# CONTROL piece of reserved_top models).
OOV = ["z", "ß", "ก", "🎉"]
# pad_to fillers are single chars from U+4E00 upwards; only these three occur
# in the sentences.
LISTED_FILLERS = ["日", "本", "語"]
# The two single-char pieces irregular=True drops (merged pieces keep them).
DROPPED = ["l", "ö"]
N_CHAR_MERGES, N_MERGES, MAX_PIECE_CHARS = 300, 600, 8

TIER_LANE_AFFINE, TIER_LANE_TABLE, TIER_LANE_WORDS, TIER_HALF, TIER_GENERAL = 1, 2, 3, 4, 0
# Limits from the kernels' headers in csrc/bpe_kernels.hip.
LANE_CHARS, LANE_BYTES = 34, 255
HALF_CHARS, HALF_BYTES = 32, 128
FAST_BYTES = 64
TILE = 128


def _merges():
    """~600 merged pieces in merge order: 300 pairs of single chars (the
    self-pairs "aa", "bb", ... among them, so that a run of one letter ties
    on the left index), then pairs of any two existing pieces, <= 8 chars."""
    rng = random.Random(20240)
    have = set(ALPHABET)
    out = []
    for c in ("a", "b", "c", "é", "あ", "😀"):
        out.append(c + c)
    have.update(out)
    while len(out) < N_CHAR_MERGES:
        p = rng.choice(ALPHABET) + rng.choice(ALPHABET)
        if p not in have:
            have.add(p)
            out.append(p)
    for p in ("aaaa", "aaa", "bbbb"):  # runs merge on: (aa, aa), (aa, a), (bb, bb)
        have.add(p)
        out.append(p)
    pool = list(ALPHABET) + out
    while len(out) < N_MERGES:
        p = rng.choice(pool) + rng.choice(pool)
        if p not in have and len(p) <= MAX_PIECE_CHARS:
            have.add(p)
            out.append(p)
            pool.append(p)
    return out


MERGES = _merges()
# The merged pieces that unused=True marks UNUSED (about 5 %).
UNUSED_PIECES = [p for p in MERGES if random.Random("unused" + p).random() < 0.05]


def _fillers(n):
    skip = set(ALPHABET) | set(OOV) | set(LISTED_FILLERS)
    out = list(LISTED_FILLERS)
    cp = 0x4E00
    while len(out) < n:
        if not 0xD800 <= cp <= 0xDFFF and chr(cp) not in skip:  # (surrogates have no UTF-8 form)
            out.append(chr(cp))
        cp += 1
    return out


class Spec:
    """A built model: blob (serialized ModelProto), pieces ((str, score,
    type) in id order), id_of (piece -> id)."""

    def __init__(self, pieces):
        self.pieces = pieces
        self.blob = model(pieces, BPE)
        self.id_of = {p: i for i, (p, _, _) in enumerate(pieces)}

    def __len__(self):
        return len(self.pieces)


def build_model(order="score", ties=False, unused=False, irregular=False, reserved_top=False, pad_to=None,
                user_defined=False):
    """The mini model (see the module docstring and _merges) as:
    order="score": pieces in score order (merged pieces, score = -merge
      index, then the chars) -> tier 1;  order="shuffled": the mini pieces'
      ids permuted with a fixed seed -> tier 2.
    ties: each 4 consecutive merged pieces share one score -> tier 3.
    unused: about 5 % of the merged pieces are UNUSED (flag + resegment).
    irregular: the single-char pieces of DROPPED are left out.
    reserved_top: the last id is the CONTROL piece "z".
    pad_to=V: single-char fillers with the lowest scores BEFORE the mini
      pieces, exactly V pieces in all: the live ids are the top ids.
    user_defined: one USER_DEFINED piece -> tier 0."""
    mini = []
    for i, p in enumerate(MERGES):
        score = -float(i // 4 + 1) if ties else -float(i + 1)
        mini.append((p, score, UNUSED if unused and p in UNUSED_PIECES else NORMAL))
    for k, c in enumerate(ALPHABET):
        if irregular and c in DROPPED:
            continue
        mini.append((c, -float(N_MERGES + 1 + k), NORMAL))
    if order == "shuffled":
        random.Random(11).shuffle(mini)
    else:
        assert order == "score"
    tail = []
    if user_defined:
        tail.append(("<tag>", 0.0, USER_DEFINED))
    if reserved_top:
        tail.append(("z", 0.0, CONTROL))
    pieces = base_pieces()
    if pad_to is not None:
        nfill = pad_to - len(pieces) - len(mini) - len(tail)
        assert nfill > len(LISTED_FILLERS)
        pieces += [(c, -float(100000 + j), NORMAL) for j, c in enumerate(_fillers(nfill))]
    pieces += mini + tail
    assert pad_to is None or len(pieces) == pad_to
    return Spec(pieces)


# ---------------------------------------------------------------------------
# Sentences
# ---------------------------------------------------------------------------
def one_char_len(b):
    """OneCharLen of the reference (util.h): by the lead byte's high nibble."""
    return (1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 3, 4)[b >> 4]


def walk_starts(s):
    """Char starts of the reference's split: OneCharLen steps clamped to the
    sentence (bpe_model.cc:121-131)."""
    out, q = [], 0
    while q < len(s):
        out.append(q)
        q += min(one_char_len(s[q]), len(s) - q)
    return out


def n_chars(s):
    return len(walk_starts(s))


def sweep():
    """For every char count 0..70, 12 sentences: random vocabulary pieces
    (about 3 % of the draws an out-of-vocabulary char instead) cut to that
    many chars."""
    rng = random.Random(31337)
    vocab = MERGES + ALPHABET
    out = []
    for c in range(71):
        for _ in range(12):
            s = ""
            while len(s) < c:
                s += rng.choice(OOV) if rng.random() < 0.03 else rng.choice(vocab)
            out.append(s[:c].encode())
    return out


def _ascii(n, seed):
    rng = random.Random(seed)
    return "".join(rng.choice(ASCII[:6]) for _ in range(n)).encode()


def limits():
    """name -> (sentence, bytes, chars): sentences written out on the kernels'
    limits; bytes / chars are what the name promises."""
    four = lambda n: ("😀𝄞" * n)[:n].encode()
    out = {
        "four32": (four(32), 128, 32),
        "four31_ascii5": (four(31) + b"abcab", 129, 36),
        "ascii32": (_ascii(32, 1), 32, 32),
        "ascii33": (_ascii(33, 2), 33, 33),
        "ascii34": (_ascii(34, 3), 34, 34),
        "ascii35": (_ascii(35, 4), 35, 35),
        "ascii64": (_ascii(64, 5), 64, 64),
        "ascii65": (_ascii(65, 6), 65, 65),
        "ascii63_two1": (_ascii(63, 7) + "é".encode(), 65, 64),
        "two32": (("éü" * 16).encode(), 64, 32),
        "two33": (("éü" * 16 + "ñ").encode(), 66, 33),
        "three34": (("あい" * 17).encode(), 102, 34),
        "three35": (("あい" * 17 + "う").encode(), 105, 35),
        "ascii128": (_ascii(128, 8), 128, 128),
        "bytes255": (("あ" * 60 + "é" * 30).encode() + _ascii(15, 9), 255, 105),
        "bytes256": (("あ" * 60 + "é" * 30).encode() + _ascii(16, 10), 256, 106),
    }
    for k in range(2, 41):
        out["a_x%d" % k] = (b"a" * k, k, k)
    return out


def edge_sentences():
    """The byte strings of test_gpu_parity._edge_sentences()."""
    ws = WS.encode()
    return [
        b"", b"a", ws, ws + b"abc", b"\xff\xfe", b"ab\x00cd", b"\xe3\x81", "日本語テキスト".encode(),
        ws + b"a" * 300, ws + (b"ab" * 2000), b"zzzzqqqq", "▁▁▁".encode(),
        "é".encode() + b"\x80\x80" + "漢".encode()[:2],
        ws + b"x\x00y", b"x\x00y", b"q\x00\x00", ws + b"the\x00a\x00",
    ]


def malformed():
    out = edge_sentences()
    out += [
        b"\x80abc", b"\xbf", b"ab\x80\x80cd",              # continuation byte first / stray
        b"abc\xc3", b"ab\xe3", b"ab\xf0", b"ab\xf0\x9f",    # lead byte (or a cut char) last
        b"\xc3abc", b"a\xe3bc", b"\xf0abcde", b"\xe3\x81a",  # lead byte followed by ASCII
        b"\xf8", b"a\xf9b", b"\xfa\xfb\xfc\xfd", b"ab\xfe\xffab", b"\xf8\x80\x80\x80\x80",
        b"ab\x00", b"\x00", b"aa\x00aa", b"abc\x00abc\x00",  # NUL inside and after a piece
        b"\xc3" * 33, b"a\x80" * 30, b"\xf0" + b"a" * 40,
    ]
    return out


def filler_sentences():
    return ["ab日cd本".encode(), "語".encode(), "日本語日本語".encode() + b"abab"]


_POOL = []


def pool():
    """Every sentence, in a fixed order: empties first, adjacent and last."""
    if not _POOL:
        _POOL.extend(_make_pool())
    return list(_POOL)


def _make_pool():
    out = [b""] + sweep() + [b"", b""] + [v[0] for v in limits().values()] + malformed() + filler_sentences()
    # Pieces as sentences (an UNUSED piece's own string pushes it), runs of
    # one multi-byte char, "z" runs for reserved_top models.
    out += [p.encode() for p in MERGES[::7] + UNUSED_PIECES] + [("é" * k).encode() for k in (2, 3, 5, 9)]
    out += [b"z", b"azbzzc", "zあz".encode()]
    out += [b""]
    return out


# ---------------------------------------------------------------------------
# Routing predictor
# ---------------------------------------------------------------------------
def first_kernel_takes(s, tier):
    """Whether the tier's first kernel takes the sentence, by the limits in
    the kernels' headers: bpe_lane_kernel <= 34 chars (OneCharLen walk) and
    <= 255 bytes; bpe_half_kernel <= 128 bytes, <= 32 chars counted as
    non-continuation bytes, and that split equal to the OneCharLen walk."""
    if tier in (TIER_LANE_AFFINE, TIER_LANE_TABLE, TIER_LANE_WORDS):
        return len(s) <= LANE_BYTES and n_chars(s) <= LANE_CHARS
    if tier == TIER_HALF:
        if len(s) > HALF_BYTES:
            return False
        noncont = [q for q, b in enumerate(s) if (b & 0xC0) != 0x80]
        return len(noncont) <= HALF_CHARS and noncont == walk_starts(s)
    return False


def route(s, tier):
    """"first", "fast" or "general": the kernel that must take sentence s on a
    model of this tier without UNUSED pieces that is not irregular."""
    if tier == TIER_GENERAL:
        return "general"
    if first_kernel_takes(s, tier):
        return "first"
    return "fast" if len(s) <= FAST_BYTES else "general"


def flagged_count(sents, tier):
    return sum(route(s, tier) == "general" for s in sents)


# ---------------------------------------------------------------------------
# Batch shapes
# ---------------------------------------------------------------------------
SIZES = (1, 2, 3, 127, 128, 129, 257, None)  # None: the whole pool
ARRANGEMENTS = ("shuffled", "refused_tile", "short_last")
_SHORT = (b"ab", b"a", b"abc", b"abca")


def batch(arrangement, n=None):
    """The pool cut to n sentences in one of three arrangements:
    shuffled: a fixed permutation.
    refused_tile: the first 128-sentence tile holds only sentences that both
      the lane and the half kernel refuse; the shuffled rest follows.
    short_last: shuffled, with a short last sentence that ends at a byte
      offset that is no multiple of 4 (the lane kernel loads the batch's last
      partial dword byte by byte)."""
    p = pool()
    random.Random(99).shuffle(p)
    if arrangement == "refused_tile":
        ref = [s for s in p if not first_kernel_takes(s, TIER_LANE_AFFINE) and not first_kernel_takes(s, TIER_HALF)]
        assert len(ref) >= TILE
        tile = ref[:TILE]
        rest = list(p)
        for s in tile:
            rest.remove(s)
        p = tile + rest
    if n is not None:
        p = p[:n]
    if arrangement == "short_last":
        total = sum(len(s) for s in p[:-1])
        p[-1] = next(s for s in _SHORT if (total + len(s)) % 4)
    return p
