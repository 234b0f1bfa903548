"""A word-closed hand model and sentences on the limits of the BPE text tiers
(test infrastructure of test_bpe_text_cpu.py and test_gpu_bpe_text.py).

Every piece is "▁"* followed by other chars; "ab" / "▁a" and "abc" / "▁ab" tie
on the score, "▁▁" merges runs of "▁", and "cd" is UNUSED: the pair (c, d) is
pushed wherever "c" meets "d", which every kernel but the literal one refuses.
predict() says, from the rules in csrc/bpe_words.hip alone, which tier must
finish a sentence."""
import bpe_cases as C
from model_builder import BPE, NORMAL, UNUSED, base_pieces, model

W = "▁".encode()
LANE_CHARS, WAVE_BYTES = 16, 1024  # kBpeWordChars, kBpeLineMaxBytes

MERGED = [("▁a", -1.0), ("ab", -1.0), ("▁▁", -2.0), ("▁ab", -3.0), ("abc", -3.0), ("cd", -4.0), ("▁▁a", -5.0),
          ("aa", -6.0), ("aaaa", -7.0), ("ああ", -8.0), ("bc", -9.0), ("de", -9.0), ("▁abc", -10.0), ("▁de", -11.0),
          ("あああ", -12.0), ("ee", -13.0), ("▁▁▁", -14.0), ("abcde", -15.0), ("eee", -16.0), ("▁e", -17.0)]
CHARS = ["a", "b", "c", "d", "e", "▁", "あ", "é"]


def hand_model(extra=()):
    pieces = base_pieces() + [(p, s, UNUSED if p == "cd" else NORMAL) for p, s in MERGED]
    pieces += [(c, -30.0 - k, NORMAL) for k, c in enumerate(CHARS)] + [(p, -50.0, NORMAL) for p in extra]
    return model(pieces, BPE)


def words(s):
    """s cut where a "▁" follows another char."""
    cuts = [p for p in range(1, len(s) - 2) if s[p:p + 3] == W and s[p - 3:p] != W]
    b = [0] + cuts + [len(s)]
    return [s[b[k]:b[k + 1]] for k in range(len(b) - 1)]


def predict(s, word_closed=True):
    """None (a first kernel finishes s), "word", "wave" or "literal"."""
    refused = b"cd" in s
    if C.route(s, C.TIER_LANE_AFFINE) != "general" and not refused:
        return None
    if len(s) <= 64 or refused:
        return "literal"
    regular = C.walk_starts(s) == [q for q, b in enumerate(s) if (b & 0xC0) != 0x80]
    if not word_closed or not regular:
        return "wave" if len(s) <= WAVE_BYTES else "literal"
    if any(C.n_chars(w) > LANE_CHARS and len(w) > WAVE_BYTES for w in words(s)):
        return "literal"
    return "word"


def edge_sentences():
    ab, A = W + b"ab", "あ".encode()
    out = [b"", b"ab", W + b"abc", b"a" * 65, A * 100, W * 3, ab * 40 + W]
    out += [b"a" * k + ab * 20 for k in (61, 62, 63, 64, 65)]           # a cut around a scan step's end
    out += [ab * k for k in (63, 64, 65, 129)]                          # words: full and partial groups
    out += [ab * 30 + W + b"a" * 15 + W + b"a" * 16 + (W + b"abc") * 5]  # a word at the lane bound, one over it
    out += [ab * 70 + W + b"ae" * 20 + (W + b"abcde") * 70 + W + A * 30 + ab]
    out += [ab * 3 + W + b"a" * k + W + b"de" for k in (1021, 1022)]    # a word of 1024 and of 1025 bytes
    out += [(b"ab" + W * 3) * 12 + b"ab", b"abc" + (W + b"abe") * 20, W * 2 + ab * 25 + W * 2]
    out += [b"ab\xf0a" + W + b"b" + ab * 20, b"ab\xf0a" + W + b"b" + ab * 400]  # walk-irregular: never split
    out += [ab * 25 + W + b"cd", b"acd", (W + b"zab" + "é".encode()) * 25, W + b"a\x00b" + ab * 25]
    return out
