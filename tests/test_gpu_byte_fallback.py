"""GPU: byte fallback.  Encode (ids, SentencePieceText) and decode of both
golden corpora under the two byte_fallback fixtures equal the `sentencepiece`
package's recorded answers through the C-ABI and the CLIs; hand models force
every encode tier and the shapes at which the token-tile epilogue
(byte_epilogue_kernels.hip) and the byte-run decode (decode_kernels.hip) can go
wrong; spm_train --byte_fallback writes the model of the same command with 256
placeholder control symbols."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import sentencepiece

import byte_fallback_ref as R
import model_builder as mb
import spm_amd as S
import test_gpu_decode as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sentencepiece-comments_amd", "lib")
ENCODE, DECODE, TRAIN = (os.path.join(LIB, x) for x in ("spm_encode", "spm_decode", "spm_train"))
pytestmark = pytest.mark.gpu
WS = "▁"
CANARY = -7
SUB, TILE = S.DECODE_SUBTILE_TOKENS, S.DECODE_TILE_TOKENS


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


_MODELS = {}


def _fixture(name):
    if name not in _MODELS:
        mbytes = R.fixture_model(name)
        _MODELS[name] = (mbytes, S.DeviceModel(mbytes))
    return _MODELS[name]


def _csr_rows(off, ids):
    return [ids[int(off[i]):int(off[i + 1])].tolist() for i in range(len(off) - 1)]


# ---- corpus parity ----

@pytest.mark.parametrize("corpus,corpus_file", R.CORPORA)
@pytest.mark.parametrize("name", R.FIXTURES)
def test_corpus_encode_ids(name, corpus, corpus_file):
    mbytes, dm = _fixture(name)
    off, ids, _, _ = R.recorded_spt(corpus, name)
    got = dm.encode_lines_device(R.corpus_lines(corpus_file))
    assert [len(r) for r in got] == np.diff(off.astype(np.int64)).tolist()
    assert np.array_equal(np.fromiter((x for r in got for x in r), np.int32, int(off[-1])), ids)


def _encode_spt(dm, lines, options=""):
    """spm_hip_encode_spt -> (piece_off, pieces int64[k, 5], norm bytes, norm_off)."""
    import torch
    dev = _dev()
    buf, off = S.to_csr(lines)
    n = len(lines)
    s = torch.cuda.current_stream(dev).cuda_stream
    d_in = torch.from_numpy(buf).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    cap = int(off[-1]) * 3 + 3 * n + 16
    d_norm = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_noff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_a = torch.empty(cap + n, dtype=torch.int32, device=dev)
    pcap = cap + 4 * n
    d_p = torch.full((pcap * 5,), CANARY, dtype=torch.int32, device=dev)
    d_po = torch.empty(n + 1, dtype=torch.int64, device=dev)
    tn, tp = ctypes.c_uint64(), ctypes.c_uint64()
    S._check(dm._L.spm_hip_encode_spt(dm.h, options.encode(), d_in.data_ptr(), d_off.data_ptr(), n, d_norm.data_ptr(),
                                      cap, d_noff.data_ptr(), d_a.data_ptr(), d_p.data_ptr(), pcap, d_po.data_ptr(),
                                      ctypes.byref(tn), ctypes.byref(tp), s))
    torch.cuda.synchronize(dev)
    p = d_p.cpu().numpy()
    assert (p[5 * tp.value:] == CANARY).all()
    return (d_po.cpu().numpy(), p[:5 * tp.value].reshape(-1, 5).astype(np.int64) & 0xFFFFFFFF,
            d_norm[:tn.value].cpu().numpy().tobytes(), d_noff.cpu().numpy())


@pytest.mark.parametrize("corpus,corpus_file", R.CORPORA)
@pytest.mark.parametrize("name", R.FIXTURES)
def test_corpus_encode_spt(name, corpus, corpus_file):
    mbytes, dm = _fixture(name)
    off, ids, begins, ends = R.recorded_spt(corpus, name)
    po, p, norm, noff = _encode_spt(dm, R.corpus_lines(corpus_file))
    assert np.array_equal(po.astype(np.uint64), off)
    assert np.array_equal(p[:, 0], ids) and np.array_equal(p[:, 1], begins) and np.array_equal(p[:, 2], ends)
    # Byte pieces carry no normalized range (piece = IdToPiece(id)); any other
    # piece's range holds its piece string.
    is_byte = np.isin(ids, np.array(R.byte_ids(mbytes)))
    assert (p[is_byte, 3] == p[is_byte, 4]).all() and (p[~is_byte, 4] > p[~is_byte, 3]).all()
    pieces = R.read_pieces(mbytes)
    line = np.searchsorted(off, np.arange(len(ids)), side="right") - 1
    for k in np.flatnonzero(~is_byte)[::53]:
        base = int(noff[line[k]])
        assert norm[base + int(p[k, 3]):base + int(p[k, 4])] == pieces[int(ids[k])][0]


@pytest.mark.parametrize("entry", ["blocking", "async"])
@pytest.mark.parametrize("corpus,corpus_file", R.CORPORA)
@pytest.mark.parametrize("name", R.FIXTURES)
def test_corpus_decode(name, corpus, corpus_file, entry):
    mbytes, dm = _fixture(name)
    off, ids, _, _ = R.recorded_spt(corpus, name)
    texts = R.recorded_texts(corpus, name)
    text, out_off, begins = D._decode(dm, ids, off, entry=entry)
    assert text == b"".join(texts)
    assert out_off == np.concatenate([[0], np.cumsum([len(t) for t in texts])]).tolist()
    if corpus == "botchan":  # begins against the restatement, per line
        ref = R.Model(mbytes)
        rows = _csr_rows(off, ids)
        want = [r[3] for i in range(0, len(rows), 11) for r in ref.decode_ids(rows[i])[1]]
        got = [b for i in range(0, len(rows), 11) for b in begins[int(off[i]):int(off[i + 1])]]
        assert got == want


def _ids_text(off, ids):
    return "".join(" ".join(str(x) for x in r) + "\n" for r in _csr_rows(off, ids)).encode()


@pytest.mark.parametrize("name", R.FIXTURES)
def test_cli_encode_and_decode(name, tmp_path):
    """spm_encode (the batch path, the small path and one-line Encode) and
    spm_decode on both corpora."""
    model = os.path.join(R.GOLD, name + ".model")
    for corpus, corpus_file in R.CORPORA:
        off, ids, _, _ = R.recorded_spt(corpus, name)
        want = _ids_text(off, ids)
        p = subprocess.run([ENCODE, "--model=" + model, "--output_format=id", os.path.join(R.GOLD, corpus_file)],
                           capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        assert p.stdout == want
        for path in ("device", "host") if corpus == "botchan" else ("device",):  # host: the processor's own loop
            d = subprocess.run([DECODE, "--model=" + model, "--input_format=id"], input=want, capture_output=True,
                               timeout=300, env=dict(os.environ, SPM_HIP_DECODE_PATH=path))
            assert d.returncode == 0, d.stderr[-2000:]
            assert d.stdout == b"".join(t + b"\n" for t in R.recorded_texts(corpus, name))
        # 60 lines: batches of 20 take the small path (EncodeIdsSmall), batches of 1 are one-line Encode.
        lines = R.corpus_lines(corpus_file)[:60]
        head = tmp_path / (corpus + ".txt")
        head.write_bytes(b"".join(l + b"\n" for l in lines))
        head_want = b"".join(want.split(b"\n")[k] + b"\n" for k in range(60))
        for batch in (20, 1):
            q = subprocess.run([ENCODE, "--model=" + model, "--output_format=id", "--batch_lines=%d" % batch, str(head)],
                               capture_output=True, timeout=300)
            assert q.returncode == 0, q.stderr[-2000:]
            assert q.stdout == head_want
    # pieces, and the extra options through the processor's host epilogue
    sp = sentencepiece.SentencePieceProcessor(model_file=model)
    text = [l.decode() for l in R.corpus_lines("botchan.txt")[:60]] + ["aあいb", "<0x41> q"]
    src = tmp_path / "pieces.txt"
    src.write_bytes("".join(l + "\n" for l in text).encode())
    q = subprocess.run([ENCODE, "--model=" + model, "--output_format=piece", "--extra_options=bos:reverse:eos", str(src)],
                       capture_output=True, timeout=300)
    assert q.returncode == 0, q.stderr[-2000:]
    want = [R.apply_options(r, "bos:reverse:eos", "<s>", "</s>") for r in sp.encode(text, out_type=str)]
    assert q.stdout == "".join(" ".join(r) + "\n" for r in want).encode()


def test_count_pieces_cli(tmp_path):
    """spm_encode --generate_vocabulary (CountPieces) counts the expanded ids."""
    name = R.FIXTURES[0]
    mbytes, _ = _fixture(name)
    off, ids, _, _ = R.recorded_spt("botchan", name)
    counts = np.bincount(ids, minlength=len(R.read_pieces(mbytes)))
    p = subprocess.run([ENCODE, "--model=" + os.path.join(R.GOLD, name + ".model"), "--generate_vocabulary",
                        os.path.join(R.GOLD, "botchan.txt")], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = dict((l.split(b"\t")[0], int(l.split(b"\t")[1])) for l in p.stdout.split(b"\n")[:-1])
    pieces = R.read_pieces(mbytes)
    want = {pieces[i][0]: int(c) for i, c in enumerate(counts) if c and pieces[i][2] not in (mb.UNKNOWN, mb.CONTROL)}
    assert got == want
    assert sum(c for pc, c in got.items() if R.piece_to_byte(pc) >= 0) == 5187


# ---- epilogue shapes on hand models ----

BASE = [(WS, -2.0, mb.NORMAL), ("a", -2.5, mb.NORMAL), ("b", -2.6, mb.NORMAL), (WS + "a", -2.2, mb.NORMAL),
        ("ab", -2.4, mb.NORMAL), (WS + "the", -2.1, mb.NORMAL)]
WIDE = BASE + [("吾輩は猫であ", -3.0, mb.NORMAL), ("吾", -3.5, mb.NORMAL)]
# tier -> (pieces, model type, fast_variant, knob)
TIERS = {
    "unigram byte": (BASE, mb.UNIGRAM, 1, None),
    "unigram wide": (WIDE, mb.UNIGRAM, 3, None),
    "unigram cooperative": (WIDE, mb.UNIGRAM, 3, "coop"),
    "unigram general": (BASE, mb.UNIGRAM, 1, "general"),
    "bpe lane": (BASE, mb.BPE, 1, None),
    "bpe general": (BASE + [("<x>", 0.0, mb.USER_DEFINED)], mb.BPE, 0, None),
}
OPTIONS = ["", "bos", "eos", "reverse", "bos:eos", "eos:bos", "reverse:bos:eos", "bos:reverse", "bos:eos:reverse",
           "eos:reverse:bos"]


def shape_lines():
    """Unknowns first and last, 4-byte chars, empty lines, 300 unknown CJK chars
    (900 ids: past a 256-token sub-tile and a 64-lane wave), and unknown tokens
    on both sides of a sub-tile (256 tokens) and a block chunk (1024 tokens)."""
    # "a" * k is k tokens in every tier ("▁a", then "a"s), so the first line's
    # unknown chars are tokens SUB - 2 .. SUB and the second's TILE - 2 .. TILE
    # of the batch (test_epilogue_shapes checks that on the device's tokens).
    lines = ["a" * (SUB - 2) + "あいう", "a" * (TILE - SUB - 3) + "あ😀い"]
    lines += ["いab the 😀", "", "い", "abい", "😀😀ab😀", "", "あ" * 300, "ab 吾輩は猫であ吾い<0x41> q", " ", ""]
    for pad in range(TILE - 6, TILE + 3):
        lines.append("a" * pad + "あ😀い")
    lines += ["", "b" * (2 * TILE) + "う", "い"]
    return lines


_SHAPES = {}


def _shape_reference(tier):
    """The package's ids of shape_lines() for every option list, computed once."""
    if tier not in _SHAPES:
        pieces, mtype, variant, knob = TIERS[tier]
        mbytes = R.hand_model(pieces, model_type=mtype)
        sp = sentencepiece.SentencePieceProcessor(model_proto=mbytes)
        plain = sp.encode(shape_lines(), out_type=int)
        # ApplyExtraOptions over the package's rows (its Python binding takes
        # only the flags add_bos / add_eos / reverse, applied as "reverse:bos:eos").
        want = {o: [R.apply_options(r, o, sp.bos_id(), sp.eos_id()) for r in plain] for o in OPTIONS}
        assert want["reverse:bos:eos"] == sp.encode(shape_lines(), out_type=int, add_bos=True, add_eos=True, reverse=True)
        assert want["bos"] == sp.encode(shape_lines(), out_type=int, add_bos=True)
        _SHAPES[tier] = (mbytes, want)
    return _SHAPES[tier]


class Encoded:
    """shape_lines() normalized and encoded on the device (model-level tokens)."""

    def __init__(self, dm, lines):
        import torch
        dev = _dev()
        buf, off = S.to_csr(lines)
        self.n = n = len(lines)
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        d_in = torch.from_numpy(buf).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        cap = int(off[-1]) * 3 + 3 * n + 16
        self.d_norm = torch.empty(cap, dtype=torch.uint8, device=dev)
        self.d_noff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        tot = ctypes.c_uint64()
        S._check(dm._L.spm_hip_normalize_batch_device(dm.h, d_in.data_ptr(), d_off.data_ptr(), n, self.d_norm.data_ptr(),
                                                      cap, self.d_noff.data_ptr(), ctypes.byref(tot), self.stream))
        self.total = tot.value
        self.d_ids = torch.empty(max(self.total, 1), dtype=torch.int32, device=dev)
        self.d_len = torch.empty(max(self.total, 1), dtype=torch.int32, device=dev)
        self.d_tok = torch.empty(n + 1, dtype=torch.int64, device=dev)
        dm.encode_device(self.d_norm.data_ptr(), self.d_noff.data_ptr(), n, self.d_ids.data_ptr(),
                         self.d_tok.data_ptr(), d_len=self.d_len.data_ptr(), stream=self.stream)
        torch.cuda.synchronize(dev)

    def finalize(self, dm, options, capacity, status=None):
        """-> (rows or None, out buffer, offsets buffer, total or status)."""
        import torch
        dev = _dev()
        d_out = torch.full((capacity + 64,), CANARY, dtype=torch.int32, device=dev)
        d_oo = torch.full((self.n + 1,), CANARY, dtype=torch.int64, device=dev)
        args = (options, self.d_ids.data_ptr(), self.d_len.data_ptr(), self.d_tok.data_ptr(), self.n,
                self.d_norm.data_ptr(), self.d_noff.data_ptr(), d_out.data_ptr(), capacity, d_oo.data_ptr())
        if status is None:
            total = dm.finalize_ids_bytes_device(*args, stream=self.stream)
        else:
            d_st = torch.full((1,), status, dtype=torch.int32, device=dev)
            dm.finalize_ids_bytes_device_async(*args, d_st.data_ptr(), stream=self.stream)
            torch.cuda.synchronize(dev)
            total = int(d_st.item())
        torch.cuda.synchronize(dev)
        return d_out.cpu().numpy(), d_oo.cpu().numpy(), total


def _rows(out, oo):
    return [out[int(oo[i]):int(oo[i + 1])].tolist() for i in range(len(oo) - 1)]


@pytest.mark.parametrize("tier", list(TIERS))
def test_epilogue_shapes(tier):
    pieces, mtype, variant, knob = TIERS[tier]
    mbytes, want = _shape_reference(tier)
    dm = S.DeviceModel(mbytes)
    assert dm.info().fast_variant == variant and dm.byte_fallback() is not None
    if knob == "coop":
        dm.set_coop_min_nb(1)
    if knob == "general":
        dm.set_force_general(True)
    lines = [l.encode() for l in shape_lines()]
    enc = Encoded(dm, lines)
    tok = enc.d_tok.cpu().numpy()
    assert int(tok[-1]) > 2 * TILE  # more than one block's chunk
    unk = enc.d_ids.cpu().numpy()[:int(tok[-1])] == 0
    for edge in (SUB, TILE):  # expanded tokens on both sides of a sub-tile and of a block's chunk
        assert unk[edge - 2:edge + 1].all()
    n_extra = {o: sum(1 for x in o.split(":") if x in ("bos", "eos")) for o in OPTIONS}
    for o in OPTIONS:
        cap = enc.total + enc.n * n_extra[o]  # the documented bound
        out, oo, total = enc.finalize(dm, o, cap)
        assert total == sum(len(r) for r in want[o]) and int(oo[-1]) == total
        assert _rows(out, oo) == want[o], o
        assert (out[total:] == CANARY).all()
        out, oo, status = enc.finalize(dm, o, cap, status=0)  # the pure stream entry
        assert status == 0 and _rows(out, oo) == want[o] and (out[total:] == CANARY).all()
    # the old entry names the new one
    with pytest.raises(S.SpmError) as e:
        dm.finalize_ids_device("", enc.d_ids.data_ptr(), enc.d_tok.data_ptr(), enc.n, 0, 0, enc.d_tok.data_ptr())
    assert e.value.code == S.SPM_INVALID_ARGUMENT and "spm_hip_finalize_ids_bytes" in str(e.value)
    assert dm.encode_raw_small(lines[:4]) is None  # SPM_UNIMPLEMENTED: callers take the batch path
    # SentencePieceText of the same lines against the package
    sp = sentencepiece.SentencePieceProcessor(model_proto=mbytes)
    po, p, _, _ = _encode_spt(dm, lines, "bos:reverse")
    rows = [R.apply_options([(x.id, x.begin, x.end) for x in sp.encode(l, out_type="proto").pieces], "bos:reverse",
                            (sp.bos_id(), 0, 0), (sp.eos_id(), 0, 0)) for l in shape_lines()]
    assert [[tuple(int(v) for v in r[:3]) for r in p[int(po[i]):int(po[i + 1])]] for i in range(len(lines))] == rows


def test_epilogue_capacity_and_status_word():
    tier = "unigram byte"
    mbytes, want = _shape_reference(tier)
    dm = S.DeviceModel(mbytes)
    enc = Encoded(dm, [l.encode() for l in shape_lines()])
    total = sum(len(r) for r in want["bos:eos"])
    with pytest.raises(S.SpmError) as e:
        enc.finalize(dm, "bos:eos", total - 1)
    assert e.value.code == S.SPM_RESOURCE_EXHAUSTED and e.value.total == total
    out, oo, status = enc.finalize(dm, "bos:eos", total - 1, status=0)
    assert status == S.SPM_RESOURCE_EXHAUSTED and (out == CANARY).all()  # nothing written
    assert int(oo[-1]) == total                                         # ... but the size a second call needs
    out, oo, status = enc.finalize(dm, "bos:eos", total, status=0)       # capacity == total succeeds
    assert status == 0 and _rows(out, oo) == want["bos:eos"]
    out, oo, status = enc.finalize(dm, "bos:eos", total, status=3)       # an earlier call of the chain failed
    assert status == 3 and (out == CANARY).all() and (oo == CANARY).all()


# ---- decode shapes ----

def _decode_model():
    return R.hand_model(BASE)


B = R.FIRST_BYTE_ID
F = B + 256 + 1  # "a"
SEQS = ([0xE6, 0x97, 0xA5], [0xF0, 0x9F, 0x98, 0x80], [0xC3, 0xA9])


def decode_rows():
    rows = []
    for edge in (SUB, TILE):  # every look-back / look-ahead distance across a sub-tile and a block edge
        for seq in SEQS:
            for d in range(len(seq) + 1):
                pad = (edge - d - sum(len(r) for r in rows)) % edge  # d bytes of seq before the edge, the rest after
                rows.append([F] * pad + [B + b for b in seq] + [F])
    rows += [
        [F, B + 0xE6, B + 0x97], [B + 0xA5, F],          # a run split across two sentences: three U+FFFD
        [B + 0xA5, B + 0x97, B + 0xE6],                  # valid when reversed
        [B + 0xE6, B + 0x97], [B + 0x97, B + 0xE6, B + 0x97, B + 0xA5, B + 0x41], [B + 0xC0, B + 0x80],
        [B + 0xED, B + 0xA0, B + 0x80], [B + 0xF0, B + 0x9F, B + 0x98, B + 0x80], [B + 0xF4, B + 0x90, B + 0x80, B + 0x80],
        [B + 0xE6, B + 256 + 3, B + 0x97, B + 0xA5],     # the run ends at a non-byte piece
        [B + 0x20, B + 0x41], [B + 0xE2, B + 0x96, B + 0x81, B + 0x41],  # no space conversion, no strip
        [B + 256, B + 0xE6, B + 0x97, B + 0xA5, B + 256 + 3],  # leading-U+2581 rule around a byte surface
        [B + 0xE6, B + 0x97, B + 256 + 3], [], [B + 0xFF], [0, B + 0x41, 0], [1, B + 0xE6, 2, B + 0x97, B + 0xA5],
        [B + 0xEF, B + 0xBF, B + 0xBD],
    ]
    return rows


@pytest.mark.parametrize("options", ["", "reverse", "bos:eos", "reverse:bos:eos"])
def test_decode_shapes(options):
    mbytes = _decode_model()
    dm = S.DeviceModel(mbytes)
    rows = decode_rows()
    ids, off = D.C.to_csr(rows)
    assert int(off[-1]) > 2 * TILE
    ref = R.Model(mbytes)
    want_text, want_off, want_begins = ref.decode_batch(ids, off, options)
    for entry in ("blocking", "async"):  # (D._decode also makes the count-only call and compares its offsets)
        assert D._decode(dm, ids, off, options, entry) == (want_text, want_off, want_begins)
    text, out_off, begins = dm.decode_csr_host(ids, off, options, with_begin=True)
    assert (text.tobytes(), out_off.tolist(), begins.tolist()) == (want_text, want_off, want_begins)
    # The bound covers a byte token's 4 bytes (here the 5 bytes of unk_surface are the longest surface).
    assert dm.decode_bound() == 5 and len(want_text) <= (int(off[-1]) + 2 * len(rows)) * dm.decode_bound()
    assert S.DeviceModel(R.hand_model([("a", -1.0, mb.NORMAL)]) + mb._ld(2, mb._ld(44, b""))).decode_bound() == 4
    # the restatement against the package on these very rows
    sp = sentencepiece.SentencePieceProcessor(model_proto=mbytes)
    sp_rows = rows if options == "" else None
    if sp_rows is not None:
        assert b"".join(sp.decode(r).encode() for r in sp_rows) == want_text
    if options == "":
        at = [i for i, r in enumerate(rows) if r == [F, B + 0xE6, B + 0x97]][0]
        assert want_text[want_off[at]:want_off[at + 2]] == b"a" + R.FFFD * 3 + b"a"
    if options == "reverse":
        at = [i for i, r in enumerate(rows) if r == [B + 0xA5, B + 0x97, B + 0xE6]][0]
        assert want_text[want_off[at]:want_off[at + 1]] == "日".encode()


# ---- trainer ----

def _train(tmp_path, tag, args):
    prefix = str(tmp_path / tag)
    p = subprocess.run([TRAIN, "--input=" + os.path.join(R.GOLD, "botchan.txt"), "--model_prefix=" + prefix] + args,
                       capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    return open(prefix + ".model", "rb").read(), open(prefix + ".vocab", "rb").read()


@pytest.mark.parametrize("mtype,extra", [("unigram", ["--vocab_size=1000"]), ("bpe", ["--vocab_size=1000"]),
                                         ("char", ["--vocab_size=400"])])
def test_spm_train_byte_fallback(mtype, extra, tmp_path):
    args = ["--model_type=" + mtype, "--character_coverage=0.98"] + extra
    placeholders = ["<ph%03d>" % b for b in range(256)]
    got, vocab = _train(tmp_path, "bf", args + ["--byte_fallback=true"])
    ref, _ = _train(tmp_path, "ph", args + ["--control_symbols=" + ",".join(placeholders)])
    # Piece for piece and score bit for score bit: the placeholder rows renamed and retyped.
    want = [(R.byte_piece(placeholders.index(p.decode())), s, R.BYTE) if p.decode() in placeholders else (p, s, t)
            for p, s, t in R.read_pieces(ref)]
    have = R.read_pieces(got)
    assert [(p, np.float32(s).tobytes(), t) for p, s, t in have] == [(p, np.float32(s).tobytes(), t) for p, s, t in want]
    assert sum(1 for _, _, t in have if t == R.BYTE) == 256
    assert [p for p, _, _ in have[:4]] == [b"<unk>", b"<s>", b"</s>", b"<0x00>"]
    flag = [w for f, wt, v in R.model_reader.fields(got) if f == 2 and wt == 2
            for g, gt, w in R.model_reader.sub_fields(v) if g == 35]
    assert flag == [1]
    assert not [1 for f, wt, v in R.model_reader.fields(ref) if f == 2 and wt == 2
                for g, gt, w in R.model_reader.sub_fields(v) if g == 35]  # absent unless the flag is on
    assert b"<0x41>\t0\n" in vocab
    # The package loads the result and encodes as this engine does.
    sp = sentencepiece.SentencePieceProcessor(model_proto=got)
    lines = R.corpus_lines("botchan.txt")[:200] + R.corpus_lines("wagahaiwa_nekodearu.txt")[:50]
    want_ids = sp.encode([l.decode() for l in lines], out_type=int)
    assert any(sp.is_byte(i) for r in want_ids for i in r)
    if mtype == "char":  # CHAR models' ids take the processor's host epilogue
        src = tmp_path / "lines.txt"
        src.write_bytes(b"".join(l + b"\n" for l in lines))
        q = subprocess.run([ENCODE, "--model=" + str(tmp_path / "bf.model"), "--output_format=id", str(src)],
                           capture_output=True, timeout=300)
        assert q.returncode == 0, q.stderr[-2000:]
        assert q.stdout == "".join(" ".join(str(i) for i in r) + "\n" for r in want_ids).encode()
    else:
        assert S.DeviceModel(got).encode_lines_device(lines) == want_ids


# ---- sample and n-best ----

def _short_lines():
    lines = [l for l in R.corpus_lines("botchan.txt") if 0 < len(l) < 60][:24]
    return lines + ["aあいb".encode(), "the 日本 cat".encode(), "😀".encode(), b"<0x41> q"]


def test_nbest_and_sample_expand_every_path(tmp_path):
    """NBestEncode and SampleEncode of the processor (spm_encode) equal the
    model-level paths of nbest_ref.py / the device sampler (each a path of
    sample_ref.py's lattice) plus the expansion."""
    import nbest_ref as NB
    import sample_ref
    name = R.FIXTURES[0]
    mbytes, dm = _fixture(name)
    model = os.path.join(R.GOLD, name + ".model")
    rm = sample_ref.Model(R.control_view(mbytes))  # the lattice does not change: BYTE rows are reserved
    bids, unk = R.byte_ids(mbytes), R.Model(mbytes).unk_id
    lines = _short_lines()
    norm = dm.normalize(lines)
    src = tmp_path / "lines.txt"
    src.write_bytes(b"".join(l + b"\n" for l in lines))

    def expanded(ids, lens, s):
        return [r[0] for r in R.expand(ids, lens, s, unk, bids)]

    want = [[expanded(p[0], p[1], s) for p in NB.nbest(rm, s, 3)[0]] for s in norm]
    assert any(i in bids for paths in want for p in paths for i in p)
    q = subprocess.run([ENCODE, "--model=" + model, "--output_format=nbest_id", "--nbest_size=3", str(src)],
                       capture_output=True, timeout=300)
    assert q.returncode == 0, q.stderr[-2000:]
    assert q.stdout == "".join(" ".join(str(i) for i in p) + "\n" for paths in want for p in paths).encode()
    q = subprocess.run([ENCODE, "--model=" + model, "--output_format=nbest_piece", "--nbest_size=3", str(src)],
                       capture_output=True, timeout=300)
    assert q.returncode == 0, q.stderr[-2000:]
    pieces = R.read_pieces(mbytes)
    assert q.stdout == b"".join(b" ".join(pieces[i][0] for i in p) + b"\n" for paths in want for p in paths)

    seed, theta = 20240611, 0.5
    buf, off = S.to_csr(norm)
    ids, lens, to = dm.sample_encode_csr_host(buf, off, theta, seed, with_lens=True)
    rows = []
    for i, s in enumerate(norm):
        a, b = int(to[i]), int(to[i + 1])
        assert rm.is_path(s, ids[a:b].tolist(), lens[a:b].tolist())
        rows.append(expanded(ids[a:b], lens[a:b], s))
    q = subprocess.run([ENCODE, "--model=" + model, "--output_format=sample_id", "--nbest_size=-1", "--alpha=%r" % theta,
                        "--random_seed=%d" % seed, str(src)], capture_output=True, timeout=300)
    assert q.returncode == 0, q.stderr[-2000:]
    assert q.stdout == "".join(" ".join(str(i) for i in r) + "\n" for r in rows).encode()
