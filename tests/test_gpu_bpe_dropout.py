"""GPU: spm_hip_bpe_dropout_encode_batch against the Python restatement
(bpe_dropout_ref.py), draw for draw.

Ids, piece lengths and token offsets are compared bit for bit, once through
the one-sentence-per-wave kernel with the general kernel behind it and once
with every sentence on the general kernel (set_force_general); the hand models
of bpe_cases add tied scores, UNUSED pieces (flag + resegment) and an
irregular vocabulary, the sentences sit on the wave kernel's bounds (128 and
1024 bytes) and on the Encode tiers' limits."""
import os

import numpy as np
import pytest

import bpe_cases as C
import bpe_dropout_ref as R
import oracle_lib as O
import spm_amd as S
import vocab_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 20241


def _read(name):
    with open("%s/%s" % (GOLD, name), "rb") as f:
        return f.read()


def _long(nb):
    """nb bytes of vocabulary chars of 1 to 4 bytes, ASCII to fill."""
    s = ("ab" + "é" + "あ" + "😀" + "abcab") * (nb // 15 + 1)
    b = s.encode()[:nb]
    while True:
        try:
            b.decode()
            break
        except UnicodeDecodeError:
            b = b[:-1]
    return b + b"a" * (nb - len(b))


def hand_sentences():
    out = C.batch("shuffled") + C.edge_sentences() + C.malformed() + [v[0] for v in C.limits().values()]
    out += [_long(n) for n in (127, 128, 129, 1023, 1024, 1025)]
    return out


class _Loaded:
    def __init__(self, blob, types=None):
        self.dm = S.DeviceModel(blob)
        self.ref = R.Model(blob, types)
        self.want = {}

    def expect(self, sents, alpha, seed, base):
        ids, lens, to = [], [], [0]
        for k, s in enumerate(sents):
            key = (s, alpha, seed, base + k)
            if key not in self.want:
                self.want[key] = R.encode(self.ref, s, alpha, seed, base + k)
            i, l = self.want[key]
            ids += i
            lens += l
            to.append(len(ids))
        return np.array(ids, np.int32), np.array(lens, np.uint32), np.array(to, np.uint64)

    def run(self, sents, alpha, seed=SEED, base=0, force_general=False):
        self.dm.set_force_general(force_general)
        try:
            buf, off = S.to_csr(sents)
            got = self.dm.bpe_dropout_encode_csr_host(buf, off, alpha, seed, index_base=base, with_lens=True)
            return got, self.dm.stats()
        finally:
            self.dm.set_force_general(False)

    def check(self, sents, alpha, seed=SEED, base=0):
        """Both routes equal the restatement (hence each other); returns the
        stats of the routed call."""
        wids, wlens, wto = self.expect(sents, alpha, seed, base)
        stats = None
        for force in (False, True):
            (ids, lens, to), st = self.run(sents, alpha, seed, base, force)
            bad = np.nonzero(to != wto)[0]
            assert bad.size == 0, "force_general=%s: token offsets differ first after sentence %d: %r" % (
                force, bad[0] - 1, sents[bad[0] - 1])
            for name, got, exp in (("ids", ids, wids), ("piece lengths", lens, wlens)):
                bad = np.nonzero(got != exp)[0]
                if bad.size:
                    k = int(np.searchsorted(wto, bad[0], side="right")) - 1
                    raise AssertionError("force_general=%s: %s differ at token %d (sentence %d: %r): got %d, want %d"
                                         % (force, name, bad[0], k, sents[k], got[bad[0]], exp[bad[0]]))
            assert st.sentences == len(sents)
            if force:
                assert st.general_path == len(sents)
            else:
                stats = st
        return stats


@pytest.fixture(scope="module")
def botchan():
    blob = _read("botchan_bpe1k.model")
    m = _Loaded(blob)
    norm = m.dm.normalize(O.read_lines_binary("%s/botchan.txt" % GOLD)[:600])
    return m, norm


@pytest.fixture(scope="module")
def hand():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Loaded(C.build_model(**{name: True}).blob)
        return cache[name]

    yield get
    cache.clear()


@pytest.mark.parametrize("alpha", [0.1, 0.5])
def test_botchan_draws_equal_the_restatement(botchan, alpha):
    m, norm = botchan
    st = m.check(norm, alpha)
    assert st.general_path == sum(len(s) > 1024 for s in norm)


@pytest.mark.parametrize("name", ["ties", "unused", "irregular"])
def test_hand_models_draws_equal_the_restatement(hand, name):
    m = hand(name)
    sents = hand_sentences()
    for alpha in (0.1, 0.5):
        st = m.check(sents, alpha)
        over = sum(len(s) > 1024 for s in sents)
        assert st.general_path >= over
        if name == "ties":
            assert st.general_path == over  # nothing else is refused
        else:
            assert st.general_path > over   # UNUSED probes / chars outside the vocabulary are flagged


def test_alpha_zero_is_encode_and_alpha_one_the_initial_split(botchan, hand):
    for m, sents in [(botchan[0], botchan[1])] + [(hand(n), hand_sentences()) for n in ("ties", "unused", "irregular")]:
        buf, off = S.to_csr(sents)
        want = m.dm.encode_csr_host(buf, off, with_lens=True)
        for force in (False, True):
            for alpha in (0.0, -1.0, float("-inf")):
                got, _ = m.run(sents, alpha, force_general=force)
                for g, w in zip(got, want):
                    assert np.array_equal(g, w), (alpha, force)
            for alpha in (1.0, 3.0, float("inf")):
                (ids, lens, to), _ = m.run(sents, alpha, force_general=force)
                wl = []
                for s in sents:
                    st = C.walk_starts(s)
                    wl += [b - a for a, b in zip(st, st[1:] + [len(s)])]
                assert np.array_equal(lens, np.array(wl, np.uint32)), (alpha, force)
                assert np.array_equal(to, np.cumsum([0] + [C.n_chars(s) for s in sents]).astype(np.uint64))
    # ... and the ids of the initial split are the restatement's.
    m, sents = hand("unused"), hand_sentences()
    m.check(sents, 1.0)


def test_a_row_depends_on_its_global_index_only(botchan):
    m, norm = botchan
    sents = norm[:200]
    alpha = 0.5
    (ids, lens, to), _ = m.run(sents, alpha, base=1000)
    rows = [(ids[int(to[k]):int(to[k + 1])].tolist(), lens[int(to[k]):int(to[k + 1])].tolist())
            for k in range(len(sents))]
    for k in (0, 1, 63, 64, 199):  # alone, at its own index
        (i1, l1, t1), _ = m.run([sents[k]], alpha, base=1000 + k)
        assert (i1.tolist(), l1.tolist()) == rows[k], k
    # Shuffled: sentence j of the new batch sits at index 1000 + j, so the
    # row of a sentence that keeps its position is unchanged and every row is
    # the restatement's for (sentence, new index).
    perm = np.random.RandomState(3).permutation(len(sents))
    shuffled = [sents[j] for j in perm]
    m.check(shuffled, alpha, base=1000)
    (ids2, lens2, to2), _ = m.run(shuffled, alpha, base=1000)
    for j, k in enumerate(perm):
        if j == k:
            assert ids2[int(to2[j]):int(to2[j + 1])].tolist() == rows[k][0]
    # 64 copies of one sentence in one call are 64 draws.
    (ids, lens, to), _ = m.run([sents[5]] * 64, alpha)
    distinct = {tuple(ids[int(to[k]):int(to[k + 1])].tolist()) for k in range(64)}
    assert len(distinct) >= 2


def test_frequencies_match_the_exact_path_probabilities(botchan):
    m, _ = botchan
    s = "▁the▁teacher".encode()
    n = 50000
    for alpha in (0.1, 0.5):
        (ids, lens, to), _ = m.run([s] * n, alpha, seed=SEED + 1)
        counts = {}
        for k in range(n):
            a, b = int(to[k]), int(to[k + 1])
            key = (tuple(ids[a:b].tolist()), tuple(lens[a:b].tolist()))
            counts[key] = counts.get(key, 0) + 1
        probs = R.path_probabilities(m.ref, s, alpha)
        assert set(counts) <= set(probs)
        dev = R.binned_deviation(probs, counts, n)
        print("alpha %.1f: %d segmentations drawn, worst deviation %.2f sigma" % (alpha, len(counts), dev))
        assert dev <= 5.0, (alpha, dev)


def test_restricted_vocabulary(botchan):
    blob = _read("botchan_bpe1k.model")
    pieces = R.byte_fallback_ref.read_pieces(blob)
    vocab = [p for k, (p, _, t) in enumerate(pieces) if k % 2 == 0]
    types = vocab_ref.set_vocabulary(pieces, vocab)
    assert vocab_ref.UNUSED in types
    m = _Loaded(blob, types)
    m.dm.set_vocabulary(vocab)
    sents = botchan[1][:300]
    for alpha in (0.1, 0.5):
        st = m.check(sents, alpha)
        assert st.general_path > 0  # UNUSED probes go to the general kernel's resegmentation


def test_device_pointer_call(botchan):
    import torch
    m, norm = botchan
    sents = norm[:300]
    buf, off = S.to_csr(sents)
    dev = torch.device("cuda", 0)
    d_b = torch.from_numpy(buf).to(dev)
    d_o = torch.from_numpy(off.view(np.int64)).to(dev)
    cap = max(int(off[-1]), 1)
    d_ids = torch.empty(cap, dtype=torch.int32, device=dev)
    d_len = torch.empty(cap, dtype=torch.int32, device=dev)
    d_tok = torch.empty(len(sents) + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    m.dm.bpe_dropout_encode_device(d_b.data_ptr(), d_o.data_ptr(), len(sents), 0.5, SEED, d_ids.data_ptr(),
                                   d_tok.data_ptr(), index_base=17, d_len=d_len.data_ptr())
    (ids, lens, to), _ = m.run(sents, 0.5, base=17)
    assert np.array_equal(d_tok.cpu().numpy().view(np.uint64), to)
    k = int(to[-1])
    assert np.array_equal(d_ids.cpu().numpy()[:k], ids)
    assert np.array_equal(d_len.cpu().numpy().view(np.uint32)[:k], lens)
    # Without piece lengths.
    d_ids.zero_()
    m.dm.bpe_dropout_encode_device(d_b.data_ptr(), d_o.data_ptr(), len(sents), 0.5, SEED, d_ids.data_ptr(),
                                   d_tok.data_ptr(), index_base=17)
    assert np.array_equal(d_ids.cpu().numpy()[:k], ids)


def test_status_codes(botchan):
    buf, off = S.to_csr(["▁hello".encode()])
    uni = S.DeviceModel(_read("test_model.model"))
    with pytest.raises(S.SpmError) as e:
        uni.bpe_dropout_encode_csr_host(buf, off, 0.5, SEED)
    assert e.value.code == 12  # SPM_UNIMPLEMENTED: not a BPE model
    host = S.DeviceModel(_read("botchan_bpe1k.model"), host_only=True)
    with pytest.raises(S.SpmError) as e:
        host.bpe_dropout_encode_csr_host(buf, off, 0.5, SEED)
    assert e.value.code == 9  # SPM_FAILED_PRECONDITION
    dm = botchan[0].dm
    with pytest.raises(S.SpmError) as e:
        dm.bpe_dropout_encode_csr_host(buf, off, float("nan"), SEED)
    assert e.value.code == 3  # SPM_INVALID_ARGUMENT
    ids, to = dm.bpe_dropout_encode_csr_host(*S.to_csr([]), 0.5, SEED)
    assert ids.size == 0 and to.tolist() == [0]
    # The unigram sampler's entry keeps refusing a BPE model.
    with pytest.raises(S.SpmError) as e:
        dm.sample_encode_csr_host(buf, off, 0.5, SEED)
    assert e.value.code == 12
