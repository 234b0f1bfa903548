"""CPU: the n-best restatement (tests/nbest_ref.py) against the fixtures made
with the pip sentencepiece, the reference's own unit tests and exhaustive
enumeration, and the host implementation (csrc/host_nbest.h through `nbest_selftest host`)
against the restatement, bit for bit — no GPU calls."""
import os
import subprocess

import pytest

import nbest_ref as NB
import sample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PKG = os.path.join(ROOT, "sentencepiece-comments_amd")
SELFTEST = os.path.join(PKG, "lib", "nbest_selftest")


def _read(name):
    return open(os.path.join(GOLD, name), "rb").read()


@pytest.fixture(scope="module")
def S():
    import spm_amd
    spm_amd.lib()  # built by __graft_entry__.build(), like lib/nbest_selftest
    return spm_amd


def _normalized(S, model, text, count):
    lines = _read(text).split(b"\n")[:count]
    return S.DeviceModel(_read(model), host_only=True).normalize(lines)


@pytest.mark.parametrize("model,text,count,nbest,fixture", [
    ("test_model.model", "botchan.txt", 200, 5, "botchan_test_model.nbest5.gz"),
    ("test_ja_model.model", "wagahaiwa_nekodearu.txt", 60, 4, "wagahaiwa_test_ja_model.nbest4.gz")])
def test_restatement_reproduces_fixture(S, model, text, count, nbest, fixture):
    """The rows the pip sentencepiece wrote (tools/make_nbest_golden.py):
    path count, path order and tie order, independent of this project."""
    want, _ = NB.read_fixture(os.path.join(GOLD, fixture))
    assert len(want) == count
    rm = R.Model(_read(model))
    for nz, rows in zip(_normalized(S, model, text, count), want):
        paths, _ = NB.nbest(rm, nz, nbest)
        assert [NB.merge_unknown(p[0], rm.unk_id) for p in paths] == rows


@pytest.mark.parametrize("nbest", [3, 8])
def test_restatement_is_the_exact_top_n(S, nbest):
    """60 short sentences (up to 180 paths each): min(N, paths) distinct paths,
    and the exact top N wherever the N-th and (N+1)-th float64 totals differ
    by more than 1e-3 (all 60 of them, at both sizes)."""
    rm = R.Model(_read("test_model.model"))
    sents = NB.short_sentences(_normalized(S, "test_model.model", "botchan.txt", 300))
    clear = 0
    for s in sents:
        got = {(tuple(p[0]), tuple(p[1])) for p in NB.nbest(rm, s, nbest)[0]}
        total, want = NB.exact_top(rm, s, nbest)
        assert len(got) == min(nbest, total)
        if want is not None:
            clear += 1
            assert got == want, s
    assert 2 * clear >= len(sents)


def test_model_nbest_test():
    mb = NB.abc_model()
    rm = R.Model(mb)
    names = {3: "a", 4: "b", 5: "c", 6: "ab", 7: "bc", 8: "abc"}
    paths, _ = NB.nbest(rm, b"abc", 10)
    assert [" ".join(names[i] for i in p[0]) for p in paths] == NB.ABC_ORDER
    assert [float(p[2]) for p in paths] == [10.0, 5.0, 2.0, 0.0]
    assert [sum(p[1]) for p in paths] == [3, 3, 3, 3]
    one, _ = NB.nbest(rm, b"abc", 1)
    assert [names[i] for i in one[0][0]] == ["abc"]
    assert NB.nbest(rm, b"", 10)[0] == [([], [], 0.0)]


def _host(tmp_path, mb, sentences, nbest, shrink_at=None):
    path = tmp_path / "m.model"
    path.write_bytes(mb)
    cmd = [SELFTEST, "host", str(path), str(nbest)] + ([str(shrink_at)] if shrink_at else [])
    out = subprocess.run(cmd, input=b"".join(s + b"\n" for s in sentences), stdout=subprocess.PIPE, check=True)
    return NB.parse_selftest(out.stdout.decode())


def _check_host(tmp_path, mb, sentences, nbest, shrink_at=None, want_shrink=None):
    rm = R.Model(mb)
    got = _host(tmp_path, mb, sentences, nbest, shrink_at)
    assert len(got) == len(sentences)
    shrunk = 0
    for s, (paths, hyps, agenda, shrinks) in zip(sentences, got):
        want, (whyps, wagenda) = NB.nbest(rm, s, nbest, shrink_at or NB.MAX_AGENDA)
        assert paths == [(p[0], p[1], NB.score_bits(p[2])) for p in want], s
        assert (hyps, agenda) == (whyps, wagenda), s
        shrunk += shrinks
    if want_shrink is not None:
        assert (shrunk > 0) == want_shrink


@pytest.mark.parametrize("nbest", [5, 64])
def test_host_matches_restatement_botchan(S, tmp_path, nbest):
    # Lines are fed to the self-test one per row: botchan's normalized lines hold no newline.
    sents = [s for s in _normalized(S, "test_model.model", "botchan.txt", 100)]
    _check_host(tmp_path, _read("test_model.model"), sents, nbest, want_shrink=False)


def test_host_all_ties(S, tmp_path):
    _check_host(tmp_path, NB.ties_model(), [b"a" * 24], 64, want_shrink=False)


def test_host_shrink_default_threshold(S, tmp_path):
    # The agenda reaches 100 000 entries (182 179 hypotheses measured).
    _check_host(tmp_path, NB.ties_model(), [b"a" * 3000], 512, want_shrink=True)


def test_host_shrink_small_threshold(S, tmp_path):
    _check_host(tmp_path, NB.ties_model(), [b"a" * 400], 512, shrink_at=10000, want_shrink=True)
