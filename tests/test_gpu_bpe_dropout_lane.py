"""GPU: the lane tier of BPE-dropout (bpe_lane_dropout_kernel) against the Python restatement, draw for
draw, on the three lane layouts of bpe_cases; spm_hip_bpe_dropout_last_stats against the routing predictor."""
import os
import subprocess
import sys

import pytest

import bpe_cases as C
import bpe_dropout_ref as R
import oracle_lib as O
import spm_amd as S

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 20241
LAYOUTS = {"score": dict(order="score"), "shuffled": dict(order="shuffled"), "ties": dict(ties=True)}
layouts = pytest.mark.parametrize("layout", list(LAYOUTS))
alphas = pytest.mark.parametrize("alpha", [0.1, 0.5])
_ZOO = {}


def _model(**kw):
    """(device model, the restatement's model) of a bpe_cases model, made once."""
    key = tuple(sorted(kw.items()))
    if key not in _ZOO:
        blob = C.build_model(**kw).blob
        _ZOO[key] = S.DeviceModel(blob), R.Model(blob)
    return _ZOO[key]


def _split(ids, lens, to):
    return [(ids[int(a):int(b)].tolist(), lens[int(a):int(b)].tolist()) for a, b in zip(to, to[1:])]


def _rows(m, sents, alpha, base=0):
    return _split(*m[0].bpe_dropout_encode_csr_host(*S.to_csr(sents), alpha, SEED, index_base=base, with_lens=True))


def _check(m, sents, alpha, base=0):
    """Rows equal the restatement's; returns (lane_tier, wave_tier, literal)."""
    got = _rows(m, sents, alpha, base)
    for k, s in enumerate(sents):
        assert got[k] == R.encode(m[1], s, alpha, SEED, base + k), (k, s)
    lane, wave, lit = m[0].bpe_dropout_stats()
    assert lane + wave + lit == len(sents) and lit == m[0].stats().general_path
    return lane, wave, lit


def _lane(sents):
    return sum(C.first_kernel_takes(s, C.TIER_LANE_AFFINE) for s in sents)


@alphas
@layouts
def test_batches_are_routed_and_limits_alone_equal_their_row_in_the_pool(layout, alpha):
    m, pool = _model(**LAYOUTS[layout]), C.batch("shuffled")
    for arr in C.ARRANGEMENTS:
        for n in (1, 127, 128, 129, 257, None):
            sents = C.batch(arr, n)
            lane, wave, lit = _check(m, sents, alpha)
            assert (lane, lit) == (_lane(sents), sum(len(s) > 1024 for s in sents)), (arr, n)
    _check(m, pool, alpha, base=1000)
    inside = _rows(m, pool, alpha, base=1000)
    for name, (s, _, _) in C.limits().items():
        k = pool.index(s)
        assert _rows(m, [s], alpha, base=1000 + k) == [inside[k]], name
        assert m[0].bpe_dropout_stats()[0] == _lane([s]), name


_CHILD = """import sys; sys.path[:0] = [%r, %r]; import bpe_cases as C, spm_amd as S
dm = S.DeviceModel(C.build_model(%s=True).blob)
for alpha in (0.1, 0.5):
    dm.bpe_dropout_encode_csr_host(*S.to_csr(C.batch("shuffled")), alpha, %d)
    print(dm.stats().general_path)"""


@pytest.mark.parametrize("kind", ["unused", "irregular"])
def test_refusals_are_the_wave_kernels(kind):
    m, sents = _model(**{kind: True}), C.batch("shuffled")
    got = [_check(m, sents, alpha) for alpha in (0.1, 0.5)]
    assert all(0 < lane < _lane(sents) for lane, _, _ in got)  # the tier ran, and refused some of its own
    p = subprocess.run([sys.executable, "-c", _CHILD % (os.path.dirname(S.__file__), os.path.dirname(__file__), kind,
                                                        SEED)], env=dict(os.environ, SPM_HIP_BPE_DROPOUT_LANE="0"),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert [lit for _, _, lit in got] == list(map(int, p.stdout.split()))


@layouts
def test_alpha_zero_is_encode_and_alpha_one_the_initial_split(layout):
    m, sents = _model(**LAYOUTS[layout]), C.batch("shuffled")
    want = _split(*m[0].encode_csr_host(*S.to_csr(sents), with_lens=True))
    assert m[0].bpe_dropout_stats() == (0, 0, 0)  # not a dropout call
    assert _rows(m, sents, 0.0) == want and m[0].bpe_dropout_stats()[0] == _lane(sents)
    for s, (_, l) in zip(sents, _rows(m, sents, 1.0)):
        st = C.walk_starts(s)
        assert l == [b - a for a, b in zip(st, st[1:] + [len(s)])], s
    assert m[0].bpe_dropout_stats()[0] == _lane(sents)


def test_botchan_runs_both_tiers_in_one_call():
    blob = open(os.path.join(GOLD, "botchan_bpe1k.model"), "rb").read()
    m = S.DeviceModel(blob), R.Model(blob)
    norm = m[0].normalize(O.read_lines_binary(os.path.join(GOLD, "botchan.txt"))[:600])
    lane, wave, lit = _check(m, norm, 0.5)
    assert lane == _lane(norm) and 0 < lane < len(norm) and wave > 0
