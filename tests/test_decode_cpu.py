"""CPU: the decode rules.

  * tests/decode_ref.py (the restatement every decode test compares against)
    equals the `sentencepiece` package on all golden id rows, through the
    committed fixtures of tools/make_decode_golden.py;
  * it gives the known answers of the reference's DecodeTest
    (sentencepiece_processor_test.cc:466-604);
  * spm_hip_decode_batch_host on a host-only model (the plain C++ loop) equals
    the restatement on the golden rows and on the hand cases, text, offsets
    and piece begins, under every extra-option order.
"""
import numpy as np
import pytest

import decode_cases as C
import decode_ref
import spm_amd

WS = C.WS.encode()
OPTIONS = ["", "reverse", "bos:eos", "reverse:bos:eos", "bos:reverse", "eos:reverse:bos:bos"]


@pytest.fixture(scope="module")
def golden():
    out = {}
    for name, model in C.GOLDEN:
        mbytes = C.golden_model(model)
        out[name] = (mbytes, decode_ref.Model(mbytes), C.golden_rows(name), C.golden_texts(name))
    return out


@pytest.mark.parametrize("name", [g[0] for g in C.GOLDEN])
def test_restatement_equals_package_on_golden_rows(golden, name):
    _, ref, rows, texts = golden[name]
    assert len(rows) == len(texts) == {"botchan_test_model": 4288, "wagahaiwa_test_ja_model": 2344}[name]
    for r, want in zip(rows, texts):
        assert ref.decode_ids(r)[0] == want


INPUT = [b"<s>", WS + b"ABC", b"<unk>", WS + b"DE", b"F", b"G" + WS + b"H", b"I", b"</s>"]


def test_reference_decode_test_known_answers():
    ref = decode_ref.Model(C.base_model())
    text, rows = ref.decode_pieces(INPUT)
    assert text == b"ABC \xE2\x81\x87  DEFG HI"
    assert [r[0] for r in rows] == INPUT
    assert [r[2] for r in rows] == [b"", b"ABC", b" \xE2\x81\x87 ", b" DE", b"F", b"G H", b"I", b""]
    assert [(r[3], r[4]) for r in rows] == [(0, 0), (0, 3), (3, 8), (8, 11), (11, 12), (12, 15), (15, 16), (16, 16)]
    assert [r[1] for r in rows] == [1, 3, 0, 4, 5, 6, 0, 2]  # the out-of-vocabulary "I" has unk's id, its own bytes


@pytest.mark.parametrize("surface,want", [(b"", b"ABC DEFG HI"), (b"<UNK>", b"ABC<UNK> DEFG HI")])
def test_reference_decode_test_unk_surface(surface, want):
    ref = decode_ref.Model(C.base_model(surface))
    text, rows = ref.decode_pieces(INPUT)
    assert text == want and len(rows) == 8


def test_restatement_state_rules():
    ref = decode_ref.Model(C.hand_model())
    assert ref.decode_ids([C.BOS, C.BARE, C.BARE, C.ABC])[0] == b"ABC"
    assert ref.decode_ids([C.WSWSA])[0] == b" A"
    assert ref.decode_ids([C.BARE, C.UNK, C.ABC])[0] == b" \xE2\x81\x87  ABC"
    assert decode_ref.Model(C.hand_model(b"")).decode_ids([C.BARE, C.UNK, C.ABC])[0] == b"ABC"
    assert ref.decode_ids([C.WSLOWER, C.LOWER])[0] == "▂x▂y".encode()
    with pytest.raises(decode_ref.DecodeError, match='option "foo" is not available.'):
        ref.parse_options("bos:foo")


def _check_host(model_bytes, rows, options):
    ref = decode_ref.Model(model_bytes)
    dm = spm_amd.DeviceModel(model_bytes, host_only=True)
    ids, off = C.to_csr(rows)
    text, out_off, begin = dm.decode_csr_host(ids, off, options, with_begin=True)
    want_text, want_off, want_begin = ref.decode_batch(ids, off, options)
    assert bytes(text) == want_text
    assert out_off.tolist() == want_off
    assert begin.tolist() == want_begin
    return dm


@pytest.mark.parametrize("name", [g[0] for g in C.GOLDEN])
def test_host_loop_golden(golden, name):
    mbytes, _, rows, texts = golden[name]
    _check_host(mbytes, rows, "")
    dm = spm_amd.DeviceModel(mbytes, host_only=True)
    ids, off = C.to_csr(rows)
    text, out_off = dm.decode_csr_host(ids, off)
    assert bytes(text) == b"".join(texts)  # ... and the package itself


@pytest.mark.parametrize("options", OPTIONS)
@pytest.mark.parametrize("surface", [None, b"", b"<UNK>"])
def test_host_loop_hand_cases(surface, options):
    dm = _check_host(C.hand_model(surface), C.hand_rows(), options)
    assert dm.decode_bound() == max(len(C.LONG), len(surface if surface is not None else b" \xE2\x81\x87 "))


def test_host_loop_empty_batch_and_errors():
    dm = spm_amd.DeviceModel(C.hand_model(), host_only=True)
    text, out_off = dm.decode_csr_host(np.zeros(0, np.int32), np.zeros(1, np.uint64))
    assert text.size == 0 and out_off.tolist() == [0]
    ids, off = C.to_csr([[C.ABC], [C.DE, 16, -1]])
    with pytest.raises(spm_amd.SpmError) as e:
        dm.decode_csr_host(ids, off)
    assert e.value.code == spm_amd.SPM_OUT_OF_RANGE and "sentence 1" in str(e.value) and "id 16" in str(e.value)
    ids, off = C.to_csr([[C.ABC, C.DE]])
    with pytest.raises(spm_amd.SpmError) as e:
        dm.decode_csr_host(ids, off, capacity=5)  # "ABC DE" needs 6
    assert e.value.code == spm_amd.SPM_RESOURCE_EXHAUSTED
    assert bytes(dm.decode_csr_host(ids, off, capacity=6)[0]) == b"ABC DE"
    for bad, msg in (("foo", 'option "foo" is not available.'),):
        with pytest.raises(spm_amd.SpmError, match=msg):
            dm.decode_csr_host(ids, off, bad)


def test_bos_option_rejected_when_its_piece_is_unknown():
    import model_builder as mb
    model = mb.model([("<unk>", 0.0, mb.UNKNOWN), ("a", -1.0, mb.NORMAL)])
    dm = spm_amd.DeviceModel(model, host_only=True)
    ids, off = C.to_csr([[1]])
    with pytest.raises(spm_amd.SpmError, match="id for `<s>` is not defined."):
        dm.decode_csr_host(ids, off, "bos")
    with pytest.raises(decode_ref.DecodeError, match="id for `</s>` is not defined."):
        decode_ref.Model(model).parse_options("eos")
