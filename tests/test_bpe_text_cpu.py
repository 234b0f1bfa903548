"""CPU: word-closedness of BPE models (spm_hip_model_bpe_word_closed) on
host-only handles: every piece is "▁"* followed by chars other than "▁"."""
import os

import pytest

import bpe_cases as C
import bpe_text_cases as T
import spm_amd as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fixture(name):
    return open(os.path.join(GOLD, name), "rb").read()


@pytest.mark.parametrize("blob,closed", [
    (lambda: _fixture("botchan_bpe1k.model"), True),
    (lambda: _fixture("botchan_bf_bpe1k.model"), True),
    (T.hand_model, True),
    (lambda: C.build_model().blob, False),           # merges of any two pieces: "a▁", "▁b▁", ...
    (lambda: T.hand_model(extra=["a▁b"]), False),
], ids=["botchan", "botchan_bf", "hand", "bpe_cases", "hand_plus_a_ws_b"])
def test_word_closed(blob, closed):
    assert S.DeviceModel(blob(), host_only=True).bpe_word_closed() is closed


def test_word_closed_is_for_bpe_models():
    with pytest.raises(S.SpmError) as e:
        S.DeviceModel(_fixture("test_model.model"), host_only=True).bpe_word_closed()
    assert e.value.code == S.SPM_INVALID_ARGUMENT
