"""What of the penalty / bias / seed options is decided on the host: the references' own known answers, the CSR of
:class:`LogitBias` and its validation, the seeds' layout, and the "all off" decision that keeps the old launches."""

import types

import pytest
import torch

from lite_llama_amd import _lib as L
from lite_llama_amd.sampling import (LogitBias, SamplingParams, _extras, _extras_off, resolve_sampling, row_seeds)
from tests import _penalties_ref as R


def test_python_philox_known_answers():
    R.check_known_answers()
    assert R.uniform_ref(0, 0) == (0x6627E8D5 >> 8) / 2 ** 24
    assert 0.0 <= R.uniform_ref(-1, 2 ** 32) < 1.0


def test_reference_rule_on_a_worked_example():
    z = torch.tensor([[4.0, -4.0, 1.0, 2.0]])
    ids = torch.tensor([[0, 0, 1, 7, 3]])
    mask = torch.tensor([[1, 1, 1, 1, 0]], dtype=torch.bool)
    out, counts, _ = R.penalties_ref(z, ids, mask, 2.0, 0.5, 0.25, {2: 1.5, 0: -2.0})
    assert counts.tolist() == [[2, 1, 0, 0]]
    # token 0: (4 - 2) / 2 - 0.5 - 0.5; token 1: -4 * 2 - 0.25 - 0.5; token 2: 1 + 1.5; token 3: masked out
    assert out.tolist() == [[0.0, -8.75, 2.5, 2.0]]


def test_the_library_exports_the_new_entries():
    assert len(L.SIGNATURES["ll_logit_penalties"]) == 23 and len(L.SIGNATURES["ll_seeded_uniform"]) == 5
    lib = L.lib()
    assert lib.ll_logit_penalties and lib.ll_seeded_uniform


def test_logit_bias_csr():
    one = LogitBias({5: 1.0, 2: float("-inf")}, 3, 8, "cpu")
    assert one.offsets.tolist() == [0, 2, 4, 6] and one.offsets.dtype == torch.int32
    assert one.ids.tolist() == [5, 2] * 3 and one.ids.dtype == torch.int32
    assert one.values.tolist() == [1.0, float("-inf")] * 3 and one.values.dtype == torch.float32
    rows = LogitBias([{1: 0.5}, None, {}, {0: -1.0, 7: 2.0}], 4, 8, "cpu")
    assert rows.offsets.tolist() == [0, 1, 1, 1, 3] and rows.ids.tolist() == [1, 0, 7]
    empty = LogitBias([None, None], 2, 8, "cpu")
    assert empty.offsets.tolist() == [0, 0, 0] and empty.ids.numel() >= 1
    assert LogitBias.of(None, 2, 8, "cpu") is None and LogitBias.of(rows, 4, 8, "cpu") is rows
    with pytest.raises(ValueError):
        LogitBias.of(rows, 3, 8, "cpu")


@pytest.mark.parametrize("bad", [{8: 1.0}, {-1: 1.0}, {1.5: 1.0}, {1: float("nan")}, {1: float("inf")}, [{1: 1.0}], "x",
                                 [{1: 1.0}, 3]])
def test_logit_bias_validation(bad):
    with pytest.raises(ValueError):
        LogitBias(bad, 2, 8, "cpu")


def test_row_seeds():
    assert row_seeds(None, 4, "cpu") is None
    assert row_seeds(7, 3, "cpu").tolist() == [7, 8, 9]
    assert row_seeds(2 ** 63 - 1, 2, "cpu").tolist() == [2 ** 63 - 1, -2 ** 63]       # wraps to int64
    assert row_seeds(-1, 2, "cpu").tolist() == [-1, 0]
    assert row_seeds([5, 5, -3], 3, "cpu").tolist() == [5, 5, -3]
    assert row_seeds(torch.tensor([1, 2]), 2, "cpu").dtype == torch.int64
    with pytest.raises(ValueError):
        row_seeds([1, 2], 3, "cpu")


def test_all_off_is_decided_without_reading_a_tensor():
    old = types.SimpleNamespace(temperature=1.0, top_p=0.9, repetition_penalty=1.1)
    assert _extras_off(*_extras(old)) and _extras_off(*_extras(SamplingParams()))
    assert _extras_off(0, 0.0, None) and _extras_off(None, None, None)
    assert not _extras_off(0.5, 0.0, None) and not _extras_off(0.0, -0.1, None) and not _extras_off(0.0, 0.0, {})
    assert not _extras_off(torch.zeros(2), 0.0, None)      # a tensor is never read: it counts as on
    # an object of the old shape and a neutral SamplingParams come back untouched, with no seeds
    assert resolve_sampling(old, 2, 8, "cpu") == (old, None)
    neutral = SamplingParams(temperature=0.7)
    assert resolve_sampling(neutral, 2, 8, "cpu") == (neutral, None)
    assert resolve_sampling(None, 2, 8, "cpu") == (None, None)


def test_resolve_builds_the_bias_once_on_a_copy():
    sp = SamplingParams(temperature=0.5, top_p=0.8, repetition_penalty=1.2, top_k=4, min_p=0.1, presence_penalty=0.3,
                        frequency_penalty=0.2, logit_bias={3: -1.0}, seed=11)
    got, seeds = resolve_sampling(sp, 2, 8, "cpu")
    assert got is not sp and isinstance(got.logit_bias, LogitBias) and isinstance(sp.logit_bias, dict)
    assert seeds.tolist() == [11, 12]
    for name in ("temperature", "top_p", "repetition_penalty", "top_k", "min_p", "presence_penalty", "frequency_penalty", "seed"):
        assert getattr(got, name) == getattr(sp, name)
    again, _ = resolve_sampling(got, 2, 8, "cpu")
    assert again is got
