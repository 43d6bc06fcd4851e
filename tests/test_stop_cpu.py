"""The stopping semantics on hand-written cases (tests/_stop_ref.py, the reference the GPU tests compare against) and
StopCriteria's validation.  No GPU."""

import pytest

from lite_llama_amd.executor import StopCriteria
from lite_llama_amd.executor import stopping as S
from tests import _stop_ref as R

PAD = 99


def _one(first, stream, **kw):
    toks, lengths, reasons = R.apply([first], [stream], pad=PAD, **kw)
    return toks[0], lengths[0], reasons[0]


def test_reason_numbers_match_the_module():
    assert (R.RUNNING, R.STOP_TOKEN, R.STOP_SEQUENCE, R.MAX_TOKENS) == (
        S.REASON_RUNNING, S.REASON_STOP_TOKEN, S.REASON_STOP_SEQUENCE, S.REASON_MAX_TOKENS) == (0, 1, 2, 3)


@pytest.mark.parametrize("at", [0, 2, 4])
def test_stop_id_at_the_first_a_middle_and_the_last_step(at):
    stream = [1, 2, 3, 4, 5]
    toks, length, reason = _one(7, stream, stop_ids=[stream[at]])
    # the finishing token is kept and counted; pads after it
    assert (length, reason) == (at + 1, R.STOP_TOKEN)
    assert toks == stream[:at + 1] + [PAD] * (len(stream) - at - 1)


def test_sequence_completed_across_column_0():
    toks, length, reason = _one(7, [8, 1, 2], stop_seqs=[[7, 8]])
    assert (length, reason) == (1, R.STOP_SEQUENCE) and toks == [8, PAD, PAD]


def test_sequence_that_would_need_a_column_left_of_0_does_not_match():
    # [6, 7, 8] would match with a 6 in the prompt: the prompt never takes part
    toks, length, reason = _one(7, [8, 1, 2], stop_seqs=[[6, 7, 8]])
    assert (length, reason) == (3, R.RUNNING) and toks == [8, 1, 2]


def test_overlap_a_a_b_in_a_a_a_b():
    a, b = 3, 4
    toks, length, reason = _one(a, [a, a, b, 5], stop_seqs=[[a, a, b]])
    assert (length, reason) == (3, R.STOP_SEQUENCE) and toks == [a, a, b, PAD]
    # ... and entirely inside the returned tokens
    toks, length, reason = _one(9, [a, a, a, b, 5], stop_seqs=[[a, a, b]])
    assert (length, reason) == (4, R.STOP_SEQUENCE) and toks == [a, a, a, b, PAD]


def test_id_and_sequence_at_the_same_step_give_reason_1():
    _, length, reason = _one(7, [1, 2, 3], stop_ids=[2], stop_seqs=[[1, 2]])
    assert (length, reason) == (2, R.STOP_TOKEN)


def test_max_tokens_and_sequence_at_the_same_step_give_reason_2():
    _, length, reason = _one(7, [1, 2, 3], stop_seqs=[[1, 2]], max_tokens=[2])
    assert (length, reason) == (2, R.STOP_SEQUENCE)
    _, length, reason = _one(7, [1, 2, 3], stop_seqs=[[1, 3]], max_tokens=[2])
    assert (length, reason) == (2, R.MAX_TOKENS)


def test_first_token_that_is_a_stop_id_gives_length_0():
    toks, length, reason = _one(7, [1, 2, 3], stop_ids=[7])
    assert (length, reason) == (0, R.STOP_TOKEN) and toks == [PAD, PAD, PAD]
    # a one-token stop sequence is completed by a sampled token only: the prefill's token does not finish the row
    toks, length, reason = _one(7, [1, 7, 3], stop_seqs=[[7]])
    assert (length, reason) == (2, R.STOP_SEQUENCE) and toks == [1, 7, PAD]


def test_a_row_that_never_stops_and_rows_are_independent():
    toks, lengths, reasons = R.apply([7, 7], [[1, 2, 3], [1, 5, 3]], stop_ids=[5], pad=PAD)
    assert lengths == [3, 2] and reasons == [R.RUNNING, R.STOP_TOKEN]
    assert toks == [[1, 2, 3], [1, 5, PAD]]


def test_frozen_rows_advance_nothing():
    ref = R.StopRef([7, 7], stop_ids=[5], pad=PAD, positions=[4, 6], seq_lens=[5, 7], cur_select=[10, 11],
                    req_idx=[1, 0], table=[[0] * 12, [0] * 12])
    ref.advance([5, 1])        # row 0 finishes here and does not advance
    assert ref.positions == [4, 7] and ref.seq_lens == [5, 8] and ref.cur_select == [12, 13]
    assert ref.table[1] == [0] * 12 and ref.table[0][7] == 13 and ref.running == 1 and ref.fed == [5, 1]
    ref.advance([1, 2])        # frozen: fed the pad, its KV row still moves (rows reserved for it), the table does not
    assert ref.positions == [4, 8] and ref.seq_lens == [5, 9] and ref.cur_select == [14, 15]
    assert ref.table[1] == [0] * 12 and ref.table[0][8] == 15 and ref.fed == [PAD, 2]
    assert ref.finished == [1, 0] and ref.lengths == [1, 2] and ref.reasons == [R.STOP_TOKEN, R.RUNNING] and ref.step == 3


def test_limits_are_exported():
    assert (S.MAX_STOP_TOKEN_IDS, S.MAX_STOP_SEQUENCES, S.MAX_STOP_SEQUENCE_LEN) == (32, 16, 8)


def test_defaults():
    c = StopCriteria(stop_token_ids=[2])
    assert c.pad_token_id == 0 and c.check_every == 8 and c.max_tokens is None and c.stop_sequences == []
    StopCriteria(max_tokens=[3, 1]).validate(vocab_size=10, batch=2)      # max_tokens alone is a criterion
    StopCriteria(stop_token_ids=list(range(32)), stop_sequences=[[1] * 8] * 16).validate(64, 5)   # at the limits


@pytest.mark.parametrize("kw", [
    dict(),                                                  # no criterion at all
    dict(stop_sequences=[[1, 2], []]),                       # an empty sequence
    dict(stop_token_ids=list(range(33))),                    # each limit exceeded
    dict(stop_sequences=[[1]] * 17),
    dict(stop_sequences=[[1] * 9]),
    dict(max_tokens=[4, 0]),                                 # a value < 1
])
def test_construction_errors(kw):
    with pytest.raises(ValueError):
        StopCriteria(**kw)


@pytest.mark.parametrize("kw", [
    dict(stop_token_ids=[10]),                               # ids outside [0, vocab)
    dict(stop_token_ids=[-1]),
    dict(stop_sequences=[[1, 10]]),
    dict(stop_token_ids=[1], max_tokens=[4, 4, 4]),          # a count that differs from the batch
])
def test_errors_against_the_model_and_the_batch(kw):
    c = StopCriteria(**kw)
    with pytest.raises(ValueError):
        c.validate(vocab_size=10, batch=2)
