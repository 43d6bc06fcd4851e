"""The token log-probability kernel (csrc/logprobs.hip) against tests/_logprobs_ref.py: top ids exactly, log-probabilities
within ``2e-5 + 1e-6 * |reference|``.

Where the bound comes from: fp32 unit roundoff u = 6e-8; a sum of positive terms accumulated as at most ~150 sequential adds
per thread plus a tree has relative error <= ~160 u = 1e-5 in the worst case, which is the absolute error it leaves in
ln S; exp2, ln and the final subtraction add a few ulp of values <= 12 resp. of |logprob|.  Every entry of every case is
compared."""

import pytest
import torch

from lite_llama_amd.sampling import TokenLogprobs, greedy_argmax, token_logprobs
from tests import _logprobs_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = [1, 3, 64, 257, 2048]
VOCABS = [1, 63, 1000, 32000, 128256, 152064]
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
MAX_BYTES = 256 << 20  # products whose logits exceed this are skipped


def _check(logits, token_ids, k, what, ref=None):
    """``ref``: a reference computed for the same logits and tokens with at least ``k`` alternatives (the first ``k`` of a
    longer list are the list for ``k``)."""
    got = token_logprobs(logits, token_ids, k)
    chosen, top_lp, top_ids = ref if ref is not None else R.ref_logprobs(logits, token_ids, k)
    top_lp, top_ids = top_lp[:, :k], top_ids[:, :k]
    rows = logits.shape[0]
    assert got.top_ids.shape == (rows, 1, k) and got.top_logprobs.shape == (rows, 1, k)
    assert got.top_ids.dtype == torch.int64 and got.top_logprobs.dtype == torch.float32
    if k:
        assert torch.equal(got.top_ids[:, 0].cpu(), top_ids), (what, "top ids")
        R.assert_close_logprobs(got.top_logprobs[:, 0], top_lp, what + " top")
    if token_ids is None:
        assert got.chosen is None
    else:
        assert got.chosen.shape == (rows, 1) and got.chosen.dtype == torch.float32
        R.assert_close_logprobs(got.chosen[:, 0], chosen, what + " chosen")
    return got


SHAPES = [(r, v, d) for r in ROWS for v in VOCABS for d in DTYPES
          if r * v * torch.empty(0, dtype=d).element_size() <= MAX_BYTES]


@pytest.mark.parametrize("rows,vocab,dtype", SHAPES, ids=[f"{r}x{v}-{str(d)[6:]}" for r, v, d in SHAPES])
def test_shapes(rows, vocab, dtype):
    g = torch.Generator().manual_seed(rows * 1000003 + vocab)
    logits = (torch.randn(rows, vocab, generator=g) * 4).to(dtype).to(DEV)
    ids = torch.randint(0, vocab, (rows,), generator=g).to(DEV)
    ref = R.ref_logprobs(logits, ids, min(20, vocab))
    for k in (0, 1, 5, 20):
        if k > vocab:
            with pytest.raises(ValueError, match="exceeds the vocabulary"):
                token_logprobs(logits, ids, k)
            continue
        _check(logits, ids, k, f"{rows}x{vocab} {dtype} k={k}", ref)
        if k and (k == 5 or vocab < 5):
            _check(logits, None, k, f"{rows}x{vocab} {dtype} k={k} no token", (None,) + ref[1:])
    if vocab > 1:
        top1 = token_logprobs(logits, None, 1).top_ids[:, 0, 0]
        assert torch.equal(top1, greedy_argmax(logits))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("rows,vocab", [(3, 1000), (64, 152064), (300, 32000)])
def test_input_kinds(rows, vocab, dtype):
    g = torch.Generator().manual_seed(7 + rows)
    wide = (torch.randn(rows, vocab, generator=g) * 12).to(dtype)
    equal = torch.full((rows, vocab), -3.25).to(dtype)
    peak = (torch.randn(rows, vocab, generator=g) * 0.5).to(dtype)
    where = torch.randint(0, vocab, (rows,), generator=g)
    peak[torch.arange(rows), where] = peak.float().max(dim=1).values.to(dtype) + 40
    mixed = (torch.randn(rows, vocab, generator=g) * 4).to(dtype)
    mixed[0] = 1.0                                   # an all-equal row among ordinary ones
    mixed[rows - 1, vocab // 2] = mixed[rows - 1].float().max().to(dtype) + 40
    for name, z in (("randn*12", wide), ("all-equal", equal), ("peak+40", peak), ("mixed", mixed)):
        z = z.to(DEV)
        least = z.float().argmin(dim=1)              # the chosen token is (one of) the least likely
        ref = R.ref_logprobs(z, least, 20)
        for k in (0, 1, 5, 20):
            _check(z, least, k, f"{name} {rows}x{vocab} {dtype} k={k} least-likely", ref)
        _check(z, where.to(DEV), 20, f"{name} {rows}x{vocab} {dtype} k=20")
    got = token_logprobs(equal.to(DEV), None, 5)
    assert torch.equal(got.top_ids[:, 0].cpu(), torch.arange(5).expand(rows, 5))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("pad", [3, 24])
def test_row_stride(pad, dtype):
    """Rows that are slices of wider storage: ``pad = 24`` keeps every row 16-byte aligned (vector loads, the last one
    partial), ``pad = 3`` does not (element loads); the storage around the rows holds huge values that must not be read
    as logits."""
    for rows, vocab in ((5, 1000), (64, 40003), (9, 152064)):
        g = torch.Generator().manual_seed(pad + vocab)
        store = torch.full((rows, vocab + pad), 30000.0).to(dtype)
        store[:, :vocab] = (torch.randn(rows, vocab, generator=g) * 4).to(dtype)
        logits = store.to(DEV)[:, :vocab]
        assert logits.stride(0) == vocab + pad and not logits.is_contiguous()
        ids = torch.randint(0, vocab, (rows,), generator=g).to(DEV)
        _check(logits, ids, 20, f"stride {vocab}+{pad} {dtype}")
        flat = (torch.randn(rows * vocab + 1, generator=g) * 4).to(dtype).to(DEV)
        off = flat[1:].view(rows, vocab)  # contiguous rows, base not 16-byte aligned
        _check(off, ids, 5, f"offset base {vocab} {dtype}")


def _column_buffers(rows, t, k):
    return TokenLogprobs(torch.full((rows, t), 7.0, device=DEV), torch.full((rows, t, k), 7.0, device=DEV),
                         torch.full((rows, t, k), 7, dtype=torch.int64, device=DEV))


def _check_columns(buf, cases, k):
    """Columns 1..3 of the 5-column buffers hold cases 0..2; guard columns 0 and 4 still hold the fill value."""
    for guard in (0, 4):
        assert torch.all(buf.chosen[:, guard] == 7.0) and torch.all(buf.top_logprobs[:, guard] == 7.0)
        assert torch.all(buf.top_ids[:, guard] == 7)
    for c, (logits, ids) in enumerate(cases):
        chosen, top_lp, top_ids = R.ref_logprobs(logits, ids, k)
        assert torch.equal(buf.top_ids[:, c + 1].cpu(), top_ids)
        R.assert_close_logprobs(buf.top_logprobs[:, c + 1], top_lp, f"column {c} top")
        R.assert_close_logprobs(buf.chosen[:, c + 1], chosen, f"column {c} chosen")


@pytest.mark.parametrize("rows,vocab", [(4, 1000), (64, 152064)])
def test_column_addressing(rows, vocab):
    k = 5
    g = torch.Generator().manual_seed(11)
    cases = [((torch.randn(rows, vocab, generator=g) * 4).half().to(DEV), torch.randint(0, vocab, (rows,), generator=g).to(DEV))
             for _ in range(3)]
    buf = _column_buffers(rows, 5, k)
    # the views [:, 1:4] are [rows, 3] buffers with a guard column on either side
    view = TokenLogprobs(buf.chosen[:, 1:4], buf.top_logprobs[:, 1:4], buf.top_ids[:, 1:4])
    col = torch.zeros(1, dtype=torch.int64, device=DEV)
    for c, (logits, ids) in enumerate(cases):
        col.fill_(c)
        token_logprobs(logits, ids, k, out=view, column=col)
    _check_columns(buf, cases, k)
    # a column outside the buffers writes nothing
    before = (buf.chosen.clone(), buf.top_logprobs.clone(), buf.top_ids.clone())
    for c in (-1, 3):
        col.fill_(c)
        token_logprobs(cases[0][0], cases[0][1], k, out=view, column=col)
    torch.cuda.synchronize()
    assert torch.equal(buf.chosen, before[0]) and torch.equal(buf.top_logprobs, before[1]) and torch.equal(buf.top_ids, before[2])
    # without a column: column 0
    buf2 = _column_buffers(rows, 2, k)
    token_logprobs(cases[1][0], cases[1][1], k, out=buf2)
    assert torch.all(buf2.chosen[:, 1] == 7.0) and torch.all(buf2.top_ids[:, 1] == 7)
    R.assert_close_logprobs(buf2.chosen[:, 0], R.ref_logprobs(*cases[1], k)[0], "default column")


@pytest.mark.parametrize("rows,vocab", [(4, 1000), (64, 152064)])
def test_column_addressing_under_graph(rows, vocab):
    """One captured launch, the column incremented on the device between replays, the logits replaced between replays."""
    k = 5
    g = torch.Generator().manual_seed(12)
    cases = [((torch.randn(rows, vocab, generator=g) * 4).half().to(DEV), torch.randint(0, vocab, (rows,), generator=g).to(DEV))
             for _ in range(3)]
    buf = _column_buffers(rows, 5, k)
    view = TokenLogprobs(buf.chosen[:, 1:4], buf.top_logprobs[:, 1:4], buf.top_ids[:, 1:4])
    col = torch.zeros(1, dtype=torch.int64, device=DEV)
    logits, ids = cases[0][0].clone(), cases[0][1].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up writes column 0, which the first replay writes again
        token_logprobs(logits, ids, k, out=view, column=col)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        token_logprobs(logits, ids, k, out=view, column=col)
        col += 1
    for z, t in cases:
        logits.copy_(z)
        ids.copy_(t)
        graph.replay()
    torch.cuda.synchronize()
    assert int(col) == 3
    _check_columns(buf, cases, k)


def test_out_of_range_token_is_nan_in_its_row_only():
    for rows, vocab in ((6, 1000), (64, 152064)):
        g = torch.Generator().manual_seed(13)
        logits = (torch.randn(rows, vocab, generator=g) * 4).half().to(DEV)
        ids = torch.randint(0, vocab, (rows,), generator=g)
        ids[1], ids[3], ids[rows - 1] = vocab, -1, 1 << 40
        got = _check(logits, ids.to(DEV), 5, f"out of range {rows}x{vocab}")
        nan = torch.isnan(got.chosen[:, 0]).cpu()
        want = torch.zeros(rows, dtype=torch.bool)
        want[[1, 3, rows - 1]] = True
        assert torch.equal(nan, want)


def test_top_k_beyond_vocab_is_rejected():
    logits = torch.zeros(2, 4, device=DEV, dtype=torch.float16)
    with pytest.raises(ValueError, match="exceeds the vocabulary"):
        token_logprobs(logits, None, 5)
    got = token_logprobs(logits, None, 4)
    assert got.top_ids[:, 0].tolist() == [[0, 1, 2, 3]] * 2
