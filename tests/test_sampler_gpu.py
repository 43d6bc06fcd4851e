"""The nucleus sampler, the argmax kernels and the repetition penalty at their edges, against tests/_sampler_ref.py.

Nucleus draws are held in two ways.  Exact cases: rows of power-of-two masses with small integer sums, where every fp32
quantity of the kernel is exact in any summation order (tests/test_sampler_cpu.py proves that of the cases, and the
premise that the hardware ``exp2`` returns exact powers of two for integral arguments is what these tests would refute):
every draw EQUALS the integer reference -- the edge rule (a ``u`` on an edge belongs to the next token), the tie order
(lowest index first), ``top_p = 0`` and zero-mass tokens are pinned with no tolerance.  Windowed cases: seeded rows against
the fp64 reference under ``accept`` at ``DELTA`` = 1e-5; no draw is exempt, and tests/test_sampler_cpu.py proves the rule
rejects a list of wrong samplers.  Argmax and the penalty are exact.  NaN logits are out of scope everywhere."""

import pytest
import torch

from lite_llama_amd.sampling import Sampler, apply_repetition_penalty, greedy_argmax, sample_top_p
from tests import _sampler_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16, torch.float32]


def _name(dtype):
    return str(dtype)[6:]


def _draw_grid(logits, temperature, top_p, u, greedy=None):
    """``[len(u), rows]`` tokens: one launch per u with every row in it (per-row temperature and top_p tensors)."""
    rows = logits.shape[0]
    ug = u.to(DEV)
    out = [sample_top_p(logits, temperature, top_p, uniform=ug[j].expand(rows), greedy=greedy).view(-1) for j in range(len(u))]
    return torch.stack(out).cpu()


def _draw_row(row, temperature, top_p, u):
    """``[len(u)]`` tokens of ONE row in one launch: an expanded view (``stride(0) == 0``), one u per repeat."""
    n = len(u)
    t = torch.full((n,), float(temperature), dtype=torch.float32, device=DEV)
    p = torch.full((n,), float(top_p), dtype=torch.float32, device=DEV)
    view = row.view(1, -1).expand(n, -1)
    assert view.stride(0) == 0
    return sample_top_p(view, t, p, uniform=u.to(DEV)).view(-1).cpu()


# ----------------------------------------------------------------------------------------------------------------- #
# nucleus sampling: exact cases
# ----------------------------------------------------------------------------------------------------------------- #
EXACT = [(name, dt, strided) for name in R.exact_cases() for dt in DTYPES for strided in (False, True)]


@pytest.mark.parametrize("name,dtype,strided", EXACT, ids=[f"{n}-{_name(d)}-{'strided' if s else 'packed'}" for n, d, s in EXACT])
def test_exact_rows_equal_the_integer_reference(name, dtype, strided):
    """Every draw of every row equals ``nucleus_exact``: no tolerance, no exemption.  ``strided``: the rows are the
    ``[:, -1, :]`` view of a ``[B, 2, V]`` tensor, as ``Sampler.sample`` passes them; the other half is filler."""
    case = R.exact_cases()[name]
    want, _ = case.expected()
    store = case.logits(dtype).to(DEV)
    logits = store[:, -1, :] if strided else store[:, -1, :].contiguous()
    assert (logits.stride(0) == 2 * case.vocab) == strided or case.vocab == 1
    t, p, u = case.temperature().to(DEV), case.top_p_f32().to(DEV), case.u_grid()
    got = _draw_grid(logits, t, p, u)
    wrong = (got != want).nonzero()
    assert wrong.numel() == 0, (name, [(f"u={float(u[j])}", f"row {r}", int(got[j, r]), int(want[j, r])) for j, r in wrong[:8].tolist()])
    # one row, every u in one launch, through a stride-0 view: the same tokens
    for r in (0, case.exps.shape[0] - 1):
        assert torch.equal(_draw_row(logits[r], t[r], p[r], u), want[:, r]), (name, r)
    # greedy rows mixed into the launch return the first maximum; the others are untouched by their neighbours
    rows = case.exps.shape[0]
    greedy = torch.arange(rows) % 2 == 0
    got = _draw_grid(logits, t, p, u[len(u) // 2:len(u) // 2 + 1], greedy=greedy.to(DEV))[0]
    first = R.first_argmax(logits)
    assert torch.equal(first, torch.argmax(logits.float().cpu(), dim=-1)) and torch.equal(greedy_argmax(logits).cpu(), first)
    assert torch.equal(got[greedy], first[greedy]) and torch.equal(got[~greedy], want[len(u) // 2][~greedy]), name


# ----------------------------------------------------------------------------------------------------------------- #
# nucleus sampling: windowed cases
# ----------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("key", R.WINDOWED, ids=[R.windowed_name(*k) for k in R.WINDOWED])
def test_seeded_rows_stay_inside_their_window(key):
    """``accept`` at DELTA on every draw of the grid ``(j + 0.37) / 257`` plus u = 0 and u = 1 - 2^-24; drawn tokens do not
    decrease as u grows; every inner token heavier than two grid steps is drawn.  Rows go eight to a launch, as the
    ``[:, -1, :]`` view of their storage, with per-row temperature and top_p tensors whose rows differ.  Prints the
    smallest delta at which the case would still pass."""
    case, (p, before) = R.windowed_case(*key), R.windowed_reference(*key)
    u = case.u_grid()
    store = case.store.to(DEV)
    bad, deltas = [], []
    for r0 in range(0, len(case.what), R.GROUP):
        sl = slice(r0, r0 + R.GROUP)
        logits = store[sl, -1, :]
        assert logits.stride(0) == 2 * key[0]
        got = _draw_grid(logits, case.temperature[sl].to(DEV), case.top_p[sl].to(DEV), u)
        for i, r in enumerate(range(r0, min(r0 + R.GROUP, len(case.what)))):
            row = (p[r], before[r], float(case.top_p[r]))
            bad += R.check_windowed(got[:, i], u, row, f"{case.name} row {r} {case.what[r]}")
            deltas.append((R.smallest_delta(got[:, i], u, row) or 1.0, case.what[r]))
            if r == r0:  # the group's first row again through a stride-0 view: the same tokens
                assert torch.equal(_draw_row(logits[0], case.temperature[r], case.top_p[r], u), got[:, 0]), (case.name, r)
    print(f"{case.name}: smallest passing delta {max(deltas)[0]:.0e} (worst row {max(deltas)[1]})")
    assert not bad, bad


@pytest.mark.parametrize("vocab,dtype", [(152064, torch.float16), (152064, torch.bfloat16), (128256, torch.float16),
                                         (128256, torch.bfloat16), (4097, torch.float32)],
                         ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_a_zero_mass_tail_is_never_drawn(vocab, dtype):
    """top_p = 1 keeps everything, so a -inf tail after the last positive token counts as kept; at u just below 1 the walk
    can run past the last positive token on rounding alone, and what it then names must still carry mass."""
    g = torch.Generator().manual_seed(vocab + 17)
    logits = torch.randn(8, vocab, generator=g) * torch.tensor([0.5, 1.0, 1.0, 1.5, 1.5, 2.0, 3.0, 3.0]).view(-1, 1)
    for r, tail in enumerate([1, 5, 63, 64, 200, 1000, 3000, 777]):
        logits[r, vocab - tail:] = float("-inf")
    logits = logits.to(dtype)
    t = torch.tensor([5.0, 1.3, 1.0, 1.3, 1.0, 1.0, 1.3, 5.0])
    tp = torch.ones(8)
    p, before = R.nucleus64(logits, t, tp)
    u = torch.tensor([1 - 2.0 ** -k for k in (24, 23, 22, 21, 20, 18, 16, 12)], dtype=torch.float64).float()
    got = _draw_grid(logits.to(DEV), t.to(DEV), tp.to(DEV), u)
    for r in range(8):
        ok = R.accept(got[:, r], u, (p[r], before[r], 1.0))
        assert bool(ok.all()), (r, got[:, r].tolist(), int((p[r] > 0).nonzero()[-1]))


# ----------------------------------------------------------------------------------------------------------------- #
# argmax
# ----------------------------------------------------------------------------------------------------------------- #
ARGMAX_LENGTHS = [1, 63, 64, 65, 1023, 1025, 16383, 16384, 16385, 152064]


def _argmax_rows(n, dtype, g):
    """The case table of one row length: seeded rows with many exact ties, then the edges."""
    x = torch.randint(-3, 4, (12, n), generator=g).to(torch.float32)
    x[1] = 1.5                                   # all equal -> 0
    x[2] = float("-inf")                         # all -inf -> 0
    x[3, -1] = 9.0                               # the maximum at the last index only
    x[4, 0] = x[4, -1] = 9.0                     # at index 0 and at the last index -> 0
    x[5] = -1.0
    x[5, 0], x[5, -1] = -0.0, 0.0                # -0 then +0: equal, the first wins
    x[6] = -1.0
    x[6, 0], x[6, -1] = 0.0, -0.0
    x[7] = float("-inf")
    x[7, -1] = -30000.0                          # one finite value among -inf
    x[8] = torch.randn(n, generator=g) * 3       # distinct values
    return x.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", ARGMAX_LENGTHS)
def test_argmax_edges(n, dtype):
    g = torch.Generator().manual_seed(n)
    x = _argmax_rows(n, dtype, g)
    want = torch.argmax(x.float(), dim=-1)
    assert torch.equal(R.first_argmax(x), want)
    assert want[1] == 0 and want[2] == 0 and want[3] == n - 1 and want[4] == 0 and want[5] == 0 and want[6] == 0
    assert torch.equal(greedy_argmax(x.to(DEV)).cpu(), want), (n, dtype)
    # [B, L, V] and its [:, -1, :] view (non-contiguous rows)
    cube = torch.stack([x.flip(0), x, x], dim=1).to(DEV)
    assert torch.equal(greedy_argmax(cube).cpu(), torch.argmax(cube.cpu().float(), dim=-1))
    view = cube[:, -1, :]
    assert not view.is_contiguous() or n == 1
    assert torch.equal(greedy_argmax(view).cpu(), want)
    assert torch.equal(greedy_argmax(cube[:, :, ::2]).cpu(), torch.argmax(cube.cpu()[:, :, ::2].float(), dim=-1))  # strided elements


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("rows", [1, 64, 600])
def test_argmax_ties_across_the_split_boundaries(rows, dtype):
    """Tied maxima at ``per - 1`` and ``per`` of the split path's chunking -- the last token of one workgroup's chunk and the
    first of the next -- for the ``chunks`` the wrapper picks at this row count; also tied across distant chunks, and with
    the later chunk holding the tie's first element at its last position."""
    vocab = 152064
    chunks, per = R.argmax_chunks(rows, vocab)
    x = torch.zeros(rows, vocab, dtype=dtype)
    picks = {}
    for r in range(rows):
        c = 1 + r % (chunks - 1)                 # the boundary between chunk c - 1 and chunk c
        kind = r % 4
        idx = [[c * per - 1, c * per], [c * per], [c * per - 1, (chunks - 1) * per, vocab - 1], [c * per, c * per + 1]][kind]
        idx = [i for i in idx if i < vocab]
        x[r, idx] = 7.0
        picks[r] = min(idx)
    want = torch.argmax(x.float(), dim=-1)
    assert want.tolist() == [picks[r] for r in range(rows)]
    assert torch.equal(greedy_argmax(x.to(DEV)).cpu(), want), (rows, chunks, per)


def test_argmax_many_vocabulary_rows_take_the_single_kernel():
    rows, vocab = 1024, 128256
    assert R.argmax_chunks(rows, vocab) is None and R.argmax_chunks(rows - 1, vocab) is not None
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randint(-3, 4, (rows, vocab), generator=g, device=DEV, dtype=torch.int8).to(torch.float16)  # many exact ties
    x[5, vocab - 1] = 9.0
    x[6, 1023], x[6, 1024] = 9.0, 9.0            # neighbouring threads of the 1024-wide walk
    x[7, 70000], x[7, 100] = 9.0, 9.0
    want = torch.argmax(x.cpu(), dim=-1)
    assert want[5] == vocab - 1 and want[6] == 1023 and want[7] == 100
    assert torch.equal(greedy_argmax(x).cpu(), want)


# ----------------------------------------------------------------------------------------------------------------- #
# repetition penalty
# ----------------------------------------------------------------------------------------------------------------- #
PENALTY_VOCABS = [1, 300, 8191, 8192, 8193, 152064, 600000]


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _penalty_case(vocab, dtype, g):
    """Six rows.  Token ids exactly at ``c_lo`` and ``c_hi - 1`` of the first, a middle and the last chunk and at
    ``vocab - 1``; one id repeated 50 times; one id masked out in one slot and live in another (and one only masked out);
    logits of +0, -0, a large negative value and -inf among the penalised tokens."""
    chunks, per = R.penalty_chunks(vocab)
    edges = set()
    for c in {0, chunks // 2, chunks - 1}:
        lo, hi = c * per, min((c + 1) * per, vocab)
        edges |= {lo, hi - 1}
    edges = sorted(edges | {vocab - 1})
    span = 96
    logits = (torch.randn(6, vocab, generator=g) * 4).to(dtype)
    special = torch.tensor([0.0, -0.0, -60000.0, float("-inf")]).to(dtype)
    ids = torch.randint(0, vocab, (6, span), generator=g)
    mask = torch.rand(6, span, generator=g) > 0.25
    ids[:, :len(edges)] = torch.tensor(edges)
    mask[:, :len(edges)] = True
    ids[1, 20:70] = ids[1, 19]                   # one id 50 times
    mask[1, 19:70] = True
    ids[2, 30] = ids[2, 31] = ids[2, 40]         # masked out in one slot, live in another
    mask[2, 30], mask[2, 31], mask[2, 40] = False, True, False
    lonely = (int(ids[2, 0]) + 1) % vocab        # only ever masked out: stays as it is
    if lonely not in ids[2, mask[2]].tolist():
        ids[2, 50], mask[2, 50] = lonely, False
    for r in (3, 4):                             # the special values sit on penalised tokens (the edge ids are live in every row)
        where = torch.tensor(edges[:4]) if len(edges) >= 4 else torch.arange(min(4, vocab))
        logits[r, where] = special[:len(where)]
    mask[5] = False                              # a span that is entirely masked
    return logits, ids, mask


@pytest.mark.parametrize("tensor_penalty", [False, True], ids=["scalar", "per-row"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("vocab", PENALTY_VOCABS)
def test_repetition_penalty_bit_for_bit(vocab, dtype, tensor_penalty):
    """The five dtype pairs the kernel dispatches (a scalar keeps the dtype, a float32 tensor promotes to float32), bit for
    bit against ``penalty_ref``, the input untouched, from a packed tensor and from a strided view."""
    g = torch.Generator().manual_seed(vocab + 3)
    logits, ids, mask = _penalty_case(vocab, dtype, g)
    store = torch.zeros(6, 2, vocab, dtype=dtype)
    store[:, 1, :] = logits
    store = store.to(DEV)
    keep = store.clone()
    pens = [torch.tensor([1.0, 1.3, 0.8, 2.0, 1.1, 1.7])] if tensor_penalty else [1.3, 0.8, 1.0]
    for pen in pens:
        want = R.penalty_ref(logits, ids, mask, pen)
        dpen = pen.to(DEV) if tensor_penalty else pen
        for lg in (store[:, 1, :], store[:, 1, :].contiguous()):
            got = apply_repetition_penalty(lg, ids.to(DEV), mask.to(DEV), dpen)
            assert got.dtype == (torch.float32 if tensor_penalty else dtype)
            assert _bits_equal(got.cpu(), want), (vocab, dtype, pen)
        if not tensor_penalty and pen == 1.0:
            assert _bits_equal(got.cpu(), logits)                       # penalty 1.0 is the identity
        assert _bits_equal(got[5].cpu(), logits[5].to(got.dtype))       # an entirely masked span: a copy
    # span = 0: a bit-identical copy
    got = apply_repetition_penalty(store[:, 1, :], ids[:, :0].to(DEV), mask[:, :0].to(DEV), pens[0].to(DEV) if tensor_penalty else 1.3)
    assert _bits_equal(got.cpu(), logits.to(got.dtype))
    assert _bits_equal(store, keep)                                     # the input is never written


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_repetition_penalty_branch_at_zero(dtype):
    """``x < 0 ? x * pen : x / pen``: +0 and -0 take the division.  For every finite positive penalty both branches give the
    same zero, so the one input that tells them apart is an infinite penalty (0 / inf = 0, 0 * inf = NaN): zeros stay zeros,
    positive logits go to +0, negative ones to -inf."""
    logits = torch.tensor([[0.0, -0.0, 2.0, -2.0, float("-inf"), 1.0]]).to(dtype)
    ids = torch.tensor([[0, 1, 2, 3, 4]])
    mask = torch.ones(1, 5, dtype=torch.bool)
    want = torch.tensor([[0.0, -0.0, 0.0, float("-inf"), float("-inf"), 1.0]]).to(dtype)
    assert _bits_equal(R.penalty_ref(logits, ids, mask, float("inf")), want)
    got = apply_repetition_penalty(logits.to(DEV), ids.to(DEV), mask.to(DEV), float("inf"))
    assert _bits_equal(got.cpu(), want), got


def test_sampler_facade_slices_penalises_and_draws():
    """``Sampler.sample`` on ``[B, L, V]`` bf16 logits: the last position, the penalty first, then the draw -- equal to the
    three steps taken by hand, and inside the window of the fp64 reference of the penalised row."""
    import types
    vocab = 4097
    g = torch.Generator().manual_seed(8)
    cube = (torch.randn(4, 3, vocab, generator=g) * 2).to(torch.bfloat16)
    ids = torch.argmax(cube[:, -1, :].float(), dim=-1).view(-1, 1)
    mask = torch.ones(4, 1, dtype=torch.bool)
    gen = types.SimpleNamespace(token_ids=ids.to(DEV), mask=mask.to(DEV))
    params = types.SimpleNamespace(temperature=0.7, top_p=0.9, repetition_penalty=1.5)
    pen = R.penalty_ref(cube[:, -1, :], ids, mask, 1.5)
    p, before = R.nucleus64(pen, torch.full((4,), 0.7), torch.full((4,), 0.9))
    for uu in (0.0, 0.31, 0.77, R.U_LAST):
        u = torch.full((4,), uu)
        got = Sampler().sample(cube.to(DEV), params, gen, uniform=u.to(DEV)).view(-1).cpu()
        for r in range(4):
            assert bool(R.accept(got[r:r + 1], u[r:r + 1], (p[r], before[r], 0.9)).all()), (uu, r, int(got[r]))
    params.temperature = 0.0
    assert torch.equal(Sampler().sample(cube.to(DEV), params, gen).view(-1).cpu(), R.first_argmax(pen))
