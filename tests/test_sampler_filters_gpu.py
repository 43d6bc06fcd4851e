"""``ll_sample_filtered`` (top-k and min-p on the nucleus sampler) against tests/_sampler_filters_ref.py.

Filters off: the tokens EQUAL ``sample_top_p``'s, on every exact case and every windowed row of tests/_sampler_ref.py, for
every spelling of "off".  Exact cases: every draw EQUALS the integer reference (tests/test_sampler_filters_cpu.py proves the
cases exact in fp32 and that the listed defects fail them).  Windowed cases: seeded rows against the fp64 reference under
``accept_filtered`` at DELTA = 1e-5, no draw exempt.  NaN logits are out of scope."""

import pytest
import torch

from lite_llama_amd import _lib as L
from lite_llama_amd.sampling import Sampler, sample_filtered, sample_top_p
from tests import _sampler_filters_ref as F
from tests import _sampler_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16, torch.float32]


def _name(dtype):
    return str(dtype)[6:]


def _grid(fn, u, rows):
    """``[len(u), rows]`` tokens: one launch per u with every row in it."""
    ug = u.to(DEV)
    return torch.stack([fn(ug[j].expand(rows)).view(-1) for j in range(len(u))]).cpu()


def _off_spellings(vocab, rows):
    """(top_k, min_p) pairs that all mean "both filters off": NULL, 0 or vocab; NULL or 0 -- scalars and per-row tensors."""
    k_rows = torch.tensor([0, vocab, -1, vocab + 7] * rows, dtype=torch.int32, device=DEV)[:rows]
    return [(None, None), (0, 0.0), (vocab, None), (None, 0.0), (vocab, 0.0), (k_rows, torch.zeros(rows, device=DEV))]


# ----------------------------------------------------------------------------------------------------------------- #
# filters off: the old kernel's tokens
# ----------------------------------------------------------------------------------------------------------------- #
OFF_EXACT = [(name, dt) for name in R.exact_cases() for dt in DTYPES]


@pytest.mark.parametrize("name,dtype", OFF_EXACT, ids=[f"{n}-{_name(d)}" for n, d in OFF_EXACT])
def test_filters_off_equal_sample_top_p_on_the_exact_cases(name, dtype):
    case = R.exact_cases()[name]
    logits = case.logits(dtype).to(DEV)[:, -1, :]
    rows = logits.shape[0]
    t, p, u = case.temperature().to(DEV), case.top_p_f32().to(DEV), case.u_grid()
    want = _grid(lambda uu: sample_top_p(logits, t, p, uniform=uu), u, rows)
    assert torch.equal(want, case.expected()[0])
    for k, mp in _off_spellings(case.vocab, rows):
        got = _grid(lambda uu: sample_filtered(logits, t, p, k, mp, uniform=uu), u, rows)
        assert torch.equal(got, want), (name, k, mp)


@pytest.mark.parametrize("key", R.WINDOWED, ids=[R.windowed_name(*k) for k in R.WINDOWED])
def test_filters_off_equal_sample_top_p_on_the_windowed_rows(key):
    case = R.windowed_case(*key)
    u = case.u_grid()
    store = case.store.to(DEV)
    logits = store[:, -1, :]
    rows = logits.shape[0]
    t, p = case.temperature.to(DEV), case.top_p.to(DEV)
    want = _grid(lambda uu: sample_top_p(logits, t, p, uniform=uu), u, rows)
    for k, mp in _off_spellings(key[0], rows):
        got = _grid(lambda uu: sample_filtered(logits, t, p, k, mp, uniform=uu), u, rows)
        assert torch.equal(got, want), (case.name, k, mp)


# ----------------------------------------------------------------------------------------------------------------- #
# exact cases
# ----------------------------------------------------------------------------------------------------------------- #
EXACT = [(name, dt) for name in F.filter_cases() for dt in DTYPES]


@pytest.mark.parametrize("name,dtype", EXACT, ids=[f"{n}-{_name(d)}" for n, d in EXACT])
def test_exact_rows_equal_the_integer_reference(name, dtype):
    """Every draw of every row equals ``filtered_exact``: no tolerance, no exemption.  The rows are the ``[:, -1, :]`` view
    of a ``[B, 2, V]`` tensor (the other half is filler) and then a packed copy; per-row ``top_k`` / ``min_p`` tensors whose
    rows differ, so every launch mixes filtered rows with rows that have a filter off."""
    case = F.filter_cases()[name]
    want, _ = case.expected()
    store = case.logits(dtype).to(DEV)
    t, p, u = case.temperature().to(DEV), case.top_p_f32().to(DEV), case.u_grid()
    k = torch.tensor(case.top_k, dtype=torch.int32, device=DEV)
    mp = torch.tensor(case.min_p, dtype=torch.float32, device=DEV)
    assert mp.cpu().tolist() == case.min_p
    rows = len(case.top_k)
    for logits in (store[:, -1, :], store[:, -1, :].contiguous()):
        got = _grid(lambda uu: sample_filtered(logits, t, p, k, mp, uniform=uu), u, rows)
        wrong = (got != want).nonzero()
        assert wrong.numel() == 0, (name, [(f"u={float(u[j])}", f"row {r}", int(got[j, r]), int(want[j, r])) for j, r in wrong[:8].tolist()])
    # one row, every u in one launch, through a stride-0 view and scalar knobs: the same tokens
    for r in (0, rows - 1):
        view = store[r, -1].view(1, -1).expand(len(u), -1)
        got = sample_filtered(view, float(t[r]), float(p[r]), case.top_k[r], case.min_p[r], uniform=u.to(DEV)).view(-1).cpu()
        assert torch.equal(got, want[:, r]), (name, r)
    # greedy rows mixed into the launch return the first maximum; the others are untouched by their neighbours
    greedy = torch.arange(rows) % 2 == 0
    mid = len(u) // 2
    got = sample_filtered(store[:, -1, :], t, p, k, mp, uniform=u[mid].to(DEV).expand(rows), greedy=greedy.to(DEV)).view(-1).cpu()
    first = R.first_argmax(store[:, -1, :])
    assert torch.equal(got[greedy], first[greedy]) and torch.equal(got[~greedy], want[mid][~greedy]), name


# ----------------------------------------------------------------------------------------------------------------- #
# windowed cases
# ----------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("key", F.W_SHAPES, ids=[f"{v}-{_name(d)}" for v, d in F.W_SHAPES])
def test_seeded_rows_stay_inside_their_window(key):
    """``accept_filtered`` at DELTA on every draw of the grid ``(j + 0.37) / 257`` plus u = 0 and u = 1 - 2^-24, for
    k in {1, 50, 1000} x min_p in {0, 0.01, 0.1} x top_p in {0.9, 1} x T in {0.3, 1}, all 36 rows in one launch per u.  Prints
    the smallest delta at which the case would still pass."""
    case, ref = F.windowed_filter_case(*key), F.windowed_filter_reference(*key)
    u = F.u_grid()
    logits = case.store.to(DEV)[:, -1, :]
    rows = logits.shape[0]
    assert rows == 36 and logits.stride(0) == 2 * key[0]
    if key[1] != torch.float32:  # equal stored logits: ties at the k-th value, all of them survivors
        assert sum(int((ref[0][r] > 0).sum()) > int(case.top_k[r]) for r in range(rows)) >= 6
    t, p, k, mp = case.temperature.to(DEV), case.top_p.to(DEV), case.top_k.to(DEV), case.min_p.to(DEV)
    got = _grid(lambda uu: sample_filtered(logits, t, p, k, mp, uniform=uu), u, rows)
    bad, deltas = [], []
    for r in range(rows):
        row = F.windowed_row(case, ref, r)
        bad += F.check_windowed_filtered(got[:, r], u, row, f"{case.name} row {r} {case.what[r]}")
        deltas.append((F.smallest_delta_filtered(got[:, r], u, row) or 1.0, case.what[r]))
    print(f"{case.name}: smallest passing delta {max(deltas)[0]:.0e} (worst row {max(deltas)[1]})")
    assert not bad, bad


# ----------------------------------------------------------------------------------------------------------------- #
# the other kernel cases
# ----------------------------------------------------------------------------------------------------------------- #
def test_rows_of_one_launch_have_their_own_parameters():
    """A row with both filters off next to a k = 1 row next to a min_p row next to a greedy row, from a strided view: each
    equals the launch that holds it alone with scalar knobs, the off row equals ``sample_top_p``, k = 1 the argmax."""
    vocab = 4097
    g = torch.Generator().manual_seed(21)
    store = (torch.randn(4, 3, vocab, generator=g) * 2).to(torch.float16).to(DEV)
    logits = store[:, 1, :]
    assert logits.stride(0) == 3 * vocab
    k = torch.tensor([0, 1, 0, 7], dtype=torch.int32, device=DEV)
    mp = torch.tensor([0.0, 0.0, 0.3, 0.0], device=DEV)
    greedy = torch.tensor([False, False, False, True], device=DEV)
    for uu in (0.0, 0.21, 0.5, 0.83, R.U_LAST):
        u = torch.full((4,), uu, device=DEV)
        got = sample_filtered(logits, 1.3, 0.9, k, mp, uniform=u, greedy=greedy).view(-1).cpu()
        assert got[0] == sample_top_p(logits[:1], 1.3, 0.9, uniform=u[:1]).item()
        assert logits[1, got[1]] == logits[1].max()                     # k = 1: a maximum (all of them survive)
        assert got[2] == sample_filtered(logits[2:3].contiguous(), 1.3, 0.9, 0, 0.3, uniform=u[:1]).item()
        assert got[3] == R.first_argmax(logits[3:4]).item()
    p, before, ratio = F.filtered64(logits[2:3], 1.3, 0)
    u = F.u_grid()
    view = logits[2].view(1, -1).expand(len(u), -1)
    got = sample_filtered(view, 1.3, 0.9, None, 0.3, uniform=u.to(DEV)).view(-1).cpu()
    assert not F.check_windowed_filtered(got, u, (p[0], before[0], ratio[0], 0.9, 0.3), "min_p row")


def test_sampler_facade_reads_top_k_and_min_p():
    """``Sampler.sample`` / ``sample_batched``: a parameter object without the attributes, or with both off, draws what it
    always drew; with them it draws what ``sample_filtered`` draws."""
    import types
    vocab = 4097
    g = torch.Generator().manual_seed(8)
    cube = (torch.randn(4, 3, vocab, generator=g) * 2).to(torch.bfloat16).to(DEV)
    u = torch.tensor([0.1, 0.4, 0.6, 0.95], device=DEV)
    plain = types.SimpleNamespace(temperature=0.7, top_p=0.9, repetition_penalty=1.0)
    off = types.SimpleNamespace(temperature=0.7, top_p=0.9, repetition_penalty=1.0, top_k=0, min_p=0.0)
    on = types.SimpleNamespace(temperature=0.7, top_p=0.9, repetition_penalty=1.0, top_k=3, min_p=0.05)
    base = sample_top_p(cube[:, -1, :], 0.7, 0.9, uniform=u)
    assert torch.equal(Sampler().sample(cube, plain, None, uniform=u), base)
    assert torch.equal(Sampler().sample(cube, off, None, uniform=u), base)
    none = types.SimpleNamespace(temperature=0.7, top_p=0.9, repetition_penalty=1.0, top_k=None, min_p=None)
    assert torch.equal(Sampler().sample(cube, none, None, uniform=u), base)      # None spells "off" as well
    want = sample_filtered(cube[:, -1, :], 0.7, 0.9, 3, 0.05, uniform=u)
    assert torch.equal(Sampler().sample(cube, on, None, uniform=u), want)
    half = types.SimpleNamespace(temperature=0.7, top_p=0.9, repetition_penalty=1.0, top_k=3, min_p=None)
    assert torch.equal(Sampler().sample(cube, half, None, uniform=u), sample_filtered(cube[:, -1, :], 0.7, 0.9, 3, 0.0, uniform=u))
    top3 = torch.topk(cube[:, -1, :].float(), 3, dim=-1).values[:, -1:]
    assert bool((cube[:, -1, :].float().gather(1, want) >= top3).all())
    col = lambda v: torch.full((4, 1), v, device=DEV)
    batched = types.SimpleNamespace(temperature=col(0.7), top_p=col(0.9), repetition_penalty=col(1.0), any_penalty=False,
                                    all_greedy=False, greedy=torch.tensor([False, True, False, False], device=DEV).view(4, 1))
    b0 = Sampler().sample_batched(cube, batched, None, uniform=u)
    batched.top_k = torch.tensor([3, 3, 0, 3], dtype=torch.int32, device=DEV)
    batched.min_p = torch.tensor([0.05, 0.05, 0.0, 0.05], device=DEV)
    b1 = Sampler().sample_batched(cube, batched, None, uniform=u).view(-1)
    assert b1[1] == b0[1, 0] == R.first_argmax(cube[1:2, -1, :]).item() and b1[2] == b0[2, 0]
    assert b1[0] == want[0, 0] and b1[3] == want[3, 0]


def test_unvalidated_min_p_entries_of_a_tensor():
    """A per-row ``min_p`` that is NaN or negative is off and one above 1 counts as 1, with top-k on and with it off: the
    tokens of the launch that says 0 (or 1) outright."""
    vocab = 4097
    g = torch.Generator().manual_seed(33)
    logits = (torch.randn(6, vocab, generator=g) * 2).to(torch.float16).to(DEV)
    k = torch.tensor([0, 5, 0, 5, 0, 5], dtype=torch.int32, device=DEV)
    odd = torch.tensor([float("nan"), float("nan"), -0.5, -0.5, 1.5, 1.5], device=DEV)
    plain = torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0, 1.0], device=DEV)
    for uu in (0.0, 0.3, 0.6, 0.9, R.U_LAST):
        u = torch.full((6,), uu, device=DEV)
        got = sample_filtered(logits, 1.5, 0.95, k, odd, uniform=u)
        assert torch.equal(got, sample_filtered(logits, 1.5, 0.95, k, plain, uniform=u)), uu
        assert torch.equal(got[:1], sample_top_p(logits[:1], 1.5, 0.95, uniform=u[:1]))
        assert bool((logits.gather(1, got)[4:] == logits[4:].max(dim=-1, keepdim=True).values).all())  # min_p = 1: a maximum


def test_bad_arguments():
    lib = L.lib()
    x = torch.zeros(2, 8, dtype=torch.float16, device=DEV)
    f = torch.ones(2, device=DEV)
    out = torch.empty(2, dtype=torch.int64, device=DEV)
    call = lambda out_p, lg, t, batch, vocab, dtype: lib.ll_sample_filtered(out_p, lg, t, f.data_ptr(), 0, 0, f.data_ptr(), 0, batch,
                                                                            vocab, 8, dtype, L.stream_ptr())
    code = L.dtype_code(torch.float16)
    assert call(out.data_ptr(), x.data_ptr(), f.data_ptr(), 2, 8, code) == 0
    assert call(out.data_ptr(), x.data_ptr(), f.data_ptr(), 0, 8, code) == 0          # an empty batch is fine
    bad_shape = call(out.data_ptr(), x.data_ptr(), f.data_ptr(), 2, 0, code)
    bad_arg = call(0, x.data_ptr(), f.data_ptr(), 2, 8, code)
    bad_dtype = call(out.data_ptr(), x.data_ptr(), f.data_ptr(), 2, 8, 99)
    top_p = lambda *a: lib.ll_sample_top_p(*a)
    assert bad_shape == top_p(out.data_ptr(), x.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), 0, 2, 0, 8, code, L.stream_ptr()) < 0
    assert bad_arg == top_p(0, x.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), 0, 2, 8, 8, code, L.stream_ptr()) < 0
    assert bad_dtype == top_p(out.data_ptr(), x.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), 0, 2, 8, 8, 99, L.stream_ptr()) < 0
    assert call(out.data_ptr(), x.data_ptr(), f.data_ptr(), -1, 8, code) == bad_shape
    assert call(out.data_ptr(), x.data_ptr(), 0, 2, 8, code) == bad_arg
    assert len({bad_shape, bad_arg, bad_dtype}) == 3
    for mp in (-0.1, 1.5):
        with pytest.raises(ValueError, match="min_p"):
            sample_filtered(x, 1.0, 1.0, 0, mp)
    with pytest.raises(ValueError, match="one entry per row"):
        sample_filtered(x, 1.0, 1.0, torch.zeros(3, dtype=torch.int32, device=DEV), 0.0)
    with pytest.raises(ValueError, match="batch, vocab"):
        sample_filtered(x[0], 1.0, 1.0)
