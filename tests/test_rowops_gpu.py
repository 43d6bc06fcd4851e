"""GPU tests of the row kernels of csrc/norm_act.hip -- ``skip_rmsnorm`` (cached, two-pass, partials and slots forms), ``moe_sum``,
``swiglu_forward`` (two tensors, column halves, interleaved pairs), relu / leaky_relu / tanh / gelu, ``rope_emb_forward`` and
``rope_and_cache`` -- held to the rounding brackets of ``tests/_rowops_ref.py`` (float64 reference, slack derived from each kernel's
own fp32 arithmetic, rounded once to the storage type; most elements are pinned to one value) at every instance of the dispatch,
on both sides of every switch, in the second trip of every grid-stride loop, in both 16-bit types.  ``tests/test_rowops_ref_cpu.py``
checks the checker: the oracle passes it, the smallest realistic faults do not.  The references run on the device in float64.

Instances reached (dispatch lines of csrc/norm_act.hip, restated in ``_rowops_ref.norm_instance`` and friends):
  skip_rmsnorm_cached<16,1> n = 8, 128; <32,1> 136, 256; <64,1> 264, 512; <256,1> 520, 2048; <256,2> 2056, 4096; <256,4> 4104, 8192;
  skip_rmsnorm_twopass<8> 8200, 65536 (32 trips); twopass<1> 300, 4103 and any operand off a 16-byte boundary (n = 2048);
  rows 1, RPB - 1, RPB, RPB + 1 of each; partials <1 | 2 | 4 vectors, 4 | 6 | 8 | 12 plane loads>, slots <1 | 2 | 4, 2 | 4 | 8 slot loads>
  with counts at, one below and one above every load count; swiglu / moe_sum / activation vector and scalar kernels past their
  4096 / 4096 / 8192-block caps; rope_kernel vector and scalar with more than 256 work items per token, rope_cache_kernel with and
  without vector table loads and with more than 1024."""

import pytest
import torch

from tests import _rowops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, BF16 = R.F16, R.BF16
IDS = {"ids": R.dname}


def K():
    import lite_llama_amd.kernels as k

    return k


def NA():
    import lite_llama_amd.kernels.norm_act as m

    return m


def _d(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def _guarded(src: torch.Tensor, offset: int = 8):
    """``(view, buffer)``: a copy of ``src`` inside a sentinel-filled buffer, ``offset`` elements in (8 keeps the 16-byte alignment,
    1 breaks it) with at least 8 sentinel elements behind it."""
    buf = R.sentinel((src.numel() + offset + 8,), src.dtype, src.device)
    view = buf[offset:offset + src.numel()].view(src.shape)
    view.copy_(src)
    return view, buf


def _guards_intact(buf: torch.Tensor, numel: int, offset: int = 8) -> bool:
    return bool(R.is_sentinel(buf[:offset]).all()) and bool(R.is_sentinel(buf[offset + numel:]).all())


def _same_bits(a, b) -> bool:
    return torch.equal(R.bits(a), R.bits(b))


# ------------------------------------------------------------------------------------------------------------------------------ #
# skip_rmsnorm
# ------------------------------------------------------------------------------------------------------------------------------ #
def _norm_call(x, r, w, eps, ylo, yhi, rb, what, offsets=(8, 8, 8)):
    """One launch on copies of ``x`` / ``r`` / ``w`` placed between sentinel guards; checks the brackets, the aliasing contract
    (``r`` updated in place and returned, ``X`` echoed when there is no residual), that ``x`` and ``w`` are left alone and that
    nothing outside the tensors is written."""
    xin, xbuf = _guarded(x, offsets[0])
    win, wbuf = _guarded(w, offsets[2])
    rin, rbuf = _guarded(r, offsets[1]) if r is not None else (None, None)
    y, r_out = K().skip_rmsnorm(xin, rin, win, eps)
    assert y.shape == x.shape and y.dtype == x.dtype
    R.assert_in_bracket(y, ylo, yhi, what + " y")
    assert _same_bits(xin, x) and _guards_intact(xbuf, x.numel(), offsets[0]), what
    assert _same_bits(win, w) and _guards_intact(wbuf, w.numel(), offsets[2]), what
    if r is not None:
        assert r_out.data_ptr() == rin.data_ptr() and r_out.shape == x.shape, what
        R.assert_in_bracket(rin, *rb, what + " r")
        assert _guards_intact(rbuf, r.numel(), offsets[1]), what
    else:
        assert r_out.data_ptr() == xin.data_ptr(), what
    return y, r_out


@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
@pytest.mark.parametrize("n", R.NORM_NS)
def test_skip_rmsnorm_rows_fall_in_their_brackets(n, dtype):
    """N(0, 1) rows at rows = 1, RPB - 1, RPB, RPB + 1 of the instance n selects, and rows of magnitude 2**-12 (eps carries the
    variance) and 200 (eps vanishes), with and without a residual, eps = 1e-6 and 1e-5."""
    row_counts = R.norm_rows(n)
    top = row_counts[-1]
    for kind in ("randn", "tiny", "big"):
        for with_res in (True, False):
            x, r, w = _d(*R.norm_inputs(kind, top, n, dtype, with_res=with_res))
            for eps in R.NORM_EPS:
                (ylo, yhi), rb = R.norm_brackets(x, r, w, eps)
                for rows in (row_counts if kind == "randn" else [top]):
                    what = f"{kind} n={n} rows={rows} res={with_res} eps={eps} {R.norm_instance(n)}"
                    _norm_call(x[:rows], None if r is None else r[:rows], w, eps, ylo[:rows], yhi[:rows],
                               None if rb is None else (rb[0][:rows], rb[1][:rows]), what)


@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
@pytest.mark.parametrize("n", R.NORM_NS)
def test_skip_rmsnorm_one_hot_rows_count_every_column(n, dtype):
    """All of a row's energy in one column -- the first, the last, the ends of every vector index, both sides of every wave and
    trip boundary: ``y`` there is ``sqrt(n) w`` when the column is counted and about ``w / sqrt(eps)`` when it is not."""
    for with_res in (True, False):
        x, r, w = _d(*R.onehot_inputs(n, dtype, with_res))
        for eps in R.NORM_EPS:
            (ylo, yhi), rb = R.norm_brackets(x, r, w, eps)
            _norm_call(x, r, w, eps, ylo, yhi, rb, f"one-hot n={n} res={with_res} eps={eps}")


@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
def test_skip_rmsnorm_off_a_16_byte_boundary_takes_the_scalar_kernel_with_the_same_values(dtype):
    """n = 2048 with x, then r, then w one element off a 16-byte boundary: the scalar two-pass kernel; ``r_out`` bit for bit what the
    aligned call gives, ``y`` in the same bracket."""
    n, rows, eps = 2048, 3, 1e-6
    assert R.norm_instance(n, aligned=False) == ("twopass", 1)
    x, r, w = _d(*R.norm_inputs("randn", rows, n, dtype))
    (ylo, yhi), rb = R.norm_brackets(x, r, w, eps)
    _, r0 = _norm_call(x, r, w, eps, ylo, yhi, rb, "aligned")
    r0 = r0.clone()
    for i, name in enumerate(("x", "r", "w")):
        offsets = tuple(1 if j == i else 8 for j in range(3))
        _, r1 = _norm_call(x, r, w, eps, ylo, yhi, rb, f"{name} off by one element", offsets)
        assert r1.data_ptr() % 16 == (2 if name == "r" else 0)
        assert _same_bits(r1, r0), name
    _norm_call(x, None, w, eps, *R.norm_brackets(x, None, w, eps)[0], None, "x off by one, no residual", (1, 8, 8))
    xo, ro, wo = _d(*R.onehot_inputs(n, dtype, aligned=False))
    (ylo, yhi), rb = R.norm_brackets(xo, ro, wo, eps)
    _norm_call(xo, ro, wo, eps, ylo, yhi, rb, "one-hot, scalar kernel", (1, 8, 8))


def test_skip_rmsnorm_zero_rows_is_a_no_op_and_a_row_past_65536_raises():
    w = torch.ones(2048, dtype=F16, device=DEV)
    r, rbuf = _guarded(torch.zeros(0, 2048, dtype=F16, device=DEV))
    y, r_out = K().skip_rmsnorm(torch.zeros(0, 2048, dtype=F16, device=DEV), r, w, 1e-6)
    torch.cuda.synchronize()
    assert y.shape == (0, 2048) and r_out.shape == (0, 2048) and bool(R.is_sentinel(rbuf).all())
    x = torch.zeros(1, 65537, dtype=F16, device=DEV)
    with pytest.raises(RuntimeError, match="65537"):
        K().skip_rmsnorm(x, None, torch.ones(65537, dtype=F16, device=DEV), 1e-6)
    with pytest.raises(RuntimeError, match="65537"):
        K().skip_rmsnorm(x, x.clone(), torch.ones(65537, dtype=F16, device=DEV), 1e-6)


# ------------------------------------------------------------------------------------------------------------------------------ #
# skip_rmsnorm over split-K planes and over MoE slots; moe_sum
# ------------------------------------------------------------------------------------------------------------------------------ #
def _summed_norm_call(make, parts, r, w, eps, dim, what):
    (ylo, yhi), rb = R.partials_brackets(parts, dim, r, w, eps)
    keep = parts.clone()
    rin, rbuf = _guarded(r)
    y, r_out = NA().skip_rmsnorm_partials(make(parts), rin, w, eps)
    assert y.shape == r.shape and y.dtype == r.dtype and r_out.data_ptr() == rin.data_ptr(), what
    R.assert_in_bracket(rin, *rb, what + " r")  # storage(x + r) with x = storage(sum): a dropped or doubled plane moves it by order 1
    R.assert_in_bracket(y, ylo, yhi, what + " y")
    assert torch.equal(parts, keep) and _guards_intact(rbuf, r.numel()), what


@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
@pytest.mark.parametrize("n", R.PART_NS)
def test_skip_rmsnorm_partials_adds_exactly_the_planes_it_was_given(n, dtype):
    """``PartialSums`` built directly from independent N(0, 1) fp32 planes, s at, below and above every plane-load count."""
    for s in R.PART_S:
        for rows in R.PART_ROWS:
            parts, r, w = _d(*R.plane_inputs(s, rows, n, dtype))
            for eps in (R.NORM_EPS if s == 8 else R.NORM_EPS[:1]):
                _summed_norm_call(lambda p: NA().PartialSums(p, (rows, n), dtype), parts, r, w, eps, 0,
                                  f"planes n={n} s={s} rows={rows} {R.partials_instance(n, s)}")


@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
@pytest.mark.parametrize("n", R.PART_NS)
def test_skip_rmsnorm_slots_and_moe_sum_add_exactly_the_slots_they_were_given(n, dtype):
    """``SlotSums``: the fused norm in its brackets, and ``materialise()`` (``ll_moe_sum``) the sequential fp32 sum rounded once."""
    for k in R.SLOT_K:
        for rows in R.PART_ROWS:
            slots, r, w = _d(*R.slot_inputs(k, rows, n, dtype))
            what = f"slots n={n} k={k} rows={rows} {R.slots_instance(n, k)}"
            for eps in (R.NORM_EPS if k == 4 else R.NORM_EPS[:1]):
                _summed_norm_call(lambda p: NA().SlotSums(p, (rows, n)), slots, r, w, eps, 1, what)
            got = NA().SlotSums(slots, (rows, n)).materialise()
            assert R.assert_in_bracket(got, *R.sum_bracket(slots, 1, dtype), what + " moe_sum") == 1.0


@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
@pytest.mark.parametrize("rows,k,n", [(3, 3, 300), (1, 8, 300), R.MOE_SUM_BIG])
def test_moe_sum_scalar_kernel_and_second_loop_trip(rows, k, n, dtype):
    if (rows, k, n) == R.MOE_SUM_BIG:
        assert R.grid_trips(rows, n, 4096) == (8, 4096, 2)
    slots = (torch.randn(rows, k, n, device=DEV, generator=torch.Generator(DEV).manual_seed(n + k))).to(dtype)
    got = NA().SlotSums(slots, (rows, n)).materialise()
    assert got.shape == (rows, n)
    assert R.assert_in_bracket(got, *R.sum_bracket(slots, 1, dtype), f"moe_sum {rows}x{k}x{n}") == 1.0


# ------------------------------------------------------------------------------------------------------------------------------ #
# swiglu_forward
# ------------------------------------------------------------------------------------------------------------------------------ #
def _swiglu_forms(g, u, forms=("two", "halves", "pairs")):
    """The forms of one ``(g, u)``: two tensors; the column halves of one ``[rows, 2n]`` buffer; its even / odd columns."""
    rows, n = g.shape
    out = {}
    for form in forms:
        if form == "two":
            a, b, buf = g.clone(), u.clone(), None
        else:
            buf = torch.empty(rows, 2 * n, dtype=g.dtype, device=g.device)
            a, b = (buf[:, :n], buf[:, n:]) if form == "halves" else (buf[:, 0::2], buf[:, 1::2])
            a.copy_(g)
            b.copy_(u)
            keep = buf.clone()
        out[form] = K().swiglu_forward(a, b)
        assert out[form].shape == g.shape and out[form].dtype == g.dtype
        if buf is not None:
            assert _same_bits(buf, keep), form
    return out


@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
@pytest.mark.parametrize("n", R.SWIGLU_NS)
def test_swiglu_three_forms_fall_in_the_bracket_and_agree_bit_for_bit(n, dtype):
    """3 N(0, 1) rows and the gate edges (+-0, +-2**-14, +-11, +-30, +-88, +-65504, bf16 +-1e30, against u = +-1, +-65504: results
    that are subnormal in the storage type, that overflow it, and that vanish).  n = 300 and 5 take the scalar kernels, n = 5 in
    the pairs form the scalar pairs load.

    Measured on the MI355X: every result that is subnormal in the storage type is pinned and met.  Where sigmoid(g) itself is an
    fp32 subnormal (g <= -87.5) the hardware reciprocal returns zero, so bf16 gets -0 where the exact value is still a normal bf16
    number (g = -88, u = 1: exact -5.33e-37, kernel -0; u = 65536: exact -3.49e-32, kernel -0; g = -87 is met exactly); fp16
    rounds all of these to -0 anyway.  ``_rowops_ref.swiglu_bracket`` reaches down to zero there and nowhere else."""
    for kind, rows in (("randn", 37), ("edges", R.swiglu_edge_rows(n, dtype))):
        g, u = _d(*R.swiglu_inputs(kind, rows, n, dtype))
        lo, hi = R.swiglu_bracket(g, u)
        out = _swiglu_forms(g, u)
        for form, got in out.items():
            R.assert_in_bracket(got, lo, hi, f"{kind} n={n} {form}")
            assert _same_bits(got, out["two"]), (kind, form)


@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
@pytest.mark.parametrize("shape", [R.SWIGLU_BIG_VEC, R.SWIGLU_BIG_SCALAR])
def test_swiglu_second_trip_of_the_grid_stride_loop(shape, dtype):
    rows, n = shape
    assert R.grid_trips(rows, n, 4096)[1:] == (4096, 2)
    gen = torch.Generator(DEV).manual_seed(n)
    g = (torch.randn(rows, n, device=DEV, generator=gen) * 3).to(dtype)
    u = (torch.randn(rows, n, device=DEV, generator=gen) * 3).to(dtype)
    lo, hi = R.swiglu_bracket(g, u)
    out = _swiglu_forms(g, u, ("two", "halves", "pairs") if n % 8 == 0 else ("two", "pairs"))
    for form, got in out.items():
        R.assert_in_bracket(got, lo, hi, f"{shape} {form}")
        assert _same_bits(got, out["two"]), form


# ------------------------------------------------------------------------------------------------------------------------------ #
# activations
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
@pytest.mark.parametrize("kind", R.ACT_KINDS)
def test_activations_fall_in_their_brackets(kind, dtype):
    fn = getattr(K(), kind)
    for numel in R.ACT_NS + (8192,):
        x = R.act_inputs(numel, dtype, DEV)
        keep = x.clone()
        got = fn(x)
        assert got.shape == x.shape and got.dtype == dtype and _same_bits(x, keep)
        share = R.assert_in_bracket(got, *R.act_bracket(x, kind), f"{kind} {numel}")
        assert share == 1.0 or kind in ("tanh", "gelu")
    inf = float("inf") if kind != "gelu" else 12.0  # gelu(-inf) is -inf * 0
    x = torch.tensor([float("nan"), -0.0, 0.0, -1.0, 2.0, inf, -inf], dtype=dtype, device=DEV)
    got = fn(x)
    R.assert_in_bracket(got, *R.act_bracket(x, kind), f"{kind} specials")
    if kind == "relu":
        assert bool(torch.isnan(got[0])) and got[1:].tolist() == [0.0, 0.0, 0.0, 2.0, float("inf"), 0.0]


@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
@pytest.mark.parametrize("kind", R.ACT_KINDS)
@pytest.mark.parametrize("shape", [(2049, 8192), (R.ACT_BIG_SCALAR,)], ids=["vector", "scalar"])
def test_activations_second_trip_of_the_grid_stride_loop(shape, kind, dtype):
    numel = shape[0] * (shape[1] if len(shape) == 2 else 1)
    assert R.grid_trips(1, numel, 8192)[1:] == (8192, 2)
    x = R.act_inputs(numel, dtype, DEV).view(shape)
    got = getattr(K(), kind)(x)
    assert got.shape == x.shape
    R.assert_in_bracket(got, *R.act_bracket(x, kind), f"{kind} {shape}")


# ------------------------------------------------------------------------------------------------------------------------------ #
# rope_emb_forward
# ------------------------------------------------------------------------------------------------------------------------------ #
def _fused_row(n_tok, heads, hd, dtype, pad=0):
    """A sentinel-filled ``[n_tok, heads * hd + pad]`` buffer and its ``[n_tok, heads, hd]`` view."""
    buf = R.sentinel((n_tok, heads * hd + pad), dtype, DEV)
    return buf, buf[:, :heads * hd].view(n_tok, heads, hd)


@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
@pytest.mark.parametrize("hd", R.ROPE_HDS)
def test_rope_emb_forward_rounds_once(hd, dtype):
    """Every head dimension (2, 6, 24 miss ``% 16``: the scalar kernel), tables in fp16, bf16 (two candidates) and fp32 (bracket), of
    width hd and hd / 2, a distinct table row per token, q / k dense and as views of one fused qkv row (token stride
    ``(hq + 2 hk) hd``; the V third and nothing else stays untouched)."""
    for hq, hk in R.rope_heads(hd):
        for bs, sl in R.ROPE_TOKENS:
            for table in R.ROPE_TABLES:
                for width in (hd, hd // 2):
                    q, k, cos, sin = _d(*R.rope_inputs(bs, sl, hq, hk, hd, dtype, table, width))
                    qb, kb = R.rope_bracket(q, cos, sin), R.rope_bracket(k, cos, sin)
                    ckeep = cos.clone()
                    for layout in ("dense", "fused"):
                        what = f"hd={hd} heads={hq},{hk} tokens={bs}x{sl} table={R.dname(table)}/{width} {layout}"
                        if layout == "dense":
                            qi, ki = q.clone(), k.clone()
                        else:
                            buf, row = _fused_row(bs * sl, hq + 2 * hk, hd, dtype)
                            qi, ki = row[:, :hq], row[:, hq:hq + hk]
                            qi.copy_(q)
                            ki.copy_(k)
                        q2, k2 = K().rope_emb_forward(qi, ki, cos, sin, bs, sl)
                        assert q2.data_ptr() == qi.data_ptr() and k2.data_ptr() == ki.data_ptr(), what  # in place
                        R.assert_in_bracket(q2, *qb, what + " q")
                        R.assert_in_bracket(k2, *kb, what + " k")
                        if layout == "fused":
                            assert bool(R.is_sentinel(row[:, hq + hk:]).all()), what
                    assert torch.equal(cos, ckeep)


@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
def test_rope_emb_forward_off_a_16_byte_boundary_takes_the_scalar_kernel_with_the_same_values(dtype):
    bs, sl, hq, hk, hd = 3, 5, 4, 2, 64
    q, k, cos, sin = _d(*R.rope_inputs(bs, sl, hq, hk, hd, dtype, F16, hd))
    q0, k0 = K().rope_emb_forward(q.clone(), k.clone(), cos, sin, bs, sl)
    qi, qbuf = _guarded(q, 1)
    ki, kbuf = _guarded(k, 1)
    q1, k1 = K().rope_emb_forward(qi, ki, cos, sin, bs, sl)
    assert q1.data_ptr() == qi.data_ptr() and q1.data_ptr() % 16 == 2
    R.assert_in_bracket(q1, *R.rope_bracket(q, cos, sin), "q off by one element")
    R.assert_in_bracket(k1, *R.rope_bracket(k, cos, sin), "k off by one element")
    assert _same_bits(q1, q0) and _same_bits(k1, k0)
    assert _guards_intact(qbuf, q.numel(), 1) and _guards_intact(kbuf, k.numel(), 1)


# ------------------------------------------------------------------------------------------------------------------------------ #
# rope_and_cache
# ------------------------------------------------------------------------------------------------------------------------------ #
def _rope_cache_case(hq, hk, hd, dtype, table, width, idx_dtype, with_pos, strided_pool, bs=3, sl=5):
    n_tok, pool_rows, max_pos = bs * sl, 40, 50
    q, k, cos, sin = _d(*R.rope_inputs(bs, sl, hq, hk, hd, dtype, table, width, rows=max_pos if with_pos else None))
    v = torch.randn(n_tok, hk, hd, device=DEV, generator=torch.Generator(DEV).manual_seed(hd + hq)).to(dtype)
    pos = torch.randperm(max_pos, device=DEV)[:n_tok] if with_pos else None
    sel = torch.randperm(pool_rows, device=DEV)[:n_tok].to(idx_dtype)  # a scattered permutation
    buf, row = _fused_row(n_tok, hq + 2 * hk, hd, dtype, pad=8)
    qi, kvi = row[:, :hq], row[:, hq:]
    qi.copy_(q)
    kvi[:, :hk].copy_(k)
    kvi[:, hk:].copy_(v)
    if strided_pool:  # token and head strides larger than the dense ones
        pbuf = R.sentinel((pool_rows, 2 * hk + 1, hd + 8), dtype, DEV)
        pool = pbuf[:, :2 * hk, :hd]
    else:
        pbuf = pool = R.sentinel((pool_rows, 2 * hk, hd), dtype, DEV)
    vec = hd % 16 == 0
    csv = vec and table != torch.float32 and width % 8 == 0
    what = (f"heads={hq},{hk} hd={hd} table={R.dname(table)}/{width} idx={idx_dtype} positions={with_pos} strided={strided_pool} "
            f"vector={vec} vector-table-loads={csv}")
    q2, kv2 = NA().rope_and_cache(qi, kvi, cos, sin, bs, sl, sel, pool, positions=pos)
    assert q2.data_ptr() == qi.data_ptr() and kv2.data_ptr() == kvi.data_ptr(), what
    R.assert_in_bracket(qi, *R.rope_bracket(q, cos, sin, pos), what + " q")
    R.assert_in_bracket(kvi[:, :hk], *R.rope_bracket(k, cos, sin, pos), what + " k")
    assert _same_bits(kvi[:, hk:], v), what  # V heads pass through
    assert bool(R.is_sentinel(buf[:, (hq + 2 * hk) * hd:]).all()), what
    assert _same_bits(pool[sel.long()], kvi), what  # pool rows are bit copies of the rotated K and the V heads
    written = torch.zeros(pbuf.shape, dtype=torch.bool, device=DEV)
    written[sel.long(), :2 * hk, :hd] = True
    assert bool(R.is_sentinel(pbuf)[~written].all()), what  # every other pool row and all padding untouched


@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_and_cache_rotates_and_scatters_in_every_variant(hd, dtype):
    """int32 / int64 ``select_index`` (the int64 cases over a pool with larger token and head strides), ``positions`` given or not,
    tables the vector loads can read (16-bit, width hd and hd / 2) and cannot (width hd / 2 + 2: rows off the 16-byte grid; fp32)."""
    hq, hk = (4, 2) if hd == 64 else (28, 4)
    for idx_dtype in (torch.int32, torch.int64):
        for with_pos in (False, True):
            for table, width in ((F16, hd), (BF16, hd // 2), (F16, hd // 2 + 2), (BF16, hd // 2 + 2), (torch.float32, hd)):
                _rope_cache_case(hq, hk, hd, dtype, table, width, idx_dtype, with_pos, idx_dtype == torch.int64)


@pytest.mark.parametrize("dtype", R.DTYPES, **IDS)
@pytest.mark.parametrize("hq,hk,hd", [(64, 8, 256), (80, 4, 24)])
def test_rope_and_cache_beyond_1024_work_items_per_token(hq, hk, hd, dtype):
    assert R.rope_work(hq, hk, hd, hd % 16 == 0, True)[1] == 2
    for with_pos, table in ((False, F16), (True, torch.float32)):
        _rope_cache_case(hq, hk, hd, dtype, table, hd, torch.int32, with_pos, with_pos)
