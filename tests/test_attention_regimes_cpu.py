"""The attention regimes' own mutation check (no GPU): at small sizes, for every input regime of tests/_attn_ref.py,
the rounding-model bound accepts a model of the kernels' legitimate rounding -- the same partitioned online softmax
with P rounded to the 16-bit operand type and the output rounded once -- and rejects deliberately broken versions
of the algorithm.  This is what lets tests/test_attention_regimes_gpu.py tell a subtly wrong kernel from a right one.
"""

import math

import pytest
import torch

from tests import _attn_ref as R

DTYPES = [torch.float16, torch.bfloat16]

# decode: one token past the length, the last token dropped, the merge without max correction, a partition skipped
# (first / last) or counted twice, two query heads of a GQA group swapped
DECODE_MUTANTS = ("past", "drop_last", "no_max_merge", "skip_first", "skip_last", "twice_last", "swap_heads")
# prefill: key i + 1 visible to row i on every row, or only where i + 1 starts a 64-key tile
PREFILL_MUTANTS = ("diag_plus1", "tile_edge")

# (regime, mutant, dtype or None for both) pairs a regime cannot see by construction -- each mutant is still rejected
# by every other regime:
# * a falling ramp puts the weight on the first tokens: the last token / partition carries ~e^-20 of it;
# * a 95 % spotlight in the last partition counted twice moves the output by W (1 - W) / (1 + W) |V| <= 0.024 |V|,
#   below bf16's 4u (vmax + |ref|) ~ 0.03 |V| (fp16 rejects it 8x over).
BLIND = {("falling", "drop_last", None), ("falling", "skip_last", None), ("falling", "twice_last", None),
         ("spotlight", "twice_last", torch.bfloat16), ("split", "twice_last", torch.bfloat16)}

DECODE_LENS = [700, 513, 300, 129, 1000, 257]   # 1 .. 8 partitions, several rows past the first partition edge
PREFILL_LENS = [64, 128, 200, 65, 1, 127]


def _rnd(x, dtype):
    return x.to(dtype).double()


def decode_model(inp, dtype, mutant=None, part=R.FD_PART, tile=32):
    """The decode kernels' algorithm in float64 with their two roundings: per partition of ``part`` tokens an online
    softmax over tiles of ``tile`` tokens, P rounded to ``dtype`` against the running maximum, the partial normalised;
    the partials merged by their log-sum-exp; the output rounded to ``dtype``.  ``mutant`` breaks one step."""
    q, pool, table, req, seq = inp["q"], inp["pool"], inp["table"], inp["req"], inp["seq"]
    hkv = inp["hkv"]
    B, hq, d = q.shape
    g = hq // hkv
    out = torch.zeros(B, hq, d, dtype=torch.float64)
    for b in range(B):
        n = int(seq[b]) + {"past": 1, "drop_last": -1}.get(mutant, 0)
        idx = table[int(req[b]), :n].long()
        kk = pool[idx, :hkv].double().repeat_interleave(g, dim=1)
        vv = pool[idx, hkv:].double().repeat_interleave(g, dim=1)
        s = torch.einsum("hd,nhd->hn", q[b].double(), kk) * inp["scale"]
        recs = []
        for p0 in range(0, n, part):
            m = torch.full((hq,), -math.inf, dtype=torch.float64)
            den = torch.zeros(hq, dtype=torch.float64)
            acc = torch.zeros(hq, d, dtype=torch.float64)
            for t0 in range(p0, min(p0 + part, n), tile):
                t1 = min(t0 + tile, p0 + part, n)
                st = s[:, t0:t1]
                m_new = torch.maximum(m, st.amax(dim=1))
                alpha = torch.exp(m - m_new)
                p = torch.exp(st - m_new[:, None])
                den = den * alpha + p.sum(dim=1)
                acc = acc * alpha[:, None] + torch.einsum("hn,nhd->hd", _rnd(p, dtype), vv[t0:t1])
                m = m_new
            recs.append((m + torch.log(den), torch.log(den), acc / den[:, None]))
        if len(recs) > 1:
            if mutant == "skip_first":
                recs = recs[1:]
            elif mutant == "skip_last":
                recs = recs[:-1]
            elif mutant == "twice_last":
                recs = recs + recs[-1:]
        lse = torch.stack([r[1] if mutant == "no_max_merge" else r[0] for r in recs])   # [P, Hq]
        w = torch.exp(lse - lse.amax(dim=0))
        out[b] = torch.einsum("ph,phd->hd", w, torch.stack([r[2] for r in recs])) / w.sum(dim=0)[:, None]
    if mutant == "swap_heads":
        for h in range(hkv):
            out[:, [h * g, h * g + 1]] = out[:, [h * g + 1, h * g]]
    return _rnd(out, dtype)


def prefill_model(inp, dtype, mutant=None, tile=64):
    """The prefill kernels' algorithm in float64: per row an online softmax (exp2, ``sm_scale`` with log2 e) over key
    tiles of ``tile``, P rounded to ``dtype``, the output rounded.  Rows are concatenated like :func:`prefill_ref`."""
    q, k, v = inp["q"], inp["k"], inp["v"]
    hq, hkv = q.shape[1], k.shape[1]
    g = hq // hkv
    outs = []
    for st, n in zip(inp["start"].tolist(), inp["seq"].tolist()):
        if n == 0:
            continue
        kk = k[st:st + n + 1].double().repeat_interleave(g, dim=1)    # (+ the first padded row: a mutant may see it)
        vv = v[st:st + n + 1].double().repeat_interleave(g, dim=1)
        s = torch.einsum("ihd,jhd->hij", q[st:st + n].double(), kk) * inp["sm_scale"]
        rows, keys = torch.arange(n)[:, None], torch.arange(n + 1)[None, :]
        vis = keys <= rows
        if mutant == "diag_plus1":
            vis = keys <= rows + 1
        elif mutant == "tile_edge":
            vis = vis | ((keys == rows + 1) & (keys % 64 == 0))
        s = s.masked_fill(~vis[None], -math.inf)
        m = torch.full((hq, n), -math.inf, dtype=torch.float64)
        den = torch.zeros(hq, n, dtype=torch.float64)
        acc = torch.zeros(hq, n, k.shape[2], dtype=torch.float64)
        for t0 in range(0, n + 1, tile):
            st_ = s[:, :, t0:t0 + tile]
            m_new = torch.maximum(m, st_.amax(dim=2))
            alpha = torch.exp2(m - m_new)
            p = torch.exp2(st_ - m_new[..., None])
            den = den * alpha + p.sum(dim=2)
            acc = acc * alpha[..., None] + torch.einsum("hij,jhd->hid", _rnd(p, dtype), vv[t0:t0 + tile])
            m = m_new
        outs.append((acc / den[..., None]).permute(1, 0, 2))
    return _rnd(torch.cat(outs), dtype)


def _decode_case(regime, dtype):
    inp = R.decode_inputs(regime, DECODE_LENS, 8, 2, 64, dtype, seed=3)
    hkv = inp["hkv"]
    ref, vmax, z, n = R.decode_ref(inp["q"], inp["pool"][:, :hkv], inp["pool"][:, hkv:], inp["scale"], inp["table"],
                                   inp["req"], inp["seq"])
    return inp, ref, R.bound(ref, vmax, z, n, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("regime", R.DECODE_REGIMES)
def test_decode_bound_accepts_the_rounding_model(regime, dtype):
    inp, ref, tol = _decode_case(regime, dtype)
    assert R.within(decode_model(inp, dtype), ref, tol) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mutant", DECODE_MUTANTS)
@pytest.mark.parametrize("regime", R.DECODE_REGIMES)
def test_decode_bound_rejects_the_mutant(regime, mutant, dtype):
    inp, ref, tol = _decode_case(regime, dtype)
    r = R.within(decode_model(inp, dtype, mutant), ref, tol)
    if (regime, mutant, None) in BLIND or (regime, mutant, dtype) in BLIND:
        assert r <= 1.0   # documented blind spot: if this starts failing, the regime got sharper -- drop the entry
    else:
        assert r > 1.0


def _prefill_case(regime, dtype):
    inp = R.prefill_inputs(regime, PREFILL_LENS, 4, 2, 64, dtype, seed=5)
    ref, vmax, z, n, idx = R.prefill_ref(inp["q"], inp["k"], inp["v"], inp["sm_scale"], inp["start"], inp["seq"])
    return inp, ref, R.bound(ref, vmax, z, n, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("regime", R.PREFILL_REGIMES)
def test_prefill_bound_accepts_the_rounding_model(regime, dtype):
    inp, ref, tol = _prefill_case(regime, dtype)
    assert R.within(prefill_model(inp, dtype), ref, tol) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mutant", PREFILL_MUTANTS)
@pytest.mark.parametrize("regime", R.PREFILL_REGIMES)
def test_prefill_bound_rejects_the_mutant(regime, mutant, dtype):
    inp, ref, tol = _prefill_case(regime, dtype)
    assert R.within(prefill_model(inp, dtype, mutant), ref, tol) > 1.0
