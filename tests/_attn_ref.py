"""Attention test helpers (not a conftest): float64 references, a tolerance derived from the kernels' rounding, and
seeded input regimes that make the softmax weights matter.

The references restate the operation directly -- ``softmax(scale * q . K^T) @ V`` over the exact 16-bit (or widened
fp8 x scale) inputs, GQA by ``repeat_interleave`` -- and share nothing with ``oracle.flash_decoding``'s chunk walk.
Every function runs on whatever device its tensors live on (the GPU tests evaluate the large cases in fp64 there).
"""

from __future__ import annotations

import math

import torch

LOG2E = 1.4426950408889634
FD_PART = 128          # tokens per decode partition (csrc/flash_decoding.hip FD_PART)
FD_GROUP_MAX = 8       # waves of the one-workgroup decode form (FD_GROUP_MAX)
POISON_V = 1.0e4       # |V| of poisoned rows (finite in fp16 and bf16)
POISON_K = 2.0e3       # |K| of poisoned rows: scores of order 1e4 against the row's queries
FP8_MAX = 448.0        # largest finite OCP e4m3 value

# unit roundoff of the 16-bit MFMA operand type (P and the output are rounded to it)
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


# ------------------------------------------------------------------------------------------------------------------- #
# references
# ------------------------------------------------------------------------------------------------------------------- #
def decode_ref(q, k_pool, v_pool, scale, table, req, seq, rows=None):
    """Paged decode attention in float64: batch row ``b`` attends pool rows ``table[req[b], :seq[b]]``.

    ``k_pool`` / ``v_pool`` ``[rows, Hkv, D]`` in any float dtype (pass the widened fp8 values x scale).  Returns
    ``(out [R, Hq, D], vmax [R, Hq], z [R, Hq], n [R])`` for the batch rows ``rows`` (default: all): ``vmax`` is the
    largest |V| over the attended rows of the head's KV head, ``z = sum_j exp(s_j - max_j s_j)`` the normaliser in units
    of the largest weight (>= 1), ``n`` the context length."""
    hq, hkv = q.shape[1], k_pool.shape[1]
    g = hq // hkv
    rows = range(q.shape[0]) if rows is None else rows
    outs, vms, zs, ns = [], [], [], []
    for b in rows:
        n = int(seq[b])
        idx = table[int(req[b]), :n].long()
        kk = k_pool[idx].double().repeat_interleave(g, dim=1)       # [n, Hq, D]
        vv = v_pool[idx].double()
        vms.append(vv.abs().amax(dim=(0, 2)).repeat_interleave(g))
        vv = vv.repeat_interleave(g, dim=1)
        s = torch.einsum("hd,nhd->hn", q[b].double(), kk) * scale
        e = torch.exp(s - s.amax(dim=-1, keepdim=True))
        z = e.sum(dim=-1)
        outs.append(torch.einsum("hn,nhd->hd", e, vv) / z[:, None])
        zs.append(z)
        ns.append(n)
    dev = q.device
    return (torch.stack(outs), torch.stack(vms), torch.stack(zs),
            torch.tensor(ns, dtype=torch.float64, device=dev))


def prefill_ref(q, k, v, sm_scale, b_start_loc, b_seq_len, chunk=512):
    """Varlen causal prefill attention in float64 with the ABI's convention: ``sm_scale`` includes log2(e) and the
    weights are ``exp2(sm_scale * q . k)``.  ``q [T, Hq, D]``, ``k`` / ``v`` ``[T, Hkv, D]`` packed; sequence ``b``
    holds rows ``start[b] .. start[b] + len[b]``.  Returns ``(out, vmax, z, n)`` over the concatenated rows of the
    sequences (``[R, Hq, D]``, ``[R, Hq]``, ``[R, Hq]``, ``[R]``: ``vmax`` the largest |V| over keys ``0..i`` of the
    head's KV head, ``z`` as in :func:`decode_ref`, ``n = i + 1``) and the packed row index of each."""
    hq, hkv = q.shape[1], k.shape[1]
    g = hq // hkv
    outs, vms, zs, ns, idx = [], [], [], [], []
    for st, ln in zip(b_start_loc.tolist(), b_seq_len.tolist()):
        if ln == 0:
            continue
        kk = k[st:st + ln].double().repeat_interleave(g, dim=1)     # [n, Hq, D]
        vv = v[st:st + ln].double()
        vcum = vv.abs().amax(dim=2).cummax(dim=0).values.repeat_interleave(g, dim=1)   # [n, Hq]
        vv = vv.repeat_interleave(g, dim=1)
        qq = q[st:st + ln].double()
        keys = torch.arange(ln, device=q.device)
        for r0 in range(0, ln, chunk):
            r1 = min(ln, r0 + chunk)
            s = torch.einsum("ihd,jhd->hij", qq[r0:r1], kk) * sm_scale          # log2 units
            causal = keys[None, :] <= torch.arange(r0, r1, device=q.device)[:, None]
            s = s.masked_fill(~causal[None], -math.inf)
            e = torch.exp2(s - s.amax(dim=-1, keepdim=True))
            z = e.sum(dim=-1)                                                    # [Hq, rows]
            outs.append(torch.einsum("hij,jhd->ihd", e, vv) / z.T[:, :, None])
            zs.append(z.T)
        vms.append(vcum)
        ns.append(torch.arange(1, ln + 1, dtype=torch.float64, device=q.device))
        idx.append(torch.arange(st, st + ln, device=q.device))
    return torch.cat(outs), torch.cat(vms), torch.cat(zs), torch.cat(ns), torch.cat(idx)


# ------------------------------------------------------------------------------------------------------------------- #
# tolerance
# ------------------------------------------------------------------------------------------------------------------- #
def bound(ref, vmax, z, n, dtype):
    """Per-element bound on ``|got - ref|`` for a kernel that keeps scores, exp, the running sums and the partition
    merge in fp32, rounds P to the 16-bit MFMA operand type and the output once to the storage type:

        |got - ref| <= 4u (vmax + |ref|)  [+ n 2^-25 vmax / z   for fp16 operands]

    ``u`` is the unit roundoff of ``dtype`` (2^-11 fp16 -- also for fp8 KV, whose widened values are fp16 operands --
    and 2^-8 bf16); ``vmax`` the largest |V| the row attends; ``z >= 1`` and ``n`` as returned by the references.

    Derivation.  Within a partition each probability is ``p = exp(s - m)`` against the running maximum ``m`` (so
    ``p <= 1``) and enters ``O = sum p v`` rounded, ``|round(p) - p| <= u p``, while the denominator ``d = sum p`` is
    summed unrounded.  Hence ``|O/d - sum p v / d| <= u sum p |v| / d <= u vmax``.  The partition merge is a convex
    combination with fp32 weights, so the merged value keeps that bound; the final rounding adds ``u |ref|``.  The fp32
    terms (score accumulation over D products of exact 16-bit values, exp2, the running sums, 1/d) are ~2^-20
    relative, absorbed by the factor 4 -- a 2x margin over the 2u vmax + u |ref| the two roundings can reach.
    fp16 additionally flushes: below 2^-14 the operand spacing is absolute (2^-24), so a rounded ``p`` may be off
    by 2^-25 in units of the running maximum.  In units of the row's global maximum that is <= 2^-25 (the running
    maximum is never larger), and the global-unit normaliser is ``z``: at most ``n 2^-25 vmax / z`` in all.  bf16
    has fp32's exponent range and no such term."""
    u = UNIT[dtype]
    tol = 4.0 * u * (vmax[..., None] + ref.abs())
    if dtype == torch.float16:
        tol = tol + (n[:, None] * 2.0 ** -25 * vmax / z)[..., None]
    return tol


def within(got, ref, tol):
    """Largest ``|got - ref| / tol`` (inf when ``got`` has a non-finite element)."""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got - ref).abs() / tol).max())


def assert_within(got, ref, tol, what):
    """Assert ``|got - ref| <= tol`` element-wise; prints and returns the largest error as a fraction of the bound."""
    r = within(got, ref, tol)
    if r > 1.0:
        got = got.double()
        err = torch.where(torch.isfinite(got), (got - ref).abs() / tol, torch.full_like(got, math.inf))
        at = [int(i) for i in torch.unravel_index(int(err.reshape(-1).argmax()), err.shape)]
        raise AssertionError(f"{what}: |err| / bound = {r:.3g} at {at}: got {float(got[tuple(at)])}, "
                             f"ref {float(ref[tuple(at)])}, bound {float(tol[tuple(at)]):.3g}")
    print(f"[attn-bound] {what}: max |err| / bound = {r:.3f}")
    return r


# ------------------------------------------------------------------------------------------------------------------- #
# input regimes
# ------------------------------------------------------------------------------------------------------------------- #
DECODE_REGIMES = ("wide", "spotlight", "split", "ramp", "falling", "offset", "poison")
PREFILL_REGIMES = ("wide", "spot0", "diag", "future", "poison")


def spot_positions(n):
    """Key positions the spotlights sweep for a context of ``n`` tokens: the first token, both sides of the first
    partition edge, the first token of the last partition and the last token before it, the last two tokens, and a
    partition in the walking waves' second lap."""
    last = FD_PART * ((n - 1) // FD_PART)
    cand = [0, FD_PART - 1, FD_PART, last, last - 1, n - 1, n - 2, FD_GROUP_MAX * FD_PART + 5]
    out = []
    for p in cand:
        if 0 <= p < n and p not in out:
            out.append(p)
    return out


def _aim(qg, target, d):
    """Least-norm key ``u`` with ``q_h . u / sqrt(d) = target_h`` for every query head ``h`` of a GQA group:
    ``qg [..., g, D]`` float64, ``target [..., g]`` -> ``[..., D]``."""
    gram = qg @ qg.transpose(-1, -2)
    return (qg.transpose(-1, -2) @ torch.linalg.solve(gram, target.unsqueeze(-1))).squeeze(-1) * math.sqrt(d)


def _spot_offset(n, sigma):
    """Score lead that gives one key 95 % of the weight over n keys of score std ``sigma`` (about 12 at 8200 keys of
    std 0.5): the other 5 % keep the background visible."""
    return math.log(19.0 * n * math.exp(sigma * sigma / 2))


def decode_inputs(regime, lens, hq, hkv, d, dtype, seed, device="cpu", pad=16, spare=16):
    """Seeded decode inputs: ``q [B, Hq, D]``, a fused pool ``[rows, 2 Hkv, D]`` (K heads then V heads, the model's
    layout), ``table [B, max(lens) + pad]`` int32, ``req`` (a permutation), ``seq``.  Scale is ``1 / sqrt(D)``.

    Every regime names ``pad`` poisoned pool rows past each ``seq[b]`` in the table (K aimed at the row's queries with
    |K| = POISON_K, V = +-POISON_V) and leaves ``spare`` rows no table names, poisoned with NaN; ``poisoned`` lists both
    sets so a caller can build the clean pool.  ``spots`` ``[B, Hq]`` holds each head's spotlight key (-1: none).

    * wide: score std 5 with 2 % of the keys at std 10 (logits reaching +-30);
    * spotlight: per (row, KV head) one key of :func:`spot_positions` leads the background (std 0.5) by about 12 --
      the odd heads of the group by 3 more, so neighbouring heads' leftover weights differ -- with V = +-3 there
      (background V std 0.5);
    * split: the heads of one GQA group spotlight different keys;
    * ramp / falling: scores rising (falling) linearly by 20 along the context, head slopes 1 .. 1.5;
    * offset: V = 4 + randn under score std 2 (checks the normaliser);
    * poison: the wide regime; the caller compares against the clean pool bit for bit."""
    gen = torch.Generator(device=device).manual_seed(seed)
    f64 = torch.float64
    B, g = len(lens), hq // hkv
    width = max(lens) + pad
    n_named = sum(lens) + B * pad
    rows = n_named + spare
    rt = math.sqrt(d)

    def randn(*shape):
        return torch.randn(*shape, generator=gen, device=device, dtype=f64)

    q = randn(B, hq, d).to(dtype)
    qd = q.double()
    qg = qd.view(B, hkv, g, d)
    sigma = {"wide": 5.0, "poison": 5.0, "offset": 2.0, "spotlight": 0.5, "split": 0.5, "ramp": 0.5,
             "falling": 0.5}[regime]
    kt = randn(B, width, hkv, d) * sigma          # per (row, token) keys, placed into the pool below
    vt = randn(B, width, hkv, d)
    if regime in ("wide", "poison"):
        heavy = torch.rand(B, width, 1, 1, generator=gen, device=device, dtype=f64) < 0.02
        kt = torch.where(heavy, kt * 2.0, kt)
    if regime == "offset":
        vt = vt + 4.0
    if regime in ("spotlight", "split"):
        vt = vt * 0.5          # the spotlit V (+-3) sets vmax: the leftover 5 % stays visible against the bound
    spots = torch.full((B, hq), -1, dtype=torch.int64, device=device)
    if regime in ("spotlight", "split"):
        for b, n in enumerate(lens):
            pos = spot_positions(n)
            off = _spot_offset(n, sigma)
            for h in range(hkv):
                if regime == "spotlight":
                    p = pos[(b * hkv + h) % len(pos)]
                    lead = off + 3.0 * (torch.arange(g, device=device, dtype=f64) % 2)
                    kt[b, p, h] = _aim(qg[b, h], lead, d)
                    vt[b, p, h] = 3.0 * torch.sign(randn(d))
                    spots[b, h * g:(h + 1) * g] = p
                else:
                    hp = [pos[(b * hkv + h + j) % len(pos)] for j in range(g)]   # head j of the group -> key hp[j]
                    for p in set(hp):
                        mask = torch.tensor([float(x == p) for x in hp], device=device, dtype=f64)
                        kt[b, p, h] = _aim(qg[b, h], off * mask, d)
                        vt[b, p, h] = 3.0 * torch.sign(randn(d))
                    spots[b, h * g:(h + 1) * g] = torch.tensor(hp, device=device)
    if regime in ("ramp", "falling"):
        slope = 1.0 + 0.5 * torch.arange(g, device=device, dtype=f64) / max(g - 1, 1)
        for b, n in enumerate(lens):
            u = _aim(qg[b], slope.expand(hkv, g), d)                  # [Hkv, D]: q_h . u / sqrt(D) = slope_h
            a = 20.0 * torch.arange(width, device=device, dtype=f64) / max(n - 1, 1)
            if regime == "falling":
                a = 20.0 - a
            kt[b] += a[:, None, None] * u[None]
    # poison past each row's length: K aimed at the row's queries, V = +-1e4
    for b, n in enumerate(lens):
        aim = torch.sign(qg[b].sum(dim=1))                            # [Hkv, D]
        kt[b, n:] = POISON_K * aim[None]
        vt[b, n:] = POISON_V * torch.sign(randn(width - n, hkv, d))
    perm = torch.randperm(rows, generator=gen, device=device)
    pool = torch.full((rows, 2 * hkv, d), math.nan, dtype=f64, device=device)
    table = torch.zeros(B, width, dtype=torch.int32, device=device)
    req = torch.randperm(B, generator=gen, device=device)
    off = 0
    poisoned = [perm[n_named:]]
    for b, n in enumerate(lens):
        r = perm[off:off + n + pad]
        off += n + pad
        table[req[b], :n + pad] = r.to(torch.int32)
        pool[r, :hkv] = kt[b, :n + pad]
        pool[r, hkv:] = vt[b, :n + pad]
        poisoned.append(r[n:])
    seq = torch.tensor(lens, dtype=torch.int32, device=device)
    return dict(q=q, pool=pool.to(dtype), table=table, req=req, seq=seq, spots=spots, scale=1.0 / rt,
                poisoned=torch.cat(poisoned), hkv=hkv)


def clean_pool(inp):
    """The pool of :func:`decode_inputs` with every poisoned row zeroed."""
    pool = inp["pool"].clone()
    pool[inp["poisoned"]] = 0
    return pool


def fp8_pool(pool, k_scale, v_scale, hkv):
    """OCP e4m3 codes of a fused 16-bit pool (K heads / k_scale, V heads / v_scale, clamped to +-448; NaN stays
    NaN) and the widened float32 values x scale the references take."""
    x = pool.float()
    x[:, :hkv] /= k_scale
    x[:, hkv:] /= v_scale
    codes = torch.where(torch.isnan(x), x, x.clamp(-FP8_MAX, FP8_MAX)).to(torch.float8_e4m3fn)
    wide = codes.float()
    wide[:, :hkv] *= k_scale
    wide[:, hkv:] *= v_scale
    return codes, wide


def prefill_inputs(regime, lens, hq, hkv, d, dtype, seed, device="cpu", gap=16):
    """Seeded packed prefill inputs ``q [T, Hq, D]``, ``k`` / ``v`` ``[T, Hkv, D]``, ``start``, ``seq`` (int32),
    ``sm_scale = log2(e) / sqrt(D)``.  Each sequence is followed by ``gap`` padded rows poisoned in every regime:
    the first half K aimed at the sequence's queries (|K| = POISON_K) and V = +-POISON_V, the second half NaN;
    ``poisoned`` lists them.

    * wide: score std 5;
    * spot0: a component shared by every query of a KV head lets key 0 lead every row by about 12;
    * diag: key i leads row i by about 12 (its own token);
    * future: key i + 1 leads row i by about 12 -- a causal mask must give it no weight;
    * poison: the wide regime; the caller compares against zeroed padding bit for bit."""
    gen = torch.Generator(device=device).manual_seed(seed)
    f64 = torch.float64
    g = hq // hkv
    rt = math.sqrt(d)

    def randn(*shape):
        return torch.randn(*shape, generator=gen, device=device, dtype=f64)

    sigma = 5.0 if regime in ("wide", "poison") else 0.5
    qs, ks, vs, starts, poisoned = [], [], [], [], []
    st = 0
    for n in lens:
        q = randn(n, hq, d)
        if regime == "spot0":
            w = randn(hkv, d)
            q = 0.6 * q + w.repeat_interleave(g, dim=0)[None]
        q = q.to(dtype).double()
        qg = q.view(n, hkv, g, d)
        k = randn(n + gap, hkv, d) * sigma
        v = randn(n + gap, hkv, d)
        off = _spot_offset(max(n, 2), sigma)
        if n and regime == "spot0":
            wq = qg.mean(dim=(0, 2))                                   # [Hkv, D]: the shared component
            k[0] = off * rt * wq / (wq * wq).sum(dim=-1, keepdim=True)
            v[0] = 3.0 * torch.sign(randn(hkv, d))
        if n and regime in ("diag", "future"):
            sh = 0 if regime == "diag" else 1
            lead = torch.full((n, hkv, g), off, device=device, dtype=f64)
            k[sh:n + sh] = _aim(qg, lead, d)
            v[sh:n + sh] = 3.0 * torch.sign(randn(n, hkv, d))
        aim = torch.sign(qg.sum(dim=(0, 2))) if n else torch.ones(hkv, d, device=device, dtype=f64)
        half = gap // 2
        k[n:n + half] = POISON_K * aim[None]
        v[n:n + half] = POISON_V * torch.sign(randn(half, hkv, d))
        k[n + half:n + gap] = math.nan
        v[n + half:n + gap] = math.nan
        qpad = torch.full((gap, hq, d), math.nan, device=device, dtype=f64)
        qs += [q, qpad]
        ks.append(k)
        vs.append(v)
        starts.append(st)
        poisoned.append(torch.arange(st + n, st + n + gap, device=device))
        st += n + gap
    return dict(q=torch.cat(qs).to(dtype), k=torch.cat(ks).to(dtype), v=torch.cat(vs).to(dtype),
                start=torch.tensor(starts, dtype=torch.int32, device=device),
                seq=torch.tensor(lens, dtype=torch.int32, device=device), sm_scale=LOG2E / rt,
                poisoned=torch.cat(poisoned))
