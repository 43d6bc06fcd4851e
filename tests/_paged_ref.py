"""Float64 reference and seeded inputs for causal prefill attention over the paged KV pool
(lite_llama_amd.kernels.prefill_paged_attention).  Runs on whatever device its tensors live on."""

from __future__ import annotations

import math

import torch

from tests._attn_ref import POISON_K, POISON_V


def paged_prefill_ref(q, k_pool, v_pool, sm_scale, table, req, start, q_len, ctx_len):
    """Sequence ``b``'s new query ``j`` (row ``start[b] + j`` of ``q``) attends to pool rows ``table[req[b], :ctx[b] + j
    + 1]``; weights ``exp2(sm_scale * q . k)`` (``sm_scale`` carries log2 e).  ``k_pool`` / ``v_pool`` ``[rows, Hkv, D]``
    in any float dtype (the widened values x scale for an e4m3 pool).  Returns ``(out [R, Hq, D], vmax [R, Hq], z [R,
    Hq], n [R], idx [R])`` over the new rows of all sequences in order, as :func:`tests._attn_ref.prefill_ref`."""
    hq, hkv = q.shape[1], k_pool.shape[1]
    g = hq // hkv
    outs, vms, zs, ns, idx = [], [], [], [], []
    for b in range(len(q_len)):
        n, c, st = int(q_len[b]), int(ctx_len[b]), int(start[b])
        if n == 0:
            continue
        rows = table[int(req[b]), :c + n].long()
        kk = k_pool[rows].double().repeat_interleave(g, dim=1)          # [c + n, Hq, D]
        vv = v_pool[rows].double()
        vcum = vv.abs().amax(dim=2).cummax(dim=0).values.repeat_interleave(g, dim=1)  # [c + n, Hq]
        vv = vv.repeat_interleave(g, dim=1)
        qq = q[st:st + n].double()
        s = torch.einsum("ihd,jhd->hij", qq, kk) * sm_scale
        keys = torch.arange(c + n, device=q.device)
        causal = keys[None, :] <= (c + torch.arange(n, device=q.device))[:, None]
        s = s.masked_fill(~causal[None], -math.inf)
        e = torch.exp2(s - s.amax(dim=-1, keepdim=True))
        z = e.sum(dim=-1)
        outs.append(torch.einsum("hij,jhd->ihd", e, vv) / z.T[:, :, None])
        zs.append(z.T)
        vms.append(vcum[c:c + n])
        ns.append(c + torch.arange(1, n + 1, dtype=torch.float64, device=q.device))
        idx.append(torch.arange(st, st + n, device=q.device))
    return torch.cat(outs), torch.cat(vms), torch.cat(zs), torch.cat(ns), torch.cat(idx)


def paged_inputs(seqs, hq, hkv, d, dtype, seed, table_kind="contiguous", device="cpu", gap=8, spare=64, sigma=1.0):
    """Seeded inputs for ``seqs = [(ctx, n), ...]``: ``q [T, Hq, D]`` (each sequence's rows followed by ``gap`` NaN
    rows), a fused pool ``[rows, 2 Hkv, D]`` and an int32 table ``[B, width]``.  ``table_kind``: ``contiguous`` (one run
    per sequence), ``permuted`` (the named rows in a random permutation) or ``shared`` (every sequence names sequence
    0's first ``min(ctx)`` rows for its prefix).  Rows the table does not name -- ``spare`` of them, also named by every
    table cell past a sequence's ``ctx + n`` -- hold poison: K aimed at the queries, V = +-POISON_V, half of them NaN;
    ``unnamed`` lists them."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    b = len(seqs)
    totals = [c + n for c, n in seqs]
    width = max(max(totals), 1) + 16
    shared = min(c for c, _ in seqs) if table_kind == "shared" else 0
    own = [t - (shared if i else 0) for i, t in enumerate(totals)]
    named = sum(own)
    perm = torch.randperm(named + spare, generator=gen)
    pool_rows, unnamed = perm[:named], perm[named:]
    if table_kind == "contiguous":
        pool_rows = torch.arange(named)
        unnamed = torch.arange(named, named + spare)
    table = torch.empty(b, width, dtype=torch.int64)
    at = 0
    for i, t in enumerate(totals):
        r = pool_rows[at:at + own[i]]
        at += own[i]
        row = torch.cat([table[0, :shared], r]) if i and shared else r
        table[i, :t] = row
        table[i, t:] = unnamed[torch.randint(0, spare, (width - t,), generator=gen)]
    pool = torch.randn(named + spare, 2 * hkv, d, generator=gen, dtype=torch.float64)
    pool[:, :hkv] *= sigma
    qs, starts, st = [], [], 0
    for c, n in seqs:
        qs += [torch.randn(n, hq, d, generator=gen, dtype=torch.float64), torch.full((gap, hq, d), math.nan)]
        starts.append(st)
        st += n + gap
    q = torch.cat(qs)
    aim = torch.sign(q[~torch.isnan(q[:, 0, 0])].sum(dim=(0, 1)))
    half = spare // 2
    pool[unnamed[:half], :hkv] = POISON_K * aim
    pool[unnamed[:half], hkv:] = POISON_V * torch.sign(torch.randn(half, hkv, d, generator=gen, dtype=torch.float64))
    pool[unnamed[half:]] = math.nan
    return dict(q=q.to(dtype).to(device), pool=pool.to(dtype).to(device), table=table.to(torch.int32).to(device),
                req=torch.arange(b, dtype=torch.int32, device=device),
                start=torch.tensor(starts, dtype=torch.int32, device=device),
                q_len=torch.tensor([n for _, n in seqs], dtype=torch.int32, device=device),
                ctx=torch.tensor([c for c, _ in seqs], dtype=torch.int32, device=device),
                max_q=max(n for _, n in seqs), max_ctx=max(c for c, _ in seqs),
                unnamed=unnamed.to(device), sm_scale=1.4426950408889634 / math.sqrt(d))
