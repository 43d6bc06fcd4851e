"""References for ``ll_logit_penalties`` and ``ll_seeded_uniform`` (csrc/sampler_penalties.hip), written from their contract
in include/lite_llama_amd.h.  No device."""

import torch

M32 = 0xFFFFFFFF


def penalties_ref(logits, token_ids, mask, r, p, f, bias=None):
    """float64 ``[B, V]``: per row ``x = z + bias``; where the count ``c > 0``: ``x = x * r if x < 0 else x / r``; then
    ``x - f * c - (p if c > 0 else 0)``.  ``r`` / ``p`` / ``f``: floats or sequences of one per row (used at the value fp32
    holds); ``bias``: ``None``, a dict, or a list of dicts / ``None``s.  Also returns the counts ``[B, V]`` (int64)."""
    z = logits.detach().cpu().to(torch.float64)
    b, v = z.shape
    counts = torch.zeros(b, v, dtype=torch.int64)
    dense = torch.zeros(b, v, dtype=torch.float64)
    out = torch.empty_like(z)

    def row_value(x, i):
        x = x[i] if isinstance(x, (list, tuple)) else (x.reshape(-1)[i] if torch.is_tensor(x) else x)
        return float(torch.tensor(float(x), dtype=torch.float32))

    for i in range(b):
        if token_ids is not None and token_ids.shape[1]:
            ids = token_ids[i].cpu()[mask[i].cpu().bool()]
            ids = ids[(ids >= 0) & (ids < v)]
            uniq, cnt = torch.unique(ids, return_counts=True)
            counts[i, uniq] = cnt
        row_bias = bias if bias is None or isinstance(bias, dict) else bias[i]
        for tok, val in (row_bias or {}).items():
            dense[i, tok] = float(torch.tensor(float(val), dtype=torch.float32))
        ri, pi, fi = row_value(r, i), row_value(p, i), row_value(f, i)
        x = z[i] + dense[i]
        seen = counts[i] > 0
        x = torch.where(seen, torch.where(x < 0, x * ri, x / ri), x)
        out[i] = x - fi * counts[i].to(torch.float64) - pi * seen.to(torch.float64)
    return out, counts, dense


def _mulhilo(a, b):
    m = a * b
    return (m >> 32) & M32, m & M32


def philox4x32_10(counter, key):
    """The four output words of Philox4x32-10 (Salmon et al., SC'11) at ``counter`` (4 words) and ``key`` (2 words)."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        hi0, lo0 = _mulhilo(0xD2511F53, c0)
        hi1, lo1 = _mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((M32, M32, M32, M32), (M32, M32), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def check_known_answers():
    for counter, key, words in KNOWN_ANSWERS:
        assert philox4x32_10(counter, key) == words, (counter, key)


def uniform_ref(seed: int, column: int) -> float:
    """``ll_seeded_uniform`` of one row: key = the seed's two halves, counter = the column's, ``(word0 >> 8) * 2^-24``."""
    s, c = seed & 0xFFFFFFFFFFFFFFFF, column & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10((c & M32, c >> 32, 0, 0), (s & M32, s >> 32))[0]
    return (w >> 8) / float(1 << 24)
